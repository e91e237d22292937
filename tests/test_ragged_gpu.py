"""GPU test: ragged batches over a KV cache through the C ABI of include/mfa_ragged.h (the rowStarts= / totalRows= keywords of
AttentionPrefill and KVCacheAppend).

The arithmetic of the ragged kernels is the padded kernels'; only where a row lives and which workgroup serves it is new.  So the
ragged launch is held to BYTE IDENTITY with the padded launch of the same sequences (queryLengths, rows = the largest count): the sink
entries when a window, sink tokens or sink logits are set, the plain entries otherwise.  Sequences have distinct random Q rows and
distinct caches, so a row served with another sequence's start, length, block-table row or scale differs in every element.

Batches (n keys, qn rows).  G = 8 (RB = 16) and G = 3 (RB = 42): (700, 40), (200, 17), (65, 1), (0, 0), (30, 16), (10, 33) -- fewer keys
than rows -- and (0, 3), rows without any key.  G = 1 (RB = 128): qn = 130, 0, 1, 128.  Caches hold NaN / 0x7f at and past every length;
the packed Q holds NaN in every row no sequence owns; O and L are pre-filled with sentinels and carry 64 sentinel rows before and
after.  Parity with the float64 model runs on the batch, the poisoned caches and the needle queries of tests/test_sink_gpu.py
(tests/cache_kit.py holds them), packed.
Maxima seen on an MI355X: DESIGN.md 4.14."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import decode_model as dm  # noqa: E402
import cache_kit as ck  # noqa: E402  (the sink batch, its poisoned caches, needle queries and bounds: the parity cases run on them)
import ragged_model as rm  # noqa: E402
import sink_model as sm  # noqa: E402
from cache_kit import FLT_MAX, PREC, SENT_L, SENT_O, bits, lengths  # noqa: E402
from metal_flash_attention_amd import AttentionPrefill, KVCacheAppend, KVCachePrecision  # noqa: E402

BATCH = list(ck.RAGGED_BATCH.SEQS)
BATCH_G1 = [(700, 130), (200, 0), (65, 1), (300, 128)]
C, HKV, PAGE, PADROWS = ck.RAGGED_BATCH.C, ck.RAGGED_BATCH.HKV, 16, 64
SETTINGS = [(0, 0, False), (130, 0, False), (130, 4, True), (0, 0, True)]        # (W, S, logits)
# (D, dtype, G, e4m3 cache, paged 16): every value of every dimension, both caches and both layouts under every G
VARIANTS = [(64, torch.bfloat16, 8, False, False), (128, torch.float16, 8, False, True), (128, torch.bfloat16, 8, True, True),
            (64, torch.float16, 8, True, False), (64, torch.float16, 3, True, True), (128, torch.bfloat16, 3, False, False),
            (64, torch.bfloat16, 1, False, True), (128, torch.float16, 1, True, False)]
SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield
    if SEEN:
        print("\nragged parity, worst err / bound at margin 1:", {k: round(v, 4) for k, v in SEEN.items()})


def batch_of(G):
    return BATCH_G1 if G == 1 else BATCH


@functools.lru_cache(maxsize=None)
def caches(D, dtype, fp8, G, paged):
    """device K, V of the batch with poison at and past every length, the launch keywords of the layout, and the per-head scales"""
    batch = ck.Batch(tuple(batch_of(G)), C, HKV, None)
    g = torch.Generator().manual_seed(D + 3 * G + 11 * fp8)
    rnd = lambda: torch.rand(batch.B, HKV, C, D, generator=g) * 2 - 1  # noqa: E731
    if fp8:
        k, v = (rnd() * 3).to(torch.float8_e4m3fn), (rnd() * 3).to(torch.float8_e4m3fn)
        rng = np.random.default_rng(D + G)
        scales = tuple(torch.from_numpy(dm.spread_scales(rng, HKV)).cuda() for _ in range(2))
    else:
        k, v, scales = rnd().to(dtype), rnd().to(dtype), (None, None)
    if paged:   # a shuffled pool that holds the pages below each length only; every other table entry names an all-poison page
        return ck.paged_pool(k, v, PAGE, batch.keep(), seed=D + G + fp8) + (scales,)
    return ck.poisoned(k, batch.keep()).cuda(), ck.poisoned(v, batch.keep()).cuda(), {}, scales


def extras(W, S, logits, Hq, padded_entry):
    """the window / sink keywords of a launch; the padded launch goes through the sink entries iff any of them is set"""
    lg = torch.from_numpy(ck.sink_logits(Hq, W + S)).cuda() if logits else None
    if padded_entry and not (W or S or logits):
        return {}, lg
    kw = {}
    if W:
        kw.update(window=W)
    if S or logits:
        kw.update(sinkTokens=S, sinkLogits=lg)
    if padded_entry and not kw.get("sinkTokens") and not logits:
        kw.update(sinkTokens=0)   # (W alone: still the sink entries, as the identity is stated)
    return kw, lg


def op_of(D, dtype, fp8, out=None):
    return AttentionPrefill(D, PREC[dtype], out, cachePrecision=KVCachePrecision.E4M3 if fp8 else None)


def padded_launch(q, k, v, lens, qlens, G, fp8, scales, cache_kw, ext):
    """-> (O, L) [B, Hq, R, D], [B, Hq, R] on the device, from sentinel-filled buffers: the launch that exists"""
    B, Hq, R, D = q.shape
    o = torch.full((B, Hq, R, D), SENT_O, dtype=q.dtype, device="cuda")
    l = torch.full((B, Hq, R), SENT_L, dtype=torch.float32, device="cuda")
    kw = dict(cache_kw)
    kw.update(rows=R, column=C, heads=Hq, batches=B, headsPerKeyValue=G, cacheLengths=lengths(lens), queryLengths=lengths(qlens), **ext)
    if fp8:
        kw.update(keyScale=scales[0], valueScale=scales[1])
    op_of(D, q.dtype, fp8).dispatch(q.cuda(), k, v, o, l, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    return o, l


def ragged_launch(qp, k, v, lens, starts, T, cap, G, fp8, scales, cache_kw, ext, column=C):
    """qp [T, Hq, D] packed -> (O buffer [64 + T + 64, Hq, D], L buffer [Hq, 64 + T + 64]) on the device, sentinels around the T rows"""
    Tq, Hq, D = qp.shape
    pad = torch.full((PADROWS, Hq, D), float("nan"), dtype=qp.dtype)
    qb = torch.cat([pad, qp, pad]).cuda()
    ob = torch.full((Tq + 2 * PADROWS, Hq, D), SENT_O, dtype=qp.dtype, device="cuda")
    lb = torch.full((Hq, Tq + 2 * PADROWS), SENT_L, dtype=torch.float32, device="cuda")
    kw = dict(cache_kw)
    kw.update(rows=cap, column=column, heads=Hq, batches=len(lens), headsPerKeyValue=G, cacheLengths=lengths(lens), rowStarts=lengths(starts), totalRows=T,
              lStrides=(Tq + 2 * PADROWS, 0), **ext)
    if fp8:
        kw.update(keyScale=scales[0], valueScale=scales[1])
    op = op_of(D, qp.dtype, fp8)
    assert op.launchForm(**kw).startswith("attn_prefill16r_d%d_" % D)
    op.dispatch(qb[PADROWS:], k, v, ob[PADROWS:], lb[:, PADROWS:], stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    return ob, lb


def identity_case(variant, setting, *, total=None, cap=None):
    """the ragged launch of the batch against the padded launch of the sequences the RULE gives (T and the cap may cut them)"""
    (D, dtype, G, fp8, paged), (W, S, logits) = VARIANTS[variant], SETTINGS[setting]
    batch = batch_of(G)
    lens, counts = [n for n, _ in batch], [qn for _, qn in batch]
    Hq, B = HKV * G, len(batch)
    starts = rm.row_starts(counts)
    Tq = starts[-1]                                   # the rows the buffers hold
    T = Tq if total is None else total                # what the launch is told
    cap = max(counts) if cap is None else cap
    owned = rm.counts_of(starts, T, cap)              # [(s_b, qn_b)]
    qlens, R = [qn for _s, qn in owned], max(max(qn for _s, qn in owned), 1)
    k, v, cache_kw, scales = caches(D, dtype, fp8, G, paged)
    g = torch.Generator().manual_seed(variant)
    qp = (torch.rand(Tq, Hq, D, generator=g) * 2 - 1).to(dtype)
    mine = np.zeros(Tq, dtype=bool)
    mine[:T] = rm.owned(starts, T, cap)
    qp[torch.from_numpy(~mine)] = float("nan")        # a row no sequence owns is never read
    qpad = torch.from_numpy(rm.unpack(qp.view(torch.int16).numpy(), starts, T, cap, R)).view(dtype)
    want_o, want_l = padded_launch(qpad, k, v, lens, qlens, G, fp8, scales, cache_kw, extras(W, S, logits, Hq, True)[0])
    ob, lb = ragged_launch(qp, k, v, lens, starts, T, cap, G, fp8, scales, cache_kw, extras(W, S, logits, Hq, False)[0])
    ob, lb, want_o, want_l = ob.cpu(), lb.cpu(), want_o.cpu(), want_l.cpu()
    # nothing else is written: the sentinel rows around, rows at or past T, rows past the cap
    keep = torch.ones(Tq + 2 * PADROWS, dtype=torch.bool)
    for s, qn in owned:
        keep[PADROWS + s:PADROWS + s + qn] = False
    assert bool((ob[keep].float() == SENT_O).all()) and bool((lb[:, keep] == SENT_L).all()), "a row no sequence owns was written"
    for b, (s, qn) in enumerate(owned):
        if qn == 0:
            continue
        got_o, got_l = ob[PADROWS + s:PADROWS + s + qn].transpose(0, 1), lb[:, PADROWS + s:PADROWS + s + qn]
        assert bool(torch.isfinite(got_o.float()).all()) and bool(torch.isfinite(got_l).all()), f"sequence {b}: poison reached a live row"
        if lens[b] == 0 and not logits:               # rows without a visible key
            assert not got_o.float().any() and bool((got_l == -FLT_MAX).all()), f"sequence {b}: a row without a visible key"
            if not (W or S):
                continue                              # (the plain identity is stated for rows that see a key)
        assert torch.equal(bits(got_o), bits(want_o[b, :, :qn])), f"sequence {b} (n {lens[b]}, qn {qn}, start {s}): O differs from the padded launch"
        assert torch.equal(got_l, want_l[b, :, :qn]), f"sequence {b} (n {lens[b]}, qn {qn}, start {s}): L differs from the padded launch"
    return owned


@pytest.mark.parametrize("setting", range(len(SETTINGS)))
@pytest.mark.parametrize("variant", range(len(VARIANTS)))
def test_byte_identity_with_the_padded_launch(variant, setting):
    identity_case(variant, setting)


@pytest.mark.parametrize("variant", [1, 4, 6])
def test_rows_at_or_past_total_rows_and_past_the_cap_keep_their_sentinels(variant):
    G = VARIANTS[variant][2]
    counts = [qn for _, qn in batch_of(G)]
    starts = rm.row_starts(counts)
    # totalRows below the end of the last sequence, which keeps 2 rows, and below its start: it loses every row, the one before it one
    owned = identity_case(variant, 2, total=starts[-2] + 2)
    assert owned[-1][1] == 2 < counts[-1]
    owned = identity_case(variant, 2, total=starts[-2] - 1)
    assert owned[-1][1] == 0 and owned[-2][1] == counts[-2] - 1
    # a cap below the largest count: that sequence's later rows stay as they were
    cap = max(counts) - 13
    owned = identity_case(variant, 2, cap=cap)
    assert max(qn for _s, qn in owned) == cap < max(counts)


@pytest.mark.parametrize("variant", range(len(ck.SINK_VARIANTS)))
def test_parity_with_the_float64_model_on_poisoned_caches(variant):
    """the batch of tests/test_sink_gpu.py, packed, under W = 130 with S = 4 and a sink logit per head: one configuration per D and
    type, at the committed bounds and margin of sink_model.compare, on caches poisoned in every tile no workgroup walks"""
    batch, (W, S), (D, dtype, G, _Rd, fp8) = ck.SINK_BATCH, (130, 4), ck.SINK_VARIANTS[variant]
    R = batch.RP
    k, v, scales = ck.base(batch, D, dtype, fp8)
    sd = (ck.dev(scales[0]), ck.dev(scales[1]))
    keep = batch.keep(tiles=ck.walked(batch, "prefill", G, R, W, S))
    q, sink, ref, info = ck.sink_reference(batch, "prefill", D, dtype, G, R, W, S, fp8)
    counts = [min(qn, R) for qn in batch.QLENS]
    starts = rm.row_starts(counts)
    T = starts[-1]
    qp = torch.from_numpy(rm.pack(q.view(torch.int16).numpy(), starts, T, R)).view(dtype)
    ext = dict(window=W, sinkTokens=S, sinkLogits=ck.dev(sink))
    results = []
    for paged in (False, True):
        if paged:
            kd, vd, kw = ck.paged_pool(k, v, 16, keep, seed=variant)
        else:
            kd, vd, kw = ck.poisoned(k, keep).cuda(), ck.poisoned(v, keep).cuda(), {}
        ob, lb = ragged_launch(qp, kd, vd, batch.LENS, starts, T, R, G, fp8, sd, kw, ext, column=batch.C)
        ob, lb = ob.cpu()[PADROWS:PADROWS + T], lb.cpu()[:, PADROWS:PADROWS + T]
        o = torch.from_numpy(rm.unpack(ob.view(torch.int16).numpy(), starts, T, R, R, fill=0)).view(dtype)
        l = torch.from_numpy(rm.unpack_l(lb.numpy(), starts, T, R, R, fill=SENT_L))
        for b, qn in enumerate(counts):               # (cache_kit.hold wants its sentinels at and past qn)
            o[b, :, qn:] = SENT_O
            l[b, :, qn:] = SENT_L
        ck.hold(batch, "prefill", o, l, ref, dtype, dtype, info, "ragged" + (" e4m3 cache" if fp8 else " 16-bit cache"), sm, SEEN, ck.sink_blind(W, S), sink)
        results.append((ob, lb))
    assert torch.equal(bits(results[0][0]), bits(results[1][0])) and torch.equal(results[0][1], results[1][1]), "paged 16 differs from the contiguous launch"


# ---------------------------------------------------------------------------------------------------------------------- the append
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("D,dtype", [(64, torch.float16), (128, torch.bfloat16)])
def test_append_is_the_per_sequence_append_byte_for_byte(D, dtype, fp8, paged):
    ck.append_is_the_per_sequence_append(ck.RAGGED_BATCH, D, dtype, fp8, paged)


def test_append_then_ragged_prefill_in_one_graph():
    """the pair captured in one torch.cuda.graph and replayed once matches the eager pair: both launches are asynchronous, copy nothing
    to the host and read the starts and lengths on the device"""
    D, dtype, G, fp8 = 128, torch.bfloat16, 8, True
    Hq = HKV * G
    kn, vn, lens, counts, starts, T, kc, vc, kw = ck.append_case(ck.RAGGED_BATCH, D, dtype, fp8, True, 5)
    fill = kc.clone()
    g = torch.Generator().manual_seed(9)
    q = (torch.rand(T, Hq, D, generator=g) * 2 - 1).to(dtype).cuda()
    dlens, dstarts = lengths(lens), lengths(starts)
    app, pre = KVCacheAppend(D, PREC[dtype], KVCachePrecision.E4M3), op_of(D, dtype, True)
    logits = torch.from_numpy(ck.sink_logits(Hq)).cuda()
    pkw = dict(kw)
    pkw["strides"] = dict(K=kw["strides"]["kCache"], V=kw["strides"]["vCache"])

    def pair(o, l):
        stream = torch.cuda.current_stream().cuda_stream
        app.dispatch(kn, vn, kc, vc, stream=stream, rows=max(counts), heads=HKV, batches=len(lens), cacheLengths=dlens, rowStarts=dstarts,
                     totalRows=T, **kw)
        pre.dispatch(q, kc, vc, o, l, stream=stream, rows=max(counts), column=C, heads=Hq, batches=len(lens), headsPerKeyValue=G,
                     cacheLengths=dlens, rowStarts=dstarts, totalRows=T, window=130, sinkTokens=4, sinkLogits=logits, **pkw)

    # (the e4m3 sentinel bytes below each length are what the sequences "already hold": finite values)
    o0, l0 = torch.full((T, Hq, D), SENT_O, dtype=dtype, device="cuda"), torch.full((Hq, T), SENT_L, dtype=torch.float32, device="cuda")
    pair(o0, l0)
    torch.cuda.synchronize()
    eager_k, eager_v = kc.clone(), vc.clone()
    kc.copy_(fill)
    vc.copy_(fill)
    o1, l1 = torch.full_like(o0, SENT_O), torch.full_like(l0, SENT_L)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pair(o1, l1)
    kc.copy_(fill)
    vc.copy_(fill)
    o1.fill_(SENT_O)
    l1.fill_(SENT_L)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(kc, eager_k) and torch.equal(vc, eager_v)
    assert torch.equal(bits(o1), bits(o0)) and torch.equal(l1, l0)
    live = torch.from_numpy(rm.owned(starts, T, max(counts)))
    assert bool(torch.isfinite(o1.cpu()[live].float()).all()) and bool((o1.cpu()[~live].float() == SENT_O).all())
