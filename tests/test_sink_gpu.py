"""GPU test: attention sinks over a KV cache through the C ABI of include/mfa_sink.h (the sinkTokens= / sinkLogits= keywords of
AttentionDecode, AttentionDecodeFP8 and AttentionPrefill).

One batch of sequences (n, qn): (700, 40) and (1500, 129) with a gap between the sink tiles and the window; (200, 40), where under
W = 130, S = 70 the sink keys reach into the window's first tile (the zones touch); (100, 130): fewer keys than rows, rows that see
their sink keys alone; (5, 5) and (0, 3): S > n, and no key at all.  Three settings: W = 130 with S = 4 (sink tile 0, at n = 700 the
window from tile 8, tiles 1-7 never loaded), S = 70 (two sink tiles, the second partial) and S = 2000 (past every key).  Decode
launches use the lengths with R = 1 or 4 rows.  Expected values: tests/sink_model.py on the inputs after their rounding; every output
element and every L of every live row is held to decode_model.bounds at sink_model.MARGIN, on needle queries, for D 64 / 128 x bf16 /
f16 x G 1 / 8 x 16-bit / e4m3 caches, with a sink logit per query head.

Poison.  Every parity launch runs on caches that hold NaN (16-bit) or 0x7f (e4m3) in every key and value at or past each length AND
in every 64-key tile no workgroup of the sequence walks -- below the window outside the sink tiles.  Paged pools (page 16) hold the
walked tiles' keys only; every other block-table entry names a valid page of the pool that is all poison.  Results must be finite,
inside the bounds, and byte-identical between the layouts.  Maxima seen on an MI355X: DESIGN.md 4.13."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import decode_model as dm  # noqa: E402
import sink_model as sm  # noqa: E402
from metal_flash_attention_amd import AttentionDecode, AttentionDecodeFP8, AttentionPrefill, GEMMOperandPrecision as P, KVCachePrecision  # noqa: E402

LOG2E = 1.4426950408889634
FLT_MAX = float(np.finfo(np.float32).max)
SEQS = [(700, 40), (200, 40), (100, 130), (5, 5), (0, 3), (1500, 129)]
LENS, QLENS = [s[0] for s in SEQS], [s[1] for s in SEQS]
B, C, RP, HKV, TILE = len(SEQS), 1536, 130, 2, 64
PREC = {torch.bfloat16: P.BF16, torch.float16: P.FP16}
SENT_O, SENT_L = -7.25, 12345.5
SETTINGS = [(130, 4), (130, 70), (130, 2000)]                       # (W, S)
# (D, dtype, G, decode R, e4m3 cache): every value of every dimension with both caches
VARIANTS = [(64, torch.bfloat16, 1, 1, False), (128, torch.float16, 8, 4, False), (128, torch.bfloat16, 8, 1, True), (64, torch.float16, 1, 4, True)]
SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield
    if SEEN:
        print("\nsink worst err / bound at margin 1:", {k: round(v, 4) for k, v in SEEN.items()})


def lengths(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


@functools.lru_cache(maxsize=None)
def base(D, dtype, fp8, seed=0):
    """k, v [B, HKV, C, D] (CPU) of the 16-bit type or e4m3, every key a value; per-head scales (float32 numpy) for e4m3, else None"""
    g = torch.Generator().manual_seed(seed + D + 7 * fp8)
    rnd = lambda: (torch.rand(B, HKV, C, D, generator=g) * 2 - 1)  # noqa: E731
    if fp8:
        rng = np.random.default_rng(seed + D)
        return (rnd() * 3).to(torch.float8_e4m3fn), (rnd() * 3).to(torch.float8_e4m3fn), (dm.spread_scales(rng, HKV), dm.spread_scales(rng, HKV))
    return rnd().to(dtype), rnd().to(dtype), (None, None)


def sink_logits(Hq, seed=0):
    """one logit per query head, natural units: a share of the softmax mass of the order of the needles'"""
    return np.random.default_rng(40 + seed).uniform(1.0, 4.0, Hq).astype(np.float32)


def walked(kind, n, qn, G, R, W, S):
    """[C // 64] bool: the 64-key tiles some workgroup of the sequence walks (from the host's range functions)"""
    out = np.zeros(C // TILE, dtype=bool)
    if kind == "decode":
        ranges = AttentionDecode.sinkPieceRange(n, R, W, S, 1, 0)
    else:
        RB, ranges = 128 // G, []
        for r0 in range(0, min(qn, R), RB):
            b, _u0, _u1, e, se = AttentionPrefill.sinkTileRange(n, min(qn, R), r0, RB, W, S)
            ranges += [(0, se * TILE), (b * TILE, e * TILE)]
    for b, e in ranges:
        out[b // TILE:-(-min(e, n) // TILE)] = True
    return out


def poison_of(t):
    return 0x7F if t.dtype == torch.float8_e4m3fn else float("nan")


def raw(t):
    return t.view(torch.uint8) if t.dtype == torch.float8_e4m3fn else t


def poisoned(t, tiles):
    """a copy with poison in every tile that is not walked (tiles[b]) and at or past LENS[b]"""
    out = raw(t.clone())
    for b, n in enumerate(LENS):
        keep = torch.from_numpy(np.repeat(tiles[b], TILE) & (np.arange(C) < n))
        out[b][:, ~keep] = poison_of(t)
    return out.view(t.dtype)


def paged_pool(k, v, page, tiles, seed):
    """shuffled pools [pages, HKV, page, D] that hold the keys of the walked tiles below n_b only, poison everywhere else, and the block
    table: an entry whose page holds no such key names page `spare`, a page of the pool that is all poison"""
    rng = np.random.default_rng(seed)
    D, pps = k.shape[3], C // page
    total = B * pps + 1
    spare = total - 1
    perm = rng.permutation(total - 1)
    pk = raw(torch.empty((total, HKV, page, D), dtype=k.dtype))
    pk[:] = poison_of(k)
    pv = pk.clone()
    table = np.full((B, pps), spare, dtype=np.int32)
    for b, n in enumerate(LENS):
        for i in range(pps):
            a, e = i * page, min((i + 1) * page, n)
            if e > a and tiles[b][a // TILE]:
                pg = int(perm[b * pps + i])
                table[b, i] = pg
                pk[pg, :, :e - a] = raw(k)[b, :, a:e]
                pv[pg, :, :e - a] = raw(v)[b, :, a:e]
    kw = dict(pageSize=page, blockTable=torch.from_numpy(table).cuda(), blockTableStride=pps, pageStrides=(HKV * page * D, HKV * page * D),
              strides=dict(K=(D, page * D, 0), V=(D, page * D, 0)))
    return pk.view(k.dtype).cuda(), pv.view(k.dtype).cuda(), kw


def launch(kind, q, k, v, G, *, W=None, S=None, logits=None, out=None, workspace=False, cache_kw=None, scales=(None, None), want_pieces=None,
           causal=True, entry="sink"):
    """-> (O, L base-2) (CPU) as the launch left them on sentinel-filled buffers.  entry "sink": the sink entries (W None: window 0);
    "window": the window entries; "plain": the entries without a window.  k, v on the device"""
    Bq, Hq, R, D = q.shape
    fp8 = k.dtype == torch.float8_e4m3fn
    odt = out or q.dtype
    o = torch.full((Bq, Hq, R, D), SENT_O, dtype=odt, device="cuda")
    l = torch.full((Bq, Hq, R), SENT_L, dtype=torch.float32, device="cuda")
    kw = dict(cache_kw or {})
    kw.update(rows=R, column=C, heads=Hq, batches=Bq, headsPerKeyValue=G, causal=causal, cacheLengths=lengths(LENS))
    if entry != "plain" and W is not None:
        kw.update(window=W)
    if entry == "sink":
        kw.update(sinkTokens=S or 0, sinkLogits=logits)
    outp = None if out is None else PREC.get(out, P.FP32)
    if kind == "decode":
        op = (AttentionDecodeFP8 if fp8 else AttentionDecode)(D, PREC[q.dtype], outp)
        if fp8:
            kw.update(keyScale=scales[0], valueScale=scales[1])
        if workspace:
            need = op.workspaceSize(**kw)
            if want_pieces is not None:
                assert need == want_pieces * Bq * Hq * R * (D + 2) * 4
                assert want_pieces == 0 or ("x %d pieces" % want_pieces) in op.launchForm(workspace=0x1000, workspaceBytes=need, **kw)
            if need:
                kw.update(workspace=torch.empty(need, dtype=torch.uint8, device="cuda"))
    else:
        op = AttentionPrefill(D, PREC[q.dtype], outp, cachePrecision=KVCachePrecision.E4M3 if fp8 else None)
        kw.update(queryLengths=lengths(QLENS))
        if fp8:
            kw.update(keyScale=scales[0], valueScale=scales[1])
    op.dispatch(q.cuda(), k, v, o, l, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    return o.cpu(), l.cpu()


def qlens_of(kind):
    return None if kind == "decode" else QLENS


@functools.lru_cache(maxsize=None)
def reference(kind, D, dtype, G, R, W, S, fp8, with_logits=True, pieces=None, causal=True, qkind="needle"):
    """(q, sink logits, model, needle info), computed once per case and shared; the model reads the values a cache stands for"""
    k, v, (ks, vs) = base(D, dtype, fp8)
    fmt, Hq = dm.fmt_of(dtype), HKV * G
    sink = sink_logits(Hq, D + G) if with_logits else None
    info = None
    if qkind == "needle":
        seen = k.float().numpy().astype(np.float64) * (ks[None, :, None, None] if fp8 else 1.0)
        q64, info = sm.needle_queries(seen, LENS, qlens_of(kind), Hq, G, R, W, S, fmt, pieces=pieces, page=16)
        q = torch.from_numpy(q64).to(dtype)
        assert torch.equal(q.to(torch.float64), torch.from_numpy(q64))
    else:
        q = (torch.rand(B, Hq, R, D, generator=torch.Generator().manual_seed(D + G + W)) * 2 - 1).to(dtype)
    ref = sm.model(q, k.float(), v.float(), LENS, qlens_of(kind), G, W, S, sink, causal=causal, pieces=pieces, kscale=ks, vscale=vs)
    return q, sink, ref, info


def dev(x):
    return None if x is None else torch.from_numpy(x).cuda()


def hold(kind, o, l, ref, dtype, out, info, tag, sink, W, S, causal=True):
    """sentinels kept at and past qn; live rows finite; a live row without a visible key holds O = 0 and L = its sink logit (base 2), or
    -FLT_MAX without logits; every live row inside the bounds"""
    R = o.shape[2]
    for b, (n, qn) in enumerate(SEQS):
        qn = R if kind == "decode" else min(qn, R)
        assert bool((o[b, :, qn:].float() == SENT_O).all()) and bool((l[b, :, qn:] == SENT_L).all()), f"sequence {b}: rows at or past {qn} were written"
        assert bool(torch.isfinite(o[b, :, :qn].float()).all()) and bool(torch.isfinite(l[b, :, :qn]).all()), f"sequence {b}: poison reached a live row"
        lo, lim = sm.frontiers(n, qn, np.arange(qn), W, causal)
        blind = torch.from_numpy(np.array([sm.visible_keys(int(a), int(e), S).size == 0 for a, e in zip(lo, lim)]))[None, :].expand(o.shape[1], -1)
        assert not o[b, :, :qn][blind].float().any(), f"sequence {b}: a row without a visible key"
        if sink is None:
            assert bool((l[b, :, :qn][blind] == -FLT_MAX).all()), f"sequence {b}: a row without a visible key"
        else:
            want = torch.from_numpy(sink)[:, None].expand(-1, qn)[blind] * np.float32(LOG2E)
            assert torch.allclose(l[b, :, :qn][blind], want, rtol=1e-6, atol=0), f"sequence {b}: a row without a visible key must hold L = its sink logit"
    fmt = dm.fmt_of(dtype)
    wo, wl, text = sm.compare(o, l / LOG2E, ref, fmt, "f32" if out == torch.float32 else fmt, LENS, qlens_of(kind), margin=1, info=info)
    SEEN[tag] = max(SEEN.get(tag, 0.0), wo, wl)
    print("%s: worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % (tag, wo, wl))
    assert wo <= sm.MARGIN and wl <= sm.MARGIN, text


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("setting", range(len(SETTINGS)))
@pytest.mark.parametrize("kind", ["decode", "prefill"])
def test_parity_with_the_model_on_poisoned_caches(kind, setting, variant):
    (W, S), (D, dtype, G, Rd, fp8) = SETTINGS[setting], VARIANTS[variant]
    R = Rd if kind == "decode" else RP
    k, v, scales = base(D, dtype, fp8)
    sd = (dev(scales[0]), dev(scales[1]))
    tiles = [walked(kind, n, qn, G, R, W, S) for n, qn in SEQS]
    if (W, S) == (130, 4):
        assert tiles[0][0] and not tiles[0][1:8].any() and tiles[0][8:11].all()   # n = 700: sink tile 0, tiles 1-7 poisoned, the window from tile 8
    if (W, S) == (130, 70):
        assert tiles[0][:2].all() and not tiles[0][2:8].any() and tiles[1][:4].all()   # two sink tiles over a gap; n = 200: the zones touch
    q, sink, ref, info = reference(kind, D, dtype, G, R, W, S, fp8)
    tag = kind + (" e4m3 cache" if fp8 else " 16-bit cache")
    kd, vd = poisoned(k, tiles).cuda(), poisoned(v, tiles).cuda()
    o, l = launch(kind, q, kd, vd, G, W=W, S=S, logits=dev(sink), scales=sd)
    hold(kind, o, l, ref, dtype, dtype, info, tag, sink, W, S)
    o32, l32 = launch(kind, q, kd, vd, G, W=W, S=S, logits=dev(sink), scales=sd, out=torch.float32)   # (unsplit: no workspace is offered)
    hold(kind, o32, l32, ref, dtype, torch.float32, info, tag, sink, W, S)
    kp, vp, kw = paged_pool(k, v, 16, tiles, seed=setting + 3 * variant)
    o2, l2 = launch(kind, q, kp, vp, G, W=W, S=S, logits=dev(sink), scales=sd, cache_kw=kw)
    assert torch.equal(o2.view(torch.int16), o.view(torch.int16)) and torch.equal(l2, l), "paged 16 differs from the contiguous launch"


@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("fp8", [False, True])
def test_decode_pieces_one_straddles_the_gap_and_one_is_empty(fp8, R):
    """W = 640, S = 4 plans three pieces at column 1536 (from 12 or 13 tiles over 12 workgroups).  n = 1500: piece 0 takes the sink tile
    and the window's first tiles; n = 100: piece 0 is empty and publishes the sink logit alone; n = 0: every piece is empty"""
    D, dtype, G, W, S = (128, torch.bfloat16, 8, 640, 4) if R == 4 else (64, torch.float16, 1, 640, 4)
    k, v, scales = base(D, dtype, fp8)
    pairs = [AttentionDecode.sinkPieceRange(1500, R, W, S, 3, p) for p in range(3)]
    assert pairs[0][0] == (0, 64) and pairs[0][1][1] > pairs[0][1][0] >= 832, pairs          # piece 0 straddles the gap
    assert AttentionDecode.sinkPieceRange(100, R, W, S, 3, 0) == ((0, 0), (0, 0))               # an empty piece 0
    tiles = [walked("decode", n, qn, G, R, W, S) for n, qn in SEQS]
    assert tiles[5][0] and not tiles[5][1:13].any()
    q, sink, ref, info = reference("decode", D, dtype, G, R, W, S, fp8, True, 3)
    for out in (None, torch.float32):
        o, l = launch("decode", q, poisoned(k, tiles).cuda(), poisoned(v, tiles).cuda(), G, W=W, S=S, logits=dev(sink), out=out, workspace=True,
                      want_pieces=3, scales=(dev(scales[0]), dev(scales[1])))
        hold("decode", o, l, ref, dtype, out or dtype, info, "decode pieces" + (" e4m3" if fp8 else ""), sink, W, S)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("kind", ["decode", "prefill"])
def test_byte_identities(kind, fp8):
    """no sinks through the sink entries = the window entry of the same W (W = 0: the plain launch); logits of -1e30 = no logits, for O
    and L, on every row that sees a key -- against the SINK kernels without logits and, at S = 0, against the WINDOW kernels"""
    D, dtype, G = 128, torch.float16, 8
    R = 4 if kind == "decode" else RP
    k, v, scales = base(D, dtype, fp8)
    sd = (dev(scales[0]), dev(scales[1]))
    q = reference(kind, D, dtype, G, R, 130, 4, fp8, qkind="uniform")[0]
    zeros = [np.ones(C // TILE, dtype=bool)] * B
    kd, vd = poisoned(k, zeros).cuda(), poisoned(v, zeros).cuda()
    never = torch.full((HKV * G,), -1e30, dtype=torch.float32, device="cuda")
    sees = torch.zeros((B, HKV * G, R), dtype=torch.bool)
    for b, (n, qn) in enumerate(SEQS):
        sees[b, :, :(R if kind == "decode" else min(qn, R)) if n else 0] = True
    same = lambda a, b: torch.equal(a[0].view(torch.int16)[sees], b[0].view(torch.int16)[sees]) and torch.equal(a[1][sees], b[1][sees])  # noqa: E731
    for W in (0, 130):
        window = launch(kind, q, kd, vd, G, W=W, scales=sd, entry="window" if W else "plain")
        none = launch(kind, q, kd, vd, G, W=W, S=0, logits=None, scales=sd)
        assert torch.equal(none[0].view(torch.int16), window[0].view(torch.int16)) and torch.equal(none[1], window[1]), f"W = {W}: no sinks differs"
        assert same(launch(kind, q, kd, vd, G, W=W, S=0, logits=never, scales=sd), window), f"W = {W}: logits of -1e30 differ from the window kernels"
    tokens = launch(kind, q, kd, vd, G, W=130, S=4, scales=sd)
    assert not same(tokens, window)
    assert same(launch(kind, q, kd, vd, G, W=130, S=4, logits=never, scales=sd), tokens), "logits of -1e30 differ from no logits"
    if kind == "decode":   # and in pieces: piece 0 folds a term of exactly 0
        split = launch(kind, q, kd, vd, G, W=640, S=4, scales=sd, workspace=True, want_pieces=3)
        assert same(launch(kind, q, kd, vd, G, W=640, S=4, logits=never, scales=sd, workspace=True, want_pieces=3), split)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("kind", ["decode", "prefill"])
def test_the_fused_logit_against_what_a_caller_could_do_from_l(kind, causal):
    """sink logits without a window (causal or not): the fused launch and the caller's O 2^L / (2^L + 2^s2) from the plain launch's
    FP32 O and L both lie inside the model's bounds (so they agree within twice the bound; they are not byte-identical).  A row
    without a key: the fused launch gives O = 0, L = s2, where the caller's formula divides 0 by 0"""
    D, dtype, G = 64, torch.bfloat16, 8
    R = 4 if kind == "decode" else RP
    k, v, _ = base(D, dtype, False)
    q, sink, ref, _info = reference(kind, D, dtype, G, R, 0, 0, False, True, None, causal, "uniform")
    tiles = [np.ones(C // TILE, dtype=bool)] * B
    kd, vd = poisoned(k, tiles).cuda(), poisoned(v, tiles).cuda()
    o, l = launch(kind, q, kd, vd, G, logits=dev(sink), out=torch.float32, causal=causal)
    hold(kind, o, l, ref, dtype, torch.float32, None, kind + " logits only", sink, 0, 0, causal)
    po, pl = launch(kind, q, kd, vd, G, out=torch.float32, causal=causal, entry="plain")
    s2 = (torch.from_numpy(sink).double() * LOG2E)[None, :, None]
    with np.errstate(all="ignore"):
        w = 1.0 / (1.0 + torch.exp2(s2 - pl.double()))
        co, cl = po.double() * w[..., None], torch.logaddexp(pl.double() / LOG2E, s2 / LOG2E)
    keyed = torch.tensor([n > 0 for n in LENS])
    for b in range(B):   # (sequences without a key: the caller has nothing to rescale; rows at and past qn hold sentinels)
        if not keyed[b]:
            co[b], cl[b] = o[b].double(), l[b].double() / LOG2E
        co[b, :, ref.L.shape[2] if kind == "decode" else min(QLENS[b], R):] = 0
    wo, wl, text = sm.compare(co.numpy(), cl.numpy(), ref, dm.fmt_of(dtype), "f32", LENS, qlens_of(kind), margin=1)
    assert wo <= sm.MARGIN and wl <= sm.MARGIN, text
    live = torch.isfinite(torch.from_numpy(ref.L)) & keyed[:, None, None]
    assert not torch.equal(co.float()[live], o[live]) or not torch.equal((cl * LOG2E).float()[live], l[live])
