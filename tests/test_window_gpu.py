"""GPU test: sliding-window attention over a KV cache through the C ABI of include/mfa_window.h (the window= keyword of AttentionDecode,
AttentionDecodeFP8 and AttentionPrefill).

One batch of sequences (n, qn) reaches the seams: empty (0, 1); fewer keys than rows (2, 3), (100, 200) -- rows without a visible key;
(5, 5), (64, 1), (65, 4) around one tile; (300, 129) and (1500, 40) across row blocks, tiles and pages.  Decode launches use the
lengths with R = 4 (or 1) rows.  Expected values: tests/window_model.py on the inputs after their rounding; every output element and
every L of every live row is held to decode_model.bounds at window_model.MARGIN, with uniform and with needle queries, for
D 64 / 128 x bf16 / f16 x G 1 / 4 / 3 x W 1 / 16 / 64 / 65 / 200.

Poison.  Every launch but the seam-identity ones runs on caches that hold NaN (16-bit) or 0x7f (e4m3) in every key and value at or
past each length AND below the first 64-key tile a workgroup of the sequence may load; paged pools hold poison in every page below the
first windowed page, and the block-table entries below it (and past the last page) name a VALID page of the pool that is all poison --
never an index outside the pool.  Results must be finite and inside the bounds.

With W in that grid a sequence spans at most five tiles and the plan has one piece, so those launches are unsplit (with and without a
workspace offered).  Pieces: W = 700 at column 1536 plans three; the short sequences leave pieces empty.  Maxima seen on an MI355X:
DESIGN.md 4.12."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402
import decode_model as dm  # noqa: E402
import window_model as wm  # noqa: E402
from cache_kit import LOG2E, PREC, SENT_L, SENT_O, lengths, poison_of, poisoned, raw, token_major  # noqa: E402
from metal_flash_attention_amd import AttentionDecode, AttentionDecodeFP8, AttentionPrefill  # noqa: E402

SEQS = [(0, 1), (2, 3), (5, 5), (64, 1), (65, 4), (300, 129), (1500, 40), (100, 200)]
LENS, QLENS = [s[0] for s in SEQS], [s[1] for s in SEQS]
B, C, RP, HKV = len(SEQS), 1536, 200, 2
BATCH = ck.Batch(tuple(SEQS), C, HKV, RP)
WINDOWS = [1, 16, 64, 65, 200]
base = functools.partial(ck.base, BATCH)
SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield
    if SEEN:
        print("\nwindow worst err / bound at margin 1:", {k: round(v, 4) for k, v in SEEN.items()})


def first_loaded(kind, n, qn, G, W):
    """the first key any workgroup of the sequence may load under window W (None: no window)"""
    if W is None or n == 0 or qn == 0:
        return 0
    if kind == "decode":
        return AttentionDecode.windowPieceRange(n, qn, W, 1, 0)[0]
    return AttentionPrefill.windowTileRange(n, qn, 0, 128 // G, W)[0] * 64


def launch(kind, q, k, v, G, W, **how):
    """W None: the plain launch (no window= keyword)"""
    return ck.launch(BATCH, kind, q, k, v, G, **({} if W is None else dict(window=W)), **how)


def qlens_of(kind):
    return None if kind == "decode" else QLENS


@functools.lru_cache(maxsize=None)
def reference(kind, D, dtype, G, R, W, qkind, fp8, pieces=None):
    """(q, model, needle info), computed once per case and shared; the model reads the values a cache stands for (poison never enters:
    it only reads a row's window)"""
    k, v, (ks, vs) = base(D, dtype, fp8)
    fmt, Hq = dm.fmt_of(dtype), HKV * G
    info = None
    if qkind == "needle":
        seen = k.float().numpy().astype(np.float64) * (ks[None, :, None, None] if fp8 else 1.0)
        q64, info = wm.needle_queries(seen, LENS, qlens_of(kind), Hq, G, R, W, fmt, pieces=pieces)
        q = torch.from_numpy(q64).to(dtype)
        assert torch.equal(q.to(torch.float64), torch.from_numpy(q64))
    else:
        q = (torch.rand(B, Hq, R, D, generator=torch.Generator().manual_seed(D + G + W)) * 2 - 1).to(dtype)
    ref = wm.model(q, k.float(), v.float(), LENS, qlens_of(kind), G, W, pieces=pieces, kscale=ks, vscale=vs)
    return q, ref, info


def firsts_of(kind, R, G, W):
    return [first_loaded(kind, n, R if kind == "decode" else min(qn, R), G, W) for n, qn in SEQS]


def hold(kind, o, l, ref, dtype, out, info, tag):
    """cache_kit.hold with this file's rule: a live row without a visible key (the model's L is not finite) holds O = 0, L = -FLT_MAX"""
    ck.hold(BATCH, kind, o, l, ref, dtype, out, info, tag, wm, SEEN, lambda b, n, qn: ~np.isfinite(ref.L[b, :, :qn]))


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("G", [1, 4, 3])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kind", ["decode", "prefill"])
def test_parity_with_the_model_on_poisoned_caches(kind, D, dtype, G, W):
    R = 4 if kind == "decode" else RP
    k, v, _ = base(D, dtype, False)
    firsts = firsts_of(kind, R, G, W)
    keep = BATCH.keep(firsts)
    kd, vd = poisoned(k, keep).cuda(), poisoned(v, keep).cuda()
    for qkind in ("needle", "uniform"):
        q, ref, info = reference(kind, D, dtype, G, R, W, qkind, False)
        for out, ws in ((None, False), (torch.float32, True)):
            o, l = launch(kind, q, kd, vd, G, W, out=out, workspace=ws, want_pieces=0 if ws and kind == "decode" else None)
            hold(kind, o, l, ref, dtype, out or dtype, info, kind + " 16-bit cache")


@pytest.mark.parametrize("case", list(enumerate(WINDOWS)))
@pytest.mark.parametrize("kind", ["decode", "prefill"])
@pytest.mark.parametrize("fp8", [False, True])
def test_layouts_and_e4m3_caches(fp8, kind, case):
    """e4m3 caches with spread scales against the model; paged 16 / 256 (poison pages, entries below the window on the spare page) and
    token-major caches byte-identical to the packed launch, whose result is held to the bounds"""
    i, W = case
    D, dtype, G = (64, 128)[i % 2], (torch.bfloat16, torch.float16)[(i // 2) % 2], (1, 4, 3)[i % 3]
    R = 4 if kind == "decode" else RP
    k, v, scales = base(D, dtype, fp8)
    sd = ck.dev_scales(scales)
    firsts = firsts_of(kind, R, G, W)
    keep = BATCH.keep(firsts)
    q, ref, info = reference(kind, D, dtype, G, R, W, "needle", fp8)
    pk, pv = poisoned(k, keep), poisoned(v, keep)
    o, l = launch(kind, q, pk.cuda(), pv.cuda(), G, W, scales=sd)
    hold(kind, o, l, ref, dtype, dtype, info, kind + (" e4m3 cache" if fp8 else " 16-bit cache"))
    for page in (16, 256):
        kp, vp, kw = ck.paged_pool(k, v, page, keep, seed=page + i)
        o2, l2 = launch(kind, q, kp, vp, G, W, scales=sd, cache_kw=kw)
        assert torch.equal(o2.view(torch.int16), o.view(torch.int16)) and torch.equal(l2, l), f"paged {page} differs from the packed launch"
    # token-major [B, C, HKV, D] (poisoned like the packed one), passed by its strides
    (kt, st), (vt, _) = token_major(pk), token_major(pv)
    o3, l3 = launch(kind, q, kt.cuda(), vt.cuda(), G, W, scales=sd, cache_kw=dict(strides=dict(K=st, V=st)))
    assert torch.equal(o3.view(torch.int16), o.view(torch.int16)) and torch.equal(l3, l), "token-major differs from the packed launch"


@pytest.mark.parametrize("kind", ["decode", "prefill"])
@pytest.mark.parametrize("fp8", [False, True])
def test_zero_batch_stride_is_the_packed_launch(fp8, kind):
    """every sequence reads sequence 6's keys (1500 of them) through a batch stride of 0: byte-identical to the packed launch on copies"""
    D, dtype, G, W = 128, torch.bfloat16, 4, 65
    R = 4 if kind == "decode" else RP
    k, v, scales = base(D, dtype, fp8)
    sd = ck.dev_scales(scales)
    q, _ref, _info = reference(kind, D, dtype, G, R, W, "uniform", fp8)
    one = [raw(t)[6:7].clone() for t in (k, v)]
    for t in one:
        t[:, :, 1500:] = poison_of(k)
    packed = [t.expand(B, -1, -1, -1).contiguous().cuda().view(k.dtype) for t in one]
    o, l = launch(kind, q, packed[0], packed[1], G, W, scales=sd)
    shared = [t.cuda().view(k.dtype) for t in one]
    o2, l2 = launch(kind, q, shared[0], shared[1], G, W, scales=sd, cache_kw=dict(strides=dict(K=(D, C * D, 0), V=(D, C * D, 0))))
    assert torch.equal(o2.view(torch.int16), o.view(torch.int16)) and torch.equal(l2, l)


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("kind", ["decode", "prefill"])
def test_a_window_past_every_key_is_the_plain_launch_byte_for_byte(kind, fp8, paged):
    """the ...w kernels with W >= column + rows (any window but 0 runs them) against the plain kernels: the same arithmetic in the same
    order, so O and L are identical bits.  (Poison at and past each length only: the plain launch reads every key below it.)"""
    D, dtype, G = 128, torch.float16, 4
    R = 4 if kind == "decode" else RP
    W = C + R
    k, v, scales = base(D, dtype, fp8)
    sd = ck.dev_scales(scales)
    q, _ref, _info = reference(kind, D, dtype, G, R, 65, "uniform", fp8)
    if paged:
        kd, vd, kw = ck.paged_pool(k, v, 16, BATCH.keep(), seed=3)
    else:
        kd, vd, kw = poisoned(k, BATCH.keep()).cuda(), poisoned(v, BATCH.keep()).cuda(), None
    op = (AttentionDecodeFP8 if fp8 else AttentionDecode)(D, PREC[dtype]) if kind == "decode" else AttentionPrefill(D, PREC[dtype])
    form = op.launchForm(window=W, rows=R, column=C, heads=HKV * G, batches=B, headsPerKeyValue=G, cacheLengths=0x1000)
    assert form.split(" ")[0] in ("attn_decode16w_d128_f16_single", "attn_decode8w_d128_f16_single", "attn_prefill16w_d128_f16"), form
    for ws in ((False, True) if kind == "decode" else (False,)):
        ow, lw = launch(kind, q, kd, vd, G, W, scales=sd, cache_kw=kw, workspace=ws, want_pieces=6 if ws else None)
        op_, lp = launch(kind, q, kd, vd, G, None, scales=sd, cache_kw=kw, workspace=ws)
        assert torch.equal(ow.view(torch.int16), op_.view(torch.int16)) and torch.equal(lw, lp), "the window kernels differ from the plain ones"


@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("fp8", [False, True])
def test_decode_pieces_some_of_them_empty(fp8, R):
    """W = 700 plans three pieces at column 1536 (12 tiles over 16 workgroups); sequences of 0 .. 300 keys leave pieces empty"""
    D, dtype, G, W = (128, torch.bfloat16, 4, 700) if R == 4 else (64, torch.float16, 3, 700)
    k, v, scales = base(D, dtype, fp8)
    firsts = firsts_of("decode", R, G, W)
    keep = BATCH.keep(firsts)
    assert any(AttentionDecode.windowPieceRange(n, R, W, 3, p)[0] == AttentionDecode.windowPieceRange(n, R, W, 3, p)[1] for n in LENS[1:] for p in range(3))
    assert firsts[6] == 768   # 1500 keys: the window starts in tile 12
    q, ref, info = reference("decode", D, dtype, G, R, W, "needle", fp8, 3)
    for out in (None, torch.float32):
        o, l = launch("decode", q, poisoned(k, keep).cuda(), poisoned(v, keep).cuda(), G, W, out=out, workspace=True, want_pieces=3, scales=ck.dev_scales(scales))
        hold("decode", o, l, ref, dtype, out or dtype, info, "decode pieces" + (" e4m3" if fp8 else ""))


def test_decode_and_prefill_agree_on_the_same_buffers():
    """G R = 16 <= 32 packed rows: the decode launch and the prefill launch of the same rows on the same buffers, each inside its own
    model's bounds (the values are one model's; the chains differ)"""
    D, dtype, G, R, W = 128, torch.bfloat16, 4, 4, 65
    k, v, _ = base(D, dtype, False)
    firsts = [min(a, b) for a, b in zip(firsts_of("decode", R, G, W), [first_loaded("prefill", n, R, G, W) for n in LENS])]
    keep = BATCH.keep(firsts)
    kd, vd = poisoned(k, keep).cuda(), poisoned(v, keep).cuda()
    q, ref, info = reference("decode", D, dtype, G, R, W, "needle", False)
    o, l = launch("decode", q, kd, vd, G, W)
    hold("decode", o, l, ref, dtype, dtype, info, "decode 16-bit cache")
    # prefill with every sequence's R rows live: queryLengths = None through a batch-wide override
    pre = AttentionPrefill(D, PREC[dtype])
    o2 = torch.full((B, HKV * G, R, D), SENT_O, dtype=dtype, device="cuda")
    l2 = torch.full((B, HKV * G, R), SENT_L, dtype=torch.float32, device="cuda")
    pre.dispatch(q.cuda(), kd, vd, o2, l2, rows=R, column=C, heads=HKV * G, batches=B, headsPerKeyValue=G, cacheLengths=lengths(LENS), window=W,
                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    pref = wm.model(q, k.float(), v.float(), LENS, [R] * B, G, W)
    assert np.array_equal(pref.O, ref.O)
    fmt = dm.fmt_of(dtype)
    wo, wl, text = wm.compare(o2.cpu(), l2.cpu() / LOG2E, pref, fmt, fmt, LENS, [R] * B, margin=1, info=info)
    SEEN["prefill 16-bit cache"] = max(SEEN.get("prefill 16-bit cache", 0.0), wo, wl)
    assert wo <= wm.MARGIN and wl <= wm.MARGIN, text
    live = torch.tensor([n > 0 for n in LENS])
    assert bool(torch.isfinite(o2.cpu().float()).all()) and float((o2.cpu().float() - o.float())[live].abs().max()) < 0.05
