"""GPU test: logit soft-capping over a KV cache through the C ABI of include/mfa_softcap.h (the softcap= keyword of AttentionDecode,
AttentionDecodeFP8 and AttentionPrefill, ragged included).

The batch is tests/test_sink_gpu.py's, the caches, the poison, the launch and the check tests/cache_kit.py's: sequences (n, qn) = (700, 40),
(200, 40), (100, 130), (5, 5), (0, 3), (1500, 129) in caches of 1536 keys; NaN (16-bit) or 0x7f (e4m3) in every key and value at or
past each length and in every 64-key tile no workgroup walks; paged pools of page 16 whose spare entries name an all-poison page.
Settings (cap, W, S, sink logits): (30, none, 0, no), (50, 130, 4, yes) and (1, 130, 70, yes) -- the last saturates: the needle keys
score 64 caps and e^(2 s / cap) overflows FP32.  Expected values: tests/softcap_model.py on the inputs after their rounding, on needle
queries scaled to several caps; every output element and every L of every live row is held to its bounds at softcap_model.MARGIN, for
D 64 / 128 / 256 x bf16 / f16 x G 1 / 8 x decode R 1 / 4 x 16-bit / e4m3 caches.  Results must be finite, inside the bounds, and
byte-identical between the contiguous, the token-major strided and the paged layout; a ragged capped prefill is byte-identical to the
padded one.  Maxima seen on an MI355X: DESIGN.md 4.16."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402
import decode_model as dm  # noqa: E402
import sink_model as sm  # noqa: E402
import softcap_model as cm  # noqa: E402
from cache_kit import LOG2E, dev, poisoned, same, token_major  # noqa: E402

BATCH = ck.SINK_BATCH
SEQS, LENS, QLENS, B, RP, HKV = list(BATCH.SEQS), BATCH.LENS, BATCH.QLENS, BATCH.B, BATCH.RP, BATCH.HKV
SETTINGS = [(30.0, 0, 0, False), (50.0, 130, 4, True), (1.0, 130, 70, True)]      # (cap, W (0: none), S, sink logits)
# (D, dtype, G, decode R, e4m3 cache): every value of every dimension with both caches
VARIANTS = [(64, torch.bfloat16, 1, 1, False), (128, torch.float16, 8, 4, False), (256, torch.bfloat16, 8, 1, True),
            (256, torch.float16, 1, 4, False), (64, torch.float16, 8, 4, True), (128, torch.bfloat16, 1, 1, True)]
base = functools.partial(ck.base, BATCH)
SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield
    if SEEN:
        print("\nsoftcap worst err / bound at margin 1:", {k: round(v, 4) for k, v in SEEN.items()})


def qlens_of(kind):
    return None if kind == "decode" else QLENS


def sink_logits(Hq, cap, seed=0):
    """one logit per query head, natural units, of the order of the cap: beside needles at cap tanh(3) a share of the mass"""
    return (cap * np.random.default_rng(50 + seed).uniform(0.8, 1.1, Hq)).astype(np.float32)


def launch(kind, q, k, v, G, *, cap=None, W=0, S=0, logits=None, want_pieces=None, **how):
    """cap None: the sink entries (the uncapped sibling).  In pieces, the launch form must name the capped kernels"""
    named = dict(window=W, sinkTokens=S, sinkLogits=logits)
    if cap is not None:
        named.update(softcap=cap)
    form = r"attn_decode%sc_d%d_.*_pieces \(" % ("8" if k.dtype == torch.float8_e4m3fn else "16", q.shape[-1])
    return ck.launch(BATCH, kind, q, k, v, G, want_pieces=want_pieces, want_form=None if want_pieces is None else form, **named, **how)


@functools.lru_cache(maxsize=None)
def reference(kind, D, dtype, G, R, cap, W, S, with_logits, fp8, pieces=None):
    """(q, sink logits, model, needle info, the uncapped model), computed once per case and shared; the models read the values a cache
    stands for"""
    k, v, (ks, vs) = base(D, dtype, fp8)
    fmt, Hq = dm.fmt_of(dtype), HKV * G
    sink = sink_logits(Hq, cap, D + G) if with_logits else None
    seen = k.float().numpy().astype(np.float64) * (ks[None, :, None, None] if fp8 else 1.0)
    q64, info = cm.needle_queries(seen, LENS, qlens_of(kind), Hq, G, R, W, S, fmt, cap, pieces=pieces, page=16)
    q = torch.from_numpy(q64).to(dtype)
    assert torch.equal(q.to(torch.float64), torch.from_numpy(q64))
    ref = cm.model(q, k.float(), v.float(), LENS, qlens_of(kind), G, W, S, sink, cap, pieces=pieces, kscale=ks, vscale=vs)
    return q, sink, ref, info


def hold(kind, o, l, ref, dtype, out, info, tag, sink, W, S):
    """cache_kit.hold with the blind rows of the frontiers under (W, S), at this model's bounds"""
    ck.hold(BATCH, kind, o, l, ref, dtype, out, info, tag, cm, SEEN, ck.sink_blind(W, S), sink)


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("setting", range(len(SETTINGS)))
@pytest.mark.parametrize("kind", ["decode", "prefill"])
def test_parity_with_the_model_on_poisoned_caches(kind, setting, variant):
    (cap, W, S, with_logits), (D, dtype, G, Rd, fp8) = SETTINGS[setting], VARIANTS[variant]
    R = Rd if kind == "decode" else RP
    k, v, scales = base(D, dtype, fp8)
    sd = (dev(scales[0]), dev(scales[1]))
    tiles = ck.walked(BATCH, kind, G, R, W, S)
    keep = BATCH.keep(tiles=tiles)
    if W:
        assert tiles[0][0] and not tiles[0][2:8].any() and tiles[0][8:11].all()   # n = 700: the sink tiles, a poisoned gap, the window from tile 8
    q, sink, ref, info = reference(kind, D, dtype, G, R, cap, W, S, with_logits, fp8)
    tag = "%s %s cache cap %g" % (kind, "e4m3" if fp8 else "16-bit", cap)
    kd, vd = poisoned(k, keep), poisoned(v, keep)
    common = dict(cap=cap, W=W, S=S, logits=dev(sink), scales=sd)
    o, l = launch(kind, q, kd.cuda(), vd.cuda(), G, **common)
    hold(kind, o, l, ref, dtype, dtype, info, tag, sink, W, S)
    o32, l32 = launch(kind, q, kd.cuda(), vd.cuda(), G, out=torch.float32, **common)   # (unsplit: no workspace is offered)
    hold(kind, o32, l32, ref, dtype, torch.float32, info, tag, sink, W, S)
    (kt, strides), (vt, _) = token_major(kd), token_major(vd)
    assert same(launch(kind, q, kt.cuda(), vt.cuda(), G, cache_kw=dict(strides=dict(K=strides, V=strides)), **common), (o, l)), \
        "the token-major strided layout differs from the contiguous launch"
    kp, vp, kw = ck.paged_pool(k, v, 16, keep, seed=setting + 3 * variant)
    assert same(launch(kind, q, kp, vp, G, cache_kw=kw, **common), (o, l)), "paged 16 differs from the contiguous launch"


@pytest.mark.parametrize("case", [(256, torch.bfloat16, 8, 1, False, 0, 6), (128, torch.float16, 8, 4, True, 1, 3), (64, torch.bfloat16, 1, 4, False, 2, 3)])
def test_decode_in_pieces(case):
    """with a workspace: no window plans 6 pieces over the 24 tiles of the column, W = 640 with S = 4 plans 3 (as the sink launch does:
    the plan does not change with a cap).  n = 1500 fills every piece, n = 100 leaves pieces empty, n = 0 all of them"""
    D, dtype, G, R, fp8, setting, pieces = case
    cap, W, S, with_logits = SETTINGS[setting]
    W = 640 if W else 0
    k, v, scales = base(D, dtype, fp8)
    tiles = ck.walked(BATCH, "decode", G, R, W, S)
    keep = BATCH.keep(tiles=tiles)
    q, sink, ref, info = reference("decode", D, dtype, G, R, cap, W, S, with_logits, fp8, pieces)
    for out in (None, torch.float32):
        o, l = launch("decode", q, poisoned(k, keep).cuda(), poisoned(v, keep).cuda(), G, cap=cap, W=W, S=S, logits=dev(sink), out=out, workspace=True,
                      want_pieces=pieces, scales=(dev(scales[0]), dev(scales[1])))
        hold("decode", o, l, ref, dtype, out or dtype, info, "decode pieces%s cap %g" % (" e4m3" if fp8 else "", cap), sink, W, S)


@pytest.mark.parametrize("case", [(256, torch.bfloat16, 8, False, 1), (64, torch.float16, 1, True, 2), (128, torch.bfloat16, 8, True, 0)])
def test_ragged_prefill_is_the_padded_capped_launch_byte_for_byte(case):
    D, dtype, G, fp8, setting = case
    cap, W, S, with_logits = SETTINGS[setting]
    k, v, scales = base(D, dtype, fp8)
    sd = (dev(scales[0]), dev(scales[1]))
    tiles = ck.walked(BATCH, "prefill", G, RP, W, S)
    keep = BATCH.keep(tiles=tiles)
    q, sink, _ref, _info = reference("prefill", D, dtype, G, RP, cap, W, S, with_logits, fp8)
    kd, vd = poisoned(k, keep).cuda(), poisoned(v, keep).cuda()
    common = dict(cap=cap, W=W, S=S, logits=dev(sink), scales=sd)
    o, l = launch("prefill", q, kd, vd, G, **common)
    counts = [min(qn, RP) for qn in QLENS]
    starts = np.concatenate([[0], np.cumsum(counts)]).tolist()
    packed = torch.cat([q[b, :, :counts[b]].permute(1, 0, 2) for b in range(B)]).contiguous()
    ro, rl = launch("prefill", packed, kd, vd, G, ragged=(starts, starts[-1]), **common)
    for b in range(B):
        s, e = starts[b], starts[b + 1]
        assert torch.equal(ro[s:e].view(torch.int16), o[b, :, :e - s].permute(1, 0, 2).contiguous().view(torch.int16)), f"sequence {b}: O differs"
        assert torch.equal(rl[:, s:e], l[b, :, :e - s]), f"sequence {b}: L differs"


@pytest.mark.parametrize("kind", ["decode", "prefill"])
def test_the_capped_kernels_run(kind):
    """the capped launch differs from the uncapped launch of the same window and sinks by more than the bound on the needle rows (and
    the uncapped one is nowhere near the capped model): the cap is applied, by the new kernels"""
    D, dtype, G, fp8 = 256, torch.bfloat16, 8, False
    cap, W, S, with_logits = SETTINGS[1]
    R = 1 if kind == "decode" else RP
    k, v, _scales = base(D, dtype, fp8)
    tiles = ck.walked(BATCH, kind, G, R, W, S)
    keep = BATCH.keep(tiles=tiles)
    q, sink, ref, info = reference(kind, D, dtype, G, R, cap, W, S, with_logits, fp8)
    kd, vd = poisoned(k, keep).cuda(), poisoned(v, keep).cuda()
    o, l = launch(kind, q, kd, vd, G, cap=cap, W=W, S=S, logits=dev(sink), out=torch.float32)
    uo, ul = launch(kind, q, kd, vd, G, cap=None, W=W, S=S, logits=dev(sink), out=torch.float32)
    bo, bl = cm.bounds(ref, dm.fmt_of(dtype), "f32")
    rows = 0
    for (b, h, r) in info:   # (a row that sees a handful of keys may give all its mass to one key either way: rows with 32 keys and more)
        n, qn = LENS[b], R if kind == "decode" else min(QLENS[b], R)
        lo, lim = sm.frontiers(n, qn, np.array([r]), W)
        if sm.visible_keys(int(lo[0]), int(lim[0]), S).size < 32:
            continue
        far = (np.abs(o[b, h, r].double().numpy() - uo[b, h, r].double().numpy()) > 2 * bo[b, h, r]).any()
        far_l = abs(float(l[b, h, r]) - float(ul[b, h, r])) / LOG2E > 2 * bl[b, h, r]
        assert far and far_l, (b, h, r)
        rows += 1
    assert rows >= 3 * HKV * G * (1 if kind == "decode" else 40)
    wo, wl, _text = cm.compare(uo, ul / LOG2E, ref, dm.fmt_of(dtype), "f32", LENS, qlens_of(kind), margin=cm.MARGIN)
    assert wo > 1.0 and wl > 1.0
