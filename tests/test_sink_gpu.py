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

import cache_kit as ck  # noqa: E402
import decode_model as dm  # noqa: E402
import sink_model as sm  # noqa: E402
from cache_kit import LOG2E, TILE, dev, poisoned  # noqa: E402
from metal_flash_attention_amd import AttentionDecode  # noqa: E402

BATCH = ck.SINK_BATCH
SEQS, C, HKV, RP = list(BATCH.SEQS), BATCH.C, BATCH.HKV, BATCH.RP
LENS, QLENS, B = BATCH.LENS, BATCH.QLENS, BATCH.B
SETTINGS = [(130, 4), (130, 70), (130, 2000)]                       # (W, S)
VARIANTS = ck.SINK_VARIANTS                                          # (D, dtype, G, decode R, e4m3 cache)
base = functools.partial(ck.base, BATCH)
walked, reference = functools.partial(ck.walked, BATCH), functools.partial(ck.sink_reference, BATCH)
SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield
    if SEEN:
        print("\nsink worst err / bound at margin 1:", {k: round(v, 4) for k, v in SEEN.items()})


def launch(kind, q, k, v, G, *, W=None, S=None, logits=None, entry="sink", **how):
    """entry "sink": the sink entries (W None: window 0); "window": the window entries; "plain": the entries without a window"""
    named = {}
    if entry != "plain" and W is not None:
        named.update(window=W)
    if entry == "sink":
        named.update(sinkTokens=S or 0, sinkLogits=logits)
    return ck.launch(BATCH, kind, q, k, v, G, **named, **how)


def qlens_of(kind):
    return None if kind == "decode" else QLENS


def hold(kind, o, l, ref, dtype, out, info, tag, sink, W, S, causal=True):
    """cache_kit.hold with the blind rows of the frontiers under (W, S): O = 0 and L = the sink logit (base 2), or -FLT_MAX without logits"""
    ck.hold(BATCH, kind, o, l, ref, dtype, out, info, tag, sm, SEEN, ck.sink_blind(W, S, causal), sink)


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("setting", range(len(SETTINGS)))
@pytest.mark.parametrize("kind", ["decode", "prefill"])
def test_parity_with_the_model_on_poisoned_caches(kind, setting, variant):
    (W, S), (D, dtype, G, Rd, fp8) = SETTINGS[setting], VARIANTS[variant]
    R = Rd if kind == "decode" else RP
    k, v, scales = base(D, dtype, fp8)
    sd = (dev(scales[0]), dev(scales[1]))
    tiles = walked(kind, G, R, W, S)
    keep = BATCH.keep(tiles=tiles)
    if (W, S) == (130, 4):
        assert tiles[0][0] and not tiles[0][1:8].any() and tiles[0][8:11].all()   # n = 700: sink tile 0, tiles 1-7 poisoned, the window from tile 8
    if (W, S) == (130, 70):
        assert tiles[0][:2].all() and not tiles[0][2:8].any() and tiles[1][:4].all()   # two sink tiles over a gap; n = 200: the zones touch
    q, sink, ref, info = reference(kind, D, dtype, G, R, W, S, fp8)
    tag = kind + (" e4m3 cache" if fp8 else " 16-bit cache")
    kd, vd = poisoned(k, keep).cuda(), poisoned(v, keep).cuda()
    o, l = launch(kind, q, kd, vd, G, W=W, S=S, logits=dev(sink), scales=sd)
    hold(kind, o, l, ref, dtype, dtype, info, tag, sink, W, S)
    o32, l32 = launch(kind, q, kd, vd, G, W=W, S=S, logits=dev(sink), scales=sd, out=torch.float32)   # (unsplit: no workspace is offered)
    hold(kind, o32, l32, ref, dtype, torch.float32, info, tag, sink, W, S)
    kp, vp, kw = ck.paged_pool(k, v, 16, keep, seed=setting + 3 * variant)
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
    tiles = walked("decode", G, R, W, S)
    keep = BATCH.keep(tiles=tiles)
    assert tiles[5][0] and not tiles[5][1:13].any()
    q, sink, ref, info = reference("decode", D, dtype, G, R, W, S, fp8, True, 3)
    for out in (None, torch.float32):
        o, l = launch("decode", q, poisoned(k, keep).cuda(), poisoned(v, keep).cuda(), G, W=W, S=S, logits=dev(sink), out=out, workspace=True,
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
    kd, vd = poisoned(k, BATCH.keep(tiles=zeros)).cuda(), poisoned(v, BATCH.keep(tiles=zeros)).cuda()
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
    keep = BATCH.keep(tiles=tiles)
    kd, vd = poisoned(k, keep).cuda(), poisoned(v, keep).cuda()
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
