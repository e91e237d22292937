"""CPU test (numpy only, no GPU): what the bounds of tests/sink_model.py can see.  On every case the rounding-emulated attention -- the
kernels' roundings and order of sums: sink tiles first, then the window's; piece 0 folds the sink logit -- lies INSIDE the per-element
bounds, and every named mutant -- a wrong attention computed on the CPU; no wrong kernel is ever run -- lies OUTSIDE them wherever the
defect changes what is summed (sink_model.mutated decides that from the geometry and the launch's options alone).  Every mutant bites
in at least one case.

The cases: a gap between the sink tile and the window (n = 700, W = 130, S = 4), zones that touch (n = 200, W = 130, S = 70), S > n,
two sink tiles with the second partial (S = 70 over a gap), decode unsplit and in 3 and 4 pieces (W = 260 over n = 700: a piece that
straddles the gap; n = 64: empty pieces), prefill over row blocks with an odd and an even sinkEnd and sequences with n < qn (rows that see their sinks alone, rows
that see nothing), with and without logits, with per-head scales, bf16 and f16, 16-bit and FP32 stores."""
import numpy as np
import pytest

import decode_model as dm
import sink_model as sm

D, HKV = 64, 2
# (G, R, fmt, scales, out, pieces, page, W, S, logits, lens)
DECODE = [
    (1, 1, "bf16", False, "bf16", None, None, 130, 4, True, [700, 200, 5, 64, 0]),
    (4, 4, "f16", True, "f32", 3, 16, 260, 4, True, [700, 1500, 300, 64]),
    (3, 4, "bf16", False, "bf16", 4, 256, 130, 70, False, [700, 200, 1500, 2]),
    (4, 1, "f16", True, "f16", None, 16, 130, 70, True, [700, 200, 50]),
    (1, 4, "bf16", False, "f32", 3, None, 0, 0, True, [700, 300, 2]),
    (8, 1, "bf16", True, "bf16", 3, None, 64, 1000, True, [700, 1500, 64]),
]
# (G, fmt, scales, out, page, W, S, logits, [(n, qn)], capacity)
PREFILL = [
    (1, "bf16", False, "bf16", None, 130, 4, True, [(700, 129), (200, 40), (100, 200), (5, 5)], 200),
    (4, "f16", True, "f32", 16, 130, 70, True, [(700, 40), (1500, 129), (100, 200), (300, 200)], 200),
    (8, "bf16", False, "bf16", 256, 130, 130, False, [(700, 129), (1500, 200), (64, 1)], 200),
    (4, "bf16", True, "f32", None, 16, 4, True, [(700, 129), (100, 200), (0, 3)], 200),
    (1, "f16", False, "f16", 16, 0, 0, True, [(300, 129), (100, 200), (64, 1)], 129),
    (3, "bf16", False, "bf16", None, 65, 1000, True, [(700, 129), (1500, 40), (100, 200)], 200),
]
CASES = [("decode", c) for c in DECODE] + [("prefill", c) for c in PREFILL]
_BUILT = {}


def build(index):
    """the case's inputs and its model, computed once and shared (never modified)"""
    if index in _BUILT:
        return _BUILT[index]
    kind, c = CASES[index]
    rng = np.random.default_rng(200 + index)
    if kind == "decode":
        G, R, fmt, scales, out, pieces, page, W, S, logits, lens = c
        qlens = None
    else:
        G, fmt, scales, out, page, W, S, logits, pairs, R = c
        lens, qlens, pieces = [n for n, _ in pairs], [qn for _, qn in pairs], None
    B, Hq, C = len(lens), HKV * G, max(lens)
    k = dm.round_to(rng.uniform(-1, 1, (B, HKV, C, D)), fmt)
    v = dm.round_to(rng.uniform(-1, 1, (B, HKV, C, D)), fmt)
    ks = dm.spread_scales(rng, HKV).astype(np.float64) if scales else None
    vs = dm.spread_scales(rng, HKV).astype(np.float64) if scales else None
    seen = k * ks[None, :, None, None] if scales else k
    sink = rng.uniform(1.0, 4.0, Hq).astype(np.float32).astype(np.float64) if logits else None   # (a share of the mass next to the needles')
    q, info = sm.needle_queries(seen, lens, qlens, Hq, G, R, W, S, fmt, pieces=pieces, page=page, seed=index)
    kw = dict(pieces=pieces, kscale=ks, vscale=vs)
    ref = sm.model(q, k, v, lens, qlens, G, W, S, sink, **kw)
    _BUILT[index] = dict(kind=kind, G=G, R=R, fmt=fmt, out=out, pieces=pieces, page=page, W=W, S=S, sink=sink, lens=lens, qlens=qlens, q=q, k=k,
                         v=v, kw=kw, ref=ref, info=info)
    return _BUILT[index]


def ratios(case, O, L, margin):
    return sm.compare(O, L, case["ref"], case["fmt"], case["out"], case["lens"], case["qlens"], margin=margin, info=case["info"])


def args(case):
    return case["q"], case["k"], case["v"], case["lens"], case["qlens"], case["G"], case["W"], case["S"], case["sink"]


def test_the_cases_reach_the_seams():
    from metal_flash_attention_amd import AttentionDecode, AttentionPrefill
    pairs = [AttentionDecode.sinkPieceRange(700, 4, 260, 4, 3, p) for p in range(3)]
    assert any(p0[1] > p0[0] and p1[1] > p1[0] for p0, p1 in pairs)                                   # a piece straddles the gap
    assert any(p0[0] == p0[1] and p1[0] == p1[1] for p0, p1 in [AttentionDecode.sinkPieceRange(64, 4, 260, 4, 3, p) for p in range(3)])   # an empty piece
    assert AttentionPrefill.sinkTileRange(700, 129, 0, 128, 130, 4)[4] == 1 and AttentionPrefill.sinkTileRange(700, 40, 0, 32, 130, 70)[4] == 2   # odd and even sinkEnd
    assert AttentionPrefill.sinkTileRange(200, 40, 0, 128, 130, 70)[4] <= 1 <= -(-70 // 64)              # the zones touch: S reaches `begin`


@pytest.mark.parametrize("index", range(len(CASES)))
def test_emulated_kernel_lies_inside_the_bounds(index):
    case = build(index)
    O, L = sm.emulated(*args(case), case["fmt"], **case["kw"])
    wo, wl, text = ratios(case, dm.store(O, case["out"]), L, 1)
    print("case %d (%s): worst err / bound at margin 1: O %.3f, L %.3f" % (index, case["kind"], wo, wl))
    assert wo * 2 <= sm.MARGIN and wl * 2 <= sm.MARGIN, text     # 2 x headroom under the committed margin
    # rows without a visible key: O = 0 and L = the sink logit exactly, or -inf without one (the model's, and the emulation's)
    blind = np.zeros(case["ref"].L.shape, dtype=bool)
    for b, n in enumerate(case["lens"]):
        qn = case["R"] if case["qlens"] is None else min(case["qlens"][b], case["R"])
        lo, lim = sm.frontiers(n, qn, np.arange(qn), case["W"])
        blind[b, :, :qn] = np.array([sm.visible_keys(int(a), int(e), case["S"]).size == 0 for a, e in zip(lo, lim)])[None, :]
    assert not O[blind].any()
    if case["sink"] is None:
        assert np.isinf(L[blind]).all() and np.isinf(case["ref"].L[blind]).all()
    else:
        want = np.broadcast_to(case["sink"][None, :, None], L.shape)[blind]
        assert np.allclose(L[blind], want, rtol=1e-12) and np.array_equal(case["ref"].L[blind], want)


@pytest.mark.parametrize("index", range(len(CASES)))
def test_every_mutant_lies_outside_the_bounds_where_it_changes_anything(index):
    case = build(index)
    O, L, _ = sm.mutated(*args(case), None, page=case["page"], **case["kw"])
    wo, wl, text = ratios(case, O, L, sm.MARGIN)
    assert wo <= 1e-3 and wl <= 1e-3, text     # (the mutated() arithmetic without a defect is inside the bounds)
    for name in sm.MUTANTS:
        O, L, changed = sm.mutated(*args(case), name, page=case["page"], **case["kw"])
        wo, wl, text = ratios(case, O, np.where(np.isfinite(L), L, -1e30), sm.MARGIN)
        if changed:
            assert (wl if name in sm.L_ONLY else wo) > 1.0, (name, wo, wl, text)
        else:
            assert wo <= 1e-3 and wl <= 1e-3, (name, text)


def test_no_mutant_is_vacuous():
    bites = {name: [] for name in sm.MUTANTS}
    for index in range(len(CASES)):
        case = build(index)
        for name in sm.MUTANTS:
            if sm.mutated(*args(case), name, page=case["page"], **case["kw"])[2]:
                bites[name].append(index)
    assert all(bites.values()), {n: b for n, b in bites.items() if not b}
    kinds = {name: {CASES[i][0] for i in b} for name, b in bites.items()}
    for name in ("sinks_one_long", "sinks_one_short", "sinks_past_frontier", "sink_tile_dropped", "gap_walked_unmasked", "low_zone_without_sinks",
                 "logit_scaled_by_rsqrt_d", "logit_scaled_by_key_scale", "l_without_sink", "blind_row_left"):
        assert kinds[name] == {"decode", "prefill"}, (name, kinds[name])   # a defect either kernel can have bites in both
