"""CPU test (numpy only, no GPU call but the library's host range functions): what the bounds of tests/tree_model.py can see.  With the
chain mask the model IS sink_model.model; on needle queries the rounding-emulated tree attention (the kernels' order of operations over
the tiles a tree launch walks) lies INSIDE the per-element bounds at tree_model.MARGIN with 2 x headroom; and every named mutant -- a
wrong tree attention computed on the CPU; no wrong kernel is ever run -- lies OUTSIDE them on at least one live element, in a decode and
in a prefill case (the two defects only prefill can have: in a prefill case).

The cases: random trees, forests whose later roots clear bit 0, arbitrary bits (j > r, bits at or past `live`); per sequence and
shared; no window, a window with sink tokens over a gap, W = rows with zones that touch; with and without sink logits; n < qn, P = 0,
n = 0, a tree that straddles a tile, (P + 1) % 64 = 0; decode unsplit and in pieces with G R = 32; prefill over four row blocks."""
import numpy as np
import pytest

import decode_model as dm
import sink_model as sm
import tree_model as tm

D, HKV = 64, 2
# (G, R, fmt, scales, out, pieces, W, S, logits, tree, shared, lens)
DECODE = [
    (8, 4, "bf16", False, "bf16", None, 0, 0, False, "forest", False, [700, 195, 70, 5, 0, 3]),
    (8, 4, "f16", True, "f32", 3, 260, 4, True, "forest", False, [700, 1500, 195, 3]),
    (1, 32, "bf16", True, "bf16", None, 130, 4, True, "random", False, [700, 223, 20]),
    (8, 4, "bf16", False, "f32", None, 4, 70, True, "arbitrary", False, [700, 70, 3]),
    (2, 16, "f16", False, "f16", None, 0, 0, False, "random", True, [700, 70, 5]),
]
# (G, fmt, scales, out, W, S, logits, tree, shared, [(n, qn)], rows)
PREFILL = [
    (8, "bf16", False, "bf16", 0, 0, False, "arbitrary", False, [(700, 40), (191, 64), (70, 33), (5, 5), (0, 3), (40, 64)], 64),
    (8, "f16", True, "f32", 130, 4, True, "random", False, [(700, 40), (191, 64), (70, 33), (40, 64)], 64),
    (1, "bf16", True, "f32", 64, 70, True, "forest", False, [(700, 64), (191, 64), (70, 33), (5, 5)], 64),
    (4, "bf16", False, "bf16", 130, 4, False, "forest", True, [(700, 40), (191, 40)], 40),
]
CASES = [("decode", c) for c in DECODE] + [("prefill", c) for c in PREFILL]
MAKERS = {"random": tm.random_tree, "forest": lambda R, rng: tm.forest(R, rng, 0.5), "arbitrary": tm.arbitrary}
_BUILT = {}


def build(index):
    """the case's inputs and its model, computed once and shared (never modified)"""
    if index in _BUILT:
        return _BUILT[index]
    kind, c = CASES[index]
    rng = np.random.default_rng(500 + index)
    if kind == "decode":
        G, R, fmt, scales, out, pieces, W, S, logits, tree, shared, lens = c
        qlens = None
    else:
        G, fmt, scales, out, W, S, logits, tree, shared, pairs, R = c
        lens, qlens, pieces = [n for n, _ in pairs], [qn for _, qn in pairs], None
    B, Hq, C = len(lens), HKV * G, max(lens)
    k = dm.round_to(rng.uniform(-1, 1, (B, HKV, C, D)), fmt)
    v = dm.round_to(rng.uniform(-1, 1, (B, HKV, C, D)), fmt)
    ks = dm.spread_scales(rng, HKV).astype(np.float64) if scales else None
    vs = dm.spread_scales(rng, HKV).astype(np.float64) if scales else None
    seen = k * ks[None, :, None, None] if scales else k
    sink = rng.uniform(1.0, 4.0, Hq).astype(np.float32).astype(np.float64) if logits else None
    masks = MAKERS[tree](R, np.random.default_rng(index)) if shared else tm.per_sequence(MAKERS[tree], B, R, index)
    q, info = tm.needle_queries(seen, lens, qlens, Hq, G, R, W, S, masks, fmt, pieces=pieces, seed=index)
    kw = dict(kscale=ks, vscale=vs)
    ref = tm.model(q, k, v, lens, qlens, G, W, S, sink, masks, pieces=pieces, **kw)
    _BUILT[index] = dict(kind=kind, G=G, R=R, fmt=fmt, out=out, W=W, S=S, sink=sink, masks=masks, lens=lens, qlens=qlens, q=q, k=k, v=v, kw=kw,
                         pieces=pieces, ref=ref, info=info)
    return _BUILT[index]


def ratios(case, O, L, margin):
    return tm.compare(O, L, case["ref"], case["fmt"], case["out"], case["lens"], case["qlens"], margin=margin, info=case["info"])


def blind_rows(case):
    """bool [B, R]: the live rows without a visible key"""
    out = np.zeros((len(case["lens"]), case["R"]), dtype=bool)
    for b, n in enumerate(case["lens"]):
        qn = case["R"] if case["qlens"] is None else min(case["qlens"][b], case["R"])
        out[b, :qn] = tm.blind(case["masks"], case["lens"], case["qlens"], case["R"], case["W"], case["S"])(b, n, qn)
    return out


def args(case):
    return case["q"], case["k"], case["v"], case["lens"], case["qlens"], case["G"], case["W"], case["S"], case["sink"], case["masks"]


@pytest.mark.parametrize("index", range(len(CASES)))
def test_the_chain_mask_is_the_sink_model(index):
    """mask_r = 2^(r + 1) - 1 with W >= rows (or none): the visible keys of today's causal launch for every (n, qn, W, S), n < qn included.
    O, L and A are sink_model.model's to the bit; the error terms too where the sequence has one row block (decode; prefill with
    G = 1) -- with several, an earlier block walks more tiles under a tree and its chain term may only grow"""
    case = build(index)
    q, k, v, lens, qlens, G, W, S, sink, _masks = args(case)
    W = W if W == 0 or W >= case["R"] else case["R"]
    B = len(lens)
    for masks in (tm.chain(case["R"]), tm.chain(case["R"], B)):
        got = tm.model(q, k, v, lens, qlens, G, W, S, sink, masks, pieces=case["pieces"], **case["kw"])
        want = sm.model(q, k, v, lens, qlens, G, W, S, sink, pieces=case["pieces"], **case["kw"])
        assert np.array_equal(got.O, want.O) and np.array_equal(got.L, want.L) and np.array_equal(got.A, want.A)
        if case["kind"] == "decode" or G == 1:
            assert np.array_equal(got.E, want.E) and np.array_equal(got.EL, want.EL)
        else:
            assert (got.E >= want.E).all() and (got.EL >= want.EL).all()
    for b, n in enumerate(lens):   # the identity on paper: the sets themselves
        qn = case["R"] if qlens is None else min(qlens[b], case["R"])
        lo, lim = sm.frontiers(n, qn, np.arange(qn), W)
        for r in range(qn):
            assert np.array_equal(tm.visible_row(n, qn, (1 << (r + 1)) - 1, W, S), np.unique(sm.visible_keys(int(lo[r]), int(lim[r]), S)))


@pytest.mark.parametrize("index", range(len(CASES)))
def test_emulated_kernel_lies_inside_the_bounds(index):
    case = build(index)
    O, L = tm.emulated(*args(case), case["fmt"], pieces=case["pieces"], **case["kw"])
    live = np.isfinite(case["ref"].L)
    assert np.isfinite(O).all() and np.isfinite(L[live]).all()
    wo, wl, text = ratios(case, dm.store(O, case["out"]), L, 1)
    print("case %d (%s): worst err / bound at margin 1: O %.3f, L %.3f" % (index, case["kind"], wo, wl))
    assert wo * 2 <= tm.MARGIN and wl * 2 <= tm.MARGIN, text     # 2 x headroom under the committed margin


@pytest.mark.parametrize("index", range(len(CASES)))
def test_every_mutant_lies_outside_the_bounds_where_it_changes_anything(index):
    case = build(index)
    O, L, changed = tm.mutated(*args(case), None, **case["kw"])
    wo, wl, text = ratios(case, O, L, tm.MARGIN)
    assert not changed and wo <= 1e-3 and wl <= 1e-3, text     # (the mutated() arithmetic without a defect is inside the bounds)
    for name in tm.MUTANTS:
        O, L, changed = tm.mutated(*args(case), name, **case["kw"])
        wo, wl, text = ratios(case, O, np.where(np.isfinite(L), L, -1e30), tm.MARGIN)
        # (a row without a visible key has no bound: it must hold O = 0 and L = -FLT_MAX or its sink logit exactly, which the GPU test
        # asserts; a defect that shows it a key gives it another L)
        woke = bool((blind_rows(case)[:, None, :] & (L != case["ref"].L)).any())
        if changed:
            assert max(wo, wl) > 1.0 or woke, (name, wo, wl, text)
        else:
            assert wo <= 1e-3 and wl <= 1e-3, (name, text)


def test_no_mutant_is_vacuous():
    """every defect changes what some row sees in a decode and in a prefill case (the prefill-only ones: in a prefill case), and by the
    test above it then lies outside the bounds there"""
    bites = {name: set() for name in tm.MUTANTS}
    for index in range(len(CASES)):
        case = build(index)
        for name in tm.MUTANTS:
            if tm.mutated(*args(case), name, **case["kw"])[2]:
                bites[name].add(CASES[index][0])
    for name, kinds in bites.items():
        assert kinds == ({"prefill"} if name in tm.PREFILL_ONLY else {"decode", "prefill"}), bites


def test_the_tile_range_written_out_is_the_library_s():
    for n in (0, 1, 63, 64, 65, 127, 128, 191, 700):
        for qn in (1, 5, 33, 64):
            for W, S in ((0, 0), (64, 0), (64, 4), (130, 70)):
                assert tm.library_tree_tile_range(n, qn, W, S) == tm.python_tree_tile_range(n, qn, W, S), (n, qn, W, S)
