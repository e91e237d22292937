"""CPU test (numpy only, no GPU): what the bounds of tests/split_model.py can see at the seams a key split adds to prefill.  On every
case the rounding-emulated split attention -- pieces in list order, merged by exp2(m_s - m*), the sink logit and the value scale after
the merge -- lies INSIDE the per-element bounds with 2 x headroom under the committed margin, and every named mutant -- a wrong split
attention computed on the CPU; no wrong kernel is ever run -- lies OUTSIDE them on every case in which the defect changes anything
(split_model.mutated decides that from the geometry and the launch's options alone).  Every mutant bites in at least one case.

The cases: three row blocks of 32 over (n, qn) = (1100, 70), pure causal prefill (70, 70) and a short queryLengths, in 3 pieces; a
window of 130 keys with 4 sink tokens in 2 pieces, where the list is one sink tile plus a short window run and piece 0 crosses the zone
seam; one row block of 128 in 2 pieces; 8 pieces over sequences with fewer tiles (empty pieces) and per-head scales; speculation trees
of 40 nodes at G = 8 in 3 and, under a window with sink tokens, 2 pieces; 64 pieces (piece 0 empty for every row block) with sink
logits; bf16 and f16, 16-bit and FP32 stores."""
import numpy as np
import pytest

import decode_model as dm
import split_model as spm
import tree_model as tm

D, HKV = 64, 2
# (G, fmt, scales, out, W, S, logits, [(n, qn)], capacity, pieces, tree)
CASES = [
    (4, "bf16", False, "bf16", 0, 0, True, [(1100, 70), (70, 70), (333, 37)], 70, 3, False),
    (4, "f16", True, "f32", 130, 4, True, [(1100, 70), (200, 40), (100, 200)], 70, 2, False),
    (1, "bf16", False, "bf16", 0, 0, False, [(700, 200), (300, 129)], 200, 2, False),
    (8, "bf16", True, "f32", 0, 0, True, [(900, 40), (70, 40), (5, 5)], 40, 8, False),
    (8, "f16", False, "f16", 0, 0, True, [(900, 40), (300, 33), (64, 40)], 40, 3, True),
    (4, "bf16", True, "bf16", 0, 0, True, [(1100, 70), (0, 3), (200, 70)], 70, 64, False),
    (8, "bf16", False, "bf16", 130, 70, False, [(900, 40), (400, 17)], 40, 2, True),
]
_BUILT = {}


def build(index):
    """the case's inputs and its model, computed once and shared (never modified)"""
    if index in _BUILT:
        return _BUILT[index]
    G, fmt, scales, out, W, S, logits, pairs, R, pieces, tree = CASES[index]
    rng = np.random.default_rng(900 + index)
    lens, qlens = [n for n, _ in pairs], [qn for _, qn in pairs]
    B, Hq, C = len(lens), HKV * G, max(lens)
    k = dm.round_to(rng.uniform(-1, 1, (B, HKV, C, D)), fmt)
    v = dm.round_to(rng.uniform(-1, 1, (B, HKV, C, D)), fmt)
    ks = dm.spread_scales(rng, HKV).astype(np.float64) if scales else None
    vs = dm.spread_scales(rng, HKV).astype(np.float64) if scales else None
    seen = k * ks[None, :, None, None] if scales else k
    sink = rng.uniform(1.0, 4.0, Hq).astype(np.float32).astype(np.float64) if logits else None
    masks = tm.per_sequence(tm.random_tree, B, R, 50 + index) if tree else None
    q, info = spm.needle_queries(seen, lens, qlens, Hq, G, R, W, S, fmt, pieces, masks=masks, seed=index)
    kw = dict(masks=masks, kscale=ks, vscale=vs)
    ref = spm.model(q, k, v, lens, qlens, G, W, S, sink, pieces, **kw)
    _BUILT[index] = dict(G=G, R=R, fmt=fmt, out=out, pieces=pieces, W=W, S=S, sink=sink, lens=lens, qlens=qlens, q=q, k=k, v=v, kw=kw, ref=ref,
                         info=info, tree=tree)
    return _BUILT[index]


def ratios(case, O, L, margin):
    return spm.compare(O, L, case["ref"], case["fmt"], case["out"], case["lens"], case["qlens"], margin=margin, info=case["info"])


def args(case):
    return case["q"], case["k"], case["v"], case["lens"], case["qlens"], case["G"], case["W"], case["S"], case["sink"], case["pieces"]


def test_the_python_rule_is_the_library_rule():
    for begin, end, sink_end in ((0, 18, 0), (15, 18, 1), (4, 4, 2), (0, 0, 0), (7, 30, 7)):
        for pieces in (1, 2, 3, 8, 64):
            for piece in range(pieces):
                assert spm.python_piece_range(begin, end, sink_end, pieces, piece) == spm.library_piece_range(begin, end, sink_end, pieces, piece)


def test_the_cases_reach_the_seams():
    se, bt, et = spm.block_range(1100, 70, 64, 4, True, 130, 4, False)
    lists = spm.piece_tiles(se, bt, et, 2)
    assert se == 1 and any(t[0] < se <= bt <= t[-1] for t in lists if t)                     # a piece crosses the zone seam
    assert any(not t for t in spm.piece_tiles(*spm.block_range(70, 40, 0, 8, True, 0, 0, False), 8))    # empty pieces
    assert not spm.piece_tiles(*spm.block_range(1100, 70, 64, 4, True, 0, 0, False), 64)[0]             # piece 0 empty
    ends = {spm.block_range(1100, 70, r0, 4, True, 0, 0, False)[2] for r0 in (0, 32, 64)}
    assert len({tuple(map(tuple, spm.piece_tiles(0, 0, e, 3))) for e in ends}) == len(ends)   # every row block has its own list


def test_the_needles_sit_either_side_of_every_piece_boundary():
    case = build(0)
    carried = {(b, t) for (b, _h, _r), (weights, _f) in case["info"].items() for t in weights}
    for b, (n, qn) in enumerate(zip(case["lens"], case["qlens"])):
        want = spm.boundary_keys(n, min(qn, case["R"]), case["G"], True, case["W"], case["S"], case["pieces"], False)
        assert want and all((b, t) in carried for t in want), (b, [t for t in want if (b, t) not in carried])


@pytest.mark.parametrize("index", range(len(CASES)))
def test_emulated_kernel_lies_inside_the_bounds(index):
    case = build(index)
    O, L = spm.emulated(*args(case), case["fmt"], **case["kw"])
    wo, wl, text = ratios(case, dm.store(O, case["out"]), L, 1)
    print("case %d: worst err / bound at margin 1: O %.3f, L %.3f" % (index, wo, wl))
    assert wo * 2 <= spm.MARGIN and wl * 2 <= spm.MARGIN, text     # 2 x headroom under the committed margin


@pytest.mark.parametrize("index", range(len(CASES)))
def test_every_mutant_lies_outside_the_bounds_where_it_changes_anything(index):
    case = build(index)
    O, L, _ = spm.mutated(*args(case), None, **case["kw"])
    wo, wl, text = ratios(case, O, L, spm.MARGIN)
    assert wo <= 1e-3 and wl <= 1e-3, text     # (the mutated() arithmetic without a defect is inside the bounds)
    assert spm.dead_rows_untouched(O, L, case["qlens"])
    for name in spm.MUTANTS:
        O, L, changed = spm.mutated(*args(case), name, **case["kw"])
        wo, wl, text = ratios(case, np.where(np.isfinite(O), O, 1e30), np.where(np.isfinite(L), L, -1e30), spm.MARGIN)
        if name in spm.DEAD_ONLY:
            assert spm.dead_rows_untouched(O, L, case["qlens"]) == (not changed), name
            assert wo <= 1e-3 and wl <= 1e-3, (name, text)
        elif changed:
            assert wo > 1.0, (name, wo, wl, text)
        else:
            assert wo <= 1e-3 and wl <= 1e-3, (name, text)


def test_no_mutant_is_vacuous():
    bites = {name: [] for name in spm.MUTANTS}
    for index in range(len(CASES)):
        case = build(index)
        for name in spm.MUTANTS:
            if spm.mutated(*args(case), name, **case["kw"])[2]:
                bites[name].append(index)
    assert all(bites.values()), {n: b for n, b in bites.items() if not b}
