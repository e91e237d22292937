"""CPU test (numpy only, no GPU): what the bounds of tests/window_model.py can see.  On every case the rounding-emulated attention --
the kernels' roundings and order of sums over the window's ranges -- lies INSIDE the per-element bounds, and every named mutant -- a
wrong attention computed on the CPU; no wrong kernel is ever run -- lies OUTSIDE them wherever the defect changes which keys a workgroup
adds up (window_model.mutated decides that from the geometry).  Every mutant bites in at least one case.

The cases cover, for decode, G 1 / 4 / 3, R 1 / 4, bf16 and f16 with per-head scales, 16-bit and FP32 stores, unsplit and 3 pieces, no
pages / 16 / 256, W 1 / 64 / 100 and n 5 / 64 / 300 / 1500 (plus n = 130 and n = 2: a window that starts within three keys of a tile
boundary, and n < R); for prefill the same and row counts that span row blocks (qn 40 / 129 / 200), W 16 / 65 / 200 (blocks without
an unmasked tile, and blocks whose low and high masked zones overlap), and sequences with n < qn."""
import numpy as np
import pytest

import decode_model as dm
import window_model as wm

D, HKV = 64, 2
LENS = [5, 64, 300, 1500]
# (G, R, fmt, scales, out, pieces, page, W, lens)
DECODE = [
    (1, 1, "bf16", False, "bf16", None, None, 1, LENS),
    (4, 4, "f16", True, "f32", 3, 16, 64, LENS + [130]),
    (3, 4, "bf16", False, "bf16", 3, 256, 100, LENS),
    (4, 1, "f16", True, "f16", None, 16, 100, LENS),
    (1, 4, "bf16", False, "f32", None, None, 64, LENS + [130, 2]),
    (3, 1, "bf16", False, "bf16", 3, None, 1, LENS),
]
# (G, fmt, scales, out, page, W, [(n, qn)], capacity)
PREFILL = [
    (1, "bf16", False, "bf16", None, 16, [(5, 5), (64, 1), (300, 129), (1500, 40), (100, 200)], 200),
    (4, "f16", True, "f32", 16, 65, [(65, 4), (300, 129), (1500, 40), (100, 200), (300, 200)], 200),
    (3, "bf16", False, "bf16", 256, 200, [(300, 129), (1500, 200), (100, 200), (64, 1)], 200),
    (4, "bf16", False, "f32", None, 1, [(5, 5), (300, 129), (1500, 40), (100, 200)], 200),
    (1, "f16", True, "f16", 16, 64, [(64, 1), (300, 129), (1500, 40), (100, 200)], 129),
    (3, "bf16", False, "bf16", None, 100, [(65, 4), (300, 129), (1500, 40), (100, 200)], 200),
]
CASES = [("decode", c) for c in DECODE] + [("prefill", c) for c in PREFILL]
_BUILT = {}


def build(index):
    """the case's inputs and its model, computed once and shared (never modified)"""
    if index in _BUILT:
        return _BUILT[index]
    kind, c = CASES[index]
    rng = np.random.default_rng(100 + index)
    if kind == "decode":
        G, R, fmt, scales, out, pieces, page, W, lens = c
        qlens = None
    else:
        G, fmt, scales, out, page, W, pairs, R = c
        lens, qlens, pieces = [n for n, _ in pairs], [qn for _, qn in pairs], None
    B, Hq, C = len(lens), HKV * G, max(lens)
    k = dm.round_to(rng.uniform(-1, 1, (B, HKV, C, D)), fmt)
    v = dm.round_to(rng.uniform(-1, 1, (B, HKV, C, D)), fmt)
    ks = dm.spread_scales(rng, HKV).astype(np.float64) if scales else None
    vs = dm.spread_scales(rng, HKV).astype(np.float64) if scales else None
    seen = k * ks[None, :, None, None] if scales else k
    q, info = wm.needle_queries(seen, lens, qlens, Hq, G, R, W, fmt, pieces=pieces, page=page, seed=index)
    kw = dict(pieces=pieces, kscale=ks, vscale=vs)
    ref = wm.model(q, k, v, lens, qlens, G, W, **kw)
    _BUILT[index] = dict(kind=kind, G=G, R=R, fmt=fmt, out=out, pieces=pieces, page=page, W=W, lens=lens, qlens=qlens, q=q, k=k, v=v, kw=kw,
                         ref=ref, info=info)
    return _BUILT[index]


def ratios(case, O, L, margin):
    wo, wl, text = wm.compare(O, L, case["ref"], case["fmt"], case["out"], case["lens"], case["qlens"], margin=margin, info=case["info"])
    return wo, wl, text


@pytest.mark.parametrize("index", range(len(CASES)))
def test_emulated_kernel_lies_inside_the_bounds(index):
    case = build(index)
    O, L = wm.emulated(case["q"], case["k"], case["v"], case["lens"], case["qlens"], case["G"], case["W"], case["fmt"], **case["kw"])
    wo, wl, text = ratios(case, dm.store(O, case["out"]), L, 1)
    print("case %d (%s): worst err / bound at margin 1: O %.3f, L %.3f" % (index, case["kind"], wo, wl))
    assert wo * 2 <= wm.MARGIN and wl * 2 <= wm.MARGIN, text     # 2 x headroom under the committed margin
    # rows without a visible key: exactly O = 0, L = -inf (the model's, and the emulation's)
    dead = ~np.isfinite(case["ref"].L)
    assert not O[dead].any() and np.isinf(L[dead]).all()


@pytest.mark.parametrize("index", range(len(CASES)))
def test_every_mutant_lies_outside_the_bounds_where_it_changes_anything(index):
    case = build(index)
    # (the mutated() arithmetic without a defect is inside the bounds: what "outside" is held against)
    O, L, _ = wm.mutated(case["q"], case["k"], case["v"], case["lens"], case["qlens"], case["G"], case["W"], None, page=case["page"], **case["kw"])
    wo, wl, text = ratios(case, O, L, wm.MARGIN)
    assert wo <= 1e-3 and wl <= 1e-3, text
    for name in wm.MUTANTS:
        O, L, changed = wm.mutated(case["q"], case["k"], case["v"], case["lens"], case["qlens"], case["G"], case["W"], name, page=case["page"], **case["kw"])
        wo, wl, text = ratios(case, O, np.where(np.isfinite(L), L, -1e30), wm.MARGIN)
        if changed:
            assert wo > 1.0, (name, wo, wl, text)
        else:
            assert wo <= 1e-3 and wl <= 1e-3, (name, text)


def test_no_mutant_is_vacuous():
    bites = {name: [] for name in wm.MUTANTS}
    for index in range(len(CASES)):
        case = build(index)
        for name in wm.MUTANTS:
            if wm.mutated(case["q"], case["k"], case["v"], case["lens"], case["qlens"], case["G"], case["W"], name, page=case["page"], **case["kw"])[2]:
                bites[name].append(index)
    assert all(bites.values()), {n: b for n, b in bites.items() if not b}
    kinds = {name: {CASES[i][0] for i in b} for name, b in bites.items()}
    for name in ("lo_one_long", "lo_one_short", "lo_of_row_0", "first_tile_dropped", "begin_early_unmasked", "first_page_from_entry_0", "ge_for_gt"):
        assert kinds[name] == {"decode", "prefill"}, (name, kinds[name])   # a defect either kernel can have bites in both
