"""CPU test (numpy only, no GPU): what the bounds of tests/softcap_model.py can see.  On needle queries scaled so that the visible
scores reach several caps -- the cap must matter -- the rounding-emulated capped attention (the kernels' order of operations and their
FP32 tanh formula) lies INSIDE the per-element bounds at softcap_model.MARGIN with 2 x headroom, and every named mutant -- a wrong
capped attention computed on the CPU; no wrong kernel is ever run -- lies OUTSIDE them on at least one live element wherever the defect
computes anything else.  Every mutant bites in a decode and in a prefill case.

The cases: caps 30 (Grok-1), 50 (Gemma 2) and 1 (saturation: needle scores of 64 caps, e^(2x) overflows FP32); no window, a window
with sink tokens over a gap, zones that touch; with and without sink logits -- of the order of the cap, so that a needle's share of
the mass goes to the sink; decode unsplit and in pieces, prefill over row blocks with n < qn; with per-head scales; bf16 and f16."""
import numpy as np
import pytest

import decode_model as dm
import softcap_model as cm

D, HKV = 64, 2
# (G, R, fmt, scales, out, pieces, W, S, logits, cap, lens)
DECODE = [
    (1, 1, "bf16", False, "bf16", None, 0, 0, False, 30.0, [700, 200, 5, 0]),
    (4, 4, "f16", True, "f32", 3, 260, 4, True, 50.0, [700, 1500, 64]),
    (8, 1, "bf16", True, "bf16", None, 130, 70, True, 1.0, [700, 200, 50]),
]
# (G, fmt, scales, out, W, S, logits, cap, [(n, qn)], capacity)
PREFILL = [
    (1, "bf16", False, "bf16", 0, 0, False, 50.0, [(300, 129), (100, 200), (5, 5)], 200),
    (4, "f16", True, "f32", 130, 70, True, 30.0, [(700, 40), (100, 200), (0, 3)], 200),
    (8, "bf16", True, "f32", 130, 4, True, 1.0, [(700, 129), (200, 40)], 129),
]
CASES = [("decode", c) for c in DECODE] + [("prefill", c) for c in PREFILL]
_BUILT = {}


def build(index):
    """the case's inputs and its model, computed once and shared (never modified)"""
    if index in _BUILT:
        return _BUILT[index]
    kind, c = CASES[index]
    rng = np.random.default_rng(300 + index)
    if kind == "decode":
        G, R, fmt, scales, out, pieces, W, S, logits, cap, lens = c
        qlens = None
    else:
        G, fmt, scales, out, W, S, logits, cap, pairs, R = c
        lens, qlens, pieces = [n for n, _ in pairs], [qn for _, qn in pairs], None
    B, Hq, C = len(lens), HKV * G, max(lens)
    k = dm.round_to(rng.uniform(-1, 1, (B, HKV, C, D)), fmt)
    v = dm.round_to(rng.uniform(-1, 1, (B, HKV, C, D)), fmt)
    ks = dm.spread_scales(rng, HKV).astype(np.float64) if scales else None
    vs = dm.spread_scales(rng, HKV).astype(np.float64) if scales else None
    seen = k * ks[None, :, None, None] if scales else k
    # (of the order of the cap: beside needles that score cap tanh(3) the sink holds a share of the mass, and capping it would move it)
    sink = (cap * rng.uniform(0.8, 1.1, Hq)).astype(np.float32).astype(np.float64) if logits else None
    q, info = cm.needle_queries(seen, lens, qlens, Hq, G, R, W, S, fmt, cap, pieces=pieces, seed=index)
    kw = dict(pieces=pieces, kscale=ks, vscale=vs)
    ref = cm.model(q, k, v, lens, qlens, G, W, S, sink, cap, **kw)
    _BUILT[index] = dict(kind=kind, G=G, R=R, fmt=fmt, out=out, W=W, S=S, sink=sink, cap=cap, lens=lens, qlens=qlens, q=q, k=k, v=v, kw=kw,
                         ref=ref, info=info, seen=seen)
    return _BUILT[index]


def ratios(case, O, L, margin):
    return cm.compare(O, L, case["ref"], case["fmt"], case["out"], case["lens"], case["qlens"], margin=margin, info=case["info"])


def args(case):
    return case["q"], case["k"], case["v"], case["lens"], case["qlens"], case["G"], case["W"], case["S"], case["sink"], case["cap"]


@pytest.mark.parametrize("index", range(len(CASES)))
def test_the_needles_reach_several_caps(index):
    case = build(index)
    reach = []
    for (b, h, r), (weights, _forbidden) in case["info"].items():
        s = (case["seen"][b, h // case["G"], sorted(weights)] @ case["q"][b, h, r]) / np.sqrt(D)
        reach.append(float(s.max()) / case["cap"])
    reach = np.array(reach)   # (but for the few rows whose only needle weighs nothing: the 16-bit rounding of q moves a score by a percent)
    assert reach.size and (reach >= (60.0 if case["cap"] == 1.0 else 2.9)).mean() >= 0.8 and reach.max() <= (70.0 if case["cap"] == 1.0 else 3.1)


@pytest.mark.parametrize("index", range(len(CASES)))
def test_emulated_kernel_lies_inside_the_bounds(index):
    case = build(index)
    O, L = cm.emulated(*args(case), case["fmt"], **case["kw"])
    live = np.isfinite(case["ref"].L)
    assert np.isfinite(O).all() and np.isfinite(L[live]).all()
    wo, wl, text = ratios(case, dm.store(O, case["out"]), L, 1)
    print("case %d (%s, cap %g): worst err / bound at margin 1: O %.3f, L %.3f" % (index, case["kind"], case["cap"], wo, wl))
    assert wo * 2 <= cm.MARGIN and wl * 2 <= cm.MARGIN, text     # 2 x headroom under the committed margin


@pytest.mark.parametrize("index", range(len(CASES)))
def test_every_mutant_lies_outside_the_bounds_where_it_changes_anything(index):
    case = build(index)
    O, L, changed = cm.mutated(*args(case), None, **case["kw"])
    wo, wl, text = ratios(case, O, L, cm.MARGIN)
    assert not changed and wo <= 1e-3 and wl <= 1e-3, text     # (the mutated() arithmetic without a defect is inside the bounds)
    for name in cm.MUTANTS:
        O, L, changed = cm.mutated(*args(case), name, fmt=case["fmt"], **case["kw"])
        wo, wl, text = ratios(case, O, np.where(np.isfinite(L) | np.isnan(L), L, -1e30), cm.MARGIN)
        if changed:
            # (an element of O or of L -- in the saturated cases the capped sink logit moves a share of the mass too small for O's bound
            # and shows in L -- but for the defects that leave O as it is)
            assert (wl if name in cm.L_ONLY else max(wo, wl)) > 1.0, (name, wo, wl, text)
        elif name != "naive_tanh":   # (where nothing overflows the naive form is the same function: its roundings are not this test's)
            assert wo <= 1e-3 and wl <= 1e-3, (name, text)


def test_no_mutant_is_vacuous():
    bites = {name: set() for name in cm.MUTANTS}
    for index in range(len(CASES)):
        case = build(index)
        for name in cm.MUTANTS:
            if cm.mutated(*args(case), name, fmt=case["fmt"], **case["kw"])[2]:
                bites[name].add(CASES[index][0])
    assert all(kinds == {"decode", "prefill"} for kinds in bites.values()), bites


@pytest.mark.parametrize("index", [i for i, (_kind, c) in enumerate(CASES) if c[-2 if _kind == "decode" else -3] == 1.0])
def test_saturation_is_finite_and_the_naive_form_is_not(index):
    """cap = 1 with scores of 64 caps and more: e^(2x) overflows FP32.  model() and emulated() are finite and agree; the form
    (e^2x - 1) / (e^2x + 1) yields NaN there -- this test can see that defect"""
    case = build(index)
    assert case["cap"] == 1.0
    ref = case["ref"]
    live = np.isfinite(ref.L)
    assert live.any() and np.isfinite(ref.O).all()
    O, L = cm.emulated(*args(case), case["fmt"], **case["kw"])
    assert np.isfinite(O).all() and np.isfinite(L[live]).all()
    wo, wl, text = ratios(case, dm.store(O, case["out"]), L, cm.MARGIN)
    assert wo <= 1.0 and wl <= 1.0, text
    On, Ln, changed = cm.mutated(*args(case), "naive_tanh", fmt=case["fmt"], **case["kw"])
    assert changed and np.isnan(On).any() and np.isnan(Ln).any()
    wo, wl, _text = ratios(case, On, Ln, cm.MARGIN)
    assert wo == np.inf and wl == np.inf


def test_the_capped_score_formula_at_both_ends():
    """1 - 2 / (1 + e^2x) in FP32: +-c2 at +-inf, never NaN, and within C_T u c2 of cap tanh(s / cap) log2(e) everywhere between"""
    for cap in (1.0, 30.0, 50.0):
        s = np.concatenate([np.linspace(-200.0, 200.0, 4001), [1e4, -1e4, 1e30, -1e30, 0.0]]) * cap / 50.0
        raw = s * 8.0   # D = 64, keyScale 1
        got = cm.capped_fp32(raw, np.float32(1.44269504089) / np.float32(8.0), 1.0, cap)
        want = cap * np.tanh(s / cap) * dm.LOG2E
        assert np.isfinite(got).all()
        c2 = cap * dm.LOG2E
        assert np.abs(got[-5:-1]) == pytest.approx(c2, rel=1e-6) and got[-1] == 0.0
        # (+ 1: the two roundings of the uncapped score's scale, which the bound counts in e_i -- 2 u on x moves t by at most 0.9 u)
        assert (np.abs(got - want) <= (cm.C_T + 1) * dm.U32 * c2).all()
        assert np.isnan(cm.capped_fp32(raw[-5:-1], np.float32(1.44269504089) / np.float32(8.0), 1.0, cap, naive=True)[[0, 2]]).all()
