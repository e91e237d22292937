"""CPU test of the oracle of tests/test_mla_gpu.py (tests/mla_model.py): on that file's cases, a correct kernel -- emulated(), the model
with the kernel's roundings and order of sums -- lies inside bounds(), and every named mutant, what a defect of the kernels or of the
host plan would compute, lies outside on at least one case where its defect can show.  MARGIN is fixed HERE, before any GPU run: the
smallest power of two with at least 2 x headroom over emulated()'s worst err / bound at margin 1.  No wrong kernel is ever run; the
piece ranges and the piece counts are the built library's own (mfa_attention_decode_piece_range, mfa_attention_mla_decode_workspace_size)."""
import numpy as np
import pytest

import mla_model as mm


def _ratio(o, l, ref, fmt, out):
    """worst |dO| / bound and |dL| / bound at margin 1 of a result before the store's rounding"""
    bo, bl = mm.bounds(ref, fmt, out, margin=1)
    wo = float((np.abs(mm.store(o, out) - ref.O) / bo).max())
    keep = np.isfinite(ref.L)
    got = np.where(np.isfinite(l), l, 0.0)
    wl = float((np.abs(got - np.where(keep, ref.L, 0.0)) / bl)[keep].max()) if keep.any() else 0.0
    if (np.isfinite(l) != keep).any():
        wl = np.inf
    return wo, wl


@pytest.fixture(scope="module")
def worst():
    """name -> (worst O ratio, worst L ratio) of emulated() on every case, once"""
    out = {}
    for name in mm.CASES:
        case, pieces, q, kv, ref, _info = mm.inputs(name)
        o, l = mm.emulated(q, kv, mm.LENS, case["causal"], mm.SCALE, case["fmt"], pieces=pieces, shared=case["layout"] == "shared")
        out[name] = _ratio(o, l, ref, case["fmt"], case["out"])
        print("%s: emulated worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % ((name,) + out[name]))
    return out


def test_the_emulated_kernel_lies_inside_the_bounds(worst):
    for name, (wo, wl) in worst.items():
        assert wo <= mm.MARGIN and wl <= mm.MARGIN, (name, wo, wl)


def test_the_margin_is_the_smallest_power_of_two_with_twice_the_headroom(worst):
    top = max(max(pair) for pair in worst.values())
    want = 1
    while want < 2 * top:
        want *= 2
    assert mm.MARGIN == want, (mm.MARGIN, want, top)


def test_the_cases_meet_what_they_are_for():
    groups = lambda c: -(-c["H"] * c["R"] // mm.ROWS)  # noqa: E731
    assert groups(mm.CASES["2 seam inside a head"]) == 2 and 11 * 3 == 33 and 32 // 3 == 10   # the seam falls inside head 10; one row is left
    assert groups(mm.CASES["3 two groups, rows 640 apart"]) == 2 and 40 % 32 != 0
    assert groups(mm.CASES["4 one row"]) == 1
    assert mm.planned_pieces(mm.CASES["1 planned"]) == 6                     # 512 // 6 sequences = 85, 24 tiles // 4 = 6
    assert mm.planned_pieces(mm.CASES["2 seam inside a head, planned"]) == 6  # 12 workgroups: 42, and 6 again
    assert 0 in mm.LENS and 5 in mm.LENS and max(mm.LENS) // mm.TILE >= 16 and any(n % mm.STEP for n in mm.LENS)
    assert any(0 < -(-n // mm.TILE) < 7 for n in mm.LENS)                    # sequences with fewer tiles than pieces


@pytest.mark.parametrize("mutant", sorted(mm.MUTANTS))
def test_every_mutant_lies_outside(mutant):
    """on at least one case where the defect can show the mutant's O or L leaves the bounds at MARGIN -- the first such case ends the
    walk; a mutant that shows nowhere fails"""
    _what, harmless = mm.MUTANTS[mutant]
    tried = []
    for name in mm.CASES:
        case, pieces, q, kv, ref, _info = mm.inputs(name)
        facts = dict(R=case["R"], H=case["H"], B=len(mm.LENS), causal=case["causal"], pieces=pieces, page=case["page"])
        if all(harmless(dict(facts, n=n)) for n in mm.LENS if n):
            continue
        bad = mm.model(q, kv, mm.LENS, case["causal"], mm.SCALE, mutant, pieces=pieces, page=case["page"], shared=case["layout"] == "shared")
        fmt, out = case["fmt"], case["out"]
        bo, bl = mm.bounds(ref, fmt, out)
        wo = float((np.abs(mm.store(bad.O, out) - ref.O) / bo).max())          # (err / bound at MARGIN: outside is > 1)
        both = np.isfinite(ref.L) & np.isfinite(bad.L)
        wl = float((np.abs(np.where(both, bad.L - np.where(both, ref.L, 0.0), 0.0)) / bl).max())
        if (np.isfinite(ref.L) != np.isfinite(bad.L)).any():
            wl = np.inf
        tried.append((name, wo, wl))
        if max(wo, wl) > 1.0:
            return
    assert tried, "no case lets %s show" % mutant
    pytest.fail("%s stays inside the bounds on every case where it can show: %r" % (mutant, tried))
