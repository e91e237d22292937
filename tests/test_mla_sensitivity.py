"""CPU test of the oracle of tests/test_mla_gpu.py (tests/mla_model.py): on that file's cases -- CASES on the batch LENS and SEAM_CASES
on the batch SEAM_LENS, whose lengths lie on the step, page, tile and column seams -- a correct kernel -- emulated(), the model
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
    for name in mm.ALL_CASES:
        case, pieces, q, kv, ref, _info = mm.inputs(name)
        o, l = mm.emulated(q, kv, case["lens"], case["causal"], mm.SCALE, case["fmt"], pieces=pieces, shared=case["layout"] == "shared")
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
    assert all(c["lens"] == mm.LENS and c["C"] == mm.C for c in mm.CASES.values())
    the_seam_cases_meet_what_they_are_for()


def the_seam_cases_meet_what_they_are_for():
    """(the second half of test_the_cases_meet_what_they_are_for)"""
    lens, C, cases = mm.SEAM_LENS, mm.SEAM_C, mm.SEAM_CASES
    assert all(c["lens"] == lens and c["C"] == C for c in cases.values()) and not set(cases) & set(mm.CASES)
    seen = mm.seen_lens(next(iter(cases.values())))
    assert any(n and n % mm.STEP == 0 for n in lens) and any(n % mm.STEP for n in lens)          # a full last step, and a partial one
    pages = sorted({c["page"] for c in cases.values() if c["page"]})
    assert pages == [16, 32, 64, 512]
    for page in (16, 32, 64):                                                 # a full last page of one and of several pages, a partial one
        assert page in seen and any(n > page and n % page == 0 for n in seen) and any(n > page and n % page for n in seen), page
    assert 512 > C                                                            # one page holds the column: blockTableStride 1
    assert C in lens and max(lens) > C and seen[lens.index(max(lens))] == C   # n == C, and n > C read as C
    assert lens[lens.index(max(lens)) + 1] == 0 and lens[-1] == 0             # the empty sequence's rows follow the one past the column
    assert {mm.STEP, 2 * mm.STEP, 3 * mm.STEP} <= set(lens)                   # exactly one, two and three steps
    assert {mm.TILE, 4 * mm.TILE, C} <= set(lens) and C == 5 * mm.TILE        # whole piece tiles: one, four, five
    eight = cases["s2 eight rows"]
    assert eight["R"] == 8 and eight["causal"] and 8 in lens and any(0 < n < 8 for n in lens)   # n == R and n < R
    assert sorted(c["pieces"] for c in cases.values() if c["pieces"] and not c["page"]) == [2, 5, 64]
    assert any(c["pieces"] and c["page"] for c in cases.values()) and any(not c["pieces"] and c["page"] for c in cases.values())
    groups = lambda c: -(-c["H"] * c["R"] // mm.ROWS)  # noqa: E731
    assert groups(cases["s1 seam inside a head, unsplit"]) == 2 and groups(cases["s3 two groups, not causal"]) == 2
    assert not cases["s3 two groups, not causal"]["causal"]


@pytest.mark.parametrize("mutant", mm.SEAM_MUTANTS)
def test_a_seam_mutant_is_invisible_to_the_old_batch(mutant):
    """the gap the seam batch closes: by its own rule the defect changes nothing on any sequence of any case of LENS (and on the
    cheapest of them the mutated model IS the model), while some sequence of SEAM_LENS lets it show"""
    _what, harmless = mm.MUTANTS[mutant]
    for name, case in mm.CASES.items():
        assert all(harmless(mm.facts_of(case, mm.planned_pieces(case), n)) for n in case["lens"] if n), name
    case, pieces, q, kv, ref, _info = mm.inputs("4 one row")
    bad = mm.model(q, kv, case["lens"], case["causal"], mm.SCALE, mutant, pieces=pieces, page=case["page"])
    assert np.array_equal(bad.O, ref.O) and np.array_equal(bad.L, ref.L)
    for name, case in mm.SEAM_CASES.items():
        assert any(not harmless(mm.facts_of(case, mm.planned_pieces(case), n)) for n in case["lens"] if n), name


@pytest.mark.parametrize("mutant", sorted(mm.MUTANTS))
def test_every_mutant_lies_outside(mutant):
    """on at least one case where the defect can show the mutant's O or L leaves the bounds at MARGIN -- the first such case ends the
    walk; a mutant that shows nowhere fails"""
    _what, harmless = mm.MUTANTS[mutant]
    tried = []
    for name in mm.ALL_CASES:
        case, pieces = mm.ALL_CASES[name], mm.planned_pieces(mm.ALL_CASES[name])
        if all(harmless(mm.facts_of(case, pieces, n)) for n in case["lens"] if n):
            continue
        case, pieces, q, kv, ref, _info = mm.inputs(name)
        bad = mm.model(q, kv, case["lens"], case["causal"], mm.SCALE, mutant, pieces=pieces, page=case["page"], shared=case["layout"] == "shared")
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
    assert np.isfinite(bad.O).all(), "a mutant computes finite wrong values"
    pytest.fail("%s stays inside the bounds on every case where it can show: %r" % (mutant, tried))
