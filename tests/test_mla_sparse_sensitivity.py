"""CPU test of the oracle of tests/test_mla_sparse_gpu.py (tests/mla_sparse_model.py): on that file's cases -- CASES and, on the seam
batch of tests/mla_model.py with lists on the seams of the visibility rule, SEAM_CASES -- a correct kernel --
emulated(), the model with the kernel's roundings, its 32-slot steps with the holes in their slots and its pieces of slots -- lies inside
the bounds, and every named mutant, what a defect of the kernels or of the host plan would compute, lies outside on at least one case
where its defect can show.  MARGIN is fixed HERE, before any GPU run: the smallest power of two with at least 2 x headroom over
emulated()'s worst err / bound at margin 1.  No wrong kernel is ever run; the piece ranges and the piece counts are the built library's
own (mfa_attention_decode_piece_range over the slots, mfa_attention_mla_sparse_decode_workspace_size)."""
import numpy as np
import pytest

import mla_sparse_model as sm


def _ratio(o, l, ref, fmt, out):
    """worst |dO| / bound and |dL| / bound at margin 1 of a result before the store's rounding"""
    bo, bl = sm.bounds(ref, fmt, out, margin=1)
    wo = float((np.abs(sm.store(o, out) - ref.O) / bo).max())
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
    for name in sm.ALL_CASES:
        case, pieces, q, kv, idx, ref, _info = sm.inputs(name)
        o, l = sm.emulated(q, kv, case["lens"], idx, case["causal"], sm.SCALE, case["fmt"], pieces=pieces, shared=case["layout"] == "shared")
        out[name] = _ratio(o, l, ref, case["fmt"], case["out"])
        print("%s: emulated worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % ((name,) + out[name]))
    return out


def test_the_emulated_kernel_lies_inside_the_bounds(worst):
    for name, (wo, wl) in worst.items():
        assert wo <= sm.MARGIN and wl <= sm.MARGIN, (name, wo, wl)


def test_the_margin_is_the_smallest_power_of_two_with_twice_the_headroom(worst):
    top = max(max(pair) for pair in worst.values())
    want = 1
    while want < 2 * top:
        want *= 2
    assert sm.MARGIN == want, (sm.MARGIN, want, top)


def test_the_cases_meet_what_they_are_for():
    cases = sm.CASES
    vis = lambda name, b, r: sm.visible(sm.inputs(name)[4][b, r], sm.LENS[b], r, cases[name]["R"], cases[name]["causal"])  # noqa: E731
    assert [cases[n]["topk"] for n in cases if n.startswith("b ")] == [1, 31, 33]
    name = "c two groups, holes scattered, a first step of holes"
    idx = sm.inputs(name)[4]
    assert cases[name]["H"] == 40 and 40 % 32 and (idx[0, 0, :32] == sm.HOLE).all() and vis(name, 0, 0)[32:].any()
    assert vis(name, 5, 0)[:64].any() and not vis(name, 5, 0)[64:96].any() and vis(name, 5, 0)[96:].any()   # holes between visible steps
    assert any((idx[b, 0, 32:] == sm.HOLE).any() and (idx[b, 0, 32:] != sm.HOLE).any() for b in range(sm.B))
    name = "d causal, past the frontier and the length"
    idx = sm.inputs(name)[4]
    assert cases[name]["H"] * cases[name]["R"] == 33 and cases[name]["causal"]
    n, R = sm.LENS[0], cases[name]["R"]
    assert (idx[0, 0] >= n).any() and ((idx[0, 0] < n) & (idx[0, 0] > 0 + n - R)).any()     # at or past the length; past row 0's frontier
    assert any(len(np.unique(idx[b, 0][vis(name, b, 0)])) < int(vis(name, b, 0).sum()) for b in range(sm.B))   # a position named twice
    assert sm.planned_pieces(cases["f pages of 16, planned"]) == 2            # 6 workgroups: 85 aimed at, 8 tiles // 4 = 2
    assert sm.planned_pieces(cases["f pages of 256, planned"]) == 2           # 12 workgroups
    assert sm.page_table(16).shape == (sm.B, sm.C // 16) and sorted(sm.page_table(256).reshape(-1)) == list(range(sm.B * sm.C // 256))
    assert -(-160 // 64) < 7                                                  # "g": pieces without a slot
    name = "i a list of holes"
    assert not vis(name, 0, 1).any() and not vis(name, 2, 0).any() and (sm.inputs(name)[4][2, 0] == sm.C - 1).all() and 0 in sm.LENS
    for name in cases:
        idx = sm.inputs(name)[4]
        assert ((idx == sm.HOLE) | ((idx >= 0) & (idx < sm.C))).all(), name
    the_seam_cases_meet_what_they_are_for()


def the_seam_cases_meet_what_they_are_for():
    """(the second half of test_the_cases_meet_what_they_are_for)"""
    cases, lens, C = sm.SEAM_CASES, sm.SEAM_LENS, sm.SEAM_C
    assert all(c["lens"] == lens and c["C"] == C for c in cases.values()) and not set(cases) & set(sm.CASES)
    assert sorted({c["topk"] for c in cases.values()}) == [32, 33, 64, 96] and sorted({c["page"] for c in cases.values() if c["page"]}) == [16, 32, 64, 512]
    assert any(c["pieces"] and c["page"] for c in cases.values()) and any(c["pieces"] and not c["page"] for c in cases.values())
    assert C in lens and max(lens) > C and max(lens) < C + sm.PAD
    for name, case in cases.items():
        idx, R, causal, paged = sm.inputs(name)[4], case["R"], case["causal"], bool(case["page"])
        assert idx.shape == (len(lens), R, case["topk"])
        assert ((idx >= (0 if paged else -sm.PAD)) | (idx == sm.HOLE)).all() and (idx < C + sm.PAD).all(), name   # inside what the launch poisons
        assert paged == (case["layout"] == "packed") and (paged or case["layout"] == "padded")
        for b, raw in enumerate(lens):
            n = min(raw, C)
            for r in range(R if n else 0):
                row, vis = idx[b, r], sm.visible(idx[b, r], n, r, R, causal)
                fr = r + max(n - R, 0)
                assert {raw - 1, raw, 0} <= set(row) and (not causal or {fr, fr + 1} <= set(row)), (name, b, r)
                assert vis[row == 0].all() and vis[row == min(fr, n - 1) if causal else row == n - 1].all(), (name, b, r)   # the first and the last visible key
                assert not vis[row == n].any() and not vis[row < 0].any() and not vis[row >= C].any()
                if causal and fr + 1 < n:
                    assert not vis[row == fr + 1].any()
                if raw >= C and (not causal or r == R - 1):
                    assert vis[row == C - 1].all() and (row == C - 1).any(), (name, b, r)                # the column's last key is visible
                if raw > C:
                    assert ((row >= C) & (row < raw)).sum() >= 3 and {C, raw - 1} <= set(row)            # positions in [C, n): holes
                if paged:
                    assert (row >= C).any() and (row[row != sm.HOLE] >= 0).all()
                else:
                    assert {-2, -17, -sm.PAD} <= set(row)


@pytest.mark.parametrize("mutant", sm.SEAM_MUTANTS)
def test_a_seam_mutant_is_invisible_to_the_old_batch(mutant):
    """by its own rule the defect changes nothing on any sequence of any case of LENS -- no length reaches the column, no list holds an
    entry below -1 -- and on one of them the mutated model IS the model; some seam case lets it show"""
    _what, harmless = sm.MUTANTS[mutant]
    for name, case in sm.CASES.items():
        idx = sm.lists_of(case)
        assert all(harmless(sm.facts_of(case, sm.planned_pieces(case), n, idx)) for n in case["lens"] if n), name
    case, pieces, q, kv, idx, ref, _info = sm.inputs("b thirty-three slots")
    bad = sm.model(q, kv, case["lens"], idx, case["causal"], sm.SCALE, mutant, pieces=pieces, page=case["page"])
    assert np.array_equal(bad.O, ref.O) and np.array_equal(bad.L, ref.L)
    assert any(not harmless(sm.facts_of(case, sm.planned_pieces(case), n, sm.lists_of(case))) for case in sm.SEAM_CASES.values() for n in case["lens"] if n)


@pytest.mark.parametrize("mutant", sorted(sm.MUTANTS))
def test_every_mutant_lies_outside(mutant):
    """on at least one case where the defect can show the mutant's O or L leaves the bounds at MARGIN -- the first such case ends the
    walk; a mutant that shows nowhere fails"""
    _what, harmless = sm.MUTANTS[mutant]
    tried = []
    for name in sm.ALL_CASES:
        case, pieces, q, kv, idx, ref, _info = sm.inputs(name)
        if all(harmless(sm.facts_of(case, pieces, n, idx)) for n in case["lens"] if n):
            continue
        bad = sm.model(q, kv, case["lens"], idx, case["causal"], sm.SCALE, mutant, pieces=pieces, page=case["page"], shared=case["layout"] == "shared")
        fmt, out = case["fmt"], case["out"]
        bo, bl = sm.bounds(ref, fmt, out, sm.MARGIN)
        wo = (np.abs(sm.store(bad.O, out) - ref.O) / bo)
        wo = float(np.where(np.isnan(wo), np.inf, wo).max())                   # (err / bound at MARGIN: outside is > 1; poison is outside)
        both = np.isfinite(ref.L) & np.isfinite(bad.L)
        wl = float((np.abs(np.where(both, bad.L - np.where(both, ref.L, 0.0), 0.0)) / bl).max())
        if (np.isfinite(ref.L) != np.isfinite(bad.L)).any():
            wl = np.inf
        tried.append((name, wo, wl))
        if max(wo, wl) > 1.0:
            return
    assert tried, "no case lets %s show" % mutant
    assert mutant not in sm.SEAM_MUTANTS or np.isfinite(bad.O).all(), "a seam mutant computes finite wrong values"
    pytest.fail("%s stays inside the bounds on every case where it can show: %r" % (mutant, tried))
