"""CPU test of the oracle of the MLA indexer's GPU files (tests/mla_index_model.py): on their cases -- the 24 logits launches and 15
selections tests/test_mla_index_gpu.py has always made, and the step, stride, head and selection-round seams of
tests/test_mla_index_seams_gpu.py -- a correct kernel, emulated_logits() / emulated_select() with the kernels' own walk, lies inside the
bound (2 x 161 x 2^-24 x sum |W| sum |q k|, no margin; the lists exactly numpy's lexsort), and every named mutant, what a defect of the
kernels or of the host plan would compute, lies outside on at least one case where its defect can show.  The mutants of NEW_MUTANTS are
proven invisible to the old cases: that was the gap.  No wrong kernel is ever run; the plans (steps, tiles) are the built library's own
(launchForm)."""
import numpy as np
import pytest

import mla_index_model as im


@pytest.fixture(scope="module")
def worst():
    """name -> emulated_logits()'s worst err / bound on every logits case, once"""
    out = {}
    for name in im.ALL_CASES:
        out[name] = im.verdict(im.emulated_logits(name), name)
    for group in (im.OLD_CASES, im.HEAD_CASES, *({n: 0 for n in im.STEP_CASES if n.startswith(p)} for p in im.PLANS)):
        print("emulated worst err / bound %.2e over %s .. %s" % (max(out[n] for n in group), next(iter(group)), list(group)[-1]))
    return out


def test_the_emulated_logits_lie_inside_the_bound(worst):
    for name, ratio in worst.items():
        assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("name", list(im.ALL_SELECT_CASES))
def test_the_emulated_selection_is_the_lexsort(name):
    assert np.array_equal(im.emulated_selection(name), im.select_wanted(name))


def test_the_cases_meet_what_they_are_for():
    plans = {p: im.plan_of("%s contiguous" % p) for p in im.PLANS}
    assert [plans[p][:2] for p in ("m2", "m4", "m8")] == [(2, 3), (4, 2), (8, 2)]
    for p, (_fmt, _H, R, lens, C) in im.PLANS.items():
        steps, tiles, form = plans[p]
        assert form == im.PLAN_FORMS[p] % "contiguous" and im.plan_of("%s paged" % p)[2] == im.PLAN_FORMS[p] % "paged"
        keys = im.STEP * im.WAVES * steps
        assert tiles >= 2 and 0 < C - (tiles - 1) * keys < keys and -(-(C - (tiles - 1) * keys) // 128) < steps   # a last tile of fewer steps
        v = set(im.visible(lens, R, True, C).reshape(-1))
        assert {keys, keys + 1} <= v                                         # a tile seam: the next tile empty, then holding one key
        assert any(n % 128 == 0 and n % keys and {n, n + 1} <= v for n in range(128, C, 128))   # a step seam inside a tile: `after < v`
        assert any(n % 32 == 0 and n % 128 and {n, n + 1} <= v for n in range(32, C, 32))       # a wave seam
        assert C in v and 0 in lens and sum(n > C for n in lens) == 2 and sum(0 < n < R for n in lens) >= 2
        assert {"%s %s" % (p, k) for k in ("contiguous", "strided", "paged", "not causal")} <= set(im.STEP_CASES)
        assert not im.STEP_CASES["%s not causal" % p]["causal"]
    assert [C - (t - 1) * 128 * s for (s, t, _f), C in zip(plans.values(), (640, 600, 1101))] == [128, 88, 77]
    assert 1101 % 4 and (1101 + 3) // 4 * 4 == 1104                          # the chain's padded stride differs from the column
    heads = im.HEAD_CASES.values()
    assert {c["H"] for c in heads} >= {1, 31, 32, 33, 64} and {c["R"] for c in heads} >= {1, 2, 32}
    assert {c["page"] for c in heads} >= {16, 64, 256, 1024} and {c["q"] for c in heads} == {"padded", "transposed"}
    assert any(c["k"] == "one page" for c in heads) and any(c["w"] == "padded" and c["R"] > 1 for c in heads)
    assert all(im.plan_of(n)[0] == 1 for n in im.HEAD_CASES) and all(im.plan_of(n)[0] == 1 for n in im.OLD_CASES)
    # the selections: ties that straddle a round, greater keys in the last round only, a list that fills in the last round, NaN inside v
    facts = {n: im.select_rows_facts(n) for n in im.NEW_SELECT_CASES}
    assert any(f["rounds"] >= 2 and f["t"][0] and f["t"][1] and f["want"] > f["t"][0] for f in facts["s equal top 4097"])
    assert any(f["rounds"] == 5 and f["want"] > sum(f["t"][:4]) for f in facts["s equal top 19999"])
    assert any(f["rounds"] == 5 and sum(f["g"][:4]) == 0 and f["g"][4] and 0 < f["want"] <= f["t"][0] for f in facts["s two levels top 5000"])
    assert any(f["rounds"] == 5 for f in facts["s normal top 5000"]) and any(f["nan"] for f in facts["s specials top 5000"])
    assert {c["topk"] for c in im.NEW_SELECT_CASES.values()} >= {1, 33, 2048, 4097, 5000, 8193, 19999}
    assert all(c["pad"] and c["column"] == 20000 and c["R"] == 2 for c in im.NEW_SELECT_CASES.values())
    assert all(max(f["rounds"] for f in im.select_rows_facts(n)) <= 2 for n in im.OLD_SELECT_CASES)


def _shows(mutant, cases, select):
    """the first case of `cases` on which the mutant can show (by its rule) and does, or None, and what was tried"""
    _what, harmless = im.MUTANTS[mutant]
    tried = []
    for name in cases:
        if select:
            if all(harmless(f) for f in im.select_rows_facts(name)):
                continue
            outside = not np.array_equal(im.emulated_selection(name, mutant), im.select_wanted(name))
        else:
            if harmless(im.logit_facts(name)):
                continue
            outside = im.verdict(im.emulated_logits(name, mutant), name) > 1.0
        tried.append(name)
        if outside:
            return name, tried
    return None, tried


@pytest.mark.parametrize("mutant", sorted(im.MUTANTS))
def test_every_mutant_lies_outside(mutant):
    """on at least one case where the defect can show the mutant's logits leave the bound (or touch a sentinel, or leave one), its lists
    differ from the lexsort's; the new cases are walked first and the first such case ends the walk; a mutant that shows nowhere fails"""
    select = mutant in im.SELECT_MUTANTS
    cases = (list(im.NEW_SELECT_CASES) + list(im.OLD_SELECT_CASES)) if select else (list(im.NEW_CASES) + list(im.OLD_CASES))
    found, tried = _shows(mutant, cases, select)
    assert tried, "no case lets %s show" % mutant
    assert found, "%s stays inside on every case where it can show: %r" % (mutant, tried)
    print("%s: outside on %r" % (mutant, found))


def test_the_new_mutants_are_the_ones_the_old_cases_cannot_see():
    """NEW_MUTANTS is exactly the set of mutants whose rule calls them harmless on every old case"""
    blind = []
    for mutant, (_what, harmless) in im.MUTANTS.items():
        if mutant in im.SELECT_MUTANTS:
            ok = all(harmless(f) for name in im.OLD_SELECT_CASES for f in im.select_rows_facts(name))
        else:
            ok = all(harmless(im.logit_facts(name)) for name in im.OLD_CASES)
        blind += [mutant] if ok else []
    assert sorted(blind) == sorted(im.NEW_MUTANTS)


@pytest.mark.parametrize("mutant", im.NEW_MUTANTS)
def test_a_new_mutant_is_invisible_to_the_old_cases(mutant):
    """by its own rule the defect changes nothing on any old case (the test above), and on old cases the mutated emulation IS the
    emulation, bit for bit; some new case lets it show (test_every_mutant_lies_outside)"""
    if mutant in im.SELECT_MUTANTS:
        for name in ("old normal top 2048", "old ties top 2048", "old equal top 33"):
            assert np.array_equal(im.emulated_selection(name, mutant), im.emulated_selection(name)), name
    else:
        for name in ("old f16 40 heads 3 rows paged", "old bf16 64 heads 1 rows strided"):
            assert np.array_equal(im.emulated_logits(name, mutant).view(np.uint32), im.emulated_logits(name).view(np.uint32)), name


@pytest.mark.parametrize("mutant", sorted(set(im.MUTANTS) - set(im.NEW_MUTANTS)))
def test_the_other_mutants_were_already_seen(mutant):
    """the mutants outside NEW_MUTANTS are defects an old case does show: they are kept so that the new cases are known not to have
    lost them"""
    select = mutant in im.SELECT_MUTANTS
    found, _tried = _shows(mutant, list(im.OLD_SELECT_CASES if select else im.OLD_CASES), select)
    assert found, mutant
