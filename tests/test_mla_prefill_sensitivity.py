"""CPU test of the oracle of tests/test_mla_prefill_gpu.py (tests/mla_prefill_model.py): on that file's cases a correct kernel --
emulated(), the model with the kernel's roundings and order of sums -- lies inside bounds(), and every named mutant, what a defect of
the kernel or of its host side would compute, lies outside on at least one sequence where its own rule says the defect can show and
inside on every sequence where its rule says it cannot.  MARGIN is fixed HERE, before any GPU run: the smallest power of two with at
least 2 x headroom over emulated()'s worst err / bound at margin 1.  Two identities hold on the emulation bit for bit: a block of rows
fed as two chunks, and a launch of at most 32 rows against mla_model.emulated().  No wrong kernel is ever run, the library is not called."""
import numpy as np
import pytest

import mla_model as mm
import mla_prefill_model as pm


def _ratios(o, l, written, ref, ref_written, fmt, out, margin):
    """per sequence: the worst of |dO| / bound and |dL| / bound of a result before the store's rounding; inf where a row that must be
    written is not (or the reverse), or where one side has a visible key and the other none"""
    bo, bl = pm.bounds(ref, fmt, out, margin=margin)
    ro = (np.abs(pm.store(o, out) - ref.O) / bo).max(axis=(1, 2, 3))
    both = np.isfinite(ref.L) & np.isfinite(l)
    rl = np.where(both, np.abs(np.where(both, l, 0.0) - np.where(both, ref.L, 0.0)) / bl, 0.0)
    rl = np.where(np.isfinite(ref.L) != np.isfinite(l), np.inf, rl)
    rl = np.where(written != ref_written, np.inf, rl)
    return np.maximum(ro, rl.max(axis=(1, 2)))


@pytest.fixture(scope="module")
def worst():
    """name -> emulated()'s worst ratio at margin 1 on every case, once"""
    out = {}
    for name in pm.CASES:
        case, q, kv, ref, written, _info = pm.inputs(name)
        o, l = pm.emulated(q, kv, case["lens"], case["qlens"], case["causal"], pm.SCALE, case["fmt"], shared=case["layout"] == "shared")
        out[name] = float(_ratios(o, l, written, ref, written, case["fmt"], case["out"], 1).max())
        print("%s: emulated worst err / bound %.3f at margin 1" % (name, out[name]))
    return out


def test_the_emulated_kernel_lies_inside_the_bounds(worst):
    for name, w in worst.items():
        assert w <= pm.MARGIN, (name, w)


def test_the_margin_is_the_smallest_power_of_two_with_twice_the_headroom(worst):
    top = max(worst.values())
    want = 1
    while want < 2 * top:
        want *= 2
    assert pm.MARGIN == want, (pm.MARGIN, want, top)


def test_the_cases_meet_what_they_are_for():
    A, B = pm.BATCH_A, pm.BATCH_B
    assert A == (((700, 100), (200, 200), (100, 33), (5, 5), (0, 0), (1500, 65), (40, 64)), 1536, 200)
    assert B[1:] == (320, 130) and set(B[0]) == {(n or qn, qn) for qn in (1, 32, 33, 64, 65, 128, 130) for n in (0, 96, 256, 320, 400)}
    assert any(qn > n for n, qn in A[0]) and max(n for n, _qn in B[0]) > B[1]                  # qn > n; a length the launch clamps
    assert set(pm.BATCH_A2[0]) <= set(A[0]) and set(pm.BATCH_B2[0]) <= set(B[0])
    cases = pm.CASES.values()
    for batch in ("A", "B"):
        heads = {c["H"] for c in cases if c["batch"].startswith(batch)}
        assert heads == {1, 5, 16, 64, 128}, (batch, heads)
        assert {c["causal"] for c in cases if c["batch"] == batch} == {True, False}
    assert {c["fmt"] for c in cases} == {"bf16", "f16"} and "f32" in {c["out"] for c in cases}
    assert {c["layout"] for c in cases} == {"packed", "shared", "ld640"} and any(c["token_major"] for c in cases)
    assert {c["page"] for c in cases if c["page"]} == {16, 64, 512} and any(c["qlens"] is None for c in cases)
    assert 64 % 5 and -(-64 // 5) == 13                                                        # H = 5: a seam inside a row's heads, 13 rows a block
    assert all(len(c["lens"]) == 2 for c in cases if c["H"] >= 64)


def test_the_range_function_against_the_mask():
    """the Python step_range the model and the emulation walk (the library's is held to the same scan in test_mla_prefill_plans.py)"""
    for causal in (True, False):
        for H in (1, 5, 16, 64, 128):
            for n in (0, 1, 31, 32, 33, 64, 65, 100):
                for qn in (1, 2, 13, 33, 64, 100):
                    for p0 in range(0, qn * H + 64, 64):
                        f, e = pm.step_range(n, qn, p0, H, causal)
                        rows = [p // H for p in range(p0, p0 + 64) if p // H < qn]
                        lims = [min(n, r + max(n - qn, 0) + 1) if causal else n for r in rows]
                        want_e = -(-max(lims) // 32) if lims and n else 0
                        want_f = min(min(lims) // 32, want_e) if lims and n else 0
                        assert (f, e) == (want_f, want_e), (causal, H, n, qn, p0)


def test_the_mutants_are_the_issue_s():
    assert set(pm.MUTANTS) == {
        "head_major_packing", "head_div_h", "frontier_from_rows", "max_dropped", "block_end_from_first_row", "second_tile_rows_of_first",
        "second_tile_mask_of_first", "unmasked_one_step_too_far", "qn_of_neighbour", "rows_past_qn_written",
        "len_minus_2", "causal_plus_1", "causal_minus_1", "length_not_clamped", "page_table_neighbour", "page_off_by_one",
        "page_boundary_key_from_next_page", "v_from_tail", "rope_left_out", "scale_sqrt_dk", "o_blocks_exchanged", "wave_partial_dropped",
        "final_partial_step_dropped", "full_last_step_dropped"}
    assert set(pm.BITLESS_MUTANTS) == {"block_end_unclamped"} and not set(pm.BITLESS_MUTANTS) & set(pm.MUTANTS)
    assert {m for m in pm.MUTANTS if m in mm.MUTANTS} >= {"len_minus_2", "causal_plus_1", "causal_minus_1", "v_from_tail", "rope_left_out",
                                                        "scale_sqrt_dk", "o_blocks_exchanged", "wave_partial_dropped"}


ORDER = ["b4 one head, token-major, fp32 out", "n2 queryLengths NULL, five heads, not causal", "a8 one cache shared", "b1 five heads",
         "a2 five heads, a seam inside a row", "n1 queryLengths NULL", "b5 a block is one row", "a7 pages of 64", "b2 pages of 16"]


@pytest.mark.parametrize("mutant", sorted(pm.MUTANTS))
def test_every_mutant_lies_outside_where_it_can_show_and_inside_where_it_cannot(mutant):
    """the cheap cases first, then the rest; the walk ends with the first case on which a sequence the rule lets the defect show on
    leaves the bounds at MARGIN.  On every case walked, every sequence the rule calls harmless stays inside."""
    _what, harmless = pm.MUTANTS[mutant]
    tried = []
    for name in ORDER + [n for n in pm.CASES if n not in ORDER]:
        case = pm.CASES[name]
        calm = [harmless(pm.facts_of(case, b)) for b in range(len(case["lens"]))]
        if all(calm):
            continue
        case, q, kv, ref, written, _info = pm.inputs(name)
        bad, bad_written = pm.model(q, kv, case["lens"], case["qlens"], case["causal"], pm.SCALE, mutant, page=case["page"],
                                    shared=case["layout"] == "shared")
        assert np.isfinite(bad.O).all(), "a mutant computes finite wrong values"
        ratios = _ratios(bad.O, bad.L, bad_written, ref, written, case["fmt"], case["out"], pm.MARGIN)   # (outside is > 1)
        for b, quiet in enumerate(calm):
            assert not quiet or ratios[b] <= 1.0, "%s shows on sequence %d of %s, where its rule says it cannot: %r" % (mutant, b, name, ratios[b])
        tried.append((name, float(ratios.max())))
        if ratios.max() > 1.0:
            return
    assert tried, "no case lets %s show" % mutant
    pytest.fail("%s stays inside the bounds on every case where it can show: %r" % (mutant, tried))


def test_the_bitless_mutant_is_the_model():
    """a block's end from an unclamped last row adds steps that are masked for every live row: no bit changes (the module's text)"""
    for name in ("b1 five heads", "a8 one cache shared"):
        case, q, kv, ref, written, _info = pm.inputs(name)
        bad, bad_written = pm.model(q, kv, case["lens"], case["qlens"], case["causal"], pm.SCALE, "block_end_unclamped",
                                    shared=case["layout"] == "shared")
        assert np.array_equal(bad.O, ref.O) and np.array_equal(bad.L, ref.L) and np.array_equal(bad_written, written)


@pytest.mark.parametrize("H,fmt", [(5, "bf16"), (16, "f16")])
def test_chunk_invariance_on_the_emulation(H, fmt):
    """emulated() of one block of qn rows equals emulated() of the same rows fed as two chunks, bit for bit: the first chunk with
    n - second keys, the second with n.  (ordered=True: an order of sums that does not depend on the call's shapes)"""
    n, qn, second, C, R = 150, 70, 26, 160, 70
    kv = mm.cache_values(fmt, 3, 1, C)
    q, _info = pm.needle_queries(kv, (n,), (qn,), H, R, True, fmt, pm.SCALE)
    whole = pm.emulated(q, kv, (n,), (qn,), True, pm.SCALE, fmt, ordered=True)
    first = pm.emulated(q[:, :, :qn - second], kv, (n - second,), (qn - second,), True, pm.SCALE, fmt, ordered=True)
    last = pm.emulated(q[:, :, qn - second:], kv, (n,), (second,), True, pm.SCALE, fmt, ordered=True)
    for i in (0, 1):
        assert np.array_equal(whole[i][:, :, :qn - second], first[i]) and np.array_equal(whole[i][:, :, qn - second:qn], last[i][:, :, :second])
    assert np.isfinite(whole[1][:, :, :qn]).all()


@pytest.mark.parametrize("name", ["1 unsplit", "s1 seam inside a head, unsplit", "5 four rows, not causal"])
def test_decode_identity_on_the_emulation(name):
    """with at most 32 rows and every sequence at its capacity, emulated() is mla_model.emulated() unsplit, bit for bit"""
    case, _pieces, q, kv, _ref, _info = mm.inputs(name)
    assert case["R"] <= 32
    shared = case["layout"] == "shared"
    want = mm.emulated(q, kv, case["lens"], case["causal"], mm.SCALE, case["fmt"], pieces=None, shared=shared)
    got = pm.emulated(q, kv, case["lens"], None, case["causal"], pm.SCALE, case["fmt"], shared=shared)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
