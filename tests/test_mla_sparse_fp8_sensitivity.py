"""CPU test of the oracle of tests/test_mla_sparse_fp8_gpu.py (tests/mla_sparse_fp8_model.py): on that file's cases -- mla_sparse_model's
CASES and SEAM_CASES restated over byte caches with a kvScale of 0.37, 3.0 and None in turn -- a correct kernel -- emulated(), the model
with the 32-slot steps and holes of attn_mla16_sparse.h and the scale roundings of attn_mla8.h -- lies inside the bounds, and every
named mutant, what a defect of the kernels or of the host plan would compute, lies outside on at least one case where its defect can
show.  MARGIN is fixed HERE, before any GPU run: the smallest power of two with at least 2 x headroom over emulated()'s worst
err / bound at margin 1.  No wrong kernel is ever run; the piece ranges, the piece counts and the codec are the built library's own
(mfa_attention_decode_piece_range over the slots, mfa_attention_mla_sparse_decode_fp8_workspace_size, mfa_kv_dequantize_e4m3)."""
import numpy as np
import pytest

import mla_sparse_fp8_model as xm
from metal_flash_attention_amd import dequantizeE4M3


def _ratio(o, l, ref, fmt, out):
    """worst |dO| / bound and |dL| / bound at margin 1 of a result before the store's rounding"""
    bo, bl = xm.bounds(ref, fmt, out, margin=1)
    wo = float((np.abs(xm.store(o, out) - ref.O) / bo).max())
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
    for name in xm.ALL_CASES:
        case, pieces, q, kvb, idx, ref, _info = xm.inputs(name)
        o, l = xm.emulated(q, kvb, case["kvscale"], case["lens"], idx, case["causal"], xm.SCALE, case["fmt"], pieces=pieces,
                           shared=case["layout"] == "shared")
        out[name] = _ratio(o, l, ref, case["fmt"], case["out"])
        print("%s (kvScale %s): emulated worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % ((name, case["kvscale"]) + out[name]))
    print("emulated worst ratio over all cases: %.3f" % max(max(pair) for pair in out.values()))
    return out


def test_the_model_s_codec_is_the_library_s():
    values = xm.dequantize(np.arange(256))
    for byte in range(256):
        want = dequantizeE4M3(byte)
        assert (np.isnan(values[byte]) and want != want) or values[byte] == want, byte
    assert [b for b in range(256) if np.isnan(values[b])] == list(xm.POISON)


def test_the_emulated_kernel_lies_inside_the_bounds(worst):
    for name, (wo, wl) in worst.items():
        assert wo <= xm.MARGIN and wl <= xm.MARGIN, (name, wo, wl)


def test_the_margin_is_the_smallest_power_of_two_with_twice_the_headroom(worst):
    top = max(max(pair) for pair in worst.values())
    want = 1
    while want < 2 * top:
        want *= 2
    assert xm.MARGIN == want, (xm.MARGIN, want, top)


def test_the_cases_are_the_sparse_model_s_over_bytes():
    import mla_sparse_model as sm
    assert list(xm.CASES) == list(sm.CASES) and list(xm.SEAM_CASES) == list(sm.SEAM_CASES)
    for i, (name, case) in enumerate(xm.ALL_CASES.items()):
        assert {k: v for k, v in case.items() if k != "kvscale"} == sm.ALL_CASES[name], name
    for group in (xm.CASES, xm.SEAM_CASES):
        assert [c["kvscale"] for c in group.values()][:3] == [0.37, 3.0, None]
    for name in xm.ALL_CASES:
        case, pieces, _q, kvb, idx, _ref, _info = xm.inputs(name)
        assert kvb.dtype == np.uint8 and not np.isin(kvb, xm.POISON).any()
        assert np.array_equal(idx, sm.inputs(name)[4]) and pieces == sm.inputs(name)[1], name
    # every kvScale meets a split launch, a paged one and the seam batch
    assert {c["kvscale"] for c in xm.ALL_CASES.values() if c["pieces"]} == {0.37, 3.0, None}
    assert {c["kvscale"] for c in xm.SEAM_CASES.values()} == {0.37, 3.0, None}


def test_the_mutants_are_those_the_model_names():
    import mla_fp8_model as fm
    import mla_sparse_model as sm
    assert set(sm.MUTANTS) <= set(xm.MUTANTS) and set(sm.SEAM_MUTANTS) <= set(xm.MUTANTS) and set(sm.DENSE_MUTANTS) <= set(xm.MUTANTS)
    # kvScale[b] of the dense e4m3 model is kvScale[b R + r] after the reduction: the combination's own kv_scale_per_row
    assert set(fm.OWN_MUTANTS) - {"kv_scale_per_sequence"} <= set(xm.MUTANTS)
    assert {"row_address_in_16bit_elements", "hole_keeps_previous_rows", "kv_scale_per_row"} <= set(xm.OWN_MUTANTS) <= set(xm.MUTANTS)


@pytest.mark.parametrize("mutant", xm.SEAM_MUTANTS)
def test_a_seam_mutant_is_invisible_to_the_old_batch(mutant):
    _what, harmless = xm.MUTANTS[mutant]
    for name, case in xm.CASES.items():
        idx = xm.lists_of(case)
        assert all(harmless(xm.facts_of(case, xm.planned_pieces(case), n, idx)) for n in case["lens"] if n), name
    case, pieces, q, kvb, idx, ref, _info = xm.inputs("b thirty-three slots")
    bad = xm.model(q, kvb, case["kvscale"], case["lens"], idx, case["causal"], xm.SCALE, mutant, pieces=pieces, page=case["page"])
    assert np.array_equal(bad.O, ref.O) and np.array_equal(bad.L, ref.L)


@pytest.mark.parametrize("mutant", sorted(xm.MUTANTS))
def test_every_mutant_lies_outside(mutant):
    """on at least one case where the defect can show the mutant's O or L leaves the bounds at MARGIN -- the first such case ends the
    walk; a mutant that shows nowhere fails"""
    _what, harmless = xm.MUTANTS[mutant]
    tried = []
    for name in xm.ALL_CASES:
        case, pieces, q, kvb, idx, ref, _info = xm.inputs(name)
        if all(harmless(xm.facts_of(case, pieces, n, idx)) for n in case["lens"] if n):
            continue
        bad = xm.model(q, kvb, case["kvscale"], case["lens"], idx, case["causal"], xm.SCALE, mutant, pieces=pieces, page=case["page"],
                       shared=case["layout"] == "shared")
        fmt, out = case["fmt"], case["out"]
        bo, bl = xm.bounds(ref, fmt, out, xm.MARGIN)
        wo = (np.abs(xm.store(bad.O, out) - ref.O) / bo)
        wo = float(np.where(np.isnan(wo), np.inf, wo).max())                   # (err / bound at MARGIN: outside is > 1; poison is outside)
        both = np.isfinite(ref.L) & np.isfinite(bad.L)
        wl = float((np.abs(np.where(both, bad.L - np.where(both, ref.L, 0.0), 0.0)) / bl).max())
        if (np.isfinite(ref.L) != np.isfinite(bad.L)).any():
            wl = np.inf
        tried.append((name, wo, wl))
        if max(wo, wl) > 1.0:
            return
    assert tried, "no case lets %s show" % mutant
    pytest.fail("%s stays inside the bounds on every case where it can show: %r" % (mutant, tried))
