"""CPU test of the oracle of tests/test_mla_cache_gpu.py (tests/mla_fp8_model.py): on that file's cases -- CASES and, on the seam batch
of tests/mla_model.py, SEAM_CASES -- a correct kernel -- emulated(),
the model with the roundings and the order of sums of attn_mla8.h -- lies inside the bounds, and every named mutant, what a defect of the
e4m3 kernels or of the host plan would compute, lies outside on at least one case where its defect can show.  MARGIN is fixed HERE,
before any GPU run: the smallest power of two with at least 2 x headroom over emulated()'s worst err / bound at margin 1.  No wrong
kernel is ever run; the piece ranges, the piece counts and the codec are the built library's own."""
import numpy as np
import pytest

import mla_fp8_model as fm
from metal_flash_attention_amd import dequantizeE4M3


def _ratio(o, l, ref, fmt, out):
    """worst |dO| / bound and |dL| / bound at margin 1 of a result before the store's rounding"""
    bo, bl = fm.bounds(ref, fmt, out, margin=1)
    wo = float((np.abs(fm.store(o, out) - ref.O) / bo).max())
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
    for name in fm.ALL_CASES:
        case, pieces, q, kvb, ref, _info = fm.inputs(name)
        o, l = fm.emulated(q, kvb, case["kvscale"], case["lens"], case["causal"], fm.SCALE, case["fmt"], pieces=pieces, shared=case["layout"] == "shared")
        out[name] = _ratio(o, l, ref, case["fmt"], case["out"])
        print("%s (kvScale %s): emulated worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % ((name, case["kvscale"]) + out[name]))
    print("emulated worst ratio over all cases: %.3f" % max(max(pair) for pair in out.values()))
    return out


def test_the_model_s_codec_is_the_library_s():
    values = fm.dequantize(np.arange(256))
    for byte in range(256):
        want = dequantizeE4M3(byte)
        assert (np.isnan(values[byte]) and want != want) or values[byte] == want, byte
    assert [b for b in range(256) if np.isnan(values[b])] == list(fm.POISON)
    kvb = fm.cache_bytes()
    assert kvb.dtype == np.uint8 and not np.isin(kvb, fm.POISON).any() and float(np.abs(fm.dequantize(kvb)).max()) == 1.0


def test_the_emulated_kernel_lies_inside_the_bounds(worst):
    for name, (wo, wl) in worst.items():
        assert wo <= fm.MARGIN and wl <= fm.MARGIN, (name, wo, wl)


def test_the_margin_is_the_smallest_power_of_two_with_twice_the_headroom(worst):
    top = max(max(pair) for pair in worst.values())
    want = 1
    while want < 2 * top:
        want *= 2
    assert fm.MARGIN == want, (fm.MARGIN, want, top)


def test_the_cases_meet_what_they_are_for():
    assert list(fm.CASES) == list(fm.mm.CASES) and all({k: v for k, v in c.items() if k != "kvscale"} == fm.mm.CASES[n] for n, c in fm.CASES.items())
    for scale in fm.KV_SCALES:   # every scale meets a launch in pieces and one without a workspace
        mine = [c for c in fm.CASES.values() if c["kvscale"] == scale]
        assert any(c["pieces"] for c in mine) and any(not c["pieces"] for c in mine), scale
    assert all(s is None or (np.log2(s) % 1) for s in fm.KV_SCALES)           # no power of two
    assert len(fm.SCALE_TAIL) >= len(fm.LENS) - 1 and all(abs(t / s - 1) > 0.2 for t in fm.SCALE_TAIL for s in fm.KV_SCALES if s)
    assert set(fm.mm.MUTANTS) < set(fm.MUTANTS) and len(fm.OWN_MUTANTS) == 7
    assert list(fm.SEAM_CASES) == list(fm.mm.SEAM_CASES)                      # (what the seam batch holds: tests/test_mla_sensitivity.py)
    assert all({k: v for k, v in c.items() if k != "kvscale"} == fm.mm.SEAM_CASES[n] for n, c in fm.SEAM_CASES.items())
    for scale in fm.KV_SCALES:
        mine = [c for c in fm.SEAM_CASES.values() if c["kvscale"] == scale]
        assert any(c["pieces"] for c in mine) and any(not c["pieces"] for c in mine) and any(c["page"] for c in mine), scale
    assert len(fm.cache_bytes(0, len(fm.SEAM_LENS), fm.SEAM_C)) == len(fm.SEAM_LENS) and not np.isin(fm.cache_bytes(0, len(fm.SEAM_LENS), fm.SEAM_C), fm.POISON).any()


@pytest.mark.parametrize("mutant", fm.SEAM_MUTANTS)
def test_a_seam_mutant_is_invisible_to_the_old_batch(mutant):
    """by its own rule the defect changes nothing on any sequence of any case of LENS; some sequence of every seam case lets it show"""
    _what, harmless = fm.MUTANTS[mutant]
    for name, case in fm.CASES.items():
        assert all(harmless(dict(fm.facts_of(case, fm.planned_pieces(case), n), kvscale=case["kvscale"])) for n in case["lens"] if n), name
    for name, case in fm.SEAM_CASES.items():
        assert any(not harmless(dict(fm.facts_of(case, fm.planned_pieces(case), n), kvscale=case["kvscale"])) for n in case["lens"] if n), name


@pytest.mark.parametrize("mutant", sorted(fm.MUTANTS))
def test_every_mutant_lies_outside(mutant):
    """on at least one case where the defect can show the mutant's O or L leaves the bounds at MARGIN -- the first such case ends the
    walk; a mutant that shows nowhere fails"""
    _what, harmless = fm.MUTANTS[mutant]
    tried = []
    for name in fm.ALL_CASES:
        case, pieces = fm.ALL_CASES[name], fm.planned_pieces(fm.ALL_CASES[name])
        if all(harmless(dict(fm.facts_of(case, pieces, n), kvscale=case["kvscale"])) for n in case["lens"] if n):
            continue
        case, pieces, q, kvb, ref, _info = fm.inputs(name)
        bad = fm.model(q, kvb, case["kvscale"], case["lens"], case["causal"], fm.SCALE, mutant, pieces=pieces, page=case["page"],
                       shared=case["layout"] == "shared")
        fmt, out = case["fmt"], case["out"]
        bo, bl = fm.bounds(ref, fmt, out, margin=fm.MARGIN)
        wo = float((np.abs(fm.store(bad.O, out) - ref.O) / bo).max())          # (err / bound at MARGIN: outside is > 1)
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
