"""CPU test: the bound the prefill GPU tests hold the kernels to (tests/prefill_model.py: decode_model.bounds on the per-sequence model
plus this kernel's longer chain) is tight enough to see a defect and loose enough for a correct kernel -- the proof of
tests/test_decode_sensitivity.py at this kernel's seams.

  * prefill_model.emulated(), a reference with the kernel's roundings and order of sums, stays inside the bound at margin 1 on every
    case (its worst err / bound is printed; DESIGN.md 4.11 records it, and MARGIN is derived from it and the kernels' figure).
  * every named mutant of prefill_model.MUTANTS -- what a defect of the kernel or the host plan would compute, evaluated in float64;
    no wrong kernel is run -- breaks the bound at the committed MARGIN on every case in which it changes anything, with the needle
    queries the GPU tests use.
"""
import functools

import numpy as np
import pytest

import decode_model as dm
import prefill_model as pm

D, HKV, R, C, PAGE = 64, 2, 140, 320, 16
SEQS = [(129, 300), (40, 200), (70, 65), (33, 33)]      # (qn, n): two row blocks at G = 1, a prefix, fewer keys than rows, no prefix
QLENS, LENS = [s[0] for s in SEQS], [s[1] for s in SEQS]
CASES = [(G, causal, fmt, scales) for G in (1, 4, 3) for causal in (True, False) for fmt, scales in (("bf16", False), ("f16", True))]
WORST = {}


def case_dict(G, causal, scales):
    return dict(n=LENS, qn=QLENS, R=R, G=G, Hkv=HKV, B=len(SEQS), causal=causal, page=PAGE, scales=scales)


@functools.lru_cache(maxsize=None)
def inputs(G, causal, fmt, scales):
    rng = np.random.default_rng(7 + G)
    k = dm.round_to(rng.uniform(-1, 1, (len(SEQS), HKV, C, D)), fmt)     # (values everywhere: a defect may read past a length)
    v = dm.round_to(rng.uniform(-1, 1, (len(SEQS), HKV, C, D)), fmt)
    ks, vs = (dm.spread_scales(rng, HKV), dm.spread_scales(rng, HKV)) if scales else (None, None)
    kseen = k * ks[None, :, None, None] if scales else k
    q, info = pm.needle_queries(kseen, LENS, QLENS, HKV * G, G, R, causal, fmt, page=PAGE)
    ref = pm.model(q, k, v, LENS, QLENS, G, causal, kscale=ks, vscale=vs)
    return q, k, v, ks, vs, ref, info


@pytest.mark.parametrize("G,causal,fmt,scales", CASES)
def test_emulated_reference_stays_inside_the_bound_at_margin_1(G, causal, fmt, scales):
    q, k, v, ks, vs, ref, info = inputs(G, causal, fmt, scales)
    O, L = pm.emulated(q, k, v, LENS, QLENS, G, causal, fmt, kscale=ks, vscale=vs)
    for out in (fmt, "f32"):
        wo, wl, text = pm.compare(dm.store(O, out), L, ref, fmt, out, LENS, QLENS, margin=1, info=info)
        WORST["emulated"] = max(WORST.get("emulated", 0.0), wo, wl)
        assert wo <= 1.0 and wl <= 1.0, text
    print("emulated reference: worst err / bound at margin 1 so far %.3f" % WORST["emulated"])
    assert 2 * WORST["emulated"] <= pm.MARGIN, "MARGIN keeps 2 x headroom over the emulated reference"


@pytest.mark.parametrize("mutant", sorted(pm.MUTANTS))
@pytest.mark.parametrize("G,causal,fmt,scales", CASES)
def test_every_mutant_breaks_the_bound(G, causal, fmt, scales, mutant):
    q, k, v, ks, vs, ref, info = inputs(G, causal, fmt, scales)
    O, L = pm.mutated(q, k, v, LENS, QLENS, G, causal, mutant, page=PAGE, kscale=ks, vscale=vs)
    changes_nothing = pm.MUTANTS[mutant][1](case_dict(G, causal, scales))
    live = np.zeros(O.shape[:3], dtype=bool)
    for b, (qn, n) in enumerate(SEQS):
        live[b, :, :qn] = n > 0
    O0, L0 = pm.mutated(q, k, v, LENS, QLENS, G, causal, None, page=PAGE, kscale=ks, vscale=vs)
    assert np.allclose(O0[live], ref.O[live], rtol=1e-9, atol=1e-12) and np.allclose(L0[live], ref.L[live], rtol=1e-9, atol=1e-12)
    same = np.array_equal(O[live], O0[live]) and np.array_equal(L[live], L0[live])
    if changes_nothing:
        assert same, "%s: declared to change nothing here, but it does" % mutant
        return
    assert not same, "%s: declared to change something here, but it does not" % mutant
    wo, wl, text = pm.compare(O, L, ref, fmt, fmt, LENS, QLENS, margin=pm.MARGIN, info=info)
    assert max(wo, wl) > 1.0, "%s (%s) stays inside the bound at margin %g: worst |dO| / bound %.3f, |dL| / bound %.3f" % (
        mutant, pm.MUTANTS[mutant][0], pm.MARGIN, wo, wl)


def test_mutant_list_names_the_seams():
    assert set(pm.MUTANTS) == {"tile_range_short", "tile_range_long_unmasked", "frontier_from_rows", "max_dropped", "unpack_mod_g", "r0_dropped",
                               "kv_head_mod", "page_table_neighbour", "page_off_by_one", "key_scale_next_head", "value_scale_next_head",
                               "value_scale_omitted"}
