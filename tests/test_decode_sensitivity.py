"""CPU test (no GPU call): the checks of tests/test_decode_gpu.py and tests/test_kvcache_gpu.py (tests/decode_kit.py) can see a wrong key.

For both input families of the GPU files (16-bit caches with K, V ~ U(-1, 1); e4m3 caches with K, V ~ N(0, 1) under per-head scales),
at 1, 31, 33, 65, 600, 4096 and 32768 keys, causal or not, split or not, paged or not, with the needle queries of
tests/decode_model.py:

  (a) the rounding-emulated reference (decode_model.emulated: P rounded to the 16-bit type, sums in wave, piece and combine order,
      the store's rounding) is inside the per-element bounds for bf16 and f16, 16-bit and FP32 O, with 2 x headroom at the committed
      margin;
  (b) every named mutant of the model (decode_model.MUTANTS) breaks the O or the L bound on every case in which it changes anything,
      under the widest bound of the four (bf16 with a bf16 O), and is exercised by at least one case.  No wrong kernel is ever run;
  (c) the same mutants under the inputs and bounds the GPU files had before (uniform or normal queries; O 5e-2, L 7e-3): the table
      of what went unnoticed, printed by `python tests/test_decode_sensitivity.py`;
  (d) the GPU files take their bound, margin and checker from decode_model (identity of the imported objects).

Split cases take their piece ranges from mfa_attention_decode_piece_range and are skipped without the library.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

import decode_model as dm  # noqa: E402

LENGTHS = (1, 31, 33, 65, 600, 4096, 32768)
#          n: (D, G, R): n < R; ordinary; G R = 32 exactly; G R odd; R = 1; 16 packed rows; the long case's group
SHAPES = {1: (64, 1, 4), 31: (128, 4, 2), 33: (64, 8, 4), 65: (128, 3, 1), 600: (128, 8, 1), 4096: (64, 4, 4), 32768: (128, 8, 1)}
HKV = 2
FAMILIES = ("u16", "fp8")


def _library():
    try:
        from metal_flash_attention_amd import _abi
        _abi.lib()
        return True
    except Exception:  # noqa: BLE001 -- not built
        return False


HAVE_LIBRARY = _library()


def cases():
    out = []
    for family in FAMILIES:
        for n in LENGTHS:
            D, G, R = SHAPES[n]
            for variant in range(4):
                causal, split = not variant & 1, bool(variant & 2)
                page = (16 if n % 2 else 64) if variant in (0, 3) else None
                out.append(dict(family=family, n=n, D=D, G=G, R=R, Hkv=2 * HKV if n > 4096 else HKV, B=1 if n > 4096 else 2, causal=causal,
                                pieces=(64 if n > 4096 else 16) if split else None, page=page, scales=family == "fp8"))
    return out


CASES = cases()
case_id = lambda c: "%s-n%d-%s-%s-%s" % (c["family"], c["n"], "causal" if c["causal"] else "full",  # noqa: E731
                                         "p%d" % c["pieces"] if c["pieces"] else "unsplit", "page%d" % c["page"] if c["page"] else "flat")


def quantise_e4m3(x):
    """float64 -> the e4m3fn values nearest to x (round-half-even, saturating at 448), as float64"""
    a = np.minimum(np.abs(x), 448.0)
    e = np.maximum(np.floor(np.log2(np.maximum(a, 2.0 ** -20))), -6.0)
    quantum = 2.0 ** (e - 3)
    return np.sign(x) * np.minimum(np.round(a / quantum) * quantum, 448.0)


def cache_values(case, fmt, seed):
    """-> k, v [B, Hkv, n, D] without the scales, kscale, vscale (None for the 16-bit family)"""
    rng = np.random.default_rng(seed)
    shape = (case["B"], case["Hkv"], case["n"], case["D"])
    if case["family"] == "u16":
        return dm.round_to(rng.uniform(-1, 1, shape), fmt), dm.round_to(rng.uniform(-1, 1, shape), fmt), None, None
    ks, vs = dm.spread_scales(rng, case["Hkv"]), dm.spread_scales(rng, case["Hkv"])
    k, v = dm.round_to(rng.standard_normal(shape), fmt), dm.round_to(rng.standard_normal(shape), fmt)
    return quantise_e4m3(k / ks[None, :, None, None]), quantise_e4m3(v / vs[None, :, None, None]), ks, vs


def old_queries(case, fmt, seed):
    rng = np.random.default_rng(seed + 1)
    shape = (case["B"], case["G"] * case["Hkv"], case["R"], case["D"])
    return dm.round_to(rng.uniform(-1, 1, shape) if case["family"] == "u16" else rng.standard_normal(shape), fmt)


_PROBLEMS = {}


def problem(case, fmt="bf16", needles=True):
    """(q, k, v, lens, keyword arguments of model(), info, the unmutated Reference), cached"""
    key = (case_id(case), fmt, needles)
    if key not in _PROBLEMS:
        if case["pieces"] and not HAVE_LIBRARY:
            pytest.skip("split cases need mfa_attention_decode_piece_range: the library is not built")
        seed = CASES.index(case)
        k, v, ks, vs = cache_values(case, fmt, seed)
        lens = np.full(case["B"], case["n"])
        Hq = case["G"] * case["Hkv"]
        geo = dict(pieces=case["pieces"], page=case["page"], kscale=ks, vscale=vs)
        if needles:
            keff = k if ks is None else k * ks.astype(np.float64)[None, :, None, None]
            q, info = dm.needle_queries(keff, lens, Hq, case["G"], case["R"], case["causal"], fmt, pieces=case["pieces"], page=case["page"])
        else:
            q, info = old_queries(case, fmt, seed), None
        ref = dm.model(q, k, v, lens, case["G"], case["causal"], **geo)
        _PROBLEMS[key] = (q, k, v, lens, geo, info, ref)
    return _PROBLEMS[key]


# ------------------------------------------------------------------------------------------------------------------------- (a)
def emulated_ratios(case, fmt):
    """worst err / bound at margin 1 of the emulated reference: {out: (O ratio, L ratio)}"""
    q, k, v, lens, geo, info, ref = problem(case, fmt)
    eo, el = dm.emulated(q, k, v, lens, case["G"], case["causal"], fmt, pieces=geo["pieces"], kscale=geo["kscale"], vscale=geo["vscale"])
    return {out: dm.compare(dm.store(eo, out), el, ref, fmt, out, lens, margin=1, info=info, pieces=geo["pieces"], page=geo["page"])
            for out in (fmt, "f32")}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_rounding_emulated_reference_is_inside_the_bounds(case):
    for fmt in ("bf16", "f16"):
        for out, (ro, rl, text) in emulated_ratios(case, fmt).items():
            print("%s %s O %s: emulated reference at margin 1: O %.3f, L %.3f of the bound" % (case_id(case), fmt, out, ro, rl))
            assert ro <= dm.MARGIN / 2.0 and rl <= dm.MARGIN / 2.0, (fmt, out, text)   # 2 x headroom under the committed margin
    _q, _k, _v, _lens, _geo, _info, ref = problem(case, "bf16")
    assert float(np.abs(ref.O).max()) >= 0.05, "the needle inputs must keep O of the order of V"


def test_the_margin_is_a_power_of_two_and_at_most_four():
    assert dm.MARGIN in (1, 2, 4)


# ------------------------------------------------------------------------------------------------------------------------- (b)
_FLAGGED = {}


def flagged(case, mutant, needles=True, old_bounds=False):
    """None where the mutant computes the model's own values; else whether the check sees it (new: per element; old: the maxima)"""
    key = (case_id(case), mutant, needles, old_bounds)
    if key not in _FLAGGED:
        _FLAGGED[key] = _flagged(case, mutant, needles, old_bounds)
    return _FLAGGED[key]


def _flagged(case, mutant, needles, old_bounds):
    q, k, v, lens, geo, info, ref = problem(case, "bf16", needles)
    with np.errstate(all="ignore"):
        bad = dm.model(q, k, v, lens, case["G"], case["causal"], mutant, **geo)
    same_o = np.array_equal(bad.O, ref.O)
    same_l = np.array_equal(bad.L, ref.L)
    if same_o and same_l:
        return None
    if old_bounds:
        keep = np.isfinite(ref.L) & np.isfinite(bad.L)
        err_l = float(np.abs(bad.L[keep] - ref.L[keep]).max()) if keep.any() else 0.0
        lost = bool((np.isfinite(ref.L) != np.isfinite(bad.L)).any())
        return float(np.abs(bad.O - ref.O).max()) > dm.OLD_TOL_O or err_l > dm.OLD_TOL_L or lost
    gl = np.where(np.isfinite(bad.L), bad.L, -1e38)
    ro, rl, _text = dm.compare(bad.O, gl, ref, "bf16", "bf16", lens, info=info, pieces=geo["pieces"], page=geo["page"])
    return ro > 1.0 or rl > 1.0


@pytest.mark.parametrize("mutant", sorted(dm.MUTANTS))
def test_each_mutant_is_flagged_wherever_it_changes_anything(mutant):
    _what, noop = dm.MUTANTS[mutant]
    exercised, missed = 0, []
    for case in CASES:
        if case["pieces"] and not HAVE_LIBRARY:
            continue
        if noop(case):
            if case["n"] <= 600:   # the named no-op cases are no-ops
                assert flagged(case, mutant) is None, (mutant, case_id(case))
            continue
        seen = flagged(case, mutant)
        assert seen is not None, "%s changes nothing on %s, which it does not name" % (mutant, case_id(case))
        exercised += 1
        if not seen:
            missed.append(case_id(case))
    assert exercised >= 1, "%s is exercised by no case" % mutant
    assert not missed, "%s goes unnoticed on %d of %d cases: %s" % (mutant, len(missed), exercised, missed)


# ------------------------------------------------------------------------------------------------------------------------- (c)
def regression_table(needles):
    """{mutant: {n: [case ids on which it changes the result and the check does not see it]}}"""
    table = {}
    for mutant in sorted(dm.MUTANTS):
        noop = dm.MUTANTS[mutant][1]
        for case in CASES:
            if noop(case) or (case["pieces"] and not HAVE_LIBRARY):
                continue
            if flagged(case, mutant, needles=needles, old_bounds=not needles) is False:
                table.setdefault(mutant, {}).setdefault(case["n"], []).append(case_id(case))
    return table


# what the former inputs under the former bounds are known to miss (a subset of the table the script prints: the issue's findings)
FORMERLY_MISSED = {"o_zero": (32768,), "key0_dropped": (4096, 32768), "len_minus_2": (4096, 32768), "causal_minus_1": (4096, 32768),
                   "causal_plus_1": (4096,), "v_rows_exchanged": (600, 4096, 32768), "v_dblocks_exchanged": (32768,),
                   "wave_last_step_dropped": (32768,), "page_off_by_one": (4096, 32768)}


@pytest.mark.skipif(not HAVE_LIBRARY, reason="the table covers the split cases: needs the library")
def test_the_former_inputs_and_bounds_missed_what_the_new_ones_flag():
    old = regression_table(needles=False)
    for mutant, lengths in FORMERLY_MISSED.items():
        for n in lengths:
            assert old.get(mutant, {}).get(n), "%s at %d keys was expected to pass the former check unnoticed" % (mutant, n)
    assert regression_table(needles=True) == {}


# ------------------------------------------------------------------------------------------------------------------------- (d)
def test_the_gpu_files_use_the_proven_bound():
    pytest.importorskip("torch")
    import decode_kit
    import test_decode_gpu
    import test_kvcache_gpu
    for module in (test_decode_gpu, test_kvcache_gpu, decode_kit):   # (decode_kit: the runners and the model check both files share)
        assert module.decode_model is dm
        assert module.MARGIN is dm.MARGIN and module.bounds is dm.bounds and module.compare is dm.compare, module.__name__
        source = open(module.__file__).read()
        for own in ("MARGIN =", "def bounds", "def compare", "margin="):
            assert own not in source, "%s must not define or pass its own %r" % (module.__name__, own)
    assert test_decode_gpu.model is dm.model and decode_kit.model is dm.model and test_kvcache_gpu.dk is decode_kit


def test_needles_cover_the_geometry_of_the_long_case():
    if not HAVE_LIBRARY:
        pytest.skip("needs mfa_attention_decode_piece_range")
    n, pieces, Hq, G = 32768, 64, 64, 8
    k = np.random.default_rng(0).uniform(-1, 1, (1, Hq // G, n, 8))
    _q, info = dm.needle_queries(k, [n], Hq, G, 1, True, "bf16", pieces=pieces)
    keys = dm.needle_keys(info)[0]
    for i in range(pieces):
        b, e = dm.library_piece_range(n, pieces, i)
        assert b in keys and e - 1 in keys, (i, b, e)
    assert {0, 31, 32, n - 1, n - 2} <= keys
    sets = [frozenset(info[(0, h, 0)][0]) for h in range(G)]
    assert len(set(sets)) == G, "the heads of one packed group must get different needle sets"


if __name__ == "__main__":
    import __graft_entry__ as entry
    entry.build()
    HAVE_LIBRARY = _library()
    old, new = regression_table(False), regression_table(True)
    print("| mutant | " + " | ".join("%d keys" % n for n in LENGTHS) + " | with needles and per-element bounds |")
    print("|---|" + "---|" * (len(LENGTHS) + 1))
    for mutant in sorted(dm.MUTANTS):
        cells = []
        for n in LENGTHS:
            live = [c for c in CASES if c["n"] == n and not dm.MUTANTS[mutant][1](c)]
            miss = len(old.get(mutant, {}).get(n, []))
            cells.append("-" if not live else "caught" if not miss else "**missed** %d/%d" % (miss, len(live)))
        print("| %s | %s | %s |" % (mutant, " | ".join(cells), "caught" if mutant not in new else "MISSED %s" % new[mutant]))
