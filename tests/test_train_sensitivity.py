"""CPU test (no GPU call): the checks of tests/test_train_parity_gpu.py can see a wrong key, a wrong row, a wrong D term.

On [B, H] grids of (R, C) = (1, 64), (64, 1), (255, 257), (300, 333), (513, 1030), (600, 600), dense and causal, with and without
per-batch lengths, with and without the library's split plan, at D = 64, 128 and 256, with the needle inputs of tests/train_model.py:

  (a) the rounding-emulated reference (train_model.emulated) is inside the per-element bounds of all six outputs at MARGIN / 2, for
      bf16 and f16 in both modes, and the needle inputs keep O and the gradients of the order of V and dO;
  (b) every named mutant of the model (train_model.MUTANTS) breaks a bound -- or writes padding, or leaves a live element unwritten --
      on every case on which it changes anything, under the widest bound (bf16, mixed mode), is a no-op exactly on the cases its
      predicate names, and is exercised at least once.  No wrong kernel is ever run.  One exception, by arithmetic (BOUND_OF): "dQ
      scaled by 1 - 2^-5" equals margin 2 x four bf16 half-ulps, is invisible under bf16 mixed on all 24 cases on which it changes
      anything, and is held to bf16 exact and f16 mixed instead (flagged on all 24 under both);
  (c) the same mutants under the inputs and tolerances the GPU files had alone before (the oracle Network's N(0, 1) operands;
      harness.TOL_MIXED, and the tighter constants of the test that owns the shape): the table of what went unnoticed, printed by
      `python tests/test_train_sensitivity.py` (it adds (4096, 4096, 128), dense and causal);
  (d) the GPU file takes its bound, margin and checker from train_model.

The 26 cases of (b) are a covering set, not the full product: every shape meets dense and causal, lengths and none; (a) runs both
types and both modes on each and on four more (D = 256 at the two large shapes and under the split plan, the 1024-key split of the
persistent forwards); the (b) cost of the product (288 cases x 36 mutants of float64 attention) buys no geometry the set lacks.
Split cases take their piece counts from mfa_attention_kernel_workspace_size and are skipped without the library.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

import train_model as tm  # noqa: E402

SHAPES = ((1, 64), (64, 1), (255, 257), (300, 333), (513, 1030), (600, 600))
HEAD_DIMENSIONS = (64, 128, 256)


def _library():
    try:
        from metal_flash_attention_amd import _abi
        _abi.lib()
        return True
    except Exception:  # noqa: BLE001 -- not built
        return False


HAVE_LIBRARY = _library()


def cases():
    out, i = [], 0
    for R, C in SHAPES:
        for causal in (False, True):
            if causal and C < R:
                continue                      # the library requires column >= row under the causal mask
            for lengths in (False, True):
                big = R * C > 200000
                D = 64 if big else HEAD_DIMENSIONS[i % 3]
                B, H = ((2, 1) if lengths else (1, 2)) if big else (2, 2)
                out.append(dict(R=R, C=C, D=D, B=B, H=H, causal=causal, lengths=lengths, pieces=False, spike=False))
                i += 1
    for (R, C), D, causal in (((513, 1030), 64, False), ((600, 600), 128, True), ((600, 600), 64, False)):
        out.append(dict(R=R, C=C, D=D, B=1, H=2, causal=causal, lengths=False, pieces=True, spike=False))
    out.append(dict(R=300, C=333, D=128, B=1, H=2, causal=False, lengths=False, pieces=False, spike=True))
    # part (a) only (no mutants: cheap): D = 256 at the two large shapes and under the split plan, which the GPU file runs
    extra = [dict(R=513, C=1030, D=256, B=1, H=2, causal=False, lengths=False, pieces=False, spike=False),
             dict(R=600, C=600, D=256, B=2, H=1, causal=True, lengths=True, pieces=False, spike=False),
             dict(R=513, C=1030, D=256, B=1, H=1, causal=False, lengths=False, pieces=True, spike=False),
             dict(R=513, C=1024, D=128, B=1, H=1, causal=False, lengths=False, pieces=True, spike=False)]
    for c in out + extra:
        c["rl"], c["cl"] = ([c["R"], max(1, c["R"] - c["R"] // 4 - 1)][:c["B"]], [c["C"], max(1, c["C"] - c["C"] // 5 - 3)][:c["B"]]) if c["lengths"] else (None, None)
        if c["lengths"] and c["B"] == 2 and c["R"] == 1:
            c["rl"] = [1, 1]
        c.update(tm.case_flags(c["R"], c["C"], c["rl"], c["cl"]))
    return out, extra


CASES, EMULATED_ONLY = cases()
case_id = lambda c: "%dx%dx%d-%s-%s-%s%s" % (c["R"], c["C"], c["D"], "causal" if c["causal"] else "dense", "lengths" if c["lengths"] else "full",  # noqa: E731
                                             "split" if c["pieces"] else "unsplit", "-spike" if c["spike"] else "")

_PROBLEMS = {}


def problem(case, fmt="bf16", mixed=True):
    """(q, k, v, dO, keyword arguments of model(), info, the unmutated Reference), cached"""
    key = (case_id(case), fmt, mixed)
    if key not in _PROBLEMS:
        pieces = None
        if case["pieces"]:
            if not HAVE_LIBRARY:
                pytest.skip("split cases need the library's plan: the library is not built")
            pieces = tm.library_pieces(case["R"], case["C"], case["D"], case["H"], case["B"], fmt, mixed)
            assert pieces and all(len(pieces[t]) > 1 for t in ("fwd", "dq", "dkv")), (case_id(case), pieces)
        geo = dict(causal=case["causal"], row_lengths=case["rl"], key_lengths=case["cl"], pieces=pieces)
        q, k, v, dO, info = tm.needle_inputs(case["B"], case["H"], case["R"], case["C"], case["D"], fmt, spike=case["spike"],
                                             seed=(CASES + EMULATED_ONLY).index(case), **geo)
        _PROBLEMS[key] = (q, k, v, dO, geo, info, tm.model(q, k, v, dO, fmt=fmt, mixed=mixed, **geo))
    return _PROBLEMS[key]


# ------------------------------------------------------------------------------------------------------------------------- (a)
def emulated_ratios(case, fmt, mixed):
    q, k, v, dO, geo, info, ref = problem(case, fmt, mixed)
    got = tm.emulated(q, k, v, dO, fmt, mixed, **geo)
    return tm.compare(got, ref, margin=1, info=info)


@pytest.mark.parametrize("case", CASES + EMULATED_ONLY, ids=case_id)
def test_the_rounding_emulated_reference_is_inside_the_bounds(case):
    for fmt in ("bf16", "f16"):
        for mixed in (False, True):
            worst, padding, text = emulated_ratios(case, fmt, mixed)
            print("%s %s %s: emulated reference at margin 1: %s" % (case_id(case), fmt, "mixed" if mixed else "exact",
                                                                   " ".join("%s %.3f" % kv for kv in worst.items())))
            assert max(worst.values()) <= tm.MARGIN / 2.0 and all(padding.values()), (fmt, mixed, text)   # 2 x headroom
    ref = problem(case, "bf16", True)[-1]
    assert float(np.nanmax(np.abs(ref.O))) >= 0.05 and float(np.nanmax(np.abs(ref.dV))) >= 0.05, "O and dV must stay of the order of V and dO"
    if case["C"] > 1:     # (one key: P = 1, dS = 0, dQ = dK = 0 exactly)
        assert float(np.nanmax(np.abs(ref.dQ))) >= 0.05 and float(np.nanmax(np.abs(ref.dK))) >= 0.05, "dQ and dK must stay of the order of dO"


def test_the_margin_is_a_power_of_two_and_at_most_four():
    assert tm.MARGIN in (1, 2, 4)


# ------------------------------------------------------------------------------------------------------------------------- (b)
_FLAGGED = {}


def flagged(case, mutant, fmt="bf16", mixed=True):
    """None where the mutant computes the model's own values; else whether compare() sees it under the bound of (fmt, mode)"""
    key = (case_id(case), mutant, fmt, mixed)
    if key not in _FLAGGED:
        q, k, v, dO, geo, info, ref = problem(case, fmt, mixed)
        with np.errstate(all="ignore"):
            bad = tm.model(q, k, v, dO, mutant=mutant, **geo)
        if all(np.array_equal(getattr(bad, n), getattr(ref, n), equal_nan=True) for n in tm.OUTPUTS):
            _FLAGGED[key] = None
        else:
            worst, padding, _text = tm.compare({n: getattr(bad, n) for n in tm.OUTPUTS}, ref, info=info)
            _FLAGGED[key] = max(worst.values()) > 1.0 or not all(padding.values())
    return _FLAGGED[key]


# The widest bound (bf16, mixed mode) for every mutant but one.  "dQ scaled by 1 - 2^-5" is below what that bound can resolve: a dQ
# element carries four half-ulps of bf16 -- P rounded, dS rounded, l summed from the rounded P (through E_L), and a fourth through E_D:
# the forward's rounded P moves D_i = rowsum(dO O) by up to u sum_j |dS_ij| wherever the needles lie -- 4 x 2^-8 of A_dQ >= |dQ|, which
# the margin of 2 makes 2^-5 exactly, before the FP16 L and the truncated D store (2^-7 |D_i|, D_i about 1.4 by the choice of dO) add
# theirs.  (MARGIN cannot be 1: a single rounding
# reaches its bound, the exact mode's emulated dV sits at 0.9 of it.)  That mutant is held to the next two bounds instead -- bf16
# exact (two half-ulps) and f16 mixed -- on every case, and test_what_the_widest_bound_cannot_resolve pins the arithmetic.
BOUND_OF = {"dq_scaled": (("bf16", False), ("f16", True))}


@pytest.mark.parametrize("mutant", sorted(tm.MUTANTS))
def test_each_mutant_is_flagged_wherever_it_changes_anything(mutant):
    _what, noop = tm.MUTANTS[mutant]
    if not HAVE_LIBRARY and noop is tm._no_split:
        pytest.skip("a mutant of the split plan: needs the library")
    for fmt, mixed in BOUND_OF.get(mutant, (("bf16", True),)):
        exercised, missed = 0, []
        for case in CASES:
            if case["pieces"] and not HAVE_LIBRARY:
                continue
            if noop(case):
                if case["R"] * case["C"] <= 200000:   # the named no-op cases are no-ops
                    assert flagged(case, mutant, fmt, mixed) is None, (mutant, case_id(case))
                continue
            seen = flagged(case, mutant, fmt, mixed)
            assert seen is not None, "%s changes nothing on %s, which it does not name" % (mutant, case_id(case))
            exercised += 1
            if not seen:
                missed.append(case_id(case))
        assert exercised >= 1, "%s is exercised by no case" % mutant
        assert not missed, "%s goes unnoticed on %d of %d cases (%s %s): %s" % (mutant, len(missed), exercised, fmt, "mixed" if mixed else "exact", missed)


def test_what_the_widest_bound_cannot_resolve():
    """bf16, mixed mode: on every case the bound of every dQ element is at least 2^-5 |dQ| (see BOUND_OF).  If a tighter derivation
    ever breaks this pin, dq_scaled belongs under the widest bound like every other mutant."""
    assert set(BOUND_OF) == {"dq_scaled"}
    for case in CASES:
        if case["C"] == 1 or (case["pieces"] and not HAVE_LIBRARY) or case["R"] * case["C"] > 200000:
            continue
        ref = problem(case)[-1]
        bd = tm.bounds(ref)["dQ"]
        live = np.broadcast_to(ref.row_live[:, None, :, None], bd.shape)
        assert (bd[live] >= 2.0 ** -5 * np.abs(ref.dQ[live])).all(), case_id(case)
        assert tm.MARGIN * 4 * tm.U_P["bf16"] == 2.0 ** -5


# ------------------------------------------------------------------------------------------------------------------------- (c)
# the present GPU checks: (R, C, D) -> the tighter constants that the test of tests/test_attention_gpu.py that owns the shape asserts
# beside harness.TOL_MIXED.  The first three shapes are test_backward_16bit_mfma's: the constants hold for low_mid = False only, its
# low_mid = True cases (the streams bench.py times) have TOL_MIXED alone; the last is the headline code objects' full-size tests.
_TIGHT = dict(O=1.5e-2, L=1e-3, D=2e-2, dV=2e-2, dK=2e-2, dQ=2e-2)
OLD_SHAPES = {
    (255, 257, 64): _TIGHT,
    (513, 1030, 64): _TIGHT,
    (1024, 1024, 128): _TIGHT,
    (4096, 4096, 128): dict(O=5e-3, D=5e-2, dV=2e-2, dK=2e-2, dQ=2e-2),
}
OLD_MUTANTS = ("o_zero", "key0_dropped", "last_key_dropped", "partial_last_tile_dropped", "tile_skipped_in_one_row_block", "causal_plus_1",
               "causal_minus_1", "wave_groups_exchanged", "v_rows_exchanged", "v_dblocks_exchanged", "l_without_key0", "dq_last_tile_dropped",
               "dq_tile_skipped_in_one_row_block", "dkv_last_step_dropped", "dkv_row_block_dropped", "d_zero", "d_wrong", "d_neighbour_row",
               "l_neighbour_row", "ds_scale_missing", "ds_scale_twice", "dq_scaled", "dk_dv_exchanged", "bwd_causal_plus_1", "bwd_causal_minus_1")


def network_inputs(R, C, D, seed=0):
    """the oracle Network's own N(0, 1) operands, as the bf16 values the device sees (packed by truncation, tests/harness.py)"""
    from oracle import Network, NetworkDescriptor
    net = Network(NetworkDescriptor(R, C, D), seed=seed)
    return tuple(tm.round_to(x, "bf16", trunc=True)[None, None] for x in (net.Q, net.K, net.V, net.dO))


def old_check_errors(shape, causal, mutant):
    """{output: maximum absolute error of the mutant against the model} on the former inputs (one head)"""
    key = ("old", shape, causal)
    if key not in _PROBLEMS:
        q, k, v, dO = network_inputs(*shape)
        _PROBLEMS[key] = (q, k, v, dO, tm.model(q, k, v, dO, causal=causal, with_bounds=False))
    q, k, v, dO, ref = _PROBLEMS[key]
    with np.errstate(all="ignore"):
        bad = tm.model(q, k, v, dO, causal=causal, mutant=mutant)
    return {n: float(np.nanmax(np.abs(getattr(bad, n) - getattr(ref, n)))) for n in tm.OUTPUTS}


def old_check_sees(shape, causal, mutant):
    """None: the mutant changes nothing there; else (seen under TOL_MIXED, seen under the shape's tighter constants or None, errors)"""
    case = dict(R=shape[0], C=shape[1], D=shape[2], H=1, B=1, causal=causal, pieces=False, spike=False, **tm.case_flags(*shape[:2]))
    if tm.MUTANTS[mutant][1](case):
        return None
    err = old_check_errors(shape, causal, mutant)
    if max(err.values()) == 0.0:
        return None
    tight = OLD_SHAPES[shape]
    return (any(err[n] > tm.OLD_TOL[n] for n in tm.OUTPUTS), None if tight is None else any(err[n] > t for n, t in tight.items()) or
            any(err[n] > tm.OLD_TOL[n] for n in tm.OUTPUTS), err)


# what the former inputs under the former bounds are known to miss (a subset of the table the script prints; the 4096 columns are the
# script's alone, for their cost).  (mutant, shape, causal): MISSED by TOL_MIXED and by the shape's tighter constants;
# MISSED_BY_TOL_MIXED: seen by the tighter constants only, so unseen in the mixed mode, whose cases assert TOL_MIXED alone
FORMERLY_MISSED = (
    ("last_key_dropped", (513, 1030, 64), True), ("dq_last_tile_dropped", (255, 257, 64), True), ("dq_scaled", (513, 1030, 64), False),
    ("dq_scaled", (513, 1030, 64), True), ("dq_scaled", (1024, 1024, 128), False),
)
FORMERLY_MISSED_BY_TOL_MIXED = (
    ("d_wrong", (513, 1030, 64), False), ("dkv_row_block_dropped", (513, 1030, 64), False), ("dkv_last_step_dropped", (513, 1030, 64), True),
    ("dq_tile_skipped_in_one_row_block", (513, 1030, 64), False), ("bwd_causal_plus_1", (513, 1030, 64), True),
    ("last_key_dropped", (1024, 1024, 128), True), ("partial_last_tile_dropped", (255, 257, 64), True), ("dq_scaled", (255, 257, 64), False),
)


def test_the_former_inputs_and_bounds_missed_what_the_new_ones_flag():
    for mutant, shape, causal in FORMERLY_MISSED + FORMERLY_MISSED_BY_TOL_MIXED:
        seen = old_check_sees(shape, causal, mutant)
        both = (mutant, shape, causal) in FORMERLY_MISSED
        assert seen is not None and not seen[0] and seen[1] == (not both), "%s at %s %s was expected to pass %s unnoticed: %s" % (
            mutant, shape, "causal" if causal else "dense", "every former check" if both else "TOL_MIXED", seen)


# ------------------------------------------------------------------------------------------------------------------------- (d)
def test_the_gpu_file_uses_the_proven_bound():
    pytest.importorskip("torch")
    import test_train_parity_gpu as gpu
    assert gpu.train_model is tm
    assert gpu.MARGIN is tm.MARGIN and gpu.bounds is tm.bounds and gpu.compare is tm.compare
    source = open(gpu.__file__).read()
    for own in ("MARGIN =", "def bounds", "def compare"):
        assert own not in source, "test_train_parity_gpu must not define its own %r" % own
    assert source.count("margin=") == source.count("margin=1") , "the only margin the GPU file may pass is 1, for the figure it prints"


def test_needles_cover_the_geometry():
    """every key of the pool is some row's needle in every head.  The transposed property: in every head every pool key is held by a
    first and a last row of a 32-row step and of a wave's 64 rows.  The 256-row blocks and the row pieces have three and two edge rows
    for 66 pool keys at twelve needles a row: one head's rows hold at least 22 of the 66, each head 20 keys further on, the four heads
    of the grid all of them.  Heads of one grid get different needle sets."""
    R, C, D, H = 513, 1030, 64, 4
    pieces = {"fwd": tm.split_ranges(C, 4, tm.TILE), "dq": tm.split_ranges(C, 4, tm.TILE), "dkv": tm.split_ranges(R, 2, tm.STEP)}
    _q, _k, _v, _dO, info = tm.needle_inputs(1, H, R, C, D, "bf16", pieces=pieces)
    held = tm.needle_keys(info)
    pool = tm.key_pool(C, pieces)
    assert len(pool) == 66 and {0, C - 1, 63, 64, 31, 32} <= set(pool) and all(pb in pool and pe - 1 in pool for pb, pe in pieces["fwd"])
    classes = tm.edge_rows(R, pieces)
    for name in ("step_first", "step_last", "wave_first", "wave_last", "piece_first", "piece_last", "block_first", "block_last"):
        few = name.startswith(("piece", "block"))
        lacking = [[t for t in pool if not set(held[(0, h)][t]) & set(classes[name])] for h in range(H)]
        for h in range(H):
            assert set(pool) <= set(held[(0, h)]), "every pool key is a needle of some row"
            assert len(lacking[h]) <= (44 if few else 0), (name, h, lacking[h])
        assert not set.intersection(*(set(x) for x in lacking)), (name, "a pool key no head's rows of this class hold")
    assert len({frozenset((t, tuple(rows)) for t, rows in held[(0, h)].items()) for h in range(H)}) == H
    assert max(len(w) for w, _f in info.values()) <= tm.CAPACITY


if __name__ == "__main__":
    import __graft_entry__ as entry
    entry.build()
    print("| mutant | " + " | ".join("%s %s" % (s, "causal" if c else "dense") for s in OLD_SHAPES for c in (False, True)) + " |")
    print("|---|" + "---|" * (2 * len(OLD_SHAPES)))
    for mutant in OLD_MUTANTS:
        cells = []
        for shape in OLD_SHAPES:
            for causal in (False, True):
                seen = old_check_sees(shape, causal, mutant)
                if seen is None:
                    cells.append("-")
                    continue
                worst = max((n for n in tm.OUTPUTS), key=lambda n: seen[2][n] / tm.OLD_TOL[n])
                what = "caught" if seen[0] else "tighter constants only" if seen[1] else "**missed**"
                cells.append("%s (%s %.2g)" % (what, worst, seen[2][worst]))
        print("| %s | %s |" % (mutant, " | ".join(cells)))
