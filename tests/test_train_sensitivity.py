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

Block masks (MASKED: eight more cases of (a) and (b)): (513, 1030) -- three row blocks of the mask, the last of one row, nine column
blocks, the last of six keys -- shared, per head and per batch entry, causal (and (600, 600)), with per-batch lengths, with an empty
last row block (dead rows), and (257, 4224) at D = 128: two mask words, bits b and b + 32 opposite, codes that repeat every 4096
keys.  The 18 mutants of train_model.MASK_MUTANTS misread the mask (a word, a stride, a bit, a run's edge key, the causal rule or the
key length inside a run, the list of row blocks, a dead row); each is exercised by at least two cases and flagged under bf16 mixed on
every case on which it changes anything, with no exception.  The former mutants run on the masked cases too: where a defect drops
keys or rows no live row sees, it changes nothing (train_model._seen).  test_needles_cover_the_geometry_of_a_mask: every run edge of
every row block has a needle on its visible and a trap on its hidden side.

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


def masked_cases():
    """block-masked cases (256 x 128 blocks): (513, 1030) has three row blocks, the last of one row, and nine column blocks, the last
    of six keys; (257, 4224) at D = 128 has 33 column blocks -- two mask words -- and codes that repeat every 4096 keys, so that key j
    of block 0 and key j + 4096 of block 32, whose bits are opposite, score alike.  Shared and per-head / per-batch masks (pairwise
    different), causal, per-batch lengths (a key length inside an active block), an empty last row block (dead rows)."""
    nm = tm.needle_mask
    out = []

    def add(name, R, C, D, B, H, mask, causal=False, rl=None, cl=None):
        c = dict(R=R, C=C, D=D, B=B, H=H, causal=causal, lengths=rl is not None, pieces=False, spike=False, rl=rl, cl=cl, mask_name=name,
                 block_mask=np.asarray(mask, dtype=bool))
        c.update(tm.case_flags(R, C, rl, cl))
        out.append(c)

    add("shared", 513, 1030, 64, 1, 2, nm(513, 1030, 1))
    grid = np.array([[nm(513, 1030, 10 + 4 * b + h, empty_last=(b, h) == (1, 3)) for h in range(4)] for b in range(2)])
    add("per-head-per-batch", 513, 1030, 128, 2, 4, grid)
    add("shared", 513, 1030, 64, 1, 2, nm(513, 1030, 2, causal=True), causal=True)
    add("shared", 600, 600, 128, 1, 1, nm(600, 600, 3, causal=True), causal=True)
    add("shared", 513, 1030, 64, 2, 1, nm(513, 1030, 4, need_blocks=(6, 8)), rl=[513, 383], cl=[1030, 821])      # key 821: inside block 6
    add("per-head-empty-last", 513, 1030, 128, 1, 2, np.array([[nm(513, 1030, 20 + h, empty_last=True) for h in range(2)]]))
    add("per-head-two-words", 257, 4224, 128, 1, 2, np.array([[nm(257, 4224, 30 + h) for h in range(2)]]))
    # (entry 0: block 0 active in the 256-row block, so that its rows hold needles among keys 0 .. 127)
    two = np.array([[next(m for m in (nm(257, 4224, s) for s in range(40, 140)) if m[0, 0])], [nm(257, 4224, 41)]])
    two[1, 0, 0, 32], two[1, 0, 0, 0] = True, False                                                             # key length 4100: inside block 32
    add("per-batch-two-words", 257, 4224, 128, 2, 1, two, rl=[257, 200], cl=[4224, 4100])
    for c in out:
        m = c["block_mask"].reshape((-1,) + c["block_mask"].shape[-2:])
        assert len({x.tobytes() for x in m}) == len(m), "the masks of one grid are pairwise different"
    return out


CASES, EMULATED_ONLY = cases()
MASKED = masked_cases()
case_id = lambda c: "%dx%dx%d-%s-%s-%s%s%s" % (c["R"], c["C"], c["D"], "causal" if c["causal"] else "dense", "lengths" if c["lengths"] else "full",  # noqa: E731
                                               "split" if c["pieces"] else "unsplit", "-spike" if c["spike"] else "",
                                               "-mask-" + c["mask_name"] if c.get("mask_name") else "")
_IDS = [case_id(c) for c in CASES + EMULATED_ONLY + MASKED]
assert len(set(_IDS)) == len(_IDS)

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
        if case.get("block_mask") is not None:
            geo["block_mask"] = case["block_mask"]
        q, k, v, dO, info = tm.needle_inputs(case["B"], case["H"], case["R"], case["C"], case["D"], fmt, spike=case["spike"],
                                             seed=_IDS.index(case_id(case)), **geo)
        _PROBLEMS[key] = (q, k, v, dO, geo, info, tm.model(q, k, v, dO, fmt=fmt, mixed=mixed, **geo))
    return _PROBLEMS[key]


# ------------------------------------------------------------------------------------------------------------------------- (a)
def emulated_ratios(case, fmt, mixed):
    q, k, v, dO, geo, info, ref = problem(case, fmt, mixed)
    got = tm.emulated(q, k, v, dO, fmt, mixed, **geo)
    return tm.compare(got, ref, margin=1, info=info)


@pytest.mark.parametrize("case", CASES + EMULATED_ONLY + MASKED, ids=case_id)
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
        for case in CASES + MASKED:
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
        assert exercised >= (2 if mutant in tm.MASK_MUTANTS else 1), "%s is exercised by %d cases" % (mutant, exercised)
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


# the former checks of block-masked launches: test_block_sparse_mask of tests/test_attention_gpu.py -- N(0, 1) operands, ONE mask shared
# by the grid (drawn as that test draws it: density 0.4, seeded by R + C), one mask word, and these constants on the maximum error
OLD_MASK_TOL = dict(O=1.5e-2, L=1e-3, D=5e-2, dV=2e-2, dK=2e-2, dQ=2e-2)
OLD_MASK_SHAPES = (((600, 900, 64), False, False), ((1024, 1024, 128), True, False), ((700, 1300, 128), False, True), ((520, 1100, 256), False, False))


def old_mask(R, C, empty):
    rng = np.random.default_rng(R + C)
    rb, cb = (R + 255) // 256, (C + 127) // 128
    bits = rng.random((rb, cb)) < 0.4
    for i in range(rb):
        if not bits[i].any() and not (empty and i == rb - 1):
            bits[i, rng.integers(0, cb)] = True
    if empty:
        bits[rb - 1, :] = False
    return bits


def old_mask_check_sees(shape, causal, empty, mutant):
    """None: the mutant changes nothing there; else (seen under OLD_MASK_TOL, {output: maximum absolute error}).  A dead row's L is
    compared where the model's is finite only, as that test does; its O and dQ must be 0 and its L below -1e30"""
    R, C, D = shape
    bits = old_mask(R, C, empty)
    case = dict(R=R, C=C, D=D, H=1, B=1, causal=causal, pieces=False, spike=False, block_mask=bits, rl=None, cl=None, **tm.case_flags(R, C))
    if tm.MUTANTS[mutant][1](case):
        return None
    key = ("old mask", shape, causal, empty)
    if key not in _PROBLEMS:
        q, k, v, dO = network_inputs(*shape)
        _PROBLEMS[key] = (q, k, v, dO, tm.model(q, k, v, dO, causal=causal, block_mask=bits, with_bounds=False))
    q, k, v, dO, ref = _PROBLEMS[key]
    with np.errstate(all="ignore"):
        bad = tm.model(q, k, v, dO, causal=causal, block_mask=bits, mutant=mutant)
        alive = ~ref.dead
        diff = {n: np.abs(getattr(bad, n) - getattr(ref, n)) for n in tm.OUTPUTS}
        diff["L"] = diff["L"][alive]
        err = {n: float(np.max(np.where(np.isnan(x), np.inf, x), initial=0.0)) for n, x in diff.items()}
        dead_ok = (bad.O[ref.dead] == 0).all() and (bad.dQ[ref.dead] == 0).all() and (bad.L[ref.dead] < -1e30).all()
    return (any(not err[n] < OLD_MASK_TOL[n] for n in tm.OUTPUTS) or not dead_ok, err)


def test_what_the_former_mask_check_never_ran():
    """the table the script prints: on its own shapes the former check sees every misreading of a mask it can
    exercise -- N(0, 1) scores at these sizes leave rows in which one key carries much of the weight, and the exact mode's FP32 L at
    1e-3 resolves one key among a few hundred -- but its one shared mask of one
    word exercises neither a second mask word nor a mask stride, and it has no per-batch key length"""
    for mutant in ("mask_word0_for_every_block", "mask_row_stride_one_word", "mask_head0_for_all", "mask_batch0_for_all", "mask_head_is_kv_head",
                   "mask_drops_key_length"):
        assert all(old_mask_check_sees(*shape, mutant) is None for shape in OLD_MASK_SHAPES), "%s was exercised" % mutant
    for mutant in ("run_starts_one_key_late", "run_ends_one_key_early", "run_reads_one_key_past"):
        assert old_mask_check_sees(*OLD_MASK_SHAPES[0], mutant)[0]


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
    import test_train_parity_mask_gpu as masked
    import test_train_parity_transposed_gpu as transposed
    for sibling in (masked, transposed):      # the masked and the transposed cases go through the same runner and define no check
        assert sibling.run_case is gpu.run_case and sibling.case is gpu.case
        text = open(sibling.__file__).read()
        assert not any(own in text for own in ("MARGIN", "margin=", "def bounds", "def compare", "compare(")), sibling.__name__


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


@pytest.mark.parametrize("causal", [False, True], ids=["dense", "causal"])
def test_needles_cover_the_geometry_of_a_mask(causal):
    """under a block mask, over a grid of four heads, with no (row block, run edge) pair left out: every run of active column blocks of
    every row block has its first and its last key as a needle of a row of that row block, and, where an inactive block lies before /
    behind it, that block's last / first key as a trap of a row of that row block; every first and last row of a 256-row block holds,
    in every head, a needle in a column block that is active for its row block and inactive for the adjacent one, and a trap in a block
    with the opposite pattern; needles are keys the row sees, traps keys it does not see; dead rows hold traps only."""
    R, C, D, H = 513, 1030, 64, 4
    bits = tm.needle_mask(R, C, 7, causal=causal)
    _q, _k, _v, _dO, info = tm.needle_inputs(1, H, R, C, D, "bf16", causal=causal, block_mask=bits)
    vis = tm.mask_views(bits, 0, 0, R, C, R, C, causal)[0]
    block = lambda t: t // tm.MASK_COLUMNS    # noqa: E731
    for (b, h, r), (needles, traps) in info.items():
        assert all(vis[r, t] for t in needles) and not any(vis[r, t] for t in traps), (h, r, needles, traps)
        assert len(needles) <= tm.CAPACITY and (len(needles) >= 2 or vis[r].sum() < 2), (h, r, needles)
    nrb = bits.shape[0]
    pairs = 0
    for i in range(nrb):
        rows = range(i * tm.BLOCK_ROWS, min((i + 1) * tm.BLOCK_ROWS, R))
        held = {t for h in range(H) for r in rows for t in info[(0, h, r)][0]}
        trapped = {t for h in range(H) for r in rows for t in info[(0, h, r)][1]}
        for s, e in tm.mask_runs(bits[i]):
            first, last = s * tm.MASK_COLUMNS, min((e + 1) * tm.MASK_COLUMNS, C) - 1
            reach = rows[-1] + C - R if causal else C - 1                           # the frontier of the row block's last row
            for key, hidden in ((first, first - 1 if s > 0 else None), (last, last + 1 if last + 1 < C else None)):
                if key > reach:
                    continue          # causal: no row of the row block sees as far
                pairs += 1
                assert key in held, ("no needle on the visible side", i, (s, e), key)
                if hidden is not None and hidden <= reach:
                    assert hidden in trapped, ("no trap on the hidden side", i, (s, e), hidden)
        for r, j in ((rows[0], i - 1), (rows[-1], i + 1)):
            if not 0 <= j < nrb:
                continue
            for h in range(H):
                needles, traps = info[(0, h, r)]
                seen = [c for c in range(bits.shape[1]) if vis[r, c * tm.MASK_COLUMNS]]
                if any(bits[i, c] and not bits[j, c] for c in seen):
                    assert any(bits[i, block(t)] and not bits[j, block(t)] for t in needles), ("no needle the adjacent row block must not see", h, r)
                if any(bits[j, c] and not bits[i, c] and c * tm.MASK_COLUMNS <= r + (C - R if causal else C) for c in range(bits.shape[1])):
                    assert any(bits[j, block(t)] and not bits[i, block(t)] for t in traps), ("no trap in a block of the adjacent row block", h, r)
    assert pairs >= 2 * nrb


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
    print()
    print("| mask mutant | " + " | ".join("%s %s%s" % (s, "causal" if c else "dense", ", empty last row block" if e else "") for s, c, e in OLD_MASK_SHAPES) + " |")
    print("|---|" + "---|" * len(OLD_MASK_SHAPES))
    for mutant in tm.MASK_MUTANTS:
        cells = []
        for shape, causal, empty in OLD_MASK_SHAPES:
            seen = old_mask_check_sees(shape, causal, empty, mutant)
            if seen is None:
                cells.append("-")
                continue
            worst = max((n for n in tm.OUTPUTS), key=lambda n: (seen[1][n] if np.isfinite(seen[1][n]) else 1e30) / OLD_MASK_TOL[n])
            cells.append("%s (%s %.2g)" % ("caught" if seen[0] else "**missed**", worst, seen[1][worst]))
        print("| %s | %s |" % (mutant, " | ".join(cells)))
