"""What tests/test_gemm_exact_gpu.py can see, held on the CPU (tests/gemm_model.py): every case of the plan meets the conditions of
the exactness premise, the plan covers what it says it covers, every mutant is caught -- bit for bit -- by every case that claims
it, and mfa_gemm_kernel_launch_form (no launch, fake pointers) flips on each term of the launch decision."""
import os
import sys
from collections import defaultdict

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import gemm_model as gm  # noqa: E402

ITEMS = gm.items()
ITEM_IDS = [i[0] for i in ITEMS]


# ---------------------------------------------------------------- rounding rules and compare -------------------------------
def test_store_rounding_rules_to_the_bit():
    # BF16 truncation against round-to-nearest: 257 = 0x43808000 sits exactly between 256 and 258
    assert gm.to_bits([257, 259, -259, 255], gm.BF16).tolist() == [0x4380, 0x4381, 0xC381, 0x437F]
    assert gm.to_bits([257, 259, -259, 255], gm.BF16, "rne").tolist() == [0x4380, 0x4382, 0xC382, 0x437F]
    # FP16 holds odd integers up to 2047; 2049 and 2051 are ties (to even: down, up), 4099 rounds up past a tie
    want = np.array([2047, 2048, 2052, 4100, -2052], np.float16).view(np.uint16).tolist()
    assert gm.to_bits([2047, 2049, 2051, 4099, -2051], gm.FP16).tolist() == want
    trunc = np.array([2047, 2048, 2050, 4096, -2050], np.float16).view(np.uint16).tolist()
    assert gm.to_bits([2047, 2049, 2051, 4099, -2051], gm.FP16, "trunc").tolist() == trunc
    assert gm.to_bits([16777215, -3], gm.FP32).view(np.float32).tolist() == [16777215.0, -3.0]
    for prec in (gm.FP32, gm.FP16, gm.BF16):
        v = gm.from_bits(np.array([gm.QUIET_NAN[prec]], gm.STORE_DTYPE[prec]), prec)
        assert np.isnan(v).all()
        canary = gm.from_bits(gm.c_canary(70000, prec), prec)
        assert np.isfinite(canary).all() and (canary != 0).all()
        assert (np.diff(gm.c_canary(70000, prec).astype(np.int64)) != 0).all()


def test_compare_reports_the_first_mismatch_and_every_canary():
    case = next(c for c in gm.plan() if c.kind == "batch" and c.precC == gm.FP32 and not c.load)
    d = gm.build(case)
    assert gm.compare(d.want, d) is None
    got = d.want.copy()
    at = 2 * case.bs[2] + 5 * case.ld[2] + 7
    got[at] ^= 1                                               # one bit of one logical element
    assert "element (batch 2, m 5, n 7)" in gm.compare(got, d)
    got = d.want.copy()
    got[case.bs[2] - 1] ^= 1                                   # a canary in the gap between entries 0 and 1
    assert "canary" in gm.compare(got, d)
    got = d.want.copy()
    got[3 * case.ld[2] + case.N] ^= 1                          # a canary in the row pitch
    assert "canary (batch 0, m 3, n %d)" % case.N in gm.compare(got, d)
    got = d.want.copy()
    got[-1] ^= 1                                               # the last element of the tail
    assert "canary" in gm.compare(got, d)
    got = d.want.copy()
    got[0] = gm.QUIET_NAN[gm.FP32]
    assert "NaN stored" in gm.compare(got, d)


# ---------------------------------------------------------------- the plan's coverage --------------------------------------
def test_plan_items_and_size():
    assert len(ITEMS) == 40 and len(set(ITEM_IDS)) == 40
    cases = gm.plan()
    assert {c.item for c in cases} == set(ITEM_IDS)
    assert len({c.name for c in cases}) == len(cases)
    for item in ITEM_IDS:
        assert 40 <= len(gm.cases_of(item)) <= 80
    assert {(c.precA, c.precB) for c in cases if gm.form_of(c) == "f32"} == set(gm.F32_PAIRS)
    for form in gm.FORMS:
        assert {(c.tA, c.tB) for c in cases if gm.form_of(c) == form} == set(gm.TRANSPOSES), form
        if form != "f32":
            assert {c.precA for c in cases if gm.form_of(c) == form} == {gm.FP16, gm.BF16}, form


@pytest.mark.parametrize("item", ITEMS, ids=ITEM_IDS)
def test_every_item_covers_its_form(item):
    name, form, pa, pb, tA, tB = item
    cases = gm.cases_of(name)
    big = form in ("g16_256", "g16_256_dma")
    block = 256 if big else 128
    own = [c for c in cases if gm.form_of(c) == form]          # the launches that run the item's own form
    assert all(c.big == big and (c.precA, c.precB, c.tA, c.tB) == (pa, pb, tA, tB) for c in cases)
    two = [c for c in own if c.kind == "shape" and c.two_block]
    # an edge in every position: 2 x 2 workgroups, the second block holds one full 32-row tile plus 1 row, and 7 columns
    assert {(c.M, c.N) for c in two} == {(block + 33, block + 7)}
    assert {(c.M, c.N) for c in cases if c.kind == "shape"} == {(block + 33, block + 7), (1, 1), (33, 70)}
    # every (C type, loadPreviousC) pair on the two-block shape, and every K of the form's list
    assert {(c.precC, c.load) for c in two} == set(gm.C_PAIRS)
    ks = {k for k in gm.K_LIST if k % 8 == 0} if form == "g16_256_dma" else set(gm.K_LIST)
    assert {c.K for c in two} == ks
    for shape in ((1, 1), (33, 70)):
        assert {c.K for c in own if c.kind == "shape" and (c.M, c.N) == shape} == ks
    # both kinds of leading dimension; an odd one never runs the DMA object
    assert {c.ldkind for c in cases if c.kind == "shape"} == ({"a8", "odd"} if form == "g16_256" else {"a16", "odd"})
    for c in cases:
        assert all(l >= t for l, t in zip(c.ld, (c.colsA, c.colsB, c.N)))
        if c.ldkind == "odd":
            assert c.ld[0] % 2 == (c.colsA + 1) % 2 and "_dma" not in gm.expected_form(c)
            assert c.ld == (c.colsA + 1, c.colsB + 3, c.N + 5)
        if c.ldkind == "a16":
            assert all(l % 8 == 0 and l - t < 8 for l, t in zip(c.ld, (c.colsA, c.colsB, c.N)))
    if form == "g16_256_dma":
        assert all(gm.form_of(c) == "g16_256_dma" for c in cases if c.ldkind == "a16" and c.kind in ("shape", "wide"))
        assert all(gm.form_of(c) == "g16_256" for c in cases if c.ldkind == "odd")
    if form == "g16_256":
        assert all(gm.form_of(c) == "g16_256" for c in cases)
    # batch: 3 distinct entries on the two-block shape at K = 136
    batch = [c for c in cases if c.kind == "batch"]
    assert len(batch) == 4 and all(c.batch == 3 and c.K == 136 and c.two_block for c in batch)
    padded, odd, shared, tight = batch
    assert all(s % 8 == 0 for s in padded.bs[:2]) and padded.bs[0] > padded.rowsA * padded.ld[0] and padded.bs[1] > padded.rowsB * padded.ld[1]
    assert odd.bs == (padded.bs[0] + 1, padded.bs[1], padded.bs[2]) and odd.bs[0] % 2 == 1
    assert shared.bs == (padded.bs[0], 0, padded.bs[2])
    assert tight.bs[:2] == (tight.rowsA * tight.ld[0], tight.rowsB * tight.ld[1])
    assert all(c.bs[2] >= c.M * c.ld[2] + 40 for c in batch)   # canaries between the entries of C
    if form == "g16_256_dma":
        assert [gm.form_of(c) for c in batch] == ["g16_256_dma", "g16_256", "g16_256_dma", "g16_256_dma"]
    for c in batch:
        d = gm.build(c)
        assert not np.array_equal(d.a[0], d.a[1]) and not np.array_equal(d.a[1], d.a[2]) and not np.array_equal(d.prev[0], d.prev[2])
        assert d.b.shape[0] == (1 if c.bs[1] == 0 else 3)
    # misaligned base: register-staged
    base = [c for c in cases if c.kind == "base"]
    assert len(base) == 1 and base[0].offA == 1 and base[0].two_block and "_dma" not in gm.expected_form(base[0])
    # wide fills at K = 72 and K = 200 on the two-block shape, in the item's own form
    wide = [c for c in cases if c.kind == "wide"]
    assert [c.K for c in wide] == [72, 200] and all(c.two_block and gm.form_of(c) == form for c in wide)
    assert {c.fill for c in wide} == {gm._wide_fill(pa, pb)}
    assert {c.precC for c in wide} == {gm.FP32, gm.BF16}


def test_every_form_claims_every_mutant_it_can_show():
    claimed = defaultdict(set)
    for c in gm.plan():
        claimed[gm.form_of(c)].update(gm.applicable(c))
    for form in gm.FORMS:
        missing = set(gm.MUTANTS) - claimed[form]
        assert missing == ({"straddling_chunk_poisons_last_row"} if form == "f32" else set()), (form, missing)
    # the claims are rules, not samples
    for c in gm.plan():
        names = set(gm.applicable(c))
        assert ("drop_last_k" in names) == (c.K >= 1)
        assert ("stale_b_tile" in names) == (c.K > 128) and ("stale_a_last_tile" in names) == (c.K > 64)
        assert {"extra_k", "row_m_stored"} <= names
        if c.two_block and c.K >= 63:
            assert ("bf16_store_rne" in names) == (c.precC == gm.BF16) and ("f16_store_trunc" in names) == (c.precC == gm.FP16)
        assert ("batch0_a" in names) == ("c_stride_one_row" in names) == (c.batch > 1)
        assert ("skip_prev_last_column" in names) == c.load
        if c.two_block:
            assert ("skip_prev_second_block" in names) == c.load
        if c.kind == "wide" and c.fill != "wide_bf16" and not (c.fill == "wide_mixed" and c.precA == gm.BF16):
            assert "operands_via_bf16" in names


# ---------------------------------------------------------------- fills and mutants, every case -----------------------------
@pytest.mark.parametrize("item", ITEM_IDS)
def test_fill_conditions_hold_and_every_claimed_mutant_is_caught(item):
    for case in gm.cases_of(item):
        d = gm.build(case)
        # the premise's conditions, asserted (not sampled): S < 2**24, exact operands, finite and in-range reference
        assert gm.fill_conditions(d) == [], case.name
        assert d.S.size == 0 or int(d.S.max()) < gm.LIMIT
        boundA, boundB, boundP, cap = gm.FILLS[case.fill]
        assert case.K <= cap and case.K * boundA(case.precA) * boundB + boundP < gm.LIMIT
        if d.a.size:
            assert np.abs(d.a).max() <= boundA(case.precA) < 2 ** gm.SIGNIFICAND_BITS[case.precA]
            assert np.abs(d.b).max() <= boundB < 2 ** gm.SIGNIFICAND_BITS[case.precB]
        if case.precC == gm.FP16:
            assert case.fill == "mid" and np.abs(d.acc + (d.prev if case.load else 0)).max() < gm.FP16_MAX
        # padding: NaN everywhere outside A and B, and the reference leaves every canary of C as it was
        for buf, prec, n in ((d.A, case.precA, case.batch * case.M * case.K), (d.B, case.precB, d.b.size)):
            assert int(np.isnan(gm.from_bits(buf, prec)).sum()) == buf.size - n >= 24
        inside = np.zeros(d.C0.size, bool)
        inside[gm._index(case.batch, case.M, case.N, case.ld[2], case.bs[2])] = True
        assert np.array_equal(d.want[~inside], d.C0[~inside]) and int((~inside).sum()) >= 24
        assert np.array_equal(d.want[inside].reshape(d.acc.shape), gm.reference(d))
        if case.K == 0:
            assert np.array_equal(gm.from_bits(gm.reference(d), case.precC), d.prev if case.load else np.zeros(d.acc.shape))
        assert gm.compare(d.want, d) is None
        for name in gm.applicable(case):
            report = gm.compare(gm.MUTANTS[name][1](d), d)
            assert report is not None, f"{case.name} claims {name} and misses it"


def test_small_fill_separates_the_two_bf16_roundings_in_thousands_of_elements():
    case = next(c for c in gm.plan() if c.kind == "shape" and c.two_block and c.K == 200 and c.precC == gm.BF16 and not c.load
                and c.M == 289)
    d = gm.build(case)
    odd_above = (np.abs(d.acc) > 255) & (d.acc % 2 != 0)
    assert odd_above.mean() > 0.15
    assert int((gm.m_bf16_store_rne(d) != d.want).sum()) > 2000


# ---------------------------------------------------------------- the launch decision, through the C ABI --------------------
def _kernel(pa, pb, pc=gm.FP32, transpose=(False, False), big=False):
    from metal_flash_attention_amd import GEMMDescriptor, GEMMKernel, GEMMKernelDescriptor, GEMMOperandPrecision as P
    d = GEMMDescriptor()
    d.matrixDimensions = (64, 64, 64)
    d.memoryPrecisions = (P(pa), P(pb), P(pc))
    d.transposeState = transpose
    kd = GEMMKernelDescriptor(descriptor=d)
    if big:
        kd.blockDimensions = (256, 256, 64)
    return GEMMKernel(kd), d


def _form(kernel, d, M=64, N=64, K=64, ld=None, batch=1, bs=None, ptrs=(0x10000, 0x20000, 0x30000)):
    d.matrixDimensions, d.leadingDimensions, d.batchDimension = (M, N, K), ld, batch
    return kernel.launch_form(*ptrs, descriptor=d, batchStrides=bs)


@pytest.mark.parametrize("prec", [gm.FP16, gm.BF16])
@pytest.mark.parametrize("transpose", gm.TRANSPOSES)
def test_launch_form_flips_on_each_term_of_the_predicate(prec, transpose):
    tA, tB = transpose
    images = ("_axm" if tA else "_akm") + ("_bkm" if tB else "_bxm")
    t = gm.PREC_NAME[prec]
    dma, reg, small = (f"gemm_16_{t}_256x256x64_w2x4_dma{images}", f"gemm_16_{t}_256x256x64_w2x4{images}",
                       f"gemm_16_{t}_128x128x64_w2x2{images}")
    k, d = _kernel(prec, prec, transpose=transpose, big=True)
    assert k.variant == f"gemm_16_{t}_256x256x64_w2x4" and k.blockDimensions == (256, 256, 64)
    assert _form(k, d) == dma
    assert _form(k, d, K=0) == dma and _form(k, d, K=8) == dma
    for K in (1, 9, 63, 65, 68):                                                       # K % 8
        assert _form(k, d, K=K, ld=(72, 72, 64)) == reg
    for ld in ((72, 72, 64), (80, 64, 64), (64, 80, 67)):                              # whole chunks; C's pitch is free
        assert _form(k, d, ld=ld) == dma
    for ld in ((65, 64, 64), (68, 64, 64), (64, 65, 64), (64, 68, 64), (71, 71, 64)):  # each leading dimension % 8
        assert _form(k, d, ld=ld) == reg
    assert _form(k, d, batch=3, bs=(4096, 4096, 4099)) == dma and _form(k, d, batch=3, bs=(4096, 0, 4096)) == dma
    for bs in ((4097, 4096, 4096), (4100, 4096, 4096), (4096, 4097, 4096), (4096, 4100, 4096)):   # each batch stride % 8
        assert _form(k, d, batch=3, bs=bs) == reg
    for ptrs in ((0x10002, 0x20000, 0x30000), (0x10008, 0x20000, 0x30000), (0x10000, 0x20002, 0x30000), (0x10000, 0x20008, 0x30000)):
        assert _form(k, d, ptrs=ptrs) == reg                                           # each base pointer % 16
    assert _form(k, d, ptrs=(0x10010, 0x20030, 0x30002)) == dma                        # C's alignment is free
    # the small block never stages through DMA
    ks, ds = _kernel(prec, prec, transpose=transpose, big=False)
    assert _form(ks, ds) == small and _form(ks, ds, K=9, ld=(73, 75, 69)) == small
    # operands of 4 GiB or more: 32-bit buffer offsets cannot cover them, the general kernel runs -- whatever the block
    huge = dict(M=1 << 21, N=64, K=1024) if not tA else dict(M=1024, N=64, K=1 << 21)
    assert _form(k, d, **huge) == "gemm_f32mfma_128x128x16_w2x2" == _form(ks, ds, **huge)
    hugeB = dict(M=64, N=1 << 21, K=1024) if tB else dict(M=64, N=1024, K=1 << 21)
    assert _form(k, d, **hugeB) == "gemm_f32mfma_128x128x16_w2x2"
    just = dict(M=(1 << 21) - 8, N=64, K=1024) if not tA else dict(M=1024, N=64, K=(1 << 21) - 8)
    assert _form(k, d, **just) == dma


def test_launch_form_of_the_general_kernel_and_refusals():
    from metal_flash_attention_amd import MFAError
    for pa, pb in gm.F32_PAIRS:
        k, d = _kernel(pa, pb, big=True)                       # a block request does not turn a mixed pair into gemm_16
        assert _form(k, d) == "gemm_f32mfma_128x128x16_w2x2" == k.variant
        assert _form(k, d, K=9, ld=(11, 67, 69), ptrs=(0x10002, 0x20002, 0x30002)) == "gemm_f32mfma_128x128x16_w2x2"
    k, d = _kernel(gm.BF16, gm.BF16)
    with pytest.raises(MFAError, match="too small"):
        _form(k, d, ld=(8, 64, 64))
    with pytest.raises(MFAError, match="null operand"):
        _form(k, d, ptrs=(0, 0x20000, 0x30000))
    with pytest.raises(MFAError, match="positive"):
        _form(k, d, M=0)


@pytest.mark.parametrize("item", ITEM_IDS)
def test_library_and_model_agree_on_the_form_of_every_planned_launch(item):
    """The model's restated predicate (what the GPU test asserts per launch) against the library's, on the plan's own arguments."""
    kernels = {}
    for case in gm.cases_of(item):
        key = (case.precC, case.big)
        if key not in kernels:
            kernels[key] = _kernel(case.precA, case.precB, case.precC, (case.tA, case.tB), case.big)
        k, d = kernels[key]
        base = 0x7F0000000000
        ptrs = (base + case.offA * gm.ELEM_SIZE[case.precA], base + (1 << 30), base + (2 << 30))
        got = _form(k, d, case.M, case.N, case.K, case.ld, case.batch, case.bs if case.batch > 1 else None, ptrs)
        assert got == gm.expected_form(case), case.name
