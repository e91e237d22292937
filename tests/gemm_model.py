"""Exact-integer model of the GEMM operator (include/mfa_gemm.h): fills, reference, plan, compare and mutants.  CPU only, numpy only.

The premise: when every operand is an integer that its storage type holds exactly, every product is an exact integer in fp32, and all
three kernels (gemm_f32mfma, gemm_16 register-staged, gemm_16 LDS-DMA) accumulate in fp32.  If
    S[m][n] = sum_k |a[m][k]| |b[k][n]| (+ |prev[m][n]|) < 2**24
every partial sum, in any order and any instruction grouping, is an integer below 2**24, so the accumulator holds the exact integer
sum_k a b (+ prev).  The stored C is then known to the bit: FP32 exact, FP16 round-to-nearest-even, BF16 truncation
(csrc/attn_common.h store_elem).  No tolerance exists anywhere in this module: `compare` is bitwise.

Everything outside a logical matrix is a canary: quiet NaN for A and B (row pitch beyond the row, gaps between batch entries, the
tail, the element in front of a misaligned base), a per-position finite bit pattern for C that must come back unchanged.

`MUTANTS` are numpy re-implementations of the defects tests/test_gemm_exact_gpu.py claims to see, applied to the reference path;
tests/test_gemm_sensitivity.py holds every case of `plan()` to catching every mutant it claims.
"""
from __future__ import annotations

import dataclasses
import functools
import zlib

import numpy as np

FP32, FP16, BF16 = 0, 1, 2          # mfa_precision / GEMMOperandPrecision
PREC_NAME = {FP32: "f32", FP16: "f16", BF16: "bf16"}
STORE_DTYPE = {FP32: np.uint32, FP16: np.uint16, BF16: np.uint16}
ELEM_SIZE = {FP32: 4, FP16: 2, BF16: 2}
QUIET_NAN = {FP32: 0x7FC00000, FP16: 0x7E00, BF16: 0x7FC0}
LIMIT = 2 ** 24                      # integers below it are exact in an fp32 accumulator
FP16_MAX = 65504

FORMS = ("f32", "g16_128", "g16_256", "g16_256_dma")
F32_PAIRS = ((FP32, FP32), (FP16, BF16), (BF16, FP32), (FP32, FP16))    # (A, B) of the general kernel's items
TRANSPOSES = ((False, False), (False, True), (True, False), (True, True))
K_LIST = (0, 1, 8, 9, 63, 64, 65, 72, 128, 136, 200)
C_PAIRS = tuple((c, load) for c in (FP32, FP16, BF16) for load in (False, True))
BATCH_K, BATCH = 136, 3
BASE_ALIGNMENT = 256                 # what the allocator of the GPU test guarantees for a buffer's first byte

# fill -> (bound of |A| by A's type, bound of |B|, bound of |prev|, largest K)
_A_WIDE = {FP32: 4095, FP16: 2047, BF16: 255}
FILLS = {
    "small": (lambda pa: 8, 8, 64, 512),
    "mid": (lambda pa: 31, 31, 1024, 512),
    "wide_bf16": (lambda pa: 255, 255, 64, 256),
    "wide_f16": (lambda pa: 2047, 15, 64, 512),
    "wide_f32": (lambda pa: 4095, 15, 64, 256),
    "wide_mixed": (lambda pa: _A_WIDE[pa], 15, 64, 256),   # the general kernel's mixed pairs: A as wide as its own type holds
}
SIGNIFICAND_BITS = {FP32: 24, FP16: 11, BF16: 8}


@dataclasses.dataclass(frozen=True)
class Case:
    item: str                 # the GPU test item that runs it: "<form>-<type>-<transposes>"
    kind: str                 # "shape" | "batch" | "base" | "wide"
    precA: int
    precB: int
    precC: int
    tA: bool
    tB: bool
    M: int
    N: int
    K: int
    ld: tuple                 # (A, B, C), elements
    load: bool
    big: bool                 # the kernel descriptor asks for the 256 x 256 block
    fill: str
    batch: int = 1
    bs: tuple = (0, 0, 0)     # batch strides, elements
    offA: int = 0             # A starts this many elements into its allocation
    ldkind: str = "a16"

    @property
    def name(self):
        return (f"{self.item}:{self.kind}:{self.M}x{self.N}x{self.K}:{self.ldkind}:C{PREC_NAME[self.precC]}{'+prev' if self.load else ''}"
                f":{self.fill}" + (f":b{self.batch}bs{self.bs}" if self.batch > 1 else "") + (":offA" if self.offA else ""))

    @property
    def rowsA(self):
        return self.K if self.tA else self.M

    @property
    def colsA(self):
        return self.M if self.tA else self.K

    @property
    def rowsB(self):
        return self.N if self.tB else self.K

    @property
    def colsB(self):
        return self.K if self.tB else self.N

    @property
    def block(self):
        return 256 if expected_form(self).startswith("gemm_16") and self.big else 128

    @property
    def two_block(self):
        return self.M > self.block and self.N > self.block


# ---------------------------------------------------------------- the launch decision, restated ------------------------------
def expected_form(case: Case) -> str:
    """The code object mfa_gemm_kernel_launch runs for `case` (csrc/mfa_gemm.hip prepare), restated from its documentation:
    the general kernel unless A and B share one 16-bit type; the 256 x 256 block only on request; LDS-DMA staging only when K,
    both leading dimensions and both batch strides are multiples of 8 elements and A and B start on 16 bytes."""
    if case.precA == FP32 or case.precA != case.precB:
        return "gemm_f32mfma_128x128x16_w2x2"
    images = ("_axm" if case.tA else "_akm") + ("_bkm" if case.tB else "_bxm")
    head = "gemm_16_" + PREC_NAME[case.precA]
    if not case.big:
        return head + "_128x128x64_w2x2" + images
    aligned = (case.K % 8 == 0 and case.ld[0] % 8 == 0 and case.ld[1] % 8 == 0 and case.bs[0] % 8 == 0 and case.bs[1] % 8 == 0
               and (BASE_ALIGNMENT + case.offA * 2) % 16 == 0)
    return head + "_256x256x64_w2x4" + ("_dma" if aligned else "") + images


def form_of(case: Case) -> str:
    name = expected_form(case)
    return "f32" if name.startswith("gemm_f32") else "g16_128" if "128x128" in name else "g16_256_dma" if "_dma" in name else "g16_256"


# ---------------------------------------------------------------- bits ------------------------------------------------------
def to_bits(values, prec, rule=None):
    """Integer (or float64) values -> the storage bits of `prec`.  rule: "rne" | "trunc" (default: the documented store rounding,
    FP16 round-to-nearest-even, BF16 truncation; FP32 holds every value this module produces exactly)."""
    v = np.asarray(values, np.float64)
    if prec == FP32:
        return v.astype(np.float32).view(np.uint32)
    rule = rule or ("rne" if prec == FP16 else "trunc")
    if prec == FP16:
        with np.errstate(over="ignore"):
            h = v.astype(np.float16)                       # numpy narrows with round-to-nearest-even
        if rule == "trunc":                                  # toward zero: step back where rounding went away from zero
            away = np.abs(h.astype(np.float64)) > np.abs(v)
            h = np.where(away, (h.view(np.uint16) - 1).astype(np.uint16).view(np.float16), h)
        return np.ascontiguousarray(h).view(np.uint16)
    u = v.astype(np.float32).view(np.uint32)
    if rule == "rne":
        u = u + 0x7FFF + ((u >> 16) & 1)
    return (u >> 16).astype(np.uint16)


def from_bits(bits, prec):
    bits = np.asarray(bits)
    if prec == FP32:
        return bits.astype(np.uint32).view(np.float32).astype(np.float64)
    if prec == FP16:
        return bits.astype(np.uint16).view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def exactly_representable(ints, prec) -> bool:
    return bool(np.array_equal(from_bits(to_bits(ints, prec, "trunc"), prec), np.asarray(ints, np.float64)))


def c_canary(count, prec):
    """Per-position finite bit patterns of the C buffer (never zero, never an Inf/NaN encoding, neighbours differ)."""
    pos = np.arange(count, dtype=np.uint64)
    if prec == FP32:
        return (0x3F000001 + (pos * 2654435761 & 0x7FFFFF)).astype(np.uint32)       # in [0.5, 1)
    u = ((pos * 40503 + 0x1234) & 0xFFFF).astype(np.uint16)
    mask = np.uint16(0x7C00 if prec == FP16 else 0x7F80)
    u = np.where((u & mask) == mask, u & np.uint16(~0x0400 & 0xFFFF if prec == FP16 else ~0x0080 & 0xFFFF), u)
    return np.where((u & np.uint16(0x7FFF)) == 0, np.uint16(0x3C01), u).astype(np.uint16)


# ---------------------------------------------------------------- data of one case ------------------------------------------
@dataclasses.dataclass
class Data:
    case: Case
    seed: int
    a: np.ndarray            # [batch, M, K] logical integers
    b: np.ndarray            # [batch or 1, K, N]
    prev: np.ndarray         # [batch, M, N]
    A: np.ndarray            # storage bits of the whole allocation (A's logical element (0, 0) sits at index offA)
    B: np.ndarray
    C0: np.ndarray           # C allocation before the launch: prev in the logical elements when loadPreviousC, canaries elsewhere
    acc: np.ndarray          # [batch, M, N] int64 sum_k a b
    S: np.ndarray            # [batch, M, N] sum_k |a| |b| (+ |prev|)
    want: np.ndarray         # C allocation after a correct launch


def _index(batch, rows, cols, ld, bs, off=0):
    z = np.arange(batch, dtype=np.int64)[:, None, None] * bs
    return off + z + np.arange(rows, dtype=np.int64)[None, :, None] * ld + np.arange(cols, dtype=np.int64)[None, None, :]


def _matmul(a, b):
    return np.rint(np.matmul(a.astype(np.float64), b.astype(np.float64))).astype(np.int64)   # exact: every sum is far below 2**53


def _draw(case: Case, seed: int):
    rng = np.random.default_rng(seed)
    boundA, boundB, boundP, _ = FILLS[case.fill]
    ra, rb = boundA(case.precA), boundB
    nb = 1 if (case.batch > 1 and case.bs[1] == 0) else case.batch
    a = rng.integers(-ra, ra + 1, (case.batch, case.M, case.K), dtype=np.int64)
    b = rng.integers(-rb, rb + 1, (nb, case.K, case.N), dtype=np.int64)
    prev = rng.integers(-boundP, boundP + 1, (case.batch, case.M, case.N), dtype=np.int64)
    return a, b, prev


def lengths(case: Case):
    """Elements of the three allocations: every batch entry, then a tail of canaries (two C rows: the store-row-M mutant of the
    last entry lands inside the allocation)."""
    nA = case.offA + (case.batch - 1) * case.bs[0] + case.rowsA * case.ld[0] + case.ld[0] + 24
    nB = (case.batch - 1) * case.bs[1] + case.rowsB * case.ld[1] + case.ld[1] + 24
    nC = (case.batch - 1) * case.bs[2] + case.M * case.ld[2] + 2 * case.ld[2] + 24
    return nA, nB, nC


def _build(case: Case, seed: int) -> Data:
    a, b, prev = _draw(case, seed)
    nA, nB, nC = lengths(case)
    A = np.full(nA, QUIET_NAN[case.precA], STORE_DTYPE[case.precA])
    B = np.full(nB, QUIET_NAN[case.precB], STORE_DTYPE[case.precB])
    ia = _index(case.batch, case.rowsA, case.colsA, case.ld[0], case.bs[0], case.offA)
    A[ia] = to_bits(a.transpose(0, 2, 1) if case.tA else a, case.precA, "trunc")
    ib = _index(b.shape[0], case.rowsB, case.colsB, case.ld[1], case.bs[1])
    B[ib] = to_bits(b.transpose(0, 2, 1) if case.tB else b, case.precB, "trunc")
    C0 = c_canary(nC, case.precC)
    if case.load:
        C0[_index(case.batch, case.M, case.N, case.ld[2], case.bs[2])] = to_bits(prev, case.precC, "trunc")
    acc = _matmul(a, b)
    S = _matmul(np.abs(a), np.abs(b)) + (np.abs(prev) if case.load else 0)
    d = Data(case, seed, a, b, prev, A, B, C0, acc, S, None)
    d.want = simulate(d)
    return d


def fill_conditions(d: Data):
    """The conditions under which the premise holds for this case; a list of the violated ones (empty = fine)."""
    c, bad = d.case, []
    if c.K > FILLS[c.fill][3]:
        bad.append("K above the fill's cap")
    if d.S.size and int(d.S.max()) >= LIMIT:
        bad.append("S >= 2**24")
    if not exactly_representable(d.a, c.precA) or not exactly_representable(d.b, c.precB):
        bad.append("an operand is not exact in its storage type")
    if c.load and not exactly_representable(d.prev, c.precC):
        bad.append("previous C is not exact in C's type")
    total = d.acc + (d.prev if c.load else 0)
    if c.precC == FP16 and int(np.abs(total).max()) >= FP16_MAX:
        bad.append("|ref| leaves the finite range of FP16")
    if not np.isfinite(from_bits(reference(d), c.precC)).all():
        bad.append("|ref| is not finite in C's type")
    return bad


@functools.lru_cache(maxsize=64)
def build(case: Case) -> Data:
    """Data of `case`.  The seed is the first, counting up from a hash of the case's name, at which the fill conditions hold (the
    FP16 range is the one a seed can miss) and -- on shapes of at most 16 elements or sums of fewer than 8 terms, where one zero
    operand element or one rounding step can swallow a defect whole -- every mutant the case claims changes a bit.  All other
    cases are held to the same in tests/test_gemm_sensitivity.py without any search."""
    seed = zlib.crc32(case.name.encode()) & 0xFFFFF
    for attempt in range(200):
        d = _build(case, seed + attempt)
        assert d.S.size == 0 or int(d.S.max()) < LIMIT, (case.name, int(d.S.max()))
        if fill_conditions(d):
            continue
        if (case.M * case.N > 16 and case.K >= 8) or all(compare(MUTANTS[m][1](d), d) is not None for m in applicable(case)):
            return d
    raise AssertionError(f"no seed in 200 meets the conditions of {case.name}")


# ---------------------------------------------------------------- reference and mutants ------------------------------------
def simulate(d: Data, acc=None, *, skip_prev=None, rule=None, bsC=None, skip_row=None, extra_row=False, poison_row=None):
    """The C allocation after a launch that accumulated `acc` (default: the exact sums).  The keyword arguments are the store-side
    defects of the mutants; with none of them this is the reference."""
    c = d.case
    acc = d.acc if acc is None else acc
    out = d.C0.copy()
    bsC = c.bs[2] if bsC is None else bsC
    idx = _index(c.batch, c.M, c.N, c.ld[2], bsC)
    inside = idx < out.size                                   # a wrong batch stride may point past the allocation: those stores are lost
    total = acc.astype(np.float64)
    if c.load:
        seen = from_bits(d.C0[np.minimum(idx, out.size - 1)], c.precC)     # what the launch reads where it is about to store
        if skip_prev is not None:
            seen = np.where(skip_prev, 0.0, seen)
        total = total + seen
    bits = to_bits(total, c.precC, rule)
    if poison_row is not None:
        bits[:, poison_row, :] = QUIET_NAN[c.precC]
    keep = np.ones(idx.shape, bool)
    if skip_row is not None:
        keep[:, skip_row, :] = False
    out[idx[inside & keep]] = bits[inside & keep]
    if extra_row:                                             # row M stored with what row M - 1's accumulator holds
        row = _index(c.batch, 1, c.N, c.ld[2], bsC, c.M * c.ld[2])
        out[row] = to_bits(acc[:, c.M - 1:c.M, :], c.precC, rule)
    return out


def reference(d: Data):
    """The exact expected bits of the logical C, [batch, M, N]: int64 A @ B (+ prev), rounded by C's rule."""
    return to_bits(d.acc + (d.prev if d.case.load else 0), d.case.precC)


def _raw(d: Data, which, z, x, k):
    """Operand element (x, k) of batch entry z as the memory holds it, k possibly outside the matrix; NaN (padding) and reads past
    the allocation count as 1."""
    c = d.case
    buf, prec, t, ld, bs, off = ((d.A, c.precA, c.tA, c.ld[0], c.bs[0], c.offA) if which == "A"
                                 else (d.B, c.precB, not c.tB, c.ld[1], c.bs[1], 0))
    idx = off + z * bs + (k * ld + x if t else x * ld + k)
    v = from_bits(buf[np.minimum(idx, buf.size - 1)], prec)
    return np.where((idx >= buf.size) | np.isnan(v), 1.0, v).astype(np.int64)


def _b(d, z):
    return d.b[z if d.b.shape[0] > 1 else 0]


def m_drop_last_k(d):
    K = d.case.K
    return simulate(d, d.acc - np.stack([np.outer(d.a[z][:, K - 1], _b(d, z)[K - 1]) for z in range(d.case.batch)]))


def m_extra_k(d):
    c = d.case
    m, n = np.arange(c.M), np.arange(c.N)
    return simulate(d, d.acc + np.stack([np.outer(_raw(d, "A", z, m, c.K), _raw(d, "B", z, n, c.K)) for z in range(c.batch)]))


def m_stale_b_tile(d):
    """tile 2 (k in [128, 192)) multiplied with the B rows tile 0 left in the same stage buffer"""
    K = d.case.K
    k = np.arange(128, min(K, 192))
    return simulate(d, d.acc + np.stack([_matmul(d.a[z][:, k], _b(d, z)[k - 128] - _b(d, z)[k]) for z in range(d.case.batch)]))


def m_stale_a_last_tile(d):
    K = d.case.K
    k = np.arange((K - 1) // 64 * 64, K)
    return simulate(d, d.acc + np.stack([_matmul(d.a[z][:, k - 64] - d.a[z][:, k], _b(d, z)[k]) for z in range(d.case.batch)]))


def m_swap_k8(d):
    """A's k and k + 8 exchanged inside the first 16-k step"""
    a = d.a[:, :, :16]
    swapped = np.concatenate([a[:, :, 8:16], a[:, :, 0:8]], axis=2)
    return simulate(d, d.acc + np.stack([_matmul(swapped[z] - a[z], _b(d, z)[:16]) for z in range(d.case.batch)]))


def m_batch0_a(d):
    return simulate(d, np.stack([_matmul(d.a[0], _b(d, z)) for z in range(d.case.batch)]))


def m_c_stride_one_row(d):
    return simulate(d, bsC=d.case.bs[2] + d.case.ld[2])


def m_skip_prev_last_column(d):
    skip = np.zeros(d.acc.shape, bool)
    skip[:, :, -1] = True
    return simulate(d, skip_prev=skip)


def m_skip_prev_second_block(d):
    skip = np.zeros(d.acc.shape, bool)
    skip[:, d.case.block:, :] = True
    return simulate(d, skip_prev=skip)


def m_bf16_store_rne(d):
    return simulate(d, rule="rne")


def m_f16_store_trunc(d):
    return simulate(d, rule="trunc")


def m_operands_via_bf16(d):
    squeeze = lambda x: from_bits(to_bits(x, BF16, "trunc"), BF16).astype(np.int64)   # noqa: E731
    return simulate(d, np.stack([_matmul(squeeze(d.a[z]), squeeze(_b(d, z))) for z in range(d.case.batch)]))


def m_last_row_unstored(d):
    return simulate(d, skip_row=d.case.M - 1)


def m_row_m_stored(d):
    return simulate(d, extra_row=True)


def m_straddling_chunk_poisons_last_row(d):
    return simulate(d, poison_row=d.case.M - 1)


def _rounding_visible(c: Case):
    # enough elements and enough terms that thousands of |C| pass the type's last exact odd integer (255 / 2047): see the fills
    return c.M * c.N >= 2048 and c.K >= 63


# name -> (applies to a case, mutated C allocation of a case's data)
MUTANTS = {
    "drop_last_k": (lambda c: c.K >= 1, m_drop_last_k),
    "extra_k": (lambda c: True, m_extra_k),
    "stale_b_tile": (lambda c: c.K > 128, m_stale_b_tile),
    "stale_a_last_tile": (lambda c: c.K > 64, m_stale_a_last_tile),
    "swap_k8": (lambda c: c.K >= 16, m_swap_k8),
    "batch0_a": (lambda c: c.batch > 1, m_batch0_a),
    "c_stride_one_row": (lambda c: c.batch > 1, m_c_stride_one_row),
    "skip_prev_last_column": (lambda c: c.load, m_skip_prev_last_column),
    "skip_prev_second_block": (lambda c: c.load and c.M > c.block, m_skip_prev_second_block),
    "bf16_store_rne": (lambda c: c.precC == BF16 and _rounding_visible(c), m_bf16_store_rne),
    "f16_store_trunc": (lambda c: c.precC == FP16 and _rounding_visible(c), m_f16_store_trunc),
    "operands_via_bf16": (lambda c: c.fill in ("wide_f16", "wide_f32") or (c.fill == "wide_mixed" and c.precA != BF16), m_operands_via_bf16),
    "last_row_unstored": (lambda c: not (c.load and c.K == 0), m_last_row_unstored),
    "row_m_stored": (lambda c: True, m_row_m_stored),
    "straddling_chunk_poisons_last_row": (lambda c: form_of(c) != "f32" and c.tA and c.M % 8 != 0 and c.K >= 1,
                                          m_straddling_chunk_poisons_last_row),
}


def applicable(case: Case):
    return [name for name, (applies, _) in MUTANTS.items() if applies(case)]


# ---------------------------------------------------------------- compare --------------------------------------------------
def compare(got_bits, d: Data):
    """Bitwise equality of a whole C allocation with the reference: every logical element and every canary.  None when equal, else
    a description of the first mismatch as (batch, m, n) with the bits it got and wanted."""
    c = d.case
    got = np.asarray(got_bits).view(STORE_DTYPE[c.precC]).reshape(-1)
    if got.size != d.want.size:
        return f"{c.name}: C allocation of {got.size} elements, expected {d.want.size}"
    wrong = np.flatnonzero(got != d.want)
    if wrong.size == 0:
        return None
    idx = _index(c.batch, c.M, c.N, c.ld[2], c.bs[2])
    logical = np.zeros(got.size, bool)
    logical[idx] = True
    first = int(wrong[0])
    z = min(first // c.bs[2], c.batch - 1) if c.batch > 1 and c.bs[2] else 0
    m, n = divmod(first - z * c.bs[2], c.ld[2])
    what = "element" if logical[first] else "canary"
    nan = " (NaN stored)" if np.isnan(from_bits(got[first:first + 1], c.precC))[0] else ""
    return (f"{c.name}: {wrong.size} of {got.size} differ ({int(logical[wrong].sum())} logical); first: {what} (batch {z}, m {m}, n {n}) "
            f"got 0x{int(got[first]):x} = {from_bits(got[first:first + 1], c.precC)[0]!r}, want 0x{int(d.want[first]):x} = "
            f"{from_bits(d.want[first:first + 1], c.precC)[0]!r}{nan}")


# ---------------------------------------------------------------- the plan -------------------------------------------------
def items():
    """(item id, form, precA, precB, tA, tB) of the GPU test's parametrisation: 3 gemm_16 forms x 2 types x 4 transpose pairs and
    the general kernel's 4 operand pairs x 4 transpose pairs."""
    out = []
    for form in FORMS[1:]:
        for prec in (FP16, BF16):
            for tA, tB in TRANSPOSES:
                out.append((f"{form}-{PREC_NAME[prec]}-{'t' if tA else 'n'}{'t' if tB else 'n'}", form, prec, prec, tA, tB))
    for pa, pb in F32_PAIRS:
        for tA, tB in TRANSPOSES:
            out.append((f"f32-{PREC_NAME[pa]}x{PREC_NAME[pb]}-{'t' if tA else 'n'}{'t' if tB else 'n'}", "f32", pa, pb, tA, tB))
    return out


def _up8(x):
    return (x + 7) // 8 * 8


def leading(ldkind, tA, tB, M, N, K):
    """a16: tight rounded up to 8 elements (16-byte rows).  a8: 4 elements more (8-byte rows: what keeps a 256 x 256 launch on the
    register-staged object at every K).  odd: + 1, + 3, + 5 (2-byte rows)."""
    tight = (M if tA else K, K if tB else N, N)
    if ldkind == "a16":
        return tuple(_up8(x) for x in tight)
    if ldkind == "a8":
        return (_up8(tight[0]) + 4, _up8(tight[1]) + 4, _up8(tight[2]))
    return (tight[0] + 1, tight[1] + 3, tight[2] + 5)


def _wide_fill(pa, pb):
    if pa == pb == BF16:
        return "wide_bf16"
    if pa == pb == FP16:
        return "wide_f16"
    return "wide_f32" if pa == pb == FP32 else "wide_mixed"


@functools.lru_cache(maxsize=1)
def plan():
    """Every launch of tests/test_gemm_exact_gpu.py, as cases grouped by item (Case.item)."""
    cases = []
    for item, form, pa, pb, tA, tB in items():
        big = form in ("g16_256", "g16_256_dma")
        two = (289, 263) if big else (161, 135)
        kinds = {"g16_256": ("a8", "odd")}.get(form, ("a16", "odd"))
        ks = tuple(k for k in K_LIST if k % 8 == 0) if form == "g16_256_dma" else K_LIST
        common = dict(item=item, precA=pa, precB=pb, tA=tA, tB=tB, big=big)
        for si, (M, N) in enumerate((two, (1, 1), (33, 70))):
            for li, ldkind in enumerate(kinds):
                for ki, K in enumerate(ks):
                    pc, load = C_PAIRS[(ki + 2 * si + 3 * li) % 6]    # rotates along K; every kind of the two-block shape sees all six
                    cases.append(Case(kind="shape", M=M, N=N, K=K, ld=leading(ldkind, tA, tB, M, N, K), precC=pc, load=load,
                                      fill="mid" if pc == FP16 else "small", ldkind=ldkind, **common))
        M, N = two
        K, ldkind = BATCH_K, kinds[0]
        ld = leading(ldkind, tA, tB, M, N, K)
        sA, sB, sC = _up8((K if tA else M) * ld[0]) + 16, _up8((N if tB else K) * ld[1]) + 24, M * ld[2] + 40
        for bs, pc, load in (((sA, sB, sC), FP32, False),                      # padded strides, multiples of 8
                             ((sA + 1, sB, sC), BF16, True),                   # the same with bsA odd
                             ((sA, 0, sC), FP16, False),                       # one B shared by all entries
                             (((K if tA else M) * ld[0], (N if tB else K) * ld[1], sC + 3), FP32, True)):   # tight A and B, C padded
            cases.append(Case(kind="batch", M=M, N=N, K=K, ld=ld, precC=pc, load=load, fill="mid" if pc == FP16 else "small",
                              ldkind=ldkind, batch=BATCH, bs=bs, **common))
        cases.append(Case(kind="base", M=M, N=N, K=K, ld=ld, precC=BF16, load=True, fill="small", ldkind=ldkind, offA=1, **common))
        wide = _wide_fill(pa, pb)
        for K, pc, load in ((72, FP32, False), (min(200, FILLS[wide][3]), BF16, True)):
            cases.append(Case(kind="wide", M=M, N=N, K=K, ld=leading(ldkind, tA, tB, M, N, K), precC=pc, load=load, fill=wide,
                              ldkind=ldkind, **common))
    return cases


def cases_of(item):
    return [c for c in plan() if c.item == item]
