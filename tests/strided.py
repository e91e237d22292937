"""Layout harness: the operands of one attention problem placed in memory by a per-operand layout description.

Every operand of a launch has its own base pointer, leadingDimension, headStride and batchStride (include/mfa.h,
mfa_launch_params).  `place()` turns (problem, layout name) into a Placement: for every operand a View -- the allocation it
lives in, its element offset there and its three strides -- in exactly the form AttentionKernel.dispatch takes.  L and D have
head and batch strides and no leading dimension.

Everything here is numpy on bit patterns (uint16 for the 16-bit types, uint32 for FP32), so the layout code runs without a GPU:
tests/test_strided_layout_plans.py plans launches from Placements with fake pointers and runs the checks below on a numpy model
of attention and its mutants; tests/test_strided_layouts_gpu.py uploads the same allocations and runs the kernels.

Poison and canary.  Every element of an allocation that belongs to no operand element -- pad columns, gaps between heads and
batch entries, the tail -- is poison: input allocations hold a quiet NaN of the operand's storage type there, output
allocations a canary bit pattern (0xCACA / 0xCACACACA, a finite number, so a NaN in an output is always something a kernel
wrote).  Padding another operand owns (the next head of a token-major tensor, the sibling slice of a fused allocation) is that
operand's real data.  After the launches `verify()` runs four checks:
  (a) every input allocation is bit-identical to what was uploaded;
  (b) every element of every output allocation no operand owns still holds the canary (whole allocation, not a tail);
  (c) no owned output element is NaN unless the packed launch produced the same NaN;
  (d) the owned elements, gathered back to [B, H, seq, D], are what the comparisons get.
A failure names the layout, the operand, the (batch, head) and the first differing (row, column).
"""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass, field

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from metal_flash_attention_amd import AttentionOperand as Op, GEMMOperandPrecision as P  # noqa: E402

INPUTS = (Op.Q, Op.K, Op.V, Op.dO)
OUTPUTS = (Op.O, Op.L, Op.D, Op.dQ, Op.dK, Op.dV)
MATRICES = (Op.Q, Op.K, Op.V, Op.O, Op.dO, Op.dQ, Op.dK, Op.dV)
VECTORS = (Op.L, Op.D)
KV_OPS = (Op.K, Op.V, Op.dK, Op.dV)
LAYOUTS = ("packed", "token", "fused", "padded", "mixed", "broadcast", "misaligned_ld", "misaligned_ptr")

BITS = {P.FP32: np.uint32, P.FP16: np.uint16, P.BF16: np.uint16}
NAN_POISON = {P.FP32: 0x7FC00000, P.FP16: 0x7E00, P.BF16: 0x7FC0}
CANARY = {P.FP32: 0xCACACACA, P.FP16: 0xCACA, P.BF16: 0xCACA}


# ---- storage types as bit patterns -------------------------------------------------------------------------------------------
def encode(x, precision):
    """float32 array -> bit patterns of `precision` (FP16: round to nearest even; BF16: truncation, as tests/harness.py packs)"""
    x = np.ascontiguousarray(x, np.float32)
    if precision == P.FP32:
        return x.view(np.uint32).copy()
    if precision == P.FP16:
        return x.astype(np.float16).view(np.uint16).copy()
    return (x.view(np.uint32) >> 16).astype(np.uint16)


def decode(bits, precision):
    bits = np.ascontiguousarray(bits)
    if precision == P.FP32:
        return bits.view(np.float32).copy()
    if precision == P.FP16:
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def is_nan(bits, precision):
    return np.isnan(decode(bits, precision))


# ---- problem, views, placement -----------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Problem:
    B: int
    Hq: int
    Hkv: int
    R: int
    C: int
    D: int
    precisions: dict = field(hash=False, compare=False, default=None)     # {operand: GEMMOperandPrecision} (memoryPrecisions)
    transposed: dict = field(hash=False, compare=False, default_factory=dict)   # {operand: bool}: stored [D][seq], ld >= seq

    def heads(self, op):
        return self.Hkv if op in KV_OPS else self.Hq

    def seq(self, op):
        return self.C if op in KV_OPS else self.R

    def shape(self, op):
        return (self.B, self.heads(op), self.seq(op)) + (() if op in VECTORS else (self.D,))

    def unit(self, op):
        """elements per 16 bytes of the operand's storage type"""
        return 4 if self.precisions[op] == P.FP32 else 8


@dataclass
class View:
    alloc: str            # name of the allocation
    offset: int           # elements from the allocation's base to element (batch 0, head 0, row 0, column 0)
    ld: int               # leadingDimension (0 for L / D: rows are one element apart)
    headStride: int
    batchStride: int
    transposed: bool = False


@dataclass
class Placement:
    layout: str
    problem: Problem
    views: dict                      # {operand: View}
    allocs: dict                     # {name: (precision, elements, "in" | "out")}

    def indices(self, op, heads=None):
        """element offsets into the allocation of every owned element, shape problem.shape(op)"""
        p, v = self.problem, self.views[op]
        B, H, S = p.B, (heads or p.heads(op)), p.seq(op)
        b = np.arange(B, dtype=np.int64).reshape(B, 1, 1, 1) * v.batchStride
        h = np.arange(H, dtype=np.int64).reshape(1, H, 1, 1) * v.headStride
        r = np.arange(S, dtype=np.int64).reshape(1, 1, S, 1)
        if op in VECTORS:
            return (v.offset + b + h + r)[..., 0]
        d = np.arange(p.D, dtype=np.int64).reshape(1, 1, 1, p.D)
        return v.offset + b + h + (d * v.ld + r if v.transposed else r * v.ld + d)

    def launch_kwargs(self):
        """leadingDimensions / headStrides / batchStrides as AttentionKernel.dispatch takes them"""
        lds = {op: v.ld for op, v in self.views.items() if op in MATRICES}
        return dict(leadingDimensions=lds, headStrides={op: v.headStride for op, v in self.views.items()},
                    batchStrides={op: v.batchStride for op, v in self.views.items()})

    def pointers(self, bases):
        """{operand: device address} from {allocation name: base address}"""
        out = {}
        for op, v in self.views.items():
            size = 4 if self.problem.precisions[op] == P.FP32 else 2
            out[op] = int(bases[v.alloc]) + v.offset * size
        return out

    def extent(self, op):
        """one past the last element offset the view owns"""
        p, v = self.problem, self.views[op]
        last = v.offset + (p.B - 1) * v.batchStride + (p.heads(op) - 1) * v.headStride
        if op in VECTORS:
            return last + p.seq(op)
        rows, cols = (p.D, p.seq(op)) if v.transposed else (p.seq(op), p.D)
        return last + (rows - 1) * v.ld + cols


class _Builder:
    def __init__(self, problem, layout):
        self.p, self.layout, self.views, self.allocs = problem, layout, {}, {}

    def alloc(self, name, op, elements, tail=64):
        kind = "in" if op in INPUTS else "out"
        self.allocs[name] = (self.p.precisions[op], int(elements) + tail, kind)

    def own(self, op, ld, hs, bs, offset=0, name=None, transposed=False):
        """a view in an allocation of its own, sized to the view's extent (+ a poisoned tail)"""
        name = name or op.name
        self.views[op] = View(name, offset, ld, hs, bs, transposed)
        pl = Placement(self.layout, self.p, self.views, self.allocs)
        self.alloc(name, op, pl.extent(op))

    def done(self):
        return Placement(self.layout, self.p, self.views, self.allocs)


def _rows_cols(p, op):
    """(rows, columns) of one head's stored matrix"""
    return (p.D, p.seq(op)) if p.transposed.get(op) else (p.seq(op), p.D)


def _round_up(x, m):
    return (x + m - 1) // m * m


def place(problem, layout):
    """Placement of every operand of `problem` under the named layout (LAYOUTS)."""
    p = problem
    b = _Builder(p, layout)
    tr = lambda op: bool(p.transposed.get(op))   # noqa: E731

    def packed(op, pad_ld=0, pad_head=0, pad_batch=0, offset=0):
        if op in VECTORS:
            hs = p.seq(op) + pad_head
            b.own(op, 0, hs, p.heads(op) * hs + pad_batch, offset)
            return
        rows, cols = _rows_cols(p, op)
        ld = (_round_up(cols, p.unit(op)) if pad_ld and tr(op) else cols) + pad_ld
        hs = rows * ld + pad_head
        b.own(op, ld, hs, p.heads(op) * hs + pad_batch, offset, transposed=tr(op))

    def token_major(op, pad_head=0):
        """[B, seq, H, D (+ pad_head)]; a transposed operand as [B, D, H, seq]"""
        rows, cols = _rows_cols(p, op)
        hs = _round_up(cols, p.unit(op)) + pad_head if tr(op) or pad_head else cols
        ld = p.heads(op) * hs
        b.own(op, ld, hs, rows * ld, transposed=tr(op))

    def head_outer(op, pad_ld=0):
        """[H, B, seq, D (+ pad_ld)]: the head stride is larger than the batch stride"""
        if op in VECTORS:
            bs = p.seq(op) + pad_ld
            b.own(op, 0, p.B * bs, bs)
            return
        rows, cols = _rows_cols(p, op)
        ld = (_round_up(cols, p.unit(op)) if pad_ld and tr(op) else cols) + pad_ld
        b.own(op, ld, p.B * rows * ld, rows * ld, transposed=tr(op))

    def fused(ops, name, slots, pad_head=0):
        """the operands as slices i of one [B, N, slots, H, D (+ pad_head)] allocation (slices beyond len(ops) belong to no operand)"""
        H, hs, N = p.heads(ops[0]), p.D + pad_head, p.seq(ops[0])
        assert all(p.heads(o) == H and p.seq(o) == N and not tr(o) for o in ops), "fused slices need equal heads and lengths"
        for i, op in enumerate(ops):
            b.views[op] = View(name, i * H * hs, slots * H * hs, hs, N * slots * H * hs)
        b.alloc(name, ops[0], p.B * N * slots * H * hs)

    if layout == "packed":
        for op in MATRICES + VECTORS:
            packed(op)
    elif layout == "token":
        for op in MATRICES:
            token_major(op)
        for op in VECTORS:
            packed(op)
    elif layout == "fused":
        fused((Op.Q, Op.K, Op.V), "QKV", 3)
        fused((Op.dQ, Op.dK, Op.dV), "dQKV", 3)
        token_major(Op.O)
        token_major(Op.dO)
        for op in VECTORS:
            packed(op)
    elif layout == "padded":
        for op in MATRICES:
            u = p.unit(op)
            packed(op, pad_ld=u, pad_head=2 * u, pad_batch=4 * u)
        packed(Op.L, pad_head=8, pad_batch=16)
        packed(Op.D, pad_head=24, pad_batch=8)
    elif layout == "mixed":
        # a different layout and a different ld per operand; the nesting of heads and batch entries differs too (a launch has ONE
        # head stride per operand, so "not in head order" can only mean a head stride above the batch stride: K, dQ and D)
        uq = uo = 8   # (16 bytes of a 16-bit type, 32 of FP32: one set of pads keeps every storage type aligned and every ld distinct)
        token_major(Op.Q)
        head_outer(Op.K)
        packed(Op.V, pad_ld=uq, pad_head=3 * uq, pad_batch=uq)
        packed(Op.O, pad_ld=2 * uo, pad_head=uo, pad_batch=5 * uo)
        if tr(Op.dO):
            packed(Op.dO, pad_ld=48, pad_head=56)
        else:
            fused((Op.dO,), "dO", 2, pad_head=16)
        head_outer(Op.dQ, pad_ld=3 * uo)
        token_major(Op.dK, pad_head=uo if p.Hkv > 1 else 4 * uo)
        packed(Op.dV, pad_ld=5 * uo, pad_head=2 * uo, pad_batch=3 * uo, offset=4 * uo)
        packed(Op.L, pad_head=8, pad_batch=16)
        head_outer(Op.D, pad_ld=24)
        _make_distinct(b)
    elif layout == "broadcast":
        assert p.Hkv == 1, "broadcast K / V: one stored head"
        for op in MATRICES + VECTORS:
            packed(op)
        for op in (Op.K, Op.V):
            b.views[op].headStride = 0
    elif layout == "misaligned_ld":
        for op in MATRICES:
            packed(op, pad_ld=1)
        for op in VECTORS:
            packed(op)
    elif layout == "misaligned_ptr":
        for op in MATRICES:
            packed(op, offset=1)
        for op in VECTORS:
            packed(op)
    else:
        raise ValueError(layout)
    return b.done()


def _make_distinct(b):
    """mixed: no two matrix operands share a leading dimension or a head stride (a swapped stride must change the addresses)"""
    for attr in ("ld", "headStride"):
        seen = set()
        for op in MATRICES:
            v = b.views[op]
            assert getattr(v, attr) not in seen, ("mixed layout: two operands share %s = %d (%s); choose other heads or pads"
                                                  % (attr, getattr(v, attr), op.name))
            seen.add(getattr(v, attr))


# ---- host images of the allocations ------------------------------------------------------------------------------------------
def build_allocations(placement, values):
    """{allocation: bit-pattern array}: inputs hold `values` ({operand: float32 [B, H, seq, D]}) at the owned elements and NaN
    poison elsewhere; outputs hold the canary everywhere."""
    p = placement.problem
    host = {}
    for name, (prec, n, kind) in placement.allocs.items():
        host[name] = np.full(n, NAN_POISON[prec] if kind == "in" else CANARY[prec], BITS[prec])
    for op in INPUTS:
        v = placement.views[op]
        x = np.asarray(values[op], np.float32)
        assert x.shape == p.shape(op), (op.name, x.shape, p.shape(op))
        host[v.alloc][placement.indices(op)] = encode(x, p.precisions[op])
    return host


def refill_outputs(placement, host):
    for name, (prec, n, kind) in placement.allocs.items():
        if kind == "out":
            host[name][:] = CANARY[prec]


def owned_mask(placement, name, valid=None):
    """bool array over allocation `name`: elements some output operand owns.  valid: {operand: bool array of problem.shape(op)[:3]}
    restricts ownership (per-batch lengths: rows / columns beyond a batch entry's length are not written and keep the canary)"""
    mask = np.zeros(placement.allocs[name][1], bool)
    for op, v in placement.views.items():
        if v.alloc != name:
            continue
        idx = placement.indices(op)
        if valid is not None and op in valid:
            keep = valid[op] if op in VECTORS else np.broadcast_to(valid[op][..., None], idx.shape)
            idx = idx[keep]
        mask[idx.reshape(-1)] = True
    return mask


def gather(placement, host, op):
    """bit patterns of the owned elements of `op`, shape problem.shape(op)"""
    return host[placement.views[op].alloc][placement.indices(op)]


def first_difference(a, b):
    """'batch b head h (row r, column c)' of the first differing element of two [B, H, seq(, D)] arrays"""
    where = np.argwhere(a != b)
    if not len(where):
        return None
    w = where[0]
    return "batch %d head %d (row %d, column %s), %d elements differ" % (w[0], w[1], w[2], w[3] if len(w) > 3 else "-", len(where))


def verify(placement, uploaded, after, packed=None, ops=OUTPUTS, valid=None, bitwise=True):
    """The four checks on the allocations read back after the launches.  uploaded / after: {allocation: bit patterns}.
    packed: {operand: bit patterns [B, H, seq(, D)]} of the packed launch (None: no bit comparison).  Returns (failures, values):
    a list of messages naming layout, operand, head and first differing element, and {operand: gathered bit patterns}."""
    p = placement.problem
    failures, got = [], {}
    for name, (prec, n, kind) in placement.allocs.items():
        if kind == "in":                                                                     # (a)
            if not np.array_equal(uploaded[name], after[name]):
                at = int(np.flatnonzero(uploaded[name] != after[name])[0])
                failures.append("%s: input allocation %s was written (first at element %d)" % (placement.layout, name, at))
        else:                                                                                # (b)
            users = [op for op, v in placement.views.items() if v.alloc == name and op in ops]
            if not users:
                continue
            stray = ~owned_mask(placement, name, valid) & (after[name] != CANARY[prec])
            if stray.any():
                at = int(np.flatnonzero(stray)[0])
                failures.append("%s: output allocation %s (%s): %d elements no operand owns were written, first at element %d (%s)"
                                % (placement.layout, name, "/".join(o.name for o in users), int(stray.sum()), at, _locate(placement, users, at)))
    for op in ops:
        prec = p.precisions[op]
        bits = gather(placement, after, op)
        got[op] = bits
        keep = np.ones(bits.shape, bool)
        if valid is not None and op in valid:
            keep = valid[op] if op in VECTORS else np.broadcast_to(valid[op][..., None], bits.shape)
            if (bits[~keep] != CANARY[prec]).any():
                failures.append("%s: %s: padding beyond a batch entry's length was written: %s"
                                % (placement.layout, op.name, first_difference(np.where(keep, CANARY[prec], bits), np.full_like(bits, CANARY[prec]))))
        nan = is_nan(bits, prec) & keep                                                      # (c)
        if packed is not None:
            nan &= ~is_nan(packed[op], prec)
        if nan.any():
            failures.append("%s: %s: NaN the packed launch does not have: %s" % (placement.layout, op.name, first_difference(nan, np.zeros_like(nan))))
        unwritten = (bits == CANARY[prec]) & keep
        if unwritten.any() and (packed is None or not np.array_equal(unwritten, (packed[op] == CANARY[prec]) & keep)):
            failures.append("%s: %s: owned elements still hold the canary: %s" % (placement.layout, op.name, first_difference(unwritten, np.zeros_like(unwritten))))
        if packed is not None and bitwise:                                                   # (d) against the packed launch
            a, b = np.where(keep, bits, 0), np.where(keep, packed[op], 0)
            if not np.array_equal(a, b):
                failures.append("%s: %s differs from the packed launch: %s" % (placement.layout, op.name, first_difference(a, b)))
    return failures, got


def _locate(placement, users, at):
    """the pad position of allocation element `at` relative to the first operand view of the allocation"""
    op = users[0]
    v, p = placement.views[op], placement.problem
    rel = at - v.offset
    if rel < 0:
        return "before %s" % op.name
    if op in VECTORS:
        return "past/between the heads of %s" % op.name
    if v.batchStride >= v.headStride:
        bi, rem = divmod(rel, v.batchStride)
        hi, rem = divmod(rem, v.headStride) if v.headStride else (0, rem)
    else:
        hi, rem = divmod(rel, v.headStride)
        bi, rem = divmod(rem, v.batchStride) if v.batchStride else (0, rem)
    row, col = divmod(rem, v.ld) if v.ld else (0, rem)
    return "relative to %s: batch %d head %d row %d column %d" % (op.name, bi, hi, row, col)


# ---- cases: one problem + layout + launch kind, shared by the CPU plan test and the GPU test ----------------------------------
@dataclass(frozen=True)
class Case:
    storage: str            # "bf16", "f16" (dO in FP16 too), "f16bf" (FP16 Q / K / V, BF16 dO: the reference's mix), "f32"
    D: int
    layout: str
    Hq: int = 3
    G: int = 1              # query heads per K / V head
    B: int = 2
    R: int = 300
    C: int = 520
    mid: bool = False       # lowPrecisionIntermediates
    out16: bool = False     # lowPrecisionOutputs
    causal: bool = False
    lengths: tuple = None   # ((row lengths per batch entry), (column lengths per batch entry))
    mask: tuple = None      # rows of booleans: 256-row blocks x 128-column blocks
    ws: bool = False        # give every launch the workspace it asks for (split launches)
    transposed: str = "none"   # stored [D][seq]: "kv": K, V, dK, dV; "all": every matrix operand; "q": Q, O, dO, dQ; "k": K, dK; "v": V, dV
    types: tuple = ("forward", "backwardQuery", "backwardKeyValue")

    @property
    def id(self):
        bits = [self.storage + ("mid" if self.mid else "") + ("out" if self.out16 else ""), "d%d" % self.D, self.layout,
                "b%dh%dg%d" % (self.B, self.Hq, self.G), "%dx%d" % (self.R, self.C)]
        bits += [w for w, on in (("causal", self.causal), ("lengths", self.lengths), ("mask", self.mask), ("ws", self.ws),
                                 ("tr" + self.transposed, self.transposed != "none")) if on]
        if len(self.types) < 3:
            bits.append("+".join(t[:3] + t[8:9] for t in self.types))
        return "-".join(bits)


def descriptor(case):
    from metal_flash_attention_amd import AttentionDescriptor
    d = AttentionDescriptor()
    d.lowPrecisionInputs = case.storage != "f32"
    d.lowPrecisionIntermediates = case.mid
    d.lowPrecisionInputType = P.BF16 if case.storage == "bf16" else P.FP16
    d.lowPrecisionOutputs = case.out16
    d.matrixDimensions = (case.R, case.C, case.D)
    tr = case.transposed
    d.transposeState = {"none": (False,) * 4, "kv": (False, True, True, False), "all": (True,) * 4, "q": (True, False, False, True),
                        "k": (False, True, False, False), "v": (False, False, True, False)}[tr]
    return d


def make_kernels(case):
    """({kernel type: AttentionKernel}, memory precisions of every operand)"""
    from metal_flash_attention_amd import AttentionKernel, AttentionKernelType
    desc = descriptor(case)
    precisions = dict(desc.memoryPrecisions)
    if case.storage == "f16":   # a caller's override of the kernel descriptor: dO next to FP16 Q / K / V in FP16 as well
        precisions[Op.dO] = P.FP16
    kernels = {}
    for t in AttentionKernelType:
        if t.name not in case.types:
            continue
        kd = desc.kernelDescriptor(t)
        if case.storage == "f16" and Op.dO in kd.memoryPrecisions:
            kd.memoryPrecisions[Op.dO] = P.FP16
        kernels[t] = AttentionKernel(kd)
    return kernels, {op: P(int(v)) for op, v in precisions.items()}


def problem_of(case, precisions, materialised=False):
    """materialised: K / V with one stored head per query head (what a broadcast launch must equal)"""
    kv, allm = (Op.K, Op.V, Op.dK, Op.dV), MATRICES
    tr = {op: True for op in {"none": (), "kv": kv, "all": allm, "q": (Op.Q, Op.O, Op.dO, Op.dQ), "k": (Op.K, Op.dK),
                              "v": (Op.V, Op.dV)}[case.transposed]}
    broadcast = case.layout == "broadcast" and not materialised
    return Problem(case.B, case.Hq, 1 if broadcast else case.Hq // case.G, case.R, case.C, case.D, precisions, tr)


def pack_mask(rows):
    """rows of booleans (256-row blocks x 128-column blocks) -> int32 words [row blocks][words], bit b of word w = column block 32 w + b"""
    words = (len(rows[0]) + 31) // 32
    out = np.zeros((len(rows), words), np.uint32)
    for i, row in enumerate(rows):
        for j, on in enumerate(row):
            if on:
                out[i, j // 32] |= np.uint32(1 << (j % 32))
    return out.view(np.int32)


def launch_kwargs(case, placement):
    kw = dict(row=case.R, column=case.C, heads=case.Hq, batches=case.B, causal=case.causal,
              headsPerKeyValue=1 if case.layout == "broadcast" else case.G)
    kw.update(placement.launch_kwargs())
    return kw


def wants_workspace(case, kernel_type):
    """forward / backwardQuery: split launches and re-layout copies when the case says so; backwardKeyValue also the slabs of a
    grouped launch (required)"""
    return case.ws or (kernel_type.name == "backwardKeyValue" and case.G > 1 and case.layout != "broadcast")


class FakeBuffer:
    """an address and a size, for planning launches without a device"""

    def __init__(self, address, nbytes):
        self.address, self.nbytes = address, nbytes

    def data_ptr(self):
        return self.address


def planned_forms(case, layout=None, kernels=None, precisions=None):
    """{kernel type name: launch form} of the case under `layout` (default: its own), planned with fake 256-byte aligned addresses"""
    if kernels is None:
        kernels, precisions = make_kernels(case)
    layout = layout or case.layout
    placement = place(problem_of(case, precisions, materialised=layout == "packed"), layout)
    bases = {name: 0x100000000 * (i + 1) for i, name in enumerate(sorted(placement.allocs))}
    ptrs = placement.pointers(bases)
    kw = launch_kwargs(case, placement)
    if layout == "packed" and case.layout == "broadcast":
        kw["headsPerKeyValue"] = 1
    if case.lengths:
        kw.update(rowLengths=0x7000000, columnLengths=0x7100000)
    if case.mask:
        kw.update(blockMask=0x7200000, blockMaskWords=int(pack_mask(case.mask).shape[1]))
    out = {}
    for t, k in kernels.items():
        ws = None
        if wants_workspace(case, t):
            need = k.workspaceSize(row=case.R, column=case.C, heads=case.Hq, batches=case.B, headsPerKeyValue=kw["headsPerKeyValue"])
            ws = FakeBuffer(0x7400000000, need) if need else None
        used = {op: ptrs[op] for op in ptrs}
        out[t.name] = k.launchForm(used, workspace=ws, **kw)
    return out
