"""Host-side mirror of the reference's attention API, over the C ABI (include/mfa.h).

Same names, argument meaning and error behaviour as the Swift types, so tests read like the
reference's own (Tests/FlashAttentionTests/Attention/SquareAttentionTest.swift:214-263):

    attentionDesc = AttentionDescriptor()
    attentionDesc.lowPrecisionInputs = False
    attentionDesc.lowPrecisionIntermediates = False
    attentionDesc.matrixDimensions = (row, column, head)
    attentionDesc.transposeState = (False, False, False, False)
    kernelDesc = attentionDesc.kernelDescriptor(type=AttentionKernelType.forward)
    kernel = AttentionKernel(descriptor=kernelDesc)
    kernel.blockDimensions, kernel.threadgroupSize, kernel.threadgroupMemoryAllocation
    kernel.dispatch(buffers, row=R, column=C)    # replaces createSource + pipeline + encoder

Reference types mirrored:
  AttentionDescriptor        Sources/FlashAttention/Attention/AttentionDescriptor/AttentionDescriptor.swift:10-148
  AttentionKernelDescriptor  Sources/FlashAttention/Attention/AttentionKernelDescriptor.swift:8-49
  AttentionKernelType        Sources/FlashAttention/Attention/AttentionKernelType.swift:10-23
  AttentionOperand           Sources/FlashAttention/Attention/AttentionOperand.swift:9-71
  AttentionKernel            Sources/FlashAttention/Attention/AttentionKernel/AttentionKernel.swift:10-51
  GEMMOperandPrecision       Sources/FlashAttention/GEMM/GEMMOperandPrecision.swift:33-60
Where the reference calls fatalError this raises MFAError (status codes of include/mfa.h).
All logic lives in the C++ library; this file only marshals.
"""
from __future__ import annotations

import ctypes
import enum
import itertools
from typing import Dict, Iterable, Mapping, Optional, Sequence, Tuple, Union

from . import _abi
from ._abi import MFAError, check, lib


class GEMMOperandPrecision(enum.IntEnum):
    FP32 = 0
    FP16 = 1
    BF16 = 2

    @property
    def name_in_shader(self) -> str:  # `.name` in Swift (GEMMOperandPrecision.swift:39-48)
        return lib().mfa_precision_name(int(self)).decode()

    @property
    def size(self) -> int:  # GEMMOperandPrecision.swift:51-59
        return int(lib().mfa_precision_size(int(self)))


class AttentionKernelType(enum.IntEnum):
    forward = 0
    backwardQuery = 1
    backwardKeyValue = 2


class AttentionOperand(enum.IntEnum):
    Q = 0
    K = 1
    S = 2
    P = 3
    V = 4
    O = 5  # noqa: E741
    L = 6
    D = 7
    dO = 8
    dV = 9
    dP = 10
    dS = 11
    dK = 12
    dQ = 13

    @property
    def description(self) -> str:
        return lib().mfa_operand_name(int(self)).decode()

    @property
    def bufferBinding(self) -> Optional[int]:
        b = int(lib().mfa_operand_buffer_binding(int(self)))
        return None if b < 0 else b


def _dict_from(array, cast=int) -> Dict[AttentionOperand, object]:
    out = {}
    for op in AttentionOperand:
        v = int(array[int(op)])
        if v >= 0:
            out[op] = cast(v)
    return out


def _fill(array, mapping: Mapping[AttentionOperand, object]) -> None:
    for i in range(_abi.MFA_OPERAND_COUNT):
        array[i] = -1
    for op, v in mapping.items():
        array[int(AttentionOperand(op))] = int(v)


class AttentionKernelDescriptor:
    """AttentionKernelDescriptor.swift:8-49 (every field optional / a dictionary)."""

    def __init__(self):
        self.blockDimensions: Optional[Tuple[int, int, int]] = None  # (parallelization, traversal, head)
        self.cacheState: Dict[AttentionOperand, bool] = {}
        self.headDimension: Optional[int] = None
        self.memoryPrecisions: Dict[AttentionOperand, GEMMOperandPrecision] = {}
        self.preferAsyncCache: Optional[bool] = None
        self.preferAsyncLoad: Optional[bool] = None
        self.registerPrecisions: Dict[AttentionOperand, GEMMOperandPrecision] = {}
        self.transposeState: Dict[AttentionOperand, bool] = {}
        self.type: Optional[AttentionKernelType] = None
        # extension: True = block dimensions / cache state no compiled variant implements are an error
        self.strictBlockDimensions: bool = False

    def _to_c(self) -> _abi.mfa_attention_kernel_descriptor:
        c = _abi.mfa_attention_kernel_descriptor()
        lib().mfa_attention_kernel_descriptor_init(ctypes.byref(c))
        if self.blockDimensions is not None:
            c.hasBlockDimensions = 1
            c.parallelization, c.traversal, c.headBlock = (int(x) for x in self.blockDimensions)
        if self.headDimension is not None:
            c.hasHeadDimension = 1
            c.headDimension = int(self.headDimension)
        _fill(c.cacheState, {k: int(bool(v)) for k, v in self.cacheState.items()})
        _fill(c.memoryPrecisions, self.memoryPrecisions)
        _fill(c.registerPrecisions, self.registerPrecisions)
        _fill(c.transposeState, {k: int(bool(v)) for k, v in self.transposeState.items()})
        c.preferAsyncCache = -1 if self.preferAsyncCache is None else int(bool(self.preferAsyncCache))
        c.preferAsyncLoad = -1 if self.preferAsyncLoad is None else int(bool(self.preferAsyncLoad))
        c.type = -1 if self.type is None else int(self.type)
        c.strictBlockDimensions = int(bool(self.strictBlockDimensions))
        return c

    @classmethod
    def _from_c(cls, c: _abi.mfa_attention_kernel_descriptor) -> "AttentionKernelDescriptor":
        d = cls()
        if c.hasBlockDimensions:
            d.blockDimensions = (int(c.parallelization), int(c.traversal), int(c.headBlock))
        if c.hasHeadDimension:
            d.headDimension = int(c.headDimension)
        d.cacheState = _dict_from(c.cacheState, bool)
        d.memoryPrecisions = _dict_from(c.memoryPrecisions, GEMMOperandPrecision)
        d.registerPrecisions = _dict_from(c.registerPrecisions, GEMMOperandPrecision)
        d.transposeState = _dict_from(c.transposeState, bool)
        d.preferAsyncCache = None if c.preferAsyncCache < 0 else bool(c.preferAsyncCache)
        d.preferAsyncLoad = None if c.preferAsyncLoad < 0 else bool(c.preferAsyncLoad)
        d.type = None if c.type < 0 else AttentionKernelType(int(c.type))
        return d


class AttentionDescriptor:
    """AttentionDescriptor.swift:10-27."""

    def __init__(self):
        self.lowPrecisionInputs: bool = False          # Q, K, V, dO
        self.lowPrecisionIntermediates: bool = False   # S, P, L, D, dP, dS
        self.matrixDimensions: Optional[Tuple[int, int, int]] = None  # (row, column, head)
        self.transposeState: Optional[Tuple[bool, bool, bool, bool]] = None  # (Q, K, V, O)
        # extension: storage type of low-precision inputs (FP16 = reference behaviour)
        self.lowPrecisionInputType: GEMMOperandPrecision = GEMMOperandPrecision.FP16
        self.lowPrecisionOutputs: bool = False   # extension: O, dQ, dK, dV stored in lowPrecisionInputType

    def _to_c(self) -> _abi.mfa_attention_descriptor:
        c = _abi.mfa_attention_descriptor()
        lib().mfa_attention_descriptor_init(ctypes.byref(c))
        c.lowPrecisionInputs = int(bool(self.lowPrecisionInputs))
        c.lowPrecisionIntermediates = int(bool(self.lowPrecisionIntermediates))
        c.lowPrecisionInputType = int(self.lowPrecisionInputType)
        c.lowPrecisionOutputs = 1 if self.lowPrecisionOutputs else 0
        if self.matrixDimensions is not None:
            c.hasMatrixDimensions = 1
            c.row, c.column, c.head = (int(x) for x in self.matrixDimensions)
        if self.transposeState is not None:
            c.hasTransposeState = 1
            c.transposeQ, c.transposeK, c.transposeV, c.transposeO = (int(bool(x)) for x in self.transposeState)
        return c

    @property
    def memoryPrecisions(self) -> Dict[AttentionOperand, GEMMOperandPrecision]:
        """AttentionDescriptor+Precisions.swift:10-146."""
        out = (ctypes.c_int8 * _abi.MFA_OPERAND_COUNT)()
        c = self._to_c()
        check(lib().mfa_attention_descriptor_memory_precisions(ctypes.byref(c), out))
        return _dict_from(out, GEMMOperandPrecision)

    @property
    def registerPrecisions(self) -> Dict[AttentionOperand, GEMMOperandPrecision]:
        """AttentionDescriptor+Precisions.swift:149-215."""
        out = (ctypes.c_int8 * _abi.MFA_OPERAND_COUNT)()
        c = self._to_c()
        check(lib().mfa_attention_descriptor_register_precisions(ctypes.byref(c), out))
        return _dict_from(out, GEMMOperandPrecision)

    def kernelDescriptor(self, type: AttentionKernelType) -> AttentionKernelDescriptor:  # noqa: A002
        """AttentionDescriptor.swift:33-130."""
        c = self._to_c()
        out = _abi.mfa_attention_kernel_descriptor()
        check(lib().mfa_attention_descriptor_kernel_descriptor(ctypes.byref(c), int(type), ctypes.byref(out)))
        return AttentionKernelDescriptor._from_c(out)


def parameterFile(type: AttentionKernelType, mixed: bool) -> str:  # noqa: A002
    """AttentionDescriptor.parameterFile(type:) (+Parameters.swift:13-39) for gfx950."""
    buf = ctypes.create_string_buffer(8192)
    check(lib().mfa_parameter_table_get(int(type), int(bool(mixed)), buf, len(buf)))
    return buf.value.decode()


def setParameterFile(type: AttentionKernelType, mixed: bool, text: str) -> None:  # noqa: A002
    """Install a parameter table (text format of AttentionParameterRow.parseTable).  `mixed=True` is the table consulted for
    every descriptor with lowPrecisionInputs (16-bit Q, K, V -> the 16-bit matrix-core code objects), with or without
    lowPrecisionIntermediates; `mixed=False` the table of FP32 inputs.  The reference consults its mixed tables only when
    BOTH flags are set (+Parameters.swift:16) -- include/mfa.h and DESIGN.md 5 give the reason for the departure."""
    check(lib().mfa_parameter_table_set(int(type), int(bool(mixed)), text.encode()))


def resetParameterFiles() -> None:
    check(lib().mfa_parameter_table_reset())


def selectParameterRow(text: str, headDimension: int) -> dict:
    """AttentionParameterRow.parseTable + AttentionDescriptor.row(table:)
    (AttentionParameterRow.swift:22-74, +Parameters.swift:41-66)."""
    row = _abi.mfa_parameter_row()
    check(lib().mfa_parameter_table_select(text.encode(), int(headDimension), ctypes.byref(row)))
    return {
        "maximumHeadDimension": int(row.maximumHeadDimension),
        "parallelization": int(row.parallelization),
        "traversal": int(row.traversal),
        "head": int(row.head),
        "cachedOperands": [op for op in AttentionOperand if row.cached[int(op)] == 1],
    }


BufferLike = Union[int, None, object]


def _pointer(b: BufferLike) -> Optional[int]:
    if b is None:
        return None
    if isinstance(b, int):
        return b
    if hasattr(b, "data_ptr"):  # torch.Tensor (device memory plumbing only)
        return int(b.data_ptr())
    raise TypeError(f"cannot take a device pointer from {type(b)!r}")


class AttentionKernel:
    """AttentionKernel.swift:10-51.  `dispatch` stands in for what the reference's callers do with
    createSource(): makeLibrary + makeComputePipelineState + setBuffer(0...9) +
    setThreadgroupMemoryLength + dispatchThreadgroups (SquareAttentionTest.swift:244-260, :319-368)."""

    def __init__(self, descriptor: AttentionKernelDescriptor):
        self._handle = ctypes.c_void_p()
        c = descriptor._to_c()
        check(lib().mfa_attention_kernel_create(ctypes.byref(c), ctypes.byref(self._handle)))
        self.type = descriptor.type

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value and _abi._lib is not None:   # module globals may be gone at exit
            _abi._lib.mfa_attention_kernel_destroy(h)
            self._handle = ctypes.c_void_p()

    @property
    def blockDimensions(self) -> Tuple[int, int, int]:
        p, t, h = ctypes.c_uint16(), ctypes.c_uint16(), ctypes.c_uint16()
        check(lib().mfa_attention_kernel_block_dimensions(self._handle, ctypes.byref(p), ctypes.byref(t), ctypes.byref(h)))
        return (p.value, t.value, h.value)

    @property
    def threadgroupSize(self) -> int:
        return int(lib().mfa_attention_kernel_threadgroup_size(self._handle))

    @property
    def threadgroupMemoryAllocation(self) -> int:
        return int(lib().mfa_attention_kernel_threadgroup_memory_allocation(self._handle))

    @property
    def variant(self) -> str:
        return lib().mfa_attention_kernel_variant(self._handle).decode()

    @property
    def fallbackVariant(self) -> str:
        """the general code object behind launches the selected variant cannot take ("" if it is the general one)"""
        return lib().mfa_attention_kernel_fallback_variant(self._handle).decode()

    @property
    def needsWorkspaceForFastPath(self) -> bool:
        """transposed operands: the matrix-core kernel runs on row-major copies in the caller's workspace (workspaceSize);
        without a workspace the launch runs `fallbackVariant`"""
        return bool(lib().mfa_attention_kernel_needs_workspace_for_fast_path(self._handle))

    @property
    def effectiveDescriptor(self) -> AttentionKernelDescriptor:
        out = _abi.mfa_attention_kernel_descriptor()
        check(lib().mfa_attention_kernel_effective_descriptor(self._handle, ctypes.byref(out)))
        return AttentionKernelDescriptor._from_c(out)

    # -- launch ------------------------------------------------------------------------------
    @staticmethod
    def _marshal(buffers, row, column, heads, batches, leadingDimensions, headStrides, batchStrides,
                 workspace=None, causal=False, rowLengths=None, columnLengths=None, blockMask=None,
                 blockMaskWords=0, blockMaskStrides=(0, 0), headsPerKeyValue=1):
        """`buffers`: dict {AttentionOperand: tensor | int} or a 10-sequence indexed by bufferBinding."""
        slots = [None] * _abi.MFA_BUFFER_SLOTS
        if isinstance(buffers, Mapping):
            for op, b in buffers.items():
                binding = AttentionOperand(op).bufferBinding
                if binding is None:
                    raise ValueError(f"operand {AttentionOperand(op).description} has no buffer binding")
                slots[binding] = b
        else:
            for i, b in enumerate(buffers):
                slots[i] = b
        arr = (ctypes.c_void_p * _abi.MFA_BUFFER_SLOTS)(*[_pointer(b) for b in slots])
        params = _abi.mfa_launch_params()
        lib().mfa_launch_params_init(ctypes.byref(params))
        params.row, params.column, params.heads, params.batches = int(row), int(column), int(heads), int(batches)
        for name, src in (("leadingDimension", leadingDimensions), ("headStride", headStrides),
                          ("batchStride", batchStrides)):
            if src:
                dst = getattr(params, name)
                for op, v in src.items():
                    dst[AttentionOperand(op).bufferBinding] = int(v)
        params.causal = int(bool(causal))
        # grouped-query attention (extension): query heads per K / V head; K, V, dK, dV strides count K / V heads
        params.headsPerKeyValue = int(headsPerKeyValue)
        # variable sequence lengths (extension): device arrays of `batches` uint32 / int32 entries
        params.rowLengths = _pointer(rowLengths)
        params.columnLengths = _pointer(columnLengths)
        # block-sparse mask (extension): device bitmap, one bit per 256 x 128 block, blockMaskWords words per row block
        params.blockMask = _pointer(blockMask)
        params.blockMaskWords = int(blockMaskWords)
        params.blockMaskHeadStride, params.blockMaskBatchStride = (int(x) for x in blockMaskStrides)
        if workspace is not None:   # caller-owned scratch for column-parallel forward launches
            params.workspace = _pointer(workspace)
            params.workspaceBytes = int(workspace.numel() * workspace.element_size()) \
                if hasattr(workspace, "numel") else int(getattr(workspace, "nbytes"))
        return arr, params, slots

    def workspaceSize(self, *, row: int, column: int, heads: int = 1, batches: int = 1, headsPerKeyValue: int = 1) -> int:
        """Bytes of scratch a launch of this shape would use if given a workspace (0 = the launch fills the GPU without
        splitting the key range).  backwardKeyValue with headsPerKeyValue > 1: the per-query-head dK / dV slabs it requires."""
        params = _abi.mfa_launch_params()
        lib().mfa_launch_params_init(ctypes.byref(params))
        params.row, params.column, params.heads, params.batches = int(row), int(column), int(heads), int(batches)
        params.headsPerKeyValue = int(headsPerKeyValue)
        out = ctypes.c_uint64()
        check(lib().mfa_attention_kernel_workspace_size(self._handle, ctypes.byref(params), ctypes.byref(out)))
        return int(out.value)

    def dispatch(self, buffers, *, row: int, column: int, heads: int = 1, batches: int = 1,
                 leadingDimensions: Optional[Mapping] = None, headStrides: Optional[Mapping] = None,
                 batchStrides: Optional[Mapping] = None, stream: Optional[int] = None,
                 workspace=None, causal: bool = False, rowLengths=None, columnLengths=None, blockMask=None,
                 blockMaskWords: int = 0, blockMaskStrides=(0, 0), headsPerKeyValue: int = 1) -> None:
        arr, params, _keep = self._marshal(buffers, row, column, heads, batches, leadingDimensions,
                                           headStrides, batchStrides, workspace, causal, rowLengths, columnLengths,
                                           blockMask, blockMaskWords, blockMaskStrides, headsPerKeyValue)
        check(lib().mfa_attention_kernel_launch(self._handle, ctypes.byref(arr), ctypes.byref(params),
                                                ctypes.c_void_p(stream or 0)))

    def launchForm(self, buffers, *, row: int, column: int, heads: int = 1, batches: int = 1,
                   leadingDimensions: Optional[Mapping] = None, headStrides: Optional[Mapping] = None,
                   batchStrides: Optional[Mapping] = None, workspace=None, causal: bool = False, rowLengths=None,
                   columnLengths=None, blockMask=None, blockMaskWords: int = 0, blockMaskStrides=(0, 0),
                   headsPerKeyValue: int = 1) -> str:
        """What `dispatch` with the same arguments would run (nothing is launched): the variant's own kernel, the general
        kernel, column-parallel pieces + combine, a re-layout pass in front, or the persistent form `attn_fwd16_p4p` --
        the name rocprofv3 shows for dense / causal forward launches at D <= 128 (mfa_attention_kernel_launch_form)."""
        arr, params, _keep = self._marshal(buffers, row, column, heads, batches, leadingDimensions, headStrides, batchStrides,
                                           workspace, causal, rowLengths, columnLengths, blockMask, blockMaskWords, blockMaskStrides,
                                           headsPerKeyValue)
        out = ctypes.create_string_buffer(512)
        check(lib().mfa_attention_kernel_launch_form(self._handle, ctypes.byref(arr), ctypes.byref(params), out, len(out)))
        return out.value.decode()

    def time(self, buffers, *, row: int, column: int, heads: int = 1, batches: int = 1,
             leadingDimensions: Optional[Mapping] = None, headStrides: Optional[Mapping] = None,
             batchStrides: Optional[Mapping] = None, stream: Optional[int] = None,
             warmup: int = 1, iterations: int = 5, workspace=None, causal: bool = False, headsPerKeyValue: int = 1) -> float:
        """Milliseconds for `iterations` back-to-back launches (HIP events on `stream`)."""
        arr, params, _keep = self._marshal(buffers, row, column, heads, batches, leadingDimensions,
                                           headStrides, batchStrides, workspace, causal, headsPerKeyValue=headsPerKeyValue)
        ms = ctypes.c_float()
        check(lib().mfa_attention_kernel_time(self._handle, ctypes.byref(arr), ctypes.byref(params),
                                              ctypes.c_void_p(stream or 0), int(warmup), int(iterations),
                                              ctypes.byref(ms)))
        return float(ms.value)


def deviceCount() -> int:
    n = ctypes.c_int()
    check(lib().mfa_device_count(ctypes.byref(n)))
    return n.value


def deviceName(device: int = 0) -> str:
    buf = ctypes.create_string_buffer(256)
    check(lib().mfa_device_name(device, buf, len(buf)))
    return buf.value.decode()


def _sinks_block(shape):
    """pops sinkTokens= / sinkLogits= from a launch's keywords -> (mfa_attention_sinks, what it points to), or None when neither is
    given (include/mfa_sink.h: the block is required by the sink entries, so None means the entries without sinks)"""
    tokens, logits = shape.pop("sinkTokens", None), shape.pop("sinkLogits", None)
    if tokens is None and logits is None:
        return None
    block = _abi.mfa_attention_sinks()
    lib().mfa_attention_sinks_init(ctypes.byref(block))
    block.sinkTokens = int(tokens or 0)
    block.sinkLogits = _pointer(logits)
    return block, logits


def _ragged_block(shape):
    """pops rowStarts= / totalRows= from a launch's keywords -> (mfa_ragged_rows, what it points to), or None when neither is given
    (include/mfa_ragged.h: packed rows, the block is required by the ragged entries)"""
    starts, total = shape.pop("rowStarts", None), shape.pop("totalRows", None)
    if starts is None and total is None:
        return None
    block = _abi.mfa_ragged_rows()
    lib().mfa_ragged_rows_init(ctypes.byref(block))
    block.rowStarts = _pointer(starts)
    block.totalRows = int(total or 0)
    return block, starts


def _softcap(shape):
    """pops softcap= from a launch's keywords -> ctypes.c_float, or None when it is not given (include/mfa_softcap.h: 0 goes through the
    soft-cap entries and is the launch without a cap; what the value may be is the library's to say)"""
    cap = shape.pop("softcap", None)
    return None if cap is None else ctypes.c_float(cap)


def _tree_block(shape):
    """pops treeMasks= / treeBatchStride= from a launch's keywords -> (mfa_attention_tree, what it points to), or None when neither is
    given (include/mfa_tree.h: a speculation tree among the new rows, the block is required by the tree entries)"""
    masks, stride = shape.pop("treeMasks", None), shape.pop("treeBatchStride", None)
    if masks is None and stride is None:
        return None
    block = _abi.mfa_attention_tree()
    lib().mfa_attention_tree_init(ctypes.byref(block))
    block.masks = _pointer(masks)
    block.batchStride = int(stride or 0)
    return block, masks


def _split_block(shape):
    """pops workspace= / workspaceBytes= / pieces= from a prefill launch's keywords -> (mfa_key_split, what it points to) (include/mfa_split.h:
    the launch cut along the keys; pieces None or 0: the host's plan, 1: unsplit; no workspace: the unsplit launch)"""
    workspace, nbytes, pieces = shape.pop("workspace", None), shape.pop("workspaceBytes", None), shape.pop("pieces", None)
    block = _abi.mfa_key_split()
    lib().mfa_key_split_init(ctypes.byref(block))
    block.workspace = _pointer(workspace)
    if nbytes is None:
        nbytes = int(workspace.numel() * workspace.element_size()) if hasattr(workspace, "numel") else 0
    block.workspaceBytes, block.pieces = int(nbytes), int(pieces or 0)
    return block, workspace


def _pointers(*buffers):
    return tuple(_pointer(b) for b in buffers)


def _packed(seq, heads, D):
    """(leadingDimension, headStride, batchStride) of a packed [batch][head][row or key][D] operand"""
    return D, int(seq) * D, int(heads) * int(seq) * D


def _packed_rows(heads, D):
    """the same of a ragged batch's packed [row][head][D] operand (include/mfa_ragged.h): no batch axis"""
    return int(heads) * D, D, 0


def _fill_shared(p, D, operands, packed, *, rows, column, heads, batches, cacheLengths, pageSize, blockTable, blockTableStride, strides, pageStrides):
    """the fields mfa_decode_params, mfa_prefill_params, mfa_kv_append_params and mfa_kv_compact_params share.  `operands`: their names in the order of the
    struct's arrays; `packed`: in the same order, the strides of an operand left out of `strides`"""
    p.rows, p.column, p.heads, p.batches, p.headDimension = int(rows), int(column), int(heads), int(batches), D
    p.pageSize, p.cacheLengths = int(pageSize), _pointer(cacheLengths)
    p.blockTable, p.blockTableStride = _pointer(blockTable), int(blockTableStride)
    lds, hss, bss = p.leadingDimension, p.headStride, p.batchStride
    for i, name in enumerate(operands):
        ld, hs, bs = strides.get(name, packed[i]) if strides else packed[i]
        lds[i], hss[i], bss[i] = int(ld), int(hs), int(bs)
    if pageStrides is not None:
        p.pageStride[0], p.pageStride[1] = int(pageStrides[0]), int(pageStrides[1])


_OPTIONS = tuple(_abi.CACHE_OPTION_TYPES)   # quant, window, sinks, ragged, softcap, tree, split: the order every family's signature keeps


def _routes(launch):
    """which options a call gives (a bool per name of _OPTIONS) -> (the entries' name up to the verb, which of _OPTIONS they take; None: none), of the
    first family of _abi.CACHE_FAMILIES[launch] that owns every given option (each family is an earlier one plus an argument); nothing
    for options no family of the launch owns"""
    table = {}
    for given in itertools.product((False, True), repeat=len(_OPTIONS)):
        names = {name for name, g in zip(_OPTIONS, given) if g}
        owners = [(family, own) for family, own in _abi.CACHE_FAMILIES[launch].items() if names <= set(own)]
        if owners:
            family, own = owners[0]
            assert own == tuple(name for name in _OPTIONS if name in own), "a family's arguments keep the order of _OPTIONS"
            table[given] = ("mfa_attention_" + launch + "_" + family, tuple(name in own for name in _OPTIONS) if own else None)
    return table


def _route(routes, quant, window, sinks, ragged, softcap, tree=None, split=None):
    """The entries a launch's options reach (`routes`: _routes of the launch) -> (their name up to the verb, the arguments the family owns).
    Each option is its ctypes argument, or None when the keywords leave it out (window: a number; a window that IS given may be 0).  An
    option that is given needs a family that owns it: a cap wins over all, ragged over window and sinks, either sink keyword reaches the
    sink entries, a window -- 0 too -- the window entries, an e4m3 decode with nothing else fp8_; a tree reaches the tree entries, which
    own neither a cap nor ragged rows; a split block (prefill's workspace= / pieces=) reaches the split entries, which own a window, sinks
    and a tree and neither of those two either.  What the family owns beyond the given options is passed as none: window 0, a NULL block"""
    if split is not None and (softcap is not None or ragged is not None):   # (no split kernel and no entry: said here)
        raise ValueError("a key split (workspace= / pieces=) goes with neither " + ("softcap=" if softcap is not None else "rowStarts= / totalRows=") +
                         ": a soft cap or ragged rows together with a split have no kernel (include/mfa_split.h)")
    if tree is not None and (softcap is not None or ragged is not None):   # (no family owns both: said here, not by the table's KeyError)
        raise ValueError("a speculation tree (treeMasks=) goes with neither " + ("softcap=" if softcap is not None else "rowStarts= / totalRows=") +
                         ": a soft cap or ragged rows together with a tree have no kernel (include/mfa_tree.h)")
    given = (quant, window, sinks, ragged, softcap, tree, split)
    entries, owned = routes[tuple(option is not None for option in given)]
    return entries, itertools.compress((quant, int(window or 0)) + given[2:], owned) if owned else ()


class _CacheAttention:
    """what AttentionDecode and AttentionPrefill share: the call of an entry mfa_attention_<LAUNCH>_<family><verb>, and the methods over it"""

    LAUNCH, ROUTES = None, None   # "decode" / "prefill", and its _routes
    OPERANDS = ("Q", "K", "V", "O")

    def _quant(self, shape):
        """the mfa_kv_quant block of a launch, by reference, and what it points to: none but for decode over an e4m3 cache"""
        return None, None

    def _call(self, verb, shape, head=(), tail=()):
        """mfa_attention_<LAUNCH>_<family><verb>(*head, params, <the family's own arguments>, *tail), the family from the keywords (_route)"""
        # (a launch without options, the common one, pays three membership tests for them)
        window = shape.pop("window", None)
        sinks = _sinks_block(shape) if "sinkTokens" in shape or "sinkLogits" in shape else None
        cap = _softcap(shape) if "softcap" in shape else None
        ragged = _ragged_block(shape) if self.LAUNCH == "prefill" and ("rowStarts" in shape or "totalRows" in shape) else None
        tree = _tree_block(shape) if "treeMasks" in shape or "treeBatchStride" in shape else None
        # (prefill's workspace= / pieces=: the launch cut along the keys, include/mfa_split.h; decode's workspace is part of its params)
        split = _split_block(shape) if self.LAUNCH == "prefill" and ("workspace" in shape or "pieces" in shape) else None
        quant, _scales = self._quant(shape)
        p, _keep = self._params(**shape) if ragged is None else self._params(ragged=ragged, **shape)
        entries, own = _route(self.ROUTES, quant, window, sinks and ctypes.byref(sinks[0]), ragged and ctypes.byref(ragged[0]), cap,
                              tree and ctypes.byref(tree[0]), split and ctypes.byref(split[0]))
        check(getattr(lib(), entries + verb)(*head, ctypes.byref(p), *own, *tail))

    def launchForm(self, **shape) -> str:
        """What `dispatch` with the same arguments would run (nothing is launched): the kernel's name and the grid; decode: the pieces
        kernel, the piece count and the combine kernel, or the single kernel."""
        out = ctypes.create_string_buffer(512)
        self._call("launch_form", shape, tail=(out, len(out)))
        return out.value.decode()

    def dispatch(self, q, k, v, o, l=None, *, stream: Optional[int] = None, **shape) -> None:
        self._call("launch", shape, _pointers(q, k, v, o, l), (ctypes.c_void_p(stream or 0),))

    def time(self, q, k, v, o, l=None, *, stream: Optional[int] = None, warmup: int = 1, iterations: int = 5, **shape) -> float:
        """Milliseconds for `iterations` back-to-back launches (HIP events on `stream`)."""
        ms = ctypes.c_float(0.0)
        self._call("time", shape, _pointers(q, k, v, o, l), (ctypes.c_void_p(stream or 0), int(warmup), int(iterations), ctypes.byref(ms)))
        return float(ms.value)


class AttentionDecode(_CacheAttention):
    """Decode attention over a KV cache (include/mfa_decode.h; an extension, the reference has no such entry): `rows` new query rows
    per sequence against caches of `heads // headsPerKeyValue` K / V heads, per-sequence lengths on the device, contiguous or paged.

        decode = AttentionDecode(headDimension=128, precision=GEMMOperandPrecision.BF16)
        need = decode.workspaceSize(rows=1, column=C, heads=64, batches=B, headsPerKeyValue=8)
        decode.dispatch(q, k, v, o, l, cacheLengths=lengths, rows=1, column=C, heads=64, batches=B, headsPerKeyValue=8,
                        strides=dict(Q=(ld, head, batch), K=..., V=..., O=...), workspace=ws)

    `strides`: operand name -> (leadingDimension, headStride, batchStride) in elements; an operand left out is packed
    ([batch][head][row or key][D]).  Paged caches: pageSize, blockTable (device int32 [batches][blockTableStride]) and
    pageStrides=(K, V); a cache operand's batchStride is then unused.

    window=W (workspaceSize, launchForm, dispatch, time): sliding-window attention, include/mfa_window.h -- row r sees its causal
    frontier and the W - 1 keys before it.  None: the plain launch; 0 goes through the window entries and is the plain launch.

    sinkTokens=S, sinkLogits=device FP32 [heads] (the same four methods): attention sinks, include/mfa_sink.h -- the keys [0, S) stay
    visible under the window (needs window >= 1), and one logit per query head joins the softmax denominator (natural-log units,
    any window).  Either keyword, even 0 / None beside the other, goes through the sink entries.

    softcap=cap (the same four methods): logit soft-capping, include/mfa_softcap.h -- the softmax sees cap tanh(score / cap), cap > 0 in
    natural-log units (Gemma 2: 50).  None: no cap; 0 goes through the soft-cap entries and is the launch without a cap.

    treeMasks=device uint64 [batches][rows] (or [rows] with treeBatchStride=0, one tree for every sequence), treeBatchStride=elements
    (the same four methods): a speculation tree among the new rows, include/mfa_tree.h -- bit j of row r's mask says that the row sees
    new token j; the prefix is seen through the window at the row's depth.  Goes with a window and sinks, not with softcap=."""

    LAUNCH, ROUTES = "decode", _routes("decode")

    def __init__(self, headDimension: int, precision: GEMMOperandPrecision = GEMMOperandPrecision.BF16,
                 outputPrecision: Optional[GEMMOperandPrecision] = None):
        self.headDimension = int(headDimension)
        self.precision = GEMMOperandPrecision(precision)
        self.outputPrecision = self.precision if outputPrecision is None else GEMMOperandPrecision(outputPrecision)

    def _params(self, *, rows: int, column: int, heads: int = 1, batches: int = 1, headsPerKeyValue: int = 1, causal: bool = True,
                lStrides: Optional[Sequence[int]] = None, workspace=None, workspaceBytes: Optional[int] = None, cacheLengths=None,
                pageSize: int = 0, blockTable=None, blockTableStride: int = 0, strides: Optional[Mapping] = None,
                pageStrides: Optional[Sequence[int]] = None):
        p = _abi.mfa_decode_params()
        lib().mfa_decode_params_init(ctypes.byref(p))
        D = self.headDimension
        new, cache = _packed(rows, heads, D), _packed(column, max(1, int(heads) // max(1, int(headsPerKeyValue))), D)
        _fill_shared(p, D, self.OPERANDS, (new, cache, cache, new), rows=rows, column=column, heads=heads, batches=batches, cacheLengths=cacheLengths,
                     pageSize=pageSize, blockTable=blockTable, blockTableStride=blockTableStride, strides=strides, pageStrides=pageStrides)
        p.headsPerKeyValue, p.causal = int(headsPerKeyValue), int(bool(causal))
        p.precision, p.outputPrecision = int(self.precision), int(self.outputPrecision)
        p.lHeadStride, p.lBatchStride = (int(lStrides[0]), int(lStrides[1])) if lStrides is not None else (int(rows), int(heads) * int(rows))
        p.workspace = _pointer(workspace)
        if workspaceBytes is None:
            workspaceBytes = int(workspace.numel() * workspace.element_size()) if hasattr(workspace, "numel") else 0
        p.workspaceBytes = int(workspaceBytes)
        return p, (cacheLengths, blockTable, workspace)

    def workspaceSize(self, **shape) -> int:
        """Bytes a launch of this shape wants to be cut along the keys (0: the plan has one piece).  Without a workspace the launch
        runs unsplit in one kernel."""
        out = ctypes.c_uint64(0)
        self._call("workspace_size", shape, tail=(ctypes.byref(out),))
        return int(out.value)

    @staticmethod
    def pieceRange(length: int, pieces: int, piece: int) -> Tuple[int, int]:
        """keys [begin, end) of piece `piece` of `pieces` for a sequence of `length` keys: the kernels' own function, on the host"""
        b, e = ctypes.c_uint32(0), ctypes.c_uint32(0)
        check(lib().mfa_attention_decode_piece_range(int(length), int(pieces), int(piece), ctypes.byref(b), ctypes.byref(e)))
        return int(b.value), int(e.value)

    @staticmethod
    def windowPieceRange(length: int, rows: int, window: int, pieces: int, piece: int) -> Tuple[int, int]:
        """keys [begin, end) of piece `piece` of `pieces` of a windowed launch (include/mfa_window.h): the kernels' own function"""
        b, e = ctypes.c_uint32(0), ctypes.c_uint32(0)
        check(lib().mfa_attention_decode_window_piece_range(int(length), int(rows), int(window), int(pieces), int(piece), ctypes.byref(b),
                                                            ctypes.byref(e)))
        return int(b.value), int(e.value)

    @staticmethod
    def sinkPieceRange(length: int, rows: int, window: int, sinkTokens: int, pieces: int, piece: int) -> Tuple[Tuple[int, int], Tuple[int, int]]:
        """((begin, end) of the sink tiles, (begin, end) of the window's tiles) of piece `piece` of `pieces` of a launch with sink
        tokens (include/mfa_sink.h): the kernels' own function, on the host"""
        b, e = _abi._U32x2(0, 0), _abi._U32x2(0, 0)
        check(lib().mfa_attention_decode_sink_piece_range(int(length), int(rows), int(window), int(sinkTokens), int(pieces), int(piece),
                                                          ctypes.byref(b), ctypes.byref(e)))
        return (int(b[0]), int(e[0])), (int(b[1]), int(e[1]))


class KVCachePrecision(enum.IntEnum):
    """precision codes of a KV cache beside the 16-bit types (include/mfa_kvcache.h)"""
    E4M3 = _abi.MFA_KV_E4M3
    E5M2 = _abi.MFA_KV_E5M2   # recognised only to be refused


class AttentionDecodeFP8(AttentionDecode):
    """Decode attention over an FP8 (OCP e4m3) KV cache (include/mfa_kvcache.h): AttentionDecode's methods and arguments -- the K / V
    strides count bytes -- plus keyScale / valueScale (device FP32 [heads // headsPerKeyValue], None = 1.0): a cache byte of K / V
    head j stands for scale[j] x e4m3(byte).  `precision` is the 16-bit type of Q."""

    def __init__(self, headDimension: int, precision: GEMMOperandPrecision = GEMMOperandPrecision.BF16,
                 outputPrecision: Optional[GEMMOperandPrecision] = None, cachePrecision: int = KVCachePrecision.E4M3):
        super().__init__(headDimension, precision, outputPrecision)
        self.cachePrecision = int(cachePrecision)

    def _quant(self, shape):
        quant = _abi.mfa_kv_quant()
        lib().mfa_kv_quant_init(ctypes.byref(quant))
        quant.cachePrecision = self.cachePrecision
        keep = (shape.pop("keyScale", None), shape.pop("valueScale", None))
        quant.keyScale, quant.valueScale = _pointer(keep[0]), _pointer(keep[1])
        return ctypes.byref(quant), keep


class AttentionPrefill(_CacheAttention):
    """Prefill attention over a KV cache (include/mfa_prefill.h): a block of up to `rows` new query rows per sequence -- longer than a
    decode step -- against caches of `heads // headsPerKeyValue` K / V heads that already hold the new tokens; per-sequence cache and
    query lengths on the device, contiguous or paged, 16-bit or FP8.

        prefill = AttentionPrefill(headDimension=128, precision=GEMMOperandPrecision.BF16)
        prefill.dispatch(q, k, v, o, l, cacheLengths=lengths, queryLengths=qlens, rows=R, column=C, heads=64, batches=B,
                         headsPerKeyValue=8, strides=dict(Q=(ld, head, batch), K=..., V=..., O=...))

    `strides`, pageSize / blockTable / blockTableStride / pageStrides, lStrides: as AttentionDecode.  cachePrecision=
    KVCachePrecision.E4M3 reads an e4m3 cache (the quantisation block is part of mfa_prefill_params, so one class serves both): the
    K / V strides then count bytes, and keyScale / valueScale (device FP32 [heads // headsPerKeyValue], None = 1.0) go with the shape
    arguments.  The launch takes no workspace unless it is cut along the keys (below).  window=W (launchForm, dispatch, time): sliding-window attention,
    include/mfa_window.h; None: the plain launch; 0 goes through the window entries and is the plain launch.  sinkTokens=S,
    sinkLogits=device FP32 [heads] (the same three): attention sinks as AttentionDecode's, include/mfa_sink.h.

    rowStarts=device uint32 [batches + 1], totalRows=T (the same three): a RAGGED batch, include/mfa_ragged.h -- q, o [T, heads, D] and
    l [heads, T] packed along the rows, sequence b owning the rows rowStarts[b] .. rowStarts[b + 1]; `rows` is then the largest row
    count of a sequence, queryLengths must stay None and Q / O / L have no batch stride (operands left out of `strides` are taken as
    contiguous [T, heads, D]).  Goes through the ragged entries whichever window and sinks.

    softcap=cap (the same three, ragged included): logit soft-capping as AttentionDecode's, include/mfa_softcap.h.

    treeMasks= / treeBatchStride= (the same three; rows <= 64, not ragged, no softcap): a speculation tree as AttentionDecode's,
    include/mfa_tree.h; treeTileRange gives the tiles every row block of a sequence then walks.

    workspace=device buffer / pieces=P (the same three, and workspaceSize; not ragged, no softcap): the launch CUT ALONG THE KEYS,
    include/mfa_split.h -- each row block's tiles in P pieces (None or 0: the host's plan; 1: unsplit; 2 .. 64: as given) that publish
    partial results to the workspace, and a combine kernel.  Either keyword goes through the split entries, with any window, sinks and
    tree; without a workspace the launch runs unsplit.  workspaceSize(pieces=...) gives the bytes, plannedSplit the piece count too,
    pieceRange the tiles of a piece.  A launch that gives neither keyword is the launch it always was."""

    LAUNCH, ROUTES = "prefill", _routes("prefill")

    def __init__(self, headDimension: int, precision: GEMMOperandPrecision = GEMMOperandPrecision.BF16,
                 outputPrecision: Optional[GEMMOperandPrecision] = None, cachePrecision: Optional[int] = None):
        self.headDimension = int(headDimension)
        self.precision = GEMMOperandPrecision(precision)
        self.outputPrecision = self.precision if outputPrecision is None else GEMMOperandPrecision(outputPrecision)
        self.cachePrecision = int(self.precision) if cachePrecision is None else int(cachePrecision)

    def _params(self, *, rows: int, column: int, heads: int = 1, batches: int = 1, headsPerKeyValue: int = 1, causal: bool = True,
                queryLengths=None, lStrides: Optional[Sequence[int]] = None, keyScale=None, valueScale=None, ragged=None, cacheLengths=None,
                pageSize: int = 0, blockTable=None, blockTableStride: int = 0, strides: Optional[Mapping] = None,
                pageStrides: Optional[Sequence[int]] = None):
        p = _abi.mfa_prefill_params()
        lib().mfa_prefill_params_init(ctypes.byref(p))
        D, kvHeads = self.headDimension, max(1, int(heads) // max(1, int(headsPerKeyValue)))
        new, cache = _packed_rows(heads, D) if ragged else _packed(rows, heads, D), _packed(int(pageSize) or column, kvHeads, D)
        if pageStrides is None and pageSize:
            pageStrides = (kvHeads * int(pageSize) * D,) * 2
        _fill_shared(p, D, self.OPERANDS, (new, cache, cache, new), rows=rows, column=column, heads=heads, batches=batches,
                     cacheLengths=cacheLengths, pageSize=pageSize, blockTable=blockTable, blockTableStride=blockTableStride, strides=strides,
                     pageStrides=pageStrides)
        p.headsPerKeyValue, p.causal = int(headsPerKeyValue), int(bool(causal))
        p.precision, p.outputPrecision, p.cachePrecision = int(self.precision), int(self.outputPrecision), self.cachePrecision
        p.queryLengths = _pointer(queryLengths)
        if lStrides is not None:
            p.lHeadStride, p.lBatchStride = int(lStrides[0]), int(lStrides[1])
        elif ragged:
            p.lHeadStride, p.lBatchStride = int(ragged[0].totalRows), 0
        else:
            p.lHeadStride, p.lBatchStride = int(rows), int(heads) * int(rows)
        p.keyScale, p.valueScale = _pointer(keyScale), _pointer(valueScale)
        return p, (cacheLengths, queryLengths, blockTable, keyScale, valueScale)

    @staticmethod
    def tileRange(length: int, queryLength: int, firstRow: int, blockRows: int, causal: bool = True) -> Tuple[int, int]:
        """(first_masked, end) of the block of rows [firstRow, firstRow + blockRows) of a sequence of `length` keys and `queryLength`
        rows, in 64-key tiles: the kernels' own function, on the host"""
        f, e = ctypes.c_uint32(0), ctypes.c_uint32(0)
        check(lib().mfa_attention_prefill_tile_range(int(length), int(queryLength), int(firstRow), int(blockRows), int(bool(causal)),
                                                     ctypes.byref(f), ctypes.byref(e)))
        return int(f.value), int(e.value)

    @staticmethod
    def windowTileRange(length: int, queryLength: int, firstRow: int, blockRows: int, window: int) -> Tuple[int, int, int, int]:
        """(begin, unmaskedBegin, unmaskedEnd, end) of the block of rows [firstRow, firstRow + blockRows) under a window of `window`
        keys, in 64-key tiles (include/mfa_window.h): the kernels' own function, on the host"""
        out = [ctypes.c_uint32(0) for _ in range(4)]
        check(lib().mfa_attention_prefill_window_tile_range(int(length), int(queryLength), int(firstRow), int(blockRows), int(window),
                                                            *(ctypes.byref(x) for x in out)))
        return tuple(int(x.value) for x in out)

    @staticmethod
    def sinkTileRange(length: int, queryLength: int, firstRow: int, blockRows: int, window: int, sinkTokens: int,
                      causal: bool = True) -> Tuple[int, int, int, int, int]:
        """(begin, unmaskedBegin, unmaskedEnd, end, sinkEnd) of the block of rows [firstRow, firstRow + blockRows) under a window of
        `window` keys (0: none) with `sinkTokens` sink keys, in 64-key tiles (include/mfa_sink.h): the tiles [0, sinkEnd) are walked
        first, then [begin, end).  The kernels' own function, on the host"""
        out = [ctypes.c_uint32(0) for _ in range(5)]
        check(lib().mfa_attention_prefill_sink_tile_range(int(length), int(queryLength), int(firstRow), int(blockRows), int(bool(causal)),
                                                          int(window), int(sinkTokens), *(ctypes.byref(x) for x in out)))
        return tuple(int(x.value) for x in out)


    @staticmethod
    def treeTileRange(length: int, queryLength: int, window: int = 0, sinkTokens: int = 0) -> Tuple[int, int, int, int, int]:
        """(begin, unmaskedBegin, unmaskedEnd, end, sinkEnd) of EVERY row block of a sequence of `length` keys and `queryLength` rows under
        a speculation tree (include/mfa_tree.h), in 64-key tiles: the kernels' own function, on the host"""
        out = [ctypes.c_uint32(0) for _ in range(5)]
        check(lib().mfa_attention_prefill_tree_tile_range(int(length), int(queryLength), int(window), int(sinkTokens),
                                                          *(ctypes.byref(x) for x in out)))
        return tuple(int(x.value) for x in out)

    def workspaceSize(self, **shape) -> int:
        """Bytes a launch of this shape needs to run cut along the keys in `pieces` pieces (None or 0: the host's plan); 0: one piece
        (include/mfa_split.h).  Without a workspace the launch runs unsplit in one kernel."""
        return self.plannedSplit(**shape)[0]

    def plannedSplit(self, **shape) -> Tuple[int, int]:
        """(workspace bytes, pieces) of workspaceSize's launch: the piece count the host planned, or the one given"""
        shape.setdefault("pieces", None)
        nbytes, pieces = ctypes.c_uint64(0), ctypes.c_uint32(0)
        self._call("workspace_size", shape, tail=(ctypes.byref(nbytes), ctypes.byref(pieces)))
        return int(nbytes.value), int(pieces.value)

    @staticmethod
    def pieceRange(beginTile: int, endTile: int, sinkEnd: int, pieces: int, piece: int) -> Tuple[Tuple[int, int], Tuple[int, int]]:
        """((begin, end) inside the sink tiles, (begin, end) inside [beginTile, endTile)) of piece `piece` of `pieces` of a row block whose
        walked list is the tiles [0, sinkEnd) ++ [beginTile, endTile) -- three of the five indices of sinkTileRange / treeTileRange
        (include/mfa_split.h): the kernels' own function, on the host"""
        b, e = _abi._U32x2(0, 0), _abi._U32x2(0, 0)
        check(lib().mfa_attention_prefill_split_piece_range(int(beginTile), int(endTile), int(sinkEnd), int(pieces), int(piece),
                                                            ctypes.byref(b), ctypes.byref(e)))
        return (int(b[0]), int(e[0])), (int(b[1]), int(e[1]))

    @staticmethod
    def raggedSlots(totalRows: int, batches: int, rows: int, blockRows: int) -> int:
        """the slots of a ragged launch (include/mfa_ragged.h): min(totalRows // blockRows + batches, batches x ceil(rows / blockRows));
        its grid is that many times the K/V heads"""
        out = ctypes.c_uint64(0)
        check(lib().mfa_attention_prefill_ragged_slots(int(totalRows), int(batches), int(rows), int(blockRows), ctypes.byref(out)))
        return int(out.value)

    @staticmethod
    def raggedBlock(rowStarts: Sequence[int], totalRows: int, rows: int, blockRows: int, slot: int) -> Tuple[Optional[int], int]:
        """(sequence, firstRow) of the row block that slot `slot` of a ragged launch serves, from HOST row starts [batches + 1]; (None, 0):
        a slot past the last row block.  The kernels' own function, on the host"""
        starts = (ctypes.c_uint32 * len(rowStarts))(*[int(x) for x in rowStarts])
        seq, first = ctypes.c_uint32(0), ctypes.c_uint32(0)
        check(lib().mfa_attention_prefill_ragged_block(starts, len(rowStarts) - 1, int(totalRows), int(rows), int(blockRows), int(slot),
                                                       ctypes.byref(seq), ctypes.byref(first)))
        return (None if seq.value == 0xFFFFFFFF else int(seq.value)), int(first.value)


class KVCacheAppend:
    """Appends the `rows` new key / value rows of every sequence to a KV cache (include/mfa_kvcache.h), quantising them to e4m3 when
    the cache is FP8 (cachePrecision=KVCachePrecision.E4M3) or copying their bits when it is the rows' 16-bit type (None).

        append = KVCacheAppend(128, GEMMOperandPrecision.BF16, KVCachePrecision.E4M3)
        append.dispatch(k_new, v_new, k_cache, v_cache, rows=1, heads=8, batches=B, column=C, cacheLengths=lengths, keyScale=ks, valueScale=vs)

    cacheLengths already includes the new rows: row r of sequence b goes to key cacheLengths[b] - rows + r.  `strides`: operand name
    (kNew, vNew, kCache, vCache) -> (leadingDimension, headStride, batchStride) in elements; an operand left out is packed
    ([batch][head][row or key][D]).  Paged caches: pageSize, blockTable, blockTableStride and pageStrides=(K, V).

    rowStarts=device uint32 [batches + 1], totalRows=T: a RAGGED batch, include/mfa_ragged.h -- kNew, vNew [T, heads, D] packed along the
    rows (left out of `strides`: contiguous), sequence b owning the rows rowStarts[b] .. rowStarts[b + 1], at most `rows` of them."""

    OPERANDS = ("kNew", "vNew", "kCache", "vCache")

    def __init__(self, headDimension: int, precision: GEMMOperandPrecision = GEMMOperandPrecision.BF16, cachePrecision: Optional[int] = None):
        self.headDimension = int(headDimension)
        self.precision = GEMMOperandPrecision(precision)
        self.cachePrecision = int(self.precision) if cachePrecision is None else int(cachePrecision)

    def _params(self, *, rows: int, heads: int, batches: int = 1, column: int = 0, keyScale=None, valueScale=None, ragged=None,
                cacheLengths=None, pageSize: int = 0, blockTable=None, blockTableStride: int = 0, strides: Optional[Mapping] = None,
                pageStrides: Optional[Sequence[int]] = None):
        p = _abi.mfa_kv_append_params()
        lib().mfa_kv_append_params_init(ctypes.byref(p))
        D = self.headDimension
        new, cache = _packed_rows(heads, D) if ragged else _packed(rows, heads, D), _packed(int(pageSize) or column, heads, D)
        _fill_shared(p, D, self.OPERANDS, (new, new, cache, cache), rows=rows, column=column, heads=heads, batches=batches,
                     cacheLengths=cacheLengths, pageSize=pageSize, blockTable=blockTable, blockTableStride=blockTableStride, strides=strides,
                     pageStrides=pageStrides)
        p.precision, p.cachePrecision = int(self.precision), self.cachePrecision
        p.keyScale, p.valueScale = _pointer(keyScale), _pointer(valueScale)
        return p

    def dispatch(self, kNew, vNew, kCache, vCache, *, stream: Optional[int] = None, **shape) -> None:
        """mfa_kv_cache_append_launch, or with rowStarts / totalRows mfa_kv_cache_append_ragged_launch, which takes the ragged block
        after the params"""
        ragged = _ragged_block(shape)
        p = self._params(ragged=ragged, **shape)
        family, own = ("", ()) if ragged is None else ("ragged_", (ctypes.byref(ragged[0]),))
        check(getattr(lib(), "mfa_kv_cache_append_" + family + "launch")(*_pointers(kNew, vNew, kCache, vCache), ctypes.byref(p), *own,
                                                                         ctypes.c_void_p(stream or 0)))


class KVCacheCompact:
    """Moves the K and V rows of the accepted path of a speculation tree to the front of the tree's slots, in place, and writes the
    lengths the sequences then have (include/mfa_compact.h): what follows a tree launch, before the next append.

        compact = KVCacheCompact(128, KVCachePrecision.E4M3)
        compact.dispatch(k_cache, v_cache, rows=R, heads=8, batches=B, column=C, cacheLengths=lengths, accepted=path, acceptedStride=R,
                         acceptedCounts=counts, maxAccepted=R, newLengths=new_lengths)

    cachePrecision: the cache's 16-bit type (GEMMOperandPrecision) or KVCachePrecision.E4M3 -- only the bytes of a row matter.
    cacheLengths includes the `rows` tree rows, as the append and the tree launch took it; node j sits at key cacheLengths[b] - rows + j.
    accepted: device int32 [batches][acceptedStride], node indices in path order; acceptedCounts: device uint32 [batches]; newLengths:
    device uint32 [batches] or None.  `strides`: operand name (kCache, vCache) -> (leadingDimension, headStride, batchStride) in
    elements; an operand left out is packed ([batch][head][key][D]).  Paged caches: pageSize, blockTable, blockTableStride and
    pageStrides=(K, V)."""

    OPERANDS = ("kCache", "vCache")

    def __init__(self, headDimension: int, cachePrecision: int = GEMMOperandPrecision.BF16):
        self.headDimension = int(headDimension)
        self.cachePrecision = int(cachePrecision)

    def _params(self, *, rows: int, heads: int, batches: int = 1, column: int = 0, cacheLengths=None, queryLengths=None, accepted=None,
                acceptedStride: Optional[int] = None, acceptedCounts=None, maxAccepted: Optional[int] = None, newLengths=None, pageSize: int = 0,
                blockTable=None, blockTableStride: int = 0, strides: Optional[Mapping] = None, pageStrides: Optional[Sequence[int]] = None):
        p = _abi.mfa_kv_compact_params()
        lib().mfa_kv_compact_params_init(ctypes.byref(p))
        D = self.headDimension
        cache = _packed(int(pageSize) or column, heads, D)
        _fill_shared(p, D, self.OPERANDS, (cache, cache), rows=rows, column=column, heads=heads, batches=batches, cacheLengths=cacheLengths,
                     pageSize=pageSize, blockTable=blockTable, blockTableStride=blockTableStride, strides=strides, pageStrides=pageStrides)
        p.cachePrecision, p.queryLengths = self.cachePrecision, _pointer(queryLengths)
        p.maxAccepted = int(rows if maxAccepted is None else maxAccepted)
        p.accepted, p.acceptedStride = _pointer(accepted), int(p.maxAccepted if acceptedStride is None else acceptedStride)
        p.acceptedCounts, p.newLengths = _pointer(acceptedCounts), _pointer(newLengths)
        return p

    def dispatch(self, kCache, vCache, *, stream: Optional[int] = None, **shape) -> None:
        """mfa_kv_cache_compact_launch"""
        p = self._params(**shape)
        check(lib().mfa_kv_cache_compact_launch(*_pointers(kCache, vCache), ctypes.byref(p), ctypes.c_void_p(stream or 0)))


class AttentionMLADecode:
    """Multi-head latent attention decode over a compressed KV cache (include/mfa_mla.h): `rows` new query rows per sequence and head,
    q [batches][heads][rows][576], against ONE cache row of 576 values per key -- all of them the key, the first 512 the value --
    shared by every head; o [batches][heads][rows][512].  The softmax scale is the model's own and must be given.

        mla = AttentionMLADecode(GEMMOperandPrecision.BF16)
        need, pieces = mla.plannedSplit(rows=1, column=C, heads=128, batches=B, scale=s)
        mla.dispatch(q, kv, o, l, cacheLengths=lengths, rows=1, column=C, heads=128, batches=B, scale=s, workspace=ws)

    `strides`: operand name (Q, KV, O) -> (leadingDimension, headStride, batchStride) in elements; an operand left out is packed (the
    cache: [batch][key][576], head stride unused).  Paged caches: pageSize, blockTable (device int32 [batches][blockTableStride]) and
    pageStride (default pageSize x the cache's leadingDimension).  pieces: None or 0 is the host's plan, 1 unsplit, 2 .. 64 as given;
    without a workspace the launch runs unsplit.  Stands alone, as KVCacheCompact: no option families."""

    OPERANDS = ("Q", "KV", "O")
    HEAD_DIMENSION, VALUE_DIMENSION = _abi.MFA_MLA_HEAD_DIMENSION, _abi.MFA_MLA_VALUE_DIMENSION

    def __init__(self, precision: GEMMOperandPrecision = GEMMOperandPrecision.BF16, outputPrecision: Optional[GEMMOperandPrecision] = None,
                 headDimension: int = _abi.MFA_MLA_HEAD_DIMENSION, valueDimension: int = _abi.MFA_MLA_VALUE_DIMENSION):
        self.precision = GEMMOperandPrecision(precision)
        self.outputPrecision = self.precision if outputPrecision is None else GEMMOperandPrecision(outputPrecision)
        self.headDimension, self.valueDimension = int(headDimension), int(valueDimension)

    def _params(self, *, rows: int, column: int, scale: float, heads: int = 1, batches: int = 1, causal: bool = True, pieces: Optional[int] = None,
                lStrides: Optional[Sequence[int]] = None, workspace=None, workspaceBytes: Optional[int] = None, cacheLengths=None,
                pageSize: int = 0, blockTable=None, blockTableStride: int = 0, strides: Optional[Mapping] = None,
                pageStride: Optional[int] = None):
        p = _abi.mfa_mla_decode_params()
        lib().mfa_mla_decode_params_init(ctypes.byref(p))
        Dk, Dv = self.headDimension, self.valueDimension
        p.rows, p.column, p.heads, p.batches = int(rows), int(column), int(heads), int(batches)
        p.headDimension, p.valueDimension, p.causal, p.scale, p.pieces = Dk, Dv, int(bool(causal)), float(scale), int(pieces or 0)
        p.precision, p.outputPrecision = int(self.precision), int(self.outputPrecision)
        p.pageSize, p.cacheLengths = int(pageSize), _pointer(cacheLengths)
        p.blockTable, p.blockTableStride = _pointer(blockTable), int(blockTableStride)
        packed = (_packed(rows, heads, Dk), (Dk, 0, int(column) * Dk), _packed(rows, heads, Dv))
        for i, name in enumerate(self.OPERANDS):
            ld, hs, bs = strides.get(name, packed[i]) if strides else packed[i]
            p.leadingDimension[i], p.headStride[i], p.batchStride[i] = int(ld), int(hs), int(bs)
        p.pageStride = int(pageStride) if pageStride is not None else int(pageSize) * int(p.leadingDimension[1])
        p.lHeadStride, p.lBatchStride = (int(lStrides[0]), int(lStrides[1])) if lStrides is not None else (int(rows), int(heads) * int(rows))
        p.workspace = _pointer(workspace)
        if workspaceBytes is None:
            workspaceBytes = int(workspace.numel() * workspace.element_size()) if hasattr(workspace, "numel") else 0
        p.workspaceBytes = int(workspaceBytes)
        return p, (cacheLengths, blockTable, workspace)

    _FAMILY = ""   # the entries are mfa_attention_mla_decode_<family><verb>

    def _own(self, shape):
        """what the family's entries take after the params, taken out of `shape` -> (ctypes arguments, what they point to)"""
        return (), None

    def _entry(self, verb):
        return getattr(lib(), "mfa_attention_mla_decode_" + self._FAMILY + verb)

    def plannedSplit(self, **shape) -> Tuple[int, int]:
        """(workspace bytes, pieces) of a launch of this shape: the piece count the host planned, or the one given; 0 bytes: one piece"""
        own, _kept = self._own(shape)
        p, _keep = self._params(**shape)
        nbytes, pieces = ctypes.c_uint64(0), ctypes.c_uint32(0)
        check(self._entry("workspace_size")(ctypes.byref(p), *own, ctypes.byref(nbytes), ctypes.byref(pieces)))
        return int(nbytes.value), int(pieces.value)

    def workspaceSize(self, **shape) -> int:
        """Bytes a launch of this shape wants to be cut along the keys (0: one piece).  Without a workspace the launch runs unsplit."""
        return self.plannedSplit(**shape)[0]

    def launchForm(self, **shape) -> str:
        """What `dispatch` with the same arguments would run (nothing is launched): the kernels' names, the grid, the piece count"""
        own, _kept = self._own(shape)
        p, _keep = self._params(**shape)
        out = ctypes.create_string_buffer(512)
        check(self._entry("launch_form")(ctypes.byref(p), *own, out, len(out)))
        return out.value.decode()

    def dispatch(self, q, kv, o, l=None, *, stream: Optional[int] = None, **shape) -> None:
        """mfa_attention_mla_decode_launch"""
        own, _kept = self._own(shape)
        p, _keep = self._params(**shape)
        check(self._entry("launch")(*_pointers(q, kv, o, l), ctypes.byref(p), *own, ctypes.c_void_p(stream or 0)))

    def time(self, q, kv, o, l=None, *, stream: Optional[int] = None, warmup: int = 1, iterations: int = 5, **shape) -> float:
        """Milliseconds for `iterations` back-to-back launches (HIP events on `stream`)."""
        own, _kept = self._own(shape)
        p, _keep = self._params(**shape)
        ms = ctypes.c_float(0.0)
        check(self._entry("time")(*_pointers(q, kv, o, l), ctypes.byref(p), *own, ctypes.c_void_p(stream or 0), int(warmup), int(iterations),
                                  ctypes.byref(ms)))
        return float(ms.value)


class AttentionMLADecodeFP8(AttentionMLADecode):
    """MLA decode over an FP8 (OCP e4m3) latent cache (include/mfa_mla_cache.h): AttentionMLADecode's methods and arguments -- the KV
    strides count bytes, multiples of 16 -- plus kvScale (device FP32, one entry, None = 1.0): a cache byte stands for
    kvScale[0] x e4m3(byte), latent and rotary part alike.  `precision` is the 16-bit type of Q.  The workspace and the piece plan are
    AttentionMLADecode's."""

    _FAMILY = "fp8_"

    def __init__(self, precision: GEMMOperandPrecision = GEMMOperandPrecision.BF16, outputPrecision: Optional[GEMMOperandPrecision] = None,
                 cachePrecision: int = KVCachePrecision.E4M3, **widths):
        super().__init__(precision, outputPrecision, **widths)
        self.cachePrecision = int(cachePrecision)

    def _own(self, shape):
        quant = _abi.mfa_mla_quant()
        lib().mfa_mla_quant_init(ctypes.byref(quant))
        quant.cachePrecision = self.cachePrecision
        keep = shape.pop("kvScale", None)
        quant.kvScale = _pointer(keep)
        return (ctypes.byref(quant),), (quant, keep)


class AttentionMLASparseDecode(AttentionMLADecode):
    """Sparse MLA decode (include/mfa_mla_sparse.h): AttentionMLADecode's methods and arguments plus `indices`, device int32
    [batches][rows][topk] -- the key POSITIONS row r of sequence b attends to, shared by all heads -- and `topk`.  -1, a position at or
    past the length and a position past the causal frontier are holes: never loaded, never scored.  indexStrides: (row, batch) in
    entries, default (topk, rows x topk).  The workspace formula is AttentionMLADecode's; the pieces are pieces of the list's slots, and
    plannedSplit / workspaceSize plan over `topk`, not over `column`.

        mla = AttentionMLASparseDecode(GEMMOperandPrecision.BF16)
        need, pieces = mla.plannedSplit(rows=1, column=C, heads=128, batches=B, scale=s, indices=idx, topk=2048)
        mla.dispatch(q, kv, o, l, cacheLengths=lengths, rows=1, column=C, heads=128, batches=B, scale=s, indices=idx, topk=2048, workspace=ws)
    """

    def _own(self, shape):
        sparse = _abi.mfa_mla_sparse()
        lib().mfa_mla_sparse_init(ctypes.byref(sparse))
        keep = shape.pop("indices", None)
        topk = int(shape.pop("topk", 0))
        strides = shape.pop("indexStrides", None)
        sparse.indices, sparse.topk = _pointer(keep), topk
        sparse.indexRowStride, sparse.indexBatchStride = (int(strides[0]), int(strides[1])) if strides is not None else (topk, int(shape.get("rows", 0)) * topk)
        return (ctypes.byref(sparse),), (sparse, keep)

    def _entry(self, verb):
        return getattr(lib(), "mfa_attention_mla_sparse_decode_" + verb)

    def launch(self, q, kv, o, l=None, **shape) -> None:
        """mfa_attention_mla_sparse_decode_launch (`dispatch` under the name the header uses)"""
        self.dispatch(q, kv, o, l, **shape)


class AttentionMLASparseDecodeFP8(AttentionMLASparseDecode):
    """Sparse MLA decode over an FP8 (OCP e4m3) latent cache (include/mfa_mla_sparse_fp8.h): AttentionMLASparseDecode's methods and
    arguments -- the KV strides count bytes, multiples of 16 -- plus kvScale (device FP32, one entry, None = 1.0): a cache byte stands
    for kvScale[0] x e4m3(byte).  `precision` is the 16-bit type of Q.  The workspace and the piece plan are AttentionMLASparseDecode's.

        mla = AttentionMLASparseDecodeFP8(GEMMOperandPrecision.BF16)
        mla.dispatch(q, kv8, o, l, cacheLengths=lengths, rows=1, column=C, heads=128, batches=B, scale=s, indices=idx, topk=2048,
                     kvScale=kv_scale, workspace=ws)
    """

    def __init__(self, precision: GEMMOperandPrecision = GEMMOperandPrecision.BF16, outputPrecision: Optional[GEMMOperandPrecision] = None,
                 cachePrecision: int = KVCachePrecision.E4M3, **widths):
        super().__init__(precision, outputPrecision, **widths)
        self.cachePrecision = int(cachePrecision)

    def _own(self, shape):
        sparse, keptSparse = super()._own(shape)
        quant = _abi.mfa_mla_quant()
        lib().mfa_mla_quant_init(ctypes.byref(quant))
        quant.cachePrecision = self.cachePrecision
        keep = shape.pop("kvScale", None)
        quant.kvScale = _pointer(keep)
        return sparse + (ctypes.byref(quant),), (keptSparse, quant, keep)

    def _entry(self, verb):
        return getattr(lib(), "mfa_attention_mla_sparse_decode_fp8_" + verb)


class AttentionMLAPrefill:
    """Multi-head latent attention prefill over the compressed KV cache (include/mfa_mla_prefill.h): a block of `rows` new query rows per
    sequence and head, of any length, q [batches][heads][rows][576], against the cache rows AttentionMLADecode reads;
    o [batches][heads][rows][512].  Sequence b uses its first queryLengths[b] rows (device uint32, None: `rows`); the others are neither
    read nor written.  The softmax scale is the model's own and must be given.

        mla = AttentionMLAPrefill(GEMMOperandPrecision.BF16)
        mla.dispatch(q, kv, o, l, cacheLengths=lengths, queryLengths=new, rows=512, column=C, heads=128, batches=B, scale=s)

    `strides`, pageSize, blockTable and pageStride as AttentionMLADecode takes them: a token-major q / o is a plain launch.  The launch
    is not cut along the keys: no pieces, no workspace, no plannedSplit."""

    OPERANDS = ("Q", "KV", "O")
    HEAD_DIMENSION, VALUE_DIMENSION = _abi.MFA_MLA_HEAD_DIMENSION, _abi.MFA_MLA_VALUE_DIMENSION
    PACKED_ROWS, KEY_STEP = _abi.MFA_MLA_PREFILL_PACKED_ROWS, _abi.MFA_MLA_PREFILL_KEY_STEP

    def __init__(self, precision: GEMMOperandPrecision = GEMMOperandPrecision.BF16, outputPrecision: Optional[GEMMOperandPrecision] = None,
                 headDimension: int = _abi.MFA_MLA_HEAD_DIMENSION, valueDimension: int = _abi.MFA_MLA_VALUE_DIMENSION):
        self.precision = GEMMOperandPrecision(precision)
        self.outputPrecision = self.precision if outputPrecision is None else GEMMOperandPrecision(outputPrecision)
        self.headDimension, self.valueDimension = int(headDimension), int(valueDimension)

    def _params(self, *, rows: int, column: int, scale: float, heads: int = 1, batches: int = 1, causal: bool = True,
                lStrides: Optional[Sequence[int]] = None, cacheLengths=None, queryLengths=None, pageSize: int = 0, blockTable=None,
                blockTableStride: int = 0, strides: Optional[Mapping] = None, pageStride: Optional[int] = None):
        p = _abi.mfa_mla_prefill_params()
        lib().mfa_mla_prefill_params_init(ctypes.byref(p))
        Dk, Dv = self.headDimension, self.valueDimension
        p.rows, p.column, p.heads, p.batches = int(rows), int(column), int(heads), int(batches)
        p.headDimension, p.valueDimension, p.causal, p.scale = Dk, Dv, int(bool(causal)), float(scale)
        p.precision, p.outputPrecision = int(self.precision), int(self.outputPrecision)
        p.pageSize, p.cacheLengths, p.queryLengths = int(pageSize), _pointer(cacheLengths), _pointer(queryLengths)
        p.blockTable, p.blockTableStride = _pointer(blockTable), int(blockTableStride)
        packed = (_packed(rows, heads, Dk), (Dk, 0, int(column) * Dk), _packed(rows, heads, Dv))
        for i, name in enumerate(self.OPERANDS):
            ld, hs, bs = strides.get(name, packed[i]) if strides else packed[i]
            p.leadingDimension[i], p.headStride[i], p.batchStride[i] = int(ld), int(hs), int(bs)
        p.pageStride = int(pageStride) if pageStride is not None else int(pageSize) * int(p.leadingDimension[1])
        p.lHeadStride, p.lBatchStride = (int(lStrides[0]), int(lStrides[1])) if lStrides is not None else (int(rows), int(heads) * int(rows))
        return p, (cacheLengths, queryLengths, blockTable)

    def launchForm(self, **shape) -> str:
        """What `dispatch` with the same arguments would run (nothing is launched): the kernel's name and the grid"""
        p, _keep = self._params(**shape)
        out = ctypes.create_string_buffer(512)
        check(lib().mfa_attention_mla_prefill_launch_form(ctypes.byref(p), out, len(out)))
        return out.value.decode()

    def dispatch(self, q, kv, o, l=None, *, stream: Optional[int] = None, **shape) -> None:
        """mfa_attention_mla_prefill_launch"""
        p, _keep = self._params(**shape)
        check(lib().mfa_attention_mla_prefill_launch(*_pointers(q, kv, o, l), ctypes.byref(p), ctypes.c_void_p(stream or 0)))

    def time(self, q, kv, o, l=None, *, stream: Optional[int] = None, warmup: int = 1, iterations: int = 5, **shape) -> float:
        """Milliseconds for `iterations` back-to-back launches (HIP events on `stream`)."""
        p, _keep = self._params(**shape)
        ms = ctypes.c_float(0.0)
        check(lib().mfa_attention_mla_prefill_time(*_pointers(q, kv, o, l), ctypes.byref(p), ctypes.c_void_p(stream or 0), int(warmup),
                                                   int(iterations), ctypes.byref(ms)))
        return float(ms.value)

    @staticmethod
    def stepRange(length: int, queryLength: int, firstPacked: int, heads: int, causal: bool = True) -> Tuple[int, int]:
        """mfa_attention_mla_prefill_step_range -> (firstMasked, end), in 32-key steps: the kernels' own range function for the block of
        the 64 packed rows from `firstPacked` (p = row x heads + head)"""
        first, end = ctypes.c_uint32(0), ctypes.c_uint32(0)
        check(lib().mfa_attention_mla_prefill_step_range(int(length), int(queryLength), int(firstPacked), int(heads), int(bool(causal)),
                                                         ctypes.byref(first), ctypes.byref(end)))
        return int(first.value), int(end.value)


class MLACacheAppend:
    """Appends the `rows` new rows of every sequence to the latent cache of MLA decode (include/mfa_mla_cache.h) -- latentNew
    [batches][rows][512] and ropeNew [batches][rows][64] become one cache row of 576 -- quantising them to e4m3 when the cache is FP8
    (cachePrecision=KVCachePrecision.E4M3, kvScale: device FP32, one entry, None = 1.0) or copying their bits when it is the rows'
    16-bit type (None).

        append = MLACacheAppend(GEMMOperandPrecision.BF16, KVCachePrecision.E4M3)
        append.dispatch(latent_new, rope_new, kv_cache, rows=1, batches=B, column=C, cacheLengths=lengths, kvScale=scale)

    cacheLengths already includes the new rows: row r of sequence b goes to key cacheLengths[b] - rows + r.  `strides`: operand name
    (latentNew, ropeNew, kvCache) -> (leadingDimension, batchStride) in elements; an operand left out is packed.  Paged caches:
    pageSize, blockTable, blockTableStride and pageStride (default pageSize x the cache's leadingDimension)."""

    OPERANDS = ("latentNew", "ropeNew", "kvCache")
    LATENT_DIMENSION, ROPE_DIMENSION = _abi.MFA_MLA_LATENT_DIMENSION, _abi.MFA_MLA_ROPE_DIMENSION

    def __init__(self, precision: GEMMOperandPrecision = GEMMOperandPrecision.BF16, cachePrecision: Optional[int] = None,
                 latentDimension: int = _abi.MFA_MLA_LATENT_DIMENSION, ropeDimension: int = _abi.MFA_MLA_ROPE_DIMENSION):
        self.precision = GEMMOperandPrecision(precision)
        self.cachePrecision = int(self.precision) if cachePrecision is None else int(cachePrecision)
        self.latentDimension, self.ropeDimension = int(latentDimension), int(ropeDimension)

    def _params(self, *, rows: int, batches: int = 1, column: int = 0, kvScale=None, cacheLengths=None, pageSize: int = 0, blockTable=None,
                blockTableStride: int = 0, strides: Optional[Mapping] = None, pageStride: Optional[int] = None):
        p = _abi.mfa_mla_append_params()
        lib().mfa_mla_append_params_init(ctypes.byref(p))
        Dl, Dr = self.latentDimension, self.ropeDimension
        p.rows, p.batches, p.column, p.pageSize = int(rows), int(batches), int(column), int(pageSize)
        p.latentDimension, p.ropeDimension, p.precision, p.cachePrecision = Dl, Dr, int(self.precision), self.cachePrecision
        p.cacheLengths, p.blockTable, p.blockTableStride = _pointer(cacheLengths), _pointer(blockTable), int(blockTableStride)
        packed = ((Dl, int(rows) * Dl), (Dr, int(rows) * Dr), (Dl + Dr, int(column) * (Dl + Dr)))
        for i, name in enumerate(self.OPERANDS):
            ld, bs = strides.get(name, packed[i]) if strides else packed[i]
            p.leadingDimension[i], p.batchStride[i] = int(ld), int(bs)
        p.pageStride = int(pageStride) if pageStride is not None else int(pageSize) * int(p.leadingDimension[2])
        p.kvScale = _pointer(kvScale)
        return p

    def dispatch(self, latentNew, ropeNew, kvCache, *, stream: Optional[int] = None, **shape) -> None:
        """mfa_mla_cache_append_launch"""
        p = self._params(**shape)
        check(lib().mfa_mla_cache_append_launch(*_pointers(latentNew, ropeNew, kvCache), ctypes.byref(p), ctypes.c_void_p(stream or 0)))


def quantizeE4M3(x: float, scale: float = 1.0) -> int:
    """the cache byte of `x` under `scale`: mfa_kv_quantize_e4m3, the contract of writer and reader"""
    return int(lib().mfa_kv_quantize_e4m3(float(x), float(scale)))


def dequantizeE4M3(byte: int) -> float:
    return float(lib().mfa_kv_dequantize_e4m3(int(byte)))
