"""ctypes declarations for include/mfa.h (the C-ABI drop-in boundary).

The product path FAILS LOUDLY when the HIP library is missing: there is no CPU or PyTorch
fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MFA_LIBRARY: developer tools (tools/ab_*.py) point this at libmfa_hip_dev.so, the -DMFA_DEV_VARIANTS build that carries
# the A/B knobs; it only chooses WHICH build of the same C ABI is loaded -- there is no fallback either way.
LIB_PATH = os.environ.get("MFA_LIBRARY") or os.path.join(_HERE, "libmfa_hip.so")

MFA_OPERAND_COUNT = 14
MFA_BUFFER_SLOTS = 10

MFA_OK = 0
STATUS_NAMES = {
    0: "MFA_OK",
    1: "MFA_ERR_INCOMPLETE_DESCRIPTOR",
    2: "MFA_ERR_INVALID_ARGUMENT",
    3: "MFA_ERR_UNSUPPORTED",
    4: "MFA_ERR_HIP",
    5: "MFA_ERR_PARSE",
}


class mfa_attention_descriptor(ctypes.Structure):
    _fields_ = [
        ("lowPrecisionInputs", ctypes.c_uint8),
        ("lowPrecisionIntermediates", ctypes.c_uint8),
        ("hasMatrixDimensions", ctypes.c_uint8),
        ("hasTransposeState", ctypes.c_uint8),
        ("row", ctypes.c_uint32),
        ("column", ctypes.c_uint32),
        ("head", ctypes.c_uint16),
        ("transposeQ", ctypes.c_uint8),
        ("transposeK", ctypes.c_uint8),
        ("transposeV", ctypes.c_uint8),
        ("transposeO", ctypes.c_uint8),
        ("lowPrecisionInputType", ctypes.c_uint8),
        ("lowPrecisionOutputs", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8 * 2),
    ]


class mfa_attention_kernel_descriptor(ctypes.Structure):
    _fields_ = [
        ("hasBlockDimensions", ctypes.c_uint8),
        ("hasHeadDimension", ctypes.c_uint8),
        ("parallelization", ctypes.c_uint16),
        ("traversal", ctypes.c_uint16),
        ("headBlock", ctypes.c_uint16),
        ("headDimension", ctypes.c_uint16),
        ("cacheState", ctypes.c_int8 * MFA_OPERAND_COUNT),
        ("memoryPrecisions", ctypes.c_int8 * MFA_OPERAND_COUNT),
        ("registerPrecisions", ctypes.c_int8 * MFA_OPERAND_COUNT),
        ("transposeState", ctypes.c_int8 * MFA_OPERAND_COUNT),
        ("preferAsyncCache", ctypes.c_int8),
        ("preferAsyncLoad", ctypes.c_int8),
        ("type", ctypes.c_int8),
        ("strictBlockDimensions", ctypes.c_int8),
    ]


class mfa_parameter_row(ctypes.Structure):
    _fields_ = [
        ("maximumHeadDimension", ctypes.c_uint16),
        ("parallelization", ctypes.c_uint16),
        ("traversal", ctypes.c_uint16),
        ("head", ctypes.c_uint16),
        ("cached", ctypes.c_int8 * MFA_OPERAND_COUNT),
    ]


class mfa_launch_params(ctypes.Structure):
    _fields_ = [
        ("row", ctypes.c_uint32),
        ("column", ctypes.c_uint32),
        ("heads", ctypes.c_uint32),
        ("batches", ctypes.c_uint32),
        ("leadingDimension", ctypes.c_int64 * MFA_BUFFER_SLOTS),
        ("headStride", ctypes.c_int64 * MFA_BUFFER_SLOTS),
        ("batchStride", ctypes.c_int64 * MFA_BUFFER_SLOTS),
        ("workspace", ctypes.c_void_p),
        ("workspaceBytes", ctypes.c_uint64),
        ("causal", ctypes.c_uint32),
        ("headsPerKeyValue", ctypes.c_uint32),
        ("rowLengths", ctypes.c_void_p),
        ("columnLengths", ctypes.c_void_p),
        ("blockMask", ctypes.c_void_p),
        ("blockMaskWords", ctypes.c_uint32),
        ("reserved2", ctypes.c_uint32),
        ("blockMaskHeadStride", ctypes.c_int64),
        ("blockMaskBatchStride", ctypes.c_int64),
    ]

MFA_MASK_BLOCK_ROWS, MFA_MASK_BLOCK_COLUMNS = 256, 128


# every symbol include/mfa.h declares: (name, restype, argtypes)
_P = ctypes.POINTER
_KERNEL = ctypes.c_void_p
_BUFS = ctypes.c_void_p * MFA_BUFFER_SLOTS
class mfa_gemm_descriptor(ctypes.Structure):   # include/mfa_gemm.h
    _fields_ = [
        ("batchDimension", ctypes.c_uint32),
        ("hasLeadingDimensions", ctypes.c_uint8), ("loadPreviousC", ctypes.c_uint8),
        ("hasMatrixDimensions", ctypes.c_uint8), ("hasMemoryPrecisions", ctypes.c_uint8),
        ("hasTransposeState", ctypes.c_uint8), ("transposeA", ctypes.c_uint8), ("transposeB", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8),
        ("leadingDimensionA", ctypes.c_uint32), ("leadingDimensionB", ctypes.c_uint32), ("leadingDimensionC", ctypes.c_uint32),
        ("M", ctypes.c_uint32), ("N", ctypes.c_uint32), ("K", ctypes.c_uint32),
        ("precisionA", ctypes.c_int32), ("precisionB", ctypes.c_int32), ("precisionC", ctypes.c_int32),
    ]


class mfa_gemm_kernel_descriptor(ctypes.Structure):
    _fields_ = [
        ("blockM", ctypes.c_uint16), ("blockN", ctypes.c_uint16), ("blockK", ctypes.c_uint16),
        ("leadingBlockA", ctypes.c_uint16), ("leadingBlockB", ctypes.c_uint16), ("leadingBlockC", ctypes.c_uint16),
        ("memoryPrecisionA", ctypes.c_int32), ("memoryPrecisionB", ctypes.c_int32), ("memoryPrecisionC", ctypes.c_int32),
        ("registerPrecisionA", ctypes.c_int32), ("registerPrecisionB", ctypes.c_int32), ("registerPrecisionC", ctypes.c_int32),
        ("splitsM", ctypes.c_uint16), ("splitsN", ctypes.c_uint16),
        ("preferAsyncLoad", ctypes.c_uint8), ("preferAsyncStore", ctypes.c_uint8),
        ("transposeA", ctypes.c_uint8), ("transposeB", ctypes.c_uint8),
        ("complete", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 3),
    ]


class mfa_gemm_launch_params(ctypes.Structure):
    _fields_ = [
        ("M", ctypes.c_uint32), ("N", ctypes.c_uint32), ("K", ctypes.c_uint32),
        ("leadingDimensionA", ctypes.c_uint32), ("leadingDimensionB", ctypes.c_uint32), ("leadingDimensionC", ctypes.c_uint32),
        ("loadPreviousC", ctypes.c_uint32), ("batchDimension", ctypes.c_uint32),
        ("batchStrideA", ctypes.c_uint64), ("batchStrideB", ctypes.c_uint64), ("batchStrideC", ctypes.c_uint64),
    ]


_GEMM = ctypes.c_void_p

GEMM_SYMBOLS = [
    ("mfa_gemm_descriptor_init", None, [ctypes.POINTER(mfa_gemm_descriptor)]),
    ("mfa_gemm_launch_params_init", None, [ctypes.POINTER(mfa_gemm_launch_params)]),
    ("mfa_gemm_descriptor_kernel_descriptor", ctypes.c_int,
     [ctypes.POINTER(mfa_gemm_descriptor), ctypes.POINTER(mfa_gemm_kernel_descriptor)]),
    ("mfa_gemm_kernel_create", ctypes.c_int, [ctypes.POINTER(mfa_gemm_kernel_descriptor), ctypes.POINTER(_GEMM)]),
    ("mfa_gemm_kernel_destroy", None, [_GEMM]),
    ("mfa_gemm_kernel_block_dimensions", ctypes.c_int,
     [_GEMM, ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint16)]),
    ("mfa_gemm_kernel_threadgroup_size", ctypes.c_uint32, [_GEMM]),
    ("mfa_gemm_kernel_threadgroup_memory_allocation", ctypes.c_uint32, [_GEMM]),
    ("mfa_gemm_kernel_variant", ctypes.c_char_p, [_GEMM]),
    ("mfa_gemm_kernel_launch", ctypes.c_int,
     [_GEMM, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(mfa_gemm_launch_params), ctypes.c_void_p]),
    ("mfa_gemm_kernel_launch_form", ctypes.c_char_p,
     [_GEMM, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(mfa_gemm_launch_params)]),
    ("mfa_gemm_kernel_time", ctypes.c_int,
     [_GEMM, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(mfa_gemm_launch_params), ctypes.c_void_p,
      ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
]

class mfa_decode_params(ctypes.Structure):   # include/mfa_decode.h
    _fields_ = [
        ("rows", ctypes.c_uint32), ("column", ctypes.c_uint32), ("heads", ctypes.c_uint32), ("batches", ctypes.c_uint32),
        ("headsPerKeyValue", ctypes.c_uint32), ("causal", ctypes.c_uint32),
        ("headDimension", ctypes.c_uint16), ("precision", ctypes.c_uint8), ("outputPrecision", ctypes.c_uint8),
        ("pageSize", ctypes.c_uint32),
        ("cacheLengths", ctypes.c_void_p), ("blockTable", ctypes.c_void_p), ("blockTableStride", ctypes.c_int64),
        ("leadingDimension", ctypes.c_int64 * 4), ("headStride", ctypes.c_int64 * 4), ("batchStride", ctypes.c_int64 * 4),
        ("pageStride", ctypes.c_int64 * 2),
        ("lHeadStride", ctypes.c_int64), ("lBatchStride", ctypes.c_int64),
        ("workspace", ctypes.c_void_p), ("workspaceBytes", ctypes.c_uint64),
    ]


MFA_DECODE_KEY_TILE, MFA_DECODE_MAX_PACKED_ROWS, MFA_DECODE_WORKGROUP_TARGET, MFA_DECODE_MAX_PIECES = 64, 32, 512, 64
_DECODE_BUFS = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

DECODE_SYMBOLS = [   # + its mfa_attention_*_{workspace_size,launch,launch_form,time} rows: the CACHE_FAMILIES loop below
    ("mfa_decode_params_init", None, [ctypes.POINTER(mfa_decode_params)]),
    ("mfa_attention_decode_piece_range", ctypes.c_int,
     [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]),
]

class mfa_kv_append_params(ctypes.Structure):   # include/mfa_kvcache.h
    _fields_ = [
        ("rows", ctypes.c_uint32), ("heads", ctypes.c_uint32), ("batches", ctypes.c_uint32), ("column", ctypes.c_uint32),
        ("headDimension", ctypes.c_uint16), ("precision", ctypes.c_uint8), ("cachePrecision", ctypes.c_uint8),
        ("pageSize", ctypes.c_uint32),
        ("cacheLengths", ctypes.c_void_p), ("blockTable", ctypes.c_void_p), ("blockTableStride", ctypes.c_int64),
        ("leadingDimension", ctypes.c_int64 * 4), ("headStride", ctypes.c_int64 * 4), ("batchStride", ctypes.c_int64 * 4),
        ("pageStride", ctypes.c_int64 * 2),
        ("keyScale", ctypes.c_void_p), ("valueScale", ctypes.c_void_p),
    ]


class mfa_kv_quant(ctypes.Structure):   # include/mfa_kvcache.h
    _fields_ = [("cachePrecision", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("keyScale", ctypes.c_void_p), ("valueScale", ctypes.c_void_p)]


MFA_KV_E4M3, MFA_KV_E5M2 = 16, 17
_QUANT = ctypes.POINTER(mfa_kv_quant)

KVCACHE_SYMBOLS = [   # + its mfa_attention_*_{workspace_size,launch,launch_form,time} rows: the CACHE_FAMILIES loop below
    ("mfa_kv_quantize_e4m3", ctypes.c_uint8, [ctypes.c_float, ctypes.c_float]),
    ("mfa_kv_dequantize_e4m3", ctypes.c_float, [ctypes.c_uint8]),
    ("mfa_kv_append_params_init", None, [ctypes.POINTER(mfa_kv_append_params)]),
    ("mfa_kv_cache_append_launch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(mfa_kv_append_params), ctypes.c_void_p]),
    ("mfa_kv_quant_init", None, [_QUANT]),
]

class mfa_prefill_params(ctypes.Structure):   # include/mfa_prefill.h
    _fields_ = [
        ("rows", ctypes.c_uint32), ("column", ctypes.c_uint32), ("heads", ctypes.c_uint32), ("batches", ctypes.c_uint32),
        ("headsPerKeyValue", ctypes.c_uint32), ("causal", ctypes.c_uint32),
        ("headDimension", ctypes.c_uint16), ("precision", ctypes.c_uint8), ("outputPrecision", ctypes.c_uint8),
        ("pageSize", ctypes.c_uint32),
        ("cacheLengths", ctypes.c_void_p), ("queryLengths", ctypes.c_void_p), ("blockTable", ctypes.c_void_p),
        ("blockTableStride", ctypes.c_int64),
        ("leadingDimension", ctypes.c_int64 * 4), ("headStride", ctypes.c_int64 * 4), ("batchStride", ctypes.c_int64 * 4),
        ("pageStride", ctypes.c_int64 * 2),
        ("lHeadStride", ctypes.c_int64), ("lBatchStride", ctypes.c_int64),
        ("cachePrecision", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
        ("keyScale", ctypes.c_void_p), ("valueScale", ctypes.c_void_p),
    ]


MFA_PREFILL_KEY_TILE, MFA_PREFILL_PACKED_ROWS, MFA_PREFILL_MAX_GROUP = 64, 128, 32
_PREFILL = ctypes.POINTER(mfa_prefill_params)
_U32P = ctypes.POINTER(ctypes.c_uint32)

PREFILL_SYMBOLS = [   # + its mfa_attention_*_{workspace_size,launch,launch_form,time} rows: the CACHE_FAMILIES loop below
    ("mfa_prefill_params_init", None, [_PREFILL]),
    ("mfa_prefill_params_size", ctypes.c_size_t, []),
    ("mfa_prefill_params_offsets", ctypes.c_int, [_U32P, ctypes.c_uint32, _U32P]),
    ("mfa_attention_prefill_tile_range", ctypes.c_int,
     [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _U32P, _U32P]),
]

_DECODE = ctypes.POINTER(mfa_decode_params)
_TIMING = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]

WINDOW_SYMBOLS = [   # include/mfa_window.h: `window` (uint32, 0 = none) after `quant` (decode; NULL: a 16-bit cache) / `params` (prefill)
    # + its mfa_attention_*_{workspace_size,launch,launch_form,time} rows: the CACHE_FAMILIES loop below
    ("mfa_attention_decode_window_piece_range", ctypes.c_int,
     [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _U32P, _U32P]),
    ("mfa_attention_prefill_window_tile_range", ctypes.c_int,
     [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _U32P, _U32P, _U32P, _U32P]),
]

class mfa_attention_sinks(ctypes.Structure):   # include/mfa_sink.h
    _fields_ = [("sinkTokens", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("sinkLogits", ctypes.c_void_p)]


_SINKS = ctypes.POINTER(mfa_attention_sinks)
_U32x2 = ctypes.c_uint32 * 2

SINK_SYMBOLS = [   # include/mfa_sink.h: `sinks` (required) after `window` (0 = none)
    # + its mfa_attention_*_{workspace_size,launch,launch_form,time} rows: the CACHE_FAMILIES loop below
    ("mfa_attention_sinks_init", None, [_SINKS]),
    ("mfa_attention_sinks_size", ctypes.c_size_t, []),
    ("mfa_attention_sinks_offsets", ctypes.c_int, [_U32P, ctypes.c_uint32, _U32P]),
    ("mfa_attention_decode_sink_piece_range", ctypes.c_int,
     [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_U32x2),
      ctypes.POINTER(_U32x2)]),
    ("mfa_attention_prefill_sink_tile_range", ctypes.c_int, [ctypes.c_uint32] * 7 + [_U32P] * 5),
]

class mfa_ragged_rows(ctypes.Structure):   # include/mfa_ragged.h
    _fields_ = [("rowStarts", ctypes.c_void_p), ("totalRows", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


_RAGGED = ctypes.POINTER(mfa_ragged_rows)

RAGGED_SYMBOLS = [   # include/mfa_ragged.h: `ragged` (required) after `sinks` (NULL = none)
    # + its mfa_attention_*_{workspace_size,launch,launch_form,time} rows: the CACHE_FAMILIES loop below
    ("mfa_ragged_rows_init", None, [_RAGGED]),
    ("mfa_ragged_rows_size", ctypes.c_size_t, []),
    ("mfa_ragged_rows_offsets", ctypes.c_int, [_U32P, ctypes.c_uint32, _U32P]),
    ("mfa_attention_prefill_ragged_slots", ctypes.c_int, [ctypes.c_uint32] * 4 + [ctypes.POINTER(ctypes.c_uint64)]),
    ("mfa_attention_prefill_ragged_block", ctypes.c_int, [_U32P] + [ctypes.c_uint32] * 5 + [_U32P, _U32P]),
    ("mfa_kv_cache_append_ragged_launch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(mfa_kv_append_params), _RAGGED, ctypes.c_void_p]),
]

SOFTCAP_SYMBOLS = []   # include/mfa_softcap.h: `softcap` (float, 0 = none) after `sinks` (NULL = none) / after `ragged`
   #    all of it mfa_attention_*_{workspace_size,launch,launch_form,time} rows: the CACHE_FAMILIES loop below

class mfa_attention_tree(ctypes.Structure):   # include/mfa_tree.h
    _fields_ = [("masks", ctypes.c_void_p), ("batchStride", ctypes.c_int64), ("reserved", ctypes.c_uint64)]


_TREE = ctypes.POINTER(mfa_attention_tree)
MFA_TREE_MAX_NODES = 64

TREE_SYMBOLS = [   # include/mfa_tree.h: `tree` (required) after `sinks` (NULL = none)
    # + its mfa_attention_*_{workspace_size,launch,launch_form,time} rows: the CACHE_FAMILIES loop below
    ("mfa_attention_tree_init", None, [_TREE]),
    ("mfa_attention_tree_size", ctypes.c_size_t, []),
    ("mfa_attention_tree_offsets", ctypes.c_int, [_U32P, ctypes.c_uint32, _U32P]),
    ("mfa_attention_prefill_tree_tile_range", ctypes.c_int, [ctypes.c_uint32] * 4 + [_U32P] * 5),
]

class mfa_key_split(ctypes.Structure):   # include/mfa_split.h
    _fields_ = [("workspace", ctypes.c_void_p), ("workspaceBytes", ctypes.c_uint64), ("pieces", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


_SPLIT = ctypes.POINTER(mfa_key_split)
MFA_PREFILL_SPLIT_MAX_PIECES, MFA_PREFILL_SPLIT_MIN_TILES, MFA_PREFILL_SPLIT_COMPUTE_UNITS = 64, 8, 256

SPLIT_SYMBOLS = [   # include/mfa_split.h: prefill cut along the keys -- `split` (required) after `tree` (NULL = none): the tree family plus an argument
    # + its mfa_attention_*_{launch,launch_form,time} rows and, this family's alone, workspace_size with its second result: the CACHE_FAMILIES loop below
    ("mfa_key_split_init", None, [_SPLIT]),
    ("mfa_key_split_size", ctypes.c_size_t, []),
    ("mfa_key_split_offsets", ctypes.c_int, [_U32P, ctypes.c_uint32, _U32P]),
    ("mfa_attention_prefill_split_piece_range", ctypes.c_int, [ctypes.c_uint32] * 5 + [ctypes.POINTER(_U32x2), ctypes.POINTER(_U32x2)]),
]

class mfa_kv_compact_params(ctypes.Structure):   # include/mfa_compact.h
    _fields_ = [
        ("rows", ctypes.c_uint32), ("heads", ctypes.c_uint32), ("batches", ctypes.c_uint32), ("column", ctypes.c_uint32),
        ("headDimension", ctypes.c_uint16), ("cachePrecision", ctypes.c_uint8), ("reserved", ctypes.c_uint8),
        ("pageSize", ctypes.c_uint32),
        ("cacheLengths", ctypes.c_void_p), ("queryLengths", ctypes.c_void_p), ("blockTable", ctypes.c_void_p), ("blockTableStride", ctypes.c_int64),
        ("accepted", ctypes.c_void_p), ("acceptedStride", ctypes.c_int64), ("acceptedCounts", ctypes.c_void_p),
        ("maxAccepted", ctypes.c_uint32), ("reserved2", ctypes.c_uint32), ("newLengths", ctypes.c_void_p),
        ("leadingDimension", ctypes.c_int64 * 2), ("headStride", ctypes.c_int64 * 2), ("batchStride", ctypes.c_int64 * 2),
        ("pageStride", ctypes.c_int64 * 2),
    ]


_COMPACT = ctypes.POINTER(mfa_kv_compact_params)

COMPACT_SYMBOLS = [   # include/mfa_compact.h: the accepted path of a speculation tree moved to the front of the tree's slots
    ("mfa_kv_compact_params_init", None, [_COMPACT]),
    ("mfa_kv_compact_params_size", ctypes.c_size_t, []),
    ("mfa_kv_compact_params_offsets", ctypes.c_int, [_U32P, ctypes.c_uint32, _U32P]),
    ("mfa_kv_cache_compact_launch", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, _COMPACT, ctypes.c_void_p]),
]

class mfa_mla_decode_params(ctypes.Structure):   # include/mfa_mla.h
    _fields_ = [
        ("rows", ctypes.c_uint32), ("column", ctypes.c_uint32), ("heads", ctypes.c_uint32), ("batches", ctypes.c_uint32),
        ("causal", ctypes.c_uint32),
        ("headDimension", ctypes.c_uint16), ("valueDimension", ctypes.c_uint16),
        ("precision", ctypes.c_uint8), ("outputPrecision", ctypes.c_uint8), ("reserved", ctypes.c_uint16),
        ("scale", ctypes.c_float), ("pageSize", ctypes.c_uint32), ("pieces", ctypes.c_uint32),
        ("cacheLengths", ctypes.c_void_p), ("blockTable", ctypes.c_void_p), ("blockTableStride", ctypes.c_int64),
        ("leadingDimension", ctypes.c_int64 * 3), ("headStride", ctypes.c_int64 * 3), ("batchStride", ctypes.c_int64 * 3),
        ("pageStride", ctypes.c_int64),
        ("lHeadStride", ctypes.c_int64), ("lBatchStride", ctypes.c_int64),
        ("workspace", ctypes.c_void_p), ("workspaceBytes", ctypes.c_uint64),
    ]


_MLA = ctypes.POINTER(mfa_mla_decode_params)
MFA_MLA_HEAD_DIMENSION, MFA_MLA_VALUE_DIMENSION, MFA_MLA_PACKED_ROWS = 576, 512, 32
_MLA_BUFS = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]   # q, kv, o, l

MLA_SYMBOLS = [   # include/mfa_mla.h: multi-head latent attention decode over a compressed KV cache; an entry of its own, no family
    ("mfa_mla_decode_params_init", None, [_MLA]),
    ("mfa_mla_decode_params_size", ctypes.c_size_t, []),
    ("mfa_mla_decode_params_offsets", ctypes.c_int, [_U32P, ctypes.c_uint32, _U32P]),
    ("mfa_attention_mla_decode_workspace_size", ctypes.c_int, [_MLA, ctypes.POINTER(ctypes.c_uint64), _U32P]),
    ("mfa_attention_mla_decode_launch", ctypes.c_int, _MLA_BUFS + [_MLA, ctypes.c_void_p]),
    ("mfa_attention_mla_decode_launch_form", ctypes.c_int, [_MLA, ctypes.c_char_p, ctypes.c_size_t]),
    ("mfa_attention_mla_decode_time", ctypes.c_int, _MLA_BUFS + [_MLA, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
]

class mfa_mla_append_params(ctypes.Structure):   # include/mfa_mla_cache.h
    _fields_ = [
        ("rows", ctypes.c_uint32), ("batches", ctypes.c_uint32), ("column", ctypes.c_uint32), ("pageSize", ctypes.c_uint32),
        ("latentDimension", ctypes.c_uint16), ("ropeDimension", ctypes.c_uint16),
        ("precision", ctypes.c_uint8), ("cachePrecision", ctypes.c_uint8), ("reserved", ctypes.c_uint16),
        ("cacheLengths", ctypes.c_void_p), ("blockTable", ctypes.c_void_p), ("blockTableStride", ctypes.c_int64),
        ("leadingDimension", ctypes.c_int64 * 3), ("batchStride", ctypes.c_int64 * 3),
        ("pageStride", ctypes.c_int64),
        ("kvScale", ctypes.c_void_p),
    ]


class mfa_mla_quant(ctypes.Structure):   # include/mfa_mla_cache.h
    _fields_ = [("cachePrecision", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("kvScale", ctypes.c_void_p)]


_MLA_APPEND, _MLA_QUANT = ctypes.POINTER(mfa_mla_append_params), ctypes.POINTER(mfa_mla_quant)
MFA_MLA_LATENT_DIMENSION, MFA_MLA_ROPE_DIMENSION = 512, 64

MLA_CACHE_SYMBOLS = [   # include/mfa_mla_cache.h: the latent cache's append, and MLA decode over an e4m3 latent cache (`quant` after `params`)
    ("mfa_mla_append_params_init", None, [_MLA_APPEND]),
    ("mfa_mla_append_params_size", ctypes.c_size_t, []),
    ("mfa_mla_append_params_offsets", ctypes.c_int, [_U32P, ctypes.c_uint32, _U32P]),
    ("mfa_mla_cache_append_launch", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _MLA_APPEND, ctypes.c_void_p]),
    ("mfa_mla_quant_init", None, [_MLA_QUANT]),
    ("mfa_attention_mla_decode_fp8_workspace_size", ctypes.c_int, [_MLA, _MLA_QUANT, ctypes.POINTER(ctypes.c_uint64), _U32P]),
    ("mfa_attention_mla_decode_fp8_launch", ctypes.c_int, _MLA_BUFS + [_MLA, _MLA_QUANT, ctypes.c_void_p]),
    ("mfa_attention_mla_decode_fp8_launch_form", ctypes.c_int, [_MLA, _MLA_QUANT, ctypes.c_char_p, ctypes.c_size_t]),
    ("mfa_attention_mla_decode_fp8_time", ctypes.c_int,
     _MLA_BUFS + [_MLA, _MLA_QUANT, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
]

class mfa_mla_sparse(ctypes.Structure):   # include/mfa_mla_sparse.h
    _fields_ = [("indices", ctypes.c_void_p), ("topk", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("indexRowStride", ctypes.c_int64), ("indexBatchStride", ctypes.c_int64)]


_MLA_SPARSE = ctypes.POINTER(mfa_mla_sparse)

MLA_SPARSE_SYMBOLS = [   # include/mfa_mla_sparse.h: MLA decode over per-row lists of key positions (`sparse` after `params`)
    ("mfa_mla_sparse_init", None, [_MLA_SPARSE]),
    ("mfa_mla_sparse_size", ctypes.c_size_t, []),
    ("mfa_mla_sparse_offsets", ctypes.c_int, [_U32P, ctypes.c_uint32, _U32P]),
    ("mfa_attention_mla_sparse_decode_workspace_size", ctypes.c_int, [_MLA, _MLA_SPARSE, ctypes.POINTER(ctypes.c_uint64), _U32P]),
    ("mfa_attention_mla_sparse_decode_launch", ctypes.c_int, _MLA_BUFS + [_MLA, _MLA_SPARSE, ctypes.c_void_p]),
    ("mfa_attention_mla_sparse_decode_launch_form", ctypes.c_int, [_MLA, _MLA_SPARSE, ctypes.c_char_p, ctypes.c_size_t]),
    ("mfa_attention_mla_sparse_decode_time", ctypes.c_int,
     _MLA_BUFS + [_MLA, _MLA_SPARSE, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
]

MLA_SPARSE_FP8_SYMBOLS = [   # include/mfa_mla_sparse_fp8.h: the sparse entries over an e4m3 latent cache (`sparse`, then `quant`, after `params`)
    ("mfa_attention_mla_sparse_decode_fp8_workspace_size", ctypes.c_int, [_MLA, _MLA_SPARSE, _MLA_QUANT, ctypes.POINTER(ctypes.c_uint64), _U32P]),
    ("mfa_attention_mla_sparse_decode_fp8_launch", ctypes.c_int, _MLA_BUFS + [_MLA, _MLA_SPARSE, _MLA_QUANT, ctypes.c_void_p]),
    ("mfa_attention_mla_sparse_decode_fp8_launch_form", ctypes.c_int, [_MLA, _MLA_SPARSE, _MLA_QUANT, ctypes.c_char_p, ctypes.c_size_t]),
    ("mfa_attention_mla_sparse_decode_fp8_time", ctypes.c_int,
     _MLA_BUFS + [_MLA, _MLA_SPARSE, _MLA_QUANT, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
]

class mfa_mla_prefill_params(ctypes.Structure):   # include/mfa_mla_prefill.h
    _fields_ = [
        ("rows", ctypes.c_uint32), ("column", ctypes.c_uint32), ("heads", ctypes.c_uint32), ("batches", ctypes.c_uint32),
        ("causal", ctypes.c_uint32),
        ("headDimension", ctypes.c_uint16), ("valueDimension", ctypes.c_uint16),
        ("precision", ctypes.c_uint8), ("outputPrecision", ctypes.c_uint8), ("reserved", ctypes.c_uint16),
        ("scale", ctypes.c_float), ("pageSize", ctypes.c_uint32),
        ("cacheLengths", ctypes.c_void_p), ("queryLengths", ctypes.c_void_p), ("blockTable", ctypes.c_void_p),
        ("blockTableStride", ctypes.c_int64),
        ("leadingDimension", ctypes.c_int64 * 3), ("headStride", ctypes.c_int64 * 3), ("batchStride", ctypes.c_int64 * 3),
        ("pageStride", ctypes.c_int64),
        ("lHeadStride", ctypes.c_int64), ("lBatchStride", ctypes.c_int64),
    ]


_MLA_PREFILL = ctypes.POINTER(mfa_mla_prefill_params)
MFA_MLA_PREFILL_PACKED_ROWS, MFA_MLA_PREFILL_KEY_STEP = 64, 32

MLA_PREFILL_SYMBOLS = [   # include/mfa_mla_prefill.h: MLA prefill over the latent cache, row blocks of any length; an entry of its own, no family
    ("mfa_mla_prefill_params_init", None, [_MLA_PREFILL]),
    ("mfa_mla_prefill_params_size", ctypes.c_size_t, []),
    ("mfa_mla_prefill_params_offsets", ctypes.c_int, [_U32P, ctypes.c_uint32, _U32P]),
    ("mfa_attention_mla_prefill_launch", ctypes.c_int, _MLA_BUFS + [_MLA_PREFILL, ctypes.c_void_p]),
    ("mfa_attention_mla_prefill_launch_form", ctypes.c_int, [_MLA_PREFILL, ctypes.c_char_p, ctypes.c_size_t]),
    ("mfa_attention_mla_prefill_time", ctypes.c_int,
     _MLA_BUFS + [_MLA_PREFILL, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    ("mfa_attention_mla_prefill_step_range", ctypes.c_int, [ctypes.c_uint32] * 5 + [_U32P, _U32P]),
]

# ---- the laddered entries of the launches over a KV cache, described once:
#     mfa_attention_<launch>_<family><verb>(*<the verb's head>, params, *<the options the family owns>, *<the verb's tail>)
# CACHE_FAMILIES: launch -> family -> the options its entries take, in the order of their signatures (each family is an earlier one plus an
# argument; attention._route picks the first that owns every option a call gives).  CACHE_VERBS: launch -> verb -> (head, tail);
# CACHE_FAMILY_VERBS: (launch, family) -> the verbs that family alone adds.
CACHE_OPTION_TYPES = {"quant": _QUANT, "window": ctypes.c_uint32, "sinks": _SINKS, "ragged": _RAGGED, "softcap": ctypes.c_float,
                      "tree": _TREE, "split": _SPLIT}
CACHE_FAMILIES = {
    "decode": {"": (), "fp8_": ("quant",), "window_": ("quant", "window"), "sink_": ("quant", "window", "sinks"),
               "softcap_": ("quant", "window", "sinks", "softcap"), "tree_": ("quant", "window", "sinks", "tree")},
    "prefill": {"": (), "window_": ("window",), "sink_": ("window", "sinks"), "ragged_": ("window", "sinks", "ragged"),
                "softcap_": ("window", "sinks", "softcap"), "ragged_softcap_": ("window", "sinks", "ragged", "softcap"),
                "tree_": ("window", "sinks", "tree"), "split_": ("window", "sinks", "tree", "split")},
}
_VERBS = {"workspace_size": ([], [ctypes.POINTER(ctypes.c_uint64)]), "launch": (_DECODE_BUFS, [ctypes.c_void_p]),
          "launch_form": ([], [ctypes.c_char_p, ctypes.c_size_t]), "time": (_DECODE_BUFS, [ctypes.c_void_p] + _TIMING)}
CACHE_VERBS = {"decode": _VERBS, "prefill": {verb: _VERBS[verb] for verb in ("launch", "launch_form", "time")}}
CACHE_FAMILY_VERBS = {("prefill", "split_"): {"workspace_size": ([], [ctypes.POINTER(ctypes.c_uint64), _U32P])}}   # (bytes, pieces)
_CACHE_PARAMS = {"decode": _DECODE, "prefill": _PREFILL}

# (the list of the header that declares each family's entries)
for _symbols, _launch, _family in ((DECODE_SYMBOLS, "decode", ""), (KVCACHE_SYMBOLS, "decode", "fp8_"), (PREFILL_SYMBOLS, "prefill", ""),
                                   (WINDOW_SYMBOLS, "decode", "window_"), (WINDOW_SYMBOLS, "prefill", "window_"),
                                   (SINK_SYMBOLS, "decode", "sink_"), (SINK_SYMBOLS, "prefill", "sink_"), (RAGGED_SYMBOLS, "prefill", "ragged_"),
                                   (SOFTCAP_SYMBOLS, "decode", "softcap_"), (SOFTCAP_SYMBOLS, "prefill", "softcap_"),
                                   (SOFTCAP_SYMBOLS, "prefill", "ragged_softcap_"), (TREE_SYMBOLS, "decode", "tree_"),
                                   (TREE_SYMBOLS, "prefill", "tree_"), (SPLIT_SYMBOLS, "prefill", "split_")):
    _own = [CACHE_OPTION_TYPES[option] for option in CACHE_FAMILIES[_launch][_family]]
    _symbols += [(f"mfa_attention_{_launch}_{_family}{verb}", ctypes.c_int, head + [_CACHE_PARAMS[_launch]] + _own + tail)
                 for verb, (head, tail) in dict(CACHE_VERBS[_launch], **CACHE_FAMILY_VERBS.get((_launch, _family), {})).items()]

SYMBOLS = [
    ("mfa_precision_name", ctypes.c_char_p, [ctypes.c_int]),
    ("mfa_precision_size", ctypes.c_int, [ctypes.c_int]),
    ("mfa_operand_name", ctypes.c_char_p, [ctypes.c_int]),
    ("mfa_operand_buffer_binding", ctypes.c_int, [ctypes.c_int]),
    ("mfa_attention_descriptor_init", None, [_P(mfa_attention_descriptor)]),
    ("mfa_attention_kernel_descriptor_init", None, [_P(mfa_attention_kernel_descriptor)]),
    ("mfa_attention_descriptor_memory_precisions", ctypes.c_int,
     [_P(mfa_attention_descriptor), _P(ctypes.c_int8)]),
    ("mfa_attention_descriptor_register_precisions", ctypes.c_int,
     [_P(mfa_attention_descriptor), _P(ctypes.c_int8)]),
    ("mfa_attention_descriptor_kernel_descriptor", ctypes.c_int,
     [_P(mfa_attention_descriptor), ctypes.c_int, _P(mfa_attention_kernel_descriptor)]),
    ("mfa_parameter_table_get", ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]),
    ("mfa_parameter_table_set", ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_char_p]),
    ("mfa_parameter_table_reset", ctypes.c_int, []),
    ("mfa_parameter_table_select", ctypes.c_int, [ctypes.c_char_p, ctypes.c_uint16, _P(mfa_parameter_row)]),
    ("mfa_attention_kernel_create", ctypes.c_int, [_P(mfa_attention_kernel_descriptor), _P(_KERNEL)]),
    ("mfa_attention_kernel_destroy", None, [_KERNEL]),
    ("mfa_attention_kernel_block_dimensions", ctypes.c_int,
     [_KERNEL, _P(ctypes.c_uint16), _P(ctypes.c_uint16), _P(ctypes.c_uint16)]),
    ("mfa_attention_kernel_threadgroup_size", ctypes.c_uint32, [_KERNEL]),
    ("mfa_attention_kernel_threadgroup_memory_allocation", ctypes.c_uint32, [_KERNEL]),
    ("mfa_attention_kernel_variant", ctypes.c_char_p, [_KERNEL]),
    ("mfa_attention_kernel_fallback_variant", ctypes.c_char_p, [_KERNEL]),
    ("mfa_attention_kernel_needs_workspace_for_fast_path", ctypes.c_int, [_KERNEL]),
    ("mfa_attention_kernel_launch_form", ctypes.c_int, [_KERNEL, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]),
    ("mfa_attention_kernel_effective_descriptor", ctypes.c_int, [_KERNEL, _P(mfa_attention_kernel_descriptor)]),
    ("mfa_launch_params_init", None, [_P(mfa_launch_params)]),
    ("mfa_attention_kernel_launch", ctypes.c_int, [_KERNEL, _P(_BUFS), _P(mfa_launch_params), ctypes.c_void_p]),
    ("mfa_attention_kernel_workspace_size", ctypes.c_int, [_KERNEL, _P(mfa_launch_params), _P(ctypes.c_uint64)]),
    ("mfa_attention_kernel_time", ctypes.c_int,
     [_KERNEL, _P(_BUFS), _P(mfa_launch_params), ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _P(ctypes.c_float)]),
    ("mfa_device_count", ctypes.c_int, [_P(ctypes.c_int)]),
    ("mfa_device_name", ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]),
    ("mfa_last_error_string", ctypes.c_char_p, []),
    ("mfa_abi_version", ctypes.c_int, []),
]

_lib = None
EXPECTED_ABI = 6   # MFA_ABI_VERSION of include/mfa.h this file mirrors


class MFAError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status


def lib() -> ctypes.CDLL:
    """Load libmfa_hip.so.  Raises (never falls back) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C metal_flash_attention_amd/csrc`. There is no fallback path.")
    # PyTorch-ROCm bundles its own libamdhip64.so.7; when a process uses both, torch's copy must be
    # the one that is resident (loading /opt/rocm's first leaves torch with a runtime that reports
    # hipErrorNoDevice).  torch is only plumbing here (device memory, streams): import it first if
    # it is installed, so the C-ABI library binds to the same HIP runtime instance.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    handle = ctypes.CDLL(LIB_PATH)
    # version first: a stale library (the .so is git-ignored and travels separately from the sources) must fail with this
    # message, not with a bare AttributeError on the first symbol it lacks
    handle.mfa_abi_version.restype = ctypes.c_int
    handle.mfa_abi_version.argtypes = []
    got = int(handle.mfa_abi_version())
    if got != EXPECTED_ABI:   # the struct mirrors above describe exactly one layout of mfa_launch_params & co.
        raise ImportError(f"{LIB_PATH} reports ABI version {got}, these bindings were written for {EXPECTED_ABI}: "
                          f"rebuild the library (make -C metal_flash_attention_amd/csrc)")
    for name, restype, argtypes in SYMBOLS + GEMM_SYMBOLS + DECODE_SYMBOLS + KVCACHE_SYMBOLS + PREFILL_SYMBOLS + WINDOW_SYMBOLS + SINK_SYMBOLS + RAGGED_SYMBOLS + SOFTCAP_SYMBOLS + TREE_SYMBOLS + COMPACT_SYMBOLS + SPLIT_SYMBOLS + MLA_SYMBOLS + MLA_CACHE_SYMBOLS + MLA_SPARSE_SYMBOLS + MLA_SPARSE_FP8_SYMBOLS + MLA_PREFILL_SYMBOLS:
        fn = getattr(handle, name)  # AttributeError if the ABI is incomplete
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = handle
    return handle


def library_path() -> str:
    """Path of the C-ABI library these bindings load (bench.py hashes it to tie a PMC profile to a build)."""
    return LIB_PATH


def check(status: int) -> None:
    if status != MFA_OK:
        raise MFAError(status, lib().mfa_last_error_string().decode())
