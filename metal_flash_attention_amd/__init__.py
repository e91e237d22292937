"""metal_flash_attention_amd -- MI355X (gfx950) FlashAttention kernel suite behind the host API
of philipturner/metal-flash-attention.  Hand-written HIP kernels + a C-ABI library
(libmfa_hip.so, include/mfa.h); this package is the thin Python mirror of the Swift types.
No CPU / PyTorch compute fallback exists: importing works without the library, using it raises.
"""
from ._abi import LIB_PATH, MFAError  # noqa: F401
from .attention import (  # noqa: F401
    AttentionDecode,
    AttentionDecodeFP8,
    AttentionDescriptor,
    AttentionKernel,
    AttentionKernelDescriptor,
    AttentionKernelType,
    AttentionMLADecode,
    AttentionMLADecodeFP8,
    AttentionMLAPrefill,
    AttentionMLASparseDecode,
    AttentionMLASparseDecodeFP8,
    AttentionOperand,
    AttentionPrefill,
    GEMMOperandPrecision,
    KVCacheAppend,
    KVCacheCompact,
    KVCachePrecision,
    MLACacheAppend,
    deviceCount,
    deviceName,
    dequantizeE4M3,
    parameterFile,
    quantizeE4M3,
    resetParameterFiles,
    selectParameterRow,
    setParameterFile,
)
from .gemm import GEMMDescriptor, GEMMKernel, GEMMKernelDescriptor  # noqa: F401,E402


def __getattr__(name):
    # the torch functions of the KV-cache loop, on first use: torch stays optional for everything above
    if name in ("kv_cache_compact", "tree_path", "flash_mla_decode", "flash_mla_decode_fp8", "mla_cache_append", "flash_mla_sparse_decode",
                "flash_mla_sparse_decode_fp8", "flash_mla_prefill"):
        from . import torch_binding
        return getattr(torch_binding, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
