"""PyTorch-ROCm binding of the three attention kernels (the "caller" layer the
reference does not have -- only its tests call the kernels, Tests/FlashAttentionTests/Attention/*.swift).

    from metal_flash_attention_amd.torch_binding import flash_attention
    o = flash_attention(q, k, v, causal=False)      # q [B, H, R, D], k / v [B, Hkv, C, D] (H % Hkv == 0); bf16, fp16 or fp32
    o.sum().backward()                              # dQ, dK, dV through backwardQuery / backwardKeyValue

    from metal_flash_attention_amd.torch_binding import flash_attention_op   # the same through torch.library ops
    f = torch.compile(lambda q, k, v: flash_attention_op(q, k, v, causal=True), fullgraph=True)

    from metal_flash_attention_amd.torch_binding import flash_decode          # token-by-token generation over a KV cache
    o = flash_decode(q, k_cache, v_cache, cache_lengths)                      # q [B, H, R, D], R = 1 or a few; forward only

    from metal_flash_attention_amd.torch_binding import kv_cache_append       # write the new tokens' K / V rows, in place
    kv_cache_append(k_new, v_new, k_cache, v_cache, cache_lengths, k_scale=ks, v_scale=vs)   # float8_e4m3fn or 16-bit caches
    o = flash_decode(q, k_cache, v_cache, cache_lengths, k_scale=ks, v_scale=vs)

forward  = AttentionKernelType.forward           -> O (the inputs' dtype, fused cast), L (fp32), both saved
backward = AttentionKernelType.backwardQuery     -> D, dQ      (needs O, dO, L)
           AttentionKernelType.backwardKeyValue  -> dK, dV     (needs L, D)
exactly the dispatch order of the reference's test (SquareAttentionTest.swift:355-368).  torch owns the
device memory and the stream; all arithmetic happens in libmfa_hip.so (no eager fallback: a missing
library or a CPU tensor raises).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from .attention import (AttentionDecode, AttentionDecodeFP8, AttentionPrefill, AttentionDescriptor, AttentionKernel, AttentionKernelType,
                        AttentionOperand as Op, GEMMOperandPrecision as P, KVCacheAppend, KVCachePrecision)

_KERNELS: Dict[Tuple, AttentionKernel] = {}


def _kernel(dtype: torch.dtype, R: int, C: int, D: int, kind: AttentionKernelType, fast_scale: bool = False) -> AttentionKernel:
    # a kernel object depends on (precisions, head dimension, type) only -- the sequence lengths are launch parameters
    # (mfa_launch_params.row / .column), so the cache is bounded by the handful of head dimensions a model uses
    fast_scale = bool(fast_scale) and dtype != torch.float32
    key = (dtype, D, kind, fast_scale)
    k = _KERNELS.get(key)
    if k is None:
        desc = AttentionDescriptor()
        desc.lowPrecisionInputs = dtype != torch.float32
        if dtype != torch.float32:
            desc.lowPrecisionInputType = P.BF16 if dtype == torch.bfloat16 else P.FP16
            desc.lowPrecisionOutputs = True     # O, dQ, dK, dV leave the kernels already in the inputs' type
        # fast_scale = the reference's mixed-precision mode (lowPrecisionIntermediates): the streams that fold the softmax scale
        # into the 16-bit operand (|dL| ~ 2e-3 with BF16), L stored in FP16 and D in BF16 (+Precisions.swift:82-83)
        desc.lowPrecisionIntermediates = fast_scale
        desc.matrixDimensions = (R, C, D)
        desc.transposeState = (False, False, False, False)
        k = _KERNELS[key] = AttentionKernel(desc.kernelDescriptor(kind))
    return k


def _check(q, k, v):
    if not (q.is_cuda and k.is_cuda and v.is_cuda):
        raise RuntimeError("flash_attention: tensors must live on the GPU (there is no CPU path)")
    if q.dtype not in (torch.bfloat16, torch.float16, torch.float32) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError("flash_attention: q, k, v must share one of bfloat16 / float16 / float32")
    # grouped-query attention: H query heads over Hkv K / V heads, query head h reads K / V head h // (H // Hkv)
    if q.dim() != 4 or k.dim() != 4 or v.shape != k.shape or q.shape[0] != k.shape[0] or q.shape[3] != k.shape[3] or \
            k.shape[1] == 0 or q.shape[1] % k.shape[1] != 0:
        raise ValueError("flash_attention: expected q [B, H, R, D] and k, v [B, Hkv, C, D] with H a multiple of Hkv "
                         f"(got q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)})")
    if k.device != q.device or v.device != q.device:
        raise RuntimeError(f"flash_attention: q, k, v must live on one device (got {q.device}, {k.device}, {v.device})")


def _check_block_mask(block_mask, R, C):
    """bitmap rows cover every 256-row block, words cover every 128-key block (the kernels index it unchecked)"""
    if block_mask.dim() != 2:
        raise ValueError("flash_attention: block_mask must be [ceil(R / 256)][words] (pack_block_mask)")
    rows_needed, words_needed = (R + 255) // 256, ((C + 127) // 128 + 31) // 32
    if block_mask.shape[0] < rows_needed or block_mask.shape[1] < words_needed:
        raise ValueError(f"flash_attention: block_mask is {tuple(block_mask.shape)}, needs at least "
                         f"({rows_needed}, {words_needed}) for R={R}, C={C}")


def _strides(B, H, R, C, D, Hkv=None):
    """packed head / batch strides; K, V, dK, dV count the Hkv K / V heads (grouped-query attention), the rest the H query heads"""
    Hkv = H if Hkv is None else Hkv
    hs = {Op.Q: R * D, Op.K: C * D, Op.V: C * D, Op.O: R * D, Op.L: R, Op.D: R,
          Op.dO: R * D, Op.dV: C * D, Op.dK: C * D, Op.dQ: R * D}
    kv = (Op.K, Op.V, Op.dK, Op.dV)
    return hs, {op: s * (Hkv if op in kv else H) for op, s in hs.items()}


def _as_strided_operand(t):
    """A [B, H, N, D] VIEW whose last dimension is contiguous (e.g. a permuted [B, N, H, D] tensor, a slice of a fused QKV
    projection) is handed to the kernels as it is: the C ABI takes a leading dimension and head / batch strides per operand
    (mfa_launch_params), so no copy is made.  Anything else is made contiguous first."""
    if t.stride(-1) != 1 or any(st < 0 for st in t.stride()) or (t.shape[2] > 1 and t.stride(2) < t.shape[3]):
        t = t.contiguous()
    return t, int(t.stride(2)) if t.shape[2] > 1 else int(t.shape[3]), int(t.stride(1)), int(t.stride(0))


def _apply_layouts(hs, bs, lds, **operands):
    """overwrite the packed strides of the given operands (name -> tensor) with their real ones"""
    out = {}
    for name, t in operands.items():
        t, ld, head, batch = _as_strided_operand(t)
        op = getattr(Op, name)
        lds[op], hs[op], bs[op] = ld, head, batch
        out[name] = t
    return out


def _run_forward(q, k, v, causal, q_lengths, k_lengths, block_mask, fast_scale):
    """forward dispatch -> (o, l, the (possibly strided) views handed to the kernel, lengths, mask arguments, fast_scale)"""
    _check(q, k, v)
    B, H, R, D = q.shape
    C, Hkv = k.shape[2], k.shape[1]
    hs, bs = _strides(B, H, R, C, D, Hkv)
    lds = {}
    views = _apply_layouts(hs, bs, lds, Q=q, K=k, V=v)
    q, k, v = views["Q"], views["K"], views["V"]
    o = torch.empty((B, H, R, D), dtype=q.dtype, device=q.device)      # fused output cast: no fp32 copy of O
    fast_scale = bool(fast_scale) and q.dtype != torch.float32
    l = torch.empty((B, H, R), dtype=torch.float16 if fast_scale else torch.float32, device=q.device)
    kernel = _kernel(q.dtype, R, C, D, AttentionKernelType.forward, fast_scale)
    need = kernel.workspaceSize(row=R, column=C, heads=H, batches=B, headsPerKeyValue=H // Hkv)
    lengths = q_lengths is not None or k_lengths is not None
    mask_kw = {}
    if block_mask is not None:   # int32 [ceil(R / 256)][words]: bit b of word w = column block 32 w + b (128 keys each)
        _check_block_mask(block_mask, R, C)
        block_mask = block_mask.to(device=q.device, dtype=torch.int32).contiguous()
        mask_kw = dict(blockMask=block_mask, blockMaskWords=int(block_mask.shape[-1]))
    if lengths:   # padding rows of the outputs are not written by the kernels: define them as zero
        o.zero_()
        l.zero_()
        q_lengths = None if q_lengths is None else q_lengths.to(device=q.device, dtype=torch.int32).contiguous()
        k_lengths = None if k_lengths is None else k_lengths.to(device=q.device, dtype=torch.int32).contiguous()
    ws = torch.empty(need, dtype=torch.uint8, device=q.device) if need and not causal and not lengths and not mask_kw else None
    # the C side launches on the CURRENT device (hipGetDevice) and this stream: make both the tensors' device
    with torch.cuda.device(q.device):
        kernel.dispatch({Op.Q: q, Op.K: k, Op.V: v, Op.O: o, Op.L: l}, row=R, column=C, heads=H, batches=B,
                        headStrides=hs, batchStrides=bs, leadingDimensions=lds,
                        stream=torch.cuda.current_stream(q.device).cuda_stream, workspace=ws, causal=causal, rowLengths=q_lengths, columnLengths=k_lengths,
                        headsPerKeyValue=H // Hkv, **mask_kw)
    return o, l, (q, k, v), (q_lengths, k_lengths), mask_kw, fast_scale


def _run_backward(q, k, v, o, l, grad_out, causal, lengths, mask_kw, fast_scale):
    """backwardQuery (writes D, dQ) then backwardKeyValue (dK, dV), the dispatch order of SquareAttentionTest.swift:355-368"""
    B, H, R, D = q.shape
    C, Hkv = k.shape[2], k.shape[1]
    G = H // Hkv
    # dO in the kernels' gradient storage type (AttentionDescriptor+Precisions.swift:13-17): BF16 whenever
    # the inputs are 16-bit (also next to FP16 Q/K/V, the reference's mix), FP32 with FP32 inputs
    do = grad_out.to(torch.float32 if q.dtype == torch.float32 else torch.bfloat16)   # no copy when it already is
    alloc = torch.zeros if lengths != (None, None) else torch.empty   # padding gets zero gradients
    dq = alloc((B, H, R, D), dtype=q.dtype, device=q.device)
    dk = alloc((B, Hkv, C, D), dtype=q.dtype, device=q.device)
    dv = alloc((B, Hkv, C, D), dtype=q.dtype, device=q.device)
    dterm = alloc((B, H, R), dtype=torch.bfloat16 if fast_scale else torch.float32, device=q.device)
    bufs = {Op.Q: q, Op.K: k, Op.V: v, Op.O: o, Op.L: l, Op.D: dterm, Op.dO: do, Op.dQ: dq, Op.dK: dk, Op.dV: dv}
    hs, bs = _strides(B, H, R, C, D, Hkv)
    lds = {}
    # saved as the (possibly strided) views the forward used; a strided grad_out (e.g. the gradient of a permuted view)
    # is passed with its own leading dimension / head / batch strides instead of being copied
    # every operand is the tensor its strides describe: an input that had to be made contiguous (torch.library path: the raw inputs
    # are what was saved) must be passed as that copy, not as the original pointer
    views = _apply_layouts(hs, bs, lds, Q=q, K=k, V=v, dO=do)
    bufs[Op.Q], bufs[Op.K], bufs[Op.V], bufs[Op.dO] = views["Q"], views["K"], views["V"], views["dO"]
    with torch.cuda.device(q.device):
        stream = torch.cuda.current_stream(q.device).cuda_stream
        for kind in (AttentionKernelType.backwardQuery, AttentionKernelType.backwardKeyValue):   # dQ writes D first
            kernel = _kernel(q.dtype, R, C, D, kind, fast_scale)
            ws = None
            if kind == AttentionKernelType.backwardKeyValue and G > 1:   # per-query-head dK / dV slabs, summed per group by the library
                ws = torch.empty(kernel.workspaceSize(row=R, column=C, heads=H, batches=B, headsPerKeyValue=G), dtype=torch.uint8, device=q.device)
            kernel.dispatch(bufs, row=R, column=C, heads=H, batches=B, headStrides=hs, batchStrides=bs, leadingDimensions=lds, stream=stream,
                            causal=causal, rowLengths=lengths[0], columnLengths=lengths[1], workspace=ws, headsPerKeyValue=G, **mask_kw)
    return dq, dk, dv


class _FlashAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal: bool, q_lengths=None, k_lengths=None, block_mask=None, fast_scale=False):
        o, l, (q, k, v), lengths, mask_kw, fast_scale = _run_forward(q, k, v, causal, q_lengths, k_lengths, block_mask, fast_scale)
        ctx.save_for_backward(q, k, v, o, l)
        ctx.causal = causal
        ctx.fast_scale = fast_scale
        ctx.lengths = lengths
        ctx.mask_kw = mask_kw
        return o

    @staticmethod
    def backward(ctx, grad_out):
        q, k, v, o, l = ctx.saved_tensors
        dq, dk, dv = _run_backward(q, k, v, o, l, grad_out, ctx.causal, ctx.lengths, ctx.mask_kw, ctx.fast_scale)
        return dq, dk, dv, None, None, None, None, None


# ---- the same two steps as torch.library custom ops: opaque to the tracer but with shape functions and an autograd formula, so a
# function that calls flash_attention_op compiles with torch.compile(fullgraph=True) (the autograd.Function above is a graph break).
# Dense / causal only; per-batch lengths and block masks stay on flash_attention().
def _register_ops():
    """defines mfa::attention_forward / mfa::attention_backward once per process (a module reload finds them already defined);
    torch < 2.4 has no torch.library.custom_op: flash_attention() keeps working there, flash_attention_op() raises."""
    if not hasattr(torch.library, "custom_op"):
        return False
    try:
        torch.ops.mfa.attention_forward  # noqa: B018 -- AttributeError when the op is not defined yet
        torch.ops.mfa.attention_backward  # noqa: B018
        return True
    except (AttributeError, RuntimeError):
        pass

    @torch.library.custom_op("mfa::attention_forward", mutates_args=(), device_types="cuda")
    def _op_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool, fast_scale: bool) -> Tuple[torch.Tensor, torch.Tensor]:
        o, l, _views, _lengths, _mask, _fast = _run_forward(q, k, v, causal, None, None, None, fast_scale)
        return o, l


    @_op_forward.register_fake
    def _op_forward_fake(q, k, v, causal, fast_scale):
        B, H, R, D = q.shape
        fast = bool(fast_scale) and q.dtype != torch.float32
        return q.new_empty((B, H, R, D)), q.new_empty((B, H, R), dtype=torch.float16 if fast else torch.float32)


    @torch.library.custom_op("mfa::attention_backward", mutates_args=(), device_types="cuda")
    def _op_backward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, o: torch.Tensor, l: torch.Tensor, grad_out: torch.Tensor,
                     causal: bool, fast_scale: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        _check(q, k, v)
        fast = bool(fast_scale) and q.dtype != torch.float32
        return _run_backward(q, k, v, o, l, grad_out, causal, (None, None), {}, fast)


    @_op_backward.register_fake
    def _op_backward_fake(q, k, v, o, l, grad_out, causal, fast_scale):
        return torch.empty_like(q, memory_format=torch.contiguous_format), torch.empty_like(k, memory_format=torch.contiguous_format), \
            torch.empty_like(v, memory_format=torch.contiguous_format)


    def _op_setup_context(ctx, inputs, output):
        q, k, v, causal, fast_scale = inputs
        o, l = output
        ctx.save_for_backward(q, k, v, o, l)
        ctx.causal, ctx.fast_scale = causal, fast_scale


    def _op_autograd(ctx, grad_o, grad_l):
        q, k, v, o, l = ctx.saved_tensors
        dq, dk, dv = torch.ops.mfa.attention_backward(q, k, v, o, l, grad_o, ctx.causal, ctx.fast_scale)
        return dq, dk, dv, None, None


    _op_forward.register_autograd(_op_autograd, setup_context=_op_setup_context)
    return True


_HAVE_OPS = _register_ops()


def flash_attention_op(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = False, fast_scale: bool = False) -> torch.Tensor:
    """flash_attention(q, k, v, causal, fast_scale=...) through the torch.library ops `mfa::attention_forward` /
    `mfa::attention_backward`: traceable by torch.compile (fullgraph) and torch.export; dense or causal."""
    if not _HAVE_OPS:
        raise RuntimeError("flash_attention_op needs torch.library.custom_op (torch >= 2.4); use flash_attention() on this torch")
    return torch.ops.mfa.attention_forward(q, k, v, causal, fast_scale)[0]


def pack_block_mask(bits: torch.Tensor) -> torch.Tensor:
    """bool [row blocks of 256][column blocks of 128] -> the int32 bitmap the kernels read."""
    rb, cb = bits.shape
    words = (cb + 31) // 32
    padded = torch.zeros((rb, words * 32), dtype=torch.int64, device=bits.device)
    padded[:, :cb] = bits.to(torch.int64)
    weights = (1 << torch.arange(32, dtype=torch.int64, device=bits.device))
    packed = (padded.view(rb, words, 32) * weights).sum(-1)
    return torch.where(packed >= 2 ** 31, packed - 2 ** 32, packed).to(torch.int32)


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = False,
                    q_lengths: torch.Tensor = None, k_lengths: torch.Tensor = None,
                    block_mask: torch.Tensor = None, fast_scale: bool = False) -> torch.Tensor:
    """softmax(q k^T / sqrt(D)) v per (batch, head); causal: row r sees column c iff c <= r + (C - R).
    q_lengths / k_lengths ([B] integers, optional): batch entry b uses only its first q_lengths[b] rows and
    k_lengths[b] keys (padded batches); padding rows of the output and of the gradients are zero.
    block_mask (optional, from pack_block_mask): blocks of 256 rows x 128 keys that are attended at all.
    fast_scale (16-bit inputs only): the reference's mixed-precision mode (lowPrecisionIntermediates) -- the softmax scale is
    folded into the 16-bit operand once instead of being applied in fp32 per score (2-4 % faster; |dL| ~ 2e-3 with bf16),
    L is kept in FP16 and D in BF16 between forward and backward."""
    return _FlashAttention.apply(q, k, v, causal, q_lengths, k_lengths, block_mask, fast_scale)


# ---- decode attention over a KV cache (include/mfa_decode.h): forward only, per-sequence lengths on the device, contiguous or paged
_DECODERS: Dict[Tuple, AttentionDecode] = {}


def _cache_strides(t, paged):
    """(leadingDimension, headStride, batchStride) of a [B or pages, Hkv, keys, D] cache view, passed through as they are"""
    return (int(t.stride(2)) if t.shape[2] > 1 else int(t.shape[3]), int(t.stride(1)), 0 if paged else int(t.stride(0)))


def _run_decode(q, k_cache, v_cache, cache_lengths, block_table, causal, fp8=False, k_scale=None, v_scale=None, window=None, sinks=None):
    if not (q.is_cuda and k_cache.is_cuda and v_cache.is_cuda and cache_lengths.is_cuda):
        raise RuntimeError("flash_decode: tensors must live on the GPU (there is no CPU path)")
    if fp8:
        if k_cache.dtype != v_cache.dtype or k_cache.dtype != torch.float8_e4m3fn:
            raise TypeError(f"flash_decode: an FP8 KV cache is torch.float8_e4m3fn for both K and V (got {k_cache.dtype}, {v_cache.dtype}); "
                            "e5m2 and fnuz caches have no kernel")
        if q.dtype not in (torch.bfloat16, torch.float16):
            raise TypeError("flash_decode: q must be bfloat16 or float16")
    elif q.dtype not in (torch.bfloat16, torch.float16) or k_cache.dtype != q.dtype or v_cache.dtype != q.dtype:
        raise TypeError("flash_decode: q and the caches must share one of bfloat16 / float16")
    paged = block_table is not None
    if q.dim() != 4 or k_cache.dim() != 4 or v_cache.shape != k_cache.shape or q.shape[3] != k_cache.shape[3] or k_cache.shape[1] == 0 or \
            q.shape[1] % k_cache.shape[1] != 0 or (not paged and k_cache.shape[0] != q.shape[0]):
        raise ValueError("flash_decode: expected q [B, H, R, D] and caches [B, Hkv, C, D] (paged: [pages, Hkv, pageSize, D]) with H a "
                         f"multiple of Hkv (got q {tuple(q.shape)}, k {tuple(k_cache.shape)}, v {tuple(v_cache.shape)})")
    B, H, R, D = q.shape
    Hkv = k_cache.shape[1]
    if cache_lengths.shape != (B,) or cache_lengths.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"flash_decode: cache_lengths must be [B] = [{B}] int32 or int64 (got {tuple(cache_lengths.shape)}, {cache_lengths.dtype})")
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if t.stride(3) != 1 or any(st < 0 for st in t.stride()):
            raise ValueError(f"flash_decode: {name} must have a contiguous last dimension (a cache is never copied)")
    kw = {}
    if paged:
        if block_table.dim() != 2 or block_table.shape[0] != B or block_table.dtype != torch.int32 or block_table.stride(1) != 1 or \
                not block_table.is_cuda:
            raise ValueError(f"flash_decode: block_table must be an int32 GPU tensor [B, pages per sequence] = [{B}, n] with a contiguous "
                             f"last dimension (got {tuple(block_table.shape)}, {block_table.dtype})")
        page = int(k_cache.shape[2])
        column = page * int(block_table.shape[1])
        kw = dict(pageSize=page, blockTable=block_table, blockTableStride=int(block_table.stride(0)),
                  pageStrides=(int(k_cache.stride(0)), int(v_cache.stride(0))))
    else:
        column = int(k_cache.shape[2])
    q = q if q.stride(3) == 1 and all(st >= 0 for st in q.stride()) else q.contiguous()
    lengths = cache_lengths.to(torch.int32)   # (no copy when it already is; stays on the device)
    o = torch.empty((B, H, R, D), dtype=q.dtype, device=q.device)
    l = torch.empty((B, H, R), dtype=torch.float32, device=q.device)
    key = (q.dtype, D, bool(fp8))
    dec = _DECODERS.get(key)
    if dec is None:
        dec = _DECODERS[key] = (AttentionDecodeFP8 if fp8 else AttentionDecode)(D, P.BF16 if q.dtype == torch.bfloat16 else P.FP16)
    if fp8:
        kw.update(keyScale=_scale_operand("flash_decode", "k_scale", k_scale, Hkv, q.device),
                  valueScale=_scale_operand("flash_decode", "v_scale", v_scale, Hkv, q.device))
    kw.update(rows=R, column=column, heads=H, batches=B, headsPerKeyValue=H // Hkv, causal=bool(causal), cacheLengths=lengths,
              strides=dict(Q=(int(q.stride(2)) if R > 1 else D, int(q.stride(1)), int(q.stride(0))),
                           K=_cache_strides(k_cache, paged), V=_cache_strides(v_cache, paged)))
    if window is not None:
        kw.update(window=int(window))
    if sinks is not None:   # (sink tokens or 0, sink logits or None): the entries of include/mfa_sink.h
        kw.update(sinkTokens=int(sinks[0]), sinkLogits=sinks[1])
    need = dec.workspaceSize(**kw)
    ws = torch.empty(need, dtype=torch.uint8, device=q.device) if need else None
    with torch.cuda.device(q.device):
        dec.dispatch(q, k_cache, v_cache, o, l, stream=torch.cuda.current_stream(q.device).cuda_stream, workspace=ws, **kw)
    return o, l


def _scale_operand(who, name, t, heads, device):
    """a per-head scale as the kernels read it: fp32 [heads] on the cache's device, contiguous; None stays None (1.0)"""
    if t is None:
        return None
    if not t.is_cuda or t.device != device:
        raise RuntimeError(f"{who}: {name} must live on the GPU of the cache (the host never reads a scale)")
    if t.shape != (heads,) or t.dtype != torch.float32:
        raise ValueError(f"{who}: {name} must be float32 [Hkv] = [{heads}] (got {tuple(t.shape)}, {t.dtype})")
    return t.contiguous()


def _run_decode_fp8(q, k_cache, v_cache, cache_lengths, block_table, causal, k_scale, v_scale):
    return _run_decode(q, k_cache, v_cache, cache_lengths, block_table, causal, True, k_scale, v_scale)


def _run_append(k_new, v_new, k_cache, v_cache, cache_lengths, block_table, k_scale, v_scale):
    who = "kv_cache_append"
    tensors = (k_new, v_new, k_cache, v_cache, cache_lengths)
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"{who}: tensors must live on the GPU (there is no CPU path)")
    if k_new.dtype not in (torch.bfloat16, torch.float16) or v_new.dtype != k_new.dtype:
        raise TypeError(f"{who}: k_new and v_new must share one of bfloat16 / float16")
    if k_cache.dtype != v_cache.dtype or k_cache.dtype not in (k_new.dtype, torch.float8_e4m3fn):
        raise TypeError(f"{who}: the caches must both be torch.float8_e4m3fn or the new rows' {k_new.dtype} (got {k_cache.dtype}, "
                        f"{v_cache.dtype}); e5m2 and fnuz caches have no kernel")
    fp8 = k_cache.dtype == torch.float8_e4m3fn
    if not fp8 and (k_scale is not None or v_scale is not None):
        raise ValueError(f"{who}: k_scale / v_scale go with a float8_e4m3fn cache; a 16-bit cache takes the rows' bits")
    paged = block_table is not None
    if k_new.dim() != 4 or v_new.shape != k_new.shape or k_cache.dim() != 4 or v_cache.shape != k_cache.shape or \
            k_cache.shape[1] != k_new.shape[1] or k_cache.shape[3] != k_new.shape[3] or (not paged and k_cache.shape[0] != k_new.shape[0]):
        raise ValueError(f"{who}: expected k_new, v_new [B, Hkv, R, D] and caches [B, Hkv, C, D] (paged: [pages, Hkv, pageSize, D]) "
                         f"(got {tuple(k_new.shape)}, {tuple(v_new.shape)}, {tuple(k_cache.shape)}, {tuple(v_cache.shape)})")
    B, Hkv, R, D = k_new.shape
    if cache_lengths.shape != (B,) or cache_lengths.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{who}: cache_lengths must be [B] = [{B}] int32 or int64 (got {tuple(cache_lengths.shape)}, {cache_lengths.dtype})")
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if t.stride(3) != 1 or any(st < 0 for st in t.stride()):
            raise ValueError(f"{who}: {name} must have a contiguous last dimension (a cache is written where it lies)")
    kw = {}
    if paged:
        if block_table.dim() != 2 or block_table.shape[0] != B or block_table.dtype != torch.int32 or block_table.stride(1) != 1 or \
                not block_table.is_cuda:
            raise ValueError(f"{who}: block_table must be an int32 GPU tensor [B, pages per sequence] = [{B}, n] with a contiguous "
                             f"last dimension (got {tuple(block_table.shape)}, {block_table.dtype})")
        block_table = block_table.contiguous()   # (the row stride is the bound on the pages a sequence may name)
        kw = dict(pageSize=int(k_cache.shape[2]), blockTable=block_table, blockTableStride=int(block_table.shape[1]),
                  pageStrides=(int(k_cache.stride(0)), int(v_cache.stride(0))))
    else:
        kw = dict(column=int(k_cache.shape[2]))
    news = [t if t.stride(3) == 1 and all(st >= 0 for st in t.stride()) else t.contiguous() for t in (k_new, v_new)]
    new_strides = lambda t: (int(t.stride(2)) if R > 1 else D, int(t.stride(1)), int(t.stride(0)))  # noqa: E731
    lengths = cache_lengths.to(torch.int32)
    key = (k_new.dtype, D, fp8)
    app = _APPENDERS.get(key)
    if app is None:
        app = _APPENDERS[key] = KVCacheAppend(D, P.BF16 if k_new.dtype == torch.bfloat16 else P.FP16, KVCachePrecision.E4M3 if fp8 else None)
    if fp8:
        kw.update(keyScale=_scale_operand(who, "k_scale", k_scale, Hkv, k_new.device), valueScale=_scale_operand(who, "v_scale", v_scale, Hkv, k_new.device))
    with torch.cuda.device(k_new.device):
        app.dispatch(news[0], news[1], k_cache, v_cache, stream=torch.cuda.current_stream(k_new.device).cuda_stream, rows=R, heads=Hkv,
                     batches=B, cacheLengths=lengths,
                     strides=dict(kNew=new_strides(news[0]), vNew=new_strides(news[1]), kCache=_cache_strides(k_cache, paged),
                                  vCache=_cache_strides(v_cache, paged)), **kw)


_APPENDERS: Dict[Tuple, KVCacheAppend] = {}
_FP8_DTYPES = tuple(getattr(torch, n) for n in ("float8_e4m3fn", "float8_e5m2", "float8_e4m3fnuz", "float8_e5m2fnuz") if hasattr(torch, n))


def _register_kvcache_ops():
    if not hasattr(torch.library, "custom_op"):
        return False
    try:
        torch.ops.mfa.attention_decode_fp8  # noqa: B018 -- AttributeError when the op is not defined yet
        torch.ops.mfa.kv_cache_append  # noqa: B018
        return True
    except (AttributeError, RuntimeError):
        pass

    @torch.library.custom_op("mfa::attention_decode_fp8", mutates_args=(), device_types="cuda")
    def _op_decode_fp8(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                       block_table: Optional[torch.Tensor], causal: bool, k_scale: Optional[torch.Tensor],
                       v_scale: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        return _run_decode_fp8(q, k_cache, v_cache, cache_lengths, block_table, causal, k_scale, v_scale)

    @_op_decode_fp8.register_fake
    def _op_decode_fp8_fake(q, k_cache, v_cache, cache_lengths, block_table, causal, k_scale, v_scale):
        B, H, R, D = q.shape
        return q.new_empty((B, H, R, D)), q.new_empty((B, H, R), dtype=torch.float32)

    @torch.library.custom_op("mfa::kv_cache_append", mutates_args=("k_cache", "v_cache"), device_types="cuda")
    def _op_append(k_new: torch.Tensor, v_new: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                   block_table: Optional[torch.Tensor], k_scale: Optional[torch.Tensor], v_scale: Optional[torch.Tensor]) -> None:
        _run_append(k_new, v_new, k_cache, v_cache, cache_lengths, block_table, k_scale, v_scale)

    @_op_append.register_fake
    def _op_append_fake(k_new, v_new, k_cache, v_cache, cache_lengths, block_table, k_scale, v_scale):
        return None

    return True


_HAVE_KVCACHE_OPS = _register_kvcache_ops()


def kv_cache_append(k_new: torch.Tensor, v_new: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                    block_table: Optional[torch.Tensor] = None, k_scale: Optional[torch.Tensor] = None,
                    v_scale: Optional[torch.Tensor] = None) -> None:
    """Writes the R new key / value rows of every sequence (k_new, v_new [B, Hkv, R, D], bf16 or fp16) into the caches IN PLACE and
    returns nothing.  cache_lengths [B] (GPU) ALREADY INCLUDES the new tokens -- the tensor flash_decode takes next: row r of sequence
    b goes to key cache_lengths[b] - R + r; rows that fall before key 0, past the cache's capacity or past the block table's row are
    not written, and no other byte of the cache is touched.  Caches: [B, Hkv, C, D] (or a strided view with a contiguous last
    dimension) or, with block_table [B, n] int32, page pools [pages, Hkv, pageSize, D]; dtype torch.float8_e4m3fn (the rows are
    quantised: byte = e4m3(x / scale[j]), round to nearest even, saturating at +-448; k_scale / v_scale fp32 [Hkv], None = 1.0) or
    the rows' own 16-bit type (bits copied; scales are an error).  Goes through the op `mfa::kv_cache_append` (mutates_args) where
    torch has custom ops."""
    for t in (k_new, v_new, k_cache, v_cache):
        if t.requires_grad:
            raise RuntimeError("kv_cache_append writes in place and has no autograd: detach the inputs")
    if not all(t.is_cuda for t in (k_new, v_new, k_cache, v_cache, cache_lengths)):
        raise RuntimeError("kv_cache_append: tensors must live on the GPU (there is no CPU path)")
    if _HAVE_KVCACHE_OPS:
        torch.ops.mfa.kv_cache_append(k_new, v_new, k_cache, v_cache, cache_lengths, block_table, k_scale, v_scale)
    else:
        _run_append(k_new, v_new, k_cache, v_cache, cache_lengths, block_table, k_scale, v_scale)


def _register_decode_op():
    if not hasattr(torch.library, "custom_op"):
        return False
    try:
        torch.ops.mfa.attention_decode  # noqa: B018 -- AttributeError when the op is not defined yet
        return True
    except (AttributeError, RuntimeError):
        pass

    @torch.library.custom_op("mfa::attention_decode", mutates_args=(), device_types="cuda")
    def _op_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                   block_table: Optional[torch.Tensor], causal: bool) -> Tuple[torch.Tensor, torch.Tensor]:
        return _run_decode(q, k_cache, v_cache, cache_lengths, block_table, causal)

    @_op_decode.register_fake
    def _op_decode_fake(q, k_cache, v_cache, cache_lengths, block_table, causal):
        B, H, R, D = q.shape
        return q.new_empty((B, H, R, D)), q.new_empty((B, H, R), dtype=torch.float32)

    return True


_HAVE_DECODE_OP = _register_decode_op()


def flash_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                 block_table: Optional[torch.Tensor] = None, causal: bool = True, return_lse: bool = False,
                 k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None, window: Optional[int] = None,
                 sink_tokens: Optional[int] = None, sink_logits: Optional[torch.Tensor] = None):
    """Attention of the R new rows of every sequence (q [B, H, R, D]; R = 1, or a few speculative tokens; G R <= 32 with G = H / Hkv)
    against its KV cache.  cache_lengths [B] (GPU, int32): valid keys per sequence INCLUDING the R new tokens, which the caller has
    already written into the cache; with `causal` row r sees key c iff c <= r + max(len - R, 0).  Caches: [B, Hkv, C, D], or any view
    of that shape with a contiguous last dimension (a token-major [B, C, Hkv, D] cache permuted, slices of a fused allocation:
    strides are passed through, nothing is copied); with block_table [B, n] int32 the caches are page pools [pages, Hkv, pageSize, D]
    and entry (b, i) names the page of keys i pageSize .. of sequence b.  Forward only.  return_lse: also L [B, H, R] fp32 in natural
    units (log of the softmax denominator, the scale included), to merge results across cache shards.  A sequence of length 0 gets
    O = 0.  Goes through the torch.library op `mfa::attention_decode` where torch has custom ops, so it traces under torch.compile.
    FP8 caches (torch.float8_e4m3fn, written by kv_cache_append): k_scale / v_scale [Hkv] fp32 on the GPU (None = 1.0), a cache byte
    of head j stands for scale[j] x e4m3(byte); the launch goes through the op `mfa::attention_decode_fp8`.  Scales with a 16-bit
    cache are an error.
    window=W (an int >= 1; needs causal): sliding-window attention -- a row sees its frontier and the W - 1 keys before it; keys, pages
    and block-table entries below the first 64-key tile a sequence's rows see are never read (include/mfa_window.h).  Goes through the
    op `mfa::attention_decode_window`, for 16-bit and e4m3 caches alike.  None: no window.
    sink_tokens=S (an int >= 1; needs window): the keys [0, S) stay visible under the window, and the keys, pages and block-table
    entries between their tiles and the window's are never read.  sink_logits [H] fp32 on the GPU (any window, causal or not): one
    learned logit per query head joins the softmax denominator and no value row -- natural-log units, not scaled by 1 / sqrt(D) or
    k_scale; L includes it (include/mfa_sink.h).  Either goes through the op `mfa::attention_decode_sink`."""
    if not (q.is_cuda and k_cache.is_cuda and v_cache.is_cuda and cache_lengths.is_cuda):
        raise RuntimeError("flash_decode: tensors must live on the GPU (there is no CPU path)")
    for t in (q, k_cache, v_cache):
        if t.requires_grad:
            raise RuntimeError("flash_decode is forward only (no autograd): detach the inputs; flash_attention is the differentiable entry")
    if sink_tokens is not None or sink_logits is not None:
        _check_sinks("flash_decode", q, window, causal, sink_tokens, sink_logits)
        if _HAVE_SINK_OPS:
            o, l = torch.ops.mfa.attention_decode_sink(q, k_cache, v_cache, cache_lengths, block_table, causal, k_scale, v_scale,
                                                       window or 0, sink_tokens or 0, sink_logits)
        else:
            o, l = _run_decode_sink(q, k_cache, v_cache, cache_lengths, block_table, causal, k_scale, v_scale, window or 0, sink_tokens or 0, sink_logits)
    elif window is not None:
        _check_window("flash_decode", window, causal)
        if _HAVE_WINDOW_OPS:
            o, l = torch.ops.mfa.attention_decode_window(q, k_cache, v_cache, cache_lengths, block_table, causal, k_scale, v_scale, window)
        else:
            o, l = _run_decode_window(q, k_cache, v_cache, cache_lengths, block_table, causal, k_scale, v_scale, window)
    elif k_cache.dtype in _FP8_DTYPES or v_cache.dtype in _FP8_DTYPES:
        if _HAVE_KVCACHE_OPS:
            o, l = torch.ops.mfa.attention_decode_fp8(q, k_cache, v_cache, cache_lengths, block_table, causal, k_scale, v_scale)
        else:
            o, l = _run_decode_fp8(q, k_cache, v_cache, cache_lengths, block_table, causal, k_scale, v_scale)
    elif k_scale is not None or v_scale is not None:
        raise ValueError("flash_decode: k_scale / v_scale go with a float8_e4m3fn cache; a 16-bit cache holds the values themselves")
    elif _HAVE_DECODE_OP:
        o, l = torch.ops.mfa.attention_decode(q, k_cache, v_cache, cache_lengths, block_table, causal)
    else:
        o, l = _run_decode(q, k_cache, v_cache, cache_lengths, block_table, causal)
    return (o, l * 0.6931471805599453) if return_lse else o


# ---- prefill attention over a KV cache (include/mfa_prefill.h): a block of new rows per sequence against a 16-bit or FP8 cache
_PREFILLERS: Dict[Tuple, AttentionPrefill] = {}


def _run_prefill(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale, window=None, sinks=None):
    who = "flash_prefill"
    if not (q.is_cuda and k_cache.is_cuda and v_cache.is_cuda and cache_lengths.is_cuda):
        raise RuntimeError(f"{who}: tensors must live on the GPU (there is no CPU path)")
    fp8 = k_cache.dtype in _FP8_DTYPES or v_cache.dtype in _FP8_DTYPES
    if q.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError(f"{who}: q must be bfloat16 or float16")
    if fp8:
        if k_cache.dtype != v_cache.dtype or k_cache.dtype != torch.float8_e4m3fn:
            raise TypeError(f"{who}: an FP8 KV cache is torch.float8_e4m3fn for both K and V (got {k_cache.dtype}, {v_cache.dtype}); "
                            "e5m2 and fnuz caches have no kernel")
    elif k_cache.dtype != q.dtype or v_cache.dtype != q.dtype:
        raise TypeError(f"{who}: q and the caches must share one of bfloat16 / float16 (or the caches are float8_e4m3fn)")
    elif k_scale is not None or v_scale is not None:
        raise ValueError(f"{who}: k_scale / v_scale go with a float8_e4m3fn cache; a 16-bit cache holds the values themselves")
    paged = block_table is not None
    if q.dim() != 4 or k_cache.dim() != 4 or v_cache.shape != k_cache.shape or q.shape[3] != k_cache.shape[3] or k_cache.shape[1] == 0 or \
            q.shape[1] % k_cache.shape[1] != 0 or (not paged and k_cache.shape[0] != q.shape[0]):
        raise ValueError(f"{who}: expected q [B, H, R, D] and caches [B, Hkv, C, D] (paged: [pages, Hkv, pageSize, D]) with H a "
                         f"multiple of Hkv (got q {tuple(q.shape)}, k {tuple(k_cache.shape)}, v {tuple(v_cache.shape)})")
    B, H, R, D = q.shape
    Hkv = k_cache.shape[1]
    for name, t in (("cache_lengths", cache_lengths), ("q_lengths", q_lengths)):
        if t is not None and (not t.is_cuda or t.shape != (B,) or t.dtype not in (torch.int32, torch.int64)):
            raise ValueError(f"{who}: {name} must be a GPU tensor [B] = [{B}] int32 or int64 (got {tuple(t.shape)}, {t.dtype})")
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if t.stride(3) != 1 or any(st < 0 for st in t.stride()):
            raise ValueError(f"{who}: {name} must have a contiguous last dimension (a cache is never copied)")
    kw = {}
    if paged:
        if block_table.dim() != 2 or block_table.shape[0] != B or block_table.dtype != torch.int32 or block_table.stride(1) != 1 or \
                not block_table.is_cuda:
            raise ValueError(f"{who}: block_table must be an int32 GPU tensor [B, pages per sequence] = [{B}, n] with a contiguous "
                             f"last dimension (got {tuple(block_table.shape)}, {block_table.dtype})")
        page = int(k_cache.shape[2])
        column = page * int(block_table.shape[1])
        kw = dict(pageSize=page, blockTable=block_table, blockTableStride=int(block_table.stride(0)),
                  pageStrides=(int(k_cache.stride(0)), int(v_cache.stride(0))))
    else:
        column = int(k_cache.shape[2])
    q = q if q.stride(3) == 1 and all(st >= 0 for st in q.stride()) else q.contiguous()
    lengths = cache_lengths.to(torch.int32)   # (no copy when it already is; stays on the device)
    qlens = None if q_lengths is None else q_lengths.to(torch.int32)
    # (rows at or past q_lengths[b] are not written by the launch: no memset is spent on them, they come back uninitialised)
    o = torch.empty((B, H, R, D), dtype=q.dtype, device=q.device)
    l = torch.empty((B, H, R), dtype=torch.float32, device=q.device)
    key = (q.dtype, D, bool(fp8))
    pre = _PREFILLERS.get(key)
    if pre is None:
        pre = _PREFILLERS[key] = AttentionPrefill(D, P.BF16 if q.dtype == torch.bfloat16 else P.FP16,
                                                  cachePrecision=KVCachePrecision.E4M3 if fp8 else None)
    if fp8:
        kw.update(keyScale=_scale_operand(who, "k_scale", k_scale, Hkv, q.device), valueScale=_scale_operand(who, "v_scale", v_scale, Hkv, q.device))
    kw.update(rows=R, column=column, heads=H, batches=B, headsPerKeyValue=H // Hkv, causal=bool(causal), cacheLengths=lengths,
              queryLengths=qlens,
              strides=dict(Q=(int(q.stride(2)) if R > 1 else D, int(q.stride(1)), int(q.stride(0))),
                           K=_cache_strides(k_cache, paged), V=_cache_strides(v_cache, paged)))
    if window is not None:
        kw.update(window=int(window))
    if sinks is not None:
        kw.update(sinkTokens=int(sinks[0]), sinkLogits=sinks[1])
    with torch.cuda.device(q.device):
        pre.dispatch(q, k_cache, v_cache, o, l, stream=torch.cuda.current_stream(q.device).cuda_stream, **kw)
    return o, l


def _register_prefill_op():
    if not hasattr(torch.library, "custom_op"):
        return False
    try:
        torch.ops.mfa.attention_prefill  # noqa: B018 -- AttributeError when the op is not defined yet
        return True
    except (AttributeError, RuntimeError):
        pass

    @torch.library.custom_op("mfa::attention_prefill", mutates_args=(), device_types="cuda")
    def _op_prefill(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                    q_lengths: Optional[torch.Tensor], block_table: Optional[torch.Tensor], causal: bool,
                    k_scale: Optional[torch.Tensor], v_scale: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        return _run_prefill(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale)

    @_op_prefill.register_fake
    def _op_prefill_fake(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale):
        B, H, R, D = q.shape
        return q.new_empty((B, H, R, D)), q.new_empty((B, H, R), dtype=torch.float32)

    return True


_HAVE_PREFILL_OP = _register_prefill_op()


def _check_window(who, window, causal):
    if isinstance(window, bool) or not isinstance(window, int) or not 1 <= window < 2 ** 32:
        raise ValueError(f"{who}: window must be an int from 1 to 2^32 - 1 (None: no window), not {window!r}")
    if not causal:
        raise ValueError(f"{who}: a sliding window needs causal=True (the window lies behind the row's causal frontier)")


def _run_decode_window(q, k_cache, v_cache, cache_lengths, block_table, causal, k_scale, v_scale, window):
    fp8 = k_cache.dtype in _FP8_DTYPES or v_cache.dtype in _FP8_DTYPES
    if not fp8 and (k_scale is not None or v_scale is not None):
        raise ValueError("flash_decode: k_scale / v_scale go with a float8_e4m3fn cache; a 16-bit cache holds the values themselves")
    return _run_decode(q, k_cache, v_cache, cache_lengths, block_table, causal, fp8, k_scale, v_scale, window)


def _register_window_ops():
    """mfa::attention_decode_window (16-bit and e4m3 caches: one op) and mfa::attention_prefill_window (include/mfa_window.h).  The
    ops without a window keep their schemas."""
    if not hasattr(torch.library, "custom_op"):
        return False
    try:
        torch.ops.mfa.attention_decode_window  # noqa: B018 -- AttributeError when the op is not defined yet
        torch.ops.mfa.attention_prefill_window  # noqa: B018
        return True
    except (AttributeError, RuntimeError):
        pass

    @torch.library.custom_op("mfa::attention_decode_window", mutates_args=(), device_types="cuda")
    def _op_decode_window(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                          block_table: Optional[torch.Tensor], causal: bool, k_scale: Optional[torch.Tensor],
                          v_scale: Optional[torch.Tensor], window: int) -> Tuple[torch.Tensor, torch.Tensor]:
        return _run_decode_window(q, k_cache, v_cache, cache_lengths, block_table, causal, k_scale, v_scale, window)

    @_op_decode_window.register_fake
    def _op_decode_window_fake(q, k_cache, v_cache, cache_lengths, block_table, causal, k_scale, v_scale, window):
        B, H, R, D = q.shape
        return q.new_empty((B, H, R, D)), q.new_empty((B, H, R), dtype=torch.float32)

    @torch.library.custom_op("mfa::attention_prefill_window", mutates_args=(), device_types="cuda")
    def _op_prefill_window(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                           q_lengths: Optional[torch.Tensor], block_table: Optional[torch.Tensor], causal: bool,
                           k_scale: Optional[torch.Tensor], v_scale: Optional[torch.Tensor], window: int) -> Tuple[torch.Tensor, torch.Tensor]:
        return _run_prefill(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale, window)

    @_op_prefill_window.register_fake
    def _op_prefill_window_fake(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale, window):
        B, H, R, D = q.shape
        return q.new_empty((B, H, R, D)), q.new_empty((B, H, R), dtype=torch.float32)

    return True


_HAVE_WINDOW_OPS = _register_window_ops()


def _check_sinks(who, q, window, causal, sink_tokens, sink_logits):
    if window is not None:
        _check_window(who, window, causal)
    if sink_tokens is not None:
        if isinstance(sink_tokens, bool) or not isinstance(sink_tokens, int) or not 1 <= sink_tokens < 2 ** 32:
            raise ValueError(f"{who}: sink_tokens must be an int from 1 to 2^32 - 1 (None: no sink tokens), not {sink_tokens!r}")
        if window is None:
            raise ValueError(f"{who}: sink_tokens needs window: the sink keys stay visible under a sliding window (without one every "
                             "key below the frontier is visible already)")
    if sink_logits is not None:
        if not isinstance(sink_logits, torch.Tensor) or sink_logits.dtype != torch.float32 or q.dim() != 4 or \
                tuple(sink_logits.shape) != (q.shape[1],) or not sink_logits.is_contiguous():
            raise ValueError(f"{who}: sink_logits must be a contiguous float32 tensor [H] = [{q.shape[1] if q.dim() == 4 else '?'}], one logit "
                             f"per query head (got {tuple(sink_logits.shape) if isinstance(sink_logits, torch.Tensor) else type(sink_logits).__name__}"
                             f"{', ' + str(sink_logits.dtype) if isinstance(sink_logits, torch.Tensor) else ''})")
        if sink_logits.device != q.device:
            raise RuntimeError(f"{who}: sink_logits must live on q's device (the host never reads a logit)")


def _run_decode_sink(q, k_cache, v_cache, cache_lengths, block_table, causal, k_scale, v_scale, window, sink_tokens, sink_logits):
    fp8 = k_cache.dtype in _FP8_DTYPES or v_cache.dtype in _FP8_DTYPES
    if not fp8 and (k_scale is not None or v_scale is not None):
        raise ValueError("flash_decode: k_scale / v_scale go with a float8_e4m3fn cache; a 16-bit cache holds the values themselves")
    return _run_decode(q, k_cache, v_cache, cache_lengths, block_table, causal, fp8, k_scale, v_scale, window or None, (sink_tokens, sink_logits))


def _register_sink_ops():
    """mfa::attention_decode_sink and mfa::attention_prefill_sink (include/mfa_sink.h): the window ops with `sink_tokens` (0: none)
    and `sink_logits` behind `window` (0: none).  The other ops keep their schemas."""
    if not hasattr(torch.library, "custom_op"):
        return False
    try:
        torch.ops.mfa.attention_decode_sink  # noqa: B018 -- AttributeError when the op is not defined yet
        torch.ops.mfa.attention_prefill_sink  # noqa: B018
        return True
    except (AttributeError, RuntimeError):
        pass

    @torch.library.custom_op("mfa::attention_decode_sink", mutates_args=(), device_types="cuda")
    def _op_decode_sink(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                        block_table: Optional[torch.Tensor], causal: bool, k_scale: Optional[torch.Tensor], v_scale: Optional[torch.Tensor],
                        window: int, sink_tokens: int, sink_logits: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        return _run_decode_sink(q, k_cache, v_cache, cache_lengths, block_table, causal, k_scale, v_scale, window, sink_tokens, sink_logits)

    @_op_decode_sink.register_fake
    def _op_decode_sink_fake(q, k_cache, v_cache, cache_lengths, block_table, causal, k_scale, v_scale, window, sink_tokens, sink_logits):
        B, H, R, D = q.shape
        return q.new_empty((B, H, R, D)), q.new_empty((B, H, R), dtype=torch.float32)

    @torch.library.custom_op("mfa::attention_prefill_sink", mutates_args=(), device_types="cuda")
    def _op_prefill_sink(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                         q_lengths: Optional[torch.Tensor], block_table: Optional[torch.Tensor], causal: bool,
                         k_scale: Optional[torch.Tensor], v_scale: Optional[torch.Tensor], window: int, sink_tokens: int,
                         sink_logits: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        return _run_prefill(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale, window or None,
                            (sink_tokens, sink_logits))

    @_op_prefill_sink.register_fake
    def _op_prefill_sink_fake(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale, window, sink_tokens, sink_logits):
        B, H, R, D = q.shape
        return q.new_empty((B, H, R, D)), q.new_empty((B, H, R), dtype=torch.float32)

    return True


_HAVE_SINK_OPS = _register_sink_ops()


def flash_prefill(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                  q_lengths: Optional[torch.Tensor] = None, block_table: Optional[torch.Tensor] = None, causal: bool = True,
                  k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None, return_lse: bool = False,
                  window: Optional[int] = None, sink_tokens: Optional[int] = None, sink_logits: Optional[torch.Tensor] = None):
    """Attention of a BLOCK of new rows of every sequence (q [B, H, R, D], any R: a chunk of a prompt, a reused prefix's tail, a long
    speculative block) against its KV cache, which already holds the new tokens (kv_cache_append first).  cache_lengths [B] (GPU):
    valid keys per sequence INCLUDING the new tokens; q_lengths [B] (GPU, None = R for every sequence): the new rows of sequence b,
    its first q_lengths[b] rows of q.  With `causal` row r sees key c iff c <= r + max(len - q_len, 0).  Rows at or past q_lengths[b]
    are not written: they come back uninitialised, in O and in L.  A live row without a visible key gets O = 0 (L: -FLT_MAX ln 2).  Caches: flash_decode's -- [B, Hkv, C, D] or any view of that shape
    with a contiguous last dimension, or with block_table [B, n] int32 page pools [pages, Hkv, pageSize, D]; bfloat16 / float16 like
    q, or torch.float8_e4m3fn with k_scale / v_scale [Hkv] fp32 on the GPU (None = 1.0; a byte of head j stands for scale[j] x
    e4m3(byte)).  The G = H / Hkv query heads of a K/V head share one workgroup (G <= 32), so K and V are read once per group.
    Forward only.  return_lse: also L [B, H, R] fp32 in natural units.  Goes through the torch.library op `mfa::attention_prefill`
    where torch has custom ops, so it traces under torch.compile.  window=W (an int >= 1; needs causal): sliding-window attention as
    flash_decode's, through the op `mfa::attention_prefill_window`; None: no window.  sink_tokens / sink_logits: attention sinks as
    flash_decode's (include/mfa_sink.h), through the op `mfa::attention_prefill_sink`; a live row without a visible key then gets
    L = the head's sink logit."""
    if not (q.is_cuda and k_cache.is_cuda and v_cache.is_cuda and cache_lengths.is_cuda):
        raise RuntimeError("flash_prefill: tensors must live on the GPU (there is no CPU path)")
    for t in (q, k_cache, v_cache):
        if t.requires_grad:
            raise RuntimeError("flash_prefill is forward only (no autograd): detach the inputs; flash_attention is the differentiable entry")
    if sink_tokens is not None or sink_logits is not None:
        _check_sinks("flash_prefill", q, window, causal, sink_tokens, sink_logits)
        if _HAVE_SINK_OPS:
            o, l = torch.ops.mfa.attention_prefill_sink(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale,
                                                        window or 0, sink_tokens or 0, sink_logits)
        else:
            o, l = _run_prefill(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale, window,
                                (sink_tokens or 0, sink_logits))
    elif window is not None:
        _check_window("flash_prefill", window, causal)
        if _HAVE_WINDOW_OPS:
            o, l = torch.ops.mfa.attention_prefill_window(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale, window)
        else:
            o, l = _run_prefill(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale, window)
    elif _HAVE_PREFILL_OP:
        o, l = torch.ops.mfa.attention_prefill(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale)
    else:
        o, l = _run_prefill(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale)
    return (o, l * 0.6931471805599453) if return_lse else o


# ---- ragged batches (include/mfa_ragged.h): packed query rows for prefill and append, one launch for a continuous-batching step
def _check_row_starts(who, row_starts, cache_lengths, max_rows):
    if not isinstance(row_starts, torch.Tensor) or not row_starts.is_cuda or row_starts.dim() != 1 or \
            row_starts.shape[0] != cache_lengths.shape[0] + 1 or row_starts.dtype not in (torch.int32, torch.int64):
        got = f"{tuple(row_starts.shape)}, {row_starts.dtype}" if isinstance(row_starts, torch.Tensor) else type(row_starts).__name__
        raise ValueError(f"{who}: row_starts must be a GPU tensor [B + 1] = [{cache_lengths.shape[0] + 1}] int32 or int64: the first packed row "
                         f"of every sequence and the end of the last (got {got})")
    if isinstance(max_rows, bool) or not isinstance(max_rows, int) or not 1 <= max_rows < 2 ** 32:
        raise ValueError(f"{who}: max_rows must be an int from 1 to 2^32 - 1, the largest row count of a sequence (the host never reads "
                         f"row_starts), not {max_rows!r}")


def _packed_operand(t):
    """a packed [T, heads, D] operand as the kernels read it: any view with a contiguous last dimension and 16-byte rows is taken where
    it lies (a slice of a fused QKV projection: strides, not a copy)"""
    ok = t.stride(2) == 1 and all(st >= 0 for st in t.stride()) and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0 and t.data_ptr() % 16 == 0
    return t if ok else t.contiguous()


def _run_prefill_ragged(q, k_cache, v_cache, cache_lengths, row_starts, max_rows, block_table, causal, k_scale, v_scale, window, sinks):
    who = "flash_prefill_ragged"
    if not (q.is_cuda and k_cache.is_cuda and v_cache.is_cuda and cache_lengths.is_cuda):
        raise RuntimeError(f"{who}: tensors must live on the GPU (there is no CPU path)")
    fp8 = k_cache.dtype in _FP8_DTYPES or v_cache.dtype in _FP8_DTYPES
    if q.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError(f"{who}: q must be bfloat16 or float16")
    if fp8:
        if k_cache.dtype != v_cache.dtype or k_cache.dtype != torch.float8_e4m3fn:
            raise TypeError(f"{who}: an FP8 KV cache is torch.float8_e4m3fn for both K and V (got {k_cache.dtype}, {v_cache.dtype}); "
                            "e5m2 and fnuz caches have no kernel")
    elif k_cache.dtype != q.dtype or v_cache.dtype != q.dtype:
        raise TypeError(f"{who}: q and the caches must share one of bfloat16 / float16 (or the caches are float8_e4m3fn)")
    elif k_scale is not None or v_scale is not None:
        raise ValueError(f"{who}: k_scale / v_scale go with a float8_e4m3fn cache; a 16-bit cache holds the values themselves")
    paged = block_table is not None
    if q.dim() != 3 or q.shape[0] == 0 or k_cache.dim() != 4 or v_cache.shape != k_cache.shape or q.shape[2] != k_cache.shape[3] or \
            k_cache.shape[1] == 0 or q.shape[1] % k_cache.shape[1] != 0:
        raise ValueError(f"{who}: expected q [T, H, D] (packed rows) and caches [B, Hkv, C, D] (paged: [pages, Hkv, pageSize, D]) with H a "
                         f"multiple of Hkv (got q {tuple(q.shape)}, k {tuple(k_cache.shape)}, v {tuple(v_cache.shape)})")
    T, H, D = q.shape
    Hkv = k_cache.shape[1]
    if cache_lengths.dim() != 1 or cache_lengths.dtype not in (torch.int32, torch.int64) or (not paged and cache_lengths.shape[0] != k_cache.shape[0]):
        raise ValueError(f"{who}: cache_lengths must be a GPU tensor [B] int32 or int64, B the caches' first dimension when they are "
                         f"contiguous (got {tuple(cache_lengths.shape)}, {cache_lengths.dtype})")
    B = int(cache_lengths.shape[0])
    _check_row_starts(who, row_starts, cache_lengths, max_rows)
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if t.stride(3) != 1 or any(st < 0 for st in t.stride()):
            raise ValueError(f"{who}: {name} must have a contiguous last dimension (a cache is never copied)")
    kw = {}
    if paged:
        if block_table.dim() != 2 or block_table.shape[0] != B or block_table.dtype != torch.int32 or block_table.stride(1) != 1 or \
                not block_table.is_cuda:
            raise ValueError(f"{who}: block_table must be an int32 GPU tensor [B, pages per sequence] = [{B}, n] with a contiguous "
                             f"last dimension (got {tuple(block_table.shape)}, {block_table.dtype})")
        page = int(k_cache.shape[2])
        column = page * int(block_table.shape[1])
        kw = dict(pageSize=page, blockTable=block_table, blockTableStride=int(block_table.stride(0)),
                  pageStrides=(int(k_cache.stride(0)), int(v_cache.stride(0))))
    else:
        column = int(k_cache.shape[2])
    q = _packed_operand(q)
    lengths, starts = cache_lengths.to(torch.int32), row_starts.to(torch.int32)   # (no copy when they already are; they stay on the device)
    # (packed rows no sequence owns are not written by the launch: no memset is spent on them, they come back uninitialised)
    o = torch.empty((T, H, D), dtype=q.dtype, device=q.device)
    l = torch.empty((H, T), dtype=torch.float32, device=q.device)
    key = (q.dtype, D, bool(fp8))
    pre = _PREFILLERS.get(key)
    if pre is None:
        pre = _PREFILLERS[key] = AttentionPrefill(D, P.BF16 if q.dtype == torch.bfloat16 else P.FP16,
                                                  cachePrecision=KVCachePrecision.E4M3 if fp8 else None)
    if fp8:
        kw.update(keyScale=_scale_operand(who, "k_scale", k_scale, Hkv, q.device), valueScale=_scale_operand(who, "v_scale", v_scale, Hkv, q.device))
    kw.update(rows=int(max_rows), column=column, heads=H, batches=B, headsPerKeyValue=H // Hkv, causal=bool(causal), cacheLengths=lengths,
              rowStarts=starts, totalRows=T,
              strides=dict(Q=(int(q.stride(0)) if T > 1 else H * D, int(q.stride(1)) if H > 1 else D, 0),
                           K=_cache_strides(k_cache, paged), V=_cache_strides(v_cache, paged)))
    if window:
        kw.update(window=int(window))
    if sinks is not None and (sinks[0] or sinks[1] is not None):
        kw.update(sinkTokens=int(sinks[0]), sinkLogits=sinks[1])
    with torch.cuda.device(q.device):
        pre.dispatch(q, k_cache, v_cache, o, l, stream=torch.cuda.current_stream(q.device).cuda_stream, **kw)
    return o, l


def _run_append_ragged(k_new, v_new, k_cache, v_cache, cache_lengths, row_starts, max_rows, block_table, k_scale, v_scale):
    who = "kv_cache_append_ragged"
    tensors = (k_new, v_new, k_cache, v_cache, cache_lengths)
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"{who}: tensors must live on the GPU (there is no CPU path)")
    if k_new.dtype not in (torch.bfloat16, torch.float16) or v_new.dtype != k_new.dtype:
        raise TypeError(f"{who}: k_new and v_new must share one of bfloat16 / float16")
    if k_cache.dtype != v_cache.dtype or k_cache.dtype not in (k_new.dtype, torch.float8_e4m3fn):
        raise TypeError(f"{who}: the caches must both be torch.float8_e4m3fn or the new rows' {k_new.dtype} (got {k_cache.dtype}, "
                        f"{v_cache.dtype}); e5m2 and fnuz caches have no kernel")
    fp8 = k_cache.dtype == torch.float8_e4m3fn
    if not fp8 and (k_scale is not None or v_scale is not None):
        raise ValueError(f"{who}: k_scale / v_scale go with a float8_e4m3fn cache; a 16-bit cache takes the rows' bits")
    paged = block_table is not None
    if k_new.dim() != 3 or k_new.shape[0] == 0 or v_new.shape != k_new.shape or k_cache.dim() != 4 or v_cache.shape != k_cache.shape or \
            k_cache.shape[1] != k_new.shape[1] or k_cache.shape[3] != k_new.shape[2]:
        raise ValueError(f"{who}: expected k_new, v_new [T, Hkv, D] (packed rows) and caches [B, Hkv, C, D] (paged: [pages, Hkv, pageSize, D]) "
                         f"(got {tuple(k_new.shape)}, {tuple(v_new.shape)}, {tuple(k_cache.shape)}, {tuple(v_cache.shape)})")
    T, Hkv, D = k_new.shape
    if cache_lengths.dim() != 1 or cache_lengths.dtype not in (torch.int32, torch.int64) or (not paged and cache_lengths.shape[0] != k_cache.shape[0]):
        raise ValueError(f"{who}: cache_lengths must be a GPU tensor [B] int32 or int64, B the caches' first dimension when they are "
                         f"contiguous (got {tuple(cache_lengths.shape)}, {cache_lengths.dtype})")
    B = int(cache_lengths.shape[0])
    _check_row_starts(who, row_starts, cache_lengths, max_rows)
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if t.stride(3) != 1 or any(st < 0 for st in t.stride()):
            raise ValueError(f"{who}: {name} must have a contiguous last dimension (a cache is written where it lies)")
    if paged:
        if block_table.dim() != 2 or block_table.shape[0] != B or block_table.dtype != torch.int32 or block_table.stride(1) != 1 or \
                not block_table.is_cuda:
            raise ValueError(f"{who}: block_table must be an int32 GPU tensor [B, pages per sequence] = [{B}, n] with a contiguous "
                             f"last dimension (got {tuple(block_table.shape)}, {block_table.dtype})")
        block_table = block_table.contiguous()   # (the row stride is the bound on the pages a sequence may name)
        kw = dict(pageSize=int(k_cache.shape[2]), blockTable=block_table, blockTableStride=int(block_table.shape[1]),
                  pageStrides=(int(k_cache.stride(0)), int(v_cache.stride(0))))
    else:
        kw = dict(column=int(k_cache.shape[2]))
    news = [_packed_operand(t) for t in (k_new, v_new)]
    new_strides = lambda t: (int(t.stride(0)) if T > 1 else Hkv * D, int(t.stride(1)) if Hkv > 1 else D, 0)  # noqa: E731
    key = (k_new.dtype, D, fp8)
    app = _APPENDERS.get(key)
    if app is None:
        app = _APPENDERS[key] = KVCacheAppend(D, P.BF16 if k_new.dtype == torch.bfloat16 else P.FP16, KVCachePrecision.E4M3 if fp8 else None)
    if fp8:
        kw.update(keyScale=_scale_operand(who, "k_scale", k_scale, Hkv, k_new.device), valueScale=_scale_operand(who, "v_scale", v_scale, Hkv, k_new.device))
    with torch.cuda.device(k_new.device):
        app.dispatch(news[0], news[1], k_cache, v_cache, stream=torch.cuda.current_stream(k_new.device).cuda_stream, rows=int(max_rows),
                     heads=Hkv, batches=B, cacheLengths=cache_lengths.to(torch.int32), rowStarts=row_starts.to(torch.int32), totalRows=T,
                     strides=dict(kNew=new_strides(news[0]), vNew=new_strides(news[1]), kCache=_cache_strides(k_cache, paged),
                                  vCache=_cache_strides(v_cache, paged)), **kw)


def _register_ragged_ops():
    """mfa::attention_prefill_ragged (`window`, `sink_tokens` 0: none) and mfa::kv_cache_append_ragged (include/mfa_ragged.h).  The other
    ops keep their schemas."""
    if not hasattr(torch.library, "custom_op"):
        return False
    try:
        torch.ops.mfa.attention_prefill_ragged  # noqa: B018 -- AttributeError when the op is not defined yet
        torch.ops.mfa.kv_cache_append_ragged  # noqa: B018
        return True
    except (AttributeError, RuntimeError):
        pass

    @torch.library.custom_op("mfa::attention_prefill_ragged", mutates_args=(), device_types="cuda")
    def _op_prefill_ragged(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor, row_starts: torch.Tensor,
                           max_rows: int, block_table: Optional[torch.Tensor], causal: bool, k_scale: Optional[torch.Tensor],
                           v_scale: Optional[torch.Tensor], window: int, sink_tokens: int,
                           sink_logits: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        return _run_prefill_ragged(q, k_cache, v_cache, cache_lengths, row_starts, max_rows, block_table, causal, k_scale, v_scale, window,
                                   (sink_tokens, sink_logits))

    @_op_prefill_ragged.register_fake
    def _op_prefill_ragged_fake(q, k_cache, v_cache, cache_lengths, row_starts, max_rows, block_table, causal, k_scale, v_scale, window,
                                sink_tokens, sink_logits):
        T, H, D = q.shape
        return q.new_empty((T, H, D)), q.new_empty((H, T), dtype=torch.float32)

    @torch.library.custom_op("mfa::kv_cache_append_ragged", mutates_args=("k_cache", "v_cache"), device_types="cuda")
    def _op_append_ragged(k_new: torch.Tensor, v_new: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                          row_starts: torch.Tensor, max_rows: int, block_table: Optional[torch.Tensor], k_scale: Optional[torch.Tensor],
                          v_scale: Optional[torch.Tensor]) -> None:
        _run_append_ragged(k_new, v_new, k_cache, v_cache, cache_lengths, row_starts, max_rows, block_table, k_scale, v_scale)

    @_op_append_ragged.register_fake
    def _op_append_ragged_fake(k_new, v_new, k_cache, v_cache, cache_lengths, row_starts, max_rows, block_table, k_scale, v_scale):
        return None

    return True


_HAVE_RAGGED_OPS = _register_ragged_ops()


def flash_prefill_ragged(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor, row_starts: torch.Tensor,
                         max_rows: int, block_table: Optional[torch.Tensor] = None, causal: bool = True,
                         k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None, return_lse: bool = False,
                         window: Optional[int] = None, sink_tokens: Optional[int] = None, sink_logits: Optional[torch.Tensor] = None):
    """flash_prefill for a RAGGED batch (a continuous-batching step: sequences with one new token beside prompt chunks): q [T, H, D]
    holds the new rows of all B sequences packed along the first axis, row_starts [B + 1] (GPU, int32 / int64, non-decreasing: the
    engine's cu_seqlens_q / query_start_loc) says where each sequence's rows begin, and max_rows (a host int) is the largest row
    count of any sequence -- rows of a sequence past it are not served.  q may be any view with a contiguous last dimension, a slice
    of a fused QKV projection included: it is read where it lies.  Caches, cache_lengths [B], block_table, scales, causal, window,
    sink_tokens and sink_logits: flash_prefill's.  Returns O [T, H, D], and with return_lse also L [H, T] fp32 in natural units; packed
    rows that no sequence owns come back uninitialised.  The launch starts no workgroup for row blocks that do not exist and computes,
    byte for byte, what flash_prefill computes for the same sequences padded to max_rows.  Forward only; goes through the op
    `mfa::attention_prefill_ragged` where torch has custom ops, so it traces under torch.compile."""
    if not (q.is_cuda and k_cache.is_cuda and v_cache.is_cuda and cache_lengths.is_cuda):
        raise RuntimeError("flash_prefill_ragged: tensors must live on the GPU (there is no CPU path)")
    for t in (q, k_cache, v_cache):
        if t.requires_grad:
            raise RuntimeError("flash_prefill_ragged is forward only (no autograd): detach the inputs; flash_attention is the differentiable entry")
    if window is not None or sink_tokens is not None or sink_logits is not None:
        # (_check_sinks reads the heads off a [B, H, R, D] query: the packed q as such a view)
        _check_sinks("flash_prefill_ragged", q.unsqueeze(0).transpose(1, 2) if q.dim() == 3 else q, window, causal, sink_tokens, sink_logits)
    if _HAVE_RAGGED_OPS:
        o, l = torch.ops.mfa.attention_prefill_ragged(q, k_cache, v_cache, cache_lengths, row_starts, max_rows, block_table, causal, k_scale,
                                                      v_scale, window or 0, sink_tokens or 0, sink_logits)
    else:
        o, l = _run_prefill_ragged(q, k_cache, v_cache, cache_lengths, row_starts, max_rows, block_table, causal, k_scale, v_scale,
                                   window or 0, (sink_tokens or 0, sink_logits))
    return (o, l * 0.6931471805599453) if return_lse else o


def kv_cache_append_ragged(k_new: torch.Tensor, v_new: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                           row_starts: torch.Tensor, max_rows: int, block_table: Optional[torch.Tensor] = None,
                           k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None) -> None:
    """kv_cache_append for a RAGGED batch, in ONE launch: k_new, v_new [T, Hkv, D] hold the new rows of all B sequences packed along
    the first axis (any view with a contiguous last dimension: the K and V slices of a fused QKV projection are read where they lie),
    row_starts [B + 1] and max_rows as flash_prefill_ragged's.  Row r of sequence b, which has qn_b = row_starts[b + 1] - row_starts[b]
    rows, goes to key cache_lengths[b] - qn_b + r (cache_lengths ALREADY INCLUDES the new tokens); kv_cache_append's drop rules, caches,
    quantisation and scales.  Goes through the op `mfa::kv_cache_append_ragged` (mutates_args) where torch has custom ops."""
    for t in (k_new, v_new, k_cache, v_cache):
        if t.requires_grad:
            raise RuntimeError("kv_cache_append_ragged writes in place and has no autograd: detach the inputs")
    if not all(t.is_cuda for t in (k_new, v_new, k_cache, v_cache, cache_lengths)):
        raise RuntimeError("kv_cache_append_ragged: tensors must live on the GPU (there is no CPU path)")
    if _HAVE_RAGGED_OPS:
        torch.ops.mfa.kv_cache_append_ragged(k_new, v_new, k_cache, v_cache, cache_lengths, row_starts, max_rows, block_table, k_scale, v_scale)
    else:
        _run_append_ragged(k_new, v_new, k_cache, v_cache, cache_lengths, row_starts, max_rows, block_table, k_scale, v_scale)
