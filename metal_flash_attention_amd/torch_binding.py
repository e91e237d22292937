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

    from metal_flash_attention_amd.torch_binding import kv_cache_compact, tree_path   # after a tree launch (tree_mask=): keep the accepted path
    accepted, counts = tree_path(tree_bits, leaf)                                      # bool [B, R, R] and a leaf per sequence
    cache_lengths = kv_cache_compact(k_cache, v_cache, cache_lengths, accepted, counts, rows=R)

forward  = AttentionKernelType.forward           -> O (the inputs' dtype, fused cast), L (fp32), both saved
backward = AttentionKernelType.backwardQuery     -> D, dQ      (needs O, dO, L)
           AttentionKernelType.backwardKeyValue  -> dK, dV     (needs L, D)
exactly the dispatch order of the reference's test (SquareAttentionTest.swift:355-368).  torch owns the
device memory and the stream; all arithmetic happens in libmfa_hip.so (no eager fallback: a missing
library or a CPU tensor raises).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

from .attention import (AttentionDecode, AttentionDecodeFP8, AttentionMLADecode, AttentionMLADecodeFP8, AttentionMLAPrefill, AttentionMLASparseDecode, AttentionMLASparseDecodeFP8, AttentionPrefill, AttentionDescriptor, AttentionKernel, AttentionKernelType,
                        AttentionOperand as Op, GEMMOperandPrecision as P, KVCacheAppend, KVCacheCompact,
                        KVCachePrecision, MLACacheAppend)

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


def pack_tree_mask(bits: torch.Tensor) -> torch.Tensor:
    """bool [..., R, R] (row r sees new token j: bits[..., r, j]; R <= 64) -> int64 [..., R], the bit pattern of the uint64 row masks
    flash_decode and flash_prefill take as tree_mask= (include/mfa_tree.h): bit j of entry r is bits[..., r, j]."""
    if bits.dim() < 2 or bits.shape[-1] != bits.shape[-2] or not 1 <= bits.shape[-1] <= 64:
        raise ValueError(f"pack_tree_mask: expected bool [..., R, R] with R from 1 to 64 (got {tuple(bits.shape)})")
    R = bits.shape[-1]
    weights = torch.tensor([(1 << j) if j < 63 else -(1 << 63) for j in range(R)], dtype=torch.int64, device=bits.device)
    return (bits.to(torch.int64) * weights).sum(-1)   # (distinct bits: the sum is their OR, bit 63 the sign)


def tree_path(tree_bits: torch.Tensor, leaf) -> Tuple[torch.Tensor, torch.Tensor]:
    """The accepted path of a speculation tree as kv_cache_compact takes it: tree_bits bool [..., R, R] (what pack_tree_mask takes; [R, R]
    with a leaf per sequence: one tree shared) and `leaf`, the index of the accepted leaf per sequence (an integer tensor [...], or an
    int) -> (accepted int32 [..., R] padded with -1, counts int32 [...]).  The path is the set bits of the leaf's row -- its ancestors and
    itself -- ordered by the popcount of each node's own row: depth order, root first, whatever the index order (a child may have a
    smaller index than its parent).  Computed where tree_bits lives; nothing is read back."""
    if tree_bits.dim() < 2 or tree_bits.shape[-1] != tree_bits.shape[-2] or not 1 <= tree_bits.shape[-1] <= 64:
        raise ValueError(f"tree_path: expected bool [..., R, R] with R from 1 to 64 (got {tuple(tree_bits.shape)})")
    R = tree_bits.shape[-1]
    leaf = torch.as_tensor(leaf, device=tree_bits.device).to(torch.int64)
    bits = tree_bits.to(torch.bool)
    if bits.dim() - 2 < leaf.dim():
        bits = bits.expand(*leaf.shape, R, R)
    if leaf.shape != bits.shape[:-2]:
        raise ValueError(f"tree_path: leaf must hold one index per tree, {tuple(bits.shape[:-2])} (got {tuple(leaf.shape)})")
    row = torch.gather(bits, -2, leaf[..., None, None].expand(*leaf.shape, 1, R)).squeeze(-2)   # [..., R]: the leaf's ancestors and itself
    depth = bits.sum(-1)                                                                        # [..., R]: each node's own popcount
    order = torch.argsort(torch.where(row, depth, R + 1), dim=-1, stable=True)                  # (nodes off the path sort last)
    counts = row.sum(-1)
    on_path = torch.arange(R, device=bits.device) < counts[..., None]
    return torch.where(on_path, order, -1).to(torch.int32), counts.to(torch.int32)


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


# ---- launches over a KV cache (include/mfa_decode.h, mfa_kvcache.h, mfa_prefill.h, mfa_window.h, mfa_sink.h, mfa_ragged.h): decode and prefill
# attention and the append that feeds them, forward only, per-sequence lengths on the device, contiguous or paged, 16-bit or e4m3
_HOSTS: Dict[Tuple, object] = {}
_FP8_DTYPES = tuple(getattr(torch, n) for n in ("float8_e4m3fn", "float8_e5m2", "float8_e4m3fnuz", "float8_e5m2fnuz") if hasattr(torch, n))
_LN2 = 0.6931471805599453


def _host(cls, dtype, D, fp8):
    """the host object of a launch: one per (class, 16-bit type, head dimension, e4m3 cache or not), kept"""
    key = (cls, dtype, D, bool(fp8))
    host = _HOSTS.get(key)
    if host is None:
        precision = P.BF16 if dtype == torch.bfloat16 else P.FP16
        if cls is AttentionDecode:
            host = (AttentionDecodeFP8 if fp8 else AttentionDecode)(D, precision)
        elif cls is KVCacheCompact:   # (no new rows: the cache's own type is all it takes)
            host = cls(D, KVCachePrecision.E4M3 if fp8 else precision)
        else:
            host = cls(D, precision, cachePrecision=KVCachePrecision.E4M3 if fp8 else None)
        _HOSTS[key] = host
    return host


def _cache_strides(t, paged):
    """(leadingDimension, headStride, batchStride) of a [B or pages, Hkv, keys, D] cache view, passed through as they are"""
    return (int(t.stride(2)) if t.shape[2] > 1 else int(t.shape[3]), int(t.stride(1)), 0 if paged else int(t.stride(0)))


def _scale_operand(who, name, t, heads, device):
    """a per-head scale as the kernels read it: fp32 [heads] on the cache's device, contiguous; None stays None (1.0)"""
    if t is None:
        return None
    if not t.is_cuda or t.device != device:
        raise RuntimeError(f"{who}: {name} must live on the GPU of the cache (the host never reads a scale)")
    if t.shape != (heads,) or t.dtype != torch.float32:
        raise ValueError(f"{who}: {name} must be float32 [Hkv] = [{heads}] (got {tuple(t.shape)}, {t.dtype})")
    return t.contiguous()


def _check_scales(who, fp8, k_scale, v_scale, write=False):
    if not fp8 and (k_scale is not None or v_scale is not None):
        raise ValueError(f"{who}: k_scale / v_scale go with a float8_e4m3fn cache; a 16-bit cache "
                         + ("takes the rows' bits" if write else "holds the values themselves"))


def _check_lengths(who, name, t, batches, tail=""):
    """a per-sequence length array: [batches] (None: any count) int32 or int64 on the GPU"""
    if not t.is_cuda or t.dim() != 1 or (batches is not None and t.shape[0] != batches) or t.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{who}: {name} must be a GPU tensor [B]{'' if batches is None else f' = [{batches}]'} int32 or int64{tail} "
                         f"(got {tuple(t.shape)}, {t.dtype})")


def _cache_layout(who, k_cache, v_cache, block_table, B, write):
    """The caches [B or pages, Hkv, keys, D] of a launch over `B` sequences as they lie, checked -- a contiguous last dimension, the block
    table -- and described -> keywords of a host class's dispatch: the paging, `column`, and `strides` with the caches' entries.  `write`:
    the launch writes the cache (append, compact) -- the words and the operand names say so, and the block table is handed over contiguous
    with its width as the stride, the bound on the pages a sequence may name."""
    paged = block_table is not None
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if t.stride(3) != 1 or any(st < 0 for st in t.stride()):
            raise ValueError(f"{who}: {name} must have a contiguous last dimension (a cache is "
                             f"{'written where it lies' if write else 'never copied'})")
    kw = {}
    if paged:
        if block_table.dim() != 2 or block_table.shape[0] != B or block_table.dtype != torch.int32 or block_table.stride(1) != 1 or \
                not block_table.is_cuda:
            raise ValueError(f"{who}: block_table must be an int32 GPU tensor [B, pages per sequence] = [{B}, n] with a contiguous "
                             f"last dimension (got {tuple(block_table.shape)}, {block_table.dtype})")
        kw.update(pageSize=int(k_cache.shape[2]), blockTable=block_table.contiguous() if write else block_table,
                  blockTableStride=int(block_table.shape[1] if write else block_table.stride(0)),
                  pageStrides=(int(k_cache.stride(0)), int(v_cache.stride(0))))
    if not (write and paged):   # (a paged write takes no column: its kernel drops a row whose page lies past the table's row)
        kw.update(column=int(k_cache.shape[2]) * (int(block_table.shape[1]) if paged else 1))
    k_name, v_name = ("kCache", "vCache") if write else ("K", "V")
    kw.update(strides={k_name: _cache_strides(k_cache, paged), v_name: _cache_strides(v_cache, paged)})
    return kw


def _cache_side(who, news, k_cache, v_cache, cache_lengths, block_table, k_scale, v_scale, *, packed=False, write=False, fp8=None):
    """Validates the cache side of a launch against its new operand(s) `news` -- q [B, H, R, D], or k_new and v_new [B, Hkv, R, D]; `packed`:
    [T, H, D], a ragged batch -- and describes it -> (fp8, B, keywords of the host class's dispatch: the lengths, the paging, the scales,
    `column`, and `strides` with the caches' entries (_cache_layout), to which the caller adds its operands').  `write`: the launch writes
    the cache (append) -- the rows' heads are the caches' and the words say so.  `fp8`: what the caller's op says the caches are (None:
    what they say)."""
    new, names = news[0], "k_new, v_new" if write else "q"
    if not all(t.is_cuda for t in (*news, k_cache, v_cache, cache_lengths)):
        raise RuntimeError(f"{who}: tensors must live on the GPU (there is no CPU path)")
    if new.dtype not in (torch.bfloat16, torch.float16) or any(t.dtype != new.dtype for t in news):
        raise TypeError(f"{who}: " + ("k_new and v_new must share one of bfloat16 / float16" if write else "q must be bfloat16 or float16"))
    if fp8 is None:
        fp8 = k_cache.dtype in _FP8_DTYPES or v_cache.dtype in _FP8_DTYPES
    if k_cache.dtype != v_cache.dtype or k_cache.dtype != (torch.float8_e4m3fn if fp8 else new.dtype):
        if write:
            raise TypeError(f"{who}: the caches must both be torch.float8_e4m3fn or the new rows' {new.dtype} (got {k_cache.dtype}, "
                            f"{v_cache.dtype}); e5m2 and fnuz caches have no kernel")
        if fp8:
            raise TypeError(f"{who}: an FP8 KV cache is torch.float8_e4m3fn for both K and V (got {k_cache.dtype}, {v_cache.dtype}); "
                            "e5m2 and fnuz caches have no kernel")
        raise TypeError(f"{who}: q and the caches must share one of bfloat16 / float16 (or the caches are float8_e4m3fn)")
    _check_scales(who, fp8, k_scale, v_scale, write)
    paged = block_table is not None
    n = 3 if packed else 4
    if any(t.dim() != n or t.shape != new.shape for t in news) or k_cache.dim() != 4 or v_cache.shape != k_cache.shape or \
            new.shape[-1] != k_cache.shape[3] or k_cache.shape[1] == 0 or \
            (new.shape[1] != k_cache.shape[1] if write else new.shape[1] % k_cache.shape[1] != 0) or \
            (new.shape[0] == 0 if packed else not paged and k_cache.shape[0] != new.shape[0]):
        heads = "Hkv" if write else "H"
        raise ValueError(f"{who}: expected {names} {f'[T, {heads}, D] (packed rows)' if packed else f'[B, {heads}, R, D]'} and caches "
                         f"[B, Hkv, C, D] (paged: [pages, Hkv, pageSize, D]){'' if write else ' with H a multiple of Hkv'} "
                         f"(got {', '.join(str(tuple(t.shape)) for t in (*news, k_cache, v_cache))})")
    Hkv = k_cache.shape[1]
    if packed:
        _check_lengths(who, "cache_lengths", cache_lengths, None if paged else k_cache.shape[0], ", B the caches' first dimension when they are contiguous")
    else:
        _check_lengths(who, "cache_lengths", cache_lengths, new.shape[0])
    B = int(cache_lengths.shape[0])
    kw = _cache_layout(who, k_cache, v_cache, block_table, B, write)
    kw.update(cacheLengths=cache_lengths.to(torch.int32))   # (no copy when it already is; stays on the device)
    if fp8:
        kw.update(keyScale=_scale_operand(who, "k_scale", k_scale, Hkv, new.device), valueScale=_scale_operand(who, "v_scale", v_scale, Hkv, new.device))
    return fp8, B, kw


def _new_operand(t):
    """a [B, heads, R, D] operand as the kernels read it, and its strides: any view with a contiguous last dimension is taken where it lies"""
    t = t if t.stride(3) == 1 and all(st >= 0 for st in t.stride()) else t.contiguous()
    return t, (int(t.stride(2)) if t.shape[2] > 1 else int(t.shape[3]), int(t.stride(1)), int(t.stride(0)))


def _packed_operand(t):
    """the same of a packed [T, heads, D] operand: a view with a contiguous last dimension and 16-byte rows is taken where it lies (a slice
    of a fused QKV projection: strides, not a copy)"""
    ok = t.stride(2) == 1 and all(st >= 0 for st in t.stride()) and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0 and t.data_ptr() % 16 == 0
    t = t if ok else t.contiguous()
    T, heads, D = t.shape
    return t, (int(t.stride(0)) if T > 1 else heads * D, int(t.stride(1)) if heads > 1 else D, 0)


def _attend(host, q, k_cache, v_cache, l_shape, kw, window, sinks, softcap, workspace=False, tree=None, pieces=None):
    """the launch of a decode or prefill host object over `kw`, on q's device and torch's current stream -> (O, L).  window, sinks -- (sink
    tokens or 0, sink logits or None) -- and softcap: None is none, and anything else reaches the entries of its header, a window 0 and
    sinks (0, None) too.  (Rows the launch does not own -- past q_lengths[b], or packed rows of no sequence -- are not written: no memset
    is spent on them, they come back uninitialised)"""
    if window is not None:
        kw["window"] = int(window)
    if sinks is not None:   # (sink tokens or 0, sink logits or None): the entries of include/mfa_sink.h
        kw["sinkTokens"], kw["sinkLogits"] = int(sinks[0]), sinks[1]
    if softcap is not None:   # the entries of include/mfa_softcap.h
        kw["softcap"] = float(softcap)
    if tree is not None:   # [R] or [B, R] int64 on the GPU: the entries of include/mfa_tree.h
        kw["treeMasks"], kw["treeBatchStride"] = tree, int(tree.stride(0)) if tree.dim() == 2 else 0
    if pieces is not None:   # prefill cut along the keys (0: the host's plan): the entries of include/mfa_split.h
        kw["pieces"] = int(pieces)
    o = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    l = torch.empty(l_shape, dtype=torch.float32, device=q.device)
    if workspace:
        need = host.workspaceSize(**kw)
        kw.update(workspace=torch.empty(need, dtype=torch.uint8, device=q.device) if need else None)
    with torch.cuda.device(q.device):
        host.dispatch(q, k_cache, v_cache, o, l, stream=torch.cuda.current_stream(q.device).cuda_stream, **kw)
    return o, l


def _run_decode(q, k_cache, v_cache, cache_lengths, block_table, causal, fp8=False, k_scale=None, v_scale=None, window=None, sinks=None, softcap=None,
                tree=None):
    """`fp8`: what the op says the caches are (None: what they say themselves -- the window, sink and soft-cap ops serve 16-bit and e4m3 caches alike)"""
    if fp8 is None:
        fp8 = k_cache.dtype in _FP8_DTYPES or v_cache.dtype in _FP8_DTYPES
    fp8, B, kw = _cache_side("flash_decode", (q,), k_cache, v_cache, cache_lengths, block_table, k_scale, v_scale, fp8=fp8)
    q, kw["strides"]["Q"] = _new_operand(q)
    _B, H, R, D = q.shape
    kw.update(rows=R, heads=H, batches=B, headsPerKeyValue=H // k_cache.shape[1], causal=bool(causal))
    return _attend(_host(AttentionDecode, q.dtype, D, fp8), q, k_cache, v_cache, (B, H, R), kw, window, sinks, softcap, workspace=True,
                   tree=None if tree is None else _tree_operand("flash_decode", tree, B, R))


def _sinks_or_none(sink_tokens, sink_logits):
    """the op boundary: an op's 0 sink tokens and None logits are no sinks (None inside this module), as its window 0 is no window"""
    return (sink_tokens, sink_logits) if sink_tokens or sink_logits is not None else None


def _run_prefill(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale, window=None, sinks=None, softcap=None,
                 tree=None, pieces=None):
    """`pieces`: None is the launch that is not cut along the keys; 0 the host's plan, 2 .. 64 as given -- the workspace is allocated here"""
    who = "flash_prefill"
    fp8, B, kw = _cache_side(who, (q,), k_cache, v_cache, cache_lengths, block_table, k_scale, v_scale)
    if q_lengths is not None:
        _check_lengths(who, "q_lengths", q_lengths, B)
    q, kw["strides"]["Q"] = _new_operand(q)
    _B, H, R, D = q.shape
    kw.update(rows=R, heads=H, batches=B, headsPerKeyValue=H // k_cache.shape[1], causal=bool(causal),
              queryLengths=None if q_lengths is None else q_lengths.to(torch.int32))
    return _attend(_host(AttentionPrefill, q.dtype, D, fp8), q, k_cache, v_cache, (B, H, R), kw, window, sinks, softcap,
                   workspace=pieces is not None, tree=None if tree is None else _tree_operand(who, tree, B, R), pieces=pieces)


def _run_prefill_ragged(q, k_cache, v_cache, cache_lengths, row_starts, max_rows, block_table, causal, k_scale, v_scale, window, sinks, softcap=None):
    """the body of the two ragged ops, in their spelling: `window` 0 and `sinks` None or (0, None) are none, translated here for both"""
    who = "flash_prefill_ragged"
    fp8, B, kw = _cache_side(who, (q,), k_cache, v_cache, cache_lengths, block_table, k_scale, v_scale, packed=True)
    _check_row_starts(who, row_starts, cache_lengths, max_rows)
    q, kw["strides"]["Q"] = _packed_operand(q)
    T, H, D = q.shape
    kw.update(rows=int(max_rows), heads=H, batches=B, headsPerKeyValue=H // k_cache.shape[1], causal=bool(causal),
              rowStarts=row_starts.to(torch.int32), totalRows=T)
    return _attend(_host(AttentionPrefill, q.dtype, D, fp8), q, k_cache, v_cache, (H, T), kw, window or None, sinks and _sinks_or_none(*sinks), softcap)


def _append(who, operand, k_new, v_new, k_cache, v_cache, cache_lengths, block_table, k_scale, v_scale, row_starts=None, max_rows=None):
    packed = operand is _packed_operand
    fp8, B, kw = _cache_side(who, (k_new, v_new), k_cache, v_cache, cache_lengths, block_table, k_scale, v_scale, packed=packed, write=True)
    if packed:
        _check_row_starts(who, row_starts, cache_lengths, max_rows)
        kw.update(rows=int(max_rows), rowStarts=row_starts.to(torch.int32), totalRows=k_new.shape[0])
    else:
        kw.update(rows=k_new.shape[2])
    (k_new, kw["strides"]["kNew"]), (v_new, kw["strides"]["vNew"]) = operand(k_new), operand(v_new)
    with torch.cuda.device(k_new.device):
        _host(KVCacheAppend, k_new.dtype, k_new.shape[-1], fp8).dispatch(
            k_new, v_new, k_cache, v_cache, stream=torch.cuda.current_stream(k_new.device).cuda_stream, heads=k_new.shape[1], batches=B, **kw)


def _run_append(k_new, v_new, k_cache, v_cache, cache_lengths, block_table, k_scale, v_scale):
    _append("kv_cache_append", _new_operand, k_new, v_new, k_cache, v_cache, cache_lengths, block_table, k_scale, v_scale)


def _run_append_ragged(k_new, v_new, k_cache, v_cache, cache_lengths, row_starts, max_rows, block_table, k_scale, v_scale):
    _append("kv_cache_append_ragged", _packed_operand, k_new, v_new, k_cache, v_cache, cache_lengths, block_table, k_scale, v_scale, row_starts, max_rows)


def _run_compact(k_cache, v_cache, cache_lengths, accepted, accepted_counts, rows, q_lengths, block_table):
    """kv_cache_compact's launch (include/mfa_compact.h) on the caches' device and torch's current stream -> new lengths int32 [B]"""
    who = "kv_cache_compact"
    if not all(t.is_cuda for t in (k_cache, v_cache, cache_lengths, accepted, accepted_counts)):
        raise RuntimeError(f"{who}: tensors must live on the GPU (there is no CPU path)")
    for name, t in (("v_cache", v_cache), ("cache_lengths", cache_lengths), ("accepted", accepted), ("accepted_counts", accepted_counts),
                    ("q_lengths", q_lengths), ("block_table", block_table)):
        if t is not None and (not t.is_cuda or t.device != k_cache.device):
            raise RuntimeError(f"{who}: {name} must live on the GPU of the cache (the host never reads it)")
    if k_cache.dtype != v_cache.dtype or k_cache.dtype not in (torch.bfloat16, torch.float16, torch.float8_e4m3fn):
        raise TypeError(f"{who}: the caches must both be bfloat16, float16 or torch.float8_e4m3fn (got {k_cache.dtype}, {v_cache.dtype}); "
                        "e5m2 and fnuz caches have no kernel")
    paged = block_table is not None
    if k_cache.dim() != 4 or v_cache.shape != k_cache.shape or k_cache.shape[1] == 0:
        raise ValueError(f"{who}: expected caches [B, Hkv, C, D] (paged: [pages, Hkv, pageSize, D]) of one shape "
                         f"(got {tuple(k_cache.shape)}, {tuple(v_cache.shape)})")
    _check_lengths(who, "cache_lengths", cache_lengths, None if paged else k_cache.shape[0], ", B the caches' first dimension when they are contiguous")
    B = int(cache_lengths.shape[0])
    if isinstance(rows, bool) or not isinstance(rows, int) or not 1 <= rows <= 64:
        raise ValueError(f"{who}: rows must be an int from 1 to 64, the rows of the tree launch (the host never reads a length), not {rows!r}")
    if accepted.dim() != 2 or accepted.shape[0] != B or accepted.dtype != torch.int32 or accepted.shape[1] == 0 or accepted.stride(1) != 1:
        raise ValueError(f"{who}: accepted must be an int32 GPU tensor [B, A] = [{B}, A] with a contiguous last dimension, the node indices of "
                         f"every sequence's path in path order (tree_path; got {tuple(accepted.shape)}, {accepted.dtype})")
    if accepted.shape[1] > 64:
        raise ValueError(f"{who}: accepted holds at most 64 nodes per sequence, one bit of a uint64 tree mask each (got {tuple(accepted.shape)})")
    _check_lengths(who, "accepted_counts", accepted_counts, B)
    if q_lengths is not None:
        _check_lengths(who, "q_lengths", q_lengths, B)
    kw = _cache_layout(who, k_cache, v_cache, block_table, B, True)
    if accepted.stride(0) < accepted.shape[1]:   # (an expanded row: one path shared is given a row per sequence)
        accepted = accepted.contiguous()
    kw.update(cacheLengths=cache_lengths.to(torch.int32), acceptedCounts=accepted_counts.to(torch.int32), accepted=accepted,
              acceptedStride=int(accepted.stride(0)), maxAccepted=int(accepted.shape[1]),
              queryLengths=None if q_lengths is None else q_lengths.to(torch.int32))
    new_lengths = torch.empty((B,), dtype=torch.int32, device=k_cache.device)
    host = _host(KVCacheCompact, k_cache.dtype, int(k_cache.shape[3]), k_cache.dtype == torch.float8_e4m3fn)
    with torch.cuda.device(k_cache.device):
        host.dispatch(k_cache, v_cache, stream=torch.cuda.current_stream(k_cache.device).cuda_stream, rows=rows, heads=int(k_cache.shape[1]),
                      batches=B, newLengths=new_lengths, **kw)
    return new_lengths


def _check_mla(who, q, kv_cache, cache_lengths, block_table, softmax_scale, pieces, fp8=False):
    """the operands of flash_mla_decode (include/mfa_mla.h) and, `fp8`, of flash_mla_decode_fp8 (include/mfa_mla_cache.h), checked where
    the public function and the op both pass: shapes, types, devices"""
    Dk = AttentionMLADecode.HEAD_DIMENSION
    if not all(t.is_cuda for t in (q, kv_cache, cache_lengths)) or (block_table is not None and not block_table.is_cuda):
        raise RuntimeError(f"{who}: tensors must live on the GPU (there is no CPU path)")
    if q.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError(f"{who}: q must be bfloat16 or float16 (got {q.dtype})")
    if fp8 and kv_cache.dtype != torch.float8_e4m3fn:
        raise TypeError(f"{who}: the latent cache must be torch.float8_e4m3fn (got {kv_cache.dtype}); a 16-bit latent cache is flash_mla_decode's, "
                        "and e5m2 and fnuz caches have no kernel")
    if not fp8 and kv_cache.dtype != q.dtype:
        raise TypeError(f"{who}: q and the latent cache must share one of bfloat16 / float16 (got {q.dtype}, {kv_cache.dtype}); e4m3 latent "
                        "caches have no kernel in this function: flash_mla_decode_fp8 reads them")
    paged = block_table is not None
    if q.dim() != 4 or kv_cache.dim() != 3 or q.shape[3] != Dk or kv_cache.shape[2] != Dk or (not paged and kv_cache.shape[0] != q.shape[0]):
        raise ValueError(f"{who}: expected q [B, H, R, {Dk}] and kv_cache [B, C, {Dk}] (paged: [pages, pageSize, {Dk}]): one row of the 512-wide "
                         f"latent and the 64-wide rotary part per key (got {tuple(q.shape)}, {tuple(kv_cache.shape)})")
    if kv_cache.stride(2) != 1 or any(st < 0 for st in kv_cache.stride()):
        raise ValueError(f"{who}: kv_cache must have a contiguous last dimension (a cache is never copied)")
    B = int(q.shape[0])
    _check_lengths(who, "cache_lengths", cache_lengths, B)
    if paged and (block_table.dim() != 2 or block_table.shape[0] != B or block_table.dtype != torch.int32 or block_table.stride(1) != 1):
        raise ValueError(f"{who}: block_table must be an int32 GPU tensor [B, pages per sequence] = [{B}, n] with a contiguous last dimension "
                         f"(got {tuple(block_table.shape)}, {block_table.dtype})")
    if isinstance(softmax_scale, bool) or not isinstance(softmax_scale, (int, float)) or not math.isfinite(softmax_scale) or not softmax_scale > 0:
        raise ValueError(f"{who}: softmax_scale must be a finite number > 0, the model's own softmax scale in natural units (it is not "
                         f"1 / sqrt(576) and has no default), not {softmax_scale!r}")
    if isinstance(pieces, bool) or not isinstance(pieces, int) or not 0 <= pieces <= 64:
        raise ValueError(f"{who}: pieces must be an int from 0 to 64 (None or 0: the host's plan, 1: unsplit), not {pieces!r}")


def _check_mla_indices(who, q, indices):
    """the lists of flash_mla_sparse_decode (include/mfa_mla_sparse.h): int32 [B, R, topk] on q's GPU, read where they lie"""
    if not indices.is_cuda or indices.device != q.device:
        raise RuntimeError(f"{who}: indices must live on the GPU of q (the host never reads a list)")
    if indices.dtype != torch.int32:
        raise TypeError(f"{who}: indices must be int32 key positions (got {indices.dtype})")
    if indices.dim() != 3 or tuple(indices.shape[:2]) != (int(q.shape[0]), int(q.shape[2])) or indices.shape[2] < 1:
        raise ValueError(f"{who}: indices must be [B, R, topk] = [{int(q.shape[0])}, {int(q.shape[2])}, topk >= 1], one list per sequence and row, "
                         f"shared by all heads (got {tuple(indices.shape)})")
    if indices.stride(2) != 1 or any(st < 0 for st in indices.stride()):
        raise ValueError(f"{who}: indices must have a contiguous last dimension (a list is never copied)")


def _run_mla_decode(q, kv_cache, cache_lengths, block_table, causal, softmax_scale, pieces, fp8=False, kv_scale=None, indices=None):
    """flash_mla_decode's launch (include/mfa_mla.h) on q's device and torch's current stream -> (O [B, H, R, 512], L [B, H, R] base 2);
    the workspace of a launch cut along the keys is allocated here.  `fp8`: flash_mla_decode_fp8's, over an e4m3 latent cache with
    `kv_scale` (include/mfa_mla_cache.h) -- the strides of such a cache count bytes, which are its elements"""
    who = ("flash_mla_sparse_decode_fp8" if fp8 else "flash_mla_sparse_decode") if indices is not None else "flash_mla_decode_fp8" if fp8 else "flash_mla_decode"
    _check_mla(who, q, kv_cache, cache_lengths, block_table, softmax_scale, pieces, fp8)
    if indices is not None:
        _check_mla_indices(who, q, indices)
    paged = block_table is not None
    q, q_strides = _new_operand(q)
    B, H, R, _Dk = q.shape
    Dv = AttentionMLADecode.VALUE_DIMENSION
    ld = int(kv_cache.stride(1)) if kv_cache.shape[1] > 1 else int(kv_cache.shape[2])
    kw = dict(rows=R, heads=H, batches=B, causal=bool(causal), scale=float(softmax_scale), pieces=int(pieces),
              cacheLengths=cache_lengths.to(torch.int32), strides={"Q": q_strides, "KV": (ld, 0, 0 if paged else int(kv_cache.stride(0)))},
              column=int(kv_cache.shape[1]) * (int(block_table.shape[1]) if paged else 1))
    if paged:
        kw.update(pageSize=int(kv_cache.shape[1]), blockTable=block_table, blockTableStride=int(block_table.stride(0)), pageStride=int(kv_cache.stride(0)))
    cls = (AttentionMLASparseDecodeFP8 if fp8 else AttentionMLASparseDecode) if indices is not None else AttentionMLADecodeFP8 if fp8 else AttentionMLADecode
    if fp8:
        kw.update(kvScale=_latent_scale(who, kv_scale, kv_cache.device))
    if indices is not None:   # `indices`: flash_mla_sparse_decode's lists (include/mfa_mla_sparse.h), passed where they lie
        topk = int(indices.shape[2])
        kw.update(indices=indices, topk=topk, indexStrides=(int(indices.stride(1)) if R > 1 else topk, int(indices.stride(0)) if B > 1 else R * topk))
    key = (cls, q.dtype)
    host = _HOSTS.get(key)
    if host is None:
        host = _HOSTS[key] = cls(P.BF16 if q.dtype == torch.bfloat16 else P.FP16)
    o = torch.empty((B, H, R, Dv), dtype=q.dtype, device=q.device)
    l = torch.empty((B, H, R), dtype=torch.float32, device=q.device)
    need = host.workspaceSize(**kw)
    kw.update(workspace=torch.empty(need, dtype=torch.uint8, device=q.device) if need else None)
    with torch.cuda.device(q.device):
        host.dispatch(q, kv_cache, o, l, stream=torch.cuda.current_stream(q.device).cuda_stream, **kw)
    return o, l


def _run_mla_prefill(q, kv_cache, cache_lengths, q_lengths, block_table, causal, softmax_scale):
    """flash_mla_prefill's launch (include/mfa_mla_prefill.h) on q's device and torch's current stream -> (O [B, H, R, 512], L [B, H, R]
    base 2).  (Rows past q_lengths[b] are not written: no memset is spent on them, they come back uninitialised)"""
    who = "flash_mla_prefill"
    _check_mla(who, q, kv_cache, cache_lengths, block_table, softmax_scale, 0)
    B = int(q.shape[0])
    if q_lengths is not None:
        _check_lengths(who, "q_lengths", q_lengths, B)
    paged = block_table is not None
    q, q_strides = _new_operand(q)
    _B, H, R, _Dk = q.shape
    Dv = AttentionMLAPrefill.VALUE_DIMENSION
    ld = int(kv_cache.stride(1)) if kv_cache.shape[1] > 1 else int(kv_cache.shape[2])
    kw = dict(rows=R, heads=H, batches=B, causal=bool(causal), scale=float(softmax_scale), cacheLengths=cache_lengths.to(torch.int32),
              queryLengths=None if q_lengths is None else q_lengths.to(torch.int32),
              strides={"Q": q_strides, "KV": (ld, 0, 0 if paged else int(kv_cache.stride(0)))},
              column=int(kv_cache.shape[1]) * (int(block_table.shape[1]) if paged else 1))
    if paged:
        kw.update(pageSize=int(kv_cache.shape[1]), blockTable=block_table, blockTableStride=int(block_table.stride(0)), pageStride=int(kv_cache.stride(0)))
    key = (AttentionMLAPrefill, q.dtype)
    host = _HOSTS.get(key)
    if host is None:
        host = _HOSTS[key] = AttentionMLAPrefill(P.BF16 if q.dtype == torch.bfloat16 else P.FP16)
    o = torch.empty((B, H, R, Dv), dtype=q.dtype, device=q.device)
    l = torch.empty((B, H, R), dtype=torch.float32, device=q.device)
    with torch.cuda.device(q.device):
        host.dispatch(q, kv_cache, o, l, stream=torch.cuda.current_stream(q.device).cuda_stream, **kw)
    return o, l


def _latent_scale(who, t, device):
    """kv_scale as the kernels read it: fp32 [1] on the cache's device; None stays None (1.0)"""
    if t is None:
        return None
    if not t.is_cuda or t.device != device:
        raise RuntimeError(f"{who}: kv_scale must live on the GPU of the cache (the host never reads a scale)")
    if t.shape != (1,) or t.dtype != torch.float32:
        raise ValueError(f"{who}: kv_scale must be float32 [1], one scale for the whole cache row (got {tuple(t.shape)}, {t.dtype})")
    return t


def _check_mla_append(who, latent_new, rope_new, kv_cache, cache_lengths, block_table, kv_scale):
    """the operands of mla_cache_append (include/mfa_mla_cache.h), checked where the public function and the op both pass -> the cache is e4m3"""
    Dl, Dr = MLACacheAppend.LATENT_DIMENSION, MLACacheAppend.ROPE_DIMENSION
    if not all(t.is_cuda for t in (latent_new, rope_new, kv_cache, cache_lengths)) or (block_table is not None and not block_table.is_cuda):
        raise RuntimeError(f"{who}: tensors must live on the GPU (there is no CPU path)")
    if latent_new.dtype not in (torch.bfloat16, torch.float16) or rope_new.dtype != latent_new.dtype:
        raise TypeError(f"{who}: latent_new and rope_new must share one of bfloat16 / float16 (got {latent_new.dtype}, {rope_new.dtype})")
    fp8 = kv_cache.dtype == torch.float8_e4m3fn
    if not fp8 and kv_cache.dtype != latent_new.dtype:
        raise TypeError(f"{who}: the latent cache must be the rows' 16-bit type or torch.float8_e4m3fn (got {kv_cache.dtype} beside "
                        f"{latent_new.dtype}); e5m2 and fnuz caches have no kernel")
    paged = block_table is not None
    if (latent_new.dim() != 3 or rope_new.dim() != 3 or kv_cache.dim() != 3 or latent_new.shape[2] != Dl or rope_new.shape[2] != Dr
            or rope_new.shape[:2] != latent_new.shape[:2] or latent_new.shape[1] == 0 or kv_cache.shape[2] != Dl + Dr
            or (not paged and kv_cache.shape[0] != latent_new.shape[0])):
        raise ValueError(f"{who}: expected latent_new [B, R, {Dl}], rope_new [B, R, {Dr}] and kv_cache [B, C, {Dl + Dr}] (paged: [pages, pageSize, "
                         f"{Dl + Dr}]) (got {tuple(latent_new.shape)}, {tuple(rope_new.shape)}, {tuple(kv_cache.shape)})")
    if kv_cache.stride(2) != 1 or any(st < 0 for st in kv_cache.stride()):
        raise ValueError(f"{who}: kv_cache must have a contiguous last dimension (a cache is written where it lies)")
    B = int(latent_new.shape[0])
    _check_lengths(who, "cache_lengths", cache_lengths, B)
    if paged and (block_table.dim() != 2 or block_table.shape[0] != B or block_table.dtype != torch.int32 or block_table.shape[1] == 0):
        raise ValueError(f"{who}: block_table must be an int32 GPU tensor [B, pages per sequence] = [{B}, n] "
                         f"(got {tuple(block_table.shape)}, {block_table.dtype})")
    if not fp8 and kv_scale is not None:
        raise ValueError(f"{who}: kv_scale goes with a float8_e4m3fn cache; a 16-bit cache takes the rows' bits")
    _latent_scale(who, kv_scale, kv_cache.device)
    return fp8


def _latent_rows(t):
    """a [B, R, width] source as the kernel reads it, and its (leadingDimension, batchStride): a view with a contiguous last dimension and
    16-byte rows is taken where it lies (a slice of a fused projection: strides, not a copy)"""
    ok = t.stride(2) == 1 and all(st >= 0 for st in t.stride()) and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0 and t.data_ptr() % 16 == 0
    t = t if ok else t.contiguous()
    return t, (int(t.stride(1)) if t.shape[1] > 1 else int(t.shape[2]), int(t.stride(0)))


def _run_mla_append(latent_new, rope_new, kv_cache, cache_lengths, block_table, kv_scale):
    """mla_cache_append's launch (include/mfa_mla_cache.h) on the cache's device and torch's current stream"""
    who = "mla_cache_append"
    fp8 = _check_mla_append(who, latent_new, rope_new, kv_cache, cache_lengths, block_table, kv_scale)
    paged = block_table is not None
    (latent_new, latent_strides), (rope_new, rope_strides) = _latent_rows(latent_new), _latent_rows(rope_new)
    B, R, _Dl = latent_new.shape
    ld = int(kv_cache.stride(1)) if kv_cache.shape[1] > 1 else int(kv_cache.shape[2])
    kw = dict(rows=R, batches=B, cacheLengths=cache_lengths.to(torch.int32), column=0 if paged else int(kv_cache.shape[1]),
              strides={"latentNew": latent_strides, "ropeNew": rope_strides, "kvCache": (ld, 0 if paged else int(kv_cache.stride(0)))})
    if paged:   # the table contiguous, its width the bound on the pages a sequence may name
        block_table = block_table.contiguous()
        kw.update(pageSize=int(kv_cache.shape[1]), blockTable=block_table, blockTableStride=int(block_table.shape[1]), pageStride=int(kv_cache.stride(0)))
    if fp8:
        kw.update(kvScale=_latent_scale(who, kv_scale, kv_cache.device))
    key = (MLACacheAppend, latent_new.dtype, fp8)
    host = _HOSTS.get(key)
    if host is None:
        host = _HOSTS[key] = MLACacheAppend(P.BF16 if latent_new.dtype == torch.bfloat16 else P.FP16, KVCachePrecision.E4M3 if fp8 else None)
    with torch.cuda.device(kv_cache.device):
        host.dispatch(latent_new, rope_new, kv_cache, stream=torch.cuda.current_stream(kv_cache.device).cuda_stream, **kw)


def _check_tree(who, q, tree_mask, causal, window, softcap):
    """tree_mask= of a public function: an int64 tensor [R] or [B, R] on q's device; causal, no cap, a window of at least R"""
    R, B = (q.shape[2], q.shape[0]) if q.dim() == 4 else (None, None)
    if not isinstance(tree_mask, torch.Tensor) or tree_mask.dtype != torch.int64 or R is None or tuple(tree_mask.shape) not in ((R,), (B, R)):
        got = f"{tuple(tree_mask.shape)}, {tree_mask.dtype}" if isinstance(tree_mask, torch.Tensor) else type(tree_mask).__name__
        raise ValueError(f"{who}: tree_mask must be an int64 tensor [R] = [{R}] (one tree for every sequence) or [B, R] = [{B}, {R}], the bit "
                         f"patterns of uint64 row masks (pack_tree_mask; got {got})")
    if tree_mask.device != q.device:
        raise RuntimeError(f"{who}: tree_mask must live on q's device (the host never reads a mask)")
    if not causal:
        raise ValueError(f"{who}: tree_mask needs causal=True (the tree replaces the causal rule among the new rows)")
    if softcap is not None:
        raise ValueError(f"{who}: tree_mask and softcap together have no kernel (include/mfa_tree.h)")
    if window is not None and isinstance(window, int) and window < R:
        raise ValueError(f"{who}: tree_mask needs a window of at least R = {R} keys (an ancestor could fall outside a descendant's window), not {window}")


def _tree_operand(who, tree, B, R):
    """the masks as the kernels read them: rows of R contiguous uint64"""
    if tuple(tree.shape) not in ((R,), (B, R)) or tree.dtype != torch.int64:
        raise ValueError(f"{who}: tree_mask must be int64 [R] = [{R}] or [B, R] = [{B}, {R}] (got {tuple(tree.shape)}, {tree.dtype})")
    return tree if tree.stride(-1) == 1 and (tree.dim() == 1 or tree.stride(0) >= R) else tree.contiguous()


def _check_window(who, window, causal):
    if isinstance(window, bool) or not isinstance(window, int) or not 1 <= window < 2 ** 32:
        raise ValueError(f"{who}: window must be an int from 1 to 2^32 - 1 (None: no window), not {window!r}")
    if not causal:
        raise ValueError(f"{who}: a sliding window needs causal=True (the window lies behind the row's causal frontier)")


def _check_softcap(who, softcap):
    if isinstance(softcap, bool) or not isinstance(softcap, (int, float)) or not math.isfinite(softcap) or not softcap > 0:
        raise ValueError(f"{who}: softcap must be a finite number > 0, the cap of cap * tanh(score / cap) in natural-log units (None: no "
                         f"cap), not {softcap!r}")


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


def _check_row_starts(who, row_starts, cache_lengths, max_rows):
    if not isinstance(row_starts, torch.Tensor) or not row_starts.is_cuda or row_starts.dim() != 1 or \
            row_starts.shape[0] != cache_lengths.shape[0] + 1 or row_starts.dtype not in (torch.int32, torch.int64):
        got = f"{tuple(row_starts.shape)}, {row_starts.dtype}" if isinstance(row_starts, torch.Tensor) else type(row_starts).__name__
        raise ValueError(f"{who}: row_starts must be a GPU tensor [B + 1] = [{cache_lengths.shape[0] + 1}] int32 or int64: the first packed row "
                         f"of every sequence and the end of the last (got {got})")
    if isinstance(max_rows, bool) or not isinstance(max_rows, int) or not 1 <= max_rows < 2 ** 32:
        raise ValueError(f"{who}: max_rows must be an int from 1 to 2^32 - 1, the largest row count of a sequence (the host never reads "
                         f"row_starts), not {max_rows!r}")


# ---- the torch.library ops: what torch.compile traces.  Schemas are inferred from the annotated signatures
def _op_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
               block_table: Optional[torch.Tensor], causal: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    return _run_decode(q, k_cache, v_cache, cache_lengths, block_table, causal)


def _op_decode_fp8(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                   block_table: Optional[torch.Tensor], causal: bool, k_scale: Optional[torch.Tensor],
                   v_scale: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    return _run_decode(q, k_cache, v_cache, cache_lengths, block_table, causal, True, k_scale, v_scale)


def _op_decode_window(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                      block_table: Optional[torch.Tensor], causal: bool, k_scale: Optional[torch.Tensor],
                      v_scale: Optional[torch.Tensor], window: int) -> Tuple[torch.Tensor, torch.Tensor]:
    return _run_decode(q, k_cache, v_cache, cache_lengths, block_table, causal, None, k_scale, v_scale, window)


def _op_decode_sink(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                    block_table: Optional[torch.Tensor], causal: bool, k_scale: Optional[torch.Tensor], v_scale: Optional[torch.Tensor],
                    window: int, sink_tokens: int, sink_logits: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    return _run_decode(q, k_cache, v_cache, cache_lengths, block_table, causal, None, k_scale, v_scale, window or None, (sink_tokens, sink_logits))


def _op_decode_softcap(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                       block_table: Optional[torch.Tensor], causal: bool, k_scale: Optional[torch.Tensor], v_scale: Optional[torch.Tensor],
                       window: int, sink_tokens: int, sink_logits: Optional[torch.Tensor], softcap: float) -> Tuple[torch.Tensor, torch.Tensor]:
    return _run_decode(q, k_cache, v_cache, cache_lengths, block_table, causal, None, k_scale, v_scale, window or None,
                       _sinks_or_none(sink_tokens, sink_logits), softcap)


def _op_decode_tree(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                    block_table: Optional[torch.Tensor], causal: bool, k_scale: Optional[torch.Tensor], v_scale: Optional[torch.Tensor],
                    window: int, sink_tokens: int, sink_logits: Optional[torch.Tensor], tree_mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return _run_decode(q, k_cache, v_cache, cache_lengths, block_table, causal, None, k_scale, v_scale, window or None,
                       _sinks_or_none(sink_tokens, sink_logits), None, tree_mask)


def _op_prefill(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                q_lengths: Optional[torch.Tensor], block_table: Optional[torch.Tensor], causal: bool,
                k_scale: Optional[torch.Tensor], v_scale: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    return _run_prefill(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale)


def _op_prefill_window(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                       q_lengths: Optional[torch.Tensor], block_table: Optional[torch.Tensor], causal: bool,
                       k_scale: Optional[torch.Tensor], v_scale: Optional[torch.Tensor], window: int) -> Tuple[torch.Tensor, torch.Tensor]:
    return _run_prefill(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale, window)


def _op_prefill_sink(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                     q_lengths: Optional[torch.Tensor], block_table: Optional[torch.Tensor], causal: bool,
                     k_scale: Optional[torch.Tensor], v_scale: Optional[torch.Tensor], window: int, sink_tokens: int,
                     sink_logits: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    return _run_prefill(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale, window or None,
                        (sink_tokens, sink_logits))


def _op_prefill_ragged(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor, row_starts: torch.Tensor,
                       max_rows: int, block_table: Optional[torch.Tensor], causal: bool, k_scale: Optional[torch.Tensor],
                       v_scale: Optional[torch.Tensor], window: int, sink_tokens: int,
                       sink_logits: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    return _run_prefill_ragged(q, k_cache, v_cache, cache_lengths, row_starts, max_rows, block_table, causal, k_scale, v_scale, window,
                               (sink_tokens, sink_logits))


def _op_prefill_softcap(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                        q_lengths: Optional[torch.Tensor], block_table: Optional[torch.Tensor], causal: bool,
                        k_scale: Optional[torch.Tensor], v_scale: Optional[torch.Tensor], window: int, sink_tokens: int,
                        sink_logits: Optional[torch.Tensor], softcap: float) -> Tuple[torch.Tensor, torch.Tensor]:
    return _run_prefill(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale, window or None,
                        _sinks_or_none(sink_tokens, sink_logits), softcap)


def _op_prefill_tree(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                     q_lengths: Optional[torch.Tensor], block_table: Optional[torch.Tensor], causal: bool,
                     k_scale: Optional[torch.Tensor], v_scale: Optional[torch.Tensor], window: int, sink_tokens: int,
                     sink_logits: Optional[torch.Tensor], tree_mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return _run_prefill(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale, window or None,
                        _sinks_or_none(sink_tokens, sink_logits), None, tree_mask)


def _op_prefill_split(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                      q_lengths: Optional[torch.Tensor], block_table: Optional[torch.Tensor], causal: bool,
                      k_scale: Optional[torch.Tensor], v_scale: Optional[torch.Tensor], window: int, sink_tokens: int,
                      sink_logits: Optional[torch.Tensor], tree: Optional[torch.Tensor], key_pieces: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(`tree`: flash_prefill's tree_mask, None for none -- the ops of include/mfa_tree.h alone spell it tree_mask)"""
    return _run_prefill(q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale, window or None,
                        _sinks_or_none(sink_tokens, sink_logits), None, tree, key_pieces)


def _op_prefill_ragged_softcap(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                               row_starts: torch.Tensor, max_rows: int, block_table: Optional[torch.Tensor], causal: bool,
                               k_scale: Optional[torch.Tensor], v_scale: Optional[torch.Tensor], window: int, sink_tokens: int,
                               sink_logits: Optional[torch.Tensor], softcap: float) -> Tuple[torch.Tensor, torch.Tensor]:
    return _run_prefill_ragged(q, k_cache, v_cache, cache_lengths, row_starts, max_rows, block_table, causal, k_scale, v_scale, window,
                               (sink_tokens, sink_logits), softcap)


def _op_append(k_new: torch.Tensor, v_new: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
               block_table: Optional[torch.Tensor], k_scale: Optional[torch.Tensor], v_scale: Optional[torch.Tensor]) -> None:
    _run_append(k_new, v_new, k_cache, v_cache, cache_lengths, block_table, k_scale, v_scale)


def _op_append_ragged(k_new: torch.Tensor, v_new: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                      row_starts: torch.Tensor, max_rows: int, block_table: Optional[torch.Tensor], k_scale: Optional[torch.Tensor],
                      v_scale: Optional[torch.Tensor]) -> None:
    _run_append_ragged(k_new, v_new, k_cache, v_cache, cache_lengths, row_starts, max_rows, block_table, k_scale, v_scale)


def _op_compact(k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor, accepted: torch.Tensor, accepted_counts: torch.Tensor,
                rows: int, q_lengths: Optional[torch.Tensor], block_table: Optional[torch.Tensor]) -> torch.Tensor:
    return _run_compact(k_cache, v_cache, cache_lengths, accepted, accepted_counts, rows, q_lengths, block_table)


def _op_mla_decode(q: torch.Tensor, kv_cache: torch.Tensor, cache_lengths: torch.Tensor, block_table: Optional[torch.Tensor], causal: bool,
                   softmax_scale: float, pieces: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(`pieces`: 0 is the host's plan, 1 unsplit, 2 .. 64 as given)"""
    return _run_mla_decode(q, kv_cache, cache_lengths, block_table, causal, softmax_scale, pieces)


def _op_mla_decode_fp8(q: torch.Tensor, kv_cache: torch.Tensor, cache_lengths: torch.Tensor, block_table: Optional[torch.Tensor], causal: bool,
                       softmax_scale: float, pieces: int, kv_scale: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """(`pieces` as attention_mla_decode's; `kv_scale` last)"""
    return _run_mla_decode(q, kv_cache, cache_lengths, block_table, causal, softmax_scale, pieces, True, kv_scale)


def _op_mla_sparse_decode(q: torch.Tensor, kv_cache: torch.Tensor, cache_lengths: torch.Tensor, indices: torch.Tensor,
                          block_table: Optional[torch.Tensor], causal: bool, softmax_scale: float, pieces: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(`pieces` as attention_mla_decode's, over the slots of a list; `indices` after the lengths)"""
    return _run_mla_decode(q, kv_cache, cache_lengths, block_table, causal, softmax_scale, pieces, indices=indices)


def _op_mla_sparse_decode_fp8(q: torch.Tensor, kv_cache: torch.Tensor, cache_lengths: torch.Tensor, indices: torch.Tensor,
                              block_table: Optional[torch.Tensor], causal: bool, softmax_scale: float, pieces: int,
                              kv_scale: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """(attention_mla_sparse_decode's arguments; `kv_scale` last, as attention_mla_decode_fp8's)"""
    return _run_mla_decode(q, kv_cache, cache_lengths, block_table, causal, softmax_scale, pieces, True, kv_scale, indices=indices)


def _op_mla_prefill(q: torch.Tensor, kv_cache: torch.Tensor, cache_lengths: torch.Tensor, q_lengths: Optional[torch.Tensor],
                    block_table: Optional[torch.Tensor], causal: bool, softmax_scale: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(`q_lengths` after the cache's lengths, as attention_prefill's; no pieces: the launch is not cut along the keys)"""
    return _run_mla_prefill(q, kv_cache, cache_lengths, q_lengths, block_table, causal, softmax_scale)


def _op_mla_append(latent_new: torch.Tensor, rope_new: torch.Tensor, kv_cache: torch.Tensor, cache_lengths: torch.Tensor,
                   block_table: Optional[torch.Tensor], kv_scale: Optional[torch.Tensor]) -> None:
    _run_mla_append(latent_new, rope_new, kv_cache, cache_lengths, block_table, kv_scale)


def _fake_mla(q, *args, **kwargs):
    B, H, R, _Dk = q.shape
    return q.new_empty((B, H, R, AttentionMLADecode.VALUE_DIMENSION)), q.new_empty((B, H, R), dtype=torch.float32)


def _fake_lengths(k_cache, v_cache, cache_lengths, *args, **kwargs):
    return cache_lengths.new_empty((cache_lengths.shape[0],), dtype=torch.int32)


def _fake_padded(q, *args, **kwargs):
    B, H, R, D = q.shape
    return q.new_empty((B, H, R, D)), q.new_empty((B, H, R), dtype=torch.float32)


def _fake_packed(q, *args, **kwargs):
    T, H, D = q.shape
    return q.new_empty((T, H, D)), q.new_empty((H, T), dtype=torch.float32)


def _fake_none(*args, **kwargs):
    return None


_IMPLS = {}


def _register_cache_op(name, impl, fake, mutates_args=()):
    """defines the op mfa::<name> -- `impl` on the GPU, `fake` for tracing -- unless this torch has no custom ops (False) or an earlier import
    defined it; either way `_call_op` finds `impl` under the name"""
    _IMPLS[name] = impl
    if not hasattr(torch.library, "custom_op"):
        return False
    try:
        getattr(torch.ops.mfa, name)   # AttributeError when the op is not defined yet
    except (AttributeError, RuntimeError):
        torch.library.custom_op("mfa::" + name, mutates_args=mutates_args, device_types="cuda")(impl).register_fake(fake)
    return True


def _call_op(have, name, *args):
    """the op where torch has custom ops, else its implementation"""
    return getattr(torch.ops.mfa, name)(*args) if have else _IMPLS[name](*args)


# the ops: (name, implementation, fake, mutated arguments).  16-bit and e4m3 caches share one window op, one sink op and one soft-cap op
# per launch kind (`window` 0 and `sink_tokens` 0: none; `softcap` > 0 last), and one tree op (`tree_mask` last); the ops before them keep
# their schemas
_CACHE_OPS = [
    ("attention_decode", _op_decode, _fake_padded, ()),
    ("attention_decode_fp8", _op_decode_fp8, _fake_padded, ()),
    ("kv_cache_append", _op_append, _fake_none, ("k_cache", "v_cache")),
    ("attention_prefill", _op_prefill, _fake_padded, ()),
    ("attention_decode_window", _op_decode_window, _fake_padded, ()),
    ("attention_prefill_window", _op_prefill_window, _fake_padded, ()),
    ("attention_decode_sink", _op_decode_sink, _fake_padded, ()),
    ("attention_prefill_sink", _op_prefill_sink, _fake_padded, ()),
    ("attention_prefill_ragged", _op_prefill_ragged, _fake_packed, ()),
    ("kv_cache_append_ragged", _op_append_ragged, _fake_none, ("k_cache", "v_cache")),
    ("attention_decode_softcap", _op_decode_softcap, _fake_padded, ()),
    ("attention_prefill_softcap", _op_prefill_softcap, _fake_padded, ()),
    ("attention_prefill_ragged_softcap", _op_prefill_ragged_softcap, _fake_packed, ()),
    ("attention_decode_tree", _op_decode_tree, _fake_padded, ()),
    ("attention_prefill_tree", _op_prefill_tree, _fake_padded, ()),
    ("kv_cache_compact", _op_compact, _fake_lengths, ("k_cache", "v_cache")),
    ("attention_prefill_split", _op_prefill_split, _fake_padded, ()),
    ("attention_mla_decode", _op_mla_decode, _fake_mla, ()),
]
_HAVE = {_op[0]: _register_cache_op(*_op) for _op in _CACHE_OPS}   # op name -> whether torch has it as a custom op
_HAVE_DECODE_OP = _HAVE["attention_decode"]
_HAVE_KVCACHE_OPS = _HAVE["attention_decode_fp8"] and _HAVE["kv_cache_append"]
_HAVE_PREFILL_OP = _HAVE["attention_prefill"]
_HAVE_WINDOW_OPS = _HAVE["attention_decode_window"] and _HAVE["attention_prefill_window"]
_HAVE_SINK_OPS = _HAVE["attention_decode_sink"] and _HAVE["attention_prefill_sink"]
_HAVE_RAGGED_OPS = _HAVE["attention_prefill_ragged"] and _HAVE["kv_cache_append_ragged"]
_HAVE_SOFTCAP_OPS = _HAVE["attention_decode_softcap"] and _HAVE["attention_prefill_softcap"] and _HAVE["attention_prefill_ragged_softcap"]
_HAVE_TREE_OPS = _HAVE["attention_decode_tree"] and _HAVE["attention_prefill_tree"]
_HAVE_COMPACT_OP = _HAVE["kv_cache_compact"]
_HAVE_SPLIT_OP = _HAVE["attention_prefill_split"]
_HAVE_MLA_OP = _HAVE["attention_mla_decode"]
# the ops of include/mfa_mla_cache.h, a list of their own: the append of the latent cache and MLA decode over an e4m3 latent cache
_MLA_CACHE_OPS = [
    ("mla_cache_append", _op_mla_append, _fake_none, ("kv_cache",)),
    ("attention_mla_decode_fp8", _op_mla_decode_fp8, _fake_mla, ()),
]
_HAVE.update({_op[0]: _register_cache_op(*_op) for _op in _MLA_CACHE_OPS})
_HAVE_MLA_CACHE_OPS = _HAVE["mla_cache_append"] and _HAVE["attention_mla_decode_fp8"]
# the op of include/mfa_mla_sparse.h, in a list of its own
_MLA_SPARSE_OPS = [
    ("attention_mla_sparse_decode", _op_mla_sparse_decode, _fake_mla, ()),
]
_HAVE.update({_op[0]: _register_cache_op(*_op) for _op in _MLA_SPARSE_OPS})
_HAVE_MLA_SPARSE_OP = _HAVE["attention_mla_sparse_decode"]
# the op of include/mfa_mla_sparse_fp8.h, in a list of its own
_MLA_SPARSE_FP8_OPS = [
    ("attention_mla_sparse_decode_fp8", _op_mla_sparse_decode_fp8, _fake_mla, ()),
]
_HAVE.update({_op[0]: _register_cache_op(*_op) for _op in _MLA_SPARSE_FP8_OPS})
_HAVE_MLA_SPARSE_FP8_OP = _HAVE["attention_mla_sparse_decode_fp8"]

# the op of include/mfa_mla_prefill.h, in a list of its own
_MLA_PREFILL_OPS = [
    ("attention_mla_prefill", _op_mla_prefill, _fake_mla, ()),
]
_HAVE.update({_op[0]: _register_cache_op(*_op) for _op in _MLA_PREFILL_OPS})
_HAVE_MLA_PREFILL_OP = _HAVE["attention_mla_prefill"]


def _forward_only(who, q, k_cache, v_cache, cache_lengths):
    if not (q.is_cuda and k_cache.is_cuda and v_cache.is_cuda and cache_lengths.is_cuda):
        raise RuntimeError(f"{who}: tensors must live on the GPU (there is no CPU path)")
    for t in (q, k_cache, v_cache):
        if t.requires_grad:
            raise RuntimeError(f"{who} is forward only (no autograd): detach the inputs; flash_attention is the differentiable entry")


def _in_place(who, k_new, v_new, k_cache, v_cache, cache_lengths):
    for t in (k_new, v_new, k_cache, v_cache):
        if t.requires_grad:
            raise RuntimeError(f"{who} writes in place and has no autograd: detach the inputs")
    if not all(t.is_cuda for t in (k_new, v_new, k_cache, v_cache, cache_lengths)):
        raise RuntimeError(f"{who}: tensors must live on the GPU (there is no CPU path)")


class _Public:
    """what _route knows of a public function: its name in messages, the op of each rung (none: the function has no such rung and its
    plain op takes the rung's arguments), whether the scales go in front of a rung's arguments (prefill's ops all take them earlier)"""

    def __init__(self, who, plain, fp8=None, window=None, sink=None, softcap=None, scales=False, packed=False, tree=None, split=None):
        self.who, self.plain, self.fp8, self.window, self.sink, self.softcap, self.scales, self.packed = who, plain, fp8, window, sink, softcap, scales, packed
        self.tree, self.split = tree, split


_DECODE = _Public("flash_decode", "attention_decode", "attention_decode_fp8", "attention_decode_window", "attention_decode_sink",
                  "attention_decode_softcap", scales=True, tree="attention_decode_tree")
_PREFILL = _Public("flash_prefill", "attention_prefill", None, "attention_prefill_window", "attention_prefill_sink", "attention_prefill_softcap",
                   tree="attention_prefill_tree", split="attention_prefill_split")
_PREFILL_RAGGED = _Public("flash_prefill_ragged", "attention_prefill_ragged", softcap="attention_prefill_ragged_softcap", packed=True)


def _route(f, q, k_cache, v_cache, causal, k_scale, v_scale, window, sink_tokens, sink_logits, softcap, tree_mask=None, key_pieces=None):
    """The keywords of the public function `f` (a _Public), checked in one order -- the key pieces, the cap, then the window, the sink tokens
    and the sink logits, then the tree, which reaches the tree op with any window and sinks -- and the op they reach -> (op, the arguments
    it takes after causal, or after the scales where they come earlier), in the ops' spelling: 0 for no window and no sink tokens, None for
    no tree.  Key pieces reach the split op with any window, sinks and tree and no cap; a cap wins over all else, either sink keyword
    reaches the sink op, a window the window op"""
    who = f.who
    if key_pieces is not None:
        if softcap is not None:
            raise ValueError(f"{who}: key_pieces and softcap together have no kernel (include/mfa_split.h)")
        if isinstance(key_pieces, bool) or not isinstance(key_pieces, int) or not 0 <= key_pieces <= 64:
            raise ValueError(f"{who}: key_pieces must be an int from 0 (the host's plan) to 64 (None: the launch is not cut along the keys), not {key_pieces!r}")
    if softcap is not None:
        _check_softcap(who, softcap)
    sinks = sink_tokens is not None or sink_logits is not None
    if window is not None or sinks:
        # (_check_sinks reads the heads off a [B, H, R, D] query: the packed q of a ragged batch as such a view)
        _check_sinks(who, q.unsqueeze(0).transpose(1, 2) if f.packed and q.dim() == 3 else q, window, causal, sink_tokens, sink_logits)
    scales = (k_scale, v_scale) if f.scales else ()
    if tree_mask is not None:
        _check_tree(who, q, tree_mask, causal, window, softcap)
    if key_pieces is not None:
        return f.split, (*scales, window or 0, sink_tokens or 0, sink_logits, tree_mask, key_pieces)
    if tree_mask is not None:
        return f.tree, (*scales, window or 0, sink_tokens or 0, sink_logits, tree_mask)
    if softcap is not None:
        return f.softcap, (*scales, window or 0, sink_tokens or 0, sink_logits, float(softcap))
    if f.sink is None or sinks:   # (a function without a sink op: its plain op takes the window and the sinks)
        return f.sink or f.plain, (*scales, window or 0, sink_tokens or 0, sink_logits)
    if window is not None:
        return f.window, (*scales, window)
    if f.fp8 is not None:
        if k_cache.dtype in _FP8_DTYPES or v_cache.dtype in _FP8_DTYPES:
            return f.fp8, scales
        _check_scales(who, False, k_scale, v_scale)   # (the op of a 16-bit cache takes no scales)
    return f.plain, ()


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
    _in_place("kv_cache_append", k_new, v_new, k_cache, v_cache, cache_lengths)
    _call_op(_HAVE_KVCACHE_OPS, "kv_cache_append", k_new, v_new, k_cache, v_cache, cache_lengths, block_table, k_scale, v_scale)


def flash_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                 block_table: Optional[torch.Tensor] = None, causal: bool = True, return_lse: bool = False,
                 k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None, window: Optional[int] = None,
                 sink_tokens: Optional[int] = None, sink_logits: Optional[torch.Tensor] = None, softcap: Optional[float] = None,
                 tree_mask: Optional[torch.Tensor] = None):
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
    k_scale; L includes it (include/mfa_sink.h).  Either goes through the op `mfa::attention_decode_sink`.
    softcap=cap (a finite number > 0, natural-log units: a checkpoint's attn_logit_softcapping, 50 in Gemma 2): the softmax sees
    cap tanh(score / cap), the score with 1 / sqrt(D) and k_scale applied; masked keys stay masked, the sink logit is not capped, L is
    that of the capped scores (include/mfa_softcap.h).  With any window and sinks, through the op `mfa::attention_decode_softcap`.
    None: no cap.
    tree_mask=int64 [R] (one tree for every sequence) or [B, R] on the GPU, the bit patterns of uint64 row masks (pack_tree_mask): the R new
    rows are the nodes of a speculation TREE, node j at key len - R + j -- row r sees new token j iff bit j of its mask is set, whatever r
    and j, and sees the cached prefix through the window at its depth, popcount(mask) - 1, not at its index (include/mfa_tree.h).  Needs
    causal and, with a window, window >= R; not with softcap.  The chain mask 2^(r + 1) - 1 is the launch without a tree, bit for bit.
    Through the op `mfa::attention_decode_tree`, with any window and sinks.  None: the causal rule."""
    _forward_only("flash_decode", q, k_cache, v_cache, cache_lengths)
    op, own = _route(_DECODE, q, k_cache, v_cache, causal, k_scale, v_scale, window, sink_tokens, sink_logits, softcap, tree_mask)
    o, l = _call_op(_HAVE[op], op, q, k_cache, v_cache, cache_lengths, block_table, causal, *own)
    return (o, l * _LN2) if return_lse else o


def flash_prefill(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                  q_lengths: Optional[torch.Tensor] = None, block_table: Optional[torch.Tensor] = None, causal: bool = True,
                  k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None, return_lse: bool = False,
                  window: Optional[int] = None, sink_tokens: Optional[int] = None, sink_logits: Optional[torch.Tensor] = None,
                  softcap: Optional[float] = None, tree_mask: Optional[torch.Tensor] = None, key_pieces: Optional[int] = None):
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
    L = the head's sink logit.  softcap=cap: logit soft-capping as flash_decode's (include/mfa_softcap.h), with any window and sinks,
    through the op `mfa::attention_prefill_softcap`; None: no cap.  tree_mask=int64 [R] or [B, R]: a speculation tree among the new rows as
    flash_decode's (include/mfa_tree.h; R <= 64, trees of different sizes through q_lengths), through the op `mfa::attention_prefill_tree`;
    None: the causal rule.  key_pieces=P: the launch CUT ALONG THE KEYS (include/mfa_split.h) -- for few row blocks over a long cache (one
    sequence, a speculation tree, a short chunk), which unsplit are a handful of workgroups that each walk the whole cache: 0 lets the host
    plan the pieces from the shapes, 2 .. 64 forces them, 1 is the unsplit launch; the workspace is allocated here.  With any window, sinks
    and tree_mask, not with softcap; through the op `mfa::attention_prefill_split`.  None: the launch is not cut, as before."""
    _forward_only("flash_prefill", q, k_cache, v_cache, cache_lengths)
    op, own = _route(_PREFILL, q, k_cache, v_cache, causal, k_scale, v_scale, window, sink_tokens, sink_logits, softcap, tree_mask, key_pieces)
    o, l = _call_op(_HAVE[op], op, q, k_cache, v_cache, cache_lengths, q_lengths, block_table, causal, k_scale, v_scale, *own)
    return (o, l * _LN2) if return_lse else o


def flash_prefill_ragged(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor, row_starts: torch.Tensor,
                         max_rows: int, block_table: Optional[torch.Tensor] = None, causal: bool = True,
                         k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None, return_lse: bool = False,
                         window: Optional[int] = None, sink_tokens: Optional[int] = None, sink_logits: Optional[torch.Tensor] = None,
                         softcap: Optional[float] = None):
    """flash_prefill for a RAGGED batch (a continuous-batching step: sequences with one new token beside prompt chunks): q [T, H, D]
    holds the new rows of all B sequences packed along the first axis, row_starts [B + 1] (GPU, int32 / int64, non-decreasing: the
    engine's cu_seqlens_q / query_start_loc) says where each sequence's rows begin, and max_rows (a host int) is the largest row
    count of any sequence -- rows of a sequence past it are not served.  q may be any view with a contiguous last dimension, a slice
    of a fused QKV projection included: it is read where it lies.  Caches, cache_lengths [B], block_table, scales, causal, window,
    sink_tokens and sink_logits: flash_prefill's.  Returns O [T, H, D], and with return_lse also L [H, T] fp32 in natural units; packed
    rows that no sequence owns come back uninitialised.  The launch starts no workgroup for row blocks that do not exist and computes,
    byte for byte, what flash_prefill computes for the same sequences padded to max_rows.  Forward only; goes through the op
    `mfa::attention_prefill_ragged` where torch has custom ops, so it traces under torch.compile.  softcap=cap: logit soft-capping as
    flash_decode's, through the op `mfa::attention_prefill_ragged_softcap`; None: no cap."""
    _forward_only("flash_prefill_ragged", q, k_cache, v_cache, cache_lengths)
    op, own = _route(_PREFILL_RAGGED, q, k_cache, v_cache, causal, k_scale, v_scale, window, sink_tokens, sink_logits, softcap)
    o, l = _call_op(_HAVE[op], op, q, k_cache, v_cache, cache_lengths, row_starts, max_rows, block_table, causal, k_scale, v_scale, *own)
    return (o, l * _LN2) if return_lse else o


def kv_cache_append_ragged(k_new: torch.Tensor, v_new: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor,
                           row_starts: torch.Tensor, max_rows: int, block_table: Optional[torch.Tensor] = None,
                           k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None) -> None:
    """kv_cache_append for a RAGGED batch, in ONE launch: k_new, v_new [T, Hkv, D] hold the new rows of all B sequences packed along
    the first axis (any view with a contiguous last dimension: the K and V slices of a fused QKV projection are read where they lie),
    row_starts [B + 1] and max_rows as flash_prefill_ragged's.  Row r of sequence b, which has qn_b = row_starts[b + 1] - row_starts[b]
    rows, goes to key cache_lengths[b] - qn_b + r (cache_lengths ALREADY INCLUDES the new tokens); kv_cache_append's drop rules, caches,
    quantisation and scales.  Goes through the op `mfa::kv_cache_append_ragged` (mutates_args) where torch has custom ops."""
    _in_place("kv_cache_append_ragged", k_new, v_new, k_cache, v_cache, cache_lengths)
    _call_op(_HAVE_RAGGED_OPS, "kv_cache_append_ragged", k_new, v_new, k_cache, v_cache, cache_lengths, row_starts, max_rows, block_table, k_scale,
             v_scale)


def kv_cache_compact(k_cache: torch.Tensor, v_cache: torch.Tensor, cache_lengths: torch.Tensor, accepted: torch.Tensor,
                     accepted_counts: torch.Tensor, rows: int, q_lengths: Optional[torch.Tensor] = None,
                     block_table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """What follows a tree launch (tree_mask= on flash_decode / flash_prefill): moves the K and V rows of the ACCEPTED path of every
    sequence's speculation tree to the front of the tree's slots IN PLACE and returns the lengths the sequences then have, int32 [B] on
    the GPU -- the tensor the next kv_cache_append takes once the new tokens are counted in.  cache_lengths [B] (GPU) is the tensor the
    tree launch took: it INCLUDES the `rows` tree rows (q_lengths [B]: the rows of sequence b, as flash_prefill's), node j of sequence b
    at key P + j with P = cache_lengths[b] - rows.  accepted int32 [B, A] (A <= 64) holds each path's node indices in path order, root
    first, accepted_counts [B] how many of them count (tree_path gives both): the row at key P + i becomes the row that stood at key
    P + accepted[b, i] BEFORE the call, for every K/V head, in K and in V -- every source is read before any destination is written, so
    indices may decrease or repeat; an index < 0 or past the tree's live rows moves nothing.  Returns P + min(accepted_counts[b], A,
    live rows).  Caches: kv_cache_append's -- [B, Hkv, C, D] or a strided view with a contiguous last dimension, or with block_table
    [B, n] int32 page pools [pages, Hkv, pageSize, D]; bfloat16, float16 or torch.float8_e4m3fn (bytes are moved, scales do not enter).
    No other byte of the caches changes.  Goes through the op `mfa::kv_cache_compact` (mutates_args) where torch has custom ops."""
    for t in (k_cache, v_cache):
        if t.requires_grad:
            raise RuntimeError("kv_cache_compact writes in place and has no autograd: detach the inputs")
    if not all(t.is_cuda for t in (k_cache, v_cache, cache_lengths, accepted, accepted_counts)):
        raise RuntimeError("kv_cache_compact: tensors must live on the GPU (there is no CPU path)")
    return _call_op(_HAVE_COMPACT_OP, "kv_cache_compact", k_cache, v_cache, cache_lengths, accepted, accepted_counts, rows, q_lengths, block_table)


def flash_mla_decode(q: torch.Tensor, kv_cache: torch.Tensor, cache_lengths: torch.Tensor, *, softmax_scale: float,
                     block_table: Optional[torch.Tensor] = None, causal: bool = True, return_lse: bool = False, pieces: Optional[int] = None):
    """Multi-head latent attention decode in its absorbed form (DeepSeek-V2 / V3 / R1, Kimi K2; include/mfa_mla.h): the R new rows of every
    sequence and head, q [B, H, R, 576] (R <= 32), against a COMPRESSED cache kv_cache [B, C, 576] that holds one row per key -- a 512-wide
    latent followed by a 64-wide rotary part -- shared by every head: all 576 columns are the key, the first 512 the value.  Returns
    O [B, H, R, 512] (the caller applies the value up-projection), and with return_lse also L [B, H, R] fp32 in natural units.
    softmax_scale is the model's own scale on q . k (1 / sqrt(192) times a YaRN factor in those checkpoints) and is required.
    cache_lengths [B] (GPU): valid keys per sequence INCLUDING the R new tokens, which the caller has already written into the cache
    (mla_cache_append, with the same lengths); with `causal` row r sees key c iff c <= r + max(len - R, 0).  kv_cache may
    be any view of that shape with a contiguous last dimension and a row stride that is a multiple of 8 (nothing is copied); with
    block_table [B, n] int32 it is a page pool [pages, pageSize, 576].  pieces: None lets the host cut the keys into pieces from the
    shapes, 1 is the unsplit launch, 2 .. 64 forces them; the workspace is allocated here.  Forward only, GPU only.  A sequence of length
    0 gets O = 0.  Goes through the torch.library op `mfa::attention_mla_decode` where torch has custom ops, so it traces under
    torch.compile."""
    who = "flash_mla_decode"
    if not (q.is_cuda and kv_cache.is_cuda and cache_lengths.is_cuda):
        raise RuntimeError(f"{who}: tensors must live on the GPU (there is no CPU path)")
    for t in (q, kv_cache):
        if t.requires_grad:
            raise RuntimeError(f"{who} is forward only (no autograd): detach the inputs")
    pieces = 0 if pieces is None else pieces
    _check_mla(who, q, kv_cache, cache_lengths, block_table, softmax_scale, pieces)
    o, l = _call_op(_HAVE_MLA_OP, "attention_mla_decode", q, kv_cache, cache_lengths, block_table, bool(causal), float(softmax_scale), int(pieces))
    return (o, l * _LN2) if return_lse else o


def flash_mla_prefill(q: torch.Tensor, kv_cache: torch.Tensor, cache_lengths: torch.Tensor, *, softmax_scale: float,
                      q_lengths: Optional[torch.Tensor] = None, block_table: Optional[torch.Tensor] = None, causal: bool = True,
                      return_lse: bool = False):
    """Multi-head latent attention prefill in its absorbed form over the compressed cache of flash_mla_decode (include/mfa_mla_prefill.h): a
    block of R new rows per sequence and head, of ANY length, q [B, H, R, 576], against kv_cache [B, C, 576] (with block_table [B, n] int32:
    a page pool [pages, pageSize, 576]) -- chunked prefill, prefix reuse, the extend step after a cache hit, a long draft block.  Returns
    O [B, H, R, 512], and with return_lse also L [B, H, R] fp32 in natural units.  softmax_scale is the model's own scale and is required.
    cache_lengths [B] (GPU): valid keys per sequence INCLUDING the new tokens, which the caller has already written (mla_cache_append).
    q_lengths [B] (GPU; None: every sequence has R): the new rows of each sequence; with `causal` row r < q_lengths[b] sees key c iff
    c <= r + max(len - q_lengths[b], 0).  Rows at or past q_lengths[b] are neither read nor written: they come back uninitialised.  A row
    without a visible key gets O = 0.  q may be any view with a contiguous last dimension and strides that are multiples of 8 -- a
    transposed token-major [B, R, H, 576] is read where it lies.  Forward only, GPU only.  Goes through the torch.library op
    `mfa::attention_mla_prefill` where torch has custom ops, so it traces under torch.compile."""
    who = "flash_mla_prefill"
    if not (q.is_cuda and kv_cache.is_cuda and cache_lengths.is_cuda) or (q_lengths is not None and not q_lengths.is_cuda):
        raise RuntimeError(f"{who}: tensors must live on the GPU (there is no CPU path)")
    for t in (q, kv_cache):
        if t.requires_grad:
            raise RuntimeError(f"{who} is forward only (no autograd): detach the inputs")
    _check_mla(who, q, kv_cache, cache_lengths, block_table, softmax_scale, 0)
    if q_lengths is not None:
        _check_lengths(who, "q_lengths", q_lengths, int(q.shape[0]))
    o, l = _call_op(_HAVE_MLA_PREFILL_OP, "attention_mla_prefill", q, kv_cache, cache_lengths, q_lengths, block_table, bool(causal), float(softmax_scale))
    return (o, l * _LN2) if return_lse else o


def mla_cache_append(latent_new: torch.Tensor, rope_new: torch.Tensor, kv_cache: torch.Tensor, cache_lengths: torch.Tensor, *,
                     block_table: Optional[torch.Tensor] = None, kv_scale: Optional[torch.Tensor] = None) -> None:
    """Writes the R new rows of every sequence into the latent cache of flash_mla_decode IN PLACE and returns nothing
    (include/mfa_mla_cache.h): latent_new [B, R, 512] (the normalised latent) and rope_new [B, R, 64] (the rotated key part), bf16 or
    fp16, become one cache row of 576.  Either may be any view with a contiguous last dimension and 16-byte rows -- the two slices of a
    fused row of 576 are read where they lie.  cache_lengths [B] (GPU) ALREADY INCLUDES the new tokens -- the tensor the decode takes
    next: row r of sequence b goes to key cache_lengths[b] - R + r; rows that fall before key 0, past the cache's capacity or past the
    block table's row are not written, and no other byte of the cache is touched.  kv_cache: [B, C, 576] (or a strided view with a
    contiguous last dimension) or, with block_table [B, n] int32, a page pool [pages, pageSize, 576]; the rows' own 16-bit type (bits
    copied; kv_scale is an error) or torch.float8_e4m3fn (the rows are quantised: byte = e4m3(x / kv_scale[0]), round to nearest even,
    saturating at +-448; kv_scale fp32 [1] on the GPU, None = 1.0 -- one scale for the latent and the rotary part alike).  R has no limit:
    a prompt's rows go in one launch.  Goes through the op `mfa::mla_cache_append` (mutates_args) where torch has custom ops."""
    who = "mla_cache_append"
    if not all(t.is_cuda for t in (latent_new, rope_new, kv_cache, cache_lengths)):
        raise RuntimeError(f"{who}: tensors must live on the GPU (there is no CPU path)")
    for t in (latent_new, rope_new, kv_cache):
        if t.requires_grad:
            raise RuntimeError(f"{who} writes in place and has no autograd: detach the inputs")
    _check_mla_append(who, latent_new, rope_new, kv_cache, cache_lengths, block_table, kv_scale)
    _call_op(_HAVE_MLA_CACHE_OPS, "mla_cache_append", latent_new, rope_new, kv_cache, cache_lengths, block_table, kv_scale)


def flash_mla_decode_fp8(q: torch.Tensor, kv_cache: torch.Tensor, cache_lengths: torch.Tensor, *, softmax_scale: float,
                         kv_scale: Optional[torch.Tensor] = None, block_table: Optional[torch.Tensor] = None, causal: bool = True,
                         return_lse: bool = False, pieces: Optional[int] = None):
    """flash_mla_decode over an FP8 latent cache (include/mfa_mla_cache.h): kv_cache [B, C, 576] torch.float8_e4m3fn (or, with
    block_table, a page pool [pages, pageSize, 576]), as mla_cache_append writes it -- one row of 576 bytes per key, half the traffic and
    half the memory of a 16-bit cache.  kv_scale fp32 [1] on the GPU (None = 1.0): a cache byte stands for kv_scale[0] x e4m3(byte),
    latent and rotary part alike; it folds into the softmax scale and the final normalisation.  q [B, H, R, 576] bf16 or fp16 (R <= 32);
    everything else -- softmax_scale (required), cache_lengths, causal, return_lse, pieces, O [B, H, R, 512] in q's type -- is
    flash_mla_decode's.  kv_cache may be any view with a contiguous last dimension and strides that are multiples of 16 (nothing is
    copied).  Forward only, GPU only.  Goes through the torch.library op `mfa::attention_mla_decode_fp8` where torch has custom ops, so it
    traces under torch.compile."""
    who = "flash_mla_decode_fp8"
    if not (q.is_cuda and kv_cache.is_cuda and cache_lengths.is_cuda):
        raise RuntimeError(f"{who}: tensors must live on the GPU (there is no CPU path)")
    for t in (q, kv_cache):
        if t.requires_grad:
            raise RuntimeError(f"{who} is forward only (no autograd): detach the inputs")
    pieces = 0 if pieces is None else pieces
    _check_mla(who, q, kv_cache, cache_lengths, block_table, softmax_scale, pieces, True)
    _latent_scale(who, kv_scale, kv_cache.device)
    o, l = _call_op(_HAVE_MLA_CACHE_OPS, "attention_mla_decode_fp8", q, kv_cache, cache_lengths, block_table, bool(causal), float(softmax_scale),
                    int(pieces), kv_scale)
    return (o, l * _LN2) if return_lse else o


def flash_mla_sparse_decode(q: torch.Tensor, kv_cache: torch.Tensor, cache_lengths: torch.Tensor, indices: torch.Tensor, *, softmax_scale: float,
                            block_table: Optional[torch.Tensor] = None, causal: bool = True, return_lse: bool = False,
                            pieces: Optional[int] = None):
    """flash_mla_decode over per-row lists of selected keys (DeepSeek-V3.2's sparse attention; include/mfa_mla_sparse.h): q [B, H, R, 576]
    and indices [B, R, topk] int32 on the GPU, the key POSITIONS row r of sequence b attends to, shared by all H heads.  A position is
    logical -- with block_table it is translated through the table as flash_mla_decode does.  -1, a position at or past
    cache_lengths[b] and, with `causal`, a position past r + max(len - R, 0) are holes: their cache rows are never loaded.  A position
    that appears twice counts twice; the order of a list is free.  A row without a visible entry gets O = 0.  indices may be any view
    with a contiguous last dimension (nothing is copied).  kv_cache (bf16 or fp16, q's type), cache_lengths, softmax_scale (required),
    return_lse and O [B, H, R, 512] are flash_mla_decode's; pieces cuts the SLOTS of a list (None: the host's plan from topk).  Forward
    only, GPU only.  Goes through the torch.library op `mfa::attention_mla_sparse_decode` where torch has custom ops, so it traces under
    torch.compile."""
    who = "flash_mla_sparse_decode"
    if not (q.is_cuda and kv_cache.is_cuda and cache_lengths.is_cuda and indices.is_cuda):
        raise RuntimeError(f"{who}: tensors must live on the GPU (there is no CPU path)")
    for t in (q, kv_cache):
        if t.requires_grad:
            raise RuntimeError(f"{who} is forward only (no autograd): detach the inputs")
    pieces = 0 if pieces is None else pieces
    _check_mla(who, q, kv_cache, cache_lengths, block_table, softmax_scale, pieces)
    _check_mla_indices(who, q, indices)
    o, l = _call_op(_HAVE_MLA_SPARSE_OP, "attention_mla_sparse_decode", q, kv_cache, cache_lengths, indices, block_table, bool(causal),
                    float(softmax_scale), int(pieces))
    return (o, l * _LN2) if return_lse else o


def flash_mla_sparse_decode_fp8(q: torch.Tensor, kv_cache: torch.Tensor, cache_lengths: torch.Tensor, indices: torch.Tensor, *,
                                softmax_scale: float, kv_scale: Optional[torch.Tensor] = None, block_table: Optional[torch.Tensor] = None,
                                causal: bool = True, return_lse: bool = False, pieces: Optional[int] = None):
    """flash_mla_sparse_decode over an FP8 latent cache (DeepSeek-V3.2 as it is served; include/mfa_mla_sparse_fp8.h): kv_cache
    [B, C, 576] torch.float8_e4m3fn (or, with block_table, a page pool [pages, pageSize, 576]) as mla_cache_append writes it, kv_scale
    fp32 [1] on the GPU (None = 1.0) as flash_mla_decode_fp8 takes it, and indices [B, R, topk] int32 on the GPU as
    flash_mla_sparse_decode takes them: logical key positions, shared by all heads; -1, a position at or past cache_lengths[b] and, with
    `causal`, a position past r + max(len - R, 0) are holes, whose 576 bytes are never loaded -- nor is any key that no list names, so
    such rows may hold the NaN bytes 0x7f / 0xff.  No temporary is gathered: the kernel reads the listed rows where they lie.
    q [B, H, R, 576] bf16 or fp16 (R <= 32), softmax_scale (required), cache_lengths, return_lse and O [B, H, R, 512] in q's type are
    flash_mla_decode's; pieces cuts the SLOTS of a list.  Forward only, GPU only.  Goes through the torch.library op
    `mfa::attention_mla_sparse_decode_fp8` where torch has custom ops, so it traces under torch.compile."""
    who = "flash_mla_sparse_decode_fp8"
    if not (q.is_cuda and kv_cache.is_cuda and cache_lengths.is_cuda and indices.is_cuda):
        raise RuntimeError(f"{who}: tensors must live on the GPU (there is no CPU path)")
    for t in (q, kv_cache):
        if t.requires_grad:
            raise RuntimeError(f"{who} is forward only (no autograd): detach the inputs")
    pieces = 0 if pieces is None else pieces
    _check_mla(who, q, kv_cache, cache_lengths, block_table, softmax_scale, pieces, True)
    _check_mla_indices(who, q, indices)
    _latent_scale(who, kv_scale, kv_cache.device)
    o, l = _call_op(_HAVE_MLA_SPARSE_FP8_OP, "attention_mla_sparse_decode_fp8", q, kv_cache, cache_lengths, indices, block_table, bool(causal),
                    float(softmax_scale), int(pieces), kv_scale)
    return (o, l * _LN2) if return_lse else o
