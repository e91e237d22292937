"""CPU test (no GPU call): the host side of the FP8 KV cache, include/mfa_kvcache.h -- exported symbols, struct layouts, the e4m3 codec
against torch's float8_e4m3fn on the CPU (every bf16 and f16 bit pattern under four scales), every refusal with its message, and the
plan of the FP8 decode launch, which is the 16-bit launch's (same grid, pieces and workspace bytes; kernels named attn_decode8_...)."""
import ctypes
import os
import re

import numpy as np
import pytest

from metal_flash_attention_amd import (AttentionDecode, AttentionDecodeFP8, GEMMOperandPrecision as P, KVCacheAppend, KVCachePrecision,
                                       MFAError, _abi)

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = 0x1000   # any non-null value: the host never reads the lengths
UNSUPPORTED, INVALID = 3, 2


def shape(**over):
    kw = dict(rows=1, column=4096, heads=64, batches=4, headsPerKeyValue=8, cacheLengths=LENGTHS)
    kw.update(over)
    return kw


def fp8_strides(D, column=4096, kv=8):
    return dict(K=(D, column * D, kv * column * D), V=(D, column * D, kv * column * D))


def test_header_symbols_exported_and_struct_layouts():
    header = open(os.path.join(ROOT, "include", "mfa_kvcache.h")).read()
    declared = set(re.findall(r"\b(mfa_(?:kv|attention_decode_fp8)_\w+)\s*\(", header))
    handle = _abi.lib()
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in include/mfa_kvcache.h but not exported"
    assert declared == {s[0] for s in _abi.KVCACHE_SYMBOLS}
    assert len(declared) == 9
    # the blocks of mfa.h and mfa_decode.h did not change
    assert int(handle.mfa_abi_version()) == 6
    assert ctypes.sizeof(_abi.mfa_decode_params) == 200
    # 4 x u32, u16 + 2 x u8, u32, 2 pointers, i64, 12 + 2 x i64, 2 pointers
    A = _abi.mfa_kv_append_params
    assert ctypes.sizeof(A) == 176
    assert (A.headDimension.offset, A.precision.offset, A.cachePrecision.offset, A.pageSize.offset) == (16, 18, 19, 20)
    assert (A.cacheLengths.offset, A.blockTable.offset, A.blockTableStride.offset, A.leadingDimension.offset) == (24, 32, 40, 48)
    assert (A.pageStride.offset, A.keyScale.offset, A.valueScale.offset) == (144, 160, 168)
    Q = _abi.mfa_kv_quant
    assert ctypes.sizeof(Q) == 24 and (Q.cachePrecision.offset, Q.keyScale.offset, Q.valueScale.offset) == (0, 8, 16)
    for macro, value in (("MFA_KV_E4M3", _abi.MFA_KV_E4M3), ("MFA_KV_E5M2", _abi.MFA_KV_E5M2)):
        assert re.search(r"#define %s\s+%d\b" % (macro, value), header), macro
    p = A()
    handle.mfa_kv_append_params_init(ctypes.byref(p))
    assert (p.precision, p.cachePrecision, p.pageSize, p.keyScale) == (int(P.BF16), int(P.BF16), 0, None)
    q = Q(7, 7, 7, 7)
    handle.mfa_kv_quant_init(ctypes.byref(q))
    assert (q.cachePrecision, q.reserved, q.keyScale, q.valueScale) == (_abi.MFA_KV_E4M3, 0, None, None)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("scale", [1.0, 0.5, 0.013, 3.7])
def test_quantize_equals_torch_for_every_16_bit_pattern(dtype, scale):
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype).float()
    x = x[~torch.isnan(x)]
    s32 = float(np.float32(scale))
    want = (x / s32).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    quantize = _abi.lib().mfa_kv_quantize_e4m3
    got = np.fromiter((quantize(float(v), s32) for v in x.numpy()), dtype=np.uint8, count=x.numel())
    wrong = np.nonzero(got != want)[0]
    assert wrong.size == 0, [(float(x[i]), int(got[i]), int(want[i])) for i in wrong[:8]]
    assert (got & 0x7F).max() <= 0x7E                    # saturates: no NaN from a finite (or infinite) input
    assert quantize(-0.0, s32) == 0x80                   # -0 is kept
    assert quantize(float("nan"), s32) & 0x7F == 0x7F    # NaN maps to NaN
    assert quantize(1e30, s32) == 0x7E and quantize(-1e30, s32) == 0xFE


def test_dequantize_equals_torch_for_every_byte():
    b = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    want = b.view(torch.float8_e4m3fn).float().numpy()
    dequantize = _abi.lib().mfa_kv_dequantize_e4m3
    got = np.array([dequantize(int(v)) for v in b], dtype=np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and int(np.isnan(want).sum()) == 2
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))   # bits: -0 included
    for v in range(256):   # a round trip through the quantiser is the identity on every finite byte
        if not np.isnan(want[v]):
            assert _abi.lib().mfa_kv_quantize_e4m3(float(want[v]), 1.0) == v


def decode_refused(status, needle, decode=None, **over):
    kw = shape(**over)
    kw.setdefault("strides", fp8_strides((decode or AttentionDecodeFP8(128)).headDimension))
    with pytest.raises(MFAError) as e:
        (decode or AttentionDecodeFP8(128, P.BF16)).launchForm(**kw)
    assert e.value.status == status, str(e.value)
    assert needle in str(e.value), str(e.value)


def test_decode_refusals_name_the_requirement():
    decode_refused(UNSUPPORTED, "e4m3", decode=AttentionDecodeFP8(128, P.BF16, cachePrecision=KVCachePrecision.E5M2))
    decode_refused(UNSUPPORTED, "e5m2", decode=AttentionDecodeFP8(128, P.BF16, cachePrecision=KVCachePrecision.E5M2))
    decode_refused(INVALID, "MFA_KV_E4M3", decode=AttentionDecodeFP8(128, P.BF16, cachePrecision=int(P.BF16)))
    decode_refused(UNSUPPORTED, "16-bit Q", decode=AttentionDecodeFP8(128, P.FP32))
    decode_refused(UNSUPPORTED, "64 and 128", decode=AttentionDecodeFP8(96, P.BF16), strides=fp8_strides(96))
    decode_refused(UNSUPPORTED, "= 40 rows", rows=5)                                   # M = 8 x 5
    decode_refused(UNSUPPORTED, "at most 32", rows=5)
    decode_refused(INVALID, "strides of K must be multiples of 16", strides=dict(K=(136, 136 * 4096, 8 * 136 * 4096)))   # fine for 16-bit
    decode_refused(INVALID, "strides of V must be multiples of 16", strides=dict(K=(128, 128 * 4096, 8 * 128 * 4096), V=(128, 128 * 4096 + 8, 0)))
    decode_refused(INVALID, "power of two from 16 to 1024", pageSize=24, blockTable=0x2000, blockTableStride=1024)
    decode_refused(INVALID, "power of two", pageSize=2048, blockTable=0x2000, blockTableStride=1024)
    decode_refused(INVALID, "needs blockTable", pageSize=64)
    decode_refused(INVALID, "cacheLengths is required", cacheLengths=None)
    d = AttentionDecodeFP8(128)
    for bufs, needle in (((0, 0x100, 0x100, 0x100), "null argument"), ((0x100, 0x108, 0x100, 0x100), "16-byte aligned")):
        with pytest.raises(MFAError) as e:
            d.dispatch(*bufs, **shape())
        assert e.value.status == INVALID and needle in str(e.value)


def append_refused(status, needle, append=None, bufs=(0x100, 0x200, 0x300, 0x400), **over):
    kw = dict(rows=1, heads=8, batches=4, column=4096, cacheLengths=LENGTHS)
    kw.update(over)
    with pytest.raises(MFAError) as e:
        (append or KVCacheAppend(128, P.BF16, KVCachePrecision.E4M3)).dispatch(*bufs, **kw)
    assert e.value.status == status, str(e.value)
    assert needle in str(e.value), str(e.value)


def test_append_refusals_name_the_requirement():
    """every one of these returns before any GPU call: the buffers are made-up addresses"""
    append_refused(UNSUPPORTED, "e4m3", append=KVCacheAppend(128, P.BF16, KVCachePrecision.E5M2))
    append_refused(UNSUPPORTED, "16-bit", append=KVCacheAppend(128, P.FP32, KVCachePrecision.E4M3))
    append_refused(INVALID, "cachePrecision", append=KVCacheAppend(128, P.BF16, int(P.FP16)))
    append_refused(UNSUPPORTED, "64 and 128", append=KVCacheAppend(96, P.BF16, KVCachePrecision.E4M3))
    append_refused(INVALID, "strides of kCache must be multiples of 16", strides=dict(kCache=(136, 136 * 4096, 8 * 136 * 4096)))
    append_refused(INVALID, "strides of vNew must be multiples of 8", strides=dict(vNew=(132, 132, 8 * 132)))
    append_refused(INVALID, "smaller than the head dimension", strides=dict(vCache=(64, 64 * 4096, 8 * 64 * 4096)))
    append_refused(INVALID, "power of two from 16 to 1024", pageSize=48, blockTable=0x2000, blockTableStride=8)
    append_refused(INVALID, "needs blockTable", pageSize=64)
    append_refused(INVALID, "blockTableStride", pageSize=64, blockTable=0x2000, blockTableStride=0)
    append_refused(INVALID, "column", column=0)
    append_refused(INVALID, "cacheLengths is required", cacheLengths=None)
    append_refused(INVALID, "go with an e4m3 cache", append=KVCacheAppend(128, P.BF16), keyScale=0x5000)
    append_refused(INVALID, "go with an e4m3 cache", append=KVCacheAppend(64, P.FP16), valueScale=0x5000)
    append_refused(INVALID, "null argument", bufs=(0x100, 0x200, 0, 0x400))
    append_refused(INVALID, "16-byte aligned", bufs=(0x100, 0x200, 0x308, 0x400))


@pytest.mark.parametrize("D,prec", [(64, P.BF16), (128, P.FP16), (128, P.BF16)])
def test_plan_is_the_16_bit_launch_plan(D, prec):
    d8, d16 = AttentionDecodeFP8(D, prec), AttentionDecode(D, prec)
    tname = "bf16" if prec == P.BF16 else "f16"
    paged = dict(pageSize=16, blockTable=0x2000, blockTableStride=2048, pageStrides=(8 * 16 * D, 8 * 16 * D),
                 strides=dict(K=(D, 16 * D, 0), V=(D, 16 * D, 0)))
    for kw in (shape(batches=1, column=32768), shape(batches=1, column=32768, rows=4), shape(batches=64, column=32768),
               shape(batches=32, column=4096), shape(batches=1, column=8 * 64), shape(batches=1, column=7 * 64),
               dict(shape(batches=1, column=32768), **paged)):
        need = d16.workspaceSize(**kw)
        assert d8.workspaceSize(**kw) == need
        for ws in (dict(workspace=0x4000, workspaceBytes=need) if need else {}, {}):
            t8, t16 = d8.launchForm(**ws, **kw), d16.launchForm(**ws, **kw)
            assert f"attn_decode8_d{D}_{tname}_" in t8 and "attn_decode16" not in t8.split(" + ")[0], t8
            # the same grid, piece count and combine kernel: the texts differ in the main kernel's family only
            assert t8.replace("attn_decode8_", "attn_decode16_") == t16, (t8, t16)
    text = d8.launchForm(workspace=0x4000, workspaceBytes=d8.workspaceSize(**shape(batches=1, column=32768)), **shape(batches=1, column=32768))
    assert f"attn_decode8_d{D}_{tname}_pieces" in text and "64 pieces" in text and f"attn_decode16_d{D}_{tname}_combine" in text, text
    need = d8.workspaceSize(**shape())
    with pytest.raises(MFAError) as e:
        d8.launchForm(workspace=0x4000, workspaceBytes=need - 4, **shape())
    assert "needs %d" % need in str(e.value)
