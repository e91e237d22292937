"""CPU test (no GPU call, through the built library): the host side of MLA prefill over an e4m3 latent cache, include/mfa_mla_prefill_fp8.h --
the header's symbols, every refusal by the name in its message, the launch forms of the unsplit and the cut launch, the workspace size
against the 16-bit cut launch's, and flash_mla_prefill_fp8 / flash_mla_prefill refusing each other's caches in words (fake tensors)."""
import ctypes
import os
import re

import pytest

from metal_flash_attention_amd import (AttentionMLAPrefill, AttentionMLAPrefillFP8, AttentionMLAPrefillFP8Split, AttentionMLAPrefillSplit,
                                       GEMMOperandPrecision as P, KVCachePrecision, MFAError, _abi)

ROOT = os.path.join(os.path.dirname(__file__), "..")
WS = 0x7F0000000000   # a pointer nobody follows: no entry here reaches the GPU


def shape(**kw):
    return dict(dict(rows=64, column=32832, heads=16, batches=1, scale=0.125, cacheLengths=WS), **kw)


def test_header_symbols_and_what_has_not_moved():
    header = open(os.path.join(ROOT, "include", "mfa_mla_prefill_fp8.h")).read()
    declared = set(re.findall(r"\b(mfa_\w+)\s*\(", header.split("#ifndef MFA_MLA_PREFILL_FP8_H")[1]))
    assert declared == {s[0] for s in _abi.MLA_PREFILL_FP8_SYMBOLS} == (
        {"mfa_attention_mla_prefill_fp8_" + s for s in ("launch", "launch_form", "time")}
        | {"mfa_attention_mla_prefill_fp8_split_" + s for s in ("launch", "launch_form", "time", "workspace_size")})
    handle = _abi.lib()
    assert handle.mfa_abi_version() == _abi.EXPECTED_ABI == 6
    assert handle.mfa_mla_prefill_params_size() == ctypes.sizeof(_abi.mfa_mla_prefill_params) == 168 and ctypes.sizeof(_abi.mfa_mla_quant) == 16
    assert issubclass(AttentionMLAPrefillFP8, AttentionMLAPrefill) and issubclass(AttentionMLAPrefillFP8Split, AttentionMLAPrefillSplit)


def test_launch_forms():
    bf, hf = AttentionMLAPrefillFP8(P.BF16), AttentionMLAPrefillFP8(P.FP16)
    assert bf.launchForm(**shape(kvScale=WS)) == "attn_mla8p_d576_bf16 (grid 16 = 16 blocks x 1 sequences, 1024 packed rows in blocks of 64, e4m3 cache, contiguous)"
    assert hf.launchForm(**shape(rows=3, heads=11, batches=2, pageSize=16, blockTable=WS, blockTableStride=4096)) == (
        "attn_mla8p_d576_f16 (grid 2 = 1 blocks x 2 sequences, 33 packed rows in blocks of 64, e4m3 cache, paged)")
    cut = AttentionMLAPrefillFP8Split(P.BF16)
    need, pieces = cut.plannedSplit(**shape())
    assert pieces == 16
    assert cut.launchForm(**shape(workspace=WS, workspaceBytes=need)) == (
        "attn_mla8pk_d576_bf16 (grid 256 = 16 blocks x 1 sequences x 16 pieces, 1024 packed rows in blocks of 64, e4m3 cache, contiguous) + "
        "attn_mla8p_d576_bf16_combine (grid 256)")
    unsplit = bf.launchForm(**shape())
    assert cut.launchForm(**shape()) == unsplit[:-1] + ", unsplit without a workspace: the plan has 16 pieces)"
    assert cut.launchForm(**shape(pieces=1, workspace=WS + 2, workspaceBytes=0)) == unsplit == cut.launchForm(**shape(column=64))


@pytest.mark.parametrize("kw", [shape(), shape(pieces=5), shape(pieces=1), shape(batches=8, heads=128), shape(rows=512, column=33280),
                                shape(rows=1, heads=1, column=100000)])
def test_the_workspace_size_is_the_16_bit_cut_launch_s(kw):
    assert AttentionMLAPrefillFP8Split(P.BF16).plannedSplit(kvScale=WS, **kw) == AttentionMLAPrefillSplit(P.BF16).plannedSplit(**kw)


def test_refusals_by_name():
    unsplit, cut = AttentionMLAPrefillFP8(P.BF16), AttentionMLAPrefillFP8Split(P.BF16)
    need, _ = cut.plannedSplit(**shape())
    e5m2 = AttentionMLAPrefillFP8(P.BF16, cachePrecision=KVCachePrecision.E5M2)
    cases = [
        (e5m2, shape(), "UNSUPPORTED", "e5m2 caches have no kernel"),
        (AttentionMLAPrefillFP8(P.BF16, cachePrecision=int(P.BF16)), shape(), "INVALID", "mfa_mla_quant.cachePrecision must be MFA_KV_E4M3"),
        (unsplit, shape(strides=dict(KV=(584, 0, 0))), "INVALID", "strides of KV must be multiples of 16 elements (16-byte rows of an e4m3 cache)"),
        (cut, shape(strides=dict(KV=(576, 0, 576 * 3 + 8))), "INVALID", "strides of KV must be multiples of 16 elements"),
        (unsplit, shape(pageSize=16, blockTable=WS, blockTableStride=4096, pageStride=16 * 576 + 8), "INVALID", "strides of KV must be multiples of 16"),
        (unsplit, shape(strides=dict(KV=(560, 0, 0))), "INVALID", "leadingDimension of KV is smaller than the head dimension"),
        (cut, shape(pieces=65), "INVALID", "mfa_key_split.pieces must be 0 (the host's plan), 1 (unsplit) or 2 .. 64"),
        (cut, shape(workspace=WS, workspaceBytes=need - 1), "INVALID",
         "workspace too small: %d bytes, the launch needs %d (mfa_attention_mla_prefill_fp8_split_workspace_size)" % (need - 1, need)),
        (cut, shape(workspace=WS + 8, workspaceBytes=need), "INVALID", "workspace must be 16-byte aligned")]
    for host, kw, status, said in cases:
        with pytest.raises(MFAError) as e:
            host.launchForm(**kw)
        assert status in str(e.value) and said in str(e.value), (said, str(e.value))
    # what mla_prefill_prepare_args refuses comes out in the 16-bit entry's words, unsplit and cut
    for kw in (shape(scale=0.0), shape(rows=0), shape(cacheLengths=None), shape(pageSize=24, blockTable=WS, blockTableStride=8)):
        words = []
        for host in (AttentionMLAPrefill(P.BF16), unsplit, cut):
            with pytest.raises(MFAError) as e:
                host.launchForm(**kw)
            words.append(str(e.value))
        assert words[0] == words[1] == words[2], words
    # the blocks themselves, and the buffers: the quant block is looked at first
    lib, out = _abi.lib(), ctypes.create_string_buffer(64)
    p, quant = unsplit._params(**shape())[0], _abi.mfa_mla_quant()
    lib.mfa_mla_quant_init(ctypes.byref(quant))
    said = lambda: lib.mfa_last_error_string().decode()  # noqa: E731
    assert lib.mfa_attention_mla_prefill_fp8_launch_form(ctypes.byref(p), None, out, len(out)) != 0 and "null mfa_mla_quant" in said()
    assert lib.mfa_attention_mla_prefill_fp8_split_launch_form(None, None, None, out, len(out)) != 0 and "null mfa_mla_quant" in said()
    assert lib.mfa_attention_mla_prefill_fp8_split_launch_form(ctypes.byref(p), None, ctypes.byref(quant), out, len(out)) != 0 and "null mfa_key_split" in said()
    quant.reserved = 3
    assert lib.mfa_attention_mla_prefill_fp8_launch_form(ctypes.byref(p), ctypes.byref(quant), out, len(out)) != 0
    assert "mfa_mla_quant.reserved must be 0, not 3" in said()
    quant.reserved = 0
    for bufs, words in (((WS, WS + 8, WS, None), "Q, KV and O must be 16-byte aligned"), ((WS, None, WS, None), "null argument")):
        assert lib.mfa_attention_mla_prefill_fp8_launch(*bufs, ctypes.byref(p), ctypes.byref(quant), None) != 0 and words in said()   # (before any GPU call)
    quant.kvScale = WS + 2
    assert lib.mfa_attention_mla_prefill_fp8_launch(WS, WS, WS, None, ctypes.byref(p), ctypes.byref(quant), None) != 0 and "kvScale must be 4-byte aligned" in said()


def test_the_torch_functions_refuse_each_other_s_caches_in_words():
    torch = pytest.importorskip("torch")
    from torch._subclasses.fake_tensor import FakeTensorMode

    import metal_flash_attention_amd as mfa
    from metal_flash_attention_amd import torch_binding as tb
    assert mfa.flash_mla_prefill_fp8 is tb.flash_mla_prefill_fp8 and tb._HAVE_MLA_PREFILL_FP8_OP
    assert [op[0] for op in tb._MLA_PREFILL_FP8_OPS] == ["attention_mla_prefill_fp8"] and tb._MLA_PREFILL_FP8_OPS[0][2] is tb._fake_mla
    assert str(torch.ops.mfa.attention_mla_prefill_fp8.default._schema) == (
        "mfa::attention_mla_prefill_fp8(Tensor q, Tensor kv_cache, Tensor cache_lengths, Tensor? q_lengths, Tensor? block_table, bool causal, "
        "float softmax_scale, SymInt key_pieces, Tensor? kv_scale) -> (Tensor, Tensor)")
    with FakeTensorMode():
        q = torch.empty((3, 16, 70, 576), dtype=torch.bfloat16, device="cuda")
        kv8 = torch.empty((3, 1024, 576), dtype=torch.float8_e4m3fn, device="cuda")
        lens, kvs = torch.empty((3,), dtype=torch.int32, device="cuda"), torch.empty((1,), dtype=torch.float32, device="cuda")
        o, lse = tb.flash_mla_prefill_fp8(q, kv8, lens, softmax_scale=0.1352, kv_scale=kvs, q_lengths=lens, return_lse=True, key_pieces=None)
        assert o.shape == (3, 16, 70, 512) and o.dtype == torch.bfloat16 and lse.shape == (3, 16, 70) and lse.dtype == torch.float32
        for call, needle in (
                (lambda: tb.flash_mla_prefill_fp8(q, kv8.to(torch.bfloat16), lens, softmax_scale=0.1),
                 "flash_mla_prefill_fp8: the latent cache must be torch.float8_e4m3fn (got torch.bfloat16); a 16-bit latent cache is flash_mla_prefill's"),
                (lambda: tb.flash_mla_prefill_fp8(q, kv8.to(torch.float8_e5m2), lens, softmax_scale=0.1), "e5m2 and fnuz caches have no kernel"),
                (lambda: tb.flash_mla_prefill(q, kv8, lens, softmax_scale=0.1),
                 "flash_mla_prefill: q and the latent cache must share one of bfloat16 / float16 (got torch.bfloat16, torch.float8_e4m3fn); e4m3 latent")):
            with pytest.raises(TypeError) as said:
                call()
            assert needle in str(said.value), str(said.value)
        with pytest.raises(ValueError, match="pieces must be an int from 0 to 64"):
            tb.flash_mla_prefill_fp8(q, kv8, lens, softmax_scale=0.1, key_pieces=65)
        with pytest.raises(ValueError, match=r"kv_scale must be float32 \[1\]"):
            tb.flash_mla_prefill_fp8(q, kv8, lens, softmax_scale=0.1, kv_scale=kvs.double())
