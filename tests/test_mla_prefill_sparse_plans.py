"""CPU test (no GPU call, through the built library and fake tensors): the host side of sparse MLA prefill,
include/mfa_mla_prefill_sparse.h -- every declared name exported and listed, the two blocks it takes unchanged, the launch form's kernel
and grid factors, every refusal in the stated order by status and words, and the torch op's list and refusals: the pointers are made up."""
import ctypes
import os
import re

import pytest

import metal_flash_attention_amd as mfa
from metal_flash_attention_amd import AttentionMLAPrefill, AttentionMLAPrefillSparse, GEMMOperandPrecision as P, MFAError, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS, Q, KV, O, L, IDX = 0x1000, 0x10000, 0x20000, 0x30000, 0x40000, 0x200000   # the host reads none of them
INVALID, UNSUPPORTED = 2, 3


def shape(**over):
    return dict(dict(rows=512, column=32768, heads=128, batches=2, scale=0.1352, cacheLengths=LENGTHS, indices=IDX, topk=2048), **over)


def test_header_symbols_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "mfa_mla_prefill_sparse.h")).read()
    declared = set(re.findall(r"\b(mfa_\w+)\s*\(", header.split("#ifndef MFA_MLA_PREFILL_SPARSE_H")[1]))
    handle = _abi.lib()
    assert declared == {s[0] for s in _abi.MLA_PREFILL_SPARSE_SYMBOLS} == {"mfa_attention_mla_prefill_sparse_" + v for v in ("launch", "launch_form", "time")}
    for name, restype, argtypes in _abi.MLA_PREFILL_SPARSE_SYMBOLS:
        fn = getattr(handle, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert int(handle.mfa_abi_version()) == 6 == _abi.EXPECTED_ABI   # mfa.h did not change
    assert handle.mfa_mla_prefill_params_size() == 168 and handle.mfa_mla_sparse_size() == 32   # nor did the two blocks
    assert mfa.AttentionMLAPrefillSparse is AttentionMLAPrefillSparse and issubclass(AttentionMLAPrefillSparse, AttentionMLAPrefill)


@pytest.mark.parametrize("heads,groups", [(16, 1), (32, 1), (40, 2), (129, 5)])   # 32 heads a workgroup at every head count
def test_the_launch_form_names_the_kernel_and_the_grid_factors(heads, groups):
    form = AttentionMLAPrefillSparse(P.FP16).launchForm(**shape(heads=heads, rows=37, batches=3, topk=45))
    assert form == "attn_mla16px1_d576_f16 (grid %d = %d groups of 32 heads x 37 rows x 3 sequences, topk 45, contiguous)" % (groups * 37 * 3, groups), form


def outcome(op, kw, kv=KV):
    try:
        op.dispatch(Q, kv, O, L, **kw)
    except MFAError as e:
        return e.status, str(e).split(": ", 1)[1]
    return 0, ""


SP = AttentionMLAPrefillSparse(P.BF16)
REFUSALS = [   # in the stated order: each case also carries every mistake of the cases BELOW it that it can, and is refused for its own
    ("null indices", SP, shape(indices=None, topk=0, rows=0), INVALID, "mfa_mla_sparse.indices is required"),
    ("topk 0", SP, shape(topk=0, indices=IDX + 2, rows=0), INVALID, "mfa_mla_sparse.topk must be at least 1"),
    ("a row stride below topk", SP, shape(indexStrides=(2047, 4096), indices=IDX + 2, rows=0), INVALID,
     "mfa_mla_sparse.indexRowStride must be at least topk = 2048 entries, not 2047"),
    ("misaligned indices", SP, shape(indices=IDX + 2, rows=0), INVALID, "mfa_mla_sparse.indices must be 4-byte aligned"),
    ("fp32 inputs", AttentionMLAPrefillSparse(P.FP32), shape(), UNSUPPORTED, "an FP32 cache has no kernel"),
    ("zero rows", SP, shape(rows=0), INVALID, "non-zero"),
    ("a cache row stride off 8 elements", SP, shape(strides=dict(KV=(580, 0, 32768 * 580))), INVALID, "strides of KV must be multiples of 8 elements"),
]


@pytest.mark.parametrize("name,op,kw,status,needle", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_a_refusal_names_its_requirement(name, op, kw, status, needle):
    got = outcome(op, kw)
    assert got[0] == status and needle in got[1], got
    if op is SP and "mfa_mla_sparse" not in needle:   # word for word the dense prefill's text for the same mistake
        dense = {k: v for k, v in kw.items() if k not in ("indices", "topk", "indexStrides")}
        assert got == outcome(AttentionMLAPrefill(P.BF16), dense)


def test_the_block_comes_first_and_the_buffers_last():
    handle = _abi.lib()
    p, _keep = SP._params(**{k: v for k, v in shape().items() if k not in ("indices", "topk")})
    out, ms = ctypes.create_string_buffer(64), ctypes.c_float(0)
    for status in (handle.mfa_attention_mla_prefill_sparse_launch(Q, KV, O, L, None, None, None),
                   handle.mfa_attention_mla_prefill_sparse_launch_form(ctypes.byref(p), None, out, 64),
                   handle.mfa_attention_mla_prefill_sparse_time(Q, KV, O, L, ctypes.byref(p), None, None, 0, 1, ctypes.byref(ms))):
        assert status == INVALID and handle.mfa_last_error_string().startswith(b"null mfa_mla_sparse: the sparse entries require the block")
    block = _abi.mfa_mla_sparse(indices=IDX, topk=64, reserved=4, indexRowStride=8, indexBatchStride=0)   # reserved ahead of the stride
    assert handle.mfa_attention_mla_prefill_sparse_launch(Q, KV, O, L, None, ctypes.byref(block), None) == INVALID
    assert handle.mfa_last_error_string() == b"mfa_mla_sparse.reserved must be 0, not 4"
    block.reserved, block.indexRowStride = 0, 64
    p.scale = 0.0                                                         # no buffer: after the block, ahead of the params' mistakes
    assert handle.mfa_attention_mla_prefill_sparse_launch_form(ctypes.byref(p), ctypes.byref(block), None, 64) == INVALID
    assert handle.mfa_last_error_string() == b"null argument"
    assert handle.mfa_attention_mla_prefill_sparse_launch(Q, KV, O, L, None, ctypes.byref(block), None) == INVALID   # NULL params: prefill's words
    assert handle.mfa_last_error_string() == b"null argument"
    got = outcome(SP, shape(), kv=KV + 8)                                 # the buffers: after everything else
    assert got[0] == INVALID and "Q, KV and O must be 16-byte aligned" in got[1], got


def test_the_torch_op_its_list_and_its_refusals():
    torch = pytest.importorskip("torch")
    from torch._subclasses.fake_tensor import FakeTensorMode
    from metal_flash_attention_amd import torch_binding as tb
    assert [op[0] for op in tb._MLA_SPARSE_PREFILL_OPS] == ["attention_mla_sparse_prefill"] and tb._MLA_SPARSE_PREFILL_OPS[0][2:] == (tb._fake_mla, ())
    assert mfa.flash_mla_sparse_prefill is tb.flash_mla_sparse_prefill
    assert str(torch.ops.mfa.attention_mla_sparse_prefill.default._schema) == (
        "mfa::attention_mla_sparse_prefill(Tensor q, Tensor kv_cache, Tensor cache_lengths, Tensor indices, Tensor? q_lengths, Tensor? block_table, "
        "bool causal, float softmax_scale) -> (Tensor, Tensor)")
    with FakeTensorMode():
        q, kv = (torch.empty(s, dtype=torch.bfloat16, device="cuda") for s in ((3, 40, 70, 576), (3, 1024, 576)))
        lens, idx = torch.empty((3,), dtype=torch.int32, device="cuda"), torch.empty((3, 70, 45), dtype=torch.int32, device="cuda")
        o, l = torch.ops.mfa.attention_mla_sparse_prefill(q, kv, lens, idx, lens, None, True, 0.1352)
        assert o.shape == (3, 40, 70, 512) and o.dtype == q.dtype and l.shape == (3, 40, 70) and l.dtype == torch.float32
        f = tb.flash_mla_sparse_prefill
        with pytest.raises(TypeError, match="softmax_scale"):
            f(q, kv, lens, idx)
        for call, error, needle in ((lambda: f(q, kv, lens, idx.long(), softmax_scale=0.1), TypeError, "indices must be int32 key positions"),
                                    (lambda: f(q.float(), kv, lens, idx, softmax_scale=0.1), TypeError, "q must be bfloat16 or float16"),
                                    (lambda: f(q, kv, lens, idx[:, :32], softmax_scale=0.1), ValueError, r"indices must be \[B, R, topk\] = \[3, 70, topk >= 1\]"),
                                    (lambda: f(q, kv, lens, idx, softmax_scale=0.1, q_lengths=lens[:2]), ValueError, "q_lengths")):
            with pytest.raises(error, match=needle):
                call()
