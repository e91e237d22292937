"""CPU test (no GPU call, through the built library and fake tensors): the host side of sparse MLA prefill over an e4m3 latent cache,
include/mfa_mla_prefill_sparse_fp8.h -- every declared name exported and listed, the three blocks it takes unchanged, the launch form's
kernel and grid factors, every refusal in the stated order by status and words, and the torch op's list: the pointers are made up."""
import ctypes
import os
import re

import pytest

import metal_flash_attention_amd as mfa
from metal_flash_attention_amd import AttentionMLAPrefillFP8, AttentionMLAPrefillSparse, AttentionMLAPrefillSparseFP8, GEMMOperandPrecision as P, MFAError, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS, Q, KV, O, L, IDX, INVALID, UNSUPPORTED = 0x1000, 0x10000, 0x20000, 0x30000, 0x40000, 0x200000, 2, 3   # (the host reads no pointer)


def shape(**over):
    return dict(dict(rows=512, column=32768, heads=128, batches=2, scale=0.1352, cacheLengths=LENGTHS), **over)


def test_header_symbols_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "mfa_mla_prefill_sparse_fp8.h")).read()
    declared = set(re.findall(r"\b(mfa_\w+)\s*\(", header.split("#ifndef MFA_MLA_PREFILL_SPARSE_FP8_H")[1]))
    handle = _abi.lib()
    assert declared == {s[0] for s in _abi.MLA_PREFILL_SPARSE_FP8_SYMBOLS} == {"mfa_attention_mla_prefill_sparse_fp8_" + v for v in ("launch", "launch_form", "time")}
    for name, restype, argtypes in _abi.MLA_PREFILL_SPARSE_FP8_SYMBOLS:
        fn = getattr(handle, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert int(handle.mfa_abi_version()) == 6 == _abi.EXPECTED_ABI   # mfa.h did not change
    assert handle.mfa_mla_prefill_params_size() == 168 and handle.mfa_mla_sparse_size() == 32 and ctypes.sizeof(_abi.mfa_mla_quant) == 16
    assert mfa.AttentionMLAPrefillSparseFP8 is AttentionMLAPrefillSparseFP8 and issubclass(AttentionMLAPrefillSparseFP8, AttentionMLAPrefillSparse)


@pytest.mark.parametrize("heads,groups", [(16, 1), (32, 1), (40, 2), (129, 5)])   # 32 heads a workgroup at every head count
def test_the_launch_form_names_the_kernel_and_the_grid_factors(heads, groups):
    form = AttentionMLAPrefillSparseFP8(P.FP16).launchForm(**shape(heads=heads, rows=37, batches=3, indices=IDX, topk=45, kvScale=LENGTHS))
    assert form == "attn_mla8px1_d576_f16 (grid %d = %d groups of 32 heads x 37 rows x 3 sequences, topk 45, contiguous)" % (groups * 37 * 3, groups), form


def outcome(sparse=True, quant=True, form=None, precision=P.BF16, kv=KV, **over):
    """the launch entry's (form: launch_form's, with that buffer) (status, words).  sparse / quant: False a NULL block, a dict its fields"""
    handle = _abi.lib()
    p, _keep = AttentionMLAPrefillSparseFP8(precision)._params(**shape(**over))
    s = _abi.mfa_mla_sparse(indices=IDX, topk=2048, indexRowStride=2048, indexBatchStride=0)
    qt = _abi.mfa_mla_quant(cachePrecision=_abi.MFA_KV_E4M3)
    for block, fields in ((s, sparse), (qt, quant)):
        for name, value in (fields.items() if isinstance(fields, dict) else ()):
            setattr(block, name, value)
    blocks = (ctypes.byref(p), ctypes.byref(s) if sparse else None, ctypes.byref(qt) if quant else None)
    status = handle.mfa_attention_mla_prefill_sparse_fp8_launch_form(*blocks, *form) if form else \
        handle.mfa_attention_mla_prefill_sparse_fp8_launch(Q, kv, O, L, *blocks, None)
    return status, handle.mfa_last_error_string().decode()


def dense(precision=P.BF16, kv=KV, **over):   # AttentionMLAPrefillFP8's answer to the same mistake
    try:
        AttentionMLAPrefillFP8(precision).dispatch(Q, kv, O, L, **shape(**over))
    except MFAError as e:
        return e.status, str(e).split(": ", 1)[1]
    return 0, ""


REFUSALS = [   # in the stated order: each case also carries mistakes of the cases BELOW it, and is refused for its own
    ("a null sparse block", dict(sparse=False, quant=False, rows=0), INVALID, "null mfa_mla_sparse: the sparse entries require the block"),
    ("a null quant block", dict(quant=False, rows=0, kv=KV + 8), INVALID, "null mfa_mla_quant: the fp8 prefill entries require the block"),
    ("a 16-bit cachePrecision", dict(quant=dict(cachePrecision=int(P.BF16), reserved=3), rows=0), INVALID, "mfa_mla_quant.cachePrecision must be MFA_KV_E4M3, not"),
    ("quant.reserved", dict(quant=dict(reserved=3), form=(None, 64), scale=0.0), INVALID, "mfa_mla_quant.reserved must be 0, not 3"),
    ("no launch_form buffer", dict(form=(None, 64), scale=0.0), INVALID, "null argument"),
    ("an FP32 Q", dict(precision=P.FP32, rows=0, kv=KV + 8), UNSUPPORTED, "an FP32 cache has no kernel"),
    ("zero rows", dict(rows=0, kv=KV + 8), INVALID, "non-zero"),
    ("a 16-bit plan's KV stride", dict(strides=dict(KV=(584, 0, 0)), kv=KV + 8), INVALID, "multiples of 16 elements (16-byte rows of an e4m3 cache)"),
    ("misaligned buffers", dict(kv=KV + 8), INVALID, "Q, KV and O must be 16-byte aligned"),
]


@pytest.mark.parametrize("name,kw,status,needle", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_a_refusal_names_its_requirement(name, kw, status, needle):
    got = outcome(**kw)
    assert got[0] == status and needle in got[1], got
    if "mfa_mla" not in needle and "form" not in kw:   # not about a block: word for word the e4m3 prefill's text for the same mistake
        assert got == dense(**kw)


def test_the_torch_op_and_its_list():
    torch = pytest.importorskip("torch")
    from torch._subclasses.fake_tensor import FakeTensorMode
    from metal_flash_attention_amd import torch_binding as tb
    assert [op[0] for op in tb._MLA_SPARSE_PREFILL_FP8_OPS] == ["attention_mla_sparse_prefill_fp8"]
    assert tb._MLA_SPARSE_PREFILL_FP8_OPS[0][2:] == (tb._fake_mla, ()) and mfa.flash_mla_sparse_prefill_fp8 is tb.flash_mla_sparse_prefill_fp8
    assert str(torch.ops.mfa.attention_mla_sparse_prefill_fp8.default._schema) == (
        "mfa::attention_mla_sparse_prefill_fp8(Tensor q, Tensor kv_cache, Tensor cache_lengths, Tensor indices, Tensor? q_lengths, "
        "Tensor? block_table, bool causal, float softmax_scale, Tensor? kv_scale) -> (Tensor, Tensor)")
    with FakeTensorMode():
        q, kv8 = torch.empty((3, 40, 70, 576), dtype=torch.bfloat16, device="cuda"), torch.empty((3, 1024, 576), dtype=torch.float8_e4m3fn, device="cuda")
        lens, idx = torch.empty((3,), dtype=torch.int32, device="cuda"), torch.empty((3, 70, 45), dtype=torch.int32, device="cuda")
        o, lse = tb.flash_mla_sparse_prefill_fp8(q, kv8, lens, idx, softmax_scale=0.1352, q_lengths=lens, return_lse=True,
                                                 kv_scale=torch.empty((1,), dtype=torch.float32, device="cuda"))
        assert o.shape == (3, 40, 70, 512) and o.dtype == q.dtype and lse.shape == (3, 40, 70) and lse.dtype == torch.float32
        with pytest.raises(TypeError) as e:
            tb.flash_mla_sparse_prefill_fp8(q, kv8.to(torch.bfloat16), lens, idx, softmax_scale=0.1)
        assert "a 16-bit latent cache is flash_mla_sparse_prefill's" in str(e.value)
