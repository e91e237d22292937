"""CPU test (fake tensors, no device): the torch binding of include/mfa_mla_sparse_fp8.h -- flash_mla_sparse_decode_fp8 reaches the op
mfa::attention_mla_sparse_decode_fp8, kept in a list of its own beside the lists that existed, with _fake_mla as its fake; what the
operands may be is said in words, the words of the two functions it combines."""
import inspect

import pytest

torch = pytest.importorskip("torch")

from torch._subclasses.fake_tensor import FakeTensorMode  # noqa: E402

import metal_flash_attention_amd as mfa  # noqa: E402
from metal_flash_attention_amd import torch_binding as tb  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _ops():
    assert hasattr(torch.library, "custom_op") and tb._HAVE_MLA_SPARSE_FP8_OP, "the installed torch has no torch.library.custom_op: the op is missing"


def operands(R=2, topk=100):
    q = torch.empty((3, 16, R, 576), dtype=torch.bfloat16, device="cuda")
    kv = torch.empty((3, 1024, 576), dtype=torch.float8_e4m3fn, device="cuda")
    pool = torch.empty((70, 64, 576), dtype=torch.float8_e4m3fn, device="cuda")
    lens = torch.empty((3,), dtype=torch.int32, device="cuda")
    table = torch.empty((3, 16), dtype=torch.int32, device="cuda")
    idx = torch.empty((3, R, topk), dtype=torch.int32, device="cuda")
    kvs = torch.empty((1,), dtype=torch.float32, device="cuda")
    return q, kv, pool, lens, table, idx, kvs


def test_the_op_s_schema_and_its_list():
    schema = str(torch.ops.mfa.attention_mla_sparse_decode_fp8.default._schema)
    assert schema == ("mfa::attention_mla_sparse_decode_fp8(Tensor q, Tensor kv_cache, Tensor cache_lengths, Tensor indices, Tensor? block_table, "
                      "bool causal, float softmax_scale, SymInt pieces, Tensor? kv_scale) -> (Tensor, Tensor)"), schema
    assert [op[0] for op in tb._MLA_SPARSE_FP8_OPS] == ["attention_mla_sparse_decode_fp8"] and tb._MLA_SPARSE_FP8_OPS[0][2] is tb._fake_mla
    assert tb._MLA_SPARSE_FP8_OPS[0][3] == ()                                               # nothing is mutated
    # the lists that existed are as they were
    assert [op[0] for op in tb._MLA_SPARSE_OPS] == ["attention_mla_sparse_decode"]
    assert [op[0] for op in tb._MLA_CACHE_OPS] == ["mla_cache_append", "attention_mla_decode_fp8"]
    assert [op[0] for op in tb._CACHE_OPS][-1] == "attention_mla_decode" and len(tb._CACHE_OPS) == 18
    assert str(torch.ops.mfa.attention_mla_sparse_decode.default._schema) == (
        "mfa::attention_mla_sparse_decode(Tensor q, Tensor kv_cache, Tensor cache_lengths, Tensor indices, Tensor? block_table, bool causal, "
        "float softmax_scale, SymInt pieces) -> (Tensor, Tensor)")
    assert mfa.flash_mla_sparse_decode_fp8 is tb.flash_mla_sparse_decode_fp8
    assert issubclass(mfa.AttentionMLASparseDecodeFP8, mfa.AttentionMLASparseDecode)


def test_the_signature():
    sig = inspect.signature(tb.flash_mla_sparse_decode_fp8)
    assert list(sig.parameters) == ["q", "kv_cache", "cache_lengths", "indices", "softmax_scale", "kv_scale", "block_table", "causal", "return_lse",
                                    "pieces"]
    scale = sig.parameters["softmax_scale"]
    assert scale.default is inspect.Parameter.empty and scale.kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["kv_scale"].default is None and sig.parameters["kv_scale"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["pieces"].default is None and sig.parameters["causal"].default is True and sig.parameters["return_lse"].default is False
    with FakeTensorMode():
        q, kv, _pool, lens, _table, idx, _kvs = operands()
        with pytest.raises(TypeError, match="softmax_scale"):
            tb.flash_mla_sparse_decode_fp8(q, kv, lens, idx)


@pytest.mark.parametrize("R, topk", [(1, 1), (2, 100), (4, 2048), (32, 33)])
def test_the_fake_gives_the_right_shapes(R, topk):
    with FakeTensorMode():
        q, kv, pool, lens, table, idx, kvs = operands(R, topk)
        o, l = torch.ops.mfa.attention_mla_sparse_decode_fp8(q, kv, lens, idx, None, True, 0.1352, 0, kvs)
        assert o.shape == (3, 16, R, 512) and o.dtype == torch.bfloat16 and l.shape == (3, 16, R) and l.dtype == torch.float32
        assert o.device.type == "cuda"
        o = tb.flash_mla_sparse_decode_fp8(q, kv, lens, idx, softmax_scale=0.1352)
        assert o.shape == (3, 16, R, 512) and o.dtype == torch.bfloat16
        o, lse = tb.flash_mla_sparse_decode_fp8(q.half(), pool, lens.long(), idx, softmax_scale=0.1352, kv_scale=kvs, block_table=table, causal=False,
                                                return_lse=True, pieces=7)
        assert o.shape == (3, 16, R, 512) and o.dtype == torch.float16 and lse.shape == (3, 16, R) and lse.dtype == torch.float32
        # a list is taken where it lies: the first topk slots of a wider allocation
        wide = torch.empty((3, R, topk + 24), dtype=torch.int32, device="cuda")[:, :, :topk]
        assert tb.flash_mla_sparse_decode_fp8(q, kv, lens, wide, softmax_scale=1.0, kv_scale=kvs).shape == (3, 16, R, 512)


def test_the_refusals_in_words():
    with FakeTensorMode():
        q, kv, pool, lens, table, idx, kvs = operands()
        f = tb.flash_mla_sparse_decode_fp8
        for call, kind, needle in (
                (lambda: f(q.cpu(), kv, lens, idx, softmax_scale=0.1), RuntimeError, "tensors must live on the GPU"),
                (lambda: f(q, kv.cpu(), lens, idx, softmax_scale=0.1), RuntimeError, "tensors must live on the GPU"),
                (lambda: f(q, kv, lens.cpu(), idx, softmax_scale=0.1), RuntimeError, "tensors must live on the GPU"),
                (lambda: f(q, kv, lens, idx.cpu(), softmax_scale=0.1), RuntimeError, "tensors must live on the GPU"),
                (lambda: f(q.clone().requires_grad_(), kv, lens, idx, softmax_scale=0.1), RuntimeError, "forward only (no autograd)"),
                # a 16-bit cache: the words of flash_mla_decode_fp8
                (lambda: f(q, kv.to(torch.bfloat16), lens, idx, softmax_scale=0.1), TypeError, "the latent cache must be torch.float8_e4m3fn (got torch.bfloat16)"),
                (lambda: f(q, kv.to(torch.float8_e5m2), lens, idx, softmax_scale=0.1), TypeError, "the latent cache must be torch.float8_e4m3fn"),
                (lambda: f(q.float(), kv, lens, idx, softmax_scale=0.1), TypeError, "q must be bfloat16 or float16"),
                # the lists: the words of flash_mla_sparse_decode
                (lambda: f(q, kv, lens, idx.long(), softmax_scale=0.1), TypeError, "indices must be int32 key positions"),
                (lambda: f(q, kv, lens, idx[0], softmax_scale=0.1), ValueError, "indices must be [B, R, topk] = [3, 2, topk >= 1]"),
                (lambda: f(q, kv, lens, idx[:, :, :0], softmax_scale=0.1), ValueError, "indices must be [B, R, topk] = [3, 2, topk >= 1]"),
                (lambda: f(q, kv, lens, idx[:, :, ::2], softmax_scale=0.1), ValueError, "indices must have a contiguous last dimension"),
                # a bad kv_scale: the words of _latent_scale
                (lambda: f(q, kv, lens, idx, softmax_scale=0.1, kv_scale=kvs.cpu()), RuntimeError, "kv_scale must live on the GPU of the cache"),
                (lambda: f(q, kv, lens, idx, softmax_scale=0.1, kv_scale=kvs.double()), ValueError, "kv_scale must be float32 [1]"),
                (lambda: f(q, kv, lens, idx, softmax_scale=0.1, kv_scale=torch.empty((3,), dtype=torch.float32, device="cuda")), ValueError,
                 "kv_scale must be float32 [1]"),
                (lambda: f(q[..., :512], kv, lens, idx, softmax_scale=0.1), ValueError, "expected q [B, H, R, 576] and kv_cache [B, C, 576]"),
                (lambda: f(q, kv, lens, idx, softmax_scale=0.0), ValueError, "softmax_scale must be a finite number > 0"),
                (lambda: f(q, kv, lens, idx, softmax_scale=0.1, pieces=65), ValueError, "pieces must be an int from 0 to 64")):
            with pytest.raises(kind) as said:
                call()
            assert needle in str(said.value) and str(said.value).startswith("flash_mla_sparse_decode_fp8"), str(said.value)


def test_the_existing_functions_refuse_in_their_own_words():
    with FakeTensorMode():
        q, kv, _pool, lens, _table, idx, _kvs = operands()
        with pytest.raises(TypeError) as said:
            tb.flash_mla_sparse_decode(q, kv, lens, idx, softmax_scale=0.1)
        assert str(said.value).startswith("flash_mla_sparse_decode: q and the latent cache must share one of bfloat16 / float16")
        with pytest.raises(TypeError) as said:
            tb.flash_mla_decode_fp8(q, kv.to(torch.bfloat16), lens, softmax_scale=0.1)
        assert str(said.value).startswith("flash_mla_decode_fp8: the latent cache must be torch.float8_e4m3fn")
