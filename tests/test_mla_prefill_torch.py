"""CPU test (fake tensors, no device): the torch binding of include/mfa_mla_prefill.h -- flash_mla_prefill reaches the op
mfa::attention_mla_prefill, registered like flash_mla_decode's with a fake implementation that gives O [B, H, R, 512] and L [B, H, R];
softmax_scale is required; what the operands may be is said in words; the ops that existed keep their schemas and their lists."""
import inspect

import pytest

torch = pytest.importorskip("torch")

from torch._subclasses.fake_tensor import FakeTensorMode  # noqa: E402

import metal_flash_attention_amd as mfa  # noqa: E402
from metal_flash_attention_amd import torch_binding as tb  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _ops():
    assert hasattr(torch.library, "custom_op") and tb._HAVE_MLA_PREFILL_OP, \
        "the installed torch has no torch.library.custom_op: mfa::attention_mla_prefill is missing"


def operands():
    q = torch.empty((3, 16, 200, 576), dtype=torch.bfloat16, device="cuda")
    kv = torch.empty((3, 1024, 576), dtype=torch.bfloat16, device="cuda")
    pool = torch.empty((70, 64, 576), dtype=torch.float16, device="cuda")
    lens = torch.empty((3,), dtype=torch.int32, device="cuda")
    table = torch.empty((3, 16), dtype=torch.int32, device="cuda")
    return q, kv, pool, lens, table


def test_the_op_s_schema_and_the_old_schemas():
    schema = str(torch.ops.mfa.attention_mla_prefill.default._schema)
    assert schema == ("mfa::attention_mla_prefill(Tensor q, Tensor kv_cache, Tensor cache_lengths, Tensor? q_lengths, Tensor? block_table, bool causal, "
                      "float softmax_scale) -> (Tensor, Tensor)"), schema
    assert "pieces" not in schema and "tree_mask" not in schema and "window" not in schema
    assert str(torch.ops.mfa.attention_mla_decode.default._schema) == (
        "mfa::attention_mla_decode(Tensor q, Tensor kv_cache, Tensor cache_lengths, Tensor? block_table, bool causal, float softmax_scale, "
        "SymInt pieces) -> (Tensor, Tensor)")
    assert [op[0] for op in tb._CACHE_OPS][-1] == "attention_mla_decode" and len(tb._CACHE_OPS) == 18     # a list of its own: no list moved
    assert [op[0] for op in tb._MLA_PREFILL_OPS] == ["attention_mla_prefill"]
    assert mfa.flash_mla_prefill is tb.flash_mla_prefill


def test_softmax_scale_is_required_and_keyword_only():
    sig = inspect.signature(tb.flash_mla_prefill)
    assert list(sig.parameters) == ["q", "kv_cache", "cache_lengths", "softmax_scale", "q_lengths", "block_table", "causal", "return_lse"]
    scale = sig.parameters["softmax_scale"]
    assert scale.default is inspect.Parameter.empty and scale.kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["q_lengths"].default is None and sig.parameters["causal"].default is True and sig.parameters["return_lse"].default is False
    with FakeTensorMode():
        q, kv, _pool, lens, _table = operands()
        with pytest.raises(TypeError, match="softmax_scale"):
            tb.flash_mla_prefill(q, kv, lens)


def test_the_fake_gives_the_right_shapes():
    with FakeTensorMode():
        q, kv, pool, lens, table = operands()
        o, l = torch.ops.mfa.attention_mla_prefill(q, kv, lens, None, None, True, 0.1352)
        assert o.shape == (3, 16, 200, 512) and o.dtype == torch.bfloat16 and l.shape == (3, 16, 200) and l.dtype == torch.float32
        assert o.device.type == "cuda"
        o = tb.flash_mla_prefill(q, kv, lens, softmax_scale=0.1352, q_lengths=lens)
        assert o.shape == (3, 16, 200, 512) and o.dtype == torch.bfloat16
        o, lse = tb.flash_mla_prefill(q.half(), pool, lens.long(), softmax_scale=0.1352, q_lengths=lens.long(), block_table=table, causal=False,
                                      return_lse=True)
        assert o.shape == (3, 16, 200, 512) and o.dtype == torch.float16 and lse.shape == (3, 16, 200) and lse.dtype == torch.float32
        # views are taken as they are: a wider allocation's first 576 columns, a token-major q [B, R, H, 576] seen as [B, H, R, 576]
        wide = torch.empty((3, 1024, 640), dtype=torch.bfloat16, device="cuda")[:, :, :576]
        token_major = torch.empty((3, 200, 16, 576), dtype=torch.bfloat16, device="cuda").transpose(1, 2)
        assert tb.flash_mla_prefill(token_major, wide, lens, softmax_scale=1.0).shape == (3, 16, 200, 512)
        assert tb.flash_mla_prefill(q[:, :, :1], kv, lens, softmax_scale=1.0).shape == (3, 16, 1, 512)          # rows <= 32 are served too


def test_the_refusals_in_words():
    with FakeTensorMode():
        q, kv, pool, lens, table = operands()
        f = tb.flash_mla_prefill
        for call, kind, needle in (
                (lambda: f(q.cpu(), kv, lens, softmax_scale=0.1), RuntimeError, "tensors must live on the GPU"),
                (lambda: f(q, kv.cpu(), lens, softmax_scale=0.1), RuntimeError, "tensors must live on the GPU"),
                (lambda: f(q, kv, lens.cpu(), softmax_scale=0.1), RuntimeError, "tensors must live on the GPU"),
                (lambda: f(q, kv, lens, softmax_scale=0.1, q_lengths=lens.cpu()), RuntimeError, "tensors must live on the GPU"),
                (lambda: f(q, pool.bfloat16(), lens, softmax_scale=0.1, block_table=table.cpu()), RuntimeError, "tensors must live on the GPU"),
                (lambda: f(q.clone().requires_grad_(), kv, lens, softmax_scale=0.1), RuntimeError, "forward only (no autograd)"),
                (lambda: f(q, kv.clone().requires_grad_(), lens, softmax_scale=0.1), RuntimeError, "forward only (no autograd)"),
                (lambda: f(q[..., :512], kv, lens, softmax_scale=0.1), ValueError, "expected q [B, H, R, 576] and kv_cache [B, C, 576]"),
                (lambda: f(q, kv[..., :512], lens, softmax_scale=0.1), ValueError, "expected q [B, H, R, 576] and kv_cache [B, C, 576]"),
                (lambda: f(q, kv[:2], lens, softmax_scale=0.1), ValueError, "expected q [B, H, R, 576] and kv_cache [B, C, 576]"),
                (lambda: f(q[0], kv, lens, softmax_scale=0.1), ValueError, "expected q [B, H, R, 576]"),
                (lambda: f(q, kv.half(), lens, softmax_scale=0.1), TypeError, "q and the latent cache must share one of bfloat16 / float16"),
                (lambda: f(q, kv.to(torch.float8_e4m3fn), lens, softmax_scale=0.1), TypeError, "e4m3 latent caches have no kernel"),
                (lambda: f(q.float(), kv.float(), lens, softmax_scale=0.1), TypeError, "q must be bfloat16 or float16"),
                (lambda: f(q, kv.transpose(1, 2).contiguous().transpose(1, 2), lens, softmax_scale=0.1), ValueError, "contiguous last dimension"),
                (lambda: f(q, kv, lens[:2], softmax_scale=0.1), ValueError, "cache_lengths must be a GPU tensor"),
                (lambda: f(q, kv, lens.float(), softmax_scale=0.1), ValueError, "cache_lengths must be a GPU tensor"),
                (lambda: f(q, kv, lens, softmax_scale=0.1, q_lengths=lens[:2]), ValueError, "q_lengths must be a GPU tensor"),
                (lambda: f(q, kv, lens, softmax_scale=0.1, q_lengths=lens.float()), ValueError, "q_lengths must be a GPU tensor"),
                (lambda: f(q, pool.bfloat16(), lens, softmax_scale=0.1, block_table=table.long()), ValueError, "block_table must be an int32 GPU tensor"),
                (lambda: f(q, pool.bfloat16(), lens, softmax_scale=0.1, block_table=table[:2]), ValueError, "block_table must be an int32 GPU tensor"),
                (lambda: f(q, kv, lens, softmax_scale=0.0), ValueError, "softmax_scale must be a finite number > 0"),
                (lambda: f(q, kv, lens, softmax_scale=float("nan")), ValueError, "softmax_scale must be a finite number > 0"),
                (lambda: f(q, kv, lens, softmax_scale=float("inf")), ValueError, "softmax_scale must be a finite number > 0"),
                (lambda: f(q, kv, lens, softmax_scale=None), ValueError, "softmax_scale must be a finite number > 0")):
            with pytest.raises(kind) as said:
                call()
            assert needle in str(said.value) and str(said.value).startswith("flash_mla_prefill"), str(said.value)
        with pytest.raises(TypeError):
            f(q, kv, lens, softmax_scale=0.1, pieces=2)            # not cut along the keys: no such argument
