"""CPU test (fake tensors, no device): the torch binding of include/mfa_mla_cache.h -- mla_cache_append reaches the op
mfa::mla_cache_append, which mutates kv_cache and returns nothing; flash_mla_decode_fp8 reaches mfa::attention_mla_decode_fp8, whose fake
is flash_mla_decode's (O [B, H, R, 512], L [B, H, R]); what the operands may be is said in words that start with the function's name;
the ops that existed keep their list, and flash_mla_decode still refuses an e4m3 cache."""
import inspect

import pytest

torch = pytest.importorskip("torch")

from torch._subclasses.fake_tensor import FakeTensorMode  # noqa: E402

import metal_flash_attention_amd as mfa  # noqa: E402
from metal_flash_attention_amd import torch_binding as tb  # noqa: E402

E4M3 = torch.float8_e4m3fn


@pytest.fixture(scope="module", autouse=True)
def _ops():
    assert hasattr(torch.library, "custom_op") and tb._HAVE_MLA_CACHE_OPS, "the installed torch has no torch.library.custom_op: the mla cache ops are missing"


def operands():
    q = torch.empty((3, 16, 2, 576), dtype=torch.bfloat16, device="cuda")
    kv = torch.empty((3, 1024, 576), dtype=E4M3, device="cuda")
    pool = torch.empty((70, 64, 576), dtype=E4M3, device="cuda")
    lens = torch.empty((3,), dtype=torch.int32, device="cuda")
    table = torch.empty((3, 16), dtype=torch.int32, device="cuda")
    scale = torch.empty((1,), dtype=torch.float32, device="cuda")
    latent = torch.empty((3, 5, 512), dtype=torch.bfloat16, device="cuda")
    rope = torch.empty((3, 5, 64), dtype=torch.bfloat16, device="cuda")
    return q, kv, pool, lens, table, scale, latent, rope


def test_the_ops_schemas_and_a_list_of_their_own():
    append = torch.ops.mfa.mla_cache_append.default._schema
    assert str(append) == ("mfa::mla_cache_append(Tensor latent_new, Tensor rope_new, Tensor(a2!) kv_cache, Tensor cache_lengths, Tensor? block_table, "
                           "Tensor? kv_scale) -> ()"), str(append)
    assert [a.name for a in append.arguments if a.alias_info is not None and a.alias_info.is_write] == ["kv_cache"]     # mutates_args
    decode = str(torch.ops.mfa.attention_mla_decode_fp8.default._schema)
    assert decode == ("mfa::attention_mla_decode_fp8(Tensor q, Tensor kv_cache, Tensor cache_lengths, Tensor? block_table, bool causal, "
                      "float softmax_scale, SymInt pieces, Tensor? kv_scale) -> (Tensor, Tensor)"), decode
    assert [op[0] for op in tb._MLA_CACHE_OPS] == ["mla_cache_append", "attention_mla_decode_fp8"]
    assert tb._MLA_CACHE_OPS[0][3] == ("kv_cache",) and tb._MLA_CACHE_OPS[1][2] is tb._fake_mla
    assert [op[0] for op in tb._CACHE_OPS][-1] == "attention_mla_decode" and len(tb._CACHE_OPS) == 18       # the old list is as it was
    assert str(torch.ops.mfa.attention_mla_decode.default._schema) == (
        "mfa::attention_mla_decode(Tensor q, Tensor kv_cache, Tensor cache_lengths, Tensor? block_table, bool causal, float softmax_scale, "
        "SymInt pieces) -> (Tensor, Tensor)")
    assert mfa.flash_mla_decode_fp8 is tb.flash_mla_decode_fp8 and mfa.mla_cache_append is tb.mla_cache_append


def test_the_signatures():
    sig = inspect.signature(tb.flash_mla_decode_fp8)
    assert list(sig.parameters) == ["q", "kv_cache", "cache_lengths", "softmax_scale", "kv_scale", "block_table", "causal", "return_lse", "pieces"]
    scale = sig.parameters["softmax_scale"]
    assert scale.default is inspect.Parameter.empty and scale.kind is inspect.Parameter.KEYWORD_ONLY
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("kv_scale", "block_table", "causal", "return_lse", "pieces"))
    assert sig.parameters["kv_scale"].default is None and sig.parameters["pieces"].default is None and sig.parameters["causal"].default is True
    sig = inspect.signature(tb.mla_cache_append)
    assert list(sig.parameters) == ["latent_new", "rope_new", "kv_cache", "cache_lengths", "block_table", "kv_scale"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[n].default is None for n in ("block_table", "kv_scale"))
    assert sig.return_annotation in (None, "None")   # (a string under postponed annotations)
    assert "mla_cache_append" in tb.flash_mla_decode.__doc__ and "no append kernel" not in tb.flash_mla_decode.__doc__
    with FakeTensorMode():
        q, kv, _pool, lens, _table, _scale, _latent, _rope = operands()
        with pytest.raises(TypeError, match="softmax_scale"):
            tb.flash_mla_decode_fp8(q, kv, lens)


def test_the_fakes_give_the_right_shapes():
    with FakeTensorMode():
        q, kv, pool, lens, table, scale, latent, rope = operands()
        o, l = torch.ops.mfa.attention_mla_decode_fp8(q, kv, lens, None, True, 0.1352, 0, scale)
        assert o.shape == (3, 16, 2, 512) and o.dtype == torch.bfloat16 and l.shape == (3, 16, 2) and l.dtype == torch.float32 and o.device.type == "cuda"
        o = tb.flash_mla_decode_fp8(q, kv, lens, softmax_scale=0.1352)
        assert o.shape == (3, 16, 2, 512) and o.dtype == torch.bfloat16
        o, lse = tb.flash_mla_decode_fp8(q.half(), pool, lens.long(), softmax_scale=0.1352, kv_scale=scale, block_table=table, causal=False, return_lse=True,
                                         pieces=7)
        assert o.shape == (3, 16, 2, 512) and o.dtype == torch.float16 and lse.shape == (3, 16, 2) and lse.dtype == torch.float32
        wide = torch.empty((3, 1024, 640), dtype=E4M3, device="cuda")[:, :, :576]             # a view is taken as it is
        assert tb.flash_mla_decode_fp8(q, wide, lens, softmax_scale=1.0).shape == (3, 16, 2, 512)
        # the append returns nothing, for e4m3 and 16-bit caches, contiguous and paged, fused rows of 576 as two views
        assert torch.ops.mfa.mla_cache_append(latent, rope, kv, lens, None, scale) is None
        assert tb.mla_cache_append(latent, rope, kv, lens, kv_scale=scale) is None
        assert tb.mla_cache_append(latent, rope, pool, lens.long(), block_table=table) is None
        assert tb.mla_cache_append(latent, rope, kv.to(torch.bfloat16), lens) is None
        fused = torch.empty((3, 5, 576), dtype=torch.float16, device="cuda")
        assert tb.mla_cache_append(fused[..., :512], fused[..., 512:], pool.to(torch.float16), lens, block_table=table) is None


def test_the_decode_refusals_in_words():
    with FakeTensorMode():
        q, kv, pool, lens, table, scale, _latent, _rope = operands()
        f = tb.flash_mla_decode_fp8
        for call, kind, needle in (
                (lambda: f(q.cpu(), kv, lens, softmax_scale=0.1), RuntimeError, "tensors must live on the GPU"),
                (lambda: f(q, kv.cpu(), lens, softmax_scale=0.1), RuntimeError, "tensors must live on the GPU"),
                (lambda: f(q, pool, lens, softmax_scale=0.1, block_table=table.cpu()), RuntimeError, "tensors must live on the GPU"),
                (lambda: f(q.clone().requires_grad_(), kv, lens, softmax_scale=0.1), RuntimeError, "forward only (no autograd)"),
                (lambda: f(q, kv.to(torch.bfloat16), lens, softmax_scale=0.1), TypeError, "the latent cache must be torch.float8_e4m3fn"),
                (lambda: f(q, kv.to(torch.float8_e5m2), lens, softmax_scale=0.1), TypeError, "e5m2 and fnuz caches have no kernel"),
                (lambda: f(q.float(), kv, lens, softmax_scale=0.1), TypeError, "q must be bfloat16 or float16"),
                (lambda: f(q[..., :512], kv, lens, softmax_scale=0.1), ValueError, "expected q [B, H, R, 576] and kv_cache [B, C, 576]"),
                (lambda: f(q, kv[:2], lens, softmax_scale=0.1), ValueError, "expected q [B, H, R, 576] and kv_cache [B, C, 576]"),
                (lambda: f(q, kv.transpose(1, 2).contiguous().transpose(1, 2), lens, softmax_scale=0.1), ValueError, "contiguous last dimension"),
                (lambda: f(q, kv, lens.float(), softmax_scale=0.1), ValueError, "cache_lengths must be a GPU tensor"),
                (lambda: f(q, pool, lens, softmax_scale=0.1, block_table=table.long()), ValueError, "block_table must be an int32 GPU tensor"),
                (lambda: f(q, kv, lens, softmax_scale=0.0), ValueError, "softmax_scale must be a finite number > 0"),
                (lambda: f(q, kv, lens, softmax_scale=0.1, pieces=65), ValueError, "pieces must be an int from 0 to 64"),
                (lambda: f(q, kv, lens, softmax_scale=0.1, kv_scale=scale.cpu()), RuntimeError, "kv_scale must live on the GPU of the cache"),
                (lambda: f(q, kv, lens, softmax_scale=0.1, kv_scale=scale.half()), ValueError, "kv_scale must be float32 [1]"),
                (lambda: f(q, kv, lens, softmax_scale=0.1, kv_scale=torch.empty((3,), dtype=torch.float32, device="cuda")), ValueError,
                 "kv_scale must be float32 [1], one scale for the whole cache row")):
            with pytest.raises(kind) as said:
                call()
            assert needle in str(said.value) and str(said.value).startswith("flash_mla_decode_fp8"), str(said.value)
        # the 16-bit function still refuses an e4m3 cache, in the words it had, and now says where to go
        with pytest.raises(TypeError) as said:
            tb.flash_mla_decode(q, kv, lens, softmax_scale=0.1)
        assert str(said.value).startswith("flash_mla_decode:") and "e4m3 latent caches have no kernel" in str(said.value) and "flash_mla_decode_fp8" in str(said.value)


def test_the_append_refusals_in_words():
    with FakeTensorMode():
        _q, kv, pool, lens, table, scale, latent, rope = operands()
        f = tb.mla_cache_append
        kv16 = kv.to(torch.bfloat16)
        for call, kind, needle in (
                (lambda: f(latent.cpu(), rope, kv, lens), RuntimeError, "tensors must live on the GPU"),
                (lambda: f(latent, rope, kv.cpu(), lens), RuntimeError, "tensors must live on the GPU"),
                (lambda: f(latent, rope, kv, lens.cpu()), RuntimeError, "tensors must live on the GPU"),
                (lambda: f(latent, rope, pool, lens, block_table=table.cpu()), RuntimeError, "tensors must live on the GPU"),
                (lambda: f(latent.clone().requires_grad_(), rope, kv, lens), RuntimeError, "writes in place and has no autograd"),
                (lambda: f(latent.float(), rope.float(), kv, lens), TypeError, "latent_new and rope_new must share one of bfloat16 / float16"),
                (lambda: f(latent, rope.half(), kv, lens), TypeError, "latent_new and rope_new must share one of bfloat16 / float16"),
                (lambda: f(latent, rope, kv.to(torch.float16), lens), TypeError, "the latent cache must be the rows' 16-bit type or torch.float8_e4m3fn"),
                (lambda: f(latent, rope, kv.to(torch.float8_e5m2), lens), TypeError, "e5m2 and fnuz caches have no kernel"),
                (lambda: f(latent[..., :256], rope, kv, lens), ValueError, "expected latent_new [B, R, 512], rope_new [B, R, 64] and kv_cache [B, C, 576]"),
                (lambda: f(latent, rope[..., :32], kv, lens), ValueError, "expected latent_new [B, R, 512], rope_new [B, R, 64]"),
                (lambda: f(latent, rope[:, :4], kv, lens), ValueError, "expected latent_new [B, R, 512], rope_new [B, R, 64]"),
                (lambda: f(latent, rope, kv[..., :512], lens), ValueError, "kv_cache [B, C, 576]"),
                (lambda: f(latent, rope, kv[:2], lens), ValueError, "kv_cache [B, C, 576]"),
                (lambda: f(latent, rope, kv.transpose(1, 2).contiguous().transpose(1, 2), lens), ValueError, "contiguous last dimension (a cache is written where it lies)"),
                (lambda: f(latent, rope, kv, lens[:2]), ValueError, "cache_lengths must be a GPU tensor"),
                (lambda: f(latent, rope, pool, lens, block_table=table.long()), ValueError, "block_table must be an int32 GPU tensor"),
                (lambda: f(latent, rope, pool, lens, block_table=table[:2]), ValueError, "block_table must be an int32 GPU tensor"),
                (lambda: f(latent, rope, kv16, lens, kv_scale=scale), ValueError, "kv_scale goes with a float8_e4m3fn cache; a 16-bit cache takes the rows' bits"),
                (lambda: f(latent, rope, kv, lens, kv_scale=scale.double()), ValueError, "kv_scale must be float32 [1]")):
            with pytest.raises(kind) as said:
                call()
            assert needle in str(said.value) and str(said.value).startswith("mla_cache_append"), str(said.value)
