"""The torch binding of include/mfa_mla_index.h: mla_index_logits, mla_index_select and mla_index_topk reach the ops mfa::mla_index_*,
kept in a list of their own, with fake implementations that give the right shapes and types; what the operands may be is said in words
(CPU: fake tensors, no device).  Marked gpu: operands that are views -- a transposed q_index, sliced weights and logits, an index cache
with padded rows, a block table with a row stride, int64 lengths -- are read where they lie and give the bits of their contiguous
copies, and one mla_index_topk inside torch.cuda.graph, replayed on changed lengths, equals the eager call."""
import inspect

import pytest

torch = pytest.importorskip("torch")

from torch._subclasses.fake_tensor import FakeTensorMode  # noqa: E402

import metal_flash_attention_amd as mfa  # noqa: E402
from metal_flash_attention_amd import torch_binding as tb  # noqa: E402

gpu = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _ops():
    assert hasattr(torch.library, "custom_op") and tb._HAVE_MLA_INDEX_OPS, "the installed torch has no torch.library.custom_op: the index ops are missing"


def operands(R=2, Hi=40, paged=False):
    qi = torch.empty((3, Hi, R, 128), dtype=torch.bfloat16, device="cuda")
    w = torch.empty((3, R, Hi), dtype=torch.float32, device="cuda")
    ki = torch.empty((70, 64, 128) if paged else (3, 1000, 128), dtype=torch.bfloat16, device="cuda")
    lens = torch.empty((3,), dtype=torch.int32, device="cuda")
    table = torch.empty((3, 16), dtype=torch.int32, device="cuda") if paged else None
    return qi, w, ki, lens, table


def test_the_ops_schemas_and_their_list():
    schema = lambda name: str(getattr(torch.ops.mfa, name).default._schema)  # noqa: E731
    assert schema("mla_index_logits") == ("mfa::mla_index_logits(Tensor q_index, Tensor weights, Tensor index_cache, Tensor cache_lengths, "
                                          "Tensor? block_table, bool causal) -> Tensor")
    assert schema("mla_index_select") == "mfa::mla_index_select(Tensor logits, Tensor cache_lengths, SymInt topk, bool causal) -> Tensor"
    assert schema("mla_index_topk") == ("mfa::mla_index_topk(Tensor q_index, Tensor weights, Tensor index_cache, Tensor cache_lengths, SymInt topk, "
                                        "Tensor? block_table, bool causal) -> Tensor")
    assert [op[0] for op in tb._MLA_INDEX_OPS] == ["mla_index_logits", "mla_index_select", "mla_index_topk"]
    assert all(op[3] == () for op in tb._MLA_INDEX_OPS)                      # nothing is mutated
    assert [op[2] for op in tb._MLA_INDEX_OPS] == [tb._fake_mla_index_logits, tb._fake_mla_index_select, tb._fake_mla_index_topk]
    assert mfa.mla_index_logits is tb.mla_index_logits and mfa.mla_index_select is tb.mla_index_select and mfa.mla_index_topk is tb.mla_index_topk


def test_the_signatures():
    for f, names in ((tb.mla_index_logits, ["q_index", "weights", "index_cache", "cache_lengths", "block_table", "causal"]),
                     (tb.mla_index_select, ["logits", "cache_lengths", "topk", "causal"]),
                     (tb.mla_index_topk, ["q_index", "weights", "index_cache", "cache_lengths", "topk", "block_table", "causal"])):
        sig = inspect.signature(f)
        assert list(sig.parameters) == names
        assert sig.parameters["causal"].default is True and sig.parameters["causal"].kind is inspect.Parameter.KEYWORD_ONLY
        assert "block_table" not in names or sig.parameters["block_table"].default is None


@pytest.mark.parametrize("R, topk, paged", [(1, 1, False), (2, 100, True), (4, 2048, False), (32, 5000, True)])
def test_the_fakes_give_the_right_shapes(R, topk, paged):
    with FakeTensorMode():
        qi, w, ki, lens, table = operands(R, paged=paged)
        column = 64 * 16 if paged else 1000
        logits = torch.ops.mfa.mla_index_logits(qi, w, ki, lens, table, True)
        assert logits.shape == (3, R, column) and logits.dtype == torch.float32 and logits.device.type == "cuda"
        lists = torch.ops.mfa.mla_index_select(logits, lens, topk, True)
        assert lists.shape == (3, R, topk) and lists.dtype == torch.int32 and lists.device.type == "cuda"
        both = torch.ops.mfa.mla_index_topk(qi, w, ki, lens, topk, table, False)
        assert both.shape == (3, R, topk) and both.dtype == torch.int32
        # the public functions; fp16, int64 lengths, views
        logits = tb.mla_index_logits(qi.half(), w, ki.half(), lens.long(), block_table=table, causal=False)
        assert logits.shape == (3, R, column) and logits.dtype == torch.float32
        assert tb.mla_index_select(logits[:, :, :500], lens, topk).shape == (3, R, topk)
        wide = torch.empty((3, R, 40, 128), dtype=torch.bfloat16, device="cuda").transpose(1, 2)
        assert tb.mla_index_topk(wide, w, ki, lens, topk, block_table=table).shape == (3, R, topk)


def test_the_refusals_in_words():
    with FakeTensorMode():
        qi, w, ki, lens, _none = operands()
        _q, _w, pool, _l, table = operands(paged=True)
        logits = torch.empty((3, 2, 1000), dtype=torch.float32, device="cuda")
        L, S, T = tb.mla_index_logits, tb.mla_index_select, tb.mla_index_topk
        for call, kind, needle in (
                (lambda: L(qi.cpu(), w, ki, lens), RuntimeError, "tensors must live on one GPU"),
                (lambda: L(qi, w.cpu(), ki, lens), RuntimeError, "tensors must live on one GPU"),
                (lambda: T(qi, w, ki.cpu(), lens, 8), RuntimeError, "tensors must live on one GPU"),
                (lambda: T(qi, w, ki, lens.cpu(), 8), RuntimeError, "tensors must live on one GPU"),
                (lambda: S(logits.cpu(), lens, 8), RuntimeError, "tensors must live on one GPU"),
                (lambda: L(qi, w, pool, lens, block_table=table.cpu()), RuntimeError, "tensors must live on one GPU"),
                (lambda: L(qi.half(), w, ki, lens), TypeError, "q_index and the index cache must share one of bfloat16 / float16"),
                (lambda: L(qi.float(), w, ki.float(), lens), TypeError, "q_index and the index cache must share one of bfloat16 / float16"),
                (lambda: T(qi, w, ki.to(torch.float8_e4m3fn), lens, 8), TypeError, "e4m3 index caches have no kernel"),
                (lambda: L(qi[..., :64], w, ki, lens), ValueError, "expected q_index [B, Hi, R, 128] and index_cache [B, C, 128]"),
                (lambda: L(qi, w, ki[..., :64], lens), ValueError, "expected q_index [B, Hi, R, 128] and index_cache [B, C, 128]"),
                (lambda: L(qi, w, ki[:2], lens), ValueError, "expected q_index [B, Hi, R, 128] and index_cache [B, C, 128]"),
                (lambda: L(qi[0], w, ki, lens), ValueError, "expected q_index [B, Hi, R, 128] and index_cache [B, C, 128]"),
                (lambda: L(torch.empty((3, 65, 2, 128), dtype=torch.bfloat16, device="cuda"), w, ki, lens), ValueError,
                 "takes 1 .. 64 index heads and 1 .. 32 rows (got Hi = 65, R = 2)"),
                (lambda: T(torch.empty((3, 40, 33, 128), dtype=torch.bfloat16, device="cuda"), w, ki, lens, 8), ValueError,
                 "takes 1 .. 64 index heads and 1 .. 32 rows (got Hi = 40, R = 33)"),
                (lambda: L(qi, w, torch.empty((3, 1000, 256), dtype=torch.bfloat16, device="cuda")[:, :, ::2], lens), ValueError,
                 "index_cache must have a contiguous last dimension"),
                (lambda: L(qi, w.transpose(1, 2), ki, lens), ValueError, "weights must be float32 [B, R, Hi] = [3, 2, 40]"),
                (lambda: L(qi, w[:, :, :39], ki, lens), ValueError, "weights must be float32 [B, R, Hi] = [3, 2, 40]"),
                (lambda: T(qi, w.double(), ki, lens, 8), ValueError, "weights must be float32 [B, R, Hi] = [3, 2, 40]"),
                (lambda: L(qi, w, pool, lens, block_table=table.long()), ValueError, "block_table must be an int32 GPU tensor [B, pages per sequence] = [3, n]"),
                (lambda: L(qi, w, pool, lens, block_table=table[:2]), ValueError, "block_table must be an int32 GPU tensor [B, pages per sequence] = [3, n]"),
                (lambda: L(qi, w, pool, lens, block_table=table[:, ::2]), ValueError, "block_table must be an int32 GPU tensor [B, pages per sequence] = [3, n]"),
                (lambda: L(qi, w, ki, lens[:2]), ValueError, "cache_lengths must be a GPU tensor [B] = [3] int32 or int64"),
                (lambda: S(logits, lens.float(), 8), ValueError, "cache_lengths must be a GPU tensor [B] = [3] int32 or int64"),
                (lambda: S(logits.double(), lens, 8), ValueError, "logits must be float32 [B, R, C] with R <= 32"),
                (lambda: S(logits[0], lens, 8), ValueError, "logits must be float32 [B, R, C] with R <= 32"),
                (lambda: S(torch.empty((3, 33, 100), dtype=torch.float32, device="cuda"), lens, 8), ValueError, "logits must be float32 [B, R, C] with R <= 32"),
                (lambda: S(logits, lens, 0), ValueError, "topk must be an int >= 1"),
                (lambda: S(logits, lens, 8.0), ValueError, "topk must be an int >= 1"),
                (lambda: S(logits, lens, True), ValueError, "topk must be an int >= 1"),
                (lambda: T(qi, w, ki, lens, "8"), ValueError, "topk must be an int >= 1")):
            with pytest.raises(kind) as said:
                call()
            assert needle in str(said.value) and str(said.value).startswith("mla_index_"), str(said.value)


def problem(paged):
    B, Hi, R, C, page = 3, 33, 2, 200, 16
    g = torch.Generator().manual_seed(41)
    lens = torch.tensor([200, 37, 129], dtype=torch.int32)
    qi = torch.randn((B, R, Hi, 128), generator=g).bfloat16().cuda().transpose(1, 2)            # [B, Hi, R, 128] over a [B, R, Hi, 128] buffer
    w = torch.full((B, R + 1, Hi + 3), float("nan"))
    w[:, :R, :Hi] = torch.randn((B, R, Hi), generator=g)
    w = w.cuda()[:, :R, :Hi]
    k = torch.randn((B, C, 128), generator=g).bfloat16()
    for b, n in enumerate(lens.tolist()):
        k[b, n:] = float("nan")
    table = None
    if not paged:
        buf = torch.full((B, C, 136), float("nan"), dtype=torch.bfloat16)
        buf[:, :, :128] = k
        ki = buf.cuda()[:, :, :128]
    else:
        pps = -(-C // page)
        order = torch.randperm(B * pps, generator=g).reshape(B, pps)
        buf = torch.full((B * pps + 1, page, 136), float("nan"), dtype=torch.bfloat16)
        wide = torch.full((B, pps + 3), B * pps, dtype=torch.int32)
        for b in range(B):
            for i in range(pps):
                rows = k[b, i * page:(i + 1) * page]
                buf[order[b, i], :len(rows), :128] = rows
                wide[b, i] = order[b, i]
        ki, table = buf.cuda()[:, :, :128], wide.cuda()[:, :pps]
        assert not table.is_contiguous()
    assert not qi.is_contiguous() and not w.is_contiguous() and not ki.is_contiguous()
    return qi, w, ki, lens.cuda(), table


@gpu
@pytest.mark.parametrize("paged", [False, True])
def test_views_give_the_bits_of_their_contiguous_copies(paged):
    qi, w, ki, lens, table = problem(paged)
    flat = dict(block_table=None if table is None else table.contiguous())
    there = dict(block_table=table)
    want = tb.mla_index_logits(qi.contiguous(), w.contiguous(), ki.contiguous(), lens, **flat)
    assert torch.isfinite(want[0, -1, :200]).all() and (want[1, :, 37:] == float("-inf")).all()
    for got in (tb.mla_index_logits(qi, w, ki, lens, **there), tb.mla_index_logits(qi, w.contiguous(), ki.contiguous(), lens.long(), **flat),
                tb.mla_index_logits(qi.contiguous(), w, ki.contiguous(), lens, **flat), tb.mla_index_logits(qi.contiguous(), w.contiguous(), ki, lens, **there)):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    wide = torch.full((3, 2, want.shape[2] + 8), float("nan"), device="cuda")
    wide[:, :, :want.shape[2]] = want
    for topk in (5, 64):
        lists = tb.mla_index_select(want, lens, topk)
        assert torch.equal(tb.mla_index_select(wide[:, :, :want.shape[2]], lens.long(), topk), lists)
        assert torch.equal(tb.mla_index_topk(qi, w, ki, lens.long(), topk, **there), lists)
        assert torch.equal(tb.mla_index_topk(qi.contiguous(), w.contiguous(), ki.contiguous(), lens, topk, **flat), lists)


@gpu
def test_the_chain_inside_a_captured_graph():
    """one capture of mla_index_topk -- a straight chain: the logits kernel, the select kernel --, replayed twice on changed lengths"""
    qi, w, ki, lens, table = problem(True)
    want = tb.mla_index_topk(qi, w, ki, lens, 33, block_table=table)          # eager (and the warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = tb.mla_index_topk(qi, w, ki, lens, 33, block_table=table)
    for new in (None, [37, 0, 100], [150, 36, 34]):                          # (never past what the cache holds: rows behind a length are NaN)
        if new is not None:
            lens.copy_(torch.tensor(new, dtype=torch.int32))
            want = tb.mla_index_topk(qi, w, ki, lens, 33, block_table=table)
        got.fill_(-9)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, want)
