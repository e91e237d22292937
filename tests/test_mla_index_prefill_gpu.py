"""The prefill indexer (include/mfa_mla_index_prefill.h) on the GPU: the index logits of a chunk per element against float64 under
mla_index_model's bound, the span seam, the selection exactly on the kernel's own logits, the chain over passes and the hand-over to the
sparse prefill bit for bit, one graph for changed lengths, and the agreement with the decode indexer at rows <= 32.  Everything the rule
does not own is poisoned: keys at or past a length and unnamed pages hold NaN and +-2^14 (ReLU turns a NaN score into 0), QI of dead rows
+-2^14, W of dead rows and W's padding NaN; the logits lie in a wider allocation of sentinels."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import metal_flash_attention_amd as mfa  # noqa: E402
from metal_flash_attention_amd import AttentionMLAIndexPrefill, GEMMOperandPrecision as P  # noqa: E402
from mla_index_model import BIG, SENTINEL, reference, select_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPE, PREC = {"bf16": torch.bfloat16, "f16": torch.float16}, {"bf16": P.BF16, "f16": P.FP16}
DI, PAGE, PAD = 128, 16, 8
# name -> (R, C, cacheLengths, queryLengths): full; the frontier starts inside tile 1 and rows 37 .. are dead; qn > n; empty; clamped
SHAPES = {"chunk": (70, 600, (600, 300, 40, 0, 700), (70, 37, 70, 0, 70)), "small": (3, 70, (70, 30, 2, 0, 90), (3, 2, 3, 0, 3)),
          "spans": (300, 300, (300,), None)}
FORMATS, LAYOUTS = ("bf16", "f16"), ("contiguous", "paged")


def frontier(lens, qlens, R, C, causal):
    """v [B, R] of the header's rule: 0 for a row at or past qn"""
    n = np.minimum(np.asarray(lens, dtype=np.int64), C)[:, None]
    qn = np.minimum(np.asarray(qlens if qlens is not None else [R] * len(lens), dtype=np.int64), R)[:, None]
    r = np.arange(R)[None, :]
    return np.where(r < qn, np.minimum(n, r + np.maximum(n - qn, 0) + 1) if causal else n, 0)


@functools.lru_cache(maxsize=None)
def problem(fmt, H, shape):
    """q, w, k as tensors of the 16-bit type (w FP32), with the float64 logits and their bound: once per (fmt, H, shape)"""
    R, C, lens, _ql = SHAPES[shape]
    g = torch.Generator().manual_seed(100 * H + R)
    q, k = (torch.randn(s, generator=g).to(DTYPE[fmt]) for s in ((len(lens), H, R, DI), (len(lens), C, DI)))
    w = torch.randn((len(lens), R, H), generator=g)
    return (q, w, k) + reference(q.double().numpy(), w.double().numpy(), k.double().numpy())


def poison(shape, dtype):
    """NaN and +-2^14 in turns"""
    x = torch.full(shape, BIG, dtype=torch.float32)
    x.view(-1)[1::2] = -BIG
    x.view(-1)[::3] = float("nan")
    return x.to(dtype)


@functools.lru_cache(maxsize=None)
def operands(fmt, H, shape, layout):
    """the operands on the device, poisoned, and the launch's keywords; `strided`: QI viewed from [B, R, H, Di], W's rows of H + 3, KI's of Di + 8"""
    q, w, k = (t.clone() for t in problem(fmt, H, shape)[:3])
    R, C, lens, ql = SHAPES[shape]
    B = len(lens)
    for b in range(B):
        k[b, min(lens[b], C):] = poison((C - min(lens[b], C), DI), k.dtype)
        if ql is not None:
            q[b, :, ql[b]:] = poison((H, R - ql[b], DI), q.dtype)
            w[b, ql[b]:] = float("nan")
    kw = dict(rows=R, column=C, indexHeads=H, batches=B, cacheLengths=torch.tensor(lens, dtype=torch.int32).cuda(),
              queryLengths=None if ql is None else torch.tensor(ql, dtype=torch.int32).cuda())
    if layout == "strided":
        wide = torch.full((B, R + 1, H + 3), float("nan"))
        wide[:, :R, :H] = w
        rows = poison((B, C, DI + 8), k.dtype)
        rows[:, :, :DI] = k
        kw.update(strides=dict(QI=(H * DI, DI, R * H * DI), KI=(DI + 8, 0, C * (DI + 8))), weightStrides=(H + 3, (R + 1) * (H + 3)))
        return q.transpose(1, 2).contiguous().cuda(), wide.cuda(), rows.cuda(), kw
    if layout == "paged":
        pps = -(-C // PAGE)
        order = np.random.default_rng(5).permutation(B * pps).reshape(B, pps)
        pool = poison((B * pps + 2, PAGE, DI), k.dtype)                       # (the rest of a last page and the two unnamed pages: poison)
        table = np.empty((B, pps + 2), dtype=np.int32)
        table[:] = B * pps + (np.arange(pps + 2) & 1)[None, :]                # pages without a valid key and entries past the last
        for b in range(B):
            for i in range(-(-min(lens[b], C) // PAGE)):
                rows = k[b, i * PAGE:(i + 1) * PAGE]
                pool[int(order[b, i]), :len(rows)] = rows
                table[b, i] = order[b, i]
        kw.update(pageSize=PAGE, blockTable=torch.from_numpy(table).cuda(), blockTableStride=pps + 2)
        k = pool
    return q.cuda(), w.cuda(), k.cuda(), kw


@functools.lru_cache(maxsize=None)
def logits_of(fmt, H, shape, layout, causal):
    """the logits launch into an allocation [B + 1][R + 1][C + PAD] of sentinels -> (the allocation on the device, downloaded)"""
    q, w, k, kw = operands(fmt, H, shape, layout)
    R, C = SHAPES[shape][:2]
    out = torch.full((kw["batches"] + 1, R + 1, C + PAD), SENTINEL, dtype=torch.float32, device="cuda")
    AttentionMLAIndexPrefill(PREC[fmt]).dispatch(q, w, k, out, stage="logits", causal=causal, logitStrides=(C + PAD, (R + 1) * (C + PAD)), **kw)
    return out, out.cpu().numpy()


def check_logits(fmt, H, shape, layout, causal):
    R, C, lens, ql = SHAPES[shape]
    ref, bound = problem(fmt, H, shape)[3:]
    got, v = logits_of(fmt, H, shape, layout, causal)[1], frontier(lens, ql, R, C, causal)
    seen = np.arange(C + PAD)[None, None, :] < np.pad(v, ((0, 1), (0, 1)))[:, :, None]
    assert np.array_equal(got[~seen].view(np.uint32), np.full(int((~seen).sum()), SENTINEL, dtype=np.float32).view(np.uint32))
    inside = seen[:len(lens), :R, :C]
    ratio = np.abs(got[:len(lens), :R, :C].astype(np.float64) - ref)[inside] / bound[inside]
    print("largest error / bound:", float(ratio.max()))
    assert not np.isnan(ratio).any() and (ratio <= 1.0).all()


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("H,shape", [(64, "chunk"), (33, "chunk"), (1, "small")])
@pytest.mark.parametrize("layout", LAYOUTS + ("strided",))
@pytest.mark.parametrize("fmt", FORMATS)
def test_logits_per_element_and_nothing_else_written(fmt, layout, H, shape, causal):
    """|logit - float64| <= 2 x 161 x 2^-24 x sum_h |W_h| sum_d |q_hd k_cd| (the chain is the decode indexer's: DESIGN.md 4.32)"""
    check_logits(fmt, H, shape, layout, causal)


def test_more_than_one_span_of_rows():
    """10 spans of 32 rows over 2 tiles: the span seam, the causal start inside a span and the ring's wrap-around"""
    kw = operands("bf16", 64, "spans", "contiguous")[3]
    assert "2 tiles of 256 keys x 10 spans of 32 rows x 1 sequences" in AttentionMLAIndexPrefill(P.BF16).launchForm(stage="logits", **kw)
    check_logits("bf16", 64, "spans", "contiguous", True)


def wanted_lists(x, v, topk):
    return np.stack([np.stack([select_ref(x[b, r], int(v[b, r]), topk) for r in range(v.shape[1])]) for b in range(v.shape[0])])


@pytest.mark.parametrize("topk", [33, 700])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_selection_exactly_the_chain_and_the_hand_over(fmt, layout, topk):
    R, C, lens, ql = SHAPES["chunk"]
    q, w, k, kw = operands(fmt, 64, "chunk", layout)
    B, index = len(lens), AttentionMLAIndexPrefill(PREC[fmt])
    alloc, x = logits_of(fmt, 64, "chunk", layout, True)
    want = wanted_lists(x, frontier(lens, ql, R, C, True), topk)
    assert (want[1, 37:] == -1).all()                                         # dead rows: all holes
    kw = dict(kw, topk=topk)
    lists = torch.full((B, R, topk), -7, dtype=torch.int32, device="cuda")
    index.dispatch(alloc, lists, stage="select", logitStrides=(C + PAD, (R + 1) * (C + PAD)), **kw)
    assert np.array_equal(lists.cpu().numpy(), want)
    # ---- the chain at the recommended workspace and at one of 32 rows: passes of 32, 32 and 6 rows
    for nbytes, passes in ((index.workspaceSize(**kw), "1 passes of 70 rows"), (32 * B * C * 4, "3 passes of 32 rows")):
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        assert index.launchForm(workspace=ws, **kw).endswith(passes)
        chained = torch.full((B, R, topk), -7, dtype=torch.int32, device="cuda")
        index.dispatch(q, w, k, chained, workspace=ws, **kw)
        assert torch.equal(chained, lists)
    # ---- the hand-over: the sparse prefill over the chained lists is the one over the reference's, and with topk >= column the dense one
    g = torch.Generator().manual_seed(3)
    qa, kv = (torch.randn(s, generator=g).to(DTYPE[fmt]).cuda() for s in ((B, 11, R, 576), (B, C, 576)))
    lens_d, ql_d = kw["cacheLengths"], kw["queryLengths"]
    o, l = mfa.flash_mla_sparse_prefill(qa, kv, lens_d, chained, softmax_scale=0.1, q_lengths=ql_d, return_lse=True)
    o2, l2 = mfa.flash_mla_sparse_prefill(qa, kv, lens_d, torch.from_numpy(want).cuda(), softmax_scale=0.1, q_lengths=ql_d, return_lse=True)
    live = torch.from_numpy(np.arange(R)[None, :] < np.minimum(ql, R)[:, None]).cuda()[:, None, :].expand(B, 11, R)
    assert torch.equal(o[live], o2[live]) and torch.equal(l[live], l2[live])
    if topk >= C:
        od, ld = mfa.flash_mla_prefill(qa, kv, lens_d, softmax_scale=0.1, q_lengths=ql_d, return_lse=True)
        assert torch.equal(o[live], od[live]) and torch.equal(l[live], ld[live])


def test_one_graph_serves_changed_lengths():
    R, C, lens, ql = SHAPES["chunk"]
    q, w, k = (t.cuda() for t in problem("bf16", 64, "chunk")[:3])            # (the lengths move: no poison behind them)
    lens_d, ql_d = (torch.tensor(x, dtype=torch.int32).cuda() for x in (lens, ql))
    run = lambda: mfa.mla_index_prefill_topk(q, w, k, lens_d, 33, q_lengths=ql_d)   # noqa: E731
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for new_lens, new_ql in ((lens, ql), ((333, 600, 70, 257, 1), (70, 70, 5, 69, 70))):
        lens_d.copy_(torch.tensor(new_lens, dtype=torch.int32))
        ql_d.copy_(torch.tensor(new_ql, dtype=torch.int32))
        eager = run()
        for _ in range(2):
            captured.fill_(-7)
            graph.replay()
            assert torch.equal(captured, eager)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_agreement_with_the_decode_indexer_at_32_rows(fmt, layout):
    """rows <= 32 and no queryLengths: the two rules coincide"""
    R, C, lens, _ql = SHAPES["chunk"]
    k, kw = operands(fmt, 64, "chunk", layout)[2:]
    q, w = problem(fmt, 64, "chunk")[0][:, :, :32].cuda(), problem(fmt, 64, "chunk")[1][:, :32].cuda()
    lens_d, table = kw["cacheLengths"].clamp(max=C), kw.get("blockTable")     # (the torch functions take a table's whole width for the column)
    new = mfa.mla_index_prefill_logits(q, w, k, lens_d, block_table=table)
    v = frontier(lens, None, 32, C, True)
    assert np.array_equal(mfa.mla_index_prefill_topk(q, w, k, lens_d, 33, block_table=table).cpu().numpy(), wanted_lists(new.cpu().numpy(), v, 33))
    old = mfa.mla_index_logits(q, w, k, lens_d, block_table=table)
    assert torch.equal(mfa.mla_index_prefill_select(old, lens_d, 33), mfa.mla_index_select(old, lens_d, 33))
    assert torch.equal(torch.isinf(new), torch.isinf(old))                    # the same positions written
