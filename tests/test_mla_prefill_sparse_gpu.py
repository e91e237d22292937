"""GPU test: sparse MLA prefill (include/mfa_mla_prefill_sparse.h) through the C ABI and through torch.  One batch -- lengths
(70, 33, 9) in a column of 96, rows' capacity 37 with q_lengths (37, 5, 0), lists of 45 slots (a partial last step) -- held per element
to the float64 model of tests/mla_sparse_model.py, run per sequence on its first qn rows (its rule with R = qn is this launch's), at
that module's bounds and MARGIN.  Every list carries -1, -7, n - 1, n, the row's frontier, the key after it and one repeat.  Every cache
row no list makes visible, Q at or past qn and the pages nobody names are NaN (tests/cache_kit.py's poison); the lists of rows at or
past qn, and the allocation around the lists, name a row of NaN; O and L lie in sentinel-filled allocations.  Beside the bounds,
identities BIT FOR BIT: 32 full rows are the sparse decode launch, and the list 0 .. column - 1 is the dense prefill launch."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402
import mla_sparse_model as sm  # noqa: E402
from metal_flash_attention_amd import AttentionMLAPrefill, AttentionMLAPrefillSparse, AttentionMLASparseDecode, GEMMOperandPrecision as P  # noqa: E402

pytestmark = pytest.mark.gpu

LENS, C, TOPK, B = (70, 33, 9), 96, 45, 3
FMTS, PAGES = ("bf16", "f16"), (None, 16)
DTYPE, PREC = {"bf16": torch.bfloat16, "f16": torch.float16}, {"bf16": P.BF16, "f16": P.FP16}
OPS = {"sparse prefill": AttentionMLAPrefillSparse, "sparse decode": AttentionMLASparseDecode, "dense prefill": AttentionMLAPrefill}
BELOW = np.stack([np.arange(C) < n for n in LENS])                        # [B][C]: the keys below each length


@functools.lru_cache(maxsize=None)
def drawn(fmt, H, R, qlens):
    """(q64, kv64, idx) of a shape, computed once and shared: distinct random positions of [0, C), then the rule's seams and one repeat"""
    rng = np.random.default_rng(31 * H + R)
    q64 = sm.round_to(rng.uniform(-1.0, 1.0, (B, H, R, sm.DK)), fmt)
    idx = np.full((B, R, TOPK), C - 1, dtype=np.int64)                    # rows at or past qn: a list nobody may read, of a row of NaN
    for b, (n, qn) in enumerate(zip(LENS, qlens)):
        for r in range(qn):
            fr = r + max(n - qn, 0)
            row = rng.permutation(C)[:TOPK]
            row[:7] = [-1, -7, n - 1, n, fr, fr + 1, row[9]]
            idx[b, r] = rng.permutation(row)
    idx[1, 1] = sm.HOLE                                                   # a live row without a visible slot
    return q64, sm.mm.cache_values(fmt, 0, B, C), idx


def kept(idx, qlens):   # [B][C]: the cache rows some list of a live row makes visible, by the rule with R = qn
    return np.concatenate([sm.keep_mask(idx[b:b + 1, :qn], True, qn, (n,), C) for b, (n, qn) in enumerate(zip(LENS, qlens))])


def cache_of(fmt, page, kv64, keep):
    """the cache on the device, NaN in every row keep [B][C] does not name (paged: a shuffled pool, NaN pages), and the layout's keywords"""
    kv = torch.from_numpy(kv64).to(DTYPE[fmt])[:, None]
    if not page:
        return ck.poisoned(kv, keep)[:, 0].contiguous().cuda(), {}
    pool, _same, table = ck.pool_host(kv, kv, page, keep, seed=page)
    return pool[:, 0].contiguous().cuda(), dict(pageSize=page, blockTable=ck.dev(table), blockTableStride=table.shape[1])


def lists_on_device(idx):
    """the lists as a view of a wider allocation whose every other entry names key C - 1, a row of NaN, and their launch keywords"""
    buf = torch.full((B, idx.shape[1] + 1, idx.shape[2] + 24), C - 1, dtype=torch.int32)
    buf[:, :idx.shape[1], :idx.shape[2]] = torch.from_numpy(idx.astype(np.int32))
    view = buf.cuda()[:, :idx.shape[1], :idx.shape[2]]
    return view, dict(indices=view, topk=idx.shape[2], indexStrides=(int(view.stride(1)), int(view.stride(0))))


def launch(kind, fmt, H, qlens, q64, cache, cache_kw, idx):
    """one launch of OPS[kind] on sentinel-filled O and L inside larger allocations, Q NaN at or past qn -> (O, L base 2) on the host"""
    R = q64.shape[2]
    q = torch.from_numpy(q64).to(DTYPE[fmt])
    for b, qn in enumerate(qlens):
        q[b, :, qn:] = float("nan")
    obuf = torch.full((B, H + 1, R + 2, sm.DV + 8), ck.SENT_O, dtype=DTYPE[fmt], device="cuda")
    lbuf = torch.full((B, H + 1, R + 1), ck.SENT_L, dtype=torch.float32, device="cuda")
    o, l = obuf[:, :H, :R, :sm.DV], lbuf[:, :H, :R]
    kw = dict(rows=R, column=C, heads=H, batches=B, scale=sm.SCALE, cacheLengths=ck.lengths(LENS), lStrides=(int(l.stride(1)), int(l.stride(0))),
              strides=dict(O=(int(o.stride(2)), int(o.stride(1)), int(o.stride(0)))), **cache_kw)
    kw.update(dict(pieces=1) if kind == "sparse decode" else dict(queryLengths=ck.lengths(qlens)))       # (decode: unsplit, every row live)
    kw.update({} if kind == "dense prefill" else lists_on_device(idx)[1])
    OPS[kind](PREC[fmt]).dispatch(q.cuda(), cache, o, l, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    own = torch.zeros_like(obuf, dtype=torch.bool)
    for b, qn in enumerate(qlens):
        own[b, :H, :qn, :sm.DV] = True
    assert bool((obuf[~own].float() == ck.SENT_O).all()), "the launch wrote outside O's live rows"
    assert bool((lbuf[~own[..., 0][:, :, :R + 1]] == ck.SENT_L).all()), "the launch wrote outside L's live rows"
    return o.cpu(), l.cpu()


@pytest.mark.parametrize("H", [40, 16])
@pytest.mark.parametrize("page", PAGES)
@pytest.mark.parametrize("fmt", FMTS)
def test_a_launch_lies_inside_the_float64_model_s_bounds(fmt, page, H):
    qlens = (37, 5, 0)
    q64, kv64, idx = drawn(fmt, H, 37, qlens)
    o, l = launch("sparse prefill", fmt, H, qlens, q64, *cache_of(fmt, page, kv64, kept(idx, qlens)), idx)
    for b, (n, qn) in enumerate(zip(LENS[:2], qlens)):                    # (sequence 2 has no live row: `launch` has held its sentinels)
        ob, lb = o[b:b + 1, :, :qn], l[b:b + 1, :, :qn]
        assert bool(torch.isfinite(ob.float()).all()) and bool(torch.isfinite(lb).all()), "poison reached a result"
        ref = sm.model(q64[b:b + 1, :, :qn], kv64[b:b + 1], (n,), idx[b:b + 1, :qn], True, sm.SCALE)
        blind = torch.from_numpy(~np.isfinite(ref.L))
        assert bool(blind.any()) == (b == 1) and not ob[blind].float().any() and bool((lb[blind] == -ck.FLT_MAX).all()), "a row without a visible slot"
        wo, wl, text = sm.compare(ob, lb / ck.LOG2E, ref, fmt, fmt, (n,), margin=1)
        print("%s page %s H %d sequence %d: worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % (fmt, page, H, b, wo, wl))
        assert wo <= sm.MARGIN and wl <= sm.MARGIN, text


@pytest.mark.parametrize("H", [40, 129])
@pytest.mark.parametrize("page", PAGES)
@pytest.mark.parametrize("fmt", FMTS)
def test_32_full_rows_are_the_sparse_decode_launch_bit_for_bit(fmt, page, H):
    qlens = (32, 32, 32)
    q64, kv64, idx = drawn(fmt, H, 32, qlens)
    args = (fmt, H, qlens, q64, *cache_of(fmt, page, kv64, kept(idx, qlens)), idx)
    assert ck.same(launch("sparse prefill", *args), launch("sparse decode", *args))


@pytest.mark.parametrize("page", PAGES)
@pytest.mark.parametrize("fmt", FMTS)
def test_the_identity_list_is_the_dense_prefill_launch_bit_for_bit(fmt, page):
    qlens = (70, 5, 0)
    q64, kv64, _idx = drawn(fmt, 40, 70, qlens)
    idx = np.broadcast_to(np.arange(C, dtype=np.int64), (B, 70, C)).copy()
    args = (fmt, 40, qlens, q64, *cache_of(fmt, page, kv64, BELOW), idx)      # NaN at and past every length
    dense = launch("dense prefill", *args)
    assert bool(torch.isfinite(dense[0][:2, :, :5].float()).all()) and dense[0][0].float().abs().max() > 0
    assert ck.same(launch("sparse prefill", *args), dense)


def test_flash_mla_sparse_prefill_end_to_end_and_in_a_graph():
    from metal_flash_attention_amd import torch_binding as tb
    qlens_host = (37, 5, 0)
    q64, kv64, idx = drawn("bf16", 40, 37, qlens_host)
    cache, cache_kw = cache_of("bf16", 16, kv64, BELOW)                   # (the replay's other lists and frontiers name other keys)
    want_o, want_l = launch("sparse prefill", "bf16", 40, qlens_host, q64, cache, cache_kw, idx)
    q, lens, qlens = torch.from_numpy(q64).to(torch.bfloat16).cuda(), ck.lengths(LENS), ck.lengths(qlens_host)
    lists = lists_on_device(idx)[0]
    run = lambda ql, li: tb.flash_mla_sparse_prefill(q, cache, lens, li, softmax_scale=sm.SCALE, q_lengths=ql,  # noqa: E731
                                                     block_table=cache_kw["blockTable"], return_lse=True)
    o, lse = run(qlens, lists)
    torch.cuda.synchronize()
    assert o.shape == (3, 40, 37, sm.DV) and o.dtype == q.dtype and lse.shape == (3, 40, 37) and lse.dtype == torch.float32

    def equal(got, want, rows):
        assert all(ck.same((got[0][b, :, :qn], got[1][b, :, :qn]), (want[0][b, :, :qn], want[1][b, :, :qn])) for b, qn in enumerate(rows))
    equal((o.cpu(), lse.cpu()), (want_o, want_l * tb._LN2), qlens_host)   # the C ABI's launch, L in natural units
    # captured once, replayed after q_lengths and the lists change in place (rows 0 .. 3 take the lists of rows 36 .. 33): both are read on the device
    other_q, other_lists = ck.lengths((4, 3, 0)), lists.flip(1).contiguous()
    want = run(other_q, other_lists)
    s_q, s_lists = qlens.clone(), lists.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(s_q, s_lists)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = run(s_q, s_lists)
    for new_q, new_lists, w, rows in ((qlens, lists, (o, lse), qlens_host), (other_q, other_lists, want, (4, 3, 0)), (qlens, lists, (o, lse), qlens_host)):
        got[0].fill_(ck.SENT_O)
        s_q.copy_(new_q)
        s_lists.copy_(new_lists)
        graph.replay()
        torch.cuda.synchronize()
        equal(got, w, rows)
        assert all(bool((got[0][b, :, qn:].float() == ck.SENT_O).all()) for b, qn in enumerate(rows)), "a replay wrote a row at or past qn"
