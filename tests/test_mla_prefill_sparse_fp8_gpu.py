"""GPU test: sparse MLA prefill over an e4m3 latent cache (include/mfa_mla_prefill_sparse_fp8.h): the batch, lists and queries of
tests/test_mla_prefill_sparse_gpu.py over the bytes of mla_fp8_model.cache_bytes, held per element to the float64 model of
tests/mla_sparse_fp8_model.py per sequence on its first qn rows (its rule with R = qn is this launch's) at that module's MARGIN, under
the poison of tests/test_mla_sparse_fp8_gpu.py (NaN bytes in every row no live list shows and every unnamed page, NaN in Q at and past
qn, kvScale in front of SCALE_TAIL, sentinels around O and L); and BIT FOR BIT against the e4m3 sparse decode and dense prefill launches."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402
import mla_fp8_model as fm  # noqa: E402
import mla_sparse_fp8_model as xm  # noqa: E402
import test_mla_prefill_sparse_gpu as t16  # noqa: E402  (its batch: lengths, q_lengths, lists and queries)
import test_mla_sparse_fp8_gpu as x8  # noqa: E402  (its byte caches, lists and kvScale on the device)
from metal_flash_attention_amd import AttentionMLAPrefillFP8, AttentionMLAPrefillSparseFP8, AttentionMLASparseDecodeFP8  # noqa: E402

pytestmark = pytest.mark.gpu

LENS, C, B, FMTS, PAGES, BELOW, kept = t16.LENS, t16.C, t16.B, t16.FMTS, t16.PAGES, t16.BELOW, t16.kept
OPS = {"sparse prefill": AttentionMLAPrefillSparseFP8, "sparse decode": AttentionMLASparseDecodeFP8, "dense prefill": AttentionMLAPrefillFP8}


def drawn(fmt, H, R, qlens):   # the 16-bit test's queries and lists of the shape, over a byte cache
    q64, _kv64, idx = t16.drawn(fmt, H, R, qlens)
    return q64, fm.cache_bytes(0, B, C), idx


def cache_of(page, kvb, keep):   # bytes on the device, the NaN bytes in every row keep [B][C] does not name and in unnamed pages
    return x8.cache_of(dict(layout="packed", page=page, lens=LENS, C=C, lists=""), kvb, keep)


def launch(kind, fmt, H, qlens, kvscale, q64, cache, cache_kw, idx):
    """one launch of OPS[kind] on sentinel-filled O and L inside larger allocations, Q NaN at or past qn -> (O, L base 2) on the host"""
    R = q64.shape[2]
    q = x8.tensor(q64, fmt)
    for b, qn in enumerate(qlens):
        q[b, :, qn:] = float("nan")
    obuf = torch.full((B, H + 1, R + 2, xm.DV + 8), ck.SENT_O, dtype=x8.DTYPE[fmt], device="cuda")
    lbuf = torch.full((B, H + 1, R + 1), ck.SENT_L, dtype=torch.float32, device="cuda")
    o, l = obuf[:, :H, :R, :xm.DV], lbuf[:, :H, :R]
    kw = dict(rows=R, column=C, heads=H, batches=B, scale=xm.SCALE, causal=True, cacheLengths=ck.lengths(LENS), lStrides=(int(l.stride(1)), int(l.stride(0))),
              kvScale=x8.scale_of(kvscale), **cache_kw)
    kw["strides"] = dict(kw.get("strides", {}), O=(int(o.stride(2)), int(o.stride(1)), int(o.stride(0))))
    kw.update(dict(pieces=1) if kind == "sparse decode" else dict(queryLengths=ck.lengths(qlens)))       # (decode: unsplit, every row live)
    kw.update({} if kind == "dense prefill" else x8.lists_on_device(idx, C, LENS)[1])
    OPS[kind](x8.PREC[fmt]).dispatch(q.cuda(), cache, o, l, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    own = torch.zeros_like(obuf, dtype=torch.bool)
    for b, qn in enumerate(qlens):
        own[b, :H, :qn, :xm.DV] = True
    assert bool((obuf[~own].float() == ck.SENT_O).all()), "the launch wrote outside O's live rows"
    assert bool((lbuf[~own[..., 0][:, :, :R + 1]] == ck.SENT_L).all()), "the launch wrote outside L's live rows"
    return o.cpu(), l.cpu()


@pytest.mark.parametrize("kvscale", [0.37, None])
@pytest.mark.parametrize("H", [40, 16])
@pytest.mark.parametrize("page", PAGES)
@pytest.mark.parametrize("fmt", FMTS)
def test_a_launch_lies_inside_the_float64_model_s_bounds(fmt, page, H, kvscale):
    qlens = (37, 5, 0)
    q64, kvb, idx = drawn(fmt, H, 37, qlens)
    o, l = launch("sparse prefill", fmt, H, qlens, kvscale, q64, *cache_of(page, kvb, kept(idx, qlens)), idx)
    for b, (n, qn) in enumerate(zip(LENS[:2], qlens)):                    # (sequence 2 has no live row: `launch` has held its sentinels)
        ob, lb = o[b:b + 1, :, :qn], l[b:b + 1, :, :qn]
        assert bool(torch.isfinite(ob.float()).all()) and bool(torch.isfinite(lb).all()), "poison reached a result"
        ref = xm.model(q64[b:b + 1, :, :qn], kvb[b:b + 1], kvscale, (n,), idx[b:b + 1, :qn], True, xm.SCALE)
        blind = torch.from_numpy(~np.isfinite(ref.L))
        assert bool(blind.any()) == (b == 1) and not ob[blind].float().any() and bool((lb[blind] == -ck.FLT_MAX).all()), "a row without a visible slot"
        wo, wl, text = xm.compare(ob, lb / ck.LOG2E, ref, fmt, fmt, (n,), margin=1)
        print("%s page %s H %d kvScale %s sequence %d: worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % (fmt, page, H, kvscale, b, wo, wl))
        assert wo <= xm.MARGIN and wl <= xm.MARGIN, text


@pytest.mark.parametrize("H", [40, 129])
@pytest.mark.parametrize("page", PAGES)
@pytest.mark.parametrize("fmt", FMTS)
def test_32_full_rows_are_the_sparse_decode_launch_bit_for_bit(fmt, page, H):
    qlens = (32, 32, 32)
    q64, kvb, idx = drawn(fmt, H, 32, qlens)
    args = (fmt, H, qlens, 0.37, q64, *cache_of(page, kvb, kept(idx, qlens)), idx)
    assert ck.same(launch("sparse prefill", *args), launch("sparse decode", *args))


@pytest.mark.parametrize("page", PAGES)
@pytest.mark.parametrize("fmt", FMTS)
def test_the_identity_list_is_the_dense_prefill_launch_bit_for_bit(fmt, page):
    qlens = (70, 5, 0)
    q64, kvb, _idx = drawn(fmt, 40, 70, qlens)
    idx = np.broadcast_to(np.arange(C, dtype=np.int64), (B, 70, C)).copy()
    args = (fmt, 40, qlens, 0.37, q64, *cache_of(page, kvb, BELOW), idx)      # poison at and past every length
    dense = launch("dense prefill", *args)
    assert bool(torch.isfinite(dense[0][:2, :, :5].float()).all()) and dense[0][0].float().abs().max() > 0
    assert ck.same(launch("sparse prefill", *args), dense)


def test_flash_mla_sparse_prefill_fp8_end_to_end_and_in_a_graph():
    from metal_flash_attention_amd import torch_binding as tb
    qlens_host = (37, 5, 0)
    q64, kvb, idx = drawn("bf16", 40, 37, qlens_host)
    cache, cache_kw = cache_of(16, kvb, BELOW)                            # (the replay's other lists and frontiers name other keys)
    want_o, want_l = launch("sparse prefill", "bf16", 40, qlens_host, 0.37, q64, cache, cache_kw, idx)
    q, lens, qlens = x8.tensor(q64, "bf16").cuda(), ck.lengths(LENS), ck.lengths(qlens_host)
    lists, scale = x8.lists_on_device(idx, C, LENS)[0], x8.scale_of(0.37)
    run = lambda ql, li: tb.flash_mla_sparse_prefill_fp8(q, cache, lens, li, softmax_scale=xm.SCALE, kv_scale=scale, q_lengths=ql,  # noqa: E731
                                                         block_table=cache_kw["blockTable"], return_lse=True)
    o, lse = run(qlens, lists)
    torch.cuda.synchronize()
    assert o.shape == (3, 40, 37, xm.DV) and o.dtype == q.dtype and lse.shape == (3, 40, 37) and lse.dtype == torch.float32

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
    with torch.cuda.graph(graph):                                         # a straight chain of one kernel
        got = run(s_q, s_lists)
    for new_q, new_lists, w, rows in ((qlens, lists, (o, lse), qlens_host), (other_q, other_lists, want, (4, 3, 0)), (qlens, lists, (o, lse), qlens_host)):
        got[0].fill_(ck.SENT_O)
        s_q.copy_(new_q)
        s_lists.copy_(new_lists)
        graph.replay()
        torch.cuda.synchronize()
        equal(got, w, rows)
        assert all(bool((got[0][b, :, qn:].float() == ck.SENT_O).all()) for b, qn in enumerate(rows)), "a replay wrote a row at or past qn"
