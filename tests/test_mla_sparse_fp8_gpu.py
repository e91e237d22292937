"""GPU test: sparse MLA decode over an e4m3 latent cache (include/mfa_mla_sparse_fp8.h) through the C ABI and through torch, held per
element to the bounds of tests/mla_sparse_fp8_model.py for O and for L on the cases tests/test_mla_sparse_fp8_sensitivity.py walks on the
CPU with the mutants: mla_sparse_model's CASES and SEAM_CASES -- its batches, its lists -- over byte caches with a kvScale of 0.37, 3.0
and None in turn.  Built in the way of tests/test_mla_sparse_gpu.py.  Every allocation is poisoned: every cache row that no list of the
launch makes visible is the NaN bytes 0x7f / 0xff (by key parity), and so are the pages no visible key lives in, the padding of strided
rows and the PAD rows around every sequence of the seam batch; the workspace is NaN; the index allocation is wider than topk and its
tail names a poisoned row; kvScale is entry 0 of a longer array whose other entries are SCALE_TAIL, what a kernel that indexed it by
sequence or by row would find; O and L lie in larger sentinel-filled allocations, which must keep every sentinel outside the launch's rows.

Beside the bounds: the paged launch against the contiguous one and one piece against no workspace, byte for byte; the identity list,
unsplit, against AttentionMLADecodeFP8 on the same inputs, bit for bit in O and L; flash_mla_sparse_decode_fp8 end to end; a decode loop
through torch -- mla_cache_append into an e4m3 page pool, lists drawn over the new length, sparse decode -- over a page seam and a
32-slot step seam; one captured graph of append -> sparse decode."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402
import mla_fp8_model as fm  # noqa: E402
import mla_sparse_fp8_model as xm  # noqa: E402
from metal_flash_attention_amd import AttentionMLADecodeFP8, AttentionMLASparseDecodeFP8, GEMMOperandPrecision as P, quantizeE4M3  # noqa: E402

pytestmark = pytest.mark.gpu

E4M3 = torch.float8_e4m3fn
DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
PREC = {"bf16": P.BF16, "f16": P.FP16, "f32": P.FP32}
TAIL = 24            # slots of an index row past topk
SEEN = {}


def tensor(x64, fmt):
    t = torch.from_numpy(np.ascontiguousarray(x64)).to(DTYPE[fmt])
    assert torch.equal(t.to(torch.float64), torch.from_numpy(np.ascontiguousarray(x64)))   # the model's values are the kernel's
    return t


def e4m3(bytes_):
    """host uint8 (numpy) -> a float8_e4m3fn tensor of those bytes"""
    return torch.from_numpy(np.ascontiguousarray(bytes_)).view(E4M3)


def scale_of(kvscale):
    """kvScale on the device as entry 0 of a longer array: a kernel that indexed it by sequence or by b R + r finds SCALE_TAIL behind it"""
    if kvscale is None:
        return None
    return torch.tensor([kvscale] + 20 * list(xm.SCALE_TAIL), dtype=torch.float32, device="cuda")[:1]


def poison_rows(shape):
    """uint8 of `shape` [.., keys, width]: 0x7f in even keys, 0xff in odd ones"""
    out = np.empty(shape, dtype=np.uint8)
    out[...] = np.where(np.arange(shape[-2]) % 2, 0xFF, 0x7F).astype(np.uint8)[:, None]
    return out


def cache_of(case, kvb, keep):
    """the byte cache on the device as the case lays it out, the NaN bytes in every row `keep` [B][C] does not name, and the launch
    keywords of the layout (the strides of an e4m3 cache count bytes)"""
    layout, page, B, C = case["layout"], case["page"], len(case["lens"]), case["C"]
    if page:                                                              # the pool of xm.page_table; a page without a kept key is not in it
        table = xm.page_table(page, None, B, C).copy()
        pps = -(-C // page)
        pool = poison_rows((B * pps + 1, page, xm.DK))
        for b in range(B):
            for i in range(pps):
                held = keep[b, i * page:(i + 1) * page]
                if held.any():
                    pool[int(table[b, i])][:len(held)][held] = kvb[b, i * page:(i + 1) * page][held]
                else:
                    table[b, i] = B * pps                                 # the last page: all poison
        if case["lists"].startswith("seam"):                              # the rows widened over [C, C + PAD): entries that name the page of poison
            wide = -(-(C + xm.PAD) // page)
            table = np.concatenate([table, np.full((B, wide - pps), B * pps, dtype=np.int32)], axis=1)
        return e4m3(pool).cuda(), dict(pageSize=page, blockTable=torch.from_numpy(table).cuda(), blockTableStride=table.shape[1])
    if layout == "padded":                                                # PAD rows of poison in front of and behind every sequence
        buf = poison_rows((B, xm.PAD + C + xm.PAD, xm.DK))
        buf[:, xm.PAD:xm.PAD + C][keep] = kvb[keep]
        dev = e4m3(buf).cuda()
        return dev[:, xm.PAD:xm.PAD + C], dict(strides=dict(KV=(xm.DK, 0, (C + 2 * xm.PAD) * xm.DK)))
    if layout == "shared":                                                # one cache for every sequence: batchStride 0
        one = np.where(keep.any(axis=0)[None, :, None], kvb[:1], poison_rows((1, C, xm.DK)))
        return e4m3(one).cuda(), dict(strides=dict(KV=(xm.DK, 0, 0)))
    held = np.where(keep[:, :, None], kvb, poison_rows((B, C, xm.DK)))
    if layout == "ld640":                                                 # rows 640 BYTES apart in a larger allocation, poison between them
        buf = np.full((B, C + 2, 640), 0xFF, dtype=np.uint8)
        buf[:, :C, :xm.DK] = held
        dev = e4m3(buf).cuda()
        return dev[:, :C, :xm.DK], dict(strides=dict(KV=(640, 0, (C + 2) * 640)))
    buf = np.full((B + 1, C, xm.DK), 0xFF, dtype=np.uint8)                # one more sequence of poison behind the last
    buf[:B] = held
    return e4m3(buf).cuda()[:B], {}


def lists_on_device(idx, C=xm.C, lens=xm.LENS):
    """the lists in a wider allocation [B, R + 1, topk + TAIL]: everything outside them names a row that is poison -- key C - 1, or, on a
    batch with a full cache, key C + 1 (in the padding behind a sequence, or in a page of poison)"""
    B, R, topk = idx.shape
    fill = C - 1 if max(lens) < C else C + 1
    assert max(lens) < C or (fill >= C and fill < C + xm.PAD)
    buf = torch.full((B, R + 1, topk + TAIL), fill, dtype=torch.int32)
    buf[:, :R, :topk] = torch.from_numpy(idx.astype(np.int32))
    dev = buf.cuda()
    view = dev[:, :R, :topk]
    return view, dict(indices=view, topk=topk, indexStrides=(int(view.stride(1)), int(view.stride(0))))


def launch(case, q64, cache, cache_kw, idx, pieces, *, op=None):
    """one launch on sentinel-filled O and L that lie inside larger allocations -> (O [B, H, R, 512], L [B, H, R] base 2) on the host.
    pieces: None runs without a workspace; a number is given as it is with a NaN-filled workspace of the size the library asks for.
    idx None: the dense e4m3 launch (op=) on the same operands"""
    fmt, H, R, B, C = case["fmt"], case["H"], case["R"], len(case["lens"]), case["C"]
    op = op or AttentionMLASparseDecodeFP8(PREC[fmt], PREC[case["out"]])
    q = tensor(q64, fmt).cuda()
    obuf = torch.full((B, H + 1, R + 2, xm.DV + 8), ck.SENT_O, dtype=DTYPE[case["out"]], device="cuda")
    lbuf = torch.full((B, H + 1, R + 1), ck.SENT_L, dtype=torch.float32, device="cuda")
    o, l = obuf[:, :H, :R, :xm.DV], lbuf[:, :H, :R]
    kw = dict(rows=R, column=C, heads=H, batches=B, scale=xm.SCALE, causal=case["causal"], cacheLengths=ck.lengths(case["lens"]),
              lStrides=(int(l.stride(1)), int(l.stride(0))), kvScale=scale_of(case["kvscale"]))
    kw.update(cache_kw)
    kw["strides"] = dict(kw.get("strides", {}), O=(int(o.stride(2)), int(o.stride(1)), int(o.stride(0))))
    if idx is not None:
        _view, idx_kw = lists_on_device(idx, C, case["lens"])
        kw.update(idx_kw)
        if pieces is not None:
            need, planned = op.plannedSplit(pieces=pieces, **kw)
            assert planned == pieces and need == (pieces * B * H * R * (xm.DV + 2) * 4 if pieces > 1 else 0)
            form = op.launchForm(pieces=pieces, workspace=0x1000, workspaceBytes=need, **kw)
            groups = -(-H // 32)
            if pieces > 1:
                assert form.startswith("attn_mla8x_d576_%s_k (grid %d = %d groups x %d rows x %d sequences x %d pieces, topk %d" % (
                    case["fmt"], groups * R * B * pieces, groups, R, B, pieces, case["topk"])), form
                assert "+ attn_mla8x_d576_%s_combine" % case["fmt"] in form
            kw.update(pieces=pieces, workspace=torch.full((max(need, 16) // 4,), float("nan"), dtype=torch.float32, device="cuda"))
    op.dispatch(q, cache, o, l, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    inside = torch.zeros_like(obuf, dtype=torch.bool)
    inside[:, :H, :R, :xm.DV] = True
    assert bool((obuf[~inside].float() == ck.SENT_O).all()), "the launch wrote outside O's rows"
    linside = torch.zeros_like(lbuf, dtype=torch.bool)
    linside[:, :H, :R] = True
    assert bool((lbuf[~linside] == ck.SENT_L).all()), "the launch wrote outside L's rows"
    return o.cpu(), l.cpu()


def hold(tag, case, idx, o, l, ref, info, natural=False, blind_at_least=None):
    """no poison in any row; a row without a visible slot holds O = 0 and L = -FLT_MAX (natural: torch's L, that times ln 2); every
    element inside the model's bounds at MARGIN"""
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(l).all()), tag + ": poison reached a result"
    blind = 0
    for b, n in enumerate(xm.seen_lens(case)):
        for r in range(case["R"]):
            if not xm.visible(idx[b, r], n, r, case["R"], case["causal"]).any():
                blind += 1
                assert not o[b, :, r].float().any() and bool((l[b, :, r] < -1e38).all() if natural else (l[b, :, r] == -ck.FLT_MAX).all()), (tag, b, r)
    assert blind >= (case["R"] if blind_at_least is None else blind_at_least)   # (the sequence of length 0 at least)
    wo, wl, text = xm.compare(o, l if natural else l / ck.LOG2E, ref, case["fmt"], case["out"], xm.seen_lens(case), margin=1, info=info)
    SEEN[tag] = max(SEEN.get(tag, 0.0), wo, wl)
    print("%s: worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % (tag, wo, wl))
    assert wo <= xm.MARGIN and wl <= xm.MARGIN, text


def kept(case, idx):
    return xm.keep_mask(idx, case["causal"], case["R"], case["lens"], case["C"])


@pytest.mark.parametrize("name", list(xm.ALL_CASES))
def test_a_case_lies_inside_the_model_s_bounds(name):
    case, pieces, q64, kvb, idx, ref, info = xm.inputs(name)
    cache, cache_kw = cache_of(case, kvb, kept(case, idx))
    o, l = launch(case, q64, cache, cache_kw, idx, pieces)
    hold("%s (kvScale %s)" % (name, case["kvscale"]), case, idx, o, l, ref, info)


PAGED = [name for name, case in xm.SEAM_CASES.items() if case["page"]]    # pages of 16, 32, 64 and 512, unsplit and in pieces


@pytest.mark.parametrize("name", ["f pages of 16, planned", "f pages of 256, planned"] + PAGED)
def test_paged_is_the_contiguous_launch_byte_for_byte(name):
    case, pieces, q64, kvb, idx, _ref, _info = xm.inputs(name)
    keep = kept(case, idx)
    pool, pool_kw = cache_of(case, kvb, keep)
    flat, flat_kw = cache_of(dict(case, page=None, layout="padded" if name in PAGED else case["layout"]), kvb, keep)
    assert ck.same(launch(case, q64, pool, pool_kw, idx, pieces), launch(case, q64, flat, flat_kw, idx, pieces))


def test_one_piece_with_a_workspace_is_the_launch_without_one():
    for name in ("a random subset, unsplit", "s sixty-four slots, eight rows", "s pages of 64, thirty-three slots"):   # ... and on the seam batch
        case, _pieces, q64, kvb, idx, _ref, _info = xm.inputs(name)
        cache, cache_kw = cache_of(case, kvb, kept(case, idx))
        assert ck.same(launch(case, q64, cache, cache_kw, idx, None), launch(case, q64, cache, cache_kw, idx, 1)), name


def test_the_identity_list_is_the_dense_e4m3_launch_bit_for_bit():
    """the list arange(1536) for every row, unsplit, against AttentionMLADecodeFP8 on the same inputs: O and L bit for bit.  The lane of
    a key, the contraction order, the order of every sum, the scale arithmetic and the masked slots' exact zeros are attn_mla8.h's; the
    trailing steps past a length are steps of holes and change nothing."""
    identity_against_dense(xm.LENS, xm.C, "packed")


def test_the_identity_list_is_the_dense_e4m3_launch_bit_for_bit_on_the_seam_batch():
    """... where lengths ARE multiples of the step, one length is the column and one lies past it"""
    identity_against_dense(xm.SEAM_LENS, xm.SEAM_C, "padded")


def identity_against_dense(lens, C, layout):
    B = len(lens)
    case = dict(fmt="f16", H=11, R=3, topk=C, causal=True, page=None, layout=layout, out="f16", lens=tuple(lens), C=C, lists="identity", kvscale=0.37)
    kvb = fm.cache_bytes(0, B, C)
    rng = np.random.default_rng(77)
    q64 = xm.round_to(rng.uniform(-1.0, 1.0, (B, case["H"], case["R"], xm.DK)), case["fmt"])
    idx = np.broadcast_to(np.arange(C, dtype=np.int64), (B, case["R"], C)).copy()
    keep = np.stack([np.arange(C) < n for n in lens])
    cache, cache_kw = cache_of(case, kvb, keep)
    sparse = launch(case, q64, cache, cache_kw, idx, None)
    dense = launch(case, q64, cache, cache_kw, None, None, op=AttentionMLADecodeFP8(PREC[case["fmt"]]))
    assert bool(torch.isfinite(dense[0].float()).all()) and dense[0].float().abs().max() > 0
    assert torch.equal(sparse[0].view(torch.int16), dense[0].view(torch.int16)), "O differs from the dense e4m3 launch"
    assert torch.equal(sparse[1].view(torch.int32), dense[1].view(torch.int32)), "L differs from the dense e4m3 launch"
    case = dict(case, fmt="bf16", out="bf16", H=40, R=1, causal=False, kvscale=3.0)     # ... and two groups of heads, not causal, bf16
    q64 = xm.round_to(rng.uniform(-1.0, 1.0, (B, case["H"], case["R"], xm.DK)), case["fmt"])
    idx = idx[:, :1]
    sparse = launch(case, q64, cache, cache_kw, idx, None)
    dense = launch(case, q64, cache, cache_kw, None, None, op=AttentionMLADecodeFP8(P.BF16))
    assert dense[0].float().abs().max() > 0
    assert torch.equal(sparse[0].view(torch.int16), dense[0].view(torch.int16)) and torch.equal(sparse[1].view(torch.int32), dense[1].view(torch.int32))


@pytest.mark.parametrize("name", ["d causal, past the frontier and the length", "f pages of 16, planned"])
def test_flash_mla_sparse_decode_fp8_end_to_end(name):
    from metal_flash_attention_amd import torch_binding as tb
    case, pieces, q64, kvb, idx, ref, info = xm.inputs(name)     # (pieces=None below is the host's plan, which is this case's)
    B, C = len(case["lens"]), case["C"]
    cache, cache_kw = cache_of(case, kvb, kept(case, idx))
    q = tensor(q64, case["fmt"]).cuda()
    lists, _kw = lists_on_device(idx)
    assert not lists.is_contiguous() and cache.dtype == E4M3      # read where they lie
    args = dict(softmax_scale=xm.SCALE, kv_scale=scale_of(case["kvscale"]), block_table=cache_kw.get("blockTable"), causal=case["causal"])
    o, lse = tb.flash_mla_sparse_decode_fp8(q, cache, ck.lengths(xm.LENS), lists, return_lse=True, **args)
    torch.cuda.synchronize()
    assert o.shape == (B, case["H"], case["R"], xm.DV) and o.dtype == q.dtype and lse.shape == (B, case["H"], case["R"]) and lse.dtype == torch.float32
    hold("flash_mla_sparse_decode_fp8, " + name, case, idx, o.cpu(), lse.cpu(), ref, info, natural=True)
    only = tb.flash_mla_sparse_decode_fp8(q, cache, ck.lengths(xm.LENS), lists, **args)
    assert torch.equal(only.view(torch.int16), o.view(torch.int16))


# ------------------------------------------------------------------------------------------------- append + sparse decode through torch
T_PAGE, T_PAGES, T_H, T_SCALE, T_TOPK = 16, 4, 5, 0.37, 40    # 4 pages a sequence: 64 keys; 40 slots: a whole step and a partial one
W_START, W_STEPS = (14, 0, 30), 6                             # 14 grows over 16; 30 over 32: a page seam, and more than 32 visible slots


def expected_rows(latent, rope, kvscale):
    """[B, R, 576] uint8 on the host: the bytes the append writes for every source row, from mfa_kv_quantize_e4m3"""
    rows = torch.cat([latent, rope], dim=2).cpu()
    scale = float(np.float32(kvscale))
    return torch.tensor([quantizeE4M3(x, scale) for x in rows.float().reshape(-1).tolist()], dtype=torch.uint8).reshape(rows.shape).numpy()


def pool_state(lens, seed):
    """sequences with lens keys already in an e4m3 page pool (poison everywhere else) -> (logical bytes, host pool, device pool, table)"""
    rng = np.random.default_rng(seed)
    B = len(lens)
    logical = fm.cache_bytes()[:B, :T_PAGE * T_PAGES].copy()
    table = rng.permutation(B * T_PAGES).astype(np.int32).reshape(B, T_PAGES)
    pool = poison_rows((B * T_PAGES + 1, T_PAGE, xm.DK))
    for b, n in enumerate(lens):
        for c in range(n):
            pool[table[b, c // T_PAGE], c % T_PAGE] = logical[b, c]
    return logical, pool, e4m3(pool).cuda(), table


def drawn_lists(rng, lens, R, topk):
    """idx [B, R, topk]: a random subset of the positions below each length plus the newest key, -1 scattered among them"""
    idx = np.full((len(lens), R, topk), xm.HOLE, dtype=np.int64)
    for b, n in enumerate(lens):
        for r in range(R):
            take = min(n - 1, topk - 5)
            row = np.concatenate([rng.choice(n - 1, size=take, replace=False) if take > 0 else [], [n - 1]]).astype(np.int64)
            idx[b, r, :len(row)] = row
            rng.shuffle(idx[b, r])
    return idx


def test_a_decode_loop_of_append_and_sparse_decode_through_torch():
    """what a serving loop does: W_STEPS steps of one token a sequence, each an append into an e4m3 pool (pages of 16, a permuted table,
    poison wherever nothing was written), lists drawn over the new length and the sparse decode over them, held to the float64 model over
    the bytes the cache HOLDS on needle queries; the bytes it holds are held to mfa_kv_quantize_e4m3.  The lengths pass 16 and 32 -- the
    first key of a new page -- and the visible slots of the longest sequence pass 32: more keys than one step holds"""
    from metal_flash_attention_amd import torch_binding as tb
    lens, cap = list(W_START), T_PAGE * T_PAGES
    ends = [n + W_STEPS for n in lens]
    assert any(a < 16 <= e for a, e in zip(lens, ends)) and any(a < 32 < e for a, e in zip(lens, ends)) and max(ends) <= cap
    assert min(max(ends) - 1, T_TOPK - 5) + 1 > 32 > min(max(lens), T_TOPK - 5) + 1     # the visible slots cross the 32-slot step
    logical, pool, dev, table = pool_state(lens, 23)
    tab = torch.from_numpy(table).cuda()
    scale = scale_of(T_SCALE)
    rng = np.random.default_rng(29)
    g = torch.Generator().manual_seed(31)
    case = dict(fmt="bf16", out="bf16", H=T_H, R=1, causal=True, C=cap)
    for step in range(W_STEPS):
        latent = (torch.randn((3, 1, 512), generator=g) * 0.3).to(torch.bfloat16)
        rope = (torch.randn((3, 1, 64), generator=g) * 0.3).to(torch.bfloat16)
        lens = [n + 1 for n in lens]
        new = expected_rows(latent, rope, T_SCALE)
        for b, n in enumerate(lens):
            logical[b, n - 1] = new[b, 0]
            pool[table[b, (n - 1) // T_PAGE], (n - 1) % T_PAGE] = new[b, 0]
        lengths = ck.lengths(lens)
        tb.mla_cache_append(latent.cuda(), rope.cuda(), dev, lengths, block_table=tab, kv_scale=scale)
        idx = drawn_lists(rng, lens, 1, T_TOPK)
        assert all((idx[b, 0] == n - 1).any() and (idx[b, 0] == xm.HOLE).any() for b, n in enumerate(lens))
        torch.cuda.synchronize()
        held = dev.view(torch.uint8).cpu().numpy()
        assert np.array_equal(held, pool), "step %d: the e4m3 pool" % step        # the whole pool, byte for byte: the appended bytes are the codec's
        seen = np.zeros_like(logical)                                             # the bytes the cache holds, read back through the table
        for b, n in enumerate(lens):
            seen[b, :n] = held[table[b, np.arange(n) // T_PAGE], np.arange(n) % T_PAGE]
        q64, info = xm.needle_queries(seen, T_SCALE, lens, idx, T_H, 1, True, "bf16", xm.SCALE, seed=step)
        lists, _kw = lists_on_device(idx, cap, lens)
        o, lse = tb.flash_mla_sparse_decode_fp8(tensor(q64, "bf16").cuda(), dev, lengths, lists, softmax_scale=xm.SCALE, kv_scale=scale,
                                                block_table=tab, return_lse=True)
        torch.cuda.synchronize()
        ref = xm.model(q64, seen, T_SCALE, lens, idx, True, xm.SCALE, page=T_PAGE)
        assert o.shape == (3, T_H, 1, xm.DV) and o.dtype == torch.bfloat16 and lse.shape == (3, T_H, 1)
        hold("decode loop, sparse e4m3", dict(case, lens=tuple(lens)), idx, o.cpu(), lse.cpu(), ref, info, natural=True, blind_at_least=0)


def test_a_captured_graph_of_append_and_sparse_decode_replays_the_eager_result():
    from metal_flash_attention_amd import torch_binding as tb
    lens = [33, 0, 50]
    _logical, _pool, dev, table = pool_state(lens, 11)
    tab = torch.from_numpy(table).cuda()
    start = dev.clone()
    scale = scale_of(T_SCALE)
    g = torch.Generator().manual_seed(29)
    latent, rope = (torch.randn((3, 2, 512), generator=g) * 0.3).to(torch.float16).cuda(), (torch.randn((3, 2, 64), generator=g) * 0.3).to(torch.float16).cuda()
    q = (torch.randn((3, T_H, 2, xm.DK), generator=g) * 0.5).to(torch.float16).cuda()
    lens = [n + 2 for n in lens]
    lengths = ck.lengths(lens)
    idx = np.concatenate([drawn_lists(np.random.default_rng(5), [n - 1 + r for n in lens], 1, 96) for r in range(2)], axis=1)   # row r sees n - 2 + r keys
    lists, _kw = lists_on_device(idx, T_PAGE * T_PAGES, lens)

    def both():
        tb.mla_cache_append(latent, rope, dev, lengths, block_table=tab, kv_scale=scale)
        return tb.flash_mla_sparse_decode_fp8(q, dev, lengths, lists, softmax_scale=xm.SCALE, kv_scale=scale, block_table=tab, return_lse=True, pieces=2)

    want = both()                                  # eager (and the warm-up outside the capture)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want[0].float()).all()) and want[0][0].float().abs().max() > 0
    want_pool = dev.clone()
    dev.copy_(start)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                  # a straight chain: append, pieces, combine
        o, lse = both()
    dev.copy_(start)
    o.zero_()
    lse.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(o.view(torch.int16), want[0].view(torch.int16)) and torch.equal(lse, want[1])
    assert torch.equal(dev.view(torch.uint8), want_pool.view(torch.uint8)) and not torch.equal(dev.view(torch.uint8), start.view(torch.uint8))
