"""GPU test: sparse MLA decode (include/mfa_mla_sparse.h) through the C ABI and through torch, held per element to the bounds of
tests/mla_sparse_model.py for O and for L.  One batch -- lengths (700, 200, 100, 5, 0, 1500) in a cache of 1536 keys -- under the cases
of mla_sparse_model.CASES, which tests/test_mla_sparse_sensitivity.py walks on the CPU with the mutants.  Every allocation is poisoned:
every cache row that no list of the launch makes visible is NaN, and so are the pages no visible key lives in, the padding of strided rows
and the whole workspace; the index allocation is wider than topk, and every value anywhere in it is -1 or a position inside [0, C) -- its
tail names a row that is NaN -- so that a wrong kernel reads poison and fails its bounds instead of faulting.  O and L lie in larger
sentinel-filled allocations, which must keep every sentinel outside the launch's rows.

mla_sparse_model.SEAM_CASES run on the seam batch of tests/mla_model.py (tests/test_mla_gpu.py says what it holds) with lists that sit on
the seams of the rule: n - 1 and n, 0, the frontier and the key after it, column - 1 of a full cache, positions in [column,
cacheLengths[b]) of the sequence handed a length past the column, entries below -1.  There every entry lies in [-PAD, C + PAD), and so
does poison: a contiguous cache keeps PAD rows of NaN in front of and behind every sequence (the batch stride spans them); paged lists
hold no negative entry, and the block table's rows are widened by entries that name the page of NaN."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402
import mla_sparse_model as sm  # noqa: E402
from metal_flash_attention_amd import AttentionMLADecode, AttentionMLASparseDecode, GEMMOperandPrecision as P  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
PREC = {"bf16": P.BF16, "f16": P.FP16, "f32": P.FP32}
TAIL = 24            # slots of an index row past topk
SEEN = {}


def tensor(x64, fmt):
    t = torch.from_numpy(np.ascontiguousarray(x64)).to(DTYPE[fmt])
    assert torch.equal(t.to(torch.float64), torch.from_numpy(np.ascontiguousarray(x64)))   # the model's values are the kernel's
    return t


def cache_of(case, kv64, keep):
    """the cache on the device as the case lays it out, NaN in every row `keep` [B][C] does not name, and the launch keywords of the layout"""
    fmt, layout, page, B, C = case["fmt"], case["layout"], case["page"], len(case["lens"]), case["C"]
    kv = tensor(kv64, fmt)
    if page:                                                              # the pool of sm.page_table; a page without a kept key is not in it
        table = sm.page_table(page, None, B, C).copy()
        pps = -(-C // page)
        pool = torch.full((B * pps + 1, page, sm.DK), float("nan"), dtype=kv.dtype)
        for b in range(B):
            for i in range(pps):
                held = torch.from_numpy(keep[b, i * page:(i + 1) * page])
                if held.any():
                    pool[int(table[b, i])][:len(held)][held] = kv[b, i * page:(i + 1) * page][held]
                else:
                    table[b, i] = B * pps                                 # the last page: all NaN
        if case["lists"].startswith("seam"):                              # the rows widened over [C, C + PAD): entries that name the page of NaN
            wide = -(-(C + sm.PAD) // page)
            table = np.concatenate([table, np.full((B, wide - pps), B * pps, dtype=np.int32)], axis=1)
        return pool.cuda(), dict(pageSize=page, blockTable=torch.from_numpy(table).cuda(), blockTableStride=table.shape[1])
    if layout == "padded":                                                # PAD rows of NaN in front of and behind every sequence
        buf = torch.full((B, sm.PAD + C + sm.PAD, sm.DK), float("nan"), dtype=kv.dtype)
        buf[:, sm.PAD:sm.PAD + C][torch.from_numpy(keep)] = kv[torch.from_numpy(keep)]
        dev = buf.cuda()
        return dev[:, sm.PAD:sm.PAD + C], dict(strides=dict(KV=(sm.DK, 0, (C + 2 * sm.PAD) * sm.DK)))
    if layout == "shared":                                                # one cache for every sequence: batchStride 0
        one = kv[:1].clone()
        one[0, torch.from_numpy(~keep.any(axis=0))] = float("nan")
        return one.cuda(), dict(strides=dict(KV=(sm.DK, 0, 0)))
    held = kv.clone()
    held[torch.from_numpy(~keep)] = float("nan")
    if layout == "ld640":                                                 # rows 640 apart in a larger allocation, NaN between them
        buf = torch.full((B, C + 2, 640), float("nan"), dtype=kv.dtype)
        buf[:, :C, :sm.DK] = held
        dev = buf.cuda()
        return dev[:, :C, :sm.DK], dict(strides=dict(KV=(640, 0, (C + 2) * 640)))
    return held.contiguous().cuda(), {}


def lists_on_device(idx, C=sm.C, lens=sm.LENS):
    """the lists in a wider allocation [B, R + 1, topk + TAIL]: everything outside them names a row that is NaN -- key C - 1, or, on a
    batch with a full cache, key C + 1 (in the padding behind a sequence, or in a page of NaN)"""
    B, R, topk = idx.shape
    fill = C - 1 if max(lens) < C else C + 1
    assert max(lens) < C or (fill >= C and fill < C + sm.PAD)
    buf = torch.full((B, R + 1, topk + TAIL), fill, dtype=torch.int32)
    buf[:, :R, :topk] = torch.from_numpy(idx.astype(np.int32))
    dev = buf.cuda()
    view = dev[:, :R, :topk]
    return view, dict(indices=view, topk=topk, indexStrides=(int(view.stride(1)), int(view.stride(0))))


def launch(case, q64, cache, cache_kw, idx, pieces, *, op=None):
    """one launch on sentinel-filled O and L that lie inside larger allocations -> (O [B, H, R, 512], L [B, H, R] base 2) on the host.
    pieces: None runs without a workspace; a number is given as it is with a NaN-filled workspace of the size the library asks for"""
    fmt, H, R, B, C = case["fmt"], case["H"], case["R"], len(case["lens"]), case["C"]
    op = op or AttentionMLASparseDecode(PREC[fmt], PREC[case["out"]])
    q = tensor(q64, fmt).cuda()
    obuf = torch.full((B, H + 1, R + 2, sm.DV + 8), ck.SENT_O, dtype=DTYPE[case["out"]], device="cuda")
    lbuf = torch.full((B, H + 1, R + 1), ck.SENT_L, dtype=torch.float32, device="cuda")
    o, l = obuf[:, :H, :R, :sm.DV], lbuf[:, :H, :R]
    kw = dict(rows=R, column=C, heads=H, batches=B, scale=sm.SCALE, causal=case["causal"], cacheLengths=ck.lengths(case["lens"]),
              lStrides=(int(l.stride(1)), int(l.stride(0))))
    kw.update(cache_kw)
    kw["strides"] = dict(kw.get("strides", {}), O=(int(o.stride(2)), int(o.stride(1)), int(o.stride(0))))
    if idx is not None:
        _view, idx_kw = lists_on_device(idx, C, case["lens"])
        kw.update(idx_kw)
        if pieces is not None:
            need, planned = op.plannedSplit(pieces=pieces, **kw)
            assert planned == pieces and need == (pieces * B * H * R * (sm.DV + 2) * 4 if pieces > 1 else 0)
            form = op.launchForm(pieces=pieces, workspace=0x1000, workspaceBytes=need, **kw)
            groups = -(-H // 32)
            if pieces > 1:
                assert form.startswith("attn_mla16x_d576_%s_k (grid %d = %d groups x %d rows x %d sequences x %d pieces, topk %d" % (
                    case["fmt"], groups * R * B * pieces, groups, R, B, pieces, case["topk"])), form
            kw.update(pieces=pieces, workspace=torch.full((max(need, 16) // 4,), float("nan"), dtype=torch.float32, device="cuda"))
    op.dispatch(q, cache, o, l, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    inside = torch.zeros_like(obuf, dtype=torch.bool)
    inside[:, :H, :R, :sm.DV] = True
    assert bool((obuf[~inside].float() == ck.SENT_O).all()), "the launch wrote outside O's rows"
    linside = torch.zeros_like(lbuf, dtype=torch.bool)
    linside[:, :H, :R] = True
    assert bool((lbuf[~linside] == ck.SENT_L).all()), "the launch wrote outside L's rows"
    return o.cpu(), l.cpu()


def hold(tag, case, idx, o, l, ref, info, natural=False):
    """no poison in any row; a row without a visible slot holds O = 0 and L = -FLT_MAX (natural: torch's L, that times ln 2); every
    element inside the model's bounds at MARGIN"""
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(l).all()), tag + ": poison reached a result"
    blind = 0
    for b, n in enumerate(sm.seen_lens(case)):
        for r in range(case["R"]):
            if not sm.visible(idx[b, r], n, r, case["R"], case["causal"]).any():
                blind += 1
                assert not o[b, :, r].float().any() and bool((l[b, :, r] < -1e38).all() if natural else (l[b, :, r] == -ck.FLT_MAX).all()), (tag, b, r)
    assert blind >= case["R"]                                             # (the sequence of length 0 at least)
    wo, wl, text = sm.compare(o, l if natural else l / ck.LOG2E, ref, case["fmt"], case["out"], sm.seen_lens(case), margin=1, info=info)
    SEEN[tag] = max(SEEN.get(tag, 0.0), wo, wl)
    print("%s: worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % (tag, wo, wl))
    assert wo <= sm.MARGIN and wl <= sm.MARGIN, text


def kept(case, idx):
    return sm.keep_mask(idx, case["causal"], case["R"], case["lens"], case["C"])


@pytest.mark.parametrize("name", list(sm.ALL_CASES))
def test_a_case_lies_inside_the_model_s_bounds(name):
    case, pieces, q64, kv64, idx, ref, info = sm.inputs(name)
    cache, cache_kw = cache_of(case, kv64, kept(case, idx))
    o, l = launch(case, q64, cache, cache_kw, idx, pieces)
    hold(name, case, idx, o, l, ref, info)


PAGED = [name for name, case in sm.SEAM_CASES.items() if case["page"]]    # pages of 16, 32, 64 and 512, unsplit and in pieces


@pytest.mark.parametrize("name", ["f pages of 16, planned", "f pages of 256, planned"] + PAGED)
def test_paged_is_the_contiguous_launch_byte_for_byte(name):
    case, pieces, q64, kv64, idx, _ref, _info = sm.inputs(name)
    keep = kept(case, idx)
    pool, pool_kw = cache_of(case, kv64, keep)
    flat, flat_kw = cache_of(dict(case, page=None, layout="padded" if name in PAGED else case["layout"]), kv64, keep)
    assert ck.same(launch(case, q64, pool, pool_kw, idx, pieces), launch(case, q64, flat, flat_kw, idx, pieces))


def test_one_piece_with_a_workspace_is_the_launch_without_one():
    for name in ("a random subset, unsplit", "s sixty-four slots, eight rows", "s pages of 64, thirty-three slots"):   # ... and on the seam batch
        case, _pieces, q64, kv64, idx, _ref, _info = sm.inputs(name)
        cache, cache_kw = cache_of(case, kv64, kept(case, idx))
        assert ck.same(launch(case, q64, cache, cache_kw, idx, None), launch(case, q64, cache, cache_kw, idx, 1)), name


def test_the_identity_list_is_the_dense_launch_bit_for_bit():
    """case j: the list arange(1536) for every row, unsplit, against the dense launch on the same inputs: O and L bit for bit.  The lane
    of a key, the order of every sum and the masked slots' exact zeros are the dense body's; the trailing steps past a length are steps
    of holes and change nothing."""
    identity_against_dense(sm.LENS, sm.C, "packed")


def test_the_identity_list_is_the_dense_launch_bit_for_bit_on_the_seam_batch():
    """... where lengths ARE multiples of the step -- the steps past them are steps of holes from their first slot on --, one length is
    the column and one lies past it: the list arange(column) is every key such a sequence has"""
    identity_against_dense(sm.SEAM_LENS, sm.SEAM_C, "padded")


def identity_against_dense(lens, C, layout):
    B = len(lens)
    case = dict(fmt="f16", H=11, R=3, topk=C, causal=True, page=None, layout=layout, out="f16", lens=tuple(lens), C=C, lists="identity")
    kv64 = sm.mm.cache_values(case["fmt"], 0, B, C)
    rng = np.random.default_rng(77)
    q64 = sm.round_to(rng.uniform(-1.0, 1.0, (B, case["H"], case["R"], sm.DK)), case["fmt"])
    idx = np.broadcast_to(np.arange(C, dtype=np.int64), (B, case["R"], C)).copy()
    keep = np.stack([np.arange(C) < n for n in lens])
    cache, cache_kw = cache_of(case, kv64, keep)
    sparse = launch(case, q64, cache, cache_kw, idx, None)
    dense = launch(case, q64, cache, cache_kw, None, None, op=AttentionMLADecode(PREC[case["fmt"]]))
    assert bool(torch.isfinite(dense[0].float()).all()) and dense[0].float().abs().max() > 0
    assert torch.equal(sparse[0].view(torch.int16), dense[0].view(torch.int16)), "O differs from the dense launch"
    assert torch.equal(sparse[1].view(torch.int32), dense[1].view(torch.int32)), "L differs from the dense launch"
    case = dict(case, fmt="bf16", out="bf16", H=40, R=1, causal=False)     # ... and two groups of heads, not causal, bf16
    q64 = sm.round_to(rng.uniform(-1.0, 1.0, (B, case["H"], case["R"], sm.DK)), case["fmt"])
    cache, cache_kw = cache_of(case, sm.mm.cache_values("bf16", 0, B, C), keep)
    idx = idx[:, :1]
    sparse = launch(case, q64, cache, cache_kw, idx, None)
    dense = launch(case, q64, cache, cache_kw, None, None, op=AttentionMLADecode(P.BF16))
    assert torch.equal(sparse[0].view(torch.int16), dense[0].view(torch.int16)) and torch.equal(sparse[1].view(torch.int32), dense[1].view(torch.int32))


@pytest.mark.parametrize("name", ["d causal, past the frontier and the length", "f pages of 16, planned"])
def test_flash_mla_sparse_decode_end_to_end(name):
    from metal_flash_attention_amd import torch_binding as tb
    case, pieces, q64, kv64, idx, ref, info = sm.inputs(name)     # (pieces=None below is the host's plan, which is this case's)
    B, C = len(case["lens"]), case["C"]
    cache, cache_kw = cache_of(case, kv64, kept(case, idx))
    q = tensor(q64, case["fmt"]).cuda()
    lists, _kw = lists_on_device(idx)
    assert not lists.is_contiguous()                              # read where they lie
    o, lse = tb.flash_mla_sparse_decode(q, cache, ck.lengths(sm.LENS), lists, softmax_scale=sm.SCALE, block_table=cache_kw.get("blockTable"),
                                        causal=case["causal"], return_lse=True)
    torch.cuda.synchronize()
    assert o.shape == (B, case["H"], case["R"], sm.DV) and o.dtype == q.dtype and lse.shape == (B, case["H"], case["R"]) and lse.dtype == torch.float32
    hold("flash_mla_sparse_decode, " + name, case, idx, o.cpu(), lse.cpu(), ref, info, natural=True)
    only = tb.flash_mla_sparse_decode(q, cache, ck.lengths(sm.LENS), lists, softmax_scale=sm.SCALE, block_table=cache_kw.get("blockTable"),
                                      causal=case["causal"])
    assert torch.equal(only.view(torch.int16), o.view(torch.int16))
