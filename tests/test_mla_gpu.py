"""GPU test: multi-head latent attention decode over a compressed cache (include/mfa_mla.h) through the C ABI and through torch, held per
element to the bounds of tests/mla_model.py for O and for L.  One batch -- lengths (700, 200, 100, 5, 0, 1500) in a cache of 1536 keys: an
empty sequence, n < R, partial tiles, sequences with fewer tiles than pieces, many tiles -- under the cases of mla_model.CASES, which
tests/test_mla_sensitivity.py walks on the CPU with the mutants.  Needle queries; NaN in every key that must not be loaded (past a
length, the tail of a last page, pages no table names, the padding of a strided row) and in the whole workspace; O and L lie in larger
sentinel-filled allocations, which must keep every sentinel outside the launch's rows.

The same machinery runs mla_model.SEAM_CASES: lengths (1, 8, 16, 32, 33, 64, 96, 256, 320, 400, 0) in a cache of 320 keys -- full last
steps, full last pages (pages of 16, 32 and 64, and one page of 512 that holds the whole column, blockTableStride 1), whole piece tiles,
n == column, and a length past the column that the launch must clamp.  What lies behind a cache is poison too: the sequence after the
one handed 400 is the empty one, one more sequence of poison follows the last, and the table entries past a sequence's pages name the
page of poison -- a kernel that does not clamp reads NaN inside the allocation."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402
import mla_model as mm  # noqa: E402
from metal_flash_attention_amd import AttentionMLADecode, GEMMOperandPrecision as P  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
PREC = {"bf16": P.BF16, "f16": P.FP16, "f32": P.FP32}
SEEN = {}


def tensor(x64, fmt):
    t = torch.from_numpy(np.ascontiguousarray(x64)).to(DTYPE[fmt])
    assert torch.equal(t.to(torch.float64), torch.from_numpy(np.ascontiguousarray(x64)))   # the model's values are the kernel's
    return t


def keep_mask(case):
    return np.stack([np.arange(case["C"]) < n for n in case["lens"]])


def whole_pages(kv, keep, page, reach):
    """the cache [B, C, 576] and keep [B][C] widened with keys nobody keeps to whole pages that cover `reach` keys: ck.pool_host gives every
    page of them that holds no kept key -- the pages past a sequence's last, the empty sequence's whole row -- the page of poison"""
    B, C = keep.shape
    wide = -(-max(C, reach) // page) * page
    kvw = torch.zeros((B, wide, kv.shape[2]), dtype=ck.raw(kv).dtype)
    kvw[:, :C] = ck.raw(kv)
    keepw = np.zeros((B, wide), dtype=bool)
    keepw[:, :C] = keep
    return kvw.view(kv.dtype), keepw


def cache_of(case, kv64):
    """the cache on the device as the case lays it out, poisoned wherever no sequence may read, and the launch keywords of the layout"""
    fmt, layout, page, B, C = case["fmt"], case["layout"], case["page"], len(case["lens"]), case["C"]
    kv = tensor(kv64, fmt)
    if page:                                                              # (a page larger than the column: ONE page a sequence)
        kvw, keepw = whole_pages(kv, keep_mask(case), page, max(case["lens"]))
        pool, _same, table = ck.pool_host(kvw[:, None], kvw[:, None], page, keepw, seed=page)
        pool = pool[:, 0].contiguous()                                    # [pages, page, 576]
        assert table.shape[1] == -(-max(C, max(case["lens"])) // page) and bool(torch.isnan(pool[-1].float()).all())
        return pool.cuda(), dict(pageSize=page, blockTable=torch.from_numpy(table).cuda(), blockTableStride=table.shape[1])
    if layout == "shared":                                                # one cache for every sequence: batchStride 0
        one = kv[:1].clone()
        one[:, max(case["lens"]):] = float("nan")
        return one.cuda(), dict(strides=dict(KV=(mm.DK, 0, 0)))
    held = ck.poisoned(kv[:, None], keep_mask(case))[:, 0]
    if layout == "ld640":                                                 # rows 640 apart in a larger allocation, NaN between them
        buf = torch.full((B, C + 2, 640), float("nan"), dtype=kv.dtype)
        buf[:, :C, :mm.DK] = held
        dev = buf.cuda()
        return dev[:, :C, :mm.DK], dict(strides=dict(KV=(640, 0, (C + 2) * 640)))
    buf = torch.full((B + 1, C, mm.DK), float("nan"), dtype=kv.dtype)     # one more sequence of poison behind the last
    buf[:B] = held
    return buf.cuda()[:B], {}


def launch(case, q64, cache, cache_kw, pieces, *, workspace=True):
    """one launch on sentinel-filled O and L that lie inside larger allocations -> (O [B, H, R, 512], L [B, H, R] base 2) on the host.
    pieces: None runs without a workspace; a number is given as it is with a NaN-filled workspace of the size the library asks for"""
    fmt, H, R, B = case["fmt"], case["H"], case["R"], len(case["lens"])
    op = AttentionMLADecode(PREC[fmt], PREC[case["out"]])
    q = tensor(q64, fmt).cuda()
    obuf = torch.full((B, H + 1, R + 2, mm.DV + 8), ck.SENT_O, dtype=DTYPE[case["out"]], device="cuda")
    lbuf = torch.full((B, H + 1, R + 1), ck.SENT_L, dtype=torch.float32, device="cuda")
    o, l = obuf[:, :H, :R, :mm.DV], lbuf[:, :H, :R]
    kw = dict(rows=R, column=case["C"], heads=H, batches=B, scale=mm.SCALE, causal=case["causal"], cacheLengths=ck.lengths(case["lens"]),
              lStrides=(int(l.stride(1)), int(l.stride(0))))             # (the lengths as the case hands them: one may lie past the column)
    kw.update(cache_kw)
    kw["strides"] = dict(kw.get("strides", {}), O=(int(o.stride(2)), int(o.stride(1)), int(o.stride(0))))
    if pieces is not None and workspace:
        need, planned = op.plannedSplit(pieces=pieces, **kw)
        assert planned == pieces and need == (pieces * B * H * R * (mm.DV + 2) * 4 if pieces > 1 else 0)
        form = op.launchForm(pieces=pieces, workspace=0x1000, workspaceBytes=need, **kw)
        groups = -(-H * R // mm.ROWS)
        if pieces > 1:
            assert form.startswith("attn_mla16_d576_%s_k (grid %d = %d groups x %d sequences x %d pieces" % (case["fmt"], groups * B * pieces, groups, B, pieces)), form
        kw.update(pieces=pieces, workspace=torch.full((max(need, 16) // 4,), float("nan"), dtype=torch.float32, device="cuda"))
    op.dispatch(q, cache, o, l, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    inside = torch.zeros_like(obuf, dtype=torch.bool)
    inside[:, :H, :R, :mm.DV] = True
    assert bool((obuf[~inside].float() == ck.SENT_O).all()), "the launch wrote outside O's rows"
    linside = torch.zeros_like(lbuf, dtype=torch.bool)
    linside[:, :H, :R] = True
    assert bool((lbuf[~linside] == ck.SENT_L).all()), "the launch wrote outside L's rows"
    return o.cpu(), l.cpu()


def hold(tag, case, o, l, ref, info, natural=False):
    """no poison in a live row; an empty sequence holds O = 0 and L = -FLT_MAX (natural: torch's L, that times ln 2); every element
    inside the model's bounds at MARGIN"""
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(l).all()), tag + ": poison reached a result"
    for b, n in enumerate(case["lens"]):
        if n == 0:
            assert not o[b].float().any() and bool((l[b] < -1e38).all() if natural else (l[b] == -ck.FLT_MAX).all()), tag + ": the empty sequence"
    wo, wl, text = mm.compare(o, l if natural else l / ck.LOG2E, ref, case["fmt"], case["out"], mm.seen_lens(case), margin=1, info=info)
    SEEN[tag] = max(SEEN.get(tag, 0.0), wo, wl)
    print("%s: worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % (tag, wo, wl))
    assert wo <= mm.MARGIN and wl <= mm.MARGIN, text


@pytest.mark.parametrize("name", list(mm.ALL_CASES))
def test_a_case_lies_inside_the_model_s_bounds(name):
    case, pieces, q64, kv64, ref, info = mm.inputs(name)
    cache, cache_kw = cache_of(case, kv64)
    o, l = launch(case, q64, cache, cache_kw, pieces)
    hold(name, case, o, l, ref, info)


def test_one_piece_with_a_workspace_is_the_launch_without_one():
    for name in ("s1 seam inside a head, unsplit", "s5 pages of 64"):      # ... on the seam batch, contiguous and paged
        case, _pieces, q64, kv64, _ref, _info = mm.inputs(name)
        cache, cache_kw = cache_of(case, kv64)
        assert ck.same(launch(case, q64, cache, cache_kw, None), launch(case, q64, cache, cache_kw, 1)), name
    case, _pieces, q64, kv64, ref, info = mm.inputs("1 unsplit")
    B = len(case["lens"])
    cache, cache_kw = cache_of(case, kv64)
    bare = launch(case, q64, cache, cache_kw, None)
    one = launch(case, q64, cache, cache_kw, 1)
    assert ck.same(bare, one)
    op = AttentionMLADecode(P.BF16)   # a workspace beside pieces = 1 is not looked at, misaligned or not
    o = torch.full((B, case["H"], case["R"], mm.DV), ck.SENT_O, dtype=torch.bfloat16, device="cuda")
    l = torch.full((B, case["H"], case["R"]), ck.SENT_L, dtype=torch.float32, device="cuda")
    ws = torch.full((64,), float("nan"), dtype=torch.float32, device="cuda")
    op.dispatch(tensor(q64, "bf16").cuda(), cache, o, l, stream=torch.cuda.current_stream().cuda_stream, rows=case["R"], column=mm.C, heads=case["H"],
                batches=B, scale=mm.SCALE, cacheLengths=ck.lengths(mm.LENS), pieces=1, workspace=ws.data_ptr() + 4, workspaceBytes=8)
    torch.cuda.synchronize()
    assert ck.same(bare, (o.cpu(), l.cpu())) and bool(torch.isnan(ws).all())


PAGED = [name for name, case in mm.SEAM_CASES.items() if case["page"]]    # pages of 16, 32, 64 and 512, unsplit and in pieces


@pytest.mark.parametrize("name", ["6 pages of 16", "6 pages of 256"] + PAGED)
def test_paged_is_the_contiguous_launch_byte_for_byte(name):
    case, pieces, q64, kv64, _ref, _info = mm.inputs(name)
    pool, pool_kw = cache_of(case, kv64)
    flat, flat_kw = cache_of(dict(case, page=None), kv64)
    assert ck.same(launch(case, q64, pool, pool_kw, pieces), launch(case, q64, flat, flat_kw, pieces))


@pytest.mark.parametrize("name", ["1 planned", "6 pages of 16"])
def test_flash_mla_decode_end_to_end(name):
    from metal_flash_attention_amd import torch_binding as tb
    case, pieces, q64, kv64, ref, info = mm.inputs(name)     # (pieces=None below is the host's plan, which is this case's)
    B = len(case["lens"])
    cache, cache_kw = cache_of(case, kv64)
    q = tensor(q64, case["fmt"]).cuda()
    o, lse = tb.flash_mla_decode(q, cache, ck.lengths(mm.LENS), softmax_scale=mm.SCALE, block_table=cache_kw.get("blockTable"), causal=case["causal"],
                                 return_lse=True)
    torch.cuda.synchronize()
    assert o.shape == (B, case["H"], case["R"], mm.DV) and o.dtype == q.dtype and lse.shape == (B, case["H"], case["R"]) and lse.dtype == torch.float32
    hold("flash_mla_decode, " + name, case, o.cpu(), lse.cpu(), ref, info, natural=True)
    only = tb.flash_mla_decode(q, cache, ck.lengths(mm.LENS), softmax_scale=mm.SCALE, block_table=cache_kw.get("blockTable"), causal=case["causal"])
    assert torch.equal(only.view(torch.int16), o.view(torch.int16))
