"""GPU test: prefill over a KV cache CUT ALONG THE KEYS, through the C ABI of include/mfa_split.h (the workspace= / pieces= keywords of
AttentionPrefill).  The caches, the poison and the check are tests/cache_kit.py's; expected values are tests/split_model.py's float64 model
on uniform and on needle queries (needles either side of every piece boundary of every row block, for every forced piece count at
once), every output element and every L of every live row held to its bounds at split_model.MARGIN.

Shapes.  D = 128 bf16, Hq = 8 over 2 K/V heads (row blocks of 32): (n, qn) = (1100, 70) -- three row blocks, the last ragged --, (70, 70)
-- pure causal prefill -- and (333, 37) -- a short queryLengths -- at capacity 70; with a fourth sequence of qn = 0, and with one of
n = 0.  D = 64 f16, G = 1, 200 rows.  D = 256 bf16, G = 8, 40 rows.  Trees: 40 nodes at G = 8 (three row blocks of 16), n = 900.
Pieces forced to 2, 3, 8 (more than the short sequences have tiles: empty pieces) and 64 (piece 0 empty for every row block), and
planned (0: the host plans 2 for the first shape).  NaN / 0x7f in every key at or past a length, in every tile nobody walks, in the rest
of the last page and in the page unnamed entries point to.  The workspace is filled with 0xFF bytes before every launch: NaN in every
slab nobody writes.  Maxima seen on an MI355X: DESIGN.md 4.20."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402
import decode_model as dm  # noqa: E402
import split_model as spm  # noqa: E402
import tree_model as tm  # noqa: E402
from cache_kit import dev, poisoned, same, token_major  # noqa: E402
from metal_flash_attention_amd import AttentionPrefill, GEMMOperandPrecision as P, KVCachePrecision  # noqa: E402

MAIN = ck.Batch(((1100, 70), (70, 70), (333, 37)), 1152, 2, 70)
MAIN_QN0 = ck.Batch(MAIN.SEQS + ((500, 0),), 1152, 2, 70)
MAIN_N0 = ck.Batch(MAIN.SEQS + ((0, 5),), 1152, 2, 70)
WIDE = ck.Batch(((700, 200), (300, 129)), 1024, 2, 200)        # D = 64 f16, G = 1: two row blocks of 128
DEEP = ck.Batch(((900, 40), (70, 40)), 1024, 2, 40)           # D = 256 bf16, G = 8: three row blocks of 16
TREE = ck.Batch(((900, 40), (300, 33), (64, 40)), 1024, 2, 40)     # (caches of 16 tiles: the host plans 2 pieces)
CHAIN = ck.Batch(((900, 16), (300, 9), (10, 16)), 960, 2, 16)   # R = 128 / G: one row block, where a chain and the causal launch walk the same list
FORCED = (2, 3, 8)
SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield
    if SEEN:
        print("\nsplit worst err / bound at margin 1:", {k: round(v, 4) for k, v in SEEN.items()})


def dev_masks(masks):
    t = torch.from_numpy(np.ascontiguousarray(masks).view(np.int64)).cuda()
    return dict(treeMasks=t, treeBatchStride=t.shape[1] if t.dim() == 2 else 0)


def launch(batch, q, k, v, G, *, pieces=None, workspace=True, out=None, cache_kw=None, scales=(None, None), lens=None, planned=None, **named):
    """-> (O, L base-2) (CPU) as the launch left them on sentinel-filled buffers; k, v on the device.  pieces None: the entries without a
    split, chosen by which of `named` are present.  Otherwise the split entries, with a workspace of the size the library names, filled
    with 0xFF bytes (workspace False: none).  planned: the piece count the library must report"""
    _B, Hq, R, D = q.shape
    fp8 = k.dtype == torch.float8_e4m3fn
    op = AttentionPrefill(D, ck.PREC[q.dtype], None if out is None else ck.PREC.get(out, P.FP32), cachePrecision=KVCachePrecision.E4M3 if fp8 else None)
    o = torch.full((batch.B, Hq, R, D), ck.SENT_O, dtype=out or q.dtype, device="cuda")
    l = torch.full((batch.B, Hq, R), ck.SENT_L, dtype=torch.float32, device="cuda")
    kw = dict(cache_kw or {})
    kw.update(rows=R, column=batch.C, heads=Hq, batches=batch.B, headsPerKeyValue=G, causal=True,
              cacheLengths=ck.lengths(batch.LENS) if lens is None else lens, queryLengths=ck.lengths(batch.QLENS))
    kw.update(named)
    if fp8:
        kw.update(keyScale=scales[0], valueScale=scales[1])
    if pieces is not None:
        need, count = op.plannedSplit(pieces=pieces, **kw)
        assert count == (planned if planned is not None else pieces or count)
        assert need == (count * batch.B * Hq * R * (D + 2) * 4 if count > 1 else 0)
        kw.update(pieces=pieces, workspace=torch.full((max(need, 16),), 0xFF, dtype=torch.uint8, device="cuda") if workspace else None)
        form = op.launchForm(**kw)
        assert (("x %d pieces" % count) in form and "attn_prefill16_combine_d%d_" % D in form) == (count > 1 and workspace), form
    op.dispatch(q.cuda(), k, v, o, l, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    return o.cpu(), l.cpu()


@functools.lru_cache(maxsize=None)
def reference(batch, D, dtype, G, W, S, with_logits, fp8, causal=True, qkind="needle", tree=None):
    """(q, sink logits, masks, the UNSPLIT model, needle info), computed once per case and shared; split_model.rechained gives the model of
    a piece count.  The needles sit either side of the boundaries of every count of FORCED at once"""
    k, v, (ks, vs) = ck.base(batch, D, dtype, fp8)
    fmt, Hq, R = dm.fmt_of(dtype), batch.HKV * G, batch.RP
    sink = ck.sink_logits(Hq, D + G) if with_logits else None
    masks = None if tree is None else tm.random_tree(R, np.random.default_rng(D)) if tree == "shared" else tm.per_sequence(tm.random_tree, batch.B, R, D + G)
    info = None
    if qkind == "needle":
        seen = k.float().numpy().astype(np.float64) * (ks[None, :, None, None] if fp8 else 1.0)
        q64, info = spm.needle_queries(seen, batch.LENS, batch.QLENS, Hq, G, R, W, S, fmt, FORCED, masks=masks, page=16)
        q = torch.from_numpy(q64).to(dtype)
        assert torch.equal(q.to(torch.float64), torch.from_numpy(q64))
    else:
        q = (torch.rand(batch.B, Hq, R, D, generator=torch.Generator().manual_seed(D + G + W)) * 2 - 1).to(dtype)
    ref = spm.unsplit_model(q, k.float(), v.float(), batch.LENS, batch.QLENS, G, W, S, sink, causal=causal, masks=masks, kscale=ks, vscale=vs)
    return q, sink, masks, ref, info


def walked_keep(batch, G, W, S, tree, causal=True):
    """[B][C] bool: the keys below each length inside the tiles some row block walks"""
    if not causal:
        return batch.keep()
    if not tree:
        return batch.keep(tiles=ck.walked(batch, "prefill", G, batch.RP, W, S))
    tiles = []
    for n, qn in batch.SEQS:
        out = np.zeros(batch.C // 64, dtype=bool)
        b, _u0, _u1, e, se = AttentionPrefill.treeTileRange(n, min(qn, batch.RP), W, S)
        out[:se] = True
        out[b:e] = True
        tiles.append(out)
    return batch.keep(tiles=tiles)


def case(batch, D, dtype, G, W=0, S=0, with_logits=True, fp8=False, causal=True, qkind="needle", tree=None):
    """-> (q, poisoned K, V on the device, keep, the launch's keywords, and hold(o, l, pieces, out, tag))"""
    k, v, scales = ck.base(batch, D, dtype, fp8)
    q, sink, masks, ref, info = reference(batch, D, dtype, G, W, S, with_logits, fp8, causal, qkind, tree)
    keep = walked_keep(batch, G, W, S, tree is not None, causal)
    named = dict(scales=ck.dev_scales(scales), causal=causal)
    if W or S or with_logits or tree is not None:
        named.update(window=W, sinkTokens=S, sinkLogits=dev(sink))
    if masks is not None:
        named.update(dev_masks(masks))
    rows = tm.blind(masks, batch.LENS, batch.QLENS, batch.RP, W, S) if masks is not None else ck.sink_blind(W, S, causal)
    blind = lambda b, n, qn: np.asarray(rows(b, n, qn), dtype=bool)   # noqa: E731  (qn = 0: an empty array, still of bools)

    def hold(o, l, pieces, out, tag):
        model = spm.rechained(ref, batch.LENS, batch.QLENS, G, W, S, sink, pieces, causal=causal, masks=masks)
        ck.hold(batch, "prefill", o, l, model, dtype, out, info, tag, spm, SEEN, blind, sink)
    return q, k, v, keep, named, hold


@pytest.mark.parametrize("qkind", ["needle", "uniform"])
@pytest.mark.parametrize("pieces", [2, 3, 8, 64, 0])
def test_parity_with_the_model_on_poisoned_caches(pieces, qkind):
    """D = 128 bf16, three row blocks of 32, sink logits bound: with 64 pieces piece 0 of every row block is empty, and the logit still
    joins every row once.  16-bit and FP32 O; L checked"""
    q, k, v, keep, named, hold = case(MAIN, 128, torch.bfloat16, 4, qkind=qkind)
    kd, vd = poisoned(k, keep).cuda(), poisoned(v, keep).cuda()
    count = pieces or 2   # (planned: 18 row blocks aim at 512 workgroups, 18 tiles of 8 give 2 pieces)
    for out in (None, torch.float32):
        o, l = launch(MAIN, q, kd, vd, 4, pieces=pieces, planned=count, out=out, **named)
        hold(o, l, count, out or torch.bfloat16, "D128 bf16 %s pieces %d" % (qkind, pieces))


@pytest.mark.parametrize("batch", [MAIN_QN0, MAIN_N0], ids=["qn0", "n0"])
def test_a_sequence_without_rows_and_one_without_keys(batch):
    q, k, v, keep, named, hold = case(batch, 128, torch.bfloat16, 4)
    o, l = launch(batch, q, poisoned(k, keep).cuda(), poisoned(v, keep).cuda(), 4, pieces=3, **named)
    hold(o, l, 3, torch.bfloat16, "D128 bf16 extra sequence")


@pytest.mark.parametrize("shape", [(WIDE, 64, torch.float16, 1), (DEEP, 256, torch.bfloat16, 8)], ids=["D64", "D256"])
@pytest.mark.parametrize("pieces", [3, 0])
def test_parity_at_the_other_head_dimensions(shape, pieces):
    batch, D, dtype, G = shape
    q, k, v, keep, named, hold = case(batch, D, dtype, G, with_logits=False)
    # (planned: caches of 16 tiles give 2 pieces of 8)
    o, l = launch(batch, q, poisoned(k, keep).cuda(), poisoned(v, keep).cuda(), G, pieces=pieces, planned=pieces or 2, **named)
    hold(o, l, pieces or 2, dtype, "D%d pieces %d" % (D, pieces))


@pytest.mark.parametrize("fp8", [False, True], ids=["16-bit", "e4m3"])
def test_layouts_are_byte_identical_and_inside_the_bounds(fp8):
    """contiguous, token-major and paged 16 (paged 256: the next test, on a cache of whole pages); e4m3 with per-head scales"""
    q, k, v, keep, named, hold = case(MAIN, 128, torch.bfloat16, 4, fp8=fp8)
    kd, vd = poisoned(k, keep), poisoned(v, keep)
    o, l = launch(MAIN, q, kd.cuda(), vd.cuda(), 4, pieces=3, **named)
    hold(o, l, 3, torch.bfloat16, "D128 %s layouts" % ("e4m3" if fp8 else "16-bit"))
    (kt, strides), (vt, _) = token_major(kd), token_major(vd)
    assert same(launch(MAIN, q, kt.cuda(), vt.cuda(), 4, pieces=3, cache_kw=dict(strides=dict(K=strides, V=strides)), **named), (o, l)), "token-major"
    kp, vp, kw = ck.paged_pool(k, v, 16, keep, seed=16)
    assert same(launch(MAIN, q, kp, vp, 4, pieces=3, cache_kw=kw, **named), (o, l)), "paged 16 differs from the contiguous launch"


def test_paged_256_on_a_cache_of_whole_pages():
    batch = ck.Batch(MAIN.SEQS, 1280, 2, 70)
    q, k, v, keep, named, hold = case(batch, 128, torch.bfloat16, 4)
    o, l = launch(batch, q, poisoned(k, keep).cuda(), poisoned(v, keep).cuda(), 4, pieces=3, **named)
    kp, vp, kw = ck.paged_pool(k, v, 256, keep, seed=5)
    assert same(launch(batch, q, kp, vp, 4, pieces=3, cache_kw=kw, **named), (o, l)), "paged 256 differs from the contiguous launch"
    hold(o, l, 3, torch.bfloat16, "D128 paged 256")


def test_e4m3_on_exactly_convertible_values_is_the_16_bit_split_launch_byte_for_byte():
    k8, v8, _scales = ck.base(MAIN, 128, torch.bfloat16, True)
    k16, v16 = k8.float().to(torch.bfloat16), v8.float().to(torch.bfloat16)
    q, _sink, _masks, _ref, _info = reference(MAIN, 128, torch.bfloat16, 4, 0, 0, True, False, True, "uniform")
    keep = MAIN.keep()
    sink = dev(ck.sink_logits(8, 1))
    a = launch(MAIN, q, poisoned(k8, keep).cuda(), poisoned(v8, keep).cuda(), 4, pieces=3, window=0, sinkTokens=0, sinkLogits=sink)
    b = launch(MAIN, q, poisoned(k16, keep).cuda(), poisoned(v16, keep).cuda(), 4, pieces=3, window=0, sinkTokens=0, sinkLogits=sink)
    assert same(a, b)


def test_not_causal():
    q, k, v, keep, named, hold = case(MAIN, 128, torch.bfloat16, 4, with_logits=False, causal=False)
    o, l = launch(MAIN, q, poisoned(k, keep).cuda(), poisoned(v, keep).cuda(), 4, pieces=3, **named)
    hold(o, l, 3, torch.bfloat16, "D128 not causal")


@pytest.mark.parametrize("pieces", [2, 3])
def test_a_window_with_sink_tokens_across_the_zone_seam(pieces):
    """W = 130, S = 4 at n = 1100: a row block's list is the sink tile plus three or four window tiles, with a poisoned gap between them; in
    2 pieces piece 0 crosses the seam, in 3 a piece is the sink tile alone"""
    q, k, v, keep, named, hold = case(MAIN, 128, torch.bfloat16, 4, W=130, S=4)
    assert not keep[0][64:14 * 64].any() and keep[0][:64].all()
    kd, vd = poisoned(k, keep), poisoned(v, keep)
    o, l = launch(MAIN, q, kd.cuda(), vd.cuda(), 4, pieces=pieces, **named)
    hold(o, l, pieces, torch.bfloat16, "D128 window 130 sinks 4")
    kp, vp, kw = ck.paged_pool(k, v, 16, keep, seed=pieces)
    assert same(launch(MAIN, q, kp, vp, 4, pieces=pieces, cache_kw=kw, **named), (o, l)), "paged 16 differs from the contiguous launch"


@pytest.mark.parametrize("tree", ["shared", "per sequence"])
@pytest.mark.parametrize("pieces", [3, 0])
def test_trees(tree, pieces):
    """40 nodes at G = 8: three row blocks of 16 that all walk the tree range's tiles; queryLengths 33 and n < qn beside it"""
    q, k, v, keep, named, hold = case(TREE, 128, torch.bfloat16, 8, tree=tree)
    o, l = launch(TREE, q, poisoned(k, keep).cuda(), poisoned(v, keep).cuda(), 8, pieces=pieces, planned=pieces or 2, **named)
    hold(o, l, pieces or 2, torch.bfloat16, "D128 tree %s pieces %d" % (tree, pieces))


def test_the_chain_mask_is_the_causal_split_launch_byte_for_byte():
    """ONLY for R <= 128 / G, one row block: there the tree range's list is the causal launch's own (with more row blocks an earlier block
    of a tree walks tiles beyond its causal end, its pieces are cut elsewhere, and the merge order differs)"""
    k, v, _ = ck.base(CHAIN, 128, torch.bfloat16, False)
    q = (torch.rand(CHAIN.B, 16, 16, 128, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(torch.bfloat16)
    keep = CHAIN.keep()
    kd, vd = poisoned(k, keep).cuda(), poisoned(v, keep).cuda()
    want = launch(CHAIN, q, kd, vd, 8, pieces=3, window=0, sinkTokens=0, sinkLogits=None)
    for masks in (tm.chain(16), tm.chain(16, CHAIN.B)):
        assert same(launch(CHAIN, q, kd, vd, 8, pieces=3, window=0, sinkTokens=0, sinkLogits=None, **dev_masks(masks)), want)


def test_one_piece_and_no_workspace_are_the_existing_entries_byte_for_byte():
    q, k, v, keep, named, _hold = case(MAIN, 128, torch.bfloat16, 4, W=130, S=4)
    kd, vd = poisoned(k, keep).cuda(), poisoned(v, keep).cuda()
    want = launch(MAIN, q, kd, vd, 4, **named)
    assert same(launch(MAIN, q, kd, vd, 4, pieces=1, **named), want), "pieces = 1"
    assert same(launch(MAIN, q, kd, vd, 4, pieces=3, workspace=False, **named), want), "a NULL workspace"
    assert same(launch(MAIN, q, kd, vd, 4, pieces=0, planned=1, **named), want), "planned: the window's six tiles are one piece"
    plain = {key: val for key, val in named.items() if key not in ("window", "sinkTokens", "sinkLogits")}
    kd, vd = poisoned(k, MAIN.keep()).cuda(), poisoned(v, MAIN.keep()).cuda()
    want = launch(MAIN, q, kd, vd, 4, **plain)
    assert same(launch(MAIN, q, kd, vd, 4, pieces=1, **plain), want), "pieces = 1, the plain entry"
    assert same(launch(MAIN, q, kd, vd, 4, pieces=0, workspace=False, planned=2, **plain), want), "planned in 2 pieces, a NULL workspace"
    tq, tk, tv, tkeep, tnamed, _ = case(TREE, 128, torch.bfloat16, 8, tree="shared")
    tkd, tvd = poisoned(tk, tkeep).cuda(), poisoned(tv, tkeep).cuda()
    assert same(launch(TREE, tq, tkd, tvd, 8, pieces=1, **tnamed), launch(TREE, tq, tkd, tvd, 8, **tnamed)), "pieces = 1, the tree entry"


def test_the_same_launch_twice_is_byte_identical_and_the_workspace_need_not_be_zeroed():
    """no atomics; and a workspace of zeros gives the bits of a workspace of 0xFF bytes: nothing is read that the launch did not write"""
    q, k, v, keep, named, _hold = case(MAIN_N0, 128, torch.bfloat16, 4)
    kd, vd = poisoned(k, keep).cuda(), poisoned(v, keep).cuda()
    first = launch(MAIN_N0, q, kd, vd, 4, pieces=8, **named)
    assert same(launch(MAIN_N0, q, kd, vd, 4, pieces=8, **named), first)
    _B, Hq, R, D = q.shape
    op = AttentionPrefill(D, P.BF16)
    o = torch.full((MAIN_N0.B, Hq, R, D), ck.SENT_O, dtype=torch.bfloat16, device="cuda")
    l = torch.full((MAIN_N0.B, Hq, R), ck.SENT_L, dtype=torch.float32, device="cuda")
    kw = dict(rows=R, column=MAIN_N0.C, heads=Hq, batches=MAIN_N0.B, headsPerKeyValue=4, cacheLengths=ck.lengths(MAIN_N0.LENS),
              queryLengths=ck.lengths(MAIN_N0.QLENS), window=0, sinkTokens=0, sinkLogits=named["sinkLogits"], pieces=8)
    kw["workspace"] = torch.zeros(op.workspaceSize(**kw), dtype=torch.uint8, device="cuda")
    op.dispatch(q.cuda(), kd, vd, o, l, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    assert same((o.cpu(), l.cpu()), first)


def test_a_captured_split_launch_replays_with_new_lengths():
    """one capture of the two kernels in torch.cuda.graph, replayed after cache_lengths changed on the device: the eager result"""
    q, k, v, _keep, named, _hold = case(MAIN, 128, torch.bfloat16, 4, qkind="uniform")
    kd, vd = k.cuda(), v.cuda()   # (every key a value: the lengths change under the capture)
    _B, Hq, R, D = q.shape
    op = AttentionPrefill(D, P.BF16)
    lens = ck.lengths(MAIN.LENS)
    qd = q.cuda()
    o = torch.full((MAIN.B, Hq, R, D), ck.SENT_O, dtype=torch.bfloat16, device="cuda")
    l = torch.full((MAIN.B, Hq, R), ck.SENT_L, dtype=torch.float32, device="cuda")
    kw = dict(rows=R, column=MAIN.C, heads=Hq, batches=MAIN.B, headsPerKeyValue=4, cacheLengths=lens, queryLengths=ck.lengths(MAIN.QLENS),
              window=0, sinkTokens=0, sinkLogits=named["sinkLogits"], pieces=3)
    kw["workspace"] = torch.full((op.workspaceSize(**kw),), 0xFF, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        op.dispatch(qd, kd, vd, o, l, stream=side.cuda_stream, **kw)   # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        op.dispatch(qd, kd, vd, o, l, stream=torch.cuda.current_stream().cuda_stream, **kw)
    for new in ([900, 640, 100], MAIN.LENS):
        lens.copy_(torch.tensor(new, dtype=torch.int32))
        o.fill_(ck.SENT_O)
        l.fill_(ck.SENT_L)
        graph.replay()
        torch.cuda.synchronize()
        got = (o.cpu(), l.cpu())
        batch = ck.Batch(tuple(zip(new, MAIN.QLENS)), MAIN.C, 2, 70)
        assert same(got, launch(batch, q, kd, vd, 4, pieces=3, window=0, sinkTokens=0, sinkLogits=named["sinkLogits"])), new
