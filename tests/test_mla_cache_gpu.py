"""GPU test of include/mfa_mla_cache.h: the append of the latent cache, byte for byte against the host's prediction, and MLA decode over
an e4m3 latent cache, held per element to the bounds of tests/mla_fp8_model.py for O and for L on the cases tests/test_mla_fp8_sensitivity.py
walks on the CPU with the mutants.  Poison (the NaN bytes 0x7f / 0xff) in every key that must not be loaded, NaN in the whole workspace,
O and L inside larger sentinel-filled allocations; the paged launch against the contiguous one and one piece against no workspace, bit
for bit; three steps of append + decode through torch into an e4m3 page pool; one captured graph of both.

On the seams: the decode cases of mla_fp8_model.SEAM_CASES (tests/test_mla_gpu.py says what that batch holds and how its caches are
laid out); an append of 40 rows a sequence whose rows cross page seams, start on one, end on the cache's last slot and straddle key 0 and
the capacity; and a decode loop of 36 one-token steps through torch, a 16-bit pool and an e4m3 pool side by side, whose three sequences
grow over the multiples of 16 up to 80."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402
import mla_fp8_model as fm  # noqa: E402
import mla_model as mm  # noqa: E402
import mla_sparse_model as sm  # noqa: E402
from metal_flash_attention_amd import AttentionMLADecodeFP8, GEMMOperandPrecision as P, quantizeE4M3  # noqa: E402
from metal_flash_attention_amd import torch_binding as tb  # noqa: E402

pytestmark = pytest.mark.gpu

E4M3 = torch.float8_e4m3fn
DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
PREC = {"bf16": P.BF16, "f16": P.FP16, "f32": P.FP32}
SEEN = {}


def tensor(x64, fmt):
    t = torch.from_numpy(np.ascontiguousarray(x64)).to(DTYPE[fmt])
    assert torch.equal(t.to(torch.float64), torch.from_numpy(np.ascontiguousarray(x64)))   # the model's values are the kernel's
    return t


def e4m3(bytes_):
    """host uint8 (numpy or tensor) -> a float8_e4m3fn tensor of those bytes"""
    t = torch.from_numpy(np.ascontiguousarray(bytes_)) if isinstance(bytes_, np.ndarray) else bytes_
    return t.view(E4M3)


def scale_of(kvscale):
    """kvScale on the device as entry 0 of a longer array: what a kernel that indexed it by sequence would find is SCALE_TAIL"""
    if kvscale is None:
        return None
    return torch.tensor([kvscale] + 2 * list(fm.SCALE_TAIL), dtype=torch.float32, device="cuda")[:1]


# ------------------------------------------------------------------------------------------------------------------------ the append
A_LENS, A_R, A_C = (700, 2, 0, 1537), 3, 1536   # a row before key 0 (length 2), a row past capacity (1537), an empty sequence
SPECIALS = [0.0, -0.0, 2.0 ** -9, -2.0 ** -9, 3 * 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -11, 7.5 * 2.0 ** -9, 2.0 ** -6, 1.0625, -1.0625, 1.1875,
            17.0, 19.0, 448.0, -448.0, 464.0, 480.0, 500.0, -1e4, float("inf"), -float("inf"), float("nan"), 0.37, 0.37 * 448, 0.37 * 464, 0.37 * 2.0 ** -10]


# ... and across the seams: 40 rows a sequence into 320 keys.  Rows 30 .. 69 start mid-page and cross 32, 48 and 64; 64 .. 103 start on a
# page start (of 16 and of 64); 280 .. 319 end on the last slot of the last page; -23 .. 16 straddle key 0 (23 dropped); 287 .. 326 straddle
# the capacity (7 dropped); the empty sequence drops all 40
S_LENS, S_R, S_C = (70, 104, 320, 17, 327, 0), 40, 320


def append_sources(dtype, lens=A_LENS, R=A_R):
    """latent_new [B, R, 512] and rope_new [B, R, 64] as strided views -- the two parts of fused rows of 576 in an allocation of rows of
    640 -- with zeros, e4m3 subnormals, ties, +-448, values beyond, infinities and NaN among ordinary values"""
    g = torch.Generator().manual_seed(5)
    fused = torch.randn((len(lens), R + 1, 640), generator=g) * 4.0
    spec = torch.tensor(SPECIALS)
    for b in range(len(lens)):
        for r in range(R):
            fused[b, r, 3 * r:3 * r + len(spec)] = spec             # in the latent part
            fused[b, r, 512 + r % 32:512 + r % 32 + len(spec)] = spec.flip(0)  # and in the rotary part
    fused = fused.to(dtype).cuda()
    return fused[:, :R, :512], fused[:, :R, 512:576]


def expected_rows(latent, rope, fp8, kvscale):
    """[B, R, 576] on the host: the bytes (uint8) or the bits (int16) the append writes for every source row"""
    rows = torch.cat([latent, rope], dim=2).cpu()
    if not fp8:
        return rows.contiguous().view(torch.int16)
    scale = 1.0 if kvscale is None else float(np.float32(kvscale))
    flat = rows.float().reshape(-1).tolist()
    return torch.tensor([quantizeE4M3(x, scale) for x in flat], dtype=torch.uint8).reshape(rows.shape)


def append_holds(lens, R, C, layout, fmt, fp8, kvscale):
    """one append into a sentinel-filled allocation -> the rows it had to drop; the WHOLE allocation holds the predicted bytes"""
    dtype = DTYPE[fmt]
    latent, rope = append_sources(dtype, lens, R)
    assert not latent.is_contiguous() and latent.stride(1) == 640 and rope.data_ptr() % 16 == 0
    want_rows = expected_rows(latent, rope, fp8, kvscale)
    raw_dtype, sentinel = (torch.uint8, 0xA5) if fp8 else (torch.int16, 0x5A5A)
    Bn = len(lens)
    paged = layout in ("pages of 16", "pages of 64", "table one page short")
    if paged:
        page = 64 if layout == "pages of 64" else 16
        pps = C // page - (layout == "table one page short")
        perm = np.random.default_rng(3).permutation(Bn * (C // page)).astype(np.int32).reshape(Bn, C // page)
        table = torch.from_numpy(perm).cuda()[:, :pps]                                    # (a view when a page short: handed over contiguous)
        alloc = torch.full((Bn * (C // page) + 1, page, 576), sentinel, dtype=raw_dtype)
        where = lambda b, pos: (int(perm[b, pos // page]), pos % page) if 0 <= pos and pos // page < pps else None  # noqa: E731
    else:
        ld = 640 if layout == "ld640" else 576
        alloc = torch.full((Bn, C + 2, ld), sentinel, dtype=raw_dtype)
        table = None
        where = lambda b, pos: (b, pos) if 0 <= pos < C else None  # noqa: E731
    want = alloc.clone()
    dropped = 0
    for b, n in enumerate(lens):
        for r in range(R):
            at = where(b, n - R + r)
            if at is None:
                dropped += 1
            else:
                want[at[0], at[1], :576] = want_rows[b, r]
    dev = alloc.cuda()
    cache = dev.view(E4M3 if fp8 else dtype)
    cache = cache if paged else cache[:, :C, :576]
    tb.mla_cache_append(latent, rope, cache, ck.lengths(lens), block_table=table, kv_scale=scale_of(kvscale))
    torch.cuda.synchronize()
    assert torch.equal(dev.cpu(), want)   # the whole allocation: no tolerance, no element left out
    return dropped


APPEND_TYPES = [("bf16", False, None), ("f16", False, None), ("bf16", True, None), ("f16", True, 0.37)]


@pytest.mark.parametrize("layout", ["contiguous", "ld640", "pages of 16", "table one page short"])
@pytest.mark.parametrize("fmt,fp8,kvscale", APPEND_TYPES)
def test_the_append_writes_the_predicted_bytes_and_nothing_else(layout, fmt, fp8, kvscale):
    dropped = append_holds(A_LENS, A_R, A_C, layout, fmt, fp8, kvscale)
    # dropped: one row before key 0 (length 2), the empty sequence's three, one past the capacity -- or all three of the page the table lacks
    assert dropped == {"table one page short": 7}.get(layout, 5)


@pytest.mark.parametrize("layout", ["contiguous", "ld640", "pages of 16", "pages of 64"])
@pytest.mark.parametrize("fmt,fp8,kvscale", APPEND_TYPES)
def test_the_append_writes_the_predicted_bytes_and_nothing_else_across_seams(layout, fmt, fp8, kvscale):
    n0, n1, n2, n3, n4, n5 = S_LENS
    assert (n0 - S_R) % 16 and (n0 - S_R) // 16 + 2 <= (n0 - 1) // 16           # mid-page, over at least two seams of 16
    assert (n0 - S_R) // 64 < (n0 - 1) // 64                                      # ... and over one of 64
    assert (n1 - S_R) % 64 == 0 and n2 == S_C and 0 < n3 < S_R and S_C < n4 < S_C + S_R and n5 == 0
    dropped = append_holds(S_LENS, S_R, S_C, layout, fmt, fp8, kvscale)
    assert dropped == (S_R - n3) + (n4 - S_C) + S_R == 23 + 7 + 40


# ------------------------------------------------------------------------------------------------------------------------ the decode
def keep_mask(case):
    return np.stack([np.arange(case["C"]) < n for n in case["lens"]])


def whole_pages(kvb, keep, page, reach):
    """the byte cache [B, C, 576] and keep [B][C] widened with keys nobody keeps to whole pages that cover `reach` keys: ck.pool_host gives
    every page of them that holds no kept key -- the pages past a sequence's last, the empty sequence's whole row -- the page of poison"""
    B, C = keep.shape
    wide = -(-max(C, reach) // page) * page
    kvw = np.zeros((B, wide, kvb.shape[2]), dtype=np.uint8)
    kvw[:, :C] = kvb
    keepw = np.zeros((B, wide), dtype=bool)
    keepw[:, :C] = keep
    return e4m3(kvw), keepw


def poison_bytes(kvb, keep):
    """a copy [B, C, 576] uint8 with 0x7f / 0xff (by key parity) in every key keep [B][C] does not name"""
    out = kvb.copy()
    bad = np.where(np.arange(kvb.shape[1]) % 2, 0xFF, 0x7F).astype(np.uint8)[None, :, None]
    return np.where(keep[:, :, None], out, bad)


def cache_of(case, kvb):
    """the byte cache on the device as the case lays it out, poisoned wherever no sequence may read, and the launch keywords of the layout"""
    layout, page, B, C = case["layout"], case["page"], len(case["lens"]), case["C"]
    if page:                                                              # (a page larger than the column: ONE page a sequence)
        kv, keepw = whole_pages(kvb, keep_mask(case), page, max(case["lens"]))
        pool, _same, table = ck.pool_host(kv[:, None], kv[:, None], page, keepw, seed=page)
        pool = pool[:, 0].contiguous()                                    # [pages, page, 576]
        assert table.shape[1] == -(-max(C, max(case["lens"])) // page) and bool((pool[-1].view(torch.uint8) == 0x7F).all())
        return pool.cuda(), dict(pageSize=page, blockTable=torch.from_numpy(table).cuda(), blockTableStride=table.shape[1])
    if layout == "shared":                                                # one cache for every sequence: batchStride 0
        one = poison_bytes(kvb[:1], (np.arange(C) < max(case["lens"]))[None])
        return e4m3(one).cuda(), dict(strides=dict(KV=(fm.DK, 0, 0)))
    held = poison_bytes(kvb, keep_mask(case))
    if layout == "ld640":                                                 # rows 640 bytes apart in a larger allocation, poison between them
        buf = np.full((B, C + 2, 640), 0xFF, dtype=np.uint8)
        buf[:, :C, :fm.DK] = held
        dev = e4m3(buf).cuda()
        return dev[:, :C, :fm.DK], dict(strides=dict(KV=(640, 0, (C + 2) * 640)))
    buf = np.full((B + 1, C, fm.DK), 0xFF, dtype=np.uint8)                # one more sequence of poison behind the last
    buf[:B] = held
    return e4m3(buf).cuda()[:B], {}


def launch(case, q64, cache, cache_kw, pieces, *, workspace=True):
    """one launch on sentinel-filled O and L that lie inside larger allocations -> (O [B, H, R, 512], L [B, H, R] base 2) on the host.
    pieces: None runs without a workspace; a number is given as it is with a NaN-filled workspace of the size the library asks for"""
    fmt, H, R, B = case["fmt"], case["H"], case["R"], len(case["lens"])
    op = AttentionMLADecodeFP8(PREC[fmt], PREC[case["out"]])
    q = tensor(q64, fmt).cuda()
    obuf = torch.full((B, H + 1, R + 2, fm.DV + 8), ck.SENT_O, dtype=DTYPE[case["out"]], device="cuda")
    lbuf = torch.full((B, H + 1, R + 1), ck.SENT_L, dtype=torch.float32, device="cuda")
    o, l = obuf[:, :H, :R, :fm.DV], lbuf[:, :H, :R]
    kw = dict(rows=R, column=case["C"], heads=H, batches=B, scale=fm.SCALE, causal=case["causal"], cacheLengths=ck.lengths(case["lens"]),
              lStrides=(int(l.stride(1)), int(l.stride(0))), kvScale=scale_of(case["kvscale"]))
    kw.update(cache_kw)
    kw["strides"] = dict(kw.get("strides", {}), O=(int(o.stride(2)), int(o.stride(1)), int(o.stride(0))))
    if pieces is not None and workspace:
        need, planned = op.plannedSplit(pieces=pieces, **kw)
        assert planned == pieces and need == (pieces * B * H * R * (fm.DV + 2) * 4 if pieces > 1 else 0)
        form = op.launchForm(pieces=pieces, workspace=0x1000, workspaceBytes=need, **kw)
        groups = -(-H * R // fm.ROWS)
        if pieces > 1:
            assert form.startswith("attn_mla8_d576_%s_k (grid %d = %d groups x %d sequences x %d pieces" % (case["fmt"], groups * B * pieces, groups, B, pieces)), form
            assert "+ attn_mla16_d576_%s_combine" % case["fmt"] in form
        kw.update(pieces=pieces, workspace=torch.full((max(need, 16) // 4,), float("nan"), dtype=torch.float32, device="cuda"))
    op.dispatch(q, cache, o, l, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    inside = torch.zeros_like(obuf, dtype=torch.bool)
    inside[:, :H, :R, :fm.DV] = True
    assert bool((obuf[~inside].float() == ck.SENT_O).all()), "the launch wrote outside O's rows"
    linside = torch.zeros_like(lbuf, dtype=torch.bool)
    linside[:, :H, :R] = True
    assert bool((lbuf[~linside] == ck.SENT_L).all()), "the launch wrote outside L's rows"
    return o.cpu(), l.cpu()


def hold(tag, fmt, out, lens, o, l, ref, info, natural=False):
    """no poison in a live row; an empty sequence holds O = 0 and L = -FLT_MAX (natural: torch's L, that times ln 2); every element
    inside the model's bounds at MARGIN"""
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(l).all()), tag + ": poison reached a result"
    for b, n in enumerate(lens):
        if n == 0:
            assert not o[b].float().any() and bool((l[b] < -1e38).all() if natural else (l[b] == -ck.FLT_MAX).all()), tag + ": the empty sequence"
    wo, wl, text = fm.compare(o, l if natural else l / ck.LOG2E, ref, fmt, out, lens, margin=1, info=info)
    SEEN[tag] = max(SEEN.get(tag, 0.0), wo, wl)
    print("%s: worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % (tag, wo, wl))
    assert wo <= fm.MARGIN and wl <= fm.MARGIN, text


@pytest.mark.parametrize("name", list(fm.ALL_CASES))
def test_a_case_lies_inside_the_model_s_bounds(name):
    case, pieces, q64, kvb, ref, info = fm.inputs(name)
    cache, cache_kw = cache_of(case, kvb)
    o, l = launch(case, q64, cache, cache_kw, pieces)
    hold("%s (kvScale %s)" % (name, case["kvscale"]), case["fmt"], case["out"], fm.seen_lens(case), o, l, ref, info)


def test_one_piece_with_a_workspace_is_the_launch_without_one():
    for name in ("1 unsplit", "s1 seam inside a head, unsplit", "s5 pages of 64"):   # ... and on the seam batch, contiguous and paged
        case, _pieces, q64, kvb, _ref, _info = fm.inputs(name)
        cache, cache_kw = cache_of(case, kvb)
        assert ck.same(launch(case, q64, cache, cache_kw, None), launch(case, q64, cache, cache_kw, 1)), name


PAGED = [name for name, case in fm.SEAM_CASES.items() if case["page"]]    # pages of 16, 32, 64 and 512, unsplit and in pieces


@pytest.mark.parametrize("name", ["6 pages of 16", "6 pages of 256"] + PAGED)
def test_paged_is_the_contiguous_launch_byte_for_byte(name):
    case, pieces, q64, kvb, _ref, _info = fm.inputs(name)
    pool, pool_kw = cache_of(case, kvb)
    flat, flat_kw = cache_of(dict(case, page=None), kvb)
    assert ck.same(launch(case, q64, pool, pool_kw, pieces), launch(case, q64, flat, flat_kw, pieces))


# ------------------------------------------------------------------------------------------------- append + decode through torch
T_PAGE, T_PAGES, T_H, T_SCALE = 16, 8, 5, 0.37    # 8 pages a sequence: 128 keys


def round_trip_state():
    """three sequences with 33, 0 and 100 keys already in an e4m3 page pool (poison everywhere else), and the logical bytes on the host"""
    lens = [33, 0, 100]
    rng = np.random.default_rng(11)
    logical = fm.cache_bytes()[:3, :T_PAGE * T_PAGES].copy()
    table = rng.permutation(3 * T_PAGES).astype(np.int32).reshape(3, T_PAGES)
    pool = np.full((3 * T_PAGES + 1, T_PAGE, fm.DK), 0x7F, dtype=np.uint8)
    for b, n in enumerate(lens):
        for c in range(n):
            pool[table[b, c // T_PAGE], c % T_PAGE] = logical[b, c]
    return lens, logical, e4m3(pool).cuda(), torch.from_numpy(table).cuda(), table


def test_three_steps_of_append_and_decode_through_torch():
    lens, logical, pool, table_dev, table = round_trip_state()
    scale = scale_of(T_SCALE)
    g = torch.Generator().manual_seed(17)
    for step, R in enumerate((4, 1, 1)):
        latent = (torch.randn((3, R, 512), generator=g) * 0.3).to(torch.bfloat16)
        rope = (torch.randn((3, R, 64), generator=g) * 0.3).to(torch.bfloat16)
        lens = [n + R for n in lens]
        new = expected_rows(latent, rope, True, T_SCALE).numpy()
        for b, n in enumerate(lens):
            logical[b, n - R:n] = new[b]
        lengths = ck.lengths(lens)
        tb.mla_cache_append(latent.cuda(), rope.cuda(), pool, lengths, block_table=table_dev, kv_scale=scale)
        q64, info = mm.needle_queries(fm.values_of(logical, T_SCALE), lens, T_H, R, True, "bf16", fm.SCALE, page=T_PAGE, seed=step)
        o, lse = tb.flash_mla_decode_fp8(tensor(q64, "bf16").cuda(), pool, lengths, softmax_scale=fm.SCALE, kv_scale=scale, block_table=table_dev, return_lse=True)
        torch.cuda.synchronize()
        held = pool.view(torch.uint8).cpu().numpy()
        for b, n in enumerate(lens):   # the pool holds the predicted bytes
            assert all((held[table[b, c // T_PAGE], c % T_PAGE] == logical[b, c]).all() for c in range(n)), (step, b)
        ref = fm.model(q64, logical, T_SCALE, lens, True, fm.SCALE, page=T_PAGE)
        assert o.shape == (3, T_H, R, fm.DV) and o.dtype == torch.bfloat16 and lse.shape == (3, T_H, R)
        hold("round trip, step %d" % step, "bf16", "bf16", lens, o.cpu(), lse.cpu(), ref, info, natural=True)


W_START, W_STEPS, W_TOPK = (14, 0, 47), 36, 96   # 14 grows over 16, 32 and 48; 0 over 16 and 32; 47 over 48, 64 and 80


def test_a_decode_loop_walks_over_the_page_and_step_seams():
    """what a serving loop does: 36 steps of one token a sequence, each an append into a 16-bit pool and into an e4m3 pool (pages of 16,
    permuted tables, poison wherever nothing was written) and then the dense, the e4m3 and the sparse decode over them, against the
    float64 models on needle queries.  Every sequence's length passes multiples of 16 and of 32 -- a last page and a last step exactly
    full, and the first key of a new page and step -- and after every step both pools hold exactly the predicted bytes"""
    assert mm.MARGIN == fm.MARGIN == sm.MARGIN
    lens, cap = list(W_START), T_PAGE * T_PAGES
    ends = [n + W_STEPS for n in lens]
    assert [[m for m in range(16, 128, 16) if a < m <= e] for a, e in zip(lens, ends)] == [[16, 32, 48], [16, 32], [48, 64, 80]] and max(ends) <= W_TOPK
    rng = np.random.default_rng(23)
    g = torch.Generator().manual_seed(31)
    tables = [rng.permutation(3 * T_PAGES).astype(np.int32).reshape(3, T_PAGES) for _ in range(2)]
    bits16 = (torch.rand((3, cap, fm.DK), generator=g) * 2 - 1).to(torch.bfloat16).view(torch.int16).numpy().copy()   # the logical caches
    bytes8 = fm.cache_bytes()[:3, :cap].copy()
    nan16 = int(torch.tensor([float("nan")], dtype=torch.bfloat16).view(torch.int16))
    pools = [np.full((3 * T_PAGES + 1, T_PAGE, fm.DK), nan16, dtype=np.int16), np.full((3 * T_PAGES + 1, T_PAGE, fm.DK), 0x7F, dtype=np.uint8)]
    for pool, table, logical in zip(pools, tables, (bits16, bytes8)):
        for b, n in enumerate(lens):
            for c in range(n):
                pool[table[b, c // T_PAGE], c % T_PAGE] = logical[b, c]
    dev16, dev8 = torch.from_numpy(pools[0]).view(torch.bfloat16).cuda(), e4m3(pools[1]).cuda()
    tab16, tab8 = (torch.from_numpy(t).cuda() for t in tables)
    scale = scale_of(T_SCALE)
    values16 = lambda: torch.from_numpy(bits16).view(torch.bfloat16).to(torch.float64).numpy()  # noqa: E731
    for step in range(W_STEPS):
        latent = (torch.randn((3, 1, 512), generator=g) * 0.3).to(torch.bfloat16)
        rope = (torch.randn((3, 1, 64), generator=g) * 0.3).to(torch.bfloat16)
        lens = [n + 1 for n in lens]
        new16, new8 = expected_rows(latent, rope, False, None).numpy(), expected_rows(latent, rope, True, T_SCALE).numpy()
        for b, n in enumerate(lens):
            bits16[b, n - 1], bytes8[b, n - 1] = new16[b, 0], new8[b, 0]
            pools[0][tables[0][b, (n - 1) // T_PAGE], (n - 1) % T_PAGE] = new16[b, 0]
            pools[1][tables[1][b, (n - 1) // T_PAGE], (n - 1) % T_PAGE] = new8[b, 0]
        lengths = ck.lengths(lens)
        tb.mla_cache_append(latent.cuda(), rope.cuda(), dev16, lengths, block_table=tab16)
        tb.mla_cache_append(latent.cuda(), rope.cuda(), dev8, lengths, block_table=tab8, kv_scale=scale)
        # the lists: every valid position, -1, and positions from the length up to the table's capacity, shuffled
        idx = np.full((3, 1, W_TOPK), sm.HOLE, dtype=np.int64)
        for b, n in enumerate(lens):
            row = np.concatenate([np.arange(n), [n, cap - 1], rng.integers(n, cap, (W_TOPK - n - 2) // 2)])
            idx[b, 0, :len(row)] = row
            rng.shuffle(idx[b, 0])
        kv64 = values16()
        q64, info = mm.needle_queries(kv64, lens, T_H, 1, True, "bf16", mm.SCALE, page=T_PAGE, seed=step)
        q = tensor(q64, "bf16").cuda()
        o, lse = tb.flash_mla_decode(q, dev16, lengths, softmax_scale=mm.SCALE, block_table=tab16, return_lse=True)
        so, slse = tb.flash_mla_sparse_decode(q, dev16, lengths, torch.from_numpy(idx.astype(np.int32)).cuda(), softmax_scale=mm.SCALE,
                                              block_table=tab16, return_lse=True, pieces=1)
        q64f, infof = mm.needle_queries(fm.values_of(bytes8, T_SCALE), lens, T_H, 1, True, "bf16", fm.SCALE, page=T_PAGE, seed=step)
        fo, flse = tb.flash_mla_decode_fp8(tensor(q64f, "bf16").cuda(), dev8, lengths, softmax_scale=fm.SCALE, kv_scale=scale, block_table=tab8,
                                           return_lse=True)
        torch.cuda.synchronize()
        assert np.array_equal(dev16.view(torch.int16).cpu().numpy(), pools[0]), "step %d: the 16-bit pool" % step   # the whole pools, bit for bit
        assert np.array_equal(dev8.view(torch.uint8).cpu().numpy(), pools[1]), "step %d: the e4m3 pool" % step
        ref = mm.model(q64, kv64, lens, True, mm.SCALE, page=T_PAGE)
        hold("decode loop, 16-bit", "bf16", "bf16", lens, o.cpu(), lse.cpu(), ref, info, natural=True)
        # the sparse launch computes the dense attention -- every key once, in another order -- over a chain of W_TOPK slots
        more = np.array([mm.chain_length(W_TOPK, None) - mm.chain_length(n, None) for n in lens]).reshape(3, 1, 1) * mm.U32
        assert (more >= 0).all()
        wide = ref._replace(E=ref.E + more[..., None] * (ref.A + np.abs(ref.O)), EL=ref.EL + more)
        hold("decode loop, sparse", "bf16", "bf16", lens, so.cpu(), slse.cpu(), wide, info, natural=True)
        reff = fm.model(q64f, bytes8, T_SCALE, lens, True, fm.SCALE, page=T_PAGE)
        hold("decode loop, e4m3", "bf16", "bf16", lens, fo.cpu(), flse.cpu(), reff, infof, natural=True)


def test_a_captured_graph_of_append_and_decode_replays_the_eager_result():
    lens, _logical, pool, table_dev, _table = round_trip_state()
    start = pool.clone()
    scale = scale_of(T_SCALE)
    g = torch.Generator().manual_seed(29)
    latent, rope = (torch.randn((3, 2, 512), generator=g) * 0.3).to(torch.float16).cuda(), (torch.randn((3, 2, 64), generator=g) * 0.3).to(torch.float16).cuda()
    q = (torch.randn((3, T_H, 2, fm.DK), generator=g) * 0.5).to(torch.float16).cuda()
    lengths = ck.lengths([n + 2 for n in lens])

    def both():
        tb.mla_cache_append(latent, rope, pool, lengths, block_table=table_dev, kv_scale=scale)
        return tb.flash_mla_decode_fp8(q, pool, lengths, softmax_scale=fm.SCALE, kv_scale=scale, block_table=table_dev, return_lse=True, pieces=2)

    want = both()                                  # eager (and the warm-up outside the capture)
    torch.cuda.synchronize()
    want_pool = pool.clone()
    pool.copy_(start)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                  # a straight chain: append, pieces, combine
        o, lse = both()
    pool.copy_(start)
    o.zero_()
    lse.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(o.view(torch.int16), want[0].view(torch.int16)) and torch.equal(lse, want[1])
    assert torch.equal(pool.view(torch.uint8), want_pool.view(torch.uint8)) and not torch.equal(pool.view(torch.uint8), start.view(torch.uint8))
