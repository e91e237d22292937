"""GPU test: multi-head latent attention prefill over the compressed cache (include/mfa_mla_prefill.h) through the C ABI and through
torch, held per element to the bounds of tests/mla_prefill_model.py for O and for L, on that module's cases (which
tests/test_mla_prefill_sensitivity.py walks on the CPU with the mutants).  Needle queries; NaN in every key that must not be loaded --
past a length, the tail of a last page, pages no table names, the padding of a strided row, a sequence of poison behind the last -- and
in Q's rows at or past qn; O and L lie in larger sentinel-filled allocations, which must keep every sentinel outside the launch's rows,
the rows at or past qn included.  The cache layouts and their poison are tests/test_mla_gpu.py's (cache_of).

Beside the bounds, identities that hold BIT FOR BIT: a launch of at most 32 rows is mfa_attention_mla_decode_launch unsplit; paged is
contiguous; a block of rows is its chunks; queryLengths NULL is queryLengths = rows; a batch is its sequences launched alone."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402
import mla_model as mm  # noqa: E402
import mla_prefill_model as pm  # noqa: E402
import test_mla_gpu as tmg  # noqa: E402
from metal_flash_attention_amd import AttentionMLAPrefill  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPE, PREC, tensor, cache_of = tmg.DTYPE, tmg.PREC, tmg.tensor, tmg.cache_of
SEEN = {}


def launch(case, q64, cache, cache_kw, *, qlens="case"):
    """one launch on sentinel-filled O and L inside larger allocations -> (O [B, H, R, 512], L [B, H, R] base 2) on the host, the rows
    nobody wrote still holding the sentinels.  Q holds NaN in the rows at or past qn.  case["token_major"]: Q and O are [B, R, H, ..]
    allocations seen through strides.  qlens: "case" is the case's (None there: queryLengths NULL), else as given."""
    fmt, H, R, B = case["fmt"], case["H"], case["R"], len(case["lens"])
    qlens = case.get("qlens") if isinstance(qlens, str) else qlens
    live = [R if qlens is None else min(x, R) for x in (case["lens"] if qlens is None else qlens)]
    tm = case.get("token_major", False)
    op = AttentionMLAPrefill(PREC[fmt], PREC[case["out"]])
    q = tensor(q64, fmt)
    for b in range(B):
        q[b, :, live[b]:] = float("nan")
    q = q.permute(0, 2, 1, 3).contiguous().cuda().permute(0, 2, 1, 3) if tm else q.cuda()
    if tm:
        obuf = torch.full((B, R + 2, H + 1, pm.DV + 8), ck.SENT_O, dtype=DTYPE[case["out"]], device="cuda")
        o = obuf[:, :R, :H, :pm.DV].permute(0, 2, 1, 3)
    else:
        obuf = torch.full((B, H + 1, R + 2, pm.DV + 8), ck.SENT_O, dtype=DTYPE[case["out"]], device="cuda")
        o = obuf[:, :H, :R, :pm.DV]
    lbuf = torch.full((B, H + 1, R + 1), ck.SENT_L, dtype=torch.float32, device="cuda")
    l = lbuf[:, :H, :R]
    strides = lambda t: (int(t.stride(2)), int(t.stride(1)), int(t.stride(0)))  # noqa: E731
    kw = dict(rows=R, column=case["C"], heads=H, batches=B, scale=pm.SCALE, causal=case["causal"], cacheLengths=ck.lengths(case["lens"]),
              queryLengths=None if qlens is None else ck.lengths(qlens), lStrides=(int(l.stride(1)), int(l.stride(0))))
    kw.update(cache_kw)
    kw["strides"] = dict(kw.get("strides", {}), Q=strides(q), O=strides(o))
    form = op.launchForm(**kw)
    blocks = -(-H * R // 64)
    assert form.startswith("attn_mla16p_d576_%s (grid %d = %d blocks x %d sequences" % (fmt, B * blocks, blocks, B)), form
    op.dispatch(q, cache, o, l, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    o, l = o.cpu(), l.cpu()
    own = torch.zeros((B, H, R), dtype=torch.bool)
    for b in range(B):
        own[b, :, :live[b]] = True
    # every sentinel outside the launch's rows: the margins of the allocations, and the rows at or past qn
    assert bool((o[~own].float() == ck.SENT_O).all()) and bool((l[~own] == ck.SENT_L).all()), "a row at or past qn was written"
    ob, lb = obuf.cpu(), lbuf.cpu()
    inside = torch.zeros_like(ob, dtype=torch.bool)
    (inside[:, :R, :H, :pm.DV] if tm else inside[:, :H, :R, :pm.DV]).fill_(True)
    assert bool((ob[~inside].float() == ck.SENT_O).all()), "the launch wrote outside O's rows"
    linside = torch.zeros_like(lb, dtype=torch.bool)
    linside[:, :H, :R] = True
    assert bool((lb[~linside] == ck.SENT_L).all()), "the launch wrote outside L's rows"
    return o, l


def hold(tag, case, o, l, ref, written, info, natural=False, sentinels=True):
    """the written rows are the model's; no poison in one; a row without a visible key holds O = 0 and L = -FLT_MAX (natural: torch's L,
    that times ln 2); every element inside the model's bounds at MARGIN.  (Rows nobody wrote: `launch` has checked their sentinels.)"""
    w = torch.from_numpy(written)
    o, l = o.clone(), l.clone()
    if sentinels:
        assert bool((l[~w] == ck.SENT_L).all()), tag + ": rows at or past qn"
    o[~w], l[~w] = 0, 0
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(l).all()), tag + ": poison reached a result"
    blind = w & torch.from_numpy(~np.isfinite(ref.L))
    assert not o[blind].float().any() and bool((l[blind] < -1e38).all() if natural else (l[blind] == -ck.FLT_MAX).all()), tag + ": a row without a key"
    wo, wl, text = mm.compare(o, l if natural else l / ck.LOG2E, ref, case["fmt"], case["out"], pm.seen_lens(case), margin=1, info=info)
    SEEN[tag] = max(SEEN.get(tag, 0.0), wo, wl)
    print("%s: worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % (tag, wo, wl))
    assert wo <= pm.MARGIN and wl <= pm.MARGIN, text


@pytest.mark.parametrize("name", list(pm.CASES))
def test_a_case_lies_inside_the_model_s_bounds(name):
    case, q64, kv64, ref, written, info = pm.inputs(name)
    cache, cache_kw = cache_of(case, kv64)
    o, l = launch(case, q64, cache, cache_kw)
    hold(name, case, o, l, ref, written, info)


@pytest.mark.parametrize("name", ["1 unsplit", "s1 seam inside a head, unsplit"])
def test_at_most_32_rows_is_the_decode_launch_bit_for_bit(name):
    """rows <= 32 and queryLengths NULL: mfa_attention_mla_decode_launch with pieces = 1, O and L"""
    case, _pieces, q64, kv64, _ref, _info = mm.inputs(name)
    assert case["R"] <= 32 and case["pieces"] is None
    cache, cache_kw = cache_of(case, kv64)
    decode = tmg.launch(case, q64, cache, cache_kw, 1)
    prefill = launch(dict(case, qlens=None), q64, cache, cache_kw)
    assert ck.same(decode, prefill), name


@pytest.mark.parametrize("name", ["b2 pages of 16", "a7 pages of 64", "b3 pages of 512, not causal", "b6 a block is half a row, pages of 64"])
def test_paged_is_the_contiguous_launch_byte_for_byte(name):
    case, q64, kv64, _ref, _written, _info = pm.inputs(name)
    assert case["page"]
    pool, pool_kw = cache_of(case, kv64)
    flat, flat_kw = cache_of(dict(case, page=None), kv64)
    assert ck.same(launch(case, q64, pool, pool_kw), launch(case, q64, flat, flat_kw))


@pytest.mark.parametrize("H,fmt", [(5, "bf16"), (128, "f16")])
def test_a_block_of_rows_is_its_chunks_bit_for_bit(H, fmt):
    """one launch of qn = 130 rows over n = 320 keys equals the launches of its rows as chunks of 70 + 48 + 12 with the lengths advanced"""
    n, qn, C = 320, 130, 320
    kv64 = mm.cache_values(fmt, 5, 1, C)
    q64, _info = pm.needle_queries(kv64, (n,), (qn,), H, qn, True, fmt, pm.SCALE)
    case = dict(fmt=fmt, H=H, R=qn, causal=True, page=None, layout="packed", out=fmt, lens=(n,), qlens=(qn,), C=C)
    cache, cache_kw = cache_of(case, kv64)
    whole = launch(case, q64, cache, cache_kw)
    start = 0
    for rows in (70, 48, 12):
        part = dict(case, R=rows, lens=(n - qn + start + rows,), qlens=(rows,))
        o, l = launch(part, q64[:, :, start:start + rows], cache, cache_kw)
        assert ck.same((o, l), (whole[0][:, :, start:start + rows], whole[1][:, :, start:start + rows])), (H, start, rows)
        start += rows
    assert start == qn


def test_query_lengths_null_is_rows_and_a_batch_is_its_sequences():
    case, q64, kv64, ref, written, info = pm.inputs("n1 queryLengths NULL")
    cache, cache_kw = cache_of(case, kv64)
    null = launch(case, q64, cache, cache_kw)
    full = launch(case, q64, cache, cache_kw, qlens=(case["R"],) * len(case["lens"]))
    assert ck.same(null, full)
    past = launch(case, q64, cache, cache_kw, qlens=(case["R"] + 9,) * len(case["lens"]))     # clamped to the capacity
    assert ck.same(null, past)
    case, q64, kv64, ref, written, info = pm.inputs("a2 five heads, a seam inside a row")
    cache, cache_kw = cache_of(case, kv64)
    o, l = launch(case, q64, cache, cache_kw)
    for b, (n, qn) in enumerate(zip(case["lens"], case["qlens"])):
        alone = dict(case, lens=(n,), qlens=(qn,))
        one, one_kw = cache_of(alone, kv64[b:b + 1])
        ob, lb = launch(alone, q64[b:b + 1], one, one_kw)
        assert ck.same((ob, lb), (o[b:b + 1], l[b:b + 1])), b


def _walk(paged, fmt="bf16", H=16, prefix=37, chunks=(70, 48, 32), C=256, page=64):
    """a model's loop through torch: mla_cache_append + flash_mla_prefill over a 150-token prompt in chunks behind a prefix that is in
    the cache already, then one flash_mla_decode step.  -> the rows of the chunked prefill, of the one-shot prefill and of the decode
    step, with the float64 values the model needs"""
    from metal_flash_attention_amd import torch_binding as tb
    B, prompt = 2, sum(chunks)
    total = prefix + prompt + 1
    rng = np.random.default_rng(11)
    kv64 = pm.round_to(rng.uniform(-1.0, 1.0, (B, total, pm.DK)), fmt)
    q64, info = pm.needle_queries(kv64, (prefix + prompt,) * B, (prompt,) * B, H, prompt, True, fmt, pm.SCALE)
    qd64 = pm.round_to(rng.uniform(-1.0, 1.0, (B, H, 1, pm.DK)) / pm.SCALE / 8, fmt)
    kv, q, qd = tensor(kv64, fmt).cuda(), tensor(q64, fmt).cuda(), tensor(qd64, fmt).cuda()
    table = None
    if paged:
        pages = C // page
        cache = torch.full((B * pages + 1, page, pm.DK), float("nan"), dtype=DTYPE[fmt], device="cuda")
        table = torch.from_numpy(np.random.default_rng(3).permutation(B * pages).reshape(B, pages).astype(np.int32)).cuda()
    else:
        cache = torch.full((B, C, pm.DK), float("nan"), dtype=DTYPE[fmt], device="cuda")
    lens = lambda x: torch.full((B,), x, dtype=torch.int32, device="cuda")  # noqa: E731
    append = lambda a, b: tb.mla_cache_append(kv[:, a:b, :512], kv[:, a:b, 512:], cache, lens(b), block_table=table)  # noqa: E731
    append(0, prefix)
    got, start = [], 0
    for rows in chunks:
        a, b = prefix + start, prefix + start + rows
        append(a, b)
        got.append(tb.flash_mla_prefill(q[:, :, start:start + rows], cache, lens(b), softmax_scale=pm.SCALE, block_table=table, return_lse=True))
        start += rows
    chunked = (torch.cat([o for o, _l in got], dim=2).cpu(), torch.cat([l for _o, l in got], dim=2).cpu())
    one_shot = tb.flash_mla_prefill(q, cache, lens(prefix + prompt), softmax_scale=pm.SCALE, block_table=table, return_lse=True)
    append(total - 1, total)
    step = tb.flash_mla_decode(qd, cache, lens(total), softmax_scale=pm.SCALE, block_table=table, return_lse=True)
    torch.cuda.synchronize()
    return dict(kv64=kv64, q64=q64, qd64=qd64, info=info, chunked=chunked, one_shot=tuple(t.cpu() for t in one_shot), step=tuple(t.cpu() for t in step),
                fmt=fmt, H=H, lens=(prefix + prompt,) * B, prompt=prompt, total=total, C=C)


@pytest.mark.parametrize("paged", [False, True])
def test_a_model_walk_appends_prefills_in_chunks_and_decodes(paged):
    w = _walk(paged)
    assert ck.same(w["chunked"], w["one_shot"]), "the prefill rows of the chunked walk are the one-shot prefill's"
    B, fmt = len(w["lens"]), w["fmt"]
    case = dict(fmt=fmt, out=fmt, C=w["C"], lens=w["lens"])
    ref, written = pm.model(w["q64"], w["kv64"], w["lens"], (w["prompt"],) * B, True, pm.SCALE, page=64 if paged else None)
    hold("walk, prefill, paged %s" % paged, case, w["one_shot"][0], w["one_shot"][1], ref, written, w["info"], natural=True, sentinels=False)
    dref = mm.model(w["qd64"], w["kv64"], (w["total"],) * B, True, pm.SCALE)
    wo, wl, text = mm.compare(w["step"][0], w["step"][1], dref, fmt, fmt, (w["total"],) * B, margin=1)
    print("walk, decode step, paged %s: worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % (paged, wo, wl))
    assert wo <= mm.MARGIN and wl <= mm.MARGIN, text


def test_flash_mla_prefill_end_to_end_and_in_a_graph():
    from metal_flash_attention_amd import torch_binding as tb
    name = "b1 five heads"
    case, q64, kv64, ref, written, info = pm.inputs(name)
    B, H, R = len(case["lens"]), case["H"], case["R"]
    cache, _kw = cache_of(case, kv64)
    q = tensor(q64, case["fmt"])
    for b, qn in enumerate(case["qlens"]):
        q[b, :, qn:] = float("nan")
    q = q.cuda()
    lens, qlens = ck.lengths(case["lens"]), ck.lengths(case["qlens"])
    o, lse = tb.flash_mla_prefill(q, cache, lens, softmax_scale=pm.SCALE, q_lengths=qlens, causal=case["causal"], return_lse=True)
    torch.cuda.synchronize()
    assert o.shape == (B, H, R, pm.DV) and o.dtype == q.dtype and lse.shape == (B, H, R) and lse.dtype == torch.float32
    hold("flash_mla_prefill, " + name, case, o.cpu(), lse.cpu(), ref, written, info, natural=True, sentinels=False)
    only = tb.flash_mla_prefill(q, cache, lens, softmax_scale=pm.SCALE, q_lengths=qlens, causal=case["causal"])
    w = torch.from_numpy(written).cuda()
    assert torch.equal(only[w].view(torch.int16), o[w].view(torch.int16))
    # a token-major q [B, R, H, 576] seen as [B, H, R, 576] is read where it lies
    tm = tb.flash_mla_prefill(q.transpose(1, 2).contiguous().transpose(1, 2), cache, lens, softmax_scale=pm.SCALE, q_lengths=qlens)
    assert torch.equal(tm[w].view(torch.int16), o[w].view(torch.int16))
    # captured once, replayed on changed lengths: the launch reads both arrays on the device
    other_lens = ck.lengths([min(n, 200) for n in pm.seen_lens(case)])
    other_qlens = ck.lengths([min(qn, 40) for qn in case["qlens"]])
    want = tb.flash_mla_prefill(q, cache, other_lens, softmax_scale=pm.SCALE, q_lengths=other_qlens, return_lse=True)
    torch.cuda.synchronize()
    s_lens, s_qlens = lens.clone(), qlens.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tb.flash_mla_prefill(q, cache, s_lens, softmax_scale=pm.SCALE, q_lengths=s_qlens, return_lse=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_o, g_lse = tb.flash_mla_prefill(q, cache, s_lens, softmax_scale=pm.SCALE, q_lengths=s_qlens, return_lse=True)
    for new_lens, new_qlens, (w_o, w_lse), rows in ((lens, qlens, (o, lse), case["qlens"]), (other_lens, other_qlens, want, other_qlens.tolist())):
        g_o.fill_(ck.SENT_O)
        g_lse.fill_(ck.SENT_L)
        s_lens.copy_(new_lens)
        s_qlens.copy_(new_qlens)
        graph.replay()
        torch.cuda.synchronize()
        for b, qn in enumerate(rows):
            assert torch.equal(g_o[b, :, :qn].view(torch.int16), w_o[b, :, :qn].view(torch.int16)) and torch.equal(g_lse[b, :, :qn], w_lse[b, :, :qn]), b
            assert bool((g_o[b, :, qn:].float() == ck.SENT_O).all()), "a replay wrote a row at or past qn"


def test_zz_the_worst_ratios_seen():
    """(prints what §4.27 of DESIGN.md quotes: the device's worst err / bound at margin 1 over the cases above)"""
    if SEEN:
        print("worst err / bound at margin 1 over %d launches: %.3f" % (len(SEEN), max(SEEN.values())))
    assert all(v <= pm.MARGIN for v in SEEN.values())
