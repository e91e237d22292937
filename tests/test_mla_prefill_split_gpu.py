"""GPU test: MLA prefill cut along the keys (include/mfa_mla_prefill_split.h) through the C ABI and through torch, on the cases, the
model, the bounds and the MARGIN of tests/mla_prefill_model.py, unchanged: the cut adds at most 2 x 64 + 12 FP32 roundings to a chain
(the combine's weights, products and sums over at most 64 pieces), about 1e-5 relative, against the 2^-9 of the bf16 rounding the bound
is made of.  The workspace is a NaN-filled larger allocation whose tail must survive; O and L lie in sentinel-filled allocations.
Beside the bounds, what holds BIT FOR BIT: one piece, or no workspace, is the unsplit launch; paged is contiguous; a launch whose
blocks have one live piece is the unsplit launch (weight exp2(0) = 1, 0 + 1 x, the same reciprocal)."""
import pytest

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402
import mla_model as mm  # noqa: E402
import mla_prefill_model as pm  # noqa: E402
import test_mla_gpu as tmg  # noqa: E402
import test_mla_prefill_gpu as tpg  # noqa: E402
from metal_flash_attention_amd import AttentionMLAPrefillSplit  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPE, PREC, tensor, cache_of = tmg.DTYPE, tmg.PREC, tmg.tensor, tmg.cache_of
SEEN = {}
TAIL = 64   # floats of sentinel behind the workspace's needed bytes


def launch(case, q64, cache, cache_kw, pieces, *, workspace=True):
    """one launch on sentinel-filled O and L -> (O, L base 2) on the host; NaN in Q's rows at or past qn and in the workspace, whose tail must survive"""
    fmt, H, R, B = case["fmt"], case["H"], case["R"], len(case["lens"])
    qlens = case.get("qlens")
    live = [R if qlens is None else min(x, R) for x in (case["lens"] if qlens is None else qlens)]
    op = AttentionMLAPrefillSplit(PREC[fmt], PREC[case["out"]])
    q = tensor(q64, fmt)
    for b in range(B):
        q[b, :, live[b]:] = float("nan")
    q = q.cuda()
    obuf = torch.full((B, H + 1, R + 2, pm.DV + 8), ck.SENT_O, dtype=DTYPE[case["out"]], device="cuda")
    lbuf = torch.full((B, H + 1, R + 1), ck.SENT_L, dtype=torch.float32, device="cuda")
    o, l = obuf[:, :H, :R, :pm.DV], lbuf[:, :H, :R]
    kw = dict(rows=R, column=case["C"], heads=H, batches=B, scale=pm.SCALE, causal=case["causal"], cacheLengths=ck.lengths(case["lens"]),
              queryLengths=None if qlens is None else ck.lengths(qlens), lStrides=(int(l.stride(1)), int(l.stride(0))), pieces=pieces)
    kw.update(cache_kw)
    kw["strides"] = dict(kw.get("strides", {}), O=(int(o.stride(2)), int(o.stride(1)), int(o.stride(0))))
    blocks, ws = -(-H * R // 64), None
    if workspace:
        need, planned = op.plannedSplit(**kw)
        assert planned == pieces and need == (pieces * B * H * R * (pm.DV + 2) * 4 if pieces > 1 else 0)
        ws = torch.full((need // 4 + TAIL,), float("nan"), dtype=torch.float32, device="cuda")
        ws[need // 4:] = ck.SENT_L
        kw.update(workspace=ws, workspaceBytes=need)
    form = op.launchForm(**kw)
    if workspace and pieces > 1:
        assert form.startswith("attn_mla16pk_d576_%s (grid %d = %d blocks x %d sequences x %d pieces" % (fmt, B * blocks * pieces, blocks, B, pieces)), form
        assert "+ attn_mla16p_d576_%s_combine (grid %d)" % (fmt, -(-B * H * R // 4)) in form, form
    else:
        assert form.startswith("attn_mla16p_d576_%s (grid %d = " % (fmt, B * blocks)), form
    op.dispatch(q, cache, o, l, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    assert ws is None or bool((ws[-TAIL:] == ck.SENT_L).all()), "the launch wrote behind its workspace"
    ob, lb, own = obuf.cpu(), lbuf.cpu(), torch.zeros((B, H + 1, R + 2), dtype=torch.bool)
    for b in range(B):
        own[b, :H, :live[b]] = True
    assert bool((ob[~own].float() == ck.SENT_O).all()) and bool((ob[..., pm.DV:].float() == ck.SENT_O).all()), "the launch wrote outside O's live rows"
    assert bool((lb[~own[:, :, :R + 1]] == ck.SENT_L).all()), "the launch wrote outside L's live rows"
    return o.cpu(), l.cpu()


def hold(tag, case, o, l, ref, written, info, **kw):
    """tests/test_mla_prefill_gpu.py's hold (sentinels, no poison, rows without a key, pm's bounds at pm.MARGIN); the worst ratio is kept here"""
    try:
        tpg.hold(tag, case, o, l, ref, written, info, **kw)
    finally:
        if tag in tpg.SEEN:
            SEEN[tag] = tpg.SEEN.pop(tag)


@pytest.mark.parametrize("name,pieces", [("b1 five heads", 2), ("b1 five heads", 7), ("b1 five heads", 64), ("b2 pages of 16", 7),
                                         ("b6 a block is half a row, pages of 64", 3), ("a3 one head, fp32 out", 5), ("a6 not causal", 4),
                                         ("n1 queryLengths NULL", 2)])
def test_a_cut_case_lies_inside_the_model_s_bounds(name, pieces):
    case, q64, kv64, ref, written, info = pm.inputs(name)
    cache, cache_kw = cache_of(case, kv64)
    o, l = launch(case, q64, cache, cache_kw, pieces)
    hold("%s, %d pieces" % (name, pieces), case, o, l, ref, written, info)


def test_one_piece_or_no_workspace_is_the_unsplit_launch_and_paged_is_contiguous():
    case, q64, kv64, _ref, _written, _info = pm.inputs("b1 five heads")
    cache, cache_kw = cache_of(case, kv64)
    unsplit = tpg.launch(case, q64, cache, cache_kw)
    assert ck.same(unsplit, launch(case, q64, cache, cache_kw, 1)), "one piece"
    assert ck.same(unsplit, launch(case, q64, cache, cache_kw, 4, workspace=False)), "four pieces without a workspace"
    case, q64, kv64, _ref, _written, _info = pm.inputs("b2 pages of 16")
    pool, pool_kw = cache_of(case, kv64)
    flat, flat_kw = cache_of(dict(case, page=None), kv64)
    assert ck.same(launch(case, q64, pool, pool_kw, 7), launch(case, q64, flat, flat_kw, 7)), "paged"


def test_one_live_piece_is_the_unsplit_launch_bit_for_bit():
    """every length <= 32: every block's walk is at most one step, which falls to the last of four pieces; the other three are empty"""
    lens, qlens, H, R = (32, 5, 20, 0), (32, 5, 3, 0), 5, 32
    kv64 = mm.cache_values("bf16", 5, len(lens), 32)
    q64, _info = pm.needle_queries(kv64, lens, qlens, H, R, True, "bf16", pm.SCALE)
    case = dict(fmt="bf16", H=H, R=R, causal=True, page=None, layout="packed", out="bf16", lens=lens, qlens=qlens, C=32)
    cache, cache_kw = cache_of(case, kv64)
    assert ck.same(tpg.launch(case, q64, cache, cache_kw), launch(case, q64, cache, cache_kw, 4))


def test_flash_mla_prefill_split_end_to_end_and_in_a_graph():
    from metal_flash_attention_amd import torch_binding as tb
    name = "b1 five heads"
    case, q64, kv64, ref, written, info = pm.inputs(name)
    cache, _kw = cache_of(case, kv64)
    q = tensor(q64, case["fmt"])
    for b, qn in enumerate(case["qlens"]):
        q[b, :, qn:] = float("nan")
    q, lens, qlens = q.cuda(), ck.lengths(case["lens"]), ck.lengths(case["qlens"])
    run = lambda n, qn, P: tb.flash_mla_prefill_split(q, cache, n, softmax_scale=pm.SCALE, q_lengths=qn, return_lse=True, key_pieces=P)  # noqa: E731
    o, lse = run(lens, qlens, 7)
    torch.cuda.synchronize()
    hold("flash_mla_prefill_split, " + name, case, o.cpu(), lse.cpu(), ref, written, info, natural=True, sentinels=False)
    w = torch.from_numpy(written).cuda()
    one, plain = run(lens, qlens, 1), tb.flash_mla_prefill(q, cache, lens, softmax_scale=pm.SCALE, q_lengths=qlens, return_lse=True)
    assert torch.equal(one[0][w].view(torch.int16), plain[0][w].view(torch.int16)) and torch.equal(one[1][w], plain[1][w])
    # captured once, replayed on changed lengths: the pieces are cut on the device from the lengths
    other_lens = ck.lengths([min(n, 200) for n in pm.seen_lens(case)])
    other_qlens = ck.lengths([min(qn, 40) for qn in case["qlens"]])
    want = run(other_lens, other_qlens, 7)
    torch.cuda.synchronize()
    s_lens, s_qlens = lens.clone(), qlens.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(s_lens, s_qlens, 7)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_o, g_lse = run(s_lens, s_qlens, 7)
    replays = ((lens, qlens, (o, lse), case["qlens"]), (other_lens, other_qlens, want, other_qlens.tolist()), (lens, qlens, (o, lse), case["qlens"]))
    for new_lens, new_qlens, (w_o, w_lse), rows in replays:
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
    """(prints what DESIGN.md 4.28 quotes: the device's worst err / bound at margin 1 over the cut launches above)"""
    if SEEN:
        print("worst err / bound at margin 1 over %d cut launches: %.3f" % (len(SEEN), max(SEEN.values())))
    assert all(v <= pm.MARGIN for v in SEEN.values())
