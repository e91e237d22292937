"""GPU test: MLA prefill over an e4m3 latent cache (include/mfa_mla_prefill_fp8.h), unsplit and cut along the keys, through the C ABI and
through torch.  Inputs are BYTES (mla_fp8_model.cache_bytes); the launch stands for mla_fp8_model.values_of(bytes, kvScale), the
reference is the float64 mla_prefill_model.model over those values with E widened by (1 + 1 / (DK + 3) + 1 / 48) and EL by
(1 + 1 / (DK + 3)) -- mla_fp8_model's derivation for the two roundings the scale adds -- compared through decode_model at MARGIN 2, the
margin both models fix.  The reference's own worst err / bound at margin 1 (mla_prefill_model.emulated over the dequantised values, on
the CPU): 0.859 (batch B, 5 heads, bf16, kvScale 0.37), 0.610 (f16, 3.0), 0.746 (B2, 128 heads, bf16, none); L 0.001.

Poison is the NaN bytes 0x7f / 0xff in every key that must not be loaded (the layouts of tests/test_mla_cache_gpu.py), NaN in Q's rows at
or past qn and in the workspace; O, L and the workspace's tail are sentinel-filled.  Beside the bounds, BIT FOR BIT: at most 32 rows is the
e4m3 decode launch at one piece; a block of rows is its chunks; paged is contiguous; one piece, or no workspace, is the unsplit launch."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402
import mla_fp8_model as mf  # noqa: E402
import mla_model as mm  # noqa: E402
import mla_prefill_model as pm  # noqa: E402
import test_mla_cache_gpu as tcg  # noqa: E402
import test_mla_prefill_gpu as tpg  # noqa: E402
from metal_flash_attention_amd import AttentionMLAPrefillFP8, AttentionMLAPrefillFP8Split  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPE, PREC, tensor, cache_of, scale_of = tcg.DTYPE, tcg.PREC, tcg.tensor, tcg.cache_of, tcg.scale_of
TAIL = 64   # floats of sentinel behind the workspace's needed bytes


def reference(q64, values, lens, qlens, causal, page=None, shared=False):
    """pm.model over the values the bytes stand for, its bounds widened as mla_fp8_model widens mla_model's"""
    ref, written = pm.model(q64, values, lens, qlens, causal, pm.SCALE, page=page, shared=shared)
    return ref._replace(E=ref.E * (1.0 + 1.0 / (pm.DK + 3) + 1.0 / 48), EL=ref.EL * (1.0 + 1.0 / (pm.DK + 3))), written


def inputs(name, kvscale):
    """a case of pm.CASES restated over a byte cache: (case, q, bytes, Reference, written, needle info)"""
    case = dict(pm.CASES[name], kvscale=kvscale)
    kvb = mf.cache_bytes(0, len(case["lens"]), case["C"])
    values, shared = mf.values_of(kvb, kvscale), case["layout"] == "shared"
    q64, info = pm.needle_queries(values, case["lens"], case["qlens"], case["H"], case["R"], case["causal"], case["fmt"], pm.SCALE,
                                  page=case["page"], shared=shared)
    ref, written = reference(q64, values, case["lens"], case["qlens"], case["causal"], case["page"], shared)
    return case, q64, kvb, ref, written, info


def launch(case, q64, cache, cache_kw, pieces=None, *, workspace=True):
    """one launch on sentinel-filled O and L inside larger allocations -> (O, L base 2) on the host.  pieces None: the unsplit entries;
    a number: the cut entries with a NaN-filled workspace whose sentinel tail must survive (workspace False: without one)"""
    fmt, H, R, B = case["fmt"], case["H"], case["R"], len(case["lens"])
    qlens, tm, cut = case.get("qlens"), case.get("token_major", False), pieces is not None
    live = [R if qlens is None else min(x, R) for x in (case["lens"] if qlens is None else qlens)]
    op = (AttentionMLAPrefillFP8Split if cut else AttentionMLAPrefillFP8)(PREC[fmt], PREC[case["out"]])
    q = tensor(q64, fmt)
    for b in range(B):
        q[b, :, live[b]:] = float("nan")
    q = q.permute(0, 2, 1, 3).contiguous().cuda().permute(0, 2, 1, 3) if tm else q.cuda()
    obuf = torch.full((B, R + 2, H + 1, pm.DV + 8) if tm else (B, H + 1, R + 2, pm.DV + 8), ck.SENT_O, dtype=DTYPE[case["out"]], device="cuda")
    o = obuf[:, :R, :H, :pm.DV].permute(0, 2, 1, 3) if tm else obuf[:, :H, :R, :pm.DV]
    lbuf = torch.full((B, H + 1, R + 1), ck.SENT_L, dtype=torch.float32, device="cuda")
    l = lbuf[:, :H, :R]
    strides = lambda t: (int(t.stride(2)), int(t.stride(1)), int(t.stride(0)))  # noqa: E731
    kw = dict(rows=R, column=case["C"], heads=H, batches=B, scale=pm.SCALE, causal=case["causal"], cacheLengths=ck.lengths(case["lens"]),
              queryLengths=None if qlens is None else ck.lengths(qlens), lStrides=(int(l.stride(1)), int(l.stride(0))),
              kvScale=scale_of(case["kvscale"]))
    kw.update(cache_kw)
    kw["strides"] = dict(kw.get("strides", {}), Q=strides(q), O=strides(o))
    blocks, ws = -(-H * R // 64), None
    if cut:
        kw.update(pieces=pieces)
        if workspace:
            need, planned = op.plannedSplit(**kw)
            assert planned == pieces and need == (pieces * B * H * R * (pm.DV + 2) * 4 if pieces > 1 else 0)
            ws = torch.full((need // 4 + TAIL,), float("nan"), dtype=torch.float32, device="cuda")
            ws[need // 4:] = ck.SENT_L
            kw.update(workspace=ws, workspaceBytes=need)
    form = op.launchForm(**kw)
    if cut and workspace and pieces > 1:
        assert form.startswith("attn_mla8pk_d576_%s (grid %d = %d blocks x %d sequences x %d pieces" % (fmt, B * blocks * pieces, blocks, B, pieces)), form
        assert "+ attn_mla8p_d576_%s_combine (grid %d)" % (fmt, -(-B * H * R // 4)) in form, form
    else:
        assert form.startswith("attn_mla8p_d576_%s (grid %d = %d blocks x %d sequences" % (fmt, B * blocks, blocks, B)), form
    op.dispatch(q, cache, o, l, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    assert ws is None or bool((ws[-TAIL:] == ck.SENT_L).all()), "the launch wrote behind its workspace"
    o, l = o.cpu(), l.cpu()
    own = torch.zeros((B, H, R), dtype=torch.bool)
    for b in range(B):
        own[b, :, :live[b]] = True
    assert bool((o[~own].float() == ck.SENT_O).all()) and bool((l[~own] == ck.SENT_L).all()), "a row at or past qn was written"
    ob, lb = obuf.cpu(), lbuf.cpu()
    inside = torch.zeros_like(ob, dtype=torch.bool)
    (inside[:, :R, :H, :pm.DV] if tm else inside[:, :H, :R, :pm.DV]).fill_(True)
    assert bool((ob[~inside].float() == ck.SENT_O).all()), "the launch wrote outside O's rows"
    lb[:, :H, :R] = ck.SENT_L
    assert bool((lb == ck.SENT_L).all()), "the launch wrote outside L's rows"
    return o, l


PARITY = ["b1 five heads", "b2 pages of 16", "b6 a block is half a row, pages of 64", "b4 one head, token-major, fp32 out", "a6 not causal",
          "a9 rows 640 apart, token-major Q and O", "n1 queryLengths NULL"]


@pytest.mark.parametrize("name,kvscale", [(name, mf.KV_SCALES[i % 3]) for i, name in enumerate(PARITY)])
def test_a_case_lies_inside_the_model_s_bounds(name, kvscale):
    case, q64, kvb, ref, written, info = inputs(name, kvscale)
    cache, cache_kw = cache_of(case, kvb)
    o, l = launch(case, q64, cache, cache_kw)
    tpg.hold("%s (kvScale %s)" % (name, kvscale), case, o, l, ref, written, info)


@pytest.mark.parametrize("name,pieces,kvscale", [("b1 five heads", 2, 0.37), ("b1 five heads", 7, 3.0), ("b2 pages of 16", 7, 0.37)])
def test_a_cut_case_lies_inside_the_model_s_bounds(name, pieces, kvscale):
    case, q64, kvb, ref, written, info = inputs(name, kvscale)
    cache, cache_kw = cache_of(case, kvb)
    o, l = launch(case, q64, cache, cache_kw, pieces)
    tpg.hold("%s, %d pieces (kvScale %s)" % (name, pieces, kvscale), case, o, l, ref, written, info)


def test_at_most_32_rows_is_the_e4m3_decode_launch_bit_for_bit():
    """rows <= 32 and queryLengths NULL: mfa_attention_mla_decode_fp8_launch at one piece, O and L"""
    lens, H, R, C = (96, 33, 5, 0), 5, 6, 96
    kvb = mf.cache_bytes(0, len(lens), C)
    q64, _info = mm.needle_queries(mf.values_of(kvb, 0.37), lens, H, R, True, "bf16", pm.SCALE)
    case = dict(fmt="bf16", H=H, R=R, causal=True, page=None, layout="packed", out="bf16", lens=lens, qlens=None, C=C, kvscale=0.37)
    cache, cache_kw = cache_of(case, kvb)
    assert ck.same(tcg.launch(case, q64, cache, cache_kw, 1), launch(case, q64, cache, cache_kw))


def test_a_block_of_rows_is_its_chunks_bit_for_bit():
    """one launch of qn = 130 rows over n = 320 keys equals the launches of its rows as chunks of 70 + 48 + 12 with the lengths advanced"""
    n, qn, C, H = 320, 130, 320, 5
    kvb = mf.cache_bytes(0, 1, C)
    q64, _info = pm.needle_queries(mf.values_of(kvb, 3.0), (n,), (qn,), H, qn, True, "f16", pm.SCALE)
    case = dict(fmt="f16", H=H, R=qn, causal=True, page=None, layout="packed", out="f16", lens=(n,), qlens=(qn,), C=C, kvscale=3.0)
    cache, cache_kw = cache_of(case, kvb)
    whole = launch(case, q64, cache, cache_kw)
    start = 0
    for rows in (70, 48, 12):
        part = dict(case, R=rows, lens=(n - qn + start + rows,), qlens=(rows,))
        got = launch(part, q64[:, :, start:start + rows], cache, cache_kw)
        assert ck.same(got, (whole[0][:, :, start:start + rows], whole[1][:, :, start:start + rows])), (start, rows)
        start += rows


def test_paged_is_contiguous_and_one_piece_or_no_workspace_is_the_unsplit_launch():
    case, q64, kvb, _ref, _written, _info = inputs("b2 pages of 16", 0.37)
    pool, pool_kw = cache_of(case, kvb)
    flat, flat_kw = cache_of(dict(case, page=None), kvb)
    assert ck.same(launch(case, q64, pool, pool_kw), launch(case, q64, flat, flat_kw)), "paged, unsplit"
    assert ck.same(launch(case, q64, pool, pool_kw, 7), launch(case, q64, flat, flat_kw, 7)), "paged, 7 pieces"
    case, q64, kvb, _ref, _written, _info = inputs("b1 five heads", 0.37)
    cache, cache_kw = cache_of(case, kvb)
    unsplit = launch(case, q64, cache, cache_kw)
    assert ck.same(unsplit, launch(case, q64, cache, cache_kw, 1)), "one piece"
    assert ck.same(unsplit, launch(case, q64, cache, cache_kw, 4, workspace=False)), "four pieces without a workspace"


def test_append_prefill_in_chunks_decode_and_a_graph_through_torch():
    """a serving loop over an e4m3 cache: mla_cache_append of a 150-token prompt behind a prefix, flash_mla_prefill_fp8 in chunks and in
    one shot, a flash_mla_decode_fp8 step, and one capture replayed on changed lengths"""
    from metal_flash_attention_amd import torch_binding as tb
    B, H, prefix, chunks, C, fmt, kvscale = 2, 16, 37, (70, 48, 32), 256, "bf16", 0.37
    prompt = sum(chunks)
    total = prefix + prompt + 1
    rng = np.random.default_rng(11)
    src = tensor(pm.round_to(rng.uniform(-1.0, 1.0, (B, total, pm.DK)), fmt), fmt).cuda()
    scale = scale_of(kvscale)
    cache = tcg.e4m3(np.full((B, C, pm.DK), 0x7F, dtype=np.uint8)).cuda()
    lens = lambda x: torch.full((B,), x, dtype=torch.int32, device="cuda")  # noqa: E731
    append = lambda a, b: tb.mla_cache_append(src[:, a:b, :512], src[:, a:b, 512:], cache, lens(b), kv_scale=scale)  # noqa: E731
    append(0, prefix + prompt)
    kvb = cache.view(torch.uint8).cpu().numpy()                  # the bytes the append wrote (poison behind them)
    values = mf.values_of(np.where(np.arange(C)[None, :, None] < prefix + prompt, kvb, 0), kvscale)
    q64, info = pm.needle_queries(values, (prefix + prompt,) * B, (prompt,) * B, H, prompt, True, fmt, pm.SCALE)
    q = tensor(q64, fmt).cuda()
    run = lambda qq, n, **kw: tb.flash_mla_prefill_fp8(qq, cache, n, softmax_scale=pm.SCALE, kv_scale=scale, return_lse=True, **kw)  # noqa: E731
    got, start = [], 0
    for rows in chunks:
        got.append(run(q[:, :, start:start + rows], lens(prefix + start + rows)))
        start += rows
    one_shot = run(q, lens(prefix + prompt))
    assert ck.same((torch.cat([o for o, _l in got], dim=2).cpu(), torch.cat([l for _o, l in got], dim=2).cpu()), tuple(t.cpu() for t in one_shot))
    ref, written = reference(q64, values, (prefix + prompt,) * B, (prompt,) * B, True)
    case = dict(fmt=fmt, out=fmt, C=C, lens=(prefix + prompt,) * B)
    tpg.hold("walk, e4m3 prefill", case, one_shot[0].cpu(), one_shot[1].cpu(), ref, written, info, natural=True, sentinels=False)
    append(total - 1, total)
    qd64 = pm.round_to(rng.uniform(-1.0, 1.0, (B, H, 1, pm.DK)) / pm.SCALE / 8, fmt)
    step = tb.flash_mla_decode_fp8(tensor(qd64, fmt).cuda(), cache, lens(total), softmax_scale=pm.SCALE, kv_scale=scale, return_lse=True)
    kvb = cache.view(torch.uint8).cpu().numpy()
    dref = mf.model(qd64, np.where(np.arange(C)[None, :, None] < total, kvb, 0).astype(np.uint8), kvscale, (total,) * B, True, pm.SCALE)
    tcg.hold("walk, e4m3 decode step", fmt, fmt, (total,) * B, step[0].cpu(), step[1].cpu(), dref, None, natural=True)
    # captured once (the cut launch: two kernels), replayed on changed lengths: the launch reads both arrays on the device
    states = [(lens(prefix + prompt), lens(prompt)), (lens(90), lens(40)), (lens(prefix + prompt), lens(prompt))]
    wants = [run(q, n, q_lengths=qn, key_pieces=3) for n, qn in states]
    torch.cuda.synchronize()
    s_lens, s_qlens = states[0][0].clone(), states[0][1].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_o, g_lse = run(q, s_lens, q_lengths=s_qlens, key_pieces=3)
    for (n, qn), (w_o, w_lse) in zip(states, wants):
        g_o.fill_(ck.SENT_O)
        g_lse.fill_(ck.SENT_L)
        s_lens.copy_(n)
        s_qlens.copy_(qn)
        graph.replay()
        torch.cuda.synchronize()
        rows = int(qn[0])
        assert torch.equal(g_o[:, :, :rows].view(torch.int16), w_o[:, :, :rows].view(torch.int16)) and torch.equal(g_lse[:, :, :rows], w_lse[:, :, :rows])
        assert bool((g_o[:, :, rows:].float() == ck.SENT_O).all()), "a replay wrote a row at or past qn"
