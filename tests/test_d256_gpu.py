"""GPU test: head dimension 256 over the KV cache through the C ABI -- decode (16-bit and e4m3 caches, split and unsplit, paged and
strided, a window with and without sinks, split and unsplit), prefill (row blocks, paged 16 with a shuffled pool, e4m3, a window
with and without sinks, ragged) and append.

Every comparison with a model goes through decode_model.compare / prefill_model.compare / sink_model.compare at the committed MARGIN,
with the test's own queries and with the needle queries of those modules; the runners and caches are those of tests/decode_kit.py and
tests/cache_kit.py (the decode, the e4m3 and the prefill file's): NaN (16-bit) or 0x7f (e4m3) at and past every length, in page tails and in
pages nobody names; canaries or sentinels around O, L and the workspace.  The shapes are the smallest that reach every path of the
D = 256 kernels: 129 keys give wave 0 a second step and every wave a first, 33 a partial second step, 0 the empty sequence; (700, 513,
65) against column 1024 plan four pieces; a prefill of (5, 70) rows over (150, 70) keys is one row block at G = 1 and several, the last
one partial, at G = 8, over three key tiles.  Worst err / bound seen on an MI355X: DESIGN.md 4.15.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402  (prefill_launch, prefill_hold, prefill_pool: prefill's runners; the ragged append)
import decode_kit as dk  # noqa: E402  (Cache, run, check_against_model: the 16-bit launch's runner and its bounds; Cache8, run8, check: the e4m3 launch's)
import decode_model as dm  # noqa: E402
import prefill_model as pm  # noqa: E402
import ragged_model as rm  # noqa: E402
import sink_model as sm  # noqa: E402
from metal_flash_attention_amd import (AttentionDecode, AttentionDecodeFP8, AttentionPrefill, GEMMOperandPrecision as P, KVCacheAppend,  # noqa: E402
                                       KVCachePrecision)

D = 256
LOG2E = 1.4426950408889634
DTYPE = {P.FP16: torch.float16, P.BF16: torch.bfloat16}
SHORT, C_SHORT = np.array([129, 33, 0], dtype=np.uint32), 192        # unsplit: three tiles plan one piece
LONG, C_LONG = np.array([700, 513, 65], dtype=np.uint32), 1024       # sixteen tiles over at most 24 workgroups: four pieces
GROUPS = [(8, 1, 1), (8, 1, 4), (8, 4, 1), (8, 4, 4), (8, 8, 1), (8, 8, 4), (6, 3, 1)]   # (Hq, G, R): G R = 32, and G R odd
SEEN = {}
W, S = 130, 4                                                        # the window and sink tokens of tests/test_sink_gpu.py


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield
    if SEEN:
        print("\nD = 256 prefill worst err / bound at margin 1:", {k: round(v, 4) for k, v in SEEN.items()})


def launches():
    """(lengths, column, workspace offered, the kernel the launch form must name)"""
    return ((SHORT, C_SHORT, True, "_single"), (LONG, C_LONG, True, "_pieces"), (LONG, C_LONG, False, "_single"))


# ---------------------------------------------------------------------------------------------------------------------- decode
@pytest.mark.parametrize("Hq,G,R", GROUPS)
@pytest.mark.parametrize("prec", [P.BF16, P.FP16])
def test_decode_parity_with_the_float64_model(prec, Hq, G, R):
    tn = "bf16" if prec == P.BF16 else "f16"
    for index, (lens, C, workspace, kernel) in enumerate(launches()):
        q, k, v = dk.make_values(3, Hq, G, R, C, D, DTYPE[prec], seed=256 + 8 * Hq + G + R)
        cache = dk.Cache(k, v, lens, "packed")
        for causal in (True, False):
            out32 = bool((index + causal + R) & 1)
            for name, qq, info in dk.both_inputs(q, k, lens, G, causal, cache, C, workspace):
                o, l, _bits, text = dk.run(qq, cache, G, C, causal=causal, workspace=workspace, out32=out32)
                assert text.startswith("attn_decode16_d256_%s%s (" % (tn, kernel)), text
                assert ("x 4 pieces" in text and "attn_decode16_d256_%s_combine" % tn in text) == (kernel == "_pieces"), text
                dk.check_against_model(f"D=256 {prec.name} Hq={Hq} G={G} R={R} causal={causal} {kernel[1:]} lens={lens.tolist()}{name}", o, l,
                                        qq, k, v, lens, G, causal, out32=out32, pieces=dk.pieces_of(text), info=info)


@pytest.mark.parametrize("Hq,G,R", [(8, 1, 4), (8, 4, 1), (8, 8, 4)])
@pytest.mark.parametrize("prec", [P.BF16, P.FP16])
def test_decode_over_an_e4m3_cache_with_per_head_scales(prec, Hq, G, R):
    tn = "bf16" if prec == P.BF16 else "f16"
    for index, (lens, C, workspace, kernel) in enumerate(launches()):
        q, kb, vb, ks, vs = dk.make_case(3, Hq, G, R, C, D, DTYPE[prec], seed=512 + G + R)
        cache = dk.Cache8(kb, vb, lens, "packed")
        out32 = bool((index + R) & 1)
        for name, qq, info in dk.both_inputs8(q, kb, ks, lens, G, True, cache, C, workspace):
            o, l, _bits, text = dk.run8(qq, cache, G, C, ks, vs, workspace=workspace, out32=out32)
            assert text.startswith("attn_decode8_d256_%s%s (" % (tn, kernel)), text
            dk.check(f"D=256 e4m3 {prec.name} G={G} R={R} {kernel[1:]} lens={lens.tolist()}{name}", o, l, qq, kb, vb, ks, vs, lens, G, True,
                     out32=out32, pieces=dk.pieces_of(text), info=info)


@pytest.mark.parametrize("layout", ["paged:16", "paged:64", "token_major", "fused"])
@pytest.mark.parametrize("fp8", [False, True])
def test_decode_layouts_are_byte_identical_to_packed(fp8, layout):
    """at the same piece count: the planned pieces, and one piece without a workspace"""
    Hq, G, R, prec = 8, 4, 4, P.FP16 if fp8 else P.BF16
    page = int(layout.split(":")[1]) if layout.startswith("paged") else None
    if fp8:
        q, k, v, ks, vs = dk.make_case(3, Hq, G, R, C_LONG, D, DTYPE[prec], seed=77)
        caches = [dk.Cache8(k, v, LONG, how, seed=5) for how in ("packed", layout)]
        inputs = dk.both_inputs8(q, k, ks, LONG, G, True, caches[1], C_LONG, True, page=page)
        run = lambda qq, cache, workspace: dk.run8(qq, cache, G, C_LONG, ks, vs, workspace=workspace)  # noqa: E731
    else:
        q, k, v = dk.make_values(3, Hq, G, R, C_LONG, D, DTYPE[prec], seed=78)
        caches = [dk.Cache(k, v, LONG, how, seed=5) for how in ("packed", layout)]
        inputs = dk.both_inputs(q, k, LONG, G, True, caches[1], C_LONG, True, page=page)
        run = lambda qq, cache, workspace: dk.run(qq, cache, G, C_LONG, workspace=workspace)  # noqa: E731
    for workspace in (True, False):
        for name, qq, info in inputs:
            _o0, l0, b0, t0 = run(qq, caches[0], workspace)
            o1, l1, b1, t1 = run(qq, caches[1], workspace)
            assert t0.replace("contiguous", "paged" if page else "contiguous") == t1 and "_d256_" in t1, (t0, t1)
            assert ("x 4 pieces" in t1) == workspace, t1
            assert torch.equal(b0, b1), f"O differs between the {layout} and the packed cache"
            assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)), f"L differs between the {layout} and the packed cache"
            if workspace and fp8:
                dk.check(f"D=256 e4m3 {layout}{name}", o1, l1, qq, k, v, ks, vs, LONG, G, True, pieces=4, page=page, info=info)
            elif workspace:
                dk.check_against_model(f"D=256 {layout}{name}", o1, l1, qq, k, v, LONG, G, True, pieces=4, page=page, info=info)


# (window, sink tokens, logits, the family's infix, the kernel the plan gives at column 1024 with a workspace): W = 130 spans five tiles
# with its sink tile, which plans one piece whatever is offered; W = 640 spans twelve or thirteen and plans three, as the split case of
# tests/test_sink_gpu.py does
SETTINGS = [(W, S, True, "s", "_single"), (640, S, True, "s", "_pieces"), (640, None, False, "w", "_pieces"), (W, None, False, "w", "_single")]


@pytest.mark.parametrize("setting", range(len(SETTINGS)))
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("dtype,G,R", [(torch.bfloat16, 8, 4), (torch.float16, 1, 1)])
def test_decode_under_a_window_with_and_without_sinks(dtype, G, R, fp8, setting):
    """on the split lengths, with the workspace the plan asks for, through the runners of tests/decode_kit.py
    (poison past every length; canaries around O, L and the workspace): the window, the sink tokens and the
    logits ride in the cache's launch keywords"""
    Wd, Sd, with_logits, infix, kernel = SETTINGS[setting]
    Hkv = 2
    Hq, fmt, lens = Hkv * G, dm.fmt_of(dtype), [int(n) for n in LONG]
    if fp8:
        _q, kb, vb, ks, vs = dk.make_case(3, Hq, G, R, C_LONG, D, dtype, seed=31 + G + setting)
        cache = dk.Cache8(kb, vb, LONG, "packed")
        kvals, vvals = dk.dequantise(kb, dk.ONES(kb)), dk.dequantise(vb, dk.ONES(vb))
        seen = kvals.numpy() * ks.astype(np.float64)[None, :, None, None]
    else:
        _q, kvals, vvals = dk.make_values(3, Hq, G, R, C_LONG, D, dtype, seed=31 + G + setting)
        cache, ks, vs = dk.Cache(kvals, vvals, LONG, "packed"), None, None
        seen = kvals.double().numpy()
    logits = np.random.default_rng(40 + setting).uniform(1.0, 4.0, Hq).astype(np.float32) if with_logits else None
    cache.kw.update(window=Wd)
    if infix == "s":
        cache.kw.update(sinkTokens=Sd, sinkLogits=torch.from_numpy(logits).cuda())
    pieces = dk.planned_pieces((3, Hq, R, D), dtype, cache, G, C_LONG, True, True, AttentionDecodeFP8 if fp8 else AttentionDecode)
    assert (pieces is not None) == (kernel == "_pieces"), pieces
    q64, info = sm.needle_queries(seen, lens, None, Hq, G, R, Wd, Sd or 0, fmt, pieces=pieces, page=16)
    q = torch.from_numpy(q64).to(dtype)
    assert torch.equal(q.to(torch.float64), torch.from_numpy(q64))
    ref = sm.model(q, kvals, vvals, lens, None, G, Wd, Sd or 0, logits, pieces=pieces, kscale=ks, vscale=vs)
    if fp8:
        o, l, _bits, text = dk.run8(q, cache, G, C_LONG, ks, vs, workspace=True)
    else:
        o, l, _bits, text = dk.run(q, cache, G, C_LONG, workspace=True)
    assert text.startswith("attn_decode%s%s_d256_%s%s (" % ("8" if fp8 else "16", infix, fmt, kernel)), text
    if pieces:
        assert "x %d pieces" % pieces in text and "+ attn_decode16_d256_%s_combine (" % fmt in text, text
    wo, wl, where = sm.compare(o, l / LOG2E, ref, fmt, fmt, lens, None, margin=1, info=info)
    print("RATIO %s O16 needles | D=256 decode window %d sinks %s%s G=%d R=%d %s | err / bound at margin 1: O %.3f L %.3f" % (
        fmt, Wd, Sd, " e4m3" if fp8 else "", G, R, kernel[1:], wo, wl))
    assert wo <= sm.MARGIN and wl <= sm.MARGIN, where


@pytest.mark.parametrize("prec,Hq,G,R,causal", [(P.BF16, 32, 8, 1, True), (P.FP16, 8, 4, 4, True), (P.BF16, 8, 1, 2, False)])
def test_decode_agrees_with_the_forward_kernel(prec, Hq, G, R, causal):
    """the parent's only route at this width, on the same buffers; both sides are held to the model's bound and to no number of their own
    beyond what tests/test_decode_gpu.py holds them to"""
    dk.agrees_with_the_forward_kernel(prec, D, Hq, G, R, causal)


# --------------------------------------------------------------------------------------------------------------------- prefill
QLENS, LENS = [5, 70], [150, 70]
PB, PR, PC, HKV = 2, 70, 192, 2


def prefill_values(dtype, G, fp8, seed=0):
    """(q, k, v as the cache holds them with poison at and past each length, the values the model reads, scales)"""
    g = torch.Generator().manual_seed(seed + 11 * G + fp8)
    rnd = lambda *s: torch.rand(*s, generator=g) * 2 - 1  # noqa: E731
    q = rnd(PB, HKV * G, PR, D).to(dtype)
    if fp8:
        k, v = (rnd(PB, HKV, PC, D) * 4).to(torch.float8_e4m3fn), (rnd(PB, HKV, PC, D) * 4).to(torch.float8_e4m3fn)
        kf, vf = k.float(), v.float()
        rng = np.random.default_rng(seed)
        scales = (dm.spread_scales(rng, HKV), dm.spread_scales(rng, HKV))
        kc, vc = k.view(torch.uint8).clone(), v.view(torch.uint8).clone()
    else:
        k, v = rnd(PB, HKV, PC, D).to(dtype), rnd(PB, HKV, PC, D).to(dtype)
        kf, vf, scales = k.float(), v.float(), (None, None)
        kc, vc = k.clone(), v.clone()
    for b, n in enumerate(LENS):
        kc[b, :, n:] = 0x7F if fp8 else float("nan")
        vc[b, :, n:] = 0x7F if fp8 else float("nan")
        kf[b, :, n:] = 0.0
        vf[b, :, n:] = 0.0
    if fp8:
        kc, vc = kc.view(torch.float8_e4m3fn), vc.view(torch.float8_e4m3fn)
    return q, kc, vc, kf, vf, scales


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("G", [1, 8])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_prefill_parity_contiguous_and_paged_16(dtype, G, fp8, causal):
    fmt, Hq = dm.fmt_of(dtype), HKV * G
    q, kc, vc, kf, vf, (ks, vs) = prefill_values(dtype, G, fp8)
    form = AttentionPrefill(D, ck.PREC[dtype], cachePrecision=KVCachePrecision.E4M3 if fp8 else None).launchForm(
        rows=PR, column=PC, heads=Hq, batches=PB, headsPerKeyValue=G, causal=causal, cacheLengths=ck.lengths(LENS))
    blocks = -(-PR // (128 // G))
    assert form.startswith("attn_prefill16_d256_%s%s (" % (fmt, "_e4m3" if fp8 else "")) and "x %d row blocks of %d rows" % (blocks, 128 // G) in form, form
    seen = kf.double().numpy() * (ks[None, :, None, None] if fp8 else 1.0)
    for kind in ("uniform", "needle"):
        info = None
        if kind == "needle":
            q64, info = pm.needle_queries(seen, LENS, QLENS, Hq, G, PR, causal, fmt, page=16)
            q = torch.from_numpy(q64).to(dtype)
            assert torch.equal(q.to(torch.float64), torch.from_numpy(q64))
        ref = pm.model(q, kf, vf, LENS, QLENS, G, causal, kscale=ks, vscale=vs)
        qn = q.clone()
        for b, n in enumerate(QLENS):
            qn[b, :, n:] = float("nan")   # rows nobody owns are never read
        for out in (None, torch.float32):
            o, l = ck.prefill_launch(qn, ck.dev(kc), ck.dev(vc), G, causal, out=out, lens=LENS, qlens=QLENS, fp8=fp8, scales=ck.dev_scales((ks, vs)))
            ck.check_dead_and_empty(o, l, LENS, QLENS)
            ck.prefill_hold(o, l, ref, dtype, out or dtype, info, "D=256 %s %s cache O%s" % (fmt, "e4m3" if fp8 else "16-bit", "32" if out else "16"), LENS, QLENS, SEEN)
            if out is None:
                base = (o, l)
        # paged 16, a shuffled pool: a row of a 16-key group that is read eight rows too low comes from another page's place
        pk, pv, kw = ck.prefill_pool(ck.raw(kc), ck.raw(vc), 16, LENS, 3 + G, 0x7F if fp8 else float("nan"))
        if fp8:
            pk, pv = pk.view(torch.float8_e4m3fn), pv.view(torch.float8_e4m3fn)
        o, l = ck.prefill_launch(qn, pk, pv, G, causal, lens=LENS, qlens=QLENS, fp8=fp8, scales=ck.dev_scales((ks, vs)), cache_kw=kw)
        ck.check_dead_and_empty(o, l, LENS, QLENS)
        assert torch.equal(o.view(torch.int16), base[0].view(torch.int16)) and torch.equal(l, base[1]), "paged 16 differs from the contiguous launch"


def sink_and_ragged_case(dtype, G, fp8, paged, sinks):
    fmt, Hq = dm.fmt_of(dtype), HKV * G
    _q, kc, vc, kf, vf, (ks, vs) = prefill_values(dtype, G, fp8, seed=5)
    seen = kf.double().numpy() * (ks[None, :, None, None] if fp8 else 1.0)
    logits = np.random.default_rng(41).uniform(1.0, 4.0, Hq).astype(np.float32) if sinks else None
    Sp = S if sinks else 0
    q64, info = sm.needle_queries(seen, LENS, QLENS, Hq, G, PR, W, Sp, fmt, page=16)
    q = torch.from_numpy(q64).to(dtype)
    for b, n in enumerate(QLENS):
        q[b, :, n:] = float("nan")
    ref = sm.model(torch.nan_to_num(q.float(), nan=0.0), kf, vf, LENS, QLENS, G, W, Sp, logits, kscale=ks, vscale=vs)
    kw = dict(rows=PR, column=PC, heads=Hq, batches=PB, headsPerKeyValue=G, causal=True, cacheLengths=ck.lengths(LENS), window=W)
    if sinks:
        kw.update(sinkTokens=S, sinkLogits=torch.from_numpy(logits).cuda())
    if fp8:
        kw.update(keyScale=torch.from_numpy(ks).cuda(), valueScale=torch.from_numpy(vs).cuda())
    kd, vd = ck.dev(kc), ck.dev(vc)
    if paged:
        kd, vd, pkw = ck.prefill_pool(ck.raw(kc), ck.raw(vc), 16, LENS, 17, 0x7F if fp8 else float("nan"))
        kw.update(pkw)
    return q, kd, vd, kw, ref, info, fmt


# every one of the sixteen window, sink and ragged prefill kernels: (type, e4m3 cache, sinks) in full, G and the layout in turn
@pytest.mark.parametrize("dtype,G,fp8,paged,sinks", [(torch.bfloat16, 8, False, True, True), (torch.float16, 1, True, False, True),
                                                     (torch.float16, 8, False, False, False), (torch.bfloat16, 1, True, True, False),
                                                     (torch.float16, 1, False, True, True), (torch.bfloat16, 8, True, False, True),
                                                     (torch.bfloat16, 1, False, False, False), (torch.float16, 8, True, True, False)])
def test_prefill_under_a_window_with_sinks_and_the_ragged_identity(dtype, G, fp8, paged, sinks):
    """W = 130 with S = 4 and logits (the sink kernels) or alone (the window kernels), held to sink_model's bound; then the same sequences packed: O and L of the ragged launch are the
    padded launch's byte for byte, with NaN in the Q rows nobody owns"""
    Hq = HKV * G
    q, kd, vd, kw, ref, info, fmt = sink_and_ragged_case(dtype, G, fp8, paged, sinks)
    op = AttentionPrefill(D, ck.PREC[dtype], cachePrecision=KVCachePrecision.E4M3 if fp8 else None)
    stream = torch.cuda.current_stream().cuda_stream
    o = torch.full((PB, Hq, PR, D), ck.SENT_O, dtype=dtype, device="cuda")
    l = torch.full((PB, Hq, PR), ck.SENT_L, dtype=torch.float32, device="cuda")
    padded = dict(kw, queryLengths=ck.lengths(QLENS))
    assert op.launchForm(**padded).startswith("attn_prefill16%s_d256_%s%s (" % ("s" if sinks else "w", fmt, "_e4m3" if fp8 else ""))
    op.dispatch(q.cuda(), kd, vd, o, l, stream=stream, **padded)
    torch.cuda.synchronize()
    o, l = o.cpu(), l.cpu()
    ck.check_dead_and_empty(o, l, LENS, QLENS)
    wo, wl, where = sm.compare(o, l / LOG2E, ref, fmt, fmt, LENS, QLENS, margin=1, info=info)
    print("RATIO %s O16 needles | D=256 prefill window %d sinks %s%s G=%d | err / bound at margin 1: O %.3f L %.3f" % (
        fmt, W, S if sinks else None, " e4m3" if fp8 else "", G, wo, wl))
    assert wo <= sm.MARGIN and wl <= sm.MARGIN, where
    # ragged: rows [0, 5) and [5, 75) of a packed Q with two rows nobody owns behind them
    starts, T = rm.row_starts(QLENS), sum(QLENS) + 2
    qp = torch.full((T, Hq, D), float("nan"), dtype=dtype)
    for b, qn in enumerate(QLENS):
        qp[starts[b]:starts[b] + qn] = q[b, :, :qn].permute(1, 0, 2)
    op_ = torch.full((T, Hq, D), ck.SENT_O, dtype=dtype, device="cuda")
    lp = torch.full((Hq, T), ck.SENT_L, dtype=torch.float32, device="cuda")
    ragged = dict(kw, rowStarts=torch.tensor(starts, dtype=torch.int32, device="cuda"), totalRows=T)
    assert op.launchForm(**ragged).startswith("attn_prefill16r_d256_%s%s (" % (fmt, "_e4m3" if fp8 else ""))
    op.dispatch(qp.cuda(), kd, vd, op_, lp, stream=stream, **ragged)
    torch.cuda.synchronize()
    op_, lp = op_.cpu(), lp.cpu()
    for b, qn in enumerate(QLENS):
        got_o, got_l = op_[starts[b]:starts[b] + qn].permute(1, 0, 2), lp[:, starts[b]:starts[b] + qn]
        assert torch.equal(got_o.contiguous().view(torch.int16), o[b, :, :qn].contiguous().view(torch.int16)), f"sequence {b}: O differs from the padded launch"
        assert torch.equal(got_l.contiguous().view(torch.int32), l[b, :, :qn].contiguous().view(torch.int32)), f"sequence {b}: L differs from the padded launch"
    assert bool((op_[sum(QLENS):].float() == ck.SENT_O).all()) and bool((lp[:, sum(QLENS):] == ck.SENT_L).all()), "a packed row nobody owns was written"


# ---------------------------------------------------------------------------------------------------------------------- append
@pytest.mark.parametrize("prec,R,layout,fp8", [(P.BF16, 4, "contiguous", True), (P.FP16, 1, "paged:16", True), (P.BF16, 1, "paged:16", False),
                                               (P.FP16, 4, "contiguous", False)])
def test_append_writes_exactly_the_named_positions(prec, R, layout, fp8):
    """e4m3: against mfa_kv_quantize_e4m3, the exported contract, element by element; a 16-bit cache: the rows' bits"""
    dk.append_writes_exactly_the_named_positions(prec, D, R, layout, fp8)


@pytest.mark.parametrize("dtype,fp8,paged", [(torch.bfloat16, True, True), (torch.float16, True, False), (torch.float16, False, False),
                                             (torch.bfloat16, False, True)])
def test_ragged_append_is_the_per_sequence_append(dtype, fp8, paged):
    ck.append_is_the_per_sequence_append(ck.RAGGED_BATCH, D, dtype, fp8, paged)


@pytest.mark.parametrize("fp8", [False, True])
def test_append_then_decode_over_the_appended_cache(fp8):
    """four rows per sequence appended to a paged 16 pool that holds the earlier keys, then decode of those rows: the appended keys are
    the rows' causal frontiers, so every one of them is some row's needle"""
    dtype, Hq, G, R, ps, per = torch.bfloat16, 8, 4, 4, 16, 6
    Hkv, B = Hq // G, 3
    lens = np.array([70, 17, 4], dtype=np.uint32)           # after the append; sequence 2 holds nothing before it
    C = per * ps
    g = torch.Generator().manual_seed(90 + fp8)
    hist_k, hist_v = ((torch.randn(B, Hkv, C, D, generator=g)).to(dtype) for _ in range(2))
    rng = np.random.default_rng(12)
    ks, vs = (dm.spread_scales(rng, Hkv), dm.spread_scales(rng, Hkv)) if fp8 else (None, None)
    stored_k = dk.quantise(hist_k, ks) if fp8 else hist_k    # what a cache of this type holds for those rows
    stored_v = dk.quantise(hist_v, vs) if fp8 else hist_v
    pages = B * per + 2
    table = torch.from_numpy(rng.permutation(pages)[:B * per].reshape(B, per).astype(np.int32))
    poison = 0x7F if fp8 else float("nan")
    poolk = torch.full((pages, Hkv, ps, D), poison, dtype=torch.uint8 if fp8 else dtype)
    poolv = poolk.clone()
    for b in range(B):
        for key in range(int(lens[b]) - R):                  # the keys before the append
            poolk[int(table[b, key // ps]), :, key % ps] = stored_k[b, :, key]
            poolv[int(table[b, key // ps]), :, key % ps] = stored_v[b, :, key]
    knew = torch.stack([hist_k[b, :, int(lens[b]) - R:int(lens[b])] for b in range(B)])
    vnew = torch.stack([hist_v[b, :, int(lens[b]) - R:int(lens[b])] for b in range(B)])
    poolk, poolv, tabled = poolk.cuda(), poolv.cuda(), table.cuda()
    lensd = torch.from_numpy(lens.astype(np.int64)).to(torch.int32).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    scales = dict(keyScale=torch.from_numpy(ks).cuda(), valueScale=torch.from_numpy(vs).cuda()) if fp8 else {}
    KVCacheAppend(D, P.BF16, KVCachePrecision.E4M3 if fp8 else None).dispatch(
        knew.cuda(), vnew.cuda(), poolk, poolv, rows=R, heads=Hkv, batches=B, cacheLengths=lensd, pageSize=ps, blockTable=tabled, blockTableStride=per,
        pageStrides=(Hkv * ps * D, Hkv * ps * D), stream=stream, **scales)
    seen_k = dk.dequantise(stored_k, ks) if fp8 else stored_k
    q, info = dk.needle_q(seen_k, lens, Hq, G, R, dtype, True, page=ps)
    assert all(min(r + max(int(lens[b]) - R, 0), int(lens[b]) - 1) in info[(b, h, r)][0] for b in range(B) for h in range(Hq) for r in range(R))
    o = torch.full((B, Hq, R, D), float("nan"), dtype=dtype, device="cuda")
    l = torch.full((B, Hq, R), float("nan"), dtype=torch.float32, device="cuda")
    (AttentionDecodeFP8 if fp8 else AttentionDecode)(D, P.BF16).dispatch(
        q.cuda(), poolk.view(torch.float8_e4m3fn) if fp8 else poolk, poolv.view(torch.float8_e4m3fn) if fp8 else poolv, o, l, rows=R, column=C, heads=Hq,
        batches=B, headsPerKeyValue=G, causal=True, cacheLengths=lensd, pageSize=ps, blockTable=tabled, blockTableStride=per,
        pageStrides=(Hkv * ps * D, Hkv * ps * D), strides=dict(K=(D, ps * D, 0), V=(D, ps * D, 0)), stream=stream, **scales)
    torch.cuda.synchronize()
    if fp8:
        dk.check("D=256 append then decode, e4m3", o.float().cpu(), l.cpu(), q, stored_k, stored_v, ks, vs, lens, G, True, page=ps, info=info)
    else:
        dk.check_against_model("D=256 append then decode, 16-bit", o.float().cpu(), l.cpu(), q, hist_k, hist_v, lens, G, True, page=ps, info=info)
