"""GPU test: the torch binding of include/mfa_sink.h -- flash_decode(..., window=W, sink_tokens=S, sink_logits=t) and the same on
flash_prefill against tests/sink_model.py under decode_model's per-element bounds, on 16-bit and e4m3 caches, contiguous and paged;
the ops exist; sink_tokens=None and sink_logits=None is the existing call bit for bit; the argument checks raise; one launch of each
inside torch.cuda.graph, replayed (where tests/test_window_torch.py has its graph test; that file has no torch.compile trace)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import decode_model as dm  # noqa: E402
import sink_model as sm  # noqa: E402
from metal_flash_attention_amd import torch_binding as tb  # noqa: E402

SEQS = [(0, 1), (5, 5), (200, 40), (700, 129), (1500, 40), (100, 130)]
LENS, QLENS = [s[0] for s in SEQS], [s[1] for s in SEQS]
B, C, HKV, G, D = len(SEQS), 1536, 2, 4, 128


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def caches(dtype, fp8):
    g = torch.Generator().manual_seed(13 + fp8)
    k, v = ((torch.rand(B, HKV, C, D, generator=g) * 2 - 1) for _ in range(2))
    if fp8:
        rng = np.random.default_rng(6)
        return (k * 3).to(torch.float8_e4m3fn), (v * 3).to(torch.float8_e4m3fn), dm.spread_scales(rng, HKV), dm.spread_scales(rng, HKV)
    return k.to(dtype), v.to(dtype), None, None


def paged(t, page):
    """[B, HKV, C, D] -> (pool [B C / page, HKV, page, D] in reversed page order, table)"""
    pps = C // page
    pool = t.view(torch.uint8 if t.dtype == torch.float8_e4m3fn else t.dtype).reshape(B, HKV, pps, page, D).permute(0, 2, 1, 3, 4).reshape(B * pps, HKV, page, D)
    order = torch.arange(B * pps - 1, -1, -1)
    table = torch.empty(B * pps, dtype=torch.int32)
    table[order] = torch.arange(B * pps, dtype=torch.int32)
    return pool[order].contiguous().view(t.dtype).cuda(), table.reshape(B, pps).cuda()


def test_the_ops_exist():
    if not tb._HAVE_SINK_OPS:
        pytest.skip("this torch has no torch.library.custom_op")
    for name in ("attention_decode_sink", "attention_prefill_sink"):
        assert "sink_tokens" in str(getattr(torch.ops.mfa, name).default._schema)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("kind,R,W,S", [("decode", 4, 130, 4), ("decode", 1, 130, 70), ("prefill", 130, 130, 4), ("prefill", 130, 130, 70)])
def test_sink_keywords_agree_with_the_model(kind, R, W, S, fp8):
    dtype = torch.bfloat16
    k, v, ks, vs = caches(dtype, fp8)
    qlens = None if kind == "decode" else QLENS
    seen = k.float().numpy().astype(np.float64) * (ks[None, :, None, None] if fp8 else 1.0)
    q64, info = sm.needle_queries(seen, LENS, qlens, HKV * G, G, R, W, S, "bf16")
    q = torch.from_numpy(q64).to(dtype)
    sink = np.random.default_rng(9).uniform(1.0, 4.0, HKV * G).astype(np.float32)
    ref = sm.model(q, k.float(), v.float(), LENS, qlens, G, W, S, sink, kscale=ks, vscale=vs)
    lens = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    kw = dict(window=W, sink_tokens=S, sink_logits=torch.from_numpy(sink).cuda(), return_lse=True)
    if fp8:
        kw.update(k_scale=torch.from_numpy(ks).cuda(), v_scale=torch.from_numpy(vs).cuda())
    if kind == "prefill":
        kw.update(q_lengths=torch.tensor(QLENS, dtype=torch.int32, device="cuda"))
    fn = tb.flash_decode if kind == "decode" else tb.flash_prefill
    o, lse = fn(q.cuda(), k.cuda(), v.cuda(), lens, **kw)
    live = torch.zeros(o.shape[:3], dtype=torch.bool)
    for b, (n, qn) in enumerate(SEQS):
        live[b, :, :R if qlens is None else min(qn, R)] = True
    oc, lc = o.cpu().float(), lse.cpu()
    oc[~live], lc[~live] = 0.0, 0.0   # (rows at or past q_lengths come back uninitialised)
    wo, wl, text = sm.compare(oc, lc, ref, "bf16", "bf16", LENS, qlens, margin=1, info=info)
    print("%s W %d S %d%s: worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % (kind, W, S, " e4m3" if fp8 else "", wo, wl))
    assert wo <= sm.MARGIN and wl <= sm.MARGIN, text
    kp, table = paged(k, 16)
    vp, _ = paged(v, 16)
    o2, lse2 = fn(q.cuda(), kp, vp, lens, block_table=table, **kw)
    assert torch.equal(o2.cpu()[live], o.cpu()[live]) and torch.equal(lse2.cpu()[live], lse.cpu()[live])


def test_no_sinks_is_the_existing_call_and_the_checks_raise():
    k, v, _, _ = caches(torch.float16, False)
    g = torch.Generator().manual_seed(3)
    lens = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    kd, vd = k.cuda(), v.cuda()
    q = (torch.rand(B, HKV * G, 4, D, generator=g) * 2 - 1).half().cuda()
    logits = torch.full((HKV * G,), 2.0, dtype=torch.float32, device="cuda")
    o, lse = tb.flash_decode(q, kd, vd, lens, window=130, sink_tokens=None, sink_logits=None, return_lse=True)
    o0, l0 = torch.ops.mfa.attention_decode_window(q, kd, vd, lens, None, True, None, None, 130)
    assert torch.equal(o, o0) and torch.equal(lse, l0 * 0.6931471805599453)
    assert not torch.equal(o, tb.flash_decode(q, kd, vd, lens, window=130, sink_tokens=4))
    assert not torch.equal(o, tb.flash_decode(q, kd, vd, lens, window=130, sink_logits=logits))
    with pytest.raises(ValueError, match="sink_tokens needs window"):
        tb.flash_decode(q, kd, vd, lens, sink_tokens=4)
    with pytest.raises(ValueError, match="sink_tokens must be an int"):
        tb.flash_prefill(q, kd, vd, lens, window=130, sink_tokens=0)
    with pytest.raises(ValueError, match="needs causal"):
        tb.flash_decode(q, kd, vd, lens, causal=False, window=5, sink_tokens=4)
    for bad in (logits.double(), logits[:3], logits.repeat(2)[::2]):
        with pytest.raises(ValueError, match="sink_logits must be a contiguous float32"):
            tb.flash_decode(q, kd, vd, lens, sink_logits=bad)
    with pytest.raises(RuntimeError, match="sink_logits must live on q's device"):
        tb.flash_prefill(q, kd, vd, lens, sink_logits=logits.cpu())


def test_sink_launches_replay_inside_a_graph():
    k, v, _, _ = caches(torch.bfloat16, False)
    g = torch.Generator().manual_seed(4)
    kd, vd = k.cuda(), v.cuda()
    lens = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    qlens = torch.tensor(QLENS, dtype=torch.int32, device="cuda")
    logits = torch.linspace(1.0, 3.0, HKV * G, dtype=torch.float32, device="cuda")
    qd = (torch.rand(B, HKV * G, 1, D, generator=g) * 2 - 1).bfloat16().cuda()
    qp = (torch.rand(B, HKV * G, 130, D, generator=g) * 2 - 1).bfloat16().cuda()
    kw = dict(sink_tokens=4, sink_logits=logits)
    want_d = tb.flash_decode(qd, kd, vd, lens, window=640, **kw)          # (three pieces and the combine kernel inside the graph)
    want_p = tb.flash_prefill(qp, kd, vd, lens, q_lengths=qlens, window=130, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got_d = tb.flash_decode(qd, kd, vd, lens, window=640, **kw)
        got_p = tb.flash_prefill(qp, kd, vd, lens, q_lengths=qlens, window=130, **kw)
    for _ in range(2):
        got_d.zero_()
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got_d, want_d)
    for b, (n, qn) in enumerate(SEQS):
        assert torch.equal(got_p[b, :, :qn], want_p[b, :, :qn])
