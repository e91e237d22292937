"""GPU test: the torch binding of include/mfa_window.h -- flash_decode(..., window=W) and flash_prefill(..., window=W) against
tests/window_model.py under decode_model's per-element bounds, on 16-bit and e4m3 caches, contiguous and paged; window=None is the
existing call bit for bit; one launch of each inside torch.cuda.graph, replayed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import decode_model as dm  # noqa: E402
import window_model as wm  # noqa: E402
from metal_flash_attention_amd import torch_binding as tb  # noqa: E402

SEQS = [(0, 1), (5, 5), (64, 1), (65, 4), (300, 129), (1500, 40), (100, 200)]
LENS, QLENS = [s[0] for s in SEQS], [s[1] for s in SEQS]
B, C, HKV, G, D = len(SEQS), 1536, 2, 4, 128


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def caches(dtype, fp8):
    g = torch.Generator().manual_seed(11 + fp8)
    k, v = ((torch.rand(B, HKV, C, D, generator=g) * 2 - 1) for _ in range(2))
    if fp8:
        rng = np.random.default_rng(5)
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


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("kind,R,W", [("decode", 4, 65), ("decode", 1, 16), ("prefill", 200, 65), ("prefill", 200, 16)])
def test_window_keyword_agrees_with_the_model(kind, R, W, fp8):
    dtype = torch.bfloat16
    k, v, ks, vs = caches(dtype, fp8)
    qlens = None if kind == "decode" else QLENS
    seen = k.float().numpy().astype(np.float64) * (ks[None, :, None, None] if fp8 else 1.0)
    q64, info = wm.needle_queries(seen, LENS, qlens, HKV * G, G, R, W, "bf16")
    q = torch.from_numpy(q64).to(dtype)
    ref = wm.model(q, k.float(), v.float(), LENS, qlens, G, W, kscale=ks, vscale=vs)
    lens = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    kw = dict(window=W, return_lse=True)
    if fp8:
        kw.update(k_scale=torch.from_numpy(ks).cuda(), v_scale=torch.from_numpy(vs).cuda())
    if kind == "prefill":
        kw.update(q_lengths=torch.tensor(QLENS, dtype=torch.int32, device="cuda"))
    fn = tb.flash_decode if kind == "decode" else tb.flash_prefill
    o, lse = fn(q.cuda(), k.cuda(), v.cuda(), lens, **kw)
    wo, wl, text = wm.compare(o.cpu(), lse.cpu(), ref, "bf16", "bf16", LENS, qlens, margin=1, info=info)
    print("%s W %d%s: worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % (kind, W, " e4m3" if fp8 else "", wo, wl))
    assert wo <= wm.MARGIN and wl <= wm.MARGIN, text
    kp, table = paged(k, 16)
    vp, _ = paged(v, 16)
    o2, lse2 = fn(q.cuda(), kp, vp, lens, block_table=table, **kw)
    live = torch.zeros(o.shape[:3], dtype=torch.bool)
    for b, (n, qn) in enumerate(SEQS):
        live[b, :, :R if qlens is None else min(qn, R)] = True
    assert torch.equal(o2.cpu()[live], o.cpu()[live]) and torch.equal(lse2.cpu()[live], lse.cpu()[live])


def test_window_none_is_the_existing_call_bit_for_bit():
    k, v, _, _ = caches(torch.float16, False)
    g = torch.Generator().manual_seed(3)
    lens = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    qlens = torch.tensor(QLENS, dtype=torch.int32, device="cuda")
    kd, vd = k.cuda(), v.cuda()
    q = (torch.rand(B, HKV * G, 4, D, generator=g) * 2 - 1).half().cuda()
    o, lse = tb.flash_decode(q, kd, vd, lens, window=None, return_lse=True)
    o0, l0 = torch.ops.mfa.attention_decode(q, kd, vd, lens, None, True)
    assert torch.equal(o, o0) and torch.equal(lse, l0 * 0.6931471805599453)
    assert not torch.equal(o, tb.flash_decode(q, kd, vd, lens, window=16))   # and a window is not
    q = (torch.rand(B, HKV * G, 200, D, generator=g) * 2 - 1).half().cuda()
    o, lse = tb.flash_prefill(q, kd, vd, lens, q_lengths=qlens, window=None, return_lse=True)
    o0, l0 = torch.ops.mfa.attention_prefill(q, kd, vd, lens, qlens, None, True, None, None)
    for b, (n, qn) in enumerate(SEQS):   # (rows at or past qn are not written)
        assert torch.equal(o[b, :, :qn], o0[b, :, :qn]) and torch.equal(lse[b, :, :qn], l0[b, :, :qn] * 0.6931471805599453)
    with pytest.raises(ValueError, match="needs causal"):
        tb.flash_decode(q[:, :, :1], kd, vd, lens, causal=False, window=5)
    with pytest.raises(ValueError, match="window must be an int"):
        tb.flash_prefill(q, kd, vd, lens, window=0)


def test_windowed_launches_replay_inside_a_graph():
    k, v, _, _ = caches(torch.bfloat16, False)
    g = torch.Generator().manual_seed(4)
    kd, vd = k.cuda(), v.cuda()
    lens = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    qlens = torch.tensor(QLENS, dtype=torch.int32, device="cuda")
    qd = (torch.rand(B, HKV * G, 1, D, generator=g) * 2 - 1).bfloat16().cuda()
    qp = (torch.rand(B, HKV * G, 200, D, generator=g) * 2 - 1).bfloat16().cuda()
    want_d = tb.flash_decode(qd, kd, vd, lens, window=700)          # (three pieces and the combine kernel inside the graph)
    want_p = tb.flash_prefill(qp, kd, vd, lens, q_lengths=qlens, window=65)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got_d = tb.flash_decode(qd, kd, vd, lens, window=700)
        got_p = tb.flash_prefill(qp, kd, vd, lens, q_lengths=qlens, window=65)
    for _ in range(2):
        got_d.zero_()
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got_d, want_d)
    for b, (n, qn) in enumerate(SEQS):
        assert torch.equal(got_p[b, :, :qn], want_p[b, :, :qn])
