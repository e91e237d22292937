"""GPU test: the torch functions at head dimension 256 -- flash_decode, flash_prefill, flash_prefill_ragged, kv_cache_append and
kv_cache_append_ragged, 16-bit and e4m3 caches with k_scale= / v_scale=, and append + decode replayed from one captured graph.  The
binding does not look at the head dimension: what these cases show is that the library behind it serves D = 256 (before it did, each
of them raised on the unsupported head dimension).  Bounds: tests/decode_model.py and tests/prefill_model.py at their MARGIN."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import decode_model as dm  # noqa: E402
import prefill_model as pm  # noqa: E402
from metal_flash_attention_amd import torch_binding as tb  # noqa: E402

D, HKV, G = 256, 2, 4
HQ = HKV * G
LENS, C = [700, 513, 65], 1024     # decode: four pieces at this column
B = len(LENS)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield


def caches(dtype, fp8, seed=0, lens=LENS):
    """(k, v as the cache holds them (CPU): NaN or 0x7f at and past every length; the values they stand for without the scales
    (float32, zeros there); scales or None)"""
    g = torch.Generator().manual_seed(seed + fp8)
    rnd = lambda: torch.rand(B, HKV, C, D, generator=g) * 2 - 1  # noqa: E731
    if fp8:
        k, v = (rnd() * 3).to(torch.float8_e4m3fn), (rnd() * 3).to(torch.float8_e4m3fn)
        rng = np.random.default_rng(seed)
        scales = (dm.spread_scales(rng, HKV), dm.spread_scales(rng, HKV))
    else:
        k, v, scales = rnd().to(dtype), rnd().to(dtype), (None, None)
    kf, vf = k.float(), v.float()
    kc, vc = (k.view(torch.uint8).clone(), v.view(torch.uint8).clone()) if fp8 else (k.clone(), v.clone())
    for b, n in enumerate(lens):
        kc[b, :, n:] = 0x7F if fp8 else float("nan")
        vc[b, :, n:] = 0x7F if fp8 else float("nan")
        kf[b, :, n:] = 0.0
        vf[b, :, n:] = 0.0
    if fp8:
        kc, vc = kc.view(torch.float8_e4m3fn), vc.view(torch.float8_e4m3fn)
    return kc, vc, kf, vf, scales


def on_device(scales):
    return dict(k_scale=torch.from_numpy(scales[0]).cuda(), v_scale=torch.from_numpy(scales[1]).cuda()) if scales[0] is not None else {}


@pytest.mark.parametrize("dtype,fp8,R", [(torch.bfloat16, False, 1), (torch.float16, True, 4)])
def test_flash_decode(dtype, fp8, R):
    fmt = dm.fmt_of(dtype)
    kc, vc, kf, vf, (ks, vs) = caches(dtype, fp8)
    lens = np.array(LENS, dtype=np.uint32)
    seen = kf.double().numpy() * (ks[None, :, None, None] if fp8 else 1.0)
    q64, info = dm.needle_queries(seen, lens, HQ, G, R, True, fmt, pieces=4)
    q = torch.from_numpy(q64).to(dtype)
    o, lse = tb.flash_decode(q.cuda(), kc.cuda(), vc.cuda(), torch.tensor(LENS, dtype=torch.int32, device="cuda"), return_lse=True, **on_device((ks, vs)))
    torch.cuda.synchronize()
    assert o.shape == (B, HQ, R, D) and o.dtype == dtype and bool(torch.isfinite(o.float()).all())
    ref = dm.model(q, kf, vf, lens, G, True, pieces=4, kscale=ks, vscale=vs)
    wo, wl, text = dm.compare(o.cpu(), lse.cpu(), ref, fmt, fmt, lens, info=info, pieces=4)
    assert wo <= 1.0 and wl <= 1.0, text   # (the margin is inside the bound compare() divides by)


@pytest.mark.parametrize("dtype,fp8", [(torch.float16, False), (torch.bfloat16, True)])
def test_flash_prefill_and_the_ragged_form(dtype, fp8):
    fmt, R = dm.fmt_of(dtype), 70
    qlens, lens = [5, 70, 33], [150, 70, 65]
    kc, vc, kf, vf, (ks, vs) = caches(dtype, fp8, seed=3, lens=lens)
    seen = kf.double().numpy() * (ks[None, :, None, None] if fp8 else 1.0)
    q64, info = pm.needle_queries(seen, lens, qlens, HQ, G, R, True, fmt)
    q = torch.from_numpy(q64).to(dtype)
    kd, vd = kc.cuda(), vc.cuda()
    dl, dq = torch.tensor(lens, dtype=torch.int32, device="cuda"), torch.tensor(qlens, dtype=torch.int32, device="cuda")
    o, lse = tb.flash_prefill(q.cuda(), kd, vd, dl, q_lengths=dq, return_lse=True, **on_device((ks, vs)))
    torch.cuda.synchronize()
    ref = pm.model(q, kf, vf, lens, qlens, G, True, kscale=ks, vscale=vs)
    wo, wl, text = pm.compare(o.cpu(), lse.cpu(), ref, fmt, fmt, lens, qlens, margin=1, info=info)
    assert wo <= pm.MARGIN and wl <= pm.MARGIN, text
    # the same sequences packed: byte for byte
    starts = [0] + [int(x) for x in np.cumsum(qlens)]
    qp = torch.cat([q[b, :, :qn].permute(1, 0, 2) for b, qn in enumerate(qlens)]).contiguous()
    assert bool(torch.isfinite(torch.stack([o[b, :, :qn].float().abs().max() for b, qn in enumerate(qlens)])).all()), "poison reached a live row"
    op, lp = tb.flash_prefill_ragged(qp.cuda(), kd, vd, dl, torch.tensor(starts, dtype=torch.int32, device="cuda"), max(qlens), return_lse=True,
                                     **on_device((ks, vs)))
    torch.cuda.synchronize()
    assert op.shape == (sum(qlens), HQ, D) and lp.shape == (HQ, sum(qlens))
    for b, qn in enumerate(qlens):
        assert torch.equal(op[starts[b]:starts[b] + qn].permute(1, 0, 2), o[b, :, :qn]), f"sequence {b}: O differs from the padded form"
        assert torch.equal(lp[:, starts[b]:starts[b] + qn], lse[b, :, :qn]), f"sequence {b}: L differs from the padded form"


@pytest.mark.parametrize("fp8", [False, True])
def test_appends_and_a_graph_of_append_plus_decode(fp8):
    """kv_cache_append_ragged writes what kv_cache_append writes; then one generation step -- append a row, decode it -- captured once
    and replayed after the lengths moved on the device: the replay follows them"""
    dtype, ps, per = torch.bfloat16, 16, 8
    g = torch.Generator().manual_seed(8 + fp8)
    rng = np.random.default_rng(8)
    pages = B * per + 1
    table = torch.from_numpy(rng.permutation(pages)[:B * per].reshape(B, per).astype(np.int32)).cuda()
    cdt = torch.float8_e4m3fn if fp8 else dtype
    # pools of poison: 0x7f bytes (e4m3 NaN), or NaN: a key read at or past a length, in a page tail or in the page nobody names shows
    pool = lambda: torch.full((pages, HKV, ps, D), 0x7F if fp8 else float("nan"), dtype=torch.uint8 if fp8 else dtype, device="cuda").view(cdt)  # noqa: E731
    fresh = pool()
    pk, pv, rk, rv = pool(), pool(), pool(), pool()
    scales = on_device((dm.spread_scales(rng, HKV), dm.spread_scales(rng, HKV))) if fp8 else {}
    counts = [40, 17, 3]                                     # the prompts: padded to 40 rows, and packed
    R = max(counts)
    kn, vn = (torch.randn(B, HKV, R, D, generator=g).to(dtype).cuda() for _ in range(2))
    lens = torch.tensor(counts, dtype=torch.int32, device="cuda")
    for b, qn in enumerate(counts):                          # per sequence: batches = 1, the rows it has
        one = torch.tensor([qn], dtype=torch.int32, device="cuda")
        tb.kv_cache_append(kn[b:b + 1, :, :qn].contiguous(), vn[b:b + 1, :, :qn].contiguous(), pk, pv, one, block_table=table[b:b + 1], **scales)
    starts = torch.tensor([0] + [int(x) for x in np.cumsum(counts)], dtype=torch.int32, device="cuda")
    knp = torch.cat([kn[b, :, :qn].permute(1, 0, 2) for b, qn in enumerate(counts)]).contiguous()
    vnp = torch.cat([vn[b, :, :qn].permute(1, 0, 2) for b, qn in enumerate(counts)]).contiguous()
    tb.kv_cache_append_ragged(knp, vnp, rk, rv, lens, starts, R, block_table=table, **scales)
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.uint8 if fp8 else torch.int16)  # noqa: E731
    assert torch.equal(bits(rk), bits(pk)) and torch.equal(bits(rv), bits(pv)), "the ragged append differs from the per-sequence appends"
    assert int((bits(pk) != bits(fresh)).any(dim=-1).sum()) == sum(counts) * HKV
    # one generation step in a graph
    k1, v1 = (torch.randn(B, HKV, 1, D, generator=g).to(dtype).cuda() for _ in range(2))
    q = (torch.rand(B, HQ, 1, D, generator=g) * 2 - 1).to(dtype).cuda()

    def step():
        tb.kv_cache_append(k1, v1, pk, pv, lens, block_table=table, **scales)
        return tb.flash_decode(q, pk, pv, lens, block_table=table, return_lse=True, **scales)

    lens += 1
    step()                                                   # (warm-up outside the capture; it writes what the replay writes again)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = step()
    for moved in (0, 1):
        lens += moved
        graph.replay()
        torch.cuda.synchronize()
        want_o, want_l = step()
        torch.cuda.synchronize()
        assert torch.equal(o, want_o) and torch.equal(lse, want_l), "the replay did not follow the device's lengths"
        assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(lse).all()), "poison reached an output"
    # and the step's result against the model, on what the pool now holds for every sequence
    n = lens.cpu().numpy().astype(np.uint32)
    kf, vf = torch.zeros(B, HKV, per * ps, D), torch.zeros(B, HKV, per * ps, D)
    for b in range(B):
        for key in range(int(n[b])):
            page = int(table[b, key // ps])
            kf[b, :, key], vf[b, :, key] = pk[page, :, key % ps].float().cpu(), pv[page, :, key % ps].float().cpu()
    ks, vs = (scales["k_scale"].cpu().numpy(), scales["v_scale"].cpu().numpy()) if fp8 else (None, None)
    ref = dm.model(q.cpu(), kf, vf, n, G, True, page=ps, kscale=ks, vscale=vs)
    wo, wl, text = dm.compare(o.cpu(), lse.cpu(), ref, "bf16", "bf16", n, page=ps)
    assert wo <= 1.0 and wl <= 1.0, text
    if not fp8:   # the second replay appended the row at key 41 of sequence 0: the bits of k1
        assert torch.equal(pk[int(table[0, 41 // ps]), :, 41 % ps], k1[0, :, 0])
