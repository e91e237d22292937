"""GPU test: flash_prefill, the torch entry of prefill attention over a KV cache -- the round trip that motivates it (a prompt fed in
chunks through kv_cache_append + flash_prefill into a paged e4m3 cache, then decode steps), chunked against one-shot prefill over a
16-bit cache, and a captured graph replayed after lengths and cache contents changed on the device.  Bounds: tests/prefill_model.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import decode_model as dm  # noqa: E402
import prefill_model as pm  # noqa: E402
from metal_flash_attention_amd.torch_binding import flash_decode, flash_prefill, kv_cache_append  # noqa: E402

LN2 = 0.6931471805599453


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield


def rnd(g, *s, dtype=torch.bfloat16):
    return ((torch.rand(*s, generator=g) * 2 - 1).to(dtype))


def held(o, lse, ref, fmt, n, qn, what):
    wo, wl, text = pm.compare(o.cpu(), lse.cpu(), ref, fmt, fmt, [n], [qn], margin=1)
    print("%s: worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % (what, wo, wl))
    assert wo <= pm.MARGIN and wl <= pm.MARGIN, what + ": " + text


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_round_trip_chunked_prefill_then_decode_over_a_paged_e4m3_cache(dtype):
    D, Hkv, G, page, prompt, steps = 128, 2, 4, 16, 300, 8
    Hq, fmt = Hkv * G, dm.fmt_of(dtype)
    g = torch.Generator().manual_seed(21)
    total = prompt + steps
    q_all, k_all, v_all = rnd(g, 1, Hq, total, D, dtype=dtype), rnd(g, 1, Hkv, total, D, dtype=dtype) * 3, rnd(g, 1, Hkv, total, D, dtype=dtype) * 3
    rng = np.random.default_rng(2)
    ks, vs = torch.from_numpy(dm.spread_scales(rng, Hkv)).cuda() / 64, torch.from_numpy(dm.spread_scales(rng, Hkv)).cuda() / 64
    pages = -(-total // page)
    perm = torch.randperm(pages + 4, generator=g)
    pool_k = torch.full((pages + 4, Hkv, page, D), 0x7F, dtype=torch.uint8, device="cuda").view(torch.float8_e4m3fn)
    pool_v = pool_k.clone()
    table = perm[:pages].to(torch.int32).reshape(1, pages).cuda()
    lens = torch.zeros(1, dtype=torch.int32, device="cuda")

    def cache_values():
        """the whole sequence as the cache holds it, dequantised, without the scales: [1, Hkv, keys, D]"""
        kk = pool_k[table[0].long()].float().permute(1, 0, 2, 3).reshape(1, Hkv, pages * page, D)
        vv = pool_v[table[0].long()].float().permute(1, 0, 2, 3).reshape(1, Hkv, pages * page, D)
        return kk.cpu(), vv.cpu()

    done = 0
    for chunk in (128, 128, 44):
        lens += chunk
        sl = slice(done, done + chunk)
        kv_cache_append(k_all[:, :, sl].cuda(), v_all[:, :, sl].cuda(), pool_k, pool_v, lens, block_table=table, k_scale=ks, v_scale=vs)
        o, lse = flash_prefill(q_all[:, :, sl].cuda(), pool_k, pool_v, lens, block_table=table, k_scale=ks, v_scale=vs, return_lse=True)
        done += chunk
        kk, vv = cache_values()
        ref = pm.model(q_all[:, :, sl], kk[:, :, :done], vv[:, :, :done], [done], [chunk], G, True, kscale=ks.cpu().numpy(), vscale=vs.cpu().numpy())
        held(o, lse, ref, fmt, done, chunk, "chunk ending at %d" % done)
    for _ in range(steps):
        lens += 1
        sl = slice(done, done + 1)
        kv_cache_append(k_all[:, :, sl].cuda(), v_all[:, :, sl].cuda(), pool_k, pool_v, lens, block_table=table, k_scale=ks, v_scale=vs)
        o, lse = flash_decode(q_all[:, :, sl].cuda(), pool_k, pool_v, lens, block_table=table, return_lse=True, k_scale=ks, v_scale=vs)
        done += 1
        kk, vv = cache_values()
        ref = dm.model(q_all[:, :, sl], kk[:, :, :done], vv[:, :, :done], [done], G, True, page=page, kscale=ks.cpu().numpy(), vscale=vs.cpu().numpy())
        wo, wl, text = dm.compare(o.cpu(), lse.cpu(), ref, fmt, fmt, [done], page=page)
        assert wo <= 1.0 and wl <= 1.0, "decode step at %d: %s" % (done, text)
    assert int(lens.item()) == total


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_chunked_against_one_shot_prefill_over_a_16_bit_cache(dtype):
    D, Hkv, G, n = 64, 2, 3, 300
    Hq, fmt = Hkv * G, dm.fmt_of(dtype)
    g = torch.Generator().manual_seed(22)
    q, k, v = rnd(g, 1, Hq, n, D, dtype=dtype), rnd(g, 1, Hkv, n, D, dtype=dtype), rnd(g, 1, Hkv, n, D, dtype=dtype)
    kc = torch.full((1, Hkv, 320, D), float("nan"), dtype=dtype, device="cuda")
    vc = kc.clone()
    lens = torch.zeros(1, dtype=torch.int32, device="cuda")
    ref = pm.model(q, k, v, [n], [n], G, True)
    done, parts = 0, []
    for chunk in (128, 128, 44):
        lens += chunk
        sl = slice(done, done + chunk)
        kv_cache_append(k[:, :, sl].cuda(), v[:, :, sl].cuda(), kc, vc, lens)
        o, lse = flash_prefill(q[:, :, sl].cuda(), kc, vc, lens, return_lse=True)
        done += chunk
        sub = dm.Reference(*(x[:, :, sl] for x in ref))   # the chunk's rows of the whole prompt's model: the same mask
        held(o, lse, pm.model(q[:, :, sl], k[:, :, :done], v[:, :, :done], [done], [chunk], G, True), fmt, done, chunk, "chunk ending at %d" % done)
        assert np.allclose(sub.O, dm.f64(pm.model(q[:, :, sl], k[:, :, :done], v[:, :, :done], [done], [chunk], G, True).O), rtol=1e-12, atol=1e-12)
        parts.append(o)
    one, lse = flash_prefill(q.cuda(), kc, vc, lens, return_lse=True)
    held(one, lse, ref, fmt, n, n, "one shot")
    held(torch.cat(parts, dim=2), lse, ref, fmt, n, n, "chunks against the whole prompt's model")


def same_live(o, lse, want, qlens):
    """bit equality over the rows the launch writes (rows at or past q_lengths come back uninitialised)"""
    return all(torch.equal(o[b, :, :qn], want[0][b, :, :qn]) and torch.equal(lse[b, :, :qn], want[1][b, :, :qn]) for b, qn in enumerate(qlens.tolist()))


def test_captured_graph_replays_after_lengths_and_cache_changed():
    D, Hkv, G, Rr, Cc, Bb, dtype = 128, 2, 4, 160, 512, 3, torch.bfloat16
    g = torch.Generator().manual_seed(23)
    q = rnd(g, Bb, Hkv * G, Rr, D).cuda()
    kc, vc = rnd(g, Bb, Hkv, Cc, D).cuda(), rnd(g, Bb, Hkv, Cc, D).cuda()
    lens = torch.tensor([400, 160, 37], dtype=torch.int32, device="cuda")
    qlens = torch.tensor([160, 100, 37], dtype=torch.int32, device="cuda")
    flash_prefill(q, kc, vc, lens, q_lengths=qlens)   # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = flash_prefill(q, kc, vc, lens, q_lengths=qlens, return_lse=True)
    graph.replay()
    torch.cuda.synchronize()
    want = flash_prefill(q, kc, vc, lens, q_lengths=qlens, return_lse=True)
    assert same_live(o, lse, want, qlens)
    lens.copy_(torch.tensor([512, 3, 300], dtype=torch.int32))
    qlens.copy_(torch.tensor([1, 160, 129], dtype=torch.int32))
    kc.copy_(rnd(g, Bb, Hkv, Cc, D))
    vc.copy_(rnd(g, Bb, Hkv, Cc, D))
    graph.replay()
    torch.cuda.synchronize()
    want = flash_prefill(q, kc, vc, lens, q_lengths=qlens, return_lse=True)
    assert same_live(o, lse, want, qlens), "the replay did not follow the device's lengths and cache"
    ref = pm.model(q.cpu(), kc.cpu(), vc.cpu(), lens.tolist(), qlens.tolist(), G, True)
    wo, wl, text = pm.compare(o.cpu(), lse.cpu(), ref, "bf16", "bf16", lens.tolist(), qlens.tolist(), margin=1)
    assert wo <= pm.MARGIN and wl <= pm.MARGIN, text


def test_refusals_of_the_torch_entry():
    q = torch.zeros(1, 4, 40, 64, dtype=torch.bfloat16, device="cuda")
    k = torch.zeros(1, 2, 64, 64, dtype=torch.bfloat16, device="cuda")
    lens = torch.tensor([40], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="k_scale / v_scale go with a float8_e4m3fn cache"):
        flash_prefill(q, k, k, lens, k_scale=torch.ones(2, device="cuda"))
    with pytest.raises(TypeError, match="share one of bfloat16 / float16"):
        flash_prefill(q.half(), k, k, lens)
    with pytest.raises(RuntimeError, match="forward only"):
        flash_prefill(q.requires_grad_(), k, k, lens)
    if hasattr(torch, "float8_e5m2"):
        with pytest.raises(TypeError, match="e5m2 and fnuz caches have no kernel"):
            flash_prefill(q.detach(), k.to(torch.float8_e5m2), k.to(torch.float8_e5m2), lens)
