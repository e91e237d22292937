"""GPU test: the torch binding of include/mfa_kvcache.h -- flash_decode over torch.float8_e4m3fn caches against the C-ABI launch,
kv_cache_append (in place, returns nothing, both cache types), the compiled ops and the errors."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from metal_flash_attention_amd import AttentionDecodeFP8, GEMMOperandPrecision as P  # noqa: E402
from metal_flash_attention_amd.torch_binding import flash_decode, kv_cache_append  # noqa: E402

E4M3 = torch.float8_e4m3fn


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield


def inputs(B, H, Hkv, R, C, D, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randn(B, H, R, D, generator=g, device="cuda").to(dtype)
    ks, vs = (0.5 + 1.5 * torch.rand(Hkv, generator=g, device="cuda") for _ in range(2))
    k, v = (torch.randn(B, Hkv, C, D, generator=g, device="cuda").to(dtype) for _ in range(2))
    kq = (k.float() / ks[None, :, None, None]).clamp(-448, 448).to(E4M3)
    vq = (v.float() / vs[None, :, None, None]).clamp(-448, 448).to(E4M3)
    lens = torch.randint(R, C + 1, (B,), generator=g, device="cuda", dtype=torch.int32)
    lens[0] = C
    if B > 2:
        lens[1], lens[2] = R, 0
    return q, kq, vq, ks, vs, lens


@pytest.mark.parametrize("dtype,D,H,Hkv,R,causal", [(torch.bfloat16, 128, 32, 4, 1, True), (torch.float16, 64, 8, 2, 4, False)])
def test_flash_decode_fp8_is_the_c_abi_launch(dtype, D, H, Hkv, R, causal):
    B, C = 5, 1500
    q, kq, vq, ks, vs, lens = inputs(B, H, Hkv, R, C, D, dtype, seed=D + R)
    o, lse = flash_decode(q, kq, vq, lens, causal=causal, return_lse=True, k_scale=ks, v_scale=vs)
    assert o.dtype == dtype and o.shape == q.shape and lse.dtype == torch.float32 and lse.shape == q.shape[:3]
    dec = AttentionDecodeFP8(D, P.BF16 if dtype == torch.bfloat16 else P.FP16)
    kw = dict(rows=R, column=C, heads=H, batches=B, headsPerKeyValue=H // Hkv, causal=causal, cacheLengths=lens, keyScale=ks, valueScale=vs)
    ws = torch.empty(max(dec.workspaceSize(**kw), 16), dtype=torch.uint8, device="cuda")
    o2, l2 = torch.empty_like(o), torch.empty_like(lse)
    dec.dispatch(q, kq, vq, o2, l2, stream=torch.cuda.current_stream().cuda_stream, workspace=ws, **kw)
    torch.cuda.synchronize()
    assert torch.equal(o, o2) and torch.equal(lse, l2 * 0.6931471805599453)
    assert bool(torch.isfinite(o.float()).all()) and bool((o[2] == 0).all())
    assert torch.equal(flash_decode(q, kq, vq, lens, None, causal, False, ks, vs), o)        # positional use
    none = flash_decode(q, kq, vq, lens, causal=causal)                                       # no scales: 1.0
    ones = torch.ones_like(ks)
    assert torch.equal(none, flash_decode(q, kq, vq, lens, causal=causal, k_scale=ones, v_scale=ones))
    assert not torch.equal(none, o)


@pytest.mark.parametrize("cache_dtype", ["fp8", "same"])
def test_kv_cache_append_mutates_in_place_and_returns_nothing(cache_dtype):
    B, Hkv, R, C, D, dtype = 4, 2, 2, 64, 128, torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(5)
    kn, vn = (torch.randn(B, Hkv, R, D, generator=g, device="cuda").to(dtype) for _ in range(2))
    ks, vs = (0.5 + 1.5 * torch.rand(Hkv, generator=g, device="cuda") for _ in range(2))
    lens = torch.tensor([2, 64, 10, 1], dtype=torch.int32, device="cuda")    # sequence 3 has one key: its first new row is dropped
    fp8 = cache_dtype == "fp8"
    if fp8:
        kc, vc = (torch.zeros(B, Hkv, C, D, dtype=torch.uint8, device="cuda").view(E4M3) for _ in range(2))
        scales = dict(k_scale=ks, v_scale=vs)
        want_k = (kn.float() / ks[None, :, None, None]).clamp(-448, 448).to(E4M3).view(torch.uint8)
        want_v = (vn.float() / vs[None, :, None, None]).clamp(-448, 448).to(E4M3).view(torch.uint8)
        bits = torch.uint8
    else:
        kc, vc = (torch.zeros(B, Hkv, C, D, dtype=dtype, device="cuda") for _ in range(2))
        scales = {}
        want_k, want_v, bits = kn.view(torch.int16), vn.view(torch.int16), torch.int16
    ptrs = (kc.data_ptr(), vc.data_ptr())
    assert kv_cache_append(kn, vn, kc, vc, lens, **scales) is None
    assert (kc.data_ptr(), vc.data_ptr()) == ptrs
    ek, ev = torch.zeros_like(kc.view(bits)), torch.zeros_like(vc.view(bits))
    for b, n in enumerate(lens.tolist()):
        for r in range(R):
            pos = n - R + r
            if pos >= 0:
                ek[b, :, pos], ev[b, :, pos] = want_k[b, :, r], want_v[b, :, r]
    assert torch.equal(kc.view(bits), ek) and torch.equal(vc.view(bits), ev)
    # a token-major cache, permuted: written where it lies
    tk = torch.zeros(B, C, Hkv, D, dtype=kc.dtype if not fp8 else torch.uint8, device="cuda")
    tv = torch.zeros_like(tk)
    if fp8:
        tk, tv = tk.view(E4M3), tv.view(E4M3)
    kv_cache_append(kn, vn, tk.permute(0, 2, 1, 3), tv.permute(0, 2, 1, 3), lens, **scales)
    assert torch.equal(tk.view(bits).permute(0, 2, 1, 3), ek) and torch.equal(tv.view(bits).permute(0, 2, 1, 3), ev)


def test_compiled_ops_trace_fullgraph():
    B, H, Hkv, R, C, D = 3, 16, 2, 1, 600, 128
    q, kq, vq, ks, vs, lens = inputs(B, H, Hkv, R, C, D, torch.bfloat16, seed=11)
    if not hasattr(torch.library, "custom_op"):
        pytest.skip("torch.library.custom_op is not available")
    lens = torch.tensor([600, 17, 300], dtype=torch.int32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    kn, vn = (torch.randn(B, Hkv, R, D, generator=g, device="cuda").to(torch.bfloat16) for _ in range(2))
    k1, v1 = kq.clone(), vq.clone()
    kv_cache_append(kn, vn, k1, v1, lens, k_scale=ks, v_scale=vs)
    eager = flash_decode(q, k1, v1, lens, k_scale=ks, v_scale=vs)

    def step(q, kn, vn, kc, vc, n, ks, vs):
        kv_cache_append(kn, vn, kc, vc, n, k_scale=ks, v_scale=vs)
        return flash_decode(q, kc, vc, n, k_scale=ks, v_scale=vs) * 2

    f = torch.compile(step, fullgraph=True, backend="aot_eager")
    k2, v2 = kq.clone(), vq.clone()
    assert torch.equal(f(q, kn, vn, k2, v2, lens, ks, vs), eager * 2)
    assert torch.equal(k2.view(torch.uint8), k1.view(torch.uint8)) and torch.equal(v2.view(torch.uint8), v1.view(torch.uint8))
    assert not torch.equal(k2.view(torch.uint8), kq.view(torch.uint8))
    assert torch.equal(torch.ops.mfa.attention_decode_fp8(q, k1, v1, lens, None, True, ks, vs)[0], eager)


def test_errors():
    q, kq, vq, ks, vs, lens = inputs(3, 16, 2, 1, 256, 128, torch.bfloat16, seed=1)
    k16, v16 = kq.to(torch.bfloat16), vq.to(torch.bfloat16)
    kn, vn = k16[:, :, :1].contiguous(), v16[:, :, :1].contiguous()
    with pytest.raises(RuntimeError, match="GPU"):
        flash_decode(q.cpu(), kq.cpu(), vq.cpu(), lens.cpu(), k_scale=ks.cpu(), v_scale=vs.cpu())
    with pytest.raises(RuntimeError, match="GPU"):
        flash_decode(q, kq, vq, lens, k_scale=ks.cpu())
    with pytest.raises(RuntimeError, match="GPU"):
        kv_cache_append(kn.cpu(), vn.cpu(), kq.cpu(), vq.cpu(), lens.cpu())
    with pytest.raises(RuntimeError, match="forward only"):
        flash_decode(q.clone().requires_grad_(), kq, vq, lens)
    with pytest.raises(RuntimeError, match="autograd"):
        kv_cache_append(kn.clone().requires_grad_(), vn, kq, vq, lens)
    with pytest.raises(ValueError, match="float8_e4m3fn cache"):
        flash_decode(q, k16, v16, lens, k_scale=ks)
    with pytest.raises(ValueError, match="float8_e4m3fn cache"):
        kv_cache_append(kn, vn, k16.clone(), v16.clone(), lens, v_scale=vs)
    e5 = kq.view(torch.uint8).view(torch.float8_e5m2)
    with pytest.raises(TypeError, match="e5m2"):
        flash_decode(q, e5, e5, lens)
    with pytest.raises(TypeError, match="e5m2"):
        kv_cache_append(kn, vn, e5.clone(), e5.clone(), lens)
    with pytest.raises(ValueError, match="k_scale"):
        flash_decode(q, kq, vq, lens, k_scale=ks[:1])
    with pytest.raises(TypeError):
        kv_cache_append(kn.to(torch.float16), vn, kq, vq, lens)


def test_needle_queries_over_an_fp8_cache_through_the_binding():
    """queries in which single keys matter (tests/decode_model.py) against the float64 model of the dequantised cache: the binding's
    own scale and stride plumbing (per-head scales pairwise 1.25 x apart, a token-major cache view)"""
    import numpy as np

    import decode_model
    B, H, Hkv, R, C, D = 4, 16, 4, 2, 700, 128
    q, kq, vq, _ks, _vs, lens = inputs(B, H, Hkv, R, C, D, torch.bfloat16, seed=17)
    rng = np.random.default_rng(17)
    ks, vs = decode_model.spread_scales(rng, Hkv), decode_model.spread_scales(rng, Hkv)
    n = lens.cpu().numpy()
    k64, v64 = kq.cpu().to(torch.float64).numpy(), vq.cpu().to(torch.float64).numpy()
    q64, info = decode_model.needle_queries(k64 * ks.astype(np.float64)[None, :, None, None], n, H, H // Hkv, R, True, "bf16")
    q = torch.from_numpy(q64).to(torch.bfloat16).cuda()
    tk = kq.view(torch.uint8).permute(0, 2, 1, 3).contiguous().view(E4M3).permute(0, 2, 1, 3)     # [B][C][Hkv][D] underneath
    tv = vq.view(torch.uint8).permute(0, 2, 1, 3).contiguous().view(E4M3).permute(0, 2, 1, 3)
    o, lse = flash_decode(q, tk, tv, lens, return_lse=True, k_scale=torch.from_numpy(ks).cuda(), v_scale=torch.from_numpy(vs).cuda())
    assert torch.equal(o, flash_decode(q, kq, vq, lens, k_scale=torch.from_numpy(ks).cuda(), v_scale=torch.from_numpy(vs).cuda()))
    ref = decode_model.model(q.cpu(), k64, v64, n, H // Hkv, True, kscale=ks, vscale=vs)
    ro, rl, text = decode_model.compare(o.float().cpu().numpy(), lse.cpu().numpy(), ref, "bf16", "bf16", n, info=info)
    print(f"RATIO bf16 O16 needles | flash_decode fp8 | err / bound at margin 1: O {ro * decode_model.MARGIN:.3f} L {rl * decode_model.MARGIN:.3f}")
    assert ro <= 1.0 and rl <= 1.0, text
    assert bool((o[2] == 0).all()) and bool((lse[2] < -1e30).all())
