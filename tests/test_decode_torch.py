"""GPU test: flash_decode (torch binding of include/mfa_decode.h) against an fp32 torch softmax reference -- contiguous, paged and
permuted-view caches, return_lse, the compiled op, and the errors."""
import math

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import harness  # noqa: E402
from metal_flash_attention_amd.torch_binding import flash_decode  # noqa: E402

TOL_O, TOL_L = harness.TOL_MIXED["O"], harness.TOL_MIXED["L"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield


def reference(q, k, v, lens, causal=True):
    """fp32 softmax attention over the first len_b keys; row r sees key c iff c <= r + max(len_b - R, 0)"""
    B, H, R, D = q.shape
    G = H // k.shape[1]
    o = torch.zeros((B, H, R, D), dtype=torch.float32, device=q.device)
    lse = torch.full((B, H, R), float("-inf"), dtype=torch.float32, device=q.device)
    for b in range(B):
        n = int(lens[b])
        if n == 0:
            continue
        kk = k[b, :, :n].float().repeat_interleave(G, dim=0)
        vv = v[b, :, :n].float().repeat_interleave(G, dim=0)
        s = q[b].float() @ kk.transpose(1, 2) / math.sqrt(D)
        if causal:
            c, r = torch.arange(n, device=q.device)[None, :], torch.arange(R, device=q.device)[:, None]
            s = s.masked_fill(~(c <= r + max(n - R, 0)), float("-inf"))
        lse[b] = torch.logsumexp(s, dim=-1)
        o[b] = torch.softmax(s, dim=-1) @ vv
    return o, lse


def inputs(B, H, Hkv, R, C, D, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: (torch.rand(*s, generator=g, device="cuda") * 2 - 1).to(dtype)  # noqa: E731
    lens = torch.randint(R, C + 1, (B,), generator=g, device="cuda", dtype=torch.int32)
    lens[0] = C
    if B > 2:
        lens[1], lens[2] = R, 0
    return rnd(B, H, R, D), rnd(B, Hkv, C, D), rnd(B, Hkv, C, D), lens


def poison(k, v, lens):
    for b in range(k.shape[0]):
        k[b, :, int(lens[b]):] = float("nan")
        v[b, :, int(lens[b]):] = float("nan")


def close(o, lse, ro, rlse, lens):
    assert not torch.isnan(o.float()).any()
    assert float((o.float() - ro).abs().max()) <= TOL_O
    if lse is not None:
        keep = lens != 0
        assert float((lse[keep] - rlse[keep]).abs().max()) <= TOL_L
        assert bool((lse[~keep] < -1e30).all())


@pytest.mark.parametrize("dtype,D,H,Hkv,R,causal", [(torch.bfloat16, 128, 32, 4, 1, True), (torch.float16, 64, 8, 2, 4, True),
                                                    (torch.bfloat16, 64, 8, 8, 2, False)])
def test_contiguous_cache_and_lse(dtype, D, H, Hkv, R, causal):
    q, k, v, lens = inputs(5, H, Hkv, R, 1500, D, dtype, seed=D + R)
    ro, rlse = reference(q, k, v, lens, causal)
    poison(k, v, lens)
    o, lse = flash_decode(q, k, v, lens, causal=causal, return_lse=True)
    assert o.dtype == dtype and o.shape == q.shape and lse.dtype == torch.float32 and lse.shape == q.shape[:3]
    close(o, lse, ro, rlse, lens)
    assert torch.equal(flash_decode(q, k, v, lens, causal=causal), o)
    assert torch.equal(flash_decode(q, k, v, lens.to(torch.int64), causal=causal), o)


def test_permuted_view_caches_are_not_copied():
    B, H, Hkv, R, C, D = 4, 16, 2, 2, 700, 128
    q, k, v, lens = inputs(B, H, Hkv, R, C, D, torch.bfloat16, seed=3)
    ro, rlse = reference(q, k, v, lens)
    poison(k, v, lens)
    packed = flash_decode(q, k, v, lens)
    token_major = torch.stack([k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)], dim=2).contiguous()   # [B][C][2][Hkv][D]: one fused allocation
    kv, vv = token_major[:, :, 0].permute(0, 2, 1, 3), token_major[:, :, 1].permute(0, 2, 1, 3)
    assert not kv.is_contiguous() and kv.shape == k.shape
    o, lse = flash_decode(q, kv, vv, lens, return_lse=True)
    assert torch.equal(o, packed)
    close(o, lse, ro, rlse, lens)
    qv = torch.randn(B, R, H, D, device="cuda").to(torch.bfloat16).permute(0, 2, 1, 3)               # a [B, R, H, D] projection, permuted
    assert torch.equal(flash_decode(qv, kv, vv, lens), flash_decode(qv.contiguous(), k, v, lens))


@pytest.mark.parametrize("page", [16, 128])
def test_paged_cache(page):
    B, H, Hkv, R, C, D = 5, 32, 4, 1, 1024, 128
    q, k, v, lens = inputs(B, H, Hkv, R, C, D, torch.bfloat16, seed=page)
    ro, rlse = reference(q, k, v, lens)
    poison(k, v, lens)
    packed = flash_decode(q, k, v, lens)
    per = C // page
    g = torch.Generator().manual_seed(page)
    order = torch.randperm(B * per + 2, generator=g)
    pool_k = torch.full((B * per + 2, Hkv, page, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    pool_v = torch.full_like(pool_k, float("nan"))
    table = torch.empty((B, per), dtype=torch.int32)
    for b in range(B):
        for i in range(per):
            pg = int(order[b * per + i])
            table[b, i] = pg
            pool_k[pg] = k[b, :, i * page:(i + 1) * page]
            pool_v[pg] = v[b, :, i * page:(i + 1) * page]
    o, lse = flash_decode(q, pool_k, pool_v, lens, block_table=table.cuda(), return_lse=True)
    assert torch.equal(o, packed)
    close(o, lse, ro, rlse, lens)


def test_compiled_op_traces_fullgraph():
    q, k, v, lens = inputs(3, 16, 2, 1, 600, 128, torch.bfloat16, seed=11)
    eager = flash_decode(q, k, v, lens)
    f = torch.compile(lambda q, k, v, n: flash_decode(q, k, v, n) * 2, fullgraph=True, backend="aot_eager")
    assert torch.equal(f(q, k, v, lens), eager * 2)
    assert torch.equal(torch.ops.mfa.attention_decode(q, k, v, lens, None, True)[0], eager)


def test_errors():
    q, k, v, lens = inputs(3, 16, 2, 1, 256, 128, torch.bfloat16, seed=1)
    with pytest.raises(RuntimeError, match="forward only"):
        flash_decode(q.clone().requires_grad_(), k, v, lens)
    with pytest.raises(RuntimeError, match="forward only"):
        flash_decode(q, k.clone().requires_grad_(), v, lens)
    pool = k.reshape(3 * 2, 2, 128, 128)[:, :, :64].contiguous()
    with pytest.raises(ValueError, match="block_table"):
        flash_decode(q, pool, pool, lens, block_table=torch.zeros((2, 4), dtype=torch.int32, device="cuda"))    # wrong batch count
    with pytest.raises(ValueError, match="block_table"):
        flash_decode(q, pool, pool, lens, block_table=torch.zeros((3, 4), dtype=torch.int64, device="cuda"))    # wrong type
    with pytest.raises(ValueError, match="block_table"):
        flash_decode(q, pool, pool, lens, block_table=torch.zeros((12,), dtype=torch.int32, device="cuda"))     # wrong rank
    with pytest.raises(TypeError):
        flash_decode(q.float(), k.float(), v.float(), lens)
    with pytest.raises(ValueError, match="cache_lengths"):
        flash_decode(q, k, v, lens[:2])
    with pytest.raises(RuntimeError, match="GPU"):
        flash_decode(q.cpu(), k.cpu(), v.cpu(), lens.cpu())


def test_needle_queries_through_the_binding():
    """queries in which single keys matter (tests/decode_model.py), through flash_decode's own stride plumbing: a token-major cache
    view and a permuted q, checked element by element against the float64 model"""
    import numpy as np

    import decode_model
    B, H, Hkv, R, C, D = 4, 16, 2, 2, 700, 128
    _q, k, v, lens = inputs(B, H, Hkv, R, C, D, torch.bfloat16, seed=13)
    n = lens.cpu().numpy()
    q64, info = decode_model.needle_queries(k.cpu(), n, H, H // Hkv, R, True, "bf16")
    q = torch.from_numpy(q64).to(torch.bfloat16).cuda()
    poison(k, v, lens)
    tk, tv = k.permute(0, 2, 1, 3).contiguous(), v.permute(0, 2, 1, 3).contiguous()              # [B][C][Hkv][D]
    qv = q.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)                                  # [B][R][H][D], permuted back
    o, lse = flash_decode(qv, tk.permute(0, 2, 1, 3), tv.permute(0, 2, 1, 3), lens, return_lse=True)
    kk, vv = torch.nan_to_num(k.cpu().float()), torch.nan_to_num(v.cpu().float())
    ref = decode_model.model(q.cpu(), kk, vv, n, H // Hkv, True)
    ro, rl, text = decode_model.compare(o.float().cpu().numpy(), lse.cpu().numpy(), ref, "bf16", "bf16", n, info=info)
    print(f"RATIO bf16 O16 needles | flash_decode | err / bound at margin 1: O {ro * decode_model.MARGIN:.3f} L {rl * decode_model.MARGIN:.3f}")
    assert ro <= 1.0 and rl <= 1.0, text
    assert float(np.abs(o.float().cpu().numpy() - ref.O).max()) <= TOL_O
    assert bool((o[2] == 0).all()) and bool((lse[2] < -1e30).all())
