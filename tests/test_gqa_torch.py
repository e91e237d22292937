"""GPU test: grouped-query attention through the torch binding -- q [B, Hq, R, D] with k, v [B, Hkv, C, D], Hq % Hkv == 0.

Gradients against an fp32 torch reference (K / V repeated per query head with repeat_interleave, math attention, autograd).
"""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from metal_flash_attention_amd.torch_binding import flash_attention, flash_attention_op  # noqa: E402

TOL = {torch.float32: 2e-4, torch.bfloat16: 6e-2, torch.float16: 3e-2}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield


def _reference(q, k, v, causal):
    G = q.shape[1] // k.shape[1]
    q, k, v = (x.detach().float().requires_grad_() for x in (q, k, v))
    kk, vv = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
    s = q @ kk.transpose(-1, -2) / q.shape[-1] ** 0.5
    if causal:
        R, C = s.shape[-2:]
        s = s.masked_fill(torch.ones(R, C, dtype=torch.bool, device=s.device).triu(C - R + 1), float("-inf"))
    o = torch.softmax(s, -1) @ vv
    return o, (q, k, v)


def _inputs(dtype, B, Hq, Hkv, R, C, D, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda *s: (torch.randn(*s, generator=g, device="cuda") * 0.5).to(dtype).requires_grad_()  # noqa: E731
    return mk(B, Hq, R, D), mk(B, Hkv, C, D), mk(B, Hkv, C, D)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("fast_scale", [False, True])
def test_gradients_match_the_torch_reference(dtype, causal, fast_scale):
    if fast_scale and dtype == torch.float32:
        pytest.skip("fast_scale applies to 16-bit inputs")
    B, Hq, Hkv, R, C, D = 2, 8, 2, 192, 256, 128
    q, k, v = _inputs(dtype, B, Hq, Hkv, R, C, D)
    o = flash_attention(q, k, v, causal=causal, fast_scale=fast_scale)
    assert o.shape == (B, Hq, R, D)
    do = torch.randn_like(o)
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), do)
    assert dk.shape == dv.shape == (B, Hkv, C, D)
    ro, leaves = _reference(q, k, v, causal)
    rq, rk, rv = torch.autograd.grad(ro, leaves, do.float())
    tol = TOL[dtype] * (2 if fast_scale else 1)
    for name, got, want in (("o", o, ro), ("dq", dq, rq), ("dk", dk, rk), ("dv", dv, rv)):
        err = (got.float() - want).abs().max().item()
        assert err <= tol * max(1.0, want.abs().max().item()), (name, err)


def test_mqa_and_strided_kv_views():
    """one K / V head; K and V as slices of a fused [B, N, (Hq + 2) D] projection: passed without a copy"""
    B, Hq, R, D = 1, 4, 128, 64
    qkv = (torch.randn(B, R, Hq + 2, D, device="cuda") * 0.5).to(torch.bfloat16).requires_grad_()
    x = qkv.transpose(1, 2)
    q, k, v = x[:, :Hq], x[:, Hq:Hq + 1], x[:, Hq + 1:]
    o = flash_attention(q, k, v, causal=True)
    (dx,) = torch.autograd.grad(o, qkv, torch.ones_like(o))
    ro, leaves = _reference(q, k, v, True)
    rq, rk, rv = torch.autograd.grad(ro, leaves, torch.ones_like(ro))
    assert (o.float() - ro).abs().max().item() < 6e-2
    ref = torch.cat([rq, rk, rv], dim=1).transpose(1, 2)
    assert (dx.float() - ref).abs().max().item() < 6e-2 * max(1.0, ref.abs().max().item())


def test_compiled_op():
    B, Hq, Hkv, R, C, D = 1, 8, 2, 128, 128, 64
    q, k, v = _inputs(torch.bfloat16, B, Hq, Hkv, R, C, D, seed=3)
    f = torch.compile(lambda q, k, v: flash_attention_op(q, k, v, causal=True), fullgraph=True)
    o = f(q, k, v)
    dq, dk, dv = torch.autograd.grad(o.float().sum(), (q, k, v))
    assert dk.shape == (B, Hkv, C, D)
    ro, leaves = _reference(q, k, v, True)
    rq, rk, rv = torch.autograd.grad(ro.sum(), leaves)
    for got, want in ((o, ro), (dq, rq), (dk, rk), (dv, rv)):
        assert (got.float() - want).abs().max().item() < 6e-2 * max(1.0, want.abs().max().item())


def test_heads_not_a_multiple_raise():
    q = torch.zeros(1, 6, 64, 64, device="cuda", dtype=torch.bfloat16)
    k = torch.zeros(1, 4, 64, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        flash_attention(q, k, k)
    with pytest.raises(ValueError):
        flash_attention_op(q, k, k)
