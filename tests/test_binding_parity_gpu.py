"""GPU parity of torch_binding.flash_attention, end to end, under the per-element bounds of tests/train_model.py on its needle inputs.

flash_attention(...) and .backward(dO) on operands that are permuted [B, N, H, D] views (leading dimension H D, no copy), in bf16 and
fp16, with fast_scale on and off, causal, with q_lengths / k_lengths, with a block mask, with Hkv < H, and through flash_attention_op.
O, dQ, dK and dV are held to the model's bound for the launch form the binding runs: 16-bit outputs (D from the stored O), dO in BF16
also next to fp16 operands (the path of the mix: the backwardKeyValue kernel the binding selects, train_model.MIX_PATH), grouped K / V
heads.  L and D are not visible here.  Padding rows must read exactly zero: the binding defines them so.  One fp16 case passes a
grad_out that BF16 cannot represent (train_model.off_grid_grad: every element three quarters of a BF16 ulp above a BF16 value, so
round-to-nearest and truncation differ on every element): the expected gradients are the model's on its BF16 round-to-nearest, and
every gradient must lie nearer to them than to the model's on the truncated grad_out.  That case runs the exact mode, where a
truncating `grad_out.to(torch.bfloat16)` is outside the bound (dQ: 1.6 x; tests/test_train_sensitivity.py proves it on the CPU and
pins that the mixed mode, at 0.7 x, would not resolve it).  The bound, the checker and the needle inputs are train_model's; this
file defines none.
"""
import numpy as np
import pytest

import train_model as tm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from metal_flash_attention_amd import AttentionKernelType  # noqa: E402
from metal_flash_attention_amd import torch_binding  # noqa: E402
from metal_flash_attention_amd.torch_binding import flash_attention, flash_attention_op, pack_block_mask  # noqa: E402

B, H, R, C = 2, 4, 300, 333
DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16}
_MODELS = {}


def binding_case(fmt, D, fast, *, causal=False, lengths=False, mask=False, Hkv=H, op=False, odd_grad=False):
    name = "%s-d%d-%s-%s%s%s%s%s%s" % (fmt, D, "fast" if fast else "exact", "causal" if causal else "dense", "-lengths" if lengths else "",
                                       "-mask" if mask else "", "-hkv%d" % Hkv if Hkv != H else "", "-op" if op else "", "-odd-grad" if odd_grad else "")
    return pytest.param(dict(fmt=fmt, D=D, fast=fast, causal=causal, lengths=lengths, mask=mask, Hkv=Hkv, op=op, odd_grad=odd_grad), id=name)


ODD_GRAD = binding_case("f16", 128, False, causal=True, odd_grad=True)
CASES = (
    binding_case("bf16", 64, True), binding_case("bf16", 128, False, causal=True), binding_case("f16", 64, True, causal=True),
    binding_case("f16", 128, False), binding_case("bf16", 128, True, lengths=True), binding_case("f16", 64, False, lengths=True),
    binding_case("bf16", 64, True, mask=True), binding_case("bf16", 128, True, Hkv=2), binding_case("f16", 64, False, causal=True, Hkv=1),
    binding_case("bf16", 128, True, causal=True, op=True), binding_case("f16", 64, False, op=True), ODD_GRAD,
)


def _strided(x, dtype):
    """float64 [B, heads, N, D] -> (a leaf tensor [B, N, heads, D] on the GPU, its [B, heads, N, D] view)"""
    base = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1, 3))).to(dtype).cuda()
    assert np.array_equal(base.double().cpu().numpy().transpose(0, 2, 1, 3), x), "the inputs must reach the device exactly"
    return base, base.permute(0, 2, 1, 3)


@pytest.mark.parametrize("c", CASES)
def test_flash_attention_inside_the_per_element_bounds(c):
    fmt, D, fast, G = c["fmt"], c["D"], c["fast"], H // c["Hkv"]
    dtype = DTYPE[fmt]
    rl, cl = ([R, 77], [C, 100]) if c["lengths"] else (None, None)
    bits = tm.needle_mask(R, C, 940) if c["mask"] else None
    kernels = {t: torch_binding._kernel(dtype, R, C, D, t, fast) for t in AttentionKernelType}
    path = tm.mix_path(kernels[AttentionKernelType.backwardKeyValue].variant) if fmt == "f16" else None
    pieces = None
    if not (c["causal"] or c["lengths"] or c["mask"]):      # the launches the binding hands a forward workspace: the library may split them
        pieces = tm.pieces_of({"fwd": tm.piece_count(kernels[AttentionKernelType.forward], "fwd", R, C, D, H, B)}, R, C)
    key = tuple(sorted((k, str(v)) for k, v in c.items() if k != "op")) + (str(pieces), path)
    if key not in _MODELS:
        geo = dict(causal=c["causal"], row_lengths=rl, key_lengths=cl, pieces=pieces)
        if bits is not None:
            geo["block_mask"] = bits
        q, k, v, dO, info = tm.needle_inputs(B, H, R, C, D, fmt, dO_fmt="bf16", heads_per_kv=G, seed=R + D, **geo)
        form = dict(fmt=fmt, mixed=fast, out=fmt, dO_fmt="bf16", dO_path=path, heads_per_kv=G, **geo)
        grad, truncated = dO, None
        if c["odd_grad"]:                                   # fp16 values BF16 cannot hold; the kernels see their BF16 round-to-nearest
            grad = tm.off_grid_grad(dO)
            dO = tm.round_to(grad, "bf16")
            assert (dO != tm.round_to(grad, "bf16", trunc=True)).all(), "the two roundings must differ on every element"
            truncated = tm.model(q, k, v, tm.round_to(grad, "bf16", trunc=True), with_bounds=False, **form)
        _MODELS[key] = (q, k, v, grad, info, tm.model(q, k, v, dO, **form), truncated)
    q, k, v, grad, info, ref, truncated = _MODELS[key]
    qb, kb, vb = (_strided(x, dtype)[0].requires_grad_(True) for x in (q, k, v))
    qv, kv, vv = qb.permute(0, 2, 1, 3), kb.permute(0, 2, 1, 3), vb.permute(0, 2, 1, 3)
    assert qv.stride(2) == H * D and kv.stride(2) == c["Hkv"] * D
    gv = _strided(grad, dtype)[1]
    if c["op"]:
        o = flash_attention_op(qv, kv, vv, causal=c["causal"], fast_scale=fast)
    else:
        o = flash_attention(qv, kv, vv, causal=c["causal"], fast_scale=fast,
                            q_lengths=None if rl is None else torch.tensor(rl, device="cuda"), k_lengths=None if cl is None else torch.tensor(cl, device="cuda"),
                            block_mask=None if bits is None else pack_block_mask(torch.from_numpy(bits)))
    o.backward(gv)
    torch.cuda.synchronize()
    assert o.dtype == dtype and all(leaf.grad.dtype == dtype for leaf in (qb, kb, vb))
    got = {"O": o.detach().double().cpu().numpy()}
    for name, leaf in (("dQ", qb), ("dK", kb), ("dV", vb)):
        got[name] = leaf.grad.permute(0, 2, 1, 3).double().cpu().numpy()
    for name in got:                                        # the binding defines padding rows as zero; the checker's sentinel is NaN
        live = ref.key_live if name in ("dK", "dV") else ref.row_live
        padding = ~np.broadcast_to(live[:, None, :, None], got[name].shape)
        assert (got[name][padding] == 0).all(), "%s: a padding row does not read exactly zero" % name
        got[name] = np.where(padding, np.nan, got[name])
    outputs = ("O", "dV", "dK", "dQ")
    at_one = tm.compare(got, ref, out=fmt, margin=1, info=info, outputs=outputs)[0]
    worst, _padding, text = tm.compare(got, ref, out=fmt, info=info, outputs=outputs)
    print("binding parity %s: err / bound at margin 1: %s; path %s; pieces %s" % (
        c, " ".join("%s %.3f" % kv_ for kv_ in at_one.items()), path, None if pieces is None else len(pieces["fwd"])))
    assert max(worst.values()) <= 1.0, "outside the bound at margin %d (%s):\n%s" % (tm.MARGIN, [k_.variant for k_ in kernels.values()], text)
    if truncated is not None:                               # nearer to the rounded grad_out's gradients than to the truncated one's
        for name in ("dV", "dK", "dQ"):
            near, far = (float(np.nansum((got[name] - getattr(m, name)) ** 2)) for m in (ref, truncated))
            print("  %s: squared distance to the model on the rounded grad_out %.3g, on the truncated %.3g" % (name, near, far))
            assert near < far, "%s follows the TRUNCATED grad_out" % name
