"""GPU parity of the training kernels (forward, dQ, dK/dV) under the per-element bounds of tests/train_model.py, on its needle inputs.

Every case launches the three kernels of one descriptor through the C ABI on a [B, H] grid (every output buffer full of NaN, one
spare batch entry behind each as the canary), compares ALL six outputs of the launch with train_model.compare -- every element of
every live row and key under the bound at the committed margin, the padding and the canary against the sentinel -- and prints the
worst err / bound at margin 1.  Each case asserts the `variant` and the `launchForm` it means to test, so that a shape cannot slide
onto another kernel unnoticed.  tests/test_train_sensitivity.py proves on the CPU that this check sees each named wrong kernel.

FP16 cases store dO in FP16 next to FP16 Q / K / V (the model's one 16-bit type); the reference's own FP16 / BF16-dO mix keeps the
checks of tests/test_attention_gpu.py.
"""
import math

import numpy as np
import pytest

import train_model
from metal_flash_attention_amd import AttentionDescriptor, AttentionKernel, AttentionKernelType, AttentionOperand, GEMMOperandPrecision
from test_attention_gpu import DKV_RS, DKV_W4, DQ_W4, FWD_8x32, parameter_rows
from train_model import MARGIN, bounds, compare  # noqa: F401 -- the one bound, margin and checker (test_train_sensitivity.py (d))

pytestmark = pytest.mark.gpu
P = GEMMOperandPrecision
Op = AttentionOperand
T = AttentionKernelType
FWD, DQ, DKV = T.forward, T.backwardQuery, T.backwardKeyValue
MODES = {"bf16-mixed": ("bf16", True), "bf16-exact": ("bf16", False), "f16-mixed": ("f16", True), "f16-exact": ("f16", False)}
_MODELS = {}


def case(name, R, C, D, modes, *, B=1, H=1, causal=False, rl=None, cl=None, workspace=False, rows=(), spike=False, variant=None, form=None):
    """variant / form: {kernel type: text the kernel's variant / the launch's form must contain; form: several joined by |, a leading !
    for text it must not contain}"""
    return [pytest.param(dict(R=R, C=C, D=D, B=B, H=H, causal=causal, rl=rl, cl=cl, workspace=workspace, rows=rows, spike=spike,
                              variant=variant or {}, form=form or {}, mode=m), id="%s-%dx%dx%d-%s" % (name, R, C, D, m)) for m in modes]


L3R, L3C = [300, 77, 1], [333, 100, 64]          # per-batch lengths: an entry shorter than a workgroup, a one-row entry
CASES = (
    # ---- forward attn_fwd16_p6 (D <= 64), backward attn_dq16_p4 / attn_dkv16_p4
    case("p6-dense", 255, 257, 64, MODES, variant={FWD: "attn_fwd16p6", DQ: "attn_dq16p4", DKV: "attn_dkv16p4"}, form={FWD: "attn_fwd16_p6"})
    + case("p6-causal", 255, 257, 64, ("bf16-mixed", "f16-exact"), H=2, causal=True, variant={FWD: "attn_fwd16p6"}, form={FWD: "attn_fwd16_p6"})
    + case("p6-lengths", 300, 333, 64, ("bf16-mixed", "f16-mixed"), B=3, H=2, rl=L3R, cl=L3C, variant={FWD: "attn_fwd16p6"},
           form={FWD: "per-batch lengths"})
    + case("p6-below-bucket", 300, 333, 40, ("bf16-mixed", "f16-exact"), variant={FWD: "attn_fwd16p6", DQ: "attn_dq16p4", DKV: "attn_dkv16p4"})
    # ---- forward attn_fwd16_p4p / attn_fwd16_p4 (D <= 128), backward attn_dq16_p4 / attn_dkv16_p4
    + case("p4p-persistent-ragged", 300, 160, 128, ("bf16-mixed", "f16-exact"), B=12, H=11, variant={FWD: "attn_fwd16p4", DQ: "attn_dq16p4", DKV: "attn_dkv16p4"},
           form={FWD: "attn_fwd16_p4p (persistent"})
    + case("p4p-causal-pairs-odd", 600, 600, 128, ("bf16-mixed", "f16-mixed"), H=2, causal=True, variant={FWD: "attn_fwd16p4"},
           form={FWD: "attn_fwd16_p4p (persistent"})
    + case("p4p-lengths", 300, 333, 128, ("bf16-mixed", "bf16-exact"), B=3, H=2, rl=L3R, cl=L3C, variant={FWD: "attn_fwd16p4"},
           form={FWD: "per-batch lengths"})
    + case("p4-causal-lengths", 300, 333, 128, ("bf16-mixed", "f16-exact"), B=3, H=2, causal=True, rl=L3R, cl=L3C, variant={FWD: "attn_fwd16p4"},
           form={FWD: "attn_fwd16p4_|!persistent"})
    + case("p4-below-bucket", 255, 257, 104, ("bf16-exact", "f16-mixed"), variant={FWD: "attn_fwd16p4", DQ: "attn_dq16p4", DKV: "attn_dkv16p4"})
    # ---- forward attn_fwd16_p5, backward attn_dq16_p5 / attn_dkv16_p5 (128 < D <= 256)
    + case("p5", 300, 333, 160, ("bf16-mixed",), variant={FWD: "attn_fwd16p5", DQ: "attn_dq16p5", DKV: "attn_dkv16p5"})
    + case("p5-causal", 255, 257, 192, ("f16-mixed", "bf16-exact"), causal=True, variant={FWD: "attn_fwd16p5", DQ: "attn_dq16p5", DKV: "attn_dkv16p5"})
    + case("p5", 300, 333, 256, ("bf16-mixed", "f16-exact"), variant={FWD: "attn_fwd16p5", DQ: "attn_dq16p5", DKV: "attn_dkv16p5"})
    + case("p5-lengths", 300, 333, 256, ("bf16-exact", "bf16-mixed"), B=3, H=2, rl=L3R, cl=L3C, variant={FWD: "attn_fwd16p5", DQ: "attn_dq16p5", DKV: "attn_dkv16p5"})
    + case("p5-below-bucket", 255, 257, 200, ("bf16-mixed",), causal=True, variant={FWD: "attn_fwd16p5", DQ: "attn_dq16p5", DKV: "attn_dkv16p5"})
    # ---- 256 < D <= 384: attn_fwd16_wide, attn_dq16w_*, attn_dkv16w_*
    + case("wide", 255, 257, 320, ("bf16-mixed", "f16-exact"), variant={FWD: "attn_fwd16w_", DQ: "attn_dq16w_", DKV: "attn_dkv16w_"})
    + case("wide-causal", 255, 257, 384, ("bf16-exact", "f16-mixed"), causal=True, variant={FWD: "attn_fwd16w_", DQ: "attn_dq16w_", DKV: "attn_dkv16w_"})
    + case("wide-lengths", 300, 333, 384, ("bf16-mixed",), B=3, H=1, rl=L3R, cl=L3C, variant={FWD: "attn_fwd16w_", DQ: "attn_dq16w_", DKV: "attn_dkv16w_"})
    # ---- the compiler-scheduled siblings, through the parameter rows of tests/test_attention_gpu.py
    + case("v3-8x32", 300, 333, 128, ("bf16-exact", "bf16-mixed"), rows=(FWD_8x32,), variant={FWD: "attn_fwd16v3"})
    + case("v3-8x32-causal", 255, 257, 64, ("f16-exact",), rows=(FWD_8x32,), causal=True, variant={FWD: "attn_fwd16v3"})
    + case("rs", 300, 333, 128, ("bf16-exact", "bf16-mixed"), rows=(DKV_RS, DQ_W4), variant={DQ: "attn_dq16p4", DKV: "attn_dkv16rs"})
    + case("rs-causal", 255, 257, 256, ("bf16-mixed", "f16-exact"), rows=(DKV_RS, DQ_W4), causal=True, variant={DQ: "attn_dq16_", DKV: "attn_dkv16rs"})
    + case("rs-lengths", 300, 333, 192, ("bf16-mixed",), rows=(DKV_RS, DQ_W4), B=3, H=2, rl=L3R, cl=L3C, variant={DQ: "attn_dq16_", DKV: "attn_dkv16rs"},
           form={DQ: "attn_dq16_", DKV: "attn_dkv16rs"})
    + case("w4", 255, 257, 64, ("bf16-exact", "f16-exact"), rows=(DKV_W4,), variant={DKV: "attn_dkv16_"})
    + case("w4-causal", 300, 333, 128, ("bf16-exact",), rows=(DKV_W4,), causal=True, variant={DKV: "attn_dkv16_"})
    + case("w4-lengths", 300, 333, 64, ("f16-exact",), rows=(DKV_W4,), B=3, H=2, rl=L3R, cl=L3C, variant={DKV: "attn_dkv16_"}, form={DKV: "attn_dkv16_"})
    # ---- column-parallel forms: pieces + combine through a workspace (forward p6 and p4p; one backward pair per family)
    + case("split-p6", 513, 1024, 64, ("bf16-mixed", "f16-exact"), workspace=True, variant={FWD: "attn_fwd16p6"},
           form={FWD: "column-parallel x|pieces by attn_fwd16_p6", DQ: "column-parallel x", DKV: "column-parallel x"})
    + case("split-p4p", 513, 1024, 128, ("bf16-mixed", "bf16-exact"), workspace=True, variant={FWD: "attn_fwd16p4", DQ: "attn_dq16p4", DKV: "attn_dkv16p4"},
           form={FWD: "column-parallel x|pieces by attn_fwd16_p4p", DQ: "column-parallel x", DKV: "column-parallel x"})
    + case("split-ragged", 513, 1030, 128, ("bf16-mixed",), workspace=True, variant={FWD: "attn_fwd16p4", DQ: "attn_dq16p4", DKV: "attn_dkv16p4"},
           form={FWD: "column-parallel x|pieces by attn_fwd16_p4,", DQ: "column-parallel x", DKV: "column-parallel x"})
    + case("split-p5", 513, 1030, 256, ("bf16-mixed", "f16-mixed"), workspace=True, variant={FWD: "attn_fwd16p5", DQ: "attn_dq16p5", DKV: "attn_dkv16p5"},
           form={FWD: "column-parallel x", DQ: "column-parallel x", DKV: "column-parallel x"})
    + case("split-causal", 600, 600, 128, ("bf16-mixed",), workspace=True, causal=True, variant={FWD: "attn_fwd16p4", DQ: "attn_dq16p4", DKV: "attn_dkv16p4"},
           form={FWD: "attn_fwd16_p4p (persistent", DQ: "column-parallel x|sibling", DKV: "column-parallel x|sibling"})
    # ---- the late dominant key that fires the deferred rescale (threshold 8)
    + case("spike", 300, 333, 128, ("bf16-mixed", "f16-exact"), H=2, spike=True, variant={FWD: "attn_fwd16p4"})
    + case("spike", 300, 333, 64, ("bf16-mixed",), H=2, spike=True, variant={FWD: "attn_fwd16p6"})
    + case("spike", 300, 333, 256, ("bf16-mixed",), H=2, spike=True, variant={FWD: "attn_fwd16p5"})
    # ---- bench.py's headline code objects at full size
    + case("headline", 4096, 4096, 128, ("bf16-mixed",), variant={FWD: "_fold", DQ: "attn_dq16p4", DKV: "attn_dkv16p4"},
           form={FWD: "attn_fwd16_p4p (persistent"})
)


def _kernels(c, fmt, mixed):
    desc = AttentionDescriptor()
    desc.lowPrecisionInputs, desc.lowPrecisionIntermediates = True, mixed
    desc.matrixDimensions = (c["R"], c["C"], c["D"])
    desc.transposeState = (False,) * 4
    desc.lowPrecisionInputType = P.BF16 if fmt == "bf16" else P.FP16
    kernels, precisions = {}, {}
    with parameter_rows(*c["rows"]):
        for t in (FWD, DQ, DKV):
            kdesc = desc.kernelDescriptor(t)
            if fmt == "f16" and Op.dO in kdesc.memoryPrecisions:
                kdesc.memoryPrecisions[Op.dO] = P.FP16
            kernels[t] = AttentionKernel(kdesc)
            precisions.update({op: P(int(p)) for op, p in kdesc.memoryPrecisions.items()})
    return kernels, precisions


def _pieces(c, kernels):
    """the library's own plan for this launch, from the workspace each kernel asks for"""
    counts = {t: train_model.piece_count(kernels[t], name, c["R"], c["C"], c["D"], c["H"], c["B"])
              for t, name in zip((FWD, DQ, DKV), train_model.KERNEL_TYPES)}
    named = {name: counts[t] for t, name in zip((FWD, DQ, DKV), train_model.KERNEL_TYPES)}
    return train_model.pieces_of(named, c["R"], c["C"]), counts


def _problem(c, fmt, mixed, pieces):
    """needle inputs and the float64 model of a case, computed once per (case, type, mode)"""
    key = (c["R"], c["C"], c["D"], c["B"], c["H"], c["causal"], str(c["rl"]), str(c["cl"]), c["spike"], fmt, mixed, str(pieces))
    if key not in _MODELS:
        geo = dict(causal=c["causal"], row_lengths=c["rl"], key_lengths=c["cl"], pieces=pieces)
        q, k, v, dO, info = train_model.needle_inputs(c["B"], c["H"], c["R"], c["C"], c["D"], fmt, spike=c["spike"], seed=c["R"] + c["D"], **geo)
        _MODELS[key] = (q, k, v, dO, info, train_model.model(q, k, v, dO, fmt=fmt, mixed=mixed, **geo))
    return _MODELS[key]


TORCH_TYPE = {P.FP32: "float32", P.FP16: "float16", P.BF16: "bfloat16"}


@pytest.mark.parametrize("c", CASES)
def test_training_kernels_inside_the_per_element_bounds(c):
    import torch
    fmt, mixed = MODES[c["mode"]]
    R, C, D, B, H = c["R"], c["C"], c["D"], c["B"], c["H"]
    kernels, prec = _kernels(c, fmt, mixed)
    for t, text in c["variant"].items():
        assert text in kernels[t].variant, (t.name, kernels[t].variant, text)
    pieces, counts = _pieces(c, kernels) if c["workspace"] else (None, {})
    q, k, v, dO, info, ref = _problem(c, fmt, mixed, pieces)

    def dev_in(x, op):
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(getattr(torch, TORCH_TYPE[prec[op]])).cuda()

    def dev_out(op, *shape):     # B live entries and one spare entry, the canary: all NaN
        return torch.full((B + 1,) + shape, float("nan"), device="cuda", dtype=getattr(torch, TORCH_TYPE[prec[op]]))

    bufs = {Op.Q: dev_in(q, Op.Q), Op.K: dev_in(k, Op.K), Op.V: dev_in(v, Op.V), Op.dO: dev_in(dO, Op.dO),
            Op.O: dev_out(Op.O, H, R, D), Op.L: dev_out(Op.L, H, R), Op.D: dev_out(Op.D, H, R),
            Op.dQ: dev_out(Op.dQ, H, R, D), Op.dK: dev_out(Op.dK, H, C, D), Op.dV: dev_out(Op.dV, H, C, D)}
    for op, x in ((Op.Q, q), (Op.K, k), (Op.V, v), (Op.dO, dO)):
        assert np.array_equal(bufs[op].double().cpu().numpy(), x), "the inputs must reach the device exactly"
    hs = {Op.Q: R * D, Op.K: C * D, Op.V: C * D, Op.O: R * D, Op.L: R, Op.D: R, Op.dO: R * D, Op.dV: C * D, Op.dK: C * D, Op.dQ: R * D}
    bs = {op: s * H for op, s in hs.items()}
    kw = dict(row=R, column=C, heads=H, batches=B, headStrides=hs, batchStrides=bs, causal=c["causal"])
    if c["rl"] is not None:
        kw["rowLengths"] = torch.tensor(c["rl"], dtype=torch.int32, device="cuda")
        kw["columnLengths"] = torch.tensor(c["cl"], dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    forms = {}
    for t in (FWD, DQ, DKV):
        ws = None
        if c["workspace"]:
            need = kernels[t].workspaceSize(row=R, column=C, heads=H, batches=B)
            ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda") if need else None
        forms[t] = kernels[t].launchForm(bufs, workspace=ws, **kw)
        for text in c["form"].get(t, "").split("|") if t in c["form"] else ():
            assert (text[1:] not in forms[t]) if text.startswith("!") else (text in forms[t]), (t.name, forms[t], text)
        kernels[t].dispatch(bufs, stream=stream, workspace=ws, **kw)
    torch.cuda.synchronize()
    raw = {op.description: bufs[op].double().cpu().numpy() for op in (Op.O, Op.L, Op.D, Op.dQ, Op.dK, Op.dV)}
    for name, x in raw.items():
        assert np.isnan(x[B]).all(), "%s: the canary entry behind the buffer was written" % name
    got = {name: x[:B] for name, x in raw.items()}
    got["L"] = got["L"] / train_model.LOG2E                 # stored in log2 units
    got["D"] = got["D"] * math.sqrt(D)                      # stored times the softmax scale
    at_one, _padding, _text = compare(got, ref, margin=1, info=info)
    worst, padding, text = compare(got, ref, info=info)
    print("train parity %s %s: err / bound at margin 1: %s; pieces %s; %s" % (
        c["mode"], (R, C, D, B, H), " ".join("%s %.3f" % kv for kv in at_one.items()), {t.name: n for t, n in counts.items()},
        " | ".join(forms[t].split(" (")[0] for t in (FWD, DQ, DKV))))
    assert all(padding.values()), "rows or keys past a per-batch length were written:\n" + text
    assert max(worst.values()) <= 1.0, "outside the bound at margin %d (%s):\n%s" % (MARGIN, [kernels[t].variant for t in kernels], text)
