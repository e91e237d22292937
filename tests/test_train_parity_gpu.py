"""GPU parity of the training kernels (forward, dQ, dK/dV) under the per-element bounds of tests/train_model.py, on its needle inputs.

Every case launches the three kernels of one descriptor through the C ABI on a [B, H] grid (every output buffer full of NaN, one
spare batch entry behind each as the canary), compares ALL six outputs of the launch with train_model.compare -- every element of
every live row and key under the bound at the committed margin, the padding and the canary against the sentinel -- and prints the
worst err / bound at margin 1.  Each case asserts the `variant` and the `launchForm` it means to test, so that a shape cannot slide
onto another kernel unnoticed.  tests/test_train_sensitivity.py proves on the CPU that this check sees each named wrong kernel.

run_case() is the one runner: tests/test_train_parity_mask_gpu.py (block masks: the model and the inputs take the mask, the mask
buffer is poisoned around every head's words) and tests/test_train_parity_transposed_gpu.py (transposed operands: only the buffers'
layout changes; the padding of every leading dimension is NaN before and after) build their cases with case() and run them here.

The mode "f32" (tests/test_train_parity_f32_gpu.py) runs FP32 operands under the model's FP32 bound and margin; a spike case of it
proves on the CPU, before the launch, that its inputs take the FP32 forward's re-base branch (train_model.rebase_proof).
FP16 cases store dO in FP16 next to FP16 Q / K / V (the model's one 16-bit type).  The launch forms of the torch binding
(tests/test_train_parity_binding_forms_gpu.py): out16= stores O, dQ, dK, dV in the inputs' type (lowPrecisionOutputs; D is then formed
from the stored O, and the model's bound says so); the modes "f16mix-mixed" / "f16mix-exact" store dO in BF16 next to FP16 Q / K / V, as
memoryPrecisions says, and the case names the path of its backwardKeyValue kernel (train_model.MIX_PATH); G= runs a grouped grid: K, V,
dK, dV lie in buffers of H heads of which the first H / G are live, a finite canary (K, V) or the sentinel (dK, dV) behind them, the
workspace of the group sum is poisoned and has a canary behind it.  A split or grouped launch with 16-bit outputs is also held BY BITS to
the rounding of what the same launch stores with that output in FP32 (O, dQ, dK and dV of a split launch -- backwardQuery reads the
same 16-bit O both times --, dK and dV of a grouped one): the cast happens once, in a combine kernel or in attn_kv_group_sum, which
no bound can see (tests/test_train_sensitivity.py FORM_UNRESOLVED).
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
MIX_MODES = {"f16mix-mixed": ("f16", True), "f16mix-exact": ("f16", False)}      # dO in BF16 next to FP16 Q / K / V
F32_MODES = {"f32": ("f32", False)}          # FP32 operands (tests/test_train_parity_f32_gpu.py): lowPrecisionInputs = False
KV_CANARY = -3.0             # K / V heads behind the live ones of a grouped grid: finite, so that a launch that reads them computes wrong values
SMALL_ROWS = slice(64, 128)  # small=True: the dO of these rows is scaled by 2^-12 (below FP16's normal range in part)
_MODELS = {}


def case(name, R, C, D, modes, *, B=1, H=1, causal=False, rl=None, cl=None, workspace=False, rows=(), spike=False, variant=None, form=None,
         mask=None, tr=None, ld=None, only=None, out16=False, G=1, path=None, small=False, shift=None):
    """variant / form: {kernel type: text the kernel's variant / the launch's form must contain; form: several joined by |, a leading !
    for text it must not contain, a leading ^ for text it must start with}.
    mask: None or dict(per="shared" | "head" | "batch" | "both", seed=, empty_last=, need_blocks=): a block mask of
    train_model.needle_mask, one for the grid or one per head / batch entry / both (pairwise different), passed with non-zero
    blockMaskStrides wherever it is not shared.
    tr: transposeState (Q, K, V, O): operand X^T lies [D][leading dimension] per head (dQ follows Q, dK K, dV V, dO O).
    ld: {operand: leading dimension} (default: the sequence length of a transposed operand, D of a row-major one); the padding columns
    hold NaN, in inputs and outputs.  only: the kernel types to run (default all three).
    out16: O, dQ, dK, dV in the inputs' type.  G: headsPerKeyValue (H query heads over H / G K / V heads).  path: the f16mix modes' path of
    the backwardKeyValue kernel ("convert_dO" | "bf16_products"), asserted against train_model.MIX_PATH.  small: SMALL_ROWS of dO x 2^-12.
    spike: True or, FP32, a member of train_model.SPIKES; shift (FP32): nats, train_model.needle_inputs."""
    return [pytest.param(dict(R=R, C=C, D=D, B=B, H=H, causal=causal, rl=rl, cl=cl, workspace=workspace, rows=rows, spike=spike,
                              variant=variant or {}, form=form or {}, mode=m, mask=mask, tr=tuple(tr or (False,) * 4), ld=ld or {},
                              only=tuple(only or (FWD, DQ, DKV)), out16=out16, G=G, path=path, small=small, shift=shift),
                         id="%s-%dx%dx%d-%s" % (name, R, C, D, m)) for m in modes]


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


def _kernels(c, fmt, mixed, fp32=None):
    """-> {kernel type: kernel}, {operand: precision}.  fp32: {kernel type: its outputs kept in FP32} on the case's descriptor (the by-bits
    launches: every input keeps its type, backwardQuery's 16-bit O too)"""
    desc = AttentionDescriptor()
    desc.lowPrecisionInputs, desc.lowPrecisionIntermediates = fmt != "f32", mixed
    desc.matrixDimensions = (c["R"], c["C"], c["D"])
    desc.transposeState = c["tr"]
    if fmt != "f32":
        desc.lowPrecisionInputType = P.BF16 if fmt == "bf16" else P.FP16
    desc.lowPrecisionOutputs = bool(c.get("out16"))
    kernels, precisions = {}, {}
    with parameter_rows(*c["rows"]):
        for t in c["only"]:
            kdesc = desc.kernelDescriptor(t)
            if fmt == "f16" and Op.dO in kdesc.memoryPrecisions and not c["mode"].startswith("f16mix"):
                kdesc.memoryPrecisions[Op.dO] = P.FP16
            for name in (fp32 or {}).get(t, ()):
                op = next(o for o in kdesc.memoryPrecisions if o.description == name)
                kdesc.memoryPrecisions[op] = P.FP32
            kernels[t] = AttentionKernel(kdesc)
            precisions.update({op: P(int(p)) for op, p in kdesc.memoryPrecisions.items()})
    return kernels, precisions


def _pieces(c, kernels):
    """the library's own plan for this launch, from the workspace each kernel asks for"""
    counts = {t: train_model.piece_count(kernels[t], name, c["R"], c["C"], c["D"], c["H"], c["B"])
              for t, name in zip((FWD, DQ, DKV), train_model.KERNEL_TYPES) if t in kernels}
    named = {name: counts[t] for t, name in zip((FWD, DQ, DKV), train_model.KERNEL_TYPES) if t in kernels}
    return train_model.pieces_of(named, c["R"], c["C"]), counts


def block_mask_of(c):
    """None, or the case's mask as bool [B, H, row blocks, column blocks] (what the model takes)"""
    m = c["mask"]
    if m is None:
        return None
    B, H = c["B"], c["H"]
    kw = dict(causal=c["causal"], empty_last=m.get("empty_last", False), need_blocks=m.get("need_blocks", ()))
    distinct = {"shared": 1, "head": H, "batch": B, "both": B * H}[m["per"]]
    masks, seed = [], m.get("seed", 0)
    while len(masks) < distinct:                             # (a small mask has few admissible patterns: draw until all differ)
        one = train_model.needle_mask(c["R"], c["C"], seed, **kw)
        seed += 1
        if not any(np.array_equal(one, x) for x in masks):
            masks.append(one)
    grid = {"shared": lambda b, h: 0, "head": lambda b, h: h, "batch": lambda b, h: b, "both": lambda b, h: b * H + h}[m["per"]]
    bits = np.array([[masks[grid(b, h)] for h in range(H)] for b in range(B)])
    assert len({x.tobytes() for x in bits.reshape((-1,) + bits.shape[2:])}) == distinct, "the masks of the grid are pairwise different"
    return bits


POISON = 0xA5C3965A          # mask words no launch may read: one before the first mask, between the heads' masks, behind the last


def mask_buffer(c, bits):
    """-> int32 array (the first word is poison: the launch gets the address of word 1), words per row block, (head, batch) strides"""
    B, H = c["B"], c["H"]
    packed = train_model.pack_mask(bits)                     # [B, H, row blocks, words]
    nrb, words = packed.shape[2:]
    per_head, per_batch = c["mask"]["per"] in ("head", "both"), c["mask"]["per"] in ("batch", "both")
    hs = nrb * words + 3 if per_head else 0
    bs = ((H * hs if per_head else nrb * words) + 5) if per_batch else 0
    nb, nh = (B if per_batch else 1), (H if per_head else 1)
    buf = np.full(1 + (nb - 1) * bs + (nh - 1) * hs + nrb * words + 4, POISON, dtype=np.uint32)
    for b in range(nb):
        for h in range(nh):
            at = 1 + b * bs + h * hs
            buf[at:at + nrb * words] = packed[b, h].reshape(-1)
    return buf.view(np.int32), words, (hs, bs)


def _problem(c, fmt, mixed, pieces, block_mask=None):
    """needle inputs and the float64 model of a case, computed once per (case, type, mode, launch form)"""
    mix = c["mode"].startswith("f16mix")
    out = fmt if c.get("out16") else "f32"
    form = (out, mix, c.get("path"), c.get("G", 1), bool(c.get("small")))
    key = (c["R"], c["C"], c["D"], c["B"], c["H"], c["causal"], str(c["rl"]), str(c["cl"]), c["spike"], c.get("shift"), fmt, mixed, str(pieces),
           None if block_mask is None else block_mask.tobytes(), form)
    if key not in _MODELS:
        geo = dict(causal=c["causal"], row_lengths=c["rl"], key_lengths=c["cl"], pieces=pieces)
        if block_mask is not None:
            geo["block_mask"] = block_mask
        extra = {}
        shifted = {} if c.get("shift") is None else dict(shift=c["shift"])
        if form != ("f32", False, None, 1, False):             # (the former cases call exactly what they called)
            extra = dict(dO_fmt="bf16" if mix else None, heads_per_kv=c.get("G", 1))
        q, k, v, dO, info = train_model.needle_inputs(c["B"], c["H"], c["R"], c["C"], c["D"], fmt, spike=c["spike"], seed=c["R"] + c["D"],
                                                      **(dict(extra, small_dO_rows=SMALL_ROWS if c.get("small") else None) if extra else {}), **shifted, **geo)
        if extra:
            extra.update(out=out, dO_path=c.get("path") if mix else None)
        _MODELS[key] = (q, k, v, dO, info, train_model.model(q, k, v, dO, fmt=fmt, mixed=mixed, **extra, **geo))
    return _MODELS[key]


TORCH_TYPE = {P.FP32: "float32", P.FP16: "float16", P.BF16: "bfloat16"}
SEQ = {Op.Q: "R", Op.O: "R", Op.dO: "R", Op.dQ: "R", Op.K: "C", Op.V: "C", Op.dK: "C", Op.dV: "C"}


def run_case(c, device="cuda", launch=True):
    """launch the case's kernels and hold all their outputs to the model's bounds (see the module's docstring) -> the launch forms.
    launch=False (any device): the forms only, nothing is started"""
    import time
    import torch
    fmt, mixed = {**MODES, **MIX_MODES, **F32_MODES}[c["mode"]]
    R, C, D, B, H = c["R"], c["C"], c["D"], c["B"], c["H"]
    G, out16, mix = c.get("G", 1), bool(c.get("out16")), c["mode"].startswith("f16mix")
    Hkv = H // G
    kernels, prec = _kernels(c, fmt, mixed)
    for t, text in c["variant"].items():
        assert text in kernels[t].variant, (t.name, kernels[t].variant, text)
    if mix:
        assert prec[Op.dO] == P.BF16 and train_model.mix_path(kernels[DKV].variant) == c["path"], (kernels[DKV].variant, c["path"])
    if out16:
        assert all(prec[op] == (P.BF16 if fmt == "bf16" else P.FP16) for op in (Op.O, Op.dQ, Op.dK, Op.dV) if op in prec), prec
    transposed = any(c["tr"])
    pieces, counts = _pieces(c, kernels) if c["workspace"] and not transposed else (None, {})
    bits = block_mask_of(c)
    if launch:
        q, k, v, dO, info, ref = _problem(c, fmt, mixed, pieces, bits)
        if fmt == "f32" and c["spike"]:      # before anything is launched: the inputs do take the forward's re-base branch (train_model.rebase_proof)
            proof = train_model.rebase_proof(q, k, v, dO, causal=c["causal"], row_lengths=c["rl"], key_lengths=c["cl"], heads_per_kv=G)
            train_model.check_rebase_proof(proof, c["spike"], c.get("shift"), C, whole=c["rl"] is None)
    else:                        # the forms only: they depend on the buffers' shapes, types and strides, not on their values
        q, dO = np.zeros((B, H, R, D)), np.zeros((B, H, R, D))
        k, v = np.zeros((B, Hkv, C, D)), np.zeros((B, Hkv, C, D))
    tq, tk, tv, to = c["tr"]
    tr_of = {Op.Q: tq, Op.dQ: tq, Op.K: tk, Op.dK: tk, Op.V: tv, Op.dV: tv, Op.O: to, Op.dO: to}
    ld_of = {op: c["ld"].get(op, c[SEQ[op]] if tr_of[op] else D) for op in SEQ}
    KV = (Op.K, Op.V, Op.dK, Op.dV)

    def shape_of(op):            # [rows][leading dimension] per head: X^T is [D][ld], X is [sequence][ld]; always H heads (a grouped grid: H / G live)
        return (H, D if tr_of[op] else c[SEQ[op]], ld_of[op])

    def view(x, op):             # the [.., sequence, D] view of a buffer laid out by shape_of
        return x[..., :c[SEQ[op]]].swapaxes(-1, -2) if tr_of[op] else x[..., :D]

    def pad(x, op):
        return x[..., (c[SEQ[op]] if tr_of[op] else D):]

    def live(x, op):             # the live heads of a [B, H, ...] buffer
        return x[:, :Hkv] if op in KV else x

    def dev_in(x, op):
        host = np.full((B,) + shape_of(op), np.nan, dtype=np.float32)
        if op in KV and G > 1:
            host[:, Hkv:] = KV_CANARY
        view(live(host, op), op)[...] = x
        return torch.from_numpy(host).to(getattr(torch, TORCH_TYPE[prec[op]])).to(device)

    def dev_out(op, *shape, dtype=None):     # B live entries and one spare entry, the canary: all NaN
        return torch.full((B + 1,) + (shape or shape_of(op)), float("nan"), device=device, dtype=dtype or getattr(torch, TORCH_TYPE[prec[op]]))

    bufs = {Op.Q: dev_in(q, Op.Q), Op.K: dev_in(k, Op.K), Op.V: dev_in(v, Op.V), Op.dO: dev_in(dO, Op.dO),
            Op.O: dev_out(Op.O), Op.L: dev_out(Op.L, H, R), Op.D: dev_out(Op.D, H, R),
            Op.dQ: dev_out(Op.dQ), Op.dK: dev_out(Op.dK), Op.dV: dev_out(Op.dV)}
    for op, x in ((Op.Q, q), (Op.K, k), (Op.V, v), (Op.dO, dO)):
        assert np.array_equal(view(live(bufs[op].double().cpu().numpy(), op), op), x), "the inputs must reach the device exactly"
    hs = {op: int(np.prod(shape_of(op)[1:])) for op in SEQ}
    hs.update({Op.L: R, Op.D: R})
    bs = {op: s * H for op, s in hs.items()}
    kw = dict(row=R, column=C, heads=H, batches=B, headStrides=hs, batchStrides=bs, causal=c["causal"])
    if G > 1:
        kw["headsPerKeyValue"] = G
    if transposed or c["ld"]:
        kw["leadingDimensions"] = {op: n for op, n in ld_of.items() if tr_of[op] or op in c["ld"]}
    if c["rl"] is not None:
        kw["rowLengths"] = torch.tensor(c["rl"], dtype=torch.int32, device=device)
        kw["columnLengths"] = torch.tensor(c["cl"], dtype=torch.int32, device=device)
    if bits is not None:
        words_host, words, strides = mask_buffer(c, bits)
        mask_dev = torch.from_numpy(words_host).to(device)
        kw.update(blockMask=mask_dev[1:], blockMaskWords=words, blockMaskStrides=strides)
    stream = torch.cuda.current_stream().cuda_stream if launch else None
    forms, spaces = {}, {}
    size_kw = dict(row=R, column=C, heads=H, batches=B, **({"headsPerKeyValue": G} if G > 1 else {}))

    def workspace_of(kernel, t):
        """None, or a workspace of 0xFF bytes (NaN in every type) with 256 canary bytes behind it; a grouped backwardKeyValue always has one"""
        if not (c["workspace"] or (G > 1 and t == DKV)):
            return None, 0
        need = kernel.workspaceSize(**size_kw)
        if not need:
            return None, 0
        room = torch.full((need + 512,), 0xFF, dtype=torch.uint8, device=device)
        at = -room.data_ptr() % 256                        # (the library asks for a 256-byte aligned workspace; a host allocation may not be)
        return room[at:at + need + 256], need

    began = time.perf_counter()
    for t in c["only"]:
        ws, need = workspace_of(kernels[t], t)
        if ws is not None or c["workspace"]:
            spaces[t] = (ws, need)
        forms[t] = kernels[t].launchForm(bufs, workspace=ws, **kw)
        for text in c["form"].get(t, "").split("|") if t in c["form"] else ():
            ok = (text[1:] not in forms[t]) if text.startswith("!") else forms[t].startswith(text[1:]) if text.startswith("^") else (text in forms[t])
            assert ok, (t.name, forms[t], text)
        if G > 1 and t == DKV:
            assert forms[t].endswith(" + attn_kv_group_sum x%d" % G), forms[t]
        if launch:
            kernels[t].dispatch(bufs, stream=stream, workspace=ws, **kw)
    if not launch:
        return forms
    torch.cuda.synchronize()
    spent = time.perf_counter() - began
    for t, (ws, need) in spaces.items():
        assert ws is None or bool((ws[need:] == 0xFF).all()), "%s: the canary behind the workspace was written" % t.name
    if bits is not None:
        assert np.array_equal(mask_dev.cpu().numpy(), words_host), "the mask buffer was written"
    outputs = tuple(n for n, t in (("O", FWD), ("L", FWD), ("D", DQ), ("dV", DKV), ("dK", DKV), ("dQ", DQ)) if t in c["only"])
    ops = {op.description: op for op in (Op.O, Op.L, Op.D, Op.dQ, Op.dK, Op.dV)}
    raw = {name: bufs[ops[name]].double().cpu().numpy() for name in outputs}
    got = {}
    for name, x in raw.items():
        assert np.isnan(x[B]).all(), "%s: the canary entry behind the buffer was written" % name
        if ops[name] in SEQ:
            assert np.isnan(pad(x[:B], ops[name])).all(), "%s: the padding of the leading dimension was written" % name
            assert np.isnan(x[:B, Hkv:]).all() or ops[name] not in KV, "%s: a head behind the live K / V heads was written" % name
            got[name] = np.ascontiguousarray(view(live(x[:B], ops[name]), ops[name]))
        else:
            got[name] = x[:B]
    if G > 1:
        for op in (Op.K, Op.V):
            assert bool((bufs[op][:, Hkv:].float() == KV_CANARY).all()), "%s: the heads behind the live ones were written" % op.name
    if out16 and (c["workspace"] or G > 1):
        # by bits: the same launch with that output in FP32 -- every input the same buffer, backwardQuery's 16-bit O included, so that it
        # forms the same D -- rounded once as the launch's store rounds (train_model.STORE_ROUNDING): the 16-bit cast of a split or
        # grouped launch happens in attn_fwd_combine / attn_bwd_combine / attn_kv_group_sum, after the FP32 sum
        held = {FWD: ("O",), DQ: ("dQ",), DKV: ("dV", "dK")}
        again = tuple(t for t in c["only"] if c["workspace"] or t == DKV)
        wide, _prec = _kernels(dict(c, only=again), fmt, mixed, fp32=held)
        for t in again:
            mine = dict(bufs)
            for name in held[t]:
                mine[ops[name]] = dev_out(ops[name], dtype=torch.float32)
            if t == FWD:
                mine[Op.L] = dev_out(Op.L, H, R)
            ws, need = workspace_of(wide[t], t)
            assert wide[t].launchForm(mine, workspace=ws, **kw) == forms[t], (wide[t].launchForm(mine, workspace=ws, **kw), forms[t])
            wide[t].dispatch(mine, stream=stream, workspace=ws, **kw)
            torch.cuda.synchronize()
            for name in held[t]:
                x32 = view(live(mine[ops[name]].double().cpu().numpy()[:B], ops[name]), ops[name])
                want = train_model.round_to(np.nan_to_num(x32, nan=0.0), fmt, trunc=fmt == "bf16" and train_model.store_rounding(forms[t]) == "trunc")
                same = np.where(np.isnan(x32), np.isnan(got[name]), got[name] == want)
                assert same.all(), "%s: the %s store of %s is not the rounding of its FP32 store at %d elements, the first at %s" % (
                    forms[t], fmt, name, int((~same).sum()), tuple(int(i) for i in np.argwhere(~same)[0]))
    if "L" in got:
        got["L"] = got["L"] / train_model.LOG2E                 # stored in log2 units
    if "D" in got:
        got["D"] = got["D"] * math.sqrt(D)                      # stored times the softmax scale
    out = fmt if out16 else "f32"
    at_one, _padding, _text = compare(got, ref, out=out, margin=1, info=info, outputs=outputs, fmt=fmt)
    worst, padding, text = compare(got, ref, out=out, info=info, outputs=outputs, fmt=fmt)
    print("train parity %s %s%s: err / bound at margin 1: %s; pieces %s; %s; %.3f s" % (
        c["mode"], (R, C, D, B, H), "".join((" out16" if out16 else "", " G=%d" % G if G > 1 else "", " " + c["path"] if mix else "")),
        " ".join("%s %.3f" % kv for kv in at_one.items()), {t.name: n for t, n in counts.items()},
        " | ".join(forms[t].split(" (")[0] for t in c["only"]), spent))
    assert all(padding.values()), "rows or keys past a per-batch length were written:\n" + text
    assert max(worst.values()) <= 1.0, "outside the bound at margin %d (%s):\n%s" % (train_model.margin_of(fmt), [kernels[t].variant for t in kernels], text)
    return forms


@pytest.mark.parametrize("c", CASES)
def test_training_kernels_inside_the_per_element_bounds(c):
    run_case(c)
