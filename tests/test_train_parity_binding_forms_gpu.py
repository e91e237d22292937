"""GPU parity of the launch forms the torch binding runs, under the per-element bounds of tests/train_model.py on its needle inputs.

torch_binding.flash_attention builds its 16-bit descriptors with lowPrecisionOutputs, hands dO over in BF16 (also next to FP16 Q / K /
V) and launches grouped grids whenever Hkv < H.  The runner, the bound, the margin and the checker are those of
tests/test_train_parity_gpu.py (run_case); here every case has at least one of

  out16   O, dQ, dK, dV stored in the inputs' type by every family's fused store (the hand-placed persistent forwards round BF16 to
          nearest, every other store truncates: train_model.STORE_ROUNDING); backwardQuery forms D from the STORED O, and the model's
          E_D says so; padding rows and the padding of a leading dimension of D + 8 keep the NaN sentinel in the 16-bit buffers;
  f16mix  dO in BF16 next to FP16 Q / K / V, on each family that has mix code, with the path of its backwardKeyValue kernel
          (train_model.MIX_PATH), once with FP32 and once with FP16 outputs; `small`: rows 64..127 of dO scaled by 2^-12, below FP16's
          normal range in part;
  G       a grouped grid (Hq = 4 over 2 K / V heads, Hq = 8 over 2), K / V / dK / dV heads behind the live ones a canary, the slab
          workspace poisoned; dK / dV with a leading dimension of D + 4 take the one-element form of the group sum
          (attn_kv_group_sum.hip wide_output: ld % 8 != 0).
A split or grouped case with 16-bit outputs is also held by bits to the rounding of its own FP32-output launch (run_case).
tests/test_train_sensitivity.py (e) proves on the CPU what this check sees of each named defect of these forms.

These are the smallest shapes at which each family still has a ragged last tile, a ragged row block and more than one tile.
"""
import pytest

from metal_flash_attention_amd import AttentionOperand
from test_attention_gpu import DKV_RS, DKV_W4, DQ_W4, FWD_8x32
from test_train_parity_gpu import DKV, DQ, FWD, L3C, L3R, case, run_case

pytestmark = pytest.mark.gpu
Op = AttentionOperand
P6 = {FWD: "attn_fwd16p6", DQ: "attn_dq16p4", DKV: "attn_dkv16p4"}
P4 = {FWD: "attn_fwd16p4", DQ: "attn_dq16p4", DKV: "attn_dkv16p4"}
P5 = {FWD: "attn_fwd16p5", DQ: "attn_dq16p5", DKV: "attn_dkv16p5"}
WIDE = {FWD: "attn_fwd16w_", DQ: "attn_dq16w_", DKV: "attn_dkv16w_"}
MIX = ("f16mix-mixed", "f16mix-exact")
SPLIT = {DQ: "column-parallel x", DKV: "column-parallel x"}


def outs(D, extra=8):
    return {op: D + extra for op in (Op.O, Op.dQ, Op.dK, Op.dV)}


CASES = (
    # ---- every 16-bit family with 16-bit outputs
    case("o16-p6", 255, 257, 64, ("bf16-mixed", "f16-exact"), out16=True, variant=P6, form={FWD: "attn_fwd16_p6"})
    + case("o16-p6-below-bucket", 300, 333, 40, ("bf16-mixed", "f16-mixed"), out16=True, variant=P6, form={FWD: "attn_fwd16_p6"})
    + case("o16-p4p", 300, 333, 128, ("bf16-mixed", "f16-exact"), out16=True, variant=P4, form={FWD: "attn_fwd16_p4p (persistent"})
    + case("o16-p4-causal-lengths", 300, 333, 128, ("bf16-mixed", "bf16-exact"), out16=True, B=3, H=2, causal=True, rl=L3R, cl=L3C, variant=P4,
           form={FWD: "attn_fwd16p4_|!persistent"})
    + case("o16-p4-below-bucket", 255, 257, 104, ("bf16-mixed", "f16-mixed"), out16=True, variant=P4)
    + case("o16-p5", 300, 333, 160, ("bf16-mixed", "f16-exact"), out16=True, variant=P5)
    + case("o16-p5-causal", 255, 257, 256, ("bf16-mixed", "f16-mixed"), out16=True, causal=True, variant=P5)
    + case("o16-wide", 255, 257, 320, ("bf16-mixed", "f16-exact"), out16=True, variant=WIDE)
    + case("o16-wide-causal", 255, 257, 384, ("bf16-mixed", "bf16-exact"), out16=True, causal=True, variant=WIDE)
    + case("o16-v3-8x32", 300, 333, 128, ("bf16-mixed", "f16-exact"), out16=True, rows=(FWD_8x32,), variant={FWD: "attn_fwd16v3"})
    + case("o16-rs", 300, 333, 128, ("bf16-mixed", "f16-exact"), out16=True, rows=(DKV_RS, DQ_W4), variant={DQ: "attn_dq16p4", DKV: "attn_dkv16rs"})
    + case("o16-w4", 255, 257, 64, ("bf16-mixed", "f16-exact"), out16=True, rows=(DKV_W4,), variant={DKV: "attn_dkv16_"})
    # ---- per-batch lengths on a [3, 2] grid: padding rows keep the sentinel in the 16-bit buffers
    + case("o16-lengths", 300, 333, 64, ("bf16-mixed", "f16-exact"), out16=True, B=3, H=2, rl=L3R, cl=L3C, variant=P6, form={FWD: "per-batch lengths"})
    + case("o16-lengths", 300, 333, 128, ("bf16-mixed",), out16=True, B=3, H=2, rl=L3R, cl=L3C, variant=P4, form={FWD: "per-batch lengths"})
    + case("o16-lengths", 300, 333, 256, ("bf16-mixed", "f16-mixed"), out16=True, B=3, H=2, rl=L3R, cl=L3C, variant=P5)
    # ---- split forms: the 16-bit cast happens in the combine kernels
    + case("o16-split", 513, 1024, 64, ("bf16-mixed", "f16-exact"), out16=True, workspace=True, variant=P6,
           form={**SPLIT, FWD: "column-parallel x|pieces by attn_fwd16_p6"})
    + case("o16-split", 513, 1030, 128, ("bf16-mixed", "f16-mixed"), out16=True, workspace=True, variant=P4,
           form={**SPLIT, FWD: "column-parallel x|pieces by attn_fwd16_p4,"})
    + case("o16-split", 513, 1030, 256, ("bf16-mixed", "bf16-exact"), out16=True, workspace=True, variant=P5, form={**SPLIT, FWD: "column-parallel x"})
    # ---- output leading dimensions of D + 8: a packed 16-bit store must not touch the neighbouring element
    + case("o16-ld", 255, 257, 64, ("bf16-mixed", "f16-exact"), out16=True, H=2, ld=outs(64), variant=P6)
    + case("o16-ld", 300, 333, 128, ("bf16-mixed",), out16=True, ld=outs(128), variant=P4)
    + case("o16-ld", 300, 333, 160, ("f16-mixed",), out16=True, ld=outs(160), variant=P5)
    # ---- a block mask of each kind
    + case("o16-mask-shared", 513, 1030, 128, ("bf16-mixed", "f16-exact"), out16=True, H=2, mask=dict(per="shared", seed=910),
           form={FWD: "(block-sparse sibling attn_fwd16v3_", DQ: "(block-sparse sibling attn_dq16_", DKV: "(block-sparse sibling attn_dkv16rs_"})
    + case("o16-mask-per-head", 300, 333, 64, ("bf16-mixed",), out16=True, B=2, H=3, mask=dict(per="head", seed=920),
           form={FWD: "(block-sparse sibling attn_fwd16v3_", DQ: "(block-sparse sibling attn_dq16_", DKV: "(block-sparse sibling attn_dkv16rs_"})
    # ---- the late dominant key that fires the deferred rescale
    + case("o16-spike", 300, 333, 128, ("bf16-mixed", "f16-exact"), out16=True, H=2, spike=True, variant=P4)
    # ---- the FP16 + BF16-dO mix: the mix streams of attn_dkv16_p4 / _p5 run the two dO products in BF16, every other kernel converts dO
    + case("mix-p4", 255, 257, 64, MIX, path="bf16_products", variant={DQ: "attn_dq16p4_f16_dObf16", DKV: "attn_dkv16p4_f16_dObf16"})
    + case("mix-p4-o16-causal", 255, 257, 64, MIX, path="bf16_products", out16=True, H=2, causal=True, variant={DKV: "attn_dkv16p4_f16_dObf16"})
    + case("mix-p4", 300, 333, 128, MIX, path="bf16_products", variant={DQ: "attn_dq16p4_f16_dObf16", DKV: "attn_dkv16p4_f16_dObf16"})
    + case("mix-p4-o16-causal-small", 300, 333, 128, MIX, path="bf16_products", out16=True, causal=True, small=True, variant={DKV: "attn_dkv16p4_f16_dObf16"})
    + case("mix-p5", 300, 333, 256, ("f16mix-mixed",), path="bf16_products", variant={DQ: "attn_dq16p5_f16_dObf16", DKV: "attn_dkv16p5_f16_dObf16"})
    + case("mix-p5-o16", 300, 333, 160, MIX, path="bf16_products", out16=True, variant={DQ: "attn_dq16p5_f16_dObf16", DKV: "attn_dkv16p5_f16_dObf16"})
    + case("mix-rs", 300, 333, 128, ("f16mix-mixed",), path="convert_dO", rows=(DKV_RS, DQ_W4), variant={DKV: "attn_dkv16rs_f16_dObf16"})
    + case("mix-rs-o16-small", 255, 257, 256, ("f16mix-exact",), path="convert_dO", out16=True, small=True, rows=(DKV_RS, DQ_W4), causal=True,
           variant={DKV: "attn_dkv16rs_f16_dObf16"})
    + case("mix-wide", 255, 257, 320, ("f16mix-exact",), path="convert_dO", variant={DQ: "attn_dq16w_f16_dObf16", DKV: "attn_dkv16w_f16_dObf16"})
    + case("mix-wide-o16", 255, 257, 384, ("f16mix-mixed",), path="convert_dO", out16=True, causal=True,
           variant={DQ: "attn_dq16w_f16_dObf16", DKV: "attn_dkv16w_f16_dObf16"})
    + case("mix-w4", 255, 257, 64, ("f16mix-exact",), path="convert_dO", rows=(DKV_W4,), variant={DKV: "attn_dkv16_f16_dObf16"})
    + case("mix-w4-o16-small", 255, 257, 64, ("f16mix-mixed",), path="convert_dO", out16=True, small=True, rows=(DKV_W4,), variant={DKV: "attn_dkv16_f16_dObf16"})
    # ---- grouped grids with 16-bit outputs
    + case("g2", 255, 257, 64, ("bf16-mixed", "f16-exact"), out16=True, H=4, G=2, variant=P6)
    + case("g4-causal", 300, 333, 128, ("bf16-mixed", "f16-mixed"), out16=True, H=8, G=4, causal=True, variant=P4)
    + case("g2-lengths", 300, 333, 256, ("bf16-mixed",), out16=True, B=3, H=4, G=2, rl=L3R, cl=L3C, variant=P5)
    + case("g4-lengths", 300, 333, 64, ("f16-exact",), out16=True, B=3, H=8, G=4, rl=L3R, cl=L3C, variant=P6)
    + case("g2-mask-per-head", 513, 1030, 128, ("bf16-mixed",), out16=True, H=4, G=2, mask=dict(per="head", seed=930))
    # (ld = 68 is no multiple of 8 elements: attn_kv_group_sum.hip wide_output() -- `v.ld % per16 == 0`, per16 = 8 for 16-bit outputs --
    # then selects attn_kv_group_sum<1>, one element per lane; launchForm prints " + attn_kv_group_sum x2" for both widths, so the case
    # cannot assert the width: if wide_output() changes, choose the leading dimension here again)
    + case("g2-one-element-sum", 255, 257, 64, ("bf16-mixed", "f16-exact"), out16=True, H=4, G=2, ld={Op.dK: 68, Op.dV: 68}, variant=P6)
    + case("g2-mix", 255, 257, 64, ("f16mix-mixed",), path="bf16_products", out16=True, H=4, G=2, variant={DKV: "attn_dkv16p4_f16_dObf16"})
)


@pytest.mark.parametrize("c", CASES)
def test_binding_launch_forms_inside_the_per_element_bounds(c):
    run_case(c)
