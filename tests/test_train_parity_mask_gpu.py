"""GPU parity of block-masked training launches (mfa_launch_params.blockMask) under the per-element bounds of tests/train_model.py.

The runner, the bound, the margin and the checker are those of tests/test_train_parity_gpu.py (run_case): three kernels through the C
ABI on a [B, H] grid, NaN-filled outputs with a canary entry, all six outputs under the checker, every case asserting the variant and
the launch form it means to test -- the block-sparse code object, the block-sparse sibling or the general kernel.  Here the needle
inputs and the model take the mask (train_model.needle_mask: run edges, neighbouring row blocks that differ, dead rows), the mask lies
in a buffer with a poisoned word before it, between the heads' masks and behind it, and per-head / per-batch masks are pairwise
different and passed with non-zero blockMaskStrides.  tests/test_train_sensitivity.py proves on the CPU that this check sees each
named misreading of a mask (train_model.MASK_MUTANTS).

Shapes: (513, 1030) is three row blocks of the mask, the last of one row, and nine column blocks, the last of six keys; (257, 4224)
at D = 128 is 33 column blocks: two mask words, bits b and b + 32 opposite, key j and key j + 4096 scoring alike (code_layout).
"""
import pytest

from metal_flash_attention_amd import AttentionOperand
from test_attention_gpu import DKV_RS, DQ_W4, FWD_8x32
from test_train_parity_gpu import DKV, DQ, FWD, L3C, L3R, MODES, case, run_case

pytestmark = pytest.mark.gpu
Op = AttentionOperand
OWN = "(block-sparse code object)"
SHARED = dict(per="shared", seed=100)
# what the default tables run under a mask: the hand-placed variants hand the launch to their compiler-scheduled siblings
ALL_SPARSE = {FWD: "(block-sparse sibling attn_fwd16v3_", DQ: "(block-sparse sibling attn_dq16_", DKV: "(block-sparse sibling attn_dkv16rs_"}
GENERAL = {FWD: "general kernel", DQ: "general kernel", DKV: "general kernel"}

CASES = (
    # ---- one mask for the grid, density 0.4, every row block alive: every head-dimension bucket, a D below each bucket once
    case("shared", 513, 1030, 64, ("bf16-mixed", "f16-exact"), H=2, mask=SHARED, variant={FWD: "attn_fwd16", DQ: "attn_dq16", DKV: "attn_dkv16"}, form=ALL_SPARSE)
    + case("shared", 513, 1030, 128, MODES, H=2, mask=SHARED, variant={FWD: "attn_fwd16", DQ: "attn_dq16", DKV: "attn_dkv16"}, form=ALL_SPARSE)
    + case("shared", 513, 1030, 192, ("f16-mixed", "bf16-exact"), mask=SHARED, form=ALL_SPARSE)
    + case("shared", 513, 1030, 256, ("bf16-mixed", "f16-exact"), mask=SHARED, form=ALL_SPARSE)
    + case("shared-below-bucket", 513, 1030, 40, ("bf16-exact",), mask=SHARED, form=ALL_SPARSE)
    + case("shared-below-bucket", 513, 1030, 104, ("f16-mixed",), mask=SHARED, form=ALL_SPARSE)
    # ---- causal: active blocks left of, on and right of the diagonal
    + case("causal", 600, 600, 128, ("bf16-mixed", "f16-exact"), H=2, causal=True, mask=dict(per="shared", seed=200), form=ALL_SPARSE)
    + case("causal", 513, 1030, 256, ("bf16-mixed",), causal=True, mask=dict(per="shared", seed=201), form=ALL_SPARSE)
    # ---- an empty last row block: dead rows (O = dQ = D = 0 exactly, a hugely negative L)
    + case("empty-last", 513, 1030, 128, ("bf16-mixed", "f16-mixed"), H=2, mask=dict(per="shared", seed=300, empty_last=True), form=ALL_SPARSE)
    # ---- per-batch lengths: key lengths 100 and 64 end inside the active block 0, 333 inside the active block 2
    + case("lengths", 300, 333, 64, ("bf16-mixed", "f16-exact"), B=3, H=2, rl=L3R, cl=L3C, mask=dict(per="shared", seed=400, need_blocks=(0, 2)), form=ALL_SPARSE)
    + case("lengths", 300, 333, 128, ("bf16-mixed", "bf16-exact"), B=3, H=2, rl=L3R, cl=L3C, mask=dict(per="shared", seed=401, need_blocks=(0, 2)), form=ALL_SPARSE)
    # ---- a mask per head and per batch entry: six pairwise different masks, non-zero strides; head stride alone, batch stride alone
    + case("per-head-per-batch", 513, 1030, 128, ("bf16-mixed",), B=2, H=3, mask=dict(per="both", seed=500), form=ALL_SPARSE)
    + case("per-head-per-batch", 300, 333, 64, ("f16-exact",), B=2, H=3, mask=dict(per="both", seed=510), form=ALL_SPARSE)
    + case("per-head", 300, 333, 64, ("bf16-mixed",), B=2, H=3, mask=dict(per="head", seed=520), form=ALL_SPARSE)
    + case("per-batch", 513, 1030, 128, ("f16-mixed",), B=2, H=3, mask=dict(per="batch", seed=530), form=ALL_SPARSE)
    # ---- two mask words per row block
    + case("two-words", 257, 4224, 128, ("bf16-mixed", "f16-exact"), H=2, mask=dict(per="head", seed=600), form=ALL_SPARSE)
    # ---- beyond the block-sparse code objects: the general kernel, same bound
    + case("wide", 300, 333, 320, ("bf16-mixed",), mask=dict(per="shared", seed=700), form=GENERAL)
    + case("misaligned", 300, 333, 64, ("bf16-mixed",), H=2, mask=dict(per="head", seed=710), ld={Op.K: 65}, form=GENERAL)
    # ---- attn_dkv16_rs lists the active row blocks of a column block in LDS
    + case("rs", 513, 1030, 128, ("bf16-mixed", "bf16-exact"), rows=(DKV_RS, DQ_W4), mask=SHARED, variant={DKV: "attn_dkv16rs"},
           form={FWD: ALL_SPARSE[FWD], DQ: ALL_SPARSE[DQ], DKV: "^attn_dkv16rs|" + OWN})
    # ---- the compiler-scheduled kernels selected themselves: their own block-sparse code objects (attn_fwd16_v3.h, attn_bwd16.h)
    + case("own", 513, 1030, 128, ("bf16-mixed", "f16-exact"), rows=(FWD_8x32, DKV_RS, DQ_W4), mask=dict(per="shared", seed=810),
           variant={FWD: "attn_fwd16v3", DKV: "attn_dkv16rs"}, form={FWD: "^attn_fwd16v3|" + OWN, DKV: OWN})
    + case("rs-per-head", 513, 1030, 256, ("f16-exact", "bf16-mixed"), H=2, rows=(DKV_RS, DQ_W4), mask=dict(per="head", seed=800), variant={DQ: "attn_dq16_", DKV: "attn_dkv16rs"},
           form={FWD: ALL_SPARSE[FWD], DQ: "^attn_dq16_|" + OWN, DKV: "^attn_dkv16rs|" + OWN})
)


@pytest.mark.parametrize("c", CASES)
def test_block_masked_training_kernels_inside_the_per_element_bounds(c):
    run_case(c)
