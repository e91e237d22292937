"""GPU parity of training launches on transposed operands (transposeState) under the per-element bounds of tests/train_model.py.

The model does not change; the buffers do (tests/test_train_parity_gpu.py run_case): operand X^T lies [D][leading dimension] per
head, the padding columns of the inputs hold NaN, transposed outputs (O^T, dQ^T, dK^T, dV^T) are NaN-filled and their padding must
still be NaN afterwards.  The needle inputs put the last-key needle into the chunk of K^T / V^T that straddles the end of the
sequence and into the last partial step of a gathered row.  Every case asserts the variant and the launch form it means to test:
the 8 x 32 kernel's in-place code objects (rows that are not 16-byte aligned are gathered element-wise), the hand-placed streams
attn_fwd16_p4_tr / attn_fwd16_p5_tr / attn_dq16_p4_tr / attn_dkv16_p4_tr, the re-layout pass (attn_relayout) around the matrix-core
kernels with a NaN-filled workspace and a canary behind it, and the general kernel where neither applies.
"""
import pytest

from metal_flash_attention_amd import AttentionOperand
from test_train_parity_gpu import DKV, DQ, FWD, case, run_case

pytestmark = pytest.mark.gpu
Op = AttentionOperand
ALL, QO, K_, V_, KV = (True,) * 4, (True, False, False, True), (False, True, False, False), (False, False, True, False), (False, True, True, False)


def odd(R, C, tr):
    """odd leading dimensions for the transposed operands: no row of X^T begins on a 16-byte boundary"""
    tq, tk, tv, to = tr
    ld = {}
    for ops, on, n in (((Op.Q, Op.dQ), tq, R + 1 + R % 2), ((Op.O, Op.dO), to, R + 3 + R % 2), ((Op.K, Op.dK), tk, C + 1 + C % 2), ((Op.V, Op.dV), tv, C + 3 + C % 2)):
        for op in ops:
            if on:
                ld[op] = n
    assert all(n % 2 == 1 for n in ld.values())
    return ld


def aligned(R, C, tr, pad=8):
    """leading dimensions `pad` elements (16 bytes) beyond the sequence: aligned rows with NaN padding behind every row"""
    tq, tk, tv, to = tr
    return {op: n + pad for ops, on, n in (((Op.Q, Op.dQ), tq, R), ((Op.O, Op.dO), to, R), ((Op.K, Op.dK), tk, C), ((Op.V, Op.dV), tv, C)) for op in ops if on}


P4TR, P5TR = "^attn_fwd16_p4_tr", "^attn_fwd16_p5_tr"
IN_PLACE = {FWD: P4TR, DQ: "^attn_dq16_p4_tr", DKV: "^attn_dkv16_p4_tr"}
RELAYOUT = {DQ: "^attn_relayout x", DKV: "^attn_relayout x"}

CASES = (
    # ---- the 8 x 32 forward's in-place code objects _tr, _tr_k, _tr_v, _tr_kv on gathered rows: key 202 sits in a straddling chunk
    case("v3-tr", 136, 203, 64, ("bf16-mixed", "f16-exact"), tr=QO, ld=odd(136, 203, QO), only=(FWD,), variant={FWD: "attn_fwd16v3"}, form={FWD: "^attn_fwd16v3|_tr"})
    + case("v3-tr-k", 136, 203, 128, ("f16-mixed", "bf16-exact"), tr=K_, ld=odd(136, 203, K_), only=(FWD,), variant={FWD: "_tr_k"}, form={FWD: "^attn_fwd16v3|_tr_k"})
    + case("v3-tr-v", 136, 203, 192, ("bf16-mixed", "f16-exact"), tr=V_, ld=odd(136, 203, V_), only=(FWD,), variant={FWD: "_tr_v"}, form={FWD: "^attn_fwd16v3|_tr_v"})
    + case("v3-tr-kv", 136, 203, 64, ("f16-mixed",), tr=ALL, ld=odd(136, 203, ALL), only=(FWD,), variant={FWD: "_tr_kv"}, form={FWD: "^attn_fwd16v3|_tr_kv"})
    + case("v3-tr-kv", 136, 203, 128, ("bf16-mixed", "f16-exact"), tr=ALL, ld=odd(136, 203, ALL), only=(FWD,), variant={FWD: "_tr_kv"}, form={FWD: "^attn_fwd16v3|_tr_kv"})
    + case("v3-tr-kv", 136, 203, 192, ("bf16-exact",), tr=ALL, ld=odd(136, 203, ALL), only=(FWD,), variant={FWD: "_tr_kv"}, form={FWD: "^attn_fwd16v3|_tr_kv"})
    # ---- attn_fwd16_p4_tr on K^T alone and on V^T alone ("folded" in the form iff mixed)
    + case("p4tr-k", 296, 456, 128, ("bf16-mixed",), tr=K_, only=(FWD,), variant={FWD: "_tr_k"}, form={FWD: P4TR + "|transposed K|folded"})
    + case("p4tr-k", 296, 456, 128, ("f16-exact",), tr=K_, only=(FWD,), variant={FWD: "_tr_k"}, form={FWD: P4TR + "|transposed K|!folded"})
    + case("p4tr-v", 296, 456, 128, ("f16-mixed",), tr=V_, only=(FWD,), variant={FWD: "_tr_v"}, form={FWD: P4TR + "|transposed V|folded"})
    + case("p4tr-v", 296, 456, 128, ("bf16-exact",), tr=V_, only=(FWD,), variant={FWD: "_tr_v"}, form={FWD: P4TR + "|transposed V|!folded"})
    + case("p4tr-k-causal", 200, 328, 104, ("f16-mixed",), causal=True, tr=K_, only=(FWD,), variant={FWD: "_tr_k"}, form={FWD: P4TR + "|transposed K|folded"})
    + case("p4tr-v-causal", 200, 328, 104, ("bf16-exact",), causal=True, tr=V_, only=(FWD,), variant={FWD: "_tr_v"}, form={FWD: P4TR + "|transposed V|!folded"})
    # ---- attn_fwd16_p5_tr
    + case("p5tr", 320, 448, 256, ("bf16-mixed",), tr=ALL, only=(FWD,), variant={FWD: "_tr_kv"}, form={FWD: P5TR + "|folded"})
    + case("p5tr", 300, 352, 152, ("f16-exact",), tr=KV, only=(FWD,), variant={FWD: "_tr_kv"}, form={FWD: P5TR + "|!folded"})
    # ---- in-place backward attn_dq16_p4_tr / attn_dkv16_p4_tr: no workspace, every operand transposed
    + case("bwd-in-place", 320, 448, 128, ("bf16-mixed", "f16-exact"), tr=ALL, form=IN_PLACE)
    + case("bwd-in-place-causal", 320, 448, 128, ("f16-mixed",), causal=True, tr=ALL, form=IN_PLACE)
    + case("bwd-in-place", 256, 256, 104, ("f16-mixed",), tr=ALL, form=IN_PLACE)
    + case("bwd-in-place-causal", 256, 256, 104, ("bf16-mixed", "bf16-exact"), causal=True, tr=ALL, form=IN_PLACE)
    # ---- a [B, H] grid through head and batch strides on transposed operands
    + case("bwd-in-place-grid", 320, 448, 128, ("bf16-mixed",), B=2, H=3, tr=ALL, form=IN_PLACE)
    # ---- the re-layout pass around the matrix-core kernels: a workspace full of NaN, a canary behind it
    + case("relayout", 300, 449, 128, ("bf16-mixed", "f16-exact"), tr=ALL, workspace=True, form=RELAYOUT)
    + case("relayout", 150, 200, 256, ("bf16-exact", "f16-mixed"), tr=ALL, ld=aligned(150, 200, ALL), workspace=True, form=RELAYOUT)
    + case("relayout-wide", 150, 200, 320, ("bf16-mixed",), tr=ALL, workspace=True, form={FWD: "^attn_relayout x", DQ: "^attn_relayout x", DKV: "^attn_relayout x"})
    # ---- no workspace and not a launch the in-place kernels take: the general kernel, same bound
    + case("general", 300, 449, 128, ("bf16-mixed",), tr=ALL, form={DQ: "general kernel", DKV: "general kernel"})
    # ---- per-batch lengths on transposed K / V in the forward: the padding is left alone
    + case("lengths", 200, 336, 128, ("bf16-mixed", "f16-exact"), B=2, H=2, rl=[200, 77], cl=[333, 100], tr=(False, True, True, True), only=(FWD,),
           variant={FWD: "_tr_kv"}, form={FWD: "_tr"})
)


@pytest.mark.parametrize("c", CASES)
def test_transposed_training_kernels_inside_the_per_element_bounds(c):
    run_case(c)
