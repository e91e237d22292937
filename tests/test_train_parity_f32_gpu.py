"""GPU parity of the FP32 training kernels under the per-element FP32 bound of tests/train_model.py (fmt = "f32"), on its needle inputs.

Every case goes through test_train_parity_gpu.run_case: every output buffer full of NaN, one spare batch entry as the canary, the
padding behind every per-batch length held to the sentinel, all six outputs compared at every element of every live row and key, the
`variant` and the `launchForm` asserted, the worst err / bound at margin 1 printed.  A spike or shift case first proves on the CPU,
from train_model.emulated()'s walk, that its inputs take the forward's re-base branch (attn_f32.h `grow`) behind tile 0 in some but
not all rows of a wave (train_model.rebase_proof / check_rebase_proof).  tests/test_train_sensitivity.py part (f) proves on the CPU
that this check sees each named wrong kernel, the six mutants of the re-base branch among them.

attn_f32_{fwd,dq,dkv}_{d64,d128} (csrc/attn_f32.h: two LDS stages in the forward, three in the backward kernels, 32-wide tiles, 128
rows or keys per workgroup): dense and causal at both head blocks and below them (zero-filled chunks); every forward tile count 1 .. 5
and both stage parities; dK / dV traversals of 1 .. 5 row tiles with fewer and more than 128 keys; one row, one key, a row block of
one row; causal with C > R and C = R; per-batch lengths; grids whose head count is and is not a multiple of 8; grouped K / V heads;
the spike family and the shift; config 3's own shape.  Then the other FP32 launch forms, which stay on the general kernels of
attn_generic.h (the same instruction, the same 32-wide tiles: the same chain term): the 32 and 256 head blocks, a transposed operand,
a leading dimension that is not 16-byte aligned, the 384 row and one D beyond it.
"""
import pytest

from metal_flash_attention_amd import AttentionOperand as Op
from test_train_parity_gpu import DKV, DQ, FWD, case, run_case

pytestmark = pytest.mark.gpu
F32 = ("f32",)
L3R, L3C = [300, 77, 1], [333, 100, 64]          # per-batch lengths: an entry shorter than a workgroup, a one-row entry, fewer keys than rows


def own(D):
    """the code objects of attn_f32.h that a row-major, aligned FP32 launch of head dimension D must run"""
    block = "_d64" if D <= 64 else "_d128"
    return {FWD: "^attn_f32_fwd" + block, DQ: "^attn_f32_dq" + block, DKV: "^attn_f32_dkv" + block}


def general(tag, why=""):
    """the general kernel of head block `tag` that the launch must stay on (`why`: the reason the library's form text gives)"""
    return {t: "^attn_generic_%s_f32mfma_%s|!attn_f32_%s" % (name, tag, "|" + why if why else "") for t, name in ((FWD, "fwd"), (DQ, "dq"), (DKV, "dkv"))}


PAGED = {FWD: "^attn_paged_fwd_f32_any_d", DQ: "^attn_paged_dq_f32_any_d", DKV: "^attn_paged_dkv_f32_any_d"}
UNALIGNED = "rows are not 16-byte aligned"


def f32(name, R, C, D, **kw):
    kw.setdefault("form", own(D))
    return case(name, R, C, D, F32, **kw)


def cases():
    out = []
    # ---- dense and causal at both head blocks and below them
    for D in (128, 64):
        out += f32("dense", 300, 333, D, H=2) + f32("causal", 300, 333, D, H=2, causal=True)
    out += f32("below-block-one-row-block", 129, 131, 100) + f32("below-block-causal", 160, 225, 72, causal=True)
    out += f32("d4", 64, 64, 4, form=general("d32")) + f32("d4-causal", 64, 64, 4, causal=True, form=general("d32"))     # (D <= 32: the 32 head block has no code object of its own)
    # ---- forward tile counts 1 .. 5, both stage parities, rings shorter than the prologue (dQ: residues of the tile count mod 3)
    for i, C in enumerate((1, 31, 32, 33, 64, 65, 96, 97, 131)):
        out += f32("tiles", 40, C, (128, 64)[i % 2])
    for i, C in enumerate((33, 65, 97)):
        out += f32("tiles-causal", C, C, (64, 128)[i % 2], causal=True)
    # ---- dK / dV traversals of 1 .. 5 row tiles; 100 keys: a workgroup with an empty wave; 200 keys: two workgroups
    for i, R in enumerate((20, 64, 95, 128, 131)):
        out += f32("row-tiles", R, 100, (128, 64)[i % 2]) + f32("row-tiles", R, 200, (64, 128)[i % 2])
    out += f32("one-row", 1, 97, 64) + f32("one-key", 33, 1, 64)
    out += f32("causal-offset", 160, 225, 128, causal=True) + f32("causal-square", 255, 255, 64, causal=True)
    # ---- per-batch lengths
    for D in (128, 64):
        out += f32("lengths", 300, 333, D, B=3, H=2, rl=L3R, cl=L3C) + f32("lengths-causal", 300, 333, D, B=3, H=2, causal=True, rl=L3R, cl=L3C)
    # ---- the two branches of fwd16_decode_block: a head count that is, and one that is not, a multiple of 8
    out += f32("grid-8-heads", 150, 160, 64, B=2, H=8) + f32("grid-11-heads", 150, 160, 128, B=3, H=11, causal=True)
    out += f32("grid-ragged", 300, 160, 128, B=12, H=11)
    # ---- grouped K / V heads: kv_head in all three kernels, the group sum
    out += f32("grouped", 255, 257, 64, H=8, G=4) + f32("grouped-causal", 255, 257, 128, B=2, H=8, G=4, causal=True)
    # ---- the re-base branch: the spike family and the shift, two heads (the spike positions differ per head)
    for D in (128, 64):
        for spike in ("a", "b", "c", "e", "f"):
            out += f32("spike-" + spike, 300, 333, D, H=2, spike=spike) + f32("spike-%s-causal" % spike, 300, 333, D, H=2, spike=spike, causal=True)
        out += f32("spike-d-causal", 300, 333, D, H=2, spike="d", causal=True)       # (the diagonal tile: causal only)
        out += f32("shift", 300, 333, D, H=2, spike="a", shift=60.0) + f32("shift-causal", 300, 333, D, H=2, spike="a", shift=60.0, causal=True)
    out += f32("shift-deep", 300, 333, 128, H=2, spike="a", shift=100.0)             # beyond FP32's exponent range (87 nats)
    out += f32("spike-e-lengths", 300, 333, 128, B=3, H=2, spike="e", causal=True, rl=L3R, cl=L3C)
    # ---- BASELINE config 3's own shape
    out += f32("config3", 4096, 4096, 128)
    # ---- the other FP32 launch forms: the general kernels
    out += f32("block32", 150, 200, 32, H=2, spike="a", form=general("d32")) + f32("block32-causal", 150, 200, 28, causal=True, form=general("d32"))
    out += f32("block256", 150, 200, 200, H=2, spike="a", causal=True, form=general("d256")) + f32("block256", 150, 200, 256, form=general("d256"))
    out += f32("transposed-K", 150, 200, 64, H=2, spike="a", tr=(False, True, False, False), form=general("d64"))
    out += f32("transposed-QO-causal", 150, 200, 128, causal=True, tr=(True, False, False, True), form=general("d128"))
    out += f32("unaligned-ld", 150, 200, 64, H=2, spike="a", ld={Op.K: 65}, form=general("d64", UNALIGNED))
    out += f32("unaligned-ld-causal", 150, 200, 128, causal=True, ld={Op.V: 129}, form=general("d128", UNALIGNED))
    out += f32("row384", 150, 200, 320, H=2, spike="a", form=general("d384")) + f32("row384-causal", 150, 200, 384, causal=True, form=general("d384"))
    out += f32("beyond384", 150, 200, 400, H=2, spike="a", form=PAGED) + f32("beyond384-causal", 150, 200, 400, causal=True, form=PAGED)
    return out


CASES = cases()


@pytest.mark.parametrize("c", CASES)
def test_fp32_kernels_inside_the_per_element_bounds(c):
    run_case(c)
