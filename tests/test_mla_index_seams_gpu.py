"""The MLA sparse indexer on its step, stride, head and selection-round seams (marked gpu).  The cases, their operands as
they lie in memory -- poison included -- and the float64 reference are tests/mla_index_model.py's, the very arrays
tests/test_mla_index_sensitivity.py shows every named mutant to leave the bound on.  Logits: per element against float64 under the bound
of 4.30, no margin, inside a wider sentinel-filled allocation that must keep every sentinel the launch does not own; the multi-step plans
are asserted from launchForm, and every layout of a plan gives the same bits.  Selection: exactly numpy's lexsort.  The chain and the
hand-over to the sparse decode: bit for bit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import metal_flash_attention_amd as mfa  # noqa: E402
from metal_flash_attention_amd import AttentionMLAIndex, GEMMOperandPrecision as P  # noqa: E402

import mla_index_model as im  # noqa: E402

gpu = pytest.mark.gpu
DTYPE, PREC = {"bf16": torch.bfloat16, "f16": torch.float16}, {"bf16": P.BF16, "f16": P.FP16}
BITS = {}


def launch_kw(name):
    """the operands of a case on the device, exactly as mla_index_model.layout() lays them out, and the launch's keywords"""
    case, lay = im.ALL_CASES[name], im.layout(name)
    dt = DTYPE[case["fmt"]]
    q, k = torch.from_numpy(lay["q"]).to(dt).cuda(), torch.from_numpy(lay["k"]).to(dt).cuda()
    w = torch.from_numpy(lay["w"]).cuda()
    ldk, bsk, psk = lay["ks"]
    kw = dict(rows=lay["R"], column=lay["C"], indexHeads=lay["H"], batches=lay["B"], causal=case["causal"], weightStrides=lay["ws"],
              strides=dict(QI=lay["qs"], KI=(ldk, 0, bsk)), cacheLengths=torch.tensor(case["lens"], dtype=torch.int32).cuda())
    if lay["table"] is not None:
        kw.update(pageSize=case["page"], pageStride=psk, blockTable=torch.from_numpy(lay["table"]).cuda(), blockTableStride=lay["table"].shape[1])
    return q, w, k, kw


def run_logits(name):
    case, lay = im.ALL_CASES[name], im.layout(name)
    B, R, C = lay["B"], lay["R"], lay["C"]
    q, w, k, kw = launch_kw(name)
    out = torch.full((B + 1, R + 1, C + im.PADW), im.SENTINEL, dtype=torch.float32, device="cuda")
    index = AttentionMLAIndex(PREC[case["fmt"]])
    index.dispatch(q, w, k, out, stage="logits", logitStrides=(C + im.PADW, (R + 1) * (C + im.PADW)), **kw)
    return out.cpu().numpy(), index.launchForm(stage="logits", **kw)


@gpu
@pytest.mark.parametrize("name", list(im.STEP_CASES))
def test_logits_of_the_multi_step_plans(name):
    """steps = 2, 4 and 8 with two or three tiles, the last one short; 32 causal rows sweep v over the wave, step and tile seams; lengths
    of 0, below the rows and past the column; once without `causal`.  Per element under 2 x 161 x 2^-24 x sum |W| sum |q k|."""
    plan = im.ALL_CASES[name]["problem"]
    got, form = run_logits(name)
    assert form == im.PLAN_FORMS[plan] % ("paged" if im.ALL_CASES[name]["page"] else "contiguous"), form
    ratio = im.verdict(got, name)
    print("%s: largest error / bound: %.3e" % (name, ratio))
    assert ratio <= 1.0
    if im.ALL_CASES[name]["causal"]:                                         # every layout gives the same bits
        first = BITS.setdefault(plan, got)
        assert np.array_equal(first.view(np.uint32), got.view(np.uint32))


@gpu
@pytest.mark.parametrize("name", list(im.HEAD_CASES))
def test_logits_of_heads_strides_pages_and_rows(name):
    """indexHeads 1, 31, 32, 33 and 64; QI through a transposed view and through padded rows and heads of +-2^14; W through a wider row
    stride with NaN padding; pages of 16, 64, 256 and one page of 1024 with blockTableStride = 1; rows 1, 2 and 32"""
    got, form = run_logits(name)
    assert " tiles of 128 keys " in form and "%d heads" % im.ALL_CASES[name]["H"] in form, form     # steps = 1
    ratio = im.verdict(got, name)
    print("%s: largest error / bound: %.3e" % (name, ratio))
    assert ratio <= 1.0


@gpu
@pytest.mark.parametrize("name", list(im.NEW_SELECT_CASES))
def test_selection_across_rounds_exactly(name):
    """five rounds of 4096: ties that straddle a round, greater keys in the last round only, lists that fill in the last round, the
    threshold found in each digit pass, NaN of both signs, infinities, denormals and +-0 inside v, topk above a round; the logits lie in
    rows of column + 8 with NaN between them, the lists in a wider allocation of sentinels"""
    case, v, x = im.select_inputs(name)
    (B, R, width), topk, tail = x.shape, case["topk"], 5
    out = torch.full((B, R, topk + tail), im.UNWRITTEN, dtype=torch.int32, device="cuda")
    AttentionMLAIndex().dispatch(torch.from_numpy(x).cuda(), out, stage="select", rows=R, column=case["column"], batches=B, topk=topk,
                                 cacheLengths=torch.tensor(case["lens"], dtype=torch.int32).cuda(), logitStrides=(width, R * width),
                                 indexStrides=(topk + tail, R * (topk + tail)))
    want = np.full((B, R, topk + tail), im.UNWRITTEN, dtype=np.int32)
    want[:, :, :topk] = im.select_wanted(name)
    assert torch.equal(out.cpu(), torch.from_numpy(want))


def torch_operands(plan):
    """a plan's values as the torch functions take them: packed tensors, NaN at and past every length"""
    name = "%s contiguous" % plan
    case, (q, w, k) = im.ALL_CASES[name], im.values("%s contiguous" % plan)
    dt = DTYPE[case["fmt"]]
    k = torch.from_numpy(k).to(dt)
    for b, n in enumerate(case["lens"]):
        k[b, n:] = float("nan")
    return case, torch.from_numpy(q).to(dt).cuda(), torch.from_numpy(w).float().cuda(), k.cuda(), torch.tensor(case["lens"], dtype=torch.int32).cuda()


@gpu
def test_the_chain_over_a_column_that_is_no_multiple_of_4():
    """column 1101: the chained entry keeps its logits in rows of 1104; its lists are the select launch's over the logits launch's, bit
    for bit, and numpy's lexsort of those logits"""
    case, qi, w, ki, lengths = torch_operands("m8")
    B, R, C = len(case["lens"]), case["R"], case["C"]
    index = AttentionMLAIndex(PREC[case["fmt"]])
    kw = dict(rows=R, column=C, indexHeads=case["H"], batches=B, topk=64, cacheLengths=lengths)
    assert index.workspaceSize(**kw) == B * R * 1104 * 4
    form = index.launchForm(workspace=0x100000, workspaceBytes=B * R * 1104 * 4, **kw)
    assert form == im.PLAN_FORMS["m8"] % "contiguous" + " + attn_mlai_select (grid 1024 = 32 rows x 32 sequences, topk 64)", form
    logits = mfa.mla_index_logits(qi, w, ki, lengths)
    v, x = im.visible(case["lens"], R, True, C), logits.cpu().numpy()
    for topk in (64, 1100):
        both = mfa.mla_index_topk(qi, w, ki, lengths, topk)
        assert both.shape == (B, R, topk) and torch.equal(both, mfa.mla_index_select(logits, lengths, topk))
        want = np.stack([np.stack([im.select_ref(x[b, r], int(v[b, r]), topk) for r in range(R)]) for b in range(B)])
        assert np.array_equal(both.cpu().numpy(), want)


@gpu
def test_the_hand_over_to_the_sparse_decode_with_lists_shorter_than_the_rows_see():
    """v > topk for most rows: the sparse decode fed the chained entry's lists equals the sparse decode fed numpy's lexsort of the same
    logits, O and L bit for bit"""
    case, qi, w, ki, lengths = torch_operands("m2")
    B, R, C, H, topk = len(case["lens"]), case["R"], case["C"], 4, 33
    v = im.visible(case["lens"], R, True, C)
    assert (v > topk).mean() > 0.5
    both = mfa.mla_index_topk(qi, w, ki, lengths, topk)
    x = mfa.mla_index_logits(qi, w, ki, lengths).cpu().numpy()
    want = torch.from_numpy(np.stack([np.stack([im.select_ref(x[b, r], int(v[b, r]), topk) for r in range(R)]) for b in range(B)])).cuda()
    g = torch.Generator().manual_seed(3)
    q = torch.randn((B, H, R, 576), generator=g).to(qi.dtype).cuda()
    kv = torch.randn((B, C, 576), generator=g).to(qi.dtype).cuda()
    mine = mfa.flash_mla_sparse_decode(q, kv, lengths, both, softmax_scale=0.1, return_lse=True, pieces=1)
    ref = mfa.flash_mla_sparse_decode(q, kv, lengths, want, softmax_scale=0.1, return_lse=True, pieces=1)
    assert torch.equal(both, want) and torch.equal(mine[0], ref[0]) and torch.equal(mine[1], ref[1])
