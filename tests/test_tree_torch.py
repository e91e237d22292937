"""GPU test: speculation trees through the torch binding -- pack_tree_mask on the device, flash_decode / flash_prefill with tree_mask=
against the C-ABI launch of include/mfa_tree.h byte for byte, and a PATH WALK at a gpt-oss-like shape (D = 64, G = 8, window 128, sink
logits): a random tree of 24 nodes through prefill and of 4 through decode; for every leaf the prefix and its root-to-leaf path are
copied into a scratch cache, today's causal launch runs on it, and the tree launch's rows of that path are held against it.  Not a byte
identity: the keys lie in other slots, so the waves sum in another order.  Both launches lie within tree_model.MARGIN bounds of the same
float64 values (the path's rows see exactly the keys the tree's rows see), so they differ by at most twice that."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402
import decode_model as dm  # noqa: E402
import tree_model as tm  # noqa: E402
from metal_flash_attention_amd import torch_binding as tb  # noqa: E402

D, G, HKV, W, C = 64, 8, 1, 128, 1152
PREFIX = (1000, 300)
LN2 = float(np.log(2.0))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def inputs(R, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    B, Hq = len(PREFIX), HKV * G
    k, v = ((torch.rand(B, HKV, C, D, generator=g) * 2 - 1).to(dtype) for _ in range(2))
    q = ((torch.rand(B, Hq, R, D, generator=g) * 2 - 1) * 3).to(dtype)
    sink = ck.sink_logits(Hq, seed)
    lens = [p + R for p in PREFIX]
    for b, n in enumerate(lens):   # what lies past a length is never read
        k[b, :, n:], v[b, :, n:] = float("nan"), float("nan")
    return q, k, v, sink, lens


def test_pack_tree_mask_round_trip_on_the_device():
    for R, seed in ((4, 0), (24, 1), (64, 2)):
        masks = tm.per_sequence(tm.random_tree, 3, R, seed)
        bits = torch.from_numpy(np.array([[[(int(masks[b, r]) >> j) & 1 for j in range(R)] for r in range(R)] for b in range(3)], dtype=bool)).cuda()
        packed = tb.pack_tree_mask(bits)
        assert packed.is_cuda and packed.dtype == torch.int64 and packed.shape == (3, R)
        assert np.array_equal(packed.cpu().numpy().view(np.uint64), masks)
        back = (packed[..., None] >> torch.arange(R, device="cuda")) & 1
        assert torch.equal(back.bool(), bits)


@pytest.mark.parametrize("kind,R,dtype,fp8", [("decode", 4, torch.bfloat16, False), ("decode", 4, torch.float16, True),
                                              ("prefill", 24, torch.bfloat16, True), ("prefill", 24, torch.float16, False)])
def test_the_public_functions_are_the_c_abi_launch_byte_for_byte(kind, R, dtype, fp8):
    q, k, v, sink, lens = inputs(R, dtype, 3 + R)
    B = len(lens)
    batch = ck.Batch(tuple((n, R) for n in lens), C, HKV, R)
    scales = (None, None)
    if fp8:
        k, v = (torch.nan_to_num(k.float(), nan=0.0) * 3).to(torch.float8_e4m3fn), (torch.nan_to_num(v.float(), nan=0.0) * 3).to(torch.float8_e4m3fn)
        scales = tuple(torch.from_numpy(dm.spread_scales(np.random.default_rng(R), HKV)).cuda() for _ in range(2))
    masks = tm.per_sequence(tm.random_tree, B, R, 9)
    tree = torch.from_numpy(masks.view(np.int64)).cuda()
    fn = tb.flash_decode if kind == "decode" else tb.flash_prefill
    dlens = ck.lengths(lens)
    for mask, stride in ((tree, R), (tree[0], 0)):
        o, lse = fn(q.cuda(), k.cuda(), v.cuda(), dlens, k_scale=scales[0], v_scale=scales[1], window=W, sink_logits=ck.dev(sink), tree_mask=mask,
                    return_lse=True)
        torch.cuda.synchronize()
        want_o, want_l = ck.launch(batch, kind, q, k.cuda(), v.cuda(), G, scales=scales, window=W, sinkTokens=0, sinkLogits=ck.dev(sink), treeMasks=mask,
                                   treeBatchStride=stride)
        assert torch.equal(o.cpu().view(torch.int16), want_o.view(torch.int16)), "O differs from the C-ABI launch"
        assert torch.equal(lse.cpu(), want_l * tb._LN2), "L differs from the C-ABI launch"
    with pytest.raises(ValueError, match="together have no kernel"):
        fn(q.cuda(), k.cuda(), v.cuda(), dlens, k_scale=scales[0], v_scale=scales[1], softcap=30.0, tree_mask=tree)


@pytest.mark.parametrize("kind,R", [("prefill", 24), ("decode", 4)])
def test_every_root_to_leaf_path_is_todays_causal_launch_on_a_scratch_cache(kind, R):
    dtype, fmt = torch.bfloat16, "bf16"
    q, k, v, sink, lens = inputs(R, dtype, 11 + R)
    B, Hq = len(lens), HKV * G
    one = tm.random_tree(R, np.random.default_rng(R + 2))   # (4 nodes: 0 - 1 - 3 and 0 - 2, two leaves)
    tree = torch.from_numpy(one.view(np.int64)).cuda()
    fn = tb.flash_decode if kind == "decode" else tb.flash_prefill
    dsink = ck.dev(sink)
    o, lse = fn(q.cuda(), k.cuda(), v.cuda(), ck.lengths(lens), window=W, sink_logits=dsink, tree_mask=tree, return_lse=True)
    o, lse = o.cpu(), lse.cpu()
    ref = tm.model(q, torch.nan_to_num(k.float()), torch.nan_to_num(v.float()), lens, None if kind == "decode" else [R] * B, G, W, 0, sink, one)
    bo, bl = tm.bounds(ref, fmt, fmt, 1)
    wo, wl, text = tm.compare(o, lse, ref, fmt, fmt, lens, None if kind == "decode" else [R] * B, margin=1)
    assert wo <= tm.MARGIN and wl <= tm.MARGIN, text                           # the tree launch itself, against the model
    nodes = [[j for j in range(R) if int(one[r]) >> j & 1] for r in range(R)]   # a node's path: its ancestors and itself
    leaves = [r for r in range(R) if not any(r in nodes[s] for s in range(r + 1, R))]
    assert len(leaves) >= 2 and max(len(nodes[r]) for r in leaves) >= 3
    worst = 0.0
    for leaf in leaves:
        path = nodes[leaf]
        d = len(path)
        if kind == "decode" and G * d > 32:
            continue
        sk, sv = k.clone(), v.clone()
        for b, p in enumerate(PREFIX):
            sk[b, :, p:], sv[b, :, p:] = float("nan"), float("nan")
            sk[b, :, p:p + d], sv[b, :, p:p + d] = k[b, :, [p + j for j in path]], v[b, :, [p + j for j in path]]
        po, pl = fn(q[:, :, path].contiguous().cuda(), sk.cuda(), sv.cuda(), ck.lengths([p + d for p in PREFIX]), window=W, sink_logits=dsink,
                    return_lse=True)
        po, pl = po.cpu(), pl.cpu()
        assert bool(torch.isfinite(po.float()).all()) and bool(torch.isfinite(pl).all())
        do = np.abs(o[:, :, path].double().numpy() - po.double().numpy()) / bo[:, :, path]
        dl = np.abs(lse[:, :, path].double().numpy() - pl.double().numpy()) / bl[:, :, path]
        worst = max(worst, float(do.max()), float(dl.max()))
    print("%s path walk: worst |tree - path| / bound at margin 1: %.3f over %d leaves" % (kind, worst, len(leaves)))
    assert worst <= 2 * tm.MARGIN
