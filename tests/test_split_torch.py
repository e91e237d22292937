"""GPU test: prefill cut along the keys through the torch binding -- flash_prefill(key_pieces=...) end to end on a 16-bit paged cache, an
e4m3 cache with per-head scales and a speculation tree, with return_lse.  Every output element and every L of every live row is held to
the bounds of tests/split_model.py at its MARGIN (the binding allocates the workspace and hands O and L back; rows at or past
q_lengths come back uninitialised and are not looked at), and the binding's launch is the C-ABI launch of include/mfa_split.h byte for
byte.  key_pieces=None is today's launch byte for byte."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402
import decode_model as dm  # noqa: E402
import split_model as spm  # noqa: E402
import tree_model as tm  # noqa: E402
from metal_flash_attention_amd import AttentionPrefill, GEMMOperandPrecision as P, KVCachePrecision  # noqa: E402
from metal_flash_attention_amd import torch_binding as tb  # noqa: E402

BATCH = ck.Batch(((1100, 70), (70, 70), (333, 37)), 1152, 2, 70)
TREE = ck.Batch(((900, 40), (300, 33), (64, 40)), 1024, 2, 40)
D, DTYPE, FMT = 128, torch.bfloat16, "bf16"
LN2 = float(np.log(2.0))
SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield
    if SEEN:
        print("\nsplit (torch) worst err / bound at margin 1:", {k: round(v, 4) for k, v in SEEN.items()})


def held(batch, o, lse, ref, tag):
    wo, wl, text = spm.compare(o.cpu(), lse.cpu(), ref, FMT, FMT, batch.LENS, batch.QLENS, margin=1)
    SEEN[tag] = max(wo, wl)
    print("%s: worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % (tag, wo, wl))
    assert wo <= spm.MARGIN and wl <= spm.MARGIN, text
    for b, qn in enumerate(batch.QLENS):
        assert bool(torch.isfinite(o[b, :, :qn].float()).all()) and bool(torch.isfinite(lse[b, :, :qn]).all()), "poison reached a live row"


def c_abi(batch, q, k, v, G, pieces, fp8=False, **kw):
    """the launch of include/mfa_split.h with the workspace it asks for -> (O, L base-2) on the device"""
    _B, Hq, R, _D = q.shape
    op = AttentionPrefill(D, P.BF16, cachePrecision=KVCachePrecision.E4M3 if fp8 else None)
    o = torch.empty((batch.B, Hq, R, D), dtype=DTYPE, device="cuda")
    l = torch.empty((batch.B, Hq, R), dtype=torch.float32, device="cuda")
    kw.update(rows=R, column=batch.C, heads=Hq, batches=batch.B, headsPerKeyValue=G, cacheLengths=ck.lengths(batch.LENS),
              queryLengths=ck.lengths(batch.QLENS), pieces=pieces)
    need = op.workspaceSize(**kw)
    kw.update(workspace=torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda") if need else None)
    op.dispatch(q, k, v, o, l, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    return o, l


def live(batch, t):
    return [t[b, :, :min(qn, batch.RP)] for b, qn in enumerate(batch.QLENS)]


@pytest.mark.parametrize("pieces", [0, 3])
def test_a_16_bit_paged_cache(pieces):
    G = 4
    k, v, _ = ck.base(BATCH, D, DTYPE, False)
    q = (torch.rand(BATCH.B, 2 * G, BATCH.RP, D, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DTYPE)
    ref = spm.model(q, k.float(), v.float(), BATCH.LENS, BATCH.QLENS, G, 0, 0, None, pieces or 2)
    kp, vp, kw = ck.paged_pool(k, v, 16, BATCH.keep(), seed=3)
    lens, qlens = ck.lengths(BATCH.LENS), ck.lengths(BATCH.QLENS)
    o, lse = tb.flash_prefill(q.cuda(), kp, vp, lens, qlens, block_table=kw["blockTable"], key_pieces=pieces, return_lse=True)
    torch.cuda.synchronize()
    held(BATCH, o, lse, ref, "paged 16-bit pieces %d" % pieces)
    co, cl = c_abi(BATCH, q.cuda(), kp, vp, G, pieces, pageSize=16, blockTable=kw["blockTable"], blockTableStride=kw["blockTableStride"],
                   pageStrides=kw["pageStrides"], strides=kw["strides"])
    for a, b in zip(live(BATCH, o) + live(BATCH, lse), live(BATCH, co) + live(BATCH, cl * tb._LN2)):
        assert torch.equal(a, b), "the binding's launch differs from the C-ABI launch"
    none = tb.flash_prefill(q.cuda(), kp, vp, lens, qlens, block_table=kw["blockTable"], key_pieces=None)
    today = tb.flash_prefill(q.cuda(), kp, vp, lens, qlens, block_table=kw["blockTable"])
    for a, b in zip(live(BATCH, none), live(BATCH, today)):
        assert torch.equal(a, b)


def test_an_e4m3_cache_with_scales_a_window_and_sinks():
    G, W, S = 4, 130, 4
    k, v, (ks, vs) = ck.base(BATCH, D, DTYPE, True)
    sink = ck.sink_logits(2 * G, 7)
    q = (torch.rand(BATCH.B, 2 * G, BATCH.RP, D, generator=torch.Generator().manual_seed(2)) * 2 - 1).to(DTYPE)
    ref = spm.model(q, k.float(), v.float(), BATCH.LENS, BATCH.QLENS, G, W, S, sink, 2, kscale=ks, vscale=vs)
    keep = BATCH.keep(tiles=ck.walked(BATCH, "prefill", G, BATCH.RP, W, S))
    o, lse = tb.flash_prefill(q.cuda(), ck.poisoned(k, keep).cuda(), ck.poisoned(v, keep).cuda(), ck.lengths(BATCH.LENS), ck.lengths(BATCH.QLENS),
                              k_scale=ck.dev(ks), v_scale=ck.dev(vs), window=W, sink_tokens=S, sink_logits=ck.dev(sink), key_pieces=2, return_lse=True)
    torch.cuda.synchronize()
    held(BATCH, o, lse, ref, "e4m3 window sinks pieces 2")
    with pytest.raises(ValueError, match="key_pieces and softcap together have no kernel"):
        tb.flash_prefill(q.cuda(), k.cuda(), v.cuda(), ck.lengths(BATCH.LENS), softcap=30.0, key_pieces=2)


def test_a_speculation_tree():
    G = 8
    k, v, _ = ck.base(TREE, D, DTYPE, False)
    q = (torch.rand(TREE.B, 2 * G, TREE.RP, D, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(DTYPE)
    masks = tm.per_sequence(tm.random_tree, TREE.B, TREE.RP, 4)
    ref = spm.model(q, k.float(), v.float(), TREE.LENS, TREE.QLENS, G, 0, 0, None, 3, masks=masks)
    keep = TREE.keep()
    tree = torch.from_numpy(masks.view(np.int64)).cuda()
    o, lse = tb.flash_prefill(q.cuda(), ck.poisoned(k, keep).cuda(), ck.poisoned(v, keep).cuda(), ck.lengths(TREE.LENS), ck.lengths(TREE.QLENS),
                              tree_mask=tree, key_pieces=3, return_lse=True)
    torch.cuda.synchronize()
    held(TREE, o, lse, ref, "tree pieces 3")
    assert dm.fmt_of(DTYPE) == FMT
