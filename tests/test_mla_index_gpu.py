"""The MLA sparse indexer (include/mfa_mla_index.h): the index logits per element against float64, the selection exactly against numpy's
lexsort, the chain and the hand-over to the sparse decode bit for bit (marked gpu), and the refusals and the struct mirror without a GPU.
Every allocation is poisoned: cache rows at or past a length, unnamed pages and row padding are NaN, logits past v are NaN, and outputs
lie in wider sentinel-filled allocations that must keep every sentinel the launch does not own."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import metal_flash_attention_amd as mfa  # noqa: E402
from metal_flash_attention_amd import AttentionMLAIndex, GEMMOperandPrecision as P, MFAError, _abi  # noqa: E402

gpu = pytest.mark.gpu
DTYPE, PREC = {"bf16": torch.bfloat16, "f16": torch.float16}, {"bf16": P.BF16, "f16": P.FP16}
LENS, C, DI, PAGE = (0, 1, 31, 32, 33, 129, 200), 200, 128, 16
SENTINEL = 12345.0
# FP32 roundings on the longest chain of a logit, counted from csrc/attn_mla_index.h: 128 for the dot product (eight MFMA steps of 16
# products each, whatever order the matrix pipe adds them in; the products of two 16-bit values are exact), 32 for the lane's chain
# acc = fma(w, max(s, 0), acc) over its 16 heads of each of the two head blocks (one rounding per fma), 1 for the add across the halves
ROUNDINGS = 128 + 32 + 1
REFS = {}


def visible(lens, R, causal=True, column=C):
    n = np.minimum(np.asarray(lens, dtype=np.int64), column)[:, None]
    r = np.arange(R)[None, :]
    return np.minimum(n, r + np.maximum(n - R, 0) + 1) if causal else np.broadcast_to(n, (len(lens), R))


def problem(fmt, H, R):
    """inputs rounded to the 16-bit type, the float64 logits and their per-element bound; computed once per (fmt, H, R)"""
    if (fmt, H, R) not in REFS:
        g = torch.Generator().manual_seed(1000 * H + R)
        q = torch.randn((len(LENS), H, R, DI), generator=g).to(DTYPE[fmt])
        k = torch.randn((len(LENS), C, DI), generator=g).to(DTYPE[fmt])
        w = torch.randn((len(LENS), R, H), generator=g)                      # both signs
        q64, k64, w64 = q.double().numpy(), k.double().numpy(), w.double().numpy()
        s = np.einsum("bhrd,bcd->brhc", q64, k64)
        mag = np.einsum("bhrd,bcd->brhc", np.abs(q64), np.abs(k64))
        ref = np.einsum("brh,brhc->brc", w64, np.maximum(s, 0.0))
        bound = 2.0 * ROUNDINGS * 2.0 ** -24 * np.einsum("brh,brhc->brc", np.abs(w64), mag)
        REFS[fmt, H, R] = dict(q=q, k=k, w=w, ref=ref, bound=bound, bits={})
    return REFS[fmt, H, R]


def index_cache(k, layout):
    """the cache on the device: NaN in every row at or past a length, in the padding of strided rows and in every page no valid key lives in"""
    B = len(LENS)
    k = k.clone()
    for b, n in enumerate(LENS):
        k[b, n:] = float("nan")
    if layout == "contiguous":
        return k.cuda(), {}
    if layout == "strided":
        buf = torch.full((B, C, DI + 8), float("nan"), dtype=k.dtype)
        buf[:, :, :DI] = k
        return buf.cuda()[:, :, :DI], dict(strides=dict(KI=(DI + 8, 0, C * (DI + 8))))
    pps = -(-C // PAGE)
    order = np.random.default_rng(5).permutation(B * pps).astype(np.int32).reshape(B, pps)
    pool = torch.full((B * pps + 1, PAGE, DI), float("nan"), dtype=k.dtype)
    table = np.full((B, pps + 2), B * pps, dtype=np.int32)                  # pages without a valid key, and entries past the last: the NaN page
    for b, n in enumerate(LENS):
        for i in range(-(-n // PAGE)):
            rows = k[b, i * PAGE:(i + 1) * PAGE]
            pool[int(order[b, i]), :len(rows)] = rows
            table[b, i] = order[b, i]
    return pool.cuda(), dict(pageSize=PAGE, blockTable=torch.from_numpy(table).cuda(), blockTableStride=pps + 2)


@gpu
@pytest.mark.parametrize("layout", ["contiguous", "strided", "paged"])
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("H", [64, 40])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_logits_per_element(fmt, H, R, layout):
    """|logit - float64| <= 2 x ROUNDINGS x 2^-24 x sum_h |W_h| sum_d |q_hd k_cd| at every visible position, ROUNDINGS = 161 as counted
    above (derived, not measured); nothing else of the allocation is written; every layout gives the same bits."""
    pr = problem(fmt, H, R)
    B, v = len(LENS), visible(LENS, R)
    cache, kw = index_cache(pr["k"], layout)
    out = torch.full((B + 1, R + 1, C + 8), SENTINEL, dtype=torch.float32, device="cuda")
    AttentionMLAIndex(PREC[fmt]).dispatch(pr["q"].cuda(), pr["w"].cuda(), cache, out, stage="logits", rows=R, column=C, indexHeads=H, batches=B,
                                          cacheLengths=torch.tensor(LENS, dtype=torch.int32).cuda(), logitStrides=(C + 8, (R + 1) * (C + 8)), **kw)
    got = out.cpu().numpy()
    seen = np.arange(C + 8)[None, None, :] < np.pad(v, ((0, 1), (0, 1)))[:, :, None]
    assert (got[~seen] == SENTINEL).all()
    err = np.abs(got[:B, :R, :C].astype(np.float64) - pr["ref"])[seen[:B, :R, :C]]
    print("largest error / bound:", float((err / pr["bound"][seen[:B, :R, :C]]).max()))
    assert (err <= pr["bound"][seen[:B, :R, :C]]).all()
    first = pr["bits"].setdefault("logits", got)
    assert np.array_equal(first.view(np.uint32), got.view(np.uint32))


def order_key(x):
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return bits ^ np.where(bits >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def select_ref(x, v, topk):
    order = np.lexsort((np.arange(v), -order_key(x[:v]).astype(np.int64)))[:topk]     # larger key first, then lower position
    return np.concatenate([np.sort(order), np.full(topk - len(order), -1)]).astype(np.int32)


VALUES = {
    "normal": lambda g, n: g.standard_normal(n),
    "equal": lambda g, n: np.full(n, 0.5),
    "ties": lambda g, n: g.choice(np.array([-1.0, -0.0, 0.0, 1.0], dtype=np.float32), n),
    "low bits": lambda g, n: (np.uint32(0x3F800000) | g.integers(0, 256, n).astype(np.uint32)).view(np.float32),
    "negative": lambda g, n: -np.abs(g.standard_normal(n)) - 0.25,
}


@gpu
@pytest.mark.parametrize("values", list(VALUES))
@pytest.mark.parametrize("topk", [1, 33, 2048])
def test_selection_exactly(topk, values):
    """two causal rows per sequence see v = n - 1 and n: v covers 0, 1, topk - 1, topk, topk + 1 and 5000"""
    column, R, tail = 5000, 2, 5
    lens = sorted({0, 1, 2, topk - 1, topk, topk + 1, topk + 2, column})
    B, v = len(lens), visible(lens, R, True, column)
    x = VALUES[values](np.random.default_rng(topk), B * R * column).astype(np.float32).reshape(B, R, column)
    x[np.arange(column)[None, None, :] >= v[:, :, None]] = np.nan
    out = torch.full((B, R, topk + tail), -7, dtype=torch.int32, device="cuda")
    AttentionMLAIndex().dispatch(torch.from_numpy(x).cuda(), out, stage="select", rows=R, column=column, batches=B, topk=topk,
                                 cacheLengths=torch.tensor(lens, dtype=torch.int32).cuda(), indexStrides=(topk + tail, R * (topk + tail)))
    want = np.full((B, R, topk + tail), -7, dtype=np.int32)
    for b in range(B):
        for r in range(R):
            want[b, r, :topk] = select_ref(x[b, r], int(v[b, r]), topk)
    assert torch.equal(out.cpu(), torch.from_numpy(want))


@gpu
def test_the_chain_and_the_hand_over_to_the_sparse_decode():
    fmt, Hi, R, H = "f16", 40, 3, 11
    pr = problem(fmt, Hi, R)
    qi, w, lengths = pr["q"].cuda(), pr["w"].cuda(), torch.tensor(LENS, dtype=torch.int32).cuda()
    ki, kw = index_cache(pr["k"], "paged")
    for topk in (33, 256):
        both = mfa.mla_index_topk(qi, w, ki, lengths, topk, block_table=kw["blockTable"])
        logits = mfa.mla_index_logits(qi, w, ki, lengths, block_table=kw["blockTable"])
        assert torch.equal(both, mfa.mla_index_select(logits, lengths, topk)) and both.shape == (len(LENS), R, topk)
    # topk >= the longest length: every visible position in order plus holes, so the sparse decode is the dense one, O and L
    g = torch.Generator().manual_seed(3)
    q = torch.randn((len(LENS), H, R, 576), generator=g).to(DTYPE[fmt]).cuda()
    kv = torch.randn((len(LENS), C, 576), generator=g).to(DTYPE[fmt]).cuda()
    dense = mfa.flash_mla_decode(q, kv, lengths, softmax_scale=0.1, return_lse=True, pieces=1)
    sparse = mfa.flash_mla_sparse_decode(q, kv, lengths, both, softmax_scale=0.1, return_lse=True, pieces=1)
    assert torch.equal(dense[0], sparse[0]) and torch.equal(dense[1], sparse[1])


LENGTHS, TABLE, WS = 0x1000, 0x5000, 0x100000   # the host reads none of them
INVALID, UNSUPPORTED = 2, 3


@pytest.mark.parametrize("stage, over, status, words", [
    ("logits", dict(di=64), UNSUPPORTED, "indexDimension = 128, not 64"),
    ("logits", dict(indexHeads=0), INVALID, "indexHeads must be 1 .. 64, not 0"),
    ("topk", dict(indexHeads=65), INVALID, "indexHeads must be 1 .. 64, not 65"),
    ("select", dict(rows=33), UNSUPPORTED, "rows = 33"),
    ("select", dict(topk=0), INVALID, "topk must be at least 1"),
    ("logits", dict(logitStrides=(4095, 4096)), INVALID, "logitRowStride must be at least column = 4096"),
    ("topk", dict(workspace=None), INVALID, "workspace is required"),
])
def test_refusals_name_the_field_and_launch_nothing(stage, over, status, words):
    kw = dict(rows=1, column=4096, indexHeads=64, batches=2, topk=2048, cacheLengths=LENGTHS, workspace=WS, workspaceBytes=1 << 20)
    kw.update(over)
    index = AttentionMLAIndex(P.BF16, kw.pop("di", DI))
    with pytest.raises(MFAError) as e:
        index.launchForm(stage=stage, **kw)
    assert e.value.status == status and words in str(e.value), str(e.value)


def test_the_struct_mirror_and_the_plan():
    handle, mirror = _abi.lib(), _abi.mfa_mla_index_params
    offsets, count = (ctypes.c_uint32 * 32)(), ctypes.c_uint32(0)
    assert handle.mfa_mla_index_params_offsets(offsets, 32, ctypes.byref(count)) == 0
    want = [getattr(mirror, name).offset for name, _t in mirror._fields_]
    assert handle.mfa_mla_index_params_size() == ctypes.sizeof(mirror) and list(offsets[:count.value]) == want
    index = AttentionMLAIndex()
    kw = dict(rows=1, column=32768, indexHeads=64, batches=32, topk=2048, cacheLengths=LENGTHS)
    assert index.workspaceSize(**kw) == 32 * 32768 * 4
    assert index.launchForm(workspace=WS, workspaceBytes=32 * 32768 * 4, **kw) == (
        "attn_mlai_d128_bf16 (grid 1024 = 32 tiles of 1024 keys x 1 rows x 32 sequences, 64 heads, contiguous) + "
        "attn_mlai_select (grid 32 = 1 rows x 32 sequences, topk 2048)")
