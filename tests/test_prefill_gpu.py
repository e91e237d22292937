"""GPU test: prefill attention over a KV cache through the C ABI of include/mfa_prefill.h (AttentionPrefill).

One batch of sequences (qn, n) covers the seams: no prefix (1, 1), (33, 33), (128, 128); the general case (129, 300), (40, 1500),
(200, 777), (5, 2049); fewer keys than rows (70, 65); no rows (0, 50): nothing written; an empty sequence (64, 0): O = 0, L = -FLT_MAX.
Expected values: tests/prefill_model.py (float64, per sequence) on the inputs after their rounding; every output element and every L
of every live row is held to decode_model.bounds at prefill_model.MARGIN, with uniform and with needle queries.  Every launch runs on
poisoned buffers -- NaN (16-bit) or 0x7f (e4m3) in every key and value at or past each length -- and on O and L pre-filled with a
sentinel, which rows at or past queryLengths[b] must keep bit for bit.  Maxima seen on an MI355X: DESIGN.md 4.11.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402
import decode_model as dm  # noqa: E402
import prefill_model as pm  # noqa: E402
from cache_kit import LOG2E, PREC, SENT_L, SENT_O, dev, lengths, strides_of  # noqa: E402
from metal_flash_attention_amd import AttentionDecode, AttentionDescriptor, AttentionKernel, AttentionKernelType, AttentionOperand as Op  # noqa: E402

SEQS = [(1, 1), (33, 33), (128, 128), (129, 300), (40, 1500), (200, 777), (5, 2049), (70, 65), (0, 50), (64, 0)]
QLENS, LENS = [s[0] for s in SEQS], [s[1] for s in SEQS]
B, R, C, HKV = len(SEQS), 200, 2112, 2
SEEN = {}
# the runners of tests/cache_kit.py on this file's batch
launch = functools.partial(ck.prefill_launch, lens=LENS, qlens=QLENS)
check_dead_and_empty = functools.partial(ck.check_dead_and_empty, lens=LENS, qlens=QLENS)
hold = functools.partial(ck.prefill_hold, lens=LENS, qlens=QLENS, seen=SEEN)
paged_pool = ck.prefill_pool


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield
    if SEEN:
        print("\nprefill worst err / bound at margin 1:", {k: round(v, 4) for k, v in SEEN.items()})


@functools.lru_cache(maxsize=None)
def values(D, dtype, G, seed=0):
    """k, v [B, HKV, C, D] of the 16-bit type (CPU), NaN at and past each length; uniform q [B, Hq, R, D]"""
    g = torch.Generator().manual_seed(seed + D + G)
    rnd = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1).to(dtype))  # noqa: E731
    q, k, v = rnd(B, HKV * G, R, D), rnd(B, HKV, C, D), rnd(B, HKV, C, D)
    for b, n in enumerate(LENS):
        k[b, :, n:] = float("nan")
        v[b, :, n:] = float("nan")
    return q, k, v


def clean(t):
    return torch.nan_to_num(t.float(), nan=0.0)


@functools.lru_cache(maxsize=None)
def reference(D, dtype, G, causal, kind):
    q, k, v = values(D, dtype, G)
    info = None
    if kind == "needle":
        q64, info = pm.needle_queries(clean(k), LENS, QLENS, HKV * G, G, R, causal, dm.fmt_of(dtype))
        q = torch.from_numpy(q64).to(dtype)
        assert torch.equal(q.to(torch.float64), torch.from_numpy(q64))
    return q, pm.model(q, clean(k), clean(v), LENS, QLENS, G, causal), info


@pytest.mark.parametrize("kind", ["uniform", "needle"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("G", [1, 4, 8, 3])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
def test_parity_with_the_model(D, dtype, G, causal, kind):
    _q, k, v = values(D, dtype, G)
    q, ref, info = reference(D, dtype, G, causal, kind)
    kd, vd = dev(k), dev(v)
    for out in (None, torch.float32):
        o, l = launch(q, kd, vd, G, causal, out=out)
        check_dead_and_empty(o, l)
        hold(o, l, ref, dtype, out or dtype, info, "16-bit cache")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_layouts_are_byte_identical_and_poison_is_never_read(dtype):
    D, G, causal = 128, 4, True
    _q, k, v = values(D, dtype, G)
    q, ref, info = reference(D, dtype, G, causal, "needle")
    base_o, base_l = launch(q, dev(k), dev(v), G, causal)
    hold(base_o, base_l, ref, dtype, dtype, info, "16-bit cache")
    zo, zl = launch(q, dev(torch.nan_to_num(k, nan=0.0)), dev(torch.nan_to_num(v, nan=0.0)), G, causal)
    assert torch.equal(zo.view(torch.int16), base_o.view(torch.int16)) and torch.equal(zl, base_l), "poison past a length changed the result"

    def same(o, l, what):
        check_dead_and_empty(o, l)
        assert torch.equal(o.view(torch.int16), base_o.view(torch.int16)), what
        assert torch.equal(l.view(torch.int32), base_l.view(torch.int32)), what

    # token-major [B][C][Hkv][D]
    ktm, vtm = (dev(t.permute(0, 2, 1, 3).contiguous()).permute(0, 2, 1, 3) for t in (k, v))
    same(*launch(q, ktm, vtm, G, causal, cache_kw=dict(strides=dict(K=strides_of(ktm), V=strides_of(vtm)))), "token-major cache")
    # K / V slices of one allocation [B][Hkv][C][2][D]
    kv = dev(torch.stack((k, v), dim=3))
    ks, vs = kv[:, :, :, 0], kv[:, :, :, 1]
    same(*launch(q, ks, vs, G, causal, cache_kw=dict(strides=dict(K=strides_of(ks), V=strides_of(vs)))), "K / V slices of one allocation")
    # Q and O windows of larger allocations
    same(*launch(q, dev(k), dev(v), G, causal, q_strided=True), "strided Q and O")
    # paged, shuffled pools, NaN in page tails and unnamed pages, garbage table entries past the last page
    for page in (16, 64, 256):
        pk, pv, kw = paged_pool(k, v, page, LENS, page, float("nan"))
        same(*launch(q, pk, pv, G, causal, cache_kw=kw), f"paged, page size {page}")
    # zero batch stride: every sequence reads sequence 4's cache (n = 1500), under its own lengths clamped to it
    lens0 = [min(n, 1500) for n in LENS]
    k0, v0 = k[4:5].expand(B, -1, -1, -1).contiguous(), v[4:5].expand(B, -1, -1, -1).contiguous()
    want_o, want_l = launch(q, dev(k0), dev(v0), G, causal, lens=lens0)
    k1, v1 = dev(k[4:5].contiguous()), dev(v[4:5].contiguous())
    o, l = launch(q, k1, v1, G, causal, lens=lens0, cache_kw=dict(strides=dict(K=(D, C * D, 0), V=(D, C * D, 0))))
    assert torch.equal(o.view(torch.int16), want_o.view(torch.int16)) and torch.equal(l, want_l), "zero batch stride"


def test_rows_without_query_lengths_and_full_capacity():
    """queryLengths NULL: every sequence has `rows`; entries above `rows` are clamped"""
    D, G, dtype = 64, 3, torch.bfloat16
    q, k, v = values(D, dtype, G)
    full = [R] * B
    ref = pm.model(q, clean(k), clean(v), LENS, full, G, True)
    o, l = launch(q, dev(k), dev(v), G, True, qlens=None)
    hold(o, l, ref, dtype, dtype, None, "16-bit cache", qlens=full)
    o2, l2 = launch(q, dev(k), dev(v), G, True, qlens=[R + 5] * B)
    assert torch.equal(o2.view(torch.int16), o.view(torch.int16)) and torch.equal(l2, l)
    check_dead_and_empty(o, l, qlens=full)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_same_buffers_through_the_decode_launch(dtype):
    """G x R <= 32 is decode's math: both launches on the same paged buffers, each held to its own bound"""
    D, G, Rd, causal = 128, 8, 4, True
    _q, k, v = values(D, dtype, G)
    lens = [max(n, Rd) for n in LENS]   # decode has no per-sequence row count: every sequence has its Rd rows
    k, v = k.clone(), v.clone()
    g = torch.Generator().manual_seed(5)
    for b, n in enumerate(lens):   # the keys the longer lengths add get values of their own
        fresh = (torch.rand(2, HKV, n, D, generator=g) * 2 - 1).to(dtype)
        k[b, :, :n] = torch.where(torch.isnan(k[b, :, :n]), fresh[0], k[b, :, :n])
        v[b, :, :n] = torch.where(torch.isnan(v[b, :, :n]), fresh[1], v[b, :, :n])
    q64, info = pm.needle_queries(clean(k), lens, [Rd] * B, HKV * G, G, Rd, causal, dm.fmt_of(dtype), page=64)
    q = torch.from_numpy(q64).to(dtype)
    ref = pm.model(q, clean(k), clean(v), lens, [Rd] * B, G, causal)
    pk, pv, kw = paged_pool(k, v, 64, lens, 9, float("nan"))
    o, l = launch(q, pk, pv, G, causal, lens=lens, qlens=None, cache_kw=dict(kw))
    hold(o, l, ref, dtype, dtype, info, "16-bit cache", lens=lens, qlens=[Rd] * B)
    od = torch.full((B, HKV * G, Rd, D), SENT_O, dtype=dtype, device="cuda")
    ld = torch.full((B, HKV * G, Rd), SENT_L, dtype=torch.float32, device="cuda")
    column = kw.pop("column")
    AttentionDecode(D, PREC[dtype]).dispatch(dev(q), pk, pv, od, ld, rows=Rd, column=column, heads=HKV * G, batches=B, headsPerKeyValue=G,
                                            causal=causal, cacheLengths=lengths(lens), stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    dref = dm.model(q, clean(k), clean(v), lens, G, causal, page=64)
    wo, wl, text = dm.compare(od.cpu(), ld.cpu() / LOG2E, dref, dm.fmt_of(dtype), dm.fmt_of(dtype), lens, info=info, page=64)
    assert wo <= 1.0 and wl <= 1.0, text   # (margin dm.MARGIN is inside the bound compare() divides by)


@pytest.mark.parametrize("dtype,D,G", [(torch.bfloat16, 128, 4), (torch.float16, 64, 8), (torch.bfloat16, 64, 1), (torch.float16, 128, 3)])
def test_same_buffers_through_the_forward_launch(dtype, D, G):
    """the library's existing route for a contiguous 16-bit cache: the forward launch with rowLengths + columnLengths + causal +
    headsPerKeyValue on the same buffers (the same mask and length rule, include/mfa.h), each side held to its own bound.  Sequences
    without rows or without keys are left out of the forward's side: the forward kernel does not define them."""
    causal = True
    _q, k, v = values(D, dtype, G)
    q, ref, info = reference(D, dtype, G, causal, "needle")
    kd, vd = dev(k), dev(v)
    o, l = launch(q, kd, vd, G, causal, out=torch.float32)
    check_dead_and_empty(o, l)
    hold(o, l, ref, dtype, torch.float32, info, "16-bit cache")
    desc = AttentionDescriptor()
    desc.lowPrecisionInputs, desc.lowPrecisionIntermediates, desc.lowPrecisionInputType = True, False, PREC[dtype]
    desc.matrixDimensions = (R, C, D)
    desc.transposeState = (False, False, False, False)
    kernel = AttentionKernel(desc.kernelDescriptor(AttentionKernelType.forward))
    Hq = HKV * G
    fo = torch.full((B, Hq, R, D), SENT_O, dtype=torch.float32, device="cuda")
    fl = torch.full((B, Hq, R), SENT_L, dtype=torch.float32, device="cuda")
    kernel.dispatch({Op.Q: dev(q), Op.K: kd, Op.V: vd, Op.O: fo, Op.L: fl}, row=R, column=C, heads=Hq, batches=B,
                    headStrides={Op.Q: R * D, Op.K: C * D, Op.V: C * D, Op.O: R * D, Op.L: R},
                    batchStrides={Op.Q: Hq * R * D, Op.K: HKV * C * D, Op.V: HKV * C * D, Op.O: Hq * R * D, Op.L: Hq * R},
                    causal=causal, rowLengths=lengths(QLENS), columnLengths=lengths(LENS), headsPerKeyValue=G,
                    stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    keep = [b for b, (qn, n) in enumerate(SEQS) if qn > 0 and n > 0]
    sub = dm.Reference(*(x[keep] for x in ref))
    finfo = {(keep.index(b), h, r): w for (b, h, r), w in info.items() if b in keep}
    wo, wl, text = pm.compare(fo.cpu()[keep], fl.cpu()[keep] / LOG2E, sub, dm.fmt_of(dtype), "f32", [LENS[b] for b in keep],
                              [QLENS[b] for b in keep], margin=1, info=finfo)
    print("forward launch on the same buffers: worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % (wo, wl))
    assert wo <= pm.MARGIN and wl <= pm.MARGIN, "forward launch: " + text


# ------------------------------------------------------------------------------------------------------------------------- FP8
@functools.lru_cache(maxsize=None)
def values8(D, G, seed=3):
    """e4m3 caches [B, HKV, C, D] (CPU; 0x7f at and past each length), the values they stand for without the scales, and the scales"""
    g = torch.Generator().manual_seed(seed + D + G)
    k8, v8 = ((torch.rand(B, HKV, C, D, generator=g) * 8 - 4).to(torch.float8_e4m3fn) for _ in range(2))
    kf, vf = k8.float(), v8.float()
    for b, n in enumerate(LENS):
        k8.view(torch.uint8)[b, :, n:] = 0x7F
        v8.view(torch.uint8)[b, :, n:] = 0x7F
        kf[b, :, n:] = 0.0
        vf[b, :, n:] = 0.0
    rng = np.random.default_rng(seed)
    return k8, v8, kf, vf, dm.spread_scales(rng, HKV), dm.spread_scales(rng, HKV)


@functools.lru_cache(maxsize=None)
def reference8(D, dtype, G, causal, kind):
    k8, v8, kf, vf, ks, vs = values8(D, G)
    q = values(D, dtype, G)[0]
    info = None
    if kind == "needle":
        q64, info = pm.needle_queries(kf.double().numpy() * ks[None, :, None, None], LENS, QLENS, HKV * G, G, R, causal, dm.fmt_of(dtype))
        q = torch.from_numpy(q64).to(dtype)
    return q, pm.model(q, kf, vf, LENS, QLENS, G, causal, kscale=ks, vscale=vs), info


@pytest.mark.parametrize("kind", ["uniform", "needle"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("G", [1, 4, 8, 3])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
def test_fp8_parity_with_the_model(D, dtype, G, causal, kind):
    k8, v8, _kf, _vf, ks, vs = values8(D, G)
    q, ref, info = reference8(D, dtype, G, causal, kind)
    scales = (torch.from_numpy(ks).cuda(), torch.from_numpy(vs).cuda())
    kd, vd = dev(k8), dev(v8)
    for out in (None, torch.float32):
        o, l = launch(q, kd, vd, G, causal, out=out, fp8=True, scales=scales)
        check_dead_and_empty(o, l)
        hold(o, l, ref, dtype, out or dtype, info, "e4m3 cache")


@pytest.mark.parametrize("G", [1, 8, 3])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
def test_fp8_bytes_against_the_same_values_in_16_bits(D, dtype, G):
    """the conversion happens before the shared images: e4m3 bytes and the same values converted exactly to the 16-bit type give the
    same bytes of O and L, contiguous and paged (page 16, 0x7f in page tails and unnamed pages)"""
    k8, v8, kf, vf, _ks, _vs = values8(D, G)
    q, _ref, _info = reference8(D, dtype, G, True, "needle")
    k16, v16 = kf.to(dtype), vf.to(dtype)
    assert torch.equal(k16.float(), kf) and torch.equal(v16.float(), vf), "e4m3 values are values of the 16-bit type"
    want_o, want_l = launch(q, dev(k16), dev(v16), G, True)
    o, l = launch(q, dev(k8), dev(v8), G, True, fp8=True)
    assert torch.equal(o.view(torch.int16), want_o.view(torch.int16)) and torch.equal(l, want_l), "contiguous e4m3 cache"
    pk, pv, kw = paged_pool(k8.view(torch.uint8), v8.view(torch.uint8), 16, LENS, 11, 0x7F)
    o, l = launch(q, pk, pv, G, True, fp8=True, cache_kw=kw)
    check_dead_and_empty(o, l)
    assert torch.equal(o.view(torch.int16), want_o.view(torch.int16)) and torch.equal(l, want_l), "paged e4m3 cache"
