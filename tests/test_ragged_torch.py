"""GPU test: the torch entries of ragged batches (metal_flash_attention_amd.torch_binding.flash_prefill_ragged and
kv_cache_append_ragged, the ops mfa::attention_prefill_ragged and mfa::kv_cache_append_ragged) against flash_prefill and
kv_cache_append on the padded form of the same sequences: byte identity of every live row and of the whole cache."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import ragged_model as rm  # noqa: E402
from metal_flash_attention_amd import torch_binding as tb  # noqa: E402

BATCH = [(700, 40), (200, 17), (65, 1), (0, 0), (30, 16), (10, 33)]
C, HKV, G, D = 768, 2, 8, 128
H = HKV * G


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield


def case(dtype, fp8, seed=0):
    lens, counts = [n for n, _ in BATCH], [qn for _, qn in BATCH]
    starts = rm.row_starts(counts)
    T, B = starts[-1], len(BATCH)
    g = torch.Generator().manual_seed(seed)
    fused = ((torch.rand(T, (H + 2 * HKV) * D, generator=g) * 2 - 1)).to(dtype).cuda()
    kc = (torch.rand(B, HKV, C, D, generator=g) * 2 - 1)
    vc = (torch.rand(B, HKV, C, D, generator=g) * 2 - 1)
    kc, vc = ((x * 3).to(torch.float8_e4m3fn) if fp8 else x.to(dtype) for x in (kc, vc))
    scales = tuple(torch.tensor(x, dtype=torch.float32, device="cuda") for x in ([0.5, 1.75], [1.25, 0.75])) if fp8 else (None, None)
    dl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    ds = torch.tensor(starts, dtype=torch.int32, device="cuda")
    return fused, kc.cuda(), vc.cuda(), scales, lens, counts, starts, T, dl, ds


def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.uint8) if t.element_size() == 1 else t


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("extra", [dict(), dict(window=130, sink_tokens=4, sink_logits=True), dict(sink_logits=True)])
def test_flash_prefill_ragged_is_flash_prefill_on_the_padded_form(dtype, fp8, extra, monkeypatch):
    fused, kc, vc, (ks, vs), lens, counts, starts, T, dl, ds = case(dtype, fp8)
    q = fused[:, :H * D].view(T, H, D)                 # a slice of a fused QKV projection: strides, not a copy
    extra = dict(extra)
    if extra.pop("sink_logits", False):
        extra["sink_logits"] = torch.linspace(1.0, 4.0, H, device="cuda")
    seen = []
    real = tb.AttentionPrefill.dispatch
    monkeypatch.setattr(tb.AttentionPrefill, "dispatch", lambda self, q_, *a, **kw: (seen.append(q_.data_ptr()), real(self, q_, *a, **kw))[1])
    o, lse = tb.flash_prefill_ragged(q, kc, vc, dl, ds, max(counts), k_scale=ks, v_scale=vs, return_lse=True, **extra)
    assert seen == [fused.data_ptr()], "q was copied on its way to the launch"
    assert o.shape == (T, H, D) and o.dtype == dtype and lse.shape == (H, T) and lse.dtype == torch.float32
    R = max(counts)
    qpad = torch.from_numpy(rm.unpack(q.cpu().view(torch.int16).numpy(), starts, T, R, R)).view(dtype).cuda()
    po, plse = tb.flash_prefill(qpad, kc, vc, dl, torch.tensor(counts, dtype=torch.int32, device="cuda"), k_scale=ks, v_scale=vs,
                                return_lse=True, **extra)
    for b, (s, qn) in enumerate(rm.counts_of(starts, T, R)):
        if qn == 0 or (lens[b] == 0 and not extra):
            continue
        assert torch.equal(bits(o[s:s + qn].transpose(0, 1)), bits(po[b, :, :qn])), f"sequence {b}: O differs from flash_prefill"
        assert torch.equal(lse[:, s:s + qn], plse[b, :, :qn]), f"sequence {b}: L differs from flash_prefill"


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("fp8", [False, True])
def test_kv_cache_append_ragged_is_kv_cache_append_per_sequence(fp8, paged):
    dtype = torch.bfloat16
    fused, kc, vc, (ks, vs), lens, counts, starts, T, dl, ds = case(dtype, fp8, 1)
    kn = fused[:, H * D:(H + HKV) * D].view(T, HKV, D)
    vn = fused[:, (H + HKV) * D:].view(T, HKV, D)
    table = None
    if paged:
        page, B = 16, len(BATCH)
        pps = C // page
        table = torch.from_numpy(np.random.default_rng(2).permutation(B * pps).astype(np.int32).reshape(B, pps)).cuda()
        kc, vc = (x.reshape(B, HKV, pps, page, D).permute(0, 2, 1, 3, 4).reshape(B * pps, HKV, page, D).contiguous() for x in (kc, vc))
    want_k, want_v, before = kc.clone(), vc.clone(), kc.clone()
    for b, qn in enumerate(counts):
        if qn:
            s = starts[b]
            one = (want_k, want_v) if paged else (want_k[b:b + 1], want_v[b:b + 1])
            tb.kv_cache_append(kn[s:s + qn].transpose(0, 1)[None], vn[s:s + qn].transpose(0, 1)[None], *one, dl[b:b + 1],
                               block_table=table[b:b + 1] if paged else None, k_scale=ks, v_scale=vs)
    tb.kv_cache_append_ragged(kn, vn, kc, vc, dl, ds, max(counts), block_table=table, k_scale=ks, v_scale=vs)
    torch.cuda.synchronize()
    assert torch.equal(bits(kc), bits(want_k)) and torch.equal(bits(vc), bits(want_v))
    assert not torch.equal(bits(kc), bits(before))


def test_refusals_in_the_words_of_the_padded_functions():
    dtype = torch.bfloat16
    fused, kc, vc, _s, lens, counts, starts, T, dl, ds = case(dtype, False)
    q = fused[:, :H * D].view(T, H, D)
    kn = fused[:, H * D:(H + HKV) * D].view(T, HKV, D)
    R = max(counts)
    with pytest.raises(TypeError, match="q must be bfloat16 or float16"):
        tb.flash_prefill_ragged(q.float(), kc, vc, dl, ds, R)
    with pytest.raises(TypeError, match="q and the caches must share one of bfloat16 / float16"):
        tb.flash_prefill_ragged(q.half(), kc, vc, dl, ds, R)
    with pytest.raises(ValueError, match="k_scale / v_scale go with a float8_e4m3fn cache"):
        tb.flash_prefill_ragged(q, kc, vc, dl, ds, R, k_scale=torch.ones(HKV, device="cuda"))
    with pytest.raises(ValueError, match=r"expected q \[T, H, D\]"):
        tb.flash_prefill_ragged(q[None], kc, vc, dl, ds, R)
    with pytest.raises(ValueError, match=r"row_starts must be a GPU tensor \[B \+ 1\]"):
        tb.flash_prefill_ragged(q, kc, vc, dl, ds[:-1], R)
    with pytest.raises(ValueError, match="row_starts must be a GPU tensor"):
        tb.flash_prefill_ragged(q, kc, vc, dl, ds.cpu(), R)
    with pytest.raises(ValueError, match="max_rows must be an int from 1"):
        tb.flash_prefill_ragged(q, kc, vc, dl, ds, 0)
    with pytest.raises(ValueError, match="must have a contiguous last dimension"):
        tb.flash_prefill_ragged(q, kc.transpose(2, 3).contiguous().transpose(2, 3), vc, dl, ds, R)
    with pytest.raises(ValueError, match="block_table must be an int32 GPU tensor"):
        tb.flash_prefill_ragged(q, kc, vc, dl, ds, R, block_table=torch.zeros((len(BATCH), 4), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="sink_tokens needs window"):
        tb.flash_prefill_ragged(q, kc, vc, dl, ds, R, sink_tokens=4)
    with pytest.raises(RuntimeError, match="forward only"):
        tb.flash_prefill_ragged(q.clone().requires_grad_(), kc, vc, dl, ds, R)
    with pytest.raises(TypeError, match="k_new and v_new must share one of bfloat16 / float16"):
        tb.kv_cache_append_ragged(kn, kn.half(), kc, vc, dl, ds, R)
    with pytest.raises(TypeError, match="the caches must both be torch.float8_e4m3fn or the new rows'"):
        tb.kv_cache_append_ragged(kn, kn, kc.half(), vc.half(), dl, ds, R)
    with pytest.raises(ValueError, match="k_scale / v_scale go with a float8_e4m3fn cache"):
        tb.kv_cache_append_ragged(kn, kn, kc, vc, dl, ds, R, v_scale=torch.ones(HKV, device="cuda"))
    with pytest.raises(ValueError, match=r"expected k_new, v_new \[T, Hkv, D\]"):
        tb.kv_cache_append_ragged(kn[None], kn[None], kc, vc, dl, ds, R)
    with pytest.raises(ValueError, match="row_starts must be a GPU tensor"):
        tb.kv_cache_append_ragged(kn, kn, kc, vc, dl, ds[:3], R)
    with pytest.raises(RuntimeError, match="no autograd"):
        tb.kv_cache_append_ragged(kn.clone().requires_grad_(), kn, kc, vc, dl, ds, R)


def test_torch_compile_traces_through_both_ops():
    if not tb._HAVE_RAGGED_OPS:
        pytest.skip("this torch has no torch.library.custom_op")
    dtype = torch.bfloat16
    fused, kc, vc, _s, lens, counts, starts, T, dl, ds = case(dtype, False, 3)
    R = max(counts)

    def step(fused, kc, vc, dl, ds):
        q = fused[:, :H * D].view(T, H, D)
        kn, vn = fused[:, H * D:(H + HKV) * D].view(T, HKV, D), fused[:, (H + HKV) * D:].view(T, HKV, D)
        tb.kv_cache_append_ragged(kn, vn, kc, vc, dl, ds, R)
        return tb.flash_prefill_ragged(q, kc, vc, dl, ds, R, window=130) * 2

    k0, v0 = kc.clone(), vc.clone()
    want = step(fused, k0, v0, dl, ds)
    got = torch.compile(step, fullgraph=True, backend="aot_eager")(fused, kc, vc, dl, ds)
    live = torch.from_numpy(rm.owned(starts, T, R)).cuda()
    assert torch.equal(bits(got[live]), bits(want[live])) and torch.equal(bits(kc), bits(k0)) and torch.equal(bits(vc), bits(v0))
