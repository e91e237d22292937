"""GPU test: the FP8 KV cache through the C ABI of include/mfa_kvcache.h -- the append launch (exact, whole buffers compared) and
decode attention over an e4m3 cache.

Decode: expected values are the float64 numpy model of tests/test_decode_gpu.py (tests/decode_kit.py holds both files' runners) applied to the DEQUANTISED cache,
scale[j] x e4m3(byte), with that file's bounds (tests/harness.py TOL_MIXED: O 5e-2, L 7e-3 after dividing by log2 e): the kernel
converts the bytes exactly to the launch's 16-bit type, the arithmetic after that is the 16-bit kernel's.  K, V ~ N(0, 1), scales per
head in [0.5, 2].  Every decode launch runs on poisoned caches (0x7f = NaN in every byte at or past a length, in the rest of a last
page and in pages nobody names) with canaries behind O and L and around the workspace.

Beside those bounds every comparison with the model is held to the per-element bounds of tests/decode_model.py, and every decode
test also runs with that module's needle queries (built from the dequantised K, so a key's share of the softmax survives the
quantisation).  The per-head scales are pairwise at least 1.25 x apart, so a scale taken from another head moves the scores or O far
outside the bound.  Non-causal launches have no forbidden key.

Maxima seen on an MI355X are recorded in DESIGN.md 4.10.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import decode_kit as dk  # noqa: E402  (the float64 model's check, the runners of both launches and their caches)
import decode_model  # noqa: E402
from decode_kit import DTYPE, LOG2E, NAN8, TOL_L, TOL_O, Cache8, both_inputs8 as both_inputs, check, dequantise, make_case, quantise, run8  # noqa: E402
from decode_model import MARGIN, bounds, compare  # noqa: E402,F401  (the bound proven by tests/test_decode_sensitivity.py)
from metal_flash_attention_amd import GEMMOperandPrecision as P  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield


# ---------------------------------------------------------------------------------------------------------------- decode parity
LENGTHS = np.array([0, 1, 31, 65, 1500, 4096, 2049, 777], dtype=np.uint32)
PARITY = [(prec, D, G, R) for prec in (P.BF16, P.FP16) for D in (64, 128) for G in (1, 4, 8) for R in (1, 4)]


@pytest.mark.parametrize("index,case", list(enumerate(PARITY)), ids=lambda x: "-".join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_parity_with_the_float64_model_on_the_dequantised_cache(index, case):
    prec, D, G, R = case
    C, B, Hq = 4096, len(LENGTHS), 2 * G
    q, kb, vb, ks, vs = make_case(B, Hq, G, R, C, D, DTYPE[prec], seed=300 + index)
    cache = Cache8(kb, vb, LENGTHS, "packed")
    for variant in range(4):   # causal x split, with FP32 O and a NULL L rotating over the cases
        causal, workspace = bool(variant & 1), bool(variant & 2)
        out32, want_l = bool((index + variant) & 1), (index + variant) % 3 != 0
        for name, qq, info in both_inputs(q, kb, ks, LENGTHS, G, causal, cache, C, workspace):
            o, l, _bits, text = run8(qq, cache, G, C, ks, vs, causal=causal, workspace=workspace, out32=out32, want_l=want_l)
            assert ("_pieces" in text) == workspace and "attn_decode8_" in text, text
            check(f"fp8 {prec.name} D={D} G={G} R={R} causal={causal} split={workspace} O32={out32}{name}", o, l, qq, kb, vb, ks, vs, LENGTHS,
                  G, causal, out32=out32, pieces=dk.pieces_of(text), info=info)


def test_one_long_sequence_in_64_pieces():
    Hq, G, R, C, D = 64, 8, 1, 32768, 128
    q, kb, vb, ks, vs = make_case(1, Hq, G, R, C, D, torch.bfloat16, seed=77)
    lens = np.array([C], dtype=np.uint32)
    cache = Cache8(kb, vb, lens, "packed")
    for name, qq, info in both_inputs(q, kb, ks, lens, G, True, cache, C, True):
        o, l, _bits, text = run8(qq, cache, G, C, ks, vs, workspace=True)
        assert "attn_decode8_d128_bf16_pieces" in text and "64 pieces" in text, text
        check("fp8 long B=1 Hq=64 G=8 D=128 C=32768" + name, o, l, qq, kb, vb, ks, vs, lens, G, True, pieces=64, info=info)
        if info is not None:   # every piece's first and last key is some row's needle
            keys = decode_model.needle_keys(info)[0]
            assert all(b in keys and e - 1 in keys for b, e in decode_model.piece_ranges(C, 64)), "a piece boundary without a needle"


@pytest.mark.parametrize("prec,D,Hq,G,R", [(P.BF16, 128, 8, 4, 4), (P.FP16, 64, 8, 1, 4), (P.BF16, 64, 16, 8, 4), (P.FP16, 128, 6, 3, 1)])
def test_fewer_keys_than_rows_and_packed_groups_at_the_tile_edges(prec, D, Hq, G, R):
    """n < R (row r sees the keys c <= r below the length), G R = 32 exactly and G R odd, over an e4m3 cache"""
    C = 600
    lens = np.array([1, 2, 3, 4, 0, 5, 600], dtype=np.uint32)
    q, kb, vb, ks, vs = make_case(len(lens), Hq, G, R, C, D, DTYPE[prec], seed=470 + G)
    cache = Cache8(kb, vb, lens, "packed")
    for workspace in (False, True):
        for causal in (True, False):
            for name, qq, info in both_inputs(q, kb, ks, lens, G, causal, cache, C, workspace):
                o, l, _bits, text = run8(qq, cache, G, C, ks, vs, causal=causal, workspace=workspace, out32=causal)
                check(f"fp8 n < R {prec.name} D={D} G={G} R={R} causal={causal} split={workspace}{name}", o, l, qq, kb, vb, ks, vs, lens, G,
                      causal, out32=causal, pieces=dk.pieces_of(text), info=info)


# ------------------------------------------------------------------------------------------------- same inputs, the 16-bit route
@pytest.mark.parametrize("prec,D,G,R", [(P.BF16, 128, 8, 1), (P.FP16, 64, 4, 4), (P.FP16, 128, 1, 4), (P.BF16, 64, 8, 4)])
def test_same_values_through_the_16_bit_launch(prec, D, G, R):
    """NULL scales; the bytes converted to the 16-bit type (exact) go through mfa_attention_decode_launch: both launches see identical
    operands and differ in summation order only (the FP8 kernel permutes the contraction index of S = Q K^T), so the bound is the one
    tests/test_decode_gpu.py applies to split against unsplit"""
    C, Hq = 4096, 2 * G
    lens = np.array([4096, 1500, 65, 31, 1, 0], dtype=np.uint32)
    q, kb, vb, _ks, _vs = make_case(len(lens), Hq, G, R, C, D, DTYPE[prec], seed=900 + D + R)
    k16, v16 = (b.view(torch.float8_e4m3fn).to(DTYPE[prec]) for b in (kb, vb))
    assert torch.equal(k16.to(torch.float64), kb.view(torch.float8_e4m3fn).to(torch.float64))   # the conversion is exact
    for workspace in (False, True):
        c8, c16 = Cache8(kb, vb, lens, "packed"), dk.Cache(k16, v16, lens, "packed")
        for name, qq, info in both_inputs(q, kb, None, lens, G, True, c8, C, workspace):
            o8, l8, _b, t8 = run8(qq, c8, G, C, None, None, workspace=workspace, out32=True)
            o16, l16, _b, t16 = dk.run(qq, c16, G, C, workspace=workspace, out32=True)
            assert t8.replace("attn_decode8_", "attn_decode16_") == t16, (t8, t16)
            do, dl = float((o8 - o16).abs().max()), float((l8 - l16).abs().max())
            print(f"fp8 against the 16-bit launch {prec.name} D={D} G={G} R={R} split={workspace}{name}: max |dO| = {do:.3e} (fp32 O), "
                  f"max |dL| = {dl:.3e}")
            assert do <= TOL_O and dl / LOG2E <= TOL_L
            # each side on its own against the model: with FP32 O this is what gives the comparison a meaning
            how = dict(out32=True, pieces=dk.pieces_of(t8), info=info)
            check(f"fp8 side {prec.name} D={D} G={G} R={R} split={workspace}{name}", o8, l8, qq, kb, vb, None, None, lens, G, True, **how)
            check(f"16-bit side {prec.name} D={D} G={G} R={R} split={workspace}{name}", o16, l16, qq, kb, vb, None, None, lens, G, True, **how)


# ------------------------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("layout", ["paged:16", "paged:64", "paged:256", "token_major", "fused", "shared"])
@pytest.mark.parametrize("prec,D,Hq,G,R", [(P.BF16, 128, 16, 8, 2), (P.FP16, 64, 8, 4, 4)])
def test_layouts_are_bit_identical_to_packed(prec, D, Hq, G, R, layout):
    C, B = 1000, 9
    q, kb, vb, ks, vs = make_case(B, Hq, G, R, C, D, DTYPE[prec], seed=21 + D, shared=layout == "shared")
    lens = dk.lengths_for(B, C, R, seed=4, page=int(layout.split(":")[1]) if ":" in layout else 64)
    page = int(layout.split(":")[1]) if ":" in layout else None
    for workspace in (False, True):
        packed, other = Cache8(kb, vb, lens, "packed"), Cache8(kb, vb, lens, layout, seed=5)
        for name, qq, info in both_inputs(q, kb, ks, lens, G, True, other, C, workspace, page=page):
            o0, l0, b0, t0 = run8(qq, packed, G, C, ks, vs, workspace=workspace)
            o1, l1, b1, t1 = run8(qq, other, G, C, ks, vs, workspace=workspace)
            assert t0.replace("contiguous", "paged") == t1.replace("contiguous", "paged"), (t0, t1)   # the same kernels and piece count
            assert torch.equal(b0, b1), f"O differs between the {layout} and the packed cache"
            assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)), f"L differs between the {layout} and the packed cache"
            check(f"fp8 {layout} {prec.name} D={D} split={workspace}{name}", o1, l1, qq, kb, vb, ks, vs, lens, G, True,
                  pieces=dk.pieces_of(t1), page=page, info=info)


# ------------------------------------------------------------------------------------------------------------------- poison
@pytest.mark.parametrize("layout", ["packed", "paged:64", "paged:16"])
@pytest.mark.parametrize("prec,D,G,R", [(P.BF16, 128, 8, 1), (P.FP16, 64, 4, 4)])
def test_bytes_past_a_length_never_reach_a_product(prec, D, G, R, layout):
    C, B, Hq = 1000, 9, 2 * G
    q, kb, vb, ks, vs = make_case(B, Hq, G, R, C, D, DTYPE[prec], seed=55)
    lens = dk.lengths_for(B, C, R, seed=6, page=64)
    for workspace in (False, True):
        for causal in (True, False):
            on, ln, bn, _t = run8(q, Cache8(kb, vb, lens, layout, seed=8, poison=NAN8), G, C, ks, vs, causal=causal, workspace=workspace)
            oz, lz, bz, _t = run8(q, Cache8(kb, vb, lens, layout, seed=8, poison=0), G, C, ks, vs, causal=causal, workspace=workspace)
            assert bool(torch.isfinite(on).all()) and bool(torch.isfinite(ln).all())
            assert torch.equal(bn, bz) and torch.equal(ln.view(torch.int32), lz.view(torch.int32)), "0x7f past a length changed an output"


# ------------------------------------------------------------------------------------------------------------------- append
APPEND = [(prec, D, R, layout, fp8) for prec in (P.BF16, P.FP16) for D in (64, 128) for R in (1, 4)
          for layout in ("contiguous", "token_major", "paged:16", "paged:64", "paged:256") for fp8 in (True, False)]


@pytest.mark.parametrize("prec,D,R,layout,fp8", APPEND)
def test_append_writes_exactly_the_named_positions(prec, D, R, layout, fp8):
    dk.append_writes_exactly_the_named_positions(prec, D, R, layout, fp8)


# ---------------------------------------------------------------------------------------------------------------- round trip
def test_eight_generation_steps_append_then_decode():
    """kv_cache_append then flash_decode on a paged FP8 cache, the lengths growing on the device; sequence 1 crosses a page boundary"""
    from metal_flash_attention_amd.torch_binding import flash_decode, kv_cache_append
    dev, dtype = "cuda", torch.bfloat16
    B, Hq, G, D, ps, per, STEPS = 3, 16, 8, 128, 16, 4, 8
    Hkv = Hq // G
    g = torch.Generator().manual_seed(2025)
    start = np.array([0, 12, 37], dtype=np.int64)          # 12 + 8 = 20 crosses key 16
    rng = np.random.default_rng(3)
    pages = B * per + 2
    table = torch.from_numpy(rng.permutation(pages)[:B * per].reshape(B, per).astype(np.int32)).to(dev)
    poolk = torch.full((pages, Hkv, ps, D), NAN8, dtype=torch.uint8, device=dev).view(torch.float8_e4m3fn)
    poolv = torch.full((pages, Hkv, ps, D), NAN8, dtype=torch.uint8, device=dev).view(torch.float8_e4m3fn)
    ks, vs = (torch.from_numpy(decode_model.spread_scales(rng, Hkv)) for _ in range(2))
    ksd, vsd = ks.to(dev), vs.to(dev)
    history_k = [torch.randn(Hkv, int(n), D, generator=g).to(dtype) for n in start]
    history_v = [torch.randn(Hkv, int(n), D, generator=g).to(dtype) for n in start]
    lens = torch.from_numpy(start).to(torch.int32).to(dev)
    for b in range(B):   # the prompt, written by the append launch itself (R = its length is not a decode shape: row by row)
        for t in range(int(start[b])):
            one = torch.zeros(B, dtype=torch.int32, device=dev)
            one[b] = t + 1
            kn = torch.zeros(B, Hkv, 1, D, dtype=dtype)
            vn = torch.zeros(B, Hkv, 1, D, dtype=dtype)
            kn[b, :, 0], vn[b, :, 0] = history_k[b][:, t], history_v[b][:, t]
            kv_cache_append(kn.to(dev), vn.to(dev), poolk, poolv, one, block_table=table, k_scale=ksd, v_scale=vsd)
    for step in range(STEPS):
        kn, vn = torch.randn(B, Hkv, 1, D, generator=g).to(dtype), torch.randn(B, Hkv, 1, D, generator=g).to(dtype)
        for b in range(B):
            history_k[b] = torch.cat([history_k[b], kn[b]], dim=1)
            history_v[b] = torch.cat([history_v[b], vn[b]], dim=1)
        n = start + step + 1
        C = int(n.max())
        kb, vb = torch.zeros(B, Hkv, C, D, dtype=torch.uint8), torch.zeros(B, Hkv, C, D, dtype=torch.uint8)
        for b in range(B):
            kb[b, :, :int(n[b])] = quantise(history_k[b][None], ks.numpy())[0]
            vb[b, :, :int(n[b])] = quantise(history_v[b][None], vs.numpy())[0]
        # the step's query: the row just appended (key n - 1, the row's frontier) and the one before it are among its needles, so
        # an append that went to another position, page or head, or stale bytes there, move O far outside the bound
        q, info = dk.needle_q(dequantise(kb, ks.numpy()), n, Hq, G, 1, dtype, True, page=ps)
        assert all(int(n[b]) - 1 in info[(b, h, 0)][0] for b in range(B) for h in range(Hq))
        lens += 1                                            # on the device
        assert kv_cache_append(kn.to(dev), vn.to(dev), poolk, poolv, lens, block_table=table, k_scale=ksd, v_scale=vsd) is None
        o, lse = flash_decode(q.to(dev), poolk, poolv, lens, block_table=table, return_lse=True, k_scale=ksd, v_scale=vsd)
        assert bool(torch.isfinite(o.float()).all())
        check(f"round trip step {step} lengths {n.tolist()}", o.float().cpu(), (lse.cpu() * LOG2E), q, kb, vb, ks.numpy(), vs.numpy(),
              n.astype(np.uint32), G, True, page=ps, info=info)
    assert lens.cpu().tolist() == (start + STEPS).tolist()
