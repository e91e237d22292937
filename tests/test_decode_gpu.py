"""GPU test: decode attention over a KV cache through the C ABI of include/mfa_decode.h.

Expected values: a float64 numpy attention (softmax in natural units per (batch, head) over the first len_b keys, the mask rule of
mfa_decode.h) on the inputs after their rounding to the 16-bit type.  Tolerances: tests/harness.py TOL_MIXED (O 5e-2, L 7e-3 after
dividing by log2 e).  Every launch of this file runs on poisoned buffers: NaN in every key and value at or past each length (for
paged caches also in the tail of last pages and in pages the table does not name), the 0xCACA canary in the padding of O and L,
around the workspace and in a guard page behind the pool; after every launch no output holds a NaN, the canaries are intact and K,
V, the table and the lengths are byte-identical to before.

Beside those bounds every comparison with the model is held to the per-element bounds of tests/decode_model.py (derived from the
number formats; tests/test_decode_sensitivity.py proves on the CPU that they flag every named defect), and every test also runs
with that module's needle queries, in which single keys -- the first and last of every step, piece and page, each row's causal
frontier -- carry a visible share of the softmax, and the key just behind a row's frontier would take the row over.  Non-causal
launches have no such forbidden key: every key below the length is visible to every row.

Maxima seen on an MI355X are recorded in DESIGN.md 4.9.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import decode_kit as dk  # noqa: E402  (the values, caches, runner and model check shared with the e4m3 and the D = 256 file)
import decode_model  # noqa: E402
from decode_kit import DTYPE, LOG2E, TOL_L, TOL_O, Cache, both_inputs, check_against_model, lengths_for, make_values, pieces_of, run  # noqa: E402
from decode_model import MARGIN, bounds, compare, model  # noqa: E402,F401  (the bound proven by tests/test_decode_sensitivity.py)
from metal_flash_attention_amd import GEMMOperandPrecision as P  # noqa: E402

@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield


PARITY = [(prec, D, Hq, G, R) for prec in (P.BF16, P.FP16) for D in (64, 128) for Hq, G in ((8, 1), (8, 4), (32, 8), (16, 16))
          for R in (1, 2, 4) if G * R <= 32]


@pytest.mark.parametrize("index,case", list(enumerate(PARITY)), ids=lambda x: "-".join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_parity_with_the_float64_model(index, case):
    prec, D, Hq, G, R = case
    C, B = 600, 10
    q, k, v = make_values(B, Hq, G, R, C, D, DTYPE[prec], seed=100 + index)
    lens = lengths_for(B, C, R, seed=index, page=256)
    cache = Cache(k, v, lens, "packed")
    for variant in range(4):   # causal x workspace, with FP32 O and a NULL L rotating over the cases
        causal, workspace = bool(variant & 1), bool(variant & 2)
        out32, want_l = bool((index + variant) & 1), (index + variant) % 3 != 0
        for name, qq, info in both_inputs(q, k, lens, G, causal, cache, C, workspace):
            o, l, _bits, text = run(qq, cache, G, C, causal=causal, workspace=workspace, out32=out32, want_l=want_l)
            assert ("_pieces" in text) == workspace, text
            check_against_model(f"{prec.name} D={D} Hq={Hq} G={G} R={R} causal={causal} split={workspace} O32={out32}{name}", o, l, qq,
                                k, v, lens, G, causal, out32=out32, pieces=pieces_of(text), info=info)


@pytest.mark.parametrize("page", [16, 64, 256])
@pytest.mark.parametrize("prec,D,Hq,G,R", [(P.BF16, 128, 32, 8, 1), (P.FP16, 64, 8, 4, 4), (P.BF16, 64, 16, 16, 2)])
def test_paged_equals_contiguous_bit_for_bit(prec, D, Hq, G, R, page):
    C, B = 1000, 9
    q, k, v = make_values(B, Hq, G, R, C, D, DTYPE[prec], seed=page + D)
    lens = lengths_for(B, C, R, seed=page, page=page)
    for workspace in (False, True):
        packed, paged = Cache(k, v, lens, "packed"), Cache(k, v, lens, f"paged:{page}", seed=page)
        for name, qq, info in both_inputs(q, k, lens, G, True, paged, C, workspace, page=page):
            o0, l0, b0, t0 = run(qq, packed, G, C, workspace=workspace)
            o1, l1, b1, t1 = run(qq, paged, G, C, workspace=workspace)
            assert t0.replace("contiguous", "paged") == t1, (t0, t1)   # the same kernels and piece count
            assert torch.equal(b0, b1), "O differs between the paged and the contiguous cache"
            assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)), "L differs between the paged and the contiguous cache"
            check_against_model(f"paged {page} {prec.name} D={D} split={workspace}{name}", o1, l1, qq, k, v, lens, G, True,
                                pieces=pieces_of(t1), page=page, info=info)


@pytest.mark.parametrize("prec,D", [(P.BF16, 128), (P.FP16, 64)])
def test_split_against_unsplit(prec, D):
    Hq, G, R, C, B = 16, 8, 2, 4096, 3
    q, k, v = make_values(B, Hq, G, R, C, D, DTYPE[prec], seed=5)
    lens = np.array([C, 1500, 65], dtype=np.uint32)
    cache = Cache(k, v, lens, "packed")
    for name, qq, info in both_inputs(q, k, lens, G, True, cache, C, True):
        o0, l0, _b, t0 = run(qq, cache, G, C, workspace=False, out32=True)
        o1, l1, _b, t1 = run(qq, cache, G, C, workspace=True, out32=True)
        assert "_single" in t0 and "_pieces" in t1 and "_combine" in t1, (t0, t1)
        do, dl = float((o0 - o1).abs().max()), float((l0 - l1).abs().max())
        print(f"split against unsplit {prec.name} D={D}{name}: max |dO| = {do:.3e} (fp32 O), max |dL| = {dl:.3e}; {t1}")
        assert do <= TOL_O and dl / LOG2E <= TOL_L
        # each side on its own against the model: with FP32 O this is what gives the comparison a meaning
        check_against_model(f"unsplit side {prec.name} D={D}{name}", o0, l0, qq, k, v, lens, G, True, out32=True, info=info)
        check_against_model(f"split side {prec.name} D={D}{name}", o1, l1, qq, k, v, lens, G, True, out32=True, pieces=pieces_of(t1), info=info)


@pytest.mark.parametrize("prec,D,Hq,G,R,causal", [(P.BF16, 128, 32, 8, 1, True), (P.FP16, 64, 8, 4, 4, True), (P.BF16, 64, 8, 1, 2, False)])
def test_agrees_with_the_forward_kernel(prec, D, Hq, G, R, causal):
    dk.agrees_with_the_forward_kernel(prec, D, Hq, G, R, causal)


@pytest.mark.parametrize("layout", ["token_major", "fused", "shared"])
@pytest.mark.parametrize("prec,D,Hq,G,R", [(P.BF16, 128, 16, 8, 2), (P.FP16, 64, 8, 2, 1)])
def test_strided_layouts_are_bit_identical_to_packed(prec, D, Hq, G, R, layout):
    C, B = 900, 8
    q, k, v = make_values(B, Hq, G, R, C, D, DTYPE[prec], seed=21, shared=layout == "shared")
    lens = lengths_for(B, C, R, seed=4)
    for workspace in (False, True):
        packed, other = Cache(k, v, lens, "packed"), Cache(k, v, lens, layout)
        for name, qq, info in both_inputs(q, k, lens, G, True, other, C, workspace):
            o0, l0, b0, _t = run(qq, packed, G, C, workspace=workspace)
            o1, l1, b1, t1 = run(qq, other, G, C, workspace=workspace)
            assert torch.equal(b0, b1) and torch.equal(l0.view(torch.int32), l1.view(torch.int32)), layout
            check_against_model(f"{layout} {prec.name} D={D} split={workspace}{name}", o1, l1, qq, k, v, lens, G, True,
                                pieces=pieces_of(t1), info=info)


def test_one_long_sequence_split():
    Hq, G, R, C, D = 64, 8, 1, 32768, 128
    q, k, v = make_values(1, Hq, G, R, C, D, torch.bfloat16, seed=77)
    lens = np.array([C], dtype=np.uint32)
    cache = Cache(k, v, lens, "packed")
    for name, qq, info in both_inputs(q, k, lens, G, True, cache, C, True):
        o, l, _bits, text = run(qq, cache, G, C, workspace=True)
        assert "_pieces" in text and "64 pieces" in text, text
        check_against_model("long B=1 Hq=64 G=8 D=128 C=32768" + name, o, l, qq, k, v, lens, G, True, pieces=64, info=info)
        if info is not None:   # every piece's first and last key is some row's needle
            keys = decode_model.needle_keys(info)[0]
            assert all(b in keys and e - 1 in keys for b, e in decode_model.piece_ranges(C, 64)), "a piece boundary without a needle"


# packed groups at the edges of the 32-wide tile: G R = 32 exactly; G R odd (the columns >= M repeat the last one: O's padding and
# the rows of the next head are checked by run()'s canaries and by the model); fewer keys than rows
@pytest.mark.parametrize("prec,D,Hq,G,R", [(P.BF16, 128, 16, 8, 4), (P.FP16, 64, 32, 16, 2), (P.BF16, 64, 6, 3, 1), (P.FP16, 128, 10, 5, 3),
                                           (P.BF16, 128, 7, 7, 1)])
def test_packed_groups_of_exactly_32_and_of_odd_size(prec, D, Hq, G, R):
    C, B = 600, 8
    assert G * R == 32 or (G * R) % 2 == 1
    q, k, v = make_values(B, Hq, G, R, C, D, DTYPE[prec], seed=31 + G)
    lens = lengths_for(B, C, R, seed=G, page=256)
    cache = Cache(k, v, lens, "packed")
    for workspace in (False, True):
        for causal in (True, False):
            for name, qq, info in both_inputs(q, k, lens, G, causal, cache, C, workspace):
                o, l, _bits, text = run(qq, cache, G, C, causal=causal, workspace=workspace)
                check_against_model(f"M={G * R} {prec.name} D={D} G={G} R={R} causal={causal} split={workspace}{name}", o, l, qq, k, v, lens,
                                    G, causal, pieces=pieces_of(text), info=info)


@pytest.mark.parametrize("prec,D,Hq,G,R", [(P.BF16, 128, 8, 4, 4), (P.FP16, 64, 4, 1, 4)])
def test_fewer_keys_than_rows(prec, D, Hq, G, R):
    """n < R: max(n - R, 0) = 0, row r sees the keys c <= r below the length"""
    C = 600
    lens = np.array([1, 2, 3, 4, 0, 5, 600], dtype=np.uint32)
    B = len(lens)
    q, k, v = make_values(B, Hq, G, R, C, D, DTYPE[prec], seed=47)
    cache = Cache(k, v, lens, "packed")
    for workspace in (False, True):
        for causal in (True, False):
            for name, qq, info in both_inputs(q, k, lens, G, causal, cache, C, workspace):
                o, l, _bits, text = run(qq, cache, G, C, causal=causal, workspace=workspace, out32=causal)
                check_against_model(f"n < R {prec.name} D={D} G={G} R={R} causal={causal} split={workspace}{name}", o, l, qq, k, v, lens, G,
                                    causal, out32=causal, pieces=pieces_of(text), info=info)
