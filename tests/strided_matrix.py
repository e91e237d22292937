"""The cases of the strided-layout tests: tests/test_strided_layouts_gpu.py runs them, tests/test_strided_layout_plans.py plans them.

MATRIX covers kernel families, not shapes: every head-dimension bucket (and one head dimension per bucket that is not a head-block
size, so that Dr < head block meets a poisoned pad column), every storage type, lowPrecisionIntermediates on and off (it selects
the `_exact` / plain backward streams and the `_fold` forward streams).  Layouts rotate through it; every family meets `mixed` and one
of `token` / `fused` (asserted on the CPU).  KINDS puts every launch kind under the mixed and the token-major layout."""
import re

from strided import Case

HEADS = (32, 64, 72, 96, 128, 136, 160, 192, 200, 256, 264, 320, 384, 400)
STORAGES = (("bf16", False), ("bf16", True), ("f16", False), ("f16bf", False), ("f16bf", True), ("f32", False))
# ragged last blocks, whole tiles (256 x 512), another ragged pair; fused slices need R == C
SHAPES = ((300, 520), (256, 512), (203, 449))
ROTATION = ("mixed", "token", "mixed", "fused", "mixed", "padded", "mixed", "token")

# cases whose aligned layout plans another launch form than the packed one, with the reason from meets_fast_requirements: compared
# against the oracle only, and not counted towards their family
PINNED = {}


def _dense():
    cases = []
    for i, D in enumerate(HEADS):
        for k, (storage, mid) in enumerate(STORAGES):
            n = i + k
            layout = ROTATION[(i + 3 * k) % len(ROTATION)]
            R, C = SHAPES[n % 3] if layout != "fused" else (328, 328)
            cases.append(Case(storage, D, layout, Hq=3 + n % 4, R=R, C=C, mid=mid))
            # the other half of the pair (mixed <-> token-major), for the buckets' own head dimension only
            if D in (32, 64, 128, 160, 192, 256, 320, 384, 400):
                other = "token" if layout == "mixed" else "mixed"
                R2, C2 = SHAPES[(n + 1) % 3]
                cases.append(Case(storage, D, other, Hq=3 + (n + 1) % 4, R=R2, C=C2, mid=mid))
    return cases


MATRIX = _dense()

MASK = ((True, False, True, True, False), (True, False, False, True, True), (False, False, False, False, False))   # 768 x 640
BUCKETS = (("bf16", 64), ("bf16", 128), ("f16bf", 256), ("f32", 128))   # 16-bit at or below 128 (p6 and p4p), above 128, FP32


def _kinds():
    cases = []
    for layout in ("mixed", "token"):
        for storage, D in BUCKETS:
            low = storage != "f32"
            cases += [
                Case(storage, D, layout, causal=True),                                        # R < C
                Case(storage, D, layout, causal=True, R=328, C=328),
                Case(storage, D, layout, lengths=((300, 131), (97, 520))),
                Case(storage, D, layout, mask=MASK, R=700, C=640),
                Case(storage, D, layout, Hq=4, G=2),
                Case(storage, D, layout, Hq=4, G=4),
                Case(storage, D, layout, transposed="all", ws=True, R=304, C=512),            # forward in place, backward re-layout
            ]
            if low:
                cases += [
                    Case(storage, D, layout, ws=True),                                        # forward and dQ column-parallel
                    Case(storage, D, layout, ws=True, causal=True),
                    Case(storage, D, layout, ws=True, B=1, Hq=3, R=1024, C=264),              # dK / dV row-parallel
                    Case(storage, D, layout, out16=True),
                    Case(storage, D, layout, out16=True, Hq=4, G=2),                          # group sums stored in 16 bits
                    Case(storage, D, layout, transposed="kv", ws=True, R=304, C=512),
                    Case(storage, D, layout, transposed="kv", ws=True, Hq=4, G=2, R=304, C=544),   # group sum: element path
                ]
        # transposed operands without a workspace: the in-place backward kernels of the 128 bucket
        cases.append(Case("bf16", 128, layout, transposed="all", R=320, C=512))
        cases.append(Case("bf16", 192, layout, transposed="kv", ws=True, R=304, C=512))
        cases.append(Case("bf16", 320, layout, transposed="all", ws=True, R=304, C=512))
        # the siblings only masked launches name: the `_fold` forward streams, the 32-row forward objects of D = 160 and 192
        cases += [Case("bf16", 64, layout, mask=MASK, R=700, C=640, mid=True), Case("f16bf", 128, layout, mask=MASK, R=700, C=640, mid=True),
                  Case("bf16", 160, layout, mask=MASK, R=700, C=640), Case("f16bf", 192, layout, mask=MASK, R=700, C=640)]
        # the forward code objects of the other transposition patterns, read in place
        cases += [Case("bf16", 64, layout, transposed=t, R=304, C=520, types=("forward",)) for t in ("q", "k", "v")]
        # persistent forward forms: more (row block, head, batch) entries than compute units
        cases.append(Case("bf16", 128, layout, B=4, Hq=24, R=700, C=264, types=("forward",)))
        cases.append(Case("f16bf", 64, layout, B=4, Hq=24, R=700, C=264, mid=True, types=("forward",)))
    # padded dK / dV views under the group sum (its 16-byte path), and D % 8 != 0 is not reachable with aligned rows
    cases += [Case("bf16", 128, "padded", Hq=4, G=2), Case("f32", 64, "padded", Hq=6, G=6), Case("f16bf", 256, "padded", Hq=4, G=4, out16=True)]
    return cases


KINDS = _kinds()

BROADCAST = [Case(s, D, "broadcast", Hq=4, types=("forward", "backwardQuery")) for s, D in BUCKETS + (("bf16", 320), ("f32", 400))]

MISALIGNED = [Case(s, D, layout, Hq=3, R=203, C=264) for s, D in (("bf16", 128), ("f16", 64), ("f16bf", 256), ("f32", 128))
              for layout in ("misaligned_ld", "misaligned_ptr")]

ALL_CASES = MATRIX + KINDS + BROADCAST + MISALIGNED


def family_of(name):
    """code-object or launch-form name -> kernel family: the name without storage type, head-dimension bucket and geometry; the tags
    that name another instruction stream stay (_exact, _fold, the transposition patterns, the 32-row forward objects' options)"""
    m = re.match(r"^(attn_[a-z0-9]+)_(?:bf16|f16)(?:_dObf16)?_d\d+_(.*)$", name)
    if m:
        tags = [t for t in ("exact", "fold", "tr_kv", "tr_k", "tr_v", "tr", "ldsdma", "ring2_spread", "kpad") if re.search(r"(^|_)%s(_|$)" % t, m.group(2))]
        if "tr_kv" in tags or "tr_k" in tags or "tr_v" in tags:
            tags = [t for t in tags if t != "tr"]
        return "_".join([m.group(1)] + tags)
    m = re.match(r"^(attn_f32_[a-z]+)_d\d+", name) or re.match(r"^(attn_generic_[a-z]+)_f32mfma", name) or re.match(r"^(attn_paged_[a-z]+)_f32", name)
    return m.group(1) if m else name
