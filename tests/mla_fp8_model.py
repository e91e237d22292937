"""The float64 model of multi-head latent attention decode over an E4M3 latent cache (include/mfa_mla_cache.h), its per-element bounds,
the byte inputs, the named mutants and the cases the CPU and GPU files share.  A plain module on top of tests/mla_model.py and
tests/decode_model.py, which it imports and changes neither (numpy only).

Inputs are BYTES.  A cache is drawn as e4m3 bytes (never 0x7f / 0xff inside a length) and the model reads kvScale x dequantize(byte):
quantisation error is no part of the bound.  The launch computes exactly mla_model's attention over those values, so

  model()          mla_model.model() over kvScale x dequantize(bytes), or a named WRONG attention (MUTANTS): every mutant of mla_model
                   that applies, and this kernel's own.  No wrong kernel is ever run.
  emulated()       the attention with the roundings and the order of sums of attn_mla8.h: what a correct kernel may give.
  CASES, inputs()  mla_model.CASES -- its lengths (700, 200, 100, 5, 0, 1500) in 1536 keys -- restated over byte caches, each with a
                   kvScale of (None, 0.37, 3.0) in turn: non-powers of two make a missing or doubled scale visible.  SEAM_CASES are
                   mla_model.SEAM_CASES -- the lengths on the step, page, tile and column seams -- restated the same way.

The bound is mla_model's (its docstring) with what attn_mla8.h adds.  The kernel contracts the same 576 exact products per score -- the
conversion e4m3 -> 16-bit is exact, and a permuted contraction order is one more order of the same sum, which the (Dk + 3) u worst case
over ONE chain already covers -- and runs the same steps, exchange, softmax and second product.  Two roundings are new:
  * the score scale is fl(fl(scale log2 e) x kvScale) where mla_model's is fl(scale log2 e): one more rounding on every score, (Dk + 4) u
    in place of (Dk + 3) u.  Every term of E and EL that the score's error enters is linear in that count, and the remaining terms are
    non-negative, so E (1 + 1 / (Dk + 3)) and EL (1 + 1 / (Dk + 3)) cover it.
  * the output: mult = fl(fl(1 / l) x kvScale) unsplit, and a piece publishes fl(o x kvScale) -- one more product on the chain, which is
    chain + 1 roundings on a sum of magnitude A + |O|.  chain >= 34 + 2 + 12 = 48, so u (A + |O|) <= E / 48.  L never meets it.
  E' = E (1 + 1 / (Dk + 3) + 1 / 48),  EL' = EL (1 + 1 / (Dk + 3)); bounds() and compare() are decode_model's over them.
MARGIN is fixed by tests/test_mla_fp8_sensitivity.py alone, before any device run: the smallest power of two with at least 2 x headroom
over emulated()'s worst err / bound at margin 1 on CASES and SEAM_CASES together.
"""
import functools

import numpy as np

import decode_model as dm
import mla_model as mm
from decode_model import Reference, bounds, compare, piece_ranges, round_to, store  # noqa: F401
from mla_model import C, DK, DV, LENS, ROWS, SCALE, SEAM_C, SEAM_LENS, SEAM_MUTANTS, STEP, TILE, facts_of, seen_lens  # noqa: F401

MARGIN = 2
KV_SCALES = (0.37, 3.0, None)
# what lies behind kvScale[0] in the array the GPU test passes: a kernel that reads kvScale[b] finds these for b = 1 ..
SCALE_TAIL = (1.9, 0.6, 2.4, 0.8, 1.3)
POISON = (0x7F, 0xFF)


def dequantize(byte):
    """float64 values of e4m3 bytes (OCP e4m3fn; mfa_kv_dequantize_e4m3, which tests/test_mla_fp8_sensitivity.py holds this to)"""
    b = np.asarray(byte, dtype=np.int64)
    e, m = (b >> 3) & 15, b & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * 2.0 ** (e - 7.0))
    out = np.where(b & 0x80, -mag, mag)
    return np.where((b & 0x7F) == 0x7F, np.nan, out)


def values_of(kvb, kvscale):
    """what the launch's cache bytes stand for: kvScale x e4m3(byte), kvScale as the FP32 number the device holds"""
    return dequantize(kvb) * (1.0 if kvscale is None else float(np.float32(kvscale)))


# ---------------------------------------------------------------------------------------------------------------------- mutants
# name -> (what the defect is, where it changes nothing).  `case` has mla_model's n, R, H, B, causal, pieces, page and kvscale.
_plain = lambda c: c["kvscale"] is None  # noqa: E731
OWN_MUTANTS = {
    "kv_scale_out_of_score": ("kvScale left out of the score", _plain),
    "kv_scale_out_of_o": ("kvScale left out of O", _plain),
    "kv_scale_twice_in_pieces": ("kvScale applied to O by the piece kernel and again at the end", lambda c: _plain(c) or not c["pieces"]),
    "k_halves_exchanged": ("the two 8-column halves of a converted 16-byte load exchanged on the K side only", lambda c: False),
    "v_halves_exchanged": ("the 16 hi halves of a d block exchanged in the V image", lambda c: False),
    "rope_read_as_16bit": ("the rotary bytes addressed as if 16-bit: rotary column c read from byte 512 + 2 c mod 64", lambda c: False),
    "kv_scale_per_sequence": ("the scale read as kvScale[b]", lambda c: _plain(c) or c["B"] == 1),
}
MUTANTS = dict(mm.MUTANTS, **OWN_MUTANTS)   # (every mutant of mla_model applies: the geometry, the mask and the pieces are its own)

_K_HALVES = np.r_[(np.arange(DV) // 16) * 16 + (np.arange(DV) % 16 + 8) % 16, np.arange(DV, DK)]   # latent only; the rotary fragment keeps its order
_V_HALVES = (np.arange(DV) // 32) * 32 + (np.arange(DV) % 32 + 16) % 32
_ROPE_DOUBLED = np.r_[np.arange(DV), DV + (2 * np.arange(DK - DV)) % (DK - DV)]


def model(q, kvb, kvscale, lens, causal, scale, mutant=None, *, pieces=None, page=None, shared=False, piece_range=None):
    """float64 attention over a byte cache kvb [B, C, 576] uint8 -> Reference(O, L, A, E', EL') (module docstring); `mutant`: a named
    wrong attention (its E / EL mean nothing)"""
    assert mutant is None or mutant in MUTANTS, mutant
    kw = dict(pieces=pieces, page=page, shared=shared, piece_range=piece_range)
    kvs = 1.0 if kvscale is None else float(np.float32(kvscale))
    deq = np.where(np.isnan(dequantize(kvb)), 0.0, dequantize(kvb))   # (poison past a length is never read by the model either)
    kv = deq * kvs
    if mutant is None:
        ref = mm.model(q, kv, lens, causal, scale, **kw)
        return Reference(ref.O, ref.L, ref.A, ref.E * (1.0 + 1.0 / (DK + 3) + 1.0 / 48), ref.EL * (1.0 + 1.0 / (DK + 3)))
    if mutant in mm.MUTANTS:
        return mm.model(q, kv, lens, causal, scale, mutant, **kw)
    split = bool(pieces) and pieces > 1
    if mutant == "kv_scale_out_of_score":       # q . (kvs k) x (scale / kvs) = q . k x scale
        return mm.model(q, kv, lens, causal, scale / kvs, **kw)
    if mutant == "k_halves_exchanged":          # q . perm(k) = perm(q) . k: the permutation is its own inverse, and V does not see it
        return mm.model(dm.f64(q)[..., _K_HALVES], kv, lens, causal, scale, **kw)
    if mutant == "rope_read_as_16bit":          # (V is the first 512 columns: only the key changes)
        return mm.model(q, kv[..., _ROPE_DOUBLED], lens, causal, scale, **kw)
    if mutant == "kv_scale_per_sequence":
        B = len(lens)
        per = np.array([kvs] + [float(np.float32(s)) for s in (SCALE_TAIL * B)[:B - 1]])
        seen = np.broadcast_to(deq[:1], (B,) + deq.shape[1:]) if shared else deq
        return mm.model(q, seen * per[:, None, None], lens, causal, scale, **dict(kw, shared=False))
    ref = mm.model(q, kv, lens, causal, scale, **kw)
    if mutant == "kv_scale_out_of_o":
        return ref._replace(O=ref.O / kvs)
    if mutant == "kv_scale_twice_in_pieces":
        return ref._replace(O=ref.O * kvs) if split else ref
    if mutant == "v_halves_exchanged":
        return ref._replace(O=ref.O[..., _V_HALVES])
    raise AssertionError(mutant)


# ------------------------------------------------------------------------------------------------- the rounding-emulated reference
def emulated(q, kvb, kvscale, lens, causal, scale, fmt, *, pieces=None, shared=False, piece_range=None):
    """the attention with the roundings and the order of sums of attn_mla8.h -> (O before the store's rounding [B, H, R, 512], L natural).
    mla_model.emulated() over the UNSCALED values e4m3(byte), with what the scale changes: the score scale is
    fl(fl(fl(scale) x fl(log2 e)) x kvScale); unsplit, O is multiplied by fl(fl(1 / l) x kvScale); a piece publishes fl(o x kvScale) and the
    combine normalises"""
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    q, deq = dm.f64(q), dequantize(kvb)
    kvs = 1.0 if kvscale is None else f32(kvscale)
    B, H, R, _ = q.shape
    O = np.zeros((B, H, R, DV))
    L = np.full((B, H, R), -np.inf)
    rows = np.arange(R)[:, None]
    NEG = -np.inf
    scale2 = f32(np.float32(np.float32(scale) * np.float32(1.44269504089)) * np.float32(kvs))
    for b in range(B):
        n = min(int(lens[b]), deq.shape[1])
        if n == 0:
            continue
        ranges = piece_ranges(n, pieces, piece_range)
        split = len(ranges) > 1
        cols = np.arange(n)[None, :]
        K = deq[0 if shared else b, :n]
        V = K[:, :DV]
        for h in range(H):
            S2 = (q[b, h] @ K.T) * scale2
            vis = np.broadcast_to(cols < n, S2.shape)
            if causal:
                vis = vis & (cols <= rows + max(n - R, 0))
            S2 = np.where(vis, S2, NEG)
            published = []
            for (pb, pe) in ranges:
                m, l, o = np.full(R, NEG), np.zeros(R), np.zeros((R, DV))
                for key0 in range(pb, pe, STEP):
                    s = S2[:, key0:min(key0 + STEP, pe)]
                    new = np.maximum(m, s.max(axis=1))
                    fin = np.isfinite(new)
                    ref = np.where(fin, new, 0.0)
                    corr = np.where(np.isfinite(m), np.exp2(np.where(np.isfinite(m), m, 0.0) - ref), 1.0)
                    p = np.where(fin[:, None], np.exp2(s - ref[:, None]), 0.0)
                    m, l, o = new, l * corr + p.sum(axis=1), o * corr[:, None] + round_to(p, fmt) @ V[key0:min(key0 + STEP, pe)]
                published.append((m, l, round_to(o * kvs, "f32") if split else o))
            mstar = np.full(R, NEG)
            for m, l, _o in published:
                mstar = np.maximum(mstar, np.where(l > 0, m, NEG))
            lt, ot = np.zeros(R), np.zeros((R, DV))
            for m, l, o in published:
                live = (l > 0) & np.isfinite(m)
                w = np.where(live, np.exp2(np.where(live, m - np.where(np.isfinite(mstar), mstar, 0.0), 0.0)), 0.0)
                lt += w * l
                ot += w[:, None] * o
            seen = lt > 0
            l0 = np.where(seen, lt, 1.0)
            mult = 1.0 / l0 if split else round_to(round_to(1.0 / l0, "f32") * kvs, "f32")
            O[b, h] = np.where(seen[:, None], ot * mult[:, None], 0.0)
            L[b, h] = np.where(seen, (np.where(seen, mstar, 0.0) + np.log2(l0)) / dm.LOG2E, -np.inf)
    return O, L


# ---------------------------------------------------------------------------------------------------------------------- the cases
# mla_model's launches, each over a byte cache with one of KV_SCALES in turn; "ld640": rows 640 BYTES apart
CASES = {name: dict(case, kvscale=KV_SCALES[i % len(KV_SCALES)]) for i, (name, case) in enumerate(mm.CASES.items())}
SEAM_CASES = {name: dict(case, kvscale=KV_SCALES[i % len(KV_SCALES)]) for i, (name, case) in enumerate(mm.SEAM_CASES.items())}
ALL_CASES = dict(CASES, **SEAM_CASES)
planned_pieces = mm.planned_pieces   # (the plan of the e4m3 launch is the 16-bit launch's: tests/test_mla_cache_plans.py)


@functools.lru_cache(maxsize=None)
def cache_bytes(seed=0, batches=len(LENS), column=C):
    """kv [B, C, 576] uint8: e4m3 bytes of magnitude <= 1.0 (codes 0x00 .. 0x38) with a random sign, every key a value -- never 0x7f / 0xff"""
    rng = np.random.default_rng(2000 + seed + (0 if (batches, column) == (len(LENS), C) else 7 * column))
    shape = (batches, column, DK)
    return (rng.integers(0, 0x39, shape) | (rng.integers(0, 2, shape) << 7)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(case, pieces, q, kv bytes, Reference, needle info) of a case of CASES or SEAM_CASES, computed once and shared; the lengths are
    the case's own (mla_model.inputs)"""
    case = ALL_CASES[name]
    pieces = planned_pieces(case)
    lens = case["lens"]
    kvb = cache_bytes(0, len(lens), case["C"])
    shared = case["layout"] == "shared"
    q, info = mm.needle_queries(values_of(kvb, case["kvscale"]), lens, case["H"], case["R"], case["causal"], case["fmt"], SCALE, pieces=pieces,
                                page=case["page"], shared=shared)
    ref = model(q, kvb, case["kvscale"], lens, case["causal"], SCALE, pieces=pieces, page=case["page"], shared=shared)
    return case, pieces, q, kvb, ref, info
