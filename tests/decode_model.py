"""The float64 model of decode attention, its per-element error bounds, the needle inputs and the named mutants (a plain module, as
tests/strided.py; numpy only).

  model()          float64 attention over the first len_b keys of a cache (the mask rule of include/mfa_decode.h), O, L and
                   A = sum_i p_i |v_i| per output element, plus the FP32 terms of the bound.  mutant= computes a named WRONG attention
                   instead (MUTANTS): what a defect of the kernels or the host plan would compute.  No wrong kernel is ever run.
  bounds()         per-element bounds on |O - O_ref| and |L - L_ref| from the number formats the kernels round to (derivation below).
  emulated()       the same attention with the kernel's roundings and summation order (P rounded to the 16-bit type against the
                   running maximum of its wave, sums per wave, per piece, then combined; the store's rounding): what a correct
                   kernel may give.  tests/test_decode_sensitivity.py requires it inside the bounds and every mutant outside.
  needle_queries() query rows in which individual keys matter.
  compare()        got against model under the bounds: worst err / bound, and the coordinates of the worst element.

The bound.  With p_i the normalised weights, the kernel computes O = sum_i p_i v_i with these roundings:
  * P is cast to the 16-bit type with round-to-nearest before the second product (`(T)p`, attn_decode16.h), the normaliser l sums
    the unrounded p: |dO| <= u_P A, u_P = 2^-8 (bf16: 8 significand bits, half an ulp) or 2^-11 (f16).
  * the store: bf16 truncates (pack16: one ulp, 2^-7), f16 rounds to nearest (2^-11), FP32 2^-23: |dO| <= u_out |O|.
  * FP32 arithmetic, u = 2^-24 per operation, every count a worst case (errors add up linearly):
      - a score is a dot product of D exact products summed in FP32 and multiplied by scale2 = fl(log2 e / sqrt D) (x keyScale):
        its error in log2 units is e_i <= (D + 3) u scale2 sum_d |q_d k_id|; then s_i - m rounds once more (u |s_i - m|), each
        rescale by exp2(m_old - m_new) likewise (their arguments sum to at most the spread of the scores), and the hardware exp2 is
        good to one ulp (2 u).  p_i so carries the RELATIVE error rel_i = ln 2 (e_i + 3 u spread) + 4 u.  It moves the numerator by
        sum_i rel_i p_i |v_i| and, through l, O by |O| sum_i rel_i p_i.
      - the accumulators: a wave adds 2 x 16 products and rescales once per step it owns, the four waves merge (5), the pieces
        combine (pieces + 1), the normalisation and the value scale (3): chain = 34 steps_per_wave + pieces + 9 roundings on a sum
        of magnitude A (numerator) and 1 (l): chain u (A + |O|).
    E = sum_i rel_i p_i |v_i| + |O| sum_i rel_i p_i + chain u (A + |O|) is what the issue calls u_acc A.
  bound_O = margin (u_P A + u_out |O| + E) + tiny,   tiny = 2^-24 (the spacing of f16 subnormals; far below any other term).
  L = m + log2 l: the shift m cancels (l is relative to it), so in natural units |dL| <= sum_i rel_i p_i + chain u
  + 4 u (|m| + |ln l| + |L|) (log2f, the add, the store, the test's division by log2 e).
  bound_L = margin EL + tiny.

MARGIN is the smallest power of two with at least 2 x headroom over the worst err / bound at margin 1 of emulated() on every case of
tests/test_decode_sensitivity.py and of the kernels on every GPU test (DESIGN.md 4.9, 4.10 record both).
"""
import math
from typing import NamedTuple

import numpy as np

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
U32 = 2.0 ** -24
TINY = 2.0 ** -24
STEP, WAVES, TILE = 32, 4, 64                      # keys per wave step, waves per workgroup, keys per piece tile (attn_decode16.h)
U_P = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
U_OUT = {"bf16": 2.0 ** -7, "f16": 2.0 ** -11, "f32": 2.0 ** -23}
MARGIN = 2
OLD_TOL_O, OLD_TOL_L = 5e-2, 7e-3                  # tests/harness.py TOL_MIXED, the bounds the GPU files asserted alone before


class Reference(NamedTuple):
    O: np.ndarray    # [B, Hq, R, D]
    L: np.ndarray    # [B, Hq, R] natural units, -inf for a row without a visible key
    A: np.ndarray    # [B, Hq, R, D] sum_i p_i |v_i|
    E: np.ndarray    # [B, Hq, R, D] the FP32 term of the O bound (absolute)
    EL: np.ndarray   # [B, Hq, R]    the FP32 bound on L (absolute, natural units)


def f64(t):
    if isinstance(t, np.ndarray):
        return t.astype(np.float64)
    return t.detach().cpu().to(dtype=__import__("torch").float64).numpy()


def fmt_of(dtype):
    return "bf16" if "bfloat16" in str(dtype) or str(dtype).endswith("BF16") else "f16"


def round_to(x, fmt, trunc=False):
    """float64 -> the values of format `fmt` (through FP32, as the kernel), round-to-nearest-even or truncated"""
    x32 = np.ascontiguousarray(x, dtype=np.float32)
    if fmt == "f32":
        return x32.astype(np.float64)
    if fmt == "f16":
        assert not trunc
        with np.errstate(over="ignore"):
            return x32.astype(np.float16).astype(np.float64)
    bits = x32.view(np.uint32)
    bits = (bits & np.uint32(0xFFFF0000)) if trunc else ((bits + np.uint32(0x7FFF) + ((bits >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000))
    return bits.view(np.float32).astype(np.float64)


def store(x, out):
    """the rounding of the O store: bf16 truncates (pack16), f16 and FP32 round to nearest"""
    return round_to(x, out, trunc=out == "bf16")


def library_piece_range(length, pieces, piece):
    from metal_flash_attention_amd import AttentionDecode
    return AttentionDecode.pieceRange(length, pieces, piece)


def piece_ranges(n, pieces, piece_range=None):
    """[(begin, end)] of every piece, from mfa_attention_decode_piece_range; one range without a split"""
    if not pieces or pieces <= 1:
        return [(0, int(n))]
    fn = piece_range or library_piece_range
    return [tuple(fn(int(n), int(pieces), i)) for i in range(int(pieces))]


def chain_length(n, pieces):
    tiles = (n + TILE - 1) // TILE
    per = -(-tiles // pieces) * TILE if pieces and pieces > 1 else n
    steps = -(-(-(-per // STEP)) // WAVES)
    return 34 * steps + (pieces or 1) + 9


# ---------------------------------------------------------------------------------------------------------------------- mutants
# name -> (what the defect is, where it changes nothing).  `case` has n, R, G, Hkv, B, causal, pieces, page, scales (bool).
MUTANTS = {
    "o_zero": ("O = 0 everywhere", lambda c: False),
    "rows_swapped": ("the R rows of a packed group swapped", lambda c: c["R"] == 1),
    "head_mod_r": ("head p % R, row p / R in place of head p / R, row p % R", lambda c: c["G"] * c["R"] == 1),
    "kv_head_mod": ("K/V head h % Hkv in place of h // G", lambda c: c["Hkv"] == 1 or c["G"] == 1),
    "wave_last_step_dropped": ("one wave never runs its last step (the step before the sequence's last)", lambda c: c["n"] <= STEP),
    "final_partial_step_dropped": ("the partial last step is not run", lambda c: c["n"] % STEP == 0),
    "len_minus_2": ("c < len replaced by c <= len - 2", lambda c: False),
    "key0_dropped": ("key 0 never seen", lambda c: False),
    "causal_plus_1": ("causal frontier one key too far", lambda c: not c["causal"] or c["R"] == 1 or c["n"] < 2),
    "causal_minus_1": ("causal frontier one key short", lambda c: not c["causal"]),
    "max_dropped": ("max(n - R, 0) replaced by n - R", lambda c: not c["causal"] or c["n"] >= c["R"]),
    "v_rows_exchanged": ("two V rows of one 16-key group exchanged", lambda c: c["n"] < 2),
    "v_dblocks_exchanged": ("the first two 32-wide d blocks of V exchanged", lambda c: False),
    "piece_loses_last_tile": ("every piece stops one 64-key tile early", lambda c: not c["pieces"]),
    "piece_overlaps": ("every piece starts one tile early, inside its neighbour", lambda c: not c["pieces"] or c["n"] <= TILE),
    "combine_ignores_maxima": ("the combine adds the pieces without exp2(m_s - m*)", lambda c: not c["pieces"] or c["n"] <= TILE),
    "combine_counts_empty": ("a piece without a visible key enters the combine as a step of zero keys scored 0", lambda c: not c["pieces"] or -(-c["n"] // TILE) >= c["pieces"]),
    "page_table_neighbour": ("the block-table row of the next sequence", lambda c: not c["page"] or c["B"] == 1),
    "page_off_by_one": ("the first 16-key group of a page read from the page before", lambda c: not c["page"] or c["n"] <= c["page"]),
    "k_contraction_permuted": ("the FP8 kernel's permutation of d applied to K only", lambda c: False),
    "key_scale_not_folded": ("keyScale left out", lambda c: not c["scales"]),
    "key_scale_next_head": ("keyScale of head j + 1", lambda c: not c["scales"] or c["Hkv"] == 1),
    "value_scale_twice": ("valueScale applied by the piece and by the combine", lambda c: not c["scales"] or not c["pieces"]),
    "value_scale_next_head": ("valueScale of head j + 1", lambda c: not c["scales"] or c["Hkv"] == 1),
}


def fp8_k_permutation(D):
    """d index the FP8 kernel contracts where the 16-bit kernel contracts d: the 8-wide blocks 1 and 2 of every 32 exchanged"""
    d = np.arange(D)
    blk = (d // 8) % 4
    return np.where(blk == 1, d + 8, np.where(blk == 2, d - 8, d))


def model(q, k, v, lens, G, causal, mutant=None, *, pieces=None, page=None, kscale=None, vscale=None, piece_range=None):
    """float64 attention -> Reference(O, L, A, E, EL).  k, v [B, Hkv, C, D] hold the cache's values WITHOUT the per-head scales when
    kscale / vscale are given.  pieces / page: the launch's geometry (they change the bound's chain length and what the mutants do,
    never the unmutated values)."""
    assert mutant is None or mutant in MUTANTS, mutant
    q, k, v = f64(q), f64(k), f64(v)
    B, Hq, R, D = q.shape
    Hkv = Hq // G
    ks = np.ones(Hkv) if kscale is None else np.asarray(kscale, dtype=np.float64)
    vs = np.ones(Hkv) if vscale is None else np.asarray(vscale, dtype=np.float64)
    O, A, E = (np.zeros((B, Hq, R, D)) for _ in range(3))
    L = np.full((B, Hq, R), -np.inf)
    EL = np.zeros((B, Hq, R))
    rows = np.arange(R)[:, None]
    for b in range(B):
        n = int(lens[b])
        if n == 0:
            continue
        ranges = piece_ranges(n, pieces, piece_range)
        split = len(ranges) > 1
        cols = np.arange(n)[None, :]
        chain = chain_length(n, pieces) * U32
        for h in range(Hq):
            j = h // G
            if mutant == "kv_head_mod":
                j = h % Hkv
            kb = (b + 1) % B if mutant == "page_table_neighbour" and page else b
            K, V = k[kb, j, :n], v[kb, j, :n]
            if mutant == "page_off_by_one" and page:
                src = np.arange(n)
                first = (src >= page) & (src % page < 16)
                src = np.where(first, src - page, src)
                K, V = k[b, j][src], v[b, j][src]
            if mutant == "v_rows_exchanged" and n >= 2:
                src = np.arange(n)
                x = 30 if n >= 32 else 0
                src[x], src[x + 1] = x + 1, x
                V = V[src]
            if mutant == "k_contraction_permuted":
                K = K[:, fp8_k_permutation(D)]
            ksc = 1.0 if mutant == "key_scale_not_folded" else ks[(j + 1) % Hkv] if mutant == "key_scale_next_head" else ks[j]
            vsc = vs[(j + 1) % Hkv] if mutant == "value_scale_next_head" else vs[j]
            if mutant == "value_scale_twice" and split:
                vsc = vsc * vsc
            qh, qrow = q[b, h], rows
            if mutant == "head_mod_r":
                p = (h % G) * R + np.arange(R)
                qh = q[b, (h // G) * G + (p % R) % G, (p // R) % R]
                qrow = ((p // R) % R)[:, None]
            S = (qh @ K.T) * (ksc / math.sqrt(D))
            limit = n - 1 if mutant == "len_minus_2" else n
            vis = np.broadcast_to(cols < limit, S.shape).copy()
            if causal:
                base = n - R if mutant == "max_dropped" else max(n - R, 0)
                off = 1 if mutant == "causal_plus_1" else -1 if mutant == "causal_minus_1" else 0
                vis &= cols <= qrow + base + off
            if mutant == "key0_dropped":
                vis[:, 0] = False
            if mutant == "wave_last_step_dropped" and n > STEP:
                t = (n - 1) // STEP - 1
                vis[:, t * STEP:(t + 1) * STEP] = False
            if mutant == "final_partial_step_dropped" and n % STEP:
                vis[:, n // STEP * STEP:] = False
            mult = np.ones(n)
            if split and mutant == "piece_loses_last_tile":
                for (pb, pe) in ranges:
                    if pe > pb:
                        vis[:, max(pb, (pe - 1) // TILE * TILE):pe] = False
            if split and mutant == "piece_overlaps":
                for (pb, pe) in ranges:
                    if pe > pb and pb >= TILE:
                        mult[pb - TILE:pb] += 1.0
            Sm = np.where(vis, S, -np.inf)
            m = Sm.max(axis=1, keepdims=True)
            seen = np.isfinite(m[:, 0])
            m0 = np.where(np.isfinite(m), m, 0.0)
            pw = np.exp(Sm - m0) * mult
            parts = []
            if split and mutant in ("combine_ignores_maxima", "combine_counts_empty"):
                for (pb, pe) in ranges:
                    parts.append((pb, pe, Sm[:, pb:pe].max(axis=1, keepdims=True) if pe > pb else np.full((R, 1), -np.inf)))
                if mutant == "combine_counts_empty" and all(np.isfinite(pm).all() for _, _, pm in parts):
                    parts = []   # no piece is empty for any row: the defect changes nothing
                if mutant == "combine_ignores_maxima" and sum(1 for pb, pe, _ in parts if pe > pb) <= 1:
                    parts = []   # one piece holds every key: nothing to weigh
            if parts:
                num, den, mstar = np.zeros((R, D)), np.zeros((R, 1)), m0.copy()
                if mutant == "combine_counts_empty":
                    mstar = np.maximum(mstar, np.where([[any(not np.isfinite(pm[r, 0]) for _, _, pm in parts)] for r in range(R)], 0.0, -np.inf))
                for (pb, pe, pm) in parts:
                    for r in range(R):
                        if np.isfinite(pm[r, 0]):
                            e = np.exp(Sm[r, pb:pe] - pm[r, 0]) * mult[pb:pe]
                            w = 1.0 if mutant == "combine_ignores_maxima" else math.exp(pm[r, 0] - mstar[r, 0])
                            num[r] += w * vsc * (e @ V[pb:pe])
                            den[r, 0] += w * e.sum()
                        elif mutant == "combine_counts_empty":
                            den[r, 0] += STEP * math.exp(0.0 - mstar[r, 0])
                seen = den[:, 0] > 0
                den0 = np.where(den > 0, den, 1.0)
                O[b, h] = np.where(seen[:, None], num / den0, 0.0)
                L[b, h] = np.where(seen, mstar[:, 0] + np.log(den0[:, 0]), -np.inf)
                continue
            l = pw.sum(axis=1, keepdims=True)
            l0 = np.where(l > 0, l, 1.0)
            P = pw / l0
            O[b, h] = (P @ V) * vsc
            L[b, h] = np.where(seen, m0[:, 0] + np.log(l0[:, 0]), -np.inf)
            if mutant is None:
                absV = np.abs(V) * abs(vsc)
                A[b, h] = P @ absV
                e2 = (D + 3) * U32 * (LOG2E * abs(ksc) / math.sqrt(D)) * (np.abs(qh) @ np.abs(K).T)
                smin = np.where(vis, S, np.inf).min(axis=1, keepdims=True)
                spread2 = np.where(seen[:, None], (m0 - np.where(np.isfinite(smin), smin, m0)) * LOG2E, 0.0)
                rel = LN2 * (e2 + 3 * U32 * spread2) + 4 * U32
                relp = (rel * P).sum(axis=1)
                E[b, h] = (rel * P) @ absV + np.abs(O[b, h]) * relp[:, None] + chain * (A[b, h] + np.abs(O[b, h]))
                Lf = np.where(seen, L[b, h], 0.0)
                EL[b, h] = relp + chain + 4 * U32 * (np.abs(m0[:, 0]) + np.abs(np.log(l0[:, 0])) + np.abs(Lf))
    if mutant == "o_zero":
        O[:] = 0.0
    if mutant == "rows_swapped":
        O, L = O[:, :, ::-1].copy(), L[:, :, ::-1].copy()
    if mutant == "v_dblocks_exchanged":
        O = np.concatenate([O[..., 32:64], O[..., :32], O[..., 64:]], axis=-1)
    return Reference(O, L, A, E, EL)


def bounds(ref, fmt, out, margin=MARGIN):
    """(bound on |O - ref.O| per element, bound on |L - ref.L| per row, natural units): see the module's docstring"""
    bo = margin * (U_P[fmt] * ref.A + U_OUT[out] * np.abs(ref.O) + ref.E) + TINY
    bl = margin * ref.EL + TINY
    return bo, bl


# ------------------------------------------------------------------------------------------------- the rounding-emulated reference
def emulated(q, k, v, lens, G, causal, fmt, *, pieces=None, kscale=None, vscale=None, piece_range=None):
    """the model with the kernel's roundings of P and its order of sums -> (O before the store's rounding [B, Hq, R, D], L natural);
    store(O, out) is what a launch with that output type may write"""
    q, k, v = f64(q), f64(k), f64(v)
    B, Hq, R, D = q.shape
    Hkv = Hq // G
    ks = np.ones(Hkv) if kscale is None else np.asarray(kscale, dtype=np.float64)
    vs = np.ones(Hkv) if vscale is None else np.asarray(vscale, dtype=np.float64)
    O = np.zeros((B, Hq, R, D))
    L = np.full((B, Hq, R), -np.inf)
    rows = np.arange(R)[:, None]
    NEG = -np.inf

    def merge(parts):
        """[(m [R], l [R], o [R, D])] -> the online-softmax merge in the given order"""
        mstar = np.full(R, NEG)
        for m, _l, _o in parts:
            mstar = np.maximum(mstar, m)
        lt, ot = np.zeros(R), np.zeros((R, D))
        for m, l, o in parts:
            w = np.where(np.isfinite(m), np.exp2(np.where(np.isfinite(m), m - np.where(np.isfinite(mstar), mstar, 0.0), 0.0)), 0.0)
            lt += w * l
            ot += w[:, None] * o
        return mstar, lt, ot

    for b in range(B):
        n = int(lens[b])
        if n == 0:
            continue
        ranges = piece_ranges(n, pieces, piece_range)
        cols = np.arange(n)[None, :]
        for h in range(Hq):
            j = h // G
            K, V = k[b, j, :n], v[b, j, :n]
            S2 = (q[b, h] @ K.T) * (ks[j] * LOG2E / math.sqrt(D))
            vis = np.broadcast_to(cols < n, S2.shape)
            if causal:
                vis = vis & (cols <= rows + max(n - R, 0))
            S2 = np.where(vis, S2, NEG)
            published = []
            for (pb, pe) in ranges:
                state = [(np.full(R, NEG), np.zeros(R), np.zeros((R, D))) for _ in range(WAVES)]
                for t, key0 in enumerate(range(pb, pe, STEP)):
                    m, l, o = state[t % WAVES]
                    s = S2[:, key0:min(key0 + STEP, pe)]
                    new = np.maximum(m, s.max(axis=1))
                    fin = np.isfinite(new)
                    ref = np.where(fin, new, 0.0)
                    corr = np.where(np.isfinite(m), np.exp2(np.where(np.isfinite(m), m, 0.0) - ref), 1.0)
                    p = np.where(fin[:, None], np.exp2(s - ref[:, None]), 0.0)
                    state[t % WAVES] = (new, l * corr + p.sum(axis=1), o * corr[:, None] + round_to(p, fmt) @ V[key0:min(key0 + STEP, pe)])
                published.append(merge(state))
            mstar, lt, ot = merge(published) if len(published) > 1 else published[0]
            seen = lt > 0
            l0 = np.where(seen, lt, 1.0)
            O[b, h] = np.where(seen[:, None], ot * vs[j] / l0[:, None], 0.0)
            L[b, h] = np.where(seen, (np.where(seen, mstar, 0.0) + np.log2(l0)) / LOG2E, -np.inf)
    return O, L


# ------------------------------------------------------------------------------------------------------------------ needle inputs
def needle_pool(n, ranges, page):
    """the keys of a sequence whose handling the launch's geometry makes special (every row also gets its own causal frontier)"""
    if n <= 0:
        return []
    last = (n - 1) // STEP * STEP
    pool = [0, 31, 32, last, last - 1]
    filled = [(pb, pe) for pb, pe in ranges if pe > pb]
    for (pb, pe) in filled:
        if (pb, pe) in (filled[0], filled[-1]):   # one key in a step of every wave: the first four steps and four in the middle
            steps = -(-(pe - pb) // STEP)
            for t in list(range(min(WAVES, steps))) + [steps // 2 + w for w in range(WAVES) if steps > 2 * WAVES]:
                pool.append(pb + t * STEP + 5 + (t % WAVES))
        if len(ranges) > 1:
            pool += [pb, pe - 1]                 # the first and the last key of every piece
    if page:
        pool += [page - 1, page, (n - 1) // page * page, (n - 1) // page * page - 1, n - 1]
    return sorted({t for t in pool if 0 <= t < n})


def needle_queries(k, lens, Hq, G, R, causal, fmt, *, pieces=None, page=None, piece_range=None, seed=0):
    """q [B, Hq, R, D] (float64 values of the 16-bit type) and, per (b, h, r), its needles {key: weight in natural units} and its
    forbidden key (or None).  k [B, Hkv, C, D]: the cache's values as the model sees them (dequantised, scale included).

    Row (h, r): q = beta sqrt(D) sum_t w_t k_t / |k_t|^2 with beta = ln n + 1 - ln |T|, so that key t scores about beta w_t and the
    needles hold a share of the softmax mass of the order of the bulk's.  T = the row's own frontier and the key before it, plus its
    share of needle_pool(): the rows of the launch take the pool's keys in turn (row index h R + r), so that rows and heads of one
    packed group differ and every pool key is some row's needle.  Scores differ by up to +-2 with the key's wave and piece (rotated
    by the packed index), so waves and pieces end with different maxima.  Causal, r < R - 1: the key after the frontier -- visible to
    the next row only -- is added with weight beta + 4: a row that reads one key too far is taken over by it.  Non-causal launches
    have no forbidden key: every key below the length is visible to every row."""
    k = f64(k)
    B, Hkv, C, D = k.shape
    q = np.zeros((B, Hq, R, D))
    info = {}
    rng = np.random.default_rng(seed)
    for b in range(B):
        n = int(lens[b])
        if n == 0:
            q[b] = round_to(rng.uniform(-1, 1, (Hq, R, D)), fmt)
            continue
        ranges = piece_ranges(n, pieces, piece_range)
        pool = needle_pool(n, ranges, page)
        starts = np.array([pb for pb, pe in ranges])
        per_row = 6
        stride = max(2 if len(pool) > 1 else 1, -(-len(pool) // per_row))
        stride = max(1, min(stride, Hq * R))
        for h in range(Hq):
            j = h // G
            for r in range(R):
                rho, p = h * R + r, (h % G) * R + r
                fr = min(r + max(n - R, 0), n - 1) if causal else n - 1
                T = {t for i, t in enumerate(pool) if i % stride == rho % stride and t <= fr}
                T |= {fr} | ({fr - 1} if fr >= 1 else set())
                beta = math.log(n) + 1.0 - math.log(len(T))
                weights = {}
                for t in sorted(T):
                    piece = int(np.searchsorted(starts, t, side="right") - 1)
                    wave = ((t - ranges[piece][0]) // STEP) % WAVES
                    weights[t] = beta + (((wave + p) % WAVES) - 1.5) * (2.0 / 3.0) + (((piece + p) % 3) - 1.0)
                forbidden = None
                if causal and r < R - 1 and r + max(n - R, 0) + 1 < n:
                    forbidden = r + max(n - R, 0) + 1
                vec = np.zeros(D)
                for t, w in list(weights.items()) + ([(forbidden, beta + 4.0)] if forbidden is not None else []):
                    kt = k[b, j, t]
                    vec += w * math.sqrt(D) * kt / max(float(kt @ kt), 1e-30)
                q[b, h, r] = vec
                info[(b, h, r)] = (weights, forbidden)
        q[b] = round_to(q[b], fmt)
    return q, info


def needle_keys(info):
    """{batch: every key that is some row's needle}"""
    out = {}
    for (b, _h, _r), (weights, _f) in info.items():
        out.setdefault(b, set()).update(weights)
    return out


def spread_scales(rng, count):
    """per-head scales in [0.5, 2], pairwise at least 1.25 x apart, in random order.  The interval holds seven such values
    (0.5 x 1.25^6 = 1.91); from the eighth head on a value returns, three heads away from its first use, so that heads j and j + 1
    never share one"""
    ladder = 0.5 * 1.25 ** np.arange(7)
    perm = rng.permutation(7)
    return np.array([ladder[perm[i % 7 if i < 7 else (i + 3) % 7]] for i in range(count)], dtype=np.float32)


# ----------------------------------------------------------------------------------------------------------------------- checker
def compare(got_o, got_l, ref, fmt, out, lens, *, margin=MARGIN, info=None, pieces=None, page=None, piece_range=None):
    """-> (worst |dO| / bound, worst |dL| / bound, text naming the worst elements).  got_l: natural units, or None.  Rows without a
    visible key are the caller's to check (O = 0, L hugely negative)."""
    go = f64(got_o)
    bo, bl = bounds(ref, fmt, out, margin)
    ratio = np.abs(go - ref.O) / bo
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    worst_o = float(ratio[at])
    b, h, r, d = (int(x) for x in at)
    text = "O worst at batch %d head %d row %d d %d (length %d): got %.6g, model %.6g, |d| / bound = %.3g" % (
        b, h, r, d, int(lens[b]), go[at], ref.O[at], worst_o)
    if info is not None and (b, h, r) in info:
        weights, forbidden = info[(b, h, r)]
        n = int(lens[b])
        ranges = piece_ranges(n, pieces, piece_range)
        where = []
        for t in sorted(weights):
            piece = max(i for i, (pb, pe) in enumerate(ranges) if pb <= t) if len(ranges) > 1 else 0
            where.append("%d (piece %d%s)" % (t, piece, ", page %d" % (t // page) if page else ""))
        text += "; the row's needles: keys " + ", ".join(where) + ("; forbidden key %d" % forbidden if forbidden is not None else "")
        text += "; a needle row" if weights else "; a bulk row"
    worst_l = 0.0
    if got_l is not None:
        gl = f64(got_l)
        keep = np.isfinite(ref.L)
        if keep.any():
            rl = np.where(keep, np.abs(gl - np.where(keep, ref.L, 0.0)) / bl, 0.0)
            rl = np.where(np.isnan(rl), np.inf, rl)
            at = np.unravel_index(int(np.argmax(rl)), rl.shape)
            worst_l = float(rl[at])
            text += "; L worst at batch %d head %d row %d: got %.8g, model %.8g, |d| / bound = %.3g" % (
                int(at[0]), int(at[1]), int(at[2]), gl[at], ref.L[at], worst_l)
    return worst_o, worst_l, text
