"""The float64 model of multi-head latent attention PREFILL over the compressed cache (include/mfa_mla_prefill.h), its per-element error
bounds, the needle inputs, the named mutants and the cases the CPU and GPU files share (a plain module after tests/mla_model.py, from
which it takes the widths, the scale, the bound's terms and chain_length; numpy only, the library is never called).

  step_range()     the kernels' range function (mla_prefill_step_range, csrc/attn_mla16_prefill.h) in Python: the 32-key steps of the
                   block of 64 packed rows from p0, p = row x H + head.  tests/test_mla_prefill_plans.py holds the library's to the mask.
  model()          float64 attention with the CALLER's scale and a per-sequence qn: row r < qn of sequence b sees key c iff c < n and,
                   causal, c <= r + max(n - qn, 0).  -> (Reference(O, L, A, E, EL), written [B, H, R]): rows at or past qn are not
                   written and hold O = 0, L = -inf, bounds 0.  mutant= computes a named WRONG attention instead (MUTANTS).
  emulated()       the same attention with the kernel's roundings and order of sums: every block walks its steps to the block's end with
                   ONE running (m, l, O) per row, P rounded to the 16-bit type against that maximum.  A step past a row's own frontier
                   is fully masked for it and changes nothing, so a row's result does not depend on its block: mla_model.emulated()'s
                   arithmetic, expression for expression, which is what makes the decode identity and the chunk invariance BIT-exact.
  needle_queries() query rows in which single keys matter: the row's frontier and the key before it, its share of the seam keys, and
                   -- causal -- the key after the frontier with the largest weight of all, which the row must not see.
  CASES, inputs()  the launches of tests/test_mla_prefill_gpu.py, which tests/test_mla_prefill_sensitivity.py walks on the CPU.

The bound is mla_model's, term for term, with the chain of the BLOCK: the accumulator of an output element walks every step of its
block's walk, end = step_range()[1], so chain = mla_model.chain_length(32 x end, 1) = 34 end + 14 roundings on sums of magnitude A and 1.
MARGIN is fixed by tests/test_mla_prefill_sensitivity.py alone, before any GPU run: the smallest power of two with at least 2 x headroom
over emulated()'s worst err / bound at margin 1 over every case (0.807, on the seam batch with five heads: MARGIN = 2).

Batches.  A: (n, qn) = (700, 100), (200, 200), (100, 33), (5, 5), (0, 0), (1500, 65), (40, 64) -- the last has qn > n -- in a cache of
1536 keys, rows' capacity 200.  B (seams): qn in {1, 32, 33, 64, 65, 128, 130} against n in {qn, 96, 256, 320, 400} in a cache of 320 keys
(400 is handed to the launch and clamped), capacity 130.  H = 64 and H = 128 run on two sequences of a batch (A2, B2); N is a batch
whose launch passes queryLengths = NULL.
"""
import functools
import math

import numpy as np

import decode_model as dm
import mla_model as mm
from decode_model import LN2, LOG2E, U32, Reference, bounds, round_to, store, U_P, U_OUT  # noqa: F401
from mla_model import DK, DV, SCALE, SLICE, STEP  # noqa: F401

BLOCK, TILE_ROWS = 64, 32           # packed rows of a workgroup, and of one of its two tiles (attn_mla16_prefill.h)
MARGIN = 2


def step_range(n, qn, p0, H, causal):
    """(firstMasked, end) in 32-key steps of the block of the 64 packed rows from p0"""
    r0 = p0 // H
    if r0 >= qn or n == 0:
        return 0, 0
    lo = hi = n
    if causal:
        off = max(n - qn, 0)
        last = min((p0 + BLOCK - 1) // H, qn - 1)
        lo, hi = min(r0 + off + 1, n), min(last + off + 1, n)
    e = -(-hi // STEP)
    return min(lo // STEP, e), e


def chain_length(n, qn, p0, H, causal):
    """mla_model.chain_length with the steps of the BLOCK's walk and pieces = 1"""
    return mm.chain_length(STEP * step_range(n, qn, p0, H, causal)[1], 1)


def _blocks(qn, H):
    return range(0, qn * H, BLOCK)


# ---------------------------------------------------------------------------------------------------------------------- mutants
# name -> (what the defect is, where it changes nothing).  `c` has n (the clamped length), raw (as the launch is handed it), C, qn, R (the
# rows' capacity), H, B, causal, page and qn_next (the neighbouring sequence's qn).
def _second_tile_live(c):
    return c["H"] * c["qn"] > TILE_ROWS


def _no_masked_step(c):
    return all(f == e for f, e in (step_range(c["n"], c["qn"], p0, c["H"], c["causal"]) for p0 in _blocks(c["qn"], c["H"])))


MUTANTS = {
    # ---- prefill's own
    "head_major_packing": ("packed row p unpacked head-major, head p / R and row p % R", lambda c: c["H"] == 1),
    "head_div_h": ("head p / H in place of p % H", lambda c: c["H"] == 1),
    "frontier_from_rows": ("the causal frontier from the rows' capacity instead of qn", lambda c: not c["causal"] or c["qn"] == c["R"] or c["n"] <= c["qn"]),
    "max_dropped": ("max(n - qn, 0) replaced by n - qn", lambda c: not c["causal"] or c["n"] >= c["qn"]),
    "block_end_from_first_row": ("the block's end taken from its FIRST row: later rows lose the keys of the steps behind it",
                                 lambda c: not c["causal"] or c["H"] % BLOCK == 0 or c["qn"] == 1),
    "second_tile_rows_of_first": ("the second 32-row tile computed with the rows of the first (p - 32)", lambda c: not _second_tile_live(c)),
    "second_tile_mask_of_first": ("the second tile's mask taken from the first tile's rows",
                                  lambda c: not c["causal"] or c["H"] % BLOCK == 0 or not _second_tile_live(c)),
    "unmasked_one_step_too_far": ("the step firstMasked run without the per-element mask", _no_masked_step),
    "qn_of_neighbour": ("queryLengths of the neighbouring sequence", lambda c: c["B"] == 1 or c["qn_next"] == c["qn"]),
    "rows_past_qn_written": ("rows at or past qn computed and written", lambda c: c["qn"] == c["R"]),
    # ---- mla_model's that still apply, with the sequence's own row count
    "len_minus_2": ("c < len replaced by c <= len - 2", lambda c: False),
    "causal_plus_1": ("causal frontier one key too far", lambda c: not c["causal"] or c["qn"] == 1 or c["n"] < 2),
    "causal_minus_1": ("causal frontier one key short", lambda c: not c["causal"]),
    "length_not_clamped": ("cacheLengths[b] not clamped to column: the keys column .. n - 1 are walked, in a packed cache the first rows "
                           "of sequence b + 1", lambda c: c["raw"] <= c["C"]),
    "page_table_neighbour": ("the block-table row of the next sequence", lambda c: not c["page"] or c["B"] == 1),
    "page_off_by_one": ("the first 16-key group of a page read from the page before", lambda c: not c["page"] or c["n"] <= c["page"]),
    "page_boundary_key_from_next_page": ("a key on the last slot of a page read from slot 0 of the page after it",
                                         lambda c: not c["page"] or c["n"] <= c["page"]),
    "v_from_tail": ("V taken from the columns 64 .. 575", lambda c: False),
    "rope_left_out": ("the rotary columns 512 .. 575 left out of the score", lambda c: False),
    "scale_sqrt_dk": ("scale 1 / sqrt(576) in place of the caller's", lambda c: False),
    "o_blocks_exchanged": ("the first two 128-column blocks of O exchanged", lambda c: False),
    "wave_partial_dropped": ("one wave's partial score left out of the sum of the step before the sequence's last", lambda c: c["n"] <= STEP),
    "final_partial_step_dropped": ("the partial last step is not run", lambda c: c["n"] % STEP == 0),
    "full_last_step_dropped": ("the last step is not run when it is full", lambda c: c["n"] % STEP != 0),
}
# A defect that costs steps and no bit: the block's end taken from row (p0 + 63) / H WITHOUT the clamp to qn - 1.  The steps it adds lie
# behind every live row's frontier -- fully masked: p = 0, the maximum untouched, +0 added -- and their keys lie below n, so the model of
# it IS the model (tests/test_mla_prefill_sensitivity.py asserts that), and no bound can see it.  What sees it is the range function's
# own test: `end` is minimal (tests/test_mla_prefill_plans.py).
BITLESS_MUTANTS = {"block_end_unclamped": "the block's end taken from row (p0 + 63) / H unclamped to qn - 1"}


def facts_of(case, b):
    """what a mutant's `harmless` rule is asked about: the case's launch and ONE sequence"""
    lens, qlens = case["lens"], seen_qlens(case)
    return dict(R=case["R"], H=case["H"], B=len(lens), causal=case["causal"], page=case["page"], C=case["C"], raw=lens[b],
                n=min(lens[b], case["C"]), qn=qlens[b], qn_next=qlens[(b + 1) % len(lens)])


def _source(mutant, r, h, H, R):
    """(head, row) whose q -- and whose frontier -- a (mutated) kernel computes packed row p = r H + h with"""
    p = r * H + h
    if mutant == "head_major_packing":
        return p // R, p % R
    if mutant == "head_div_h":
        return (p // H) % H, p // H
    if mutant == "second_tile_rows_of_first" and p % BLOCK >= TILE_ROWS:
        return (p - TILE_ROWS) % H, (p - TILE_ROWS) // H
    return h, r


def model(q, kv, lens, qlens, causal, scale, mutant=None, *, page=None, shared=False):
    """float64 attention -> (Reference(O, L, A, E, EL), written).  q [B, H, R, 576] (R: the rows' capacity), kv [B, C, 576] (shared:
    sequence b reads kv[0], a launch with batchStride 0), qlens None: every sequence has R rows.  A length past the cache's C rows is
    clamped to C, a row count past R to R."""
    assert mutant is None or mutant in MUTANTS or mutant in BITLESS_MUTANTS, mutant
    q, kv = dm.f64(q), dm.f64(kv)
    B, H, R, _ = q.shape
    O, A, E = (np.zeros((B, H, R, DV)) for _ in range(3))
    L = np.full((B, H, R), -np.inf)
    EL = np.zeros((B, H, R))
    written = np.zeros((B, H, R), dtype=bool)
    sc = 1.0 / math.sqrt(DK) if mutant == "scale_sqrt_dk" else float(scale)
    qls = [R if qlens is None else min(int(x), R) for x in (lens if qlens is None else qlens)]
    for b in range(B):
        n = min(int(lens[b]), kv.shape[1])
        if mutant == "length_not_clamped":
            n = int(lens[b])
        qn = qls[b]
        live = qn                                          # the rows the launch computes and writes
        if mutant == "qn_of_neighbour":
            qn = live = qls[(b + 1) % B]
        if mutant == "rows_past_qn_written":
            live = R
        written[b, :, :live] = True
        if n == 0 or live == 0:
            continue
        cols = np.arange(n)[None, :]
        src_b = 0 if shared else b
        if mutant == "page_table_neighbour" and page:
            src_b = (b + 1) % B
        K = kv[src_b, :n]
        if n > kv.shape[1]:                     # (length_not_clamped alone: the rows behind the cache's last are the next sequence's)
            K = np.concatenate([kv[src_b], kv[(src_b + 1) % B]])[:n]
        if mutant == "page_off_by_one" and page:
            src = np.arange(n)
            K = kv[src_b][np.where((src >= page) & (src % page < 16), src - page, src)]
        if mutant == "page_boundary_key_from_next_page" and page:
            src = np.arange(n)
            K = kv[src_b][np.where((src % page == page - 1) & (src + 1 < n), src + 1, src)]
        V = K[:, 64:DK] if mutant == "v_from_tail" else K[:, :DV]
        Ks = K[:, :DV] if mutant == "rope_left_out" else K
        absV = np.abs(V)
        rows = np.arange(live)
        for h in range(H):
            picked = [_source(mutant, r, h, H, R) for r in rows]
            qh = np.stack([q[b, hh % H, min(rr, R - 1)] for hh, rr in picked])
            frow = np.array([rr for _hh, rr in picked])[:, None]      # the row the frontier is taken from
            if mutant == "second_tile_mask_of_first":
                p = rows * H + h
                frow = np.where(p % BLOCK >= TILE_ROWS, (p - TILE_ROWS) // H, rows)[:, None]
            qs = qh[:, :DV] if mutant == "rope_left_out" else qh
            raw = qs @ Ks.T
            if mutant == "wave_partial_dropped" and n > STEP:
                t = (n - 1) // STEP - 1
                lost = np.r_[2 * SLICE:3 * SLICE, DV + 32:DV + 48]   # wave 2's columns
                raw[:, t * STEP:(t + 1) * STEP] -= qh[:, lost] @ K[t * STEP:(t + 1) * STEP][:, lost].T
            S = raw * sc
            limit = n - 1 if mutant == "len_minus_2" else n
            vis = np.broadcast_to(cols < limit, S.shape).copy()
            base = n - R if mutant == "frontier_from_rows" else n - qn
            base = base if mutant == "max_dropped" else max(base, 0)
            if causal:
                shift = 1 if mutant == "causal_plus_1" else -1 if mutant == "causal_minus_1" else 0
                vis &= cols <= frow + base + shift
            if mutant == "final_partial_step_dropped" and n % STEP:
                vis[:, n // STEP * STEP:] = False
            if mutant == "full_last_step_dropped" and n % STEP == 0:
                vis[:, n - STEP:] = False
            if mutant in ("block_end_from_first_row", "unmasked_one_step_too_far"):
                for p0 in _blocks(live, H):
                    mine = ((rows * H + h) // BLOCK == p0 // BLOCK)
                    f, e = step_range(min(n, kv.shape[1]), qn, p0, H, causal)
                    if mutant == "block_end_from_first_row":
                        first_end = -(-min(p0 // H + base + 1, n) // STEP) if causal else e
                        vis[mine, first_end * STEP:] = False
                    elif f < e:   # every key of step f counts for every row; a key at or past n comes in as zeros: score 0, value 0
                        hi = min((f + 1) * STEP, n)
                        vis[mine, f * STEP:hi] = True
            Sm = np.where(vis, S, -np.inf)
            m = Sm.max(axis=1, keepdims=True)
            extra = np.zeros(live)                          # softmax mass of the zero keys past n that an unmasked step lets in
            if mutant == "unmasked_one_step_too_far":
                for p0 in _blocks(live, H):
                    f, e = step_range(n, qn, p0, H, causal)
                    if f < e and (f + 1) * STEP > n:
                        extra[(rows * H + h) // BLOCK == p0 // BLOCK] = (f + 1) * STEP - n
                m = np.where((extra > 0)[:, None], np.maximum(m, 0.0), m)
            seen = np.isfinite(m[:, 0])
            m0 = np.where(np.isfinite(m), m, 0.0)
            pw = np.exp(Sm - m0)
            l = pw.sum(axis=1, keepdims=True) + (extra * np.exp(0.0 - m0[:, 0]))[:, None]
            l0 = np.where(l > 0, l, 1.0)
            P = pw / l0
            O[b, h, :live] = P @ V
            L[b, h, :live] = np.where(seen, m0[:, 0] + np.log(l0[:, 0]), -np.inf)
            if mutant is None:
                Ob = O[b, h, :live]
                A[b, h, :live] = P @ absV
                chain = np.array([chain_length(n, qn, (r * H + h) // BLOCK * BLOCK, H, causal) for r in rows]) * U32
                e2 = (DK + 3) * U32 * (LOG2E * sc) * (np.abs(qh) @ np.abs(K).T)
                smin = np.where(vis, S, np.inf).min(axis=1, keepdims=True)
                spread2 = np.where(seen[:, None], (m0 - np.where(np.isfinite(smin), smin, m0)) * LOG2E, 0.0)
                rel = LN2 * (e2 + 3 * U32 * spread2) + 4 * U32
                relp = (rel * P).sum(axis=1)
                E[b, h, :live] = (rel * P) @ absV + np.abs(Ob) * relp[:, None] + chain[:, None] * (A[b, h, :live] + np.abs(Ob))
                Lf = np.where(seen, L[b, h, :live], 0.0)
                EL[b, h, :live] = relp + chain + 4 * U32 * (np.abs(m0[:, 0]) + np.abs(np.log(l0[:, 0])) + np.abs(Lf))
    if mutant == "o_blocks_exchanged":
        O = np.concatenate([O[..., SLICE:2 * SLICE], O[..., :SLICE], O[..., 2 * SLICE:]], axis=-1)
    return Reference(O, L, A, E, EL), written


# ------------------------------------------------------------------------------------------------- the rounding-emulated reference
def emulated(q, kv, lens, qlens, causal, scale, fmt, *, shared=False, ordered=False):
    """the model with the kernel's roundings and its order of sums -> (O before the store's rounding [B, H, R, 512], L natural; rows at or
    past qn hold 0 and -inf).  Every row walks the 32-key steps from 0 to the end of ITS block's walk (step_range) with one running
    (m, l, O), in mla_model.emulated()'s expressions.  ordered: both products are summed element by element in an order that does not
    depend on how many rows or keys the call holds (numpy's matrix product is free to block a sum by the operands' shapes), which is what
    a bit-for-bit comparison of two DIFFERENT launches of the same rows needs; slower, for small cases."""
    q, kv = dm.f64(q), dm.f64(kv)
    B, H, R, _ = q.shape
    O = np.zeros((B, H, R, DV))
    L = np.full((B, H, R), -np.inf)
    NEG = -np.inf
    scale2 = float(np.float32(np.float32(scale) * np.float32(1.44269504089)))
    for b in range(B):
        n = min(int(lens[b]), kv.shape[1])
        qn = R if qlens is None else min(int(qlens[b]), R)
        if n == 0 or qn == 0:
            continue
        rows = np.arange(qn)[:, None]
        cols = np.arange(n)[None, :]
        K = kv[0 if shared else b, :n]
        V = K[:, :DV]
        for h in range(H):
            if ordered:
                S2 = np.stack([(q[b, h, :qn] * K[c][None, :]).sum(axis=1) for c in range(n)], axis=1) * scale2
            else:
                S2 = (q[b, h, :qn] @ K.T) * scale2
            vis = np.broadcast_to(cols < n, S2.shape)
            if causal:
                vis = vis & (cols <= rows + max(n - qn, 0))
            S2 = np.where(vis, S2, NEG)
            ends = np.array([step_range(n, qn, (r * H + h) // BLOCK * BLOCK, H, causal)[1] for r in range(qn)])
            m, l, o = np.full(qn, NEG), np.zeros(qn), np.zeros((qn, DV))
            for key0 in range(0, int(ends.max()) * STEP, STEP):
                walks = ends * STEP > key0                                # the rows whose block walks this step
                s = np.where(walks[:, None], S2[:, key0:min(key0 + STEP, n)], NEG)
                Vs = V[key0:min(key0 + STEP, n)]
                if ordered and s.shape[1] < STEP:                         # a partial last step as the kernel holds it: 32 keys, the
                    short = STEP - s.shape[1]                             # missing ones masked and their values zero
                    s, Vs = np.pad(s, ((0, 0), (0, short)), constant_values=NEG), np.pad(Vs, ((0, short), (0, 0)))
                new = np.maximum(m, s.max(axis=1))
                fin = np.isfinite(new)
                ref = np.where(fin, new, 0.0)
                corr = np.where(np.isfinite(m), np.exp2(np.where(np.isfinite(m), m, 0.0) - ref), 1.0)
                p = np.where(fin[:, None], np.exp2(s - ref[:, None]), 0.0)
                pv = (round_to(p, fmt)[:, :, None] * Vs[None, :, :]).sum(axis=1) if ordered else round_to(p, fmt) @ Vs
                m, l, o = new, l * corr + p.sum(axis=1), o * corr[:, None] + pv
            seen = l > 0
            l0 = np.where(seen, l, 1.0)
            O[b, h, :qn] = np.where(seen[:, None], o / l0[:, None], 0.0)
            L[b, h, :qn] = np.where(seen, (np.where(seen, m, 0.0) + np.log2(l0)) / LOG2E, -np.inf)
    return O, L


# ------------------------------------------------------------------------------------------------------------------ needle inputs
def needle_queries(kv, lens, qlens, H, R, causal, fmt, scale, *, page=None, shared=False, seed=0):
    """q [B, H, R, 576] (float64 values of the 16-bit type) and, per (b, h, r < qn), its needles {key: weight in natural units} and its
    forbidden key (or None): decode_model.needle_queries' construction with the sequence's own row count.  Row (h, r): q = (1 / scale)
    sum_t w_t k_t / |k_t|^2 with w_t near beta = ln n + 1 - ln |T|, so that key t scores about w_t.  T = the row's own frontier and the
    key before it, plus its share of the seam keys (decode_model.needle_pool: the first and last steps, the page seams) and of the ends
    of the 32-key steps around the row's block's walk.  Causal, with a key behind the frontier: that key -- visible to the next row only
    -- is added with weight beta + 4: a row that reads one key too far is taken over by it.  Rows at or past qn hold plain values (a
    launch puts NaN there)."""
    kv = dm.f64(kv)
    B = len(lens)
    rng = np.random.default_rng(seed)
    q = round_to(rng.uniform(-1, 1, (B, H, R, DK)), fmt)
    info = {}
    for b in range(B):
        n = min(int(lens[b]), kv.shape[1])
        qn = R if qlens is None else min(int(qlens[b]), R)
        if n == 0:
            continue
        K = kv[0 if shared else b]
        pool = dm.needle_pool(n, [(0, n)], page)
        stride = max(1, min(max(2 if len(pool) > 1 else 1, -(-len(pool) // 6)), H * max(qn, 1)))
        off = max(n - qn, 0)
        for r in range(qn):
            for h in range(H):
                p = r * H + h
                fr = min(r + off, n - 1) if causal else n - 1
                f, e = step_range(n, qn, p // BLOCK * BLOCK, H, causal)
                T = {t for i, t in enumerate(pool) if i % stride == p % stride and t <= fr}
                T |= {t for t in (f * STEP - 1, f * STEP, e * STEP - 1) if 0 <= t <= fr and (t + p) % 3 == 0}
                T |= {fr} | ({fr - 1} if fr >= 1 else set())
                beta = math.log(n) + 1.0 - math.log(len(T))
                weights = {t: beta + ((((t // STEP) + p) % 4) - 1.5) * (2.0 / 3.0) for t in sorted(T)}
                forbidden = fr + 1 if causal and fr + 1 < n else None
                vec = np.zeros(DK)
                for t, w in list(weights.items()) + ([(forbidden, beta + 4.0)] if forbidden is not None else []):
                    vec += w * K[t] / max(float(K[t] @ K[t]), 1e-30)
                q[b, h, r] = round_to(vec / scale, fmt)
                info[(b, h, r)] = (weights, forbidden)
    return q, info


# ---------------------------------------------------------------------------------------------------------------------- the cases
BATCH_A = (((700, 100), (200, 200), (100, 33), (5, 5), (0, 0), (1500, 65), (40, 64)), 1536, 200)
BATCH_A2 = (((1500, 65), (40, 64)), 1536, 200)                          # two of them, for the head counts whose q is large
BATCH_B = (tuple((n or qn, qn) for qn in (1, 32, 33, 64, 65, 128, 130) for n in (0, 96, 256, 320, 400)), 320, 130)   # (0: n = qn)
BATCH_B2 = (((320, 130), (96, 65)), 320, 130)
BATCH_N = (((320, 70), (70, 70), (33, 70), (0, 70), (400, 70), (256, 70)), 320, 70)   # queryLengths NULL: every sequence has 70 rows
BATCHES = {"A": BATCH_A, "A2": BATCH_A2, "B": BATCH_B, "B2": BATCH_B2, "N": BATCH_N}


# name -> the launch: fmt, H, causal, page, layout ("packed"; "ld640": cache rows 640 elements apart in a larger allocation; "shared":
# batchStride 0, every sequence reads sequence 0's cache), token_major (Q and O [B, R, H, ..] seen through strides), out, and its batch:
# lens as the launch is handed them, qlens (None: queryLengths NULL), C keys, R rows of capacity
def _case(fmt, H, batch, causal=True, page=None, layout="packed", out=None, token_major=False):
    seqs, C, R = BATCHES[batch]
    null = batch == "N"
    return dict(fmt=fmt, H=H, causal=causal, page=page, layout=layout, out=out or fmt, token_major=token_major, batch=batch,
                lens=tuple(s[0] for s in seqs), qlens=None if null else tuple(s[1] for s in seqs), C=C, R=R)


CASES = {
    "a1 sixteen heads": _case("bf16", 16, "A"),
    "a2 five heads, a seam inside a row": _case("f16", 5, "A"),
    "a3 one head, fp32 out": _case("bf16", 1, "A", out="f32"),
    "a4 a block is one row": _case("bf16", 64, "A2"),
    "a5 a block is half a row": _case("f16", 128, "A2"),
    "a6 not causal": _case("bf16", 16, "A", causal=False),
    "a7 pages of 64": _case("f16", 16, "A", page=64),
    "a8 one cache shared": _case("bf16", 5, "A", layout="shared"),
    "a9 rows 640 apart, token-major Q and O": _case("bf16", 16, "A", layout="ld640", token_major=True),
    "b1 five heads": _case("bf16", 5, "B"),
    "b2 pages of 16": _case("f16", 16, "B", page=16),
    "b3 pages of 512, not causal": _case("bf16", 16, "B", causal=False, page=512),
    "b4 one head, token-major, fp32 out": _case("f16", 1, "B", out="f32", token_major=True),
    "b5 a block is one row": _case("f16", 64, "B2"),
    "b6 a block is half a row, pages of 64": _case("bf16", 128, "B2", page=64),
    "n1 queryLengths NULL": _case("bf16", 16, "N"),
    "n2 queryLengths NULL, five heads, not causal": _case("f16", 5, "N", causal=False),
}


def seen_lens(case):
    """the lengths the launch of a case reads: the case's, clamped to its column"""
    return tuple(min(n, case["C"]) for n in case["lens"])


def seen_qlens(case):
    """the row counts the launch of a case reads: the case's (None: the capacity), clamped to the capacity"""
    return tuple(case["R"] if case["qlens"] is None else min(x, case["R"]) for x in (case["lens"] if case["qlens"] is None else case["qlens"]))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(case, q, kv, Reference, written, needle info) of a case, computed once and shared"""
    case = CASES[name]
    lens = case["lens"]
    kv = mm.cache_values(case["fmt"], 0, len(lens), case["C"])
    shared = case["layout"] == "shared"
    q, info = needle_queries(kv, lens, case["qlens"], case["H"], case["R"], case["causal"], case["fmt"], SCALE, page=case["page"], shared=shared)
    ref, written = model(q, kv, lens, case["qlens"], case["causal"], SCALE, page=case["page"], shared=shared)
    return case, q, kv, ref, written, info
