"""The float64 model of multi-head latent attention decode over a compressed cache (include/mfa_mla.h), its per-element error bounds,
the needle inputs, the named mutants and the cases the CPU and GPU files share (a plain module after tests/decode_model.py, from which it
takes Reference, bounds, compare, U_P, U_OUT, round_to, store and piece_ranges; numpy only).

  model()          float64 attention with the CALLER's scale over the first len_b rows of a cache [B, C, 576]: every head reads the same
                   row, 576 columns as its key and the first 512 as its value.  O, L, A = sum_i p_i |v_i| and the FP32 terms E / EL of
                   the bound.  mutant= computes a named WRONG attention instead (MUTANTS).  No wrong kernel is ever run.
  emulated()       the same attention with the kernel's roundings and order of sums: what a correct kernel may give.
  needle_queries() query rows in which single keys matter (decode_model's, rescaled to the caller's scale).
  CASES, inputs()  the launches of tests/test_mla_gpu.py, which tests/test_mla_sensitivity.py walks on the CPU.

The bound is decode_model's, term for term (its docstring), with what the kernel of attn_mla16.h changes:
  * the score.  A score is a dot product of Dk = 576 exact products.  The kernel sums it as FOUR chains of 144 (a wave's nine matrix
    instructions over its 128 latent and 16 rotary columns), adds the four partials in FP32, ((w0 + w1) + w2) + w3, and multiplies by
    scale2 = fl(scale log2 e), itself one rounding away from scale log2 e: at most 144 + 3 + 2 roundings on any product.  The bound keeps
    the worst case of ONE chain over all columns, e_i <= (Dk + 3) u scale log2(e) sum_d |q_d k_id|, which covers both orders.
  * the chain.  All four waves walk the SAME 32-key steps and each keeps its own 128 columns of O^T: one accumulator per output element
    walks every step of the piece -- per step one rescale and 2 x 16 products (34 with the row sum's add) -- and there is no merge of
    waves.  steps = ceil(keys of the largest piece / 32), a piece being ceil(tiles / pieces) 64-key tiles.  Then, unsplit: the half-wave
    add of l, the reciprocal and the product (3).  Split: the pieces publish unrounded FP32; the combine kernel forms exp2(m_s - m*)
    (3), walks the pieces in order with one product and one add each (2 pieces), adds l over the wave (6), and normalises (2).
    chain = 34 steps + 2 pieces + 12 covers both (pieces = 1 unsplit), on a sum of magnitude A (numerator) and 1 (l).
  * P is rounded to the 16-bit type against the row's one running maximum (u_P A); the store rounds as decode's (u_out |O|).
MARGIN is fixed by tests/test_mla_sensitivity.py alone, before any GPU run: the smallest power of two with at least 2 x headroom over
emulated()'s worst err / bound at margin 1 on CASES and SEAM_CASES together.

Two batches.  LENS in a cache of C keys is the batch of CASES.  SEAM_LENS in a cache of SEAM_C keys is the batch of SEAM_CASES: lengths ON
the seams a serving loop meets every few tokens -- full last steps, full last pages, whole piece tiles, n == column and n > column (the
launch is handed 400; the header clamps it to the column, and so do model() and emulated(): a length past the cache's rows is read as
the cache's rows).  A case carries its batch (lens, C); inputs() serves both dicts.
"""
import functools
import math

import numpy as np

import decode_model as dm
from decode_model import LN2, LOG2E, U32, Reference, bounds, compare, piece_ranges, round_to, store, U_P, U_OUT  # noqa: F401

DK, DV = 576, 512
STEP, TILE, ROWS = 32, 64, 32       # keys per step, keys per piece tile, packed rows of a workgroup (attn_mla16.h)
SLICE = 128                         # latent columns of a wave; its rotary columns are 16
MARGIN = 2
SCALE = 0.1352337788608801          # 1 / sqrt(192) x (0.1 ln 40 + 1)^2: DeepSeek-V3's softmax scale under YaRN
LENS, C = (700, 200, 100, 5, 0, 1500), 1536
# the seam batch: one, two and three steps exactly (32, 64, 96), one key, n < R and n == R for R = 8, one past a step, full last pages for
# every page size from 16 to 64, one and four whole tiles, n == column and n > column.  The sequence of 400 is followed by the empty one:
# a kernel that does not clamp walks into that sequence's rows, which a launch fills with poison.
SEAM_LENS, SEAM_C = (1, 8, 16, 32, 33, 64, 96, 256, 320, 400, 0), 320


def chain_length(n, pieces):
    tiles = (n + TILE - 1) // TILE
    per = -(-tiles // pieces) * TILE if pieces and pieces > 1 else n
    return 34 * (-(-per // STEP)) + 2 * (pieces or 1) + 12


# ---------------------------------------------------------------------------------------------------------------------- mutants
# name -> (what the defect is, where it changes nothing).  `case` has n (the clamped length), raw (the length the launch is handed), C,
# R, H, B, causal, pieces, page.
MUTANTS = {
    "len_minus_2": ("c < len replaced by c <= len - 2", lambda c: False),
    "causal_plus_1": ("causal frontier one key too far", lambda c: not c["causal"] or c["R"] == 1 or c["n"] < 2),
    "causal_minus_1": ("causal frontier one key short", lambda c: not c["causal"]),
    "max_dropped": ("max(n - R, 0) replaced by n - R", lambda c: not c["causal"] or c["n"] >= c["R"]),
    "wave_partial_dropped": ("one wave's partial score left out of the sum of the step before the sequence's last", lambda c: c["n"] <= STEP),
    "final_partial_step_dropped": ("the partial last step is not run", lambda c: c["n"] % STEP == 0),
    "full_last_step_dropped": ("the last step is not run when it is full", lambda c: c["n"] % STEP != 0),
    "length_not_clamped": ("cacheLengths[b] not clamped to column: the keys column .. n - 1 are walked, in a packed cache the first rows "
                           "of sequence b + 1", lambda c: c["raw"] <= c["C"]),
    "page_boundary_key_from_next_page": ("a key on the last slot of a page read from slot 0 of the page after it",
                                         lambda c: not c["page"] or c["n"] <= c["page"]),
    "piece_loses_last_tile": ("every piece stops one 64-key tile early", lambda c: not c["pieces"]),
    "piece_overlaps": ("every piece starts one tile early, inside its neighbour", lambda c: not c["pieces"] or c["n"] <= TILE),
    "combine_ignores_maxima": ("the combine adds the pieces without exp2(m_s - m*)", lambda c: not c["pieces"] or c["n"] <= TILE),
    "combine_counts_empty": ("a piece without a visible key enters the combine as a step of zero keys scored 0",
                             lambda c: not c["pieces"] or -(-c["n"] // TILE) >= c["pieces"]),
    "page_table_neighbour": ("the block-table row of the next sequence", lambda c: not c["page"] or c["B"] == 1),
    "page_off_by_one": ("the first 16-key group of a page read from the page before", lambda c: not c["page"] or c["n"] <= c["page"]),
    "rows_swapped": ("the R rows of a head swapped", lambda c: c["R"] == 1),
    "v_from_tail": ("V taken from the columns 64 .. 575", lambda c: False),
    "rope_left_out": ("the rotary columns 512 .. 575 left out of the score", lambda c: False),
    "scale_sqrt_dk": ("scale 1 / sqrt(576) in place of the caller's", lambda c: False),
    "o_blocks_exchanged": ("the first two 128-column blocks of O exchanged", lambda c: False),
    "group_head_wrap": ("a packed row at or past 32 computed with the head of row p - 32", lambda c: c["H"] * c["R"] <= ROWS),
    "head_mod_r": ("head p % R in place of p / R", lambda c: c["R"] == 1 or c["H"] == 1),
}


SEAM_MUTANTS = ("full_last_step_dropped", "length_not_clamped")   # invisible on LENS by their own rule: only SEAM_CASES show them


def facts_of(case, pieces, n):
    """what a mutant's `harmless` rule is asked about: the case's launch and ONE sequence, n as the launch is handed it"""
    return dict(R=case["R"], H=case["H"], B=len(case["lens"]), causal=case["causal"], pieces=pieces, page=case["page"], C=case["C"], raw=n,
                n=min(n, case["C"]))


def _query_of(mutant, h, r, H, R):
    """(head, row) whose q a (mutated) kernel reads for packed row p = h R + r"""
    p = h * R + r
    if mutant == "head_mod_r":
        return (p % R) % H, (p // R) % R
    if mutant == "group_head_wrap" and p >= ROWS:
        return (p - ROWS) // R, r
    return h, r


def model(q, kv, lens, causal, scale, mutant=None, *, pieces=None, page=None, shared=False, piece_range=None):
    """float64 attention -> Reference(O, L, A, E, EL).  q [B, H, R, 576], kv [B, C, 576] (shared: sequence b reads kv[0], a launch with
    batchStride 0).  pieces / page: the launch's geometry (they change the bound's chain length and what the mutants do, never the
    unmutated values).  A length past the cache's C rows is clamped to C, as the launch clamps it to `column`."""
    assert mutant is None or mutant in MUTANTS, mutant
    q, kv = dm.f64(q), dm.f64(kv)
    B, H, R, _ = q.shape
    O, A, E = (np.zeros((B, H, R, DV)) for _ in range(3))
    L = np.full((B, H, R), -np.inf)
    EL = np.zeros((B, H, R))
    sc = 1.0 / math.sqrt(DK) if mutant == "scale_sqrt_dk" else float(scale)
    for b in range(B):
        n = min(int(lens[b]), kv.shape[1])
        if mutant == "length_not_clamped":
            n = int(lens[b])
        if n == 0:
            continue
        ranges = piece_ranges(n, pieces, piece_range)
        split = len(ranges) > 1
        cols = np.arange(n)[None, :]
        chain = chain_length(n, pieces) * U32
        src_b = 0 if shared else b
        if mutant == "page_table_neighbour" and page:
            src_b = (b + 1) % B
        K = kv[src_b, :n]
        if n > kv.shape[1]:                     # (length_not_clamped alone: the rows behind the cache's last are the next sequence's)
            K = np.concatenate([kv[src_b], kv[(src_b + 1) % B]])[:n]
        if mutant == "page_off_by_one" and page:
            src = np.arange(n)
            first = (src >= page) & (src % page < 16)
            K = kv[src_b][np.where(first, src - page, src)]
        if mutant == "page_boundary_key_from_next_page" and page:
            src = np.arange(n)
            K = kv[src_b][np.where((src % page == page - 1) & (src + 1 < n), src + 1, src)]
        V = K[:, 64:DK] if mutant == "v_from_tail" else K[:, :DV]
        Ks = K[:, :DV] if mutant == "rope_left_out" else K
        absV = np.abs(V)
        for h in range(H):
            picked = [_query_of(mutant, h, r, H, R) for r in range(R)]
            qh = np.stack([q[b, hh, rr] for hh, rr in picked])
            qrow = np.array([rr for _hh, rr in picked])[:, None]
            qs = qh[:, :DV] if mutant == "rope_left_out" else qh
            raw = qs @ Ks.T
            if mutant == "wave_partial_dropped" and n > STEP:
                t = (n - 1) // STEP - 1
                lost = np.r_[2 * SLICE:3 * SLICE, DV + 32:DV + 48]   # wave 2's columns
                raw[:, t * STEP:(t + 1) * STEP] -= qh[:, lost] @ K[t * STEP:(t + 1) * STEP][:, lost].T
            S = raw * sc
            limit = n - 1 if mutant == "len_minus_2" else n
            vis = np.broadcast_to(cols < limit, S.shape).copy()
            if causal:
                base = n - R if mutant == "max_dropped" else max(n - R, 0)
                off = 1 if mutant == "causal_plus_1" else -1 if mutant == "causal_minus_1" else 0
                vis &= cols <= qrow + base + off
            if mutant == "final_partial_step_dropped" and n % STEP:
                vis[:, n // STEP * STEP:] = False
            if mutant == "full_last_step_dropped" and n % STEP == 0:
                vis[:, n - STEP:] = False
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
                num, den, mstar = np.zeros((R, DV)), np.zeros((R, 1)), m0.copy()
                if mutant == "combine_counts_empty":
                    mstar = np.maximum(mstar, np.where([[any(not np.isfinite(pm[r, 0]) for _, _, pm in parts)] for r in range(R)], 0.0, -np.inf))
                for (pb, pe, pm) in parts:
                    for r in range(R):
                        if np.isfinite(pm[r, 0]):
                            e = np.exp(Sm[r, pb:pe] - pm[r, 0]) * mult[pb:pe]
                            w = 1.0 if mutant == "combine_ignores_maxima" else math.exp(pm[r, 0] - mstar[r, 0])
                            num[r] += w * (e @ V[pb:pe])
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
            O[b, h] = P @ V
            L[b, h] = np.where(seen, m0[:, 0] + np.log(l0[:, 0]), -np.inf)
            if mutant is None:
                A[b, h] = P @ absV
                e2 = (DK + 3) * U32 * (LOG2E * sc) * (np.abs(qh) @ np.abs(K).T)
                smin = np.where(vis, S, np.inf).min(axis=1, keepdims=True)
                spread2 = np.where(seen[:, None], (m0 - np.where(np.isfinite(smin), smin, m0)) * LOG2E, 0.0)
                rel = LN2 * (e2 + 3 * U32 * spread2) + 4 * U32
                relp = (rel * P).sum(axis=1)
                E[b, h] = (rel * P) @ absV + np.abs(O[b, h]) * relp[:, None] + chain * (A[b, h] + np.abs(O[b, h]))
                Lf = np.where(seen, L[b, h], 0.0)
                EL[b, h] = relp + chain + 4 * U32 * (np.abs(m0[:, 0]) + np.abs(np.log(l0[:, 0])) + np.abs(Lf))
    if mutant == "rows_swapped":
        O, L = O[:, :, ::-1].copy(), L[:, :, ::-1].copy()
    if mutant == "o_blocks_exchanged":
        O = np.concatenate([O[..., SLICE:2 * SLICE], O[..., :SLICE], O[..., 2 * SLICE:]], axis=-1)
    return Reference(O, L, A, E, EL)


# ------------------------------------------------------------------------------------------------- the rounding-emulated reference
def emulated(q, kv, lens, causal, scale, fmt, *, pieces=None, shared=False, piece_range=None):
    """the model with the kernel's roundings and its order of sums -> (O before the store's rounding [B, H, R, 512], L natural): the scale
    is fl(fl(scale) x fl(log2 e)); a piece walks its keys in 32-key steps with ONE running (m, l, O) per row, P rounded to the 16-bit type
    against that maximum; the pieces are combined in order; store(O, out) is what a launch with that output type may write"""
    q, kv = dm.f64(q), dm.f64(kv)
    B, H, R, _ = q.shape
    O = np.zeros((B, H, R, DV))
    L = np.full((B, H, R), -np.inf)
    rows = np.arange(R)[:, None]
    NEG = -np.inf
    scale2 = float(np.float32(np.float32(scale) * np.float32(1.44269504089)))
    for b in range(B):
        n = min(int(lens[b]), kv.shape[1])
        if n == 0:
            continue
        ranges = piece_ranges(n, pieces, piece_range)
        cols = np.arange(n)[None, :]
        K = kv[0 if shared else b, :n]
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
                published.append((m, l, o))
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
            O[b, h] = np.where(seen[:, None], ot / l0[:, None], 0.0)
            L[b, h] = np.where(seen, (np.where(seen, mstar, 0.0) + np.log2(l0)) / LOG2E, -np.inf)
    return O, L


# ------------------------------------------------------------------------------------------------------------------ needle inputs
def needle_queries(kv, lens, H, R, causal, fmt, scale, *, pieces=None, page=None, shared=False, piece_range=None, seed=0):
    """q [B, H, R, 576] (float64 values of the 16-bit type) and, per (b, h, r), its needles and its forbidden key: decode_model's
    needle_queries over the one cache "head" with all H heads in its group -- the same packed index p = h R + r -- rescaled from
    1 / sqrt(Dk) to the caller's scale, so that a needle scores what it scores there"""
    kv = dm.f64(kv)
    B = len(lens)
    lens = [min(int(n), kv.shape[1]) for n in lens]
    seen = np.broadcast_to(kv[:1], (B,) + kv.shape[1:]) if shared else kv
    q, info = dm.needle_queries(seen[:, None], lens, H, H, R, causal, fmt, pieces=pieces, page=page, piece_range=piece_range, seed=seed)
    return round_to(q / (scale * math.sqrt(DK)), fmt), info


# ---------------------------------------------------------------------------------------------------------------------- the cases
# name -> the launch: fmt, H, R, causal, pieces (None: no workspace; "plan": the host's; a number: forced), page, layout ("packed",
# "ld640": rows 640 elements apart in a larger allocation, "shared": batchStride 0, every sequence reads sequence 0's cache), out, and
# the batch it runs on: lens as the launch is handed them, in a cache of C keys
def _case(fmt, H, R, causal=True, pieces=None, page=None, layout="packed", out=None, lens=LENS, C=C):
    return dict(fmt=fmt, H=H, R=R, causal=causal, pieces=pieces, page=page, layout=layout, out=out or fmt, lens=tuple(lens), C=C)


def _seam(fmt, H, R, **kw):
    return _case(fmt, H, R, lens=SEAM_LENS, C=SEAM_C, **kw)


CASES = {
    "1 unsplit": _case("bf16", 16, 1),
    "1 planned": _case("bf16", 16, 1, pieces="plan"),
    "2 seam inside a head": _case("f16", 11, 3),
    "2 seam inside a head, planned": _case("f16", 11, 3, pieces="plan"),
    "3 two groups, rows 640 apart": _case("bf16", 40, 1, pieces="plan", layout="ld640"),
    "3 two groups, one cache shared": _case("bf16", 40, 1, layout="shared"),
    "4 one row": _case("bf16", 1, 1, pieces="plan"),
    "5 eight rows": _case("bf16", 4, 8, pieces="plan"),
    "5 four rows, not causal": _case("bf16", 4, 4, causal=False),
    "6 pages of 16": _case("f16", 16, 4, pieces="plan", page=16),
    "6 pages of 256": _case("f16", 16, 4, page=256),
    "7 two pieces": _case("bf16", 16, 1, pieces=2),
    "7 seven pieces": _case("bf16", 16, 1, pieces=7),
    "7 sixty-four pieces, fp32 out": _case("bf16", 16, 1, pieces=64, out="f32"),
}


# the seam batch: the column is five 64-key tiles; n = 64 has one tile, n = 256 exactly four, so forced pieces leave pieces without a
# tile (64 pieces), a last piece of one tile (2: 3 + 2) and one tile a piece (5).  Pages of 512 hold the whole column in ONE page: the
# table has one entry a sequence
SEAM_CASES = {
    "s1 seam inside a head, unsplit": _seam("f16", 11, 3),
    "s2 eight rows": _seam("bf16", 4, 8),
    "s3 two groups, not causal": _seam("bf16", 40, 1, causal=False),
    "s4 two pieces": _seam("bf16", 16, 1, pieces=2),
    "s4 five pieces": _seam("f16", 11, 3, pieces=5),
    "s4 sixty-four pieces, fp32 out": _seam("bf16", 4, 8, pieces=64, out="f32"),
    "s5 pages of 16": _seam("f16", 16, 4, page=16),
    "s5 pages of 32, two pieces": _seam("bf16", 16, 2, pieces=2, page=32),
    "s5 pages of 64": _seam("f16", 11, 3, page=64),
    "s5 pages of 64, five pieces": _seam("bf16", 16, 1, pieces=5, page=64),
    "s6 pages of 512, one a sequence": _seam("bf16", 16, 2, page=512),
    "s6 pages of 512, two pieces": _seam("f16", 16, 1, pieces=2, page=512),
}
ALL_CASES = dict(CASES, **SEAM_CASES)


def seen_lens(case):
    """the lengths the launch of a case reads: the case's, clamped to its column"""
    return tuple(min(n, case["C"]) for n in case["lens"])


def planned_pieces(case):
    """the piece count the launch of a case runs in (None: unsplit), from the library's own plan"""
    if case["pieces"] is None:
        return None
    if case["pieces"] != "plan":
        return int(case["pieces"])
    from metal_flash_attention_amd import AttentionMLADecode
    _bytes, pieces = AttentionMLADecode().plannedSplit(rows=case["R"], column=case["C"], heads=case["H"], batches=len(case["lens"]), scale=SCALE,
                                                       cacheLengths=0x1000)   # (the host never reads the lengths)
    return pieces if pieces > 1 else None


@functools.lru_cache(maxsize=None)
def cache_values(fmt, seed=0, batches=len(LENS), column=C):
    """kv [B, C, 576] float64 values of the 16-bit type, every key a value (the empty sequence's and those past a length too: what a
    mutant reads there is finite)"""
    rng = np.random.default_rng(1000 + seed + (fmt == "f16") + (0 if (batches, column) == (len(LENS), C) else 7 * column))
    return round_to(rng.uniform(-1.0, 1.0, (batches, column, DK)), fmt)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(case, pieces, q, kv, Reference, needle info) of a case of CASES or SEAM_CASES, computed once and shared; the lengths are the
    case's own (case["lens"] as the launch is handed them, seen_lens(case) as it reads them)"""
    case = ALL_CASES[name]
    pieces = planned_pieces(case)
    lens = case["lens"]
    kv = cache_values(case["fmt"], 0, len(lens), case["C"])
    shared = case["layout"] == "shared"
    q, info = needle_queries(kv, lens, case["H"], case["R"], case["causal"], case["fmt"], SCALE, pieces=pieces, page=case["page"], shared=shared)
    ref = model(q, kv, lens, case["causal"], SCALE, pieces=pieces, page=case["page"], shared=shared)
    return case, pieces, q, kv, ref, info
