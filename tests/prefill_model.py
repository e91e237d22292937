"""The float64 model of prefill attention over a KV cache (include/mfa_prefill.h), its bounds and needle inputs: tests/decode_model.py
applied per sequence with that sequence's own row count, plus the longer accumulation chain of the prefill kernel (a plain module; numpy
only).

  model()           per sequence b: decode_model.model on the first qn_b rows and the first n_b keys (R = qn_b, so its causal rule
                    c <= r + max(n - qn, 0) is this launch's).  Rows at or past qn_b keep O = 0, L = -inf and are the caller's to check.
  needle_queries()  decode_model's needle construction over the keys THIS launch's geometry makes special.
  compare()         decode_model.compare over the live rows of every sequence: no element of a live row is left out.

The chain.  decode_model's bound counts, in E and EL, `chain` FP32 roundings on the accumulators: a decode wave walks a QUARTER of a
sequence's 32-key steps (34 roundings per step: 2 x 16 products added by the two matrix instructions of a step into one accumulator
element, one rescale, one for the row sum's own step), then 4 waves merge (5) and the result is normalised (pieces + 9 in all).  The
prefill kernel's wave walks EVERY step of the keys its row sees -- there is no split across waves and no merge -- so its chain is
  chain_prefill(n) = 34 ceil(n / 32) + 4      (the steps; the half-wave sum of l, 1 / l, the value scale, the product)
against decode_model.chain_length(n, None) = 34 ceil(ceil(n / 32) / 4) + 10.  model() adds the difference, times u = 2^-24, times
(A + |O|) to E and times 1 to EL, outside decode_model (which returns A and O for that purpose).  n is the sequence's length, an upper
bound on what any causal row sees.
"""
import math

import numpy as np

import decode_model as dm

TILE, ROWS = 64, 128   # MFA_PREFILL_KEY_TILE, MFA_PREFILL_PACKED_ROWS
MARGIN = dm.MARGIN     # decode's protocol: the smallest power of two with 2 x headroom over the measured worst err / bound


def chain_prefill(n):
    return 34 * (-(-int(n) // dm.STEP)) + 4


def extra_chain(n):
    return max(0, chain_prefill(n) - dm.chain_length(int(n), None)) * dm.U32


def model(q, k, v, lens, qlens, G, causal, *, kscale=None, vscale=None):
    """q [B, Hq, R, D], k / v [B, Hkv, C, D] (the cache's values WITHOUT the scales when kscale / vscale are given) -> dm.Reference over
    [B, Hq, R]; rows at or past qlens[b] hold O = 0, L = -inf, bounds 0"""
    q, k, v = dm.f64(q), dm.f64(k), dm.f64(v)
    B, Hq, R, D = q.shape
    O, A, E = (np.zeros((B, Hq, R, D)) for _ in range(3))
    L = np.full((B, Hq, R), -np.inf)
    EL = np.zeros((B, Hq, R))
    for b in range(B):
        n, qn = int(lens[b]), min(int(qlens[b]), R)
        if qn == 0 or n == 0:
            continue
        ref = dm.model(q[b:b + 1, :, :qn], k[b:b + 1], v[b:b + 1], [n], G, causal, kscale=kscale, vscale=vscale)
        x = extra_chain(n)
        O[b, :, :qn], L[b, :, :qn], A[b, :, :qn] = ref.O[0], ref.L[0], ref.A[0]
        E[b, :, :qn] = ref.E[0] + x * (ref.A[0] + np.abs(ref.O[0]))
        EL[b, :, :qn] = ref.EL[0] + x
    return dm.Reference(O, L, A, E, EL)


def library_tile_range(n, qn, r0, RB, causal):
    from metal_flash_attention_amd import AttentionPrefill
    return AttentionPrefill.tileRange(n, qn, r0, RB, causal)


def needle_pool(n, qn, G, causal, page, tile_range=None):
    """keys of a sequence the launch's geometry makes special: key 0, 15 / 16, 63 / 64, the first and last key of every page, the last
    tile's first key and the key before it, and the keys either side of first_masked and end of every row block"""
    if n <= 0 or qn <= 0:
        return []
    fn = tile_range or library_tile_range
    RB = ROWS // G
    last = (n - 1) // TILE * TILE
    pool = [0, 15, 16, 63, 64, last, last - 1, n - 1]
    if page:
        for p0 in range(0, n, page):
            pool += [p0, min(p0 + page, n) - 1]
    for r0 in range(0, qn, RB):
        f, e = fn(n, qn, r0, RB, causal)
        pool += [f * TILE - 1, f * TILE, e * TILE - 1, e * TILE, (e - 1) * TILE]
    return sorted({t for t in pool if 0 <= t < n})


def needle_queries(k, lens, qlens, Hq, G, R, causal, fmt, *, page=None, tile_range=None, seed=0):
    """q [B, Hq, R, D] (float64 values of the 16-bit type) and per (b, h, r) its needles {key: weight} and forbidden key: the
    construction of decode_model.needle_queries (q = beta sqrt(D) sum_t w_t k_t / |k_t|^2; every row carries its own frontier and the
    key before it plus its share of the pool, dealt to the rows in turn; a causal row also carries the key AFTER its frontier with
    weight beta + 4, which takes the row over if it is read).  Rows at or past qlens[b] are uniform random."""
    k = dm.f64(k)
    B, Hkv, C, D = k.shape
    rng = np.random.default_rng(seed)
    q = dm.round_to(rng.uniform(-1, 1, (B, Hq, R, D)), fmt)
    info = {}
    for b in range(B):
        n, qn = int(lens[b]), min(int(qlens[b]), R)
        if n == 0 or qn == 0:
            continue
        pool = needle_pool(n, qn, G, causal, page, tile_range)
        off = max(n - qn, 0)
        per_row = 6
        stride = max(1, min(max(2 if len(pool) > 1 else 1, -(-len(pool) // per_row)), Hq * qn))
        for h in range(Hq):
            j = h // G
            for r in range(qn):
                rho = h * qn + r
                fr = min(r + off, n - 1) if causal else n - 1
                T = {t for i, t in enumerate(pool) if i % stride == rho % stride and t <= fr}
                T |= {fr} | ({fr - 1} if fr >= 1 else set())
                beta = math.log(n) + 1.0 - math.log(len(T))
                weights = {t: beta + (((t // dm.STEP + rho) % 4) - 1.5) * (2.0 / 3.0) for t in sorted(T)}
                forbidden = fr + 1 if causal and fr + 1 < n else None
                vec = np.zeros(D)
                for t, w in list(weights.items()) + ([(forbidden, beta + 4.0)] if forbidden is not None else []):
                    kt = k[b, j, t]
                    vec += w * math.sqrt(D) * kt / max(float(kt @ kt), 1e-30)
                q[b, h, r] = dm.round_to(vec, fmt)
                info[(b, h, r)] = (weights, forbidden)
    return q, info


def compare(got_o, got_l, ref, fmt, out, lens, qlens, *, margin=MARGIN, info=None):
    """worst |dO| / bound and |dL| / bound over every live row of every sequence (and text naming the worst); got_l natural units or None"""
    worst_o = worst_l = 0.0
    text = ""
    go = dm.f64(got_o)
    gl = None if got_l is None else dm.f64(got_l)
    for b in range(go.shape[0]):
        n, qn = int(lens[b]), min(int(qlens[b]), go.shape[2])
        if n == 0 or qn == 0:
            continue
        sub = dm.Reference(*(x[b:b + 1, :, :qn] for x in ref))
        sinfo = None if info is None else {(0, h, r): v for (bb, h, r), v in info.items() if bb == b}
        wo, wl, t = dm.compare(go[b:b + 1, :, :qn], None if gl is None else gl[b:b + 1, :, :qn], sub, fmt, out, [n], margin=margin, info=sinfo)
        if wo >= worst_o or wl > worst_l:
            text = "sequence %d (qn %d, n %d): %s" % (b, qn, n, t)
        worst_o, worst_l = max(worst_o, wo), max(worst_l, wl)
    return worst_o, worst_l, text


# ------------------------------------------------------------------------------------------------- the rounding-emulated reference
def emulated(q, k, v, lens, qlens, G, causal, fmt, *, kscale=None, vscale=None):
    """the attention with the kernel's roundings and order of sums -> (O before the store's rounding [B, Hq, R, D], L natural): one wave
    per packed row walks the 32-key steps in order; the running maximum sees visible keys only; P is rounded to the 16-bit type
    against the running maximum, l sums the unrounded p; one normalisation with the value scale at the end.  (A step without a
    visible key for a row leaves its state as it is, so where the block's tile range ends does not enter.)"""
    q, k, v = dm.f64(q), dm.f64(k), dm.f64(v)
    B, Hq, R, D = q.shape
    Hkv = Hq // G
    ks = np.ones(Hkv) if kscale is None else np.asarray(kscale, dtype=np.float64)
    vs = np.ones(Hkv) if vscale is None else np.asarray(vscale, dtype=np.float64)
    O = np.zeros((B, Hq, R, D))
    L = np.full((B, Hq, R), -np.inf)
    for b in range(B):
        n, qn = int(lens[b]), min(int(qlens[b]), R)
        if n == 0 or qn == 0:
            continue
        cols, rows = np.arange(n)[None, :], np.arange(qn)[:, None]
        vis = np.broadcast_to(cols < n, (qn, n))
        if causal:
            vis = vis & (cols <= rows + max(n - qn, 0))
        for h in range(Hq):
            j = h // G
            S2 = np.where(vis, (q[b, h, :qn] @ k[b, j, :n].T) * (ks[j] * dm.LOG2E / math.sqrt(D)), -np.inf)
            m, l, o = np.full(qn, -np.inf), np.zeros(qn), np.zeros((qn, D))
            for key0 in range(0, n, dm.STEP):
                s = S2[:, key0:key0 + dm.STEP]
                new = np.maximum(m, s.max(axis=1))
                fin = np.isfinite(new)
                ref = np.where(fin, new, 0.0)
                corr = np.where(np.isfinite(m), np.exp2(np.where(np.isfinite(m), m, 0.0) - ref), 1.0)
                p = np.where(fin[:, None], np.exp2(s - ref[:, None]), 0.0)
                m, l, o = new, l * corr + p.sum(axis=1), o * corr[:, None] + dm.round_to(p, fmt) @ v[b, j, key0:min(key0 + dm.STEP, n)]
            seen = l > 0
            l0 = np.where(seen, l, 1.0)
            O[b, h, :qn] = np.where(seen[:, None], o * vs[j] / l0[:, None], 0.0)
            L[b, h, :qn] = np.where(seen, (np.where(seen, m, 0.0) + np.log2(l0)) / dm.LOG2E, -np.inf)
    return O, L


# ---------------------------------------------------------------------------------------------------------------------- mutants
# name -> (what the defect is, where it changes nothing).  `case`: per-sequence lists n, qn; R (capacity), G, Hkv, B, causal, page, scales
def _any(case, pred):
    return any(pred(n, qn) for n, qn in zip(case["n"], case["qn"]) if n > 0 and qn > 0)


MUTANTS = {
    "tile_range_short": ("every block stops one 64-key tile early", lambda c: False),
    "tile_range_long_unmasked": ("every block runs one tile more and takes one tile more for unmasked: tile first_masked without the mask",
                                 lambda c: False),
    "frontier_from_rows": ("causal frontier from the capacity `rows` instead of queryLengths[b]",
                           lambda c: not c["causal"] or not _any(c, lambda n, qn: qn < c["R"] and n > qn)),
    "max_dropped": ("max(n - qn, 0) replaced by n - qn", lambda c: not c["causal"] or not _any(c, lambda n, qn: n < qn)),
    "unpack_mod_g": ("Q of packed row p taken from head p % G, row p / G in place of head p / RB, row p % RB", lambda c: c["G"] == 1),
    "r0_dropped": ("Q and frontier of row p % RB without the block's first row", lambda c: not _any(c, lambda n, qn: qn > ROWS // c["G"])),
    "kv_head_mod": ("K/V head h % Hkv in place of h // G", lambda c: c["Hkv"] == 1 or c["G"] == 1),
    "page_table_neighbour": ("the block-table row of the next sequence", lambda c: not c["page"] or c["B"] == 1),
    "page_off_by_one": ("the first 16-key group of a page read from the page before", lambda c: not c["page"] or not _any(c, lambda n, qn: n > c["page"])),
    "key_scale_next_head": ("keyScale of head j + 1", lambda c: not c["scales"] or c["Hkv"] == 1),
    "value_scale_next_head": ("valueScale of head j + 1", lambda c: not c["scales"] or c["Hkv"] == 1),
    "value_scale_omitted": ("valueScale left out", lambda c: not c["scales"]),
}


def mutated(q, k, v, lens, qlens, G, causal, mutant, *, page=None, kscale=None, vscale=None, tile_range=None):
    """float64 attention with the named defect -> (O [B, Hq, R, D], L natural [B, Hq, R]): what a kernel or host plan with that defect
    would compute.  No wrong kernel is ever run.  k, v [B, Hkv, C, D] must hold values wherever a defect may read (the neighbour's keys)."""
    assert mutant is None or mutant in MUTANTS, mutant   # (None: the same arithmetic without a defect, what "changes nothing" is held against)
    q, k, v = dm.f64(q), dm.f64(k), dm.f64(v)
    B, Hq, R, D = q.shape
    Hkv, RB = Hq // G, ROWS // G
    fn = tile_range or library_tile_range
    ks = np.ones(Hkv) if kscale is None else np.asarray(kscale, dtype=np.float64)
    vs = np.ones(Hkv) if vscale is None else np.asarray(vscale, dtype=np.float64)
    O = np.zeros((B, Hq, R, D))
    L = np.full((B, Hq, R), -np.inf)
    for b in range(B):
        n, qn = int(lens[b]), min(int(qlens[b]), R)
        if n == 0 or qn == 0:
            continue
        npad = (-(-n // TILE) + 1) * TILE        # one tile past the last: keys at or past n come in as zeros
        cols, rows = np.arange(npad)[None, :], np.arange(qn)
        r0s = rows // RB * RB
        for h in range(Hq):
            j = h % Hkv if mutant == "kv_head_mod" else h // G
            kb = (b + 1) % B if mutant == "page_table_neighbour" and page else b
            src = np.arange(n)
            if mutant == "page_off_by_one" and page:
                src = np.where((src >= page) & (src % page < 16), src - page, src)
            K, V = np.zeros((npad, D)), np.zeros((npad, D))
            K[:n], V[:n] = k[kb, j][src], v[kb, j][src]
            src_h, src_r = np.full(qn, h), rows
            if mutant == "unpack_mod_g":
                p = (h % G) * RB + (rows - r0s)
                src_h, src_r = (h // G) * G + p % G, np.minimum(r0s + p // G, qn - 1)
            if mutant == "r0_dropped":
                src_r = rows - r0s
            ksc = ks[(j + 1) % Hkv] if mutant == "key_scale_next_head" else ks[j]
            vsc = vs[(j + 1) % Hkv] if mutant == "value_scale_next_head" else 1.0 if mutant == "value_scale_omitted" else vs[j]
            S = (q[b, src_h, src_r] @ K.T) * (ksc / math.sqrt(D))
            vis = np.broadcast_to(cols < n, S.shape).copy()
            if causal:
                base = n - qn if mutant == "max_dropped" else max(n - R, 0) if mutant == "frontier_from_rows" else max(n - qn, 0)
                vis &= cols <= src_r[:, None] + base
            if mutant in ("tile_range_short", "tile_range_long_unmasked"):
                for r0 in range(0, qn, RB):
                    f, e = fn(n, qn, r0, RB, causal)
                    blk = slice(r0, min(r0 + RB, qn))
                    if mutant == "tile_range_short":
                        vis[blk, max(e - 1, 0) * TILE:] = False
                    else:
                        vis[blk, f * TILE:(f + 1) * TILE] = True
            Sm = np.where(vis, S, -np.inf)
            m = Sm.max(axis=1, keepdims=True)
            seen = np.isfinite(m[:, 0])
            m0 = np.where(np.isfinite(m), m, 0.0)
            pw = np.exp(Sm - m0)
            l = pw.sum(axis=1, keepdims=True)
            l0 = np.where(l > 0, l, 1.0)
            O[b, h, :qn] = np.where(seen[:, None], (pw / l0) @ V * vsc, 0.0)
            L[b, h, :qn] = np.where(seen, m0[:, 0] + np.log(l0[:, 0]), -np.inf)
    return O, L
