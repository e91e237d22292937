"""The float64 model of sliding-window attention over a KV cache (include/mfa_window.h), decode and prefill, its bounds, needle inputs,
rounding-emulated reference and named mutants (a plain module; numpy only).  Everything about formats, bounds and comparison is
tests/decode_model.py's (round_to, bounds, compare, Reference, the constants): nothing of it is repeated here.

The rule.  n keys, qn rows (decode: qn = R), frontier f(r) = r + max(n - qn, 0); row r sees key c iff c < n, c <= f(r), c + W > f(r):
the keys lo(r) <= c < lim(r) with lim = min(n, f + 1), lo = max(f + 1, W) - W.

  model()      row r's windowed attention IS plain attention over the keys [lo(r), lim(r)) alone, so model() runs decode_model.model on
               that slice, one row at a time (R = 1, no causal cut), and gets O, L, A and the FP32 terms of the bound from it.  Only the
               CHAIN term is replaced: decode_model counted chain_length(visible keys, None) roundings on the accumulators; the
               windowed kernels walk
                 decode:  pieces of the tiles [lo0 / 64, ceil(n / 64)), lo0 = lo(0): 34 ceil(ceil(longest piece / 32) / 4) + pieces + 9
                 prefill: every 32-key step of the block's tiles [begin, end), one wave:   34 x 2 (end - begin) + 4
               (the counts of decode_model.chain_length and prefill_model.chain_prefill over the tiles actually walked, not over n:
               a bound from n would be looser than the kernels need).  The difference, times u = 2^-24, goes on E (times A + |O|)
               and EL, outside decode_model, as prefill_model does.
  emulated()   the same attention with the kernels' roundings and order of sums over the window's ranges.
  needle_queries()  decode_model's construction (q = beta sqrt(D) sum_t w_t k_t / |k_t|^2) over the keys the window makes special; the
               key below a row's window and the key past its frontier carry weight beta + 4: read, either takes the row over.
  mutated()    a named WRONG attention (MUTANTS) and whether the defect changes anything for the case, decided from the geometry
               alone (which keys each row adds up, and from where), never from a result.  No wrong kernel is ever run.
"""
import math

import numpy as np

import decode_model as dm

TILE, STEP, WAVES, ROWS = dm.TILE, dm.STEP, dm.WAVES, 128   # (ROWS: MFA_PREFILL_PACKED_ROWS)
MARGIN = dm.MARGIN     # decode's protocol: the smallest power of two with 2 x headroom over the measured worst err / bound


def library_piece_range(n, rows, window, pieces, piece):
    from metal_flash_attention_amd import AttentionDecode
    return AttentionDecode.windowPieceRange(n, rows, window, pieces, piece)


def library_tile_range(n, qn, r0, RB, window):
    from metal_flash_attention_amd import AttentionPrefill
    return AttentionPrefill.windowTileRange(n, qn, r0, RB, window)


def frontiers(n, qn, rows, W, off=None):
    """(lo, lim) arrays of the rows `rows` (any integer array)"""
    off = max(n - qn, 0) if off is None else off
    f1 = np.asarray(rows, dtype=np.int64) + off + 1
    return np.maximum(f1, W) - W, np.minimum(f1, n)


def piece_ranges(n, R, W, pieces, piece_range=None):
    """[(begin, end)] of every piece of a windowed decode launch (one piece: the unsplit kernel's range)"""
    fn = piece_range or library_piece_range
    P = int(pieces) if pieces and pieces > 1 else 1
    return [tuple(fn(int(n), int(R), int(W), P, i)) for i in range(P)]


def blocks_of(kind, qn, G):
    """[(first row, one past the last live row)] of the workgroups of one sequence and K / V head"""
    if kind == "decode":
        return [(0, qn)]
    RB = ROWS // G
    return [(r0, min(r0 + RB, qn)) for r0 in range(0, qn, RB)]


def chain_decode(ranges):
    per = max([e - b for b, e in ranges] + [0])
    return 34 * (-(-(-(-per // STEP)) // WAVES)) + len(ranges) + 9


def chain_prefill(begin, end):
    return 34 * 2 * (end - begin) + 4


# ---------------------------------------------------------------------------------------------------------------------- the model
def model(q, k, v, lens, qlens, G, W, *, pieces=None, kscale=None, vscale=None, piece_range=None, tile_range=None):
    """q [B, Hq, R, D], k / v [B, Hkv, C, D] (WITHOUT the scales when kscale / vscale are given) -> dm.Reference over [B, Hq, R].
    qlens None: a decode launch (every sequence has R rows, `pieces` its piece count); otherwise prefill.  Rows at or past qlens[b]
    and rows without a visible key hold O = 0, L = -inf, bounds 0."""
    q, k, v = dm.f64(q), dm.f64(k), dm.f64(v)
    B, Hq, R, D = q.shape
    kind = "decode" if qlens is None else "prefill"
    O, A, E = (np.zeros((B, Hq, R, D)) for _ in range(3))
    L = np.full((B, Hq, R), -np.inf)
    EL = np.zeros((B, Hq, R))
    tr = tile_range or library_tile_range
    for b in range(B):
        n, qn = int(lens[b]), R if qlens is None else min(int(qlens[b]), R)
        if n == 0 or qn == 0:
            continue
        lo, lim = frontiers(n, qn, np.arange(qn), W)
        if kind == "decode":
            chains = {0: chain_decode(piece_ranges(n, R, W, pieces, piece_range))}
        else:
            chains = {}
            for r0, _r1 in blocks_of(kind, qn, G):
                bt, _u0, _u1, et = tr(n, qn, r0, ROWS // G, W)
                chains[r0] = chain_prefill(bt, et)
        for r in range(qn):
            a, e = int(lo[r]), int(lim[r])
            if e <= a:
                continue
            ref = dm.model(q[b:b + 1, :, r:r + 1], k[b:b + 1, :, a:e], v[b:b + 1, :, a:e], [e - a], G, False, kscale=kscale, vscale=vscale)
            chain = chains[0] if kind == "decode" else chains[r // (ROWS // G) * (ROWS // G)]
            x = (chain - dm.chain_length(e - a, None)) * dm.U32
            O[b, :, r], L[b, :, r], A[b, :, r] = ref.O[0, :, 0], ref.L[0, :, 0], ref.A[0, :, 0]
            E[b, :, r] = ref.E[0, :, 0] + x * (ref.A[0, :, 0] + np.abs(ref.O[0, :, 0]))
            EL[b, :, r] = ref.EL[0, :, 0] + x
    return dm.Reference(O, L, A, E, EL)


def compare(got_o, got_l, ref, fmt, out, lens, qlens, *, margin=MARGIN, info=None):
    """dm.compare (decode) / prefill_model.compare (prefill: live rows only) -> (worst |dO| / bound, worst |dL| / bound, text)"""
    if qlens is None:
        return dm.compare(got_o, got_l, ref, fmt, out, lens, margin=margin, info=info)
    import prefill_model as pm
    return pm.compare(got_o, got_l, ref, fmt, out, lens, qlens, margin=margin, info=info)


# ------------------------------------------------------------------------------------------------- the rounding-emulated reference
def _walk(S2, V, steps, fmt):
    """one wave's chain: S2 [rows, keys] base-2 scores (-inf where masked), the 32-key steps at `steps` -> (m, l, o) un-normalised"""
    rows, D = S2.shape[0], V.shape[1]
    m, l, o = np.full(rows, -np.inf), np.zeros(rows), np.zeros((rows, D))
    for key0 in steps:
        s = S2[:, key0:key0 + STEP]
        new = np.maximum(m, s.max(axis=1))
        fin = np.isfinite(new)
        ref = np.where(fin, new, 0.0)
        corr = np.where(np.isfinite(m), np.exp2(np.where(np.isfinite(m), m, 0.0) - ref), 1.0)
        p = np.where(fin[:, None], np.exp2(s - ref[:, None]), 0.0)
        m, l, o = new, l * corr + p.sum(axis=1), o * corr[:, None] + dm.round_to(p, fmt) @ V[key0:key0 + STEP]
    return m, l, o


def _merge(parts):
    """[(m, l, o)] -> the online-softmax merge in the given order (waves of a workgroup; pieces in the combine kernel)"""
    mstar = parts[0][0].copy()
    for m, _l, _o in parts[1:]:
        mstar = np.maximum(mstar, m)
    m0 = np.where(np.isfinite(mstar), mstar, 0.0)
    lt, ot = np.zeros_like(parts[0][1]), np.zeros_like(parts[0][2])
    for m, l, o in parts:
        w = np.where(np.isfinite(m), np.exp2(np.where(np.isfinite(m), m, 0.0) - m0), 0.0)
        lt += w * l
        ot += w[:, None] * o
    return mstar, lt, ot


def _fold(part, s2):
    """the sink logit (base-2 units, [rows]) joins a state (m, l, o): what piece 0 publishes, and what the final normalisation does"""
    m, l, o = part
    mn = np.maximum(m, s2)
    c = np.where(np.isfinite(m), np.exp2(np.where(np.isfinite(m), m, 0.0) - mn), 0.0)
    return mn, l * c + np.exp2(s2 - mn), o * c[:, None]


def scaled_scores(kscale, G, D):
    """the score function of the uncapped kernels: raw dot products x keyScale log2(e) / sqrt(D), -inf where masked"""
    return lambda raw, vis, b, h, rows: np.where(vis, raw * ((1.0 if kscale is None else float(kscale[h // G])) * dm.LOG2E / math.sqrt(D)), -np.inf)


def emulated_walk(q, k, v, lens, qlens, G, fmt, visible, steps, score, *, logits=None, vscale=None):
    """the one walk of the window, sink and soft-cap emulations -> (O before the store's rounding [B, Hq, R, D], L natural).  Per
    workgroup (wm.blocks_of) and query head: visible(n, qn, rows, npad) is the mask [rows, npad]; steps(n, qn, r0) the 32-key steps
    [piece][wave][key0]; score(raw, vis, b, h, rows) the base-2 scores, -inf where masked.  A piece's waves merge, the pieces are
    combined; piece 0 folds the sink logit in, unsplit launches apply it at the final normalisation.  P is rounded to the 16-bit type
    against the running maximum, l sums the unrounded p, the maximum sees visible keys only."""
    q, k, v = dm.f64(q), dm.f64(k), dm.f64(v)
    B, Hq, R, D = q.shape
    kind = "decode" if qlens is None else "prefill"
    vs = np.ones(Hq // G) if vscale is None else np.asarray(vscale, dtype=np.float64)
    O = np.zeros((B, Hq, R, D))
    L = np.full((B, Hq, R), -np.inf)
    for b in range(B):
        n, qn = int(lens[b]), R if qlens is None else min(int(qlens[b]), R)
        if qn == 0:
            continue
        npad = (-(-max(n, 1) // TILE)) * TILE
        for r0, r1 in blocks_of(kind, qn, G):
            vis = visible(n, qn, np.arange(r0, r1), npad)
            waves = steps(n, qn, r0)
            for h in range(Hq):
                j = h // G
                K, V = np.zeros((npad, D)), np.zeros((npad, D))
                K[:n], V[:n] = k[b, j, :n], v[b, j, :n]
                S2 = score(q[b, h, r0:r1] @ K.T, vis, b, h, slice(r0, r1))
                published = [_merge([_walk(S2, V, w, fmt) for w in piece]) if len(piece) > 1 else _walk(S2, V, piece[0], fmt) for piece in waves]
                s2 = None if logits is None else np.full(r1 - r0, float(logits[h]) * dm.LOG2E)
                if s2 is not None and len(published) > 1:
                    published[0] = _fold(published[0], s2)
                mstar, lt, ot = _merge(published) if len(published) > 1 else published[0]
                if s2 is not None and len(published) == 1:
                    mstar, lt, ot = _fold((mstar, lt, ot), s2)
                seen = lt > 0
                l0 = np.where(seen, lt, 1.0)
                O[b, h, r0:r1] = np.where(seen[:, None], ot * vs[j] / l0[:, None], 0.0)
                L[b, h, r0:r1] = np.where(seen, (np.where(seen, mstar, 0.0) + np.log2(l0)) / dm.LOG2E, -np.inf)
    return O, L


def emulated(q, k, v, lens, qlens, G, W, fmt, *, pieces=None, kscale=None, vscale=None, piece_range=None, tile_range=None):
    """the windowed attention with the kernels' roundings and order of sums: emulated_walk over the window's ranges.  decode: per piece
    of the window range the four waves take its 32-key steps in turn.  prefill: one wave walks every step of the block's tiles
    [begin, end) in order"""
    R = q.shape[2]

    def visible(n, qn, rows, npad):
        lo, lim = frontiers(n, qn, rows, W)
        cols = np.arange(npad)[None, :]
        return (cols >= lo[:, None]) & (cols < lim[:, None])

    def steps(n, qn, r0):
        if n == 0:
            return [[[]]]
        if qlens is None:
            return [[list(range(pb + w * STEP, pe, WAVES * STEP)) for w in range(WAVES)] for pb, pe in piece_ranges(n, R, W, pieces, piece_range)]
        bt, _u0, _u1, et = (tile_range or library_tile_range)(n, qn, r0, ROWS // G, W)
        return [[list(range(bt * TILE, et * TILE, STEP))]]

    return emulated_walk(q, k, v, lens, qlens, G, fmt, visible, steps, scaled_scores(kscale, G, q.shape[3]), vscale=vscale)


# ------------------------------------------------------------------------------------------------------------------ needle inputs
def needle_pool(n, qn, R, G, W, kind, pieces=None, page=None, piece_range=None, tile_range=None):
    """keys of a sequence the window's geometry makes special: lo(r) - 1, lo(r), lo(r) + 1 of the first and last row; the first and last
    key of every workgroup's first tile; both sides of unmaskedBegin and unmaskedEnd of every row block; both sides of every window
    piece boundary; the first key of the first windowed page and the first key loaded; the last step's first key, the key before it and
    the last key"""
    if n <= 0 or qn <= 0:
        return []
    lo, _lim = frontiers(n, qn, np.array([0, qn - 1]), W)
    pool = [int(x) + d for x in lo for d in (-1, 0, 1)]
    last = (n - 1) // STEP * STEP
    pool += [last, last - 1, n - 1]
    firsts = []
    if kind == "decode":
        ranges = [r for r in piece_ranges(n, R, W, pieces, piece_range) if r[1] > r[0]]
        for pb, pe in ranges:
            pool += [pb - 1, pb, pe - 1, pe]
        firsts = [ranges[0][0]] if ranges else []
    else:
        tr = tile_range or library_tile_range
        for r0, _r1 in blocks_of(kind, qn, G):
            bt, u0, u1, et = tr(n, qn, r0, ROWS // G, W)
            if et > bt:
                firsts.append(bt * TILE)
                pool += [u0 * TILE - 1, u0 * TILE, u1 * TILE - 1, u1 * TILE, et * TILE - 1, (et - 1) * TILE]
    for first in firsts:
        pool += [first, first + TILE - 1]
        if page:
            pool += [first // page * page, first // page * page + page - 1, first // page * page + page]
    return sorted({t for t in pool if 0 <= t < n})


def needle_queries(k, lens, qlens, Hq, G, R, W, fmt, *, pieces=None, page=None, piece_range=None, tile_range=None, seed=0):
    """q [B, Hq, R, D] (float64 values of the 16-bit type) and per live (b, h, r) its needles {key: weight} and ONE forbidden key for
    dm.compare's text (the key below the window where there is one, else the key past the frontier).  Every row carries its frontier and
    the key before it, the first key of its window and the one after, and its share of needle_pool() inside its window, dealt to the
    rows in turn.  Both forbidden keys -- lo(r) - 1 and f(r) + 1, where they exist below n -- enter q with weight beta + 4."""
    k = dm.f64(k)
    B, _Hkv, _C, D = k.shape
    kind = "decode" if qlens is None else "prefill"
    rng = np.random.default_rng(seed)
    q = dm.round_to(rng.uniform(-1, 1, (B, Hq, R, D)), fmt)
    info = {}
    for b in range(B):
        n, qn = int(lens[b]), R if qlens is None else min(int(qlens[b]), R)
        if n == 0 or qn == 0:
            continue
        pool = needle_pool(n, qn, R, G, W, kind, pieces, page, piece_range, tile_range)
        lo, lim = frontiers(n, qn, np.arange(qn), W)
        for h in range(Hq):
            j = h // G
            for r in range(qn):
                a, e = int(lo[r]), int(lim[r])
                if e <= a:
                    continue   # (no visible key: the row stays uniform random, its output is the caller's to check)
                rho, fr = h * qn + r, e - 1
                inside = [t for t in pool if a <= t <= fr]
                stride = max(1, min(max(2 if len(inside) > 1 else 1, -(-len(inside) // 6)), Hq * qn))
                T = {t for i, t in enumerate(inside) if i % stride == rho % stride} | {fr, max(fr - 1, a), a, min(a + 1, fr)}
                beta = math.log(e - a) + 1.0 - math.log(len(T))
                weights = {t: beta + (((t // STEP + rho) % 4) - 1.5) * (2.0 / 3.0) for t in sorted(T)}
                forbidden = [t for t in (a - 1, fr + 1) if 0 <= t < n]
                vec = np.zeros(D)
                for t, w in list(weights.items()) + [(t, beta + 4.0) for t in forbidden]:
                    kt = k[b, j, t]
                    vec += w * math.sqrt(D) * kt / max(float(kt @ kt), 1e-30)
                q[b, h, r] = dm.round_to(vec, fmt)
                info[(b, h, r)] = (weights, forbidden[0] if forbidden else None)
    return q, info


# ---------------------------------------------------------------------------------------------------------------------- mutants
# name -> what the defect is.  Whether it changes anything for a case is decided by mutated() from the geometry (third return value).
MUTANTS = {
    "lo_one_long": "lower frontier one key long: lo - 1",
    "lo_one_short": "lower frontier one key short: lo + 1",
    "lo_of_row_0": "every row uses the lower frontier of the workgroup's first row",
    "lo_from_rows": "lower frontier from the capacity `rows` instead of queryLengths[b]",
    "lo_max_unclamped": "max(n - qn, 0) replaced by n - qn in the lower frontier",
    "first_tile_dropped": "the workgroup's first tile is not walked",
    "begin_early_unmasked": "begin one tile early, and that tile without the lower mask",
    "low_zone_unmasked": "prefill: the tiles [begin, unmaskedBegin) run without any mask",
    "pieces_over_0_n": "decode: pieces cut over [0, n) as without a window, the pieces that begin below the window's first tile dropped whole",
    "piece_range_without_rows": "decode: the piece range from lo0 = max(n, W) - W, as if rows were 1",
    "first_page_from_entry_0": "the first windowed page taken from block-table entry 0",
    "parity_opposite": "prefill: the buffer of tile t taken as t & 1: with an odd `begin` the first tile is computed from the buffer that was never filled (zeros)",
    "ge_for_gt": "c + W >= f in place of c + W > f",
}


def _py_piece_ranges(n, first_tile, pieces):
    tiles = max(-(-n // TILE) - first_tile, 0)
    out = []
    for p in range(pieces):
        b, e = (first_tile + p * tiles // pieces) * TILE, min((first_tile + (p + 1) * tiles // pieces) * TILE, n)
        out.append((min(b, e), e))
    return out


def _geometry(n, qn, R, G, W, kind, r0, r1, mutant, pieces, page, piece_range, tile_range):
    """what the workgroup of rows [r0, r1) adds up: vis [rows, npad] and, per key, where its K / V rows come from (src, -1: zeros)"""
    npad = (-(-n // TILE) + 1) * TILE
    cols = np.arange(npad)[None, :]
    rows = np.arange(r0, r1)
    lo, lim = frontiers(n, qn, rows, W)
    if mutant == "lo_one_long":
        lo = np.maximum(lo - 1, 0)
    elif mutant == "lo_one_short":
        lo = lo + 1
    elif mutant == "lo_of_row_0":
        lo = np.full_like(lo, lo[0])
    elif mutant == "lo_from_rows":
        lo, _ = frontiers(n, qn, rows, W, off=max(n - R, 0))
    elif mutant == "lo_max_unclamped":
        lo, _ = frontiers(n, qn, rows, W, off=n - qn)
        lo = np.maximum(lo, 0)
    elif mutant == "ge_for_gt":
        lo = np.maximum(rows + max(n - qn, 0) - W, 0)
    vis = (cols >= lo[:, None]) & (cols < lim[:, None])
    P = int(pieces) if pieces and pieces > 1 else 1
    if kind == "decode":
        ranges = piece_ranges(n, R, W, P, piece_range)
        first = ranges[0][0]
        if mutant == "pieces_over_0_n" and P > 1:
            ranges = [(b, e) for b, e in _py_piece_ranges(n, 0, P) if b >= first]
        if mutant == "piece_range_without_rows":
            ranges = _py_piece_ranges(n, (max(n, W) - W) // TILE, P)
    else:
        bt, u0, u1, et = (tile_range or library_tile_range)(n, qn, r0, ROWS // G, W)
        ranges, first = [(bt * TILE, min(et * TILE, npad))], bt * TILE
        if mutant == "low_zone_unmasked":
            vis[:, bt * TILE:u0 * TILE] = True
    loaded = np.zeros(npad, dtype=bool)
    for b, e in ranges:
        loaded[b:e] = True
    filled = [r for r in ranges if r[1] > r[0]]
    if mutant == "first_tile_dropped" and filled:
        loaded[filled[0][0]:filled[0][0] + TILE] = False
    if mutant == "begin_early_unmasked" and filled and filled[0][0] >= TILE:
        early = slice(filled[0][0] - TILE, filled[0][0])
        loaded[early] = True
        vis[:, early] = cols[:, early] < lim[:, None]
    vis &= loaded[None, :]
    src = np.where(np.arange(npad) < n, np.arange(npad), -1)
    if mutant == "first_page_from_entry_0" and page and filled:
        p0 = filled[0][0] // page
        src = np.where((src >= 0) & (np.arange(npad) // page == p0), np.arange(npad) - p0 * page, src)
    if mutant == "parity_opposite" and kind == "prefill" and filled and (first // TILE) % 2 == 1:
        src[first:first + TILE] = -1
    return vis, src


def mutated(q, k, v, lens, qlens, G, W, mutant, *, pieces=None, page=None, kscale=None, vscale=None, piece_range=None, tile_range=None):
    """float64 attention with the named defect (None: without one) -> (O [B, Hq, R, D], L natural [B, Hq, R], changed): `changed` is
    whether any workgroup adds up another set of keys, or a visible key from another place, than without the defect"""
    assert mutant is None or mutant in MUTANTS, mutant
    q, k, v = dm.f64(q), dm.f64(k), dm.f64(v)
    B, Hq, R, D = q.shape
    Hkv = Hq // G
    kind = "decode" if qlens is None else "prefill"
    ks = np.ones(Hkv) if kscale is None else np.asarray(kscale, dtype=np.float64)
    vs = np.ones(Hkv) if vscale is None else np.asarray(vscale, dtype=np.float64)
    O = np.zeros((B, Hq, R, D))
    L = np.full((B, Hq, R), -np.inf)
    changed = False
    for b in range(B):
        n, qn = int(lens[b]), R if qlens is None else min(int(qlens[b]), R)
        if n == 0 or qn == 0:
            continue
        for r0, r1 in blocks_of(kind, qn, G):
            vis, src = _geometry(n, qn, R, G, W, kind, r0, r1, mutant, pieces, page, piece_range, tile_range)
            if mutant is not None:
                vis0, src0 = _geometry(n, qn, R, G, W, kind, r0, r1, None, pieces, page, piece_range, tile_range)
                changed = changed or bool((vis != vis0).any()) or bool((vis.any(axis=0) & (src != src0)).any())
            for h in range(Hq):
                j = h // G
                K = np.where(src[:, None] >= 0, k[b, j][np.maximum(src, 0)], 0.0)
                V = np.where(src[:, None] >= 0, v[b, j][np.maximum(src, 0)], 0.0)
                S = np.where(vis, (q[b, h, r0:r1] @ K.T) * (ks[j] / math.sqrt(D)), -np.inf)
                m = S.max(axis=1, keepdims=True)
                seen = np.isfinite(m[:, 0])
                m0 = np.where(np.isfinite(m), m, 0.0)
                pw = np.exp(S - m0)
                l0 = np.where(seen, pw.sum(axis=1), 1.0)
                O[b, h, r0:r1] = np.where(seen[:, None], (pw / l0[:, None]) @ V * vs[j], 0.0)
                L[b, h, r0:r1] = np.where(seen, m0[:, 0] + np.log(l0), -np.inf)
    return O, L, changed
