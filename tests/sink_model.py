"""The float64 model of attention sinks over a KV cache (include/mfa_sink.h), decode and prefill: sink TOKENS (the keys [0, S) stay
visible under a sliding window) and sink LOGITS (one per query head, in the softmax denominator only), with bounds, needle inputs, a
rounding-emulated reference and named mutants (a plain module; numpy only).  Formats, bounds and comparison are tests/decode_model.py's,
the window's frontiers and helpers tests/window_model.py's: nothing of either is repeated here.

The rule.  n, qn, f(r), lim(r) = min(n, f + 1), lo(r) = max(f + 1, W) - W as in window_model (W = 0: lo = 0; not causal: lim = n).
Row r sees key c iff c < lim and (c >= lo or c < S).  With a sink logit s (natural units, NOT scaled by 1 / sqrt(D) or a key scale)
O = sum p v / (l + e^(s - m)) and L = log(sum e^score + e^s); a live row without a visible key has O = 0, L = s.

  model()      row r's attention IS decode_model.model over the concatenated key slice [0, min(S, lo)) ++ [lo, lim), one row at a
               time; the sink logit then multiplies O, A and the FP32 term by w = 1 / (1 + e^(s - L0)) and L = logaddexp(L0, s), in
               float64.  The CHAIN term is counted over the tiles actually walked -- the LIST [0, sinkTiles) ++ [first, last), not n:
                 decode:  34 ceil(ceil(keys of the longest piece / 32) / 4) + pieces + 9
                 prefill: 34 x 2 (sinkEnd + end - begin) + 4
               plus 2 roundings with a sink logit (its exp2 and the sum).
  emulated()   the kernels' roundings and order of sums: sink tiles first, then the window's; a piece's 32-key steps go to the four
               waves in turn by their position in the piece's list; piece 0 folds the sink logit into its (m, l); unsplit launches
               and prefill apply it at the final normalisation.
  needle_queries()  window_model's construction over the visible keys; the first key past the sinks (key S, where it lies below lo),
               the key lo - 1 and the key past the frontier carry weight beta + 4: read, any of them takes the row over.
  mutated()    a named WRONG attention (MUTANTS) and whether the defect changes anything, decided from the geometry alone.
"""
import math

import numpy as np

import decode_model as dm
import window_model as wm

TILE, STEP, WAVES, ROWS = wm.TILE, wm.STEP, wm.WAVES, wm.ROWS
MARGIN = dm.MARGIN     # nothing new is fixed here: decode_model's bound and margin


def library_piece_range(n, rows, window, sinks, pieces, piece):
    from metal_flash_attention_amd import AttentionDecode
    return AttentionDecode.sinkPieceRange(n, rows, window, sinks, pieces, piece)


def library_tile_range(n, qn, r0, RB, causal, window, sinks):
    from metal_flash_attention_amd import AttentionPrefill
    return AttentionPrefill.sinkTileRange(n, qn, r0, RB, window, sinks, causal=causal)


def frontiers(n, qn, rows, W, causal=True):
    """(lo, lim) arrays of the rows `rows`; W = 0: no window"""
    rows = np.asarray(rows, dtype=np.int64)
    if not causal:
        return np.zeros_like(rows), np.full_like(rows, n)
    lo, lim = wm.frontiers(n, qn, rows, W if W else 2 ** 40)
    return lo, lim


def piece_ranges(n, R, W, S, pieces, piece_range=None):
    """[((b0, e0), (b1, e1))] of every piece of a decode launch (one piece: the unsplit kernel's ranges)"""
    fn = piece_range or library_piece_range
    P = int(pieces) if pieces and pieces > 1 else 1
    return [tuple(fn(int(n), int(R), int(W), int(S), P, i)) for i in range(P)]


def steps_of(pair):
    """the 32-key steps of a piece, in the order of its tile list: the sink range, then the window range"""
    return [k0 for b, e in pair for k0 in range(b, e, STEP)]


def chain_decode(pairs, logits):
    per = max([sum(e - b for b, e in pair) for pair in pairs] + [0])
    return 34 * (-(-(-(-per // STEP)) // WAVES)) + len(pairs) + 9 + (2 if logits else 0)


def chain_prefill(sink_end, begin, end, logits):
    return 34 * 2 * (sink_end + end - begin) + 4 + (2 if logits else 0)


def visible_keys(lo, lim, S):
    """the key indices a row with frontiers (lo, lim) sees, ascending"""
    return np.concatenate([np.arange(min(S, lo, lim)), np.arange(min(lo, lim), lim)]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------- the model
def model(q, k, v, lens, qlens, G, W, S=0, logits=None, *, causal=True, pieces=None, kscale=None, vscale=None, piece_range=None,
          tile_range=None):
    """q [B, Hq, R, D], k / v [B, Hkv, C, D] (WITHOUT the scales when kscale / vscale are given), logits [Hq] natural units or None
    -> dm.Reference over [B, Hq, R].  qlens None: a decode launch; otherwise prefill.  Rows at or past qlens[b] hold O = 0, L = -inf,
    bounds 0; so do rows without a visible key when there is no sink logit -- with one they hold O = 0, L = the logit."""
    q, k, v = dm.f64(q), dm.f64(k), dm.f64(v)
    B, Hq, R, D = q.shape
    kind = "decode" if qlens is None else "prefill"
    sink = None if logits is None else np.asarray(logits, dtype=np.float64)
    O, A, E = (np.zeros((B, Hq, R, D)) for _ in range(3))
    L = np.full((B, Hq, R), -np.inf)
    EL = np.zeros((B, Hq, R))
    tr = tile_range or library_tile_range
    for b in range(B):
        n, qn = int(lens[b]), R if qlens is None else min(int(qlens[b]), R)
        if qn == 0:
            continue
        lo, lim = frontiers(n, qn, np.arange(qn), W, causal)
        if kind == "decode":
            chains = {0: chain_decode(piece_ranges(n, R, W, S, pieces, piece_range), sink is not None)}
        else:
            chains = {}
            for r0, _r1 in wm.blocks_of(kind, qn, G):
                bt, _u0, _u1, et, se = tr(n, qn, r0, ROWS // G, causal, W, S)
                chains[r0] = chain_prefill(se, bt, et, sink is not None)
        for r in range(qn):
            idx = visible_keys(int(lo[r]), int(lim[r]), S)
            chain = chains[0] if kind == "decode" else chains[r // (ROWS // G) * (ROWS // G)]
            if idx.size == 0:
                if sink is not None:
                    L[b, :, r] = sink
                    EL[b, :, r] = 4 * dm.U32 * np.abs(sink)
                continue
            ref = dm.model(q[b:b + 1, :, r:r + 1], k[b:b + 1][:, :, idx], v[b:b + 1][:, :, idx], [idx.size], G, False, kscale=kscale, vscale=vscale)
            x = (chain - dm.chain_length(idx.size, None)) * dm.U32
            o0, l0, a0, e0, el0 = ref.O[0, :, 0], ref.L[0, :, 0], ref.A[0, :, 0], ref.E[0, :, 0], ref.EL[0, :, 0]
            w = np.ones(Hq) if sink is None else 1.0 / (1.0 + np.exp(sink - l0))
            O[b, :, r], A[b, :, r] = o0 * w[:, None], a0 * w[:, None]
            L[b, :, r] = l0 if sink is None else np.logaddexp(l0, sink)
            E[b, :, r] = e0 * w[:, None] + x * (A[b, :, r] + np.abs(O[b, :, r]))
            EL[b, :, r] = el0 + x + (0.0 if sink is None else 4 * dm.U32 * (np.abs(sink) + np.abs(L[b, :, r])))
    return dm.Reference(O, L, A, E, EL)


def compare(got_o, got_l, ref, fmt, out, lens, qlens, *, margin=MARGIN, info=None):
    """dm.compare (decode) / over the live rows of every sequence (prefill) -> (worst |dO| / bound, worst |dL| / bound, text).  Unlike
    prefill_model.compare a sequence WITHOUT keys is compared too: with a sink logit its rows have a finite L"""
    if qlens is None:
        return dm.compare(got_o, got_l, ref, fmt, out, lens, margin=margin, info=info)
    worst_o = worst_l = 0.0
    text = ""
    go = dm.f64(got_o)
    gl = None if got_l is None else dm.f64(got_l)
    for b in range(go.shape[0]):
        n, qn = int(lens[b]), min(int(qlens[b]), go.shape[2])
        if qn == 0:
            continue
        sub = dm.Reference(*(x[b:b + 1, :, :qn] for x in ref))
        sinfo = None if info is None else {(0, h, r): v for (bb, h, r), v in info.items() if bb == b}
        wo, wl, t = dm.compare(go[b:b + 1, :, :qn], None if gl is None else gl[b:b + 1, :, :qn], sub, fmt, out, [n], margin=margin, info=sinfo)
        if wo >= worst_o or wl > worst_l:
            text = "sequence %d (qn %d, n %d): %s" % (b, qn, n, t)
        worst_o, worst_l = max(worst_o, wo), max(worst_l, wl)
    return worst_o, worst_l, text


# ------------------------------------------------------------------------------------------------- the rounding-emulated reference
def emulated(q, k, v, lens, qlens, G, W, S, logits, fmt, *, causal=True, pieces=None, kscale=None, vscale=None, piece_range=None,
             tile_range=None, score=None):
    """-> (O before the store's rounding [B, Hq, R, D], L natural): window_model.emulated_walk over the sink tiles, then the window's
    (see the module's text).  score: another score function than the uncapped kernels' (softcap_model's)"""
    R = q.shape[2]

    def visible(n, qn, rows, npad):
        lo, lim = frontiers(n, qn, rows, W, causal)
        cols = np.arange(npad)[None, :]
        return (cols < lim[:, None]) & ((cols >= lo[:, None]) | (cols < S))

    def steps(n, qn, r0):
        if qlens is None:
            return [[steps_of(pair)[w::WAVES] for w in range(WAVES)] for pair in piece_ranges(n, R, W, S, pieces, piece_range)]
        bt, _u0, _u1, et, se = (tile_range or library_tile_range)(n, qn, r0, ROWS // G, causal, W, S)
        return [[list(range(0, se * TILE, STEP)) + list(range(bt * TILE, et * TILE, STEP))]]

    return wm.emulated_walk(q, k, v, lens, qlens, G, fmt, visible, steps, score or wm.scaled_scores(kscale, G, q.shape[3]), logits=logits,
                            vscale=vscale)


# ------------------------------------------------------------------------------------------------------------------ needle inputs
def needle_pool(n, qn, R, G, W, S, kind, pieces=None, page=None, piece_range=None, tile_range=None):
    """keys the geometry makes special: the window's (lo(r) - 1, lo, lo + 1 of the first and last row), the sinks' (0, S - 1, S and
    both sides of every sink tile's edge), both sides of every piece range and of every prefill zone, the page that holds key S, the
    last step's first key, the key before it and the last key"""
    if n <= 0 or qn <= 0:
        return []
    lo, _lim = frontiers(n, qn, np.array([0, qn - 1]), W)
    pool = [int(x) + d for x in lo for d in (-1, 0, 1)] + [0, S - 1, S, S + 1]
    last = (n - 1) // STEP * STEP
    pool += [last, last - 1, n - 1]
    for t in range(1, -(-min(S, n) // TILE) + 1):
        pool += [t * TILE - 1, t * TILE]
    if kind == "decode":
        for pair in piece_ranges(n, R, W, S, pieces, piece_range):
            for pb, pe in pair:
                if pe > pb:
                    pool += [pb - 1, pb, pe - 1, pe]
    else:
        tr = tile_range or library_tile_range
        for r0, _r1 in wm.blocks_of(kind, qn, G):
            bt, u0, u1, et, se = tr(n, qn, r0, ROWS // G, True, W, S)
            if et > bt or se:
                pool += [x * TILE + d for x in (se, bt, u0, u1, et) for d in (-1, 0)] + [(et - 1) * TILE]
    if page and S:
        pool += [S // page * page - 1, S // page * page, S // page * page + page - 1, S // page * page + page]
    return sorted({t for t in pool if 0 <= t < n})


def needle_queries(k, lens, qlens, Hq, G, R, W, S, fmt, *, pieces=None, page=None, piece_range=None, tile_range=None, seed=0):
    """q [B, Hq, R, D] (float64 values of the 16-bit type) and per live (b, h, r) its needles {key: weight} and ONE forbidden key for
    the comparison's text.  Every row carries its frontier and the key before it, the first key of its window and the one after, sink
    key 0 and the last sink key below its window, and its share of needle_pool() among the keys it sees.  The forbidden keys -- key S
    where it lies below lo(r), lo(r) - 1 where it is no sink key, f(r) + 1 below n -- enter q with weight beta + 4."""
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
        pool = needle_pool(n, qn, R, G, W, S, kind, pieces, page, piece_range, tile_range)
        lo, lim = frontiers(n, qn, np.arange(qn), W)
        for h in range(Hq):
            j = h // G
            for r in range(qn):
                a, e = int(lo[r]), int(lim[r])
                seen = visible_keys(a, e, S)
                if seen.size == 0:
                    continue   # (no visible key: the row stays uniform random, its output is the caller's to check)
                sees = set(seen.tolist())
                rho = h * qn + r
                inside = [t for t in pool if t in sees]
                stride = max(1, min(max(2 if len(inside) > 1 else 1, -(-len(inside) // 6)), Hq * qn))
                own = {int(seen[-1]), int(seen[max(seen.size - 2, 0)]), int(seen[0]), min(a, e - 1) if a < e else int(seen[0]),
                       min(a + 1, e - 1) if a < e else int(seen[0]), min(S, a, e) - 1 if min(S, a, e) > 0 else int(seen[0])}
                T = {t for i, t in enumerate(inside) if i % stride == rho % stride} | own
                beta = math.log(seen.size) + 1.0 - math.log(len(T))
                weights = {t: beta + (((t // STEP + rho) % 4) - 1.5) * (2.0 / 3.0) for t in sorted(T)}
                forbidden = [t for t in (S, a - 1, e) if 0 <= t < n and t not in sees]
                vec = np.zeros(D)
                for t, w in list(weights.items()) + [(t, beta + 4.0) for t in dict.fromkeys(forbidden)]:
                    kt = k[b, j, t]
                    vec += w * math.sqrt(D) * kt / max(float(kt @ kt), 1e-30)
                q[b, h, r] = dm.round_to(vec, fmt)
                info[(b, h, r)] = (weights, forbidden[0] if forbidden else None)
    return q, info


# ---------------------------------------------------------------------------------------------------------------------- mutants
MUTANTS = {
    "sinks_one_long": "one sink key too many: c < S + 1",
    "sinks_one_short": "one sink key too few: c < S - 1",
    "sinks_past_frontier": "sink keys admitted past the row's causal frontier: c < min(S, n) in place of c < min(S, lim)",
    "sink_tile_dropped": "the sink tiles [0, sinkTiles) are not walked",
    "gap_walked_unmasked": "the tiles between the sink tiles and the window's first tile are walked, without the lower mask",
    "pieces_over_window_tiles": "decode: the pieces cut over the window's tiles [first, last) only, the sink tiles dropped",
    "second_range_dropped": "decode: a piece that straddles the gap walks its sink range only",
    "parity_from_t_minus_begin": "prefill: the buffer of window tile t taken as (t - begin) & 1: with an odd sinkEnd every window tile is computed from the buffer of the tile walked before it",
    "low_zone_without_sinks": "the window's masked tiles without `c < S`: sink keys inside them are lost",
    "logit_scaled_by_rsqrt_d": "the sink logit multiplied by 1 / sqrt(D)",
    "logit_scaled_by_key_scale": "the sink logit multiplied by the K / V head's keyScale",
    "logit_once_per_piece": "decode: every piece folds the sink logit in, not piece 0 alone",
    "l_without_sink": "L stored without the sink term",
    "blind_row_left": "a live row without a visible key keeps L = -FLT_MAX although a sink logit is bound",
}
L_ONLY = ("l_without_sink", "blind_row_left")   # defects that leave O as it is: they show in L


def _geometry(n, qn, R, G, W, S, kind, r0, r1, mutant, pieces, piece_range, tile_range):
    """what the workgroup of rows [r0, r1) adds up: vis [rows, npad] and, per key, where its K / V rows come from (src, -1: zeros)"""
    npad = (-(-max(n, 1) // TILE) + 1) * TILE
    cols = np.arange(npad)[None, :]
    rows = np.arange(r0, r1)
    lo, lim = frontiers(n, qn, rows, W)
    s = S + 1 if mutant == "sinks_one_long" else max(S - 1, 0) if mutant == "sinks_one_short" else S
    slim = np.full_like(lim, min(s, n)) if mutant == "sinks_past_frontier" else np.minimum(s, lim)
    window = (cols >= lo[:, None]) & (cols < lim[:, None])
    vis = window | (cols < slim[:, None])
    P = int(pieces) if pieces and pieces > 1 else 1
    if kind == "decode":
        pairs = piece_ranges(n, R, W, S, P, piece_range)
        sink_tiles = max([pair[0][1] for pair in pairs] + [0])
        first = min([pair[1][0] for pair in pairs if pair[1][1] > pair[1][0]] + [npad])
        if mutant == "pieces_over_window_tiles" and P > 1:
            pairs = [((0, 0), (b, e)) for b, e in wm._py_piece_ranges(n, first // TILE if first < npad else -(-n // TILE), P)]
        if mutant == "second_range_dropped":
            pairs = [(p0, (p1[0], p1[0]) if p0[1] > p0[0] else p1) for p0, p1 in pairs]
        ranges = [r for pair in pairs for r in pair]
        walk = None
    else:
        bt, u0, u1, et, se = (tile_range or library_tile_range)(n, qn, r0, ROWS // G, True, W, S)
        ranges, sink_tiles, first = [(0, se * TILE), (bt * TILE, min(et * TILE, npad))], se * TILE, bt * TILE
        walk = list(range(se)) + list(range(bt, et))
    loaded = np.zeros(npad, dtype=bool)
    for b, e in ranges:
        loaded[b:e] = True
    if mutant == "sink_tile_dropped":
        loaded[:sink_tiles] = False
    if mutant == "gap_walked_unmasked" and first < npad and first > sink_tiles:
        loaded[sink_tiles:first] = True
        vis[:, sink_tiles:first] = cols[:, sink_tiles:first] < lim[:, None]
    if mutant == "low_zone_without_sinks" and first < npad:
        vis[:, first:] = window[:, first:]
    vis &= loaded[None, :]
    src = np.where(np.arange(npad) < n, np.arange(npad), -1)
    if mutant == "parity_from_t_minus_begin" and walk is not None and sink_tiles // TILE % 2 == 1:
        for at in range(sink_tiles // TILE, len(walk)):
            t, prev = walk[at], walk[at - 1]
            src[t * TILE:(t + 1) * TILE] = np.where(np.arange(prev * TILE, (prev + 1) * TILE) < n, np.arange(prev * TILE, (prev + 1) * TILE), -1)
    return vis, src


def mutated(q, k, v, lens, qlens, G, W, S, logits, mutant, *, pieces=None, page=None, kscale=None, vscale=None, piece_range=None,
            tile_range=None):
    """float64 attention with the named defect (None: without one) -> (O [B, Hq, R, D], L natural [B, Hq, R], changed): `changed` is
    whether any workgroup adds up another set of keys, a visible key from another place, or another sink term than without the defect"""
    assert mutant is None or mutant in MUTANTS, mutant
    q, k, v = dm.f64(q), dm.f64(k), dm.f64(v)
    B, Hq, R, D = q.shape
    Hkv = Hq // G
    kind = "decode" if qlens is None else "prefill"
    ks = np.ones(Hkv) if kscale is None else np.asarray(kscale, dtype=np.float64)
    vs = np.ones(Hkv) if vscale is None else np.asarray(vscale, dtype=np.float64)
    sink = None if logits is None else np.asarray(logits, dtype=np.float64)
    P = int(pieces) if pieces and pieces > 1 else 1
    O = np.zeros((B, Hq, R, D))
    L = np.full((B, Hq, R), -np.inf)
    changed = False
    if sink is not None:
        changed = mutant == "logit_scaled_by_rsqrt_d" or (mutant == "logit_scaled_by_key_scale" and kscale is not None) or \
            (mutant == "logit_once_per_piece" and kind == "decode" and P > 1) or mutant == "l_without_sink"
    for b in range(B):
        n, qn = int(lens[b]), R if qlens is None else min(int(qlens[b]), R)
        if qn == 0:
            continue
        for r0, r1 in wm.blocks_of(kind, qn, G):
            vis, src = _geometry(n, qn, R, G, W, S, kind, r0, r1, mutant, pieces, piece_range, tile_range)
            if mutant is not None:
                vis0, src0 = _geometry(n, qn, R, G, W, S, kind, r0, r1, None, pieces, piece_range, tile_range)
                changed = changed or bool((vis != vis0).any()) or bool((vis.any(axis=0) & (src != src0)).any())
            for h in range(Hq):
                j = h // G
                K = np.where(src[:, None] >= 0, k[b, j][np.clip(src, 0, k.shape[2] - 1)], 0.0)
                V = np.where(src[:, None] >= 0, v[b, j][np.clip(src, 0, k.shape[2] - 1)], 0.0)
                Sc = np.where(vis, (q[b, h, r0:r1] @ K.T) * (ks[j] / math.sqrt(D)), -np.inf)
                m = Sc.max(axis=1, keepdims=True)
                seen = np.isfinite(m[:, 0])
                m0 = np.where(np.isfinite(m), m, 0.0)
                pw = np.exp(Sc - m0)
                l0 = np.where(seen, pw.sum(axis=1), 1.0)
                o = np.where(seen[:, None], (pw / l0[:, None]) @ V * vs[j], 0.0)
                lse = np.where(seen, m0[:, 0] + np.log(l0), -np.inf)
                if sink is not None:
                    s = sink[h]
                    if mutant == "logit_scaled_by_rsqrt_d":
                        s = s / math.sqrt(D)
                    if mutant == "logit_scaled_by_key_scale":
                        s = s * ks[j]
                    if mutant == "logit_once_per_piece" and kind == "decode":
                        s = s + math.log(P)
                    w = 1.0 / (1.0 + np.exp(s - lse))
                    o = o * w[:, None]
                    full = np.logaddexp(lse, s)
                    if mutant == "blind_row_left":
                        changed = changed or bool((~seen).any())
                        full = np.where(seen, full, -np.inf)
                    lse = lse if mutant == "l_without_sink" else full
                O[b, h, r0:r1], L[b, h, r0:r1] = o, lse
    return O, L, changed
