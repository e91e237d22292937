"""The float64 model of prefill CUT ALONG THE KEYS (include/mfa_split.h), with bounds, needle inputs, a rounding-emulated reference and
named mutants at the seams the split adds (a plain module; numpy only).  Formats, bounds and comparison are tests/decode_model.py's; the
rule of visibility, the sink fold and the needle construction tests/sink_model.py's and, with a speculation tree, tests/tree_model.py's;
the walk of a chain and the merge tests/window_model.py's: nothing of them is repeated or edited here.

The launch.  A row block walks the tile list [0, sinkEnd) ++ [begin, end) of ITS OWN five indices (the library's tile-range functions;
with a tree the same list for every row block).  Piece i of P takes the positions [i W / P, (i + 1) W / P) of that list of W tiles
(piece_tiles: the rule written out; library_piece_range: the kernels' own function).  A piece publishes un-normalised (m, l, O); the
combine kernel merges a row's pieces by the weights exp2(m_s - m*), then folds the sink logit and applies the value scale, once.

  model()      sink_model.model (trees: tree_model.model) with the chain term of a split launch in place of the unsplit one.  Counted
               from the code: a piece is one wave's chain over its own tiles, 34 roundings per 32-key step as in prefill_model, and
               the longest piece of a row block has ceil(W / P) tiles = 2 ceil(W / P) steps; prefill16_combine_body then spends, on a
               row's O and l alike, per piece ONE weight (the exp2), ONE product (weight x slab value) and ONE add (into the
               accumulator: the serial adds over a lane's pieces and the log2 of the shuffle tree's are at most P together), and at
               the end the FOUR roundings of the unsplit normalisation (the sum of l, 1 / l, the value scale, the product), plus the
               sink logit's two (its exp2 and the sum):
                 chain_split = 34 x 2 ceil(W / P) + 3 P + 4 (+ 2)        against        34 x 2 W + 4 (+ 2)  unsplit.
               O, L and A are the unsplit model's exactly; E and EL move by (chain_split - chain_unsplit) x 2^-24.
  emulated()   the kernels' roundings and order of sums: every piece is window_model._walk over the 32-key steps of its tiles in list
               order (P rounded to the 16-bit type against the running maximum), the pieces merge in list order by exp2(m_s - m*)
               (window_model._merge), THEN the sink logit folds and the value scale multiplies.
  needle_queries()  sink_model's / tree_model's construction with the keys either side of every piece boundary of every row block
               added to the pool: the last key of the tile before a boundary and the first key of the tile after it.
  mutated()    a named WRONG split attention (MUTANTS), float64, piece by piece, and whether the defect changes anything.

MARGIN is decode_model's: nothing new is fixed here.
"""
import contextlib
import math

import numpy as np

import decode_model as dm
import sink_model as sm
import tree_model as tm
import window_model as wm

TILE, STEP, ROWS = sm.TILE, sm.STEP, sm.ROWS
MARGIN = dm.MARGIN
SENTINEL = -7.25          # what the rows at or past qn of mutated()'s outputs hold: a launch leaves them alone
MAX_PIECES = 64


def library_piece_range(begin, end, sink_end, pieces, piece):
    from metal_flash_attention_amd import AttentionPrefill
    return AttentionPrefill.pieceRange(begin, end, sink_end, pieces, piece)


def python_piece_range(begin, end, sink_end, pieces, piece):
    """the rule of include/mfa_split.h, written out: ((b0, e0) inside the sink tiles, (b1, e1) inside [begin, end))"""
    W = sink_end + end - begin
    t0, t1 = piece * W // pieces, (piece + 1) * W // pieces
    return (min(t0, sink_end), min(t1, sink_end)), (begin + max(t0 - sink_end, 0), begin + max(t1 - sink_end, 0))


def walked_list(sink_end, begin, end):
    return list(range(sink_end)) + list(range(begin, end))


def piece_tiles(sink_end, begin, end, pieces, piece_range=None):
    """[piece] -> its tiles, in the order walked"""
    fn = piece_range or python_piece_range
    out = []
    for i in range(pieces):
        (b0, e0), (b1, e1) = fn(begin, end, sink_end, pieces, i)
        out.append(list(range(b0, e0)) + list(range(b1, e1)))
    return out


def block_range(n, qn, r0, G, causal, W, S, tree):
    """(sinkEnd, begin, end) of the row block at r0: the library's own tile ranges"""
    if tree:
        bt, _u0, _u1, et, se = tm.library_tree_tile_range(n, qn, W, S)
    else:
        bt, _u0, _u1, et, se = sm.library_tile_range(n, qn, r0, ROWS // G, causal, W, S)
    return se, bt, et


def chain_split(sink_end, begin, end, pieces, logits):
    tiles = sink_end + end - begin
    return 34 * 2 * (-(-tiles // pieces)) + 3 * pieces + 4 + (2 if logits else 0)


def _visible_row(n, qn, r, b, W, S, causal, masks):
    if masks is not None:
        return tm.visible_row(n, qn, tm.row_mask(masks, b, r), W, S)
    lo, lim = sm.frontiers(n, qn, np.array([r]), W, causal)
    return sm.visible_keys(int(lo[0]), int(lim[0]), S)


# ---------------------------------------------------------------------------------------------------------------------- the model
def model(q, k, v, lens, qlens, G, W, S, logits, pieces, *, causal=True, masks=None, kscale=None, vscale=None):
    """-> dm.Reference over [B, Hq, R]: the unsplit model with the split launch's chain term (see the module's text)"""
    return rechained(unsplit_model(q, k, v, lens, qlens, G, W, S, logits, causal=causal, masks=masks, kscale=kscale, vscale=vscale),
                     lens, qlens, G, W, S, logits, pieces, causal=causal, masks=masks)


def unsplit_model(q, k, v, lens, qlens, G, W, S, logits, *, causal=True, masks=None, kscale=None, vscale=None):
    """the model of the launch that is not cut: tree_model's with masks, else sink_model's (which a caller may share among piece counts)"""
    if masks is not None:
        return tm.model(q, k, v, lens, qlens, G, W, S, logits, masks, kscale=kscale, vscale=vscale)
    return sm.model(q, k, v, lens, qlens, G, W, S, logits, causal=causal, kscale=kscale, vscale=vscale)


def rechained(base, lens, qlens, G, W, S, logits, pieces, *, causal=True, masks=None):
    """`base` (unsplit_model's) with the chain term of a launch in `pieces` pieces in place of the unsplit one; `base` is not modified"""
    E, EL = base.E.copy(), base.EL.copy()
    R = E.shape[2]
    for b in range(E.shape[0]):
        n, qn = int(lens[b]), min(int(qlens[b]), R)
        for r0, r1 in wm.blocks_of("prefill", qn, G):
            se, bt, et = block_range(n, qn, r0, G, causal, W, S, masks is not None)
            delta = (chain_split(se, bt, et, pieces, logits is not None) - sm.chain_prefill(se, bt, et, logits is not None)) * dm.U32
            for r in range(r0, r1):
                if _visible_row(n, qn, r, b, W, S, causal, masks).size:
                    E[b, :, r] += delta * (base.A[b, :, r] + np.abs(base.O[b, :, r]))
                    EL[b, :, r] += delta
    assert (E >= 0).all() and (EL >= 0).all()
    return dm.Reference(base.O, base.L, base.A, E, EL)


compare = sm.compare
bounds = dm.bounds


def _mask_of(n, qn, rows, b, W, S, causal, masks, npad):
    out = np.zeros((len(rows), npad), dtype=bool)
    for i, r in enumerate(rows):
        out[i, _visible_row(n, qn, int(r), b, W, S, causal, masks)] = True
    return out


# ------------------------------------------------------------------------------------------------- the rounding-emulated reference
def emulated(q, k, v, lens, qlens, G, W, S, logits, pieces, fmt, *, causal=True, masks=None, kscale=None, vscale=None, piece_range=None):
    """-> (O before the store's rounding [B, Hq, R, D], L natural): see the module's text"""
    q, k, v = dm.f64(q), dm.f64(k), dm.f64(v)
    B, Hq, R, D = q.shape
    vs = np.ones(Hq // G) if vscale is None else np.asarray(vscale, dtype=np.float64)
    score = wm.scaled_scores(kscale, G, D)
    O = np.zeros((B, Hq, R, D))
    L = np.full((B, Hq, R), -np.inf)
    for b in range(B):
        n, qn = int(lens[b]), min(int(qlens[b]), R)
        npad = (-(-max(n, 1) // TILE)) * TILE
        for r0, r1 in wm.blocks_of("prefill", qn, G):
            vis = _mask_of(n, qn, np.arange(r0, r1), b, W, S, causal, masks, npad)
            se, bt, et = block_range(n, qn, r0, G, causal, W, S, masks is not None)
            lists = piece_tiles(se, bt, et, pieces, piece_range)
            for h in range(Hq):
                j = h // G
                K, V = np.zeros((npad, D)), np.zeros((npad, D))
                K[:n], V[:n] = k[b, j, :n], v[b, j, :n]
                S2 = score(q[b, h, r0:r1] @ K.T, vis, b, h, slice(r0, r1))
                parts = [wm._walk(S2, V, [t * TILE + half for t in tiles for half in (0, STEP)], fmt) for tiles in lists]
                mstar, lt, ot = wm._merge(parts)
                if logits is not None:
                    mstar, lt, ot = wm._fold((mstar, lt, ot), np.full(r1 - r0, float(logits[h]) * dm.LOG2E))
                seen = lt > 0
                l0 = np.where(seen, lt, 1.0)
                O[b, h, r0:r1] = np.where(seen[:, None], ot * vs[j] / l0[:, None], 0.0)
                L[b, h, r0:r1] = np.where(seen, (np.where(seen, mstar, 0.0) + np.log2(l0)) / dm.LOG2E, -np.inf)
    return O, L


# ------------------------------------------------------------------------------------------------------------------ needle inputs
def boundary_keys(n, qn, G, causal, W, S, pieces, tree, piece_range=None):
    """the keys either side of every piece boundary of every row block of a sequence; pieces: a count, or several (one q for all)"""
    pool = []
    for r0, _r1 in wm.blocks_of("prefill", qn, G):
        se, bt, et = block_range(n, qn, r0, G, causal, W, S, tree)
        for count in (pieces if isinstance(pieces, (tuple, list)) else (pieces,)):
            for tiles in piece_tiles(se, bt, et, count, piece_range):
                if tiles:
                    pool += [tiles[0] * TILE - 1, tiles[0] * TILE, tiles[-1] * TILE + TILE - 1, (tiles[-1] + 1) * TILE]
    return sorted({t for t in pool if 0 <= t < n})


@contextlib.contextmanager
def _pool_with_boundaries(G, causal, W, S, pieces, tree, piece_range):
    """sink_model.needle_pool (which tree_model's construction calls too) plus boundary_keys(), for the time of one construction"""
    plain = sm.needle_pool

    def pool(n, qn, R, G_, W_, S_, kind, *args, **kw):
        return sorted(set(plain(n, qn, R, G_, W_, S_, kind, *args, **kw)) | set(boundary_keys(n, qn, G, causal, W, S, pieces, tree, piece_range)))
    sm.needle_pool = pool
    try:
        yield
    finally:
        sm.needle_pool = plain


def needle_queries(k, lens, qlens, Hq, G, R, W, S, fmt, pieces, *, masks=None, page=None, piece_range=None, seed=0):
    """q and info as sink_model.needle_queries / tree_model.needle_queries give them, the pool widened by the piece boundaries"""
    with _pool_with_boundaries(G, True, W, S, pieces, masks is not None, piece_range):
        if masks is not None:
            return tm.needle_queries(k, lens, qlens, Hq, G, R, W, S, masks, fmt, page=page, seed=seed)
        return sm.needle_queries(k, lens, qlens, Hq, G, R, W, S, fmt, page=page, seed=seed)


# ---------------------------------------------------------------------------------------------------------------------- mutants
MUTANTS = {
    "piece_one_tile_short": "every piece but the last stops one tile early: the tile in front of a boundary is dropped.  Nothing changes where "
                            "no such piece holds a tile with a visible key in it",
    "piece_one_tile_long": "every piece but the last walks the next piece's first tile too: that tile is counted twice.  Nothing changes "
                           "where that tile holds no visible key",
    "pieces_from_sequence_begin": "the pieces laid from the SEQUENCE's first tile (the first row block's `begin`) instead of the block's own: a "
                                  "later row block under a window walks tiles below its window and loses as many at its frontier.  Nothing "
                                  "changes where every row block starts at the same tile (no window, one row block, a tree)",
    "weight_left_out": "the combine sums the pieces' O and l without the weights exp2(m_s - m*).  Nothing changes for a row with one piece that saw a key",
    "weight_of_next_piece": "piece s merged with the weight of piece s + 1 (the last with its own).  Nothing changes for a row with one "
                            "piece that saw a key",
    "l_unweighted": "O merged with the weights, l summed without them.  Nothing changes for a row with one piece that saw a key",
    "logit_once_per_piece": "every piece folds the sink logit in: the denominator holds it P times.  Nothing changes without sink logits",
    "logit_lost_when_piece_0_empty": "piece 0 folds the sink logit, and a piece without a tile publishes nothing of it: the logit is lost where the "
                                     "row block has fewer tiles than pieces.  Nothing changes without sink logits or where piece 0 has a tile",
    "value_scale_twice": "the value scale applied by the pieces and by the combine kernel.  Nothing changes without value scales",
    "empty_piece_read": "the O slab of a piece whose l is 0 read as if written: 0 x NaN.  Nothing changes where every piece of every live row saw a key",
    "dead_rows_written": "rows at or past queryLengths[b] merged and written.  Nothing changes where every sequence has `rows` rows",
}
DEAD_ONLY = ("dead_rows_written",)   # defects that leave the live rows alone: they show in the rows past qn


def _mutant_lists(n, qn, r0, G, causal, W, S, pieces, tree, mutant):
    se, bt, et = block_range(n, qn, r0, G, causal, W, S, tree)
    lists = piece_tiles(se, bt, et, pieces)
    walk = walked_list(se, bt, et)
    if mutant == "piece_one_tile_short":
        lists = [tiles[:-1] if i < pieces - 1 else tiles for i, tiles in enumerate(lists)]
    if mutant == "piece_one_tile_long":
        ends = np.cumsum([len(t) for t in lists])
        lists = [tiles + (walk[ends[i]:ends[i] + 1] if i < pieces - 1 else []) for i, tiles in enumerate(lists)]
    if mutant == "pieces_from_sequence_begin" and not tree:
        _se0, bt0, _et0 = block_range(n, qn, 0, G, causal, W, S, tree)
        lists = [[t if t < se else t - (bt - bt0) for t in tiles] for tiles in lists]   # (sinkEnd <= begin: t < sinkEnd is a sink tile)
    return lists, se, bt, et


def mutated(q, k, v, lens, qlens, G, W, S, logits, pieces, mutant, *, causal=True, masks=None, kscale=None, vscale=None):
    """float64 split attention with the named defect (None: without one) -> (O [B, Hq, R, D], L natural [B, Hq, R], changed).  Rows at or
    past qn hold SENTINEL unless the defect writes them.  `changed`: whether the defect changes what any live row sums, merges or folds,
    or (DEAD_ONLY) what a dead row holds"""
    assert mutant is None or mutant in MUTANTS, mutant
    q, k, v = dm.f64(q), dm.f64(k), dm.f64(v)
    B, Hq, R, D = q.shape
    Hkv = Hq // G
    ks = np.ones(Hkv) if kscale is None else np.asarray(kscale, dtype=np.float64)
    vs = np.ones(Hkv) if vscale is None else np.asarray(vscale, dtype=np.float64)
    sink = None if logits is None else np.asarray(logits, dtype=np.float64)
    tree = masks is not None
    O = np.full((B, Hq, R, D), SENTINEL)
    L = np.full((B, Hq, R), SENTINEL)
    changed = False
    if mutant == "logit_once_per_piece":
        changed = sink is not None and any(min(int(x), R) > 0 for x in qlens)
    if mutant == "value_scale_twice":
        changed = vscale is not None and bool((vs != 1.0).any())
    for b in range(B):
        n, qn = int(lens[b]), min(int(qlens[b]), R)
        if mutant == "dead_rows_written" and qn < R:
            changed = True
            O[b, :, qn:], L[b, :, qn:] = 0.0, -np.inf   # (slabs nobody wrote: whatever they hold, the sentinel is gone)
        npad = (-(-max(n, 1) // TILE) + 1) * TILE
        for r0, r1 in wm.blocks_of("prefill", qn, G):
            vis = _mask_of(n, qn, np.arange(r0, r1), b, W, S, causal, masks, npad)
            lists, se, bt, et = _mutant_lists(n, qn, r0, G, causal, W, S, pieces, tree, mutant)
            lists0 = piece_tiles(se, bt, et, pieces)
            count = lambda ls: np.stack([sum((vis[:, t * TILE:(t + 1) * TILE].sum(axis=1) for t in tiles), np.zeros(r1 - r0)) for tiles in ls])  # noqa: E731
            seen0 = count(lists0)            # [piece][row]: visible keys the row sums in the piece, without the defect
            if mutant in ("piece_one_tile_short", "piece_one_tile_long", "pieces_from_sequence_begin"):
                tiles_of = lambda ls: [sorted(t for t in tiles if vis[:, t * TILE:(t + 1) * TILE].any()) for tiles in ls]  # noqa: E731
                changed = changed or tiles_of(lists) != tiles_of(lists0)
            if mutant in ("weight_left_out", "weight_of_next_piece", "l_unweighted"):
                changed = changed or bool(((seen0 > 0).sum(axis=0) > 1).any())
            if mutant == "logit_lost_when_piece_0_empty":
                changed = changed or (sink is not None and not lists0[0])
            if mutant == "empty_piece_read":
                changed = changed or bool((seen0 == 0).any())
            for h in range(Hq):
                j = h // G
                K, V = np.zeros((npad, D)), np.zeros((npad, D))
                K[:n], V[:n] = k[b, j, :n], v[b, j, :n]
                Sc = np.where(vis, (q[b, h, r0:r1] @ K.T) * (ks[j] / math.sqrt(D)), -np.inf)
                parts = []
                for tiles in lists:
                    cols = np.array([t * TILE + c for t in tiles for c in range(TILE)], dtype=np.int64)
                    s = Sc[:, cols] if cols.size else np.full((r1 - r0, 1), -np.inf)
                    m = s.max(axis=1)
                    m0 = np.where(np.isfinite(m), m, 0.0)
                    p = np.exp(s - m0[:, None])
                    parts.append((m, p.sum(axis=1), p @ V[cols] if cols.size else np.zeros((r1 - r0, D))))
                mstar = np.max(np.stack([m for m, _l, _o in parts]), axis=0)
                ms0 = np.where(np.isfinite(mstar), mstar, 0.0)
                weights = [np.where(np.isfinite(m), np.exp(np.where(np.isfinite(m), m, 0.0) - ms0), 0.0) for m, _l, _o in parts]
                if mutant == "weight_of_next_piece":
                    weights = weights[1:] + weights[-1:]
                lt, ot = np.zeros(r1 - r0), np.zeros((r1 - r0, D))
                for (m, l, o), w in zip(parts, weights):
                    live = l > 0
                    wo = np.where(live, 1.0, 0.0) if mutant == "weight_left_out" else w
                    wl = np.where(live, 1.0, 0.0) if mutant in ("weight_left_out", "l_unweighted") else w
                    lt += wl * l
                    ot += wo[:, None] * o
                    if mutant == "empty_piece_read":
                        ot = np.where(live[:, None], ot, np.nan)
                seen = lt > 0
                l0 = np.where(seen, lt, 1.0)
                o = np.where(seen[:, None], ot / l0[:, None] * vs[j], np.where(np.isnan(ot), np.nan, 0.0))
                if mutant == "value_scale_twice":
                    o = o * vs[j]
                lse = np.where(seen, ms0 + np.log(l0), -np.inf)
                if sink is not None and not (mutant == "logit_lost_when_piece_0_empty" and not lists0[0]):
                    s = sink[h] + (math.log(pieces) if mutant == "logit_once_per_piece" else 0.0)
                    o = o * (1.0 / (1.0 + np.exp(s - lse)))[:, None]
                    lse = np.logaddexp(lse, s)
                O[b, h, r0:r1], L[b, h, r0:r1] = o, lse
    return O, L, changed


def dead_rows_untouched(O, L, qlens):
    """the hygiene check of the GPU tests, on mutated()'s outputs: rows at or past qn hold the sentinel"""
    R = O.shape[2]
    return all(bool((O[b, :, min(int(qn), R):] == SENTINEL).all()) and bool((L[b, :, min(int(qn), R):] == SENTINEL).all()) for b, qn in enumerate(qlens))
