"""The float64 model of speculation trees over a KV cache (include/mfa_tree.h), decode and prefill, with bounds, needle inputs, a
rounding-emulated reference and named mutants (a plain module; numpy only).  Formats, bounds and comparison are tests/decode_model.py's;
the sink fold, the piece ranges, the chain counts and the walk of the emulation tests/sink_model.py's and tests/window_model.py's:
nothing of them is repeated or edited here.

The rule.  n keys, qn new rows, P = max(n - qn, 0), live = min(qn, n); row r carries mask_r = masks[b][r] & (2^live - 1) and
d_r = max(popcount(mask_r), 1).  It sees the PREFIX key c < P iff there is no window, or c >= max(P + d_r, W) - W, or c < S, and the
NEW-TOKEN key P <= c < n iff bit c - P of mask_r is set -- whatever r and c - P.  The sink logit, the scales and the blind rows are
sink_model's.

  model()      row r's attention IS decode_model.model over its visible keys, one row at a time, then sink_model's fold.  The CHAIN
               term is counted over the tiles walked: decode sink_model's (the piece plan does not change), prefill
               34 x 2 (sinkEnd + end - begin) + 4 over the tiles of the TREE range, which every row block walks.  With the chain mask
               O, L and A are sink_model.model's exactly, and E / EL too wherever the walks agree (one row block per sequence).
  emulated()   window_model.emulated_walk over the tree's visible keys and walked steps.
  needle_queries()  needles on the keys the geometry makes special (the row's own node, its deepest and its first ancestor, the last
               prefix key, its window's first key, sink key 0); the keys it must NOT see -- the neighbours of its mask's bits among the
               new tokens, node 0 and the node below its own where their bits are clear, the key below its window -- enter q with weight
               beta + 4: read, any of them takes the row over.
  mutated()    a named WRONG tree attention (MUTANTS), float64, and whether the defect changes what any row sees.

MARGIN is decode_model's: nothing new is fixed here.
"""
import math

import numpy as np

import decode_model as dm
import sink_model as sm
import window_model as wm

TILE, STEP, WAVES, ROWS = sm.TILE, sm.STEP, sm.WAVES, sm.ROWS
MARGIN = dm.MARGIN     # nothing new is fixed here: decode_model's bound and margin
FULL = (1 << 64) - 1


def library_tree_tile_range(n, qn, window, sinks):
    from metal_flash_attention_amd import AttentionPrefill
    return AttentionPrefill.treeTileRange(n, qn, window, sinks)


def python_tree_tile_range(n, qn, W, S):
    """the range of include/mfa_tree.h, written out: (begin, unmaskedBegin, unmaskedEnd, end, sinkEnd)"""
    if n == 0 or qn == 0:
        return (0, 0, 0, 0, 0)
    P, live = max(n - qn, 0), min(qn, n)
    lo = lambda f: (max(f, W) - W) if W else 0   # noqa: E731
    b, e = lo(P + 1) // TILE, -(-n // TILE)
    u0, u1 = -(-lo(P + live) // TILE), P // TILE
    if u0 >= u1:
        u0 = u1 = b
    return (b, u0, u1, e, min(-(-min(S, P) // TILE), b))


# ---------------------------------------------------------------------------------------------------------------------- trees
def chain(R, B=None):
    """mask_r = 2^(r + 1) - 1: today's causal rule"""
    row = np.array([(1 << (r + 1)) - 1 for r in range(R)], dtype=np.uint64)
    return row if B is None else np.tile(row, (B, 1))


def random_tree(R, rng):
    """node 0 is the root, node j's parent is uniform among the earlier nodes: mask_j = mask_parent | 2^j"""
    masks = [1]
    for j in range(1, R):
        masks.append(masks[int(rng.integers(0, j))] | (1 << j))
    return np.array(masks, dtype=np.uint64)


def forest(R, rng, roots=0.3):
    """several roots: a node is a root -- it sees only itself -- with probability `roots`, else a child of an earlier node"""
    masks = [1]
    for j in range(1, R):
        masks.append((1 << j) if rng.random() < roots else masks[int(rng.integers(0, j))] | (1 << j))
    return np.array(masks, dtype=np.uint64)


def arbitrary(R, rng):
    """any bits, j > r included, and bits at or past R that the kernels must ignore; every fifth row sees no new token at all"""
    out = rng.integers(0, 1 << 63, R, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, R, dtype=np.uint64)
    out[4::5] &= np.uint64(FULL ^ ((1 << R) - 1) if R < 64 else 0)
    return out


def per_sequence(make, B, R, seed):
    """[B, R] uint64: another tree for every sequence"""
    return np.stack([make(R, np.random.default_rng(seed + 17 * b)) for b in range(B)])


def row_mask(masks, b, r):
    """the mask of row r of sequence b as a Python int; masks [R] (one tree for all) or [B, R]"""
    m = np.asarray(masks)
    return int(m[r]) if m.ndim == 1 else int(m[b, r])


# ------------------------------------------------------------------------------------------------------------------ visibility
def geometry(n, qn):
    return max(n - qn, 0), min(qn, n)


def window_start(P, d, W):
    return (max(P + d, W) - W) if W else 0


def visible_row(n, qn, mask, W, S):
    """the ascending key indices a row with `mask` sees"""
    P, live = geometry(n, qn)
    mask &= (1 << live) - 1
    d = max(bin(mask).count("1"), 1)
    lo = window_start(P, d, W)
    prefix = [c for c in range(min(S, lo, P))] + list(range(min(lo, P), P))
    return np.array(prefix + [P + j for j in range(live) if mask >> j & 1], dtype=np.int64)


def visible(n, qn, rows, masks_of, W, S, npad):
    """bool [rows, npad]; masks_of(r) -> the row's mask"""
    out = np.zeros((len(rows), npad), dtype=bool)
    for i, r in enumerate(rows):
        out[i, visible_row(n, qn, masks_of(int(r)), W, S)] = True
    return out


def chains_of(kind, n, qn, R, G, W, S, pieces, logits, piece_range, tree_range):
    if kind == "decode":
        return sm.chain_decode(sm.piece_ranges(n, R, W, S, pieces, piece_range), logits)
    bt, _u0, _u1, et, se = (tree_range or library_tree_tile_range)(n, qn, W, S)
    return sm.chain_prefill(se, bt, et, logits)


# ---------------------------------------------------------------------------------------------------------------------- the model
def model(q, k, v, lens, qlens, G, W, S, logits, masks, *, pieces=None, kscale=None, vscale=None, piece_range=None, tree_range=None):
    """q [B, Hq, R, D], k / v [B, Hkv, C, D] (WITHOUT the scales when kscale / vscale are given), logits [Hq] natural units or None,
    masks [R] or [B, R] uint64 -> dm.Reference over [B, Hq, R].  qlens None: a decode launch.  (sink_model.model's arithmetic, row by row)"""
    q, k, v = dm.f64(q), dm.f64(k), dm.f64(v)
    B, Hq, R, D = q.shape
    kind = "decode" if qlens is None else "prefill"
    sink = None if logits is None else np.asarray(logits, dtype=np.float64)
    O, A, E = (np.zeros((B, Hq, R, D)) for _ in range(3))
    L = np.full((B, Hq, R), -np.inf)
    EL = np.zeros((B, Hq, R))
    for b in range(B):
        n, qn = int(lens[b]), R if qlens is None else min(int(qlens[b]), R)
        if qn == 0:
            continue
        chain_b = chains_of(kind, n, qn, R, G, W, S, pieces, sink is not None, piece_range, tree_range)
        for r in range(qn):
            idx = visible_row(n, qn, row_mask(masks, b, r), W, S)
            if idx.size == 0:
                if sink is not None:
                    L[b, :, r] = sink
                    EL[b, :, r] = 4 * dm.U32 * np.abs(sink)
                continue
            ref = dm.model(q[b:b + 1, :, r:r + 1], k[b:b + 1][:, :, idx], v[b:b + 1][:, :, idx], [idx.size], G, False, kscale=kscale, vscale=vscale)
            x = (chain_b - dm.chain_length(idx.size, None)) * dm.U32
            o0, l0, a0, e0, el0 = ref.O[0, :, 0], ref.L[0, :, 0], ref.A[0, :, 0], ref.E[0, :, 0], ref.EL[0, :, 0]
            w = np.ones(Hq) if sink is None else 1.0 / (1.0 + np.exp(sink - l0))
            O[b, :, r], A[b, :, r] = o0 * w[:, None], a0 * w[:, None]
            L[b, :, r] = l0 if sink is None else np.logaddexp(l0, sink)
            E[b, :, r] = e0 * w[:, None] + x * (A[b, :, r] + np.abs(O[b, :, r]))
            EL[b, :, r] = el0 + x + (0.0 if sink is None else 4 * dm.U32 * (np.abs(sink) + np.abs(L[b, :, r])))
    return dm.Reference(O, L, A, E, EL)


bounds = dm.bounds
compare = sm.compare


def blind(masks, lens, qlens, R, W, S):
    """cache_kit.hold's rule of the rows without a visible key: rows(b, n, qn) -> bool [qn]"""
    def rows(b, n, qn):
        return np.array([visible_row(n, qn, row_mask(masks, b, r), W, S).size == 0 for r in range(qn)])
    return rows


# ------------------------------------------------------------------------------------------------- the rounding-emulated reference
def emulated(q, k, v, lens, qlens, G, W, S, logits, masks, fmt, *, pieces=None, kscale=None, vscale=None, piece_range=None, tree_range=None):
    """-> (O before the store's rounding [B, Hq, R, D], L natural): window_model.emulated_walk, one sequence at a time (its callbacks do
    not say which sequence they serve), over the tree's visible keys; decode walks sink_model's pieces, every prefill row block the tiles
    of the tree range"""
    B, _Hq, R, D = q.shape
    outs = []
    for b in range(B):
        def vis(n, qn, rows, npad, b=b):
            return visible(n, qn, rows, lambda r: row_mask(masks, b, r), W, S, npad)

        def steps(n, qn, r0):
            if qlens is None:
                return [[sm.steps_of(pair)[w::WAVES] for w in range(WAVES)] for pair in sm.piece_ranges(n, R, W, S, pieces, piece_range)]
            bt, _u0, _u1, et, se = (tree_range or library_tree_tile_range)(n, qn, W, S)
            return [[list(range(0, se * TILE, STEP)) + list(range(bt * TILE, et * TILE, STEP))]]

        outs.append(wm.emulated_walk(q[b:b + 1], k[b:b + 1], v[b:b + 1], lens[b:b + 1], None if qlens is None else qlens[b:b + 1], G, fmt, vis, steps,
                                     wm.scaled_scores(kscale, G, D), logits=logits, vscale=vscale))
    return np.concatenate([o for o, _l in outs]), np.concatenate([l for _o, l in outs])


# ------------------------------------------------------------------------------------------------------------------ needle inputs
def forbidden_keys(n, qn, r, mask, W, S):
    """keys of the sequence the row must not see, most telling first: the new tokens beside its mask's bits, node 0, the node below its
    own and the one above it where their bits are clear, and the key below its window where that is no sink key"""
    P, live = geometry(n, qn)
    mask &= (1 << live) - 1
    sees = set(visible_row(n, qn, mask, W, S).tolist())
    bits = [j for j in range(live) if mask >> j & 1]
    near = [j + d for j in bits[-2:] + bits[:1] for d in (1, -1)] + [0, r - 1, r + 1, live - 1]
    lo = window_start(P, max(len(bits), 1), W)
    keys = [P + j for j in near if 0 <= j < live] + [lo - 1, S]
    return [c for c in dict.fromkeys(keys) if 0 <= c < n and c not in sees]


def needle_queries(k, lens, qlens, Hq, G, R, W, S, masks, fmt, *, pieces=None, page=None, seed=0):
    """q [B, Hq, R, D] (float64 values of the 16-bit type) and per live (b, h, r) its needles {key: weight} and ONE forbidden key for
    the comparison's text (sink_model.needle_queries' construction over the tree's visible keys)"""
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
        P, live = geometry(n, qn)
        pool = sm.needle_pool(n, qn, R, G, W, S, kind, pieces, page) + [P - 1, P, n - 1]
        for r in range(qn):
            mask = row_mask(masks, b, r) & ((1 << live) - 1)
            seen = visible_row(n, qn, mask, W, S)
            if seen.size == 0:
                continue   # (no visible key: the row stays uniform random, its output is the caller's to check)
            sees = set(seen.tolist())
            bits = [P + j for j in range(live) if mask >> j & 1]
            lo = window_start(P, max(len(bits), 1), W)
            own = {int(seen[-1]), int(seen[0])} | set(bits[-3:]) | set(bits[:1]) | ({P + r} & sees) | ({P - 1, lo, lo + 1, 0, min(S, lo) - 1} & sees)
            forbidden = forbidden_keys(n, qn, r, mask, W, S)[:4]
            inside = [t for t in sorted(set(pool)) if t in sees]
            for h in range(Hq):
                j = h // G
                rho = h * qn + r
                stride = max(1, min(max(2 if len(inside) > 1 else 1, -(-len(inside) // 6)), Hq * qn))
                T = {t for i, t in enumerate(inside) if i % stride == rho % stride} | own
                beta = math.log(seen.size) + 1.0 - math.log(len(T))
                weights = {t: beta + (((t // STEP + rho) % 4) - 1.5) * (2.0 / 3.0) for t in sorted(T)}
                vec = np.zeros(D)
                for t, w in list(weights.items()) + [(t, beta + 4.0) for t in forbidden]:
                    kt = k[b, j, t]
                    vec += w * math.sqrt(D) * kt / max(float(kt @ kt), 1e-30)
                q[b, h, r] = dm.round_to(vec, fmt)
                info[(b, h, r)] = (weights, forbidden[0] if forbidden else None)
    return q, info


# ---------------------------------------------------------------------------------------------------------------------- mutants
MUTANTS = {
    "causal_instead_of_mask": "the causal rule among the new tokens: row r sees node j iff j <= r",
    "bit_one_key_late": "bit j tested against key P + j + 1",
    "bit_one_key_early": "bit j tested against key P + j - 1",
    "mask_of_packed_row": "the mask indexed by the lane's packed row (head x rows + row) instead of its row: wrong for every head but the group's first",
    "mask_of_batch_0": "batch 0's masks for every sequence",
    "high_word_dropped": "prefill: the low 32 bits of the mask only",
    "frontier_from_row_index": "the window's frontier taken from the row's index, P + r + 1, instead of its depth",
    "key_p_unmasked": "unmaskedEnd = floor((P + 1) / 64): where (P + 1) % 64 = 0 the tile that ends with key P runs unmasked and every row sees key P",
    "bits_past_live": "bits at or past `live` honoured: they name rows past the keys, read as zeros, and count into the depth",
    "causal_end_tile": "prefill: a row block stops at the tile of its last row's own key, as the causal launch does",
}
PREFILL_ONLY = ("high_word_dropped", "causal_end_tile")


def _mutant_visible(n, qn, R, G, kind, r0, r1, h, b, masks, W, S, mutant, npad):
    """bool [r1 - r0, npad] of what query head h's rows r0 .. r1 - 1 add up under the defect; keys at or past n come in as zeros"""
    P, live = geometry(n, qn)
    flat = np.asarray(masks).reshape(-1)
    stride = 0 if np.asarray(masks).ndim == 1 else np.asarray(masks).shape[1]
    out = np.zeros((r1 - r0, npad), dtype=bool)
    RB = qn if kind == "decode" else ROWS // G
    for i, r in enumerate(range(r0, r1)):
        at = (0 if mutant == "mask_of_batch_0" else b) * stride + r
        if mutant == "mask_of_packed_row":
            at = b * stride + ((h % G) * R + r if kind == "decode" else r0 + (h % G) * RB + (r - r0))
        raw = int(flat[at % flat.size])
        if mutant == "high_word_dropped" and kind == "prefill":
            raw &= 0xFFFFFFFF
        mask = raw if mutant == "bits_past_live" else raw & ((1 << live) - 1)
        if mutant == "bits_past_live" and kind == "decode":
            mask &= 0xFFFFFFFF   # (decode holds the low word)
        d = max(bin(mask).count("1"), 1)
        lo = window_start(P, r + 1 if mutant == "frontier_from_row_index" else d, W)
        out[i, :min(S, lo, P)] = True
        out[i, min(lo, P):P] = True
        shift = {"bit_one_key_late": 1, "bit_one_key_early": -1}.get(mutant, 0)
        for j in range(64):
            c = P + j + shift
            if mutant == "causal_instead_of_mask":
                on = j <= r and j < live
            else:
                on = bool(mask >> j & 1)
            if on and P <= c < npad and (c < n or mutant == "bits_past_live"):
                out[i, c] = True
        if mutant == "key_p_unmasked" and (P + 1) % TILE == 0 and P < n:
            out[i, P] = True
    if mutant == "causal_end_tile" and kind == "prefill":
        out[:, -(-min(n, P + r1) // TILE) * TILE:] = False
    return out


def mutated(q, k, v, lens, qlens, G, W, S, logits, masks, mutant, *, kscale=None, vscale=None):
    """float64 tree attention with the named defect (None: without one) -> (O [B, Hq, R, D], L natural [B, Hq, R], changed): `changed`
    is whether any row adds up another set of keys than without the defect"""
    assert mutant is None or mutant in MUTANTS, mutant
    q, k, v = dm.f64(q), dm.f64(k), dm.f64(v)
    B, Hq, R, D = q.shape
    Hkv = Hq // G
    kind = "decode" if qlens is None else "prefill"
    ks = np.ones(Hkv) if kscale is None else np.asarray(kscale, dtype=np.float64)
    vs = np.ones(Hkv) if vscale is None else np.asarray(vscale, dtype=np.float64)
    sink = None if logits is None else np.asarray(logits, dtype=np.float64)
    O = np.zeros((B, Hq, R, D))
    L = np.full((B, Hq, R), -np.inf)
    changed = False
    for b in range(B):
        n, qn = int(lens[b]), R if qlens is None else min(int(qlens[b]), R)
        if qn == 0:
            continue
        npad = (-(-max(n, 1) // TILE) + 2) * TILE
        for r0, r1 in wm.blocks_of(kind, qn, G):
            for h in range(Hq):
                j = h // G
                vis = _mutant_visible(n, qn, R, G, kind, r0, r1, h, b, masks, W, S, mutant, npad)
                if mutant is not None:
                    changed = changed or bool((vis != _mutant_visible(n, qn, R, G, kind, r0, r1, h, b, masks, W, S, None, npad)).any())
                K, V = np.zeros((npad, D)), np.zeros((npad, D))
                K[:n], V[:n] = k[b, j, :n], v[b, j, :n]
                Sc = np.where(vis, (q[b, h, r0:r1] @ K.T) * (ks[j] / math.sqrt(D)), -np.inf)
                m = Sc.max(axis=1, keepdims=True)
                seen = np.isfinite(m[:, 0])
                m0 = np.where(np.isfinite(m), m, 0.0)
                pw = np.exp(Sc - m0)
                l0 = np.where(seen, pw.sum(axis=1), 1.0)
                o = np.where(seen[:, None], (pw / l0[:, None]) @ V * vs[j], 0.0)
                lse = np.where(seen, m0[:, 0] + np.log(l0), -np.inf)
                if sink is not None:
                    o = o * (1.0 / (1.0 + np.exp(sink[h] - lse)))[:, None]
                    lse = np.logaddexp(lse, sink[h])
                O[b, h, r0:r1], L[b, h, r0:r1] = o, lse
    return O, L, changed
