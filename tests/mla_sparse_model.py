"""The float64 model of SPARSE multi-head latent attention decode (include/mfa_mla_sparse.h), its bounds, needle inputs, named mutants
and the cases the CPU and GPU files share (a plain module; numpy only).  It REDUCES to tests/mla_model.py: a launch over lists is B x R
one-row launches of the dense model.  Pair (b, r) becomes a sequence of its own whose cache holds the rows its VISIBLE slots name, taken
in slot order (a position named twice is there twice), read by all H heads without a causal mask -- visibility was decided when the
cache was gathered.

  visible()        the rule of the header: slot j of row r is visible iff 0 <= c < len_b and, causal, c <= r + max(len_b - R, 0).
  model()          mla_model.model() over the gathered caches -> Reference(O, L, A, E, EL) in the launch's shapes [B, H, R, ...].  The
                   bound's chain is taken over the topk SLOTS the kernel walks, holes included: chain_length(topk, pieces) replaces the
                   gathered length's in E and EL.  mutant= computes a named WRONG attention instead.  No wrong kernel is ever run.
  emulated()       the kernel's roundings and order of sums: 32-SLOT steps with the holes kept in their slots (a step of holes changes
                   nothing), pieces of slots, the pieces combined in order.
  needle_queries() mla_model's needle rows over the gathered caches: the last two visible slots and the geometry's special slots.
  CASES, inputs()  the launches of tests/test_mla_sparse_gpu.py, which tests/test_mla_sparse_sensitivity.py walks on the CPU.

Mutants.  Those of mla_model that are statements about columns survive the reduction unchanged and are passed through (DENSE_MUTANTS).
Its mutants about lengths, the causal frontier, steps, pieces, pages and packing are statements about the dense walk over key ranges;
their counterparts over a list are this module's own (MUTANTS), each a change of which slots are visible or of what a slot reads.
MARGIN is fixed by tests/test_mla_sparse_sensitivity.py alone, before any GPU run: the smallest power of two with at least 2 x headroom
over emulated()'s worst err / bound at margin 1 on CASES.
"""
import functools

import numpy as np

import decode_model as dm
import mla_model as mm
from decode_model import LOG2E, U32, Reference, piece_ranges, round_to
from mla_model import DK, DV, LENS, SCALE, STEP, C, bounds, chain_length, compare, store  # noqa: F401

MARGIN = 2
HOLE = -1
B = len(LENS)

DENSE_MUTANTS = ("v_from_tail", "rope_left_out", "scale_sqrt_dk", "o_blocks_exchanged")
# name -> (what the defect is, where it changes nothing).  `case` has R, H, causal, pieces (None: unsplit), page, topk
MUTANTS = {
    "list_of_next_row": ("the list of row r + 1", lambda c: c["R"] == 1),
    "list_of_next_sequence": ("the list of sequence b + 1", lambda c: False),
    "position_as_physical_slot": ("a position used as a physical slot of a paged cache: the block table skipped", lambda c: not c["page"]),
    "minus_one_reads_key_0": ("-1 read as key 0", lambda c: False),
    "length_not_masked": ("a position at or past the length not masked", lambda c: False),
    "causal_dropped": ("the causal test dropped for listed keys", lambda c: not c["causal"]),
    "slots_past_topk_read": ("the slots past topk of the last step read from the allocation instead of being holes", lambda c: c["topk"] % STEP == 0),
    "halves_exchanged": ("the validity bits of a step's two 16-key halves exchanged", lambda c: False),
    "bit_r_tested": ("bit r tested in place of bit crow(r, hi)", lambda c: False),
    "repeat_counted_once": ("a repeated position counted once", lambda c: False),
    "piece_range_on_positions": ("the piece's end applied to key positions as well as to slots", lambda c: not c["pieces"]),
    "holes_step_resets_m": ("a step of 32 holes resets the running maximum", lambda c: False),
    "head_mod_32": ("head 32 group + q taken modulo 32", lambda c: c["H"] <= 32),
    "rows_swapped": ("the R rows of a head swapped", lambda c: c["R"] == 1),
}
MUTANTS.update({name: mm.MUTANTS[name] for name in DENSE_MUTANTS})


def visible(c, n, r, R, causal):
    """the header's rule for position(s) c of row r of a sequence of length n"""
    c = np.asarray(c, dtype=np.int64)
    ok = (c >= 0) & (c < n)
    if causal:
        ok &= c <= r + max(n - R, 0)
    return ok


def page_table(page, seed=None):
    """the permuted block table [B, C // page] of the paged cases (numpy; the GPU file lays its pool out by it)"""
    pps = C // page
    return np.random.default_rng(page if seed is None else seed).permutation(B * pps).reshape(B, pps).astype(np.int32)


def gathered(kv, lens, idx, R, causal, mutant=None, *, pieces=None, page=None, shared=False, piece_range=None):
    """what every (b, r) attends to -> list over b R + r of (rows [n', 576] float64, slots [n'] the slot each row came from).  A slot that
    a (mutated) kernel scores without having loaded a row reads zeros: score 0, value 0."""
    kv = dm.f64(kv)
    idx = np.asarray(idx, dtype=np.int64)
    topk = idx.shape[2]
    flat = idx.reshape(-1)
    ranges = piece_ranges(topk, pieces, piece_range)
    table = page_table(page) if page else None
    out = []
    for b in range(B):
        n = int(lens[b])
        src = 0 if shared else b
        for r in range(R):
            lb, lr = b, r
            if mutant == "list_of_next_row":
                lr = (r + 1) % R
            if mutant == "list_of_next_sequence":
                lb = (b + 1) % B
            c = idx[lb, lr].copy()
            steps = -(-topk // STEP) * STEP
            if mutant == "slots_past_topk_read" and topk % STEP:   # the allocation is packed: the next list follows, then nothing
                at = (lb * R + lr) * topk + np.arange(steps)
                c = np.where(at < flat.size, flat[np.minimum(at, flat.size - 1)], HOLE)
            else:
                c = np.concatenate([c, np.full(steps - topk, HOLE, dtype=np.int64)])
            if mutant == "minus_one_reads_key_0":
                c = np.where(c == HOLE, 0, c)
            ok = visible(c, n if mutant != "length_not_masked" else C, r, R, causal and mutant not in ("causal_dropped", "length_not_masked"))
            if mutant == "length_not_masked" and causal:   # (the frontier still holds for the keys below the length)
                ok &= (c >= n) | (c <= r + max(n - R, 0))
            if mutant == "repeat_counted_once":
                _u, first = np.unique(c, return_index=True)
                once = np.zeros(len(c), dtype=bool)
                once[first] = True
                ok &= once
            if mutant == "piece_range_on_positions":
                for (pb, pe) in ranges:
                    ok[pb:pe] &= c[pb:pe] < pe
            loaded = ok.copy()                                   # rows a kernel has in registers; the others are zeros
            j = np.arange(steps)
            if mutant == "halves_exchanged":
                ok = ok[j ^ 16]
            if mutant == "bit_r_tested":   # slot j = crow(r, hi) = (r & 3) + 8 (r >> 2) + 4 hi takes the bit of slot r = (j & 3) + 4 (j >> 3)
                ok = ok[j // STEP * STEP + ((j % STEP) & 3) + 4 * ((j % STEP) >> 3)]
            if mutant == "holes_step_resets_m":
                for (pb, pe) in ranges:
                    dead = [s for s in range(pb, min(pe, steps), STEP) if not ok[s:min(s + STEP, pe)].any()]
                    if dead:
                        ok[pb:dead[-1]] = False
            slots = np.nonzero(ok)[0]
            rows = np.zeros((len(slots), DK))
            for i, s in enumerate(slots):
                if not loaded[s]:
                    continue
                if mutant == "position_as_physical_slot" and page:   # physical slot c of the pool: the key that lives there, or poison
                    hit = np.argwhere(table == c[s] // page)
                    rows[i] = kv[0 if shared else hit[0][0], hit[0][1] * page + c[s] % page] if len(hit) else np.nan
                else:
                    rows[i] = kv[src, c[s]]
            out.append((rows, slots))
    return out


def _reduced(q, parts):
    """q [B, H, R, 576] and gathered() -> the dense model's operands: q' [B R, H, 1, 576], kv' [B R, n'max, 576], lens'"""
    B_, H, R, _ = q.shape
    width = max(1, max(len(rows) for rows, _s in parts))
    kvg = np.zeros((B_ * R, width, DK))
    for i, (rows, _s) in enumerate(parts):
        kvg[i, :len(rows)] = rows
    return np.ascontiguousarray(np.transpose(q, (0, 2, 1, 3)).reshape(B_ * R, H, 1, DK)), kvg, [len(rows) for rows, _s in parts]


def _unreduced(x, B_, R):
    """[B R, H, 1, ...] -> [B, H, R, ...]"""
    x = x.reshape((B_, R) + x.shape[1:])
    return np.ascontiguousarray(np.moveaxis(x[:, :, :, 0], 1, 2))


def model(q, kv, lens, idx, causal, scale, mutant=None, *, pieces=None, page=None, shared=False, piece_range=None):
    """float64 attention over the lists -> Reference(O, L, A, E, EL), [B, H, R, ...]"""
    assert mutant is None or mutant in MUTANTS, mutant
    q = dm.f64(q)
    B_, H, R, _ = q.shape
    topk = np.asarray(idx).shape[2]
    parts = gathered(kv, lens, idx, R, causal, None if mutant in DENSE_MUTANTS else mutant, pieces=pieces, page=page, shared=shared, piece_range=piece_range)
    if mutant == "head_mod_32":
        q = q[:, np.arange(H) % 32]
    q1, kvg, lens1 = _reduced(q, parts)
    ref = mm.model(q1, kvg, lens1, False, scale, mutant if mutant in DENSE_MUTANTS else None)
    O, L, A, E, EL = (_unreduced(x, B_, R) for x in ref)
    # the chain the kernel walks is the list's, holes included, and its pieces are pieces of slots
    walked = np.array([chain_length(n1, None) if n1 else 0 for n1 in lens1], dtype=np.float64).reshape(B_, 1, R)
    more = np.where(walked > 0, chain_length(topk, pieces) - walked, 0.0) * U32
    E = E + more[..., None] * (A + np.abs(O))
    EL = EL + more
    if mutant == "rows_swapped":
        O, L = O[:, :, ::-1].copy(), L[:, :, ::-1].copy()
    return Reference(O, L, A, E, EL)


def emulated(q, kv, lens, idx, causal, scale, fmt, *, pieces=None, shared=False, piece_range=None):
    """the model with the kernel's roundings and order of sums -> (O before the store's rounding [B, H, R, 512], L natural): mla_model's
    emulated() over SLOTS -- a hole keeps its slot with score -inf and a zero row, a step is 32 slots, a piece is a range of slots"""
    q, kv = dm.f64(q), dm.f64(kv)
    idx = np.asarray(idx, dtype=np.int64)
    B_, H, R, _ = q.shape
    topk = idx.shape[2]
    O = np.zeros((B_, H, R, DV))
    L = np.full((B_, H, R), -np.inf)
    NEG = -np.inf
    scale2 = float(np.float32(np.float32(scale) * np.float32(1.44269504089)))
    ranges = piece_ranges(topk, pieces, piece_range)
    for b in range(B_):
        n = int(lens[b])
        for r in range(R):
            c = idx[b, r]
            ok = visible(c, n, r, R, causal)
            K = np.where(ok[:, None], kv[0 if shared else b][np.where(ok, c, 0)], 0.0)
            V = K[:, :DV]
            S2 = np.where(ok[None, :], (q[b, :, r] @ K.T) * scale2, NEG)    # [H, topk]
            published = []
            for (pb, pe) in ranges:
                m, l, o = np.full(H, NEG), np.zeros(H), np.zeros((H, DV))
                for s0 in range(pb, pe, STEP):
                    s = S2[:, s0:min(s0 + STEP, pe)]
                    new = np.maximum(m, s.max(axis=1))
                    fin = np.isfinite(new)
                    ref = np.where(fin, new, 0.0)
                    corr = np.where(np.isfinite(m), np.exp2(np.where(np.isfinite(m), m, 0.0) - ref), 1.0)
                    p = np.where(fin[:, None], np.exp2(s - ref[:, None]), 0.0)
                    m, l, o = new, l * corr + p.sum(axis=1), o * corr[:, None] + round_to(p, fmt) @ V[s0:min(s0 + STEP, pe)]
                published.append((m, l, o))
            mstar = np.full(H, NEG)
            for m, l, _o in published:
                mstar = np.maximum(mstar, np.where(l > 0, m, NEG))
            lt, ot = np.zeros(H), np.zeros((H, DV))
            for m, l, o in published:
                live = (l > 0) & np.isfinite(m)
                w = np.where(live, np.exp2(np.where(live, m - np.where(np.isfinite(mstar), mstar, 0.0), 0.0)), 0.0)
                lt += w * l
                ot += w[:, None] * o
            seen = lt > 0
            l0 = np.where(seen, lt, 1.0)
            O[b, :, r] = np.where(seen[:, None], ot / l0[:, None], 0.0)
            L[b, :, r] = np.where(seen, (np.where(seen, mstar, 0.0) + np.log2(l0)) / LOG2E, -np.inf)
    return O, L


def needle_queries(kv, lens, idx, H, R, causal, fmt, scale, *, pieces=None, shared=False, piece_range=None, seed=0):
    """q [B, H, R, 576] (float64 values of the 16-bit type) and, per (b, h, r), its needles -- keyed by the index of the visible slot in
    the gathered cache -- from mla_model.needle_queries over the gathered caches (not causal there: no forbidden key; a hole's row is
    not in the cache at all, and the mutants of the list are what shows a hole that was read)"""
    parts = gathered(kv, lens, idx, R, causal, shared=shared)
    width = max(1, max(len(rows) for rows, _s in parts))
    kvg = np.zeros((B * R, width, DK))
    for i, (rows, _s) in enumerate(parts):
        kvg[i, :len(rows)] = rows
    q1, info1 = mm.needle_queries(kvg, [len(rows) for rows, _s in parts], H, 1, False, fmt, scale, seed=seed)
    info = {(i // R, h, i % R): v for (i, h, _z), v in info1.items()}
    return _unreduced(q1, B, R), info


# ---------------------------------------------------------------------------------------------------------------------- the cases
def _case(fmt, H, R, topk, lists, causal=True, pieces=None, page=None, layout="packed", out=None):
    return dict(fmt=fmt, H=H, R=R, topk=topk, lists=lists, causal=causal, pieces=pieces, page=page, layout=layout, out=out or fmt)


# lists: how the lists are drawn (lists_of).  pieces: None runs without a workspace; "plan" is the host's; a number is forced
CASES = {
    "a random subset, unsplit": _case("bf16", 16, 1, 64, "subset"),
    "b one slot": _case("f16", 8, 2, 1, "subset"),
    "b thirty-one slots": _case("f16", 8, 2, 31, "mixed"),
    "b thirty-three slots": _case("f16", 8, 2, 33, "mixed"),
    "c two groups, holes scattered, a first step of holes": _case("bf16", 40, 1, 100, "scattered"),
    "d causal, past the frontier and the length": _case("f16", 11, 3, 96, "mixed"),
    "e four rows, not causal": _case("bf16", 4, 4, 80, "mixed", causal=False),
    "f pages of 16, planned": _case("f16", 16, 1, 512, "mixed", pieces="plan", page=16),
    "f pages of 256, planned": _case("bf16", 16, 2, 512, "mixed", pieces="plan", page=256),
    "g two pieces": _case("bf16", 16, 1, 160, "mixed", pieces=2),
    "g seven pieces": _case("bf16", 16, 1, 160, "mixed", pieces=7),
    "g sixty-four pieces, fp32 out": _case("bf16", 16, 1, 160, "mixed", pieces=64, out="f32"),
    "h rows 640 apart": _case("bf16", 40, 1, 70, "mixed", layout="ld640"),
    "h one cache shared": _case("bf16", 16, 2, 70, "mixed", layout="shared"),
    "i a list of holes": _case("bf16", 4, 2, 40, "empty row"),
}


def lists_of(case, seed=0):
    """idx [B, R, topk] int64: every entry is -1 or a position in [0, C)"""
    R, topk, kind = case["R"], case["topk"], case["lists"]
    rng = np.random.default_rng(4000 + seed + topk + 7 * R)
    idx = np.full((B, R, topk), HOLE, dtype=np.int64)
    for b, n in enumerate(LENS):
        for r in range(R):
            limit = min(n, r + max(n - R, 0) + 1) if case["causal"] else n        # positions below it are visible
            take = min(limit, topk if kind == "subset" else max(1, (3 * topk) // 4))
            row = np.full(topk, HOLE, dtype=np.int64)
            row[:take] = rng.choice(limit, size=take, replace=False) if take else []
            if kind != "subset" and topk > take:                                  # holes of every kind: past the frontier, past the length, -1
                rest = topk - take
                extra = [HOLE] * rest
                if n < C:
                    extra[:rest // 2] = list(rng.integers(n, C, size=rest // 2))
                if case["causal"] and limit < n and rest >= 3:
                    extra[-1] = limit                                             # the first key past the frontier
                    extra[-2] = n - 1
                row[take:] = extra
            rng.shuffle(row)
            idx[b, r] = row
    if kind == "scattered":                                                       # the whole first step of sequence 0 is holes
        idx[0, 0, :STEP] = HOLE
        idx[B - 1, 0, 2 * STEP:3 * STEP] = HOLE                                   # ... and a step of holes between visible ones for another
    if kind == "empty row":
        idx[0, R - 1] = HOLE
        idx[2, 0] = C - 1                                                         # a list that names only a key past the length
    if topk >= 8 and kind == "mixed":                                             # a position named twice counts twice
        for b, n in enumerate(LENS):
            if n >= 8:
                good = np.nonzero(visible(idx[b, 0], n, 0, R, case["causal"]))[0]
                hole = np.nonzero(idx[b, 0] == HOLE)[0]
                if len(good) and len(hole):
                    idx[b, 0, hole[0]] = idx[b, 0, good[0]]
    assert ((idx == HOLE) | ((idx >= 0) & (idx < C))).all()
    return idx


def planned_pieces(case):
    """the piece count the launch of a case runs in (None: unsplit), from the library's own plan"""
    if case["pieces"] is None:
        return None
    if case["pieces"] != "plan":
        return int(case["pieces"])
    from metal_flash_attention_amd import AttentionMLASparseDecode
    _bytes, pieces = AttentionMLASparseDecode().plannedSplit(rows=case["R"], column=C, heads=case["H"], batches=B, scale=SCALE, cacheLengths=0x1000,
                                                             indices=0x2000, topk=case["topk"])   # (the host reads neither)
    return pieces if pieces > 1 else None


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(case, pieces, q, kv, idx, Reference, needle info) of a case, computed once and shared"""
    case = CASES[name]
    pieces = planned_pieces(case)
    kv = mm.cache_values(case["fmt"])
    idx = lists_of(case)
    shared = case["layout"] == "shared"
    q, info = needle_queries(kv, LENS, idx, case["H"], case["R"], case["causal"], case["fmt"], SCALE, pieces=pieces, shared=shared)
    ref = model(q, kv, LENS, idx, case["causal"], SCALE, pieces=pieces, page=case["page"], shared=shared)
    return case, pieces, q, kv, idx, ref, info


def keep_mask(idx, causal, R):
    """[B][C]: the cache rows some list of the launch makes visible -- everything else may hold poison"""
    keep = np.zeros((B, C), dtype=bool)
    for b, n in enumerate(LENS):
        for r in range(R):
            c = idx[b, r]
            keep[b, c[visible(c, n, r, R, causal)]] = True
    return keep
