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
  CASES, inputs()  the launches of tests/test_mla_sparse_gpu.py, which tests/test_mla_sparse_sensitivity.py walks on the CPU.  SEAM_CASES
                   run on mla_model's seam batch (SEAM_LENS in SEAM_C keys) with lists that sit ON the rule's seams: n - 1, n, 0, the
                   frontier and the key after it, column - 1 and the positions in [column, cacheLengths[b]) of the sequence handed a
                   length past the column, entries below -1.  A case carries its batch (lens, C).

Mutants.  Those of mla_model that are statements about columns survive the reduction unchanged and are passed through (DENSE_MUTANTS).
Its mutants about lengths, the causal frontier, steps, pieces, pages and packing are statements about the dense walk over key ranges;
their counterparts over a list are this module's own (MUTANTS), each a change of which slots are visible or of what a slot reads.
MARGIN is fixed by tests/test_mla_sparse_sensitivity.py alone, before any GPU run: the smallest power of two with at least 2 x headroom
over emulated()'s worst err / bound at margin 1 on CASES and SEAM_CASES together.
"""
import functools

import numpy as np

import decode_model as dm
import mla_model as mm
from decode_model import LOG2E, U32, Reference, piece_ranges, round_to
from mla_model import DK, DV, LENS, SCALE, SEAM_C, SEAM_LENS, STEP, C, bounds, chain_length, compare, seen_lens, store  # noqa: F401

MARGIN = 2
HOLE = -1
B = len(LENS)
PAD = 96             # rows of poison a seam launch keeps in front of and behind every sequence: where an entry in [-PAD, C + PAD) lands

DENSE_MUTANTS = ("v_from_tail", "rope_left_out", "scale_sqrt_dk", "o_blocks_exchanged")
# name -> (what the defect is, where it changes nothing).  `case` has R, H, causal, pieces (None: unsplit), page, topk, n (the clamped
# length), raw (the length the launch is handed), C and negatives (the lists hold an entry below -1)
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
    "length_not_clamped": ("cacheLengths[b] not clamped to column: a listed position in [column, cacheLengths[b]) is visible and reads "
                           "the row of sequence b + 1 that lies there in a packed cache", lambda c: c["raw"] <= c["C"]),
    "only_minus_one_is_a_hole": ("only -1 is a hole: an entry below -1 is scored, with the row of key 0", lambda c: not c["negatives"]),
    "last_key_of_the_column_hidden": ("the length clamped to column - 1: the last key a full cache holds is a hole",
                                      lambda c: c["n"] < c["C"]),
}
SEAM_MUTANTS = ("length_not_clamped", "only_minus_one_is_a_hole", "last_key_of_the_column_hidden")   # only SEAM_CASES show them
MUTANTS.update({name: mm.MUTANTS[name] for name in DENSE_MUTANTS})


def visible(c, n, r, R, causal):
    """the header's rule for position(s) c of row r of a sequence of length n"""
    c = np.asarray(c, dtype=np.int64)
    ok = (c >= 0) & (c < n)
    if causal:
        ok &= c <= r + max(n - R, 0)
    return ok


def facts_of(case, pieces, n, idx):
    """what a mutant's `harmless` rule is asked about: the case's launch, its lists and ONE sequence, n as the launch is handed it"""
    return dict(R=case["R"], H=case["H"], B=len(case["lens"]), causal=case["causal"], pieces=pieces, page=case["page"], topk=case["topk"],
                C=case["C"], raw=n, n=min(n, case["C"]), negatives=bool((np.asarray(idx) < HOLE).any()))


def page_table(page, seed=None, batches=B, column=C):
    """the permuted block table [B, ceil(C / page)] of the paged cases (numpy; the GPU file lays its pool out by it)"""
    pps = -(-column // page)
    return np.random.default_rng(page if seed is None else seed).permutation(batches * pps).reshape(batches, pps).astype(np.int32)


def gathered(kv, lens, idx, R, causal, mutant=None, *, pieces=None, page=None, shared=False, piece_range=None):
    """what every (b, r) attends to -> list over b R + r of (rows [n', 576] float64, slots [n'] the slot each row came from).  A slot that
    a (mutated) kernel scores without having loaded a row reads zeros: score 0, value 0."""
    kv = dm.f64(kv)
    idx = np.asarray(idx, dtype=np.int64)
    B, C = len(lens), kv.shape[1]                                # (the batch is the caller's: a length past the cache's C rows is clamped)
    topk = idx.shape[2]
    flat = idx.reshape(-1)
    ranges = piece_ranges(topk, pieces, piece_range)
    table = page_table(page, None, B, C) if page else None
    out = []
    for b in range(B):
        n = min(int(lens[b]), C)
        if mutant == "length_not_clamped":
            n = int(lens[b])
        if mutant == "last_key_of_the_column_hidden":
            n = min(n, C - 1)
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
            if mutant == "only_minus_one_is_a_hole" and n:
                c = np.where(c < HOLE, 0, c)
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
                elif c[s] >= C:                                     # (length_not_clamped alone: behind the cache's last row lies the next sequence)
                    rows[i] = kv[(src + 1) % B, c[s] - C]
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
        n = min(int(lens[b]), kv.shape[1])
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
    B = len(lens)
    width = max(1, max(len(rows) for rows, _s in parts))
    kvg = np.zeros((B * R, width, DK))
    for i, (rows, _s) in enumerate(parts):
        kvg[i, :len(rows)] = rows
    q1, info1 = mm.needle_queries(kvg, [len(rows) for rows, _s in parts], H, 1, False, fmt, scale, seed=seed)
    info = {(i // R, h, i % R): v for (i, h, _z), v in info1.items()}
    return _unreduced(q1, B, R), info


# ---------------------------------------------------------------------------------------------------------------------- the cases
def _case(fmt, H, R, topk, lists, causal=True, pieces=None, page=None, layout="packed", out=None, lens=LENS, C=C):
    return dict(fmt=fmt, H=H, R=R, topk=topk, lists=lists, causal=causal, pieces=pieces, page=page, layout=layout, out=out or fmt,
                lens=tuple(lens), C=C)


def _seam(fmt, H, R, topk, **kw):
    """a case on the seam batch.  Contiguous ("padded": PAD rows of poison around every sequence) its lists hold entries below -1; paged
    they hold none, and positions up to C + PAD instead, which a widened block table sends to the page of poison"""
    kw.setdefault("layout", "packed" if kw.get("page") else "padded")
    return _case(fmt, H, R, topk, "seam, paged" if kw.get("page") else "seam", lens=SEAM_LENS, C=SEAM_C, **kw)


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


# topk 32, 64 and 96 are whole steps (no slot past topk pads the last one), 33 is one slot more.  96 slots are two 64-slot tiles: two pieces
SEAM_CASES = {
    "s thirty-two slots, a seam inside a head": _seam("f16", 11, 3, 32),
    "s sixty-four slots, eight rows": _seam("bf16", 4, 8, 64),
    "s ninety-six slots, two groups, not causal": _seam("bf16", 40, 1, 96, causal=False),
    "s ninety-six slots, two pieces": _seam("f16", 16, 2, 96, pieces=2),
    "s thirty-three slots": _seam("f16", 8, 2, 33),
    "s pages of 16, thirty-two slots": _seam("bf16", 16, 1, 32, page=16),
    "s pages of 32, ninety-six slots, two pieces": _seam("f16", 11, 3, 96, pieces=2, page=32),
    "s pages of 64, thirty-three slots": _seam("bf16", 4, 8, 33, page=64),
    "s pages of 512, sixty-four slots": _seam("f16", 16, 2, 64, page=512),
}
ALL_CASES = dict(CASES, **SEAM_CASES)


def seam_lists_of(case, rng):
    """idx [B, R, topk] on the seams of the rule `0 <= c < min(len, column)` and, causal, `c <= frontier`: every list of a live
    sequence holds n - 1, n, 0 and, causal, the row's frontier and the key after it; where the launch is handed n > column also
    column - 1 (visible), column, column + 1 and n - 1 (holes); then entries below -1 (-2, -17, -PAD; contiguous caches only) or, paged,
    positions up to column + PAD - 1; the rest are visible positions and -1, shuffled"""
    R, topk, lens, C_, paged = case["R"], case["topk"], case["lens"], case["C"], bool(case["page"])
    idx = np.full((len(lens), R, topk), HOLE, dtype=np.int64)
    for b, raw in enumerate(lens):
        n = min(raw, C_)
        if n == 0:
            idx[b] = rng.integers(0, C_, (R, topk))                  # the empty sequence: every position is a hole
            continue
        for r in range(R):
            fr = r + max(n - R, 0)
            must = [raw - 1, raw, 0] + ([fr, fr + 1] if case["causal"] else [])
            if raw > C_:
                must += [C_ - 1, C_, C_ + 1]
            must += [C_ + PAD - 1, C_ + 5] if paged else [-2, -17, -PAD]
            must = list(dict.fromkeys(must))
            limit = min(n, fr + 1) if case["causal"] else n
            free = np.setdiff1d(np.arange(limit), must)
            take = min(len(free), (3 * (topk - len(must))) // 4)
            row = np.full(topk, HOLE, dtype=np.int64)
            row[:len(must)] = must
            row[len(must):len(must) + take] = rng.choice(free, size=take, replace=False)
            rng.shuffle(row)
            idx[b, r] = row
    lo, hi = (0, C_ + PAD) if paged else (-PAD, C_ + PAD)
    assert ((idx == HOLE) | ((idx >= lo) & (idx < hi))).all()
    return idx


def lists_of(case, seed=0):
    """idx [B, R, topk] int64: every entry is -1 or a position in [0, C) -- on the seam batch (seam_lists_of) in [-PAD, C + PAD)"""
    R, topk, kind = case["R"], case["topk"], case["lists"]
    LENS, C, B = case["lens"], case["C"], len(case["lens"])
    rng = np.random.default_rng(4000 + seed + topk + 7 * R)
    if kind.startswith("seam"):
        return seam_lists_of(case, rng)
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
    _bytes, pieces = AttentionMLASparseDecode().plannedSplit(rows=case["R"], column=case["C"], heads=case["H"], batches=len(case["lens"]), scale=SCALE, cacheLengths=0x1000,
                                                             indices=0x2000, topk=case["topk"])   # (the host reads neither)
    return pieces if pieces > 1 else None


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(case, pieces, q, kv, idx, Reference, needle info) of a case of CASES or SEAM_CASES, computed once and shared; the lengths are
    the case's own (case["lens"] as the launch is handed them, seen_lens(case) as it reads them)"""
    case = ALL_CASES[name]
    pieces = planned_pieces(case)
    lens = case["lens"]
    kv = mm.cache_values(case["fmt"], 0, len(lens), case["C"])
    idx = lists_of(case)
    shared = case["layout"] == "shared"
    q, info = needle_queries(kv, lens, idx, case["H"], case["R"], case["causal"], case["fmt"], SCALE, pieces=pieces, shared=shared)
    ref = model(q, kv, lens, idx, case["causal"], SCALE, pieces=pieces, page=case["page"], shared=shared)
    return case, pieces, q, kv, idx, ref, info


def keep_mask(idx, causal, R, lens=LENS, column=C):
    """[B][C]: the cache rows some list of the launch makes visible -- everything else may hold poison"""
    keep = np.zeros((len(lens), column), dtype=bool)
    for b, n in enumerate(lens):
        n = min(n, column)
        for r in range(R):
            c = idx[b, r]
            keep[b, c[visible(c, n, r, R, causal)]] = True
    return keep
