"""The float64 model of SPARSE multi-head latent attention decode over an E4M3 latent cache (include/mfa_mla_sparse_fp8.h), its bounds,
needle inputs, named mutants and the cases the CPU and GPU files share (a plain module; numpy only).  It REDUCES to
tests/mla_fp8_model.py the way tests/mla_sparse_model.py reduces to tests/mla_model.py: a launch over lists is B x R one-row launches of
the dense e4m3 model.  Pair (b, r) becomes a sequence of its own whose BYTE cache holds the rows its visible slots name, taken in slot
order (a position named twice is there twice), read by all H heads without a causal mask.  Inputs are bytes: quantisation error is no
part of the bound.

  model()          mla_fp8_model.model() over the gathered byte rows -> Reference(O, L, A, E', EL') in the launch's shapes.  The bound is
                   mla_fp8_model's E' / EL' with the chain taken over the topk SLOTS the kernel walks, holes included:
                   chain_length(topk, pieces) replaces the gathered length's.  mutant= computes a named WRONG attention instead.  No
                   wrong kernel is ever run.
  emulated()       the kernel's roundings and order of sums: 32-SLOT steps with the holes kept in their slots as zero bytes, pieces of
                   slots combined in order, and attn_mla8.h's scale roundings -- the score scale fl(fl(scale log2 e) x kvScale), unsplit
                   mult = fl(fl(1 / l) x kvScale), a piece publishes fl(o x kvScale).
  CASES, inputs()  mla_sparse_model's CASES and SEAM_CASES -- its lists, unchanged -- restated over byte caches (mla_fp8_model.cache_bytes),
                   each with a kvScale of mla_fp8_model.KV_SCALES (0.37, 3.0, None) in turn.  "ld640": rows 640 BYTES apart.

Mutants.  mla_sparse_model.MUTANTS (its seam mutants and the four column mutants it passes through included) are statements about which
slots are visible and what a slot reads: they are computed by ITS gathered() over the byte rows.  mla_fp8_model.OWN_MUTANTS are
statements about columns and the scale and survive the reduction unchanged.  The combination's own (OWN_MUTANTS):
  row_address_in_16bit_elements   the row's byte offset doubled, the 16-bit sparse body's `ko * 2` kept: position c of sequence b reads
                                  row 2 (b C + c) of the packed cache, poison past its end.  Changes nothing nowhere.
  hole_keeps_previous_rows        a hole's row taken from the registers of the step before instead of zero bytes.  From the second step
                                  of a piece on those are finite values, and p = 0 exactly: nothing changes.  In the FIRST step of a
                                  piece there is no step before: the registers hold anything, the NaN bytes included, and 0 x NaN is
                                  NaN in every column of O.  Changes nothing where no list has a hole in the first step of a piece.
  kv_scale_per_row                the scale read as kvScale[b R + r].  Changes nothing where kvScale is None or B R = 1.
MARGIN is fixed by tests/test_mla_sparse_fp8_sensitivity.py alone, before any device run: the smallest power of two with at least 2 x
headroom over emulated()'s worst err / bound at margin 1 on CASES and SEAM_CASES together.
"""
import functools

import numpy as np

import decode_model as dm
import mla_fp8_model as fm
import mla_sparse_model as sm
from decode_model import LOG2E, U32, Reference, bounds, compare, piece_ranges, round_to, store  # noqa: F401
from mla_fp8_model import KV_SCALES, POISON, SCALE_TAIL, dequantize, values_of  # noqa: F401
from mla_model import DK, DV, LENS, SCALE, SEAM_C, SEAM_LENS, STEP, C, chain_length, seen_lens  # noqa: F401
from mla_sparse_model import HOLE, PAD, keep_mask, lists_of, page_table, visible  # noqa: F401

MARGIN = 2
B = len(LENS)

_plain = lambda c: c["kvscale"] is None  # noqa: E731
# name -> (what the defect is, where it changes nothing).  `case` has mla_sparse_model's facts plus kvscale and first_step_hole (some
# list of the launch has a hole in the first step of a piece)
OWN_MUTANTS = {
    "row_address_in_16bit_elements": ("a row address formed in 16-bit elements: the byte offset doubled", lambda c: False),
    "hole_keeps_previous_rows": ("a hole's row taken from the previous step's registers instead of zero bytes", lambda c: not c["first_step_hole"]),
    "kv_scale_per_row": ("the scale read as kvScale[b R + r]", lambda c: _plain(c) or c["B"] * c["R"] == 1),
}
SEAM_MUTANTS = sm.SEAM_MUTANTS
FP8_MUTANTS = tuple(fm.OWN_MUTANTS)
MUTANTS = dict(sm.MUTANTS)
# (of mla_fp8_model's own, kvScale[b] is kvScale[b R + r] after the reduction: it is this module's kv_scale_per_row)
MUTANTS.update({name: fm.OWN_MUTANTS[name] for name in FP8_MUTANTS if name != "kv_scale_per_sequence"})
MUTANTS.update(OWN_MUTANTS)


def _hole_in_a_first_step(ok, topk, pieces, piece_range=None):
    """ok [topk]: the visible slots of one list -> a piece with slots has a hole in its first 32 (a partial first step's tail included)"""
    return any(pe > pb and (pe - pb < STEP or not ok[pb:pb + STEP].all()) for (pb, pe) in piece_ranges(topk, pieces, piece_range))


def first_step_hole(case, pieces, idx):
    """some list of the launch has a hole in the first step of a piece"""
    return any(_hole_in_a_first_step(visible(idx[b, r], min(raw, case["C"]), r, case["R"], case["causal"]), case["topk"], pieces)
               for b, raw in enumerate(case["lens"]) for r in range(case["R"]))


def facts_of(case, pieces, n, idx):
    """mla_sparse_model's facts of ONE sequence plus what the mutants of this module ask about"""
    return dict(sm.facts_of(case, pieces, n, idx), kvscale=case["kvscale"], first_step_hole=first_step_hole(case, pieces, idx))


def _bytes_of(rows):
    """float rows that gathered() took out of a byte cache -> uint8; a row it calls poison (NaN) is the NaN byte"""
    return np.where(np.isnan(rows), float(POISON[0]), rows).astype(np.uint8)


def gathered(kvb, lens, idx, R, causal, mutant=None, **kw):
    """mla_sparse_model.gathered() over a byte cache -> list over b R + r of (byte rows [n', 576] uint8, slots [n']); a slot scored
    without a loaded row reads zero bytes"""
    return [(_bytes_of(rows), slots) for rows, slots in sm.gathered(np.asarray(kvb, dtype=np.float64), lens, idx, R, causal, mutant, **kw)]


def _reduced(q, parts):
    """q [B, H, R, 576] and gathered() -> the dense e4m3 model's operands: q' [B R, H, 1, 576], bytes [B R, n'max, 576], lens'"""
    B_, H, R, _ = q.shape
    width = max(1, max(len(rows) for rows, _s in parts))
    kvg = np.zeros((B_ * R, width, DK), dtype=np.uint8)
    for i, (rows, _s) in enumerate(parts):
        kvg[i, :len(rows)] = rows
    return np.ascontiguousarray(np.transpose(q, (0, 2, 1, 3)).reshape(B_ * R, H, 1, DK)), kvg, [len(rows) for rows, _s in parts]


def model(q, kvb, kvscale, lens, idx, causal, scale, mutant=None, *, pieces=None, page=None, shared=False, piece_range=None):
    """float64 attention over the lists and a byte cache kvb [B, C, 576] uint8 -> Reference(O, L, A, E', EL'), [B, H, R, ...]; `mutant`:
    a named wrong attention (its E / EL mean nothing)"""
    assert mutant is None or mutant in MUTANTS, mutant
    q = dm.f64(q)
    kvb = np.asarray(kvb, dtype=np.uint8)
    idx = np.asarray(idx, dtype=np.int64)
    B_, H, R, _ = q.shape
    topk = idx.shape[2]
    of_lists = mutant in sm.MUTANTS and mutant not in sm.DENSE_MUTANTS and mutant not in ("head_mod_32", "rows_swapped")
    parts = gathered(kvb, lens, idx, R, causal, mutant if of_lists else None, pieces=pieces, page=page, shared=shared, piece_range=piece_range)
    if mutant == "row_address_in_16bit_elements":
        flat = kvb.reshape(-1, DK)
        good = gathered(np.zeros_like(kvb), lens, idx, R, causal, shared=shared)   # (the slots alone)
        parts = []
        for i, (_rows, slots) in enumerate(good):
            b, r = divmod(i, R)
            at = 2 * ((0 if shared else b) * kvb.shape[1] + idx[b, r][slots])
            rows = np.where((at < len(flat))[:, None], flat[np.minimum(at, len(flat) - 1)], POISON[0]).astype(np.uint8)
            parts.append((rows, slots))
    if mutant == "head_mod_32":
        q = q[:, np.arange(H) % 32]
    q1, kvg, lens1 = _reduced(q, parts)
    inner = None
    if mutant in sm.DENSE_MUTANTS or mutant in FP8_MUTANTS:
        inner = mutant
    if mutant == "kv_scale_per_row":
        inner = "kv_scale_per_sequence"
    poisoned = np.array([bool(((rows & 0x7F) == 0x7F).any()) for rows, _s in parts])
    # (mla_fp8_model reads a NaN byte as 0 -- poison past a length, which it never reads; a mutant that READS poison computes NaN)
    ref = fm.model(q1, kvg, kvscale, lens1, False, scale, inner, pieces=pieces if inner == "kv_scale_twice_in_pieces" else None)
    O, L, A, E, EL = (sm._unreduced(x, B_, R) for x in ref)
    if poisoned.any():
        bad = poisoned.reshape(B_, 1, R)
        O, L = np.where(bad[..., None], np.nan, O), np.where(bad, np.nan, L)
    if mutant == "hole_keeps_previous_rows":
        for b in range(B_):
            for r in range(R):
                if _hole_in_a_first_step(visible(idx[b, r], min(int(lens[b]), kvb.shape[1]), r, R, causal), topk, pieces, piece_range):
                    O[b, :, r] = np.nan
    # the chain the kernel walks is the list's, holes included, and its pieces are pieces of slots: E' and EL' over that chain
    walked = np.array([chain_length(n1, None) if n1 else 0 for n1 in lens1], dtype=np.float64).reshape(B_, 1, R)
    more = np.where(walked > 0, chain_length(topk, pieces) - walked, 0.0) * U32
    E = E + more[..., None] * (A + np.abs(O)) * (1.0 + 1.0 / (DK + 3) + 1.0 / 48)
    EL = EL + more * (1.0 + 1.0 / (DK + 3))
    if mutant == "rows_swapped":
        O, L = O[:, :, ::-1].copy(), L[:, :, ::-1].copy()
    return Reference(O, L, A, E, EL)


def emulated(q, kvb, kvscale, lens, idx, causal, scale, fmt, *, pieces=None, shared=False, piece_range=None):
    """the model with the kernel's roundings and order of sums -> (O before the store's rounding [B, H, R, 512], L natural):
    mla_sparse_model.emulated() over the UNSCALED values e4m3(byte) -- a hole keeps its slot with score -inf and a row of zero bytes --
    with mla_fp8_model.emulated()'s scale roundings"""
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    q = dm.f64(q)
    deq = dequantize(kvb)
    idx = np.asarray(idx, dtype=np.int64)
    kvs = 1.0 if kvscale is None else f32(kvscale)
    B_, H, R, _ = q.shape
    topk = idx.shape[2]
    O = np.zeros((B_, H, R, DV))
    L = np.full((B_, H, R), -np.inf)
    NEG = -np.inf
    scale2 = f32(np.float32(np.float32(scale) * np.float32(1.44269504089)) * np.float32(kvs))
    ranges = piece_ranges(topk, pieces, piece_range)
    split = len(ranges) > 1
    for b in range(B_):
        n = min(int(lens[b]), deq.shape[1])
        for r in range(R):
            c = idx[b, r]
            ok = visible(c, n, r, R, causal)
            K = np.where(ok[:, None], deq[0 if shared else b][np.where(ok, c, 0)], 0.0)
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
                published.append((m, l, round_to(o * kvs, "f32") if split else o))
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
            mult = 1.0 / l0 if split else round_to(round_to(1.0 / l0, "f32") * kvs, "f32")
            O[b, :, r] = np.where(seen[:, None], ot * mult[:, None], 0.0)
            L[b, :, r] = np.where(seen, (np.where(seen, mstar, 0.0) + np.log2(l0)) / LOG2E, -np.inf)
    return O, L


def needle_queries(kvb, kvscale, lens, idx, H, R, causal, fmt, scale, *, pieces=None, shared=False, seed=0):
    """mla_sparse_model.needle_queries over the values the bytes stand for"""
    return sm.needle_queries(values_of(kvb, kvscale), lens, idx, H, R, causal, fmt, scale, pieces=pieces, shared=shared, seed=seed)


# ---------------------------------------------------------------------------------------------------------------------- the cases
CASES = {name: dict(case, kvscale=KV_SCALES[i % len(KV_SCALES)]) for i, (name, case) in enumerate(sm.CASES.items())}
SEAM_CASES = {name: dict(case, kvscale=KV_SCALES[i % len(KV_SCALES)]) for i, (name, case) in enumerate(sm.SEAM_CASES.items())}
ALL_CASES = dict(CASES, **SEAM_CASES)


def planned_pieces(case):
    """the piece count the launch of a case runs in (None: unsplit), from the library's own plan"""
    if case["pieces"] is None:
        return None
    if case["pieces"] != "plan":
        return int(case["pieces"])
    from metal_flash_attention_amd import AttentionMLASparseDecodeFP8
    _bytes, pieces = AttentionMLASparseDecodeFP8().plannedSplit(rows=case["R"], column=case["C"], heads=case["H"], batches=len(case["lens"]), scale=SCALE,
                                                                cacheLengths=0x1000, indices=0x2000, topk=case["topk"],
                                                                strides={"KV": (DK, 0, case["C"] * DK)})   # (the host reads neither)
    return pieces if pieces > 1 else None


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(case, pieces, q, kv bytes, idx, Reference, needle info) of a case of CASES or SEAM_CASES, computed once and shared"""
    case = ALL_CASES[name]
    pieces = planned_pieces(case)
    lens = case["lens"]
    kvb = fm.cache_bytes(0, len(lens), case["C"])
    idx = lists_of(case)
    shared = case["layout"] == "shared"
    q, info = needle_queries(kvb, case["kvscale"], lens, idx, case["H"], case["R"], case["causal"], case["fmt"], SCALE, pieces=pieces, shared=shared)
    ref = model(q, kvb, case["kvscale"], lens, idx, case["causal"], SCALE, pieces=pieces, page=case["page"], shared=shared)
    return case, pieces, q, kvb, idx, ref, info
