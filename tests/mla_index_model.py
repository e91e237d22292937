"""The float64 model of the MLA sparse indexer (include/mfa_mla_index.h), its bound, an emulation of both kernels as they are written
(csrc/attn_mla_index.h), named mutants and the cases the CPU and GPU files share (a plain module; numpy only).

  reference()        float64 logits [B, R, C] and the per-element bound 2 x 161 x 2^-24 x sum_h |W_h| sum_d |q_hd k_cd| of DESIGN.md 4.30,
                     per sequence with matmuls.
  layout()           a case's operands AS THEY LIE IN MEMORY: flat FP32 arrays that hold values of the 16-bit type, with their strides, the
                     block table and the poison.  The GPU file uploads exactly these; emulated_logits() reads exactly these, through the
                     same address arithmetic as the kernel, so a mutant of a stride or of the table reads what the wrong kernel would.
  emulated_logits()  the logits kernel's walk in FP32: grid index -> (row, tile, batch) with the library's own (steps, tiles) (plan_of():
                     parsed from launchForm), wave w of step s at tile0 + 32 (4 s + w), loops that end at key0 >= v, lanes at or past v on
                     zeros and without a store, the head sum as an fma chain -- block 0 then 1, crow order, one add across the halves --
                     and fmaxf's NaN rule.  It fills the sentinel-filled allocation the GPU launch fills; verdict() judges either.
  emulated_select()  the select kernel as written: order key, four 8-bit passes with (prefix, mask, want), rounds of 4096 in (u, wave,
                     lane) order with greaterBase / tieBase carried, slot = greater_before + min(ties_before, want), the slot < topk guard
                     and the early stop.  select_ref() is numpy's lexsort.
  MUTANTS            name -> (what the defect is, harmless(facts)).  mutant= makes either emulation compute what a defect of the kernel or
                     of the host plan would.  No wrong kernel is ever run.

Poison.  ReLU is fmaxf(s, 0) and fmaxf(NaN, 0) = 0: a key row of NaN read by mistake gives a logit of exactly 0, not NaN.  NaN stays
behind every length (it proves "never stored": such a position keeps its sentinel), but no argument rests on NaN becoming visible: the
padding of strided QI rows and heads and one of the two unnamed pages hold +-2^14, whose products are about 2^14 where the bound is about
1e-3; the padding of W holds NaN, which fma does propagate.  tests/test_mla_index_sensitivity.py shows with these very arrays that every
stride, page and length mutant leaves the bound."""
import functools
import re
import zlib

import numpy as np

from decode_model import round_to

DI, STEP, WAVES = 128, 32, 4
ROUNDINGS = 128 + 32 + 1            # derived, not measured
U32 = 2.0 ** -24
SENTINEL = 12345.0
BIG = 2.0 ** 14
PADW = 8                            # a logits allocation is [B + 1][R + 1][C + PADW]
ROUND = 4096                        # positions of a round of the select kernel's ordered pass
UNWRITTEN = -7
LENGTHS, TABLE = 0x1000, 0x5000     # (pointers the host never reads: launchForm launches nothing)


def visible(lens, R, causal=True, column=None, mutant=None):
    """v [B, R] of the header's rule; the mutants of the rule are said here"""
    n = np.asarray(lens, dtype=np.int64)
    if mutant != "length_not_clamped":
        n = np.minimum(n, column)
    n = n[:, None]
    r = np.arange(R)[None, :]
    if mutant == "causal_ignored":
        causal = False
    if mutant == "causal_forced":
        causal = True
    if not causal:
        return np.broadcast_to(n, (len(lens), R)).copy()
    return np.minimum(n, r + np.maximum(n - R, 0) + (0 if mutant == "frontier_off_by_one" else 1))


def crow(r, hi):
    return (r & 3) + 8 * (r >> 2) + 4 * hi


# ------------------------------------------------------------------------------------------------------------------ the logits cases
def _logits(fmt, H, R, lens, C, causal=True, k="contiguous", page=0, q="packed", w="packed", problem=None):
    return dict(fmt=fmt, H=H, R=R, lens=tuple(lens), C=C, causal=causal, k=k, page=page, q=q, w=w, problem=problem)


OLD_LENS, OLD_C = (0, 1, 31, 32, 33, 129, 200), 200
# the causal sweep of 32 rows (v = n - 31 .. n) crosses: a wave seam (48, 272 ...), a step seam -- `after < v` turning false at 128 k and
# true one key later (144, 400) --, a tile seam with one key in the next tile (the tile's size + 16), v = column; besides 0, lengths
# below the 32 rows and two lengths past the column
M2_LENS = (0, 1, 5, 20, 33, 48, 128, 144, 256, 257, 272, 400, 528, 640, 641, 1140)
M4_LENS = (0, 1, 5, 20, 31, 32, 33, 48, 64, 96, 128, 130, 144, 160, 200, 255, 257, 272, 300, 383, 385, 400, 511, 513, 528, 544, 576, 590, 599,
           600, 601, 1100)
M8_LENS = (0, 1, 5, 20, 31, 33, 48, 64, 130, 144, 257, 272, 385, 400, 513, 528, 640, 656, 768, 784, 900, 912, 1000, 1024, 1025, 1040, 1055,
           1072, 1100, 1101, 1102, 3000)
SMALL_LENS = (0, 1, 2, 31, 33, 129, 200, 201, 999)   # column 200: two lengths past it

# the multi-step plans: name -> (fmt, H, R, lens, C); every layout and one launch without `causal` of each
PLANS = {"m2": ("bf16", 64, 32, M2_LENS, 640), "m4": ("f16", 33, 32, M4_LENS, 600), "m8": ("bf16", 40, 32, M8_LENS, 1101)}
PLAN_FORMS = {
    "m2": "attn_mlai_d128_bf16 (grid 1536 = 3 tiles of 256 keys x 32 rows x 16 sequences, 64 heads, %s)",
    "m4": "attn_mlai_d128_f16 (grid 2048 = 2 tiles of 512 keys x 32 rows x 32 sequences, 33 heads, %s)",
    "m8": "attn_mlai_d128_bf16 (grid 2048 = 2 tiles of 1024 keys x 32 rows x 32 sequences, 40 heads, %s)",
}
STEP_CASES = {}
for _p, (_fmt, _H, _R, _lens, _C) in PLANS.items():
    for _k in ("contiguous", "strided", "paged"):
        STEP_CASES["%s %s" % (_p, _k)] = _logits(_fmt, _H, _R, _lens, _C, k=_k, page=16 if _k == "paged" else 0, problem=_p)
    STEP_CASES["%s not causal" % _p] = _logits(_fmt, _H, _R, _lens, _C, causal=False, problem=_p)

# heads, strides of QI and W, pages, rows: small columns, steps = 1
HEAD_CASES = {
    "h one head": _logits("bf16", 1, 2, SMALL_LENS, 200, q="padded", w="padded"),
    "h 31 heads, QI transposed": _logits("f16", 31, 1, SMALL_LENS, 200, q="transposed", w="padded", k="strided"),
    "h 32 heads, 32 rows, pages of 64": _logits("bf16", 32, 32, SMALL_LENS, 200, q="padded", w="padded", k="paged", page=64),
    "h 33 heads, pages of 256": _logits("f16", 33, 2, (0, 1, 255, 256, 257, 300, 301), 300, q="transposed", w="padded", k="paged", page=256),
    "h 33 heads, not causal": _logits("bf16", 33, 3, SMALL_LENS, 200, causal=False, q="padded", w="packed"),
    "h 64 heads, one page of 1024": _logits("bf16", 64, 1, (0, 700, 1024, 2000), 1024, q="padded", w="packed", k="one page", page=1024),
    "h 64 heads, 32 rows, QI transposed": _logits("f16", 64, 32, SMALL_LENS, 200, q="transposed", w="padded", k="paged", page=16),
    "h 40 heads, two rows, not causal": _logits("f16", 40, 2, SMALL_LENS, 200, causal=False, q="transposed", w="padded", k="strided"),
}
NEW_CASES = dict(STEP_CASES, **HEAD_CASES)
# the 24 launches tests/test_mla_index_gpu.py has always made (their VALUES are that file's problem(); see old_case_operands)
OLD_CASES = {"old %s %d heads %d rows %s" % (f, H, R, k): _logits(f, H, R, OLD_LENS, OLD_C, k=k, page=16 if k == "paged" else 0, problem=("old", f, H, R))
             for f in ("bf16", "f16") for H in (64, 40) for R in (1, 3) for k in ("contiguous", "strided", "paged")}
ALL_CASES = dict(OLD_CASES, **NEW_CASES)


@functools.lru_cache(maxsize=None)
def values(name):
    """(q [B, H, R, 128], w [B, R, H], k [B, C, 128]) float64, q and k values of the 16-bit type, w FP32 of both signs"""
    case = ALL_CASES[name]
    key = case["problem"] or name
    if isinstance(key, tuple):                                               # the old file's own inputs, bit for bit
        import test_mla_index_gpu as old
        pr = old.problem(*key[1:])
        return pr["q"].double().numpy(), pr["w"].double().numpy(), pr["k"].double().numpy()
    return _values(key, case["fmt"], case["H"], case["R"], len(case["lens"]), case["C"])


@functools.lru_cache(maxsize=None)
def _values(key, fmt, H, R, B, C):
    g = np.random.default_rng(zlib.crc32(key.encode()))
    q = round_to(g.standard_normal((B, H, R, DI)), fmt)
    k = round_to(g.standard_normal((B, C, DI)), fmt)
    w = g.standard_normal((B, R, H)).astype(np.float32).astype(np.float64)
    return q, w, k


_REFS = {}


def reference(q, w, k, lens=None, R=None, causal=True, column=None):
    """float64 logits [B, R, C] and their per-element bound, at EVERY position (visible() says which the launch owns; the lengths, R,
    causal and column are taken for the signature's sake and do not enter the values)"""
    B, H, R_, _ = q.shape
    C = k.shape[1]
    ref, bound = np.empty((B, R_, C)), np.empty((B, R_, C))
    for b in range(B):                                                       # per sequence: [H R, 128] x [128, C]
        s = (q[b].reshape(H * R_, DI) @ k[b].T).reshape(H, R_, C)
        mag = (np.abs(q[b]).reshape(H * R_, DI) @ np.abs(k[b]).T).reshape(H, R_, C)
        ref[b] = np.einsum("rh,hrc->rc", w[b], np.maximum(s, 0.0))
        bound[b] = 2.0 * ROUNDINGS * U32 * np.einsum("rh,hrc->rc", np.abs(w[b]), mag)
    return ref, bound


def reference_of(name):
    case = ALL_CASES[name]
    key = case["problem"] or name
    if key not in _REFS:
        q, w, k = values(name)
        _REFS[key] = reference(q, w, k, case["lens"], case["R"], case["causal"], case["C"])
    return _REFS[key]


@functools.lru_cache(maxsize=None)
def plan_of(name):
    """(steps, tiles, the logits launch's form) of a case, from the built library's launchForm: never re-derived here"""
    from metal_flash_attention_amd import AttentionMLAIndex, GEMMOperandPrecision as P
    case = ALL_CASES[name]
    kw = dict(rows=case["R"], column=case["C"], indexHeads=case["H"], batches=len(case["lens"]), cacheLengths=LENGTHS)
    if case["page"]:
        kw.update(pageSize=case["page"], blockTable=TABLE, blockTableStride=-(-case["C"] // case["page"]) + 2)
    form = AttentionMLAIndex(P.BF16 if case["fmt"] == "bf16" else P.FP16).launchForm(stage="logits", **kw)
    tiles, keys = (int(n) for n in re.search(r"(\d+) tiles of (\d+) keys", form).groups())
    assert keys % (STEP * WAVES) == 0
    return keys // (STEP * WAVES), tiles, form


# ------------------------------------------------------------------------------------------------------- the operands in memory
@functools.lru_cache(maxsize=None)
def layout(name):
    """dict(q, w, k: flat float32 arrays; qs = (ld, hs, bs); ws = (row, batch); ks = (ld, bs or 0, page stride or 0); table [B, stride]
    int32 or None, shift) -- every element no visible key needs is poison"""
    case = ALL_CASES[name]
    q, w, k = values(name)
    B, H, R, _ = q.shape
    C, lens, P = case["C"], case["lens"], case["page"]
    g = np.random.default_rng(7)
    big = lambda shape: (BIG * g.choice(np.array([-1.0, 1.0]), shape)).astype(np.float32)   # noqa: E731
    out = dict(B=B, H=H, R=R, C=C)
    if case["q"] == "packed":
        out.update(q=q.astype(np.float32).reshape(-1), qs=(DI, R * DI, H * R * DI))
    elif case["q"] == "transposed":                                          # a [B, R, H, Di] buffer viewed as [B, H, R, Di]
        out.update(q=np.ascontiguousarray(np.transpose(q, (0, 2, 1, 3)), dtype=np.float32).reshape(-1), qs=(H * DI, DI, R * H * DI))
    else:                                                                    # rows of Di + 8, a row and a head of padding
        buf = big((B, H + 1, R + 1, DI + 8))
        buf[:, :H, :R, :DI] = q
        out.update(q=buf.reshape(-1), qs=(DI + 8, (R + 1) * (DI + 8), (H + 1) * (R + 1) * (DI + 8)))
    if case["w"] == "packed":
        out.update(w=w.astype(np.float32).reshape(-1), ws=(H, R * H))
    else:                                                                    # a row stride wider than the heads, a row of batch padding
        buf = np.full((B, R + 1, H + 3), np.nan, dtype=np.float32)
        buf[:, :R, :H] = w
        out.update(w=buf.reshape(-1), ws=(H + 3, (R + 1) * (H + 3)))
    k = k.astype(np.float32)
    for b, n in enumerate(lens):
        k[b, n:] = np.nan
    out.update(table=None, shift=0)
    if case["k"] == "contiguous":
        out.update(k=k.reshape(-1), ks=(DI, C * DI, 0))
    elif case["k"] == "strided":
        buf = np.full((B, C, DI + 8), np.nan, dtype=np.float32)
        buf[:, :, :DI] = k
        out.update(k=buf.reshape(-1), ks=(DI + 8, C * (DI + 8), 0))
    else:
        pps = -(-C // P)
        one = case["k"] == "one page"                                        # blockTableStride = 1
        assert not one or pps == 1
        order = np.random.default_rng(5).permutation(B * pps).astype(np.int32).reshape(B, pps)
        pool = np.full((B * pps + 2, P, DI), np.nan, dtype=np.float32)
        pool[B * pps + 1] = big((P, DI))                                     # the unnamed pages: one of NaN, one of +-2^14
        table = np.empty((B, pps + (0 if one else 2)), dtype=np.int32)
        table[:] = B * pps + (np.arange(table.shape[1]) & 1)[None, :]
        for b, n in enumerate(lens):
            for i in range(-(-min(n, C) // P)):
                rows = k[b, i * P:(i + 1) * P]
                pool[order[b, i], :len(rows)] = rows
                table[b, i] = order[b, i]
        out.update(k=pool.reshape(-1), ks=(DI, 0, P * DI), table=table, shift=P.bit_length() - 1)
    return out


def _take(buf, idx):
    """buf[idx], NaN where an address leaves the allocation (the model cannot fault)"""
    ok = (idx >= 0) & (idx < buf.size)
    return np.where(ok, buf[np.clip(idx, 0, buf.size - 1)], np.float32(np.nan))


# -------------------------------------------------------------------------------------------------------- the logits kernel's walk
_CHAINS = {}


def _chain(Q, W, K, H, mutant):
    """the arithmetic of one sequence: Q [H, R, 128], W [R, H], K [n, 128] FP32 -> [R, n] FP32: the dot products in FP32 (any order: the
    bound covers every order), then per lane half the fma chain over its heads, block 0 then 1, and one add across the halves"""
    key = (hash(Q.tobytes()), hash(W.tobytes()), hash(K.tobytes()), Q.shape, K.shape, mutant)
    if key in _CHAINS:
        return _CHAINS[key]
    R, n = Q.shape[1], K.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        S = (Q.reshape(-1, DI) @ K.T).reshape(Q.shape[0], R, n)
        S = np.fmax(S, np.float32(0.0))                                     # fmaxf: NaN gives 0
        two = H > (33 if mutant == "second_block_from_34" else 32)
        halves = []
        for hi in (0, 1):
            acc = np.zeros((R, n), dtype=np.float32)
            for hb in ((0, 1) if two else (0,)):
                for r in range(16):
                    h = 32 * hb + crow(r, hi)
                    if h < H:                                                # (a head at or past H: fma(0, 0, acc) = acc)
                        acc = (W[:, h, None].astype(np.float64) * S[h].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
            halves.append(acc)
        total = halves[0] if mutant == "halves_not_added" else halves[0] + halves[1]
    _CHAINS[key] = total
    return total


def emulated_logits(name, mutant=None, plan=None):
    """the allocation [B + 1][R + 1][C + PADW] of FP32 sentinels after the logits launch of a case, as the kernel -- or a mutant -- fills it"""
    assert mutant is None or mutant in MUTANTS, mutant
    case, lay = ALL_CASES[name], layout(name)
    B, H, R, C, lens = lay["B"], lay["H"], lay["R"], lay["C"], case["lens"]
    steps, tiles = plan or plan_of(name)[:2]
    lrs, lbs = C + PADW, (R + 1) * (C + PADW)
    size = (B + 1) * lbs
    v = visible(lens, R, case["causal"], C, mutant)
    src = np.full(size, -1, dtype=np.int64)                                  # the key a position's value was computed from; -2: from zeros
    who = np.zeros(size, dtype=np.int64)                                     # ... by the workgroup of (batch, row): batch R + row
    walked = steps - 1 if mutant == "last_step_dropped" else steps
    # [wave][step][lane]: wave w of step s takes the keys tile0 + 32 (4 s + w) + lane
    offset = (STEP * np.arange(WAVES)[:, None, None] + STEP * WAVES * np.arange(walked)[None, :, None] + np.arange(STEP)[None, None, :]).astype(np.int64)
    first = offset[:, :1, :] if walked else offset
    for g in range(tiles * R * B if walked else 0):
        row, bt = g % R, g // R
        tile, batch = (bt // tiles, bt % tiles) if mutant == "tile_and_batch_exchanged" else (bt % tiles, bt // tiles)
        if batch >= B:
            continue
        vv = int(v[batch, row])
        tile0 = tile * STEP * WAVES * (1 if mutant == "tile0_ignores_steps" else steps)
        if tile0 >= vv:
            continue
        c = tile0 + offset                                                   # a step whose key0 is at or past v is not walked: no c < v in it
        held = np.broadcast_to(tile0 + first, c.shape) if mutant == "next_keys_not_taken" else c   # the keys in kreg
        at = batch * lbs + row * lrs + c
        st = (c < vv) & (at < size)
        src[at[st]] = np.where(held < vv, held, -2)[st]
        who[at[st]] = batch * R + row
    out = np.full(size, SENTINEL, dtype=np.float32)
    ldq, hsq, bsq = lay["qs"]
    wrs, wbs = lay["ws"]
    ldk, bsk, psk = lay["ks"]
    if mutant == "q_head_stride_packed":
        hsq = R * DI
    if mutant == "w_row_stride_packed":
        wrs = H
    d = np.arange(DI)
    for b in range(B):
        mine = (who // R == b) & (src != -1)
        if not mine.any():
            continue
        n = int(src[mine].max()) + 1
        Q = _take(lay["q"], b * bsq + np.arange(H)[:, None, None] * hsq + np.arange(R)[None, :, None] * ldq + d[None, None, :])
        if mutant == "head_32_left_out":
            Q[H - 1] = 0.0
        W = _take(lay["w"], b * wbs + np.arange(R)[:, None] * wrs + np.arange(H)[None, :])
        c = np.arange(max(n, 1))
        if lay["table"] is None:
            base = b * bsk + c * ldk
        else:
            P = 1 << lay["shift"]
            of = (c // STEP * STEP) if mutant == "page_of_the_first_lane" else c
            flat = lay["table"].reshape(-1).astype(np.int64)
            entry = b * lay["table"].shape[1] + (of >> lay["shift"])
            base = np.where(entry < flat.size, flat[np.minimum(entry, flat.size - 1)] * psk + (c & (P - 1)) * ldk, -10 ** 12)   # (past the table: no page)
        K = _take(lay["k"], base[:, None] + d[None, :])
        L = _chain(Q, W, K, H, mutant if mutant in ("second_block_from_34", "halves_not_added") else None)
        at = np.nonzero(mine)[0]
        s_ = src[at]
        out[at] = np.where(s_ >= 0, L[who[at] % R, np.maximum(s_, 0)], np.float32(0.0))
    return out.reshape(B + 1, R + 1, C + PADW)


def verdict(alloc, name, causal=None):
    """worst err / bound of a filled allocation; inf where a sentinel the launch does not own was touched, an owned position was not
    written (it still holds the sentinel: far outside) or is NaN"""
    case = ALL_CASES[name]
    ref, bound = reference_of(name)
    B, R, C = ref.shape
    v = visible(case["lens"], R, case["causal"] if causal is None else causal, C)
    seen = np.arange(C + PADW)[None, None, :] < np.pad(v, ((0, 1), (0, 1)))[:, :, None]
    if not (alloc[~seen] == SENTINEL).all():
        return np.inf
    inside = seen[:B, :R, :C]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.abs(alloc[:B, :R, :C].astype(np.float64) - ref)[inside] / bound[inside]
    if ratio.size == 0:
        return 0.0
    return float(np.where(np.isnan(ratio), np.inf, ratio).max())


def logit_facts(name):
    """what a logits mutant's `harmless` rule is asked about"""
    case = ALL_CASES[name]
    steps, tiles, _form = plan_of(name)
    return dict(H=case["H"], R=case["R"], B=len(case["lens"]), causal=case["causal"], C=case["C"], longest=max(case["lens"]), page=case["page"],
                steps=steps, tiles=tiles, q=case["q"], w=case["w"])


# ------------------------------------------------------------------------------------------------------------------- the selection
def order_key(x):
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return bits ^ np.where(bits >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def select_ref(x, v, topk):
    order = np.lexsort((np.arange(v), -order_key(x[:v]).astype(np.int64)))[:topk]     # larger key first, then lower position
    return np.concatenate([np.sort(order), np.full(topk - len(order), -1)]).astype(np.int32)


def emulated_select(x, v, topk, mutant=None):
    """the list [topk] of one row as the select kernel writes it into slots that hold UNWRITTEN; x is the row where it lies (at least v
    logits)"""
    assert mutant is None or mutant in MUTANTS, mutant
    out = np.full(topk, UNWRITTEN, dtype=np.int32)
    if v <= topk:
        i = np.arange(topk)
        return np.where(i < v, i, -1).astype(np.int32)
    key = order_key(x[:v]).astype(np.int64)
    if mutant == "nan_below_everything":
        key = np.where(np.isnan(x[:v]), 0, key)
    prefix = mask = 0
    want, pick = topk, (0, 0)
    for shift in (24, 16, 8, 0):
        cand = key[(key & mask) == prefix]
        hist = np.bincount((cand >> shift) & 255, minlength=256)
        above = np.concatenate([np.cumsum(hist[::-1])[::-1][1:], [0]])       # the candidates of higher bins
        hit = np.nonzero((above < want) & (want <= above + hist))[0]
        if len(hit):                                                         # (true for exactly one bin of a correct kernel; else pick is stale)
            pick = (int(hit[0]), want if mutant == "want_not_reduced" else want - int(above[hit[0]]))
        prefix |= pick[0] << shift
        mask |= 0xFF << shift
        want = pick[1]
    greater_base = tie_base = 0
    before = np.zeros((2, ROUND // 64), dtype=np.int64)                      # the round before's (u, wave) totals
    for i0 in range(0, v, ROUND):
        if mutant == "stops_a_round_early" and i0 + ROUND >= v:
            break
        if mutant == "tie_base_not_carried":
            tie_base = 0
        if mutant == "greater_base_not_carried":
            greater_base = 0
        seg = np.full(ROUND, -1, dtype=np.int64)
        seg[:min(ROUND, v - i0)] = key[i0:i0 + ROUND]
        flags = np.stack([seg > prefix, (seg == prefix)]).astype(np.int64).reshape(2, ROUND // 64, 64)   # [greater | tie][(u, wave)][lane]
        inwave = np.cumsum(flags, axis=2) - flags
        totals = flags.sum(axis=2)
        used = before if mutant == "totals_of_the_round_before" else totals
        bases = np.cumsum(used, axis=1) - used
        g_before = (inwave[0] + bases[0][:, None] + greater_base).reshape(-1)
        t_before = (inwave[1] + bases[1][:, None] + tie_base).reshape(-1)
        greater_base += int(used[0].sum())
        tie_base += int(used[1].sum())
        before = totals
        slot = g_before + np.minimum(t_before, want)
        g, t = flags[0].reshape(-1) != 0, flags[1].reshape(-1) != 0
        write = (g | (t & (t_before < want))) & (slot < topk)
        out[slot[write]] = i0 + np.nonzero(write)[0]                         # (ascending position: a slot written twice keeps the later one)
        if greater_base + min(tie_base, want) >= topk:
            break
    return out


def select_facts(x, v, topk, lrs=None, column=None, R=1):
    """what a select mutant's `harmless` rule is asked about, for ONE row: the true threshold's counts per round of 4096"""
    f = dict(v=v, topk=topk, reads=v > topk, packed=lrs in (None, column) or R == 1, nan=False, rounds=0, g=[], t=[], want=0)
    if v <= topk:
        return f
    key = order_key(x[:v]).astype(np.int64)
    T = np.sort(key)[::-1][topk - 1]
    g = [int((key[i:i + ROUND] > T).sum()) for i in range(0, v, ROUND)]
    t = [int((key[i:i + ROUND] == T).sum()) for i in range(0, v, ROUND)]
    want = topk - sum(g)
    walked = len(g)
    for i in range(len(g)):
        if sum(g[:i + 1]) + min(sum(t[:i + 1]), want) >= topk:
            walked = i + 1
            break
    f.update(nan=bool(np.isnan(x[:v]).any()), rounds=walked, g=g[:walked], t=t[:walked], want=want, all_rounds=len(g))
    return f


VALUES = {   # the old file's five
    "normal": lambda g, n: g.standard_normal(n),
    "equal": lambda g, n: np.full(n, 0.5),
    "ties": lambda g, n: g.choice(np.array([-1.0, -0.0, 0.0, 1.0], dtype=np.float32), n),
    "low bits": lambda g, n: (np.uint32(0x3F800000) | g.integers(0, 256, n).astype(np.uint32)).view(np.float32),
    "negative": lambda g, n: -np.abs(g.standard_normal(n)) - 0.25,
}


def _specials(g, n):
    x = g.standard_normal(n).astype(np.float32)
    odd = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,
                    0x00000000, 0x80000000], dtype=np.uint32).view(np.float32)   # NaN of both signs, +-inf, denormals, +-0
    at = g.random(n) < 0.25
    x[at] = g.choice(odd, int(at.sum()))
    return x


def _byte(shift, base):
    return lambda g, n: (np.uint32(base) | (g.integers(0, 256, n).astype(np.uint32) << np.uint32(shift))).view(np.float32)


# positions are laid out per row of `column`: a set that depends on the position takes n = rows x column in row-major order
NEW_VALUES = dict(VALUES, **{
    "specials": _specials,
    "digit 1": _byte(8, 0x3F800000),      # the keys differ in one byte only: the threshold is found in that pass and the ties are heavy
    "digit 2": _byte(16, 0x3F000000),
    "digit 3": _byte(24, 0x00400000),     # sign and exponent: 0x00400000 .. 0xFF400000, all finite
})
SELECT_COLUMN, SELECT_PAD = 20000, 8


def _two_levels(g, n):
    """0.5 everywhere, 1.0 in the LAST round of every row of 20000: the greater keys sit only there, the admitted ties in the first"""
    x = np.full(n, 0.5, dtype=np.float32).reshape(-1, SELECT_COLUMN)
    x[:, 4 * ROUND:] = 1.0
    return x.reshape(-1)


NEW_VALUES["two levels"] = _two_levels


def _select(values, topk, column=SELECT_COLUMN, R=2, pad=SELECT_PAD, lens=None):
    if lens is None:   # v = n - 1 and n: around topk, around every round's end, the column and past it
        lens = sorted({0, 1, topk, topk + 1, topk + 2, ROUND, ROUND + 1, 2 * ROUND + 1, 3 * ROUND + 1, 4 * ROUND + 1, column - 1, column, column + 5000})
    return dict(values=values, topk=topk, column=column, R=R, pad=pad, lens=tuple(lens))


OLD_SELECT_CASES = {"old %s top %d" % (name, topk): _select(name, topk, 5000, 2, 0, sorted({0, 1, 2, topk - 1, topk, topk + 1, topk + 2, 5000}))
                    for topk in (1, 33, 2048) for name in VALUES}
NEW_SELECT_CASES = {
    "s equal top 4097": _select("equal", 4097), "s equal top 8193": _select("equal", 8193), "s equal top 19999": _select("equal", 19999),
    "s two levels top 5000": _select("two levels", 5000), "s two levels top 33": _select("two levels", 33),
    "s normal top 5000": _select("normal", 5000), "s normal top 4097": _select("normal", 4097), "s normal top 1": _select("normal", 1),
    "s ties top 8193": _select("ties", 8193), "s low bits top 5000": _select("low bits", 5000),
    "s digit 1 top 2048": _select("digit 1", 2048), "s digit 2 top 4097": _select("digit 2", 4097), "s digit 3 top 5000": _select("digit 3", 5000),
    "s specials top 33": _select("specials", 33), "s specials top 5000": _select("specials", 5000), "s specials top 19999": _select("specials", 19999),
    "s negative top 2048": _select("negative", 2048),
}
ALL_SELECT_CASES = dict(OLD_SELECT_CASES, **NEW_SELECT_CASES)


@functools.lru_cache(maxsize=None)
def select_inputs(name):
    """(case, v [B, R], the logits allocation [B, R, column + pad] float32: NaN at and past v and in the padding)"""
    case = ALL_SELECT_CASES[name]
    column, R, lens, topk = case["column"], case["R"], case["lens"], case["topk"]
    B, v = len(lens), visible(lens, R, True, column)
    if name in OLD_SELECT_CASES:                                             # the old file's own draw
        x = VALUES[case["values"]](np.random.default_rng(topk), B * R * column).astype(np.float32).reshape(B, R, column)
    else:
        x = NEW_VALUES[case["values"]](np.random.default_rng(zlib.crc32(name.encode())), B * R * column).astype(np.float32).reshape(B, R, column)
    x = np.concatenate([x, np.full((B, R, case["pad"]), np.nan, dtype=np.float32)], axis=2)
    x[np.arange(column + case["pad"])[None, None, :] >= v[:, :, None]] = np.nan
    return case, v, x


@functools.lru_cache(maxsize=None)
def select_wanted(name):
    """int32 [B, R, topk]: select_ref of every row"""
    case, v, x = select_inputs(name)
    return np.stack([np.stack([select_ref(x[b, r], int(v[b, r]), case["topk"]) for r in range(case["R"])]) for b in range(len(case["lens"]))])


def emulated_selection(name, mutant=None):
    """emulated_select over every row of a case, each read where it lies in the allocation (a mutant of the row stride reads elsewhere)"""
    case, v, x = select_inputs(name)
    B, R, width = x.shape
    lrs = case["column"] if mutant == "logit_row_stride_packed" else width
    flat = np.concatenate([x.reshape(-1), np.full(width, np.nan, dtype=np.float32)])
    return np.stack([np.stack([emulated_select(flat[b * R * width + r * lrs:][:width], int(v[b, r]), case["topk"], mutant) for r in range(R)])
                     for b in range(B)])


def select_rows_facts(name):
    case, v, x = select_inputs(name)
    return [select_facts(x[b, r], int(v[b, r]), case["topk"], x.shape[2], case["column"], case["R"] if r else 1)
            for b in range(x.shape[0]) for r in range(case["R"])]


# ---------------------------------------------------------------------------------------------------------------------- the mutants
def _carried(f, what):
    """no round after the first meets a non-zero base of `what`"""
    return all(sum(f[what][:i]) == 0 for i in range(1, f["rounds"]))


LOGIT_MUTANTS = {
    "next_keys_not_taken": ("step s + 1 multiplies step s's keys: kreg = knext left out", lambda f: f["steps"] == 1),
    "tile0_ignores_steps": ("tile0 = tile x 128, without the steps", lambda f: f["steps"] == 1 or f["tiles"] == 1),
    "last_step_dropped": ("s + 1 < steps applied to the compute loop", lambda f: False),
    "tile_and_batch_exchanged": ("bt / tiles taken for the tile and bt % tiles for the sequence", lambda f: f["B"] == 1 and f["tiles"] == 1),
    "second_block_from_34": ("two = H > 33: the second head block of 33 heads skipped", lambda f: f["H"] != 33),
    "head_32_left_out": ("head < H - 1 on the load: the last head's queries are zeros", lambda f: False),
    "length_not_clamped": ("cacheLengths[b] not clamped to column", lambda f: f["longest"] <= f["C"]),
    "causal_ignored": ("every row sees the whole length", lambda f: not f["causal"] or f["R"] == 1),
    "causal_forced": ("the causal frontier applied to a launch without `causal`", lambda f: f["causal"] or f["R"] == 1),
    "frontier_off_by_one": ("v = min(n, r + max(n - R, 0)): the row's own key hidden", lambda f: not f["causal"]),
    "q_head_stride_packed": ("R x 128 used for QI's head stride", lambda f: f["q"] == "packed" or f["H"] == 1),
    "w_row_stride_packed": ("indexHeads used for W's row stride", lambda f: f["w"] == "packed" or f["R"] == 1),
    "page_of_the_first_lane": ("every lane of a wave uses lane 0's page", lambda f: f["page"] == 0 or f["page"] >= STEP),
    "halves_not_added": ("the add across the lane halves left out", lambda f: f["H"] <= 4),
}
SELECT_MUTANTS = {
    "tie_base_not_carried": ("tieBase restarts at 0 every round", lambda f: not f["reads"] or _carried(f, "t")),
    "greater_base_not_carried": ("greaterBase restarts at 0 every round", lambda f: not f["reads"] or _carried(f, "g")),
    "want_not_reduced": ("a pass hands `want` on without taking off the candidates above the bin", lambda f: not f["reads"] or sum(f["g"]) == 0),
    "totals_of_the_round_before": ("the ordered pass reads totals[buf ^ 1]", lambda f: not f["reads"]),
    "nan_below_everything": ("a NaN's key is 0: below every number", lambda f: not f["reads"] or not f["nan"]),
    "logit_row_stride_packed": ("column used for the logits' row stride", lambda f: not f["reads"] or f["packed"]),
    "stops_a_round_early": ("the ordered pass leaves out the last round of [0, v)", lambda f: not f["reads"] or f["rounds"] < f["all_rounds"]),
}
MUTANTS = dict(LOGIT_MUTANTS, **SELECT_MUTANTS)
# the mutants no launch of tests/test_mla_index_gpu.py could see (tests/test_mla_index_sensitivity.py proves each): the gap
NEW_MUTANTS = ("next_keys_not_taken", "tile0_ignores_steps", "second_block_from_34", "length_not_clamped", "causal_forced", "q_head_stride_packed",
               "w_row_stride_packed", "nan_below_everything", "logit_row_stride_packed")
