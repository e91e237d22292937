"""The float64 model of logit soft-capping over a KV cache (include/mfa_softcap.h), decode and prefill, with bounds, needle inputs,
a rounding-emulated reference and named mutants (a plain module; numpy only).  Formats, bounds and comparison are
tests/decode_model.py's; frontiers, visible keys, chains, piece and tile ranges, the sink fold and the needles tests/sink_model.py's
(which takes the window's from tests/window_model.py): nothing of them is repeated or edited here.

The rule.  raw = q . k, s = raw keyScale / sqrt(D) the natural-unit score the softmax sees without a cap; with cap > 0 it sees
s' = cap tanh(s / cap) -- on VISIBLE keys only (sink_model's rule of visibility, unchanged).  The sink logit is neither capped nor
scaled; L = log(sum e^s' + e^sink); a live row without a visible key has O = 0 and L = the logit (-inf without one).

  model()      float64 attention over the visible keys with the capped scores, sink_model's sink fold and chains (the tiles walked
               do not change with a cap), and the terms of decode_model's bound with ONE more term in a score's error:
                 * tanh is 1-Lipschitz, so the error e_i of the uncapped score (decode_model: (D + 3) u scale2 sum |q k|) passes through
                   cap tanh(. / cap) unamplified;
                 * the arithmetic of the tanh adds C_T u cap log2(e) in base-2 units, C_T = 12, counted on the formula the kernels use
                   (attn_cache_step.h): y = c2 (1 - 2 rcp(1 + exp2(kc raw))), kc = fl(fl(scale2 keyScale) c1), c1 = fl(2 / cap),
                   c2 = fl(cap fl(log2 e)).  With x = s / cap, t = tanh x, E = e^(2x), d = 1 + E, t = 1 - 2 / d; u = 2^-24 per rounding:
                     - the argument carries two roundings that the uncapped score does not (c1 and the product with it): relative
                       2 u on x, which moves t by (1 - t^2) |x| 2 u <= 0.45 x 2 u = 0.9 u       ((1 - t^2) |x| <= 0.45 for every x)
                     - v_exp_f32, one ulp = 2 u relative on E: dt = 2 E / d^2 x 2 u = (1 - t^2) u <= 1 u
                     - d = fl(1 + E), u relative: dt = (2 / d) u = (1 - t) u <= 2 u
                     - v_rcp_f32, one ulp = 2 u relative on 1 / d: dt = (1 - t) 2 u <= 4 u
                     - 2 r is exact; fl(1 - 2 r): |t| u <= 1 u                                  (the cancellation near 0: ABSOLUTE u)
                     - c2 carries two roundings and the product with t one: 3 u relative on y, |y| <= c2
                   in all (0.9 + 1 + 2 + 4 + 1 + 3) u c2 = 11.9 u c2 <= 12 u c2.  Derived, not tuned.
               The spread term of the bound is that of the capped scores (what s - m and the rescales see).
  emulated()   the kernels' order of operations -- sink_model.emulated's walk, fold and merge -- on scores from the FP32 tanh formula
               above, every step of it rounded to FP32 (exp2 overflowing to +inf as v_exp_f32 does).
  needle_queries()  sink_model's needles, each row scaled so that the best of its needle keys scores max(3 cap, 64) in natural units: several caps,
               and with cap = 1 at least 64 caps, where e^(2x) overflows FP32.
  mutated()    a named WRONG capped attention (MUTANTS), float64 -- except "naive_tanh", the overflowing formula in FP32.

MARGIN is decode_model's protocol: the smallest power of two with 2 x headroom over the worst err / bound at margin 1 of emulated() on
the cases of tests/test_softcap_sensitivity.py and of the kernels on those of tests/test_softcap_gpu.py (DESIGN.md 4.16 records both).
"""
import math

import numpy as np

import decode_model as dm
import sink_model as sm
import window_model as wm

TILE, STEP, WAVES, ROWS = sm.TILE, sm.STEP, sm.WAVES, sm.ROWS
C_T = 12               # roundings of the tanh arithmetic, in units of u cap log2(e) (derived in the module's text)
MARGIN = dm.MARGIN     # nothing new is fixed here: decode_model's margin holds with the one new term

frontiers, visible_keys = sm.frontiers, sm.visible_keys


def capped(s, cap):
    """cap tanh(s / cap), float64; cap None: s"""
    return s if cap is None else cap * np.tanh(s / cap)


def _visible(n, qn, rows, W, S, causal, npad):
    lo, lim = frontiers(n, qn, rows, W, causal)
    cols = np.arange(npad)[None, :]
    return (cols < lim[:, None]) & ((cols >= lo[:, None]) | (cols < S))


def _chains(kind, n, qn, R, G, W, S, causal, pieces, logits, piece_range, tile_range):
    """row -> the chain length of its workgroup (sink_model's counts: the walked tiles do not change with a cap)"""
    if kind == "decode":
        c = sm.chain_decode(sm.piece_ranges(n, R, W, S, pieces, piece_range), logits)
        return np.full(qn, c)
    tr = tile_range or sm.library_tile_range
    out = np.zeros(qn)
    for r0, r1 in wm.blocks_of(kind, qn, G):
        bt, _u0, _u1, et, se = tr(n, qn, r0, ROWS // G, causal, W, S)
        out[r0:r1] = sm.chain_prefill(se, bt, et, logits)
    return out


# ---------------------------------------------------------------------------------------------------------------------- the model
def model(q, k, v, lens, qlens, G, W, S=0, logits=None, cap=None, *, causal=True, pieces=None, kscale=None, vscale=None, piece_range=None,
          tile_range=None):
    """q [B, Hq, R, D], k / v [B, Hkv, C, D] (WITHOUT the scales when kscale / vscale are given), logits [Hq] natural units or None,
    cap > 0 natural units or None (no cap: sink_model.model's values) -> dm.Reference over [B, Hq, R].  qlens None: decode."""
    q, k, v = dm.f64(q), dm.f64(k), dm.f64(v)
    B, Hq, R, D = q.shape
    Hkv = Hq // G
    kind = "decode" if qlens is None else "prefill"
    ks = np.ones(Hkv) if kscale is None else np.asarray(kscale, dtype=np.float64)
    vs = np.ones(Hkv) if vscale is None else np.asarray(vscale, dtype=np.float64)
    sink = None if logits is None else np.asarray(logits, dtype=np.float64)
    O, A, E = (np.zeros((B, Hq, R, D)) for _ in range(3))
    L = np.full((B, Hq, R), -np.inf)
    EL = np.zeros((B, Hq, R))
    for b in range(B):
        n, qn = int(lens[b]), R if qlens is None else min(int(qlens[b]), R)
        if qn == 0:
            continue
        vis = _visible(n, qn, np.arange(qn), W, S, causal, max(n, 1))[:, :n]
        seen = vis.any(axis=1)
        chain = _chains(kind, n, qn, R, G, W, S, causal, pieces, sink is not None, piece_range, tile_range) * dm.U32
        for h in range(Hq):
            j = h // G
            if sink is not None:   # (rows without a visible key; the others are overwritten below)
                L[b, h, :qn] = np.where(seen, -np.inf, sink[h])
                EL[b, h, :qn] = np.where(seen, 0.0, 4 * dm.U32 * abs(sink[h]))
            if not seen.any():
                continue
            K, V, qh = k[b, j, :n], v[b, j, :n], q[b, h, :qn]
            Sc = np.where(vis, capped((qh @ K.T) * (ks[j] / math.sqrt(D)), cap), -np.inf)
            m = Sc.max(axis=1, keepdims=True)
            m0 = np.where(np.isfinite(m), m, 0.0)
            pw = np.exp(Sc - m0)
            l0 = np.where(seen, pw.sum(axis=1), 1.0)
            P = pw / l0[:, None]
            absV = np.abs(V) * abs(vs[j])
            o0, a0 = (P @ V) * vs[j], P @ absV
            lse = m0[:, 0] + np.log(l0)
            e2 = (D + 3) * dm.U32 * (dm.LOG2E * abs(ks[j]) / math.sqrt(D)) * (np.abs(qh) @ np.abs(K).T)
            if cap is not None:
                e2 = e2 + C_T * dm.U32 * cap * dm.LOG2E
            smin = np.where(vis, Sc, np.inf).min(axis=1, keepdims=True)
            spread2 = np.where(seen[:, None], (m0 - np.where(np.isfinite(smin), smin, m0)) * dm.LOG2E, 0.0)
            rel = dm.LN2 * (e2 + 3 * dm.U32 * spread2) + 4 * dm.U32
            relp = (rel * P).sum(axis=1)
            w = np.ones(qn) if sink is None else 1.0 / (1.0 + np.exp(sink[h] - lse))
            ow, aw = o0 * w[:, None], a0 * w[:, None]
            lfull = lse if sink is None else np.logaddexp(lse, sink[h])
            e = ((rel * P) @ absV + np.abs(o0) * relp[:, None]) * w[:, None] + chain[:, None] * (aw + np.abs(ow))
            el = relp + chain + 4 * dm.U32 * (np.abs(m0[:, 0]) + np.abs(np.log(l0)) + np.abs(lse))
            if sink is not None:
                el = el + 4 * dm.U32 * (abs(sink[h]) + np.abs(lfull))
            keep = seen[:, None]
            O[b, h, :qn], A[b, h, :qn], E[b, h, :qn] = np.where(keep, ow, 0.0), np.where(keep, aw, 0.0), np.where(keep, e, 0.0)
            L[b, h, :qn] = np.where(seen, lfull, L[b, h, :qn])
            EL[b, h, :qn] = np.where(seen, el, EL[b, h, :qn])
    return dm.Reference(O, L, A, E, EL)


bounds = dm.bounds
compare = sm.compare


# ------------------------------------------------------------------------------------------------- the rounding-emulated reference
def f32(x):
    return np.asarray(x, dtype=np.float32)


def capped_fp32(raw, scale2, keyscale, cap, naive=False):
    """the kernels' capped base-2 score from the raw dot products (float64 -> float64 values of FP32), every step rounded to FP32:
    c2 (1 - 2 rcp(1 + exp2(kc raw))).  naive: (E - 1) / (E + 1), the form that is inf / inf once E overflows"""
    one, two = np.float32(1.0), np.float32(2.0)
    kc = f32(f32(f32(scale2) * f32(keyscale)) * f32(two / np.float32(cap)))
    c2 = f32(np.float32(cap) * np.float32(1.44269504089))
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp2(f32(f32(raw) * kc))
        t = (e - one) / (e + one) if naive else one - two * (one / (one + e))
        return (c2 * t).astype(np.float64)


def emulated(q, k, v, lens, qlens, G, W, S, logits, cap, fmt, *, causal=True, pieces=None, kscale=None, vscale=None, piece_range=None,
             tile_range=None, naive=False):
    """-> (O before the store's rounding [B, Hq, R, D], L natural): sink_model.emulated's roundings and order of sums on the scores of
    capped_fp32 (cap None: sink_model.emulated itself)"""
    if cap is None:
        return sm.emulated(q, k, v, lens, qlens, G, W, S, logits, fmt, causal=causal, pieces=pieces, kscale=kscale, vscale=vscale,
                           piece_range=piece_range, tile_range=tile_range)
    B, Hq, R, D = q.shape
    ks = np.ones(Hq // G) if kscale is None else np.asarray(kscale, dtype=np.float64)
    scale2 = np.float32(1.44269504089) / np.sqrt(np.float32(D))
    bad = np.zeros((B, Hq, R), dtype=bool)   # (naive only.  fmaxf drops a NaN score, its exp2 does not: P, l and O of the row are NaN)

    def score(raw, vis, b, h, rows):
        S2 = np.where(vis, capped_fp32(raw, scale2, ks[h // G], cap, naive), -np.inf)
        bad[b, h, rows] = np.isnan(S2).any(axis=1)
        return np.where(np.isnan(S2), -np.inf, S2)

    O, L = sm.emulated(q, k, v, lens, qlens, G, W, S, logits, fmt, causal=causal, pieces=pieces, vscale=vscale, piece_range=piece_range,
                       tile_range=tile_range, score=score)
    return np.where(bad[..., None], np.nan, O), np.where(bad, np.nan, L)


# ------------------------------------------------------------------------------------------------------------------ needle inputs
def needle_score(cap):
    """what a row's needle keys score, natural units: several caps, and at least 64 (cap = 1: e^(2 s / cap) overflows FP32)"""
    return max(3.0 * cap, 64.0)


def needle_queries(k, lens, qlens, Hq, G, R, W, S, fmt, cap, **kw):
    """sink_model.needle_queries, every needle row scaled so that the best of its needle keys scores needle_score(cap) -- the cap must
    matter.  (Rows without a visible key, and the few rows whose only needle weighs nothing, stay as they are.)  -> (q, info)"""
    q, info = sm.needle_queries(k, lens, qlens, Hq, G, R, W, S, fmt, **kw)
    k = dm.f64(k)
    D = k.shape[3]
    for (b, h, r), (weights, _forbidden) in info.items():
        best = float((k[b, h // G, sorted(weights)] @ q[b, h, r]).max()) / math.sqrt(D)
        if best > 0.5:
            q[b, h, r] *= needle_score(cap) / best
    return dm.round_to(q, fmt), info


# ---------------------------------------------------------------------------------------------------------------------- mutants
MUTANTS = {
    "cap_ignored": "the scores are not capped",
    "cap_not_multiplied_back": "tanh(s / cap) not multiplied back by cap",
    "cap_on_raw_dot": "the cap applied to the raw dot product, before 1 / sqrt(D)",
    "cap_in_base2_units": "the cap taken in base-2 units: c2 = cap in place of cap log2(e) and c1 on the base-2 score",
    "key_scale_after_cap": "the e4m3 keyScale applied after the cap instead of before",
    "sink_logit_capped": "the sink logit passed through the cap",
    "l_of_uncapped_scores": "L of the uncapped scores",
    "naive_tanh": "tanh as (e^2x - 1) / (e^2x + 1) in FP32: inf / inf once e^2x overflows",
}
L_ONLY = ("l_of_uncapped_scores",)   # defects that leave O as it is: they show in L


def mutated(q, k, v, lens, qlens, G, W, S, logits, cap, mutant, *, causal=True, kscale=None, vscale=None, fmt="bf16", **_geometry):
    """float64 capped attention with the named defect (None: without one) -> (O [B, Hq, R, D], L natural [B, Hq, R], changed).
    `changed`: whether the defect computes anything else -- always, but for key_scale_after_cap without scales, sink_logit_capped without
    logits, cap_not_multiplied_back at cap = 1 and naive_tanh where nothing overflows (it is then the same function up to rounding).  naive_tanh: emulated() with that form"""
    assert mutant is None or mutant in MUTANTS, mutant
    if mutant == "naive_tanh":
        O, L = emulated(q, k, v, lens, qlens, G, W, S, logits, cap, fmt, causal=causal, kscale=kscale, vscale=vscale, naive=True, **_geometry)
        return O, L, bool(np.isnan(O).any() or np.isnan(L).any())
    q, k, v = dm.f64(q), dm.f64(k), dm.f64(v)
    B, Hq, R, D = q.shape
    Hkv = Hq // G
    ks = np.ones(Hkv) if kscale is None else np.asarray(kscale, dtype=np.float64)
    vs = np.ones(Hkv) if vscale is None else np.asarray(vscale, dtype=np.float64)
    sink = None if logits is None else np.asarray(logits, dtype=np.float64)
    changed = mutant is not None and not (mutant == "key_scale_after_cap" and kscale is None) and not (mutant == "sink_logit_capped" and sink is None) \
        and not (mutant == "cap_not_multiplied_back" and cap == 1.0)
    O = np.zeros((B, Hq, R, D))
    L = np.full((B, Hq, R), -np.inf)
    for b in range(B):
        n, qn = int(lens[b]), R if qlens is None else min(int(qlens[b]), R)
        if qn == 0:
            continue
        vis = _visible(n, qn, np.arange(qn), W, S, causal, max(n, 1))[:, :n]
        seen = vis.any(axis=1)
        for h in range(Hq):
            j = h // G
            if not seen.any():   # (no row sees a key: O = 0, L = the sink logit as the defect has it)
                if sink is not None:
                    L[b, h, :qn] = float(capped(sink[h], cap)) if mutant == "sink_logit_capped" else sink[h]
                continue
            raw = q[b, h, :qn] @ k[b, j, :n].T
            s = raw * (ks[j] / math.sqrt(D))
            if mutant == "cap_ignored":
                sc = s
            elif mutant == "cap_not_multiplied_back":
                sc = np.tanh(s / cap)
            elif mutant == "cap_on_raw_dot":
                sc = capped(raw, cap) * (ks[j] / math.sqrt(D))
            elif mutant == "cap_in_base2_units":
                sc = capped(s * dm.LOG2E, cap) / dm.LOG2E
            elif mutant == "key_scale_after_cap":
                sc = capped(raw / math.sqrt(D), cap) * ks[j]
            else:
                sc = capped(s, cap)
            Sc = np.where(vis, sc, -np.inf)
            m = Sc.max(axis=1, keepdims=True)
            m0 = np.where(np.isfinite(m), m, 0.0)
            pw = np.exp(Sc - m0)
            l0 = np.where(seen, pw.sum(axis=1), 1.0)
            o = np.where(seen[:, None], (pw / l0[:, None]) @ v[b, j, :n] * vs[j], 0.0)
            lse = np.where(seen, m0[:, 0] + np.log(l0), -np.inf)
            if mutant == "l_of_uncapped_scores":
                Su = np.where(vis, s, -np.inf)
                mu = np.where(seen, Su.max(axis=1), 0.0)
                lse_out = np.where(seen, mu + np.log(np.where(seen, np.exp(Su - mu[:, None]).sum(axis=1), 1.0)), -np.inf)
            else:
                lse_out = lse
            if sink is not None:
                t = float(capped(sink[h], cap)) if mutant == "sink_logit_capped" else sink[h]
                o = o * (1.0 / (1.0 + np.exp(t - lse)))[:, None]
                lse_out = np.logaddexp(lse_out, t)
            O[b, h, :qn], L[b, h, :qn] = o, lse_out
    return O, L, changed
