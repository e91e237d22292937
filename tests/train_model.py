"""The float64 model of training attention (forward, dQ, dK/dV) on a [B, H, R | C, D] grid, its per-element error bounds, the needle
inputs and the named mutants (a plain module, as tests/decode_model.py, whose rounding helpers and constants it reuses; numpy only).

  model()           float64 O, L (natural units), D = rowsum(dO O), dV, dK, dQ under the library's causal rule and per-batch length
                    rule (include/mfa.h: row r of entry b sees column c iff c < columnLengths[b] and, causal, c <= r +
                    max(columnLengths[b] - rowLengths[b], 0)), the magnitude sums of the bounds and the bounds' error terms.
                    mutant= computes a named WRONG attention instead (MUTANTS).  No wrong kernel is ever run.
                    block_mask= (model, emulated, needle_inputs, needle_plan): bool [row blocks, column blocks], shared by the grid,
                    or [B, H, row blocks, column blocks]; blocks of BLOCK_ROWS = 256 rows x MASK_COLUMNS = 128 keys
                    (MFA_MASK_BLOCK_ROWS, MFA_MASK_BLOCK_COLUMNS).  Row r sees key c iff the rule above holds AND the bit of
                    (r // 256, c // 128) is set.  A live row that sees no key is DEAD: O = dQ = D = 0 exactly, no contribution to
                    dK / dV, L hugely negative (include/mfa.h; the model says -inf, compare() asks for < -1e30 and for exact zeros).
                    The bound needs no new term: every sum runs over the visible (i, j) with the model's p, and the FP32 chain
                    keeps C / 8, an upper bound on the matrix instructions of the blocks that are run.
                    out= (the type O, dQ, dK, dV are stored in), dO_fmt= / dO_path= (the FP16 + BF16-dO mix), heads_per_kv= (K, V,
                    dK, dV of H / G heads): the launch forms of the torch binding, derived at the end of the bound below.
  bounds()          per-element bounds on all six outputs (derivation below).
  emulated()        the same computation with the kernels' roundings and summation orders: what a correct kernel may give.
  needle_inputs()   Q, K, V and dO in which individual keys and individual rows matter; under a mask the needles are keys the row
                    sees and a small set of TRAP keys it must not see is left unsuppressed (needle_plan).
  needle_mask()     a random mask with what the needle plan asks for (neighbouring row blocks that differ both ways, run edges).
  compare()         got against model under the bounds: worst err / bound per output and where; padding must keep the buffer's value.
  fmt = "f32"       model(), bounds(), emulated(), needle_inputs() and compare() take FP32 operands (the bound: the end of this text);
                    needle_inputs(spike= "a" .. "f", shift= nats) drive the re-base branch of attn_f32_fwd, rebase_proof() shows from
                    emulated()'s walk that they do, F32_MUTANTS are that branch's named defects (_rebase_walk).
  split_ranges()    the ranges of a traversal cut into pieces as the kernels cut it (piece i takes the units
                    [i n / s, (i + 1) n / s) of 64 keys or 32 rows: attn_dq16_p4.h `tile_lo`, attn_dkv16_p4.h `lo`, `up`);
                    library_piece_count() reads the piece count s from the library's own plan (mfa_attention_kernel_workspace_size).

The bound.  Write u = 2^-8 (bf16) or 2^-11 (f16) for half a unit in the last place of the inputs' 16-bit type (round-to-nearest:
`v_cvt_pk_*_f32` in every stream generator), u32 = 2^-24, scale = 1 / sqrt(D), p_ij the model's softmax weights,
T_ij = scale sum_d |q_id k_jd|.  Every term is a worst case and errors add up linearly.

  Scores.  Exact mode (lowPrecisionIntermediates = 0): a score is D exact products summed in FP32 and scaled in FP32, p_ij carries
  the relative error rho_ij = ln 2 ((D + 3) u32 log2e T_ij + 3 u32 spread_i) + 4 u32 (decode_model's term).  Mixed mode: one operand
  of S = Q K^T is multiplied by log2e / sqrt(D) and rounded to the 16-bit type once (forward and backwardQuery: Q'; backwardKeyValue:
  K'; include/mfa.h), every product then moves by u: rho_ij += u T_ij.  This is the term that grows with a needle's score.
  Forward.  P enters P V in the 16-bit type: u A_O, A_O = sum_j p_ij |v_jd|.  Exact mode: l sums the unrounded P.  Mixed mode (FOLD
  streams): l sums the ROUNDED P: u |O| more.  p~ = p (1 + rho) moves the numerator by sum_j rho_ij p_ij |v_jd|
  and, through l, O by |O| sum_j rho_ij p_ij.  FP32 chains (per 16- or 32-deep matrix instruction, per deferred rescale, per wave,
  per piece, the combine, the normalisation): chain = C / 8 + pieces + 16 roundings on A_O + |O|.  The store: U_OUT |O|.
    E_O = u A_O + [mixed] u |O| + sum_j rho p |v| + |O| sum_j rho p + chain u32 (A_O + |O|)
  L = m + log2 l in log2 units, stored in FP32 (exact mode) or FP16 (mixed mode: half an ulp is 2^-11 |L|, the same in natural units):
    E_L = sum_j rho_ij p_ij + [mixed] u + chain u32 + 4 u32 (|m| + |ln l| + |L|) + (2^-11 [mixed] or 2^-23) |L|
  D = sum_d dO_id O_id from the FP32 O the forward launch stored, in FP32.  An error eps_j p_ij of the forward weights moves O_d by
  sum_j eps_j p_ij (v_jd - O_d) where l sums the same rounded P (mixed mode), by sum_j eps_j p_ij v_jd where it does not (exact mode),
  hence D by sum_j eps_j p_ij (dP_ij - D_i) or sum_j eps_j p_ij dP_ij, dP_ij = sum_d dO_id v_jd: a sum over KEYS, far below the sum
  over d of the O bounds.  D is stored in FP32 (exact mode) or in BF16 by truncation (mixed mode: up to 2^-7 |D_i|);
  backwardKeyValue reads the stored value back:
    E_D = sum_j p_ij (u (|dP_ij - D_i| [mixed] or |dP_ij|) + rho_ij |dP_ij - D_i|) + chain u32 (sum_j p_ij |dP_ij| + |D_i|)
          + ((D + 2) u32 + 2^-23) sum_d |dO_id O_id| + (2^-7 [mixed] or 2^-23) |D_i|
  Backward.  P_ij = exp2(s'_ij - L_i) with the STORED L: rho^b_ij = rho_ij + E_L_i (an FP16 L is one common relative error on a whole
  row of P).  P is rounded to 16 bits for dV (u); dP_ij = sum_d dO_id v_jd in FP32 (e_dP = (D + 3) u32 sum_d |dO v|);
  dS_ij = P (dP - D) is formed from the ROUNDED P in the role-split kernels (u, charged to every kernel) and rounded to 16 bits (u):
    e_dS_ij = p_ij ((rho^b_ij + u) |dP_ij - D_i| + e_dP_ij + E_D_i) + u |dS_ij|
    E_dV = sum_i p_ij (rho^b_ij + u) |dO_id| + chain_r u32 A_dV,          A_dV = sum_i p_ij |dO_id|
    E_dQ = scale sum_j e_dS_ij |k_jd| + chain u32 A_dQ,                   A_dQ = scale sum_j |dS_ij| |k_jd|
    E_dK = scale sum_i e_dS_ij |q_id| + chain_r u32 A_dK,                 A_dK = scale sum_i |dS_ij| |q_id|
  (the last products read K and Q as stored and the softmax scale multiplies the FP32 result: attn_dq16_p4.h `dQ = scale * dS' K`,
  attn_dkv16_p4.h `dK = scale * dS'^T Q`; the scaled, rounded K' of the mixed mode feeds S only.)  An error dL of a row's L moves dQ
  by dL A_dQ, dK and dV by dL times the row's share of A_dK and A_dV; an error dD of a row's D moves dQ by dD scale sum_j p_ij |k_jd|
  (Reference.PK) and dK by dD scale p_ij |q_id|.
  What the mixed bf16 bound does NOT resolve: a relative defect of 2^-5 on dQ.  E_dQ holds three half-ulps of its own (the rounded P,
  the rounded dS, l summed from the rounded P through E_L) and a fourth through E_D: the forward's rounded P moves D_i by up to
  u sum_j |dS_ij|, and the truncated store by 2^-7 |D_i| more (D_i is about 1.4 by needle_inputs' choice of dO; the smaller |D_i|, the
  smaller this share, but the u sum_j |dS_ij| part stays).  4 x 2^-8 of A_dQ >= |dQ| is 2^-5 exactly at margin 2, before the FP16 L
  and the D store are added: "dQ scaled by 1 - 2^-5" sits at 0.85 to 0.9 of the bound there, at 1.6 under bf16 exact, at 4 to 5 under
  f16 mixed (tests/test_train_sensitivity.py BOUND_OF).
  FP16 inputs: P (at most 2^8 against the running maximum, at most 1 in the backward pass) and dS lose their relative accuracy below
  2^-14: every visible (i, j) adds the absolute error f = 2^-25 to p_ij and f (|dP_ij - D_i| + sqrt(D)) to dS_ij (BF16 has FP32's
  exponent range: f = 0).  The sqrt(D): the role-split and wide dK / dV kernels round dS' = scale P (dP - D) -- the scale folded in
  BEFORE the 16-bit rounding, as the reference does (attn_dkv16_rs.h `(T)(p4[i] * (x[r] * a.scale - d4[i]))`, attn_dkv16_wide.h the
  same line) -- so FP16's floor f sits on scale dS.  Found by tests/test_train_parity_gpu.py: attn_dkv16w_f16_d320 and
  attn_dkv16rs_f16_d256 left dK elements of 1.5e-6 at 1.1 times a bound that had the floor on dS itself.
  bound_X = margin (E_X + U_OUT[out] |X|) + tiny,   tiny = 2^-24.

The launch forms of the torch binding (out=, dO_fmt= / dO_path=, heads_per_kv=; FORM_MUTANTS are their named defects).
  16-bit outputs (out = "bf16" | "f16": lowPrecisionOutputs).  backwardQuery reads the O the forward STORED (attn_dq16_p4.h `o32`,
  attn_dq16_p5.h, attn_bwd16.h): D~_i = sum_d dO_id st(O~_id), O~ the computed O (|O~ - O| <= E_O) and st its rounding to `out`.
  st(x) - x = -delta x with 0 <= delta < 2^-7 where the BF16 store truncates (one sign per element: every product moves towards 0), and
  |delta| <= 2^-8 (BF16) or 2^-11 (FP16) where it rounds to nearest (STORE_ROUNDING: the hand-placed persistent forwards do, every other
  store truncates).  With x_d = dO_id O_id, pos = sum of the positive x_d, neg = sum of the |negative x_d|:
    truncation  D~ - D = -sum_d delta_d x_d lies in [-2^-7 pos, +2^-7 neg]:  at most 2^-7 max(pos, neg);
    nearest     at most 2^-8 (pos + neg) <= 2^-7 max(pos, neg): the one term covers both roundings with decode_model.U_OUT;
    where O~_id and O_id differ in sign |O~_id| <= E_O_id, and elsewhere |O~_id| <= |O_id| + E_O_id:  U_OUT sum_d |dO_id| E_O_id more;
    FP16: no sign rule, U_OUT (pos + neg), and FP16's subnormal floor 2^-25 sum_d |dO_id| for elements of O below 2^-14.
    E_D += U_OUT[out] (max(pos, neg) [bf16] or pos + neg [f16]) + U_OUT[out] sum_d |dO_id| E_O_id + [f16] 2^-25 sum_d |dO_id|
  in place of the 2^-23 sum_d |dO_id O_id| of an FP32 O.  It reaches e_dS, E_dQ and E_dK through E_D as every other term of it does.
  On the needle inputs (bf16 mixed, (255, 257, 64) causal and (300, 333, 128)) E_D grows 2.1 to 2.6 fold, a truncating store moves D
  by at most 0.46 to 0.70 of the new term, "D wrong by 2^-4" falls from 3.2 - 3.7 to 1.3 - 1.7 times the bound and stays flagged.
  The FP16 + BF16-dO mix (fmt = "f16", dO_fmt = "bf16": the reference's memoryPrecisions).  Every backwardQuery kernel, and the
  backwardKeyValue kernels of MIX_PATH's "convert_dO" rows, convert dO to FP16 element by element through `(T)(float)`
  (attn_bwd16.h convert_chunk).  BF16's 8 significant bits fit FP16's 11: the conversion is exact down to 2^-14; below, the result is
  an FP16 subnormal, a multiple of 2^-24: an absolute error of at most 2^-25 per element (above 65504 it is infinite: out of the
  contract).  Charged wherever dO enters a product:
    convert_dO     e_dP_ij += 2^-25 sum_d |v_jd|,   E_D_i += 2^-25 sum_d |O_id|,   E_dV_jd += 2^-25 sum_i p_ij
  "bf16_products" (the mix streams of attn_dkv16_p4 / _p5: attn_dkv16_p4.h `stream_mix`): backwardKeyValue reads dO as stored and runs
  its two products in BF16 -- V converted to BF16 once (half an ulp: 2^-8 relative on every product of dP), P packed to BF16 for
  dV (u = 2^-8 in E_dV in place of 2^-11); S, dS and dK keep FP16's u.  D and dQ come from backwardQuery, which converts:
    bf16_products  e_dP_ij (dK side) += 2^-8 sum_d |dO_id v_jd|,   E_dV: u -> 2^-8,   E_D and E_dQ as under convert_dO
  Two variants, never their maximum: the union would loosen dV eightfold on the families that convert.
  Grouped K / V heads (heads_per_kv = G; K, V [B, H / G, C, D], query head h reads head h // G).  backwardKeyValue leaves every query
  head's FP32 dK / dV in a slab; attn_kv_group_sum adds the G slabs of a group in the order g = 0 .. G - 1 in FP32 and stores once:
    E_dV (group) = sum_g E_dV (member g) + G u32 sum_g A_dV (member g)        (dK alike); the store term U_OUT |dV| once, on the sum.

MARGIN is the smallest power of two, at most 4, with at least 2 x headroom over the worst err / bound at margin 1 of emulated() on
every case of tests/test_train_sensitivity.py and of the kernels on every case of tests/test_train_parity_gpu.py and of the files
that run their cases through it (DESIGN.md 4.18 records both maxima).

FP32 operands (fmt = "f32": csrc/attn_f32.h; `mixed` is meaningless and refused; the outputs are always FP32).  u = 0: no operand, P
or dS is rounded to 16 bits, and FP16's floor f is 0.  What remains is the rho term and the FP32 chains, re-derived from the kernels
as read.  s2 = log2e s are the scores in log2 units, T2_ij = log2e T_ij, m the kernel's REFERENCE maximum in log2 units.
  Scores (attn_f32_fwd).  Q is multiplied by scale2 = fl(log2e / sqrt(D)) once (pin_fragments: one rounding per element, u32 T2 on a
  score).  A score is an FP32 chain on v_mfma_f32_32x32x2_f32: one instruction contracts two head dimensions (d = 8 T + i from the
  hi = 0 lanes, 8 T + 4 + i from the hi = 1 lanes; two roundings at the most), D / 2 instructions, D roundings.  The accumulator
  STARTS at -m (mfma_bias: ones . (-m), exact), so every partial sum is bounded by |m| + T2 and each rounding by u32 (|m| + T2): the
  cancellation term in |m|.  A firing tile subtracts delta (`s[r] -= delta`: one rounding of the same size) and adds it to m
  (`m += delta`: u32 |m|, which every later tile starts from).  In all (D + 3) u32 (T2_ij + M_ij) in log2 units, M_ij = the larger of
  |m| before and after the tile of key j.  m follows the kernel's rule (32-key tiles; tile 0 sets m to its maximum; a later tile
  re-bases iff its maximum exceeds m by more than 8), walked in float64 (_rebase_walk).  A tile whose maximum lies within 2^-8 of the
  threshold may go either way in FP32; m then differs by about 8: such a row carries M + 8 on every key.
  fast_exp2 is __builtin_amdgcn_exp2f, one v_exp_f32: 1 ulp = 2 u32 (the CDNA ISA's stated accuracy of the transcendental unit);
  the sum `psum += s[r]` adds 1, the product with V or dP one more:
    rho_ij = ln 2 u32 ((D + 3) (T2_ij + M_ij) + 2 (max_j M_ij + 8)) + 4 u32
  (the last bracket: the general kernels of attn_generic.h start a score at 0, scale it and subtract the RUNNING maximum in one fma,
  `s[r] * a.scale2 - m`, and re-base at every growth: two roundings on |m_run|, which lies between tile 0's maximum and the row's,
  hence within 8 of an M of the row.)
  Forward chains.  O^T += V^T P^T on the same instruction: two keys per instruction, C roundings on A_O + |O|.  l: 16 additions per
  half-wave and tile, one `l += psum` per tile, half_add once (C / 32 + 17); one re-base per firing tile multiplies l and O by
  corr = fast_exp2(-delta) (the same factor on both: its own error cancels in O; one rounding each: 2 per tile at the most);
  half_max is exact; 1 / l_tot (v_rcp_f32, 1 ulp = 2) and the product with it (1).  chain = C + 3 ceil(C / 32) + pieces + 24.
    E_O = sum_j rho p |v| + |O| sum_j rho p + chain u32 (A_O + |O|)
  L = m + log2f(l_tot): log2f is one v_log_f32 under the library's fast-math build or OCML's log2f, both within 1 ulp = 2 u32 |log2 l|;
  the kernel's m and l are the reference's, not the row maximum's: |m_ref| <= |m| + 8 and |log2 l_ref| <= |log2 l| + 8 in log2 units:
    E_L = sum_j rho p + chain u32 + 4 u32 (|m| + |ln l| + |L| + 16 ln 2) + 2^-23 |L|
  D = scale sum_d dO O (attn_f32_dq: D / 2 fma per half-wave, half_add, the product with scale, the FP32 store): the terms of the
  exact mode above, with this chain.
  Backward.  attn_f32_dq: S' - L and dP - D / scale leave the matrix pipe from accumulators started at -L and -sum(dO o O): D
  roundings each on |L2| + T2 and on |D_i| + sum_d |dO v|; P = fast_exp2 (2 u32), dS = P (dP - D) (1):
    rho^b_ij = ln 2 (D + 3) u32 (T2_ij + |L2_i|) + 4 u32 + E_L_i,      e_dP_ij = (D + 3) u32 (sum_d |dO_id v_jd| + |D_i|)
  dQ^T += K^T dS^T over 32-KEY tiles, two keys per instruction: chain (C roundings) on A_dQ.  attn_f32_dkv: K is multiplied by
  -scale2 and V by -scale once (one rounding per element, inside the D + 3), the accumulators start at the stored L and D of the
  tile's 32 ROWS; dV^T += dO^T P and dK^T += Q^T dS over 32-row tiles, two rows per instruction: chain_r = R + 3 ceil(R / 32) +
  pieces + 24 roundings on A_dV and A_dK.  The group sum is as above.
  The general FP32 kernels (attn_generic.h: the 32 and 256 head blocks, transposed operands, unaligned leading dimensions, the 384
  row and the paged route beyond it) run the same arithmetic on the same instruction with the same tiles of 32 keys or rows
  (attn_f32.h's header says so; `BT = 32` there, `BC = 32` and 32-row steps here), and attn_paged.h (D > 384: `BR = 32, BC = 32`)
  adds its scores and outputs up in plain fma chains, one rounding per product, over 32-key and 32-row tiles: the chain counts one
  rounding per product and three per 32-wide tile, and so holds for every FP32 launch form.
  emulated(fmt="f32") walks the forward as the kernel does: Q' once, the chain of a score in the kernel's order of d from -m, 32-key
  tiles, the re-base rule (threshold 8; tile 0 always sets m; corr = exp2(-delta) on O and l; the firing tile's scores shifted;
  later tiles start from the new m), l per half-wave, the P V sum in the kernel's order of keys.  trace= receives, per grid entry,
  the per-tile maxima relative to m and which rows fired in which tile (rebase_proof reads it).
MARGIN_F32 is measured the same way (DESIGN.md 4.25 records the maxima of emulated() and of the kernels).
"""
import math
from typing import NamedTuple

import numpy as np

from decode_model import LN2, LOG2E, TINY, U32, U_OUT, U_P, f64, fmt_of, round_to, store  # noqa: F401 -- one set of rounding helpers

TILE, STEP, WAVE_ROWS, BLOCK_ROWS = 64, 32, 64, 256   # keys per tile, keys / rows per step, rows per wave, rows per row block
RESCALE_THRESHOLD = 8.0                               # log2 units: the deferred rescale of the forward streams (include/mfa.h)
MARGIN = 2
F16_FLOOR = 2.0 ** -25                                # half the spacing of FP16's subnormals: P and dS below 2^-14 in that type
OUTPUTS = ("O", "L", "D", "dV", "dK", "dQ")
U_OF = dict(U_P, f32=0.0)                             # u of the bound: half an ulp of the operands' 16-bit type; FP32 operands round nothing to 16 bits
MARGIN_F32 = 1                                        # fmt = "f32": measured like MARGIN
F32_TILE, F32_THRESHOLD = 32, 8.0                     # attn_f32.h BT, RESCALE_ABOVE (log2 units)
SPIKES = ("a", "b", "c", "d", "e", "f")               # needle_inputs(spike=): the family of late dominant keys (spike_keys)
SHIFT, SHIFT_DEEP = 60.0, 100.0                       # needle_inputs(shift=), nats: inside and beyond FP32's exponent range (87 nats)
OLD_TOL_FP32 = 2e-5                                   # tests/harness.py TOL_FP32
OLD_TOL = dict(O=5e-2, L=7e-3, D=1e-1, dV=5e-2, dK=5e-2, dQ=5e-2)   # tests/harness.py TOL_MIXED


class Reference(NamedTuple):
    O: np.ndarray; L: np.ndarray; D: np.ndarray; dV: np.ndarray; dK: np.ndarray; dQ: np.ndarray   # noqa: E702
    A: dict          # the magnitude sums: O, dV, dQ, dK
    E: dict          # per output, every term of the bound except the store's, at margin 1
    PK: np.ndarray   # [B, H, R, D] scale sum_j p_ij |k_jd|: what a unit error of the row's D moves in dQ (an error of L moves A["dQ"])
    row_live: np.ndarray   # [B, R] rows below the entry's row length
    key_live: np.ndarray   # [B, C]
    dead: np.ndarray = None    # [B, H, R] live rows that see no key (a block mask): O = dQ = D = 0 exactly, L hugely negative


# ---------------------------------------------------------------------------------------------------------------------- mutants
# name -> (what the defect is, where it changes nothing).  `case` has R, C, H, B, causal, pieces (bool), spike (bool), all_whole_tiles,
# row_lengths_differ, row_padding, key_padding (case_flags) and, a masked case, block_mask, rl, cl: under a mask a defect that drops
# keys or rows changes nothing where no live row sees them (_seen: from the mask, the lengths and the causal flag)
_no_split = lambda c: not c["pieces"]          # noqa: E731


def _seen(c, rows=None, keys=None):
    """under a block mask: whether, in some grid entry, a live row of rows(row length) sees a key of keys(key length) (slices; None:
    all).  Without a mask: True (the predicates below are then what they were)"""
    if c.get("block_mask") is None:
        return True
    rl, cl = _lengths(c.get("rl"), c["B"], c["R"]), _lengths(c.get("cl"), c["B"], c["C"])
    for b in range(c["B"]):
        for h in range(c["H"]):
            vis = mask_views(c["block_mask"], b, h, c["R"], c["C"], int(rl[b]), int(cl[b]), c["causal"])[0][:int(rl[b])]
            if vis[rows(int(rl[b])) if rows else slice(None), keys(int(cl[b])) if keys else slice(None)].any():
                return True
    return False


_last_block = lambda n: slice((n - 1) // BLOCK_ROWS * BLOCK_ROWS, n)     # noqa: E731
_last_tile = lambda n: slice((n - 1) // TILE * TILE, n)                  # noqa: E731
MUTANTS = {
    # forward
    "o_zero": ("O = 0 everywhere", lambda c: False),
    "key0_dropped": ("key 0 never seen", lambda c: not _seen(c, None, lambda n: slice(0, 1))),
    "last_key_dropped": ("the last key never seen", lambda c: not _seen(c, None, lambda n: slice(n - 1, n))),
    "partial_last_tile_dropped": ("the partial last 64-key tile is not run",
                                  lambda c: c["all_whole_tiles"] or not _seen(c, None, lambda n: slice(n // TILE * TILE, n if n % TILE else 0))),
    "tile_skipped_in_one_row_block": ("keys 64..127 skipped in the LAST row block only",
                                      lambda c: c["C"] <= TILE or not _seen(c, _last_block, lambda n: slice(TILE, 2 * TILE))),
    "causal_plus_1": ("forward: causal frontier one key too far", lambda c: not c["causal"] or c["R"] == 1),
    "causal_minus_1": ("forward: causal frontier one key short", lambda c: not c["causal"]),
    "wave_groups_exchanged": ("rows 0..63 and 64..127 of row block 0 exchanged in O and L", lambda c: c["R"] <= WAVE_ROWS),
    "row_block_next_head_kv": ("row block 0 served from the next head's K / V", lambda c: c["H"] == 1),
    "v_rows_exchanged": ("two V rows of one 16-key group exchanged",
                         lambda c: c["C"] < 2 or not _seen(c, None, lambda n: slice(30, 32) if n >= 32 else slice(0, 2))),
    "v_dblocks_exchanged": ("the first two 32-wide d blocks of V exchanged", lambda c: c.get("D", 64) < 64),
    "rescale_o_not_l": ("the deferred rescale (threshold 8) applied to O but not to l", lambda c: not c["spike"]),
    "l_without_key0": ("l without key 0: wrong in L only", lambda c: not _seen(c, None, lambda n: slice(0, 1))),
    "row_length_next_batch": ("the row length of batch b + 1 used for batch b", lambda c: not c["row_lengths_differ"]),
    "piece_loses_last_tile": ("forward: every piece stops one 64-key tile early", _no_split),
    "piece_overlaps": ("forward: every piece starts one tile early, inside its neighbour", _no_split),
    "combine_ignores_maxima": ("the forward combine adds the pieces without exp2(m_s - m*)", _no_split),
    # backward
    "dq_last_tile_dropped": ("dQ without its last key tile", lambda c: c["C"] == 1 or not _seen(c, None, _last_tile)),
    "dq_tile_skipped_in_one_row_block": ("dQ without keys 64..127 in the LAST row block only",
                                         lambda c: c["C"] <= TILE or not _seen(c, _last_block, lambda n: slice(TILE, 2 * TILE))),
    "dkv_last_step_dropped": ("dK / dV without the last 32-row step", lambda c: not _seen(c, lambda n: slice((n - 1) // STEP * STEP, n))),
    "dkv_row_block_dropped": ("dK / dV without the last 256-row block", lambda c: not _seen(c, _last_block)),
    "d_zero": ("D term = 0", lambda c: False),
    "d_wrong": ("D wrong by 2^-4", lambda c: False),
    "d_neighbour_row": ("D of the neighbouring row", lambda c: c["R"] == 1),
    "d_next_head": ("D of the next head", lambda c: c["H"] == 1),
    "l_neighbour_row": ("L of the neighbouring row in the backward pass", lambda c: c["R"] == 1),
    "ds_scale_missing": ("the softmax scale left out of dS", lambda c: c["C"] == 1),
    "ds_scale_twice": ("the softmax scale applied twice to dS", lambda c: c["C"] == 1),
    "dq_scaled": ("dQ scaled by 1 - 2^-5", lambda c: c["C"] == 1),
    "dk_dv_exchanged": ("dK and dV exchanged", lambda c: False),
    "bwd_causal_plus_1": ("backward only: causal frontier one key too far", lambda c: not c["causal"] or c["R"] == 1),
    "bwd_causal_minus_1": ("backward only: causal frontier one key short", lambda c: not c["causal"]),
    "dq_reads_padding_keys": ("the key AT the key length contributes to dQ", lambda c: not c["key_padding"]),
    "dkv_reads_padding_rows": ("the row AT the row length contributes to dK / dV", lambda c: not c["row_padding"]),
    "bwd_combine_drops_slab": ("attn_bwd_combine drops the second piece's slab", _no_split),
    "bwd_combine_adds_slab_twice": ("attn_bwd_combine adds the second piece's slab twice", _no_split),
}
# the launch forms of the torch binding (16-bit outputs, the FP16 + BF16-dO mix, grouped K / V heads).  `case` also has out ("f32" |
# "bf16" | "f16"), mix (dO_fmt differs from fmt), small_dO (a block of dO rows scaled by 2^-12) and G (heads_per_kv)
_out32 = lambda c: c.get("out", "f32") == "f32"      # noqa: E731
_no_mix = lambda c: not c.get("mix")                 # noqa: E731
_no_group = lambda c: c.get("G", 1) == 1             # noqa: E731
FORM_MUTANTS = {
    "d_from_unstored_o_next_head": ("16-bit outputs: D formed from the O of head h + 1", lambda c: _out32(c) or c["H"] == 1),
    "o16_row_pairs_exchanged": ("16-bit outputs: rows 0 and 1 exchanged in the O store only (D from the right rows)", lambda c: _out32(c) or c["R"] < 2),
    "out16_last_chunk_dropped": ("16-bit outputs: the last 8 elements of row 0 of O, dQ and dK keep the sentinel", _out32),
    "out16_piece_rounded_before_combine": ("16-bit outputs under a split plan: every piece's partial rounded to 16 bits before the sum",
                                           lambda c: _out32(c) or not c["pieces"]),
    "dO_bits_as_input_type": ("the mix: dO's BF16 bits read as FP16", _no_mix),
    "dO_small_flushed": ("the mix: dO elements below 2^-14 read as zero (the code converts them to FP16 subnormals)",
                         lambda c: _no_mix(c) or not c.get("small_dO")),
    "dO_converted_in_dv_only": ("the mix: backwardKeyValue's dP reads dO's unconverted bits", _no_mix),
    "group_slab_dropped": ("attn_kv_group_sum without the slab of the group's second member", _no_group),
    "group_slab_twice": ("attn_kv_group_sum adds the slab of the group's second member twice", _no_group),
    "group_sum_head_is_query_head": ("query head h's slab added to K / V head h instead of h // G", _no_group),
    "group_store_rounds_each_slab": ("16-bit outputs: every slab of a group rounded to 16 bits before the sum", lambda c: _no_group(c) or _out32(c)),
}
MUTANTS.update(FORM_MUTANTS)
# the re-base branch of attn_f32_fwd (attn_f32.h `if (__builtin_amdgcn_ballot_w64(grow) != 0)`), walked by _rebase_walk.  `case` also
# has D, spike (False | True | "a" .. "f": SPIKES) and shift (None or nats).  A spike case leaves key 0 out of its unspiked rows'
# needles, so rows of every kind fire behind tile 0; FP32's exponent range is +-126 log2 units = +-87 nats: a first tile that keeps
# m = 0 computes the same softmax until a shift takes exp2 out of that range (SHIFT_DEEP)
F32_MUTANTS = {
    "rebase_l_not_o": ("FP32 forward: a re-base after tile 0 corrects l but not O", lambda c: not c["spike"]),
    "rebase_scores_not_shifted": ("FP32 forward: the firing tile (after tile 0) keeps s instead of s - delta", lambda c: not c["spike"]),
    "rebase_bias_stale": ("FP32 forward: tiles after a re-base still start from the old -m", lambda c: not c["spike"]),
    "first_tile_keeps_m0": ("FP32 forward: tile 0 re-bases only if mx > 8", lambda c: (c.get("shift") or 0.0) < SHIFT_DEEP),
    "rebase_only_first_db": ("FP32 forward: the correction reaches the first accumulator block of O only (d = NDB i + 0)", lambda c: not c["spike"]),
    # (D = 4: the keys' codes repeat every four keys, both halves of a tile hold every code and so the same maximum)
    "rebase_other_half": ("FP32 forward: the hi = 1 lanes re-base by their own half's maximum (half_max lost)", lambda c: c["D"] == 4),
}
MUTANTS.update(F32_MUTANTS)
# block-mask mutants: each misreads the mask (mask_views); "changes nothing" where the misread visibility of every live row equals the
# true one, which follows from the case's mask, its words, whether it is shared, causal and the lengths -- never from a result
MASK_MUTANTS = {
    "mask_ignored": "all three kernels run dense",
    "mask_ignored_dq": "dQ runs dense after a masked forward",
    "mask_ignored_dkv": "dK / dV run dense after a masked forward",
    "mask_word0_for_every_block": "column block cb reads bit cb & 31 of word 0",
    "mask_row_stride_one_word": "row block rb reads at rb x 1 words instead of rb x words",
    "mask_bit_plus_1": "column block cb reads the bit of cb + 1",
    "mask_next_row_block": "row block rb reads the words of rb + 1 (the last one reads its own)",
    "mask_per_tile": "the forward takes bit t of the 64-key tile index t instead of t >> 1",
    "mask_head0_for_all": "the mask's head stride taken as 0",
    "mask_batch0_for_all": "the mask's batch stride taken as 0",
    "mask_head_is_kv_head": "under a per-head mask, head h reads mask h // 2",
    "run_starts_one_key_late": "the first key of every run of active blocks dropped",
    "run_ends_one_key_early": "the last key of every run of active blocks dropped",
    "run_reads_one_key_past": "the first key of the inactive block behind a run read",
    "mask_drops_causal_in_later_runs": "the causal rule applied in the first run of a row block only",
    "mask_drops_key_length": "the key-length clamp lost in the last active block",
    "dkv_last_row_block_unlisted": "dK / dV without the last ACTIVE row block of every column block",
    "dead_row_uniform": "a dead row gets the mean of V and L = 0 instead of O = 0 and a hugely negative L",
}
for _name, _what in MASK_MUTANTS.items():
    MUTANTS[_name] = (_what, lambda c, _n=_name: not mask_mutant_changes(c, _n))


def case_flags(R, C, row_lengths=None, key_lengths=None):
    """the fields of a case the predicates read that follow from its lengths"""
    rl, cl = list(row_lengths or [R]), list(key_lengths or [C])
    return dict(all_whole_tiles=all(n % TILE == 0 for n in cl), row_lengths_differ=len(set(rl)) > 1, row_padding=any(n < R for n in rl),
                key_padding=any(n < C for n in cl))


def split_ranges(n, count, unit):
    """[(begin, end)] of a traversal of n keys (unit 64: dQ, forward) or rows (unit 32: dK / dV) cut into `count` pieces"""
    units = -(-int(n) // unit)
    return [(min(n, unit * (i * units // count)), min(n, unit * ((i + 1) * units // count))) for i in range(count)]


KERNEL_TYPES = ("fwd", "dq", "dkv")          # in the order of AttentionKernelType: forward, backwardQuery, backwardKeyValue


def piece_count(kernel, kernel_type, R, C, D, heads, batches):
    """pieces of the library's own plan for a launch of `kernel` given a workspace (1: not split): the workspace it asks for
    (mfa_attention_kernel_workspace_size) over one piece's slabs (mfa_kernel.hip split_workspace_bytes)"""
    need = kernel.workspaceSize(row=R, column=C, heads=heads, batches=batches)
    per = heads * batches * {"fwd": R * (D + 2) * 4, "dq": R * D * 4, "dkv": 2 * C * D * 4}[kernel_type]
    assert need % per == 0, (kernel_type, need, per)
    return max(1, need // per)


def pieces_of(counts, R, C):
    """{"fwd": key ranges, "dq": key ranges, "dkv": row ranges} for the kernel types that are split, or None"""
    res = {t: split_ranges(R if t == "dkv" else C, n, STEP if t == "dkv" else TILE) for t, n in counts.items() if n > 1}
    return res or None


def library_piece_count(kernel_type, R, C, D, heads, batches, fmt="bf16", mixed=True):
    """piece_count() of the kernel the default tables select for this shape, type and mode"""
    from metal_flash_attention_amd import AttentionDescriptor, AttentionKernel, AttentionKernelType, GEMMOperandPrecision
    d = AttentionDescriptor()
    d.lowPrecisionInputs, d.lowPrecisionIntermediates = True, mixed
    d.matrixDimensions = (R, C, D)
    d.transposeState = (False,) * 4
    d.lowPrecisionInputType = GEMMOperandPrecision.BF16 if fmt == "bf16" else GEMMOperandPrecision.FP16
    t = list(AttentionKernelType)[KERNEL_TYPES.index(kernel_type)]
    return piece_count(AttentionKernel(d.kernelDescriptor(t)), kernel_type, R, C, D, heads, batches)


def library_pieces(R, C, D, heads, batches, fmt="bf16", mixed=True):
    """{"fwd": key ranges, "dq": key ranges, "dkv": row ranges} of the library's plan, or None where no kernel type is split"""
    return pieces_of({t: library_piece_count(t, R, C, D, heads, batches, fmt, mixed) for t in KERNEL_TYPES}, R, C)


def _lengths(lens, B, full):
    return np.full(B, full, dtype=np.int64) if lens is None else np.minimum(np.asarray(lens, dtype=np.int64), full)


def _visible(R, C, rlen, clen, causal, shift=0):
    rows, cols = np.arange(R)[:, None], np.arange(C)[None, :]
    vis = np.broadcast_to(cols < clen, (R, C)).copy()
    if causal:
        vis &= cols <= rows + max(clen - rlen, 0) + shift
    return vis


MASK_COLUMNS = 128                                    # keys per mask block (MFA_MASK_BLOCK_COLUMNS; BLOCK_ROWS rows: MFA_MASK_BLOCK_ROWS)


def mask_bits(block_mask, b, h):
    """the bool [row blocks, column blocks] of grid entry (b, h): block_mask is that array, shared, or [B, H, row blocks, column blocks]"""
    m = np.asarray(block_mask, dtype=bool)
    return m if m.ndim == 2 else m[b, h]


def pack_mask(bits):
    """bool [..., row blocks, column blocks] -> uint32 [..., row blocks, words]: bit b of word w = column block 32 w + b (mfa.h)"""
    bits = np.asarray(bits, dtype=bool)
    ncb = bits.shape[-1]
    words = -(-ncb // 32)
    padded = np.zeros(bits.shape[:-1] + (words * 32,), dtype=np.uint64)
    padded[..., :ncb] = bits
    return (padded.reshape(bits.shape[:-1] + (words, 32)) << np.arange(32, dtype=np.uint64)).sum(axis=-1).astype(np.uint32)


def mask_dense(bits, R, C, columns=MASK_COLUMNS):
    return np.repeat(np.repeat(np.asarray(bits, dtype=bool), BLOCK_ROWS, axis=0)[:R], columns, axis=1)[:, :C]


def mask_runs(active):
    """[(first, last column block)] of the runs of consecutive active blocks of one row block"""
    res, start = [], None
    for cb, on in enumerate(list(active) + [False]):
        if on and start is None:
            start = cb
        elif not on and start is not None:
            res.append((start, cb - 1))
            start = None
    return res


def _read_flat(bits, word, bit, R, C, columns=MASK_COLUMNS):
    """the dense visibility of a kernel that reads bit `bit` of word `word` ([row blocks, n] index arrays) of the packed mask"""
    flat = pack_mask(bits).reshape(-1)
    ok = word < flat.size
    return mask_dense(((flat[np.minimum(word, flat.size - 1)] >> bit.astype(np.uint32)) & 1).astype(bool) & ok, R, C, columns)


def mask_views(block_mask, b, h, R, C, rlen, clen, causal, mutant=None):
    """-> (the true visibility [R, C], what the forward, dQ and dK / dV kernels of `mutant` see)"""
    base = _visible(R, C, rlen, clen, causal)
    if block_mask is None:
        return base, base, base, base
    bits = mask_bits(block_mask, b, h)
    true = base & mask_dense(bits, R, C)
    if mutant not in MASK_MUTANTS or mutant == "dead_row_uniform":
        return true, true, true, true
    m = np.asarray(block_mask, dtype=bool)
    nrb, ncb = bits.shape
    words = -(-ncb // 32)
    rb, cb = np.meshgrid(np.arange(nrb), np.arange(ncb), indexing="ij")
    blocks = lambda i: slice(i * BLOCK_ROWS, min((i + 1) * BLOCK_ROWS, R))   # noqa: E731
    if mutant == "mask_ignored":
        return true, base, base, base
    if mutant == "mask_ignored_dq":
        return true, true, base, true
    if mutant == "mask_ignored_dkv":
        return true, true, true, base
    if mutant == "mask_per_tile":
        t = np.arange(-(-C // TILE))[None, :] + 0 * np.arange(nrb)[:, None]
        return true, base & _read_flat(bits, np.arange(nrb)[:, None] * words + (t >> 5), t & 31, R, C, TILE), true, true
    if mutant == "dkv_last_row_block_unlisted":
        wrong = true.copy()
        for c in range(ncb):
            listed = [i for i in range(nrb) if bits[i, c] and i * BLOCK_ROWS < rlen]
            if listed:
                wrong[blocks(listed[-1]), c * MASK_COLUMNS:(c + 1) * MASK_COLUMNS] = False
        return true, true, true, wrong
    if mutant in ("mask_head0_for_all", "mask_batch0_for_all", "mask_head_is_kv_head"):
        other = bits if m.ndim == 2 else m[b, 0] if mutant == "mask_head0_for_all" else m[0, h] if mutant == "mask_batch0_for_all" else m[b, h // 2]
        wrong = base & mask_dense(other, R, C)
    elif mutant == "mask_word0_for_every_block":
        wrong = base & _read_flat(bits, rb * words, cb & 31, R, C)
    elif mutant == "mask_row_stride_one_word":
        wrong = base & _read_flat(bits, rb + (cb >> 5), cb & 31, R, C)
    elif mutant == "mask_bit_plus_1":
        wrong = base & _read_flat(bits, rb * words + ((cb + 1) >> 5), (cb + 1) & 31, R, C)
    elif mutant == "mask_next_row_block":
        wrong = base & _read_flat(bits, np.minimum(rb + 1, nrb - 1) * words + (cb >> 5), cb & 31, R, C)
    else:
        wrong = true.copy()
        rows, cols = np.arange(R)[:, None], np.arange(C)[None, :]
        for i in range(nrb):
            runs = mask_runs(bits[i])
            for n, (s, e) in enumerate(runs):
                first, behind = s * MASK_COLUMNS, (e + 1) * MASK_COLUMNS
                if mutant == "run_starts_one_key_late" and first < C:
                    wrong[blocks(i), first] = False
                elif mutant == "run_ends_one_key_early" and min(behind, clen) - 1 >= first:
                    wrong[blocks(i), min(behind, clen) - 1] = False
                elif mutant == "run_reads_one_key_past" and behind < C:
                    wrong[blocks(i), behind] = base[blocks(i), behind]
                elif mutant == "mask_drops_causal_in_later_runs" and n > 0:
                    wrong[blocks(i), first:behind] = np.broadcast_to(cols < clen, (R, C))[blocks(i), first:behind]
                elif mutant == "mask_drops_key_length" and n == len(runs) - 1:
                    keep = (cols <= rows + max(clen - rlen, 0)) if causal else np.ones((R, C), dtype=bool)
                    wrong[blocks(i), e * MASK_COLUMNS:behind] = keep[blocks(i), e * MASK_COLUMNS:min(behind, C)]
    return true, wrong, wrong, wrong


def mask_mutant_changes(case, mutant):
    """whether a mask mutant sees, on some live row of some grid entry of the case, other keys than the model (or, dead_row_uniform,
    whether the case has a dead row): from the case's mask, lengths and causal flag alone"""
    bm = case.get("block_mask")
    if bm is None:
        return False
    per = np.asarray(bm).ndim == 4
    words = -(-np.asarray(bm).shape[-1] // 32)
    if (mutant in ("mask_word0_for_every_block", "mask_row_stride_one_word") and words == 1) or \
            (mutant in ("mask_head0_for_all", "mask_batch0_for_all", "mask_head_is_kv_head") and not per) or \
            (mutant == "mask_drops_causal_in_later_runs" and not case["causal"]) or (mutant == "mask_drops_key_length" and not case["key_padding"]):
        return False
    R, C, B, H = case["R"], case["C"], case["B"], case["H"]
    rl, cl = _lengths(case.get("rl"), B, R), _lengths(case.get("cl"), B, C)
    for b in range(B):
        for h in range(H):
            views = mask_views(bm, b, h, R, C, int(rl[b]), int(cl[b]), case["causal"], mutant)
            live = views[0][:int(rl[b])]
            if mutant == "dead_row_uniform":
                if not live.any(axis=1).all():
                    return True
            elif any(not np.array_equal(live, x[:int(rl[b])]) for x in views[1:]):
                return True
    return False


def needle_mask(R, C, seed, *, density=0.4, causal=False, empty_last=False, need_blocks=()):
    """a random bool [row blocks, column blocks] with what the needle plan asks of a mask: every row block alive (empty_last: all but
    the last), every pair of adjacent live row blocks with a column block active in the one and not in the other in BOTH directions,
    (three column blocks or more) a run of two blocks, a run that starts behind block 0 and a run that ends before the last block;
    causal: every live row block has an active block at or left of its first row's frontier, one row block an active block wholly
    right of its last row's frontier; every block of need_blocks active in some row block; more than 32 column blocks: bits b and
    b + 32 opposite"""
    rng = np.random.default_rng(seed)
    nrb, ncb = -(-R // BLOCK_ROWS), -(-C // MASK_COLUMNS)
    off = max(C - R, 0)
    for _try in range(20000):
        bits = rng.random((nrb, ncb)) < density
        if ncb > 32:
            bits[:, 32:] = ~bits[:, :ncb - 32]
        live = nrb - 1 if empty_last else nrb
        bits[live:] = False
        runs = [r for i in range(live) for r in mask_runs(bits[i])]
        ok = all(bits[i].any() for i in range(live)) and all(bits[:live, c].any() for c in need_blocks)
        if ncb >= 2:
            ok = ok and all((bits[i] & ~bits[i + 1]).any() and (~bits[i] & bits[i + 1]).any() for i in range(live - 1))
        if ncb >= 3:
            ok = ok and any(e > s for s, e in runs) and any(s > 0 for s, e in runs) and any(e < ncb - 1 for s, e in runs)
        if causal:
            ok = ok and all(bits[i, :(i * BLOCK_ROWS + off) // MASK_COLUMNS + 1].any() for i in range(live))
            ok = ok and any(bits[i, (min((i + 1) * BLOCK_ROWS, R) - 1 + off) // MASK_COLUMNS + 1:].any() for i in range(live))
        if ok:
            return bits
    raise AssertionError("no mask of this shape meets the needle plan's conditions")


def _softmax(S, vis, mult=None):
    Sm = np.where(vis, S, -np.inf)
    m = Sm.max(axis=1, keepdims=True)
    m0 = np.where(np.isfinite(m), m, 0.0)
    pw = np.exp(Sm - m0)
    if mult is not None:
        pw = pw * mult
    l = pw.sum(axis=1, keepdims=True)
    l0 = np.where(l > 0, l, 1.0)
    return pw / l0, m0[:, 0], l0[:, 0]


def crow(r, hi):
    """the key (forward, dQ) or row (dK / dV) of a 32-wide tile that register r of half-wave hi holds (attn_common.h crow)"""
    return (r & 3) + 8 * (r >> 2) + 4 * hi


def _fp32_range(p):
    """float64 weights as fast_exp2 returns them: infinite from 2^128 on, zero below 2^-126 (v_exp_f32 flushes subnormal results:
    LLVM's own exp2 lowering for AMDGPU scales its argument for that reason; __builtin_amdgcn_exp2f is the bare instruction)"""
    with np.errstate(all="ignore"):
        return np.where(p >= 2.0 ** 128, np.inf, np.where(p < 2.0 ** -126, 0.0, p))


def _rebase_walk(S2, V, mutant=None):
    """attn_f32_fwd's online softmax around a reference maximum, in float64: S2 [R, C] scores in log2 units (-inf: not seen), V [C, D]
    -> O, L in log2 units, trace {before, after: m a tile's scores start from / m behind the tile, mx: the tile's maximum relative to
    `before` ([R, tiles]), fired: rows that took the re-base branch in a tile after tile 0}.  Per half-wave hi: its reference m, its
    l, the columns d = NDB crow(r, hi) + db of O; the scores of a tile start from the hi = 0 lanes' bias.  Unmutated this is softmax."""
    R, C = S2.shape
    Dh = V.shape[1]
    ndb = 2 if Dh <= 64 else 4
    tiles = -(-C // F32_TILE)
    S2 = np.concatenate([S2, np.full((R, tiles * F32_TILE - C), -np.inf)], axis=1)
    V = np.concatenate([V, np.zeros((tiles * F32_TILE - C, Dh))])
    half = np.arange(F32_TILE) % 8 >= 4                 # keys of a tile the hi = 1 lanes hold (crow)
    cols = (np.arange(Dh) // ndb) % 8 >= 4              # columns of O the hi = 1 lanes hold
    first_db = np.arange(Dh) % ndb == 0
    m, l, o, bias = np.zeros((2, R)), np.zeros((2, R)), np.zeros((R, Dh)), np.zeros(R)
    tr = {n: np.zeros((R, tiles)) for n in ("before", "after", "mx")}
    tr["fired"] = np.zeros((R, tiles), dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(tiles):
            s = S2[:, j * F32_TILE:(j + 1) * F32_TILE] - bias[:, None]
            whole = s.max(axis=1)
            p = np.zeros_like(s)
            for h in (0, 1):
                mine = half == bool(h)
                mx = s[:, mine].max(axis=1) if mutant == "rebase_other_half" and h == 1 else whole
                grow = mx > F32_THRESHOLD if j > 0 or mutant == "first_tile_keeps_m0" else np.ones(R, dtype=bool)
                delta = np.where(grow, mx, 0.0)
                lost = np.isneginf(delta)               # (rebase_other_half, tile 0, no key in the half: s - mask_value = 0 on its 16 slots)
                delta = np.where(lost, 0.0, delta)
                corr = np.ones(R) if j == 0 else np.exp2(-delta)
                m[h] += delta
                l[h] *= corr
                reach = (cols == bool(h)) & (first_db if mutant == "rebase_only_first_db" and j > 0 else True)
                if not (mutant == "rebase_l_not_o" and j > 0):
                    o[:, reach] *= corr[:, None]
                kept = mutant == "rebase_scores_not_shifted" and j > 0
                ph = np.where(lost[:, None], 1.0, np.exp2(s[:, mine] - (0.0 if kept else delta[:, None])))
                p[:, mine] = _fp32_range(ph)
                l[h] += p[:, mine].sum(axis=1)
                if h == 0:
                    tr["before"][:, j], tr["mx"][:, j], tr["fired"][:, j] = bias, whole, grow & (j > 0)
            o += np.where(p > 0, p, 0.0) @ V[j * F32_TILE:(j + 1) * F32_TILE]
            if not (mutant == "rebase_bias_stale" and j > 0):
                bias = m[0].copy()
            tr["after"][:, j] = m[0]
        ltot = l[0] + l[1]
        return o / ltot[:, None], m[0] + np.log2(ltot), tr


DO_PATHS = ("convert_dO", "bf16_products")             # how a backwardKeyValue kernel of the FP16 + BF16-dO mix reads dO (docstring)
# backwardKeyValue variant prefix -> its path in the mix, with the source line it was read from (the first matching prefix holds).
# Every backwardQuery kernel converts (attn_dq16_p4.h:148, attn_dq16_p5.h:189, attn_bwd16.h:114 `convert_chunk<T, TG>`).
MIX_PATH = (
    ("attn_dkv16p4", "bf16_products"),    # attn_dkv16_p4.h:129 `if constexpr (stream_mix(STREAM)) ... convert_chunk<__bf16, T>(vx)`, P packed by the stream
    ("attn_dkv16p5", "bf16_products"),    # attn_dkv16_p5.h:142-144, the same conversion of V; first_is_bf16 (:210)
    ("attn_dkv16rs", "convert_dO"),       # attn_dkv16_rs.h:176 `convert_chunk<T, TG>(greg[i])`
    ("attn_dkv16w_", "convert_dO"),       # attn_dkv16_wide.h:121, the same line
    ("attn_dkv16_", "convert_dO"),        # attn_bwd16.h:491, the same line (the one-wave kernel)
)
# the rounding of the 16-bit stores, per family: FP16 always rounds to nearest (`(_Float16)x`, `v_cvt_pk_f16_f32`); BF16:
STORE_ROUNDING = (
    ("attn_fwd16_p4p", "nearest"),        # tools/p4pgen.py:449 `v_cvt_pk_bf16_f32` under cfg.o16 (the hand-placed persistent streams)
    ("attn_fwd16_p6", "nearest"),         # tools/p6gen.py:612, the same instruction under cfg.o16
    ("", "trunc"),                        # every other store: attn_fwd16_common.h:32 pack16 (store_block_rows; attn_fwd16_v3.h:877, attn_fwd16_wide.h:338),
)                                         # attn_common.h:71 f32_to_bf16_trunc (store_elem: the combine kernels; attn_kv_group_sum.hip:74)


U_BF16 = U_P["bf16"]
SMALL_DO = 2.0 ** -14                                 # FP16's smallest normal number


def mix_path(variant):
    return next(path for prefix, path in MIX_PATH if variant.startswith(prefix))


def store_rounding(form):
    """the BF16 rounding of the store of a launch whose form (launchForm) is `form`: STORE_ROUNDING's first matching prefix"""
    return next(rounding for prefix, rounding in STORE_ROUNDING if form.startswith(prefix))


def off_grid_grad(dO):
    """BF16 values -> FP16 values three quarters of a BF16 ulp further from zero (six FP16 ulps: exact above 2^-14): round-to-nearest
    takes every element one BF16 ulp up in magnitude, truncation gives dO back -- a grad_out on which the two roundings differ everywhere"""
    _m, e = np.frexp(dO)                              # |dO| = m 2^e, m in [0.5, 1): the BF16 ulp is 2^(e - 8)
    grad = dO + np.sign(dO) * 0.75 * np.exp2(e - 8.0)
    assert np.array_equal(round_to(grad, "f16"), grad) and (np.abs(dO) >= SMALL_DO).all() and (dO != 0).all()
    return grad


def _bits_as_f16(x):
    """BF16 values -> the FP16 values of the same 16 bits"""
    bits = (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    with np.errstate(all="ignore"):
        return bits.view(np.float16).astype(np.float64)


def model(q, k, v, dO, *, causal=False, row_lengths=None, key_lengths=None, pieces=None, block_mask=None, mutant=None, fmt="bf16", mixed=True,
          with_bounds=True, out="f32", dO_fmt=None, dO_path=None, heads_per_kv=1):
    """-> Reference (with_bounds=False: A, E and PK stay zero).  pieces: None or {"fwd": [(key begin, end)], "dq": [(key begin, end)], "dkv": [(row begin, end)]} (they change the
    bound's chain and what the mutants do, never the unmutated values).  A mutated run leaves NaN where its launch writes nothing."""
    assert mutant is None or mutant in MUTANTS, mutant
    q, k, v, dO = f64(q), f64(k), f64(v), f64(dO)
    B, H, R, Dh = q.shape
    C = k.shape[2]
    Gq = int(heads_per_kv)
    Hkv = H // Gq
    assert H == Hkv * Gq and k.shape[1] == Hkv and v.shape[1] == Hkv, (q.shape, k.shape, Gq)
    mix = dO_fmt is not None and dO_fmt != fmt
    assert not mix or ((fmt, dO_fmt) == ("f16", "bf16") and dO_path in DO_PATHS), (fmt, dO_fmt, dO_path)
    ofmt = out                                        # (`out` names the outputs below)
    out16 = ofmt != "f32"
    scale = 1.0 / math.sqrt(Dh)
    f32 = fmt == "f32"
    assert not f32 or (not mixed and not mix and ofmt == "f32" and block_mask is None), "FP32 operands: exact mode, FP32 outputs, no mask"
    assert mutant not in F32_MUTANTS or f32, "the re-base mutants are attn_f32_fwd's"
    u = U_OF[fmt]
    fl = F16_FLOOR if fmt == "f16" else 0.0
    cf = F16_FLOOR if mix else 0.0                    # dO converted to FP16: exact mantissa, FP16's subnormal floor
    products = mix and dO_path == "bf16_products"     # backwardKeyValue: V and P rounded to BF16 for dP and dV
    rl, cl = _lengths(row_lengths, B, R), _lengths(key_lengths, B, C)
    rl_used = np.roll(rl, -1) if mutant == "row_length_next_batch" else rl
    pieces = pieces or {}
    npieces = max(len(pieces.get("fwd", ())), len(pieces.get("dq", ())), len(pieces.get("dkv", ())), 1)
    chain, chain_r = (C / 8 + npieces + 16) * U32, (R / 8 + npieces + 16) * U32
    if f32:      # two keys (rows) per matrix instruction, one rounding each; 32-wide tiles: the sums of l, one re-base on l and O
        chain, chain_r = (C + 3 * -(-C // F32_TILE) + npieces + 24) * U32, (R + 3 * -(-R // F32_TILE) + npieces + 24) * U32
    out = {n: np.full((B, H, R, Dh) if n in ("O", "dQ") else (B, Hkv, C, Dh), np.nan) for n in ("O", "dV", "dK", "dQ")}
    out["L"], out["D"] = np.full((B, H, R), np.nan), np.full((B, H, R), np.nan)
    slabs = {}                                        # (b, h) -> a query head's dV, dK and their E and A: summed per group below
    A = {n: np.zeros_like(out[n]) for n in ("O", "dV", "dK", "dQ")}
    E = {n: np.zeros_like(out[n]) for n in OUTPUTS}
    PK = np.zeros((B, H, R, Dh))
    dead_rows = np.zeros((B, H, R), dtype=bool)
    want_bounds = mutant is None and with_bounds
    fwd = {}
    for b in range(B):
        rlen, clen = int(rl_used[b]), int(cl[b])
        for h in range(H):
            hk = (h + 1) % H if mutant == "row_block_next_head_kv" else h
            K, V = k[b, h // Gq], v[b, h // Gq]
            S = (q[b, h] @ K.T) * scale
            vis, visF, visQ, visK = mask_views(block_mask, b, h, R, C, rlen, clen, causal, mutant)
            md = True if block_mask is None else mask_dense(mask_bits(block_mask, b, h), R, C)
            mult = None
            if mutant == "causal_plus_1":
                visF = _visible(R, C, rlen, clen, causal, +1) & md
            elif mutant == "causal_minus_1":
                visF = _visible(R, C, rlen, clen, causal, -1) & md
            elif mutant in ("key0_dropped", "last_key_dropped", "partial_last_tile_dropped", "tile_skipped_in_one_row_block"):
                visF = vis.copy()
                if mutant == "key0_dropped":
                    visF[:, 0] = False
                elif mutant == "last_key_dropped":
                    visF[:, clen - 1] = False
                elif mutant == "partial_last_tile_dropped" and clen % TILE:
                    visF[:, clen // TILE * TILE:] = False
                elif mutant == "tile_skipped_in_one_row_block":
                    visF[(rlen - 1) // BLOCK_ROWS * BLOCK_ROWS:, TILE:2 * TILE] = False
            Vf = V
            if mutant == "v_rows_exchanged" and clen >= 2:
                src = np.arange(C)
                x = 30 if clen >= 32 else 0
                src[x], src[x + 1] = x + 1, x
                Vf = V[src]
            if mutant == "piece_loses_last_tile" and len(pieces.get("fwd", ())) > 1:
                visF = visF.copy()
                for pb, pe in pieces["fwd"]:
                    pe = min(pe, clen)
                    if pe > pb:
                        visF[:, max(pb, (pe - 1) // TILE * TILE):pe] = False
            if mutant == "piece_overlaps" and len(pieces.get("fwd", ())) > 1:
                mult = np.ones(C)
                for pb, pe in pieces["fwd"]:
                    if min(pe, clen) > pb and pb >= TILE:
                        mult[pb - TILE:pb] += 1.0
            P, m, l = _softmax(S, visF, mult)
            O = P @ Vf
            L = m + np.log(l)
            unseeing = ~visF.any(axis=1)                  # dead rows (of this forward): O = 0 as computed, L hugely negative
            if mutant == "dead_row_uniform":
                O[unseeing] = Vf[:clen].mean(axis=0)
            else:
                L = np.where(unseeing, -np.inf, L)
            if mutant == "row_block_next_head_kv":     # rows of block 0 from head h + 1's K / V
                S1 = (q[b, h] @ k[b, hk // Gq].T) * scale
                P1, m1, l1 = _softmax(S1, visF)
                blk = slice(0, BLOCK_ROWS)
                O[blk], L[blk] = (P1 @ v[b, hk // Gq])[blk], (m1 + np.log(l1))[blk]
            if mutant == "combine_ignores_maxima" and len(pieces.get("fwd", ())) > 1:
                num, den = np.zeros((R, Dh)), np.zeros(R)
                Sm = np.where(visF, S, -np.inf)
                for pb, pe in pieces["fwd"]:
                    pe = min(pe, clen)
                    if pe <= pb:
                        continue
                    pm = Sm[:, pb:pe].max(axis=1)
                    ok = np.isfinite(pm)
                    e = np.where(ok[:, None], np.exp(Sm[:, pb:pe] - np.where(ok, pm, 0.0)[:, None]), 0.0)
                    num += e @ Vf[pb:pe]
                    den += e.sum(axis=1)
                O = num / den[:, None]
                L = m + np.log(den)
            if mutant == "rescale_o_not_l":
                S2 = np.where(visF, S, -np.inf) * LOG2E
                run, lm, fired = np.full(R, -1e30), np.zeros(R), np.zeros(R, dtype=bool)
                for t0 in range(0, clen, TILE):
                    tm = S2[:, t0:t0 + TILE].max(axis=1)
                    fired |= (tm > run + RESCALE_THRESHOLD) & (lm > 0)
                    run = np.where(tm > run + RESCALE_THRESHOLD, tm, run)     # O is rescaled here; l is not
                    lm = lm + np.exp2(S2[:, t0:t0 + TILE] - run[:, None]).sum(axis=1)
                ltrue = np.exp2(S2 - run[:, None]).sum(axis=1)
                O = np.where(fired[:, None], O * (ltrue / lm)[:, None], O)
                L = np.where(fired, (run + np.log2(lm)) / LOG2E, L)
            if mutant in F32_MUTANTS:      # rows on which the mutated walk gives the unmutated walk's values keep the model's own
                S2w = np.where(visF, S, -np.inf) * LOG2E
                Ow, Lw, _tr = _rebase_walk(S2w, Vf)
                Om, Lm, _tr = _rebase_walk(S2w, Vf, mutant)
                with np.errstate(all="ignore"):
                    same = np.isclose(Om, Ow, rtol=1e-9, atol=1e-12).all(axis=1) & np.isclose(Lm, Lw, rtol=1e-9, atol=1e-9)
                O, L = np.where(same[:, None], O, Om), np.where(same, L, Lm / LOG2E)
            if mutant == "l_without_key0":
                with np.errstate(divide="ignore", invalid="ignore"):
                    L = L + np.log1p(-P[:, 0])
            if mutant == "wave_groups_exchanged":
                n = max(0, min(WAVE_ROWS, rlen - WAVE_ROWS))
                O, L = O.copy(), L.copy()
                O[:n], O[WAVE_ROWS:WAVE_ROWS + n] = O[WAVE_ROWS:WAVE_ROWS + n].copy(), O[:n].copy()
                L[:n], L[WAVE_ROWS:WAVE_ROWS + n] = L[WAVE_ROWS:WAVE_ROWS + n].copy(), L[:n].copy()
            if mutant == "v_dblocks_exchanged" and Dh >= 64:
                O = np.concatenate([O[:, 32:64], O[:, :32], O[:, 64:]], axis=1)
            if mutant == "o_zero":
                O = np.zeros_like(O)
            if mutant == "out16_piece_rounded_before_combine" and out16 and len(pieces.get("fwd", ())) > 1:
                O = sum(store(P[:, pb:min(pe, clen)] @ Vf[pb:min(pe, clen)], ofmt) for pb, pe in pieces["fwd"] if min(pe, clen) > pb)
            fwd[(b, h)] = (S, P, m, l, O, L, (dO[b, h] * O).sum(axis=1), vis, visQ, visK, md)
    for b in range(B):
        rlen, clen = int(rl_used[b]), int(cl[b])
        live_r = np.arange(R) < rlen
        live_c = np.arange(C) < clen
        for h in range(H):
            S, P0, m, l, O, L, Dv, vis, visQ, visK, md = fwd[(b, h)]
            dead_rows[b, h] = live_r & ~vis.any(axis=1)
            K, V, Q, G = k[b, h // Gq], v[b, h // Gq], q[b, h], dO[b, h]
            Gk_all = G                                 # dO as backwardKeyValue's dP product reads it
            if mix and mutant == "dO_bits_as_input_type":
                G = Gk_all = _bits_as_f16(G)
            elif mix and mutant == "dO_small_flushed":
                G = Gk_all = np.where(np.abs(G) < SMALL_DO, 0.0, G)
            elif mix and mutant == "dO_converted_in_dv_only":
                Gk_all = _bits_as_f16(G)
            if G is not dO[b, h]:
                with np.errstate(all="ignore"):
                    Dv = (G * O).sum(axis=1)
            if mutant == "d_from_unstored_o_next_head" and out16:
                Dv = (G * fwd[(b, (h + 1) % H)][4]).sum(axis=1)
            if mutant == "d_zero":
                Dv = np.zeros(R)
            elif mutant == "d_wrong":
                Dv = Dv * (1.0 + 2.0 ** -4)
            elif mutant == "d_neighbour_row":
                Dv = np.concatenate([Dv[1:rlen], Dv[:1], Dv[rlen:]])
            elif mutant == "d_next_head":
                Dv = fwd[(b, (h + 1) % H)][6]
            Lb = np.concatenate([L[1:rlen], L[:1], L[rlen:]]) if mutant == "l_neighbour_row" else L
            visB = visQ
            if mutant == "bwd_causal_plus_1":
                visB = visK = _visible(R, C, rlen, clen, causal, +1) & md
            elif mutant == "bwd_causal_minus_1":
                visB = visK = _visible(R, C, rlen, clen, causal, -1) & md
            with np.errstate(over="ignore", invalid="ignore"):
                Pall = np.exp(S - Lb[:, None])          # the backward kernels' P = exp(s - L), for every (row, key) of the buffers
                Pb = np.where(visB, Pall, 0.0)
                dP = G @ V.T
                dS = Pb * (dP - Dv[:, None])
                dPk = dP if Gk_all is G else Gk_all @ V.T
                PbK, dSK = (Pb, dS) if visK is visB and dPk is dP else (np.where(visK, Pall, 0.0), np.where(visK, Pall, 0.0) * (dPk - Dv[:, None]))
            # ---- dQ: rows below the row length, keys the pass reads
            Pq, dSq = Pb, dS
            if mutant in ("dq_last_tile_dropped", "dq_tile_skipped_in_one_row_block", "dq_reads_padding_keys"):
                keep = np.ones((R, C), dtype=bool)
                if mutant == "dq_last_tile_dropped":
                    keep[:, (clen - 1) // TILE * TILE:] = False
                elif mutant == "dq_tile_skipped_in_one_row_block":
                    keep[(rlen - 1) // BLOCK_ROWS * BLOCK_ROWS:, TILE:2 * TILE] = False
                dSq = np.where(keep, dS, 0.0)
                if mutant == "dq_reads_padding_keys" and clen < C:
                    dSq = dSq.copy()
                    dSq[:, clen] = Pall[:, clen] * (dP[:, clen] - Dv)
            dq_scale = {"ds_scale_missing": 1.0, "ds_scale_twice": scale * scale}.get(mutant, scale)
            dQ = dq_scale * (dSq @ K)
            if mutant == "dq_scaled":
                dQ = dQ * (1.0 - 2.0 ** -5)
            if mutant in ("bwd_combine_drops_slab", "bwd_combine_adds_slab_twice") and len(pieces.get("dq", ())) > 1:
                pb, pe = pieces["dq"][1]
                slab = dq_scale * (dSq[:, pb:pe] @ K[pb:pe])
                dQ = dQ - slab if mutant == "bwd_combine_drops_slab" else dQ + slab
            # ---- dK / dV: keys below the key length, rows the pass reads
            rows_in = live_r.copy()
            if mutant == "dkv_last_step_dropped":
                rows_in[(rlen - 1) // STEP * STEP:] = False
            elif mutant == "dkv_row_block_dropped":
                rows_in[(rlen - 1) // BLOCK_ROWS * BLOCK_ROWS:] = False
            Pk, dSk = PbK[rows_in], dSK[rows_in]
            Gk, Qk = G[rows_in], Q[rows_in]
            if mutant == "dkv_reads_padding_rows" and rlen < R:
                prow = np.where(live_c, Pall[rlen], 0.0)[None, :]
                Pk, dSk = np.concatenate([Pk, prow]), np.concatenate([dSk, prow * (dP[rlen] - Dv[rlen])[None, :]])
                Gk, Qk = np.concatenate([Gk, G[rlen:rlen + 1]]), np.concatenate([Qk, Q[rlen:rlen + 1]])
            dV = Pk.T @ Gk
            dK = dq_scale * (dSk.T @ Qk)
            if mutant in ("bwd_combine_drops_slab", "bwd_combine_adds_slab_twice") and len(pieces.get("dkv", ())) > 1:
                pb, pe = pieces["dkv"][1]
                sel = np.zeros(R, dtype=bool)
                sel[pb:pe] = True
                sel &= live_r
                sv, sk = PbK[sel].T @ G[sel], dq_scale * (dSK[sel].T @ Q[sel])
                sign = -1.0 if mutant == "bwd_combine_drops_slab" else 1.0
                dV, dK = dV + sign * sv, dK + sign * sk
            if mutant == "dk_dv_exchanged":
                dV, dK = dK, dV
            if mutant == "out16_piece_rounded_before_combine" and out16:
                if len(pieces.get("dq", ())) > 1:
                    dQ = sum(store(dq_scale * (dSq[:, pb:min(pe, clen)] @ K[pb:min(pe, clen)]), ofmt) for pb, pe in pieces["dq"] if min(pe, clen) > pb)
                if len(pieces.get("dkv", ())) > 1:
                    sel = [live_r & (np.arange(R) >= pb) & (np.arange(R) < pe) for pb, pe in pieces["dkv"]]
                    dV = sum(store(PbK[x].T @ G[x], ofmt) for x in sel if x.any())
                    dK = sum(store(dq_scale * (dSK[x].T @ Q[x]), ofmt) for x in sel if x.any())
            Dout = Dv
            Oout = O
            if mutant == "o16_row_pairs_exchanged" and out16 and rlen >= 2:
                Oout = np.concatenate([O[1:2], O[:1], O[2:]])
            for name, val, live in (("O", Oout, live_r), ("L", L, live_r), ("D", Dout, live_r), ("dQ", dQ, live_r)):
                out[name][b, h][live] = val[live]
            if mutant == "out16_last_chunk_dropped" and out16:
                out["O"][b, h, 0, -8:], out["dQ"][b, h, 0, -8:] = np.nan, np.nan
            slabs[(b, h)] = [dV, dK, None, None, None, None, live_c]
            if not want_bounds:
                continue
            # ---- the magnitude sums and the error terms (margin 1, without the stores)
            P = np.where(live_r[:, None], P0, 0.0)
            aK, aV, aQ, aG = np.abs(K), np.abs(V), np.abs(Q), np.abs(G)
            T = scale * (aQ @ aK.T)
            smin = np.where(vis, S, np.inf).min(axis=1)
            spread2 = np.where(np.isfinite(smin), (m - np.where(np.isfinite(smin), smin, m)) * LOG2E, 0.0)
            rho = LN2 * ((Dh + 3) * U32 * LOG2E * T + 3 * U32 * spread2[:, None]) + 4 * U32
            if f32:     # the chain of a score starts at -m: M, the kernel's reference maximum around every key's tile (docstring)
                _o, _l2, walk = _rebase_walk(np.where(vis, S, -np.inf) * LOG2E, V)
                Mt = np.maximum(np.abs(walk["before"]), np.abs(walk["after"]))
                with np.errstate(invalid="ignore"):
                    Mt = Mt + 8.0 * (np.abs(walk["mx"] - F32_THRESHOLD) < 2.0 ** -8)[:, 1:].any(axis=1)[:, None]
                Mkey = np.repeat(Mt, F32_TILE, axis=1)[:, :C]
                rho = LN2 * U32 * ((Dh + 3) * (LOG2E * T + Mkey) + 2 * (Mt.max(axis=1)[:, None] + 8.0)) + 4 * U32
            visl = (vis & live_r[:, None]).astype(np.float64)
            if mixed:
                rho = rho + u * T
            rp = rho * P
            relp = rp.sum(axis=1) + fl * visl.sum(axis=1)
            AO = P @ aV
            absO = np.abs(np.where(live_r[:, None], O, 0.0))
            EO = u * AO + (u * absO if mixed else 0.0) + fl * (visl @ aV) + rp @ aV + absO * relp[:, None] + chain * (AO + absO)
            GO = np.where(live_r[:, None], G * O, 0.0)
            if ofmt == "f32":
                stored = U_OUT["f32"] * np.abs(GO).sum(axis=1)
            elif ofmt == "bf16":   # one sign per element: the positive and the negative products move D in opposite directions
                stored = U_OUT[ofmt] * (np.maximum(np.maximum(GO, 0.0).sum(axis=1), np.maximum(-GO, 0.0).sum(axis=1)) + (aG * EO).sum(axis=1))
            else:
                stored = U_OUT[ofmt] * (np.abs(GO).sum(axis=1) + (aG * EO).sum(axis=1)) + F16_FLOOR * np.where(live_r, aG.sum(axis=1), 0.0)
            L = np.where(np.isfinite(L), L, 0.0)          # (a dead row: every term of its bounds is 0 but the constants)
            Lf = np.where(live_r, L, 0.0)
            EL = relp + (u if mixed else 0.0) + chain + 4 * U32 * (np.abs(m) + np.abs(np.log(l)) + np.abs(Lf)) + (2.0 ** -11 if mixed else 2.0 ** -23) * np.abs(Lf)
            if f32:
                EL = EL + 4 * U32 * 16 * LN2
            Df = np.where(live_r, Dv, 0.0)
            dP = np.where(live_r[:, None], dP, 0.0)
            dev = np.abs(dP - Df[:, None])
            ED = (P * (u * (dev if mixed else np.abs(dP)) + rho * dev)).sum(axis=1) + fl * (visl * np.abs(dP)).sum(axis=1) \
                + chain * ((P * np.abs(dP)).sum(axis=1) + np.abs(Df)) + (Dh + 2) * U32 * (aG * absO).sum(axis=1) + stored \
                + cf * absO.sum(axis=1) + (2.0 ** -7 if mixed else 2.0 ** -23) * np.abs(Df)
            rhob = rho + EL[:, None]
            dSl = np.where(live_r[:, None], dS, 0.0)
            edP = (Dh + 3) * U32 * (aG @ aV.T)
            if f32:     # the backward accumulators start at -L and -D (dQ) or at L and D (dK / dV)
                rhob = LN2 * U32 * (Dh + 3) * LOG2E * (T + np.abs(Lf)[:, None]) + 4 * U32 + EL[:, None]
                edP = edP + (Dh + 3) * U32 * np.abs(Df)[:, None]
            eds = P * ((rhob + u) * dev + edP + cf * aV.sum(axis=1)[None, :] + ED[:, None]) + u * np.abs(dSl) + fl * visl * (dev + math.sqrt(Dh))
            # backwardKeyValue of the mix: dO converted as in backwardQuery, or (bf16_products) V rounded to BF16 and dO as stored
            eds_k = eds + P * (U_BF16 * (aG @ aV.T) - cf * aV.sum(axis=1)[None, :]) if products else eds
            u_dv = U_BF16 if products else u
            A["O"][b, h] = AO
            A["dQ"][b, h] = scale * (np.abs(dSl) @ aK)
            PK[b, h] = scale * (P @ aK)
            E["O"][b, h], E["L"][b, h], E["D"][b, h] = EO, EL, ED
            AdV, AdK = P.T @ aG, scale * (np.abs(dSl).T @ aQ)
            EdV = (P * (rhob + u_dv) + fl * visl).T @ aG + (0.0 if products else cf) * P.sum(axis=0)[:, None] + chain_r * AdV
            E["dQ"][b, h] = scale * (eds @ aK) + chain * A["dQ"][b, h]
            slabs[(b, h)][2:6] = EdV, scale * (eds_k.T @ aQ) + chain_r * AdK, AdV, AdK
    for b in range(B):            # dK / dV of K / V head j: the slabs of its G query heads, in the order g = 0 .. G - 1 (attn_kv_group_sum)
        for j in range(Hkv):
            members = [slabs[(b, j * Gq + g)] for g in range(Gq)]
            if mutant == "group_slab_dropped" and Gq > 1:
                members = members[:1] + members[2:]
            elif mutant == "group_slab_twice" and Gq > 1:
                members = members[:2] + members[1:]
            elif mutant == "group_sum_head_is_query_head" and Gq > 1:
                members = [slabs[(b, j)]]
            each = (lambda x: store(x, ofmt)) if mutant == "group_store_rounds_each_slab" and out16 and Gq > 1 else (lambda x: x)
            live = members[0][6]
            out["dV"][b, j][live] = sum(each(m_[0]) for m_ in members)[live]
            out["dK"][b, j][live] = sum(each(m_[1]) for m_ in members)[live]
            if mutant == "out16_last_chunk_dropped" and out16:
                out["dK"][b, j, 0, -8:] = np.nan
            if want_bounds:
                more = Gq * U32 if Gq > 1 else 0.0       # the group sum's FP32 additions, on the summed magnitudes
                A["dV"][b, j], A["dK"][b, j] = sum(m_[4] for m_ in members), sum(m_[5] for m_ in members)
                E["dV"][b, j] = sum(m_[2] for m_ in members) + more * A["dV"][b, j]
                E["dK"][b, j] = sum(m_[3] for m_ in members) + more * A["dK"][b, j]
    row_live = np.arange(R)[None, :] < rl[:, None]
    key_live = np.arange(C)[None, :] < cl[:, None]
    return Reference(out["O"], out["L"], out["D"], out["dV"], out["dK"], out["dQ"], A, E, PK, row_live, key_live, dead_rows)


def margin_of(fmt=None):
    return MARGIN_F32 if fmt == "f32" else MARGIN


def bounds(ref, out="f32", margin=None, fmt=None):
    """{output: per-element bound}: see the module's docstring.  `out`: the type O, dQ, dK, dV are stored in (L and D: their own
    store is part of E, the mode decides it).  fmt: the operands' type the Reference was built for (it decides the default margin)"""
    margin = margin_of(fmt) if margin is None else margin
    assert fmt != "f32" or out == "f32"
    res = {}
    for name in OUTPUTS:
        x = np.nan_to_num(getattr(ref, name), nan=0.0)
        st = 0.0 if name in ("L", "D") else U_OUT[out] * np.abs(x)
        res[name] = margin * (ref.E[name] + st) + TINY
    return res


# ------------------------------------------------------------------------------------------------- the rounding-emulated reference
def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def emulated(q, k, v, dO, fmt, mixed, *, causal=False, row_lengths=None, key_lengths=None, pieces=None, block_mask=None, out="f32",
             o_rounding="trunc", dO_fmt=None, dO_path=None, heads_per_kv=1, trace=None, forward_only=False):
    """the model with the kernels' roundings and order of sums -> {output: array}, NaN where nothing is written: Q' (K' in
    backwardKeyValue) rounded once in the mixed mode, 64-key tiles under the deferred rescale, P and dS rounded to the 16-bit type,
    l from the rounded P in the mixed mode, pieces merged, L in FP16 and D in truncated BF16 in the mixed mode, the stores.
    out: O, dQ, dK, dV are stored in that type and D is formed from the STORED O; o_rounding ("trunc" | "nearest"): the rounding of
    the forward's BF16 O store (STORE_ROUNDING; FP16 always rounds to nearest, the gradients' BF16 stores always truncate).  dO_fmt /
    dO_path: the FP16 + BF16-dO mix (model()).  heads_per_kv: the FP32 slabs of a group are added in the order g = 0 .. G - 1 and the sum is
    stored once.  fmt = "f32": the walk of attn_f32.h (docstring; _emulated_f32); trace (a dict) receives {(b, h): the walk's per-tile
    record}, forward_only leaves the gradients and D unwritten"""
    if fmt == "f32":
        assert not mixed and out == "f32" and block_mask is None and not pieces and (dO_fmt or fmt) == fmt
        return _emulated_f32(f64(q), f64(k), f64(v), f64(dO), causal, row_lengths, key_lengths, int(heads_per_kv), trace, forward_only)
    q, k, v, dO = f64(q), f64(k), f64(v), f64(dO)
    B, H, R, Dh = q.shape
    C = k.shape[2]
    Gq = int(heads_per_kv)
    mix = dO_fmt is not None and dO_fmt != fmt
    assert not mix or dO_path in DO_PATHS
    products = mix and dO_path == "bf16_products"
    scale = 1.0 / math.sqrt(Dh)
    s2c = float(np.float32(LOG2E * scale))
    rl, cl = _lengths(row_lengths, B, R), _lengths(key_lengths, B, C)
    pieces = pieces or {}
    res = {n: np.full((B, H, R, Dh) if n in ("O", "dQ") else (B, H // Gq, C, Dh), np.nan) for n in ("O", "dV", "dK", "dQ")}
    res["L"], res["D"] = np.full((B, H, R), np.nan), np.full((B, H, R), np.nan)
    for b in range(B):
        rlen, clen = int(rl[b]), int(cl[b])
        for h in range(H):
            vis = mask_views(block_mask, b, h, R, C, rlen, clen, causal)[0][:rlen, :clen]
            dead = ~vis.any(axis=1)                       # (a dead row: no tile is run, l = 0; O = 0 and L hugely negative by rule)
            Q, K, V, G = q[b, h, :rlen], k[b, h // Gq, :clen], v[b, h // Gq, :clen], dO[b, h, :rlen]
            if mix:                                       # (T)(float): attn_bwd16.h convert_chunk
                G = round_to(G, fmt)
            Gk, Vk, pfmt = (dO[b, h, :rlen], round_to(V, "bf16"), "bf16") if products else (G, V, fmt)
            if mixed:
                S2q = _f32(round_to(Q * s2c, fmt) @ K.T)
                S2k = _f32(Q @ round_to(K * s2c, fmt).T)
            else:
                S2q = S2k = _f32(_f32(Q @ K.T) * s2c)
            S2 = np.where(vis, S2q, -np.inf)
            parts = []
            for pb, pe in (pieces.get("fwd") or [(0, clen)]):
                pe = min(pe, clen)
                run, l, o = np.full(rlen, -1e30), np.zeros(rlen), np.zeros((rlen, Dh))
                for t0 in range(pb, pe, TILE):
                    s = S2[:, t0:min(t0 + TILE, pe)]
                    tm = s.max(axis=1)
                    new = np.where(tm > run + RESCALE_THRESHOLD, tm, run)
                    corr = _f32(np.exp2(run - new))
                    p = _f32(np.exp2(s - new[:, None]))
                    pr = round_to(p, fmt)
                    l = _f32(l * corr + (pr if mixed else p).sum(axis=1))
                    o = _f32(o * corr[:, None] + pr @ V[t0:min(t0 + TILE, pe)])
                    run = new
                parts.append((run, l, o))
            mstar = np.max([p[0] for p in parts], axis=0)
            lt = sum(_f32(np.exp2(m_ - mstar)) * l_ for m_, l_, _o in parts)
            ot = sum(_f32(np.exp2(m_ - mstar))[:, None] * o_ for m_, _l, o_ in parts)
            lt = np.where(dead, 1.0, lt)
            O = round_to(_f32(ot / lt[:, None]), out, trunc=out == "bf16" and o_rounding == "trunc")
            L2 = np.where(dead, -np.inf, _f32(mstar + np.log2(lt)))
            L2 = round_to(L2, "f16") if mixed else L2
            Dv = _f32((G * O).sum(axis=1))
            Dst = round_to(Dv * scale, "bf16", trunc=True) / scale if mixed else Dv
            dP = _f32(G @ V.T)
            with np.errstate(over="ignore"):
                Pq = np.where(vis, _f32(np.exp2(S2q - L2[:, None])), 0.0)
                Pk = np.where(vis, _f32(np.exp2(S2k - L2[:, None])), 0.0)
            dSq = round_to(round_to(Pq, fmt) * (dP - Dv[:, None]), fmt)
            dPk = _f32(Gk @ Vk.T) if products else dP
            dSk = round_to(scale * round_to(Pk, fmt) * (dPk - Dst[:, None]), fmt)     # dS' = scale dS: attn_dkv16_rs.h
            dQ = sum(_f32(dSq[:, pb:pe] @ K[pb:pe]) for pb, pe in (pieces.get("dq") or [(0, clen)])) * scale
            rr = [(pb, min(pe, rlen)) for pb, pe in (pieces.get("dkv") or [(0, rlen)])]
            dV = sum(_f32(round_to(Pk[pb:pe], pfmt).T @ Gk[pb:pe]) for pb, pe in rr if pe > pb)
            dK = sum(_f32(dSk[pb:pe].T @ Q[pb:pe]) for pb, pe in rr if pe > pb)
            res["O"][b, h, :rlen], res["L"][b, h, :rlen], res["D"][b, h, :rlen] = O, L2 / LOG2E, Dst
            res["dQ"][b, h, :rlen] = store(_f32(dQ), out)
            if h % Gq == 0:
                sv, sk = _f32(dV), _f32(dK)
            else:
                sv, sk = _f32(sv + _f32(dV)), _f32(sk + _f32(dK))
            if h % Gq == Gq - 1:
                res["dV"][b, h // Gq, :clen], res["dK"][b, h // Gq, :clen] = store(sv, out), store(sk, out)
    return res


def _chain32(init, A, B):
    """init [n, m] + A [n, D] B [m, D]^T as one first product of attn_f32.h adds it up: one FP32 rounding per matrix instruction, which
    contracts d = 8 T + i (hi = 0) and 8 T + 4 + i (hi = 1)"""
    Dh = A.shape[1]
    pad = -Dh % 8
    A, B = np.pad(A, ((0, 0), (0, pad))), np.pad(B, ((0, 0), (0, pad)))
    acc = np.array(init, dtype=np.float64)
    for T in range((Dh + pad) // 8):
        for i in range(4):
            d0, d1 = 8 * T + i, 8 * T + 4 + i
            acc = _f32(acc + A[:, d0:d0 + 1] * B[None, :, d0] + A[:, d1:d1 + 1] * B[None, :, d1])
    return acc


def _accum32(acc, W, X):
    """acc [n, D] + W [n, 32] X [32, D] as one second product adds a 32-wide tile up: step t contracts crow(t, 0) and crow(t, 1)"""
    for t in range(16):
        a, b = crow(t, 0), crow(t, 1)
        acc = _f32(acc + W[:, a:a + 1] * X[a] + W[:, b:b + 1] * X[b])
    return acc


def _emulated_f32(q, k, v, dO, causal, row_lengths, key_lengths, Gq, trace, forward_only):
    B, H, R, Dh = q.shape
    C = k.shape[2]
    sc = float(np.float32(1.0 / math.sqrt(Dh)))
    s2c = float(np.float32(LOG2E / math.sqrt(Dh)))
    rl, cl = _lengths(row_lengths, B, R), _lengths(key_lengths, B, C)
    res = {n: np.full((B, H, R, Dh) if n in ("O", "dQ") else (B, H // Gq, C, Dh), np.nan) for n in ("O", "dV", "dK", "dQ")}
    res["L"], res["D"] = np.full((B, H, R), np.nan), np.full((B, H, R), np.nan)
    half = np.arange(F32_TILE) % 8 >= 4
    order = [[crow(r, hi) for r in range(16)] for hi in (0, 1)]
    for b in range(B):
        rlen, clen = int(rl[b]), int(cl[b])
        tiles, rtiles = -(-clen // F32_TILE), -(-rlen // F32_TILE)
        vis = np.pad(_visible(R, C, rlen, clen, causal)[:rlen, :clen], ((0, rtiles * F32_TILE - rlen), (0, tiles * F32_TILE - clen)))
        for h in range(H):
            padk, padr = ((0, tiles * F32_TILE - clen), (0, 0)), ((0, rtiles * F32_TILE - rlen), (0, 0))
            Q, G = np.pad(q[b, h, :rlen], padr), np.pad(dO[b, h, :rlen], padr)          # (the bounds-checked resources fill with zeros)
            K, V = np.pad(k[b, h // Gq, :clen], padk), np.pad(v[b, h // Gq, :clen], padk)
            Q2 = _f32(Q * s2c)
            n = Q.shape[0]
            # ---- forward: 32-key tiles around the reference maximum m
            m, l, o = np.zeros(n), np.zeros((2, n)), np.zeros((n, Dh))
            rec = {name: np.zeros((n, tiles)) for name in ("before", "mx", "at")}
            rec["fired"] = np.zeros((n, tiles), dtype=bool)
            with np.errstate(all="ignore"):
                for j in range(tiles):
                    t = slice(j * F32_TILE, (j + 1) * F32_TILE)
                    s = np.where(vis[:, t], _chain32(np.repeat(-m[:, None], F32_TILE, axis=1), Q2, K[t]), -np.inf)
                    mx = s.max(axis=1)
                    grow = (mx > F32_THRESHOLD) if j else np.ones(n, dtype=bool)
                    rec["before"][:, j], rec["mx"][:, j], rec["fired"][:, j], rec["at"][:, j] = m, mx, grow & (j > 0), s.argmax(axis=1)
                    delta = np.where(grow, mx, 0.0)
                    corr = _f32(np.exp2(-delta)) if j else np.ones(n)
                    m = _f32(m + delta)
                    l, o = _f32(l * corr), _f32(o * corr[:, None])
                    p = _f32(np.exp2(_f32(s - delta[:, None])))
                    for hi in (0, 1):
                        psum = np.zeros(n)
                        for r in order[hi]:
                            psum = _f32(psum + p[:, r])
                        l[hi] = _f32(l[hi] + psum)
                    o = _accum32(o, p, V[t])
                ltot = _f32(l[0] + l[1])
                live = np.arange(n) < rlen                  # (rows past the length: Q, dO, L and D read as zeros, nothing is stored)
                O = np.where(live[:, None], _f32(o * _f32(1.0 / ltot)[:, None]), 0.0)
                L2 = np.where(live, _f32(m + _f32(np.log2(ltot))), 0.0)
            if trace is not None:
                trace[(b, h)] = {name: x[:rlen] for name, x in rec.items()}
            res["O"][b, h, :rlen], res["L"][b, h, :rlen] = O[:rlen], L2[:rlen] / LOG2E
            if forward_only:
                continue
            # ---- backwardQuery: accumulators started at -L and -sum(dO o O), three stages of 32-key tiles
            dsum = _f32((G * O).sum(axis=1))
            Dst = _f32(dsum * sc)
            with np.errstate(all="ignore"):
                P = _f32(np.exp2(_chain32(np.repeat(-L2[:, None], K.shape[0], axis=1), Q2, K)))
                dS = np.where(vis, _f32(P * _chain32(np.repeat(-dsum[:, None], K.shape[0], axis=1), G, V)), 0.0)
            acc = np.zeros((n, Dh))
            for j in range(tiles):
                acc = _accum32(acc, dS[:, j * F32_TILE:(j + 1) * F32_TILE], K[j * F32_TILE:(j + 1) * F32_TILE])
            res["dQ"][b, h, :rlen], res["D"][b, h, :rlen] = _f32(acc * sc)[:rlen], Dst[:rlen] / sc
            # ---- backwardKeyValue: K and V pre-multiplied, accumulators started at the stored L and D of a 32-row tile
            with np.errstate(all="ignore"):
                Pk = np.where(vis.T, _f32(np.exp2(-_chain32(np.repeat(L2[None, :], K.shape[0], axis=0), _f32(-s2c * K), Q))), 0.0)
                X = np.where(vis.T, _f32(Pk * _chain32(np.repeat(Dst[None, :], K.shape[0], axis=0), _f32(-sc * V), G)), 0.0)   # = -dS'
            dV, dK = np.zeros((K.shape[0], Dh)), np.zeros((K.shape[0], Dh))
            for j in range(rtiles):
                t = slice(j * F32_TILE, (j + 1) * F32_TILE)
                dV, dK = _accum32(dV, Pk[:, t], G[t]), _accum32(dK, X[:, t], Q[t])
            dV, dK = dV[:clen], -dK[:clen]
            if h % Gq == 0:
                sv, sk = dV, dK
            else:
                sv, sk = _f32(sv + dV), _f32(sk + dK)
            if h % Gq == Gq - 1:
                res["dV"][b, h // Gq, :clen], res["dK"][b, h // Gq, :clen] = sv, sk
    return res


# ------------------------------------------------------------------------------------------------------------------ needle inputs
def key_pool(clen, pieces=None):
    """the keys whose handling the kernels' geometry makes special, most important first: key 0, the last key, the first and last key
    of every piece, both sides of every 64-key tile edge, both sides of every 32-key step edge"""
    pool = [0, clen - 1]
    for name in ("fwd", "dq"):
        for pb, pe in (pieces or {}).get(name, ()):
            pool += [pb, min(pe, clen) - 1]
    pool += [t for e in range(TILE, clen, TILE) for t in (e - 1, e)]
    pool += [t for e in range(STEP, clen, TILE) for t in (e - 1, e)]
    seen, res = set(), []
    for t in pool:
        if 0 <= t < clen and t not in seen:
            seen.add(t)
            res.append(t)
    return res


def edge_rows(rlen, pieces=None):
    """{class: rows}: the first and the last row of every 32-row step, of every wave's 64 rows and of every 256-row block (a ragged
    last one ends at the last live row), and of every row piece of a split dK / dV launch"""
    res = {}
    for name, n in (("step", STEP), ("wave", WAVE_ROWS), ("block", BLOCK_ROWS)):
        res[name + "_first"] = list(range(0, rlen, n))
        res[name + "_last"] = [min(r + n, rlen) - 1 for r in range(0, rlen, n)]
    for pb, pe in (pieces or {}).get("dkv", ()):
        if min(pe, rlen) > pb:
            res.setdefault("piece_first", []).append(pb)
            res.setdefault("piece_last", []).append(min(pe, rlen) - 1)
    return res


PER_ROW, CAPACITY = 3, 12    # pool keys of an ordinary row; most needles a row may carry


def mask_key_pool(active, clen):
    """the keys a row block's mask makes special: the first and the last key of every run of active column blocks, both sides of
    every 128-key block edge inside a run"""
    pool = []
    for s, e in mask_runs(active):
        pool += [s * MASK_COLUMNS, min((e + 1) * MASK_COLUMNS, clen) - 1]
        pool += [t for c in range(s + 1, e + 1) for t in (c * MASK_COLUMNS - 1, c * MASK_COLUMNS)]
    return [t for t in pool if 0 <= t < clen and active[t // MASK_COLUMNS]]


def run_edge_traps(active, C):
    """[(run, side, key)]: the last key of the inactive block before every run, the first key of the inactive block behind it"""
    res = []
    for s, e in mask_runs(active):
        if s > 0:
            res.append(((s, e), "before", s * MASK_COLUMNS - 1))
        if (e + 1) * MASK_COLUMNS < C:
            res.append(((s, e), "behind", (e + 1) * MASK_COLUMNS))
    return res


def _unique(keys, clen):
    seen, res = set(), []
    for t in keys:
        if 0 <= t < clen and t not in seen:
            seen.add(t)
            res.append(t)
    return res


def needle_plan(R, C, rlen, clen, causal, pieces, salt, spike=False, bits=None):
    """-> [set of needle keys per row r < R], [sorted trap keys per row].  Every row: its first visible key (key 0 without a mask: so
    that no later needle fires the deferred rescale; a spike case keeps it for its spiked rows only), causal: its last visible key
    (the frontier) and the key before it, PER_ROW pool keys in rotation (`salt`: heads
    and batch entries differ); the last row of every 256-row block also key 64 (a tile skipped in one block only shows in that block).  Transposed property: every pool key, in the pool's order of importance, is handed to one row of each
    class of edge_rows() that sees it and still has room (CAPACITY needles).  The step and wave classes hold every pool key.  The block
    and piece classes have few rows (R = 513: three first rows of a block, two of a piece, 66 pool keys): each head and batch entry
    starts its walk of the pool 2 (CAPACITY - 2) keys further on, so a grid of several heads covers between them what one head's
    rows cannot hold (tests/test_train_sensitivity.py asserts the counts).
    bits (bool [row blocks, column blocks], the mask of this grid entry): a row draws from the keys it SEES; its pool is its row
    block's mask_key_pool() and then the keys of key_pool() that lie in active blocks.  The first and the last row of every 256-row
    block hold a needle in a column block that is active for their row block and inactive for the adjacent one.
    Traps (keys the row leaves unsuppressed though it must not see them: a row that reads one is taken over): the key after the
    frontier (causal), else the key AT the key length (padding); under a mask also one key of run_edge_traps(), in rotation over
    the rows and with the salt (up to three where the row block has fewer rows than its runs have edges), and, for the first and last row of a 256-row block, a key in a column block that is INACTIVE for its
    row block and active for the adjacent one."""
    off = max(clen - rlen, 0)
    pool = key_pool(clen, pieces)
    rows = [set() for _ in range(R)]
    traps = [set() for _ in range(R)]
    front = [min(r + off, clen - 1) if causal else clen - 1 for r in range(R)]
    classes = edge_rows(min(rlen, R), pieces)
    edges = {r for members in classes.values() for r in members}
    nb = None if bits is None else np.asarray(bits, dtype=bool)
    nrb = -(-R // BLOCK_ROWS)
    if nb is None:
        sees = lambda r, t: 0 <= t <= front[r]                                                     # noqa: E731
        pools = [pool] * nrb
        first, last = [0] * R, front
    else:
        sees = lambda r, t: 0 <= t <= front[r] and bool(nb[r // BLOCK_ROWS, t // MASK_COLUMNS])    # noqa: E731
        pools = [_unique(mask_key_pool(nb[i], clen) + [t for t in pool if nb[i, t // MASK_COLUMNS]], clen) for i in range(nrb)]
        pool = _unique([t for i in range(nrb) for t in mask_key_pool(nb[i], clen)] + pool, clen)
        first, last = [None] * R, [None] * R
        for r in range(R):
            seen = [c for c in np.flatnonzero(nb[r // BLOCK_ROWS]) if c * MASK_COLUMNS <= front[r]]
            if seen:
                first[r], last[r] = seen[0] * MASK_COLUMNS, min((seen[-1] + 1) * MASK_COLUMNS - 1, front[r])
    for r in range(R):
        if first[r] is None:
            continue                                       # a dead row: no needle, its traps only
        if not spike:
            rows[r].add(first[r])
        if causal:
            rows[r] |= {last[r]} | ({last[r] - 1} if sees(r, last[r] - 1) else set())
        own = pools[r // BLOCK_ROWS]
        for i in range(0 if r in edges or not own else PER_ROW):      # (an edge row's room goes to the keys its classes hand it)
            t = own[(r * PER_ROW + i + salt * 5) % len(own)]
            if sees(r, t):
                rows[r].add(t)
    for r in classes["block_last"]:                        # a ragged last block may be ONE row: every block sees keys 64..127 dropped
        if sees(r, TILE):
            rows[r].add(TILE)
    if nb is not None:
        for r in range(min(rlen, R)):
            i = r // BLOCK_ROWS
            hidden = [t for _run, _side, t in run_edge_traps(nb[i], C) if t <= front[r] and t < clen]
            few = min(3, -(-len(hidden) // (min((i + 1) * BLOCK_ROWS, rlen, R) - i * BLOCK_ROWS)))    # (a one-row block: up to three a row)
            for n in range(few):
                traps[r].add(hidden[((r + salt) * few + n) % len(hidden)])
        inside = lambda r, c: min(c * MASK_COLUMNS + (salt * 37 + 5) % MASK_COLUMNS, front[r], clen - 1)    # noqa: E731
        for side, step in (("block_first", -1), ("block_last", 1)):
            for r in classes[side]:
                i, j = r // BLOCK_ROWS, r // BLOCK_ROWS + step
                if not 0 <= j < nrb or j * BLOCK_ROWS >= rlen:
                    continue
                reach = [c for c in range(nb.shape[1]) if c * MASK_COLUMNS <= min(front[r], clen - 1)]
                mine = [c for c in reach if nb[i, c] and not nb[j, c]]
                theirs = [c for c in reach if nb[j, c] and not nb[i, c]]
                if mine and first[r] is not None:
                    rows[r].add(inside(r, mine[salt % len(mine)]))
                if theirs:
                    traps[r].add(inside(r, theirs[salt % len(theirs)]))
        # the first and the last key of every run go to rows of their own row block before anything else takes the room: a ragged
        # last row block may be ONE row of CAPACITY needles, so each head and batch entry starts three run edges further on
        for i in range(nrb):
            members = list(range(i * BLOCK_ROWS, min((i + 1) * BLOCK_ROWS, rlen, R)))
            ends = _unique([t for s, e in mask_runs(nb[i]) for t in (s * MASK_COLUMNS, min((e + 1) * MASK_COLUMNS, clen) - 1)], clen)
            at = (salt * 3) % len(ends) if ends else 0
            for n, t in enumerate(ends[at:] + ends[:at] if members else ()):
                seers = [r for r in members if sees(r, t)]
                for j in range(min(len(seers), 8)):
                    r = seers[(n * 37 + salt + j) % len(seers)]
                    if t in rows[r]:
                        break
                    if len(rows[r]) < CAPACITY:
                        rows[r].add(t)
                        break
    for kind in ("piece", "block", "wave", "step"):        # (a piece's edge rows are mostly block edge rows too: what they hold counts twice)
        start = (salt * 2 * (CAPACITY - 2)) % len(pool) if kind in ("piece", "block") else 0
        for side in ("_first", "_last"):
            members = classes.get(kind + side, [])
            for i, t in enumerate(pool[start:] + pool[:start] if members else ()):
                for j in range(len(members)):
                    r = members[(i + salt + j) % len(members)]
                    if t in rows[r]:
                        break
                    if sees(r, t) and len(rows[r]) < CAPACITY:
                        rows[r].add(t)
                        break
    for r in range(R):
        for t in (last[r], None if last[r] is None else last[r] - 1, first[r]):   # never a one-needle row where there is a second key: dS would vanish
            if len(rows[r]) < 2 and t is not None and sees(r, t):
                rows[r].add(t)
        f = front[r] + 1 if causal else clen
        if f < C:
            traps[r].add(f)
    return rows, [sorted(t) for t in traps]


def code_layout(C, Dh, h=0):
    """(mA, mB, dims): key j carries the code (j % mA, (j // mA) % mB) as a 1 on dimension dims[j % mA] and a 1 on dimension
    dims[mA + (j // mA) % mB]; mA mB >= C where D has room for mA + mB dimensions (else codes repeat every mA mB keys); `dims`
    spreads the code over all 32-wide d blocks and differs between heads.  The other D - mA - mB dimensions are free."""
    mA = int(math.ceil(math.sqrt(C)))
    mB = -(-C // mA)
    if mA + mB > Dh:
        mA = Dh // 2
        mB = Dh - mA
    stride = next(s for s in (7, 11, 13, 1) if math.gcd(s, Dh) == 1)
    return mA, mB, (np.arange(Dh) * stride + 5 * h) % Dh


SUPPRESSED = 9.0    # nats below the needles: the score of a key that shares one code half with no needle of the row (18: neither half)


def spike_keys(spike, r, salt, last, clen):
    """[(key, nats above the row's other keys)] of row r whose last visible key is `last`, or [] (the row is not spiked).  True: the
    single late key of the 16-bit cases (row 40 of every 64: its last visible key).  The family for 32-key tiles (SPIKES), every
    spike behind tile 0; rows 3 mod 4 stay unspiked ("f": every other row), so that spiked and unspiked lanes share every wave:
      a  one key 9 nats up in a whole tile 1 .., at residue (5 r + salt) mod 32: 32 consecutive rows walk every residue, both
         half-waves (crow) and, with the tile index (r / 2 + salt), both LDS stages
      b  the tile's parity follows the row's: odd rows in odd tiles, even rows in even tiles
      c  a key of the partial last tile (rows that see it)
      d  a key of the row's diagonal tile: its last visible key or one of the two before it
      e  a staircase: three (even rows) or four (odd rows) successive tiles, 9, 15, 21, 27 nats: each tops the one before by 6 nats
         (8.66 log2 units), so the branch fires tile after tile and the bias is rewritten each time
      f  as a, every other row"""
    if not spike:
        return []
    if spike is True:
        return [(last, SUPPRESSED)] if r % TILE == 40 else []
    assert spike in SPIKES, spike
    if r % 2 == 0 if spike == "f" else r % 4 == 3:
        return []
    full, at = (last + 1) // F32_TILE, (5 * r + salt) % F32_TILE           # whole tiles the row sees
    if spike in ("a", "f"):
        return [((1 + (r // 2 + salt) % (full - 1)) * F32_TILE + at, SUPPRESSED)] if full >= 2 else []
    if spike == "b":
        if full < 3:
            return []
        tile = 1 + 2 * ((r // 2 + salt) % (full // 2)) if r % 2 else 2 + 2 * ((r // 2 + salt) % ((full - 1) // 2))
        return [(tile * F32_TILE + at, SUPPRESSED)]
    if spike == "c":
        t0 = clen // F32_TILE * F32_TILE
        return [(t0 + (r + salt) % (last - t0 + 1), SUPPRESSED)] if clen % F32_TILE and t0 and last >= t0 else []
    if spike == "d":
        return [(last - (r + salt) % 3, SUPPRESSED)] if last - 2 >= F32_TILE else []
    n = 3 + r % 2
    if full < n + 1:
        return []
    first = 1 + (r // 4 + salt) % (full - n)
    return [((first + i) * F32_TILE + at, SUPPRESSED + 6.0 * i) for i in range(n)]


def shift_of(shift, r):
    """the per-row score shift of needle_inputs(shift=) in nats: 32 consecutive rows walk +-shift in 32 steps"""
    return shift * ((7 * r) % 32 / 15.5 - 1.0)


def needle_inputs(B, H, R, C, Dh, fmt, *, causal=False, row_lengths=None, key_lengths=None, pieces=None, block_mask=None, spike=False, seed=0,
                  dO_fmt=None, small_dO_rows=None, heads_per_kv=1, shift=None):
    """-> q, k, v, dO (float64 values of the 16-bit type, asserted exact) and info {(b, h, r): (needle keys, trap keys)}.

    The tension: in the mixed mode a score moves by u T_ij, T_ij = scale sum_d |q_d k_jd| >= |s_ij|, so a needle that stands
    ln(keys) + c ABOVE a background at 0 carries a relative error of u (ln(keys) + c) -- 3 % at 257 keys in bf16, which would hide
    every defect below that.  Softmax is shift invariant and T is not: here the needles score about 0 and the background is pushed
    DOWN.  Key j carries a two-part one-hot code (code_layout) and U(-1, 1) on the free dimensions; V, dO ~ U(-1, 1), dense.  Row r
    with needles T: q = -SUPPRESSED sqrt(D) on every code dimension that no key of T uses, +-sqrt(D) / 8 or / 16 on those T uses and on two
    free dimensions (few-hot: a score spread of +-0.5 at T_ij <= 0.5).  A key scores 0 +- 0.5 where both halves of its code are used by T --
    T itself and at most |T|^2 - |T| further keys, needles by the same right -- and -9 or -18 otherwise: the needles have T_ij < 1,
    the background's large T_ij multiplies weights of e^-9.  The trap keys (needle_plan) are a few more keys the row does not
    suppress: a row that reads one gains a needle.  Where codes repeat (C > mA mB) key j and key j + mA mB score alike: the alias of a
    needle in a block the row's mask hides is a trap by itself, the alias of a trap in a visible block a needle; the model stays the truth.  dP_ij - D_i = dO_i . (v_j - O_i) is of the order of |dO| sqrt(D) / 3 on every needle.
    spike: row 40 of every 64 keeps key 0 and its last visible key t* only and adds +9 sqrt(D) on the second
    code dimension of t*: t* scores +9, the keys of its code run (its neighbours, all late) 0: the late dominant key that fires the
    deferred rescale.  Rows at and past the row length are built like live rows (a kernel that reads them moves dK / dV).
    dO_fmt (default fmt): the type dO is built in and must survive the cast to ("bf16" beside fmt = "f16": the reference's mix); in the
    mix no dO element lies below 2^-14 in magnitude (FP16's smallest normal number) except in small_dO_rows (a slice of rows), whose dO
    is scaled by 2^-12 as a whole -- Q, K, V and with them every needle stay as they are.  heads_per_kv = G: K and V are [B, H / G, C,
    D], query head h reads head h // G and takes that head's code layout; the members of a group draw their needles with different
    salts, so their needle keys differ.
    fmt = "f32": FP32 values.  spike may name a member of SPIKES (spike_keys): a spiked row keeps one key of tile 0 -- the key whose
    first code half is the first spike's own, so that no other key of the spike's code run is lifted -- and its spike keys only.
    shift (nats; FP32 only): the last free dimension is taken out of the draw and carries a per-row constant a_i in Q and b = 1 in
    K: every score of row i moves by shift_of(shift, i) -- +-shift inside every 32-row wave --, which softmax cancels exactly
    (shift = 0.0: the same inputs with a_i = 0, the comparison case; dO is drawn along the unshifted O either way)."""
    rng = np.random.default_rng(seed)
    assert shift is None or (fmt == "f32" and block_mask is None)
    Gq = int(heads_per_kv)
    dO_fmt = dO_fmt or fmt
    k = round_to(rng.uniform(-1, 1, (B, H // Gq, C, Dh)), fmt)
    v = round_to(rng.uniform(-1, 1, (B, H // Gq, C, Dh)), fmt)
    dO = round_to(rng.uniform(-1, 1, (B, H, R, Dh)), fmt)
    q = np.zeros((B, H, R, Dh))
    rl, cl = _lengths(row_lengths, B, R), _lengths(key_lengths, B, C)
    info = {}
    gamma = float(round_to(np.array([SUPPRESSED * math.sqrt(Dh)]), fmt)[0])
    keys = np.arange(C)
    for h in range(H):
        mA, mB, dims = code_layout(C, Dh, h // Gq)
        free = dims[mA + mB:]
        if shift is not None:
            assert len(free) >= 3, "the shift needs a spare head dimension"
            free, spare = free[:-1], free[-1]
        ka, kb = keys % mA, (keys // mA) % mB
        for b in range(B):
            k[b, h // Gq][:, dims[:mA + mB]] = 0.0
            k[b, h // Gq, keys, dims[ka]] = 1.0
            k[b, h // Gq, keys, dims[mA + kb]] = 1.0
            if shift is not None:
                k[b, h // Gq, :, spare] = 1.0
            assert block_mask is None or not spike
            rows, traps = needle_plan(R, C, int(rl[b]), int(cl[b]), causal, pieces, b * H + h, bool(spike),
                                      None if block_mask is None else mask_bits(block_mask, b, h))
            off = max(int(cl[b]) - int(rl[b]), 0)
            for r in range(R):
                T = set(rows[r])
                last = min(r + off, int(cl[b]) - 1) if causal else int(cl[b]) - 1
                spikes = [(t, nats) for t, nats in spike_keys(spike, r, b * H + h, last, int(cl[b])) if t >= mA]
                if len({int(kb[t]) for t, _n in spikes}) < len(spikes):       # (two spikes in one code run: C > 1024)
                    spikes = []
                spiked = bool(spikes)
                if spiked:
                    T = {0 if spike is True else spikes[0][0] % mA} | {t for t, _n in spikes}
                U = sorted(T | set(traps[r]))
                row = np.zeros(Dh)
                row[dims[:mA + mB]] = -gamma
                lifted = np.unique(np.concatenate([dims[ka[U]], dims[mA + kb[U]]]))
                row[lifted] = rng.choice([-1.0, -0.5, 0.5, 1.0], len(lifted)) * 0.125 * math.sqrt(Dh)     # few-hot: +-0.125 per code half
                for t, nats in spikes:
                    row[dims[mA + kb[t]]] = gamma if nats == SUPPRESSED else float(round_to(np.array([nats * math.sqrt(Dh)]), fmt)[0])
                if len(free):                      # and two free dimensions: T_ij = scale sum_d |q_d k_jd| <= 0.5 on a needle
                    row[free[(r * 2 + np.arange(2)) % len(free)]] = rng.choice([-1.0, 1.0], 2) * 0.125 * math.sqrt(Dh)
                q[b, h, r] = row
                info[(b, h, r)] = (sorted(T), tuple(traps[r]))
    q = round_to(q, fmt)
    for b in range(B):          # dO = U(-1, 1) + 8 / D units along the row's O: D_i = dO_i . O_i is then about 1.4 + noise in every row
        for h in range(H):
            vis = mask_views(block_mask, b, h, R, C, int(rl[b]), int(cl[b]), causal)[0]
            P, _m, _l = _softmax((q[b, h] @ k[b, h // Gq].T) / math.sqrt(Dh), vis)
            O = P @ v[b, h // Gq]
            rms = np.sqrt((O * O).mean(axis=1, keepdims=True))
            dO[b, h] = round_to(dO[b, h] + (8.0 / Dh) * O / np.where(rms > 0, rms, 1.0), dO_fmt)
    if shift:
        for h in range(H):
            spare = code_layout(C, Dh, h // Gq)[2][-1]
            q[:, h, :, spare] = round_to(shift_of(shift, np.arange(R)) * math.sqrt(Dh), fmt)[None, :]
    if dO_fmt != fmt:
        dO = np.where(np.abs(dO) < SMALL_DO, np.where(dO < 0, -SMALL_DO, SMALL_DO), dO)
    if small_dO_rows is not None:
        dO[:, :, small_dO_rows] *= 2.0 ** -12
    for x, f in ((q, fmt), (k, fmt), (v, fmt), (dO, dO_fmt)):
        assert np.array_equal(round_to(x, f), x) and np.isfinite(x).all(), "the inputs must survive the cast to the 16-bit type"
    return q, k, v, dO, info


def needle_keys(info):
    """{(b, h): {key: [rows that hold it as a needle]}}"""
    res = {}
    for (b, h, r), (needles, _traps) in info.items():
        for t in needles:
            res.setdefault((b, h), {}).setdefault(t, []).append(r)
    return res


def rebase_proof(q, k, v, dO, *, causal=False, row_lengths=None, key_lengths=None, heads_per_kv=1):
    """what the FP32 forward's re-base branch does on these inputs, from emulated()'s walk and with nothing launched: the kernel's
    rule (j > 0 and the tile's maximum relative to m above 8 log2 units) applied to the walk's per-tile maxima ->
    dict(mixed: (wave, tile) pairs in which some but not all live rows of a 32-row wave take the branch, residues: the positions mod 32
    of the keys that fired it, parities: the tile indices mod 2, last_tile: fires in a row's last visible tile, longest: the longest run of
    successive firing tiles of one row, rows: rows that fire at all, far_first: the largest |m| tile 0 sets, in log2 units)"""
    trace = {}
    emulated(q, k, v, dO, "f32", False, causal=causal, row_lengths=row_lengths, key_lengths=key_lengths, heads_per_kv=heads_per_kv,
             trace=trace, forward_only=True)
    res = dict(mixed=0, residues=set(), parities=set(), last_tile=0, longest=0, rows=0, far_first=0.0)
    for rec in trace.values():
        fired = rec["mx"] > F32_THRESHOLD
        fired[:, 0] = False
        assert np.array_equal(fired, rec["fired"])
        for w in range(0, fired.shape[0], 32):
            res["mixed"] += int((fired[w:w + 32].any(axis=0) & ~fired[w:w + 32].all(axis=0)).sum())
        res["residues"] |= {int(x) for x in rec["at"][fired]}
        res["parities"] |= {int(j) % 2 for j in np.nonzero(fired)[1]}
        seen = np.isfinite(rec["mx"])                                  # tiles in which the row sees a key
        res["last_tile"] += int((fired & seen & ~np.concatenate([seen[:, 1:], np.zeros((len(seen), 1), dtype=bool)], axis=1)).sum())
        run = np.zeros(fired.shape[0], dtype=int)
        for j in range(fired.shape[1]):
            run = np.where(fired[:, j], run + 1, 0)
            res["longest"] = max(res["longest"], int(run.max(initial=0)))
        res["rows"] += int(fired.any(axis=1).sum())
        res["far_first"] = max(res["far_first"], float(np.abs(rec["before"][:, 1]).max()) if fired.shape[1] > 1 else 0.0)
    return res


def check_rebase_proof(proof, spike, shift=None, C=None, whole=True):
    """what a spike (and shift) case of the FP32 forward must show before anything is launched: the branch fires behind tile 0 in some
    but not all rows of a wave, in tiles of both parities (both LDS stages); the keys that fire it take every residue mod 32 -- "c":
    every position of the partial last tile of C keys (whole: no per-batch length shortens it), and the fire is in the row's last
    tile; "d": also in the last visible tile; "e": some row fires in three successive tiles or more; shift: tile 0 sets an m as far
    from 0 as the shift reaches (0.9 shift log2e)"""
    assert spike in SPIKES and proof["mixed"] >= 1 and proof["parities"] == {0, 1}, (spike, proof)
    want = set(range(C % F32_TILE)) if spike == "c" and whole else set() if spike == "c" else set(range(F32_TILE))
    assert want <= proof["residues"], (spike, sorted(want - proof["residues"]))
    assert proof["last_tile"] >= 1 or spike not in ("c", "d"), (spike, proof)
    assert proof["longest"] >= 3 or spike != "e", (spike, proof)
    assert not shift or proof["far_first"] >= 0.9 * shift * LOG2E, (shift, proof)


# ----------------------------------------------------------------------------------------------------------------------- checker
def compare(got, ref, *, out="f32", margin=None, info=None, outputs=OUTPUTS, fmt=None):
    """got {output: array, NaN (the buffer's sentinel) where the launch wrote nothing} against the model -> ({output: worst err /
    bound over EVERY element of every live row or key}, {output: True where the padding kept the sentinel}, text naming the worst
    elements).  fmt: as in bounds()."""
    bd = bounds(ref, out, margin, fmt)
    worst, padding, lines = {}, {}, []
    for name in outputs:
        g = f64(got[name])
        want = getattr(ref, name)
        live = ref.key_live if name in ("dV", "dK") else ref.row_live      # [B, n]
        mask = np.broadcast_to(live[:, None, :] if g.ndim == 3 else live[:, None, :, None], g.shape)
        with np.errstate(invalid="ignore"):
            ratio = np.abs(g - want) / bd[name]
        ratio = np.where(mask, np.where(np.isnan(ratio), np.inf, ratio), 0.0)
        if ref.dead is not None and name in ("O", "L", "D", "dQ"):      # a dead row: exactly 0; its L only hugely negative (mfa.h)
            dead = ref.dead if g.ndim == 3 else np.broadcast_to(ref.dead[..., None], g.shape)
            with np.errstate(invalid="ignore"):
                wrong = ~(g < -1e30) if name == "L" else g != 0.0
            ratio = np.where(dead, np.where(wrong, np.inf, 0.0), ratio)
        at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        worst[name] = float(ratio[at])
        padding[name] = bool(np.isnan(g[~mask]).all())
        text = "%s worst at %s: got %.6g, model %.6g, |d| / bound = %.3g" % (name, tuple(int(x) for x in at), g[at], want[at], worst[name])
        if info is not None and name in ("O", "L", "D", "dQ") and tuple(int(x) for x in at[:3]) in info:
            needles, traps = info[tuple(int(x) for x in at[:3])]
            text += " (the row's needles: keys %s%s)" % (needles, "; trap keys %s" % list(traps) if traps else "")
        if not padding[name]:
            text += "; PADDING WRITTEN"
        lines.append(text)
    return worst, padding, "\n".join(lines)
