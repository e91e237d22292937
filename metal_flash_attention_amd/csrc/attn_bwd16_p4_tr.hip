// attn_bwd16_p4_tr.hip -- launchers of the backward kernels that read transposed operands in place (attn_dq16_p4_tr.h: K^T / V^T;
// attn_dkv16_p4_tr.h: Q^T / dO^T).  prepare_launch (mfa_kernel.hip) routes a transposed backward launch that carries no workspace
// here when bwd16_p4_tr_launch takes it (with a workspace, the re-layout path runs: the caller chose it); MFA_BWD16_TR=0 is the
// developer library's A/B knob; nullptr = the launch is not one these kernels take (the general kernel serves it).
#include "attn_dq16_p4_tr.h"
#include "attn_dkv16_p4_tr.h"
#include "launchers.h"

namespace mfa {

static bool rows_aligned(const OperandView &v) {
  return ((reinterpret_cast<uintptr_t>(v.ptr) | (uint64_t)v.ld * 2 | (uint64_t)v.headStride * 2 | (uint64_t)v.batchStride * 2) & 15) == 0;
}

// l.grid = (blocks of the parallelization dimension, heads, batches); the kernels' own blocks are 256 rows / keys
template <typename T, int STREAM, typename TG = T> static void launch_dq_tr(const Launch &l) {
  const uint32_t blocks = (l.args.R + 255) / 256;
  Fwd16Grid g{blocks, l.grid.y, l.grid.z};
  const dim3 flat(blocks * l.grid.y * l.grid.z);
  if (l.args.causal) l.start(&attn_dq16_p4_tr<T, STREAM, true, TG>, flat, dim3(256), dq4::LDS_BYTES, l.args, g);
  else l.start(&attn_dq16_p4_tr<T, STREAM, false, TG>, flat, dim3(256), dq4::LDS_BYTES, l.args, g);
}

template <typename T, int STREAM> static void launch_dkv_tr(const Launch &l) {
  const uint32_t blocks = (l.args.C + 255) / 256;
  Fwd16Grid g{blocks, l.grid.y, l.grid.z};
  const dim3 flat(blocks * l.grid.y * l.grid.z);
  if (l.args.causal) l.start(&attn_dkv16_p4_tr<T, STREAM, true>, flat, dim3(256), dkv4::LDS_BYTES, l.args, g);
  else l.start(&attn_dkv16_p4_tr<T, STREAM, false>, flat, dim3(256), dkv4::LDS_BYTES, l.args, g);
}

// what the in-place kernels take (their headers): 16-bit operands of one type (dO may be BF16 next to FP16), 64 < D <= 128, no
// per-batch lengths, no block mask; backwardQuery: K^T and V^T in whole 64-key tiles of aligned rows; backwardKeyValue: Q^T and dO^T
// in whole 32-row steps of aligned rows, L / D stored as the reference stores them (FP16 + BF16, or both FP32)
static bool takes(int type, const KernelArgs &a) {
  const int p = a.op[SLOT_Q].precision, pg = a.op[SLOT_dO].precision;
  const bool gmix = p == PREC_FP16 && pg == PREC_BF16;
  if (p == PREC_FP32 || a.op[SLOT_K].precision != p || a.op[SLOT_V].precision != p || (pg != p && !gmix)) return false;
  if (a.rowLen || a.colLen || a.mask || a.D <= 64 || a.D > 128 || a.D % 8) return false;
  // grouped-query launches: these kernels address K / V by the query head (the divisor in their prologue kept hipcc's register
  // allocator from finishing this unit)
  if (a.kvHeadMul || a.kvHeadShift) return false;
  if (a.causal && a.C < a.R) return false;
  if (type == 1) {
    if (!a.op[SLOT_K].transposed || !a.op[SLOT_V].transposed || a.C % 64 != 0) return false;
    return rows_aligned(a.op[SLOT_K]) && rows_aligned(a.op[SLOT_V]);
  }
  if (!a.op[SLOT_Q].transposed || !a.op[SLOT_dO].transposed || a.R % 32 != 0) return false;
  if (!rows_aligned(a.op[SLOT_Q]) || !rows_aligned(a.op[SLOT_dO])) return false;
  const int lp = a.op[SLOT_L].precision, dp = a.op[SLOT_D].precision;
  return (lp == PREC_FP16 && dp == PREC_BF16) || (lp == PREC_FP32 && dp == PREC_FP32);
}

// type: 1 = backwardQuery, 2 = backwardKeyValue (mfa_kernel_type); fold: the descriptor keeps the attention matrix in 16-bit registers
const char *bwd16_p4_tr_launch(int type, bool fold, const Launch &l) {
  const KernelArgs &a = l.args;
  if (!takes(type, a)) return nullptr;
  const int p = a.op[SLOT_Q].precision;
  const bool gmix = p == PREC_FP16 && a.op[SLOT_dO].precision == PREC_BF16;   // the reference's own mix: FP16 Q, K, V with BF16 dO (+Precisions.swift:13-17)
  if (type == 1) {
    if (p == PREC_BF16) fold ? launch_dq_tr<__bf16, dq4tr::S_BF16_FOLD_TR>(l) : launch_dq_tr<__bf16, dq4tr::S_BF16_EXACT_TR>(l);
    else if (gmix) fold ? launch_dq_tr<_Float16, dq4tr::S_F16_FOLD_TR, __bf16>(l) : launch_dq_tr<_Float16, dq4tr::S_F16_EXACT_TR, __bf16>(l);
    else fold ? launch_dq_tr<_Float16, dq4tr::S_F16_FOLD_TR>(l) : launch_dq_tr<_Float16, dq4tr::S_F16_EXACT_TR>(l);
    return "attn_dq16_p4_tr (four waves x 64 rows, hand-placed stream on transposed K / V in place, no workspace)";
  }
  const bool mixed = a.op[SLOT_L].precision == PREC_FP16;
  if (p == PREC_BF16) mixed ? launch_dkv_tr<__bf16, dkv4tr::S_BF16_MIXED_TR>(l) : launch_dkv_tr<__bf16, dkv4tr::S_BF16_F32_TR>(l);
  else if (gmix) mixed ? launch_dkv_tr<_Float16, dkv4tr::S_F16_DOBF16_MIXED_TR>(l) : launch_dkv_tr<_Float16, dkv4tr::S_F16_DOBF16_F32_TR>(l);
  else mixed ? launch_dkv_tr<_Float16, dkv4tr::S_F16_MIXED_TR>(l) : launch_dkv_tr<_Float16, dkv4tr::S_F16_F32_TR>(l);
  return "attn_dkv16_p4_tr (four waves x 64 keys, hand-placed stream on transposed Q / dO in place, no workspace)";
}

} // namespace mfa
