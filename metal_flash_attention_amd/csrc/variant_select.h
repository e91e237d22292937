// variant_select.h -- which pre-compiled code object serves an attention kernel descriptor (variant_select.cpp; host only).
#pragma once
#include "launchers.h"
#include "mfa_internal.h"

namespace mfa {

// operand of a buffer slot
inline int slot_operand(int slot) {
  static const int ops[MFA_BUFFER_SLOTS] = {MFA_Q, MFA_K, MFA_V, MFA_O, MFA_L, MFA_D, MFA_dO, MFA_dV, MFA_dK, MFA_dQ};
  return ops[slot];
}

// operands each kernel type touches (+Source.swift:72-103)
inline bool slot_used(int type, int slot) {
  switch (type) {
    case MFA_FORWARD: return slot <= 4;
    case MFA_BACKWARD_QUERY: return slot <= 6 || slot == 9;
    default: return slot <= 2 || (slot >= 4 && slot <= 8);
  }
}

// matrix operands with one row per query row (`row` long); K, V, dK, dV are `column` long (AttentionKernel.swift:157-187)
inline bool row_operand(int op) { return op == MFA_Q || op == MFA_O || op == MFA_dO || op == MFA_dQ; }

struct Selection {
  VariantInfo variant;                          // preferred code object
  VariantInfo general;                          // general code object of the head-dimension bucket
  bool fast = false;                            // `variant` is a matrix-core code object and `general` its fallback
  bool relayout = false;                        // transposed operands: `variant` runs on row-major copies in the caller's workspace
  mfa_attention_kernel_descriptor effective;    // what `variant` really does
};

// `kd` has passed the descriptor checks of mfa_attention_kernel_create.  An error is recorded through fail()
mfa_status select_variant(const mfa_attention_kernel_descriptor &kd, Selection *out);

} // namespace mfa
