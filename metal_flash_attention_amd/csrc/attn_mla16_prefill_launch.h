// attn_mla16_prefill_launch.h -- what the two translation units of MLA prefill share on the host: attn_mla16_prefill.hip (the unsplit
// launch, include/mfa_mla_prefill.h) checks a parameter block and fills the kernels' argument block; attn_mla16_prefill_split.hip
// (the launch cut along the keys, include/mfa_mla_prefill_split.h) refuses what that refuses in its words and cuts the same block.
#pragma once
#include "../../include/mfa_mla_prefill.h"
#include "attn_mla16_prefill.h"

namespace mfa {
// every check of the unsplit launch that needs no GPU; on MFA_OK *args is its argument block (buffer pointers null, no pieces)
mfa_status mla_prefill_prepare_args(const mfa_mla_prefill_params *p, MlaPrefillArgs *args);
} // namespace mfa
