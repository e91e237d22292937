// attn_decode_plan.h -- the host plan of a decode launch, shared by the 16-bit launch (attn_decode16.hip, which owns it) and the
// launch over an FP8 cache (attn_decode8.hip): one set of checks, one piece count, one workspace formula, one combine kernel.
#pragma once
#include "../../include/mfa_decode.h"
#include "attn_decode16.h"

namespace mfa {

struct DecodeHostPlan {
  DecodeArgs args;                       // buffer pointers not yet bound
  uint32_t pieces, planned, blocks;      // as the launch runs (1 without a workspace); what the host would cut; batches x K/V heads
  uint32_t lds;                          // dynamic LDS of the main kernel
  void (*combine)(const DecodeArgs);     // attn_decode16_d<D>_<type>_combine
  const char *combineName;
};

// every check of mfa_attention_decode_launch that needs no GPU, for `params` as they stand
mfa_status decode_host_plan(const mfa_decode_params *params, DecodeHostPlan *out);
// bytes of the workspace of `pieces` pieces
uint64_t decode_workspace_bytes(uint32_t pieces, const mfa_decode_params *params);

} // namespace mfa
