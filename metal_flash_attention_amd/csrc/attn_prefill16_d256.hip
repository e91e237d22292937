// attn_prefill16_d256.hip -- the prefill kernels of head dimension 256 (attn_prefill16.h): a translation unit of their
// own, so that the two units compile side by side; attn_prefill16.hip's table selects them like the others.
// (Not named attn_fwd16*: the Makefile gives those -ffinite-math-only, and this unit's inputs may hold NaN past a length.)
#include <hip/hip_runtime.h>

#include "attn_prefill16.h"

MFA_PREFILL_KERNELS(MFA_PREFILL_DEFINE, bf16, __bf16, 256)
MFA_PREFILL_KERNELS(MFA_PREFILL_DEFINE, f16, _Float16, 256)
MFA_PREFILL_COMBINE_DEFINE(bf16, __bf16, 256)
MFA_PREFILL_COMBINE_DEFINE(f16, _Float16, 256)
