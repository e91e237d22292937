// variant_select.cpp -- which pre-compiled code object serves an attention kernel descriptor (host only: no kernel is defined here).
//
// Replaces, for gfx950, the reference's AttentionKernel(descriptor:) + createSource() (Sources/FlashAttention/Attention/
// AttentionKernel/AttentionKernel.swift:27-50; AttentionKernel+Source.swift:11-55): instead of emitting shader source for a JIT, the
// descriptor selects one of the code objects.  Candidates: every compiled code object that can serve the descriptor.  The general
// (fp32-arithmetic) kernel of the head-dimension bucket always can; the matrix-core kernels need Q, K, V (and dO) in ONE 16-bit
// type, outputs in FP32 or the inputs' type, and a head dimension that is a multiple of 8 (16-byte chunks).
#include "variant_select.h"

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace mfa {
namespace {

typedef mfa_attention_kernel_descriptor Desc;
typedef std::vector<VariantInfo> Candidates;

// head-dimension buckets of the 16-bit matrix-core code objects of a kernel type (the forward has a D = 32 object, the backward pair
// starts at 64 and runs smaller heads zero-padded; 320 / 384: the head blocks of 256 < D <= 384); 0 = none (D > 384: fp32 arithmetic)
int bucket16(int D, int type) {
  static const int buckets[] = {32, 64, 96, 128, 160, 192, 256, 320, 384};
  for (int b : buckets) {
    if (b == 32 && type != MFA_FORWARD) continue;
    if (b == 96 && type != MFA_BACKWARD_KEY_VALUE) continue;   // forward and dQ: the 128 objects are faster on D <= 96 than 96-wide ones
    if (D <= b) return b;
  }
  return 0;
}

int generic_bucket(int D) {
  static const int buckets[] = {32, 64, 128, 256, 384};
  for (int b : buckets)
    if (D <= b) return b;
  return -1;
}

// the general code object of the descriptor: the fp32-arithmetic kernel of the head-dimension bucket, or the any-D kernel
mfa_status general_variant(const Desc &kd, VariantInfo *general) {
  const int type = kd.type, D = kd.headDimension, bucket = generic_bucket(D);
  bool found = false;
  if (bucket > 0) {
    switch (type) {
      case MFA_FORWARD: found = generic_fwd_variant(bucket, general); break;
      case MFA_BACKWARD_QUERY: found = generic_dq_variant(bucket, general); break;
      default: found = generic_dkv_variant(bucket, general); break;
    }
  }
  if (!found) {
    // D > 384: the reference falls through to its tables' last row and pages the accumulators through the output buffers
    // (+Parameters.swift:60-65, +Accumulate.swift:403-469); so do the any-D kernels -- which therefore need those buffers in FP32,
    // as the reference always has them (+Precisions.swift:140-143)
    static const int outs[3][2] = {{MFA_O, MFA_O}, {MFA_dQ, MFA_dQ}, {MFA_dK, MFA_dV}};
    for (int i = 0; i < 2; ++i)
      if (kd.memoryPrecisions[outs[type][i]] != MFA_FP32)
        return fail(MFA_ERR_UNSUPPORTED, "head dimension " + std::to_string(D) + " > 384 pages the accumulators through the output buffer: " +
                                             mfa_operand_name(outs[type][i]) + " must be FP32 (lowPrecisionOutputs is not available there)");
    found = paged_variant(type, general);
  }
  if (!found) return fail(MFA_ERR_UNSUPPORTED, "no gfx950 code object for head dimension " + std::to_string(D));
  return MFA_OK;
}

// FP32 descriptors (every operand FP32, nothing transposed, D % 4 == 0) at the 64 / 128 head blocks ARE the FP32 production
// kernels of attn_f32.h: own variant name, own LDS bytes, same block dimensions as the general kernel that stays their sibling
bool f32_production(const Desc &kd) {
  bool allF32 = (kd.headDimension % 4) == 0;
  for (int slot = 0; slot < MFA_BUFFER_SLOTS && allF32; ++slot) {
    if (!slot_used(kd.type, slot)) continue;
    const int op = slot_operand(slot);
    allF32 = kd.memoryPrecisions[op] == MFA_FP32 && (op == MFA_L || op == MFA_D || kd.transposeState[op] == 0);
  }
  return allF32;
}

// what the matrix-core candidates are asked for
struct Request {
  const Desc &kd;
  int type, D, bucket;   // bucket16 of (D, type)
  int pq, pg;            // storage types of Q = K = V and of dO
  bool lowP;             // the attention matrix in 16-bit registers
};

// storage types and head dimension the matrix-core kernels of the kernel type take
bool matrix_core_operands(const Request &q) {
  const Desc &kd = q.kd;
  if (q.pq == MFA_FP32 || q.pq != kd.memoryPrecisions[MFA_K] || q.pq != kd.memoryPrecisions[MFA_V] || (q.D % 8) != 0) return false;
  auto f32_or_inputs = [&](int op) { return kd.memoryPrecisions[op] == MFA_FP32 || kd.memoryPrecisions[op] == q.pq; };
  switch (q.type) {
    case MFA_FORWARD: return f32_or_inputs(MFA_O);
    case MFA_BACKWARD_QUERY: return q.pg != MFA_FP32 && f32_or_inputs(MFA_O) && f32_or_inputs(MFA_dQ);
    default:
      return q.pg != MFA_FP32 && f32_or_inputs(MFA_dK) && f32_or_inputs(MFA_dV) && kd.memoryPrecisions[MFA_dK] == kd.memoryPrecisions[MFA_dV];
  }
}

// ---- candidate tables.  One row = one candidate of descriptors in `bucket`: the compiler-scheduled kernel of the kernel type's
// family at bucket `over` (BASE), or a hand-placed variant laid over that kernel: it arrives filled by it and overwrites the routes
// it serves, so the block-sparse, split ... launches it does not take keep their owner.  The order of the rows of a bucket is
// behaviour: the first candidate wins a tie on (distance, headBlock) and the strict error lists the candidates in order -- the
// product default first, i.e. a hand-placed variant in front of the kernel it is laid over.
enum Kernel { BASE, P4, P5, P6, W4 };
struct Row {
  int bucket;
  Kernel kernel;
  int over;
  bool (*when)(const Request &) = nullptr;   // nullptr: always
};

// the family of a kernel type: eight / four 32-row waves (attn_fwd16_v3.h), 32-row waves (attn_bwd16.h attn_dq16), role-split wave
// pairs (attn_dkv16_rs.h); head blocks 320 / 384: attn_fwd16_wide.h and the backward pair of attn_bwd16_wide.hip
bool base_variant(const Request &q, int bucket, VariantInfo *out) {
  switch (q.type) {
    case MFA_FORWARD: return bucket > 256 ? fwd16_wide_variant(q.pq, bucket, out) : fwd16_v3_variant(q.pq, bucket, 0, out);
    case MFA_BACKWARD_QUERY: return bucket > 256 ? dq16_wide_variant(q.pq, q.pg, bucket, out) : dq16_variant(q.pq, q.pg, bucket, out);
    default: return bucket > 256 ? dkv16_wide_variant(q.pq, q.pg, bucket, out) : dkv16_rs_variant(q.pq, q.pg, bucket, 0, out);
  }
}

// `c` arrives filled by base_variant(q, bucket).  A descriptor that holds the attention matrix in 16-bit registers (the reference's
// lowPrecisionIntermediates: P, and for FP16 also S, +Precisions.swift:149-215) selects the stream that pre-multiplies Q by the
// softmax scale in the 16-bit type; otherwise the scale is applied in fp32 per score
bool lay_over(const Request &q, Kernel kernel, int bucket, VariantInfo *c) {
  const int impl = q.lowP ? 10 : 0, lprec = q.kd.memoryPrecisions[MFA_L], dprec = q.kd.memoryPrecisions[MFA_D];   // (fixed per dK/dV stream)
  switch (q.type) {
    case MFA_FORWARD:
      if (kernel == P4) return fwd16_p4_variant(q.pq, bucket, impl, c);
      if (kernel == P5) return fwd16_p5_variant(q.pq, bucket, impl, c);
      return kernel == P6 && fwd16_p6_variant(q.pq, q.lowP, c);
    case MFA_BACKWARD_QUERY:
      if (kernel == P4) return dq16_p4_variant(q.pq, q.pg, bucket, impl, c);
      return kernel == P5 && dq16_p5_variant(q.pq, q.pg, bucket, impl, c);
    default:
      if (kernel == P4) return dkv16_p4_variant(q.pq, q.pg, lprec, dprec, bucket, 0, c);
      if (kernel == P5) return dkv16_p5_variant(q.pq, q.pg, lprec, dprec, bucket, c);
      return kernel == W4 && dkv16_variant(q.pq, q.pg, bucket, c);
  }
}

// the FOLD streams of attn_fwd16_p6.h from D = 16 on: with fewer terms per score the rounding of Q' = Q log2(e)/sqrt(D) to BF16 no
// longer averages out and L leaves the reference's 7e-3
bool p6_serves_d32(const Request &q) { return q.D >= 16 || !q.lowP; }

// P4 (bucket 128): four waves x 64 rows, hand-placed stream (attn_fwd16_p4.h); block-sparse launches keep the route of the 8 x 32 kernel.
// P6 (buckets 32 and 64 of the eight-wave kernel): four waves x 64 rows, persistent, 64-key steps (attn_fwd16_p6.h, round 5);
// mixed-precision descriptors get the streams with the row sums in the matrix pipe.  | 64 | 256 | 32 | 64 | selects the eight 32-row
// waves of attn_fwd16_v3.h, which also keep this kernel's block-sparse launches.  D <= 32: the same kernel on zero-padded chunks,
// selected by a | 32 | 256 | 64 | 64 | row; the launches it does not serve -- per-batch lengths, an L of the other storage type, pieces
// that are not whole multiples of four tiles -- go to the D = 64 eight-wave kernels, so it is laid over THEIR variant: 256-row blocks
// for split grids and choose_splits.
// P5 (buckets 160, 192, 256): four waves x 64 rows, 32-key steps (attn_fwd16_p5.h).
// 320, 384: the `| 384 | ... |` rows of the reference's mixed tables (AttentionDescriptor+Parameters.swift:113, :120) on the 16-bit
// matrix cores (attn_fwd16_wide.h, round 6; until then fp32 arithmetic on 16-bit storage, 1/16 of the rate)
const Row forwardRows[] = {
    {32, P6, 64, p6_serves_d32}, {32, BASE, 32},
    {64, P6, 64},       {64, BASE, 64},
    {128, P4, 128},     {128, BASE, 128},
    {160, P5, 160},     {160, BASE, 160},
    {192, P5, 192},     {192, BASE, 192},
    {256, P5, 256},     {256, BASE, 256},
    {320, BASE, 320},   {384, BASE, 384},
};

// P4 (buckets 64, 128): four waves x 64 rows, hand-placed stream (attn_dq16_p4.h).
// P5 (buckets 160, 192, 256): two wave pairs x 64 rows, hand-placed role-split stream (attn_dq16_p5.h), in front of the four 32-row
// waves of the same bucket (| D | 128 | 64 | D | selects those).
// 320, 384 (round 6): attn_bwd16_wide.hip; until then fp32 arithmetic on 16-bit storage, 1/16 of the rate.  Dense, causal, per-batch
// lengths; block masks keep the general kernel (the fallback)
const Row backwardQueryRows[] = {
    {64, P4, 64},     {64, BASE, 64},
    {128, P4, 128},   {128, BASE, 128},
    {160, P5, 160},   {160, BASE, 160},
    {192, P5, 192},   {192, BASE, 192},
    {256, P5, 256},   {256, BASE, 256},
    {320, BASE, 320}, {384, BASE, 384},
};

// P4 (buckets 64, 128): four waves x 64 keys, hand-placed stream (attn_dkv16_p4.h).
// P5 (buckets 160, 192, 256): two wave pairs x 64 keys, hand-placed role-split stream (attn_dkv16_p5.h), in front of the 32-key pairs
// of the same bucket (| D | 64 | 32 | D | selects those).
// 64 < D <= 96: the 128 bucket's stream is 1.4 x faster than the 96-wide role-split pairs (profiles/r02_bucket96_dkv.txt) and is what
// the default table row asks for; a | 96 | 128 | 32 | 96 | row selects these.
// W4, one wave per key block (attn_bwd16.h; D = 64, 128 only): laid over the role-split kernel, whose block-sparse and split routes it
// keeps -- at bucket 96 that is the 128 one, next to whose other candidates it stands.
// 320, 384 (round 6): attn_dkv16_wide.h, as for backwardQuery
const Row backwardKeyValueRows[] = {
    {64, P4, 64},     {64, BASE, 64},   {64, W4, 64},
    {96, BASE, 96},   {96, P4, 128},    {96, BASE, 128},  {96, W4, 128},
    {128, P4, 128},   {128, BASE, 128}, {128, W4, 128},
    {160, P5, 160},   {160, BASE, 160},
    {192, P5, 192},   {192, BASE, 192},
    {256, P5, 256},   {256, BASE, 256},
    {320, BASE, 320}, {384, BASE, 384},
};

template <size_t N>
void add_rows(const Request &q, const Row (&rows)[N], Candidates *out) {
  for (const Row &row : rows) {
    if (row.bucket != q.bucket || (row.when && !row.when(q))) continue;
    VariantInfo c;
    if (!base_variant(q, row.over, &c)) continue;
    if (row.kernel != BASE && !lay_over(q, row.kernel, row.over, &c)) continue;
    out->push_back(c);
  }
}

// Forward, transposed operands (transposeState, AttentionKernelDescriptor.swift:28-42) up to D = 256: code objects that read and
// write them in place, like the reference (AttentionKernel.swift:189-204) -- one per pattern of (K, V), Q and O are run-time flags
// of those (attn_fwd16_v3.h, TR).  No workspace, no re-layout pass.  Launches with K^T and / or V^T that the hand-placed streams take
// (attn_fwd16_p4_tr.h at bucket 128, attn_fwd16_p5_tr.h above) go to those: one candidate, whose other launches stay with the TR kernel
// (a bucket or pattern without a stream leaves it as it is)
void add_transposed_forward(const Request &q, Candidates *out) {
  const int pattern = (q.kd.transposeState[MFA_K] ? 1 : 0) | (q.kd.transposeState[MFA_V] ? 2 : 0);
  VariantInfo c;
  if (!fwd16_v3_tr_variant(q.pq, q.bucket, pattern, &c)) return;
  if (pattern != 0 && q.bucket == 128) fwd16_p4_tr_variant(q.pq, pattern, q.lowP, &c);
  if (pattern != 0 && q.bucket > 128) fwd16_p5_tr_variant(q.pq, q.bucket, pattern, q.lowP, &c);
  out->push_back(c);
}

#ifdef MFA_DEV_VARIANTS
// Developer builds only (make DEV=1 -> libmfa_hip_dev.so): environment knobs for A/B runs and timing-only ablations.
// The product library contains neither this code nor the code objects it selects.
void dev_knobs(const Request &q, Candidates *candidates, bool *f32) {
  if (std::getenv("MFA_F32_GENERAL")) *f32 = false;
  VariantInfo dev;
  bool have = false;
  const int type = q.type, pq = q.pq, pg = q.pg, bucket = generic_bucket(q.D);
  const char *knob = std::getenv("MFA_FWD16_IMPL");
  if (type == MFA_FORWARD && knob && !candidates->empty()) {
    if (std::strcmp(knob, "v1") == 0) have = fwd16_variant(pq, bucket, &dev);
    else if (std::strncmp(knob, "v2:", 3) == 0) have = fwd16_v2_variant(pq, bucket, std::atoi(knob + 3), &dev);
    else if (std::strncmp(knob, "v3:", 3) == 0) have = fwd16_v3_variant(pq, bucket, std::atoi(knob + 3), &dev);
    else if (std::strncmp(knob, "v4:", 3) == 0) have = fwd16_v4_variant(pq, bucket, std::atoi(knob + 3), &dev);
    else if (std::strncmp(knob, "p4:", 3) == 0) have = fwd16_v3_variant(pq, bucket, 0, &dev) && fwd16_p4_variant(pq, bucket, std::atoi(knob + 3), &dev);
    else if (std::strncmp(knob, "p5:", 3) == 0) have = fwd16_v3_variant(pq, bucket, 0, &dev) && fwd16_p5_variant(pq, bucket, std::atoi(knob + 3), &dev);
  }
  knob = std::getenv("MFA_DKV16_IMPL");
  if (type == MFA_BACKWARD_KEY_VALUE && knob && !candidates->empty()) {
    const int bk = bucket < 64 ? 64 : bucket;
    if (std::strcmp(knob, "w4") == 0) have = dkv16_variant(pq, pg, bk, &dev);
    else if (std::strncmp(knob, "rs:", 3) == 0) have = dkv16_rs_variant(pq, pg, bk, std::atoi(knob + 3), &dev);
    else if (std::strncmp(knob, "p4:", 3) == 0)
      have = dkv16_rs_variant(pq, pg, bk, 0, &dev) && dkv16_p4_variant(pq, pg, q.kd.memoryPrecisions[MFA_L], q.kd.memoryPrecisions[MFA_D], bk, std::atoi(knob + 3), &dev);
  }
  knob = std::getenv("MFA_DQ16_IMPL");
  if (type == MFA_BACKWARD_QUERY && knob && !candidates->empty() && std::strncmp(knob, "p4:", 3) == 0)
    have = dq16_variant(pq, pg, bucket, &dev) && dq16_p4_variant(pq, pg, bucket, std::atoi(knob + 3), &dev);
  if (type != MFA_FORWARD && std::getenv("MFA_BWD16_DISABLE")) candidates->clear();
  if (have) { candidates->clear(); candidates->push_back(dev); }
}
#endif

// how far candidate `c` is from the descriptor's parameter-table row (0: exact match)
int distance(const Desc &kd, const VariantInfo &c) {
  const int type = kd.type;
  // left-hand operands of the kernel type: (first, second) = (Q, -) / (Q, dO) / (K, V)
  const int firstLeft = type == MFA_BACKWARD_KEY_VALUE ? MFA_K : MFA_Q;
  const int secondLeft = type == MFA_FORWARD ? MFA_Q : type == MFA_BACKWARD_QUERY ? MFA_dO : MFA_V;
  bool accumulatorsCached;
  switch (type) {
    case MFA_FORWARD: accumulatorsCached = kd.cacheState[MFA_O] != 0; break;
    case MFA_BACKWARD_QUERY: accumulatorsCached = kd.cacheState[MFA_dQ] != 0; break;
    default: accumulatorsCached = kd.cacheState[MFA_dK] != 0 && kd.cacheState[MFA_dV] != 0; break;
  }
  int d = 0;
  if (c.headBlock < kd.headBlock) d += 8;   // (every candidate's head block holds D; among equals the smaller one wins in choose)
  if (c.parallelization != kd.parallelization) d += 4;
  if (c.traversal != kd.traversal) d += 2;
  if (c.cacheLeft != (kd.cacheState[firstLeft] != 0)) d += 1;
  if (type != MFA_FORWARD && c.cacheSecond != (kd.cacheState[secondLeft] != 0)) d += 1;
  // accumulators stay in registers in every code object except the paged one (D > 384: paged through the output buffers,
  // +Accumulate.swift:403-469): a row that asks for what the candidate does is an exact match either way
  if (accumulatorsCached == c.pagedAccumulators) d += 1;
  return d;
}

// The parameter-table row decides among the candidates (AttentionDescriptor.swift:37-54 -> AttentionKernel.swift:27-50: in the
// reference blockDimensions and cacheState ARE the kernel).  Exact match on (parallelization, traversal, head block, cached left-hand
// operands) wins; otherwise the nearest candidate serves the launch and mfa_attention_kernel_effective_descriptor reports what it
// really does -- unless the descriptor asks for strictBlockDimensions, in which case an unmatched row is an error.
mfa_status choose(const Desc &kd, const Candidates &candidates, VariantInfo *out) {
  size_t best = 0;
  for (size_t i = 1; i < candidates.size(); ++i) {
    const int di = distance(kd, candidates[i]), db = distance(kd, candidates[best]);
    if (di < db || (di == db && candidates[i].headBlock < candidates[best].headBlock)) best = i;
  }
  if (kd.strictBlockDimensions && distance(kd, candidates[best]) != 0) {
    std::string have;
    for (const VariantInfo &c : candidates)
      have += " (" + std::to_string(c.parallelization) + ", " + std::to_string(c.traversal) + ", " + std::to_string(c.headBlock) +
              (c.cacheLeft ? ", left operands cached)" : ", left operands streamed)");
    return fail(MFA_ERR_UNSUPPORTED, "no code object implements block dimensions (" + std::to_string(kd.parallelization) + ", " +
                                         std::to_string(kd.traversal) + ", " + std::to_string(kd.headBlock) +
                                         ") with the requested cache state; compiled (parallelization, traversal, head):" + have);
  }
  *out = candidates[best];
  return MFA_OK;
}

// the descriptor of what `variant` really does
void fill_effective(const Desc &kd, const VariantInfo &variant, bool fast, Desc *effective) {
  const int type = kd.type;
  *effective = kd;
  // register precisions the code object REALLY uses (AttentionDescriptor+Precisions.swift:149-215 describes Apple's choices):
  // the matrix-core kernels feed P (forward, dK/dV) and dS (backward) to the MFMA in the inputs' 16-bit type whatever
  // lowPrecisionIntermediates says; S, dP, the accumulators, L and D terms are fp32 registers in every kernel
  if (fast) {
    const int8_t pq = (int8_t)kd.memoryPrecisions[MFA_Q];
    effective->registerPrecisions[MFA_P] = pq;
    if (type != MFA_FORWARD) effective->registerPrecisions[MFA_dS] = pq;
    effective->registerPrecisions[MFA_S] = MFA_FP32;
    if (type != MFA_FORWARD) effective->registerPrecisions[MFA_dP] = MFA_FP32;
  }
  effective->parallelization = variant.parallelization;
  effective->traversal = variant.traversal;
  effective->headBlock = variant.headBlock;
  // accumulators always live in registers on gfx950; left-hand operands per variant
  const int8_t accCached = variant.pagedAccumulators ? 0 : 1;
  switch (type) {
    case MFA_FORWARD:
      effective->cacheState[MFA_Q] = variant.cacheLeft;
      effective->cacheState[MFA_O] = accCached;
      break;
    case MFA_BACKWARD_QUERY:
      effective->cacheState[MFA_Q] = variant.cacheLeft;
      effective->cacheState[MFA_dO] = variant.cacheSecond;
      effective->cacheState[MFA_dQ] = accCached;
      break;
    default:
      effective->cacheState[MFA_K] = variant.cacheLeft;
      effective->cacheState[MFA_V] = variant.cacheSecond;
      effective->cacheState[MFA_dK] = effective->cacheState[MFA_dV] = accCached;
      break;
  }
}

} // namespace

mfa_status select_variant(const Desc &kd, Selection *out) {
  mfa_status st = general_variant(kd, &out->general);
  if (st != MFA_OK) return st;
  const int type = kd.type, D = kd.headDimension;
  const Request q{kd, type, D, bucket16(D, type), kd.memoryPrecisions[MFA_Q], kd.memoryPrecisions[MFA_dO], kd.registerPrecisions[MFA_P] > MFA_FP32};
  bool transposed = false;   // some matrix operand of the kernel type is stored transposed
  for (int slot = 0; slot < MFA_BUFFER_SLOTS; ++slot)
    if (slot_used(type, slot) && slot != SLOT_L && slot != SLOT_D && kd.transposeState[slot_operand(slot)]) transposed = true;
  // transposed operands: the forward kernel reads them in place up to D = 256; its head blocks 320 / 384 and the backward kernels run
  // on row-major copies in the caller's workspace (the re-layout pass; without a workspace: the general kernel in place)
  const bool inPlace = transposed && type == MFA_FORWARD && q.bucket <= 256;
  Candidates candidates;   // matrix-core candidates, the product default first
  if (matrix_core_operands(q)) {
    if (inPlace) add_transposed_forward(q, &candidates);
    else if (type == MFA_FORWARD) add_rows(q, forwardRows, &candidates);
    else if (type == MFA_BACKWARD_QUERY) add_rows(q, backwardQueryRows, &candidates);
    else add_rows(q, backwardKeyValueRows, &candidates);
  }
  bool f32 = f32_production(kd);
#ifdef MFA_DEV_VARIANTS
  dev_knobs(q, &candidates, &f32);
#endif
  if (f32) f32_variant(type, generic_bucket(D), &out->general);
  // (the general kernel is not a candidate next to matrix-core variants: its block dimensions coincide with some of theirs,
  // and a table edit must not silently move a 16-bit problem onto fp32 arithmetic; it serves the launches they cannot)
  out->fast = !candidates.empty();
  if (!out->fast) candidates.push_back(out->general);
  st = choose(kd, candidates, &out->variant);
  if (st != MFA_OK) return st;
  out->relayout = out->fast && transposed && !inPlace;
  fill_effective(kd, out->variant, out->fast, &out->effective);
  return MFA_OK;
}

} // namespace mfa
