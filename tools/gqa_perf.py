"""Grouped-query attention against the same launch on K / V materialised per query head (mfa_launch_params.headsPerKeyValue).

Shape: Hq = 64 query heads over Hkv = 8 K / V heads (G = 8), N = 4096, D = 128, bf16 inputs and outputs (the torch binding's
descriptor), dense and causal.  One process; the grouped and the materialised launch alternate, each timed by
mfa_attention_kernel_time (HIP events around `iterations` back-to-back launches), median of `--rounds` rounds.  backwardKeyValue's
grouped time includes attn_kv_group_sum.

    python tools/gqa_perf.py                 # the table
    python tools/gqa_perf.py --trace-only    # a few launches of each, nothing timed: run under rocprofv3 --kernel-trace --stats
                                             # for attn_kv_group_sum's own kernel time (--group-sum-bytes prints what it moves)
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from metal_flash_attention_amd import AttentionDescriptor, AttentionKernel, AttentionKernelType, AttentionOperand, GEMMOperandPrecision  # noqa: E402

T = AttentionKernelType
Op = AttentionOperand
HQ, HKV, N, D = 64, 8, 4096, 128
G = HQ // HKV


def group_sum_bytes():
    """slabs read (fp32, Hq heads) + dK / dV written (bf16, Hkv heads)"""
    return 2 * HQ * N * D * 4 + 2 * HKV * N * D * 2


def setup():
    d = AttentionDescriptor()
    d.lowPrecisionInputs, d.lowPrecisionIntermediates = True, False
    d.lowPrecisionInputType, d.lowPrecisionOutputs = GEMMOperandPrecision.BF16, True
    d.matrixDimensions, d.transposeState = (N, N, D), (False,) * 4
    kernels = {t: AttentionKernel(d.kernelDescriptor(t)) for t in T}
    dt = {GEMMOperandPrecision.FP32: torch.float32, GEMMOperandPrecision.BF16: torch.bfloat16, GEMMOperandPrecision.FP16: torch.float16}
    prec = d.memoryPrecisions

    def buffers(kv_heads):
        bufs, hs, bs = {}, {}, {}
        for op in (Op.Q, Op.K, Op.V, Op.O, Op.L, Op.D, Op.dO, Op.dV, Op.dK, Op.dQ):
            heads = kv_heads if op in (Op.K, Op.V, Op.dK, Op.dV) else HQ
            per = N if op in (Op.L, Op.D) else N * D
            bufs[op] = (torch.randn(heads * per, device="cuda") * 0.5).to(dt[prec[op]])
            hs[op], bs[op] = per, heads * per
        return bufs, hs, bs
    return kernels, {"grouped": buffers(HKV), "materialised": buffers(HQ)}


def time_all(kernels, sets, causal, rounds, iterations):
    out = {}
    for t in T:
        samples = {"grouped": [], "materialised": []}
        for _ in range(rounds):
            for name in ("materialised", "grouped"):   # alternate
                bufs, hs, bs = sets[name]
                g = G if name == "grouped" else 1
                k = kernels[t]
                need = k.workspaceSize(row=N, column=N, heads=HQ, headsPerKeyValue=g)
                ws = torch.empty(need, dtype=torch.uint8, device="cuda") if need else None
                ms = k.time(bufs, row=N, column=N, heads=HQ, headStrides=hs, batchStrides=bs, warmup=2, iterations=iterations,
                            workspace=ws, causal=causal, headsPerKeyValue=g)
                samples[name].append(ms / iterations)
        out[t] = {n: statistics.median(v) for n, v in samples.items()}
        bufs, hs, bs = sets["grouped"]
        need = kernels[t].workspaceSize(row=N, column=N, heads=HQ, headsPerKeyValue=G)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda") if need else None
        out[t]["form"] = kernels[t].launchForm(bufs, row=N, column=N, heads=HQ, headStrides=hs, batchStrides=bs, workspace=ws,
                                               causal=causal, headsPerKeyValue=G)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--group-sum-bytes", action="store_true")
    a = ap.parse_args()
    if a.group_sum_bytes:
        print(group_sum_bytes())
        return
    kernels, sets = setup()
    if a.trace_only:
        time_all(kernels, sets, False, 1, 3)
        torch.cuda.synchronize()
        return
    print("Hq %d, Hkv %d (G %d), N %d, D %d, bf16; median of %d rounds x %d launches, ms per launch" % (HQ, HKV, G, N, D, a.rounds, a.iterations))
    names = {T.forward: "forward", T.backwardQuery: "dQ", T.backwardKeyValue: "dK/dV (+ group sum)"}
    for causal in (False, True):
        res = time_all(kernels, sets, causal, a.rounds, a.iterations)
        print("%s:" % ("causal" if causal else "dense"))
        for t in T:
            r = res[t]
            print("  %-20s materialised %8.3f  grouped %8.3f  grouped / materialised %.3f   [%s]" % (
                names[t], r["materialised"], r["grouped"], r["grouped"] / r["materialised"], r["form"]))
    print("attn_kv_group_sum moves %d bytes (slabs read + dK / dV written)" % group_sum_bytes())


if __name__ == "__main__":
    main()
