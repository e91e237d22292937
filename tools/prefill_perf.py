"""Prefill attention over a KV cache (include/mfa_prefill.h) against what the library offered before it: the forward launch with
headsPerKeyValue + rowLengths + columnLengths + causal on a contiguous 16-bit cache, and -- for a paged or e4m3 cache, which the forward
launch cannot read -- a torch gather (and dequantise) of the pages into a contiguous 16-bit buffer followed by that forward launch.
All arms run from one library, in one process.

Shapes: bf16, D = 128 or 256 (--head-dim, default 128), Hq = 64 query heads, G = 8 and G = 1, causal; a chunk of R = 512 and 2048 new rows against n = 4096 / 32768
cached keys (the chunk's own keys included), B = 1 and 8 sequences, every sequence full.  Arms:
  (a16) (a256)  the prefill launch on a paged cache, page sizes 16 and 256, shuffled tables
  (a')          the prefill launch on the contiguous cache
  (a8)          the prefill launch on a paged e4m3 cache (page 16, per-head scales)
  (b)           the forward launch on the contiguous cache
  (b')          gather of the page-16 pool into a contiguous buffer (index_select + one strided copy) + (b)
  (b'8)         the same from the e4m3 pool (the copy converts to bf16; a per-head scale would be one more pass, not counted) + (b)

Method (tools/decode_perf.py's): every launch of an arm reads a DIFFERENT copy of the cache, rotating over enough copies that their sum
is above the 256 MiB Infinity Cache (--rotate-bytes; at least two copies); a page pool is the contiguous copy's own memory seen as
[pages][Hkv][page][D] under a shuffled table (timing does not depend on the values).  `launches` consecutive launches of an arm are
captured into one graph; a round is device events around one replay, the arms alternate, and the table gives the median and the
spread (min .. max) of --rounds rounds after a warm-up replay of each.  roof = 4 B Hq D x (visible row-key pairs) FLOP over the time,
as a fraction of 2500 TFLOP/s (the bf16 matrix peak bench.py uses).

    python tools/prefill_perf.py                 # the table
    python tools/prefill_perf.py --head-dim 256  # the same table at D = 256 (every arm)
    python tools/prefill_perf.py --quick         # B = 1, n = 4096 only (a rehearsal)
    python tools/prefill_perf.py --trace-only    # a few launches of each arm of the largest shape, nothing timed: for a kernel trace
"""
import argparse
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from metal_flash_attention_amd import (AttentionDescriptor, AttentionKernel, AttentionKernelType, AttentionOperand as Op, AttentionPrefill,  # noqa: E402
                                       GEMMOperandPrecision as P, KVCachePrecision, _abi)

HQ = 64
PEAK = 2500e12
ARMS = ("a16", "a256", "a'", "a8", "b", "b'", "b'8")


def forward_kernel(R, C, D):
    d = AttentionDescriptor()
    d.lowPrecisionInputs, d.lowPrecisionIntermediates = True, False
    d.lowPrecisionInputType, d.lowPrecisionOutputs = P.BF16, True
    d.matrixDimensions, d.transposeState = (R, C, D), (False,) * 4
    return AttentionKernel(d.kernelDescriptor(AttentionKernelType.forward))


class Row:
    def __init__(self, B, C, R, G, rotate_bytes, D):
        self.B, self.C, self.R, self.G, self.D = B, C, R, G, D
        Hkv = self.Hkv = HQ // G
        g = torch.Generator().manual_seed(B * 131 + C + R + G)
        self.lens = torch.full((B,), C, dtype=torch.int32, device="cuda")
        self.qlens = torch.full((B,), R, dtype=torch.int32, device="cuda")
        cache_bytes = 2 * B * Hkv * C * D * 2
        self.copies = max(2, min(64, -(-rotate_bytes // cache_bytes)))
        make = lambda: torch.empty(B, Hkv, C, D, dtype=torch.bfloat16, device="cuda").normal_(0.0, 0.5)  # noqa: E731
        self.q = torch.empty(B, HQ, R, D, dtype=torch.bfloat16, device="cuda").normal_()
        self.k, self.v = [make() for _ in range(self.copies)], [make() for _ in range(self.copies)]
        self.k8, self.v8 = [t.to(torch.float8_e4m3fn) for t in self.k], [t.to(torch.float8_e4m3fn) for t in self.v]
        self.kscale, self.vscale = (0.5 + 1.5 * torch.rand(Hkv, device="cuda") for _ in range(2))
        self.o = torch.empty(B, HQ, R, D, dtype=torch.bfloat16, device="cuda")
        self.l = torch.empty(B, HQ, R, dtype=torch.float32, device="cuda")
        self.gk, self.gv = torch.empty_like(self.k[0]), torch.empty_like(self.v[0])   # where (b') gathers to
        self.flop = 4.0 * B * HQ * D * (R * (C - R) + R * (R + 1) / 2)
        self.pre = AttentionPrefill(D, P.BF16)
        self.pre8 = AttentionPrefill(D, P.BF16, cachePrecision=KVCachePrecision.E4M3)
        self.kw = dict(rows=R, column=C, heads=HQ, batches=B, headsPerKeyValue=G, causal=True, cacheLengths=self.lens, queryLengths=self.qlens)
        self.paged = {}
        for page in (16, 256):
            per = C // page
            table = torch.randperm(B * per, generator=g).view(B, per).to(torch.int32).cuda()
            self.paged[page] = (table, dict(self.kw, pageSize=page, blockTable=table, blockTableStride=per, pageStrides=(Hkv * page * D,) * 2,
                                            strides=dict(K=(D, page * D, 0), V=(D, page * D, 0))))
        self.index = self.paged[16][0].view(-1).long()
        self.form = self.pre.launchForm(**self.kw)
        self.forward = forward_kernel(R, C, D)
        self.hs = {Op.Q: R * D, Op.K: C * D, Op.V: C * D, Op.O: R * D, Op.L: R}
        self.bs = {Op.Q: HQ * R * D, Op.K: Hkv * C * D, Op.V: Hkv * C * D, Op.O: HQ * R * D, Op.L: HQ * R}

    def gather(self, pool, dst):
        """the pages of every sequence, in order, into the contiguous [B][Hkv][C][D] buffer (converting when the pool is e4m3)"""
        B, Hkv, per, D = self.B, self.Hkv, self.C // 16, self.D
        pages = pool.view(B * per, Hkv, 16, D).index_select(0, self.index)
        dst.view(B, Hkv, per, 16, D).copy_(pages.view(B, per, Hkv, 16, D).permute(0, 2, 1, 3, 4))

    def fwd(self, k, v, stream):
        self.forward.dispatch({Op.Q: self.q, Op.K: k, Op.V: v, Op.O: self.o, Op.L: self.l}, row=self.R, column=self.C, heads=HQ,
                              batches=self.B, headStrides=self.hs, batchStrides=self.bs, causal=True, rowLengths=self.qlens,
                              columnLengths=self.lens, headsPerKeyValue=self.G, stream=stream)

    def launch(self, arm, i, stream):
        c = i % self.copies
        if arm in ("a16", "a256"):
            self.pre.dispatch(self.q, self.k[c], self.v[c], self.o, self.l, stream=stream, **self.paged[int(arm[1:])][1])
        elif arm == "a'":
            self.pre.dispatch(self.q, self.k[c], self.v[c], self.o, self.l, stream=stream, **self.kw)
        elif arm == "a8":
            self.pre8.dispatch(self.q, self.k8[c], self.v8[c], self.o, self.l, stream=stream, keyScale=self.kscale, valueScale=self.vscale,
                               **self.paged[16][1])
        elif arm == "b":
            self.fwd(self.k[c], self.v[c], stream)
        else:
            pk, pv = (self.k8[c], self.v8[c]) if arm == "b'8" else (self.k[c], self.v[c])
            self.gather(pk, self.gk)
            self.gather(pv, self.gv)
            self.fwd(self.gk, self.gv, stream)

    def graph(self, arm, launches):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            stream = torch.cuda.current_stream().cuda_stream
            for i in range(launches):
                self.launch(arm, i, stream)
        return g


def once(graph):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    graph.replay()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def measure(row, rounds, window_ms):
    stream = torch.cuda.current_stream().cuda_stream
    est = {}
    for arm in ARMS:   # warm every arm (code objects) and size the window
        row.launch(arm, 0, stream)
        torch.cuda.synchronize()
        probe = row.graph(arm, row.copies)
        once(probe)
        est[arm] = once(probe) / row.copies
        del probe
    graphs = {a: (row.graph(a, n), n) for a, n in ((a, max(row.copies, min(2000, int(window_ms / max(est[a], 1e-4))))) for a in ARMS)}
    samples = {a: [] for a in ARMS}
    for a in ARMS:
        once(graphs[a][0])
    for _ in range(rounds):
        for a in ARMS:   # alternate
            g, n = graphs[a]
            samples[a].append(once(g) / n * 1e3)
    return {a: (statistics.median(v), min(v), max(v), graphs[a][1]) for a, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head-dim", type=int, default=128, choices=(128, 256), help="the head dimension of every row (every arm)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=60.0, help="device time one timed replay aims at")
    ap.add_argument("--rotate-bytes", type=int, default=1 << 30)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--quick", action="store_true", help="B = 1, n = 4096 only (a rehearsal)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "prefill_perf.py measures on the GPU: there is nothing to report without one"
    print("library sha256 %s" % hashlib.sha256(open(_abi.library_path(), "rb").read()).hexdigest())
    if a.trace_only:
        row = Row(8, 32768, 2048, 8, a.rotate_bytes, a.head_dim)
        s = torch.cuda.current_stream().cuda_stream
        for i in range(3):
            for arm in ARMS:
                row.launch(arm, i, s)
        torch.cuda.synchronize()
        return
    print("bf16, D %d, Hq %d, causal, full sequences; us per launch: median (min .. max) of %d rounds, launches per replay after x; "
          "roof = fraction of %.0f TFLOP/s" % (a.head_dim, HQ, a.rounds, PEAK / 1e12))
    for G in (8, 1):
        for R in (512, 2048):
            for C in (4096, 32768):
                for B in (1, 8):
                    if a.quick and (B != 1 or C != 4096):
                        continue
                    row = Row(B, C, R, G, a.rotate_bytes, a.head_dim)
                    r = measure(row, a.rounds, a.window_ms)
                    print("G %d  R %4d  n %5d  B %d  copies %2d  %s" % (G, R, C, B, row.copies, row.form), flush=True)
                    for arm in ARMS:
                        med, lo, hi, n = r[arm]
                        print("    (%-4s) %10.1f (%10.1f .. %10.1f) x%-4d  roof %.3f" % (arm, med, lo, hi, n, row.flop / (med * 1e-6) / PEAK), flush=True)
                    print("    (a16)/(b') %.3f   (a256)/(b') %.3f   (a')/(b) %.3f   (a8)/(a16) %.3f   (a8)/(b'8) %.3f   (a16)/(a') %.3f" % (
                        r["a16"][0] / r["b'"][0], r["a256"][0] / r["b'"][0], r["a'"][0] / r["b"][0], r["a8"][0] / r["a16"][0],
                        r["a8"][0] / r["b'8"][0], r["a16"][0] / r["a'"][0]), flush=True)
                    del row, r
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
