"""Decode attention over a KV cache (include/mfa_decode.h) against the only route the library had before it: the ordinary forward
launch with headsPerKeyValue + columnLengths + causal.  Both arms run from one library, in one process.

Shapes: bf16, D = 128 or 256 (--head-dim, default 128), Hq = 64 query heads over Hkv = 8 K / V heads (G = 8); R = 1 and 4 new rows; B = 1, 8, 64 sequences; caches of
4096 and 32768 keys, all full or with seeded mixed lengths (uniform between a quarter and the whole of the cache); the B = 8 rows
also with a paged cache (page sizes 16 and 256, shuffled pages) -- the forward launch cannot read pages, so their arm (b) is the
contiguous launch of the same shape.

Method: every launch of an arm reads a DIFFERENT copy of the cache, rotating over enough copies that their sum is well above the
256 MiB Infinity Cache (--rotate-bytes, default 1 GiB; the count is printed per row).  `launches` consecutive launches of an arm are
captured into one graph (the launch makes no host call that a capture forbids), so the host's enqueue cost stays out of the window;
a round is device events around one replay, the two arms alternate, and the table gives the median and the spread (min .. max) of
--rounds rounds after a warm-up replay of each.  us per launch therefore includes the launch boundaries (two kernels per split decode
launch).  TB/s = algorithmic bytes (sum_b len_b x Hkv x D x 2 operands x 2 bytes, plus Q and O) over arm (a)'s time per launch.

    python tools/decode_perf.py                  # the table
    python tools/decode_perf.py --trace-only     # a few launches of each arm, nothing timed: for rocprofv3 --kernel-trace --stats
    python tools/decode_perf.py --head-dim 256   # the same table at D = 256 (both arms; the forward launch is D = 256's only other route)
    python tools/decode_perf.py --fp8            # another table: decode over an e4m3 cache (include/mfa_kvcache.h) against the 16-bit
                                                 # decode launch, R = 1, same method; plus the append launch at B = 64
"""
import argparse
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from metal_flash_attention_amd import (AttentionDecode, AttentionDecodeFP8, KVCacheAppend, KVCachePrecision, AttentionDescriptor, AttentionKernel, AttentionKernelType, AttentionOperand as Op,  # noqa: E402
                                       GEMMOperandPrecision as P, _abi)

HQ, HKV = 64, 8
G = HQ // HKV


def forward_kernel(R, C, D):
    d = AttentionDescriptor()
    d.lowPrecisionInputs, d.lowPrecisionIntermediates = True, False
    d.lowPrecisionInputType, d.lowPrecisionOutputs = P.BF16, True
    d.matrixDimensions, d.transposeState = (R, C, D), (False,) * 4
    return AttentionKernel(d.kernelDescriptor(AttentionKernelType.forward))


class Row:
    def __init__(self, B, C, R, mixed, page, rotate_bytes, D):
        self.B, self.C, self.R, self.mixed, self.page, self.D = B, C, R, mixed, page, D
        g = torch.Generator().manual_seed(B * 131 + C + R)
        lens = torch.randint(C // 4, C + 1, (B,), generator=g, dtype=torch.int32) if mixed else torch.full((B,), C, dtype=torch.int32)
        self.keys = int(lens.sum())
        self.lens = lens.cuda()
        cache_bytes = 2 * B * HKV * C * D * 2
        self.copies = max(2, min(64, -(-rotate_bytes // cache_bytes)))
        self.q = torch.randn(B, HQ, R, D, device="cuda").to(torch.bfloat16)
        self.k = [(torch.randn(B, HKV, C, D, device="cuda") * 0.5).to(torch.bfloat16) for _ in range(self.copies)]
        self.v = [(torch.randn(B, HKV, C, D, device="cuda") * 0.5).to(torch.bfloat16) for _ in range(self.copies)]
        self.o = torch.empty(B, HQ, R, D, dtype=torch.bfloat16, device="cuda")
        self.l = torch.empty(B, HQ, R, dtype=torch.float32, device="cuda")
        self.bytes = self.keys * HKV * D * 2 * 2 + 2 * B * HQ * R * D * 2
        self.decode = AttentionDecode(D, P.BF16)
        self.kw = dict(rows=R, column=C, heads=HQ, batches=B, headsPerKeyValue=G, causal=True, cacheLengths=self.lens)
        if page:
            per = C // page
            perm = torch.randperm(B * per, generator=g)
            inv = torch.empty_like(perm)
            inv[perm] = torch.arange(B * per)
            pool = lambda t: t.view(B, HKV, per, page, D).permute(0, 2, 1, 3, 4).reshape(B * per, HKV, page, D)[inv.cuda()].contiguous()  # noqa: E731
            self.pk, self.pv = [pool(t) for t in self.k], [pool(t) for t in self.v]
            self.table = perm.view(B, per).to(torch.int32).cuda()   # page of (b, i) = where block b per + i went
            self.kw.update(pageSize=page, blockTable=self.table, blockTableStride=per, pageStrides=(HKV * page * D,) * 2,
                           strides=dict(K=(D, page * D, 0), V=(D, page * D, 0)))
        need = self.decode.workspaceSize(**self.kw)
        self.ws = torch.empty(need, dtype=torch.uint8, device="cuda") if need else None
        self.form = self.decode.launchForm(workspace=self.ws, **self.kw)
        self.forward = forward_kernel(R, C, D)
        self.hs = {Op.Q: R * D, Op.K: C * D, Op.V: C * D, Op.O: R * D, Op.L: R}
        self.bs = {Op.Q: HQ * R * D, Op.K: HKV * C * D, Op.V: HKV * C * D, Op.O: HQ * R * D, Op.L: HQ * R}

    def launch(self, arm, i, stream):
        c = i % self.copies
        if arm == "decode":
            k, v = (self.pk[c], self.pv[c]) if self.page else (self.k[c], self.v[c])
            self.decode.dispatch(self.q, k, v, self.o, self.l, stream=stream, workspace=self.ws, **self.kw)
        else:
            self.forward.dispatch({Op.Q: self.q, Op.K: self.k[c], Op.V: self.v[c], Op.O: self.o, Op.L: self.l}, row=self.R, column=self.C,
                                  heads=HQ, batches=self.B, headStrides=self.hs, batchStrides=self.bs, causal=True,
                                  columnLengths=self.lens, headsPerKeyValue=G, stream=stream)

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
    for arm in ("forward", "decode"):   # warm both arms (code objects, LDS limits) and size the window
        row.launch(arm, 0, stream)
        torch.cuda.synchronize()
        probe = row.graph(arm, row.copies)
        once(probe)
        est[arm] = once(probe) / row.copies
    out = {}
    graphs = {arm: (row.graph(arm, n), n) for arm, n in ((a, max(row.copies, min(4000, int(window_ms / max(est[a], 1e-4))))) for a in est)}
    samples = {arm: [] for arm in graphs}
    for arm in graphs:
        once(graphs[arm][0])
    for _ in range(rounds):
        for arm in ("forward", "decode"):   # alternate
            g, n = graphs[arm]
            samples[arm].append(once(g) / n * 1e3)
    for arm, v in samples.items():
        out[arm] = (statistics.median(v), min(v), max(v), graphs[arm][1])
    return out


class RowFP8:
    """R = 1: the FP8 decode launch (arm "fp8") and the 16-bit decode launch (arm "bf16") of the same shape, each rotating over its own
    cache copies whose sum is >= rotate_bytes; "append": the append launch that precedes a decode step (e4m3 cache)"""

    def __init__(self, B, C, mixed, rotate_bytes, D):
        self.B, self.C, self.R, self.mixed, self.D = B, C, 1, mixed, D
        g = torch.Generator().manual_seed(B * 131 + C + 1)
        lens = torch.randint(C // 4, C + 1, (B,), generator=g, dtype=torch.int32) if mixed else torch.full((B,), C, dtype=torch.int32)
        self.keys = int(lens.sum())
        self.lens = lens.cuda()
        self.q = torch.randn(B, HQ, 1, D, device="cuda").to(torch.bfloat16)
        self.o = torch.empty(B, HQ, 1, D, dtype=torch.bfloat16, device="cuda")
        self.l = torch.empty(B, HQ, 1, dtype=torch.float32, device="cuda")
        self.kscale, self.vscale = (0.5 + 1.5 * torch.rand(HKV, device="cuda") for _ in range(2))
        self.copies, self.k, self.v = {}, {}, {}
        for arm, esz in (("bf16", 2), ("fp8", 1)):
            n = self.copies[arm] = max(2, min(64, -(-rotate_bytes // (2 * B * HKV * C * D * esz))))
            make = (lambda: (torch.randn(B, HKV, C, D, device="cuda") * 0.5).to(torch.bfloat16)) if esz == 2 else \
                (lambda: (torch.randn(B, HKV, C, D, device="cuda") * 0.5).to(torch.float8_e4m3fn))
            self.k[arm], self.v[arm] = [make() for _ in range(n)], [make() for _ in range(n)]
        self.bytes = {"bf16": self.keys * HKV * D * 2 * 2 + 2 * B * HQ * D * 2, "fp8": self.keys * HKV * D * 2 + 2 * B * HQ * D * 2}
        self.dec = {"bf16": AttentionDecode(D, P.BF16), "fp8": AttentionDecodeFP8(D, P.BF16)}
        self.kw = {"bf16": dict(rows=1, column=C, heads=HQ, batches=B, headsPerKeyValue=G, causal=True, cacheLengths=self.lens)}
        self.kw["fp8"] = dict(self.kw["bf16"], keyScale=self.kscale, valueScale=self.vscale)
        need = self.dec["bf16"].workspaceSize(**self.kw["bf16"])
        assert need == self.dec["fp8"].workspaceSize(**self.kw["fp8"])
        self.ws = torch.empty(need, dtype=torch.uint8, device="cuda") if need else None
        self.form = self.dec["fp8"].launchForm(workspace=self.ws, **self.kw["fp8"])
        self.append = KVCacheAppend(D, P.BF16, KVCachePrecision.E4M3)
        self.knew, self.vnew = (torch.randn(B, HKV, 1, D, device="cuda").to(torch.bfloat16) for _ in range(2))
        self.copies["append"] = self.copies["fp8"]

    def launch(self, arm, i, stream):
        if arm == "append":
            c = i % self.copies["fp8"]
            self.append.dispatch(self.knew, self.vnew, self.k["fp8"][c], self.v["fp8"][c], stream=stream, rows=1, heads=HKV, batches=self.B,
                                 column=self.C, cacheLengths=self.lens, keyScale=self.kscale, valueScale=self.vscale)
            return
        c = i % self.copies[arm]
        self.dec[arm].dispatch(self.q, self.k[arm][c], self.v[arm][c], self.o, self.l, stream=stream, workspace=self.ws, **self.kw[arm])

    def graph(self, arm, launches):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            stream = torch.cuda.current_stream().cuda_stream
            for i in range(launches):
                self.launch(arm, i, stream)
        return g


def measure_arms(row, arms, rounds, window_ms):
    """measure() for any set of arms of a row whose copy count is per arm"""
    stream = torch.cuda.current_stream().cuda_stream
    est = {}
    for arm in arms:
        row.launch(arm, 0, stream)
        torch.cuda.synchronize()
        probe = row.graph(arm, row.copies[arm])
        once(probe)
        est[arm] = once(probe) / row.copies[arm]
    graphs = {arm: (row.graph(arm, n), n) for arm, n in ((a, max(row.copies[a], min(4000, int(window_ms / max(est[a], 1e-4))))) for a in arms)}
    samples = {arm: [] for arm in arms}
    for arm in arms:
        once(graphs[arm][0])
    for _ in range(rounds):
        for arm in arms:   # alternate
            g, n = graphs[arm]
            samples[arm].append(once(g) / n * 1e3)
    return {arm: (statistics.median(v), min(v), max(v), graphs[arm][1]) for arm, v in samples.items()}


def main_fp8(a):
    print("bf16 Q, D %d, Hq %d, Hkv %d (G %d), causal, R 1; arm (a) = decode over an e4m3 cache with per-head scales, arm (b) = the 16-bit decode "
          "launch; us per launch: median (min .. max) of %d rounds; TB/s = each arm's own algorithmic bytes over its time; achievable HBM "
          "rate 6.0-6.3 TB/s" % (a.head_dim, HQ, HKV, G, a.rounds))
    for B in (1, 8, 64):
        for C in (4096, 32768):
            if a.quick and (B == 64 or C != 4096):
                continue
            for mixed in (False, True):
                row = RowFP8(B, C, mixed, a.rotate_bytes, a.head_dim)
                arms = ("bf16", "fp8") + (("append",) if B == 64 else ())
                r = measure_arms(row, arms, a.rounds, a.window_ms)
                (fa, flo, fhi, fn), (ba, blo, bhi, bn) = r["fp8"], r["bf16"]
                extra = ""
                if "append" in r:
                    extra = " | append %6.1f (%6.1f .. %6.1f) x%d" % r["append"]
                print("B %2d  keys %5d %-5s copies %2d / %2d | (a) fp8 %9.1f (%9.1f .. %9.1f) x%-4d | (b) 16-bit %9.1f (%9.1f .. %9.1f) x%-4d | "
                      "(a)/(b) %5.3f | (a) %5.2f TB/s (b) %5.2f TB/s | %s%s" % (
                          B, C, "mixed" if mixed else "full", row.copies["fp8"], row.copies["bf16"], fa, flo, fhi, fn, ba, blo, bhi, bn, fa / ba,
                          row.bytes["fp8"] / (fa * 1e-6) / 1e12, row.bytes["bf16"] / (ba * 1e-6) / 1e12,
                          row.form.split(" (")[0] + (" + combine" if "combine" in row.form else ""), extra), flush=True)
                del row
                torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fp8", action="store_true", help="the e4m3-cache decode launch against the 16-bit decode launch (another table)")
    ap.add_argument("--head-dim", type=int, default=128, choices=(128, 256), help="the head dimension of every row (both arms)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=150.0, help="device time one timed replay aims at")
    ap.add_argument("--rotate-bytes", type=int, default=1 << 30)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--quick", action="store_true", help="B = 1 and 8 at 4096 keys only (a rehearsal)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "decode_perf.py measures on the GPU: there is nothing to report without one"
    sha = hashlib.sha256(open(_abi.library_path(), "rb").read()).hexdigest()
    print("library sha256 %s" % sha)
    if a.fp8:
        return main_fp8(a)
    print("bf16, D %d, Hq %d, Hkv %d (G %d), causal; arm (a) = decode launch, arm (b) = forward launch with headsPerKeyValue + "
          "columnLengths + causal; us per launch: median (min .. max) of %d rounds; achievable HBM rate 6.0-6.3 TB/s" % (a.head_dim, HQ, HKV, G, a.rounds))
    rows = []
    for R in (1, 4):
        for B in (1, 8, 64):
            for C in (4096, 32768):
                if a.quick and (B == 64 or C != 4096):
                    continue
                for mixed in (False, True):
                    for page in ((0, 16, 256) if B == 8 else (0,)):
                        rows.append((B, C, R, mixed, page))
    for B, C, R, mixed, page in rows:
        row = Row(B, C, R, mixed, page, a.rotate_bytes, a.head_dim)
        if a.trace_only:
            s = torch.cuda.current_stream().cuda_stream
            for i in range(3):
                row.launch("forward", i, s)
                row.launch("decode", i, s)
            torch.cuda.synchronize()
            continue
        r = measure(row, a.rounds, a.window_ms)
        (fa, flo, fhi, fn), (da, dlo, dhi, dn) = r["forward"], r["decode"]
        print("B %2d  keys %5d %-5s R %d  %-9s copies %2d | (a) %9.1f (%9.1f .. %9.1f) x%-4d | (b) %10.1f (%10.1f .. %10.1f) x%-4d | "
              "(b)/(a) %6.2f | (a) %5.2f TB/s | %s" % (B, C, "mixed" if mixed else "full", R, ("page %d" % page) if page else "contig", row.copies,
                                                      da, dlo, dhi, dn, fa, flo, fhi, fn, fa / da, row.bytes / (da * 1e-6) / 1e12,
                                                      row.form.split(" (")[0] + (" + combine" if "combine" in row.form else "")), flush=True)
        del row
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
