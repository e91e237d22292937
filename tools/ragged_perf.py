"""Ragged batches over a KV cache (include/mfa_ragged.h) against the route the library had before them: the padded prefill launch
(queryLengths, rows = the largest count) of the same sequences, and one append launch per sequence.  Both arms run from one library,
in one process; arm (b) is existing code, so it is what the library did before.

Shapes: bf16, D = 128, Hq = 64 query heads over Hkv = 8 K / V heads (G = 8, RB = 16), paged cache (page 16, shuffled pages), cache
lengths of 4096, causal.  Batches: 63 sequences of 1 row + 1 of 2048 rows; 255 of 1 row + 1 of 4096 rows; and 8 x 512 rows, where the
two grids coincide -- that row prices the slot search itself: (a) / (b) there is its overhead.  The append row: the packed launch
against B launches with batches = 1.

Method (tools/decode_perf.py's): every launch of an arm reads a DIFFERENT copy of the cache, rotating over enough copies that their
sum is well above the 256 MiB Infinity Cache (--rotate-bytes; the count is printed per row).  Consecutive launches of an arm are
captured into one graph, so the host's enqueue cost stays out of the window; a round is device events around one replay, the two
arms alternate, and the table gives the median and the spread (min .. max) of --rounds rounds after a warm-up replay of each.

    python tools/ragged_perf.py                  # the table
    python tools/ragged_perf.py --quick          # the small mixed batch and the uniform batch only (a rehearsal)
"""
import argparse
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from metal_flash_attention_amd import AttentionPrefill, GEMMOperandPrecision as P, KVCacheAppend, _abi  # noqa: E402

HQ, HKV, D, PAGE, C = 64, 8, 128, 16, 4096
G = HQ // HKV
MAX_NODES = 4000   # kernel nodes of one captured graph


class Row:
    """one batch: `counts` rows per sequence, every cache length C"""

    def __init__(self, counts, rotate_bytes):
        self.counts, self.B, self.R = counts, len(counts), max(counts)
        B, R = self.B, self.R
        starts = [0]
        for c in counts:
            starts.append(starts[-1] + c)
        self.T = T = starts[-1]
        g = torch.Generator().manual_seed(B * 131 + T)
        self.lens = torch.full((B,), C, dtype=torch.int32, device="cuda")
        self.qlens = torch.tensor(counts, dtype=torch.int32, device="cuda")
        self.starts = torch.tensor(starts, dtype=torch.int32, device="cuda")
        per = C // PAGE
        cache_bytes = 2 * B * HKV * C * D * 2
        self.copies = max(2, min(64, -(-rotate_bytes // cache_bytes)))
        pool = lambda: (torch.randn(B * per, HKV, PAGE, D, device="cuda") * 0.5).to(torch.bfloat16)  # noqa: E731
        self.pk, self.pv = [pool() for _ in range(self.copies)], [pool() for _ in range(self.copies)]
        self.table = torch.randperm(B * per, generator=g).view(B, per).to(torch.int32).cuda()
        # packed operands, and the padded ones the existing launch wants: only a sequence's own rows are ever read or written
        self.q = torch.randn(T, HQ, D, device="cuda").to(torch.bfloat16)
        self.o = torch.empty(T, HQ, D, dtype=torch.bfloat16, device="cuda")
        self.l = torch.empty(HQ, T, dtype=torch.float32, device="cuda")
        self.qpad = torch.empty(B, HQ, R, D, dtype=torch.bfloat16, device="cuda")
        for b, c in enumerate(counts):
            self.qpad[b, :, :c] = self.q[starts[b]:starts[b] + c].transpose(0, 1)
        self.opad = torch.empty(B, HQ, R, D, dtype=torch.bfloat16, device="cuda")
        self.lpad = torch.empty(B, HQ, R, dtype=torch.float32, device="cuda")
        self.prefill = AttentionPrefill(D, P.BF16)
        cache = dict(pageSize=PAGE, blockTable=self.table, blockTableStride=per, pageStrides=(HKV * PAGE * D,) * 2,
                     strides=dict(K=(D, PAGE * D, 0), V=(D, PAGE * D, 0)))
        shape = dict(rows=R, column=C, heads=HQ, batches=B, headsPerKeyValue=G, causal=True, cacheLengths=self.lens)
        self.kw = {"ragged": dict(shape, rowStarts=self.starts, totalRows=T, **cache), "padded": dict(shape, queryLengths=self.qlens, **cache)}
        self.forms = {arm: self.prefill.launchForm(**kw) for arm, kw in self.kw.items()}
        # the append: the packed launch, and one launch per sequence
        self.append = KVCacheAppend(D, P.BF16)
        self.knew, self.vnew = (torch.randn(T, HKV, D, device="cuda").to(torch.bfloat16) for _ in range(2))
        self.kseq = [(self.knew[starts[b]:starts[b] + c].transpose(0, 1).contiguous(), self.vnew[starts[b]:starts[b] + c].transpose(0, 1).contiguous())
                     for b, c in enumerate(counts)]
        self.akw = dict(heads=HKV, pageSize=PAGE, blockTableStride=per, pageStrides=(HKV * PAGE * D,) * 2,
                        strides=dict(kCache=(D, PAGE * D, 0), vCache=(D, PAGE * D, 0)))
        self.nodes = {"ragged": 1, "padded": 1, "append ragged": 1, "append per sequence": B}

    def launch(self, arm, i, stream):
        c = i % self.copies
        if arm == "ragged":
            self.prefill.dispatch(self.q, self.pk[c], self.pv[c], self.o, self.l, stream=stream, **self.kw[arm])
        elif arm == "padded":
            self.prefill.dispatch(self.qpad, self.pk[c], self.pv[c], self.opad, self.lpad, stream=stream, **self.kw[arm])
        elif arm == "append ragged":
            self.append.dispatch(self.knew, self.vnew, self.pk[c], self.pv[c], stream=stream, rows=self.R, batches=self.B, cacheLengths=self.lens,
                                 blockTable=self.table, rowStarts=self.starts, totalRows=self.T, **self.akw)
        else:
            for b, count in enumerate(self.counts):
                self.append.dispatch(self.kseq[b][0], self.kseq[b][1], self.pk[c], self.pv[c], stream=stream, rows=count, batches=1,
                                     cacheLengths=self.lens[b:], blockTable=self.table[b:], **self.akw)

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


def measure(row, arms, rounds, window_ms):
    """-> arm: (median, min, max) us per launch (a per-sequence append: per B launches), launches per replay"""
    stream = torch.cuda.current_stream().cuda_stream
    est = {}
    for arm in arms:   # warm both arms (code objects, LDS limits) and size the window
        row.launch(arm, 0, stream)
        torch.cuda.synchronize()
        n = max(1, min(row.copies, MAX_NODES // row.nodes[arm]))
        probe = row.graph(arm, n)
        once(probe)
        est[arm] = once(probe) / n
    count = {a: max(min(row.copies, MAX_NODES // row.nodes[a]), min(MAX_NODES // row.nodes[a], int(window_ms / max(est[a], 1e-4)))) for a in arms}
    graphs = {a: (row.graph(a, count[a]), count[a]) for a in arms}
    samples = {a: [] for a in arms}
    for a in arms:
        once(graphs[a][0])
    for _ in range(rounds):
        for a in arms:   # alternate
            g, n = graphs[a]
            samples[a].append(once(g) / n * 1e3)
    return {a: (statistics.median(v), min(v), max(v), graphs[a][1]) for a, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0, help="device time one timed replay aims at")
    ap.add_argument("--rotate-bytes", type=int, default=1 << 30)
    ap.add_argument("--quick", action="store_true", help="63 x 1 + 2048 and 8 x 512 only (a rehearsal)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ragged_perf.py measures on the GPU: there is nothing to report without one"
    print("library sha256 %s" % hashlib.sha256(open(_abi.library_path(), "rb").read()).hexdigest())
    print("bf16, D %d, Hq %d, Hkv %d (G %d), causal, paged %d, cache lengths %d; arm (a) = the ragged launch, arm (b) = the padded launch with "
          "queryLengths (prefill) / one launch per sequence (append); us per launch (append (b): per B launches): median (min .. max) of %d rounds"
          % (D, HQ, HKV, G, PAGE, C, a.rounds))
    batches = [("63 x 1 + 1 x 2048", [1] * 63 + [2048]), ("255 x 1 + 1 x 4096", [1] * 255 + [4096]), ("8 x 512 (uniform)", [512] * 8)]
    if a.quick:
        batches = [batches[0], batches[2]]
    for name, counts in batches:
        row = Row(counts, a.rotate_bytes)
        r = measure(row, ("ragged", "padded"), a.rounds, a.window_ms)
        (ra, rlo, rhi, rn), (pa, plo, phi, pn) = r["ragged"], r["padded"]
        spread = max((rhi - rlo) / ra, (phi - plo) / pa)
        print("prefill %-19s copies %2d | (a) %9.1f (%9.1f .. %9.1f) x%-4d | (b) %9.1f (%9.1f .. %9.1f) x%-4d | (a)/(b) %6.3f | spread %5.3f | "
              "(a) grid %s (b) grid %s" % (name, row.copies, ra, rlo, rhi, rn, pa, plo, phi, pn, ra / pa, spread,
                                           row.forms["ragged"].split("grid ")[1].split(" =")[0], row.forms["padded"].split("grid ")[1].split(" =")[0]), flush=True)
        if counts[0] == 1 and (len(counts) == 256 or a.quick):
            r = measure(row, ("append ragged", "append per sequence"), a.rounds, a.window_ms)
            (ra, rlo, rhi, rn), (pa, plo, phi, pn) = r["append ragged"], r["append per sequence"]
            print("append  %-19s copies %2d | (a) %9.1f (%9.1f .. %9.1f) x%-4d | (b) %9.1f (%9.1f .. %9.1f) x%-4d | (a)/(b) %6.3f | "
                  "(b) is %d launches" % (name, row.copies, ra, rlo, rhi, rn, pa, plo, phi, pn, ra / pa, row.B), flush=True)
        del row
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
