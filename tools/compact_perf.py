"""The KV-cache compaction of the accepted speculation-tree path (include/mfa_compact.h) against the append launch that writes the same
bytes and against what a caller had on a contiguous cache, in one process: a sibling of tools/tree_perf.py.  Every timed call is ONE
launch (arm (t): its four torch kernels) between two events on a different copy of the cache -- consecutive launches, whichever their
arms, rotate over the copies --; the arms alternate launch by launch inside a round; a round's figure is the mean of its launches, a
cell's the median and min .. max of --rounds rounds.

Arms:
  (c)  the compaction of a of R rows, K and V, one launch                        -- kv_cache_compact_b128 / _b256
  (a)  the append launch for the same a rows: existing code that writes the same bytes, the yardstick  -- kv_cache_append_d128_*
  (t)  what a caller had on a contiguous cache: index_select into a temporary plus index_copy_, for K and for V (bytes, 16-bit and e4m3 alike)
Shapes: D = 128, Hkv 8, B = 8 and 64, caches of 1024 keys with 1000 valid, (a, R) = (3, 4) and (8, 64); 16-bit and e4m3 caches.  The launch
moves at most a few hundred KiB: it should be bound by launch latency.  No ratio is fixed in advance.

    python tools/compact_perf.py > profiles/compact_perf.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from metal_flash_attention_amd import GEMMOperandPrecision as P, KVCacheAppend, KVCacheCompact, KVCachePrecision  # noqa: E402

D, HKV, C, N = 128, 8, 1024, 1000
CELLS = ((3, 4), (8, 64))


class Cell:
    """rotating copies of a cache of B sequences, the accepted path and the new rows: what every arm reads and writes"""

    def __init__(self, B, a, R, fp8, rotate_bytes):
        self.B, self.a, self.R, self.fp8 = B, a, R, fp8
        item = 1 if fp8 else 2
        self.copies = max(2, min(16, -(-rotate_bytes // (2 * B * HKV * C * D * item))))
        kind = torch.float8_e4m3fn if fp8 else torch.bfloat16
        self.k = [(torch.randn(B, HKV, C, D, device="cuda", dtype=torch.bfloat16) * 0.5).to(kind) for _ in range(self.copies)]
        self.v = [(torch.randn(B, HKV, C, D, device="cuda", dtype=torch.bfloat16) * 0.5).to(kind) for _ in range(self.copies)]
        self.lengths = torch.full((B,), N, dtype=torch.int32, device="cuda")            # includes the R tree rows
        path = [R - 1 - i for i in range(a)]                                            # the tree's last rows, reversed: none in place
        self.accepted = torch.tensor([path] * B, dtype=torch.int32, device="cuda")
        self.counts = torch.full((B,), a, dtype=torch.int32, device="cuda")
        self.new_lengths = torch.empty((B,), dtype=torch.int32, device="cuda")
        self.after = torch.full((B,), N - R + a, dtype=torch.int32, device="cuda")      # what the append arm writes below
        self.k_new, self.v_new = (torch.randn(B, HKV, a, D, device="cuda").to(torch.bfloat16) for _ in range(2))
        self.source = torch.tensor([N - R + j for j in path], device="cuda")
        self.target = torch.arange(N - R, N - R + a, device="cuda")
        self.compact = KVCacheCompact(D, KVCachePrecision.E4M3 if fp8 else P.BF16)
        self.append = KVCacheAppend(D, P.BF16, KVCachePrecision.E4M3 if fp8 else None)

    def run(self, arm, i, stream):
        k, v = self.k[i % self.copies], self.v[i % self.copies]
        if arm == "c":
            self.compact.dispatch(k, v, stream=stream, rows=self.R, heads=HKV, batches=self.B, column=C, cacheLengths=self.lengths,
                                  accepted=self.accepted, acceptedStride=self.a, maxAccepted=self.a, acceptedCounts=self.counts, newLengths=self.new_lengths)
        elif arm == "a":
            self.append.dispatch(self.k_new, self.v_new, k, v, stream=stream, rows=self.a, heads=HKV, batches=self.B, column=C, cacheLengths=self.after)
        else:
            for t in (k.view(torch.uint8), v.view(torch.uint8)):
                t.index_copy_(2, self.target, t.index_select(2, self.source))

    def once(self, arm, i, stream):
        """microseconds of one launch of an arm on copy i"""
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        self.run(arm, i, stream)
        stop.record()
        stop.synchronize()
        return 1e3 * start.elapsed_time(stop)


def measure(cell, rounds, launches):
    """{arm: (median, min, max)} us per launch; the arms alternate launch by launch, one warm-up pass first"""
    stream = torch.cuda.current_stream().cuda_stream
    arms = ("c", "a", "t")
    for arm in arms:
        cell.once(arm, 0, stream)
    per = {arm: [] for arm in arms}
    at = 1
    for _ in range(rounds):
        took = {arm: 0.0 for arm in arms}
        for _i in range(launches):
            for arm in arms:
                took[arm] += cell.once(arm, at, stream)
                at += 1
        for arm in arms:
            per[arm].append(took[arm] / launches)
    return {arm: (statistics.median(x), min(x), max(x)) for arm, x in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--rotate-bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    print("tools/compact_perf.py -- the compaction of a of R tree rows (c) against the append launch for the same a rows (a) and a torch")
    print("index_select + index_copy_ for K and V on the contiguous cache (t); us per launch between two events, median of %d rounds of %d" % (
        args.rounds, args.launches))
    print("launches (min .. max); D %d, Hkv %d, caches of %d keys with %d valid; %s" % (D, HKV, C, N, torch.cuda.get_device_name(0)))
    for a, R in CELLS:
        for fp8 in (False, True):
            for B in (8, 64):
                cell = Cell(B, a, R, fp8, args.rotate_bytes)
                res = measure(cell, args.rounds, args.launches)
                print("a %d of R %2d  %-6s B %2d  %2d copies   " % (a, R, "e4m3" if fp8 else "16-bit", B, cell.copies) +
                      "   ".join("(%s) %7.1f (%.1f .. %.1f)" % (arm, *res[arm]) for arm in ("c", "a", "t")) +
                      "   (c)/(a) %.3f   (t)/(c) %.2f" % (res["c"][0] / res["a"][0], res["t"][0] / res["c"][0]), flush=True)
                del cell
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
