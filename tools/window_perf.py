"""Sliding-window attention over a KV cache (include/mfa_window.h) against the plain launches of the same library, in one process.

Arms, decode (R = 1) and prefill (R = 512) alike, bf16, D = 128, Hq = 64 over Hkv = 8, B = 8 full sequences:
  (w)  the windowed launch at (n, W)
  (W)  the plain launch over a cache of W keys          -- the same bytes: the expectation is (w) within this arm's min .. max spread
  (n)  the plain launch over the cache of n keys        -- what a windowed layer costs without the window
It is not fixed as a number: (w) passes if its median lies within the min .. max of (W).

Method (tools/decode_perf.py's): every launch of an arm reads a DIFFERENT copy of its cache, rotating over enough copies that their sum
is well above the 256 MiB Infinity Cache (--rotate-bytes); `launches` consecutive launches of an arm are captured into one graph; a
round is device events around one replay, the arms alternate, and the table gives the median and min .. max of --rounds rounds after a
warm-up replay of each.

    python tools/window_perf.py > profiles/window_perf.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from metal_flash_attention_amd import AttentionDecode, AttentionPrefill, GEMMOperandPrecision as P  # noqa: E402

HQ, HKV, D, B = 64, 8, 128, 8
G = HQ // HKV
SHAPES = [(4096, 1024), (32768, 1024), (32768, 4096)]   # (n, W)


class Arm:
    """one launch kind over rotating copies of a cache of C keys, all sequences full; window None: the plain launch"""

    def __init__(self, kind, R, C, window, rotate_bytes):
        self.kind, self.R, self.C, self.window = kind, R, C, window
        self.copies = max(2, min(64, -(-rotate_bytes // (2 * B * HKV * C * D * 2))))
        self.q = torch.randn(B, HQ, R, D, device="cuda").to(torch.bfloat16)
        self.k = [(torch.randn(B, HKV, C, D, device="cuda") * 0.5).to(torch.bfloat16) for _ in range(self.copies)]
        self.v = [(torch.randn(B, HKV, C, D, device="cuda") * 0.5).to(torch.bfloat16) for _ in range(self.copies)]
        self.o = torch.empty(B, HQ, R, D, dtype=torch.bfloat16, device="cuda")
        self.l = torch.empty(B, HQ, R, dtype=torch.float32, device="cuda")
        self.op = (AttentionDecode if kind == "decode" else AttentionPrefill)(D, P.BF16)
        self.kw = dict(rows=R, column=C, heads=HQ, batches=B, headsPerKeyValue=G, causal=True,
                       cacheLengths=torch.full((B,), C, dtype=torch.int32, device="cuda"))
        if window is not None:
            self.kw.update(window=window)
        if kind == "decode":
            need = self.op.workspaceSize(**self.kw)
            self.kw.update(workspace=torch.empty(need, dtype=torch.uint8, device="cuda") if need else None)
        self.form = self.op.launchForm(**self.kw)

    def launch(self, i, stream):
        c = i % self.copies
        self.op.dispatch(self.q, self.k[c], self.v[c], self.o, self.l, stream=stream, **self.kw)

    def graph(self, launches):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            stream = torch.cuda.current_stream().cuda_stream
            for i in range(launches):
                self.launch(i, stream)
        return g


def once(graph):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    graph.replay()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def measure(arms, rounds, window_ms):
    """{name: (median, min, max) us per launch}: the arms alternate, `rounds` rounds after a warm-up replay of each"""
    graphs = {}
    for name, arm in arms.items():
        arm.launch(0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        probe = arm.graph(arm.copies)
        once(probe)
        est = once(probe) / arm.copies
        n = max(arm.copies, min(4000, int(window_ms / max(est, 1e-4))))
        graphs[name] = (arm.graph(n), n)
        once(graphs[name][0])
    samples = {name: [] for name in arms}
    for _ in range(rounds):
        for name, (g, n) in graphs.items():
            samples[name].append(once(g) * 1e3 / n)
    return {name: (statistics.median(s), min(s), max(s)) for name, s in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--rotate-bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    print("tools/window_perf.py -- windowed launch (w) against the plain launch over W keys (W) and over n keys (n); us per launch,")
    print("median of %d rounds (min .. max); bf16, D %d, Hq %d, Hkv %d, B %d full sequences; %s" % (
        args.rounds, D, HQ, HKV, B, torch.cuda.get_device_name(0)))
    for kind, R in (("decode", 1), ("prefill", 512)):
        for n, W in SHAPES:
            arms = {"w": Arm(kind, R, n, W, args.rotate_bytes), "W": Arm(kind, R, max(W, R), None, args.rotate_bytes),
                    "n": Arm(kind, R, n, None, args.rotate_bytes)}
            res = measure(arms, args.rounds, args.window_ms)
            inside = res["W"][1] <= res["w"][0] <= res["W"][2]
            print("%-7s R %4d  n %6d  W %5d   " % (kind, R, n, W) + "   ".join(
                "(%s) %8.1f (%.1f .. %.1f)" % (a, *res[a]) for a in ("w", "W", "n")) +
                "   (w)/(W) %.3f  (n)/(w) %.2f   (w) within (W)'s spread: %s" % (res["w"][0] / res["W"][0], res["n"][0] / res["w"][0], "yes" if inside else "NO"))
            print("        (w) " + arms["w"].form)
            del arms
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
