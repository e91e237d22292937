"""Attention sinks over a KV cache (include/mfa_sink.h) against the windowed launch of the same (n, W), in one process: a sibling of
tools/window_perf.py, whose Arm, method and measure() it reuses.

Arms, decode (R = 1) and prefill (R = 512) alike, bf16, D = 128, Hq = 64 over Hkv = 8, B = 8 full sequences:
  (w)  the windowed launch at (n, W)                                   -- mfa_window.h
  (s)  the same launch with S = 4 sink tokens and one sink logit per query head    -- mfa_sink.h
The expectation, not fixed as a number: (s) costs (w) plus the read of ONE more 64-key tile per workgroup -- (s)/(w) near
(tiles of W + 1) / (tiles of W) for decode, which is bound by the bytes of K and V, and less than that for prefill.

    python tools/sink_perf.py > profiles/sink_perf.txt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import window_perf as wp  # noqa: E402

SINK_TOKENS = 4


class SinkArm(wp.Arm):
    """the windowed arm plus sink tokens and sink logits (the keywords go in before the workspace is sized: the plan counts the sink tile)"""

    def __init__(self, kind, R, C, window, rotate_bytes):
        super().__init__(kind, R, C, window, rotate_bytes)
        self.logits = torch.linspace(-1.0, 3.0, wp.HQ, dtype=torch.float32, device="cuda")
        self.kw.update(sinkTokens=SINK_TOKENS, sinkLogits=self.logits)
        if kind == "decode":
            self.kw.pop("workspace", None)
            need = self.op.workspaceSize(**self.kw)
            self.kw.update(workspace=torch.empty(need, dtype=torch.uint8, device="cuda") if need else None)
        self.form = self.op.launchForm(**self.kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--rotate-bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    print("tools/sink_perf.py -- the windowed launch (w) at (n, W) against the same launch with %d sink tokens and sink logits (s); us per launch," % SINK_TOKENS)
    print("median of %d rounds (min .. max); bf16, D %d, Hq %d, Hkv %d, B %d full sequences; %s" % (
        args.rounds, wp.D, wp.HQ, wp.HKV, wp.B, torch.cuda.get_device_name(0)))
    for kind, R in (("decode", 1), ("prefill", 512)):
        for n, W in wp.SHAPES:
            arms = {"w": wp.Arm(kind, R, n, W, args.rotate_bytes), "s": SinkArm(kind, R, n, W, args.rotate_bytes)}
            res = wp.measure(arms, args.rounds, args.window_ms)
            tiles = -(-(W + R - 1) // 64) + 1
            print("%-7s R %4d  n %6d  W %5d   " % (kind, R, n, W) + "   ".join("(%s) %8.1f (%.1f .. %.1f)" % (a, *res[a]) for a in ("w", "s")) +
                  "   (s)/(w) %.3f   one more tile of %d: %.3f" % (res["s"][0] / res["w"][0], tiles, (tiles + 1) / tiles))
            print("        (s) " + arms["s"].form)
            del arms
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
