"""The prefill indexer (include/mfa_mla_index_prefill.h) at the shapes of a DeepSeek-V3.2 prompt chunk -- 64 index heads of 128, topk = 2048,
the last R rows of a context of C = 32768 index keys, causal -- beside what a caller had without it, in one process:

  (l) the logits launch    mfa_mla_index_prefill_logits_time
  (s) the select launch    mfa_mla_index_prefill_select_time, on the logits (l) wrote
  (x) the chained entry    mfa_mla_index_prefill_topk_time: passes of rows, the logits in the recommended workspace
  (a) the host loop the decode indexer allows: R / 32 calls of mfa_mla_index_topk_launch on 32 rows each, the cache lengths of call j
      faked to C - R + 32 (j + 1) so that the decode rule yields prefill's frontier
  (t) the torch composition of mla_index_perf.py -- einsum, ReLU, weighted sum, causal mask, topk -- on the first Rt rows, as many as keep
      its [B, Rt, Hi, C] FP32 intermediate within --torch-bytes; its figure is scaled by R / Rt

Every timed call is ONE call of an arm between two events, on a different copy of the index cache -- consecutive calls, whichever their
arms, rotate over at least --rotate-bytes of copies; the arms alternate call by call inside a round; a round's figure is the mean of its
calls, a cell's the median and min .. max of --rounds rounds.  Before timing, (a)'s lists are held equal to (x)'s, entry for entry.

    python tools/mla_index_prefill_perf.py > profiles/mla_index_prefill_perf.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from metal_flash_attention_amd import AttentionMLAIndex, AttentionMLAIndexPrefill, GEMMOperandPrecision as P  # noqa: E402

DI = 128
ARMS = ("l", "s", "x", "a", "t")


class Cell:
    """rotating copies of the index caches of B sequences of C keys, and the operands of every arm"""

    def __init__(self, B, C, H, R, topk, rotate_bytes, torch_bytes):
        self.B, self.C, self.H, self.R, self.topk = B, C, H, R, topk
        bf = torch.bfloat16
        self.copies = max(2, min(64, -(-rotate_bytes // (B * C * DI * 2))))
        self.ki = [torch.randn(B, C, DI, device="cuda", dtype=bf) for _ in range(self.copies)]
        self.qi = torch.randn(B, H, R, DI, device="cuda", dtype=bf)
        self.w = torch.randn(B, R, H, device="cuda") * H ** -0.5
        self.lengths = torch.full((B,), C, dtype=torch.int32, device="cuda")
        self.logits = torch.empty(B, R, C, device="cuda")
        self.indices = torch.empty(B, R, topk, device="cuda", dtype=torch.int32)
        self.index = AttentionMLAIndexPrefill(P.BF16)
        self.kw = dict(rows=R, column=C, indexHeads=H, batches=B, topk=topk, cacheLengths=self.lengths)
        self.ws = torch.empty(self.index.workspaceSize(**self.kw), dtype=torch.uint8, device="cuda")
        self.form = self.index.launchForm(workspace=self.ws, **self.kw)
        # ---- (a): 32 rows a call, each with its own lengths
        self.decode = AttentionMLAIndex(P.BF16)
        self.calls = -(-R // 32)
        self.faked = [torch.full((B,), C - R + min(32 * (j + 1), R), dtype=torch.int32, device="cuda") for j in range(self.calls)]
        self.loop_indices = torch.empty(B, R, topk, device="cuda", dtype=torch.int32)
        self.loop_ws = torch.empty(B * 32 * C * 4, dtype=torch.uint8, device="cuda")
        self.torch_rows = max(1, min(R, torch_bytes // (B * H * C * 4)))

    def loop(self, i, stream):
        """what the parent offers: the decode indexer's chain on 32 rows at a time, the operands read where they lie"""
        R, H, C, topk = self.R, self.H, self.C, self.topk
        for j in range(self.calls):
            rows = min(32, R - 32 * j)
            self.decode.dispatch(self.qi[:, :, 32 * j:], self.w[:, 32 * j:], self.ki[i], self.loop_indices[:, 32 * j:], stream=stream, rows=rows,
                                 column=C, indexHeads=H, batches=self.B, topk=topk, cacheLengths=self.faked[j], workspace=self.loop_ws,
                                 strides=dict(QI=(DI, R * DI, H * R * DI)), weightStrides=(H, R * H), indexStrides=(topk, R * topk))

    def torch_topk(self, i):
        """the composition as a caller writes it (a bf16 einsum), on the first torch_rows rows"""
        Rt, C, R = self.torch_rows, self.C, self.R
        s = torch.einsum("bhrd,bcd->brhc", self.qi[:, :, :Rt], self.ki[i]).float()
        logits = (torch.relu(s) * self.w[:, :Rt, :, None]).sum(dim=2)
        hidden = torch.arange(C, device="cuda")[None, :] > (torch.arange(Rt, device="cuda")[:, None] + C - R)
        return torch.topk(logits.masked_fill(hidden[None], float("-inf")), self.topk, dim=-1).indices

    def once(self, arm, i, stream):
        """microseconds of one call of an arm on copy i"""
        i %= self.copies
        if arm == "l":
            return 1e3 * self.index.time(self.qi, self.w, self.ki[i], self.logits, stage="logits", stream=stream, warmup=0, iterations=1, **self.kw)
        if arm == "s":
            return 1e3 * self.index.time(self.logits, self.indices, stage="select", stream=stream, warmup=0, iterations=1, **self.kw)
        if arm == "x":
            return 1e3 * self.index.time(self.qi, self.w, self.ki[i], self.indices, stage="topk", stream=stream, warmup=0, iterations=1,
                                         workspace=self.ws, **self.kw)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        if arm == "a":
            self.loop(i, stream)
        else:
            self.torch_topk(i)
        stop.record()
        stop.synchronize()
        return 1e3 * start.elapsed_time(stop) * (self.R / self.torch_rows if arm == "t" else 1.0)

    def check(self, stream):
        """(a)'s lists equal (x)'s on copy 0"""
        self.once("x", 0, stream)
        self.loop(0, stream)
        torch.cuda.synchronize()
        assert torch.equal(self.indices, self.loop_indices), "the loop of 32-row launches and the chained entry disagree"


def measure(cell, rounds, launches):
    """{arm: (median, min, max)} us per call; the arms alternate call by call, one warm-up pass first"""
    stream = torch.cuda.current_stream().cuda_stream
    for arm in ARMS:
        cell.once(arm, 0, stream)
    cell.check(stream)
    per = {arm: [] for arm in ARMS}
    at = 1
    for _ in range(rounds):
        took = {arm: 0.0 for arm in ARMS}
        for _i in range(launches):
            for arm in ARMS:
                took[arm] += cell.once(arm, at, stream)
                at += 1
        for arm in ARMS:
            per[arm].append(took[arm] / launches)
    return {arm: (statistics.median(x), min(x), max(x)) for arm, x in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--rotate-bytes", type=int, default=1 << 30)
    ap.add_argument("--torch-bytes", type=int, default=8 << 30)
    ap.add_argument("--column", type=int, default=32768)
    ap.add_argument("--topk", type=int, default=2048)
    ap.add_argument("--heads", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--rows", type=int, nargs="+", default=[64, 512, 4096])
    args = ap.parse_args()
    print("tools/mla_index_prefill_perf.py -- the prefill indexer, %d index heads, topk %d, the last R rows of %d keys, causal, bf16: the logits" % (
        args.heads, args.topk, args.column))
    print("launch (l), the select launch (s), the chained entry (x), against the loop of 32-row decode-indexer launches (a) and torch's einsum +")
    print("relu + weighted sum + topk on Rt rows scaled to R (t); us per call between two events, median of %d rounds of %d calls (min .. max);" % (
        args.rounds, args.launches))
    print("TFLOP/s: 2 x Hi x 128 x the visible (row, key) pairs over (l)'s median; %s" % torch.cuda.get_device_name(0))
    for B in args.batches:
        for R in args.rows:
            cell = Cell(B, args.column, args.heads, R, args.topk, args.rotate_bytes, args.torch_bytes)
            res = measure(cell, args.rounds, args.launches)
            pairs = B * sum(args.column - R + r + 1 for r in range(R))
            line = "B %2d  R %4d  Rt %4d  %d copies   " % (B, R, cell.torch_rows, cell.copies)
            line += "   ".join("(%s) %9.1f (%.1f .. %.1f)" % (arm, *res[arm]) for arm in ARMS)
            line += "   (l) %6.1f TFLOP/s   (a)/(x) %.2f   %s" % (2 * args.heads * DI * pairs / (res["l"][0] * 1e-6) / 1e12, res["a"][0] / res["x"][0], cell.form)
            print(line, flush=True)
            del cell
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
