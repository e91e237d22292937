"""The MLA sparse indexer (include/mfa_mla_index.h) at the shapes of DeepSeek-V3.2 decode -- 64 index heads of 128, topk = 2048 out of
a cache of C = 32768 index keys -- beside what a caller has without it, in one process:

  (l) the logits launch    mfa_mla_index_logits_time
  (s) the select launch    mfa_mla_index_select_time, on the logits (l) wrote
  (f) the chained entry    mfa_mla_index_topk_time: both kernels, the logits in a workspace
  (t) the torch composition on the same tensors: einsum of the index queries against every key, ReLU, the weighted sum over the heads,
      torch.topk -- four launches and a [B, R, Hi, C] FP32 intermediate

Every timed call is ONE call of an arm between two events, on a different copy of the index cache -- consecutive calls, whichever
their arms, rotate over at least --rotate-bytes of copies; the arms alternate call by call inside a round; a round's figure is the mean
of its calls, a cell's the median and min .. max of --rounds rounds.  Every sequence holds C keys.  Before timing, (f)'s lists are held
against (t)'s: the same SET of positions wherever the k-th and (k+1)-th logits differ by more than the two sums' rounding.

    python tools/mla_index_perf.py > profiles/mla_index_perf.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from metal_flash_attention_amd import AttentionMLAIndex, GEMMOperandPrecision as P  # noqa: E402

DI = 128
ARMS = ("l", "s", "f", "t")


class Cell:
    """rotating copies of the index caches of B sequences of C keys, and the operands of every arm"""

    def __init__(self, B, C, H, R, topk, rotate_bytes):
        self.B, self.C, self.H, self.R, self.topk = B, C, H, R, topk
        bf = torch.bfloat16
        self.copies = max(2, min(64, -(-rotate_bytes // (B * C * DI * 2))))
        self.ki = [torch.randn(B, C, DI, device="cuda", dtype=bf) for _ in range(self.copies)]
        self.qi = torch.randn(B, H, R, DI, device="cuda", dtype=bf)
        self.w = torch.randn(B, R, H, device="cuda") * H ** -0.5
        self.lengths = torch.full((B,), C, dtype=torch.int32, device="cuda")
        self.logits = torch.empty(B, R, C, device="cuda")
        self.indices = torch.empty(B, R, topk, device="cuda", dtype=torch.int32)
        self.index = AttentionMLAIndex(P.BF16)
        self.kw = dict(rows=R, column=C, indexHeads=H, batches=B, topk=topk, cacheLengths=self.lengths, causal=False)
        self.ws = torch.empty(self.index.workspaceSize(**self.kw), dtype=torch.uint8, device="cuda")
        self.form = self.index.launchForm(workspace=self.ws, **self.kw)

    def torch_topk(self, i, exact=False):
        """the composition as a caller writes it (a bf16 einsum); `exact`: on FP32 copies of the operands, for the check"""
        s = torch.einsum("bhrd,bcd->brhc", self.qi.float(), self.ki[i].float()) if exact else torch.einsum("bhrd,bcd->brhc", self.qi, self.ki[i]).float()
        logits = (torch.relu(s) * self.w[..., None]).sum(dim=2)
        return logits, torch.topk(logits, self.topk, dim=-1).indices

    def once(self, arm, i, stream):
        """microseconds of one call of an arm on copy i"""
        i %= self.copies
        if arm == "l":
            return 1e3 * self.index.time(self.qi, self.w, self.ki[i], self.logits, stage="logits", stream=stream, warmup=0, iterations=1, **self.kw)
        if arm == "s":
            return 1e3 * self.index.time(self.logits, self.indices, stage="select", stream=stream, warmup=0, iterations=1, **self.kw)
        if arm == "f":
            return 1e3 * self.index.time(self.qi, self.w, self.ki[i], self.indices, stage="topk", stream=stream, warmup=0, iterations=1,
                                         workspace=self.ws, **self.kw)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        self.torch_topk(i)
        stop.record()
        stop.synchronize()
        return 1e3 * start.elapsed_time(stop)

    def check(self, stream):
        """(f) against (t) on copy 0: every position torch keeps whose logit clears the k-th by a margin is in the list, and the reverse"""
        self.once("f", 0, stream)
        torch.cuda.synchronize()
        logits, theirs = self.torch_topk(0, exact=True)
        mine = self.indices.long()
        assert bool((mine >= 0).all()) and bool((mine[..., 1:] > mine[..., :-1]).all())
        kth = logits.gather(-1, theirs)[..., -1:]
        margin = 1e-3 * logits.abs().max()
        picked = torch.zeros_like(logits, dtype=torch.bool).scatter_(-1, mine, True)
        assert not bool(((logits > kth + margin) & ~picked).any()) and not bool(((logits < kth - margin) & picked).any())


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rotate-bytes", type=int, default=1 << 30)
    ap.add_argument("--column", type=int, default=32768)
    ap.add_argument("--topk", type=int, default=2048)
    ap.add_argument("--heads", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--rows", type=int, nargs="+", default=[1])
    args = ap.parse_args()
    print("tools/mla_index_perf.py -- the MLA indexer, %d index heads, topk %d out of %d keys, bf16: the logits launch (l), the select launch (s)," % (
        args.heads, args.topk, args.column))
    print("the chained entry (f), against torch's einsum + relu + weighted sum + topk on the same tensors (t); us per call between two events,")
    print("median of %d rounds of %d calls (min .. max); TB/s: the keys' bytes, B x C x 256, over (l)'s median; %s" % (
        args.rounds, args.launches, torch.cuda.get_device_name(0)))
    for B in args.batches:
        for R in args.rows:
            cell = Cell(B, args.column, args.heads, R, args.topk, args.rotate_bytes)
            res = measure(cell, args.rounds, args.launches)
            line = "B %2d  R %d  %d copies   " % (B, R, cell.copies)
            line += "   ".join("(%s) %7.1f (%.1f .. %.1f)" % (arm, *res[arm]) for arm in ARMS)
            line += "   (l) %5.2f TB/s   (f)/(t) %.2f   %s" % (B * args.column * DI * 2 / (res["l"][0] * 1e-6) / 1e12, res["f"][0] / res["t"][0], cell.form)
            print(line, flush=True)
            del cell
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
