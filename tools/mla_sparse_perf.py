"""Sparse MLA decode (include/mfa_mla_sparse.h) at the shapes of DeepSeek-V3.2 decode -- topk = 2048 listed keys a query token out of a
cache of C = 32768 -- beside the two things a caller could do without it, in one process:

  (xs) the sparse launch, SORTED lists, contiguous cache [B, C, 576], through mfa_attention_mla_sparse_decode_time
  (xr) the same with the lists in RANDOM order
  (xp) random lists over a paged cache (pages of 64 keys, shuffled pool)
  (m)  the dense MLA launch (mfa_attention_mla_decode_time) over a cache of C = topk keys: the same number of rows walked by the code
       that existed before -- NOT the same answer; the yardstick of what a walk of 2048 rows costs
  (t)  torch.gather of the listed rows into a temporary [B R, topk, 576], then (m)'s launch on it (B R sequences of one row; its Q is
       laid out beforehand, outside the timing): the same answer, what a caller has without this entry

Every timed call is ONE launch (arm (t): the gather and the launch) between two events on a different copy of the cache -- consecutive
launches, whichever their arms, rotate over the copies, at least --rotate-bytes of them; the arms alternate launch by launch inside a
round; a round's figure is the mean of its launches, a cell's the median and min .. max of --rounds rounds.  Every sequence holds C keys;
a list is topk distinct positions drawn uniformly from them.

    python tools/mla_sparse_perf.py > profiles/mla_sparse_perf.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from metal_flash_attention_amd import AttentionMLADecode, AttentionMLASparseDecode, GEMMOperandPrecision as P  # noqa: E402

DK, DV, PAGE = 576, 512, 64
SCALE = 0.1352337788608801
ARMS = ("xs", "xr", "xp", "m", "t")


class Cell:
    """rotating copies of the caches of B sequences of C keys, the lists and the operands of every arm"""

    def __init__(self, B, C, H, R, topk, rotate_bytes):
        self.B, self.C, self.H, self.R, self.topk = B, C, H, R, topk
        bf = torch.bfloat16
        self.copies = max(2, min(8, -(-rotate_bytes // (B * C * DK * 2))))
        self.kv = [(torch.randn(B, C, DK, device="cuda", dtype=bf) * 0.5) for _ in range(self.copies)]
        pages = B * C // PAGE
        self.pool = [kv.view(pages, PAGE, DK) for kv in self.kv]                        # the same bytes, named through a shuffled table
        self.table = torch.randperm(pages, device="cuda").to(torch.int32).view(B, C // PAGE)
        # topk distinct positions below the causal frontier of row 0 (C - R), in random order and sorted
        self.random = torch.rand(B, R, C - R, device="cuda").argsort(dim=-1)[:, :, :topk].to(torch.int32).contiguous()
        self.sorted = self.random.sort(dim=-1).values.contiguous()
        self.q = torch.randn(B, H, R, DK, device="cuda", dtype=bf)
        self.o = torch.empty(B, H, R, DV, device="cuda", dtype=bf)
        self.l = torch.empty(B, H, R, device="cuda", dtype=torch.float32)
        self.lengths = torch.full((B,), C, dtype=torch.int32, device="cuda")
        self.sparse = AttentionMLASparseDecode(P.BF16)
        self.kw = dict(rows=R, column=C, heads=H, batches=B, scale=SCALE, cacheLengths=self.lengths, topk=topk)
        self.paged_kw = dict(self.kw, pageSize=PAGE, blockTable=self.table, blockTableStride=C // PAGE)
        need, self.pieces = self.sparse.plannedSplit(indices=self.random, **self.kw)
        self.ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
        # arm (m): the dense launch over caches of topk keys
        self.dense = AttentionMLADecode(P.BF16)
        self.mkv = [(torch.randn(B, topk, DK, device="cuda", dtype=bf) * 0.5) for _ in range(self.copies)]
        self.mlengths = torch.full((B,), topk, dtype=torch.int32, device="cuda")
        self.mkw = dict(rows=R, column=topk, heads=H, batches=B, scale=SCALE, cacheLengths=self.mlengths)
        mneed, self.mpieces = self.dense.plannedSplit(**self.mkw)
        self.mws = torch.empty(max(mneed, 16), dtype=torch.uint8, device="cuda")
        # arm (t): B R sequences of one row over the gathered rows
        self.tq = self.q.transpose(1, 2).reshape(B * R, H, 1, DK).contiguous()
        self.to = torch.empty(B * R, H, 1, DV, device="cuda", dtype=bf)
        self.tl = torch.empty(B * R, H, 1, device="cuda", dtype=torch.float32)
        self.tlengths = torch.full((B * R,), topk, dtype=torch.int32, device="cuda")
        self.tkw = dict(rows=1, column=topk, heads=H, batches=B * R, scale=SCALE, cacheLengths=self.tlengths, causal=False)
        tneed, self.tpieces = self.dense.plannedSplit(**self.tkw)
        self.tws = torch.empty(max(tneed, 16), dtype=torch.uint8, device="cuda")
        self.gather = self.random.long().view(B, R * topk, 1).expand(B, R * topk, DK)

    def once(self, arm, i, stream):
        """microseconds of one launch of an arm on copy i"""
        i %= self.copies
        if arm in ("xs", "xr"):
            return 1e3 * self.sparse.time(self.q, self.kv[i], self.o, self.l, stream=stream, warmup=0, iterations=1, workspace=self.ws,
                                          indices=self.sorted if arm == "xs" else self.random, **self.kw)
        if arm == "xp":
            return 1e3 * self.sparse.time(self.q, self.pool[i], self.o, self.l, stream=stream, warmup=0, iterations=1, workspace=self.ws,
                                          indices=self.random, **self.paged_kw)
        if arm == "m":
            return 1e3 * self.dense.time(self.q, self.mkv[i], self.o, self.l, stream=stream, warmup=0, iterations=1, workspace=self.mws, **self.mkw)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        tmp = torch.gather(self.kv[i], 1, self.gather).view(self.B * self.R, self.topk, DK)
        self.dense.dispatch(self.tq, tmp, self.to, self.tl, stream=stream, workspace=self.tws, **self.tkw)
        stop.record()
        stop.synchronize()
        return 1e3 * start.elapsed_time(stop)


def measure(cell, rounds, launches):
    """{arm: (median, min, max)} us per launch; the arms alternate launch by launch, one warm-up pass first"""
    stream = torch.cuda.current_stream().cuda_stream
    for arm in ARMS:
        cell.once(arm, 0, stream)
    cell.once("xr", 0, stream)
    torch.cuda.synchronize()
    # (xr) and (t) compute the same thing on copy 0, in another order of sums -- loosely; the tests hold the launch to its bounds
    want = cell.to.view(cell.B, cell.R, cell.H, DV).transpose(1, 2).float()
    err = (cell.o.float() - want).abs().max().item()
    assert err < 2e-2, err
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
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--heads", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 2])       # (one cell: what a kernel trace in a run of its own is taken on)
    args = ap.parse_args()
    print("tools/mla_sparse_perf.py -- sparse MLA decode over lists of %d keys out of %d: sorted lists (xs), random lists (xr), random lists over" % (
        args.topk, args.column))
    print("pages of %d keys (xp), against the dense MLA launch over a cache of %d keys (m) and torch.gather + that launch (t); bf16; us per launch" % (
        PAGE, args.topk))
    print("between two events, median of %d rounds of %d launches (min .. max); TB/s: listed bytes, B x R x topk x 1152, over (xr)'s median; %s" % (
        args.rounds, args.launches, torch.cuda.get_device_name(0)))
    for B in args.batches:
        for H in args.heads:
            for R in args.rows:
                cell = Cell(B, args.column, H, R, args.topk, args.rotate_bytes)
                res = measure(cell, args.rounds, args.launches)
                line = "B %2d  H %3d  R %d  pieces %2d (m: %2d, t: %2d)  %d copies   " % (B, H, R, cell.pieces, cell.mpieces, cell.tpieces, cell.copies)
                line += "   ".join("(%s) %7.1f (%.1f .. %.1f)" % (arm, *res[arm]) for arm in ARMS)
                line += "   %5.2f TB/s   (xr)/(m) %.2f  (m) spread %.2f .. %.2f   (xs)/(xr) %.2f   (xp)/(xr) %.2f   (xr)/(t) %.2f" % (
                    B * R * args.topk * DK * 2 / (res["xr"][0] * 1e-6) / 1e12, res["xr"][0] / res["m"][0], res["m"][1] / res["m"][0],
                    res["m"][2] / res["m"][0], res["xs"][0] / res["xr"][0], res["xp"][0] / res["xr"][0], res["xr"][0] / res["t"][0])
                print(line, flush=True)
                del cell
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
