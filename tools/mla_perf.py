"""Multi-head latent attention decode over a compressed cache (include/mfa_mla.h) at the shapes of DeepSeek-V2 / V3 decode, beside the two
things it can be held against in one process -- the parent commit has no path at this width:

  (m)  the MLA launch over a contiguous cache [B, C, 576], through mfa_attention_mla_decode_time       -- attn_mla16_d576_bf16[_k + _combine]
  (p)  the same over a paged cache (pages of 64 keys, shuffled pool)
  (d)  flash_decode's launch at D = 256, G = 8, one K/V head, over the SAME NUMBER OF CACHE BYTES a sequence (C x 1152 / 1024 keys of
       K and V), through mfa_attention_decode_time: the library's own decode kernel as the yardstick of bytes per second
  (t)  the same attention composed from torch matmuls (bmm, softmax in FP32, bmm over the cache's first 512 columns): what a user has today

Every timed call is ONE launch (arm (t): its torch kernels) between two events on a different copy of the cache -- consecutive launches,
whichever their arms, rotate over the copies, at least --rotate-bytes of them --; the arms alternate launch by launch inside a round; a
round's figure is the mean of its launches, a cell's the median and min .. max of --rounds rounds.  Every sequence holds C keys.  Unique
bytes per second counts each cache byte once: B x C x 1152 over the time, whatever the number of workgroups that read it.

    python tools/mla_perf.py > profiles/mla_perf.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from metal_flash_attention_amd import AttentionDecode, AttentionMLADecode, GEMMOperandPrecision as P  # noqa: E402

DK, DV, PAGE = 576, 512, 64
SCALE = 0.1352337788608801
DD, DG = 256, 8                      # arm (d): head dimension, query heads on its one K/V head


class Cell:
    """rotating copies of the caches of B sequences of C keys and the operands of every arm"""

    def __init__(self, B, C, H, rotate_bytes):
        self.B, self.C, self.H = B, C, H
        self.bytes = B * C * DK * 2
        self.copies = max(2, min(16, -(-rotate_bytes // self.bytes)))
        bf = torch.bfloat16
        self.kv = [(torch.randn(B, C, DK, device="cuda", dtype=bf) * 0.5) for _ in range(self.copies)]
        pages = B * C // PAGE
        self.pool = [kv.view(pages, PAGE, DK) for kv in self.kv]                        # the same bytes, named through a shuffled table
        self.table = torch.randperm(pages, device="cuda").to(torch.int32).view(B, C // PAGE)
        self.q = torch.randn(B, H, 1, DK, device="cuda", dtype=bf)
        self.o = torch.empty(B, H, 1, DV, device="cuda", dtype=bf)
        self.l = torch.empty(B, H, 1, device="cuda", dtype=torch.float32)
        self.lengths = torch.full((B,), C, dtype=torch.int32, device="cuda")
        self.mla = AttentionMLADecode(P.BF16)
        self.kw = dict(rows=1, column=C, heads=H, batches=B, scale=SCALE, cacheLengths=self.lengths)
        self.paged_kw = dict(self.kw, pageSize=PAGE, blockTable=self.table, blockTableStride=C // PAGE)
        need, self.pieces = self.mla.plannedSplit(**self.kw)
        self.ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
        assert self.mla.plannedSplit(**self.paged_kw) == (need, self.pieces)
        # arm (d): one K/V head of D = 256 holding the same bytes a sequence, K and V together
        self.Cd = C * DK * 2 // (2 * DD * 2)
        self.dk = [torch.randn(B, 1, self.Cd, DD, device="cuda", dtype=bf) * 0.5 for _ in range(self.copies)]
        self.dv = [torch.randn(B, 1, self.Cd, DD, device="cuda", dtype=bf) * 0.5 for _ in range(self.copies)]
        self.dq = torch.randn(B, DG, 1, DD, device="cuda", dtype=bf)
        self.do = torch.empty(B, DG, 1, DD, device="cuda", dtype=bf)
        self.dl = torch.empty(B, DG, 1, device="cuda", dtype=torch.float32)
        self.dlengths = torch.full((B,), self.Cd, dtype=torch.int32, device="cuda")
        self.decode = AttentionDecode(DD, P.BF16)
        self.dkw = dict(rows=1, column=self.Cd, heads=DG, batches=B, headsPerKeyValue=DG, cacheLengths=self.dlengths)
        dneed = self.decode.workspaceSize(**self.dkw)
        self.dws = torch.empty(max(dneed, 16), dtype=torch.uint8, device="cuda")
        self.dpieces = dneed // (B * DG * (DD + 2) * 4)

    def once(self, arm, i, stream):
        """microseconds of one launch of an arm on copy i"""
        i %= self.copies
        if arm == "m":
            return 1e3 * self.mla.time(self.q, self.kv[i], self.o, self.l, stream=stream, warmup=0, iterations=1, workspace=self.ws, **self.kw)
        if arm == "p":
            return 1e3 * self.mla.time(self.q, self.pool[i], self.o, self.l, stream=stream, warmup=0, iterations=1, workspace=self.ws, **self.paged_kw)
        if arm == "d":
            return 1e3 * self.decode.time(self.dq, self.dk[i], self.dv[i], self.do, self.dl, stream=stream, warmup=0, iterations=1,
                                          workspace=self.dws, **self.dkw)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        kv = self.kv[i]
        s = torch.bmm(self.q.view(self.B, self.H, DK), kv.transpose(1, 2))
        w = torch.softmax(s.float() * SCALE, dim=-1).to(torch.bfloat16)
        self.torch_o = torch.bmm(w, kv[:, :, :DV])
        stop.record()
        stop.synchronize()
        return 1e3 * start.elapsed_time(stop)


def measure(cell, rounds, launches):
    """{arm: (median, min, max)} us per launch; the arms alternate launch by launch, one warm-up pass first"""
    stream = torch.cuda.current_stream().cuda_stream
    arms = ("m", "p", "d", "t")
    for arm in arms:
        cell.once(arm, 0, stream)
    cell.once("m", 0, stream)   # (the paged arm reads the pool through its shuffled table: other keys a sequence, and it writes the same O)
    torch.cuda.synchronize()
    # the arms compute the same thing: (m) against (t), loosely -- the tests hold (m) to its bounds
    err = (cell.o.float().view(cell.B, cell.H, DV) - cell.torch_o.float()).abs().max().item()
    assert err < 2e-2, err
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rotate-bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    print("tools/mla_perf.py -- MLA decode over a compressed cache, contiguous (m) and in pages of %d keys (p), against the D = 256, G = 8 decode" % PAGE)
    print("launch over the same cache bytes (d) and the same attention from torch matmuls (t); R = 1, bf16, every sequence C keys; us per launch")
    print("between two events, median of %d rounds of %d launches (min .. max); TB/s: unique cache bytes, B x C x 1152, over the median; %s" % (
        args.rounds, args.launches, torch.cuda.get_device_name(0)))
    seen = {}
    for B in (1, 8, 64):
        for C in (4096, 32768):
            for H in (16, 128):
                cell = Cell(B, C, H, args.rotate_bytes)
                res = measure(cell, args.rounds, args.launches)
                tb = lambda arm: cell.bytes / (res[arm][0] * 1e-6) / 1e12  # noqa: E731
                seen[(B, C, H)] = res["m"][0]
                line = "B %2d  C %5d  H %3d  %2d pieces (d: %2d)  %2d copies   " % (B, C, H, cell.pieces, cell.dpieces, cell.copies)
                line += "   ".join("(%s) %8.1f (%.1f .. %.1f) %5.2f TB/s" % (arm, *res[arm], tb(arm)) for arm in ("m", "p", "d"))
                line += "   (t) %9.1f (%.1f .. %.1f)   (m)/(d) %.2f   (t)/(m) %.1f" % (*res["t"], res["m"][0] / res["d"][0], res["t"][0] / res["m"][0])
                if H == 128:
                    line += "   H 128 / H 16: %.2f" % (res["m"][0] / seen[(B, C, 16)])
                print(line, flush=True)
                del cell
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
