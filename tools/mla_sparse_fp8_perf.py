"""Sparse MLA decode over an e4m3 latent cache (include/mfa_mla_sparse_fp8.h) at the shapes of DeepSeek-V3.2 decode -- topk = 2048 listed
keys a query token out of a cache of C = 32768 -- with the method of tools/mla_sparse_perf.py, beside the 16-bit launch it halves the
bytes of and beside what a caller of an e4m3 cache had before it, in one process:

  (x16) the 16-bit sparse launch (mfa_attention_mla_sparse_decode_time) over the SAME TOKENS as bf16 and the same lists: the yardstick
  (x8)  the new launch (mfa_attention_mla_sparse_decode_fp8_time) over the bytes                   -- attn_mla8x_d576_bf16[_k + _combine]
  (x8g) with --other-library PATH: (x8) from another build of the library in the same process (built with two steps of rows in flight,
        -DMFA_MLA8X_FLIGHT=2), launch by launch beside (x8)
  (t8)  torch.gather of the listed BYTES into a temporary [B R, topk, 576], then the dense e4m3 launch (mfa_attention_mla_decode_fp8) on
        it (B R sequences of one row; its Q is laid out beforehand, outside the timing): the same answer, what a caller had

Every timed call is ONE launch (arm (t8): the gather and the launch) between two events on a different copy of the cache -- consecutive
launches, whichever their arms, rotate over the copies, at least --rotate-bytes of them; the arms alternate launch by launch inside a
round; a round's figure is the mean of its launches, a cell's the median and min .. max of --rounds rounds.  Every sequence holds C keys;
a list is topk distinct positions drawn uniformly from them, in random order; the caches are contiguous.

    python tools/mla_sparse_fp8_perf.py [--other-library PATH] > profiles/mla_sparse_fp8_perf.txt
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from metal_flash_attention_amd import (AttentionMLADecodeFP8, AttentionMLASparseDecode, AttentionMLASparseDecodeFP8,  # noqa: E402
                                       GEMMOperandPrecision as P, _abi)
from metal_flash_attention_amd.attention import _pointers  # noqa: E402

DK, DV = 576, 512
SCALE, KV_SCALE = 0.1352337788608801, 0.37
E4M3 = torch.float8_e4m3fn


def random_bytes(*shape):
    """e4m3 bytes of magnitude <= 1 with a random sign: never 0x7f / 0xff"""
    return (torch.randint(0, 0x39, shape, device="cuda", dtype=torch.uint8) | (torch.randint(0, 2, shape, device="cuda", dtype=torch.uint8) << 7))


class Cell:
    """rotating copies of the two caches of B sequences of C keys -- the same tokens as bytes and as bf16 --, the lists and the operands"""

    def __init__(self, B, C, H, R, topk, rotate_bytes, other):
        self.B, self.C, self.H, self.R, self.topk = B, C, H, R, topk
        bf = torch.bfloat16
        self.copies = max(2, min(8, -(-rotate_bytes // (B * C * DK * 2))))
        self.kv8 = [random_bytes(B, C, DK).view(E4M3) for _ in range(self.copies)]
        self.kv16 = [kv.to(bf) * KV_SCALE for kv in self.kv8]   # (the product rounds to bf16: the check below is loose)
        # topk distinct positions below the causal frontier of row 0 (C - R), in random order
        self.lists = torch.rand(B, R, C - R, device="cuda").argsort(dim=-1)[:, :, :topk].to(torch.int32).contiguous()
        self.q = torch.randn(B, H, R, DK, device="cuda", dtype=bf)
        self.o = {arm: torch.empty(B, H, R, DV, device="cuda", dtype=bf) for arm in ("x16", "x8", "x8g")}
        self.l = torch.empty(B, H, R, device="cuda", dtype=torch.float32)
        self.lengths = torch.full((B,), C, dtype=torch.int32, device="cuda")
        self.kvscale = torch.tensor([KV_SCALE], dtype=torch.float32, device="cuda")
        self.x16, self.x8 = AttentionMLASparseDecode(P.BF16), AttentionMLASparseDecodeFP8(P.BF16)
        self.kw = dict(rows=R, column=C, heads=H, batches=B, scale=SCALE, cacheLengths=self.lengths, topk=topk, indices=self.lists)
        need, self.pieces = self.x16.plannedSplit(**self.kw)
        assert self.x8.plannedSplit(kvScale=self.kvscale, **self.kw) == (need, self.pieces)
        self.ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
        self.other = other
        # arm (t8): B R sequences of one row over the gathered bytes
        self.dense = AttentionMLADecodeFP8(P.BF16)
        self.tq = self.q.transpose(1, 2).reshape(B * R, H, 1, DK).contiguous()
        self.to = torch.empty(B * R, H, 1, DV, device="cuda", dtype=bf)
        self.tl = torch.empty(B * R, H, 1, device="cuda", dtype=torch.float32)
        self.tlengths = torch.full((B * R,), topk, dtype=torch.int32, device="cuda")
        self.tkw = dict(rows=1, column=topk, heads=H, batches=B * R, scale=SCALE, cacheLengths=self.tlengths, causal=False)
        tneed, self.tpieces = self.dense.plannedSplit(**self.tkw)
        self.tws = torch.empty(max(tneed, 16), dtype=torch.uint8, device="cuda")
        self.gather = self.lists.long().view(B, R * topk, 1).expand(B, R * topk, DK)

    def once(self, arm, i, stream):
        """microseconds of one launch of an arm on copy i"""
        i %= self.copies
        if arm == "x16":
            return 1e3 * self.x16.time(self.q, self.kv16[i], self.o[arm], self.l, stream=stream, warmup=0, iterations=1, workspace=self.ws, **self.kw)
        if arm == "x8":
            return 1e3 * self.x8.time(self.q, self.kv8[i], self.o[arm], self.l, stream=stream, warmup=0, iterations=1, workspace=self.ws,
                                      kvScale=self.kvscale, **self.kw)
        if arm == "x8g":   # the other library's entry over this library's blocks
            shape = dict(self.kw, workspace=self.ws, kvScale=self.kvscale)
            own, _kept = self.x8._own(shape)
            p, _keep = self.x8._params(**shape)
            ms = ctypes.c_float(0.0)
            status = self.other(*_pointers(self.q, self.kv8[i], self.o[arm], self.l), ctypes.byref(p), *own, ctypes.c_void_p(stream), 0, 1,
                                ctypes.byref(ms))
            assert status == 0, status
            return 1e3 * float(ms.value)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        tmp = torch.gather(self.kv8[i].view(torch.uint8), 1, self.gather).view(self.B * self.R, self.topk, DK).view(E4M3)
        self.dense.dispatch(self.tq, tmp, self.to, self.tl, stream=stream, workspace=self.tws, kvScale=self.kvscale, **self.tkw)
        stop.record()
        stop.synchronize()
        return 1e3 * start.elapsed_time(stop)


def measure(cell, arms, rounds, launches):
    """{arm: (median, min, max)} us per launch; the arms alternate launch by launch, one warm-up pass first on copy 0"""
    stream = torch.cuda.current_stream().cuda_stream
    for arm in arms:
        cell.once(arm, 0, stream)
    torch.cuda.synchronize()
    # the arms compute the same attention on copy 0, in another order of sums -- loosely; the tests hold the launch to its bounds
    want = cell.to.view(cell.B, cell.R, cell.H, DV).transpose(1, 2).float()
    for arm in arms[:-1]:
        err = (cell.o[arm].float() - want).abs().max().item()
        assert err < 2e-2, (arm, err)
    if "x8g" in arms:   # two builds of one body: the same bits
        assert torch.equal(cell.o["x8g"].view(torch.int16), cell.o["x8"].view(torch.int16))
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
    ap.add_argument("--column", type=int, default=32768)
    ap.add_argument("--topk", type=int, default=2048)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--heads", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--other-library", default=None, help="another build of libmfa_hip.so whose sparse e4m3 launch is arm (x8g)")
    ap.add_argument("--other-name", default="a build with -DMFA_MLA8X_FLIGHT=2")
    args = ap.parse_args()
    other = None
    if args.other_library:
        handle = ctypes.CDLL(args.other_library)
        other = handle.mfa_attention_mla_sparse_decode_fp8_time
        other.restype, other.argtypes = next((r, a) for n, r, a in _abi.MLA_SPARSE_FP8_SYMBOLS if n == "mfa_attention_mla_sparse_decode_fp8_time")
    arms = ("x16", "x8") + (("x8g",) if other else ()) + ("t8",)
    print("tools/mla_sparse_fp8_perf.py -- sparse MLA decode over random lists of %d keys out of %d: the 16-bit launch (x16), the e4m3 launch over the" % (
        args.topk, args.column))
    print("same tokens as bytes (x8)%s, and torch.gather of the bytes + the dense e4m3 launch (t8); bf16 Q; us per launch between two events," % (
        ", (x8g): (x8) of %s" % args.other_name if other else ""))
    print("median of %d rounds of %d launches (min .. max); TB/s: listed bytes, B x R x topk x 576, over (x8)'s median; %s" % (
        args.rounds, args.launches, torch.cuda.get_device_name(0)))
    for B in args.batches:
        for H in args.heads:
            for R in args.rows:
                cell = Cell(B, args.column, H, R, args.topk, args.rotate_bytes, other)
                res = measure(cell, arms, args.rounds, args.launches)
                line = "B %2d  H %3d  R %d  pieces %2d (t8: %2d)  %d copies   " % (B, H, R, cell.pieces, cell.tpieces, cell.copies)
                line += "   ".join("(%s) %7.1f (%.1f .. %.1f)" % (arm, *res[arm]) for arm in arms)
                line += "   %5.2f TB/s   (x8)/(x16) %.2f   (x8)/(t8) %.2f  (x8) spread %.2f .. %.2f  (t8) spread %.2f .. %.2f" % (
                    B * R * args.topk * DK / (res["x8"][0] * 1e-6) / 1e12, res["x8"][0] / res["x16"][0], res["x8"][0] / res["t8"][0],
                    res["x8"][1] / res["x8"][0], res["x8"][2] / res["x8"][0], res["t8"][1] / res["t8"][0], res["t8"][2] / res["t8"][0])
                if other:
                    line += "   (x8g)/(x8) %.2f" % (res["x8g"][0] / res["x8"][0])
                print(line, flush=True)
                del cell
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
