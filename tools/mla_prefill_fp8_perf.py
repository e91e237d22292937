"""MLA prefill over an e4m3 latent cache (include/mfa_mla_prefill_fp8.h) at the shapes of a serving loop's chunked prefill -- `rows` new
rows per sequence behind a prefix that is in the cache already -- beside what a caller with such a cache could do without it, and beside
the 16-bit launch over a 16-bit copy of the same cache, in one process (the protocol of tools/mla_prefill_perf.py):

  (f1)  the new launch at one piece, one mfa_attention_mla_prefill_fp8_launch
  (fp)  the new launch at the host's plan, mfa_attention_mla_prefill_fp8_split_launch with pieces = 0 and the workspace it asks for
  (c8)  the only route there was for an e4m3 cache: ceil(rows / 32) mfa_attention_mla_decode_fp8_launch calls of 32 rows each with the
        lengths advanced, at the host's plan
  (n16) mfa_attention_mla_prefill_split_launch at the host's plan over a bf16 copy of the cache (kvScale = 0.5: the copy holds the very
        values the bytes stand for, and (f1) and (n16) are compared on the warm-up pass)

--parent-lib names the library the decode launches of (c8) are taken from: the PARENT commit's build is the yardstick, not the code
under test (this change touches none of decode's translation units; without the option the arm runs this build's decode and the header
line says so).

Every timed call is one whole route between two events on a different copy of the cache -- consecutive calls, whichever their arms,
rotate over the copies, at least --rotate-bytes of 16-bit cache -- the arms alternate call by call inside a round; a round's figure is
the mean of its calls, a cell's the median and min .. max of --rounds rounds.  The calls of a round are as many as fit --round-ms per arm
(at least 1, at most --launches).  bf16 Q, causal, contiguous caches.  (f) below is the better of (f1) and (fp); (n16) is already at its
plan, which is (fp)'s: (fp)/(n16) is kernel against kernel -- what the e4m3 read buys a prefill, against the 0.76 - 0.78 the e4m3 decode
step reaches.

    python tools/mla_prefill_fp8_perf.py --parent-lib PARENT/libmfa_hip.so > profiles/mla_prefill_fp8_perf.txt
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from metal_flash_attention_amd import (AttentionMLADecodeFP8, AttentionMLAPrefillFP8, AttentionMLAPrefillFP8Split, AttentionMLAPrefillSplit,  # noqa: E402
                                       GEMMOperandPrecision as P, _abi, dequantizeE4M3)

DK, DV, CHUNK = 576, 512, 32
SCALE, KV_SCALE = 0.1352337788608801, 0.5
ARMS = ("f1", "fp", "c8", "n16")


class Decode8:
    """mfa_attention_mla_decode_fp8_launch / _workspace_size of a library: this build's, or the one --parent-lib names"""

    def __init__(self, path):
        self.lib = _abi.lib() if path is None else ctypes.CDLL(path)
        self.host = AttentionMLADecodeFP8(P.BF16)
        for name in ("mfa_attention_mla_decode_fp8_launch", "mfa_attention_mla_decode_fp8_workspace_size"):
            fn, mine = getattr(self.lib, name), getattr(_abi.lib(), name)
            fn.restype, fn.argtypes = mine.restype, mine.argtypes

    def workspace(self, p, quant):
        need, pieces = ctypes.c_uint64(0), ctypes.c_uint32(0)
        assert self.lib.mfa_attention_mla_decode_fp8_workspace_size(ctypes.byref(p), ctypes.byref(quant), ctypes.byref(need), ctypes.byref(pieces)) == 0
        return int(need.value), int(pieces.value)

    def launch(self, q, kv, o, l, p, quant, stream):
        st = self.lib.mfa_attention_mla_decode_fp8_launch(q, kv, o, l, ctypes.byref(p), ctypes.byref(quant), ctypes.c_void_p(stream))
        assert st == 0, st


class Cell:
    """rotating copies of the e4m3 cache of B sequences of prefix + rows keys and of its bf16 copy, and the operands of every arm"""

    def __init__(self, B, H, rows, prefix, rotate_bytes, decode):
        self.B, self.H, self.rows, self.prefix, self.decode = B, H, rows, prefix, decode
        bf = torch.bfloat16
        self.C = C = prefix + rows
        self.copies = max(2, min(8, -(-rotate_bytes // (B * C * DK * 2))))
        lut = torch.tensor([dequantizeE4M3(b) * KV_SCALE for b in range(256)], dtype=torch.float32, device="cuda")
        self.kv8, self.kv16 = [], []
        for _ in range(self.copies):   # bytes of magnitude <= 1.0 with a random sign (never 0x7f / 0xff), and the values they stand for
            b8 = (torch.randint(0, 0x39, (B, C, DK), device="cuda", dtype=torch.uint8) | (torch.randint(0, 2, (B, C, DK), device="cuda", dtype=torch.uint8) << 7))
            self.kv8.append(b8.view(torch.float8_e4m3fn))
            self.kv16.append(torch.stack([lut[b8[b].long()].to(bf) for b in range(B)]))
        self.q = torch.randn(B, H, rows, DK, device="cuda", dtype=bf)
        self.o = torch.empty(B, H, rows, DV, device="cuda", dtype=bf)
        self.o16 = torch.empty(B, H, rows, DV, device="cuda", dtype=bf)
        self.l = torch.empty(B, H, rows, device="cuda", dtype=torch.float32)
        self.lengths = torch.full((B,), C, dtype=torch.int32, device="cuda")
        self.kvs = torch.tensor([KV_SCALE], dtype=torch.float32, device="cuda")
        kw = dict(rows=rows, column=C, heads=H, batches=B, scale=SCALE, cacheLengths=self.lengths)
        self.f1, self.fp, self.n16 = AttentionMLAPrefillFP8(P.BF16), AttentionMLAPrefillFP8Split(P.BF16), AttentionMLAPrefillSplit(P.BF16)
        need8, self.pieces = self.fp.plannedSplit(kvScale=self.kvs, **kw)
        need16, pieces16 = self.n16.plannedSplit(**kw)
        assert (need8, self.pieces) == (need16, pieces16)
        # arm (c8): a decode launch per 32 rows, the lengths advanced; Q, O and L are read and written where they lie
        ends = torch.stack([torch.full((B,), prefix + min(r0 + CHUNK, rows), dtype=torch.int32) for r0 in range(0, rows, CHUNK)]).cuda()
        strides = dict(Q=(DK, rows * DK, H * rows * DK), O=(DV, rows * DV, H * rows * DV))
        self.quant = _abi.mfa_mla_quant()
        _abi.lib().mfa_mla_quant_init(ctypes.byref(self.quant))
        self.quant.kvScale = self.kvs.data_ptr()
        self.chunks, need = [], need8
        for j, r0 in enumerate(range(0, rows, CHUNK)):
            plan = decode.host._params(rows=min(CHUNK, rows - r0), column=C, heads=H, batches=B, scale=SCALE, cacheLengths=ends[j], strides=strides,
                                       lStrides=(rows, H * rows), pieces=0)[0]
            nbytes, self.decode_pieces = decode.workspace(plan, self.quant)   # (kept: the plan of the last chunk, the longest cache)
            need = max(need, nbytes)
            self.chunks.append(((self.q.data_ptr() + r0 * DK * 2, self.o.data_ptr() + r0 * DV * 2, self.l.data_ptr() + r0 * 4), plan))
        self.ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
        for _at, plan in self.chunks:
            plan.workspace, plan.workspaceBytes = self.ws.data_ptr(), need
        self.ends = ends
        self.kw = kw

    def pairs(self):
        return self.rows * self.prefix + self.rows * (self.rows + 1) // 2

    def once(self, arm, i, stream):
        """microseconds of one route of an arm on copy i"""
        i %= self.copies
        if arm == "f1":
            return 1e3 * self.f1.time(self.q, self.kv8[i], self.o, self.l, stream=stream, warmup=0, iterations=1, kvScale=self.kvs, **self.kw)
        if arm == "fp":
            return 1e3 * self.fp.time(self.q, self.kv8[i], self.o, self.l, stream=stream, warmup=0, iterations=1, kvScale=self.kvs, workspace=self.ws, **self.kw)
        if arm == "n16":
            return 1e3 * self.n16.time(self.q, self.kv16[i], self.o16, self.l, stream=stream, warmup=0, iterations=1, workspace=self.ws, **self.kw)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for (qp, op, lp), plan in self.chunks:
            self.decode.launch(qp, self.kv8[i].data_ptr(), op, lp, plan, self.quant, stream)
        stop.record()
        stop.synchronize()
        return 1e3 * start.elapsed_time(stop)


def measure(cell, rounds, launches, round_ms, arms=ARMS):
    """{arm: (median, min, max)} us per route; the arms alternate call by call, one warm-up pass first"""
    stream = torch.cuda.current_stream().cuda_stream
    first, outs = {}, {}
    for arm in arms:
        first[arm] = cell.once(arm, 0, stream)
        torch.cuda.synchronize()
        outs[arm] = (cell.o16 if arm == "n16" else cell.o).float().clone()
    # the routes compute the same attention over the same values on copy 0, in other orders of sums -- loosely; the tests hold the bounds
    for arm in arms[1:]:
        err = (outs[arm] - outs[arms[0]]).abs().max().item()
        assert err < 3e-2, (arm, err)
    calls = max(1, min(launches, int(round_ms * 1e3 / max(first.values()))))
    per = {arm: [] for arm in arms}
    at = 1
    for _ in range(rounds):
        took = {arm: 0.0 for arm in arms}
        for _i in range(calls):
            for arm in arms:
                took[arm] += cell.once(arm, at, stream)
                at += 1
        for arm in arms:
            per[arm].append(took[arm] / calls)
    return {arm: (statistics.median(x), min(x), max(x)) for arm, x in per.items()}, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--round-ms", type=float, default=150.0)
    ap.add_argument("--rotate-bytes", type=int, default=1 << 30)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--heads", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--rows", type=int, nargs="+", default=[64, 512, 2048])
    ap.add_argument("--prefix", type=int, nargs="+", default=[0, 4096, 32768])
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    decode = Decode8(args.parent_lib)
    print("tools/mla_prefill_fp8_perf.py -- MLA prefill over an e4m3 latent cache: the new launch at one piece (f1) and at the host's plan (fp;")
    print("pieces) against ceil(rows / 32) e4m3 decode launches with the lengths advanced at the host's plan (c8; dpieces: the last chunk's) and")
    print("the 16-bit prefill at the host's plan over a bf16 copy of the cache (n16); bf16 Q, causal, contiguous caches of prefix + rows keys,")
    print("kvScale 0.5; us per route between two events, median of %d rounds (min .. max) of up to %d calls; (f) = the better of (f1), (fp);" % (
        args.rounds, args.launches))
    print("decode launches from %s; %s" % ("the parent commit's library" if args.parent_lib else "THIS build (its decode units are the parent's)",
                                           torch.cuda.get_device_name(0)))
    for B in args.batches:
        for H in args.heads:
            for rows in args.rows:
                for prefix in args.prefix:
                    cell = Cell(B, H, rows, prefix, args.rotate_bytes, decode)
                    res, calls = measure(cell, args.rounds, args.launches, args.round_ms)
                    f = min(res["f1"][0], res["fp"][0])
                    flops = 2.0 * (DK + DV) * cell.pairs() * H * B
                    line = "B %d  H %3d  rows %4d  prefix %5d  blocks %5d  pieces %2d  dpieces %2d  %d copies  %2d calls   " % (
                        B, H, rows, prefix, B * -(-rows * H // 64), cell.pieces, cell.decode_pieces, cell.copies, calls)
                    line += "   ".join("(%s) %9.1f (%.1f .. %.1f)" % (arm, *res[arm]) for arm in ARMS)
                    line += "   (f) %6.1f TFLOP/s   (c8)/(f) %5.2f   (f)/(n16) %5.2f   (fp)/(n16) %5.2f" % (
                        flops / (f * 1e-6) / 1e12, res["c8"][0] / f, f / res["n16"][0], res["fp"][0] / res["n16"][0])
                    print(line, flush=True)
                    del cell
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
