"""MLA prefill over the latent cache (include/mfa_mla_prefill.h) at the shapes of a serving loop's chunked prefill -- `rows` new rows per
sequence behind a prefix that is in the cache already -- beside the two things a caller could do without it, in one process:

  (n)  the new launch, one mfa_attention_mla_prefill_launch
  (c1) the only route there was: ceil(rows / 32) mfa_attention_mla_decode_launch calls of 32 rows each with the lengths advanced, UNSPLIT
  (cp) the same at the host's plan (pieces = 0 with the workspace the library asks for)
  (t)  torch: bmm + causal mask + softmax + bmm over the absorbed form, a sequence (and, where the scores would not fit, a group of
       heads) at a time

--parent-lib names the library the decode launches of (c1) / (cp) are taken from: the PARENT commit's build is the yardstick, not the
code under test (this change touches none of decode's translation units; without the option the arms run this build's decode and the
header line says so).

Every timed call is one whole route between two events on a different copy of the cache -- consecutive calls, whichever their arms,
rotate over the copies, at least --rotate-bytes of them; the arms alternate call by call inside a round; a round's figure is the mean of
its calls, a cell's the median and min .. max of --rounds rounds.  The calls of a round are as many as fit --round-ms per arm (at least
1, at most --launches).  bf16, causal, contiguous cache.  TFLOP/s: 2 x (576 + 512) x visible (row, key) pairs x heads over (n)'s median.

    python tools/mla_prefill_perf.py --parent-lib PARENT/libmfa_hip.so > profiles/mla_prefill_perf.txt
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from metal_flash_attention_amd import AttentionMLADecode, AttentionMLAPrefill, GEMMOperandPrecision as P, _abi  # noqa: E402

DK, DV, CHUNK = 576, 512, 32
SCALE = 0.1352337788608801
ARMS = ("n", "c1", "cp", "t")


class Decode:
    """mfa_attention_mla_decode_launch / _workspace_size of a library: this build's, or the one --parent-lib names"""

    def __init__(self, path):
        self.lib = _abi.lib() if path is None else ctypes.CDLL(path)
        self.host = AttentionMLADecode(P.BF16)
        for name in ("mfa_attention_mla_decode_launch", "mfa_attention_mla_decode_workspace_size"):
            fn, mine = getattr(self.lib, name), getattr(_abi.lib(), name)
            fn.restype, fn.argtypes = mine.restype, mine.argtypes

    def params(self, **kw):
        return self.host._params(**kw)[0]

    def workspace(self, p):
        need, pieces = ctypes.c_uint64(0), ctypes.c_uint32(0)
        assert self.lib.mfa_attention_mla_decode_workspace_size(ctypes.byref(p), ctypes.byref(need), ctypes.byref(pieces)) == 0
        return int(need.value), int(pieces.value)

    def launch(self, q, kv, o, l, p, stream):
        st = self.lib.mfa_attention_mla_decode_launch(q, kv, o, l, ctypes.byref(p), ctypes.c_void_p(stream))
        assert st == 0, st


class Cell:
    """rotating copies of the cache of B sequences of prefix + rows keys, and the operands of every arm"""

    def __init__(self, B, H, rows, prefix, rotate_bytes, decode):
        self.B, self.H, self.rows, self.prefix, self.decode = B, H, rows, prefix, decode
        bf = torch.bfloat16
        self.C = C = prefix + rows
        self.copies = max(2, min(8, -(-rotate_bytes // (B * C * DK * 2))))
        self.kv = [(torch.randn(B, C, DK, device="cuda", dtype=bf) * 0.5) for _ in range(self.copies)]
        self.q = torch.randn(B, H, rows, DK, device="cuda", dtype=bf)
        self.o = torch.empty(B, H, rows, DV, device="cuda", dtype=bf)
        self.l = torch.empty(B, H, rows, device="cuda", dtype=torch.float32)
        self.lengths = torch.full((B,), C, dtype=torch.int32, device="cuda")
        self.new = AttentionMLAPrefill(P.BF16)
        self.kw = dict(rows=rows, column=C, heads=H, batches=B, scale=SCALE, cacheLengths=self.lengths)
        # arms (c1), (cp): a decode launch per 32 rows, the lengths advanced; Q, O and L are read and written where they lie
        self.chunks = []
        ends = torch.stack([torch.full((B,), prefix + min(r0 + CHUNK, rows), dtype=torch.int32) for r0 in range(0, rows, CHUNK)]).cuda()
        strides = dict(Q=(DK, rows * DK, H * rows * DK), O=(DV, rows * DV, H * rows * DV))
        need = 0
        for j, r0 in enumerate(range(0, rows, CHUNK)):
            R = min(CHUNK, rows - r0)
            kw = dict(rows=R, column=C, heads=H, batches=B, scale=SCALE, cacheLengths=ends[j], strides=strides, lStrides=(rows, H * rows))
            one = decode.params(pieces=1, **kw)
            plan = decode.params(pieces=0, **kw)
            nbytes, pieces = decode.workspace(plan)
            need = max(need, nbytes)
            at = (self.q.data_ptr() + r0 * DK * 2, self.o.data_ptr() + r0 * DV * 2, self.l.data_ptr() + r0 * 4)
            self.chunks.append((at, one, plan))
        self.pieces = pieces                                  # the plan of the last chunk (the longest cache)
        self.ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
        for _at, _one, plan in self.chunks:
            plan.workspace, plan.workspaceBytes = self.ws.data_ptr(), need
        self.ends = ends
        # arm (t): heads at a time so that the FP32 scores of a group stay below 2 GiB
        self.group = max(1, min(H, (1 << 31) // (rows * C * 4)))
        r = torch.arange(rows, device="cuda")[:, None]
        self.mask = torch.arange(C, device="cuda")[None, :] > r + prefix          # [rows, C]: True is hidden
        self.to = torch.empty(B, H, rows, DV, device="cuda", dtype=bf)

    def pairs(self):
        return self.rows * self.prefix + self.rows * (self.rows + 1) // 2

    def once(self, arm, i, stream):
        """microseconds of one route of an arm on copy i"""
        kv = self.kv[i % self.copies]
        if arm == "n":
            return 1e3 * self.new.time(self.q, kv, self.o, self.l, stream=stream, warmup=0, iterations=1, **self.kw)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        if arm in ("c1", "cp"):
            for (qp, op, lp), one, plan in self.chunks:
                self.decode.launch(qp, kv.data_ptr(), op, lp, one if arm == "c1" else plan, stream)
        else:
            for b in range(self.B):
                K = kv[b]
                for h0 in range(0, self.H, self.group):
                    s = torch.matmul(self.q[b, h0:h0 + self.group], K.t()).float() * SCALE
                    s.masked_fill_(self.mask, float("-inf"))
                    self.to[b, h0:h0 + self.group] = torch.matmul(torch.softmax(s, dim=-1).to(K.dtype), K[:, :DV])
        stop.record()
        stop.synchronize()
        return 1e3 * start.elapsed_time(stop)


def measure(cell, rounds, launches, round_ms, arms):
    """{arm: (median, min, max)} us per route; the arms alternate call by call, one warm-up pass first"""
    stream = torch.cuda.current_stream().cuda_stream
    first = {arm: cell.once(arm, 0, stream) for arm in arms}
    torch.cuda.synchronize()
    if "t" in arms:   # (n) and (t) compute the same thing on copy 0, in another order of sums -- loosely; the tests hold the launch to its bounds
        err = (cell.o.float() - cell.to.float()).abs().max().item()
        assert err < 3e-2, err
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
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    arms = tuple(a for a in ARMS if not (a == "t" and args.no_torch))
    decode = Decode(args.parent_lib)
    print("tools/mla_prefill_perf.py -- MLA prefill over the latent cache: the new launch (n) against ceil(rows / 32) decode launches with the")
    print("lengths advanced, unsplit (c1) and at the host's plan (cp; pieces: the last chunk's), and torch bmm + mask + softmax + bmm (t); bf16,")
    print("causal, contiguous cache of prefix + rows keys; us per route between two events, median of %d rounds (min .. max) of up to %d calls;" % (
        args.rounds, args.launches))
    print("decode launches from %s; %s" % ("the parent commit's library" if args.parent_lib else "THIS build (its decode units are the parent's)",
                                           torch.cuda.get_device_name(0)))
    for B in args.batches:
        for H in args.heads:
            for rows in args.rows:
                for prefix in args.prefix:
                    cell = Cell(B, H, rows, prefix, args.rotate_bytes, decode)
                    res, calls = measure(cell, args.rounds, args.launches, args.round_ms, arms)
                    flops = 2.0 * (DK + DV) * cell.pairs() * H * B
                    line = "B %d  H %3d  rows %4d  prefix %5d  blocks %5d  pieces %2d  %d copies  %2d calls   " % (
                        B, H, rows, prefix, B * -(-rows * H // 64), cell.pieces, cell.copies, calls)
                    line += "   ".join("(%s) %9.1f (%.1f .. %.1f)" % (arm, *res[arm]) for arm in arms)
                    line += "   (n) %6.1f TFLOP/s   (c1)/(n) %5.2f   (cp)/(n) %5.2f" % (
                        flops / (res["n"][0] * 1e-6) / 1e12, res["c1"][0] / res["n"][0], res["cp"][0] / res["n"][0])
                    if "t" in arms:
                        line += "   (t)/(n) %5.2f" % (res["t"][0] / res["n"][0])
                    print(line, flush=True)
                    del cell
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
