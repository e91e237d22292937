"""Sparse MLA prefill (include/mfa_mla_prefill_sparse.h) at the shapes of a DeepSeek-V3.2 prompt chunk -- bf16, topk = 2048 out of a
cache of C = 32768 keys, H = 128 and 16 heads, B = 1 and 8 sequences, 64, 512 and 4096 rows -- beside the two routes a caller has
without it, in one process:

  (x) the sparse prefill   mfa_attention_mla_prefill_sparse_launch: one launch, 32 heads of a row a workgroup
  (a) the decode loop      mfa_attention_mla_sparse_decode_launch, rows / 32 launches of 32 rows each over the same lists, each with the
                           pieces and the workspace its own plan asks for, the per-chunk lengths made ahead of the clock
  (b) the dense prefill    mfa_attention_mla_prefill_launch at the same shape: every key below the frontier

Every sequence holds C keys.  A row's list is 2048 DISTINCT positions scattered over the first 16384 keys (start + j x an odd stride,
modulo 16384): every one is visible to every row under either rule, so (x) and (a) do the same work.  Before timing, (x)'s O and L are
held against (a)'s with every launch unsplit, bit for bit.  A timed call is ONE call of an arm between two events (for (a): its whole loop), on a different copy of
the cache each time; the arms alternate call by call inside a round; a round's figure is the mean of its calls -- as many as fit
--call-ms, at least one -- a cell's the median and min .. max of --rounds rounds.

    python tools/mla_sparse_prefill_perf.py > profiles/mla_sparse_prefill_perf.txt

With MFA_LIBRARY naming a library built with -DMFA_MLAPX_TWO_TILES, (x) is the two-tile kernel where H > 32 (its launch form says px).

--fp8: the same cells over an E4M3 latent cache (include/mfa_mla_prefill_sparse_fp8.h; bytes of magnitude <= 1 under a kvScale of 0.5).
(x) is mfa_attention_mla_prefill_sparse_fp8_launch, beside (a) the 16-bit sparse prefill above on the dequantised cache -- what a caller
who keeps a 16-bit copy runs --, (b) the loop of mfa_attention_mla_sparse_decode_fp8_launch at that launch's own plan and (c) the dense
mfa_attention_mla_prefill_fp8_launch; (x) is held against (b) unsplit, bit for bit.

    python tools/mla_sparse_prefill_perf.py --fp8 > profiles/mla_sparse_prefill_fp8_perf.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from metal_flash_attention_amd import (AttentionMLAPrefill, AttentionMLAPrefillFP8, AttentionMLAPrefillSparse, AttentionMLAPrefillSparseFP8,  # noqa: E402
                                       AttentionMLASparseDecode, AttentionMLASparseDecodeFP8, GEMMOperandPrecision as P)

DK, DV, CHUNK, WINDOW = 576, 512, 32, 16384
SCALE = 0.1352337788608801
KV_SCALE = 0.5
ARMS = {False: (("x", "sparse"), ("a", "loop"), ("b", "dense")),                          # (label, what it runs) by --fp8
        True: (("x", "sparse"), ("a", "sparse16"), ("b", "loop"), ("c", "dense"))}


class Cell:
    """rotating copies of the latent caches of B sequences of C keys, and the operands of every arm"""

    def __init__(self, B, C, H, R, topk, rotate_bytes, fp8=False):
        assert R % CHUNK == 0 and C - R >= WINDOW and topk <= WINDOW
        self.B, self.C, self.H, self.R, self.topk = B, C, H, R, topk
        bf = torch.bfloat16
        self.copies = max(2, min(8, -(-rotate_bytes // (B * C * DK * 2))))
        self.scale = {}
        if fp8:   # bytes that are never NaN; kv16: the values they stand for, exactly
            code = lambda: (torch.randint(0, 0x39, (B, C, DK), device="cuda") | (torch.randint(0, 2, (B, C, DK), device="cuda") << 7)).to(torch.uint8)  # noqa: E731
            self.kv = [code().view(torch.float8_e4m3fn) for _ in range(self.copies)]
            self.kv16 = [(kv.float() * KV_SCALE).to(bf) for kv in self.kv]
            self.scale = dict(kvScale=torch.tensor([KV_SCALE], dtype=torch.float32, device="cuda"))
            self.sparse16 = AttentionMLAPrefillSparse(P.BF16)
        else:
            self.kv = [torch.randn(B, C, DK, device="cuda", dtype=bf) for _ in range(self.copies)]
        self.q = torch.randn(B, H, R, DK, device="cuda", dtype=bf)
        self.o = torch.empty(B, H, R, DV, device="cuda", dtype=bf)
        self.l = torch.empty(B, H, R, device="cuda")
        start = torch.randint(0, WINDOW, (B, R, 1), device="cuda")
        stride = 2 * torch.randint(0, WINDOW // 2, (B, R, 1), device="cuda") + 1
        self.indices = ((start + stride * torch.arange(topk, device="cuda")) % WINDOW).to(torch.int32)
        self.lengths = torch.full((B,), C, dtype=torch.int32, device="cuda")
        # chunk j of the loop: rows [32 j, 32 j + 32) as a launch of 32 rows whose frontier is prefill's, c <= r + (C - R) + 32 j
        self.chunk_lengths = [torch.full((B,), C - R + CHUNK * (j + 1), dtype=torch.int32, device="cuda") for j in range(R // CHUNK)]
        kinds = (AttentionMLAPrefillSparseFP8, AttentionMLASparseDecodeFP8, AttentionMLAPrefillFP8) if fp8 else \
            (AttentionMLAPrefillSparse, AttentionMLASparseDecode, AttentionMLAPrefill)
        self.sparse, self.decode, self.dense = (kind(P.BF16) for kind in kinds)
        whole = lambda t: (int(t.stride(2)), int(t.stride(1)), int(t.stride(0)))  # noqa: E731
        self.kw = dict(rows=R, column=C, heads=H, batches=B, scale=SCALE, cacheLengths=self.lengths)
        self.lists = dict(indices=self.indices, topk=topk)
        self.chunk_kw = dict(rows=CHUNK, column=C, heads=H, batches=B, scale=SCALE, topk=topk, indexStrides=(topk, R * topk),
                             strides=dict(Q=whole(self.q), O=whole(self.o)), lStrides=(int(self.l.stride(1)), int(self.l.stride(0))), **self.scale)
        need = self.decode.workspaceSize(indices=self.indices, cacheLengths=self.lengths, **self.chunk_kw)
        self.ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda") if need else None
        self.form = self.sparse.launchForm(**self.kw, **self.lists, **self.scale)
        self.chunk_form = self.decode.launchForm(indices=self.indices, cacheLengths=self.lengths, workspace=self.ws, **self.chunk_kw)

    def loop(self, kv, o, l, stream, planned=True):
        """(a); planned False: every launch unsplit, the arithmetic (x) repeats bit for bit"""
        cut = dict(workspace=self.ws) if planned else dict(pieces=1)
        for j, lengths in enumerate(self.chunk_lengths):
            rows = slice(CHUNK * j, CHUNK * (j + 1))
            self.decode.dispatch(self.q[:, :, rows], kv, o[:, :, rows], l[:, :, rows], stream=stream, indices=self.indices[:, rows],
                                 cacheLengths=lengths, **cut, **self.chunk_kw)

    def once(self, arm, i, stream):
        """microseconds of one call of an arm on copy i"""
        kv = self.kv[i % self.copies]
        if arm == "sparse":
            return 1e3 * self.sparse.time(self.q, kv, self.o, self.l, stream=stream, warmup=0, iterations=1, **self.kw, **self.lists, **self.scale)
        if arm == "sparse16":
            return 1e3 * self.sparse16.time(self.q, self.kv16[i % self.copies], self.o, self.l, stream=stream, warmup=0, iterations=1, **self.kw, **self.lists)
        if arm == "dense":
            return 1e3 * self.dense.time(self.q, kv, self.o, self.l, stream=stream, warmup=0, iterations=1, **self.kw, **self.scale)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        self.loop(kv, self.o, self.l, stream)
        stop.record()
        stop.synchronize()
        return 1e3 * start.elapsed_time(stop)

    def check(self, stream):
        """(x) against (a) with every launch unsplit, on copy 0: O and L bit for bit.  (A launch its plan cuts into pieces rounds P
        against each piece's own maximum: the same attention, other last bits.)"""
        o, l = torch.zeros_like(self.o), torch.zeros_like(self.l)
        self.loop(self.kv[0], o, l, stream, planned=False)
        self.sparse.dispatch(self.q, self.kv[0], self.o, self.l, stream=stream, **self.kw, **self.lists, **self.scale)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(self.l).all()) and bool(self.o.float().abs().max() > 0)
        assert torch.equal(o.view(torch.int16), self.o.view(torch.int16)) and torch.equal(l, self.l), "the sparse prefill and the unsplit decode loop differ: max |dO| %g, max |dL| %g" % (
            float((o.float() - self.o.float()).abs().max()), float((l - self.l).abs().max()))


def measure(cell, arms, rounds, call_ms):
    """{label: (median, min, max)} us per call; the arms alternate call by call, one warm-up call of each first"""
    stream = torch.cuda.current_stream().cuda_stream
    first = {arm: cell.once(arm, 0, stream) for _label, arm in arms}
    cell.check(stream)
    calls = {arm: max(1, min(20, int(call_ms * 1e3 / first[arm]))) for _label, arm in arms}
    per = {arm: [] for _label, arm in arms}
    at = 1
    for _ in range(rounds):
        took = {arm: 0.0 for _label, arm in arms}
        for i in range(max(calls.values())):
            for _label, arm in arms:
                if i < calls[arm]:
                    took[arm] += cell.once(arm, at, stream)
                    at += 1
        for _label, arm in arms:
            per[arm].append(took[arm] / calls[arm])
    return {label: (statistics.median(per[arm]), min(per[arm]), max(per[arm])) for label, arm in arms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--call-ms", type=float, default=100.0, help="calls of an arm in a round: what fits this many milliseconds, 1 .. 20")
    ap.add_argument("--rotate-bytes", type=int, default=1 << 30)
    ap.add_argument("--column", type=int, default=32768)
    ap.add_argument("--topk", type=int, default=2048)
    ap.add_argument("--heads", type=int, nargs="+", default=[128, 16])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--rows", type=int, nargs="+", default=[64, 512, 4096])
    ap.add_argument("--fp8", action="store_true", help="an e4m3 latent cache: (x) the fp8 sparse prefill, (a) the 16-bit one on the dequantised cache, "
                    "(b) the fp8 decode loop, (c) the dense fp8 prefill")
    args = ap.parse_args()
    arms = ARMS[args.fp8]
    if args.fp8:
        print("tools/mla_sparse_prefill_perf.py --fp8 -- sparse MLA prefill over an e4m3 latent cache, topk %d out of %d keys, bf16 Q: the one launch (x)" % (
            args.topk, args.column))
        print("against the 16-bit sparse prefill on the dequantised cache (a), a loop of e4m3 sparse decode launches of 32 rows over the same lists (b)")
        print("and the dense e4m3 prefill at the same shape (c); us per call between two events, median of")
    else:
        print("tools/mla_sparse_prefill_perf.py -- sparse MLA prefill, topk %d out of %d keys, bf16: the one launch (x) against a loop of sparse decode" % (
            args.topk, args.column))
        print("launches of 32 rows over the same lists (a) and the dense prefill at the same shape (b); us per call between two events, median of")
    print("%d rounds (min .. max); TFLOP/s: 2 x B x H x rows x topk x (576 + 512) over (x)'s median; %s" % (args.rounds, torch.cuda.get_device_name(0)))
    for H in args.heads:
        for B in args.batches:
            for R in args.rows:
                cell = Cell(B, args.column, H, R, args.topk, args.rotate_bytes, args.fp8)
                res = measure(cell, arms, args.rounds, args.call_ms)
                line = "H %3d  B %d  rows %4d   " % (H, B, R)
                line += "   ".join("(%s) %9.1f (%.1f .. %.1f)" % (label, *res[label]) for label, _arm in arms)
                line += "   (x) %5.1f TFLOP/s   " % (2.0 * B * H * R * args.topk * (DK + DV) / (res["x"][0] * 1e-6) / 1e12)
                line += "".join("(%s)/(x) %.2f   " % (label, res[label][0] / res["x"][0]) for label, _arm in arms[1:])
                line += "%s | loop of %d x %s" % (cell.form, R // CHUNK, cell.chunk_form)
                print(line, flush=True)
                del cell
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
