"""MLA decode over an e4m3 latent cache (include/mfa_mla_cache.h) beside the 16-bit launch it halves the bytes of, at the shapes and with
the method of tools/mla_perf.py, and the latent cache's append beside a torch scatter of the same rows:

  (m)  the 16-bit launch over a contiguous cache [B, C, 576] bf16, through mfa_attention_mla_decode_time      -- attn_mla16_d576_bf16[_k + _combine]
  (f)  the e4m3 launch over the SAME TOKENS as bytes (the 16-bit cache holds exactly the values of the bytes, kvScale 0.37 on both
       sides), through mfa_attention_mla_decode_fp8_time                                                   -- attn_mla8_d576_bf16[_k] + the same combine
  (g)  with --other-library PATH: (f) from another build of the library in the same process (a build with another number of steps of
       loads in flight, -DMFA_MLA8_FLIGHT=n), launch by launch beside (f)

Every timed call is ONE launch between two events on a different copy of its cache -- consecutive launches rotate over the copies, at
least --rotate-bytes of them --; the arms alternate launch by launch inside a round; a round's figure is the mean of its launches, a
cell's the median and min .. max of --rounds rounds.  Every sequence holds C keys.  TB/s counts each cache byte once: B x C x 576 for (f).

The append (B = 64 sequences into a pool of pages of 64 keys, R = 1 and R = 512 rows each): mla_cache_append into a bf16 pool (a) and an
e4m3 pool (a8) against torch's index_copy_ of the same rows, already fused to rows of 576, into the same pool (t), and for the e4m3 pool
after torch's own division and cast (t8).  Microseconds per call between two events around --launches calls.

    python tools/mla_fp8_perf.py > profiles/mla_fp8_perf.txt
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from metal_flash_attention_amd import AttentionMLADecode, AttentionMLADecodeFP8, GEMMOperandPrecision as P, _abi  # noqa: E402
from metal_flash_attention_amd import torch_binding as tb  # noqa: E402
from metal_flash_attention_amd.attention import _pointers  # noqa: E402

DK, DV, PAGE = 576, 512, 64
SCALE, KV_SCALE = 0.1352337788608801, 0.37
E4M3 = torch.float8_e4m3fn


def random_bytes(*shape):
    """e4m3 bytes of magnitude <= 1 with a random sign: never 0x7f / 0xff"""
    return (torch.randint(0, 0x39, shape, device="cuda", dtype=torch.uint8) | (torch.randint(0, 2, shape, device="cuda", dtype=torch.uint8) << 7))


class Cell:
    """rotating copies of the two caches of B sequences of C keys -- the same tokens as bytes and as bf16 -- and the operands"""

    def __init__(self, B, C, H, rotate_bytes, other):
        self.B, self.C, self.H = B, C, H
        self.bytes = {"m": B * C * DK * 2, "f": B * C * DK, "g": B * C * DK}
        self.copies = max(2, min(16, -(-rotate_bytes // self.bytes["m"])))
        self.kv8 = [random_bytes(B, C, DK).view(E4M3) for _ in range(self.copies)]
        self.kv16 = [kv.to(torch.bfloat16) * KV_SCALE for kv in self.kv8]   # (the product rounds to bf16: the check below is loose)
        bf = torch.bfloat16
        self.q = torch.randn(B, H, 1, DK, device="cuda", dtype=bf)
        self.o = {arm: torch.empty(B, H, 1, DV, device="cuda", dtype=bf) for arm in "mfg"}
        self.l = torch.empty(B, H, 1, device="cuda", dtype=torch.float32)
        self.lengths = torch.full((B,), C, dtype=torch.int32, device="cuda")
        self.kvscale = torch.tensor([KV_SCALE], dtype=torch.float32, device="cuda")
        self.mla, self.fp8 = AttentionMLADecode(P.BF16), AttentionMLADecodeFP8(P.BF16)
        self.kw = dict(rows=1, column=C, heads=H, batches=B, scale=SCALE, cacheLengths=self.lengths)
        need, self.pieces = self.mla.plannedSplit(**self.kw)
        assert self.fp8.plannedSplit(**self.kw) == (need, self.pieces)
        self.ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
        self.other = other

    def once(self, arm, i, stream):
        """microseconds of one launch of an arm on copy i"""
        i %= self.copies
        if arm == "m":
            return 1e3 * self.mla.time(self.q, self.kv16[i], self.o[arm], self.l, stream=stream, warmup=0, iterations=1, workspace=self.ws, **self.kw)
        if arm == "f":
            return 1e3 * self.fp8.time(self.q, self.kv8[i], self.o[arm], self.l, stream=stream, warmup=0, iterations=1, workspace=self.ws,
                                       kvScale=self.kvscale, **self.kw)
        shape = dict(self.kw, workspace=self.ws, kvScale=self.kvscale)   # (g): the other library's entry over this library's blocks
        own, _kept = self.fp8._own(shape)
        p, _keep = self.fp8._params(**shape)
        ms = ctypes.c_float(0.0)
        status = self.other(*_pointers(self.q, self.kv8[i], self.o[arm], self.l), ctypes.byref(p), *own, ctypes.c_void_p(stream), 0, 1, ctypes.byref(ms))
        assert status == 0, status
        return 1e3 * float(ms.value)


def measure(cell, arms, rounds, launches):
    """{arm: (median, min, max)} us per launch; the arms alternate launch by launch, one warm-up pass first on copy 0"""
    stream = torch.cuda.current_stream().cuda_stream
    for arm in arms:
        cell.once(arm, 0, stream)
    torch.cuda.synchronize()
    for arm in arms[1:]:   # the arms compute the same attention: loosely here -- the tests hold (f) to its bounds
        err = (cell.o[arm].float() - cell.o["m"].float()).abs().max().item()
        assert err < 2e-2, (arm, err)
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


def append_rows(B, R, rounds, launches):
    """{arm: (median, min, max)} us per call of the append arms; every sequence holds C0 keys before the call"""
    C0, pages_per = 2048, (2048 + 512) // PAGE
    g = torch.Generator(device="cuda").manual_seed(1)
    latent = torch.randn(B, R, 512, device="cuda", dtype=torch.bfloat16, generator=g)
    rope = torch.randn(B, R, 64, device="cuda", dtype=torch.bfloat16, generator=g)
    fused = torch.cat([latent, rope], dim=2).reshape(B * R, DK)
    table = torch.randperm(B * pages_per, device="cuda").to(torch.int32).view(B, pages_per)
    pool16 = torch.zeros(B * pages_per, PAGE, DK, device="cuda", dtype=torch.bfloat16)
    pool8 = torch.zeros(B * pages_per, PAGE, DK, device="cuda", dtype=torch.uint8).view(E4M3)
    lengths = torch.full((B,), C0 + R, dtype=torch.int32, device="cuda")
    pos = C0 + torch.arange(R, device="cuda")[None, :].expand(B, R)
    slots = (table.long().gather(1, pos // PAGE) * PAGE + pos % PAGE).reshape(-1)
    scale = torch.tensor([KV_SCALE], dtype=torch.float32, device="cuda")
    flat16, flat8 = pool16.view(-1, DK), pool8.view(torch.uint8).view(-1, DK)
    calls = {
        "a": lambda: tb.mla_cache_append(latent, rope, pool16, lengths, block_table=table),
        "t": lambda: flat16.index_copy_(0, slots, fused),
        "a8": lambda: tb.mla_cache_append(latent, rope, pool8, lengths, block_table=table, kv_scale=scale),
        "t8": lambda: flat8.index_copy_(0, slots, (fused.float() / KV_SCALE).clamp(-448, 448).to(E4M3).view(torch.uint8)),
    }
    for call in calls.values():
        call()
    torch.cuda.synchronize()
    assert torch.equal(pool16.view(-1, DK)[slots], fused)   # (a) and (t) wrote the same rows
    per = {arm: [] for arm in calls}
    for _ in range(rounds):
        for arm, call in calls.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _i in range(launches):
                call()
            stop.record()
            stop.synchronize()
            per[arm].append(1e3 * start.elapsed_time(stop) / launches)
    return {arm: (statistics.median(x), min(x), max(x)) for arm, x in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rotate-bytes", type=int, default=1 << 30)
    ap.add_argument("--other-library", default=None, help="another build of libmfa_hip.so whose e4m3 launch is arm (g)")
    ap.add_argument("--other-name", default="other build")
    args = ap.parse_args()
    other = None
    if args.other_library:
        handle = ctypes.CDLL(args.other_library)
        other = handle.mfa_attention_mla_decode_fp8_time
        other.restype, other.argtypes = next((r, a) for n, r, a in _abi.MLA_CACHE_SYMBOLS if n == "mfa_attention_mla_decode_fp8_time")
    arms = ("m", "f") + (("g",) if other else ())
    print("tools/mla_fp8_perf.py -- MLA decode over a 16-bit latent cache (m) and over the same tokens as e4m3 bytes (f)%s; R = 1, bf16 Q, every" % (
        ", and (g): (f) of %s" % args.other_name if other else ""))
    print("sequence C keys, contiguous; us per launch between two events, median of %d rounds of %d launches (min .. max); TB/s: unique cache" % (
        args.rounds, args.launches))
    print("bytes (B x C x 1152 for (m), B x C x 576 for (f)) over the median; %s" % torch.cuda.get_device_name(0))
    for B in (1, 8, 64):
        for C in (4096, 32768):
            for H in (16, 128):
                cell = Cell(B, C, H, args.rotate_bytes, other)
                res = measure(cell, arms, args.rounds, args.launches)
                tb_s = lambda arm: cell.bytes[arm] / (res[arm][0] * 1e-6) / 1e12  # noqa: E731
                line = "B %2d  C %5d  H %3d  %2d pieces  %2d copies   " % (B, C, H, cell.pieces, cell.copies)
                line += "   ".join("(%s) %8.1f (%.1f .. %.1f) %5.2f TB/s" % (arm, *res[arm], tb_s(arm)) for arm in arms)
                line += "   (f)/(m) %.2f" % (res["f"][0] / res["m"][0])
                if other:
                    line += "   (g)/(f) %.2f" % (res["g"][0] / res["f"][0])
                print(line, flush=True)
                del cell
                torch.cuda.empty_cache()
    print("append of R rows to each of 64 sequences, pages of %d keys; us per call over %d calls, median of %d rounds (min .. max): (a) mla_cache_append" % (
        PAGE, args.launches, args.rounds))
    print("into a bf16 pool, (t) torch index_copy_ of the fused rows; (a8) mla_cache_append into an e4m3 pool, (t8) torch divide, cast and index_copy_")
    for R in (1, 512):
        res = append_rows(64, R, args.rounds, args.launches)
        print("B 64  R %3d   " % R + "   ".join("(%s) %7.1f (%.1f .. %.1f)" % (arm, *res[arm]) for arm in ("a", "t", "a8", "t8")) +
              "   (a)/(t) %.2f   (a8)/(t8) %.2f" % (res["a"][0] / res["t"][0], res["a8"][0] / res["t8"][0]), flush=True)


if __name__ == "__main__":
    main()
