"""MLA prefill cut along the keys (include/mfa_mla_prefill_split.h) at the shapes of tools/mla_prefill_perf.py whose unsplit launch has
fewer than 256 workgroups, and two where the plan says one piece, by that tool's protocol (its Cell and measure: rotating copies of the
cache, arms alternated call by call, one route between two events, median and min .. max of --rounds rounds):

  (s)  the new launch at the host's plan, one mfa_attention_mla_prefill_split_launch (both kernels)
  (n)  the unsplit launch, mfa_attention_mla_prefill_launch
  (cp) the loop of ceil(rows / 32) decode launches at the host's plan

(n) and (cp) are taken from the library --parent-lib names: the PARENT commit's build is the yardstick (without the option they run this
build's, and the header line says so).  --sweep: the plan's two constants instead -- (s) at the pieces the plan would choose with
MIN_STEPS in {8, 16, 32} and the target in {256, 512}, B = 1, H = 16, rows in {64, 512} over 4096 and 32768 keys.  bf16, causal,
contiguous cache.

    python tools/mla_prefill_split_perf.py --parent-lib PARENT/libmfa_hip.so > profiles/mla_prefill_split_perf.txt
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import mla_prefill_perf as base  # noqa: E402
from metal_flash_attention_amd import AttentionMLAPrefillSplit, GEMMOperandPrecision as P, _abi  # noqa: E402

# (B, H, rows, prefix): the rows of DESIGN 4.27's table with B x blocks < 256, then two where the plan says one piece
CELLS = [(B, H, rows, prefix) for B, H, rows in ((1, 16, 64), (1, 16, 512), (1, 128, 64), (8, 16, 64)) for prefix in (0, 4096, 32768)]
CELLS += [(1, 16, 2048, 4096), (8, 128, 64, 4096)]
SWEEP = [(1, 16, rows, prefix) for rows in (64, 512) for prefix in (4096, 32768)]


def choose_pieces(blocks, steps, target, min_steps, most=64):
    """choose_pieces of csrc/cache_launch.cpp"""
    if blocks >= target:
        return 1
    s = min(target // blocks, steps // min_steps, most)
    return 1 if s < 2 else s


class Parent(base.Decode):
    """the decode entries and mfa_attention_mla_prefill_time of a library: this build's, or the one --parent-lib names"""

    def __init__(self, path):
        super().__init__(path)
        fn, mine = self.lib.mfa_attention_mla_prefill_time, _abi.lib().mfa_attention_mla_prefill_time
        fn.restype, fn.argtypes = mine.restype, mine.argtypes


class Cell(base.Cell):
    def __init__(self, B, H, rows, prefix, rotate_bytes, parent, forced=()):
        super().__init__(B, H, rows, prefix, rotate_bytes, parent)
        self.split = AttentionMLAPrefillSplit(P.BF16)
        nbytes, self.planned = self.split.plannedSplit(**self.kw)
        self.sbytes = max([nbytes, 16] + [self.split.plannedSplit(pieces=f, **self.kw)[0] for f in forced])
        self.sws = torch.empty(self.sbytes, dtype=torch.uint8, device="cuda")
        self.unsplit = self.new._params(**self.kw)[0]

    def once(self, arm, i, stream):
        kv = self.kv[i % self.copies]
        if arm == "n":
            ms = ctypes.c_float(0.0)
            st = self.decode.lib.mfa_attention_mla_prefill_time(self.q.data_ptr(), kv.data_ptr(), self.o.data_ptr(), self.l.data_ptr(),
                                                                 ctypes.byref(self.unsplit), ctypes.c_void_p(stream), 0, 1, ctypes.byref(ms))
            assert st == 0, st
            return 1e3 * ms.value
        if arm[0] in "sp":   # "s": the plan; "p<N>": N pieces as given
            return 1e3 * self.split.time(self.q, kv, self.o, self.l, stream=stream, warmup=0, iterations=1, workspace=self.sws,
                                         workspaceBytes=self.sbytes, pieces=int(arm[1:] or 0), **self.kw)
        return super().once(arm, i, stream)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--round-ms", type=float, default=150.0)
    ap.add_argument("--rotate-bytes", type=int, default=1 << 30)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    parent = Parent(args.parent_lib)
    print("tools/mla_prefill_split_perf.py -- MLA prefill cut along the keys: %s; bf16, causal, contiguous cache of prefix + rows keys;" % (
        "(s) at the pieces the plan chooses with (MIN_STEPS / target)" if args.sweep else
        "the new launch at the host's plan (s), the unsplit launch (n), the loop of decode launches at its plan (cp)"))
    print("us per route between two events, median of %d rounds (min .. max) of up to %d calls; (n) and (cp) from %s; %s" % (
        args.rounds, args.launches, "the parent commit's library" if args.parent_lib else "THIS build", torch.cuda.get_device_name(0)))
    for B, H, rows, prefix in (SWEEP if args.sweep else CELLS):
        blocks, steps = B * -(-rows * H // 64), -(-(prefix + rows) // 32)
        pairs = [(ms, t) for ms in (8, 16, 32) for t in (256, 512)]
        counts = sorted({choose_pieces(blocks, steps, t, ms) for ms, t in pairs}) if args.sweep else []
        cell = Cell(B, H, rows, prefix, args.rotate_bytes, parent, counts)
        arms = tuple("p%d" % c for c in counts) if args.sweep else ("s", "n", "cp")
        res, calls = base.measure(cell, args.rounds, args.launches, args.round_ms, arms)
        line = "B %d  H %3d  rows %4d  prefix %5d  blocks %5d  %d copies  %2d calls   " % (B, H, rows, prefix, blocks, cell.copies, calls)
        if args.sweep:
            line += "   ".join("%2d pieces [%s] %8.1f (%.1f .. %.1f)" % (
                c, " ".join("%d/%d" % pr for pr in pairs if choose_pieces(blocks, steps, pr[1], pr[0]) == c), *res["p%d" % c]) for c in counts)
        else:
            line += "pieces %2d (cp: %2d)   " % (cell.planned, cell.pieces)
            line += "   ".join("(%s) %9.1f (%.1f .. %.1f)" % (arm, *res[arm]) for arm in arms)
            line += "   (n)/(s) %5.2f   (cp)/(s) %5.2f" % (res["n"][0] / res["s"][0], res["cp"][0] / res["s"][0])
        print(line, flush=True)
        del cell
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
