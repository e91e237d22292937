"""Prefill over a KV cache cut along the keys (include/mfa_split.h) against the same launch unsplit, and a sweep of forced piece counts
that checks the two constants of the host's plan (MFA_PREFILL_SPLIT_MIN_TILES and the workgroup target).  Both arms run from one library,
in one process; the unsplit arm is the launch of the other headers, whose kernels the split did not change.

Shapes: bf16, Hq = 64 query heads over 8 K/V heads, D = 128, B = 1 and 4 sequences, every sequence full; new rows: a 16-node and a
64-node speculation tree (random trees), a 128-row and a 512-row chunk of a chunked prefill; n = 4096 / 32768 / 131072 cached keys (the
new rows' own keys included); a paged 16-bit cache (page 16, shuffled table) and a paged e4m3 cache with per-head scales.  One more row
at D = 256 and one at D = 64 (B = 1, the 16-node tree, n = 32768).  Arms:
  (split)    the split launch with the pieces the host plans, its workspace allocated once
  (unsplit)  the launch with the same parameters through the entries without a split
  --sweep: the split launch with 2, 4, ... 64 pieces forced, beside the unsplit launch

Method (tools/prefill_perf.py's): every launch of an arm reads a DIFFERENT copy of the cache, rotating over enough copies that their sum
is above the 256 MiB Infinity Cache (--rotate-bytes, at least two copies; the largest row, B = 4 at n = 131072, holds two copies of a
2 GiB 16-bit cache and two of the 1 GiB e4m3 one: about 6.5 GiB of the card); a page pool is the contiguous copy's own memory under a
shuffled table.  Consecutive launches of an arm are captured into one graph; a round is device events around one replay, the arms
alternate, and the table gives the median and the spread (min .. max) of --rounds rounds after a warm-up replay of each.  GB/s: the
K and V bytes of the sequences' keys over the time.  ratio = split / unsplit medians; `ok` where the plan chooses more than one piece
and the split launch's median does not exceed the unsplit launch's MAXIMUM over the same rounds, `SLOWER` where it does.

Every group of rows (a B and an n; the extra head dimensions; the sweep) is a child process of its own under `timeout`, one after the
other, and nothing more is started after one that failed.

    python tools/prefill_split_perf.py                 # the table, then the sweep
    python tools/prefill_split_perf.py --quick         # B = 1, n = 4096 and 32768 only, no sweep (a rehearsal)
"""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HQ, G = 64, 8
KINDS = (("tree16", 16, True), ("tree64", 64, True), ("rows128", 128, False), ("rows512", 512, False))


def random_tree_masks(R, seed):
    import random
    rnd = random.Random(seed)
    masks = [1]
    for j in range(1, R):
        masks.append(masks[rnd.randrange(j)] | (1 << j))
    return [m - (1 << 64) if m >= 1 << 63 else m for m in masks]


class Row:
    def __init__(self, torch, B, C, R, tree, fp8, D, rotate_bytes):
        from metal_flash_attention_amd import AttentionPrefill, GEMMOperandPrecision as P, KVCachePrecision
        self.torch, self.B, self.C, self.R, self.D, self.fp8 = torch, B, C, R, D, fp8
        Hkv = HQ // G
        esz = 1 if fp8 else 2
        self.bytes = 2 * B * Hkv * C * D * esz
        self.copies = max(2, min(64, -(-rotate_bytes // self.bytes)))
        make = lambda: torch.empty(B, Hkv, C, D, dtype=torch.bfloat16, device="cuda").normal_(0.0, 0.5)  # noqa: E731
        self.k, self.v = [], []
        for _ in range(self.copies):
            for dst in (self.k, self.v):
                t = make()
                dst.append(t.to(torch.float8_e4m3fn) if fp8 else t)
                del t
        self.q = torch.empty(B, HQ, R, D, dtype=torch.bfloat16, device="cuda").normal_()
        self.o = torch.empty(B, HQ, R, D, dtype=torch.bfloat16, device="cuda")
        self.l = torch.empty(B, HQ, R, dtype=torch.float32, device="cuda")
        self.op = AttentionPrefill(D, P.BF16, cachePrecision=KVCachePrecision.E4M3 if fp8 else None)
        per = C // 16
        table = torch.randperm(B * per, generator=torch.Generator().manual_seed(B + C + R)).view(B, per).to(torch.int32).cuda()
        self.keep = [table, torch.full((B,), C, dtype=torch.int32, device="cuda"), torch.full((B,), R, dtype=torch.int32, device="cuda")]
        self.kw = dict(rows=R, column=C, heads=HQ, batches=B, headsPerKeyValue=G, causal=True, cacheLengths=self.keep[1], queryLengths=self.keep[2],
                       pageSize=16, blockTable=table, blockTableStride=per, pageStrides=(Hkv * 16 * D,) * 2, strides=dict(K=(D, 16 * D, 0), V=(D, 16 * D, 0)))
        if fp8:
            self.keep += [0.5 + 1.5 * torch.rand(Hkv, device="cuda") for _ in range(2)]
            self.kw.update(keyScale=self.keep[-2], valueScale=self.keep[-1])
        if tree:
            self.keep.append(torch.tensor(random_tree_masks(R, R), dtype=torch.int64, device="cuda"))
            self.kw.update(treeMasks=self.keep[-1], treeBatchStride=0)
        self.workspaces = {}

    def split_kw(self, pieces):
        if pieces not in self.workspaces:
            need, count = self.op.plannedSplit(pieces=pieces, **self.kw)
            ws = self.torch.empty(max(need, 16), dtype=self.torch.uint8, device="cuda")
            self.workspaces[pieces] = (dict(self.kw, pieces=pieces, workspace=ws), count)
        return self.workspaces[pieces]

    def launch(self, arm, i, stream):
        c = i % self.copies
        kw = self.kw if arm == "unsplit" else self.split_kw(0 if arm == "split" else int(arm))[0]
        self.op.dispatch(self.q, self.k[c], self.v[c], self.o, self.l, stream=stream, **kw)

    def graph(self, arm, launches):
        g = self.torch.cuda.CUDAGraph()
        with self.torch.cuda.graph(g):
            stream = self.torch.cuda.current_stream().cuda_stream
            for i in range(launches):
                self.launch(arm, i, stream)
        return g


def once(torch, graph):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    graph.replay()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def measure(torch, row, arms, rounds, window_ms):
    stream = torch.cuda.current_stream().cuda_stream
    est = {}
    for arm in arms:   # warm every arm (code objects) and size the window
        row.launch(arm, 0, stream)
        torch.cuda.synchronize()
        probe = row.graph(arm, row.copies)
        once(torch, probe)
        est[arm] = once(torch, probe) / row.copies
        del probe
    graphs = {a: (row.graph(a, n), n) for a, n in ((a, max(row.copies, min(1000, int(window_ms / max(est[a], 1e-4))))) for a in arms)}
    samples = {a: [] for a in arms}
    for a in arms:
        once(torch, graphs[a][0])
    for _ in range(rounds):
        for a in arms:   # alternate
            g, n = graphs[a]
            samples[a].append(once(torch, g) / n * 1e3)
    return {a: (statistics.median(v), min(v), max(v), graphs[a][1]) for a, v in samples.items()}


def child(a):
    import torch

    from metal_flash_attention_amd import _abi
    assert torch.cuda.is_available(), "prefill_split_perf.py measures on the GPU: there is nothing to report without one"
    print("library sha256 %s" % hashlib.sha256(open(_abi.library_path(), "rb").read()).hexdigest()[:16], flush=True)
    what = a.group.split(",")
    if what[0] == "sweep":
        for name, R, tree in (KINDS[0], KINDS[2]):
            row = Row(torch, 1, 32768, R, tree, False, 128, a.rotate_bytes)
            arms = ["unsplit"] + [str(p) for p in (2, 4, 8, 16, 32, 64)]
            r = measure(torch, row, arms, a.rounds, a.window_ms)
            blocks = (HQ // G) * -(-R // (128 // G))
            print("sweep  B 1  n 32768  %-7s  D 128  16-bit  (%d row blocks x K/V heads, 512 tiles)" % (name, blocks), flush=True)
            for arm in arms:
                med, lo, hi, n = r[arm]
                p = 1 if arm == "unsplit" else int(arm)
                print("    pieces %-7s %9.1f us (%9.1f .. %9.1f) x%-4d  %4d workgroups  %3d tiles a piece  %7.1f GB/s" % (
                    arm, med, lo, hi, n, blocks * p, 512 // p, row.bytes / (med * 1e-6) / 1e9), flush=True)
            del row, r
            torch.cuda.empty_cache()
        return
    if what[0] == "dims":
        rows = [(1, 32768, KINDS[0], False, 256), (1, 32768, KINDS[0], False, 64)]
    else:
        B, C = int(what[0]), int(what[1])
        rows = [(B, C, kind, fp8, 128) for kind in KINDS for fp8 in (False, True)]
    for B, C, (name, R, tree), fp8, D in rows:
        row = Row(torch, B, C, R, tree, fp8, D, a.rotate_bytes)
        count = row.split_kw(0)[1]
        r = measure(torch, row, ("split", "unsplit"), a.rounds, a.window_ms)
        (sm, slo, shi, sn), (um, ulo, uhi, un) = r["split"], r["unsplit"]
        verdict = "one piece: the same launch" if count == 1 else "ok" if sm <= uhi else "SLOWER"
        print("B %d  n %6d  %-7s  D %3d  %-6s  copies %2d  pieces %2d | split %9.1f us (%9.1f .. %9.1f) x%-4d %7.1f GB/s | unsplit %9.1f us (%9.1f .. %9.1f) "
              "x%-4d %7.1f GB/s | ratio %.3f  %s" % (B, C, name, D, "e4m3" if fp8 else "16-bit", row.copies, count, sm, slo, shi, sn,
                                                     row.bytes / (sm * 1e-6) / 1e9, um, ulo, uhi, un, row.bytes / (um * 1e-6) / 1e9, sm / um, verdict), flush=True)
        del row, r
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0, help="device time one timed replay aims at")
    ap.add_argument("--rotate-bytes", type=int, default=1 << 30)
    ap.add_argument("--quick", action="store_true", help="B = 1, n = 4096 and 32768 only, no sweep (a rehearsal)")
    ap.add_argument("--step-seconds", type=int, default=240, help="the time limit of one group of rows")
    ap.add_argument("--group", help="(internal) the rows of one child process: 'B,n', 'dims' or 'sweep'")
    a = ap.parse_args()
    if a.group:
        return child(a)
    groups = ["%d,%d" % (B, C) for B in (1, 4) for C in (4096, 32768, 131072) if not a.quick or (B == 1 and C < 131072)]
    groups += [] if a.quick else ["dims", "sweep"]
    print("bf16, Hq %d over %d K/V heads, paged 16, full sequences; us per launch: median (min .. max) of %d rounds, launches per replay after x"
          % (HQ, HQ // G, a.rounds), flush=True)
    for group in groups:   # one after the other, each under its own time limit; nothing more is started after a failure
        rc = subprocess.run(["timeout", "-k", "10", str(a.step_seconds), sys.executable, os.path.abspath(__file__), "--group", group, "--rounds", str(a.rounds),
                             "--window-ms", str(a.window_ms), "--rotate-bytes", str(a.rotate_bytes)]).returncode
        if rc != 0:
            print("group %s ended with status %d: nothing more is started" % (group, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
