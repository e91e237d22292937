#!/usr/bin/env python3
"""developer A/B of two builds of the library on the speed of the launches cut along the keys -- decode (include/mfa_decode.h) and
prefill through the split entries (include/mfa_split.h) -- for a change that touches their host plan or their kernels:

    python tools/split_ab.py [--a metal_flash_attention_amd/libmfa_hip_prev.so] [--b metal_flash_attention_amd/libmfa_hip.so] [--rounds 4]

Timed by the library's own `_time` entries (10 warm-up and --iterations timed launches per shape).  The two libraries alternate, a fresh
child process each (the library is chosen at import, MFA_LIBRARY) under its own time limit, --rounds times, taking turns at going
first; nothing more is started after a child that failed.  Per shape: the medians, the first library's spread (max / min over its
rounds) and whether the second's median stays within it.  Shapes: decode at D 128 bf16, Hq 64 over 8 K/V heads, R 1 and 4, B 1 and 8,
full caches of 4096 and 32768 keys (tools/decode_perf.py's rows that split); prefill: the 16-node tree and the 128-row chunk of
DESIGN.md 4.20 (B 1, 32768 keys, paged 16, the planned pieces).
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tree_masks(R, seed):
    import random
    rnd, masks = random.Random(seed), [1]
    for j in range(1, R):
        masks.append(masks[rnd.randrange(j)] | (1 << j))
    return masks


class Case:
    """the operands of one launch, seeded; `decode`: through AttentionDecode(FP8), else AttentionPrefill with pieces= / workspace="""

    def __init__(self, torch, decode, D, dtype, B, Hq, Hkv, R, C, lens, qlens=None, page=0, fp8=False, logits=False, tree=False, pieces=0):
        from metal_flash_attention_amd import AttentionDecode, AttentionDecodeFP8, AttentionPrefill, GEMMOperandPrecision as P, KVCachePrecision
        g = torch.Generator().manual_seed(D * 7 + B * 3 + R + C + page + int(fp8))
        rand = lambda *shape: torch.rand(*shape, generator=g) * 2 - 1   # noqa: E731
        self.torch = torch
        self.q = rand(B, Hq, R, D).to(dtype).cuda()
        kv = [(rand(B, Hkv, C, D) * 0.5) for _ in range(2)]
        self.keep = [torch.tensor(lens, dtype=torch.int32).cuda()]
        self.kw = dict(rows=R, column=C, heads=Hq, batches=B, headsPerKeyValue=Hq // Hkv, causal=True, cacheLengths=self.keep[0])
        if page:   # the pages of sequence b, shuffled: page of (b, i) = where block b per + i went
            per = C // page
            perm = torch.randperm(B * per, generator=g)
            inv = torch.empty_like(perm)
            inv[perm] = torch.arange(B * per)
            kv = [t.view(B, Hkv, per, page, D).permute(0, 2, 1, 3, 4).reshape(B * per, Hkv, page, D)[inv].contiguous() for t in kv]
            self.keep.append(perm.view(B, per).to(torch.int32).cuda())
            self.kw.update(pageSize=page, blockTable=self.keep[-1], blockTableStride=per, pageStrides=(Hkv * page * D,) * 2,
                           strides=dict(K=(D, page * D, 0), V=(D, page * D, 0)))
        self.k, self.v = (t.cuda().to(torch.float8_e4m3fn if fp8 else dtype) for t in kv)
        prec = P.BF16 if dtype == torch.bfloat16 else P.FP16
        if fp8:
            self.keep += [(0.25 + 3.0 * torch.rand(Hkv, generator=g)).cuda() for _ in range(2)]   # spread scales
            self.kw.update(keyScale=self.keep[-2], valueScale=self.keep[-1])
        if decode:
            self.op = (AttentionDecodeFP8 if fp8 else AttentionDecode)(D, prec)
        else:
            self.op = AttentionPrefill(D, prec, cachePrecision=KVCachePrecision.E4M3 if fp8 else None)
            if qlens is not None:
                self.keep.append(torch.tensor(qlens, dtype=torch.int32).cuda())
                self.kw.update(queryLengths=self.keep[-1])
        if logits:
            self.keep.append((rand(Hq) * 3).cuda())
            self.kw.update(sinkLogits=self.keep[-1])
        if tree:
            self.keep.append(torch.tensor(tree_masks(R, R + D), dtype=torch.int64).cuda())
            self.kw.update(treeMasks=self.keep[-1], treeBatchStride=0)
        need = self.op.workspaceSize(**self.kw) if decode else self.op.plannedSplit(pieces=pieces, **self.kw)[0]
        assert need > 0, "every case of this tool is cut along the keys"
        self.ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
        self.kw.update(workspace=self.ws, **({} if decode else dict(pieces=pieces)))
        self.form = self.op.launchForm(**self.kw)
        assert "combine" in self.form, self.form
        self.o = torch.zeros(B, Hq, R, D, dtype=dtype, device="cuda")
        self.l = torch.zeros(B, Hq, R, dtype=torch.float32, device="cuda")

    def microseconds(self, iterations):
        ms = self.op.time(self.q, self.k, self.v, self.o, self.l, stream=self.torch.cuda.current_stream().cuda_stream, warmup=10, iterations=iterations, **self.kw)
        return ms / iterations * 1e3


def time_cases(torch):
    for R in (1, 4):
        for B in (1, 8):
            for C in (4096, 32768):
                yield "decode R%d B%d %d keys" % (R, B, C), dict(decode=True, D=128, dtype=torch.bfloat16, B=B, Hq=64, Hkv=8, R=R, C=C, lens=(C,) * B)
    for name, R, tree in (("tree16", 16, True), ("rows128", 128, False)):
        yield "prefill %s B1 32768 keys paged 16" % name, dict(decode=False, D=128, dtype=torch.bfloat16, B=1, Hq=64, Hkv=8, R=R, C=32768, lens=(32768,),
                                                              qlens=(R,), page=16, tree=tree)


def child(a):
    import torch
    assert torch.cuda.is_available(), "split_ab.py runs launches on the GPU: there is nothing to compare without one"
    for name, kw in time_cases(torch):
        case = Case(torch, **kw)
        case.microseconds(20)   # (code objects, the clocks)
        print("TIME\t%s\t%.3f\t%s" % (name, case.microseconds(a.iterations), case.form.split(" (")[0]), flush=True)
        del case
        torch.cuda.empty_cache()
    return 0


def start(lib, extra, seconds):
    """one child process with `lib`, under its own time limit -> (status, its output)"""
    env = dict(os.environ, MFA_LIBRARY=os.path.join(ROOT, lib))
    r = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--child"] + extra, env=env,
                       capture_output=True, text=True)
    return r.returncode, r.stdout + r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", default="metal_flash_attention_amd/libmfa_hip_prev.so")
    ap.add_argument("--b", default="metal_flash_attention_amd/libmfa_hip.so")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--step-seconds", type=int, default=180, help="the time limit of one child process")
    ap.add_argument("--child", action="store_true", help="(internal) one library's launches")
    a = ap.parse_args()
    if a.child:
        return child(a)
    print("A = %s\nB = %s" % (a.a, a.b), flush=True)
    assert a.rounds >= 3
    times = {"A": {}, "B": {}}
    for i in range(a.rounds):
        for tag, lib in (("A", a.a), ("B", a.b))[::-1 if i % 2 else 1]:   # alternate, and take turns at going first
            rc, text = start(lib, ["--iterations", str(a.iterations)], a.step_seconds)
            if rc != 0:
                print(text[-3000:] + "\n%s ended with status %d: nothing more is started" % (lib, rc))
                return rc or 1
            for line in text.splitlines():
                if line.startswith("TIME\t"):
                    _t, name, us, _kernel = line.split("\t")
                    times[tag].setdefault(name, []).append(float(us))
    slower = 0
    print("us per launch, median of %d rounds (all rounds); spread = A's max / min; ok: B's median <= A's median x A's spread" % a.rounds)
    for name, av in times["A"].items():
        bv = times["B"][name]
        am, bm, spread = statistics.median(av), statistics.median(bv), max(av) / min(av)
        ok = bm <= am * spread
        slower += not ok
        print("%-36s A %9.2f (%s)  B %9.2f (%s)  B/A %.4f  A's spread %.4f  %s" % (
            name, am, " ".join("%.2f" % x for x in av), bm, " ".join("%.2f" % x for x in bv), bm / am, spread, "ok" if ok else "SLOWER"), flush=True)
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
