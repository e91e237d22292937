"""Speculation trees over a KV cache (include/mfa_tree.h) against their sibling, the sink-family causal launch of the same shape, in one
process, on the `_time` entries of the C ABI: a sibling of tools/softcap_perf.py.  Every timed call is ONE launch between two events on a
different copy of the cache -- consecutive launches, whichever their arms, rotate over copies that sum well above the Infinity Cache, so
no arm reads what the arm before it has just pulled in --; the arms alternate launch by launch inside a round; a round's figure is the
mean of its launches, a cell's the median and min .. max of --rounds rounds.

Arms, all with one sink logit per query head and no window, so that all run the sink BODY over the whole cache:
  (s)  the sink-family causal launch                          -- attn_decode16s_* / attn_decode8s_* / attn_prefill16s_*
  (c)  the tree launch with the chain mask 2^(r + 1) - 1      -- attn_decode16t_* / attn_decode8t_* / attn_prefill16t_*
  (t)  the tree launch with a random tree (parent uniform among the earlier nodes)
  (p)  what a caller has today for that tree: one sink-family chain launch per root-to-leaf path, rows = the path's length, summed
Shapes: D = 128, Hq 64 over Hkv 8 (G = 8), B = 8, caches of 4096 and 32768 keys, all sequences full; decode R = 4 and prefill R = 64;
16-bit and e4m3 caches.  No ratio is fixed in advance: decode is bound by the bytes of K and V and is expected to stay at parity.

    python tools/tree_perf.py > profiles/tree_perf.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tree_model as tm  # noqa: E402
from metal_flash_attention_amd import AttentionDecode, AttentionDecodeFP8, AttentionPrefill, GEMMOperandPrecision as P, KVCachePrecision  # noqa: E402

D, HQ, HKV, B = 128, 64, 8, 8
LENGTHS = (4096, 32768)


class Cache:
    """rotating copies of a cache of C keys, all sequences full, and the new rows: what every arm of a cell reads and writes"""

    def __init__(self, R, C, fp8, rotate_bytes):
        self.R, self.C, self.fp8 = R, C, fp8
        self.copies = max(2, min(64, -(-rotate_bytes // (2 * B * HKV * C * D * (1 if fp8 else 2)))))
        kind = torch.float8_e4m3fn if fp8 else torch.bfloat16
        self.q = torch.randn(B, HQ, R, D, device="cuda").to(torch.bfloat16)
        self.k = [(torch.randn(B, HKV, C, D, device="cuda", dtype=torch.bfloat16) * 0.5).to(kind) for _ in range(self.copies)]
        self.v = [(torch.randn(B, HKV, C, D, device="cuda", dtype=torch.bfloat16) * 0.5).to(kind) for _ in range(self.copies)]
        self.o = torch.empty(B, HQ, R, D, dtype=torch.bfloat16, device="cuda")
        self.l = torch.empty(B, HQ, R, dtype=torch.float32, device="cuda")
        self.lengths = torch.full((B,), C, dtype=torch.int32, device="cuda")
        self.logits = torch.linspace(-1.0, 3.0, HQ, dtype=torch.float32, device="cuda")


class Arm:
    """one launch kind over a Cache: the sink-family launch of `rows` rows, with `masks` the tree launch"""

    def __init__(self, kind, cache, rows, masks=None):
        c = self.cache = cache
        if kind == "decode":
            self.op = (AttentionDecodeFP8 if c.fp8 else AttentionDecode)(D, P.BF16)
        else:
            self.op = AttentionPrefill(D, P.BF16, cachePrecision=KVCachePrecision.E4M3 if c.fp8 else None)
        self.kw = dict(rows=rows, column=c.C, heads=HQ, batches=B, headsPerKeyValue=HQ // HKV, causal=True, cacheLengths=c.lengths, sinkLogits=c.logits,
                       strides=dict(Q=(D, c.R * D, HQ * c.R * D), O=(D, c.R * D, HQ * c.R * D)), lStrides=(c.R, HQ * c.R))
        if masks is not None:
            self.masks = torch.from_numpy(masks.view(np.int64)).cuda()
            self.kw.update(treeMasks=self.masks, treeBatchStride=0)
        if kind == "decode":
            need = self.op.workspaceSize(**self.kw)
            self.kw.update(workspace=torch.empty(need, dtype=torch.uint8, device="cuda") if need else None)
        self.form = self.op.launchForm(**self.kw)

    def once(self, i, stream):
        """microseconds of one launch on copy i"""
        c = self.cache
        return 1e3 * self.op.time(c.q, c.k[i % c.copies], c.v[i % c.copies], c.o, c.l, stream=stream, warmup=0, iterations=1, **self.kw)


def measure(arms, rounds, launches):
    """{arm: (median, min, max)} us per launch; the arms alternate launch by launch, one warm-up pass first"""
    stream = torch.cuda.current_stream().cuda_stream
    for a in arms.values():
        a.once(0, stream)
    per = {name: [] for name in arms}
    at = 1
    for _ in range(rounds):
        took = {name: 0.0 for name in arms}
        for _i in range(launches):
            for name, a in arms.items():   # (every launch on the copy read longest ago, whichever arm read it)
                took[name] += a.once(at, stream)
                at += 1
        for name in arms:
            per[name].append(took[name] / launches)
    return {name: (statistics.median(x), min(x), max(x)) for name, x in per.items()}


def paths_of(masks):
    """the lengths of the root-to-leaf paths of a tree"""
    R = len(masks)
    nodes = [[j for j in range(R) if int(masks[r]) >> j & 1] for r in range(R)]
    return [len(nodes[r]) for r in range(R) if not any(r in nodes[s] for s in range(r + 1, R))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--rotate-bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    print("tools/tree_perf.py -- the sink-family causal launch (s) against the tree launch with the chain mask (c) and with a random tree (t), and")
    print("the chain launches over that tree's root-to-leaf paths, summed (p); us per launch, median of %d rounds of %d launches (min .. max);" % (
        args.rounds, args.launches))
    print("D %d, Hq %d over Hkv %d, B %d, bf16 Q, one sink logit per query head, no window, all sequences full; %s" % (D, HQ, HKV, B, torch.cuda.get_device_name(0)))
    for kind, R in (("decode", 4), ("prefill", 64)):
        tree = tm.random_tree(R, np.random.default_rng(R + 2))
        paths = paths_of(tree)
        print("%s R %d: the random tree has %d leaves, paths of %s nodes" % (kind, R, len(paths), sorted(paths)))
        for fp8 in (False, True):
            for n in LENGTHS:
                cache = Cache(R, n, fp8, args.rotate_bytes)
                arms = {"s": Arm(kind, cache, R), "c": Arm(kind, cache, R, tm.chain(R)), "t": Arm(kind, cache, R, tree)}
                for d in sorted(set(paths)):
                    arms["p%d" % d] = Arm(kind, cache, d)
                res = measure(arms, args.rounds, args.launches)
                alt = sum(res["p%d" % d][0] for d in paths)
                print("%-7s %-6s n %5d   " % (kind, "e4m3" if fp8 else "16-bit", n) +
                      "   ".join("(%s) %8.1f (%.1f .. %.1f)" % (a, *res[a]) for a in ("s", "c", "t")) +
                      "   (c)/(s) %.3f   (t)/(s) %.3f   (p) %9.1f   (p)/(t) %.2f" % (res["c"][0] / res["s"][0], res["t"][0] / res["s"][0], alt, alt / res["t"][0]),
                      flush=True)
                if n == LENGTHS[-1]:
                    print("        (t) " + arms["t"].form)
                del arms, cache
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
