"""Logit soft-capping over a KV cache (include/mfa_softcap.h) against its sibling, the sink-family launch of the same shape, in one
process: a sibling of tools/sink_perf.py, whose method it shares (tools/window_perf.py's measure(): every launch of an arm reads a
different copy of the cache, rotating over copies that sum well above the Infinity Cache; the launches of an arm are captured into one
graph; the arms alternate round by round; median and min .. max of --rounds rounds).

Arms, both with one sink logit per query head, so that both run the sink BODY and differ in the cap alone:
  (s)  the sink-family launch at (n, W)                 -- attn_decode16s_* / attn_decode8s_* / attn_prefill16s_*
  (c)  the same launch with softcap = 50                -- attn_decode16c_* / attn_decode8c_* / attn_prefill16c_*
Shapes are Gemma 2's layers: D = 256 with Hq 16 over Hkv 8 (9B) and D = 128 with Hq 32 over Hkv 16 (27B); caches of 4096 and 8192
keys, all sequences full; the local layers' window of 4096 and the global layers' none; B = 1, 8, 64; decode R = 1 and prefill
chunks of 512 rows; 16-bit and e4m3 caches.  No ratio is fixed in advance: decode is bound by the bytes of K and V and is expected to
stay close to its sibling; prefill is bound by arithmetic, and the two more transcendentals per score will show.

    python tools/softcap_perf.py > profiles/softcap_perf.txt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import window_perf as wp  # noqa: E402
from metal_flash_attention_amd import AttentionDecode, AttentionDecodeFP8, AttentionPrefill, GEMMOperandPrecision as P, KVCachePrecision  # noqa: E402

MODELS = [(256, 16, 8), (128, 32, 16)]   # (D, Hq, Hkv)
LENGTHS, WINDOWS, BATCHES, CAP = (4096, 8192), (4096, 0), (1, 8, 64), 50.0


class Cache:
    """rotating copies of a cache of C keys, all sequences full, and the new rows: what both arms of a cell read and write"""

    def __init__(self, D, HQ, HKV, B, R, C, fp8, rotate_bytes):
        self.D, self.HQ, self.HKV, self.B, self.R, self.C, self.fp8 = D, HQ, HKV, B, R, C, fp8
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
    """one launch kind over a Cache: the sink-family launch, with `cap` its capped sibling (the interface wp.measure() drives)"""

    def __init__(self, kind, cache, window, cap):
        c = self.cache = cache
        self.copies = c.copies
        if kind == "decode":
            self.op = (AttentionDecodeFP8 if c.fp8 else AttentionDecode)(c.D, P.BF16)
        else:
            self.op = AttentionPrefill(c.D, P.BF16, cachePrecision=KVCachePrecision.E4M3 if c.fp8 else None)
        self.kw = dict(rows=c.R, column=c.C, heads=c.HQ, batches=c.B, headsPerKeyValue=c.HQ // c.HKV, causal=True, cacheLengths=c.lengths,
                       window=window, sinkLogits=c.logits)
        if cap:
            self.kw.update(softcap=cap)
        if kind == "decode":
            need = self.op.workspaceSize(**self.kw)
            self.kw.update(workspace=torch.empty(need, dtype=torch.uint8, device="cuda") if need else None)
        self.form = self.op.launchForm(**self.kw)

    def launch(self, i, stream):
        c = self.cache
        self.op.dispatch(c.q, c.k[i % c.copies], c.v[i % c.copies], c.o, c.l, stream=stream, **self.kw)

    graph = wp.Arm.graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--rotate-bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    print("tools/softcap_perf.py -- the sink-family launch (s) at (n, W) against the same launch with softcap %g (c); us per launch," % CAP)
    print("median of %d rounds (min .. max); bf16 Q, one sink logit per query head in both arms, all sequences full; %s" % (
        args.rounds, torch.cuda.get_device_name(0)))
    for kind, R in (("decode", 1), ("prefill", 512)):
        for D, HQ, HKV in MODELS:
            for fp8 in (False, True):
                ratios = []
                for n in LENGTHS:
                    for B in BATCHES:
                        cache = Cache(D, HQ, HKV, B, R, n, fp8, args.rotate_bytes)
                        for W in WINDOWS:
                            arms = {"s": Arm(kind, cache, W, None), "c": Arm(kind, cache, W, CAP)}
                            res = wp.measure(arms, args.rounds, args.window_ms)
                            ratios.append(res["c"][0] / res["s"][0])
                            print("%-7s D %3d Hq %2d Hkv %2d %-6s n %5d  W %4d  B %2d   " % (kind, D, HQ, HKV, "e4m3" if fp8 else "16-bit", n, W, B) +
                                  "   ".join("(%s) %8.1f (%.1f .. %.1f)" % (a, *res[a]) for a in ("s", "c")) + "   (c)/(s) %.3f" % ratios[-1], flush=True)
                            if W == WINDOWS[-1] and B == BATCHES[-1] and n == LENGTHS[-1]:
                                print("        (c) " + arms["c"].form)
                            del arms
                        del cache
                        torch.cuda.empty_cache()
                print("%-7s D %3d %-6s (c)/(s): min %.3f  max %.3f  mean %.3f" % (kind, D, "e4m3" if fp8 else "16-bit", min(ratios), max(ratios),
                                                                                  sum(ratios) / len(ratios)), flush=True)


if __name__ == "__main__":
    main()
