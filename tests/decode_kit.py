"""The runners of the decode GPU tests over the KV cache (a plain module: no test, no fixture), shared by tests/test_decode_gpu.py,
tests/test_kvcache_gpu.py and tests/test_d256_gpu.py: input values, caches in every layout with poison past every length, one launch
with canaries around O, L and the workspace (run for 16-bit caches, run8 for e4m3), and the comparison with the float64 model under the
bound, the tolerance and the checker of tests/decode_model.py, which tests/test_decode_sensitivity.py proves and this module takes as
they are (that test reads this file).
"""
import re

import numpy as np
import torch

import decode_model
import harness
from decode_model import MARGIN, bounds, compare, model  # noqa: F401  (the bound proven by tests/test_decode_sensitivity.py)
from metal_flash_attention_amd import (AttentionDecode, AttentionDecodeFP8, AttentionDescriptor, AttentionKernel, AttentionKernelType,
                                       AttentionOperand as Op, GEMMOperandPrecision as P, KVCacheAppend, KVCachePrecision, _abi)

DTYPE = {P.FP16: torch.float16, P.BF16: torch.bfloat16}
LOG2E = 1.4426950408889634
TOL_O, TOL_L = harness.TOL_MIXED["O"], harness.TOL_MIXED["L"]
CANARY16, CANARY32 = 0xCACA - 0x10000, 0xCACACACA - (1 << 32)   # as signed integers of the same bits
PAD = 8            # canary elements behind every O row
GUARD = 256        # canary bytes on either side of the workspace
SEEN = {}          # maxima seen, printed per test (-s)

NAN8 = 0x7F


def make_values(B, Hq, G, R, C, D, dtype, seed, shared=False):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1).to(dtype))  # noqa: E731
    q, k, v = rnd(B, Hq, R, D), rnd(1 if shared else B, Hq // G, C, D), rnd(1 if shared else B, Hq // G, C, D)
    if shared:
        k, v = k.expand(B, -1, -1, -1).contiguous(), v.expand(B, -1, -1, -1).contiguous()
    return q, k, v


def pieces_of(text):
    found = re.search(r"(\d+) pieces", text)
    return int(found.group(1)) if found else None


def planned_pieces(shape, dtype, cache, G, C, causal, workspace, decode=AttentionDecode):
    """the piece count the launch will use (the host's plan; nothing is launched), None for an unsplit launch"""
    if not workspace:
        return None
    B, Hq, R, D = shape
    prec = P.BF16 if dtype == torch.bfloat16 else P.FP16
    dec = decode(D, prec, prec)
    kw = dict(cache.kw, rows=R, column=C, heads=Hq, batches=B, headsPerKeyValue=G, causal=causal, cacheLengths=cache.lens)
    need = dec.workspaceSize(**kw)
    return pieces_of(dec.launchForm(workspace=0x4000, workspaceBytes=need, **kw)) if need else None


def needle_q(k, lens, Hq, G, R, dtype, causal, pieces=None, page=None):
    """needle queries (tests/decode_model.py) for a cache whose values, as the model sees them, are k -> (q, info)"""
    q64, info = decode_model.needle_queries(k, lens, Hq, G, R, causal, decode_model.fmt_of(dtype), pieces=pieces, page=page)
    q = torch.from_numpy(q64).to(dtype)
    assert torch.equal(q.to(torch.float64), torch.from_numpy(q64)), "needle queries are values of the 16-bit type"
    return q, info


def lengths_for(B, C, R, seed, page=64):
    rng = np.random.default_rng(seed)
    fixed = [C, R, 0, 63, 64, 65, page - 1, page + 1]
    lens = [min(C, x) for x in fixed][:B]
    lens += [int(x) for x in rng.integers(R, C + 1, size=max(0, B - len(lens)))]
    return np.array(lens, dtype=np.uint32)


class Cache:
    """K and V on the device in one of the layouts, poisoned past every length; .kw are the layout's launch arguments"""

    def __init__(self, k, v, lens, layout, seed=0):
        B, Hkv, C, D = k.shape
        dev, dtype = "cuda", k.dtype
        nan = float("nan")
        self.guards = []
        kk, vv = k.clone(), v.clone()
        if layout != "shared":
            for b in range(B):
                kk[b, :, int(lens[b]):] = nan
                vv[b, :, int(lens[b]):] = nan
        kw = {}
        if layout == "packed":
            self.k, self.v = kk.to(dev), vv.to(dev)
        elif layout == "token_major":   # [B][C][Hkv][D]
            self.k, self.v = kk.permute(0, 2, 1, 3).contiguous().to(dev), vv.permute(0, 2, 1, 3).contiguous().to(dev)
            st = (Hkv * D, D, C * Hkv * D)
            kw["strides"] = dict(K=st, V=st)
        elif layout == "fused":         # K and V as slices of one [B][Hkv][C][2][D] allocation
            self.both = torch.stack([kk, vv], dim=3).contiguous().to(dev)
            self.k, self.v = self.both[:, :, :, 0], self.both[:, :, :, 1]
            st = (2 * D, C * 2 * D, Hkv * C * 2 * D)
            kw["strides"] = dict(K=st, V=st)
        elif layout == "shared":        # zero batch stride: one cache (the longest sequence's) for the whole batch
            n = int(max(lens))
            kk[:, :, n:] = nan
            vv[:, :, n:] = nan
            self.k, self.v = kk[0].contiguous().to(dev), vv[0].contiguous().to(dev)
            st = (D, C * D, 0)
            kw["strides"] = dict(K=st, V=st)
        else:                           # "paged:<page size>": a pool [pages][Hkv][page][D], shuffled, with unnamed pages and a guard page
            ps = int(layout.split(":")[1])
            per = (C + ps - 1) // ps
            rng = np.random.default_rng(seed)
            used = [(b, i) for b in range(B) for i in range((int(lens[b]) + ps - 1) // ps)]
            pages = len(used) + 3       # three pages nobody names: all NaN
            order = rng.permutation(pages)
            poolk = torch.full((pages + 1, Hkv, ps, D), nan, dtype=dtype)
            poolv = torch.full((pages + 1, Hkv, ps, D), nan, dtype=dtype)
            table = np.full((B, per + 2), int(order[len(used)]), dtype=np.int32)   # entries past the last page name a NaN page
            for slot, (b, i) in enumerate(used):
                pg = int(order[slot])
                n = min(ps, C - i * ps)
                poolk[pg, :, :n] = kk[b, :, i * ps:i * ps + n]
                poolv[pg, :, :n] = vv[b, :, i * ps:i * ps + n]
                table[b, i] = pg
            self.poolk, self.poolv = poolk.to(dev), poolv.to(dev)
            for pool in (self.poolk, self.poolv):   # the guard page behind the pool
                pool.view(torch.int16)[pages] = CANARY16
                self.guards.append((pool.view(torch.int16)[pages], CANARY16))
            self.k, self.v = self.poolk, self.poolv
            self.table = torch.from_numpy(table).to(dev)
            kw.update(pageSize=ps, blockTable=self.table, blockTableStride=per + 2, pageStrides=(Hkv * ps * D, Hkv * ps * D),
                      strides=dict(K=(D, ps * D, 0), V=(D, ps * D, 0)))
        self.kw = kw
        self.lens = torch.from_numpy(lens.astype(np.int64)).to(torch.int32).to(dev)   # uint32 bits
        holders = [getattr(self, n) for n in ("both", "poolk", "poolv", "table") if hasattr(self, n)] or [self.k, self.v]
        self.holders = holders + [self.lens]
        self.before = [h.clone() for h in self.holders]

    def unchanged(self):
        bits = lambda t: t.view(torch.int16) if t.dtype in (torch.float16, torch.bfloat16) else t  # noqa: E731
        return all(torch.equal(bits(a), bits(b)) for a, b in zip(self.holders, self.before)) and \
            all(bool((g == c).all()) for g, c in self.guards)


def run(q, cache, G, C, causal=True, workspace=True, out32=False, want_l=True, form=None):
    """one launch -> (O fp32 [B, Hq, R, D], L fp32 [B, Hq, R] or None, O's stored bits, the launch form); checks poison and canaries"""
    B, Hq, R, D = q.shape
    prec = P.BF16 if q.dtype == torch.bfloat16 else P.FP16
    dec = AttentionDecode(D, prec, P.FP32 if out32 else prec)
    dev = "cuda"
    qd = q.to(dev)
    odt = torch.float32 if out32 else q.dtype
    ibits = torch.int32 if out32 else torch.int16
    ocan = CANARY32 if out32 else CANARY16
    o = torch.empty((B, Hq, R, D + PAD), dtype=odt, device=dev)
    o.view(ibits).fill_(ocan)
    l = torch.empty((B, Hq, R + 3), dtype=torch.float32, device=dev)
    l.view(torch.int32).fill_(CANARY32)
    strides = dict(cache.kw.get("strides", {}))
    strides["O"] = (D + PAD, R * (D + PAD), Hq * R * (D + PAD))
    kw = dict(cache.kw, rows=R, column=C, heads=Hq, batches=B, headsPerKeyValue=G, causal=causal, cacheLengths=cache.lens,
              strides=strides, lStrides=(R + 3, Hq * (R + 3)))
    need = dec.workspaceSize(**kw)
    ws = None
    if workspace and need:
        ws = torch.empty(need + 2 * GUARD, dtype=torch.uint8, device=dev)
        ws.view(torch.int16).fill_(CANARY16)
        ws[GUARD:GUARD + need].view(torch.float32).fill_(float("nan"))   # what the launch may use starts as poison
        kw.update(workspace=int(ws.data_ptr()) + GUARD, workspaceBytes=need)
    text = dec.launchForm(**kw)
    dec.dispatch(qd, cache.k, cache.v, o, l if want_l else None, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    assert cache.unchanged(), "the launch wrote K, V, the table, the lengths or the pool's guard page"
    assert bool((o.view(ibits)[..., D:] == ocan).all()), "O padding overwritten"
    assert bool((l.view(torch.int32)[..., R:] == CANARY32).all()), "L padding overwritten"
    if not want_l:
        assert bool((l.view(torch.int32) == CANARY32).all()), "L written although NULL was passed"
    if ws is not None:
        assert bool((ws[:GUARD].view(torch.int16) == CANARY16).all()) and bool((ws[GUARD + need:].view(torch.int16) == CANARY16).all()), \
            "workspace written beyond the reported size"
    ov = o[..., :D]
    assert not bool(torch.isnan(ov.float()).any()), "NaN in O"
    lv = l[..., :R].cpu() if want_l else None
    if want_l:
        assert not bool(torch.isnan(lv).any()), "NaN in L"
    return ov.float().cpu(), lv, ov.contiguous().view(ibits).cpu(), text


def check_against_model(tag, got_o, got_l, q, k, v, lens, G, causal, out32=False, pieces=None, page=None, info=None, kscale=None,
                        vscale=None):
    """the former bounds on the maxima, and the per-element bounds of tests/decode_model.py on O and on L wherever L was written;
    k, v are the cache's values without kscale / vscale when those are given"""
    ref = model(q, k, v, lens, G, causal, pieces=pieces, page=page, kscale=kscale, vscale=vscale)
    ref_o, ref_l = ref.O, ref.L
    err_o = float(np.abs(got_o.numpy().astype(np.float64) - ref_o).max())
    SEEN[tag + " O"] = max(SEEN.get(tag + " O", 0.0), err_o)
    print(f"{tag}: max |dO| = {err_o:.3e}", end="")
    err_l = 0.0
    nat_l = None
    if got_l is not None:
        gl = got_l.numpy().astype(np.float64)
        empty = np.isinf(ref_l)
        assert (gl[empty] < -1e30).all(), "an empty sequence must get a hugely negative L"
        if (~empty).any():
            err_l = float(np.abs(gl[~empty] / LOG2E - ref_l[~empty]).max())
        print(f", max |dL| = {err_l:.3e}", end="")
        nat_l = gl / LOG2E
    print()
    assert err_o <= TOL_O, (tag, err_o)
    assert err_l <= TOL_L, (tag, err_l)
    for b in np.nonzero(lens == 0)[0]:
        assert float(got_o[b].abs().max()) == 0.0, "an empty sequence must get O = 0"
    fmt = decode_model.fmt_of(q.dtype)
    ratio_o, ratio_l, text = compare(got_o.numpy(), nat_l, ref, fmt, "f32" if out32 else fmt, lens, info=info, pieces=pieces, page=page)
    print(f"RATIO {fmt} O{'32' if out32 else '16'} {'needles' if info is not None else 'plain'} | {tag} | err / bound at margin 1: "
          f"O {ratio_o * MARGIN:.3f} L {ratio_l * MARGIN:.3f}")
    assert ratio_o <= 1.0 and ratio_l <= 1.0, (tag, text)
    return err_o, err_l


def both_inputs(q, k, lens, G, causal, cache, C, workspace, page=None, decode=AttentionDecode):
    """the test's own queries, then the needle queries for the same cache and launch geometry: [(name, q, info)]"""
    B, Hq, R, _D = q.shape
    pieces = planned_pieces(q.shape, q.dtype, cache, G, C, causal, workspace, decode)
    nq, info = needle_q(k, lens, Hq, G, R, q.dtype, causal, pieces=pieces, page=page)
    return [("", q, None), (" needles", nq, info)]


def agrees_with_the_forward_kernel(prec, D, Hq, G, R, causal):
    """the parent's only route for this shape: the ordinary forward launch with headsPerKeyValue, columnLengths and causal, on the same
    buffers (sequences of length 0 left out: the forward kernel does not define them)"""
    C, B = 700, 8
    q, k, v = make_values(B, Hq, G, R, C, D, DTYPE[prec], seed=9)
    lens = lengths_for(B, C, R, seed=3)
    cache = Cache(k, v, lens, "packed")
    desc = AttentionDescriptor()
    desc.lowPrecisionInputs, desc.lowPrecisionIntermediates, desc.lowPrecisionInputType = True, False, prec
    desc.matrixDimensions = (R, C, D)
    desc.transposeState = (False, False, False, False)
    kernel = AttentionKernel(desc.kernelDescriptor(AttentionKernelType.forward))
    Hkv = Hq // G
    keep = torch.from_numpy(lens != 0)
    for name, qq, info in both_inputs(q, k, lens, G, causal, cache, C, True):
        o, l, _bits, text = run(qq, cache, G, C, causal=causal, out32=True)
        fo = torch.zeros((B, Hq, R, D), dtype=torch.float32, device="cuda")
        fl = torch.zeros((B, Hq, R), dtype=torch.float32, device="cuda")
        kernel.dispatch({Op.Q: qq.cuda(), Op.K: cache.k, Op.V: cache.v, Op.O: fo, Op.L: fl}, row=R, column=C, heads=Hq, batches=B,
                        headStrides={Op.Q: R * D, Op.K: C * D, Op.V: C * D, Op.O: R * D, Op.L: R},
                        batchStrides={Op.Q: Hq * R * D, Op.K: Hkv * C * D, Op.V: Hkv * C * D, Op.O: Hq * R * D, Op.L: Hq * R},
                        causal=causal, columnLengths=cache.lens, headsPerKeyValue=G, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        do = float((o[keep] - fo.cpu()[keep]).abs().max())
        dl = float((l[keep] - fl.cpu()[keep]).abs().max()) / LOG2E
        print(f"decode against forward {prec.name} D={D} G={G} R={R}{name}: max |dO| = {do:.3e}, max |dL| = {dl:.3e}")
        assert do <= TOL_O and dl <= TOL_L
        # each side on its own against the model (the forward launch on the sequences it defines: those with a key)
        check_against_model(f"decode side {prec.name} D={D} G={G} R={R}{name}", o, l, qq, k, v, lens, G, causal, out32=True,
                            pieces=pieces_of(text), info=info)
        some = np.nonzero(lens != 0)[0]
        sub = {(int(np.nonzero(some == b)[0][0]), h, r): x for (b, h, r), x in info.items() if b in some} if info is not None else None
        check_against_model(f"forward side {prec.name} D={D} G={G} R={R}{name}", fo.cpu()[keep], fl.cpu()[keep], qq[keep], k[keep], v[keep],
                            lens[some], G, causal, out32=True, info=sub)


# --------------------------------------------------------------------------------------------------- e4m3 caches
def quantise(x, scales):
    """[B, Hkv, C, D] 16-bit values -> e4m3 bytes (uint8) under per-head scales: torch's conversion, which tests/test_kvcache_plans.py
    shows to be mfa_kv_quantize_e4m3 for every 16-bit pattern"""
    s = torch.from_numpy(np.asarray(scales, dtype=np.float32))[None, :, None, None]
    return (x.float() / s).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


def dequantise(b, scales):
    """bytes -> float64 scale[j] x e4m3(byte)"""
    s = torch.from_numpy(np.asarray(scales, dtype=np.float64))[None, :, None, None]
    return b.view(torch.float8_e4m3fn).to(torch.float64) * s


def make_case(B, Hq, G, R, C, D, dtype, seed, shared=False):
    g = torch.Generator().manual_seed(seed)
    Hkv = Hq // G
    q = torch.randn(B, Hq, R, D, generator=g).to(dtype)
    k, v = (torch.randn(1 if shared else B, Hkv, C, D, generator=g).to(dtype) for _ in range(2))
    if shared:
        k, v = k.expand(B, -1, -1, -1).contiguous(), v.expand(B, -1, -1, -1).contiguous()
    rng = np.random.default_rng(seed)
    ks, vs = decode_model.spread_scales(rng, Hkv), decode_model.spread_scales(rng, Hkv)
    return q, quantise(k, ks), quantise(v, vs), ks, vs


class Cache8:
    """K and V bytes on the device in one of the layouts of Cache, `poison` in every byte a launch must not load"""

    def __init__(self, k, v, lens, layout, seed=0, poison=NAN8):
        B, Hkv, C, D = k.shape
        dev = "cuda"
        kk, vv = k.clone(), v.clone()
        if layout != "shared":
            for b in range(B):
                kk[b, :, int(lens[b]):] = poison
                vv[b, :, int(lens[b]):] = poison
        kw = {}
        if layout == "packed":
            self.k, self.v = kk.to(dev), vv.to(dev)
        elif layout == "token_major":
            self.k, self.v = kk.permute(0, 2, 1, 3).contiguous().to(dev), vv.permute(0, 2, 1, 3).contiguous().to(dev)
            st = (Hkv * D, D, C * Hkv * D)
            kw["strides"] = dict(K=st, V=st)
        elif layout == "fused":
            self.both = torch.stack([kk, vv], dim=3).contiguous().to(dev)
            self.k, self.v = self.both[:, :, :, 0], self.both[:, :, :, 1]
            st = (2 * D, C * 2 * D, Hkv * C * 2 * D)
            kw["strides"] = dict(K=st, V=st)
        elif layout == "shared":
            n = int(max(lens))
            kk[:, :, n:] = poison
            vv[:, :, n:] = poison
            self.k, self.v = kk[0].contiguous().to(dev), vv[0].contiguous().to(dev)
            st = (D, C * D, 0)
            kw["strides"] = dict(K=st, V=st)
        else:   # "paged:<page size>": a shuffled pool with three pages nobody names and a guard page behind it
            ps = int(layout.split(":")[1])
            per = (C + ps - 1) // ps
            rng = np.random.default_rng(seed)
            used = [(b, i) for b in range(B) for i in range((int(lens[b]) + ps - 1) // ps)]
            pages = len(used) + 3
            order = rng.permutation(pages)
            poolk = torch.full((pages + 1, Hkv, ps, D), poison, dtype=torch.uint8)
            poolv = torch.full((pages + 1, Hkv, ps, D), poison, dtype=torch.uint8)
            table = np.full((B, per + 2), int(order[len(used)]), dtype=np.int32)
            for slot, (b, i) in enumerate(used):
                pg = int(order[slot])
                n = min(ps, C - i * ps)
                poolk[pg, :, :n] = kk[b, :, i * ps:i * ps + n]
                poolv[pg, :, :n] = vv[b, :, i * ps:i * ps + n]
                table[b, i] = pg
            self.poolk, self.poolv = poolk.to(dev), poolv.to(dev)
            self.k, self.v = self.poolk, self.poolv
            self.table = torch.from_numpy(table).to(dev)
            kw.update(pageSize=ps, blockTable=self.table, blockTableStride=per + 2, pageStrides=(Hkv * ps * D, Hkv * ps * D),
                      strides=dict(K=(D, ps * D, 0), V=(D, ps * D, 0)))
        self.kw = kw
        self.lens = torch.from_numpy(lens.astype(np.int64)).to(torch.int32).to(dev)
        holders = [getattr(self, n) for n in ("both", "poolk", "poolv", "table") if hasattr(self, n)] or [self.k, self.v]
        self.holders = holders + [self.lens]
        self.before = [h.clone() for h in self.holders]

    def unchanged(self):
        return all(torch.equal(a, b) for a, b in zip(self.holders, self.before))


def run8(q, cache, G, C, ks=None, vs=None, causal=True, workspace=True, out32=False, want_l=True):
    """one FP8 launch -> (O fp32, L fp32 or None, O's stored bits, the launch form); checks NaN, canaries and that the cache is intact"""
    B, Hq, R, D = q.shape
    prec = P.BF16 if q.dtype == torch.bfloat16 else P.FP16
    dec = AttentionDecodeFP8(D, prec, P.FP32 if out32 else prec)
    dev = "cuda"
    odt, ibits, ocan = (torch.float32, torch.int32, CANARY32) if out32 else (q.dtype, torch.int16, CANARY16)
    o = torch.empty((B, Hq, R, D + PAD), dtype=odt, device=dev)
    o.view(ibits).fill_(ocan)
    l = torch.empty((B, Hq, R + 3), dtype=torch.float32, device=dev)
    l.view(torch.int32).fill_(CANARY32)
    strides = dict(cache.kw.get("strides", {}))
    strides["O"] = (D + PAD, R * (D + PAD), Hq * R * (D + PAD))
    ksd = None if ks is None else torch.from_numpy(ks).to(dev)
    vsd = None if vs is None else torch.from_numpy(vs).to(dev)
    kw = dict(cache.kw, rows=R, column=C, heads=Hq, batches=B, headsPerKeyValue=G, causal=causal, cacheLengths=cache.lens,
              strides=strides, lStrides=(R + 3, Hq * (R + 3)), keyScale=ksd, valueScale=vsd)
    need = dec.workspaceSize(**kw)
    ws = None
    if workspace and need:
        ws = torch.empty(need + 2 * GUARD, dtype=torch.uint8, device=dev)
        ws.view(torch.int16).fill_(CANARY16)
        ws[GUARD:GUARD + need].view(torch.float32).fill_(float("nan"))
        kw.update(workspace=int(ws.data_ptr()) + GUARD, workspaceBytes=need)
    text = dec.launchForm(**kw)
    dec.dispatch(q.to(dev), cache.k, cache.v, o, l if want_l else None, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    assert cache.unchanged(), "the launch wrote K, V, the table or the lengths"
    assert bool((o.view(ibits)[..., D:] == ocan).all()), "O padding overwritten"
    assert bool((l.view(torch.int32)[..., R:] == CANARY32).all()), "L padding overwritten"
    if not want_l:
        assert bool((l.view(torch.int32) == CANARY32).all()), "L written although NULL was passed"
    if ws is not None:
        assert bool((ws[:GUARD].view(torch.int16) == CANARY16).all()) and bool((ws[GUARD + need:].view(torch.int16) == CANARY16).all()), \
            "workspace written beyond the reported size"
    ov = o[..., :D]
    assert bool(torch.isfinite(ov.float()).all()), "O is not finite"
    lv = l[..., :R].cpu() if want_l else None
    if want_l:
        assert not bool(torch.isnan(lv).any()), "NaN in L"
    return ov.float().cpu(), lv, ov.contiguous().view(ibits).cpu(), text


ONES = lambda b: np.ones(b.shape[1], dtype=np.float32)  # noqa: E731


def check(tag, o, l, q, kb, vb, ks, vs, lens, G, causal, **how):
    """the model sees the bytes' own values and the scales apart, as the kernel does (how: out32, pieces, page, info)"""
    return check_against_model(tag, o, l, q, dequantise(kb, ONES(kb)), dequantise(vb, ONES(vb)), lens, G, causal,
                                     kscale=None if ks is None else ks, vscale=None if vs is None else vs, **how)


def both_inputs8(q, kb, ks, lens, G, causal, cache, C, workspace, page=None):
    """the test's own queries and the needle queries for the dequantised K: [(name, q, info)]"""
    return both_inputs(q, dequantise(kb, ONES(kb) if ks is None else ks), lens, G, causal, cache, C, workspace, page=page,
                             decode=AttentionDecodeFP8)


def contract_bytes(x, scales):
    """mfa_kv_quantize_e4m3 itself, element by element: [B, Hkv, R, D] 16-bit values -> uint8"""
    quantize = _abi.lib().mfa_kv_quantize_e4m3
    xf = x.float().numpy()
    out = np.empty(xf.shape, dtype=np.uint8)
    for j in range(xf.shape[1]):
        s = float(scales[j])
        flat = xf[:, j].reshape(-1)
        out[:, j] = np.fromiter((quantize(float(t), s) for t in flat), dtype=np.uint8, count=flat.size).reshape(xf[:, j].shape)
    return torch.from_numpy(out)


def append_writes_exactly_the_named_positions(prec, D, R, layout, fp8):
    dtype, dev = DTYPE[prec], "cuda"
    Hkv = 3
    paged = layout.startswith("paged")
    ps = int(layout.split(":")[1]) if paged else 0
    column = 3 * ps if paged else 200            # capacity of one sequence
    per = column // ps if paged else 0
    # none; fewer than R (for R = 4: the first row falls before key 0); exactly the capacity; a last page partly full; past the
    # capacity (the rows behind it are dropped); an ordinary one
    lens = np.array([0, R - 1, column, (2 * ps + 5) if paged else 77, column + 2, max(R, 9)], dtype=np.int64)
    B = len(lens)
    g = torch.Generator().manual_seed(D + R + len(layout))
    knew, vnew = (torch.randn(B, Hkv, R, D, generator=g) * 3).to(dtype), (torch.randn(B, Hkv, R, D, generator=g) * 3).to(dtype)
    knew[0, 0, 0, :4] = torch.tensor([1000.0, -1000.0, -0.0, 2.0 ** -10]).to(dtype)   # (sequence 0 is not written; 5 is)
    knew[5, 0, 0, :4] = torch.tensor([1000.0, -1000.0, -0.0, 2.0 ** -10]).to(dtype)
    ks, vs = (0.5 + 1.5 * torch.rand(Hkv, generator=g).numpy().astype(np.float32) for _ in range(2))
    edt = torch.uint8 if fp8 else torch.int16
    if fp8:
        wk, wv = contract_bytes(knew, ks), contract_bytes(vnew, vs)
    else:
        wk, wv = knew.view(torch.int16), vnew.view(torch.int16)
    # the caches, pre-filled with a byte pattern, as [slot][Hkv][keys][D] views of their buffers
    rng = np.random.default_rng(7)
    if paged:
        pages = B * per + 2
        shape_, perm = (pages, Hkv, ps, D), (0, 1, 2, 3)
        order = rng.permutation(pages)
        table = torch.from_numpy(order[:B * per].reshape(B, per).astype(np.int32))
    elif layout == "token_major":
        shape_, perm = (B, column, Hkv, D), (0, 2, 1, 3)
    else:
        shape_, perm = (B, Hkv, column, D), (0, 1, 2, 3)
    esz = 1 if fp8 else 2
    bufs = [torch.from_numpy(rng.integers(0, 256, size=int(np.prod(shape_)) * esz + 64, dtype=np.uint8)) for _ in range(2)]   # 64 guard bytes
    expect = [b.clone() for b in bufs]
    views = [e[:int(np.prod(shape_)) * esz].view(edt).view(shape_).permute(perm) for e in expect]
    for b in range(B):
        for r in range(R):
            pos = int(lens[b]) - R + r
            if pos < 0 or pos >= column:
                continue
            slot, at = (int(table[b, pos // ps]), pos % ps) if paged else (b, pos)
            views[0][slot, :, at] = wk[b, :, r]
            views[1][slot, :, at] = wv[b, :, r]
    dbufs = [b.to(dev) for b in bufs]
    kw = dict(rows=R, heads=Hkv, batches=B, cacheLengths=torch.from_numpy(lens).to(torch.int32).to(dev))
    if paged:
        kw.update(pageSize=ps, blockTable=table.to(dev), blockTableStride=per, pageStrides=(Hkv * ps * D, Hkv * ps * D))
    else:
        kw.update(column=column)
        if layout == "token_major":
            st = (Hkv * D, D, column * Hkv * D)
            kw.update(strides=dict(kCache=st, vCache=st))
    if fp8:
        kw.update(keyScale=torch.from_numpy(ks).to(dev), valueScale=torch.from_numpy(vs).to(dev))
    hold = kw.get("blockTable")
    KVCacheAppend(D, prec, KVCachePrecision.E4M3 if fp8 else None).dispatch(knew.to(dev), vnew.to(dev), dbufs[0], dbufs[1],
                                                                            stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    for name, got, want in zip("KV", dbufs, expect):
        got = got.cpu()
        wrong = torch.nonzero(got != want).flatten()
        assert wrong.numel() == 0, f"{name} cache: {wrong.numel()} bytes differ from the model, first at {wrong[:4].tolist()}"
    written = sum(1 for b in range(B) for r in range(R) if 0 <= int(lens[b]) - R + r < column)
    assert written >= 3 and not torch.equal(expect[0], bufs[0])   # the case does write something
    del hold
