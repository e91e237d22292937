"""GPU test: decode attention over a KV cache through the C ABI of include/mfa_decode.h.

Expected values: a float64 numpy attention (softmax in natural units per (batch, head) over the first len_b keys, the mask rule of
mfa_decode.h) on the inputs after their rounding to the 16-bit type.  Tolerances: tests/harness.py TOL_MIXED (O 5e-2, L 7e-3 after
dividing by log2 e).  Every launch of this file runs on poisoned buffers: NaN in every key and value at or past each length (for
paged caches also in the tail of last pages and in pages the table does not name), the 0xCACA canary in the padding of O and L,
around the workspace and in a guard page behind the pool; after every launch no output holds a NaN, the canaries are intact and K,
V, the table and the lengths are byte-identical to before.

Beside those bounds every comparison with the model is held to the per-element bounds of tests/decode_model.py (derived from the
number formats; tests/test_decode_sensitivity.py proves on the CPU that they flag every named defect), and every test also runs
with that module's needle queries, in which single keys -- the first and last of every step, piece and page, each row's causal
frontier -- carry a visible share of the softmax, and the key just behind a row's frontier would take the row over.  Non-causal
launches have no such forbidden key: every key below the length is visible to every row.

Maxima seen on an MI355X are recorded in DESIGN.md 4.9.
"""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import decode_model  # noqa: E402
import harness  # noqa: E402
from decode_model import MARGIN, bounds, compare, model  # noqa: E402,F401  (the bound proven by tests/test_decode_sensitivity.py)
from metal_flash_attention_amd import (AttentionDecode, AttentionDescriptor, AttentionKernel, AttentionKernelType,  # noqa: E402
                                       AttentionOperand as Op, GEMMOperandPrecision as P)

DTYPE = {P.FP16: torch.float16, P.BF16: torch.bfloat16}
LOG2E = 1.4426950408889634
TOL_O, TOL_L = harness.TOL_MIXED["O"], harness.TOL_MIXED["L"]
CANARY16, CANARY32 = 0xCACA - 0x10000, 0xCACACACA - (1 << 32)   # as signed integers of the same bits
PAD = 8            # canary elements behind every O row
GUARD = 256        # canary bytes on either side of the workspace
SEEN = {}          # maxima seen, printed per test (-s)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield


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


PARITY = [(prec, D, Hq, G, R) for prec in (P.BF16, P.FP16) for D in (64, 128) for Hq, G in ((8, 1), (8, 4), (32, 8), (16, 16))
          for R in (1, 2, 4) if G * R <= 32]


@pytest.mark.parametrize("index,case", list(enumerate(PARITY)), ids=lambda x: "-".join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_parity_with_the_float64_model(index, case):
    prec, D, Hq, G, R = case
    C, B = 600, 10
    q, k, v = make_values(B, Hq, G, R, C, D, DTYPE[prec], seed=100 + index)
    lens = lengths_for(B, C, R, seed=index, page=256)
    cache = Cache(k, v, lens, "packed")
    for variant in range(4):   # causal x workspace, with FP32 O and a NULL L rotating over the cases
        causal, workspace = bool(variant & 1), bool(variant & 2)
        out32, want_l = bool((index + variant) & 1), (index + variant) % 3 != 0
        for name, qq, info in both_inputs(q, k, lens, G, causal, cache, C, workspace):
            o, l, _bits, text = run(qq, cache, G, C, causal=causal, workspace=workspace, out32=out32, want_l=want_l)
            assert ("_pieces" in text) == workspace, text
            check_against_model(f"{prec.name} D={D} Hq={Hq} G={G} R={R} causal={causal} split={workspace} O32={out32}{name}", o, l, qq,
                                k, v, lens, G, causal, out32=out32, pieces=pieces_of(text), info=info)


@pytest.mark.parametrize("page", [16, 64, 256])
@pytest.mark.parametrize("prec,D,Hq,G,R", [(P.BF16, 128, 32, 8, 1), (P.FP16, 64, 8, 4, 4), (P.BF16, 64, 16, 16, 2)])
def test_paged_equals_contiguous_bit_for_bit(prec, D, Hq, G, R, page):
    C, B = 1000, 9
    q, k, v = make_values(B, Hq, G, R, C, D, DTYPE[prec], seed=page + D)
    lens = lengths_for(B, C, R, seed=page, page=page)
    for workspace in (False, True):
        packed, paged = Cache(k, v, lens, "packed"), Cache(k, v, lens, f"paged:{page}", seed=page)
        for name, qq, info in both_inputs(q, k, lens, G, True, paged, C, workspace, page=page):
            o0, l0, b0, t0 = run(qq, packed, G, C, workspace=workspace)
            o1, l1, b1, t1 = run(qq, paged, G, C, workspace=workspace)
            assert t0.replace("contiguous", "paged") == t1, (t0, t1)   # the same kernels and piece count
            assert torch.equal(b0, b1), "O differs between the paged and the contiguous cache"
            assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)), "L differs between the paged and the contiguous cache"
            check_against_model(f"paged {page} {prec.name} D={D} split={workspace}{name}", o1, l1, qq, k, v, lens, G, True,
                                pieces=pieces_of(t1), page=page, info=info)


@pytest.mark.parametrize("prec,D", [(P.BF16, 128), (P.FP16, 64)])
def test_split_against_unsplit(prec, D):
    Hq, G, R, C, B = 16, 8, 2, 4096, 3
    q, k, v = make_values(B, Hq, G, R, C, D, DTYPE[prec], seed=5)
    lens = np.array([C, 1500, 65], dtype=np.uint32)
    cache = Cache(k, v, lens, "packed")
    for name, qq, info in both_inputs(q, k, lens, G, True, cache, C, True):
        o0, l0, _b, t0 = run(qq, cache, G, C, workspace=False, out32=True)
        o1, l1, _b, t1 = run(qq, cache, G, C, workspace=True, out32=True)
        assert "_single" in t0 and "_pieces" in t1 and "_combine" in t1, (t0, t1)
        do, dl = float((o0 - o1).abs().max()), float((l0 - l1).abs().max())
        print(f"split against unsplit {prec.name} D={D}{name}: max |dO| = {do:.3e} (fp32 O), max |dL| = {dl:.3e}; {t1}")
        assert do <= TOL_O and dl / LOG2E <= TOL_L
        # each side on its own against the model: with FP32 O this is what gives the comparison a meaning
        check_against_model(f"unsplit side {prec.name} D={D}{name}", o0, l0, qq, k, v, lens, G, True, out32=True, info=info)
        check_against_model(f"split side {prec.name} D={D}{name}", o1, l1, qq, k, v, lens, G, True, out32=True, pieces=pieces_of(t1), info=info)


@pytest.mark.parametrize("prec,D,Hq,G,R,causal", [(P.BF16, 128, 32, 8, 1, True), (P.FP16, 64, 8, 4, 4, True), (P.BF16, 64, 8, 1, 2, False)])
def test_agrees_with_the_forward_kernel(prec, D, Hq, G, R, causal):
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


@pytest.mark.parametrize("layout", ["token_major", "fused", "shared"])
@pytest.mark.parametrize("prec,D,Hq,G,R", [(P.BF16, 128, 16, 8, 2), (P.FP16, 64, 8, 2, 1)])
def test_strided_layouts_are_bit_identical_to_packed(prec, D, Hq, G, R, layout):
    C, B = 900, 8
    q, k, v = make_values(B, Hq, G, R, C, D, DTYPE[prec], seed=21, shared=layout == "shared")
    lens = lengths_for(B, C, R, seed=4)
    for workspace in (False, True):
        packed, other = Cache(k, v, lens, "packed"), Cache(k, v, lens, layout)
        for name, qq, info in both_inputs(q, k, lens, G, True, other, C, workspace):
            o0, l0, b0, _t = run(qq, packed, G, C, workspace=workspace)
            o1, l1, b1, t1 = run(qq, other, G, C, workspace=workspace)
            assert torch.equal(b0, b1) and torch.equal(l0.view(torch.int32), l1.view(torch.int32)), layout
            check_against_model(f"{layout} {prec.name} D={D} split={workspace}{name}", o1, l1, qq, k, v, lens, G, True,
                                pieces=pieces_of(t1), info=info)


def test_one_long_sequence_split():
    Hq, G, R, C, D = 64, 8, 1, 32768, 128
    q, k, v = make_values(1, Hq, G, R, C, D, torch.bfloat16, seed=77)
    lens = np.array([C], dtype=np.uint32)
    cache = Cache(k, v, lens, "packed")
    for name, qq, info in both_inputs(q, k, lens, G, True, cache, C, True):
        o, l, _bits, text = run(qq, cache, G, C, workspace=True)
        assert "_pieces" in text and "64 pieces" in text, text
        check_against_model("long B=1 Hq=64 G=8 D=128 C=32768" + name, o, l, qq, k, v, lens, G, True, pieces=64, info=info)
        if info is not None:   # every piece's first and last key is some row's needle
            keys = decode_model.needle_keys(info)[0]
            assert all(b in keys and e - 1 in keys for b, e in decode_model.piece_ranges(C, 64)), "a piece boundary without a needle"


# packed groups at the edges of the 32-wide tile: G R = 32 exactly; G R odd (the columns >= M repeat the last one: O's padding and
# the rows of the next head are checked by run()'s canaries and by the model); fewer keys than rows
@pytest.mark.parametrize("prec,D,Hq,G,R", [(P.BF16, 128, 16, 8, 4), (P.FP16, 64, 32, 16, 2), (P.BF16, 64, 6, 3, 1), (P.FP16, 128, 10, 5, 3),
                                           (P.BF16, 128, 7, 7, 1)])
def test_packed_groups_of_exactly_32_and_of_odd_size(prec, D, Hq, G, R):
    C, B = 600, 8
    assert G * R == 32 or (G * R) % 2 == 1
    q, k, v = make_values(B, Hq, G, R, C, D, DTYPE[prec], seed=31 + G)
    lens = lengths_for(B, C, R, seed=G, page=256)
    cache = Cache(k, v, lens, "packed")
    for workspace in (False, True):
        for causal in (True, False):
            for name, qq, info in both_inputs(q, k, lens, G, causal, cache, C, workspace):
                o, l, _bits, text = run(qq, cache, G, C, causal=causal, workspace=workspace)
                check_against_model(f"M={G * R} {prec.name} D={D} G={G} R={R} causal={causal} split={workspace}{name}", o, l, qq, k, v, lens,
                                    G, causal, pieces=pieces_of(text), info=info)


@pytest.mark.parametrize("prec,D,Hq,G,R", [(P.BF16, 128, 8, 4, 4), (P.FP16, 64, 4, 1, 4)])
def test_fewer_keys_than_rows(prec, D, Hq, G, R):
    """n < R: max(n - R, 0) = 0, row r sees the keys c <= r below the length"""
    C = 600
    lens = np.array([1, 2, 3, 4, 0, 5, 600], dtype=np.uint32)
    B = len(lens)
    q, k, v = make_values(B, Hq, G, R, C, D, DTYPE[prec], seed=47)
    cache = Cache(k, v, lens, "packed")
    for workspace in (False, True):
        for causal in (True, False):
            for name, qq, info in both_inputs(q, k, lens, G, causal, cache, C, workspace):
                o, l, _bits, text = run(qq, cache, G, C, causal=causal, workspace=workspace, out32=causal)
                check_against_model(f"n < R {prec.name} D={D} G={G} R={R} causal={causal} split={workspace}{name}", o, l, qq, k, v, lens, G,
                                    causal, out32=causal, pieces=pieces_of(text), info=info)
