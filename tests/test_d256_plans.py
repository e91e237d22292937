"""CPU test (no GPU call): head dimension 256 over the KV cache.

  (a) the host side plans D = 256 instead of refusing it: decode, prefill and append select the d256 kernels, the workspace follows the
      one formula, and piece counts, grids, row blocks and ragged slots are those of D = 128 for the same shape -- the launch form of
      D = 256 is the text of D = 128 with the kernels' names changed.  D = 96 and D = 512 are still refused, in words that name 256.
  (b) the bound of tests/decode_model.py carries to D = 256: the rounding-emulated reference stays at or below MARGIN / 2 of the bound
      at margin 1 on needle inputs, for every case of CASES;
  (c) two mutants of what is new at this width -- V's d blocks 4 and 5 exchanged, K's columns 128 .. 255 never contracted -- break the
      bound at MARGIN on every one of those cases.  They are built by handing model() altered inputs; no wrong kernel is ever run.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

import decode_model as dm  # noqa: E402
import test_decode_sensitivity as tds  # noqa: E402  (its cache values: the two input families of the GPU files)
from metal_flash_attention_amd import (AttentionDecode, AttentionDecodeFP8, AttentionPrefill, GEMMOperandPrecision as P, KVCacheAppend,  # noqa: E402
                                       KVCachePrecision, MFAError)

UNSUPPORTED, INVALID = 3, 2
LENGTHS, TABLE, LOGITS, STARTS, WORKSPACE = 0x1000, 0x2000, 0x3000, 0x5000, 0x4000   # non-null: the host never reads them
TYPES = ((P.BF16, "bf16"), (P.FP16, "f16"))
FAMILIES = (("", {}), ("w", dict(window=130)), ("s", dict(window=130, sinkTokens=4, sinkLogits=LOGITS)))


def dshape(**over):
    kw = dict(rows=1, column=4096, heads=64, batches=4, headsPerKeyValue=8, cacheLengths=LENGTHS)
    kw.update(over)
    return kw


def pshape(**over):
    kw = dict(rows=300, column=4096, heads=24, batches=5, headsPerKeyValue=8, cacheLengths=LENGTHS)
    kw.update(over)
    return kw


def refused(status, needle, call, *args, **kw):
    with pytest.raises(MFAError) as e:
        call(*args, **kw)
    assert e.value.status == status, str(e.value)
    assert needle in str(e.value), str(e.value)


def decoder(D, prec, fp8):
    return AttentionDecodeFP8(D, prec) if fp8 else AttentionDecode(D, prec)


# ------------------------------------------------------------------------------------------------------------------------- (a)
def test_decode_plans_select_the_d256_kernels():
    for prec, tn in TYPES:
        for fp8 in (False, True):
            bits = "8" if fp8 else "16"
            for infix, extra in FAMILIES:
                wide, ref = decoder(256, prec, fp8), decoder(128, prec, fp8)
                for shape in (dshape(), dshape(batches=1, column=32768), dshape(rows=4, batches=3, column=1024), dshape(heads=8, headsPerKeyValue=1),
                              dshape(pageSize=16, blockTable=TABLE, blockTableStride=256, batches=2)):
                    kw = dict(shape, **extra)
                    need, need128 = wide.workspaceSize(**kw), ref.workspaceSize(**kw)
                    single = wide.launchForm(**kw)
                    assert single.startswith("attn_decode%s%s_d256_%s_single (" % (bits, infix, tn)), single
                    assert single.replace("_d256_", "_d128_") == ref.launchForm(**kw)
                    if not need:
                        assert not need128
                        continue
                    split = wide.launchForm(workspace=WORKSPACE, workspaceBytes=need, **kw)
                    assert split.startswith("attn_decode%s%s_d256_%s_pieces (" % (bits, infix, tn)), split
                    assert "+ attn_decode16_d256_%s_combine (" % tn in split, split
                    # the piece count is D = 128's, the workspace the one formula: pieces x B x Hq x R x (D + 2) x 4
                    assert split.replace("_d256_", "_d128_") == ref.launchForm(workspace=WORKSPACE, workspaceBytes=need128, **kw)
                    pieces = int(split.split(" pieces")[0].split()[-1])
                    assert need == pieces * kw["batches"] * kw["heads"] * kw["rows"] * (256 + 2) * 4
                    assert need128 == pieces * kw["batches"] * kw["heads"] * kw["rows"] * (128 + 2) * 4
                    refused(INVALID, "needs %d" % need, wide.launchForm, workspace=WORKSPACE, workspaceBytes=need - 4, **kw)
    # one sequence, 8 K / V heads, 32768 keys: 64 pieces, as at every other width
    assert AttentionDecode(256).workspaceSize(**dshape(batches=1, column=32768)) == 64 * 64 * 258 * 4


def test_prefill_plans_select_the_d256_kernels():
    for prec, tn in TYPES:
        for fp8 in (False, True):
            wide, ref = (AttentionPrefill(D, prec, cachePrecision=KVCachePrecision.E4M3 if fp8 else None) for D in (256, 128))
            ragged = dict(rowStarts=STARTS, totalRows=471)
            for infix, extra in FAMILIES + (("r", ragged), ("r", dict(ragged, window=65, sinkTokens=4, sinkLogits=LOGITS))):
                for shape in (pshape(), pshape(headsPerKeyValue=1), pshape(headsPerKeyValue=3), pshape(pageSize=16, blockTable=TABLE, blockTableStride=256)):
                    kw = dict(shape, **extra)
                    text = wide.launchForm(**kw)
                    assert text.startswith("attn_prefill16%s_d256_%s%s (" % (infix, tn, "_e4m3" if fp8 else "")), text
                    assert text.replace("_d256_", "_d128_") == ref.launchForm(**kw)   # grid, row blocks and slots do not depend on D
    assert AttentionPrefill(256, P.BF16).launchForm(rows=300, column=4096, heads=24, batches=2, headsPerKeyValue=8, cacheLengths=LENGTHS) == \
        "attn_prefill16_d256_bf16 (grid 114 = 2 sequences x 3 K/V heads x 19 row blocks of 16 rows x 8 heads, contiguous)"
    slots = AttentionPrefill.raggedSlots(471, 5, 300, 16)
    assert "grid %d = %d slots x 3 K/V heads" % (3 * slots, slots) in AttentionPrefill(256, P.FP16).launchForm(**pshape(rowStarts=STARTS, totalRows=471))


def test_append_takes_d256_and_the_refusals_name_it():
    bufs = (0x10000, 0x20000, 0x30000, 0x40000)
    ashape = dict(rows=4, heads=8, batches=4, column=4096, cacheLengths=LENGTHS)
    for prec, _tn in TYPES:
        for cache in (None, KVCachePrecision.E4M3):
            for extra in ({}, dict(rowStarts=STARTS, totalRows=11)):
                # D = 256 passes every check of the plan: what is refused is the misaligned buffer, before any GPU call
                refused(INVALID, "16-byte aligned", KVCacheAppend(256, prec, cache).dispatch, 0x10000, 0x20008, 0x30000, 0x40000, **ashape, **extra)
                for D in (96, 512):
                    refused(UNSUPPORTED, "head dimensions 256, 64 and 128, not %d" % D, KVCacheAppend(D, prec, cache).dispatch, *bufs, **ashape, **extra)
    for D in (96, 512):
        for fp8 in (False, True):
            for _infix, extra in FAMILIES:
                refused(UNSUPPORTED, "head dimensions 256, 64 and 128, not %d" % D, decoder(D, P.BF16, fp8).launchForm, **dshape(**extra))
                refused(UNSUPPORTED, "head dimensions 256, 64 and 128, not %d" % D, decoder(D, P.BF16, fp8).workspaceSize, **dshape(**extra))
                pre = AttentionPrefill(D, P.FP16, cachePrecision=KVCachePrecision.E4M3 if fp8 else None)
                refused(UNSUPPORTED, "head dimensions 256, 64 and 128, not %d" % D, pre.launchForm, **pshape(**extra))
        refused(UNSUPPORTED, "head dimensions 256, 64 and 128, not %d" % D, AttentionPrefill(D).launchForm, **pshape(rowStarts=STARTS, totalRows=471))


# ------------------------------------------------------------------------------------------------------------------- (b) and (c)
D = 256
KEYS = (1, 31, 33, 129, 700)
GROUPS = ((1, 4), (4, 2), (8, 4), (3, 1), (8, 1))   # (G, R): n < R at one key; ordinary; G R = 32; odd; the generation step


def cases():
    out = []
    for family in tds.FAMILIES:
        for n in KEYS:
            for G, R in GROUPS:
                for causal in (True, False):
                    for page in (None, 16):
                        out.append(dict(family=family, n=n, D=D, G=G, R=R, Hkv=2, B=1, causal=causal, pieces=None, page=page, scales=family == "fp8"))
    return out


CASES = cases()
_PROBLEMS = {}


def problem(index, fmt):
    """(q, k, v, lens, keyword arguments of model(), info, the Reference) of CASES[index] in the 16-bit type `fmt`, computed once"""
    if (index, fmt) not in _PROBLEMS:
        case = CASES[index]
        k, v, ks, vs = tds.cache_values(case, fmt, 1000 + index)
        lens = np.full(case["B"], case["n"])
        geo = dict(pieces=None, page=case["page"], kscale=ks, vscale=vs)
        keff = k if ks is None else k * ks.astype(np.float64)[None, :, None, None]
        q, info = dm.needle_queries(keff, lens, case["G"] * case["Hkv"], case["G"], case["R"], case["causal"], fmt, page=case["page"])
        _PROBLEMS[(index, fmt)] = (q, k, v, lens, geo, info, dm.model(q, k, v, lens, case["G"], case["causal"], **geo))
    return _PROBLEMS[(index, fmt)]


@pytest.mark.parametrize("n", KEYS)
def test_the_bound_carries_to_d256(n):
    worst = 0.0
    for index, case in enumerate(CASES):
        if case["n"] != n:
            continue
        for fmt in ("bf16", "f16"):
            q, k, v, lens, geo, info, ref = problem(index, fmt)
            eo, el = dm.emulated(q, k, v, lens, case["G"], case["causal"], fmt, kscale=geo["kscale"], vscale=geo["vscale"])
            for out in (fmt, "f32"):
                ro, rl, text = dm.compare(dm.store(eo, out), el, ref, fmt, out, lens, margin=1, info=info, page=geo["page"])
                worst = max(worst, ro, rl)
                assert ro <= dm.MARGIN / 2.0 and rl <= dm.MARGIN / 2.0, (tds.case_id(case), case["G"], case["R"], fmt, out, text)
    print("D = 256, %d keys: the emulated reference at margin 1: worst %.3f of the bound" % (n, worst))


def v_blocks_4_and_5_exchanged(k, v):
    """what a V image whose d blocks 4 and 5 changed places would feed the second product: columns 128 .. 159 <-> 160 .. 191"""
    w = v.copy()
    w[..., 128:160], w[..., 160:192] = v[..., 160:192], v[..., 128:160]
    return k, w


def k_upper_half_zeroed(k, v):
    """what a contraction that stops at d = 128 computes: the second half of the K loads, or of the parked Q fragments, never used"""
    z = k.copy()
    z[..., 128:] = 0.0
    return z, v


@pytest.mark.parametrize("mutant", [v_blocks_4_and_5_exchanged, k_upper_half_zeroed], ids=lambda f: f.__name__)
def test_the_mutants_of_the_new_width_break_the_bound(mutant):
    weakest = np.inf
    for index, case in enumerate(CASES):
        q, k, v, lens, geo, info, ref = problem(index, "bf16")
        with np.errstate(all="ignore"):
            bad = dm.model(q, *mutant(k, v), lens, case["G"], case["causal"], **geo)
        gl = np.where(np.isfinite(bad.L), bad.L, -1e38)
        ro, rl, text = dm.compare(bad.O, gl, ref, "bf16", "bf16", lens, info=info, page=geo["page"])   # the widest bound of the four
        weakest = min(weakest, max(ro, rl))
        assert ro > 1.0 or rl > 1.0, (mutant.__name__, tds.case_id(case), case["G"], case["R"], text)
    print("%s: the weakest case exceeds the bound at MARGIN %.0f times" % (mutant.__name__, weakest))
