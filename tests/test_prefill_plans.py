"""CPU test (no GPU call): the host side of prefill attention over a KV cache, include/mfa_prefill.h -- exported symbols, the parameter
block's layout against the library's own sizeof / offsetof, every refusal with its message, the launch-form text, the tile-range
function (the very function the kernels run: prefill_tile_range, csrc/attn_prefill16.h) against a brute-force scan of the mask, the
fake-tensor path of the torch op and the needle inputs of tests/prefill_model.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import prefill_model as pm
from metal_flash_attention_amd import AttentionPrefill, GEMMOperandPrecision as P, KVCachePrecision, MFAError, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = 0x1000   # any non-null value: the host never reads the lengths
TILE = _abi.MFA_PREFILL_KEY_TILE
UNSUPPORTED, INVALID = 3, 2


def shape(**over):
    kw = dict(rows=512, column=4096, heads=64, batches=4, headsPerKeyValue=8, cacheLengths=LENGTHS)
    kw.update(over)
    return kw


def refused(status, needle, prefill=None, **over):
    with pytest.raises(MFAError) as e:
        (prefill or AttentionPrefill(128, P.BF16)).launchForm(**shape(**over))
    assert e.value.status == status, str(e.value)
    assert needle in str(e.value), str(e.value)


def test_header_symbols_exported():
    header = open(os.path.join(ROOT, "include", "mfa_prefill.h")).read()
    declared = set(re.findall(r"\b(mfa_(?:prefill|attention_prefill)_\w+)\s*\(", header))
    handle = _abi.lib()
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in include/mfa_prefill.h but not exported"
    assert declared == {s[0] for s in _abi.PREFILL_SYMBOLS}
    assert len(declared) == 7
    for macro, value in (("MFA_PREFILL_KEY_TILE", TILE), ("MFA_PREFILL_PACKED_ROWS", _abi.MFA_PREFILL_PACKED_ROWS),
                         ("MFA_PREFILL_MAX_GROUP", _abi.MFA_PREFILL_MAX_GROUP)):
        assert re.search(r"#define %s\s+%d\b" % (macro, value), header), macro
    assert int(handle.mfa_abi_version()) == 6   # mfa.h did not change


def test_struct_mirror_matches_the_library():
    handle = _abi.lib()
    assert ctypes.sizeof(_abi.mfa_prefill_params) == int(handle.mfa_prefill_params_size())
    fields = [name for name, _t in _abi.mfa_prefill_params._fields_]
    offsets = (ctypes.c_uint32 * 64)()
    count = ctypes.c_uint32(0)
    assert handle.mfa_prefill_params_offsets(offsets, 64, ctypes.byref(count)) == 0
    assert count.value == len(fields)
    for i, name in enumerate(fields):
        assert getattr(_abi.mfa_prefill_params, name).offset == offsets[i], name
    # the header's declaration order is the mirror's
    header = open(os.path.join(ROOT, "include", "mfa_prefill.h")).read()
    body = header[header.index("typedef struct mfa_prefill_params {"):header.index("} mfa_prefill_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for n in re.findall(r"[\s\*,](\w+)(?:\[\d+\])?\s*(?=[,;])", body)]
    assert declared == fields, declared
    p = _abi.mfa_prefill_params()
    ctypes.memset(ctypes.byref(p), 0xFF, ctypes.sizeof(p))
    handle.mfa_prefill_params_init(ctypes.byref(p))
    assert (p.precision, p.outputPrecision, p.cachePrecision, p.headsPerKeyValue, p.causal, p.pageSize) == (int(P.BF16), int(P.BF16), int(P.BF16), 1, 1, 0)
    assert p.queryLengths is None and p.keyScale is None and p.valueScale is None and p.blockTableStride == 0


def test_refusals_name_the_requirement():
    e4m3 = AttentionPrefill(128, P.BF16, cachePrecision=KVCachePrecision.E4M3)
    refused(UNSUPPORTED, "16-bit Q", prefill=AttentionPrefill(128, P.FP32))
    refused(UNSUPPORTED, "64 and 128, not 96", prefill=AttentionPrefill(96, P.BF16))
    refused(UNSUPPORTED, "at most 32, not 64", headsPerKeyValue=64)
    refused(INVALID, "multiple of headsPerKeyValue", heads=60)
    for page in (8, 48, 2048):
        refused(INVALID, "power of two from 16 to 1024", pageSize=page, blockTable=0x2000, blockTableStride=4096)
    refused(INVALID, "multiples of 8 elements", strides=dict(K=(132, 4096 * 132, 8 * 4096 * 132)))      # a K stride of 4 (mod 8)
    refused(INVALID, "strides of K must be multiples of 8", strides=dict(K=(128, 4, 0)))
    refused(INVALID, "multiples of 16 elements (16-byte rows of an e4m3 cache)", prefill=e4m3, strides=dict(V=(136, 4096 * 136, 8 * 4096 * 136)))
    refused(INVALID, "strides of K must be multiples of 16", prefill=e4m3, strides=dict(K=(128, 8, 0)))
    refused(UNSUPPORTED, "e5m2", prefill=AttentionPrefill(128, P.BF16, cachePrecision=KVCachePrecision.E5M2))
    refused(INVALID, "cachePrecision must be", prefill=AttentionPrefill(128, P.BF16, cachePrecision=int(P.FP16)))
    refused(INVALID, "go with an e4m3 cache", keyScale=0x3000)
    refused(INVALID, "cacheLengths is required", cacheLengths=None)
    refused(INVALID, "needs blockTable", pageSize=64)
    refused(INVALID, "blockTableStride must hold the 64 pages", pageSize=64, blockTable=0x2000, blockTableStride=63)
    refused(INVALID, "non-zero", rows=0)
    refused(INVALID, "outputPrecision", prefill=AttentionPrefill(128, P.BF16, P.FP16))
    # pointers: checked by the launch itself, before any GPU call (the process never opens the device)
    pre = AttentionPrefill(128, P.BF16)
    for bufs, needle in (((0x10008, 0x20000, 0x30000, 0x40000, None), "16-byte aligned"), ((0x10000, 0x20000, 0x30004, 0x40000, None), "16-byte aligned"),
                         ((0x10000, 0x20000, 0x30000, 0x40000, 0x50002), "L must be 4-byte aligned"), ((0, 0x20000, 0x30000, 0x40000, None), "null argument")):
        with pytest.raises(MFAError) as e:
            pre.dispatch(*bufs, **shape())
        assert e.value.status == INVALID and needle in str(e.value), str(e.value)
    with pytest.raises(MFAError) as e:
        e4m3.dispatch(0x10000, 0x20000, 0x30000, 0x40000, None, keyScale=0x3002, **shape())
    assert e.value.status == INVALID and "keyScale and valueScale must be 4-byte aligned" in str(e.value)


@pytest.mark.parametrize("G,RB", [(1, 128), (8, 16), (3, 42)])
def test_launch_form_names_the_kernel_and_grid(G, RB):
    heads, B, rows = 24, 2, 300
    blocks = -(-rows // RB)
    for prec, tn in ((P.BF16, "bf16"), (P.FP16, "f16")):
        for D in (64, 128):
            for fp8 in (False, True):
                pre = AttentionPrefill(D, prec, cachePrecision=KVCachePrecision.E4M3 if fp8 else None)
                for paged in (False, True):
                    kw = dict(pageSize=16, blockTable=0x2000, blockTableStride=256) if paged else {}
                    text = pre.launchForm(**shape(rows=rows, heads=heads, batches=B, headsPerKeyValue=G, **kw))
                    name = "attn_prefill16_d%d_%s%s" % (D, tn, "_e4m3" if fp8 else "")
                    assert text == "%s (grid %d = %d sequences x %d K/V heads x %d row blocks of %d rows x %d heads, %s)" % (
                        name, B * (heads // G) * blocks, B, heads // G, blocks, RB, G, "paged" if paged else "contiguous"), text
    # G x rows <= 32, decode's territory, is accepted too
    assert "1 row blocks of 16 rows" in AttentionPrefill(128, P.BF16).launchForm(**shape(rows=4))


def brute_force(n, qn, r0, RB, causal):
    """(visible [rows, n] for the live rows of the block) from the mask rule of include/mfa_prefill.h"""
    rows = np.arange(r0, min(r0 + RB, qn))[:, None]
    cols = np.arange(n)[None, :]
    vis = np.broadcast_to(cols < n, (rows.shape[0], n)).copy()
    if causal:
        vis &= cols <= rows + max(n - qn, 0)
    return vis


@pytest.mark.parametrize("causal", [True, False])
def test_tile_range_against_the_mask(causal):
    for n in (0, 1, 63, 64, 65, 127, 128, 129, 1000):
        for qn in (1, 16, 42, 128, 200):
            for RB in (128, 16, 42):
                for r0 in range(0, qn + RB, RB):   # (one block past the last live row too)
                    f, e = AttentionPrefill.tileRange(n, qn, r0, RB, causal)
                    vis = brute_force(n, qn, r0, RB, causal)
                    tiles = -(-n // TILE)
                    seen = [bool(vis[:, t * TILE:(t + 1) * TILE].any()) for t in range(tiles)] if vis.size else []
                    want_end = max([t + 1 for t, s in enumerate(seen) if s], default=0)
                    assert e == want_end, (n, qn, r0, RB, causal, f, e, want_end)     # every visible key below, and the smallest such bound
                    assert 0 <= f <= e
                    for t in range(f):                                                # unmasked tiles hold no masked (row, key)
                        assert vis[:, t * TILE:(t + 1) * TILE].all() and (t + 1) * TILE <= n, (n, qn, r0, RB, causal, f, e, t)
                    full = [t for t in range(tiles) if (t + 1) * TILE <= n and vis[:, t * TILE:(t + 1) * TILE].all()] if vis.size else []
                    assert f == len(full), (n, qn, r0, RB, causal, f, full)           # and every such tile is found
    with pytest.raises(MFAError):
        AttentionPrefill.tileRange(64, 64, 0, 0, True)


def test_fake_tensor_path_gives_shapes_without_a_device():
    torch = pytest.importorskip("torch")
    from torch._subclasses.fake_tensor import FakeTensorMode
    from metal_flash_attention_amd import torch_binding as tb
    if not tb._HAVE_PREFILL_OP:
        pytest.skip("this torch has no torch.library.custom_op")
    with FakeTensorMode():
        q = torch.empty((2, 8, 300, 128), dtype=torch.bfloat16, device="cuda")
        k = torch.empty((2, 2, 1024, 128), dtype=torch.float8_e4m3fn, device="cuda")
        lens = torch.empty((2,), dtype=torch.int32, device="cuda")
        scale = torch.empty((2,), dtype=torch.float32, device="cuda")
        o, l = torch.ops.mfa.attention_prefill(q, k, k, lens, lens, None, True, scale, scale)
        assert o.shape == (2, 8, 300, 128) and o.dtype == torch.bfloat16 and l.shape == (2, 8, 300) and l.dtype == torch.float32
        assert tb.flash_prefill(q, k, k, lens, k_scale=scale).shape == (2, 8, 300, 128)
        o, lse = tb.flash_prefill(q.half(), k, k, lens, q_lengths=lens, return_lse=True)
        assert o.dtype == torch.float16 and lse.shape == (2, 8, 300)


def test_model_adds_the_longer_chain():
    import decode_model as dm
    assert pm.chain_prefill(1000) == 34 * 32 + 4 and dm.chain_length(1000, None) == 34 * 8 + 10
    rng = np.random.default_rng(0)
    q, k, v = (dm.round_to(rng.uniform(-1, 1, s), "bf16") for s in ((1, 2, 5, 64), (1, 1, 300, 64), (1, 1, 300, 64)))
    ref = pm.model(q, k, v, [300], [3], 2, True)
    base = dm.model(q[:, :, :3], k, v, [300], 2, True)
    x = pm.extra_chain(300)
    assert x == (34 * 10 + 4 - (34 * 3 + 10)) * dm.U32
    assert np.array_equal(ref.O[:, :, :3], base.O) and np.allclose(ref.E[:, :, :3], base.E + x * (base.A + np.abs(base.O)), rtol=1e-15, atol=0)
    assert np.allclose(ref.EL[:, :, :3], base.EL + x, rtol=1e-15, atol=0)
    assert not ref.O[:, :, 3:].any() and np.isinf(ref.L[:, :, 3:]).all()


@pytest.mark.parametrize("G,causal", [(1, True), (8, True), (3, False)])
def test_needles_cover_the_geometry(G, causal):
    import decode_model as dm
    rng = np.random.default_rng(1)
    Hq, D, page = 2 * G, 64, 16
    lens, qlens = [300, 65, 1500], [129, 70, 40]
    k = dm.round_to(rng.uniform(-1, 1, (3, 2, 1500, D)), "bf16")
    q, info = pm.needle_queries(k, lens, qlens, Hq, G, 129, causal, "bf16", page=page)
    RB = 128 // G
    for b, (n, qn) in enumerate(zip(lens, qlens)):
        keys = set()
        for (bb, h, r), (weights, forbidden) in info.items():
            if bb != b:
                continue
            fr = min(r + max(n - qn, 0), n - 1) if causal else n - 1
            assert fr in weights and (fr == 0 or fr - 1 in weights) and max(weights) <= fr
            assert forbidden == (fr + 1 if causal and fr + 1 < n else None)
            keys |= set(weights)
        reach = max(min(qn - 1 + max(n - qn, 0), n - 1) if causal else n - 1, 0)
        want = {0, 15, 16, 63, 64, (n - 1) // TILE * TILE} | {p0 for p0 in range(0, n, page)} | {min(p0 + page, n) - 1 for p0 in range(0, n, page)}
        for r0 in range(0, qn, RB):
            f, e = AttentionPrefill.tileRange(n, qn, r0, RB, causal)
            want |= {f * TILE - 1, f * TILE, e * TILE - 1, (e - 1) * TILE}
        want = {t for t in want if 0 <= t <= reach}
        assert want <= keys, (b, sorted(want - keys))
