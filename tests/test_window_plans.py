"""CPU test (no GPU call): the host side of sliding-window attention over a KV cache, include/mfa_window.h -- exported symbols, window 0
as the plain launch, every refusal with its message, the launch-form texts and the piece plan, and the two range functions (the very
functions the kernels run: decode_window_piece_range, csrc/attn_decode16.h, and prefill_window_tile_range, csrc/attn_prefill16.h)
against brute-force scans of the mask; the fake-tensor path of the two torch ops."""
import os
import re

import numpy as np
import pytest

from metal_flash_attention_amd import AttentionDecode, AttentionDecodeFP8, AttentionPrefill, GEMMOperandPrecision as P, KVCachePrecision, MFAError, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = 0x1000   # any non-null value: the host never reads the lengths
TILE = 64
UNSUPPORTED, INVALID = 3, 2


def dshape(**over):
    kw = dict(rows=1, column=32768, heads=64, batches=1, headsPerKeyValue=8, cacheLengths=LENGTHS)
    kw.update(over)
    return kw


def pshape(**over):
    kw = dict(rows=512, column=4096, heads=64, batches=4, headsPerKeyValue=8, cacheLengths=LENGTHS)
    kw.update(over)
    return kw


def refused(status, needle, call, **kw):
    with pytest.raises(MFAError) as e:
        call(**kw)
    assert e.value.status == status, str(e.value)
    assert needle in str(e.value), str(e.value)


def test_header_symbols_exported():
    header = open(os.path.join(ROOT, "include", "mfa_window.h")).read()
    assert '#include "mfa_prefill.h"' in header
    declared = set(re.findall(r"\b(mfa_attention_(?:decode|prefill)_window_\w+)\s*\(", header))
    handle = _abi.lib()
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in include/mfa_window.h but not exported"
    assert declared == {s[0] for s in _abi.WINDOW_SYMBOLS}
    assert len(declared) == 9
    assert int(handle.mfa_abi_version()) == 6   # mfa.h did not change


def test_window_zero_is_the_plain_launch():
    for D, prec in ((64, P.FP16), (128, P.BF16)):
        for cls in (AttentionDecode, AttentionDecodeFP8):
            dec = cls(D, prec)
            for kw in (dshape(), dshape(workspace=0x100000, workspaceBytes=1 << 30), dshape(rows=4, column=300, pageSize=16, blockTable=0x2000, blockTableStride=32)):
                assert dec.launchForm(window=0, **kw) == dec.launchForm(**kw)
                assert dec.workspaceSize(window=0, **kw) == dec.workspaceSize(**kw)
                assert "window" not in dec.launchForm(window=0, **kw)
        for cache in (None, KVCachePrecision.E4M3):
            pre = AttentionPrefill(D, prec, cachePrecision=cache)
            assert pre.launchForm(window=0, **pshape()) == pre.launchForm(**pshape())
    # only 0 does that: a window past every key still runs the window kernels
    assert AttentionDecode(128, P.BF16).launchForm(window=2 ** 32 - 1, **dshape()).startswith("attn_decode16w_d128_bf16_single ")
    assert AttentionPrefill(128, P.BF16).launchForm(window=4096 + 512, **pshape()).startswith("attn_prefill16w_d128_bf16 ")
    # window 0 without causal is a plain non-causal launch, not a refusal
    assert AttentionDecode(128, P.BF16).launchForm(window=0, causal=False, **dshape()) == AttentionDecode(128, P.BF16).launchForm(causal=False, **dshape())


def test_refusals_name_the_requirement():
    dec, dec8, pre = AttentionDecode(128, P.BF16), AttentionDecodeFP8(128, P.BF16), AttentionPrefill(128, P.BF16)
    e4m3 = AttentionPrefill(128, P.BF16, cachePrecision=KVCachePrecision.E4M3)
    for call, shape in ((dec.launchForm, dshape), (dec.workspaceSize, dshape), (dec8.launchForm, dshape), (pre.launchForm, pshape), (e4m3.launchForm, pshape)):
        refused(INVALID, "a sliding window needs causal", call, window=7, causal=False, **shape())
    # the inherited refusals, through the new entries
    W = dict(window=100)
    refused(UNSUPPORTED, "64 and 128, not 96", AttentionDecode(96, P.BF16).launchForm, **W, **dshape())
    refused(UNSUPPORTED, "at most 32", dec.launchForm, **W, **dshape(rows=8))
    refused(UNSUPPORTED, "FP32", AttentionDecode(128, P.FP32).launchForm, **W, **dshape())
    refused(INVALID, "cacheLengths is required", dec.launchForm, **W, **dshape(cacheLengths=None))
    refused(INVALID, "power of two from 16 to 1024", dec.launchForm, **W, **dshape(pageSize=48, blockTable=0x2000, blockTableStride=4096))
    refused(INVALID, "blockTableStride must hold the 512 pages", dec.launchForm, **W, **dshape(pageSize=64, blockTable=0x2000, blockTableStride=2))
    refused(INVALID, "multiples of 16 elements (16-byte rows of an e4m3 cache)", dec8.launchForm, **W, **dshape(strides=dict(K=(136, 32768 * 136, 8 * 32768 * 136))))
    refused(UNSUPPORTED, "e5m2", AttentionDecodeFP8(128, P.BF16, cachePrecision=KVCachePrecision.E5M2).launchForm, **W, **dshape())
    refused(INVALID, "workspace too small", dec.launchForm, window=4096, **dshape(workspace=0x100000, workspaceBytes=16))
    refused(UNSUPPORTED, "at most 32, not 64", pre.launchForm, **W, **pshape(headsPerKeyValue=64))
    refused(INVALID, "go with an e4m3 cache", pre.launchForm, **W, **pshape(keyScale=0x3000))
    refused(INVALID, "needs blockTable", pre.launchForm, **W, **pshape(pageSize=64))
    refused(INVALID, "non-zero", pre.launchForm, **W, **pshape(rows=0))
    for bufs, needle in (((0x10008, 0x20000, 0x30000, 0x40000, None), "16-byte aligned"), ((0, 0x20000, 0x30000, 0x40000, None), "null argument"),
                         ((0x10000, 0x20000, 0x30000, 0x40000, 0x50002), "L must be 4-byte aligned")):
        for obj, shape in ((dec, dshape), (pre, pshape)):   # pointers: checked before any GPU call (the process never opens the device)
            with pytest.raises(MFAError) as e:
                obj.dispatch(*bufs, **W, **shape())
            assert e.value.status == INVALID and needle in str(e.value), str(e.value)
    for bad in (dict(pieces=0, piece=0), dict(pieces=2, piece=2), dict(window=0), dict(rows=0)):
        kw = dict(length=100, rows=1, window=5, pieces=1, piece=0)
        kw.update(bad)
        with pytest.raises(MFAError):
            AttentionDecode.windowPieceRange(**kw)
    with pytest.raises(MFAError):
        AttentionPrefill.windowTileRange(64, 64, 0, 16, 0)
    with pytest.raises(MFAError):
        AttentionPrefill.windowTileRange(64, 64, 0, 0, 5)


def planned(column, rows, W, blocks):
    """the piece plan of include/mfa_window.h, on paper: (tiles planned from, pieces)"""
    tiles = min(-(-(W + rows - 1) // TILE) + 1, -(-column // TILE))
    if blocks >= _abi.MFA_DECODE_WORKGROUP_TARGET:
        return tiles, 1
    s = min(_abi.MFA_DECODE_WORKGROUP_TARGET // blocks, tiles // 4, _abi.MFA_DECODE_MAX_PIECES)
    return tiles, (1 if s < 2 else s)


@pytest.mark.parametrize("W", [1, 200, 1000, 4096, 40000])
def test_decode_launch_form_and_workspace_follow_the_window_plan(W):
    heads, G, B, rows, column = 16, 4, 2, 2, 32768
    blocks = B * heads // G
    tiles, pieces = planned(column, rows, W, blocks)
    for prec, tn in ((P.BF16, "bf16"), (P.FP16, "f16")):
        for D in (64, 128):
            for fp8 in (False, True):
                dec = (AttentionDecodeFP8 if fp8 else AttentionDecode)(D, prec)
                kw = dshape(rows=rows, column=column, heads=heads, batches=B, headsPerKeyValue=G)
                fam = "attn_decode8w" if fp8 else "attn_decode16w"
                need = dec.workspaceSize(window=W, **kw)
                assert need == (pieces * B * heads * rows * (D + 2) * 4 if pieces > 1 else 0)
                assert need <= dec.workspaceSize(**kw)
                tail = "contiguous, window %d: planned from %d tiles" % (W, tiles)
                text = dec.launchForm(window=W, **kw)
                if pieces > 1:
                    assert text == "%s_d%d_%s_single (grid %d sequences x K/V heads, %d packed rows, %s, unsplit without a workspace: the plan has %d pieces)" % (
                        fam, D, tn, blocks, G * rows, tail, pieces), text
                    text = dec.launchForm(window=W, workspace=0x100000, workspaceBytes=need, **kw)
                    assert text == "%s_d%d_%s_pieces (grid %d = %d sequences x K/V heads x %d pieces, %d packed rows, %s) + attn_decode16_d%d_%s_combine (grid %d)" % (
                        fam, D, tn, blocks * pieces, blocks, pieces, G * rows, tail, D, tn, (B * heads * rows + 3) // 4), text
                else:
                    assert text == "%s_d%d_%s_single (grid %d sequences x K/V heads, %d packed rows, %s)" % (fam, D, tn, blocks, G * rows, tail), text


def test_workspace_shrinks_with_the_window():
    dec = AttentionDecode(128, P.BF16)
    sizes = [dec.workspaceSize(window=W, **dshape()) for W in (64, 1024, 4096, 16384, 2 ** 31)]
    assert sizes == sorted(sizes) and sizes[0] == 0 and sizes[1] < sizes[2] < sizes[3]
    assert sizes[-1] == dec.workspaceSize(**dshape())   # a window past every key: column's own plan


def test_prefill_launch_form_names_the_window_kernels():
    heads, B, rows, G = 24, 2, 300, 8
    for prec, tn in ((P.BF16, "bf16"), (P.FP16, "f16")):
        for D in (64, 128):
            for fp8 in (False, True):
                pre = AttentionPrefill(D, prec, cachePrecision=KVCachePrecision.E4M3 if fp8 else None)
                for paged in (False, True):
                    kw = dict(pageSize=16, blockTable=0x2000, blockTableStride=256) if paged else {}
                    text = pre.launchForm(window=65, **pshape(rows=rows, heads=heads, batches=B, headsPerKeyValue=G, **kw))
                    assert text == "attn_prefill16w_d%d_%s%s (grid %d = %d sequences x %d K/V heads x %d row blocks of %d rows x %d heads, %s, window 65)" % (
                        D, tn, "_e4m3" if fp8 else "", B * (heads // G) * 19, B, heads // G, 19, 16, G, "paged" if paged else "contiguous"), text


def visible(n, qn, rows, W):
    """[rows, n] from the rule of include/mfa_window.h, written as the rule"""
    r, c = np.asarray(rows)[:, None], np.arange(n)[None, :]
    f = r + max(n - qn, 0)
    return (c < n) & (c <= f) & (c + W > f)


def test_window_piece_range_against_the_mask():
    for n in (0, 1, 63, 64, 65, 200, 1000):
        for R in (1, 4):
            for W in (1, 2, 63, 64, 65, 200, 5000):
                vis = visible(n, R, np.arange(R), W)
                tiles = -(-n // TILE)
                want = [t for t in range(tiles) if vis[:, t * TILE:(t + 1) * TILE].any()]
                for pieces in (1, 2, 3, 7, 64):
                    ranges = [AttentionDecode.windowPieceRange(n, R, W, pieces, p) for p in range(pieces)]
                    case = (n, R, W, pieces, ranges)
                    covered = []
                    at = ranges[0][0]
                    for b, e in ranges:
                        assert b == at or b == e, case          # disjoint, ordered, gap-free (an empty piece sits anywhere at or below the end)
                        assert b <= e <= n and b % TILE == 0 and (e % TILE == 0 or e == n), case
                        covered += list(range(b // TILE, -(-e // TILE)))
                        at = max(at, e)
                    assert covered == want, case                 # exactly the tiles that hold a key some row sees
    assert AttentionDecode.windowPieceRange(2 ** 32 - 1, 1, 2 ** 32 - 1, 64, 63)[1] == 2 ** 32 - 1


def test_window_tile_range_against_the_mask():
    for W in (1, 16, 64, 65, 129, 5000):
        for n in (0, 1, 63, 64, 65, 127, 128, 129, 1000):
            for qn in (1, 16, 42, 128, 200):               # (n < qn is in the grid: 1 .. 129 against 200)
                for RB in (128, 16, 42):
                    for r0 in range(0, qn + RB, RB):       # (one block past the last live row too)
                        b, u0, u1, e = AttentionPrefill.windowTileRange(n, qn, r0, RB, W)
                        case = (W, n, qn, r0, RB, (b, u0, u1, e))
                        vis = visible(n, qn, np.arange(r0, min(r0 + RB, qn)), W)
                        tiles = -(-n // TILE)
                        seen = [t for t in range(tiles) if vis.size and vis[:, t * TILE:(t + 1) * TILE].any()]
                        full = [t for t in range(tiles) if vis.size and (t + 1) * TILE <= n and vis[:, t * TILE:(t + 1) * TILE].all()]
                        if seen:
                            assert (b, e) == (seen[0], seen[-1] + 1), case     # the tightest bounds
                        else:
                            assert b == e, case
                        assert b <= u0 <= u1 <= e, case
                        assert list(range(u0, u1)) == full, case               # exactly the fully visible tiles


def test_fake_tensor_path_gives_shapes_without_a_device():
    torch = pytest.importorskip("torch")
    from torch._subclasses.fake_tensor import FakeTensorMode
    from metal_flash_attention_amd import torch_binding as tb
    if not tb._HAVE_WINDOW_OPS:
        pytest.skip("this torch has no torch.library.custom_op")
    with FakeTensorMode():
        q = torch.empty((2, 8, 300, 128), dtype=torch.bfloat16, device="cuda")
        k8 = torch.empty((2, 2, 1024, 128), dtype=torch.float8_e4m3fn, device="cuda")
        k16 = torch.empty((2, 2, 1024, 128), dtype=torch.bfloat16, device="cuda")
        lens = torch.empty((2,), dtype=torch.int32, device="cuda")
        scale = torch.empty((2,), dtype=torch.float32, device="cuda")
        o, l = torch.ops.mfa.attention_prefill_window(q, k8, k8, lens, lens, None, True, scale, scale, 100)
        assert o.shape == (2, 8, 300, 128) and o.dtype == torch.bfloat16 and l.shape == (2, 8, 300) and l.dtype == torch.float32
        o, l = torch.ops.mfa.attention_decode_window(q[:, :, :2], k16, k16, lens, None, True, None, None, 100)
        assert o.shape == (2, 8, 2, 128) and l.shape == (2, 8, 2)
        assert tb.flash_prefill(q, k16, k16, lens, window=65).shape == (2, 8, 300, 128)
        o, lse = tb.flash_decode(q[:, :, :1].half(), k8, k8, lens, k_scale=scale, window=7, return_lse=True)
        assert o.dtype == torch.float16 and o.shape == (2, 8, 1, 128) and lse.shape == (2, 8, 1)
    for bad in (0, -1, True, 2 ** 32, 1.5):
        with pytest.raises(ValueError, match="window must be an int"):
            tb._check_window("flash_decode", bad, True)
    with pytest.raises(ValueError, match="needs causal"):
        tb._check_window("flash_decode", 5, False)
