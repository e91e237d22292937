"""CPU test (no GPU call): the host side of attention sinks over a KV cache, include/mfa_sink.h -- exported symbols and the struct
mirror, a block without sinks as the window launch, every refusal with its message, the launch-form texts and the piece plan, and the
two range functions (the very functions the kernels run: decode_sink_piece_range, csrc/attn_decode16.h, and prefill_sink_tile_range,
csrc/attn_prefill16.h) against brute-force scans of the mask; the fake-tensor path of the two torch ops."""
import ctypes
import os
import re

import numpy as np
import pytest

from metal_flash_attention_amd import AttentionDecode, AttentionDecodeFP8, AttentionPrefill, GEMMOperandPrecision as P, KVCachePrecision, MFAError, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS, LOGITS = 0x1000, 0x3000   # any non-null values: the host never reads the lengths or the logits
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


def refused(status, needle, call, *args, **kw):
    with pytest.raises(MFAError) as e:
        call(*args, **kw)
    assert e.value.status == status, str(e.value)
    assert needle in str(e.value), str(e.value)


def test_header_symbols_exported_and_the_struct_mirror():
    header = open(os.path.join(ROOT, "include", "mfa_sink.h")).read()
    assert '#include "mfa_window.h"' in header
    declared = set(re.findall(r"\b(mfa_attention_(?:decode_sink|prefill_sink|sinks)_\w+)\s*\(", header))
    handle = _abi.lib()
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in include/mfa_sink.h but not exported"
    assert declared == {s[0] for s in _abi.SINK_SYMBOLS}
    assert len(declared) == 12
    assert int(handle.mfa_abi_version()) == 6   # mfa.h did not change
    assert ctypes.sizeof(_abi.mfa_attention_sinks) == int(handle.mfa_attention_sinks_size()) == 16
    offsets, count = (ctypes.c_uint32 * 8)(), ctypes.c_uint32(0)
    assert handle.mfa_attention_sinks_offsets(offsets, 8, ctypes.byref(count)) == 0
    mirror = [getattr(_abi.mfa_attention_sinks, name).offset for name, _ in _abi.mfa_attention_sinks._fields_]
    assert list(offsets[:count.value]) == mirror == [0, 4, 8]
    block = _abi.mfa_attention_sinks(7, 7, 7)
    handle.mfa_attention_sinks_init(ctypes.byref(block))
    assert (block.sinkTokens, block.reserved, block.sinkLogits) == (0, 0, None)


def test_a_block_without_sinks_is_the_window_launch():
    for D, prec in ((64, P.FP16), (128, P.BF16)):
        for cls in (AttentionDecode, AttentionDecodeFP8):
            dec = cls(D, prec)
            for kw in (dshape(), dshape(workspace=0x100000, workspaceBytes=1 << 30), dshape(rows=4, column=300, pageSize=16, blockTable=0x2000, blockTableStride=32)):
                for W in (0, 7, 4096):
                    assert dec.launchForm(window=W, sinkTokens=0, **kw) == dec.launchForm(window=W, **kw)
                    assert dec.workspaceSize(window=W, sinkTokens=0, sinkLogits=None, **kw) == dec.workspaceSize(window=W, **kw)
                assert dec.launchForm(sinkTokens=0, **kw) == dec.launchForm(**kw)      # no window keyword: window 0
        for cache in (None, KVCachePrecision.E4M3):
            pre = AttentionPrefill(D, prec, cachePrecision=cache)
            for W in (0, 65):
                assert pre.launchForm(window=W, sinkTokens=0, **pshape()) == pre.launchForm(window=W, **pshape())
    # anything else runs the sink kernels: logits alone, without a window and without causal
    assert AttentionDecode(128, P.BF16).launchForm(sinkLogits=LOGITS, **dshape()).startswith("attn_decode16s_d128_bf16_single ")
    assert AttentionDecodeFP8(64, P.FP16).launchForm(sinkLogits=LOGITS, causal=False, **dshape()).startswith("attn_decode8s_d64_f16_single ")
    assert AttentionPrefill(128, P.BF16).launchForm(sinkLogits=LOGITS, causal=False, **pshape()).startswith("attn_prefill16s_d128_bf16 ")
    assert AttentionPrefill(64, P.FP16, cachePrecision=KVCachePrecision.E4M3).launchForm(window=9, sinkTokens=1, **pshape()).startswith("attn_prefill16s_d64_f16_e4m3 ")


def test_refusals_name_the_requirement():
    dec, dec8, pre = AttentionDecode(128, P.BF16), AttentionDecodeFP8(128, P.BF16), AttentionPrefill(128, P.BF16)
    for call, shape in ((dec.launchForm, dshape), (dec.workspaceSize, dshape), (dec8.launchForm, dshape), (pre.launchForm, pshape)):
        refused(INVALID, "sink tokens need a window", call, sinkTokens=4, **shape())
        refused(INVALID, "sink tokens need a window", call, window=0, sinkTokens=4, sinkLogits=LOGITS, **shape())
        refused(INVALID, "sink tokens need causal", call, window=7, sinkTokens=4, causal=False, **shape())
        refused(INVALID, "a sliding window needs causal", call, window=7, sinkLogits=LOGITS, causal=False, **shape())
    # the range functions refuse the same combinations
    refused(INVALID, "a sliding window needs causal", AttentionPrefill.sinkTileRange, 100, 100, 0, 16, 5, 4, causal=False)
    refused(INVALID, "sink tokens need a window", AttentionPrefill.sinkTileRange, 100, 100, 0, 16, 0, 4)
    refused(INVALID, "sink tokens need a window", AttentionDecode.sinkPieceRange, 100, 1, 0, 4, 1, 0)
    refused(INVALID, "blockRows must be non-zero", AttentionPrefill.sinkTileRange, 100, 100, 0, 0, 5, 4)
    for bad in (dict(pieces=0, piece=0), dict(pieces=2, piece=2), dict(rows=0)):
        kw = dict(length=100, rows=1, window=5, sinkTokens=2, pieces=1, piece=0)
        kw.update(bad)
        with pytest.raises(MFAError):
            AttentionDecode.sinkPieceRange(**kw)
    # a NULL block, straight through the C entries
    handle = _abi.lib()
    p, _keep = dec._params(**dshape())
    pp, _keep = pre._params(**pshape())
    out, size = ctypes.create_string_buffer(512), ctypes.c_uint64(0)
    for status in (handle.mfa_attention_decode_sink_launch_form(ctypes.byref(p), None, 5, None, out, len(out)),
                   handle.mfa_attention_decode_sink_workspace_size(ctypes.byref(p), None, 5, None, ctypes.byref(size)),
                   handle.mfa_attention_decode_sink_launch(0x10000, 0x20000, 0x30000, 0x40000, None, ctypes.byref(p), None, 5, None, None),
                   handle.mfa_attention_prefill_sink_launch_form(ctypes.byref(pp), 5, None, out, len(out)),
                   handle.mfa_attention_prefill_sink_launch(0x10000, 0x20000, 0x30000, 0x40000, None, ctypes.byref(pp), 5, None, None)):
        assert status == INVALID and "null mfa_attention_sinks" in handle.mfa_last_error_string().decode()
    # the inherited refusals, through the new entries
    S = dict(window=100, sinkTokens=4, sinkLogits=LOGITS)
    refused(UNSUPPORTED, "64 and 128, not 96", AttentionDecode(96, P.BF16).launchForm, **S, **dshape())
    refused(UNSUPPORTED, "at most 32", dec.launchForm, **S, **dshape(rows=8))
    refused(INVALID, "cacheLengths is required", dec.launchForm, **S, **dshape(cacheLengths=None))
    refused(INVALID, "workspace too small", dec.launchForm, window=4096, sinkTokens=4, **dshape(workspace=0x100000, workspaceBytes=16))
    refused(UNSUPPORTED, "at most 32, not 64", pre.launchForm, **S, **pshape(headsPerKeyValue=64))
    refused(INVALID, "needs blockTable", pre.launchForm, **S, **pshape(pageSize=64))
    for obj, shape in ((dec, dshape), (pre, pshape)):   # pointers: checked before any GPU call (the process never opens the device)
        with pytest.raises(MFAError) as e:
            obj.dispatch(0x10000, 0x20000, 0x30000, 0x40000, None, window=100, sinkLogits=0x50002, **shape())
        assert e.value.status == INVALID and "sinkLogits must be 4-byte aligned" in str(e.value), str(e.value)


def planned(column, rows, W, S, blocks):
    """the piece plan of include/mfa_sink.h, on paper: (tiles planned from, pieces)"""
    tiles = -(-column // TILE)
    if W:
        tiles = min(-(-(W + rows - 1) // TILE) + 1 + -(-S // TILE), tiles)
    if blocks >= _abi.MFA_DECODE_WORKGROUP_TARGET:
        return tiles, 1
    s = min(_abi.MFA_DECODE_WORKGROUP_TARGET // blocks, tiles // 4, _abi.MFA_DECODE_MAX_PIECES)
    return tiles, (1 if s < 2 else s)


@pytest.mark.parametrize("W,S,logits", [(200, 4, False), (1000, 70, True), (4096, 4, True), (40000, 1, False), (0, 0, True), (700, 0, True)])
def test_decode_launch_form_and_workspace_follow_the_planned_tiles(W, S, logits):
    heads, G, B, rows, column = 16, 4, 2, 2, 32768
    blocks = B * heads // G
    tiles, pieces = planned(column, rows, W, S, blocks)
    sinks = dict(sinkTokens=S, sinkLogits=LOGITS if logits else None)
    for prec, tn in ((P.BF16, "bf16"), (P.FP16, "f16")):
        for D in (64, 128):
            for fp8 in (False, True):
                dec = (AttentionDecodeFP8 if fp8 else AttentionDecode)(D, prec)
                kw = dshape(rows=rows, column=column, heads=heads, batches=B, headsPerKeyValue=G)
                fam = "attn_decode8s" if fp8 else "attn_decode16s"
                need = dec.workspaceSize(window=W, **sinks, **kw)
                assert need == (pieces * B * heads * rows * (D + 2) * 4 if pieces > 1 else 0)
                assert need >= dec.workspaceSize(window=W, **kw)     # the sink tiles only ever add to the window's plan
                tail = "contiguous" + (", window %d%s: planned from %d tiles" % (W, ", sink tokens %d" % S if S else "", tiles) if W else "") + \
                    (", sink logits" if logits else "")
                text = dec.launchForm(window=W, **sinks, **kw)
                if pieces > 1:
                    assert text == "%s_d%d_%s_single (grid %d sequences x K/V heads, %d packed rows, %s, unsplit without a workspace: the plan has %d pieces)" % (
                        fam, D, tn, blocks, G * rows, tail, pieces), text
                    text = dec.launchForm(window=W, workspace=0x100000, workspaceBytes=need, **sinks, **kw)
                    assert text == "%s_d%d_%s_pieces (grid %d = %d sequences x K/V heads x %d pieces, %d packed rows, %s) + attn_decode16_d%d_%s_combine (grid %d)" % (
                        fam, D, tn, blocks * pieces, blocks, pieces, G * rows, tail, D, tn, (B * heads * rows + 3) // 4), text
                else:
                    assert text == "%s_d%d_%s_single (grid %d sequences x K/V heads, %d packed rows, %s)" % (fam, D, tn, blocks, G * rows, tail), text


def test_prefill_launch_form_names_the_sinks():
    heads, B, rows, G = 24, 2, 300, 8
    for prec, tn in ((P.BF16, "bf16"), (P.FP16, "f16")):
        for D in (64, 128):
            for fp8 in (False, True):
                pre = AttentionPrefill(D, prec, cachePrecision=KVCachePrecision.E4M3 if fp8 else None)
                for W, S, logits, tail in ((65, 4, True, ", window 65, sink tokens 4, sink logits"), (65, 70, False, ", window 65, sink tokens 70"),
                                           (0, 0, True, ", sink logits"), (9, 0, True, ", window 9, sink logits")):
                    text = pre.launchForm(window=W, sinkTokens=S, sinkLogits=LOGITS if logits else None,
                                          **pshape(rows=rows, heads=heads, batches=B, headsPerKeyValue=G))
                    assert text == "attn_prefill16s_d%d_%s%s (grid %d = %d sequences x %d K/V heads x %d row blocks of %d rows x %d heads, contiguous%s)" % (
                        D, tn, "_e4m3" if fp8 else "", B * (heads // G) * 19, B, heads // G, 19, 16, G, tail), text


def visible(n, qn, rows, W, S):
    """[rows, n] from the rule of include/mfa_sink.h, written as the rule"""
    r, c = np.asarray(rows)[:, None], np.arange(n)[None, :]
    f = r + max(n - qn, 0)
    lim = np.minimum(n, f + 1)
    lo = np.maximum(f + 1, W) - W if W else np.zeros_like(f)
    return (c < lim) & ((c >= lo) | (c < S))


def test_sink_piece_range_against_the_tile_list():
    for n in (0, 1, 63, 64, 65, 200, 700, 1000):
        for R in (1, 4):
            for W in (1, 2, 64, 65, 130, 200, 5000):
                for S in (0, 1, 4, 64, 65, 70, 200, 5000):
                    vis = visible(n, R, np.arange(R), W, S)
                    first = (max(max(n - R, 0) + 1, W) - W) // TILE
                    sink_tiles = min(-(-min(S, n) // TILE), first)
                    walked = list(range(sink_tiles)) + list(range(first, -(-n // TILE)))
                    # the list holds every tile with a visible key; its window part holds nothing else, its sink part whole sink tiles
                    assert all(t in walked for t in range(-(-n // TILE)) if vis[:, t * TILE:(t + 1) * TILE].any()), (n, R, W, S)
                    for pieces in (1, 2, 3, 7, 64):
                        pairs = [AttentionDecode.sinkPieceRange(n, R, W, S, pieces, p) for p in range(pieces)]
                        case = (n, R, W, S, pieces, pairs)
                        covered, at = [], [0, first * TILE]
                        for pair in pairs:
                            for i, (b, e) in enumerate(pair):
                                assert b <= e <= n and b % TILE == 0 and (e % TILE == 0 or e == n), case
                                if e > b:
                                    assert b == at[i] or not covered, case     # disjoint, ordered, gap-free inside each part of the list
                                    at[i] = e
                            assert pair[0][1] <= sink_tiles * TILE and (pair[1][0] >= first * TILE or pair[1][0] == pair[1][1]), case
                            covered += [t for b, e in pair for t in range(b // TILE, -(-e // TILE))]
                        assert covered == walked, case                        # the union is exactly the walked list, in its order
                        sizes = [len([t for b, e in pair for t in range(b // TILE, -(-e // TILE))]) for pair in pairs]
                        assert max(sizes) - min(sizes) <= 1, case              # equal shares of the LIST
                        if S == 0:
                            assert [pair[1] for pair in pairs] == [AttentionDecode.windowPieceRange(n, R, W, pieces, p) for p in range(pieces)], case
                            assert all(pair[0] == (0, 0) for pair in pairs), case
    # window 0: the plain pieces
    assert [AttentionDecode.sinkPieceRange(1000, 2, 0, 0, 3, p)[1] for p in range(3)] == [AttentionDecode.pieceRange(1000, 3, p) for p in range(3)]
    assert AttentionDecode.sinkPieceRange(2 ** 32 - 1, 1, 2 ** 32 - 1, 2 ** 32 - 1, 64, 63)[1][1] == 2 ** 32 - 1


def test_the_three_decode_piece_ranges_nest():
    """the plain range is the window range of a window nothing falls out of; the window range is the sink range without sink tokens"""
    for n in (0, 1, 63, 64, 65, 1000):
        for pieces in (1, 3, 7):
            for R in (1, 2, 32):
                plain = [AttentionDecode.pieceRange(n, pieces, p) for p in range(pieces)]
                for W in (n + R, n + R + 1, 2 ** 32 - 1):
                    assert [AttentionDecode.windowPieceRange(n, R, W, pieces, p) for p in range(pieces)] == plain, (n, pieces, R, W)
                for W in (1, 64, 100, n + R):
                    windowed = [AttentionDecode.windowPieceRange(n, R, W, pieces, p) for p in range(pieces)]
                    sunk = [AttentionDecode.sinkPieceRange(n, R, W, 0, pieces, p) for p in range(pieces)]
                    assert [pair[0][0] == pair[0][1] for pair in sunk] == [True] * pieces, (n, pieces, R, W, sunk)
                    assert [pair[1] for pair in sunk] == windowed, (n, pieces, R, W)


def test_sink_tile_range_against_the_mask():
    for W in (1, 16, 64, 65, 129, 5000):
        for S in (0, 1, 4, 64, 70, 200):
            for n in (0, 1, 63, 64, 65, 127, 128, 129, 700, 1000):
                for qn in (1, 16, 42, 128, 200):               # (n < qn is in the grid)
                    for RB in (128, 16, 42):
                        for r0 in range(0, qn + RB, RB):       # (one block past the last live row too)
                            b, u0, u1, e, se = AttentionPrefill.sinkTileRange(n, qn, r0, RB, W, S)
                            case = (W, S, n, qn, r0, RB, (b, u0, u1, e, se))
                            vis = visible(n, qn, np.arange(r0, min(r0 + RB, qn)), W, S)
                            tiles = -(-n // TILE)
                            seen = [t for t in range(tiles) if vis.size and vis[:, t * TILE:(t + 1) * TILE].any()]
                            assert se <= b <= u0 <= u1 <= e, case
                            walked = list(range(se)) + list(range(b, e))
                            assert all(t in walked for t in seen), case                 # no tile outside holds a visible key
                            if not seen:
                                assert (b, u0, u1, e, se) == (0, 0, 0, 0, 0), case
                            else:
                                assert walked[-1] == seen[-1], case
                                assert all(t in seen for t in range(se)), case          # every sink tile walked holds a visible key
                            for t in range(u0, u1):
                                assert (t + 1) * TILE <= n and vis[:, t * TILE:(t + 1) * TILE].all(), case   # unmasked tiles: fully visible
                            if S == 0:
                                assert (b, u0, u1, e) == AttentionPrefill.windowTileRange(n, qn, r0, RB, W) and se == 0, case
    # window 0: the plain launch's two indices, causal or not
    for causal in (True, False):
        assert AttentionPrefill.sinkTileRange(1000, 200, 128, 128, 0, 0, causal=causal) == (0, 0) + AttentionPrefill.tileRange(1000, 200, 128, 128, causal) + (0,)


def test_fake_tensor_path_and_argument_checks_without_a_device():
    torch = pytest.importorskip("torch")
    from torch._subclasses.fake_tensor import FakeTensorMode
    from metal_flash_attention_amd import torch_binding as tb
    if not tb._HAVE_SINK_OPS:
        pytest.skip("this torch has no torch.library.custom_op")
    with FakeTensorMode():
        q = torch.empty((2, 8, 300, 128), dtype=torch.bfloat16, device="cuda")
        k8 = torch.empty((2, 2, 1024, 128), dtype=torch.float8_e4m3fn, device="cuda")
        k16 = torch.empty((2, 2, 1024, 128), dtype=torch.bfloat16, device="cuda")
        lens = torch.empty((2,), dtype=torch.int32, device="cuda")
        scale = torch.empty((2,), dtype=torch.float32, device="cuda")
        logits = torch.empty((8,), dtype=torch.float32, device="cuda")
        o, l = torch.ops.mfa.attention_prefill_sink(q, k8, k8, lens, lens, None, True, scale, scale, 100, 4, logits)
        assert o.shape == (2, 8, 300, 128) and o.dtype == torch.bfloat16 and l.shape == (2, 8, 300) and l.dtype == torch.float32
        o, l = torch.ops.mfa.attention_decode_sink(q[:, :, :2], k16, k16, lens, None, True, None, None, 0, 0, logits)
        assert o.shape == (2, 8, 2, 128) and l.shape == (2, 8, 2)
        assert tb.flash_prefill(q, k16, k16, lens, window=65, sink_tokens=4).shape == (2, 8, 300, 128)
        o, lse = tb.flash_decode(q[:, :, :1].half(), k8, k8, lens, k_scale=scale, sink_logits=logits, return_lse=True)
        assert o.dtype == torch.float16 and o.shape == (2, 8, 1, 128) and lse.shape == (2, 8, 1)
        for bad in (0, -1, True, 2 ** 32, 1.5):
            with pytest.raises(ValueError, match="sink_tokens must be an int"):
                tb.flash_decode(q[:, :, :1], k16, k16, lens, window=5, sink_tokens=bad)
        with pytest.raises(ValueError, match="sink_tokens needs window"):
            tb.flash_prefill(q, k16, k16, lens, sink_tokens=4)
        with pytest.raises(ValueError, match="needs causal"):
            tb.flash_decode(q[:, :, :1], k16, k16, lens, window=5, sink_tokens=4, causal=False)
        for bad in (logits.half(), logits[:4], torch.empty((8, 2), dtype=torch.float32, device="cuda")[:, 0], torch.empty((1, 8), dtype=torch.float32, device="cuda")):
            with pytest.raises(ValueError, match="sink_logits must be a contiguous float32"):
                tb.flash_decode(q[:, :, :1], k16, k16, lens, sink_logits=bad)
        with pytest.raises(RuntimeError, match="sink_logits must live on q's device"):
            tb.flash_prefill(q, k16, k16, lens, sink_logits=torch.empty((8,), dtype=torch.float32, device="cpu"))
