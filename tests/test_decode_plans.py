"""CPU test (no GPU call): the host side of decode attention, include/mfa_decode.h -- exported symbols, the parameter block's layout,
every refusal with its message, the plan (pieces, workspace bytes, launch-form text) and the piece -> key-range function, which is the
very function the kernels run (decode_piece_range, csrc/attn_decode16.h)."""
import ctypes
import os
import re

import numpy as np
import pytest

from metal_flash_attention_amd import AttentionDecode, GEMMOperandPrecision as P, MFAError, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = 0x1000   # any non-null value: the host never reads the lengths
TILE = _abi.MFA_DECODE_KEY_TILE
TARGET = _abi.MFA_DECODE_WORKGROUP_TARGET


def shape(**over):
    kw = dict(rows=1, column=4096, heads=64, batches=4, headsPerKeyValue=8, cacheLengths=LENGTHS)
    kw.update(over)
    return kw


def refused(status, needle, decode=None, **over):
    with pytest.raises(MFAError) as e:
        (decode or AttentionDecode(128, P.BF16)).launchForm(**shape(**over))
    assert e.value.status == status, str(e.value)
    assert needle in str(e.value), str(e.value)


def test_header_symbols_exported_and_struct_size():
    header = open(os.path.join(ROOT, "include", "mfa_decode.h")).read()
    declared = set(re.findall(r"\b(mfa_(?:decode|attention_decode)_\w+)\s*\(", header))
    handle = _abi.lib()
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in include/mfa_decode.h but not exported"
    assert declared == {s[0] for s in _abi.DECODE_SYMBOLS}
    assert len(declared) == 6
    # 6 x u32, u16 + 2 x u8, u32, 2 pointers, i64, 12 + 2 + 2 x i64, pointer, u64
    assert ctypes.sizeof(_abi.mfa_decode_params) == 200
    assert _abi.mfa_decode_params.cacheLengths.offset == 32 and _abi.mfa_decode_params.workspace.offset == 184
    for macro, value in (("MFA_DECODE_KEY_TILE", TILE), ("MFA_DECODE_WORKGROUP_TARGET", TARGET),
                         ("MFA_DECODE_MAX_PACKED_ROWS", _abi.MFA_DECODE_MAX_PACKED_ROWS), ("MFA_DECODE_MAX_PIECES", _abi.MFA_DECODE_MAX_PIECES)):
        assert re.search(r"#define %s\s+%d\b" % (macro, value), header), macro
    assert int(handle.mfa_abi_version()) == 6   # mfa.h did not change
    p = _abi.mfa_decode_params()
    handle.mfa_decode_params_init(ctypes.byref(p))
    assert (p.precision, p.outputPrecision, p.headsPerKeyValue, p.causal, p.pageSize) == (int(P.BF16), int(P.BF16), 1, 1, 0)


def test_refusals_name_the_requirement():
    UNSUPPORTED, INVALID = 3, 2
    refused(UNSUPPORTED, "16-bit", decode=AttentionDecode(128, P.FP32))
    refused(UNSUPPORTED, "64 and 128", decode=AttentionDecode(96, P.BF16))
    refused(UNSUPPORTED, "mfa_attention_kernel_launch", rows=5)                       # M = 8 x 5 = 40
    refused(UNSUPPORTED, "= 40 rows", rows=5)
    refused(INVALID, "multiple of headsPerKeyValue", heads=60)
    refused(INVALID, "power of two from 16 to 1024", pageSize=24, blockTable=0x2000, blockTableStride=1024)
    refused(INVALID, "power of two", pageSize=2048, blockTable=0x2000, blockTableStride=1024)
    refused(INVALID, "needs blockTable", pageSize=64)
    refused(INVALID, "blockTableStride", pageSize=64, blockTable=0x2000, blockTableStride=63)   # 4096 keys = 64 pages
    refused(INVALID, "cacheLengths is required", cacheLengths=None)
    refused(INVALID, "strides of K must be multiples of 8", strides=dict(K=(132, 132 * 4096, 8 * 132 * 4096)))
    refused(INVALID, "strides of O must be multiples of 4", strides=dict(O=(130, 130, 64 * 130)))
    refused(INVALID, "smaller than the head dimension", strides=dict(V=(64, 64 * 4096, 8 * 64 * 4096)))
    need = AttentionDecode(128).workspaceSize(**shape())
    assert need > 0
    refused(INVALID, "needs %d" % need, workspace=0x4000, workspaceBytes=need - 4)
    refused(INVALID, "16-byte aligned", workspace=0x4004, workspaceBytes=need)
    refused(INVALID, "outputPrecision", decode=AttentionDecode(128, P.BF16, P.FP16))
    # the launch itself: null and misaligned buffers are refused before any GPU call
    d = AttentionDecode(128)
    for bufs, needle in (((0, 0x100, 0x100, 0x100), "null argument"), ((0x100, 0x108, 0x100, 0x100), "16-byte aligned")):
        with pytest.raises(MFAError) as e:
            d.dispatch(*bufs, **shape())
        assert e.value.status == INVALID and needle in str(e.value)


@pytest.mark.parametrize("D,prec", [(64, P.BF16), (128, P.FP16)])
def test_plan_workspace_and_launch_form(D, prec):
    d = AttentionDecode(D, prec)
    tname = "bf16" if prec == P.BF16 else "f16"
    # one sequence, 8 K / V heads, 32768 keys: 512 / 8 = 64 pieces
    kw = shape(batches=1, column=32768)
    need = d.workspaceSize(**kw)
    assert need == 64 * 1 * 64 * 1 * (D + 2) * 4
    text = d.launchForm(workspace=0x4000, workspaceBytes=need, **kw)
    assert f"attn_decode16_d{D}_{tname}_pieces" in text and "64 pieces" in text and f"attn_decode16_d{D}_{tname}_combine" in text, text
    text = d.launchForm(**kw)   # no workspace: one kernel, unsplit
    assert f"attn_decode16_d{D}_{tname}_single" in text and "_pieces" not in text and "combine" not in text, text
    # R = 4: the formula counts the rows
    assert d.workspaceSize(**shape(batches=1, column=32768, rows=4)) == 64 * 64 * 4 * (D + 2) * 4
    # batches x K/V heads at the chip's workgroup target: no split
    full = shape(batches=TARGET // 8, column=32768)
    assert d.workspaceSize(**full) == 0
    assert "_single" in d.launchForm(workspace=0x4000, workspaceBytes=1 << 20, **full)
    # just below it there is nothing to gain either (one piece per workgroup)
    assert d.workspaceSize(**shape(batches=TARGET // 8 - 1, column=32768)) == 0
    # half the target: two pieces; a short cache keeps at least four tiles per piece
    assert d.workspaceSize(**shape(batches=TARGET // 16, column=32768)) == 2 * (TARGET // 16) * 64 * (D + 2) * 4
    assert d.workspaceSize(**shape(batches=1, column=8 * TILE)) == 2 * 64 * (D + 2) * 4
    assert d.workspaceSize(**shape(batches=1, column=7 * TILE)) == 0
    # paged launches plan the same pieces and say so
    paged = d.launchForm(workspace=0x4000, workspaceBytes=need, pageSize=16, blockTable=0x2000, blockTableStride=2048,
                         pageStrides=(8 * 16 * D, 8 * 16 * D), strides=dict(K=(D, 16 * D, 0), V=(D, 16 * D, 0)), **kw)
    assert "64 pieces" in paged and "paged" in paged, paged


def check_ranges(length, pieces):
    prev = 0
    for i in range(pieces):
        b, e = AttentionDecode.pieceRange(length, pieces, i)
        assert b == prev, (length, pieces, i, b, prev)          # in order, disjoint, no gap
        assert b <= e <= length
        assert b % TILE == 0                                     # whole tiles ...
        assert e % TILE == 0 or e == length                      # ... except the sequence's last
        prev = e
    assert prev == length                                        # the union is [0, length)


def test_piece_ranges_tile_the_sequence():
    rng = np.random.default_rng(2024)
    column = 32768
    edge = [0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, column - 1, column, 2 ** 32 - 1]
    for length in edge:
        for pieces in (1, 2, 3, 7, 16, 63, 64):
            check_ranges(length, pieces)
    for _ in range(3000):
        check_ranges(int(rng.integers(0, column + 1)), int(rng.integers(1, 65)))
    # equal shares: pieces differ by at most one tile
    for length, pieces in ((32768, 64), (10000, 7), (4097, 16)):
        sizes = [(lambda be: (be[1] - be[0] + TILE - 1) // TILE)(AttentionDecode.pieceRange(length, pieces, i)) for i in range(pieces)]
        assert max(sizes) - min(sizes) <= 1, sizes
    with pytest.raises(MFAError):
        AttentionDecode.pieceRange(100, 4, 4)
    with pytest.raises(MFAError):
        AttentionDecode.pieceRange(100, 0, 0)
