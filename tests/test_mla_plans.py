"""CPU test (no GPU call, through the built library): the host side of multi-head latent attention decode, include/mfa_mla.h -- every
declared name exported, the ctypes mirror against sizeof and every offset, the workspace formula at a hand-computed shape, the plan's
piece counts (decode's own choose_pieces and constants over batches x groups), the launch form's kernel names and grid, and every
refusal by status and words, before any GPU call: the pointers are made up."""
import ctypes
import os
import re

import pytest

import metal_flash_attention_amd as mfa
from metal_flash_attention_amd import AttentionMLADecode, GEMMOperandPrecision as P, MFAError, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS, TABLE, Q, KV, O, L, WS = 0x1000, 0x5000, 0x10000, 0x20000, 0x30000, 0x40000, 0x100000   # the host never reads what they point to
INVALID, UNSUPPORTED = 2, 3
SCALE = 0.1352


def test_header_symbols_exported_and_the_ctypes_mirror():
    header = open(os.path.join(ROOT, "include", "mfa_mla.h")).read()
    assert '#include "mfa_decode.h"' in header
    declared = set(re.findall(r"\b(mfa_\w+)\s*\(", header.split("#ifndef MFA_MLA_H")[1]))
    handle = _abi.lib()
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in include/mfa_mla.h but not exported"
    assert declared == {s[0] for s in _abi.MLA_SYMBOLS}
    assert declared == {"mfa_mla_decode_params_" + s for s in ("init", "size", "offsets")} | {
        "mfa_attention_mla_decode_" + s for s in ("workspace_size", "launch", "launch_form", "time")}
    for name, restype, argtypes in _abi.MLA_SYMBOLS:
        fn = getattr(handle, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert int(handle.mfa_abi_version()) == 6 == _abi.EXPECTED_ABI   # mfa.h did not change
    assert mfa.AttentionMLADecode is AttentionMLADecode and "AttentionMLADecode" in dir(mfa)
    assert "mla" not in " ".join(_abi.CACHE_FAMILIES["decode"]) and "mla" not in " ".join(_abi.CACHE_FAMILIES["prefill"])   # an entry of its own


def test_the_struct_mirror_matches():
    handle = _abi.lib()
    mirror = _abi.mfa_mla_decode_params
    assert handle.mfa_mla_decode_params_size() == ctypes.sizeof(mirror) == 176
    offsets, count = (ctypes.c_uint32 * 32)(), ctypes.c_uint32(0)
    assert handle.mfa_mla_decode_params_offsets(offsets, 32, ctypes.byref(count)) == 0
    want = [getattr(mirror, name).offset for name, _t in mirror._fields_]
    assert count.value == len(want) == 24 and list(offsets[:24]) == want
    assert [name for name, _t in mirror._fields_] == [
        "rows", "column", "heads", "batches", "causal", "headDimension", "valueDimension", "precision", "outputPrecision", "reserved", "scale",
        "pageSize", "pieces", "cacheLengths", "blockTable", "blockTableStride", "leadingDimension", "headStride", "batchStride", "pageStride",
        "lHeadStride", "lBatchStride", "workspace", "workspaceBytes"]
    few, count = (ctypes.c_uint32 * 2)(7, 7), ctypes.c_uint32(0)                    # a small capacity: the count is still said
    assert handle.mfa_mla_decode_params_offsets(few, 2, ctypes.byref(count)) == 0 and count.value == 24 and list(few) == want[:2]
    assert handle.mfa_mla_decode_params_offsets(None, 2, ctypes.byref(count)) == INVALID
    block = mirror(rows=5, causal=0, scale=3.0, pieces=9, workspace=8)
    handle.mfa_mla_decode_params_init(ctypes.byref(block))
    assert (block.rows, block.causal, block.scale, block.pieces, block.workspace) == (0, 1, 0.0, 0, None)          # no default scale
    assert (block.headDimension, block.valueDimension, block.precision, block.outputPrecision) == (576, 512, int(P.BF16), int(P.BF16))


def test_the_host_class_fills_the_block():
    p, _keep = AttentionMLADecode(P.FP16, P.FP32)._params(rows=3, column=4096, heads=11, batches=2, scale=SCALE, cacheLengths=LENGTHS, causal=False)
    assert (p.rows, p.column, p.heads, p.batches, p.causal, p.headDimension, p.valueDimension) == (3, 4096, 11, 2, 0, 576, 512)
    assert (p.precision, p.outputPrecision, p.pieces, p.pageSize, p.cacheLengths) == (int(P.FP16), int(P.FP32), 0, 0, LENGTHS)
    assert abs(p.scale - SCALE) < 1e-8
    assert list(p.leadingDimension) == [576, 576, 512] and list(p.headStride) == [3 * 576, 0, 3 * 512]
    assert list(p.batchStride) == [11 * 3 * 576, 4096 * 576, 11 * 3 * 512] and (p.lHeadStride, p.lBatchStride) == (3, 33)
    p, _keep = AttentionMLADecode()._params(rows=1, column=512, heads=4, batches=2, scale=1.0, pieces=3, cacheLengths=LENGTHS, pageSize=64, blockTable=TABLE,
                                            blockTableStride=9, strides=dict(KV=(640, 0, 0)), workspace=WS, workspaceBytes=77)
    assert (p.pieces, p.pageSize, p.blockTable, p.blockTableStride, p.pageStride, p.workspace, p.workspaceBytes) == (3, 64, TABLE, 9, 64 * 640, WS, 77)


def shape(**over):
    kw = dict(rows=1, column=4096, heads=16, batches=2, scale=SCALE, cacheLengths=LENGTHS)
    kw.update(over)
    return kw


def test_the_workspace_is_the_one_formula_and_the_plan_is_decode_s():
    mla = AttentionMLADecode()
    # by hand: 2 sequences x 1 group = 2 workgroups; 512 // 2 = 256 aimed at, 4096 / 64 = 64 tiles / 4 = 16 pieces at most
    assert mla.plannedSplit(**shape()) == (16 * 2 * 16 * 1 * (512 + 2) * 4, 16)
    assert mla.workspaceSize(**shape()) == 1052672
    # heads = 128: four groups a sequence, 8 workgroups -> 64, held to 16 by the tiles; a short cache: 256 keys are 4 tiles, one piece
    assert mla.plannedSplit(**shape(heads=128))[1] == 16 and mla.plannedSplit(**shape(column=256)) == (0, 1)
    assert mla.plannedSplit(**shape(column=32768))[1] == 64                                   # 512 tiles / 4 = 128, 256 aimed at: the cap of 64
    assert mla.plannedSplit(**shape(column=32768, batches=64))[1] == 8                        # 64 workgroups: 512 // 64
    assert mla.plannedSplit(**shape(column=32768, batches=64, heads=128))[1] == 2             # 256 workgroups
    assert mla.plannedSplit(**shape(column=32768, batches=128, heads=128)) == (0, 1)          # 512 workgroups: no split
    assert mla.plannedSplit(**shape(rows=3, heads=11))[1] == 16                               # M = 33: two groups, 4 workgroups -> 128, 16 by tiles
    # pieces as given: 1 is unsplit, 2 .. 64 are taken, whatever the plan
    assert mla.plannedSplit(**shape(pieces=1)) == (0, 1) and mla.plannedSplit(**shape(pieces=0))[1] == 16
    assert mla.plannedSplit(**shape(pieces=7)) == (7 * 2 * 16 * 514 * 4, 7) and mla.plannedSplit(**shape(column=256, pieces=64))[1] == 64
    # a workspace the params already carry is not looked at
    assert mla.plannedSplit(**shape(workspace=WS + 4, workspaceBytes=1)) == (1052672, 16)
    # the same function and constants as decode: D = 256 with one K/V head a sequence has the same workgroups
    from metal_flash_attention_amd import AttentionDecode
    assert AttentionDecode(256).workspaceSize(rows=1, column=4096, heads=8, batches=2, headsPerKeyValue=8,
                                                   cacheLengths=LENGTHS) == 16 * 2 * 8 * (256 + 2) * 4


def test_the_launch_form_names_the_kernels_and_the_grid():
    bf, hf = AttentionMLADecode(P.BF16), AttentionMLADecode(P.FP16)
    need = bf.workspaceSize(**shape())
    form = bf.launchForm(**shape(workspace=WS, workspaceBytes=need))
    assert form == ("attn_mla16_d576_bf16_k (grid 32 = 1 groups x 2 sequences x 16 pieces, 16 packed rows, contiguous) + "
                    "attn_mla16_d576_bf16_combine (grid 8)"), form
    form = bf.launchForm(**shape())
    assert form == "attn_mla16_d576_bf16 (grid 2 = 1 groups x 2 sequences, 16 packed rows, contiguous, unsplit without a workspace: the plan has 16 pieces)", form
    form = hf.launchForm(**shape(rows=3, heads=11, pieces=5, workspace=WS, workspaceBytes=5 * 2 * 33 * 514 * 4, pageSize=16, blockTable=TABLE, blockTableStride=256))
    assert form == ("attn_mla16_d576_f16_k (grid 20 = 2 groups x 2 sequences x 5 pieces, 33 packed rows, paged) + "
                    "attn_mla16_d576_f16_combine (grid 17)"), form
    assert hf.launchForm(**shape(pieces=1, workspace=WS, workspaceBytes=16)) == "attn_mla16_d576_f16 (grid 2 = 1 groups x 2 sequences, 16 packed rows, contiguous)"
    assert bf.launchForm(**shape(heads=128, column=256)) == "attn_mla16_d576_bf16 (grid 8 = 4 groups x 2 sequences, 128 packed rows, contiguous)"
    for name in ("attn_mla16_d576_bf16", "attn_mla16_d576_bf16_k", "attn_mla16_d576_bf16_combine", "attn_mla16_d576_f16", "attn_mla16_d576_f16_k",
                 "attn_mla16_d576_f16_combine"):
        assert not re.fullmatch(r"attn_[a-z0-9]+_(bf16|f16|f32)_d\d+_\w+", name)   # not the form tests/test_variant_coverage.py holds to its map


def outcome(op, q, kv, o, l, kw):
    try:
        op.dispatch(q, kv, o, l, **kw)
    except MFAError as e:
        return e.status, str(e).split(": ", 1)[1]
    return 0, ""


def test_every_refusal_names_its_requirement():
    handle = _abi.lib()
    assert handle.mfa_attention_mla_decode_launch(Q, KV, O, L, None, None) == INVALID and handle.mfa_last_error_string() == b"null argument"
    out = ctypes.create_string_buffer(64)
    assert handle.mfa_attention_mla_decode_launch_form(None, out, 64) == INVALID and handle.mfa_last_error_string() == b"null argument"
    nbytes = ctypes.c_uint64(7)
    assert handle.mfa_attention_mla_decode_workspace_size(None, ctypes.byref(nbytes), None) == INVALID and nbytes.value == 0
    bf = AttentionMLADecode(P.BF16)
    need = bf.workspaceSize(**shape())
    cases = {
        "widths (512, 512)": (AttentionMLADecode(P.BF16, headDimension=512), shape(), UNSUPPORTED, "(576, 512), not (512, 512)"),
        "widths (576, 256)": (AttentionMLADecode(P.BF16, valueDimension=256), shape(), UNSUPPORTED, "(576, 512), not (576, 256)"),
        "fp32 inputs": (AttentionMLADecode(P.FP32), shape(), UNSUPPORTED, "an FP32 cache has no kernel"),
        "a bf16 output beside f16 inputs": (AttentionMLADecode(P.FP16, P.BF16), shape(), INVALID, "outputPrecision must be the inputs' 16-bit type or MFA_FP32"),
        "scale 0": (bf, shape(scale=0.0), INVALID, "scale is required"),
        "scale below 0": (bf, shape(scale=-0.1), INVALID, "scale is required"),
        "scale inf": (bf, shape(scale=float("inf")), INVALID, "scale is required"),
        "scale nan": (bf, shape(scale=float("nan")), INVALID, "scale is required"),
        "zero heads": (bf, shape(heads=0), INVALID, "rows, column, heads and batches must be non-zero"),
        "33 rows": (bf, shape(rows=33), UNSUPPORTED, "at most 32 rows per sequence, not 33"),
        "65 pieces": (bf, shape(pieces=65), INVALID, "pieces must be 0 (the host's plan), 1 (unsplit) or 2 .. 64, not 65"),
        "null cacheLengths": (bf, shape(cacheLengths=None), INVALID, "cacheLengths is required"),
        "a short workspace": (bf, shape(workspace=WS, workspaceBytes=need - 1), INVALID,
                              "workspace too small: %d bytes, the launch needs %d (mfa_attention_mla_decode_workspace_size)" % (need - 1, need)),
        "a misaligned workspace": (bf, shape(workspace=WS + 8, workspaceBytes=need), INVALID, "workspace must be 16-byte aligned"),
        "page size 24": (bf, shape(pageSize=24, blockTable=TABLE, blockTableStride=512), INVALID, "pageSize must be a power of two from 16 to 1024"),
        "page size 2048": (bf, shape(pageSize=2048, blockTable=TABLE, blockTableStride=512), INVALID, "pageSize must be a power of two from 16 to 1024"),
        "paged without a table": (bf, shape(pageSize=16), INVALID, "needs blockTable"),
        "a short table row": (bf, shape(pageSize=16, blockTable=TABLE, blockTableStride=255), INVALID, "blockTableStride must hold the 256 pages"),
        "a cache row stride off 8 elements": (bf, shape(strides=dict(KV=(580, 0, 4096 * 580))), INVALID, "strides of KV must be multiples of 8 elements"),
        "a cache row below 576": (bf, shape(strides=dict(KV=(512, 0, 4096 * 512))), INVALID, "leadingDimension of KV is smaller than the head dimension"),
        "a page stride off 8 elements": (bf, shape(pageSize=16, blockTable=TABLE, blockTableStride=256, pageStride=16 * 576 + 4), INVALID,
                                         "strides of KV must be multiples of 8 elements"),
        "a Q head stride off 8 elements": (bf, shape(strides=dict(Q=(576, 580, 16 * 580))), INVALID, "strides of Q must be multiples of 8 elements"),
        "an O row stride off 4 elements": (bf, shape(strides=dict(O=(514, 514, 16 * 514))), INVALID, "strides of O must be multiples of 4 elements"),
        "an O row below 512": (bf, shape(strides=dict(O=(256, 256, 16 * 256))), INVALID, "leadingDimension of O is smaller than the head dimension"),
    }
    for name, (op, kw, status, needle) in cases.items():
        got = outcome(op, Q, KV, O, L, kw)
        assert got[0] == status and needle in got[1], (name, got)
    # the buffers: null or misaligned, after everything else
    for q, kv, o, l, needle in ((None, KV, O, L, "null argument"), (Q, None, O, L, "null argument"), (Q, KV, None, L, "null argument"),
                                (Q, KV + 8, O, L, "Q, KV and O must be 16-byte aligned"), (Q, KV, O, L + 2, "L must be 4-byte aligned")):
        got = outcome(bf, q, kv, o, l, shape(pieces=1))
        assert got[0] == INVALID and needle in got[1], got
    # decode's own words for the same mistakes
    from metal_flash_attention_amd import AttentionDecode
    dec = AttentionDecode(128)
    base = dict(rows=1, column=4096, heads=8, batches=2, headsPerKeyValue=8, cacheLengths=LENGTHS)
    for mine, theirs in ((shape(workspace=WS + 8, workspaceBytes=need), dict(base, workspace=WS + 8, workspaceBytes=1 << 30)),
                         (shape(pageSize=24, blockTable=TABLE, blockTableStride=512), dict(base, pageSize=24, blockTable=TABLE, blockTableStride=512)),
                         (shape(cacheLengths=None), dict(base, cacheLengths=None))):
        with pytest.raises(MFAError) as said:
            dec.dispatch(Q, KV, KV, O, L, **theirs)
        assert outcome(bf, Q, KV, O, L, mine)[1] == str(said.value).split(": ", 1)[1]
    # a misaligned workspace nobody needs is accepted: the plan of a 256-key cache has one piece, pieces = 1 is unsplit (the form is
    # asked, nothing is launched)
    assert "attn_mla16_d576_bf16 (" in bf.launchForm(**shape(column=256, workspace=WS + 8, workspaceBytes=3))
    assert "attn_mla16_d576_bf16 (" in bf.launchForm(**shape(pieces=1, workspace=WS + 2, workspaceBytes=0))
    # timing arguments
    ms = ctypes.c_float(0)
    p, _keep = bf._params(**shape())
    assert handle.mfa_attention_mla_decode_time(Q, KV, O, L, ctypes.byref(p), None, 0, 0, ctypes.byref(ms)) == INVALID
    assert handle.mfa_last_error_string() == b"bad timing arguments"
