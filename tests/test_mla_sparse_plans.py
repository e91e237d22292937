"""CPU test (no GPU call, through the built library): the host side of sparse MLA decode, include/mfa_mla_sparse.h -- every declared
name exported and listed, the ctypes mirror of mfa_mla_sparse against sizeof and every offset, the workspace formula at a hand-computed
shape, the plan over the 64-slot tiles of topk, the launch form's text, every refusal of the block by status and words, the dense
launch's refusals in the dense launch's words, and the dense entries' launch forms unchanged: the pointers are made up."""
import ctypes
import os
import re

import pytest

import metal_flash_attention_amd as mfa
from metal_flash_attention_amd import AttentionMLADecode, AttentionMLASparseDecode, GEMMOperandPrecision as P, MFAError, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS, TABLE, Q, KV, O, L, WS, IDX = 0x1000, 0x5000, 0x10000, 0x20000, 0x30000, 0x40000, 0x100000, 0x200000   # the host reads none of them
INVALID, UNSUPPORTED = 2, 3
SCALE = 0.1352
ENTRIES = ("workspace_size", "launch", "launch_form", "time")


def shape(**over):
    kw = dict(rows=1, column=32768, heads=16, batches=2, scale=SCALE, cacheLengths=LENGTHS, indices=IDX, topk=2048)
    kw.update(over)
    return kw


def dense(kw):
    return {k: v for k, v in kw.items() if k not in ("indices", "topk", "indexStrides")}


def test_header_symbols_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "mfa_mla_sparse.h")).read()
    assert '#include "mfa_mla.h"' in header
    declared = set(re.findall(r"\b(mfa_\w+)\s*\(", header.split("#ifndef MFA_MLA_SPARSE_H")[1]))
    handle = _abi.lib()
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in include/mfa_mla_sparse.h but not exported"
    assert declared == {s[0] for s in _abi.MLA_SPARSE_SYMBOLS}
    assert declared == {"mfa_mla_sparse_" + s for s in ("init", "size", "offsets")} | {"mfa_attention_mla_sparse_decode_" + s for s in ENTRIES}
    for name, restype, argtypes in _abi.MLA_SPARSE_SYMBOLS:
        fn = getattr(handle, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert int(handle.mfa_abi_version()) == 6 == _abi.EXPECTED_ABI   # mfa.h did not change
    assert mfa.AttentionMLASparseDecode is AttentionMLASparseDecode and "AttentionMLASparseDecode" in dir(mfa)
    assert not set(s[0] for s in _abi.MLA_SPARSE_SYMBOLS) & set(s[0] for s in _abi.MLA_SYMBOLS + _abi.MLA_CACHE_SYMBOLS)
    for text in ("COUNTS TWICE", "NEVER LOADED", "Deliberately not here", "e4m3 latent caches under a list", "physical-slot indices",
                 "per-row list lengths other than through -1", "more than\n * 32 packed rows", "sharing one list between the rows of a sequence"):
        assert text in header, text


def test_the_struct_mirror_matches():
    handle = _abi.lib()
    mirror = _abi.mfa_mla_sparse
    assert handle.mfa_mla_sparse_size() == ctypes.sizeof(mirror) == 32
    offsets, count = (ctypes.c_uint32 * 8)(), ctypes.c_uint32(0)
    assert handle.mfa_mla_sparse_offsets(offsets, 8, ctypes.byref(count)) == 0
    want = [getattr(mirror, name).offset for name, _t in mirror._fields_]
    assert count.value == len(want) == 5 and list(offsets[:5]) == want == [0, 8, 12, 16, 24]
    assert [name for name, _t in mirror._fields_] == ["indices", "topk", "reserved", "indexRowStride", "indexBatchStride"]
    few, count = (ctypes.c_uint32 * 2)(7, 7), ctypes.c_uint32(0)                    # a small capacity: the count is still said
    assert handle.mfa_mla_sparse_offsets(few, 2, ctypes.byref(count)) == 0 and count.value == 5 and list(few) == want[:2]
    assert handle.mfa_mla_sparse_offsets(None, 2, ctypes.byref(count)) == INVALID
    block = mirror(indices=8, topk=5, reserved=3, indexRowStride=9, indexBatchStride=11)
    handle.mfa_mla_sparse_init(ctypes.byref(block))
    assert (block.indices, block.topk, block.reserved, block.indexRowStride, block.indexBatchStride) == (None, 0, 0, 0, 0)
    assert handle.mfa_mla_decode_params_size() == 176                              # the params are the dense launch's, unchanged


def test_the_host_class_fills_the_block():
    op = AttentionMLASparseDecode(P.FP16)
    (ref,), (block, keep) = op._own(shape(rows=3, topk=100))
    assert (block.indices, block.topk, block.reserved, block.indexRowStride, block.indexBatchStride, keep) == (IDX, 100, 0, 100, 300, IDX)
    (ref,), (block, keep) = op._own(shape(rows=3, topk=100, indexStrides=(128, 0)))
    assert (block.indexRowStride, block.indexBatchStride) == (128, 0)
    left = shape()
    op._own(left)
    assert not {"indices", "topk", "indexStrides"} & set(left)     # what is the block's does not reach the params


def test_the_workspace_is_the_one_formula_and_the_plan_runs_over_the_slots():
    mla = AttentionMLASparseDecode()
    # by hand: 2 sequences x 1 row x 1 group = 2 workgroups, 512 // 2 = 256 aimed at; 2048 slots are 32 tiles, / 4 = 8 pieces at most
    assert mla.plannedSplit(**shape()) == (8 * 2 * 16 * 1 * (512 + 2) * 4, 8)
    assert mla.workspaceSize(**shape()) == 526336
    assert mla.plannedSplit(**shape(topk=64)) == (0, 1)                                      # one tile: nothing to cut
    assert mla.plannedSplit(**shape(topk=2049))[1] == 8                                      # 33 tiles // 4
    assert mla.plannedSplit(**shape(topk=2048 + 256))[1] == 9
    # the column does not enter the plan, only the list does
    assert mla.plannedSplit(**shape(column=2048)) == mla.plannedSplit(**shape()) == mla.plannedSplit(**shape(column=131072))
    assert AttentionMLADecode().plannedSplit(**dense(shape()))[1] == 64                      # (the dense plan over the same params)
    # the workgroups are batches x rows x groups of 32 HEADS: rows multiply them, heads only past 32
    assert mla.plannedSplit(**shape(batches=64))[1] == 8                                     # 64 workgroups: 512 // 64 = 8, and 8 by the tiles
    assert mla.plannedSplit(**shape(batches=64, rows=2))[1] == 4                             # 128 workgroups
    assert mla.plannedSplit(**shape(batches=64, rows=2, heads=128))[1] == 1                  # 512 workgroups: no split
    assert mla.plannedSplit(**shape(batches=64, heads=33))[1] == 4                           # two groups, the second of one head
    assert mla.plannedSplit(**shape(rows=3, heads=11))[1] == 8                               # M = 33 rows are still ONE group of 11 heads, 6 workgroups
    # pieces as given
    assert mla.plannedSplit(**shape(pieces=1)) == (0, 1) and mla.plannedSplit(**shape(pieces=0))[1] == 8
    assert mla.plannedSplit(**shape(pieces=7, rows=3, heads=11)) == (7 * 2 * 11 * 3 * 514 * 4, 7) and mla.plannedSplit(**shape(topk=1, pieces=64))[1] == 64
    assert mla.plannedSplit(**shape(workspace=WS + 4, workspaceBytes=1)) == (526336, 8)      # a workspace the params carry is not looked at


def test_the_launch_form_names_the_kernels_the_grid_and_topk():
    bf, hf = AttentionMLASparseDecode(P.BF16), AttentionMLASparseDecode(P.FP16)
    need = bf.workspaceSize(**shape())
    form = bf.launchForm(**shape(workspace=WS, workspaceBytes=need))
    assert form == ("attn_mla16x_d576_bf16_k (grid 16 = 1 groups x 1 rows x 2 sequences x 8 pieces, topk 2048, contiguous) + "
                    "attn_mla16x_d576_bf16_combine (grid 8)"), form
    form = bf.launchForm(**shape())
    assert form == ("attn_mla16x_d576_bf16 (grid 2 = 1 groups x 1 rows x 2 sequences, topk 2048, contiguous, unsplit without a workspace: "
                    "the plan has 8 pieces)"), form
    form = hf.launchForm(**shape(rows=3, heads=40, topk=100, pieces=5, workspace=WS, workspaceBytes=5 * 2 * 120 * 514 * 4, pageSize=16, blockTable=TABLE,
                                 blockTableStride=2048))
    assert form == ("attn_mla16x_d576_f16_k (grid 60 = 2 groups x 3 rows x 2 sequences x 5 pieces, topk 100, paged) + "
                    "attn_mla16x_d576_f16_combine (grid 60)"), form
    assert hf.launchForm(**shape(pieces=1, workspace=WS, workspaceBytes=16)) == (
        "attn_mla16x_d576_f16 (grid 2 = 1 groups x 1 rows x 2 sequences, topk 2048, contiguous)")
    assert bf.launchForm(**shape(heads=128, topk=64)) == "attn_mla16x_d576_bf16 (grid 8 = 4 groups x 1 rows x 2 sequences, topk 64, contiguous)"


def test_the_dense_entries_answer_as_before():
    """the launch forms of the entries of mfa_mla.h for the same params: the texts tests/test_mla_plans.py pins"""
    bf = AttentionMLADecode(P.BF16)
    kw = dense(shape(column=4096))
    need = bf.workspaceSize(**kw)
    assert need == 1052672
    assert bf.launchForm(workspace=WS, workspaceBytes=need, **kw) == (
        "attn_mla16_d576_bf16_k (grid 32 = 1 groups x 2 sequences x 16 pieces, 16 packed rows, contiguous) + attn_mla16_d576_bf16_combine (grid 8)")
    assert bf.launchForm(**kw) == ("attn_mla16_d576_bf16 (grid 2 = 1 groups x 2 sequences, 16 packed rows, contiguous, unsplit without a workspace: "
                                   "the plan has 16 pieces)")


def outcome(op, q, kv, o, l, kw):
    try:
        op.dispatch(q, kv, o, l, **kw)
    except MFAError as e:
        return e.status, str(e).split(": ", 1)[1]
    return 0, ""


def test_every_refusal_names_its_requirement():
    handle = _abi.lib()
    sp = AttentionMLASparseDecode(P.BF16)
    p, _keep = sp._params(**dense(shape()))
    # a NULL block, at every entry, before anything else is looked at
    out, nbytes, ms = ctypes.create_string_buffer(64), ctypes.c_uint64(7), ctypes.c_float(0)
    for status in (handle.mfa_attention_mla_sparse_decode_launch(Q, KV, O, L, ctypes.byref(p), None, None),
                   handle.mfa_attention_mla_sparse_decode_launch(Q, KV, O, L, None, None, None),
                   handle.mfa_attention_mla_sparse_decode_launch_form(ctypes.byref(p), None, out, 64),
                   handle.mfa_attention_mla_sparse_decode_workspace_size(ctypes.byref(p), None, ctypes.byref(nbytes), None),
                   handle.mfa_attention_mla_sparse_decode_time(Q, KV, O, L, ctypes.byref(p), None, None, 0, 1, ctypes.byref(ms))):
        assert status == INVALID and handle.mfa_last_error_string().startswith(b"null mfa_mla_sparse: the sparse entries require the block")
    assert nbytes.value == 0
    # NULL params beside a good block: the dense launch's words
    (block,), _kept = sp._own(shape())
    assert handle.mfa_attention_mla_sparse_decode_launch(Q, KV, O, L, None, block, None) == INVALID and handle.mfa_last_error_string() == b"null argument"
    assert handle.mfa_attention_mla_sparse_decode_launch_form(None, block, out, 64) == INVALID and handle.mfa_last_error_string() == b"null argument"
    assert handle.mfa_attention_mla_sparse_decode_launch_form(ctypes.byref(p), block, None, 64) == INVALID
    need = sp.workspaceSize(**shape())
    cases = {
        "null indices": (sp, shape(indices=None), INVALID, "mfa_mla_sparse.indices is required"),
        "topk 0": (sp, shape(topk=0), INVALID, "mfa_mla_sparse.topk must be at least 1"),
        "a row stride below topk": (sp, shape(indexStrides=(2047, 4096)), INVALID,
                                    "mfa_mla_sparse.indexRowStride must be at least topk = 2048 entries, not 2047"),
        "misaligned indices": (sp, shape(indices=IDX + 2), INVALID, "mfa_mla_sparse.indices must be 4-byte aligned"),
        # the block first, then the params
        "null indices beside 33 rows": (sp, shape(indices=None, rows=33), INVALID, "mfa_mla_sparse.indices is required"),
        # what the dense plan refuses, in its words
        "widths (512, 512)": (AttentionMLASparseDecode(P.BF16, headDimension=512), shape(), UNSUPPORTED, "(576, 512), not (512, 512)"),
        "fp32 inputs": (AttentionMLASparseDecode(P.FP32), shape(), UNSUPPORTED, "an FP32 cache has no kernel"),
        "a bf16 output beside f16 inputs": (AttentionMLASparseDecode(P.FP16, P.BF16), shape(), INVALID,
                                            "outputPrecision must be the inputs' 16-bit type or MFA_FP32"),
        "scale 0": (sp, shape(scale=0.0), INVALID, "scale is required"),
        "scale nan": (sp, shape(scale=float("nan")), INVALID, "scale is required"),
        "zero heads": (sp, shape(heads=0), INVALID, "rows, column, heads and batches must be non-zero"),
        "33 rows": (sp, shape(rows=33), UNSUPPORTED, "at most 32 rows per sequence, not 33"),
        "65 pieces": (sp, shape(pieces=65), INVALID, "pieces must be 0 (the host's plan), 1 (unsplit) or 2 .. 64, not 65"),
        "null cacheLengths": (sp, shape(cacheLengths=None), INVALID, "cacheLengths is required"),
        "page size 24": (sp, shape(pageSize=24, blockTable=TABLE, blockTableStride=4096), INVALID, "pageSize must be a power of two from 16 to 1024"),
        "paged without a table": (sp, shape(pageSize=16), INVALID, "needs blockTable"),
        "a short table row": (sp, shape(pageSize=16, blockTable=TABLE, blockTableStride=2047), INVALID, "blockTableStride must hold the 2048 pages"),
        "a cache row stride off 8 elements": (sp, shape(strides=dict(KV=(580, 0, 4096 * 580))), INVALID, "strides of KV must be multiples of 8 elements"),
        "a Q head stride off 8 elements": (sp, shape(strides=dict(Q=(576, 580, 16 * 580))), INVALID, "strides of Q must be multiples of 8 elements"),
        "an O row stride off 4 elements": (sp, shape(strides=dict(O=(514, 514, 16 * 514))), INVALID, "strides of O must be multiples of 4 elements"),
        # the workspace: decode's words, this header's entry
        "a short workspace": (sp, shape(workspace=WS, workspaceBytes=need - 1), INVALID,
                              "workspace too small: %d bytes, the launch needs %d (mfa_attention_mla_sparse_decode_workspace_size)" % (need - 1, need)),
        "a misaligned workspace": (sp, shape(workspace=WS + 8, workspaceBytes=need), INVALID, "workspace must be 16-byte aligned"),
    }
    for name, (op, kw, status, needle) in cases.items():
        got = outcome(op, Q, KV, O, L, kw)
        assert got[0] == status and needle in got[1], (name, got)
    # reserved != 0: through the block itself
    (block,), (raw, _idx) = sp._own(shape())
    raw.reserved = 4
    assert handle.mfa_attention_mla_sparse_decode_launch(Q, KV, O, L, ctypes.byref(p), block, None) == INVALID
    assert handle.mfa_last_error_string() == b"mfa_mla_sparse.reserved must be 0, not 4"
    # word for word the dense launch's text for the same mistake
    dn = AttentionMLADecode(P.BF16)
    for over in (dict(rows=33), dict(scale=0.0), dict(pageSize=24, blockTable=TABLE, blockTableStride=4096), dict(strides=dict(KV=(580, 0, 4096 * 580)))):
        assert outcome(sp, Q, KV, O, L, shape(**over)) == outcome(dn, Q, KV, O, L, dense(shape(**over))) != (0, "")
    # the buffers: null or misaligned, after everything else
    for q, kv, o, l, needle in ((None, KV, O, L, "null argument"), (Q, None, O, L, "null argument"), (Q, KV, None, L, "null argument"),
                                (Q, KV + 8, O, L, "Q, KV and O must be 16-byte aligned"), (Q, KV, O, L + 2, "L must be 4-byte aligned")):
        got = outcome(sp, q, kv, o, l, shape(pieces=1))
        assert got[0] == INVALID and needle in got[1], got
    # a misaligned workspace nobody needs is accepted (the form is asked, nothing is launched)
    assert "attn_mla16x_d576_bf16 (" in sp.launchForm(**shape(topk=64, workspace=WS + 8, workspaceBytes=3))
    assert "attn_mla16x_d576_bf16 (" in sp.launchForm(**shape(pieces=1, workspace=WS + 2, workspaceBytes=0))
    # timing arguments
    (block,), _kept = sp._own(shape())
    assert handle.mfa_attention_mla_sparse_decode_time(Q, KV, O, L, ctypes.byref(p), block, None, 0, 0, ctypes.byref(ms)) == INVALID
    assert handle.mfa_last_error_string() == b"bad timing arguments"
