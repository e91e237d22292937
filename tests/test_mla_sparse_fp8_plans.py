"""CPU test (no GPU call, through the built library): the host side of sparse MLA decode over an e4m3 latent cache,
include/mfa_mla_sparse_fp8.h -- every declared name exported and listed, sizes and the piece plan equal to the 16-bit sparse entry's at
the same shapes, the launch form's text, every refusal by status and words IN THE ORDER the header states (the sparse block, the quant
block, the dense e4m3 plan in its words, the grid and the workspace), and the launch forms of the 16-bit sparse and the dense e4m3
entries unchanged: the pointers are made up."""
import ctypes
import os
import re

import metal_flash_attention_amd as mfa
from metal_flash_attention_amd import (AttentionMLADecodeFP8, AttentionMLASparseDecode, AttentionMLASparseDecodeFP8, GEMMOperandPrecision as P,
                                       KVCachePrecision, MFAError, _abi)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS, TABLE, Q, KV, O, L, WS, IDX, KVS = 0x1000, 0x5000, 0x10000, 0x20000, 0x30000, 0x40000, 0x100000, 0x200000, 0x300000   # the host reads none
INVALID, UNSUPPORTED = 2, 3
SCALE = 0.1352
ENTRIES = ("workspace_size", "launch", "launch_form", "time")
PREFIX = "mfa_attention_mla_sparse_decode_fp8_"


def shape(**over):
    kw = dict(rows=1, column=32768, heads=16, batches=2, scale=SCALE, cacheLengths=LENGTHS, indices=IDX, topk=2048, kvScale=KVS)
    kw.update(over)
    return kw


def sparse16(kw):
    return {k: v for k, v in kw.items() if k != "kvScale"}


def dense8(kw):
    return {k: v for k, v in kw.items() if k not in ("indices", "topk", "indexStrides")}


def test_header_symbols_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "mfa_mla_sparse_fp8.h")).read()
    assert '#include "mfa_mla_sparse.h"' in header and '#include "mfa_mla_cache.h"' in header
    declared = set(re.findall(r"\b(mfa_\w+)\s*\(", header.split("#ifndef MFA_MLA_SPARSE_FP8_H")[1]))
    handle = _abi.lib()
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in include/mfa_mla_sparse_fp8.h but not exported"
    assert declared == {s[0] for s in _abi.MLA_SPARSE_FP8_SYMBOLS} == {PREFIX + s for s in ENTRIES}
    for name, restype, argtypes in _abi.MLA_SPARSE_FP8_SYMBOLS:
        fn = getattr(handle, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert int(handle.mfa_abi_version()) == 6 == _abi.EXPECTED_ABI   # mfa.h did not change, and no struct was added
    assert "struct" not in header.split("#ifndef MFA_MLA_SPARSE_FP8_H")[1]
    assert mfa.AttentionMLASparseDecodeFP8 is AttentionMLASparseDecodeFP8 and "AttentionMLASparseDecodeFP8" in dir(mfa)
    assert issubclass(AttentionMLASparseDecodeFP8, AttentionMLASparseDecode)
    assert not {s[0] for s in _abi.MLA_SPARSE_FP8_SYMBOLS} & {s[0] for s in _abi.MLA_SYMBOLS + _abi.MLA_CACHE_SYMBOLS + _abi.MLA_SPARSE_SYMBOLS}
    for text in ("BUILT HERE", "Order of the refusals", "COUNTS TWICE", "NEVER LOADED", "the NaN bytes 0x7f / 0xff included", "Empty rows",
                 "bit for bit", "Deliberately not here", "the 656-byte layout", "per-token or per-128-column scales", "physical-slot indices",
                 "rows > 32", "sharing one list between the rows of a sequence", "more than 32\n * packed rows per workgroup"):
        assert text in header, text
    order = [header.index(t) for t in ("1. the sparse block", "2. the quant block", "3. everything the dense e4m3 launch", "4. the grid's size")]
    assert order == sorted(order)


def test_the_host_class_fills_both_blocks():
    op = AttentionMLASparseDecodeFP8(P.FP16)
    left = shape(rows=3, topk=100)
    (sref, qref), (kept, quant, keep) = op._own(left)
    block, idx = kept
    assert (block.indices, block.topk, block.reserved, block.indexRowStride, block.indexBatchStride, idx) == (IDX, 100, 0, 100, 300, IDX)
    assert (quant.cachePrecision, quant.reserved, quant.kvScale, keep) == (int(KVCachePrecision.E4M3), 0, KVS, KVS)
    assert not {"indices", "topk", "indexStrides", "kvScale"} & set(left)     # what is the blocks' does not reach the params
    (_s, _q), (_kept, quant, keep) = op._own(shape(kvScale=None))
    assert quant.kvScale is None and keep is None


def test_sizes_and_the_plan_are_the_16_bit_sparse_entry_s():
    x8, x16 = AttentionMLASparseDecodeFP8(), AttentionMLASparseDecode()
    assert x8.plannedSplit(**shape()) == (8 * 2 * 16 * 1 * (512 + 2) * 4, 8) and x8.workspaceSize(**shape()) == 526336
    for over in (dict(), dict(topk=64), dict(topk=2049), dict(topk=2048 + 256), dict(column=2048), dict(column=131072), dict(batches=64),
                 dict(batches=64, rows=2), dict(batches=64, rows=2, heads=128), dict(batches=64, heads=33), dict(rows=3, heads=11), dict(pieces=1),
                 dict(pieces=7, rows=3, heads=11), dict(topk=1, pieces=64), dict(workspace=WS + 4, workspaceBytes=1),
                 dict(pageSize=64, blockTable=TABLE, blockTableStride=512), dict(kvScale=None)):
        assert x8.plannedSplit(**shape(**over)) == x16.plannedSplit(**sparse16(shape(**over))), over
    assert x8.plannedSplit(**shape(topk=64)) == (0, 1) and x8.plannedSplit(**shape(batches=64, rows=2))[1] == 4
    assert AttentionMLADecodeFP8().plannedSplit(**dense8(shape()))[1] == 64                  # (the dense e4m3 plan over the same params)


def test_the_launch_form_names_the_kernels_the_grid_and_topk():
    bf, hf = AttentionMLASparseDecodeFP8(P.BF16), AttentionMLASparseDecodeFP8(P.FP16)
    need = bf.workspaceSize(**shape())
    form = bf.launchForm(**shape(workspace=WS, workspaceBytes=need))
    assert form == ("attn_mla8x_d576_bf16_k (grid 16 = 1 groups x 1 rows x 2 sequences x 8 pieces, topk 2048, contiguous) + "
                    "attn_mla8x_d576_bf16_combine (grid 8)"), form
    form = bf.launchForm(**shape())
    assert form == ("attn_mla8x_d576_bf16 (grid 2 = 1 groups x 1 rows x 2 sequences, topk 2048, contiguous, unsplit without a workspace: "
                    "the plan has 8 pieces)"), form
    form = hf.launchForm(**shape(rows=3, heads=40, topk=100, pieces=5, workspace=WS, workspaceBytes=5 * 2 * 120 * 514 * 4, pageSize=16, blockTable=TABLE,
                                 blockTableStride=2048, kvScale=None))
    assert form == ("attn_mla8x_d576_f16_k (grid 60 = 2 groups x 3 rows x 2 sequences x 5 pieces, topk 100, paged) + "
                    "attn_mla8x_d576_f16_combine (grid 60)"), form
    assert hf.launchForm(**shape(pieces=1, workspace=WS, workspaceBytes=16)) == (
        "attn_mla8x_d576_f16 (grid 2 = 1 groups x 1 rows x 2 sequences, topk 2048, contiguous)")
    assert bf.launchForm(**shape(heads=128, topk=64)) == "attn_mla8x_d576_bf16 (grid 8 = 4 groups x 1 rows x 2 sequences, topk 64, contiguous)"
    # the text is the 16-bit sparse entry's with the new kernel names
    x16 = AttentionMLASparseDecode(P.BF16)
    for over in (dict(), dict(workspace=WS, workspaceBytes=need), dict(heads=128, topk=64)):
        assert bf.launchForm(**shape(**over)) == x16.launchForm(**sparse16(shape(**over))).replace("attn_mla16x_", "attn_mla8x_")


def test_the_existing_entries_answer_as_before():
    """the launch forms of the 16-bit sparse entry and of the dense e4m3 entry for the same params: the texts their own files pin"""
    x16 = AttentionMLASparseDecode(P.BF16)
    need = x16.workspaceSize(**sparse16(shape()))
    assert x16.launchForm(**sparse16(shape(workspace=WS, workspaceBytes=need))) == (
        "attn_mla16x_d576_bf16_k (grid 16 = 1 groups x 1 rows x 2 sequences x 8 pieces, topk 2048, contiguous) + attn_mla16x_d576_bf16_combine (grid 8)")
    d8 = AttentionMLADecodeFP8(P.BF16)
    kw = dense8(shape(column=4096))
    need = d8.workspaceSize(**kw)
    assert need == 1052672
    assert d8.launchForm(workspace=WS, workspaceBytes=need, **kw) == (
        "attn_mla8_d576_bf16_k (grid 32 = 1 groups x 2 sequences x 16 pieces, 16 packed rows, contiguous) + attn_mla16_d576_bf16_combine (grid 8)")
    assert d8.launchForm(**kw) == ("attn_mla8_d576_bf16 (grid 2 = 1 groups x 2 sequences, 16 packed rows, contiguous, unsplit without a workspace: "
                                   "the plan has 16 pieces)")


def outcome(op, q, kv, o, l, kw):
    try:
        op.dispatch(q, kv, o, l, **dict(kw))
    except MFAError as e:
        return e.status, str(e).split(": ", 1)[1]
    return 0, ""


def test_every_refusal_names_its_requirement_in_the_header_s_order():
    handle = _abi.lib()
    fn = {verb: getattr(handle, PREFIX + verb) for verb in ENTRIES}
    sp = AttentionMLASparseDecodeFP8(P.BF16)
    p, _keep = sp._params(**dense8(sparse16(shape())))
    (block, quant), _kept = sp._own(shape())
    out, nbytes, ms = ctypes.create_string_buffer(64), ctypes.c_uint64(7), ctypes.c_float(0)
    last = handle.mfa_last_error_string
    # 1. a NULL sparse block, at every entry, before anything else is looked at -- a NULL quant block and NULL params included
    for status in (fn["launch"](Q, KV, O, L, ctypes.byref(p), None, quant, None),
                   fn["launch"](Q, KV, O, L, None, None, None, None),
                   fn["launch_form"](ctypes.byref(p), None, None, out, 64),
                   fn["workspace_size"](ctypes.byref(p), None, quant, ctypes.byref(nbytes), None),
                   fn["time"](Q, KV, O, L, ctypes.byref(p), None, None, None, 0, 1, ctypes.byref(ms))):
        assert status == INVALID and last().startswith(b"null mfa_mla_sparse: the sparse entries require the block")
    assert nbytes.value == 0
    # 2. a NULL quant block beside a good sparse block, at every entry, before the params are looked at
    for status in (fn["launch"](Q, KV, O, L, ctypes.byref(p), block, None, None),
                   fn["launch"](Q, KV, O, L, None, block, None, None),
                   fn["launch_form"](ctypes.byref(p), block, None, out, 64),
                   fn["workspace_size"](ctypes.byref(p), block, None, ctypes.byref(nbytes), None),
                   fn["time"](Q, KV, O, L, ctypes.byref(p), block, None, None, 0, 1, ctypes.byref(ms))):
        assert status == INVALID and last().startswith(b"null mfa_mla_quant: the fp8 entries require the block")
    # 3. NULL params beside two good blocks: the dense launch's words
    assert fn["launch"](Q, KV, O, L, None, block, quant, None) == INVALID and last() == b"null argument"
    assert fn["launch_form"](None, block, quant, out, 64) == INVALID and last() == b"null argument"
    assert fn["workspace_size"](None, block, quant, ctypes.byref(nbytes), None) == INVALID and last() == b"null argument"
    assert fn["launch_form"](ctypes.byref(p), block, quant, None, 64) == INVALID
    assert fn["workspace_size"](ctypes.byref(p), block, quant, None, None) == INVALID and last() == b"null argument"
    need = sp.workspaceSize(**shape())
    bf16_cache = AttentionMLASparseDecodeFP8(P.BF16, cachePrecision=int(P.BF16))
    e5m2_cache = AttentionMLASparseDecodeFP8(P.BF16, cachePrecision=int(KVCachePrecision.E5M2))
    cases = {
        # 1. the sparse block, in mfa_mla_sparse.h's words
        "null indices": (sp, shape(indices=None), INVALID, "mfa_mla_sparse.indices is required"),
        "topk 0": (sp, shape(topk=0), INVALID, "mfa_mla_sparse.topk must be at least 1"),
        "a row stride below topk": (sp, shape(indexStrides=(2047, 4096)), INVALID,
                                    "mfa_mla_sparse.indexRowStride must be at least topk = 2048 entries, not 2047"),
        "misaligned indices": (sp, shape(indices=IDX + 2), INVALID, "mfa_mla_sparse.indices must be 4-byte aligned"),
        # ... before the quant block and before the params
        "null indices beside a 16-bit cache": (bf16_cache, shape(indices=None), INVALID, "mfa_mla_sparse.indices is required"),
        "null indices beside 33 rows": (sp, shape(indices=None, rows=33), INVALID, "mfa_mla_sparse.indices is required"),
        # 2. the quant block, in mfa_mla_cache.h's words, before the params
        "a 16-bit cache": (bf16_cache, shape(), INVALID, "mfa_mla_quant.cachePrecision must be MFA_KV_E4M3, not %d" % int(P.BF16)),
        "a 16-bit cache beside 33 rows": (bf16_cache, shape(rows=33), INVALID, "mfa_mla_quant.cachePrecision must be MFA_KV_E4M3"),
        # 3. what the dense e4m3 plan refuses, in its words
        "widths (512, 512)": (AttentionMLASparseDecodeFP8(P.BF16, headDimension=512), shape(), UNSUPPORTED, "(576, 512), not (512, 512)"),
        "an fp32 Q": (AttentionMLASparseDecodeFP8(P.FP32), shape(), UNSUPPORTED, "takes a 16-bit Q (precision MFA_BF16 or MFA_FP16); an FP32 Q has no kernel"),
        "a bf16 output beside an f16 Q": (AttentionMLASparseDecodeFP8(P.FP16, P.BF16), shape(), INVALID,
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
        "a cache row stride off 16 bytes": (sp, shape(strides=dict(KV=(584, 0, 4096 * 584))), INVALID, "strides of KV must be multiples of 16 elements"),
        "a Q head stride off 8 elements": (sp, shape(strides=dict(Q=(576, 580, 16 * 580))), INVALID, "strides of Q must be multiples of 8 elements"),
        "an O row stride off 4 elements": (sp, shape(strides=dict(O=(514, 514, 16 * 514))), INVALID, "strides of O must be multiples of 4 elements"),
        # ... before the workspace
        "33 rows beside a short workspace": (sp, shape(rows=33, workspace=WS, workspaceBytes=1, pieces=2), UNSUPPORTED, "at most 32 rows per sequence"),
        # 4. the workspace: decode's words, this header's entry
        "a short workspace": (sp, shape(workspace=WS, workspaceBytes=need - 1), INVALID,
                              "workspace too small: %d bytes, the launch needs %d (mfa_attention_mla_sparse_decode_fp8_workspace_size)" % (need - 1, need)),
        "a misaligned workspace": (sp, shape(workspace=WS + 8, workspaceBytes=need), INVALID, "workspace must be 16-byte aligned"),
    }
    for name, (op, kw, status, needle) in cases.items():
        got = outcome(op, Q, KV, O, L, kw)
        assert got[0] == status and needle in got[1], (name, got)
    # e5m2: whatever the dense e4m3 entry says of it
    assert outcome(e5m2_cache, Q, KV, O, L, shape()) == outcome(AttentionMLADecodeFP8(P.BF16, cachePrecision=int(KVCachePrecision.E5M2)), Q, KV, O, L,
                                                                dense8(shape())) != (0, "")
    # reserved != 0: through the sparse block itself
    (block2, quant2), ((raw, _idx), _quant, _scale) = sp._own(shape())
    raw.reserved = 4
    assert fn["launch"](Q, KV, O, L, ctypes.byref(p), block2, quant2, None) == INVALID
    assert last() == b"mfa_mla_sparse.reserved must be 0, not 4"
    # word for word the dense e4m3 launch's text for the same mistake
    dn = AttentionMLADecodeFP8(P.BF16)
    for over in (dict(rows=33), dict(scale=0.0), dict(pageSize=24, blockTable=TABLE, blockTableStride=4096), dict(strides=dict(KV=(584, 0, 4096 * 584))),
                 dict(heads=0), dict(pieces=65), dict(cacheLengths=None)):
        assert outcome(sp, Q, KV, O, L, shape(**over)) == outcome(dn, Q, KV, O, L, dense8(shape(**over))) != (0, "")
    assert outcome(AttentionMLASparseDecodeFP8(P.FP32), Q, KV, O, L, shape()) == outcome(AttentionMLADecodeFP8(P.FP32), Q, KV, O, L, dense8(shape()))
    # word for word the 16-bit sparse launch's text for a mistake of the sparse block
    x16 = AttentionMLASparseDecode(P.BF16)
    for over in (dict(indices=None), dict(topk=0), dict(indexStrides=(2047, 4096)), dict(indices=IDX + 2)):
        assert outcome(sp, Q, KV, O, L, shape(**over)) == outcome(x16, Q, KV, O, L, sparse16(shape(**over))) != (0, "")
    # the buffers and the scale's pointer: null or misaligned, after everything else
    for q, kv, o, l, kvs, needle in ((None, KV, O, L, KVS, "null argument"), (Q, None, O, L, KVS, "null argument"), (Q, KV, None, L, KVS, "null argument"),
                                     (Q, KV + 8, O, L, KVS, "Q, KV and O must be 16-byte aligned"), (Q, KV, O, L + 2, KVS, "L must be 4-byte aligned"),
                                     (Q, KV, O, L, KVS + 2, "kvScale must be 4-byte aligned")):
        got = outcome(sp, q, kv, o, l, shape(pieces=1, kvScale=kvs))
        assert got[0] == INVALID and needle in got[1], got
    # a misaligned workspace nobody needs is accepted (the form is asked, nothing is launched)
    assert "attn_mla8x_d576_bf16 (" in sp.launchForm(**shape(topk=64, workspace=WS + 8, workspaceBytes=3))
    assert "attn_mla8x_d576_bf16 (" in sp.launchForm(**shape(pieces=1, workspace=WS + 2, workspaceBytes=0))
    # timing arguments
    assert fn["time"](Q, KV, O, L, ctypes.byref(p), block, quant, None, 0, 0, ctypes.byref(ms)) == INVALID
    assert last() == b"bad timing arguments"
