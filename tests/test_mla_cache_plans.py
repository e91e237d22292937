"""CPU test (no GPU call, through the built library): the host side of include/mfa_mla_cache.h -- the append of the latent cache and MLA
decode over an e4m3 latent cache.  Every declared name exported and listed in _abi.MLA_CACHE_SYMBOLS, the ctypes mirrors against sizeof
and every offset, the launch forms' kernel names with the 16-bit launch's grids, workspace size and piece count equal to the 16-bit
launch's on a grid of shapes, and every refusal by status and words, before any GPU call: the pointers are made up."""
import ctypes
import itertools
import os
import re

import metal_flash_attention_amd as mfa
from metal_flash_attention_amd import (AttentionMLADecode, AttentionMLADecodeFP8, GEMMOperandPrecision as P, KVCachePrecision, MFAError,
                                       MLACacheAppend, _abi)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS, TABLE, Q, KV, O, L, WS, SCALES = 0x1000, 0x5000, 0x10000, 0x20000, 0x30000, 0x40000, 0x100000, 0x50000   # never read by the host
LATENT, ROPE = 0x60000, 0x70000
INVALID, UNSUPPORTED = 2, 3
SCALE = 0.1352


def test_header_symbols_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "mfa_mla_cache.h")).read()
    assert '#include "mfa_mla.h"' in header and '#include "mfa_kvcache.h"' in header
    declared = set(re.findall(r"\b(mfa_\w+)\s*\(", header.split("#ifndef MFA_MLA_CACHE_H")[1]))
    handle = _abi.lib()
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in include/mfa_mla_cache.h but not exported"
    assert declared == {s[0] for s in _abi.MLA_CACHE_SYMBOLS}
    assert declared == {"mfa_mla_append_params_" + s for s in ("init", "size", "offsets")} | {"mfa_mla_cache_append_launch", "mfa_mla_quant_init"} | {
        "mfa_attention_mla_decode_fp8_" + s for s in ("workspace_size", "launch", "launch_form", "time")}
    for name, restype, argtypes in _abi.MLA_CACHE_SYMBOLS:
        fn = getattr(handle, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert not {s[0] for s in _abi.MLA_CACHE_SYMBOLS} & {s[0] for s in _abi.MLA_SYMBOLS} and len(_abi.MLA_SYMBOLS) == 7   # a list of its own
    assert int(handle.mfa_abi_version()) == 6 == _abi.EXPECTED_ABI   # mfa.h did not change
    assert mfa.AttentionMLADecodeFP8 is AttentionMLADecodeFP8 and mfa.MLACacheAppend is MLACacheAppend
    assert issubclass(AttentionMLADecodeFP8, AttentionMLADecode)
    for said in ("more than 32 packed rows", "ragged append", "per-token or per-128-column scales", "656-byte", "e5m2", "FP8 Q", "FP8 matrix",
                 "a window, sinks, a soft cap or trees", "prefill over the", "compaction of a latent cache"):
        assert said in " ".join(header.replace(" *", "").split()), said   # what is deliberately not here


def test_the_struct_mirrors_match():
    handle = _abi.lib()
    mirror = _abi.mfa_mla_append_params
    assert handle.mfa_mla_append_params_size() == ctypes.sizeof(mirror) == 112
    offsets, count = (ctypes.c_uint32 * 32)(), ctypes.c_uint32(0)
    assert handle.mfa_mla_append_params_offsets(offsets, 32, ctypes.byref(count)) == 0
    want = [getattr(mirror, name).offset for name, _t in mirror._fields_]
    assert count.value == len(want) == 16 and list(offsets[:16]) == want
    assert [name for name, _t in mirror._fields_] == [
        "rows", "batches", "column", "pageSize", "latentDimension", "ropeDimension", "precision", "cachePrecision", "reserved", "cacheLengths",
        "blockTable", "blockTableStride", "leadingDimension", "batchStride", "pageStride", "kvScale"]
    few, count = (ctypes.c_uint32 * 2)(7, 7), ctypes.c_uint32(0)
    assert handle.mfa_mla_append_params_offsets(few, 2, ctypes.byref(count)) == 0 and count.value == 16 and list(few) == want[:2]
    assert handle.mfa_mla_append_params_offsets(None, 2, ctypes.byref(count)) == INVALID
    block = mirror(rows=5, column=9, kvScale=8, cachePrecision=16)
    handle.mfa_mla_append_params_init(ctypes.byref(block))
    assert (block.rows, block.column, block.kvScale, block.pageSize) == (0, 0, None, 0)
    assert (block.latentDimension, block.ropeDimension, block.precision, block.cachePrecision) == (512, 64, int(P.BF16), int(P.BF16))
    quant = _abi.mfa_mla_quant(cachePrecision=3, reserved=4, kvScale=8)
    assert ctypes.sizeof(quant) == 16 and [(_abi.mfa_mla_quant.cachePrecision.offset, _abi.mfa_mla_quant.reserved.offset, _abi.mfa_mla_quant.kvScale.offset)] == [(0, 4, 8)]
    handle.mfa_mla_quant_init(ctypes.byref(quant))
    assert (quant.cachePrecision, quant.reserved, quant.kvScale) == (_abi.MFA_KV_E4M3, 0, None)
    assert handle.mfa_mla_decode_params_size() == 176   # the decode block is the 16-bit launch's, unchanged


def test_the_host_classes_fill_the_blocks():
    p = MLACacheAppend(P.FP16, KVCachePrecision.E4M3)._params(rows=3, batches=2, column=4096, cacheLengths=LENGTHS, kvScale=SCALES)
    assert (p.rows, p.batches, p.column, p.pageSize, p.precision, p.cachePrecision, p.kvScale) == (3, 2, 4096, 0, int(P.FP16), 16, SCALES)
    assert list(p.leadingDimension) == [512, 64, 576] and list(p.batchStride) == [3 * 512, 3 * 64, 4096 * 576]
    p = MLACacheAppend()._params(rows=1, batches=2, cacheLengths=LENGTHS, pageSize=64, blockTable=TABLE, blockTableStride=9,
                                 strides=dict(latentNew=(576, 576), ropeNew=(576, 576), kvCache=(640, 0)))
    assert (p.cachePrecision, p.pageSize, p.blockTable, p.blockTableStride, p.pageStride) == (int(P.BF16), 64, TABLE, 9, 64 * 640)
    assert list(p.leadingDimension) == [576, 576, 640] and list(p.batchStride) == [576, 576, 0]


def shape(**over):
    kw = dict(rows=1, column=4096, heads=16, batches=2, scale=SCALE, cacheLengths=LENGTHS)
    kw.update(over)
    return kw


def test_the_launch_forms_name_the_e4m3_kernels_on_the_16_bit_launch_s_grids():
    for fmt, prec in (("bf16", P.BF16), ("f16", P.FP16)):
        fp8, plain = AttentionMLADecodeFP8(prec), AttentionMLADecode(prec)
        need = plain.workspaceSize(**shape())
        shapes = (shape(), shape(workspace=WS, workspaceBytes=need), shape(pieces=1, workspace=WS, workspaceBytes=16), shape(heads=128, column=256),
                  shape(rows=3, heads=11, pieces=5, workspace=WS, workspaceBytes=5 * 2 * 33 * 514 * 4, pageSize=16, blockTable=TABLE, blockTableStride=256),
                  shape(kvScale=SCALES, workspace=WS, workspaceBytes=need))
        for kw in shapes:
            theirs = plain.launchForm(**{k: v for k, v in kw.items() if k != "kvScale"})
            mine = fp8.launchForm(**kw)
            assert mine == re.sub(r"attn_mla16_d576_%s(_k)? \(" % fmt, r"attn_mla8_d576_%s\1 (" % fmt, theirs) != theirs, (mine, theirs)
        form = fp8.launchForm(**shape(workspace=WS, workspaceBytes=need))
        assert form == ("attn_mla8_d576_%s_k (grid 32 = 1 groups x 2 sequences x 16 pieces, 16 packed rows, contiguous) + "
                        "attn_mla16_d576_%s_combine (grid 8)" % (fmt, fmt)), form
        assert fp8.launchForm(**shape(pieces=1)) == "attn_mla8_d576_%s (grid 2 = 1 groups x 2 sequences, 16 packed rows, contiguous)" % fmt


def test_workspace_and_pieces_are_the_16_bit_launch_s():
    fp8, plain = AttentionMLADecodeFP8(), AttentionMLADecode()
    for rows, heads, batches, column, pieces in itertools.product((1, 3, 32), (1, 11, 16, 128), (1, 2, 64, 128), (256, 4096, 32768), (None, 1, 7, 64)):
        kw = shape(rows=rows, heads=heads, batches=batches, column=column, pieces=pieces)
        assert fp8.plannedSplit(**kw) == plain.plannedSplit(**kw), kw
    assert fp8.plannedSplit(**shape()) == (16 * 2 * 16 * 1 * (512 + 2) * 4, 16) and fp8.workspaceSize(**shape(kvScale=SCALES)) == 1052672
    assert fp8.plannedSplit(**shape(workspace=WS + 4, workspaceBytes=1)) == (1052672, 16)   # a workspace the params carry is not looked at


def outcome(call):
    try:
        call()
    except MFAError as e:
        return e.status, str(e).split(": ", 1)[1]
    return 0, ""


def test_every_decode_refusal_names_its_requirement():
    handle = _abi.lib()
    bf = AttentionMLADecodeFP8(P.BF16)
    p, _keep = bf._params(**shape())
    quant = _abi.mfa_mla_quant()
    handle.mfa_mla_quant_init(ctypes.byref(quant))
    out, nbytes, pieces, ms = ctypes.create_string_buffer(64), ctypes.c_uint64(7), ctypes.c_uint32(7), ctypes.c_float(0)
    # a NULL quant block, by name, from all four entries
    for status in (handle.mfa_attention_mla_decode_fp8_launch(Q, KV, O, L, ctypes.byref(p), None, None),
                   handle.mfa_attention_mla_decode_fp8_launch_form(ctypes.byref(p), None, out, 64),
                   handle.mfa_attention_mla_decode_fp8_workspace_size(ctypes.byref(p), None, ctypes.byref(nbytes), ctypes.byref(pieces)),
                   handle.mfa_attention_mla_decode_fp8_time(Q, KV, O, L, ctypes.byref(p), None, None, 0, 1, ctypes.byref(ms))):
        assert status == INVALID and handle.mfa_last_error_string().startswith(b"null mfa_mla_quant: the fp8 entries require the block")
    assert (nbytes.value, pieces.value) == (0, 0)
    assert handle.mfa_attention_mla_decode_fp8_launch(Q, KV, O, L, None, ctypes.byref(quant), None) == INVALID
    assert handle.mfa_last_error_string() == b"null argument"
    assert handle.mfa_attention_mla_decode_fp8_time(Q, KV, O, L, ctypes.byref(p), ctypes.byref(quant), None, 0, 0, ctypes.byref(ms)) == INVALID
    assert handle.mfa_last_error_string() == b"bad timing arguments"
    need = bf.workspaceSize(**shape())
    cases = {
        "e5m2": (AttentionMLADecodeFP8(P.BF16, cachePrecision=KVCachePrecision.E5M2), shape(), UNSUPPORTED, "e5m2 caches have no kernel"),
        "a 16-bit cache precision": (AttentionMLADecodeFP8(P.BF16, cachePrecision=int(P.BF16)), shape(), INVALID, "mfa_mla_quant.cachePrecision must be MFA_KV_E4M3"),
        "an FP32 Q": (AttentionMLADecodeFP8(P.FP32), shape(), UNSUPPORTED, "an FP32 Q has no kernel"),
        "a bf16 output beside an f16 Q": (AttentionMLADecodeFP8(P.FP16, P.BF16), shape(), INVALID, "outputPrecision must be the inputs' 16-bit type or MFA_FP32"),
        "widths (512, 512)": (AttentionMLADecodeFP8(P.BF16, headDimension=512), shape(), UNSUPPORTED, "(576, 512), not (512, 512)"),
        "scale 0": (bf, shape(scale=0.0), INVALID, "scale is required"),
        "33 rows": (bf, shape(rows=33), UNSUPPORTED, "at most 32 rows per sequence, not 33"),
        "65 pieces": (bf, shape(pieces=65), INVALID, "pieces must be 0 (the host's plan), 1 (unsplit) or 2 .. 64, not 65"),
        "null cacheLengths": (bf, shape(cacheLengths=None), INVALID, "cacheLengths is required"),
        "a short workspace": (bf, shape(workspace=WS, workspaceBytes=need - 1), INVALID,
                              "workspace too small: %d bytes, the launch needs %d (mfa_attention_mla_decode_fp8_workspace_size)" % (need - 1, need)),
        "a misaligned workspace": (bf, shape(workspace=WS + 8, workspaceBytes=need), INVALID, "workspace must be 16-byte aligned"),
        "a row stride off 16 bytes": (bf, shape(strides=dict(KV=(584, 0, 4096 * 592))), INVALID,
                                      "strides of KV must be multiples of 16 elements (16-byte rows of an e4m3 cache)"),
        "a batch stride off 16 bytes": (bf, shape(strides=dict(KV=(576, 0, 4096 * 576 + 8))), INVALID, "strides of KV must be multiples of 16 elements"),
        "a page stride off 16 bytes": (bf, shape(pageSize=16, blockTable=TABLE, blockTableStride=256, pageStride=16 * 576 + 8), INVALID,
                                       "strides of KV must be multiples of 16 elements"),
        "a cache row below 576": (bf, shape(strides=dict(KV=(512, 0, 4096 * 512))), INVALID, "leadingDimension of KV is smaller than the head dimension"),
        "a Q head stride off 8 elements": (bf, shape(strides=dict(Q=(576, 580, 16 * 580))), INVALID, "strides of Q must be multiples of 8 elements"),
        "page size 24": (bf, shape(pageSize=24, blockTable=TABLE, blockTableStride=512), INVALID, "pageSize must be a power of two from 16 to 1024"),
        "a short table row": (bf, shape(pageSize=16, blockTable=TABLE, blockTableStride=255), INVALID, "blockTableStride must hold the 256 pages"),
    }
    for name, (op, kw, status, needle) in cases.items():
        got = outcome(lambda: op.dispatch(Q, KV, O, L, **kw))
        assert got[0] == status and needle in got[1], (name, got)
    # the buffers and the scale, after everything else
    for q, kv, o, l, scale, needle in ((Q, None, O, L, None, "null argument"), (Q, KV + 8, O, L, None, "Q, KV and O must be 16-byte aligned"),
                                       (Q, KV, O, L + 2, None, "L must be 4-byte aligned"), (Q, KV, O, L, SCALES + 2, "kvScale must be 4-byte aligned")):
        got = outcome(lambda: bf.dispatch(q, kv, o, l, **shape(pieces=1, kvScale=scale)))
        assert got[0] == INVALID and needle in got[1], got
    # the 16-bit entries still take strides of 8 and say what they said
    plain = AttentionMLADecode(P.BF16)
    assert "attn_mla16_d576_bf16 (" in plain.launchForm(**shape(pieces=1, strides=dict(KV=(584, 0, 4096 * 584))))
    assert "an FP32 cache has no kernel" in outcome(lambda: AttentionMLADecode(P.FP32).dispatch(Q, KV, O, L, **shape()))[1]


def append_shape(**over):
    kw = dict(rows=3, batches=2, column=4096, cacheLengths=LENGTHS)
    kw.update(over)
    return kw


def test_every_append_refusal_names_its_requirement():
    handle = _abi.lib()
    assert handle.mfa_mla_cache_append_launch(LATENT, ROPE, KV, None, None) == INVALID and handle.mfa_last_error_string() == b"null argument"
    bf, e4 = MLACacheAppend(P.BF16), MLACacheAppend(P.BF16, KVCachePrecision.E4M3)
    paged = dict(column=0, pageSize=16, blockTable=TABLE, blockTableStride=4)
    cases = {
        "a scale beside a 16-bit cache": (bf, append_shape(kvScale=SCALES), INVALID, "kvScale goes with an e4m3 cache (MFA_KV_E4M3); a 16-bit cache takes the rows' bits unscaled"),
        "e5m2": (MLACacheAppend(P.BF16, KVCachePrecision.E5M2), append_shape(), UNSUPPORTED, "e5m2 caches have no kernel"),
        "fp32 rows": (MLACacheAppend(P.FP32), append_shape(), UNSUPPORTED, "the new latent / rotary rows must be 16-bit"),
        "an f16 cache beside bf16 rows": (MLACacheAppend(P.BF16, int(P.FP16)), append_shape(), INVALID, "cachePrecision must be the rows' 16-bit type (`precision`) or MFA_KV_E4M3"),
        "a latent of 256": (MLACacheAppend(P.BF16, latentDimension=256), append_shape(), UNSUPPORTED, "(latentDimension, ropeDimension) = (512, 64), not (256, 64)"),
        "a rotary part of 128": (MLACacheAppend(P.BF16, ropeDimension=128), append_shape(), UNSUPPORTED, "(latentDimension, ropeDimension) = (512, 64), not (512, 128)"),
        "zero rows": (bf, append_shape(rows=0), INVALID, "rows and batches must be non-zero"),
        "null cacheLengths": (bf, append_shape(cacheLengths=None), INVALID, "cacheLengths is required"),
        "a contiguous cache without a capacity": (bf, append_shape(column=0), INVALID, "column (the capacity of a contiguous cache) must be non-zero"),
        "page size 24": (bf, append_shape(**dict(paged, pageSize=24)), INVALID, "pageSize must be a power of two from 16 to 1024"),
        "paged without a table": (bf, append_shape(**dict(paged, blockTable=None)), INVALID, "needs blockTable"),
        "a table without a row": (bf, append_shape(**dict(paged, blockTableStride=0)), INVALID, "blockTableStride must be positive"),
        "a latent row below 512": (bf, append_shape(strides=dict(latentNew=(256, 3 * 256))), INVALID, "leadingDimension of latentNew is smaller than the head dimension"),
        "a rotary row below 64": (bf, append_shape(strides=dict(ropeNew=(32, 96))), INVALID, "leadingDimension of ropeNew is smaller than the head dimension"),
        "a latent row stride off 8": (bf, append_shape(strides=dict(latentNew=(516, 3 * 516))), INVALID, "strides of latentNew must be multiples of 8 elements"),
        "a rotary batch stride off 8": (bf, append_shape(strides=dict(ropeNew=(64, 196))), INVALID, "strides of ropeNew must be multiples of 8 elements"),
        "a cache row below 576": (bf, append_shape(strides=dict(kvCache=(512, 4096 * 512))), INVALID, "leadingDimension of kvCache is smaller than the head dimension"),
        "a 16-bit cache stride off 8": (bf, append_shape(strides=dict(kvCache=(580, 4096 * 580))), INVALID, "strides of kvCache must be multiples of 8 elements"),
        "an e4m3 cache stride off 16": (e4, append_shape(strides=dict(kvCache=(584, 4096 * 592))), INVALID, "strides of kvCache must be multiples of 16 elements"),
        "an e4m3 page stride off 16": (e4, append_shape(**dict(paged, pageStride=16 * 576 + 8)), INVALID, "strides of kvCache must be multiples of 16 elements"),
    }
    for name, (op, kw, status, needle) in cases.items():
        got = outcome(lambda: op.dispatch(LATENT, ROPE, KV, **kw))
        assert got[0] == status and needle in got[1], (name, got)
    for latent, rope, kv, scale, needle in ((None, ROPE, KV, None, "null argument"), (LATENT, None, KV, None, "null argument"), (LATENT, ROPE, None, None, "null argument"),
                                            (LATENT + 8, ROPE, KV, None, "latentNew, ropeNew and kvCache must be 16-byte aligned"),
                                            (LATENT, ROPE, KV + 8, None, "latentNew, ropeNew and kvCache must be 16-byte aligned"),
                                            (LATENT, ROPE, KV, SCALES + 1, "kvScale must be 4-byte aligned")):
        got = outcome(lambda: e4.dispatch(latent, rope, kv, **append_shape(kvScale=scale)))
        assert got[0] == INVALID and needle in got[1], got
