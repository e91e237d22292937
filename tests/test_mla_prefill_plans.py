"""CPU test (no GPU call, through the built library): the host side of multi-head latent attention prefill, include/mfa_mla_prefill.h --
every declared name exported, the ctypes mirror against sizeof and every offset, the host class's block, the launch form's kernel name
and grid, the range function (the very function the kernels run: mla_prefill_step_range, csrc/attn_mla16_prefill.h) against a
brute-force walk of the mask, and every refusal by status and words, before any GPU call: the pointers are made up.  MLA decode still
refuses 33 rows in its own words."""
import ctypes
import os
import re

import numpy as np
import pytest

import metal_flash_attention_amd as mfa
from metal_flash_attention_amd import AttentionMLADecode, AttentionMLAPrefill, GEMMOperandPrecision as P, MFAError, _abi

import mla_prefill_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS, QLENGTHS, TABLE, Q, KV, O, L = 0x1000, 0x2000, 0x5000, 0x10000, 0x20000, 0x30000, 0x40000   # the host never reads what they point to
INVALID, UNSUPPORTED = 2, 3
SCALE = 0.1352


def test_header_symbols_exported_and_the_ctypes_mirror():
    header = open(os.path.join(ROOT, "include", "mfa_mla_prefill.h")).read()
    assert '#include "mfa_mla.h"' in header
    declared = set(re.findall(r"\b(mfa_\w+)\s*\(", header.split("#ifndef MFA_MLA_PREFILL_H")[1]))
    handle = _abi.lib()
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in include/mfa_mla_prefill.h but not exported"
    assert declared == {s[0] for s in _abi.MLA_PREFILL_SYMBOLS}
    assert declared == {"mfa_mla_prefill_params_" + s for s in ("init", "size", "offsets")} | {
        "mfa_attention_mla_prefill_" + s for s in ("launch", "launch_form", "time", "step_range")}
    for name, restype, argtypes in _abi.MLA_PREFILL_SYMBOLS:
        fn = getattr(handle, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert int(handle.mfa_abi_version()) == 6 == _abi.EXPECTED_ABI   # mfa.h did not change
    assert mfa.AttentionMLAPrefill is AttentionMLAPrefill and "AttentionMLAPrefill" in dir(mfa)
    assert "mla" not in " ".join(_abi.CACHE_FAMILIES["decode"]) and "mla" not in " ".join(_abi.CACHE_FAMILIES["prefill"])   # in no family table
    assert "MFA_MLA_PREFILL_PACKED_ROWS 64" in header and _abi.MFA_MLA_PREFILL_PACKED_ROWS == 64 == AttentionMLAPrefill.PACKED_ROWS
    assert "MFA_MLA_PREFILL_KEY_STEP 32" in header and _abi.MFA_MLA_PREFILL_KEY_STEP == 32 == pm.STEP
    assert not hasattr(AttentionMLAPrefill, "plannedSplit") and not hasattr(AttentionMLAPrefill, "workspaceSize")
    for said in ("key pieces", "e4m3 latent caches", "ragged", "lists of key positions", "a window, sinks, a soft cap or trees"):
        assert said in header.split("Deliberately not here")[1], said


def test_the_struct_mirror_matches_and_decode_s_did_not_move():
    handle = _abi.lib()
    mirror = _abi.mfa_mla_prefill_params
    assert handle.mfa_mla_prefill_params_size() == ctypes.sizeof(mirror) == 168
    offsets, count = (ctypes.c_uint32 * 32)(), ctypes.c_uint32(0)
    assert handle.mfa_mla_prefill_params_offsets(offsets, 32, ctypes.byref(count)) == 0
    want = [getattr(mirror, name).offset for name, _t in mirror._fields_]
    assert count.value == len(want) == 22 and list(offsets[:22]) == want
    decode = [name for name, _t in _abi.mfa_mla_decode_params._fields_]
    mine = [name for name, _t in mirror._fields_]
    assert [n for n in decode if n not in ("pieces", "workspace", "workspaceBytes")] == [n for n in mine if n != "queryLengths"]
    assert mine.index("queryLengths") == mine.index("cacheLengths") + 1
    few, count = (ctypes.c_uint32 * 2)(7, 7), ctypes.c_uint32(0)                    # a small capacity: the count is still said
    assert handle.mfa_mla_prefill_params_offsets(few, 2, ctypes.byref(count)) == 0 and count.value == 22 and list(few) == want[:2]
    assert handle.mfa_mla_prefill_params_offsets(None, 2, ctypes.byref(count)) == INVALID
    block = mirror(rows=5, causal=0, scale=3.0, queryLengths=8)
    handle.mfa_mla_prefill_params_init(ctypes.byref(block))
    assert (block.rows, block.causal, block.scale, block.queryLengths) == (0, 1, 0.0, None)          # no default scale
    assert (block.headDimension, block.valueDimension, block.precision, block.outputPrecision) == (576, 512, int(P.BF16), int(P.BF16))
    assert handle.mfa_mla_decode_params_size() == ctypes.sizeof(_abi.mfa_mla_decode_params) == 176   # no existing struct moved


def test_the_host_class_fills_the_block():
    p, _keep = AttentionMLAPrefill(P.FP16, P.FP32)._params(rows=300, column=4096, heads=11, batches=2, scale=SCALE, cacheLengths=LENGTHS,
                                                            queryLengths=QLENGTHS, causal=False)
    assert (p.rows, p.column, p.heads, p.batches, p.causal, p.headDimension, p.valueDimension) == (300, 4096, 11, 2, 0, 576, 512)
    assert (p.precision, p.outputPrecision, p.pageSize, p.cacheLengths, p.queryLengths) == (int(P.FP16), int(P.FP32), 0, LENGTHS, QLENGTHS)
    assert abs(p.scale - SCALE) < 1e-8
    assert list(p.leadingDimension) == [576, 576, 512] and list(p.headStride) == [300 * 576, 0, 300 * 512]
    assert list(p.batchStride) == [11 * 300 * 576, 4096 * 576, 11 * 300 * 512] and (p.lHeadStride, p.lBatchStride) == (300, 3300)
    p, _keep = AttentionMLAPrefill()._params(rows=70, column=512, heads=4, batches=2, scale=1.0, cacheLengths=LENGTHS, pageSize=64, blockTable=TABLE,
                                             blockTableStride=9, strides=dict(KV=(640, 0, 0), Q=(4 * 576, 576, 70 * 4 * 576)))
    assert (p.queryLengths, p.pageSize, p.blockTable, p.blockTableStride, p.pageStride) == (None, 64, TABLE, 9, 64 * 640)
    assert (p.leadingDimension[0], p.headStride[0], p.batchStride[0]) == (4 * 576, 576, 70 * 4 * 576)          # a token-major Q is a plain launch


def shape(**over):
    kw = dict(rows=200, column=4096, heads=16, batches=2, scale=SCALE, cacheLengths=LENGTHS)
    kw.update(over)
    return kw


def test_the_launch_form_names_the_kernel_and_the_grid():
    bf, hf = AttentionMLAPrefill(P.BF16), AttentionMLAPrefill(P.FP16)
    form = bf.launchForm(**shape())
    assert form == "attn_mla16p_d576_bf16 (grid 100 = 50 blocks x 2 sequences, 3200 packed rows in blocks of 64, contiguous)", form
    form = hf.launchForm(**shape(rows=13, heads=5, batches=3, pageSize=16, blockTable=TABLE, blockTableStride=256, queryLengths=QLENGTHS))
    assert form == "attn_mla16p_d576_f16 (grid 6 = 2 blocks x 3 sequences, 65 packed rows in blocks of 64, paged)", form
    for rows, heads, batches in ((1, 1, 1), (32, 2, 1), (33, 2, 4), (2048, 128, 8), (1, 128, 2), (200, 64, 7)):
        form = bf.launchForm(**shape(rows=rows, heads=heads, batches=batches))
        blocks = -(-rows * heads // 64)
        assert form.startswith("attn_mla16p_d576_bf16 (grid %d = %d blocks x %d sequences" % (batches * blocks, blocks, batches)), form
    assert not re.fullmatch(r"attn_[a-z0-9]+_(bf16|f16|f32)_d\d+_\w+", "attn_mla16p_d576_bf16")


def brute(n, qn, H, causal):
    """(firstMasked, end) of every block of a sequence by walking the mask, key by key: vis[r][c] is the header's rule; a step is SEEN by a
    block when some live row of it sees some key of the step, and CUT when some live row does not see some key of it.  end = one past
    the last seen step; firstMasked = the first cut step, held to end.  One block more than the sequence has: it has no live row."""
    p0s = np.arange(0, qn * H + 64, 64)
    if n == 0 or qn == 0:
        return p0s, np.zeros((len(p0s), 2), dtype=np.int64)
    steps = -(-n // 32) + 1
    c, r = np.arange(32 * steps)[None, :], np.arange(qn)[:, None]
    vis = (c < n) & ((c <= r + max(n - qn, 0)) if causal else True)
    vis = np.broadcast_to(vis, (qn, 32 * steps)).reshape(qn, steps, 32)
    seen_rows = np.concatenate([np.zeros((1, steps), dtype=np.int64), np.cumsum(vis.any(axis=2), axis=0)])      # [rows + 1, steps]
    cut_rows = np.concatenate([np.zeros((1, steps), dtype=np.int64), np.cumsum(~vis.all(axis=2), axis=0)])
    r0 = np.minimum(p0s // H, qn)
    r1 = np.minimum((p0s + 63) // H + 1, qn)                      # the block's live rows are r0 .. r1 - 1
    seen = seen_rows[r1] - seen_rows[r0] > 0                      # [blocks, steps]
    cut = cut_rows[r1] - cut_rows[r0] > 0
    idx = np.arange(steps)[None, :]
    end = np.where(seen, idx + 1, 0).max(axis=1)
    first = np.where(cut, idx, steps).min(axis=1)
    return p0s, np.stack([np.minimum(first, end), end], axis=1)


@pytest.mark.parametrize("H", [1, 5, 16, 64, 128])
def test_step_range_against_a_brute_force_walk_of_the_mask(H):
    """over every (length, qn) <= 100, every block and both masks: no visible (row, key) pair at or past `end`, none cut below
    `firstMasked`, `end` minimal -- and firstMasked as large as the mask lets it be"""
    handle = _abi.lib()
    fn = handle.mfa_attention_mla_prefill_step_range
    f, e = ctypes.c_uint32(7), ctypes.c_uint32(7)
    fp, ep = ctypes.byref(f), ctypes.byref(e)
    sr = AttentionMLAPrefill.stepRange
    for causal in (1, 0):
        for n in range(0, 101):
            for qn in range(0, 101):
                p0s, want = brute(n, qn, H, causal)
                for p0, (wf, we) in zip(p0s.tolist(), want.tolist()):
                    assert fn(n, qn, p0, H, causal, fp, ep) == 0 and (f.value, e.value) == (wf, we), (n, qn, p0, H, causal, f.value, e.value, wf, we)
    assert sr(100, 100, 64, H, True) == pm.step_range(100, 100, 64, H, True)                  # the model's Python function is the same one
    assert sr(2 ** 32 - 1, 2 ** 32 - 1, 0, 1, True) == (0, 2) and sr(2 ** 32 - 1, 1, 0, 1, True) == (2 ** 27 - 1, 2 ** 27)   # no 32-bit wrap
    assert handle.mfa_attention_mla_prefill_step_range(10, 10, 0, 0, 1, ctypes.byref(f), ctypes.byref(e)) == INVALID
    assert handle.mfa_last_error_string() == b"heads must be non-zero"
    assert handle.mfa_attention_mla_prefill_step_range(10, 10, 0, 1, 1, None, ctypes.byref(e)) == INVALID


def outcome(op, q, kv, o, l, kw):
    try:
        op.dispatch(q, kv, o, l, **kw)
    except MFAError as e:
        return e.status, str(e).split(": ", 1)[1]
    return 0, ""


def test_every_refusal_names_its_requirement():
    handle = _abi.lib()
    assert handle.mfa_attention_mla_prefill_launch(Q, KV, O, L, None, None) == INVALID and handle.mfa_last_error_string() == b"null argument"
    out = ctypes.create_string_buffer(64)
    assert handle.mfa_attention_mla_prefill_launch_form(None, out, 64) == INVALID and handle.mfa_last_error_string() == b"null argument"
    bf = AttentionMLAPrefill(P.BF16)
    cases = {
        "widths (512, 512)": (AttentionMLAPrefill(P.BF16, headDimension=512), shape(), UNSUPPORTED, "(576, 512), not (512, 512)"),
        "widths (576, 256)": (AttentionMLAPrefill(P.BF16, valueDimension=256), shape(), UNSUPPORTED, "(576, 512), not (576, 256)"),
        "widths (192, 128)": (AttentionMLAPrefill(P.BF16, headDimension=192, valueDimension=128), shape(), UNSUPPORTED, "(576, 512), not (192, 128)"),
        "fp32 Q": (AttentionMLAPrefill(P.FP32), shape(), UNSUPPORTED, "an FP32 cache has no kernel"),
        "a bf16 output beside f16 inputs": (AttentionMLAPrefill(P.FP16, P.BF16), shape(), INVALID, "outputPrecision must be the inputs' 16-bit type or MFA_FP32"),
        "scale 0": (bf, shape(scale=0.0), INVALID, "scale is required"),
        "scale below 0": (bf, shape(scale=-0.1), INVALID, "scale is required"),
        "scale inf": (bf, shape(scale=float("inf")), INVALID, "scale is required"),
        "scale nan": (bf, shape(scale=float("nan")), INVALID, "scale is required"),
        "zero rows": (bf, shape(rows=0), INVALID, "rows, column, heads and batches must be non-zero"),
        "zero heads": (bf, shape(heads=0), INVALID, "rows, column, heads and batches must be non-zero"),
        "null cacheLengths": (bf, shape(cacheLengths=None), INVALID, "cacheLengths is required"),
        "page size 8": (bf, shape(pageSize=8, blockTable=TABLE, blockTableStride=512), INVALID, "pageSize must be a power of two from 16 to 1024"),
        "page size 48": (bf, shape(pageSize=48, blockTable=TABLE, blockTableStride=512), INVALID, "pageSize must be a power of two from 16 to 1024"),
        "page size 2048": (bf, shape(pageSize=2048, blockTable=TABLE, blockTableStride=512), INVALID, "pageSize must be a power of two from 16 to 1024"),
        "paged without a table": (bf, shape(pageSize=16), INVALID, "needs blockTable"),
        "a short table row": (bf, shape(pageSize=16, blockTable=TABLE, blockTableStride=255), INVALID, "blockTableStride must hold the 256 pages"),
        "a cache row stride off 8 elements": (bf, shape(strides=dict(KV=(580, 0, 4096 * 580))), INVALID, "strides of KV must be multiples of 8 elements"),
        "a cache row below 576": (bf, shape(strides=dict(KV=(512, 0, 4096 * 512))), INVALID, "leadingDimension of KV is smaller than the head dimension"),
        "a page stride off 8 elements": (bf, shape(pageSize=16, blockTable=TABLE, blockTableStride=256, pageStride=16 * 576 + 4), INVALID,
                                         "strides of KV must be multiples of 8 elements"),
        "a Q head stride off 8 elements": (bf, shape(strides=dict(Q=(576, 580, 16 * 200 * 580))), INVALID, "strides of Q must be multiples of 8 elements"),
        "an O row stride off 4 elements": (bf, shape(strides=dict(O=(514, 200 * 514, 16 * 200 * 514))), INVALID, "strides of O must be multiples of 4 elements"),
        "an O row below 512": (bf, shape(strides=dict(O=(256, 200 * 256, 16 * 200 * 256))), INVALID, "leadingDimension of O is smaller than the head dimension"),
        "rows x heads past the grid": (bf, shape(rows=2 ** 25, heads=128), INVALID, "must fit a grid of 2^31 - 1 workgroups"),
    }
    for name, (op, kw, status, needle) in cases.items():
        got = outcome(op, Q, KV, O, L, kw)
        assert got[0] == status and needle in got[1], (name, got)
    # the buffers: null or misaligned, after everything else
    for q, kv, o, l, needle in ((None, KV, O, L, "null argument"), (Q, None, O, L, "null argument"), (Q, KV, None, L, "null argument"),
                                (Q + 8, KV, O, L, "Q, KV and O must be 16-byte aligned"), (Q, KV + 8, O, L, "Q, KV and O must be 16-byte aligned"),
                                (Q, KV, O + 4, L, "Q, KV and O must be 16-byte aligned"), (Q, KV, O, L + 2, "L must be 4-byte aligned")):
        got = outcome(bf, q, kv, o, l, shape())
        assert got[0] == INVALID and needle in got[1], got
    # mfa_mla.h's own words where the requirement is the same
    dec = AttentionMLADecode(P.BF16)
    small = dict(rows=1, column=4096, heads=16, batches=2, scale=SCALE, cacheLengths=LENGTHS)
    for over in (dict(cacheLengths=None), dict(pageSize=48, blockTable=TABLE, blockTableStride=512), dict(scale=0.0), dict(heads=0),
                 dict(pageSize=16), dict(strides=dict(KV=(580, 0, 4096 * 580)))):
        mine, theirs = outcome(bf, Q, KV, O, L, shape(**over)), outcome(dec, Q, KV, O, L, dict(small, **over))
        assert mine == theirs and mine[0] != 0, (over, mine, theirs)
    # timing arguments
    ms = ctypes.c_float(0)
    p, _keep = bf._params(**shape())
    assert handle.mfa_attention_mla_prefill_time(Q, KV, O, L, ctypes.byref(p), None, 0, 0, ctypes.byref(ms)) == INVALID
    assert handle.mfa_last_error_string() == b"bad timing arguments"


def test_decode_still_refuses_33_rows_in_its_present_words():
    got = outcome(AttentionMLADecode(P.BF16), Q, KV, O, L, dict(rows=33, column=4096, heads=16, batches=2, scale=SCALE, cacheLengths=LENGTHS))
    assert got == (UNSUPPORTED, "MLA decode takes at most 32 rows per sequence, not 33: a longer block of query rows is a prefill, which is not "
                                "served over the latent cache"), got
    assert "attn_mla16p" not in AttentionMLADecode(P.BF16).launchForm(rows=32, column=4096, heads=16, batches=2, scale=SCALE, cacheLengths=LENGTHS)
