"""CPU test (no GPU call): the host side of speculation trees over a KV cache, include/mfa_tree.h -- exported symbols and the ctypes
mirror, the tree kernels' names for every head dimension, type and cache, the decode plan (workspace and pieces) as the sink launch's,
every refusal by status and message with the order of two mistakes pinned in tests/golden/tree_refusals.json, and the tile range of a
prefill launch against brute force."""
import ctypes
import json
import os
import re

import pytest

from metal_flash_attention_amd import AttentionDecode, AttentionDecodeFP8, AttentionPrefill, GEMMOperandPrecision as P, KVCachePrecision, MFAError, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tree_refusals.json")
LENGTHS, LOGITS, MASKS, STARTS = 0x1000, 0x3000, 0x7000, 0x5000   # any non-null values: the host never reads what they point to
INVALID, UNSUPPORTED = 2, 3
TYPES = ((P.BF16, "bf16"), (P.FP16, "f16"))
DIMS = (64, 128, 256)
FAMILIES = (dict(), dict(window=0), dict(window=130), dict(window=130, sinkTokens=4), dict(sinkLogits=LOGITS), dict(window=4096, sinkTokens=70, sinkLogits=LOGITS))
TREE = dict(treeMasks=MASKS, treeBatchStride=0)


def dshape(**over):
    kw = dict(rows=4, column=32768, heads=16, batches=2, headsPerKeyValue=8, cacheLengths=LENGTHS)
    kw.update(over)
    return kw


def pshape(**over):
    kw = dict(rows=64, column=4096, heads=64, batches=4, headsPerKeyValue=8, cacheLengths=LENGTHS)
    kw.update(over)
    return kw


def test_header_symbols_exported_and_the_ctypes_mirror():
    header = open(os.path.join(ROOT, "include", "mfa_tree.h")).read()
    assert '#include "mfa_sink.h"' in header
    declared = set(re.findall(r"\b(mfa_attention_\w+)\s*\(", header))
    handle = _abi.lib()
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in include/mfa_tree.h but not exported"
    assert declared == {s[0] for s in _abi.TREE_SYMBOLS}
    assert declared == {"mfa_attention_decode_tree_" + s for s in ("workspace_size", "launch", "launch_form", "time")} | \
        {"mfa_attention_prefill_tree_" + s for s in ("launch", "launch_form", "time", "tile_range")} | \
        {"mfa_attention_tree_" + s for s in ("init", "size", "offsets")}
    for name, restype, argtypes in _abi.TREE_SYMBOLS:
        fn = getattr(handle, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
        if name.endswith(("_launch", "_launch_form", "_time", "_workspace_size")):   # `tree` follows `sinks`
            assert argtypes.count(_abi._TREE) == 1 and argtypes[argtypes.index(_abi._TREE) - 1] is _abi._SINKS
    assert int(handle.mfa_abi_version()) == 6   # mfa.h did not change
    assert _abi.MFA_TREE_MAX_NODES == int(re.search(r"#define MFA_TREE_MAX_NODES (\d+)u", header).group(1)) == 64


def test_the_struct_mirror_matches():
    handle = _abi.lib()
    assert handle.mfa_attention_tree_size() == ctypes.sizeof(_abi.mfa_attention_tree) == 24
    offsets, count = (ctypes.c_uint32 * 8)(), ctypes.c_uint32(0)
    assert handle.mfa_attention_tree_offsets(offsets, 8, ctypes.byref(count)) == 0
    mirror = [getattr(_abi.mfa_attention_tree, name).offset for name, _t in _abi.mfa_attention_tree._fields_]
    assert count.value == len(mirror) == 3 and list(offsets[:3]) == mirror
    assert [name for name, _t in _abi.mfa_attention_tree._fields_] == ["masks", "batchStride", "reserved"]
    block = _abi.mfa_attention_tree(masks=1, batchStride=2, reserved=3)
    handle.mfa_attention_tree_init(ctypes.byref(block))
    assert (block.masks, block.batchStride, block.reserved) == (None, 0, 0)


def test_a_tree_launch_runs_the_tree_family_on_the_sink_launch_s_plan():
    for D in DIMS:
        for prec, tn in TYPES:
            for fam in FAMILIES:
                sink = dict(sinkTokens=0, sinkLogits=None)
                sink.update(fam)
                for fp8 in (False, True):
                    dec = (AttentionDecodeFP8 if fp8 else AttentionDecode)(D, prec)
                    name = "attn_decode%st_d%d_%s" % ("8" if fp8 else "16", D, tn)
                    kw = dshape()
                    need = dec.workspaceSize(**TREE, **fam, **kw)
                    assert need == dec.workspaceSize(**sink, **kw), (D, fam)                  # the sink launch's workspace
                    assert need > 0 or fam.get("window") == 130                               # (a short window plans one piece)
                    for ws in (dict(), dict(workspace=0x100000, workspaceBytes=need)):
                        for tree, said in ((TREE, ", tree masks shared"), (dict(treeMasks=MASKS, treeBatchStride=4), ", tree masks per sequence")):
                            text, want = dec.launchForm(**tree, **ws, **fam, **kw), dec.launchForm(**ws, **sink, **kw)
                            assert text.startswith(name + ("_pieces" if need and ws else "_single") + " ("), text
                            want = re.sub(r"^attn_decode(16|8)[ws]?_d", r"attn_decode\1t_d", want)   # the same pieces, grid and combine kernel
                            if need and ws:
                                assert text == want.replace(") + attn", said + ") + attn") and "_combine (grid" in text, (text, want)
                            elif need:
                                assert text == want.replace(", unsplit without", said + ", unsplit without"), (text, want)
                            else:
                                assert text == want[:-1] + said + ")", (text, want)
                    pre = AttentionPrefill(D, prec, cachePrecision=KVCachePrecision.E4M3 if fp8 else None)
                    text, want = pre.launchForm(**TREE, **fam, **pshape()), pre.launchForm(**sink, **pshape())
                    assert text.startswith("attn_prefill16t_d%d_%s%s (" % (D, tn, "_e4m3" if fp8 else "")), text
                    assert text == re.sub(r"^attn_prefill16[ws]?_d", "attn_prefill16t_d", want)[:-1] + ", tree masks shared)", (text, want)


def outcome(call, *args, **kw):
    try:
        call(*args, **kw)
    except MFAError as e:
        return [e.status, str(e).split(": ", 1)[1]]
    except ValueError as e:
        return ["ValueError", str(e)]
    return [0, ""]


def refusal_cases():
    dec, dec8, pre = AttentionDecode(128, P.BF16), AttentionDecodeFP8(256, P.FP16), AttentionPrefill(64, P.BF16)
    bufs = (0x10000, 0x20000, 0x30000, 0x40000, None)
    cases = {
        "decode accepted": (dec.launchForm, dict(**TREE, **dshape())),
        "decode not causal": (dec.launchForm, dict(causal=False, **TREE, **dshape())),
        "prefill not causal": (pre.launchForm, dict(causal=False, **TREE, **pshape())),
        "decode window below rows": (dec.workspaceSize, dict(window=3, **TREE, **dshape())),
        "decode window of rows accepted": (dec.launchForm, dict(window=4, **TREE, **dshape())),
        "prefill window below rows": (pre.launchForm, dict(window=63, sinkTokens=4, **TREE, **pshape())),
        "prefill window of rows accepted": (pre.launchForm, dict(window=64, sinkTokens=70, **TREE, **pshape())),
        "prefill 65 rows": (pre.launchForm, dict(**TREE, **pshape(rows=65))),
        "prefill 64 rows accepted": (pre.launchForm, dict(**TREE, **pshape(rows=64))),
        "decode 33 packed rows": (dec.launchForm, dict(**TREE, **dshape(rows=5))),
        "decode null masks": (dec8.launchForm, dict(treeBatchStride=0, **dshape())),
        "prefill null masks": (pre.dispatch, bufs, dict(treeBatchStride=64, **pshape())),
        "decode misaligned masks": (dec.dispatch, bufs, dict(treeMasks=MASKS + 4, **dshape())),
        "prefill misaligned masks": (pre.time, bufs, dict(treeMasks=MASKS + 1, **pshape())),
        "prefill stride below rows": (pre.launchForm, dict(treeMasks=MASKS, treeBatchStride=63, **pshape())),
        "decode softcap with a tree": (dec.launchForm, dict(softcap=50.0, **TREE, **dshape())),
        "prefill softcap with a tree": (pre.launchForm, dict(softcap=50.0, **TREE, **pshape())),
        "prefill ragged with a tree": (pre.launchForm, dict(rowStarts=STARTS, totalRows=100, **TREE, **pshape())),
        # two mistakes: which one is reported
        "not causal and a small window": (dec.launchForm, dict(causal=False, window=3, **TREE, **dshape())),
        "sink tokens without a window, not causal": (pre.launchForm, dict(causal=False, sinkTokens=4, **TREE, **pshape())),
        "not causal and null masks": (pre.launchForm, dict(causal=False, treeBatchStride=0, **pshape())),
        "small window and 65 rows": (pre.launchForm, dict(window=10, **TREE, **pshape(rows=65))),
        "65 rows and null masks": (pre.launchForm, dict(treeBatchStride=0, **pshape(rows=65))),
        "null masks and an fp32 query": (AttentionPrefill(64, P.FP32).launchForm, dict(treeBatchStride=0, **pshape())),
        "misaligned masks and head dimension 96": (AttentionDecode(96, P.BF16).launchForm, dict(treeMasks=MASKS + 4, **dshape())),
        "small window and a small workspace": (dec.launchForm, dict(window=3, workspace=0x100000, workspaceBytes=16, **TREE, **dshape())),
        "a tree and a small workspace": (dec.launchForm, dict(workspace=0x100000, workspaceBytes=16, **TREE, **dshape())),
        "a tree and a null Q": (dec.dispatch, (None, 0x20000, 0x30000, 0x40000, None), dict(treeMasks=MASKS + 4, **dshape())),
    }
    return {name: outcome(c[0], *(c[1] if len(c) == 3 else ()), **c[-1]) for name, c in cases.items()}


def test_every_refusal_by_status_and_message_in_the_pinned_order():
    got = refusal_cases()
    want = {  # (status, what the message names)
        "decode not causal": (INVALID, "a speculation tree needs causal"), "prefill not causal": (INVALID, "a speculation tree needs causal"),
        "decode window below rows": (INVALID, "window = 3 < rows = 4"), "prefill window below rows": (INVALID, "window = 63 < rows = 64"),
        "prefill 65 rows": (UNSUPPORTED, "at most 64 nodes"), "decode 33 packed rows": (UNSUPPORTED, "at most 32"),
        "decode null masks": (INVALID, "mfa_attention_tree.masks is required"), "prefill null masks": (INVALID, "mfa_attention_tree.masks is required"),
        "decode misaligned masks": (INVALID, "masks must be 8-byte aligned"), "prefill misaligned masks": (INVALID, "masks must be 8-byte aligned"),
        "prefill stride below rows": (INVALID, "batchStride must be 0"),
        "decode softcap with a tree": ("ValueError", "softcap="), "prefill softcap with a tree": ("ValueError", "softcap="),
        "prefill ragged with a tree": ("ValueError", "rowStarts="),
        "not causal and a small window": (INVALID, "a sliding window needs causal"),
        "sink tokens without a window, not causal": (INVALID, "sink tokens need a window"),
        "not causal and null masks": (INVALID, "a speculation tree needs causal"),
        "small window and 65 rows": (INVALID, "window = 10 < rows = 65"), "65 rows and null masks": (UNSUPPORTED, "at most 64 nodes"),
        "null masks and an fp32 query": (INVALID, "mfa_attention_tree.masks is required"),
        "misaligned masks and head dimension 96": (INVALID, "masks must be 8-byte aligned"),
        "small window and a small workspace": (INVALID, "window = 3 < rows = 4"), "a tree and a small workspace": (INVALID, "workspace too small"),
        "a tree and a null Q": (INVALID, "masks must be 8-byte aligned"),
    }
    for name, (status, needle) in want.items():
        assert got[name][0] == status and needle in got[name][1], (name, got[name])
    for name in got:
        assert name in want or got[name] == [0, ""], (name, got[name])
    assert got == json.load(open(GOLDEN)), "the refusals' statuses, words or order moved: tests/golden/tree_refusals.json"


def test_a_null_tree_block_is_refused_and_a_null_sinks_block_is_not():
    handle = _abi.lib()
    dec, pre = AttentionDecode(256, P.BF16), AttentionPrefill(256, P.BF16)
    p, _keep = dec._params(**dshape())
    pp, _keep = pre._params(**pshape())
    out, size = ctypes.create_string_buffer(512), ctypes.c_uint64(7)
    tree = _abi.mfa_attention_tree()
    handle.mfa_attention_tree_init(ctypes.byref(tree))
    tree.masks = MASKS
    assert handle.mfa_attention_decode_tree_launch_form(ctypes.byref(p), None, 0, None, ctypes.byref(tree), out, len(out)) == 0
    assert out.value.decode() == dec.launchForm(**TREE, **dshape()) and out.value.startswith(b"attn_decode16t_d256_bf16_single ")
    assert handle.mfa_attention_prefill_tree_launch_form(ctypes.byref(pp), 130, None, ctypes.byref(tree), out, len(out)) == 0
    assert out.value.startswith(b"attn_prefill16t_d256_bf16 ") and out.value.endswith(b", window 130, tree masks shared)")
    for status in (handle.mfa_attention_decode_tree_launch_form(ctypes.byref(p), None, 0, None, None, out, len(out)),
                   handle.mfa_attention_decode_tree_workspace_size(ctypes.byref(p), None, 0, None, None, ctypes.byref(size)),
                   handle.mfa_attention_prefill_tree_launch_form(ctypes.byref(pp), 0, None, None, out, len(out)),
                   handle.mfa_attention_prefill_tree_launch(0x10000, 0x20000, 0x30000, 0x40000, None, ctypes.byref(pp), 0, None, None, None)):
        assert status == INVALID and "null mfa_attention_tree" in handle.mfa_last_error_string().decode()
    assert size.value == 0 and out.value == b""


def brute(n, qn, W, S):
    """(every key some row can see under some mask, the prefix keys inside EVERY row's window)"""
    P, live = max(n - qn, 0), min(qn, n)
    lo = lambda d: (max(P + d, W) - W) if W else 0   # noqa: E731
    some = set(range(P, n)) | set(range(min(S, P)))
    for d in range(1, live + 1):
        some |= set(range(min(lo(d), P), P))
    every = set(range(P))
    for d in range(1, live + 1):
        every &= set(range(min(lo(d), P), P))
    return some, every


def test_the_tile_range_against_brute_force():
    for n in (0, 1, 63, 64, 65, 127, 128, 191, 700):
        for qn in (1, 5, 33, 64):
            for W in (0, 64, 130):
                for S in (0, 4, 70):
                    if S and not W:   # (sink tokens need a window: refused)
                        with pytest.raises(MFAError):
                            AttentionPrefill.treeTileRange(n, qn, W, S)
                        continue
                    begin, u0, u1, end, sink_end = AttentionPrefill.treeTileRange(n, qn, W, S)
                    tag = (n, qn, W, S, (begin, u0, u1, end, sink_end))
                    if n == 0:
                        assert (begin, u0, u1, end, sink_end) == (0, 0, 0, 0, 0), tag
                        continue
                    some, every = brute(n, qn, W, S)
                    walked = set(range(0, sink_end * 64)) | set(range(begin * 64, end * 64))
                    assert some <= walked, tag                                                    # every visible key lies in a walked tile
                    assert set(range(u0 * 64, u1 * 64)) <= every, tag                             # an unmasked tile: prefix keys every row sees
                    assert sink_end <= begin <= u0 <= u1 <= end and end == -(-n // 64), tag
                    P = max(n - qn, 0)
                    assert u1 <= P // 64 and not (u1 * 64 <= P < (u1 + 1) * 64 and u1 > P // 64), tag   # key P is a tree key: its tile is masked
                    # tight: the first tile holds a key some row sees, and the tile below unmaskedBegin / at unmaskedEnd is not all-visible
                    assert any(c in some for c in range(begin * 64, begin * 64 + 64)), tag
                    if u0 < u1:
                        assert not set(range((u0 - 1) * 64, u0 * 64)) <= every or u0 == 0, tag
                        assert not set(range(u1 * 64, u1 * 64 + 64)) <= every, tag
