"""CPU test (no GPU call): the host side of prefill cut along the keys, include/mfa_split.h -- exported symbols and the ctypes mirror,
the piece function against a brute-force partition of every row block's own tile list, the workspace formula and the planned piece
count against the rule as the header states it, the launch-form texts of split, forced and unsplit-without-workspace launches for every
head dimension, type, cache and with a tree, every refusal by status and message, and the torch binding's routes on fake tensors."""
import ctypes
import inspect
import itertools
import os
import re

import pytest

from metal_flash_attention_amd import AttentionPrefill, GEMMOperandPrecision as P, KVCachePrecision, MFAError, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS, LOGITS, MASKS, STARTS, WS = 0x1000, 0x3000, 0x7000, 0x5000, 0x100000   # any non-null values: the host never reads what they point to
INVALID, UNSUPPORTED = 2, 3
TYPES = ((P.BF16, "bf16"), (P.FP16, "f16"))
DIMS = (64, 128, 256)
TREE = dict(treeMasks=MASKS, treeBatchStride=0)
BIG = 1 << 40


def pshape(**over):
    kw = dict(rows=16, column=32768, heads=64, batches=1, headsPerKeyValue=8, cacheLengths=LENGTHS)
    kw.update(over)
    return kw


def test_header_symbols_exported_and_the_ctypes_mirror():
    header = open(os.path.join(ROOT, "include", "mfa_split.h")).read()
    assert '#include "mfa_tree.h"' in header
    declared = set(re.findall(r"\b(mfa_(?:attention|key)_\w+)\s*\(", header))
    handle = _abi.lib()
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in include/mfa_split.h but not exported"
    assert declared == {s[0] for s in _abi.SPLIT_SYMBOLS}
    assert declared == {"mfa_attention_prefill_split_" + s for s in ("launch", "launch_form", "time", "workspace_size", "piece_range")} | \
        {"mfa_key_split_" + s for s in ("init", "size", "offsets")}
    for name, restype, argtypes in _abi.SPLIT_SYMBOLS:
        fn = getattr(handle, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
        if name.endswith(("_launch", "_launch_form", "_time", "_workspace_size")):   # `split` follows `tree`, which follows `sinks`
            at = argtypes.index(_abi._SPLIT)
            assert argtypes.count(_abi._SPLIT) == 1 and argtypes[at - 1] is _abi._TREE and argtypes[at - 2] is _abi._SINKS
    # the five entries' signatures written out, as include/mfa_split.h declares them: the table that generates four of them is not its own witness
    void, u32, u32p = ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)
    bufs, params = [void] * 5, [ctypes.POINTER(_abi.mfa_prefill_params)]
    own = [u32, ctypes.POINTER(_abi.mfa_attention_sinks), ctypes.POINTER(_abi.mfa_attention_tree), ctypes.POINTER(_abi.mfa_key_split)]
    pair = ctypes.POINTER(ctypes.c_uint32 * 2)
    written_out = {
        "launch": bufs + params + own + [void],
        "launch_form": params + own + [ctypes.c_char_p, ctypes.c_size_t],
        "time": bufs + params + own + [void, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)],
        "workspace_size": params + own + [ctypes.POINTER(ctypes.c_uint64), u32p],
        "piece_range": [u32] * 5 + [pair, pair],
    }
    for verb, argtypes in written_out.items():
        fn = getattr(handle, "mfa_attention_prefill_split_" + verb)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == argtypes, verb
    assert int(handle.mfa_abi_version()) == 6   # mfa.h did not change
    for name in ("MAX_PIECES", "MIN_TILES", "COMPUTE_UNITS"):
        assert getattr(_abi, "MFA_PREFILL_SPLIT_" + name) == int(re.search(r"#define MFA_PREFILL_SPLIT_%s (\d+)u" % name, header).group(1))
    prefill = open(os.path.join(ROOT, "include", "mfa_prefill.h")).read()
    assert "mfa_split.h" in prefill and "mfa_prefill_params" in prefill
    assert handle.mfa_prefill_params_size() == ctypes.sizeof(_abi.mfa_prefill_params)   # the params did not change


def test_the_struct_mirror_matches():
    handle = _abi.lib()
    assert handle.mfa_key_split_size() == ctypes.sizeof(_abi.mfa_key_split) == 24
    offsets, count = (ctypes.c_uint32 * 8)(), ctypes.c_uint32(0)
    assert handle.mfa_key_split_offsets(offsets, 8, ctypes.byref(count)) == 0
    mirror = [getattr(_abi.mfa_key_split, name).offset for name, _t in _abi.mfa_key_split._fields_]
    assert count.value == len(mirror) == 4 and list(offsets[:4]) == mirror
    assert [name for name, _t in _abi.mfa_key_split._fields_] == ["workspace", "workspaceBytes", "pieces", "reserved"]
    block = _abi.mfa_key_split(workspace=1, workspaceBytes=2, pieces=3, reserved=4)
    handle.mfa_key_split_init(ctypes.byref(block))
    assert (block.workspace, block.workspaceBytes, block.pieces, block.reserved) == (None, 0, 0, 0)


def walked(five):
    begin, _u0, _u1, end, sink_end = five
    return list(range(sink_end)) + list(range(begin, end))


def test_the_piece_range_against_a_brute_force_partition():
    """the pieces of a block hold every tile of [0, sinkEnd) ++ [begin, end) -- the five indices from the EXISTING tile-range functions --
    exactly once, in order, with sizes that differ by at most one"""
    lists = set()
    for n in (0, 1, 63, 64, 65, 200, 1100):
        for qn in (1, 37, 70, 200):
            for W in (0, 1, 65, 130):
                for S in (0, 4, 70):
                    if S and not W:
                        continue   # (sink tokens need a window: refused by the range functions)
                    for causal in (True, False):
                        if W and not causal:
                            continue   # (a window needs causal)
                        for RB in (16, 32, 128):
                            for r0 in range(0, qn, RB):
                                lists.add(AttentionPrefill.sinkTileRange(n, qn, r0, RB, W, S, causal=causal))
                    if qn <= 64 and (W == 0 or W >= qn):
                        lists.add(AttentionPrefill.treeTileRange(n, qn, W, S))
    assert len(lists) > 60 and any(five[4] and five[3] > five[0] > five[4] for five in lists)   # sink tiles, a gap, window tiles
    for five in lists:
        want = walked(five)
        for pieces in (1, 2, 3, 8, 64):
            got, sizes = [], []
            for piece in range(pieces):
                (b0, e0), (b1, e1) = AttentionPrefill.pieceRange(five[0], five[3], five[4], pieces, piece)
                assert 0 <= b0 <= e0 <= five[4] and five[0] <= b1 <= e1 <= five[3], (five, pieces, piece)
                assert e0 == b0 or b1 == e1 or (e0 == five[4] and b1 == five[0]), (five, pieces, piece)   # a piece crosses the seam in list order only
                got += list(range(b0, e0)) + list(range(b1, e1))
                sizes.append(e0 - b0 + e1 - b1)
            assert got == want, (five, pieces)
            assert max(sizes) - min(sizes) <= 1 and sum(sizes) == len(want), (five, pieces, sizes)
    with pytest.raises(MFAError, match="piece must be below pieces"):
        AttentionPrefill.pieceRange(0, 4, 0, 3, 3)
    with pytest.raises(MFAError, match="sinkEnd <= beginTile <= endTile"):
        AttentionPrefill.pieceRange(1, 4, 2, 3, 0)


def planned_by_the_rule(batches, kv_heads, rows, column, D, G, window=0, sinks=0):
    """include/mfa_split.h: min(target / blocks, tiles / MIN_TILES, MAX_PIECES), below 2: 1"""
    blocks = batches * kv_heads * -(-rows // (128 // G))
    tiles = -(-column // 64)
    if window:
        tiles = min(tiles, -(-(window + rows - 1) // 64) + 1 + -(-sinks // 64))
    target = _abi.MFA_PREFILL_SPLIT_COMPUTE_UNITS * (1 if D == 256 else 2)
    if blocks >= target:
        return 1
    count = min(target // blocks, tiles // _abi.MFA_PREFILL_SPLIT_MIN_TILES, _abi.MFA_PREFILL_SPLIT_MAX_PIECES)
    return count if count >= 2 else 1


PLANS = [  # (batches, K/V heads, rows, column, D, G, window, sink tokens) -> pieces
    ((1, 8, 16, 32768, 128, 8, 0, 0), 64), ((1, 8, 64, 32768, 128, 8, 0, 0), 16), ((1, 8, 128, 32768, 128, 8, 0, 0), 8),
    ((1, 8, 512, 32768, 128, 8, 0, 0), 2), ((4, 8, 16, 4096, 128, 8, 0, 0), 8), ((4, 8, 512, 131072, 128, 8, 0, 0), 1),
    ((1, 8, 16, 32768, 256, 8, 0, 0), 32), ((1, 8, 16, 32768, 64, 8, 0, 0), 64), ((1, 8, 16, 1024, 128, 8, 0, 0), 2),
    ((1, 8, 16, 960, 128, 8, 0, 0), 1), ((1, 8, 16, 131072, 128, 8, 4096, 0), 8), ((1, 8, 16, 131072, 128, 8, 4096, 130), 8),
    ((3, 2, 70, 1152, 128, 4, 0, 0), 2), ((1, 1, 1, 1 << 20, 128, 1, 0, 0), 64),
]


@pytest.mark.parametrize("plan", PLANS)
def test_the_workspace_formula_and_the_planned_piece_count(plan):
    (batches, kv, rows, column, D, G, W, S), pieces = plan
    assert planned_by_the_rule(batches, kv, rows, column, D, G, W, S) == pieces
    pre = AttentionPrefill(D, P.BF16)
    kw = dict(rows=rows, column=column, heads=kv * G, batches=batches, headsPerKeyValue=G, cacheLengths=LENGTHS)
    if W:
        kw.update(window=W, sinkTokens=S)
    per = batches * kv * G * rows * (D + 2) * 4
    assert pre.plannedSplit(**kw) == (per * pieces if pieces > 1 else 0, pieces)
    assert pre.workspaceSize(**kw) == (per * pieces if pieces > 1 else 0)
    assert pre.workspaceSize(pieces=1, **kw) == 0 and pre.plannedSplit(pieces=1, **kw) == (0, 1)
    assert pre.plannedSplit(pieces=5, **kw) == (per * 5, 5)                                           # forced: as given
    assert pre.plannedSplit(pieces=0, workspace=WS, workspaceBytes=1, **kw) == pre.plannedSplit(**kw)   # a bound workspace is not looked at


def test_launch_forms():
    for D in DIMS:
        for prec, tn in TYPES:
            for fp8 in (False, True):
                pre = AttentionPrefill(D, prec, cachePrecision=KVCachePrecision.E4M3 if fp8 else None)
                tail8 = "_e4m3" if fp8 else ""
                for tree in (False, True):
                    opts = dict(TREE) if tree else {}
                    kw = pshape(**opts)
                    planned = 32 if D == 256 else 64
                    said = ", tree masks shared" if tree else ""
                    unsplit = pre.launchForm(**(dict(window=0, sinkTokens=0, sinkLogits=None, **kw) if tree else kw))
                    assert unsplit.startswith("attn_prefill16%s_d%d_%s%s (grid 8 = " % ("t" if tree else "", D, tn, tail8)), unsplit
                    body = "1 sequences x 8 K/V heads x 1 row blocks of 16 rows x 8 heads"
                    name = "attn_prefill16%sk_d%d_%s%s" % ("t" if tree else "s", D, tn, tail8)
                    combine = " + attn_prefill16_combine_d%d_%s (grid 256)" % (D, tn)
                    assert pre.launchForm(workspace=WS, workspaceBytes=BIG, **kw) == \
                        "%s (grid %d = %s x %d pieces, contiguous%s)%s" % (name, 8 * planned, body, planned, said, combine)
                    assert pre.launchForm(pieces=3, workspace=WS, workspaceBytes=BIG, **kw) == \
                        "%s (grid 24 = %s x 3 pieces as given, contiguous%s)%s" % (name, body, said, combine)
                    assert pre.launchForm(pieces=0, **kw) == unsplit[:-1] + ", unsplit without a workspace: the plan has %d pieces)" % planned
                    assert pre.launchForm(pieces=3, **kw) == unsplit[:-1] + ", unsplit without a workspace: the plan has 3 pieces)"
                    assert pre.launchForm(pieces=1, workspace=WS, workspaceBytes=BIG, **kw) == unsplit     # one piece: the launch that exists
    pre = AttentionPrefill(128, P.BF16)
    text = pre.launchForm(pieces=2, workspace=WS, workspaceBytes=BIG, window=130, sinkTokens=4, sinkLogits=LOGITS, pageSize=16, blockTable=0x9000,
                          blockTableStride=2048, **pshape())
    assert text == ("attn_prefill16sk_d128_bf16 (grid 16 = 1 sequences x 8 K/V heads x 1 row blocks of 16 rows x 8 heads x 2 pieces as given, paged, "
                    "window 130, sink tokens 4, sink logits) + attn_prefill16_combine_d128_bf16 (grid 256)")
    # a launch that gives neither keyword is the launch it always was, whatever else it gives
    assert pre.launchForm(**pshape()) == "attn_prefill16_d128_bf16 (grid 8 = 1 sequences x 8 K/V heads x 1 row blocks of 16 rows x 8 heads, contiguous)"


def outcome(call, *args, **kw):
    try:
        call(*args, **kw)
    except MFAError as e:
        return [e.status, str(e).split(": ", 1)[1]]
    except ValueError as e:
        return ["ValueError", str(e)]
    return [0, ""]


def test_every_refusal_by_status_and_message():
    pre = AttentionPrefill(128, P.BF16)
    bufs = (0x10000, 0x20000, 0x30000, 0x40000, None)
    need = pre.workspaceSize(pieces=3, **pshape())
    assert need == 3 * 64 * 16 * 130 * 4
    cases = {
        "accepted": ((pre.launchForm, dict(pieces=3, workspace=WS, workspaceBytes=need, **pshape())), (0, "")),
        "64 pieces accepted": ((pre.launchForm, dict(pieces=64, workspace=WS, workspaceBytes=BIG, **pshape())), (0, "")),
        "65 pieces": ((pre.launchForm, dict(pieces=65, **pshape())), (INVALID, "mfa_key_split.pieces must be 0 (the host's plan), 1 (unsplit) or 2 .. 64")),
        "65 pieces, size": ((pre.workspaceSize, dict(pieces=65, **pshape())), (INVALID, "not 65")),
        "short workspace": ((pre.launchForm, dict(pieces=3, workspace=WS, workspaceBytes=need - 1, **pshape())),
                            (INVALID, "workspace too small: %d bytes, the launch needs %d (mfa_attention_prefill_split_workspace_size)" % (need - 1, need))),
        "short workspace, launch": ((pre.dispatch, bufs, dict(pieces=3, workspace=WS, workspaceBytes=16, **pshape())), (INVALID, "the launch needs %d" % need)),
        "misaligned workspace": ((pre.time, bufs, dict(pieces=3, workspace=WS + 8, workspaceBytes=need, **pshape())), (INVALID, "workspace must be 16-byte aligned")),
        "a misaligned workspace nobody needs": ((pre.launchForm, dict(pieces=1, workspace=WS + 8, workspaceBytes=0, **pshape())), (0, "")),
        "softcap": ((pre.launchForm, dict(pieces=3, softcap=50.0, **pshape())), ("ValueError", "softcap=")),
        "ragged": ((pre.launchForm, dict(workspace=WS, rowStarts=STARTS, totalRows=100, **pshape())), ("ValueError", "rowStarts=")),
        "a tree of 65 rows": ((pre.launchForm, dict(pieces=3, **TREE, **pshape(rows=65))), (UNSUPPORTED, "at most 64 nodes")),
        "sink tokens without a window": ((pre.launchForm, dict(pieces=3, sinkTokens=4, **pshape())), (INVALID, "sink tokens need a window")),
        "65 pieces and not causal under a window": ((pre.launchForm, dict(pieces=65, window=5, causal=False, **pshape())), (INVALID, "a sliding window needs causal")),
    }
    for name, (c, (status, needle)) in cases.items():
        got = outcome(c[0], *(c[1] if len(c) == 3 else ()), **c[-1])
        assert got[0] == status and needle in got[1], (name, got)
    # a NULL split block, through the C entries themselves
    handle = _abi.lib()
    pp, _keep = pre._params(**pshape())
    out, size, count = ctypes.create_string_buffer(512), ctypes.c_uint64(7), ctypes.c_uint32(7)
    for status in (handle.mfa_attention_prefill_split_launch_form(ctypes.byref(pp), 0, None, None, None, out, len(out)),
                   handle.mfa_attention_prefill_split_workspace_size(ctypes.byref(pp), 0, None, None, None, ctypes.byref(size), ctypes.byref(count)),
                   handle.mfa_attention_prefill_split_time(0x10000, 0x20000, 0x30000, 0x40000, None, ctypes.byref(pp), 0, None, None, None, None, 1, 1, None),
                   handle.mfa_attention_prefill_split_launch(0x10000, 0x20000, 0x30000, 0x40000, None, ctypes.byref(pp), 0, None, None, None, None)):
        assert status == INVALID and "null mfa_key_split" in handle.mfa_last_error_string().decode()
    assert size.value == 0 and count.value == 1 and out.value == b""
    # the C entry refuses a cap's and ragged rows' absence by construction: it has no such argument; NULL sinks and a NULL tree are none
    split = _abi.mfa_key_split()
    handle.mfa_key_split_init(ctypes.byref(split))
    assert handle.mfa_attention_prefill_split_launch_form(ctypes.byref(pp), 0, None, None, ctypes.byref(split), out, len(out)) == 0
    assert out.value.decode() == pre.launchForm(pieces=0, **pshape())


def test_every_split_call_reaches_the_split_family_of_the_table():
    """the split block is one more option of attention._route: with any of a window, sinks and a tree it reaches mfa_attention_prefill_split_,
    which is handed window 0 and NULL blocks for what the call leaves out; decode has no such family"""
    from metal_flash_attention_amd import attention as at
    assert at._OPTIONS == ("quant", "window", "sinks", "ragged", "softcap", "tree", "split")
    assert _abi.CACHE_FAMILIES["prefill"]["split_"] == ("window", "sinks", "tree", "split")
    routes = at._routes("prefill")
    assert routes is not at.AttentionPrefill.ROUTES and routes == at.AttentionPrefill.ROUTES
    sinks, tree, split = object(), object(), object()   # (whatever the caller passes by reference goes through as it is)
    for given in itertools.product((False, True), repeat=3):
        w, s, t = (value if g else None for value, g in zip((130, sinks, tree), given))
        entries, own = at._route(routes, None, w, s, None, None, t, split)
        assert entries == "mfa_attention_prefill_split_" and tuple(own) == (130 if given[0] else 0, s, t, split), given
        assert routes[(False, given[0], given[1], False, False, given[2], True)] == (entries, (False, True, True, False, False, True, True))
    assert tuple(at._route(routes, None, 0, None, None, None, None, split)[1]) == (0, None, None, split)   # a window that is given as 0
    assert at._route(routes, None, 130, sinks, None, None, tree)[0] == "mfa_attention_prefill_tree_"      # no split block: the family it always was
    assert not any(given[0] or given[6] for given in routes if given[3] or given[4]) and not any(given[6] for given in at._routes("decode"))
    text = "a key split (workspace= / pieces=) goes with neither %s: a soft cap or ragged rows together with a split have no kernel (include/mfa_split.h)"
    for softcap, ragged, t, said in ((ctypes.c_float(50.0), None, None, "softcap="), (None, object(), None, "rowStarts= / totalRows="),
                                     (ctypes.c_float(50.0), object(), None, "softcap="), (ctypes.c_float(50.0), None, tree, "softcap=")):
        with pytest.raises(ValueError) as refused:
            at._route(routes, None, None, None, ragged, softcap, t, split)
        assert str(refused.value) == text % said
    pre = AttentionPrefill(128, P.BF16)
    for kw, said in ((dict(pieces=3, softcap=50.0), "softcap="), (dict(workspace=WS, rowStarts=STARTS, totalRows=100), "rowStarts= / totalRows="),
                     (dict(pieces=0, softcap=50.0, **TREE), "softcap=")):
        for call in (pre.launchForm, pre.workspaceSize, pre.plannedSplit):
            assert outcome(call, **kw, **pshape()) == ["ValueError", text % said]


# ------------------------------------------------------------------------------------------------ the torch binding, on fake tensors
torch = pytest.importorskip("torch")


def _operands():
    q = torch.empty((2, 8, 40, 64), dtype=torch.bfloat16, device="cuda")
    k16 = torch.empty((2, 2, 1024, 64), dtype=torch.bfloat16, device="cuda")
    k8 = torch.empty((2, 2, 1024, 64), dtype=torch.float8_e4m3fn, device="cuda")
    lens = torch.empty((2,), dtype=torch.int32, device="cuda")
    scale = torch.empty((2,), dtype=torch.float32, device="cuda")
    logits = torch.empty((8,), dtype=torch.float32, device="cuda")
    shared = torch.empty((40,), dtype=torch.int64, device="cuda")
    return q, k16, k8, lens, scale, logits, shared


def test_the_fake_tensor_routes(monkeypatch):
    from torch._subclasses.fake_tensor import FakeTensorMode

    from metal_flash_attention_amd import torch_binding as tb
    if not tb._HAVE_SPLIT_OP:
        pytest.skip("this torch has no torch.library.custom_op")
    schema = str(torch.ops.mfa.attention_prefill_split.default._schema)
    assert re.search(r"Tensor\? sink_logits, Tensor\? tree, (Sym)?[Ii]nt key_pieces\) -> \(Tensor, Tensor\)$", schema.rstrip()), schema
    for name, _impl, _fake, _mutates in tb._CACHE_OPS:
        if name != "attention_prefill_split":
            assert "key_pieces" not in str(getattr(torch.ops.mfa, name).default._schema), name
    assert "key_pieces" in inspect.signature(tb.flash_prefill).parameters
    assert "key_pieces" not in inspect.signature(tb.flash_prefill_ragged).parameters and "key_pieces" not in inspect.signature(tb.flash_decode).parameters
    calls = []
    real = tb._call_op

    def spy(have, name, *args):
        calls.append((name, args))
        return real(have, name, *args)

    monkeypatch.setattr(tb, "_call_op", spy)
    with FakeTensorMode():
        q, k16, k8, lens, scale, logits, shared = _operands()
        # None: today's ops with today's arguments
        for kw, op, own in ((dict(), "attention_prefill", 0), (dict(window=130), "attention_prefill_window", 1),
                            (dict(window=130, sink_tokens=4, sink_logits=logits), "attention_prefill_sink", 3), (dict(tree_mask=shared), "attention_prefill_tree", 4),
                            (dict(softcap=30.0), "attention_prefill_softcap", 4)):
            del calls[:]
            with_none = tb.flash_prefill(q, k16, k16, lens, key_pieces=None, **kw)
            (first,) = list(calls)
            del calls[:]
            without = tb.flash_prefill(q, k16, k16, lens, **kw)
            assert first[0] == calls[0][0] == op and len(first[1]) == len(calls[0][1]) == 9 + own and with_none.shape == without.shape
        # 0 and 3: the split op, the window, sinks and tree in its spelling, the pieces last
        for pieces in (0, 3, 64, 1):
            del calls[:]
            o, lse = tb.flash_prefill(q, k8, k8, lens, lens, k_scale=scale, v_scale=scale, window=130, sink_tokens=4, sink_logits=logits, tree_mask=shared,
                                      key_pieces=pieces, return_lse=True)
            ((name, args),) = calls
            assert name == "attention_prefill_split" and args[9:12] == (130, 4, logits) and args[12] is shared and args[13] == pieces
            assert o.shape == (2, 8, 40, 64) and o.dtype == torch.bfloat16 and lse.shape == (2, 8, 40) and lse.dtype == torch.float32
        del calls[:]
        tb.flash_prefill(q, k16, k16, lens, key_pieces=0)
        assert calls[0][0] == "attention_prefill_split" and calls[0][1][9:] == (0, 0, None, None, 0)
        with pytest.raises(ValueError, match="key_pieces and softcap together have no kernel"):
            tb.flash_prefill(q, k16, k16, lens, softcap=30.0, key_pieces=0)
        for bad in (65, -1, 2.0, True):
            with pytest.raises(ValueError, match="key_pieces must be an int from 0"):
                tb.flash_prefill(q, k16, k16, lens, key_pieces=bad)
        with pytest.raises(ValueError, match="tree_mask needs causal=True"):   # the other keywords keep their checks beside it
            tb.flash_prefill(q, k16, k16, lens, causal=False, tree_mask=shared, key_pieces=3)
