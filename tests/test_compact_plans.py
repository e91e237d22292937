"""CPU test (no GPU call): the host side of the KV-cache compaction, include/mfa_compact.h -- exported symbols and the ctypes mirror with
sizeof and every offset, the ABI version, every refusal by status and message with the order of two mistakes pinned in
tests/golden/compact_refusals.json, tree_path on a chain, a forest and a tree whose children have smaller indices than their parents, and
the torch op's schema and fake implementation."""
import ctypes
import json
import os
import re

import pytest

from metal_flash_attention_amd import GEMMOperandPrecision as P, KVCacheCompact, KVCachePrecision, MFAError, _abi
import metal_flash_attention_amd as mfa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "compact_refusals.json")
LENGTHS, ACCEPTED, COUNTS, NEW, TABLE, K, V = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x10000, 0x20000   # the host never reads what they point to
INVALID, UNSUPPORTED = 2, 3


def test_header_symbols_exported_and_the_ctypes_mirror():
    header = open(os.path.join(ROOT, "include", "mfa_compact.h")).read()
    assert '#include "mfa_tree.h"' in header
    declared = set(re.findall(r"\b(mfa_kv_\w+)\s*\(", header.split("#ifndef MFA_COMPACT_H")[1]))
    handle = _abi.lib()
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in include/mfa_compact.h but not exported"
    assert declared == {s[0] for s in _abi.COMPACT_SYMBOLS}
    assert declared == {"mfa_kv_compact_params_" + s for s in ("init", "size", "offsets")} | {"mfa_kv_cache_compact_launch"}
    for name, restype, argtypes in _abi.COMPACT_SYMBOLS:
        fn = getattr(handle, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert int(handle.mfa_abi_version()) == 6 == _abi.EXPECTED_ABI   # mfa.h did not change
    assert "MFA_ABI_VERSION 6" in open(os.path.join(ROOT, "include", "mfa.h")).read()
    assert mfa.KVCacheCompact is KVCacheCompact and "KVCacheCompact" in dir(mfa)


def test_the_struct_mirror_matches():
    handle = _abi.lib()
    mirror = _abi.mfa_kv_compact_params
    assert handle.mfa_kv_compact_params_size() == ctypes.sizeof(mirror) == 160
    offsets, count = (ctypes.c_uint32 * 32)(), ctypes.c_uint32(0)
    assert handle.mfa_kv_compact_params_offsets(offsets, 32, ctypes.byref(count)) == 0
    want = [getattr(mirror, name).offset for name, _t in mirror._fields_]
    assert count.value == len(want) == 22 and list(offsets[:22]) == want
    assert [name for name, _t in mirror._fields_] == [
        "rows", "heads", "batches", "column", "headDimension", "cachePrecision", "reserved", "pageSize", "cacheLengths", "queryLengths",
        "blockTable", "blockTableStride", "accepted", "acceptedStride", "acceptedCounts", "maxAccepted", "reserved2", "newLengths",
        "leadingDimension", "headStride", "batchStride", "pageStride"]
    few, count = (ctypes.c_uint32 * 2)(7, 7), ctypes.c_uint32(0)                    # a small capacity: the count is still said
    assert handle.mfa_kv_compact_params_offsets(few, 2, ctypes.byref(count)) == 0 and count.value == 22 and list(few) == want[:2]
    assert handle.mfa_kv_compact_params_offsets(None, 2, ctypes.byref(count)) == INVALID
    block = mirror(rows=5, cachePrecision=1, maxAccepted=9, newLengths=8)
    handle.mfa_kv_compact_params_init(ctypes.byref(block))
    assert (block.rows, block.cachePrecision, block.maxAccepted, block.newLengths, block.pageSize) == (0, int(P.BF16), 0, None, 0)


def test_the_host_class_fills_the_block():
    p = KVCacheCompact(128, KVCachePrecision.E4M3)._params(rows=12, heads=2, batches=3, column=256, cacheLengths=LENGTHS, accepted=ACCEPTED,
                                                           acceptedCounts=COUNTS, newLengths=NEW, queryLengths=0x6000)
    assert (p.rows, p.heads, p.batches, p.column, p.headDimension, p.cachePrecision, p.pageSize) == (12, 2, 3, 256, 128, 16, 0)
    assert (p.cacheLengths, p.queryLengths, p.accepted, p.acceptedCounts, p.newLengths) == (LENGTHS, 0x6000, ACCEPTED, COUNTS, NEW)
    assert (p.maxAccepted, p.acceptedStride) == (12, 12)                             # left out: the tree's rows, packed
    assert list(p.leadingDimension) == [128, 128] and list(p.headStride) == [256 * 128] * 2 and list(p.batchStride) == [2 * 256 * 128] * 2
    p = KVCacheCompact(64)._params(rows=4, heads=2, batches=3, cacheLengths=LENGTHS, accepted=ACCEPTED, acceptedCounts=COUNTS, maxAccepted=3,
                                   acceptedStride=8, pageSize=16, blockTable=TABLE, blockTableStride=9, pageStrides=(4096, 8192),
                                   strides=dict(kCache=(128, 64, 0)))
    assert (p.cachePrecision, p.maxAccepted, p.acceptedStride, p.pageSize, p.blockTable, p.blockTableStride) == (int(P.BF16), 3, 8, 16, TABLE, 9)
    assert list(p.pageStride) == [4096, 8192] and (p.leadingDimension[0], p.headStride[0]) == (128, 64)
    assert (p.leadingDimension[1], p.headStride[1]) == (64, 16 * 64) and p.newLengths is None


def shape(**over):
    kw = dict(rows=12, heads=2, batches=3, column=256, cacheLengths=LENGTHS, accepted=ACCEPTED, acceptedCounts=COUNTS, newLengths=NEW)
    kw.update(over)
    return kw


def paged(**over):
    kw = dict(column=0, pageSize=16, blockTable=TABLE, blockTableStride=16, pageStrides=(2 * 16 * 128, 2 * 16 * 128))
    kw.update(over)
    return shape(**kw)


def outcome(op, k, v, kw):
    try:
        op.dispatch(k, v, **kw)
    except MFAError as e:
        return [e.status, str(e).split(": ", 1)[1]]
    return [0, ""]


def refusal_cases():
    """every case is refused before any GPU call: the pointers are made up"""
    c16, c8, e5, f32 = KVCacheCompact(128, P.BF16), KVCacheCompact(128, KVCachePrecision.E4M3), KVCacheCompact(128, KVCachePrecision.E5M2), KVCacheCompact(128, P.FP32)
    cases = {
        "an e5m2 cache": (e5, K, V, shape()),
        "an fp32 cache": (f32, K, V, shape()),
        "head dimension 96": (KVCacheCompact(96, P.FP16), K, V, shape()),
        "zero rows": (c16, K, V, shape(rows=0)),
        "zero heads": (c16, K, V, shape(heads=0)),
        "zero batches": (c8, K, V, shape(batches=0)),
        "a grid above 2^31 - 1 workgroups": (c16, K, V, shape(heads=2 ** 30, batches=2)),
        "65 rows": (c16, K, V, shape(rows=65, maxAccepted=4)),
        "65 accepted": (c16, K, V, shape(maxAccepted=65)),
        "maxAccepted 0": (c16, K, V, shape(maxAccepted=0)),
        "a stride below maxAccepted": (c16, K, V, shape(maxAccepted=8, acceptedStride=7)),
        "null cacheLengths": (c16, K, V, shape(cacheLengths=None)),
        "null accepted": (c16, K, V, shape(accepted=None)),
        "null acceptedCounts": (c8, K, V, shape(acceptedCounts=None)),
        "misaligned accepted": (c16, K, V, shape(accepted=ACCEPTED + 2)),
        "newLengths is cacheLengths": (c16, K, V, shape(newLengths=LENGTHS)),
        "newLengths overlaps the end of cacheLengths": (c16, K, V, shape(newLengths=LENGTHS + 8)),
        "newLengths overlaps the start of cacheLengths": (c16, K, V, shape(newLengths=LENGTHS - 8)),
        "misaligned newLengths": (c16, K, V, shape(newLengths=NEW + 2)),
        "page size 24": (c16, K, V, paged(pageSize=24)),
        "paged without a table": (c16, K, V, paged(blockTable=None)),
        "a table stride of 0": (c16, K, V, paged(blockTableStride=0)),
        "contiguous without a column": (c16, K, V, shape(column=0)),
        "a leading dimension below D": (c16, K, V, shape(strides=dict(kCache=(64, 256 * 128, 2 * 256 * 128)))),
        "16-bit strides off 8 elements": (c16, K, V, shape(strides=dict(vCache=(132, 256 * 132, 2 * 256 * 132)))),
        "e4m3 strides off 16 elements": (c8, K, V, shape(strides=dict(kCache=(136, 256 * 136, 2 * 256 * 136)))),
        "a page stride off 8 elements": (c16, K, V, paged(pageStrides=(4100, 4096))),
        "a null K cache": (c16, None, V, shape()),
        "a null V cache": (c16, K, None, shape()),
        "a misaligned V cache": (c8, K, V + 8, shape()),
        # two mistakes: which one is reported
        "e5m2 and head dimension 96": (KVCacheCompact(96, KVCachePrecision.E5M2), K, V, shape()),
        "head dimension 96 and zero rows": (KVCacheCompact(96, P.BF16), K, V, shape(rows=0)),
        "zero rows and maxAccepted 65": (c16, K, V, shape(rows=0, maxAccepted=65)),
        "a grid too large and 65 rows": (c16, K, V, shape(heads=2 ** 30, batches=2, rows=65, maxAccepted=4)),
        "65 rows and a short stride": (c16, K, V, shape(rows=65, maxAccepted=8, acceptedStride=7)),
        "maxAccepted 0 and null accepted": (c16, K, V, shape(maxAccepted=0, accepted=None)),
        "a short stride and null cacheLengths": (c16, K, V, shape(maxAccepted=8, acceptedStride=7, cacheLengths=None)),
        "null accepted and null acceptedCounts": (c16, K, V, shape(accepted=None, acceptedCounts=None)),
        "null acceptedCounts and misaligned accepted": (c16, K, V, shape(acceptedCounts=None, accepted=ACCEPTED + 1)),
        "misaligned accepted and overlapping newLengths": (c16, K, V, shape(accepted=ACCEPTED + 1, newLengths=LENGTHS)),
        "overlapping newLengths and page size 24": (c16, K, V, paged(newLengths=LENGTHS + 4, pageSize=24)),
        "page size 24 and bad strides": (c16, K, V, paged(pageSize=24, pageStrides=(4100, 4096))),
        "bad strides and a null cache": (c16, None, V, shape(strides=dict(kCache=(64, 256 * 128, 2 * 256 * 128)))),
        "a null cache and a misaligned one": (c16, None, V + 8, shape()),
    }
    return {name: outcome(*c) for name, c in cases.items()}


def test_every_refusal_by_status_and_message_in_the_pinned_order():
    handle = _abi.lib()
    assert handle.mfa_kv_cache_compact_launch(K, V, None, None) == INVALID and handle.mfa_last_error_string() == b"null argument"
    got = refusal_cases()
    want = {  # (status, what the message names)
        "an e5m2 cache": (UNSUPPORTED, "e5m2 caches have no kernel"), "an fp32 cache": (INVALID, "cachePrecision must be"),
        "head dimension 96": (UNSUPPORTED, "head dimensions 64, 128 and 256, not 96"),
        "zero rows": (INVALID, "rows, heads and batches must be non-zero"), "zero heads": (INVALID, "rows, heads and batches must be non-zero"),
        "zero batches": (INVALID, "rows, heads and batches must be non-zero"),
        "a grid above 2^31 - 1 workgroups": (INVALID, "2 x heads x batches must fit a grid"), "a grid too large and 65 rows": (INVALID, "must fit a grid"),
        "65 rows": (UNSUPPORTED, "at most 64 nodes: rows = 65"), "65 accepted": (UNSUPPORTED, "maxAccepted = 65"),
        "maxAccepted 0": (INVALID, "maxAccepted must be non-zero"), "a stride below maxAccepted": (INVALID, "acceptedStride must be at least maxAccepted"),
        "null cacheLengths": (INVALID, "cacheLengths is required"), "null accepted": (INVALID, "accepted is required"),
        "null acceptedCounts": (INVALID, "acceptedCounts is required"), "misaligned accepted": (INVALID, "accepted must be 4-byte aligned"),
        "newLengths is cacheLengths": (INVALID, "newLengths must not overlap cacheLengths"),
        "newLengths overlaps the end of cacheLengths": (INVALID, "newLengths must not overlap cacheLengths"),
        "newLengths overlaps the start of cacheLengths": (INVALID, "newLengths must not overlap cacheLengths"),
        "misaligned newLengths": (INVALID, "newLengths must be 4-byte aligned"),
        "page size 24": (INVALID, "pageSize must be a power of two"), "paged without a table": (INVALID, "needs blockTable"),
        "a table stride of 0": (INVALID, "blockTableStride must be positive"), "contiguous without a column": (INVALID, "column (the capacity"),
        "a leading dimension below D": (INVALID, "leadingDimension of kCache is smaller"),
        "16-bit strides off 8 elements": (INVALID, "strides of vCache must be multiples of 8"),
        "e4m3 strides off 16 elements": (INVALID, "strides of kCache must be multiples of 16"),
        "a page stride off 8 elements": (INVALID, "strides of kCache must be multiples of 8"),
        "a null K cache": (INVALID, "null argument"), "a null V cache": (INVALID, "null argument"),
        "a misaligned V cache": (INVALID, "kCache and vCache must be 16-byte aligned"),
        "e5m2 and head dimension 96": (UNSUPPORTED, "e5m2 caches have no kernel"), "head dimension 96 and zero rows": (UNSUPPORTED, "not 96"),
        "zero rows and maxAccepted 65": (INVALID, "must be non-zero"), "65 rows and a short stride": (UNSUPPORTED, "rows = 65"),
        "maxAccepted 0 and null accepted": (INVALID, "maxAccepted must be non-zero"),
        "a short stride and null cacheLengths": (INVALID, "acceptedStride must be at least"),
        "null accepted and null acceptedCounts": (INVALID, "accepted is required"),
        "null acceptedCounts and misaligned accepted": (INVALID, "acceptedCounts is required"),
        "misaligned accepted and overlapping newLengths": (INVALID, "accepted must be 4-byte aligned"),
        "overlapping newLengths and page size 24": (INVALID, "newLengths must not overlap"),
        "page size 24 and bad strides": (INVALID, "pageSize must be a power of two"),
        "bad strides and a null cache": (INVALID, "leadingDimension of kCache"),
        "a null cache and a misaligned one": (INVALID, "null argument"),
    }
    assert set(got) == set(want)
    for name, (status, needle) in want.items():
        assert got[name][0] == status and needle in got[name][1], (name, got[name])
    assert got == json.load(open(GOLDEN)), "the refusals' statuses, words or order moved: tests/golden/compact_refusals.json"
    # the words the append launch has for the same mistakes
    from metal_flash_attention_amd import KVCacheAppend
    for over in (dict(pageSize=24, blockTable=TABLE, blockTableStride=4), dict(column=0), dict(strides=dict(kCache=(132, 256 * 132, 0)))):
        kw = dict(rows=1, heads=2, batches=3, column=256, cacheLengths=LENGTHS)
        kw.update(over)
        with pytest.raises(MFAError) as said:
            KVCacheAppend(128, P.BF16).dispatch(K, V, K, V, **kw)
        both = dict(kw, rows=12, accepted=ACCEPTED, acceptedCounts=COUNTS)
        assert outcome(KVCacheCompact(128, P.BF16), K, V, both)[1] == str(said.value).split(": ", 1)[1]


# ---------------------------------------------------------------------------------------------------- the torch side
torch = pytest.importorskip("torch")


def bits_of(parents):
    """bool [R, R] of a tree given as parent indices (-1: a root): row r holds r and its ancestors"""
    R = len(parents)
    bits = torch.zeros((R, R), dtype=torch.bool)
    for r in range(R):
        node = r
        while node >= 0:
            bits[r, node] = True
            node = parents[node]
    return bits


def test_tree_path_on_a_chain_a_forest_and_children_below_their_parents():
    from metal_flash_attention_amd import torch_binding as tb
    assert mfa.tree_path is tb.tree_path and mfa.kv_cache_compact is tb.kv_cache_compact
    chain = bits_of([-1, 0, 1, 2, 3])
    accepted, count = tb.tree_path(chain, 3)
    assert accepted.dtype == torch.int32 and count.dtype == torch.int32 and accepted.tolist() == [0, 1, 2, 3, -1] and int(count) == 4
    accepted, counts = tb.tree_path(chain, torch.tensor([4, 0]))                      # one tree, a leaf per sequence
    assert accepted.tolist() == [[0, 1, 2, 3, 4], [0, -1, -1, -1, -1]] and counts.tolist() == [5, 1]
    forest = bits_of([-1, -1, 0, 1, 2, 2, 3])                                         # two roots: 0 -> 2 -> {4, 5}, 1 -> 3 -> 6
    accepted, counts = tb.tree_path(torch.stack([forest, forest, forest]), torch.tensor([5, 6, 1]))
    assert accepted.tolist() == [[0, 2, 5, -1, -1, -1, -1], [1, 3, 6, -1, -1, -1, -1], [1, -1, -1, -1, -1, -1, -1]] and counts.tolist() == [3, 3, 1]
    upward = bits_of([3, 0, 1, -1, 2])                                                # the root is node 3; 3 -> 0 -> 1 -> 2 -> 4: children below parents
    accepted, counts = tb.tree_path(upward[None], torch.tensor([2]))
    assert accepted.tolist() == [[3, 0, 1, 2, -1]] and counts.tolist() == [4]
    accepted, count = tb.tree_path(upward, 4)
    assert accepted.tolist() == [3, 0, 1, 2, 4] and int(count) == 5
    full = bits_of(list(range(1, 64)) + [-1])                                         # 64 nodes, a reversed chain: node 63 is the root
    accepted, count = tb.tree_path(full, 0)
    assert accepted.tolist() == list(range(63, -1, -1)) and int(count) == 64
    for bad in (torch.zeros((65, 65), dtype=torch.bool), torch.zeros((4, 5), dtype=torch.bool), torch.zeros((4,), dtype=torch.bool)):
        with pytest.raises(ValueError, match="tree_path: expected bool"):
            tb.tree_path(bad, 0)
    with pytest.raises(ValueError, match="one index per tree"):
        tb.tree_path(torch.stack([chain, chain]), torch.tensor([1, 2, 3]))


def test_the_op_s_schema_and_its_fake_implementation():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from metal_flash_attention_amd import torch_binding as tb
    assert hasattr(torch.library, "custom_op") and tb._HAVE_COMPACT_OP, "the installed torch has no torch.library.custom_op: mfa::kv_cache_compact is missing"
    schema = str(torch.ops.mfa.kv_cache_compact.default._schema)
    assert schema == ("mfa::kv_cache_compact(Tensor(a0!) k_cache, Tensor(a1!) v_cache, Tensor cache_lengths, Tensor accepted, Tensor accepted_counts, "
                      "SymInt rows, Tensor? q_lengths, Tensor? block_table) -> Tensor"), schema
    with FakeTensorMode():
        k16 = torch.empty((3, 2, 256, 128), dtype=torch.bfloat16, device="cuda")
        pool = torch.empty((50, 2, 16, 64), dtype=torch.float8_e4m3fn, device="cuda")
        lens = torch.empty((3,), dtype=torch.int32, device="cuda")
        accepted = torch.empty((3, 12), dtype=torch.int32, device="cuda")
        table = torch.empty((3, 16), dtype=torch.int32, device="cuda")
        out = torch.ops.mfa.kv_cache_compact(k16, k16.clone(), lens, accepted, lens, 12, None, None)
        assert out.shape == (3,) and out.dtype == torch.int32 and out.device.type == "cuda"
        out = tb.kv_cache_compact(pool, pool.clone(), lens.long(), accepted, lens, 12, q_lengths=lens, block_table=table)
        assert out.shape == (3,) and out.dtype == torch.int32
        for call, kind, needle in (
                (lambda: tb.kv_cache_compact(k16.cpu(), k16, lens, accepted, lens, 12), RuntimeError, "tensors must live on the GPU"),
                (lambda: tb.kv_cache_compact(k16, k16, lens, accepted.cpu(), lens, 12), RuntimeError, "tensors must live on the GPU"),
                (lambda: tb.kv_cache_compact(k16.requires_grad_(), k16, lens, accepted, lens, 12), RuntimeError, "writes in place and has no autograd")):
            with pytest.raises(kind, match=needle):
                call()


def test_the_binding_s_refusals_in_words():
    """_run_compact's own checks run before any launch: on the CPU they are reached with tensors that only claim to be on the GPU"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    from metal_flash_attention_amd import torch_binding as tb
    with FakeTensorMode():
        k16 = torch.empty((3, 2, 256, 128), dtype=torch.bfloat16, device="cuda")
        lens = torch.empty((3,), dtype=torch.int32, device="cuda")
        accepted = torch.empty((3, 12), dtype=torch.int32, device="cuda")
        run = tb._run_compact
        elsewhere = type("Elsewhere", (), dict(is_cuda=True, device=torch.device("cuda", (k16.device.index or 0) + 1)))()
        for call, kind, needle in (
                (lambda: run(k16, k16.half(), lens, accepted, lens, 12, None, None), TypeError, "the caches must both be bfloat16, float16 or torch.float8_e4m3fn"),
                (lambda: run(k16.float(), k16.float(), lens, accepted, lens, 12, None, None), TypeError, "the caches must both be"),
                (lambda: run(k16, k16[:, :1], lens, accepted, lens, 12, None, None), ValueError, "expected caches"),
                (lambda: run(k16, k16, lens[:2], accepted, lens, 12, None, None), ValueError, "cache_lengths must be a GPU tensor"),
                (lambda: run(k16, k16, lens, accepted, lens, 65, None, None), ValueError, "rows must be an int from 1 to 64"),
                (lambda: run(k16, k16, lens, accepted, lens, True, None, None), ValueError, "rows must be an int from 1 to 64"),
                (lambda: run(k16, k16, lens, accepted.long(), lens, 12, None, None), ValueError, "accepted must be an int32 GPU tensor"),
                (lambda: run(k16, k16, lens, accepted[:2], lens, 12, None, None), ValueError, "accepted must be an int32 GPU tensor"),
                (lambda: run(k16, k16, lens, torch.empty((3, 65), dtype=torch.int32, device="cuda"), lens, 12, None, None), ValueError,
                 "at most 64 nodes per sequence"),
                (lambda: run(k16, k16, lens, accepted, lens.float(), 12, None, None), ValueError, "accepted_counts must be a GPU tensor"),
                (lambda: run(k16, k16, lens, accepted, lens, 12, lens[:1], None), ValueError, "q_lengths must be a GPU tensor"),
                (lambda: run(k16, k16, lens, accepted, lens, 12, None, lens), ValueError, "block_table must be an int32 GPU tensor"),
                (lambda: run(k16.transpose(2, 3), k16.transpose(2, 3), lens, accepted, lens, 12, None, None), ValueError, "contiguous last dimension"),
                # another GPU than the caches': its pointer must not reach the launch (a stand-in: a one-GPU machine has no cuda:1 to allocate on)
                (lambda: run(k16, k16, elsewhere, accepted, lens, 12, None, None), RuntimeError, "cache_lengths must live on the GPU of the cache"),
                (lambda: run(k16, k16, lens, elsewhere, lens, 12, None, None), RuntimeError, "accepted must live on the GPU of the cache"),
                (lambda: run(k16, k16, lens, accepted, lens, 12, elsewhere, None), RuntimeError, "q_lengths must live on the GPU of the cache"),
                (lambda: run(k16, k16, lens, accepted, lens, 12, None, elsewhere), RuntimeError, "block_table must live on the GPU of the cache")):
            with pytest.raises(kind) as said:
                call()
            assert needle in str(said.value) and str(said.value).startswith("kv_cache_compact: "), str(said.value)
