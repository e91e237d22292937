"""CPU test (no GPU call): the host side of ragged batches over a KV cache, include/mfa_ragged.h -- exported symbols and the struct
mirror, every refusal with its message, the launch-form text, the slot bound and the slot function (the very function the kernels'
lane-parallel form must answer like: prefill_ragged_block, csrc/attn_prefill16.h) against a brute-force scan, and the fake-tensor
path of the two torch ops."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import ragged_model as rm
from metal_flash_attention_amd import AttentionPrefill, GEMMOperandPrecision as P, KVCacheAppend, KVCachePrecision, MFAError, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS, LOGITS, STARTS = 0x1000, 0x3000, 0x5000   # any non-null values: the host never reads the lengths, the logits or the starts
UNSUPPORTED, INVALID = 3, 2


def pshape(**over):
    kw = dict(rows=512, column=4096, heads=64, batches=4, headsPerKeyValue=8, cacheLengths=LENGTHS, rowStarts=STARTS, totalRows=700)
    kw.update(over)
    return kw


def ashape(**over):
    kw = dict(rows=512, heads=8, batches=4, column=4096, cacheLengths=LENGTHS, rowStarts=STARTS, totalRows=700)
    kw.update(over)
    return kw


def refused(status, needle, call, *args, **kw):
    with pytest.raises(MFAError) as e:
        call(*args, **kw)
    assert e.value.status == status, str(e.value)
    assert needle in str(e.value), str(e.value)


def test_header_symbols_exported_and_the_struct_mirror():
    header = open(os.path.join(ROOT, "include", "mfa_ragged.h")).read()
    assert '#include "mfa_sink.h"' in header
    declared = set(re.findall(r"\b(mfa_(?:attention_prefill_ragged|ragged_rows|kv_cache_append_ragged)_\w+)\s*\(", header))
    handle = _abi.lib()
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in include/mfa_ragged.h but not exported"
    assert declared == {s[0] for s in _abi.RAGGED_SYMBOLS}
    assert len(declared) == 9
    assert int(handle.mfa_abi_version()) == 6   # mfa.h did not change
    assert ctypes.sizeof(_abi.mfa_ragged_rows) == int(handle.mfa_ragged_rows_size()) == 16
    offsets, count = (ctypes.c_uint32 * 8)(), ctypes.c_uint32(0)
    assert handle.mfa_ragged_rows_offsets(offsets, 8, ctypes.byref(count)) == 0
    mirror = [getattr(_abi.mfa_ragged_rows, name).offset for name, _ in _abi.mfa_ragged_rows._fields_]
    assert list(offsets[:count.value]) == mirror == [0, 8, 12]
    block = _abi.mfa_ragged_rows(7, 7, 7)
    handle.mfa_ragged_rows_init(ctypes.byref(block))
    assert (block.rowStarts, block.totalRows, block.reserved) == (None, 0, 0)
    # the existing structs did not grow
    assert int(handle.mfa_prefill_params_size()) == ctypes.sizeof(_abi.mfa_prefill_params) and int(handle.mfa_attention_sinks_size()) == 16


def test_refusals_name_the_field():
    pre, app = AttentionPrefill(128, P.BF16), KVCacheAppend(128, P.BF16)
    handle = _abi.lib()
    bufs = (0x10000, 0x20000, 0x30000, 0x40000)
    for call in (pre.launchForm, lambda **kw: pre.dispatch(*bufs, None, **kw), lambda **kw: pre.time(*bufs, None, **kw)):
        refused(INVALID, "rowStarts is required", call, **pshape(rowStarts=None))
        refused(INVALID, "totalRows must be non-zero", call, **pshape(totalRows=0))
        refused(INVALID, "queryLengths must be NULL for a ragged launch", call, **pshape(queryLengths=0x7000))
        refused(INVALID, "batchStride of Q and O must be 0", call, **pshape(strides=dict(Q=(8192, 128, 8192))))
        refused(INVALID, "batchStride of Q and O must be 0", call, **pshape(strides=dict(O=(8192, 128, 64))))
        refused(INVALID, "lBatchStride must be 0", call, **pshape(lStrides=(700, 700 * 64)))
    refused(INVALID, "rowStarts is required", lambda **kw: app.dispatch(*bufs, **kw), **ashape(rowStarts=None))
    refused(INVALID, "totalRows must be non-zero", lambda **kw: app.dispatch(*bufs, **kw), **ashape(totalRows=0))
    refused(INVALID, "batchStride of kNew and vNew must be 0", lambda **kw: app.dispatch(*bufs, **kw), **ashape(strides=dict(kNew=(1024, 128, 1024))))
    refused(INVALID, "batchStride of kNew and vNew must be 0", lambda **kw: app.dispatch(*bufs, **kw), **ashape(strides=dict(vNew=(1024, 128, 8))))
    # a NULL block, straight through the C entries (the keywords cannot say it)
    pp, _keep = pre._params(ragged=None, **{k: v for k, v in pshape().items() if k not in ("rowStarts", "totalRows")})
    ap = app._params(ragged=None, **{k: v for k, v in ashape().items() if k not in ("rowStarts", "totalRows")})
    out, ms = ctypes.create_string_buffer(512), ctypes.c_float(0)
    for status in (handle.mfa_attention_prefill_ragged_launch_form(ctypes.byref(pp), 0, None, None, out, len(out)),
                   handle.mfa_attention_prefill_ragged_launch(*bufs, None, ctypes.byref(pp), 0, None, None, None),
                   handle.mfa_attention_prefill_ragged_time(*bufs, None, ctypes.byref(pp), 0, None, None, None, 1, 1, ctypes.byref(ms)),
                   handle.mfa_kv_cache_append_ragged_launch(*bufs, ctypes.byref(ap), None, None)):
        assert status == INVALID and "null mfa_ragged_rows" in handle.mfa_last_error_string().decode()
    # the inherited refusals, through the new entries: the sinks', the window's, the prefill's and the append's, in their words
    refused(INVALID, "sink tokens need a window", pre.launchForm, sinkTokens=4, **pshape())
    refused(INVALID, "sink tokens need causal", pre.launchForm, window=7, sinkTokens=4, causal=False, **pshape())
    refused(INVALID, "a sliding window needs causal", pre.launchForm, window=7, causal=False, **pshape())
    refused(UNSUPPORTED, "64 and 128, not 96", AttentionPrefill(96, P.BF16).launchForm, **pshape())
    refused(UNSUPPORTED, "at most 32, not 64", pre.launchForm, **pshape(headsPerKeyValue=64))
    refused(INVALID, "needs blockTable", pre.launchForm, **pshape(pageSize=64))
    refused(INVALID, "cacheLengths is required", pre.launchForm, **pshape(cacheLengths=None))
    refused(INVALID, "rows, column, heads and batches must be non-zero", pre.launchForm, **pshape(rows=0))
    refused(INVALID, "Q", pre.launchForm, **pshape(strides=dict(Q=(8196, 128, 0))))          # strides of Q: multiples of 8
    refused(UNSUPPORTED, "64 and 128, not 96", lambda **kw: KVCacheAppend(96, P.BF16).dispatch(*bufs, **kw), **ashape())
    refused(INVALID, "cacheLengths is required", lambda **kw: app.dispatch(*bufs, **kw), **ashape(cacheLengths=None))
    with pytest.raises(MFAError) as e:   # pointers: checked before any GPU call (the process never opens the device)
        pre.dispatch(0x10000, 0x20000, 0x30000, 0x40008, None, **pshape())
    assert e.value.status == INVALID and "16-byte aligned" in str(e.value), str(e.value)
    with pytest.raises(MFAError) as e:
        app.dispatch(0x10000, 0x20008, 0x30000, 0x40000, **ashape())
    assert e.value.status == INVALID and "16-byte aligned" in str(e.value), str(e.value)
    # the range functions
    refused(INVALID, "blockRows must be non-zero", AttentionPrefill.raggedSlots, 100, 2, 50, 0)
    refused(INVALID, "blockRows must be non-zero", AttentionPrefill.raggedBlock, [0, 50, 100], 100, 50, 0, 0)
    # a grid no launch can hold, named
    refused(UNSUPPORTED, "row blocks exceed 2^31 - 1", pre.launchForm, **pshape(rows=2 ** 32 - 1, batches=64, totalRows=2 ** 32 - 1))


def test_launch_form_is_the_pinned_text():
    heads, B, rows, G, T = 24, 5, 300, 8, 471
    for prec, tn in ((P.BF16, "bf16"), (P.FP16, "f16")):
        for D in (64, 128):
            for fp8 in (False, True):
                pre = AttentionPrefill(D, prec, cachePrecision=KVCachePrecision.E4M3 if fp8 else None)
                for paged in (False, True):
                    for W, S, logits, tail in ((None, None, False, ""), (0, 0, False, ""), (65, None, False, ", window 65"),
                                               (65, 4, True, ", window 65, sink tokens 4, sink logits"), (65, 70, False, ", window 65, sink tokens 70"),
                                               (0, 0, True, ", sink logits"), (9, 0, True, ", window 9, sink logits")):
                        kw = pshape(rows=rows, heads=heads, batches=B, headsPerKeyValue=G, totalRows=T)
                        if paged:
                            kw.update(pageSize=16, blockTable=0x2000, blockTableStride=256)
                        if W is not None:
                            kw.update(window=W)
                        if S is not None or logits:
                            kw.update(sinkTokens=S, sinkLogits=LOGITS if logits else None)
                        slots = min(T // 16 + B, B * 19)
                        assert slots == AttentionPrefill.raggedSlots(T, B, rows, 16) == 34
                        assert pre.launchForm(**kw) == (
                            "attn_prefill16r_d%d_%s%s (grid %d = %d slots x %d K/V heads, row blocks of %d rows x %d heads, %d packed rows of %d "
                            "sequences, at most %d rows each, %s%s)" % (D, tn, "_e4m3" if fp8 else "", slots * (heads // G), slots, heads // G, 16, G, T, B,
                                                                       rows, "paged" if paged else "contiguous", tail))
    # the padded launch's text did not change
    assert AttentionPrefill(128, P.BF16).launchForm(rows=300, column=4096, heads=24, batches=2, headsPerKeyValue=8, cacheLengths=LENGTHS) == \
        "attn_prefill16_d128_bf16 (grid 114 = 2 sequences x 3 K/V heads x 19 row blocks of 16 rows x 8 heads, contiguous)"
    # the uniform batch: the two grids coincide
    assert AttentionPrefill.raggedSlots(8 * 512, 8, 512, 16) == 8 * 32
    # the issue's batch: 255 one-row sequences and one chunk of 4096 rows, against 65536 padded row blocks per K/V head
    assert AttentionPrefill.raggedSlots(255 + 4096, 256, 4096, 16) == 527


def check_slots(starts, T, cap, RB, monotone):
    B = len(starts) - 1
    want = rm.slot_map(starts, T, cap, RB)
    slots = AttentionPrefill.raggedSlots(T, B, cap, RB)
    case = (starts, T, cap, RB)
    assert slots == rm.slots(T, B, cap, RB), case
    if monotone:
        assert slots >= len(want), case                  # the bound holds: every live row block has a slot inside the grid
    got = [AttentionPrefill.raggedBlock(starts, T, cap, RB, i) for i in range(max(slots, len(want)) + 2)]
    assert got[:len(want)] == want, case                  # every live row block of every sequence, served by exactly one slot, in order
    assert all(g == (None, 0) for g in got[len(want):]), case   # and the slots past the total serve nothing
    for b, r0 in got[:len(want)]:                         # no access outside [0, T): the block's live rows lie inside its sequence's rows
        s, qn = rm.counts_of(starts, T, cap)[b]
        assert r0 % RB == 0 and r0 < qn and s + qn <= T, case


@pytest.mark.parametrize("RB", [4, 16, 42, 128])
def test_slots_and_the_slot_map_against_a_brute_force_scan(RB):
    rng = np.random.default_rng(RB)
    pool = [0, 1, RB - 1, RB, RB + 1, 3 * RB + 5]
    for B in range(1, 10):
        draws = list(itertools.product(pool, repeat=B)) if B <= 3 else [tuple(rng.choice(pool, B)) for _ in range(60)]
        for counts in draws:
            top = max(counts)
            starts = rm.row_starts(counts)
            T = starts[-1]
            for cap in sorted({max(top - 1, 1), max(top, 1), top + 7, max(RB - 1, 1)}):   # below and above the largest count
                check_slots(starts, max(T, 1), cap, RB, True)
            if T > 2:                                  # starts clamped by T: the last sequences lose rows, or all of them
                check_slots(starts, T - 1, max(top, 1), RB, True)
                check_slots(starts, T // 2, max(top, 1), RB, True)
    # a decreasing pair: the sequence whose end lies below its start has qn = 0, and nothing reaches past T
    for starts in ([0, 3 * RB, RB, 2 * RB + 1], [5, 2, 9, 9, 4, 20], [2 ** 32 - 1, 0, 7]):
        for T in (1, RB, 2 * RB + 1, 10 * RB):
            check_slots(starts, T, 3 * RB + 5, RB, False)
            assert all(qn == 0 for (s, qn), a, e in zip(rm.counts_of(starts, T, 10 ** 6), starts, starts[1:]) if e < a)
    # no wrap-around at the top of the range
    assert AttentionPrefill.raggedBlock([0, 2 ** 32 - 1], 2 ** 32 - 1, 2 ** 32 - 1, 128, (2 ** 32 - 1) // 128) == (0, (2 ** 32 - 1) // 128 * 128)
    assert AttentionPrefill.raggedBlock([0, 2 ** 32 - 1], 2 ** 32 - 1, 2 ** 32 - 1, 128, (2 ** 32 - 1) // 128 + 1) == (None, 0)


def test_pack_and_unpack_are_inverse():
    counts, cap = [40, 17, 1, 0, 16, 33], 35
    starts = rm.row_starts(counts)
    T = starts[-1]
    rng = np.random.default_rng(0)
    padded = rng.standard_normal((len(counts), 3, 40, 8)).astype(np.float32)
    packed = rm.pack(padded, starts, T, cap, fill=-1)
    assert packed.shape == (T, 3, 8) and (packed[~rm.owned(starts, T, cap)] == -1).all()
    back = rm.unpack(packed, starts, T, cap, 40, fill=7)
    for b, c in enumerate(counts):
        assert (back[b, :, :min(c, cap)] == padded[b, :, :min(c, cap)]).all() and (back[b, :, min(c, cap):] == 7).all()
    l = rng.standard_normal((3, T)).astype(np.float32)
    assert (rm.unpack_l(l, starts, T, cap, 40)[0, :, :35] == l[:, :35]).all()


def test_fake_tensor_path_and_argument_checks_without_a_device():
    torch = pytest.importorskip("torch")
    from torch._subclasses.fake_tensor import FakeTensorMode
    from metal_flash_attention_amd import torch_binding as tb
    if not tb._HAVE_RAGGED_OPS:
        pytest.skip("this torch has no torch.library.custom_op")
    with FakeTensorMode():
        T, H, Hkv, D, B = 107, 8, 2, 128, 6
        fused = torch.empty((T, (H + 2 * Hkv) * D), dtype=torch.bfloat16, device="cuda")
        q = fused[:, :H * D].view(T, H, D)
        kn, vn = fused[:, H * D:(H + Hkv) * D].view(T, Hkv, D), fused[:, (H + Hkv) * D:].view(T, Hkv, D)
        k8 = torch.empty((B, Hkv, 1024, D), dtype=torch.float8_e4m3fn, device="cuda")
        k16 = torch.empty((B, Hkv, 1024, D), dtype=torch.bfloat16, device="cuda")
        lens = torch.empty((B,), dtype=torch.int32, device="cuda")
        starts = torch.empty((B + 1,), dtype=torch.int32, device="cuda")
        scale = torch.empty((Hkv,), dtype=torch.float32, device="cuda")
        logits = torch.empty((H,), dtype=torch.float32, device="cuda")
        o, l = torch.ops.mfa.attention_prefill_ragged(q, k8, k8, lens, starts, 40, None, True, scale, scale, 100, 4, logits)
        assert o.shape == (T, H, D) and o.dtype == torch.bfloat16 and l.shape == (H, T) and l.dtype == torch.float32
        assert torch.ops.mfa.kv_cache_append_ragged(kn, vn, k16, k16, lens, starts, 40, None, None, None) is None
        assert tb.flash_prefill_ragged(q, k16, k16, lens, starts, 40, window=65, sink_tokens=4).shape == (T, H, D)
        o, lse = tb.flash_prefill_ragged(q.half(), k8, k8, lens, starts, 40, k_scale=scale, sink_logits=logits, return_lse=True)
        assert o.dtype == torch.float16 and o.shape == (T, H, D) and lse.shape == (H, T)
        assert tb.kv_cache_append_ragged(kn, vn, k8, k8, lens, starts, 40, k_scale=scale) is None
        # flash_prefill's refusals, in its words
        for bad in (0, -1, True, 2 ** 32, 1.5):
            with pytest.raises(ValueError, match="sink_tokens must be an int"):
                tb.flash_prefill_ragged(q, k16, k16, lens, starts, 40, window=5, sink_tokens=bad)
            with pytest.raises(ValueError, match="window must be an int"):
                tb.flash_prefill_ragged(q, k16, k16, lens, starts, 40, window=bad)
        with pytest.raises(ValueError, match="sink_tokens needs window"):
            tb.flash_prefill_ragged(q, k16, k16, lens, starts, 40, sink_tokens=4)
        with pytest.raises(ValueError, match="needs causal"):
            tb.flash_prefill_ragged(q, k16, k16, lens, starts, 40, window=5, causal=False)
        for bad in (logits.half(), logits[:4], torch.empty((1, H), dtype=torch.float32, device="cuda")):
            with pytest.raises(ValueError, match="sink_logits must be a contiguous float32"):
                tb.flash_prefill_ragged(q, k16, k16, lens, starts, 40, sink_logits=bad)
        with pytest.raises(RuntimeError, match="forward only"):
            tb.flash_prefill_ragged(q.float().requires_grad_().bfloat16(), k16, k16, lens, starts, 40)
        with pytest.raises(RuntimeError, match="no autograd"):
            tb.kv_cache_append_ragged(kn.float().requires_grad_().bfloat16(), vn, k16, k16, lens, starts, 40)
    for name in ("attention_prefill_ragged", "kv_cache_append_ragged"):
        assert hasattr(torch.ops.mfa, name)
    # what only the op's body checks (the fake path never runs it): the same words, on CPU tensors
    q = torch.zeros((10, 8, 64), dtype=torch.bfloat16)
    k = torch.zeros((2, 2, 64, 64), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="tensors must live on the GPU"):
        tb.flash_prefill_ragged(q, k, k, torch.zeros(2, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), 5)
    with pytest.raises(RuntimeError, match="tensors must live on the GPU"):
        tb.kv_cache_append_ragged(q[:, :2], q[:, :2], k, k, torch.zeros(2, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), 5)
