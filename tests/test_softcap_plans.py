"""CPU test (no GPU call): the host side of logit soft-capping over a KV cache, include/mfa_softcap.h -- exported symbols and the
ctypes mirror, softcap = 0 as the launch of the header below for every family, the capped kernels' names for every head dimension
and type, the workspace of a capped launch, every refusal of a bad cap with its one wording, and a NULL `sinks`."""
import ctypes
import os
import re

import pytest

from metal_flash_attention_amd import AttentionDecode, AttentionDecodeFP8, AttentionPrefill, GEMMOperandPrecision as P, KVCachePrecision, MFAError, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS, LOGITS, STARTS = 0x1000, 0x3000, 0x5000   # any non-null values: the host never reads the lengths, the logits or the row starts
INVALID = 2
WORDING = "softcap must be 0 (no cap) or a finite positive number"
TYPES = ((P.BF16, "bf16"), (P.FP16, "f16"))
DIMS = (64, 128, 256)
# the families below the cap: plain, window, sink tokens, sink logits, both
FAMILIES = (dict(), dict(window=0), dict(window=130), dict(window=130, sinkTokens=4), dict(sinkLogits=LOGITS), dict(window=4096, sinkTokens=70, sinkLogits=LOGITS))


def dshape(**over):
    kw = dict(rows=1, column=32768, heads=64, batches=1, headsPerKeyValue=8, cacheLengths=LENGTHS)
    kw.update(over)
    return kw


def pshape(**over):
    kw = dict(rows=512, column=4096, heads=64, batches=4, headsPerKeyValue=8, cacheLengths=LENGTHS)
    kw.update(over)
    return kw


def rshape(**over):
    return pshape(rowStarts=STARTS, totalRows=1000, **over)


def refused(needle, call, *args, **kw):
    with pytest.raises(MFAError) as e:
        call(*args, **kw)
    assert e.value.status == INVALID, str(e.value)
    assert needle in str(e.value), str(e.value)


def test_header_symbols_exported_and_the_ctypes_mirror():
    header = open(os.path.join(ROOT, "include", "mfa_softcap.h")).read()
    assert '#include "mfa_sink.h"' in header and '#include "mfa_ragged.h"' in header
    declared = set(re.findall(r"\b(mfa_attention_\w*softcap_\w+)\s*\(", header))
    handle = _abi.lib()
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in include/mfa_softcap.h but not exported"
    assert declared == {s[0] for s in _abi.SOFTCAP_SYMBOLS}
    assert declared == {"mfa_attention_decode_softcap_" + s for s in ("workspace_size", "launch", "launch_form", "time")} | \
        {"mfa_attention_prefill_%ssoftcap_%s" % (r, s) for r in ("", "ragged_") for s in ("launch", "launch_form", "time")}
    for name, restype, argtypes in _abi.SOFTCAP_SYMBOLS:
        fn = getattr(handle, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes and argtypes.count(ctypes.c_float) == 1
        at = argtypes.index(ctypes.c_float)   # `softcap` follows `sinks`, or `ragged` in the ragged entries
        assert argtypes[at - 1] is (_abi._RAGGED if "ragged" in name else _abi._SINKS)
    assert int(handle.mfa_abi_version()) == 6   # mfa.h did not change


def test_softcap_zero_is_the_launch_of_the_header_below_for_every_family():
    for D in DIMS:
        for prec, _tn in TYPES:
            for cls in (AttentionDecode, AttentionDecodeFP8):
                dec = cls(D, prec)
                for kw in (dshape(), dshape(workspace=0x100000, workspaceBytes=1 << 30), dshape(rows=4, column=300, pageSize=16, blockTable=0x2000, blockTableStride=32)):
                    for fam in FAMILIES:
                        assert dec.launchForm(softcap=0, **fam, **kw) == dec.launchForm(**fam, **kw), (D, fam)
                        assert re.match(r"attn_decode(16|8)[ws]?_d%d_" % D, dec.launchForm(softcap=0.0, **fam, **kw))
                        assert dec.workspaceSize(softcap=0, **fam, **kw) == dec.workspaceSize(**fam, **kw)
            for cache in (None, KVCachePrecision.E4M3):
                pre = AttentionPrefill(D, prec, cachePrecision=cache)
                for fam in FAMILIES:
                    assert pre.launchForm(softcap=0, **fam, **pshape()) == pre.launchForm(**fam, **pshape()), (D, fam)
                    text = pre.launchForm(softcap=0, **fam, **rshape())
                    assert text == pre.launchForm(**fam, **rshape()) and text.startswith("attn_prefill16r_d%d_" % D), (D, fam)


def test_a_capped_launch_runs_the_capped_family_whatever_its_window_and_sinks():
    for D in DIMS:
        for prec, tn in TYPES:
            for fam in FAMILIES:
                for fp8 in (False, True):
                    dec = (AttentionDecodeFP8 if fp8 else AttentionDecode)(D, prec)
                    name = "attn_decode%sc_d%d_%s" % ("8" if fp8 else "16", D, tn)
                    kw = dshape(heads=16, batches=2, headsPerKeyValue=4)
                    need = dec.workspaceSize(softcap=50.0, **fam, **kw)
                    sink = dict(sinkTokens=0, sinkLogits=None)
                    sink.update(fam)
                    assert need == dec.workspaceSize(**sink, **kw), (D, fam)                  # the sink launch's workspace
                    assert need > 0 or fam.get("window") == 130                               # (a short window plans one piece)
                    # the text of the launch below with the capped family's name and the cap put in: nothing else of the plan moves
                    for ws in (dict(), dict(workspace=0x100000, workspaceBytes=need)):
                        text, want = dec.launchForm(softcap=50.0, **ws, **fam, **kw), dec.launchForm(**ws, **sink, **kw)
                        kernel = name + ("_pieces" if need and ws else "_single")
                        assert text.startswith(kernel + " ("), text
                        want = re.sub(r"^attn_decode(16|8)[ws]?_d", r"attn_decode\1c_d", want)
                        if need and ws:
                            assert text == want.replace(") + attn", ", softcap 50) + attn") and text.endswith("attn_decode16_d%d_%s_combine (grid 8)" % (D, tn)), (text, want)
                        elif need:
                            assert text == want.replace(", unsplit without", ", softcap 50, unsplit without"), (text, want)
                        else:
                            assert text == want[:-1] + ", softcap 50)", (text, want)
                    pre = AttentionPrefill(D, prec, cachePrecision=KVCachePrecision.E4M3 if fp8 else None)
                    tail = "_e4m3" if fp8 else ""
                    text = pre.launchForm(softcap=50.0, **fam, **pshape())
                    want = pre.launchForm(**sink, **pshape())
                    assert text.startswith("attn_prefill16c_d%d_%s%s (" % (D, tn, tail)) and text.endswith(", softcap 50)"), text
                    assert text == re.sub(r"^attn_prefill16[ws]?_d", "attn_prefill16c_d", want)[:-1] + ", softcap 50)", (text, want)
                    text = pre.launchForm(softcap=1.0, **fam, **rshape())
                    want = pre.launchForm(**fam, **rshape())
                    assert text.startswith("attn_prefill16rc_d%d_%s%s (" % (D, tn, tail)), text
                    assert text == want.replace("r_d%d" % D, "rc_d%d" % D, 1)[:-1] + ", softcap 1)", (text, want)
    # not causal, no window: the capped family still
    assert AttentionDecode(256, P.BF16).launchForm(softcap=50, causal=False, **dshape()).startswith("attn_decode16c_d256_bf16_single ")
    assert AttentionPrefill(256, P.FP16).launchForm(softcap=50, causal=False, **pshape()).startswith("attn_prefill16c_d256_f16 ")


def test_a_bad_cap_is_refused_in_one_wording_by_every_entry():
    dec, dec8, pre = AttentionDecode(128, P.BF16), AttentionDecodeFP8(256, P.FP16), AttentionPrefill(64, P.BF16)
    for bad in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        for call, shape in ((dec.launchForm, dshape), (dec.workspaceSize, dshape), (dec8.launchForm, dshape), (pre.launchForm, pshape), (pre.launchForm, rshape)):
            refused(WORDING, call, softcap=bad, **shape())
            refused(WORDING, call, softcap=bad, window=130, sinkTokens=4, sinkLogits=LOGITS, **shape())
        for obj, shape in ((dec, dshape), (pre, pshape), (pre, rshape)):   # before any GPU call: the process never opens the device
            refused(WORDING, obj.dispatch, 0x10000, 0x20000, 0x30000, 0x40000, None, softcap=bad, **shape())
            refused(WORDING, obj.time, 0x10000, 0x20000, 0x30000, 0x40000, None, softcap=bad, **shape())
    # the inherited refusals, through the new entries
    refused("sink tokens need a window", dec.launchForm, softcap=50, sinkTokens=4, **dshape())
    refused("a sliding window needs causal", pre.launchForm, softcap=50, window=7, causal=False, **pshape())
    refused("workspace too small", dec.launchForm, softcap=50, **dshape(workspace=0x100000, workspaceBytes=16))
    refused("sinkLogits must be 4-byte aligned", dec.dispatch, 0x10000, 0x20000, 0x30000, 0x40000, None, softcap=50, sinkLogits=0x50002, **dshape())


def test_a_null_sinks_block_is_accepted_and_a_null_ragged_block_is_not():
    handle = _abi.lib()
    dec, pre = AttentionDecode(256, P.BF16), AttentionPrefill(256, P.BF16)
    p, _keep = dec._params(**dshape())
    pp, _keep = pre._params(**pshape())
    out, size, cap = ctypes.create_string_buffer(512), ctypes.c_uint64(0), ctypes.c_float(50.0)
    assert handle.mfa_attention_decode_softcap_launch_form(ctypes.byref(p), None, 0, None, cap, out, len(out)) == 0
    assert out.value.decode() == dec.launchForm(softcap=50.0, **dshape()) and out.value.startswith(b"attn_decode16c_d256_bf16_single ")
    assert handle.mfa_attention_decode_softcap_workspace_size(ctypes.byref(p), None, 0, None, cap, ctypes.byref(size)) == 0
    assert size.value == dec.workspaceSize(**dshape()) > 0
    assert handle.mfa_attention_prefill_softcap_launch_form(ctypes.byref(pp), 130, None, cap, out, len(out)) == 0
    assert out.value.startswith(b"attn_prefill16c_d256_bf16 ") and out.value.endswith(b", window 130, softcap 50)")
    # softcap 0 with a NULL block: the window launch, the plain one without a window
    assert handle.mfa_attention_prefill_softcap_launch_form(ctypes.byref(pp), 130, None, ctypes.c_float(0.0), out, len(out)) == 0
    assert out.value.decode() == pre.launchForm(window=130, **pshape())
    assert handle.mfa_attention_decode_softcap_launch_form(ctypes.byref(p), None, 0, None, ctypes.c_float(0.0), out, len(out)) == 0
    assert out.value.decode() == dec.launchForm(**dshape())
    # an all-zero block is no sinks either
    block = _abi.mfa_attention_sinks()
    handle.mfa_attention_sinks_init(ctypes.byref(block))
    assert handle.mfa_attention_decode_softcap_launch_form(ctypes.byref(p), None, 0, ctypes.byref(block), cap, out, len(out)) == 0
    assert out.value.decode() == dec.launchForm(softcap=50.0, **dshape())
    # the ragged entries keep requiring their block
    assert handle.mfa_attention_prefill_ragged_softcap_launch_form(ctypes.byref(pp), 0, None, None, cap, out, len(out)) == INVALID
    assert "null mfa_ragged_rows" in handle.mfa_last_error_string().decode()
