"""What the Python host layer hands to the C ABI for every launch over a KV cache, pinned without a GPU.

Host classes (AttentionDecode, AttentionDecodeFP8, AttentionPrefill, KVCacheAppend): `attention.lib` is replaced by a recording proxy.
Entries ending in `_launch` / `_time` are not called (the proxy answers 0); everything else is called through.  Per call the proxy
records the symbol, the bytes of every ctypes.Structure passed by reference and the integer arguments; the `*_init` helpers run but
are not recorded (the bytes they leave behind are).  The entry each case must reach is a literal here; the recorded calls are the
fixture tests/golden/cache_launch_marshalling.json (the soft cap's cases: cache_launch_marshalling_softcap.json), written by this module's own recorder:

    PYTHONPATH=. python tests/test_cache_launch_marshalling.py        # rewrites the fixture from the sources as they are

Torch layer (the five _run_* functions of torch_binding, and the implementations of the decode ops, which hold the translation of the
ops' spelling of none -- window 0, sink_tokens 0 -- to the None the module uses inside): FakeTensorMode tensors, the host classes' dispatch / workspaceSize replaced
by recorders of their keywords, torch.cuda.device / current_stream stubbed in torch_binding's namespace.
"""
import ctypes
import json
import os

import pytest

from metal_flash_attention_amd import GEMMOperandPrecision as P, MFAError, attention
from metal_flash_attention_amd.attention import AttentionDecode, AttentionDecodeFP8, AttentionPrefill, KVCacheAppend, KVCachePrecision

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cache_launch_marshalling.json")
# The cases of the soft cap (every keyword set and torch case with "softcap" in its name) are a fixture of their own, in the same form.
# GOLDEN is one line of 83 kB: adding to it would rewrite that line, and the bytes recorded before the soft cap existed would no longer
# stand in the history as the proof that the older cases did not move
GOLDEN_SOFTCAP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cache_launch_marshalling_softcap.json")

# fake device pointers: the host never reads what they point to
Q, K, V, O, L = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
LENGTHS, QLENGTHS, LOGITS, STARTS, TABLE, WORKSPACE, KSCALE, VSCALE, STREAM = 0x1000, 0x1100, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x7100, 0x770

_BYREF = type(ctypes.byref(ctypes.c_int()))


class _Recorder:
    """stands in for the loaded library"""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name.endswith("_init"):
            return fn

        def call(*args):
            self.calls.append([name] + [self._describe(a) for a in args])
            return 0 if name.endswith(("_launch", "_time")) else fn(*args)
        return call

    @staticmethod
    def _describe(a):
        if isinstance(a, _BYREF):
            return {"struct": bytes(a._obj).hex()} if isinstance(a._obj, ctypes.Structure) else "out"
        if isinstance(a, ctypes.c_void_p):
            return a.value
        if isinstance(a, ctypes.Array):
            return "buffer"
        if isinstance(a, ctypes.c_float):
            return a.value
        assert a is None or isinstance(a, int), a
        return a


# ---- the cases: (class, keyword set) -> keywords; the methods of the class run over each
DECODE_BASE = dict(rows=1, column=256, heads=4, batches=2, headsPerKeyValue=2, cacheLengths=LENGTHS)
PREFILL_BASE = dict(rows=70, column=256, heads=4, batches=2, headsPerKeyValue=2, cacheLengths=LENGTHS)
APPEND_BASE = dict(rows=3, heads=2, batches=2, column=256, cacheLengths=LENGTHS)
PAGED = dict(pageSize=16, blockTable=TABLE, blockTableStride=20)
RAGGED = dict(rowStarts=STARTS, totalRows=100)

# keyword set -> (keywords, the family of entries an attention launch must reach: the literal between the class's prefix and the method's suffix)
ATTENTION_SETS = {
    "nothing": ({}, ""),
    "window_none": (dict(window=None), ""),
    "window_0": (dict(window=0), "window_"),
    "window_65": (dict(window=65), "window_"),
    "sinks_0_none_beside_window": (dict(sinkTokens=0, sinkLogits=None, window=65), "sink_"),
    "sink_tokens_0_alone": (dict(sinkTokens=0), "sink_"),
    "sink_tokens_window": (dict(sinkTokens=4, window=130), "sink_"),
    "sink_logits_alone": (dict(sinkLogits=LOGITS), "sink_"),
    "paged_page_strides": (dict(PAGED, pageStrides=(2 * 16 * 128 + 256, 2 * 16 * 128 + 512)), ""),
    "paged_packed": (dict(PAGED), ""),
    "paged_window_sinks": (dict(PAGED, window=65, sinkTokens=4, sinkLogits=LOGITS), "sink_"),
    "strides_k_only": (dict(strides=dict(K=(2 * 128, 128, 256 * 2 * 128 + 1024))), ""),
    "strides_q_window": (dict(strides=dict(Q=(256, 128 * 80, 4 * 128 * 80)), window=65), "window_"),
    "l_strides": (dict(lStrides=(96, 4 * 96)), ""),
    "not_causal": (dict(causal=False, sinkLogits=LOGITS), "sink_"),
    "softcap_50": (dict(softcap=50.0), "softcap_"),
    "softcap_0": (dict(softcap=0), "softcap_"),
    "softcap_window": (dict(softcap=50.0, window=65), "softcap_"),
    "softcap_sink_logits": (dict(softcap=50.0, sinkLogits=LOGITS), "softcap_"),
    "softcap_window_sinks": (dict(softcap=50.0, window=65, sinkTokens=4, sinkLogits=LOGITS), "softcap_"),
}
DECODE_ONLY_SETS = {
    "workspace_int": (dict(workspace=WORKSPACE, workspaceBytes=1 << 20), ""),
    "workspace_int_window": (dict(workspace=WORKSPACE, workspaceBytes=1 << 20, window=65), "window_"),
    "rows_4": (dict(rows=4, sinkTokens=4, window=130, sinkLogits=LOGITS), "sink_"),
}
PREFILL_ONLY_SETS = {
    "query_lengths": (dict(queryLengths=QLENGTHS), ""),
    "ragged": (dict(RAGGED), "ragged_"),
    "ragged_window_sinks": (dict(RAGGED, window=65, sinkTokens=4, sinkLogits=LOGITS), "ragged_"),
    "ragged_window_no_sinks": (dict(RAGGED, window=65), "ragged_"),
    "ragged_window_0_sink_0": (dict(RAGGED, window=0, sinkTokens=0), "ragged_"),
    "ragged_total_rows_only": (dict(totalRows=100), "ragged_"),
    "ragged_paged_l_strides": (dict(RAGGED, **PAGED, lStrides=(104, 0), strides=dict(O=(4 * 128 + 64, 128, 0))), "ragged_"),
    "ragged_softcap": (dict(RAGGED, softcap=50.0), "ragged_softcap_"),
    "ragged_softcap_window_sinks": (dict(RAGGED, softcap=50.0, window=65, sinkTokens=4, sinkLogits=LOGITS), "ragged_softcap_"),
}
FP8_SETS = {
    "scales": (dict(keyScale=KSCALE, valueScale=VSCALE), ""),
    "key_scale_window": (dict(keyScale=KSCALE, window=65), "window_"),
    "scales_sinks": (dict(keyScale=KSCALE, valueScale=VSCALE, sinkLogits=LOGITS), "sink_"),
    "scales_softcap": (dict(keyScale=KSCALE, valueScale=VSCALE, softcap=50.0), "softcap_"),
}
APPEND_SETS = {
    "nothing": ({}, ""),
    "paged_page_strides": (dict(PAGED, pageStrides=(2 * 16 * 128, 2 * 16 * 128 + 512), column=0), ""),
    "paged_packed": (dict(PAGED), ""),
    "strides_v_new_only": (dict(strides=dict(vNew=(3 * 128, 128, 2 * 3 * 128 * 3))), ""),
    "scales": (dict(keyScale=KSCALE, valueScale=VSCALE), ""),
    "ragged": (dict(RAGGED), "ragged_"),
    "ragged_paged": (dict(RAGGED, **PAGED, strides=dict(kNew=(3 * 2 * 128, 128, 0))), "ragged_"),
    "ragged_row_starts_only": (dict(rowStarts=STARTS), "ragged_"),
}

SUFFIX = {"workspaceSize": "workspace_size", "launchForm": "launch_form", "dispatch": "launch", "time": "time"}


def _host_classes():
    """name -> (object, base keywords, keyword sets, methods, the entries' prefix, the family a plain launch reaches)"""
    decode_sets = dict(ATTENTION_SETS, **DECODE_ONLY_SETS)
    prefill_sets = dict(ATTENTION_SETS, **PREFILL_ONLY_SETS)
    decode_methods, prefill_methods = ("workspaceSize", "launchForm", "dispatch", "time"), ("launchForm", "dispatch", "time")
    return {
        "decode_bf16_d128": (AttentionDecode(128, P.BF16), DECODE_BASE, decode_sets, decode_methods, "mfa_attention_decode_", ""),
        "decode_f16_d64_f32out": (AttentionDecode(64, P.FP16, P.FP32), DECODE_BASE, {k: decode_sets[k] for k in ("nothing", "window_65", "paged_packed")},
                                  decode_methods, "mfa_attention_decode_", ""),
        "decode_fp8_bf16_d128": (AttentionDecodeFP8(128, P.BF16), DECODE_BASE, dict(decode_sets, **FP8_SETS), decode_methods,
                                 "mfa_attention_decode_", "fp8_"),
        "prefill_bf16_d128": (AttentionPrefill(128, P.BF16), PREFILL_BASE, prefill_sets, prefill_methods, "mfa_attention_prefill_", ""),
        "prefill_e4m3_f16_d64": (AttentionPrefill(64, P.FP16, cachePrecision=KVCachePrecision.E4M3), PREFILL_BASE, dict(prefill_sets, **FP8_SETS),
                                 prefill_methods, "mfa_attention_prefill_", ""),
        "append_bf16_d128": (KVCacheAppend(128, P.BF16), APPEND_BASE, {k: v for k, v in APPEND_SETS.items() if k != "scales"}, ("dispatch",),
                             "mfa_kv_cache_append_", ""),
        "append_e4m3_f16_d64": (KVCacheAppend(64, P.FP16, KVCachePrecision.E4M3), APPEND_BASE, APPEND_SETS, ("dispatch",), "mfa_kv_cache_append_", ""),
    }


def _host_cases():
    for cls, (obj, base, sets, methods, prefix, plain) in _host_classes().items():
        for set_name, (extra, family) in sets.items():
            for method in methods:
                yield f"{cls}/{set_name}/{method}", obj, dict(base, **extra), method, prefix + (family or plain) + SUFFIX[method]


def _run_host_case(obj, keywords, method):
    """the calls one method makes, and what it gave back (or the exception of a shape the library refuses)"""
    recorder = _Recorder(attention._abi.lib())
    saved, attention.lib = attention.lib, lambda: recorder
    try:
        if method == "dispatch" and isinstance(obj, KVCacheAppend):
            result = obj.dispatch(Q, K, V, O, stream=STREAM, **keywords)
        elif method == "dispatch":
            result = obj.dispatch(Q, K, V, O, L, stream=STREAM, **keywords)
        elif method == "time":
            result = obj.time(Q, K, V, O, None, warmup=2, iterations=3, **keywords)
        else:
            result = getattr(obj, method)(**keywords)
    except MFAError:
        result = "MFAError"
    finally:
        attention.lib = saved
    return {"calls": recorder.calls, "result": result}


def record_host(softcap):
    """{class: {keyword set: {method: [the entry's arguments, the method's result]}}}, equal structs stored once: {"struct": index}.
    `softcap`: the cases of GOLDEN_SOFTCAP, else those of GOLDEN"""
    structs, cases = [], {}
    for case, obj, keywords, method, entry in _host_cases():
        if ("softcap" in case) != softcap:
            continue
        got = _run_host_case(obj, keywords, method)
        assert [call[0] for call in got["calls"]] == [entry], (case, got["calls"])
        args = got["calls"][0][1:]
        for i, a in enumerate(args):
            if isinstance(a, dict):
                if a["struct"] not in structs:
                    structs.append(a["struct"])
                args[i] = {"struct": structs.index(a["struct"])}
        cls, set_name, _method = case.split("/")
        cases.setdefault(cls, {}).setdefault(set_name, {})[method] = [args, got["result"]]
    return {"structs": structs, "cases": cases}


@pytest.fixture(scope="module")
def golden():
    """both fixtures as one, the structs of the host cases put back in place of their indices"""
    merged = {"host": {}, "torch": {}}
    for path in (GOLDEN, GOLDEN_SOFTCAP):
        with open(path) as f:
            part = json.load(f)
        for cls, sets in part["host"]["cases"].items():
            for set_name, methods in sets.items():
                for method, (args, result) in methods.items():
                    args = [{"struct": part["host"]["structs"][a["struct"]]} if isinstance(a, dict) else a for a in args]
                    merged["host"].setdefault(cls, {}).setdefault(set_name, {})[method] = [args, result]
        merged["torch"].update(part["torch"])
    return merged


_HOST_CASES = list(_host_cases())


def test_the_fixture_holds_exactly_the_cases(golden):
    cases = golden["host"]
    assert sorted(f"{c}/{s}/{m}" for c in cases for s in cases[c] for m in cases[c][s]) == sorted(case for case, *_ in _HOST_CASES)
    assert sorted(golden["torch"]) == sorted(_TORCH_CASES)


@pytest.mark.parametrize("case,obj,keywords,method,entry", _HOST_CASES, ids=[c[0] for c in _HOST_CASES])
def test_host_class_reaches_the_entry_with_the_bytes(case, obj, keywords, method, entry, golden):
    got = _run_host_case(obj, keywords, method)
    assert [call[0] for call in got["calls"]] == [entry], "one call, to the entry the keywords choose"
    cls, set_name, _method = case.split("/")
    args, result = golden["host"][cls][set_name][method]
    assert json.loads(json.dumps([got["calls"][0][1:], got["result"]])) == [args, result]


def test_documented_routing_rules():
    """0 goes through the window entries; either sink keyword, even 0 / None beside the other, through the sink entries; ragged through the
    ragged entries whichever window and sinks; the sink block of a ragged launch without sink keywords is NULL"""
    entries = {case: entry for case, _o, _k, _m, entry in _HOST_CASES}
    assert entries["decode_bf16_d128/window_0/dispatch"] == "mfa_attention_decode_window_launch"
    assert entries["decode_fp8_bf16_d128/nothing/workspaceSize"] == "mfa_attention_decode_fp8_workspace_size"
    assert entries["decode_fp8_bf16_d128/window_none/time"] == "mfa_attention_decode_fp8_time"
    assert entries["decode_fp8_bf16_d128/window_0/launchForm"] == "mfa_attention_decode_window_launch_form"
    assert entries["decode_bf16_d128/sinks_0_none_beside_window/time"] == "mfa_attention_decode_sink_time"
    assert entries["prefill_bf16_d128/sink_tokens_0_alone/dispatch"] == "mfa_attention_prefill_sink_launch"
    assert entries["prefill_e4m3_f16_d64/ragged_window_sinks/launchForm"] == "mfa_attention_prefill_ragged_launch_form"
    assert entries["append_bf16_d128/ragged/dispatch"] == "mfa_kv_cache_append_ragged_launch"
    obj = AttentionPrefill(128, P.BF16)
    call = _run_host_case(obj, dict(PREFILL_BASE, **RAGGED, window=65), "dispatch")["calls"][0]
    assert call[7:9] == [65, None] and isinstance(call[9], dict)
    call = _run_host_case(obj, dict(PREFILL_BASE, **RAGGED), "dispatch")["calls"][0]
    assert call[7:9] == [0, None]
    call = _run_host_case(AttentionDecode(128, P.BF16), dict(DECODE_BASE, sinkLogits=LOGITS), "dispatch")["calls"][0]
    assert call[7:9] == [None, 0] and isinstance(call[9], dict), "a 16-bit cache: NULL quant, window None -> 0, then the sink block"


# ---- the torch layer
torch = pytest.importorskip("torch")
from torch._subclasses.fake_tensor import FakeTensorMode   # noqa: E402

from metal_flash_attention_amd import torch_binding as tb   # noqa: E402


def _describe_value(v):
    if isinstance(v, torch.Tensor):
        return ["tensor", list(v.shape), str(v.dtype), list(v.stride())]   # (a tensor as the fixture holds it)
    if isinstance(v, dict):
        return {k: _describe_value(x) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return [_describe_value(x) for x in v]
    assert v is None or isinstance(v, (bool, int, float)), v
    return v


class _TorchProxy:
    """torch as torch_binding sees it, with the two calls that need a device stubbed"""

    class cuda:
        class device:
            def __init__(self, device): pass
            def __enter__(self): return self
            def __exit__(self, *exc): return False

        @staticmethod
        def current_stream(device=None):
            class stream:
                cuda_stream = STREAM
            return stream

    def __getattr__(self, name):
        return getattr(torch, name)


def _record_launches(monkeypatch):
    """the keywords the torch layer hands to the host classes, in order; `.need` is what workspaceSize answers"""
    class Log(list):
        need = 0
    log = Log()

    def recorder(cls, method):
        def record(self, *buffers, **keywords):
            log.append({"class": cls.__name__, "method": method, "headDimension": self.headDimension, "precision": int(self.precision),
                        "cachePrecision": getattr(self, "cachePrecision", None), "buffers": _describe_value(buffers),
                        "keywords": _describe_value(keywords)})
            return log.need if method == "workspaceSize" else None
        return record
    for cls in (AttentionDecode, AttentionDecodeFP8):
        monkeypatch.setattr(cls, "workspaceSize", recorder(cls, "workspaceSize"))
    for cls in (AttentionDecode, AttentionDecodeFP8, AttentionPrefill, KVCacheAppend):
        monkeypatch.setattr(cls, "dispatch", recorder(cls, "dispatch"))
    monkeypatch.setattr(tb, "torch", _TorchProxy())
    return log


@pytest.fixture
def launches(monkeypatch):
    return _record_launches(monkeypatch)


def _t(shape, dtype=torch.bfloat16):
    return torch.empty(shape, dtype=dtype, device="cuda")


B, H, HKV, C, D = 2, 4, 2, 256, 128
E4M3 = torch.float8_e4m3fn


def _operands():
    """fake tensors by name (call under FakeTensorMode)"""
    t = {}
    t["q1"], t["q3"], t["q70"] = _t((B, H, 1, D)), _t((B, H, 3, D)), _t((B, H, 70, D))
    t["q3_view"] = _t((B, 3, H, D)).permute(0, 2, 1, 3)                    # token-major: strides passed through
    t["q3_t"] = _t((B, H, D, 3)).transpose(2, 3)                           # last dimension not contiguous: copied
    t["q1_f16_d64"] = _t((B, H, 1, 64), torch.float16)
    t["k"], t["v"] = _t((B, HKV, C, D)), _t((B, HKV, C, D))
    t["k_view"], t["v_view"] = (_t((B, C, 2 * HKV, D)).permute(0, 2, 1, 3)[:, i * HKV:(i + 1) * HKV] for i in (0, 1))   # a fused K|V allocation
    t["k8"], t["v8"] = _t((B, HKV, C, D), E4M3), _t((B, HKV, C, D), E4M3)
    t["k8_d64"], t["v8_d64"] = _t((B, HKV, C, 64), E4M3), _t((B, HKV, C, 64), E4M3)
    t["pool_k"], t["pool_v"] = _t((40, HKV, 16, D)), _t((41, HKV, 16, D))[1:]
    t["pool_k8"], t["pool_v8"] = _t((40, HKV, 16, D), E4M3), _t((40, HKV, 16, D), E4M3)
    t["table"] = _t((B, 24), torch.int32)[:, :16]                          # stride(0) = 24 > its width 16
    t["lens"], t["lens64"] = _t((B,), torch.int32), _t((B,), torch.int64)
    t["qlens"] = _t((B,), torch.int64)
    t["ks"], t["vs"] = _t((HKV,), torch.float32), _t((2 * HKV,), torch.float32)[::2]
    t["logits"], t["logits_h1"] = _t((H,), torch.float32), _t((1,), torch.float32)
    t["starts"] = _t((B + 1,), torch.int32)
    t["kn1"], t["vn1"] = _t((B, HKV, 1, D)), _t((B, HKV, 1, D))
    t["kn3"], t["vn3"] = _t((B, HKV, 3, D)), _t((B, 3, HKV, D)).permute(0, 2, 1, 3)
    t["kn3_t"] = _t((B, HKV, D, 3)).transpose(2, 3)
    t["kn1_f16_d64"] = _t((B, HKV, 1, 64), torch.float16)
    t["qp"], t["qp_t1"], t["qp_h1"] = _t((100, H, D)), _t((1, H, D)), _t((100, 1, D))     # packed rows
    t["qp_odd"] = _t((100, H, D + 4))[:, :, :D]                            # rows not 16-byte multiples apart: copied
    t["knp"], t["vnp"] = _t((100, HKV, D)), _t((100, HKV, D))
    t["knp_t1"], t["vnp_t1"] = _t((1, HKV, D)), _t((1, HKV, D))
    t["knp_h1"], t["vnp_h1"] = _t((100, 1, D)), _t((100, 1, D))
    t["k_h1"], t["v_h1"] = _t((B, 1, C, D)), _t((B, 1, C, D))
    return t


# name -> (function, need, arguments: operand names as strings, everything else as it is)
_TORCH_CASES = {
    "decode/contiguous_r1": ("_run_decode", 0, ("q1", "k", "v", "lens", None, True)),
    "decode/workspace_r3_view_caches_int64_lengths": ("_run_decode", 4096, ("q3_view", "k_view", "v_view", "lens64", None, False)),
    "decode/q_copied": ("_run_decode", 0, ("q3_t", "k", "v", "lens", None, True)),
    "decode/paged_wide_table": ("_run_decode", 0, ("q1", "pool_k", "pool_v", "lens", "table", True)),
    "decode/fp8_scales": ("_run_decode", 0, ("q1", "k8", "v8", "lens", None, True, True, "ks", "vs")),
    "decode/fp8_no_scales_f16_d64": ("_run_decode", 0, ("q1_f16_d64", "k8_d64", "v8_d64", "lens", None, True, True, None, None)),
    "decode/fp8_wrapper": ("op:attention_decode_fp8", 0, ("q1", "pool_k8", "pool_v8", "lens", "table", True, "ks", None)),
    "decode/window": ("_run_decode", 0, ("q1", "k", "v", "lens", None, True, False, None, None, 65)),
    "decode/window_and_sinks": ("_run_decode", 512, ("q3", "k", "v", "lens", None, True, False, None, None, 65, (4, "logits"))),
    "decode/sinks_zero": ("_run_decode", 0, ("q1", "k", "v", "lens", None, True, False, None, None, None, (0, None))),
    "decode/window_wrapper_fp8": ("op:attention_decode_window", 0, ("q1", "k8", "v8", "lens", None, True, "ks", "vs", 65)),
    "decode/sink_wrapper_window_0": ("op:attention_decode_sink", 0, ("q1", "k", "v", "lens", None, True, None, None, 0, 0, "logits")),
    "decode/window_wrapper_softcap": ("op:attention_decode_softcap", 0, ("q1", "k", "v", "lens", None, True, None, None, 0, 0, None, 50.0)),
    "decode/window_wrapper_fp8_window_sinks_softcap": ("op:attention_decode_softcap", 512, ("q3", "k8", "v8", "lens", None, True, "ks", "vs", 65, 4, "logits", 30.0)),
    "prefill/contiguous": ("_run_prefill", 0, ("q70", "k", "v", "lens", None, None, True, None, None)),
    "prefill/r1_query_lengths_view_caches": ("_run_prefill", 0, ("q1", "k_view", "v_view", "lens64", "qlens", None, False, None, None)),
    "prefill/q_copied": ("_run_prefill", 0, ("q3_t", "k", "v", "lens", None, None, True, None, None)),
    "prefill/paged_wide_table_fp8_scales": ("_run_prefill", 0, ("q70", "pool_k8", "pool_v8", "lens", None, "table", True, "ks", "vs")),
    "prefill/fp8_no_scales": ("_run_prefill", 0, ("q70", "k8", "v8", "lens", None, None, True, None, None)),
    "prefill/window_and_sinks": ("_run_prefill", 0, ("q70", "k", "v", "lens", None, None, True, None, None, 65, (4, "logits"))),
    "prefill/window": ("_run_prefill", 0, ("q3_view", "k", "v", "lens", None, None, True, None, None, 65)),
    "prefill/sinks_zero": ("_run_prefill", 0, ("q70", "k", "v", "lens", None, None, True, None, None, None, (0, None))),
    "prefill/softcap": ("_run_prefill", 0, ("q70", "k", "v", "lens", None, None, True, None, None, None, None, 50.0)),
    "prefill/softcap_window_sinks_fp8": ("_run_prefill", 0, ("q70", "k8", "v8", "lens", "qlens", None, True, "ks", None, 65, (4, "logits"), 30.0)),
    "prefill_ragged/softcap": ("_run_prefill_ragged", 0, ("qp", "k", "v", "lens", "starts", 70, None, True, None, None, 0, (0, None), 50.0)),
    "prefill_ragged/softcap_window_sinks": ("_run_prefill_ragged", 0, ("qp", "k", "v", "lens", "starts", 70, None, True, None, None, 65, (4, "logits"), 30.0)),
    "prefill_ragged/contiguous": ("_run_prefill_ragged", 0, ("qp", "k", "v", "lens", "starts", 70, None, True, None, None, 0, (0, None))),
    "prefill_ragged/t1": ("_run_prefill_ragged", 0, ("qp_t1", "k", "v", "lens64", "starts", 1, None, True, None, None, 65, (4, "logits"))),
    "prefill_ragged/h1_view_caches": ("_run_prefill_ragged", 0, ("qp_h1", "k_h1", "v_h1", "lens", "starts", 70, None, False, None, None, 0, (0, "logits_h1"))),
    "prefill_ragged/q_copied_paged_fp8": ("_run_prefill_ragged", 0, ("qp_odd", "pool_k8", "pool_v8", "lens", "starts", 70, "table", True, "ks", "vs", 65, None)),
    "append/contiguous_r1": ("_run_append", 0, ("kn1", "vn1", "k", "v", "lens", None, None, None)),
    "append/r3_view_rows_view_caches": ("_run_append", 0, ("kn3", "vn3", "k_view", "v_view", "lens64", None, None, None)),
    "append/rows_copied": ("_run_append", 0, ("kn3_t", "vn3", "k", "v", "lens", None, None, None)),
    "append/paged_wide_table": ("_run_append", 0, ("kn1", "vn1", "pool_k", "pool_v", "lens", "table", None, None)),
    "append/fp8_scales": ("_run_append", 0, ("kn3", "vn3", "k8", "v8", "lens", None, "ks", "vs")),
    "append/fp8_no_scales_f16_d64": ("_run_append", 0, ("kn1_f16_d64", "kn1_f16_d64", "k8_d64", "v8_d64", "lens", None, None, None)),
    "append_ragged/contiguous": ("_run_append_ragged", 0, ("knp", "vnp", "k", "v", "lens", "starts", 70, None, None, None)),
    "append_ragged/t1_fp8_scales": ("_run_append_ragged", 0, ("knp_t1", "vnp_t1", "k8", "v8", "lens64", "starts", 1, None, "ks", "vs")),
    "append_ragged/h1": ("_run_append_ragged", 0, ("knp_h1", "vnp_h1", "k_h1", "v_h1", "lens", "starts", 70, None, None, None)),
    "append_ragged/paged_wide_table": ("_run_append_ragged", 0, ("knp", "vnp", "pool_k", "pool_v", "lens", "starts", 70, "table", None, None)),
}


def _resolve(arg, t):
    if isinstance(arg, str):
        return t[arg]
    return tuple(_resolve(a, t) for a in arg) if isinstance(arg, tuple) else arg


def _function(name):
    """a function of torch_binding, or with "op:" the implementation of a torch op: what the op runs on the GPU, with the op's spelling
    of none (window 0, sink_tokens 0)"""
    return tb._IMPLS[name[3:]] if name.startswith("op:") else getattr(tb, name)


def _run_torch_case(case, log):
    function, need, args = _TORCH_CASES[case]
    del log[:]
    log.need = need
    with FakeTensorMode():
        t = _operands()
        result = _function(function)(*(_resolve(a, t) for a in args))
    launches = list(log)
    if "decode" in function:   # workspaceSize sees dispatch's keywords without the workspace and the stream: kept once
        assert [x["method"] for x in launches] == ["workspaceSize", "dispatch"] and launches[0]["buffers"] == []
        sized, run = ({k: v for k, v in x.items() if k not in ("method", "buffers", "keywords")} for x in launches)
        assert sized == run and launches[0]["keywords"] == {k: v for k, v in launches[1]["keywords"].items() if k not in ("workspace", "stream")}
    return {"launches": launches[-1:], "result": _describe_value(result)}


@pytest.mark.parametrize("case", sorted(_TORCH_CASES))
def test_torch_layer_hands_the_host_classes_these_keywords(case, launches, golden):
    got = _run_torch_case(case, launches)
    methods = [(x["class"], x["method"]) for x in got["launches"]]
    function, need, args = _TORCH_CASES[case]
    if "decode" in function:
        cls = "AttentionDecodeFP8" if any(isinstance(a, str) and "8" in a for a in args[1:3]) else "AttentionDecode"
        assert methods == [(cls, "dispatch")]
        workspace = got["launches"][0]["keywords"]["workspace"]
        assert workspace == (["tensor", [need], "torch.uint8", [1]] if need else None)
    else:
        assert methods == [("AttentionPrefill" if "prefill" in function else "KVCacheAppend", "dispatch")]
    assert got["launches"][-1]["keywords"]["stream"] == STREAM
    assert json.loads(json.dumps(got)) == golden["torch"][case]


def test_table_stride_for_attention_and_table_width_for_append(launches):
    """attention passes the block table where it lies, with stride(0); append passes a contiguous copy, with its width"""
    assert _run_torch_case("decode/paged_wide_table", launches)["launches"][0]["keywords"]["blockTableStride"] == 24
    assert _run_torch_case("prefill/paged_wide_table_fp8_scales", launches)["launches"][0]["keywords"]["blockTableStride"] == 24
    for case in ("append/paged_wide_table", "append_ragged/paged_wide_table"):
        keywords = _run_torch_case(case, launches)["launches"][0]["keywords"]
        assert keywords["blockTableStride"] == 16 and keywords["blockTable"] == ["tensor", [B, 16], "torch.int32", [16, 1]]
    strides = _run_torch_case("decode/contiguous_r1", launches)["launches"][0]["keywords"]["strides"]
    assert strides["Q"] == [D, D, H * D], "R = 1: the leading dimension is D whatever stride(2) says"


# one refusal of each kind per function: (function, arguments, exception, the substring today's tests match)
_REFUSALS = {
    "decode/cpu_tensor": ("_run_decode", ("q1_cpu", "k", "v", "lens", None, True), RuntimeError, "must live on the GPU"),
    "decode/dtype": ("_run_decode", ("q1_f16", "k", "v", "lens", None, True), TypeError, "must share one of bfloat16 / float16"),
    "decode/fp8_kind": ("_run_decode", ("q1", "k_e5m2", "k_e5m2", "lens", None, True, True), TypeError, "e5m2 and fnuz caches have no kernel"),
    "decode/shape": ("_run_decode", ("q1", "k_h3", "k_h3", "lens", None, True), ValueError, "with H a multiple of Hkv"),
    "decode/cache_lengths": ("_run_decode", ("q1", "k", "v", "lens3", None, True), ValueError, "cache_lengths must be"),
    "decode/last_dimension": ("_run_decode", ("q1", "k_t", "k_t", "lens", None, True), ValueError, "k_cache must have a contiguous last dimension"),
    "decode/block_table": ("_run_decode", ("q1", "pool_k", "pool_v", "lens", "table64", True), ValueError, "block_table must be an int32 GPU tensor"),
    "decode/scale_shape": ("_run_decode", ("q1", "k8", "v8", "lens", None, True, True, "logits", None), ValueError, "k_scale must be float32 [Hkv]"),
    "decode/scale_device": ("_run_decode", ("q1", "k8", "v8", "lens", None, True, True, None, "ks_cpu"), RuntimeError, "v_scale must live on the GPU of the cache"),
    "decode_window/scales_16bit": ("op:attention_decode_window", ("q1", "k", "v", "lens", None, True, "ks", None, 65), ValueError, "go with a float8_e4m3fn cache"),
    "decode_sink/scales_16bit": ("op:attention_decode_sink", ("q1", "k", "v", "lens", None, True, None, "ks", 65, 4, None), ValueError, "go with a float8_e4m3fn cache"),
    "prefill/cpu_tensor": ("_run_prefill", ("q70", "k", "v", "lens_cpu", None, None, True, None, None), RuntimeError, "must live on the GPU"),
    "prefill/dtype": ("_run_prefill", ("q1_f16", "k", "v", "lens", None, None, True, None, None), TypeError, "must share one of bfloat16 / float16"),
    "prefill/q_dtype": ("_run_prefill", ("q1_f32", "k", "v", "lens", None, None, True, None, None), TypeError, "q must be bfloat16 or float16"),
    "prefill/fp8_kind": ("_run_prefill", ("q70", "k_e5m2", "k_e5m2", "lens", None, None, True, None, None), TypeError, "e5m2 and fnuz caches have no kernel"),
    "prefill/scales_16bit": ("_run_prefill", ("q70", "k", "v", "lens", None, None, True, "ks", None), ValueError, "go with a float8_e4m3fn cache"),
    "prefill/shape": ("_run_prefill", ("q70", "k", "k_h3", "lens", None, None, True, None, None), ValueError, "expected q [B, H, R, D]"),
    "prefill/cache_lengths": ("_run_prefill", ("q70", "k", "v", "lens_f", None, None, True, None, None), ValueError, "cache_lengths must be"),
    "prefill/q_lengths": ("_run_prefill", ("q70", "k", "v", "lens", "lens3", None, True, None, None), ValueError, "q_lengths must be"),
    "prefill/last_dimension": ("_run_prefill", ("q70", "k", "k_t", "lens", None, None, True, None, None), ValueError, "v_cache must have a contiguous last dimension"),
    "prefill/block_table": ("_run_prefill", ("q70", "pool_k", "pool_v", "lens", None, "table3", True, None, None), ValueError, "block_table must be an int32 GPU tensor"),
    "prefill/scale_dtype": ("_run_prefill", ("q70", "k8", "v8", "lens", None, None, True, "ks_f16", None), ValueError, "k_scale must be float32 [Hkv]"),
    "prefill_ragged/cpu_tensor": ("_run_prefill_ragged", ("qp_cpu", "k", "v", "lens", "starts", 70, None, True, None, None, 0, None), RuntimeError, "must live on the GPU"),
    "prefill_ragged/dtype": ("_run_prefill_ragged", ("qp", "k_f16", "k_f16", "lens", "starts", 70, None, True, None, None, 0, None), TypeError, "must share one of bfloat16 / float16"),
    "prefill_ragged/scales_16bit": ("_run_prefill_ragged", ("qp", "k", "v", "lens", "starts", 70, None, True, None, "ks", 0, None), ValueError, "go with a float8_e4m3fn cache"),
    "prefill_ragged/shape": ("_run_prefill_ragged", ("q70", "k", "v", "lens", "starts", 70, None, True, None, None, 0, None), ValueError, "expected q [T, H, D] (packed rows)"),
    "prefill_ragged/cache_lengths": ("_run_prefill_ragged", ("qp", "k", "v", "lens3", "starts", 70, None, True, None, None, 0, None), ValueError, "cache_lengths must be a GPU tensor [B]"),
    "prefill_ragged/row_starts": ("_run_prefill_ragged", ("qp", "k", "v", "lens", "lens", 70, None, True, None, None, 0, None), ValueError, "row_starts must be a GPU tensor [B + 1]"),
    "prefill_ragged/max_rows": ("_run_prefill_ragged", ("qp", "k", "v", "lens", "starts", 0, None, True, None, None, 0, None), ValueError, "max_rows must be an int from 1"),
    "prefill_ragged/last_dimension": ("_run_prefill_ragged", ("qp", "k_t", "k_t", "lens", "starts", 70, None, True, None, None, 0, None), ValueError, "k_cache must have a contiguous last dimension"),
    "prefill_ragged/block_table": ("_run_prefill_ragged", ("qp", "pool_k", "pool_v", "lens", "starts", 70, "table_t", True, None, None, 0, None), ValueError, "block_table must be an int32 GPU tensor"),
    "append/cpu_tensor": ("_run_append", ("kn1", "vn1", "k", "v_cpu", "lens", None, None, None), RuntimeError, "must live on the GPU"),
    "append/rows_dtype": ("_run_append", ("kn1", "kn1_f16", "k", "v", "lens", None, None, None), TypeError, "k_new and v_new must share one of bfloat16 / float16"),
    "append/cache_dtype": ("_run_append", ("kn1", "vn1", "k_f16", "k_f16", "lens", None, None, None), TypeError, "the caches must both be torch.float8_e4m3fn or the new rows'"),
    "append/scales_16bit": ("_run_append", ("kn1", "vn1", "k", "v", "lens", None, "ks", None), ValueError, "a 16-bit cache takes the rows' bits"),
    "append/shape": ("_run_append", ("kn1", "vn1", "k_h3", "k_h3", "lens", None, None, None), ValueError, "expected k_new, v_new [B, Hkv, R, D]"),
    "append/cache_lengths": ("_run_append", ("kn1", "vn1", "k", "v", "lens3", None, None, None), ValueError, "cache_lengths must be"),
    "append/last_dimension": ("_run_append", ("kn1", "vn1", "k_t", "k_t", "lens", None, None, None), ValueError, "k_cache must have a contiguous last dimension"),
    "append/block_table": ("_run_append", ("kn1", "vn1", "pool_k", "pool_v", "lens", "table64", None, None), ValueError, "block_table must be an int32 GPU tensor"),
    "append/scale_shape": ("_run_append", ("kn1", "vn1", "k8", "v8", "lens", None, None, "logits"), ValueError, "v_scale must be float32 [Hkv]"),
    "append_ragged/cpu_tensor": ("_run_append_ragged", ("knp", "vnp", "k", "v", "lens_cpu", "starts", 70, None, None, None), RuntimeError, "must live on the GPU"),
    "append_ragged/rows_dtype": ("_run_append_ragged", ("knp_f32", "knp_f32", "k", "v", "lens", "starts", 70, None, None, None), TypeError, "k_new and v_new must share one of bfloat16 / float16"),
    "append_ragged/cache_dtype": ("_run_append_ragged", ("knp", "vnp", "k_e5m2", "k_e5m2", "lens", "starts", 70, None, None, None), TypeError, "e5m2 and fnuz caches have no kernel"),
    "append_ragged/scales_16bit": ("_run_append_ragged", ("knp", "vnp", "k", "v", "lens", "starts", 70, None, None, "ks"), ValueError, "a 16-bit cache takes the rows' bits"),
    "append_ragged/shape": ("_run_append_ragged", ("kn1", "vn1", "k", "v", "lens", "starts", 70, None, None, None), ValueError, "expected k_new, v_new [T, Hkv, D] (packed rows)"),
    "append_ragged/cache_lengths": ("_run_append_ragged", ("knp", "vnp", "k", "v", "lens3", "starts", 70, None, None, None), ValueError, "cache_lengths must be a GPU tensor [B]"),
    "append_ragged/row_starts": ("_run_append_ragged", ("knp", "vnp", "k", "v", "lens", "starts_f", 70, None, None, None), ValueError, "row_starts must be a GPU tensor [B + 1]"),
    "append_ragged/last_dimension": ("_run_append_ragged", ("knp", "vnp", "k", "k_t", "lens", "starts", 70, None, None, None), ValueError, "v_cache must have a contiguous last dimension"),
    "append_ragged/block_table": ("_run_append_ragged", ("knp", "vnp", "pool_k", "pool_v", "lens", "starts", 70, "table3", None, None), ValueError, "block_table must be an int32 GPU tensor"),
}


def _bad_operands(t):
    t["q1_cpu"], t["qp_cpu"] = torch.empty((B, H, 1, D), dtype=torch.bfloat16, device="cpu"), torch.empty((100, H, D), dtype=torch.bfloat16, device="cpu")
    t["v_cpu"], t["lens_cpu"] = torch.empty((B, HKV, C, D), dtype=torch.bfloat16, device="cpu"), torch.empty((B,), dtype=torch.int32, device="cpu")
    t["ks_cpu"] = torch.empty((HKV,), dtype=torch.float32, device="cpu")
    t["q1_f16"], t["q1_f32"], t["kn1_f16"] = _t((B, H, 1, D), torch.float16), _t((B, H, 1, D), torch.float32), _t((B, HKV, 1, D), torch.float16)
    t["knp_f32"] = _t((100, HKV, D), torch.float32)
    t["k_f16"], t["k_e5m2"] = _t((B, HKV, C, D), torch.float16), _t((B, HKV, C, D), torch.float8_e5m2)
    t["k_h3"] = _t((B, 3, C, D))
    t["k_t"] = _t((B, HKV, D, C)).transpose(2, 3)
    t["lens3"], t["lens_f"], t["starts_f"] = _t((3,), torch.int32), _t((B,), torch.float32), _t((B + 1,), torch.float32)
    t["table64"], t["table3"], t["table_t"] = _t((B, 16), torch.int64), _t((3, 16), torch.int32), _t((16, B), torch.int32).t()
    t["ks_f16"] = _t((HKV,), torch.float16)
    return t


@pytest.mark.parametrize("case", sorted(_REFUSALS))
def test_torch_layer_refusals(case, launches):
    function, args, exception, needle = _REFUSALS[case]
    who = {"_run_decode": "flash_decode", "op:attention_decode_window": "flash_decode", "op:attention_decode_sink": "flash_decode", "_run_prefill": "flash_prefill",
           "_run_prefill_ragged": "flash_prefill_ragged", "_run_append": "kv_cache_append", "_run_append_ragged": "kv_cache_append_ragged"}[function]
    with FakeTensorMode():
        t = _bad_operands(_operands())
        with pytest.raises(exception) as raised:
            _function(function)(*(_resolve(a, t) for a in args))
    message = str(raised.value)
    assert type(raised.value) is exception and message.startswith(who + ": ") and needle in message, message
    assert not launches, "nothing is dispatched after a refusal"


def record_torch(softcap):
    mp = pytest.MonkeyPatch()
    try:
        log = _record_launches(mp)
        return {case: json.loads(json.dumps(_run_torch_case(case, log))) for case in sorted(_TORCH_CASES) if ("softcap" in case) == softcap}
    finally:
        mp.undo()


if __name__ == "__main__":
    for path, softcap in ((GOLDEN, False), (GOLDEN_SOFTCAP, True)):
        fixture = {"host": json.loads(json.dumps(record_host(softcap))), "torch": record_torch(softcap)}
        with open(path, "w") as f:
            json.dump(fixture, f, indent=None, separators=(",", ":"), sort_keys=True)
            f.write("\n")
        print(f"wrote {path}: {sum(len(m) for c in fixture['host']['cases'].values() for m in c.values())} host cases, "
              f"{len(fixture['torch'])} torch cases, {os.path.getsize(path)} bytes")
