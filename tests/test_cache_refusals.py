"""What the C entries over a KV cache answer to a bad call, pinned without a GPU: for every entry family of decode and prefill,
`launch_form` (and decode's `workspace_size`) is called with one fault at a time -- one input per refusal of the launches' `prepare`
that needs no GPU, the entries' own null-argument rules -- and with the pairs of faults whose order decides which one speaks.  Per case
the fixture tests/golden/cache_refusals.json holds the status, the message (none for a call that is accepted) and what the
out-parameter holds afterwards (an accepted launch form's text): the entries zero `*bytes` and `out[0]` at different points, and that
is behaviour.  Families that answer a fault alike share one entry.  Written by this module's own recorder:

    PYTHONPATH=. python tests/test_cache_refusals.py        # rewrites the fixture from the sources as they are
"""
import ctypes
import json
import os

import pytest

from metal_flash_attention_amd import _abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cache_refusals.json")

FP32, FP16, BF16, E4M3, E5M2 = 0, 1, 2, _abi.MFA_KV_E4M3, _abi.MFA_KV_E5M2
LENGTHS, QLENGTHS, LOGITS, STARTS, TABLE, WORKSPACE, KSCALE = 0x1000, 0x1100, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000
UNSET_TEXT, UNSET_BYTES = b"unset", 0xDEADBEEF

# launch -> family -> the arguments the family's entries take between `params` and the verb's tail
FAMILIES = {
    "decode": {"": (), "fp8_": ("quant",), "window_": ("quant", "window"), "sink_": ("quant", "window", "sinks"),
               "softcap_": ("quant", "window", "sinks", "softcap")},
    "prefill": {"": (), "window_": ("window",), "sink_": ("window", "sinks"), "ragged_": ("window", "sinks", "ragged"),
                "softcap_": ("window", "sinks", "softcap"), "ragged_softcap_": ("window", "sinks", "ragged", "softcap")},
}
VERBS = {"decode": ("launch_form", "workspace_size"), "prefill": ("launch_form",)}


def _call_spec(launch, family):
    """a call the family accepts: the fields of its params and its own arguments, which a fault then changes"""
    own = FAMILIES[launch][family]
    D, rows, column, heads, batches, G = 128, (1 if launch == "decode" else 70), 256, 4, 2, 2
    ragged = "ragged" in own
    new = (heads * D, D, 0) if ragged else (D, rows * D, heads * rows * D)
    cache = (D, column * D, (heads // G) * column * D)
    spec = dict(rows=rows, column=column, heads=heads, batches=batches, headsPerKeyValue=G, causal=1, headDimension=D, precision=BF16,
                outputPrecision=BF16, pageSize=0, cacheLengths=LENGTHS, blockTable=None, blockTableStride=0,
                leadingDimension=[new[0], cache[0], cache[0], new[0]], headStride=[new[1], cache[1], cache[1], new[1]],
                batchStride=[new[2], cache[2], cache[2], new[2]], pageStride=[0, 0],
                lHeadStride=100 if ragged else rows, lBatchStride=0 if ragged else heads * rows,
                null_params=False, null_out=False, capacity=512)
    if launch == "decode":
        spec.update(workspace=None, workspaceBytes=0)
    else:
        spec.update(cachePrecision=BF16, queryLengths=None, keyScale=None, valueScale=None)
    spec.update(quant=dict(cachePrecision=E4M3, keyScale=None, valueScale=None) if family == "fp8_" else None,
                window=0, sinks=dict(sinkTokens=0, sinkLogits=None) if family == "sink_" else None,
                ragged=dict(rowStarts=STARTS, totalRows=100), softcap=0.0)
    return spec


def _e4m3(spec):
    """the call over an e4m3 cache: decode says so in `quant`, prefill in its params"""
    if "cachePrecision" in spec:
        spec["cachePrecision"] = E4M3
    else:
        spec["quant"] = dict(cachePrecision=E4M3, keyScale=None, valueScale=None)


def _set(**fields):
    return lambda spec: spec.update(fields)


def _at(name, index, value):
    def change(spec):
        spec[name][index] = value
    return change


def _both(*changes):
    def change(spec):
        for c in changes:
            c(spec)
    return change


def _e4m3_and(change):
    return _both(_e4m3, change)


def _quant(**fields):
    return lambda spec: spec.update(quant=dict(dict(cachePrecision=E4M3, keyScale=None, valueScale=None), **fields))


def _ragged(**fields):
    return lambda spec: spec["ragged"].update(fields)


_SINKS = dict(sinkTokens=4, sinkLogits=LOGITS)
_PAGED = dict(pageSize=16, blockTable=TABLE, blockTableStride=16, pageStride=[2 * 16 * 128, 2 * 16 * 128])
_PIECES = dict(column=4096, headStride=[128, 4096 * 128, 4096 * 128, 128], batchStride=[4 * 128, 2 * 4096 * 128, 2 * 4096 * 128, 4 * 128])

# fault -> (the arguments a family must own for the fault to be expressible, the launches it applies to, the change)
FAULTS = {
    "nothing": ((), ("decode", "prefill"), _set()),
    "accepted_window_sinks_cap": (("window", "sinks", "softcap"), ("decode", "prefill"), _set(window=65, sinks=dict(_SINKS), softcap=50.0)),
    "accepted_e4m3_scales": ((), ("prefill",), _both(_e4m3, _set(keyScale=KSCALE))),
    "accepted_quant": (("quant",), ("decode",), _quant(keyScale=KSCALE)),
    "accepted_paged": ((), ("decode", "prefill"), _set(**_PAGED)),
    "accepted_pieces": ((), ("decode",), _set(**_PIECES, workspace=WORKSPACE, workspaceBytes=1 << 24)),
    "accepted_pieces_no_workspace": ((), ("decode",), _set(**_PIECES)),
    # the entries' own rules
    "null_params": ((), ("decode", "prefill"), _set(null_params=True)),
    "null_out": ((), ("decode", "prefill"), _set(null_out=True)),
    "capacity_0": ((), ("decode", "prefill"), _set(capacity=0)),
    "null_quant": (("quant",), ("decode",), _set(quant=None)),
    "null_sinks": (("sinks",), ("decode", "prefill"), _set(sinks=None)),
    "null_ragged": (("ragged",), ("prefill",), _set(ragged=None)),
    "null_sinks_null_out": (("sinks",), ("decode", "prefill"), _set(sinks=None, null_out=True)),
    "null_ragged_null_out": (("ragged",), ("prefill",), _set(ragged=None, null_out=True)),
    "null_quant_null_out": (("quant",), ("decode",), _set(quant=None, null_out=True)),
    "null_params_null_out": ((), ("decode", "prefill"), _set(null_params=True, null_out=True)),
    "null_sinks_null_params": (("sinks",), ("decode", "prefill"), _set(sinks=None, null_params=True)),
    # a ragged block
    "ragged_no_row_starts": (("ragged",), ("prefill",), _ragged(rowStarts=None)),
    "ragged_total_rows_0": (("ragged",), ("prefill",), _ragged(totalRows=0)),
    "ragged_query_lengths": (("ragged",), ("prefill",), _set(queryLengths=QLENGTHS)),
    "ragged_batch_stride_q": (("ragged",), ("prefill",), _at("batchStride", 0, 4 * 128)),
    "ragged_batch_stride_o": (("ragged",), ("prefill",), _at("batchStride", 3, 4 * 128)),
    "ragged_l_batch_stride": (("ragged",), ("prefill",), _set(lBatchStride=400)),
    "ragged_row_blocks": (("ragged",), ("prefill",), _set(batches=1 << 20, rows=1 << 20)),
    "ragged_grid": (("ragged",), ("prefill",), _both(_set(batches=1 << 20, rows=1 << 16, heads=1 << 16), _ragged(totalRows=0xFFFFFFFF))),
    # a window, sinks, a cap
    "sink_tokens_no_window": (("window", "sinks"), ("decode", "prefill"), _set(sinks=dict(_SINKS))),
    "sink_tokens_not_causal": (("window", "sinks"), ("decode", "prefill"), _set(window=65, sinks=dict(_SINKS), causal=0)),
    "window_not_causal": (("window",), ("decode", "prefill"), _set(window=65, causal=0)),
    "softcap_negative": (("softcap",), ("decode", "prefill"), _set(softcap=-1.0)),
    "softcap_nan": (("softcap",), ("decode", "prefill"), _set(softcap=float("nan"))),
    "softcap_inf": (("softcap",), ("decode", "prefill"), _set(softcap=float("inf"))),
    # an e4m3 cache
    "quant_e5m2": (("quant",), ("decode",), _quant(cachePrecision=E5M2)),
    "quant_16bit": (("quant",), ("decode",), _quant(cachePrecision=BF16)),
    "quant_fp32_q": (("quant",), ("decode",), _both(_quant(), _set(precision=FP32))),
    "e4m3_k_stride": ((), ("prefill",), _e4m3_and(_at("leadingDimension", 1, 136))),
    "quant_v_stride": (("quant",), ("decode",), _both(_quant(), _at("headStride", 2, 256 * 128 + 8))),
    "cache_e5m2": ((), ("prefill",), _set(cachePrecision=E5M2)),
    "cache_other_16bit": ((), ("prefill",), _set(cachePrecision=FP16)),
    "scales_16bit_cache": ((), ("prefill",), _set(valueScale=KSCALE)),
    # the shape
    "precision_fp32": ((), ("decode", "prefill"), _set(precision=FP32)),
    "precision_unknown": ((), ("decode", "prefill"), _set(precision=9, cachePrecision=9)),
    "output_precision": ((), ("decode", "prefill"), _set(outputPrecision=FP16)),
    "head_dimension_96": ((), ("decode", "prefill"), _set(headDimension=96)),
    "rows_0": ((), ("decode", "prefill"), _set(rows=0)),
    "batches_0": ((), ("decode", "prefill"), _set(batches=0)),
    "heads_not_a_multiple": ((), ("decode", "prefill"), _set(heads=5)),
    "packed_rows": ((), ("decode",), _set(rows=17)),
    "group_64": ((), ("prefill",), _set(heads=64, headsPerKeyValue=64)),
    "no_cache_lengths": ((), ("decode", "prefill"), _set(cacheLengths=None)),
    "page_size_24": ((), ("decode", "prefill"), _set(**dict(_PAGED, pageSize=24))),
    "page_size_2048": ((), ("decode", "prefill"), _set(**dict(_PAGED, pageSize=2048))),
    "no_block_table": ((), ("decode", "prefill"), _set(**dict(_PAGED, blockTable=None))),
    "block_table_stride": ((), ("decode", "prefill"), _set(**dict(_PAGED, blockTableStride=15))),
    "leading_dimension_q": ((), ("decode", "prefill"), _at("leadingDimension", 0, 64)),
    "stride_k": ((), ("decode", "prefill"), _at("headStride", 1, 256 * 128 + 4)),
    "page_stride_v": ((), ("decode", "prefill"), _set(**dict(_PAGED, pageStride=[2 * 16 * 128, 2 * 16 * 128 + 4]))),
    "stride_o": ((), ("decode", "prefill"), _at("leadingDimension", 3, 130)),
    "grid": ((), ("prefill",), _set(batches=1 << 20, heads=4096)),
    "workspace_small": ((), ("decode",), _set(**_PIECES, workspace=WORKSPACE, workspaceBytes=16)),
    "workspace_misaligned": ((), ("decode",), _set(**_PIECES, workspace=WORKSPACE + 8, workspaceBytes=1 << 24)),
    # two faults: today's order decides which one speaks
    "window_not_causal_and_precision_fp32": (("window",), ("decode", "prefill"), _set(window=65, causal=0, precision=FP32)),
    "quant_16bit_and_head_dimension_96": (("quant",), ("decode",), _both(_quant(cachePrecision=BF16), _set(headDimension=96))),
    "quant_v_stride_and_rows_0": (("quant",), ("decode",), _both(_quant(), _at("headStride", 2, 256 * 128 + 8), _set(rows=0))),
    "e4m3_k_stride_and_no_cache_lengths": ((), ("prefill",), _e4m3_and(_both(_at("leadingDimension", 1, 136), _set(cacheLengths=None)))),
    "ragged_no_row_starts_and_softcap_negative": (("ragged", "softcap"), ("prefill",), _both(_ragged(rowStarts=None), _set(softcap=-1.0))),
    "null_ragged_and_softcap_negative": (("ragged", "softcap"), ("prefill",), _set(ragged=None, softcap=-1.0)),
    "softcap_negative_and_head_dimension_96": (("softcap",), ("decode", "prefill"), _set(softcap=-1.0, headDimension=96)),
    "softcap_nan_and_sink_tokens_no_window": (("softcap", "sinks", "window"), ("decode", "prefill"), _set(softcap=float("nan"), sinks=dict(_SINKS))),
}


def _struct(cls, fields):
    s = cls()
    for name, value in fields.items():
        if isinstance(value, list):
            for i, v in enumerate(value):
                getattr(s, name)[i] = v
        elif name in dict(cls._fields_):
            setattr(s, name, value)
    return s


def _cases():
    for launch, families in FAMILIES.items():
        for family, own in families.items():
            for verb in VERBS[launch]:
                faults = [f for f, (needs, launches, _c) in FAULTS.items() if launch in launches and set(needs) <= set(own)]
                yield f"{launch}/{family or 'plain'}/{verb}", launch, family, verb, faults


def _run(launch, family, verb, fault):
    """-> [status, the message of a refusal or the text of a launch form (None: neither), the out-parameter afterwards]"""
    lib = _abi.lib()
    spec = _call_spec(launch, family)
    FAULTS[fault][2](spec)
    params = _struct(_abi.mfa_decode_params if launch == "decode" else _abi.mfa_prefill_params, spec)
    blocks = {"quant": _abi.mfa_kv_quant, "sinks": _abi.mfa_attention_sinks, "ragged": _abi.mfa_ragged_rows}
    own = []
    for name in FAMILIES[launch][family]:
        if name in blocks:
            own.append(None if spec[name] is None else ctypes.byref(_struct(blocks[name], spec[name])))
        else:
            own.append(ctypes.c_float(spec[name]) if name == "softcap" else int(spec[name]))
    p = None if spec["null_params"] else ctypes.byref(params)
    entry = getattr(lib, f"mfa_attention_{launch}_{family}{verb}")
    if verb == "workspace_size":
        out = ctypes.c_uint64(UNSET_BYTES)
        status = entry(p, *own, None if spec["null_out"] else ctypes.byref(out))
        left = "unset" if out.value == UNSET_BYTES else int(out.value)
        return [status, lib.mfa_last_error_string().decode() if status else None, left]
    out = ctypes.create_string_buffer(UNSET_TEXT, 512)
    status = entry(p, *own, None if spec["null_out"] else out, spec["capacity"])
    return [status, lib.mfa_last_error_string().decode() if status else None, out.value.decode()]


def record():
    """{"<launch>/<verb>": {fault: [[the families that answer alike, status, message, out-parameter], ...]}}: most faults are answered in
    the same words by every family that can express them"""
    fixture = {}
    for _case, launch, family, verb, faults in _cases():
        for fault in faults:
            answer = json.loads(json.dumps(_run(launch, family, verb, fault)))
            groups = fixture.setdefault(f"{launch}/{verb}", {}).setdefault(fault, [])
            alike = [g for g in groups if g[1:] == answer]
            if alike:
                alike[0][0].append(family)
            else:
                groups.append([[family]] + answer)
    return fixture


@pytest.fixture(scope="module")
def golden():
    """-> {"<launch>/<family or plain>/<verb>": {fault: [status, message, out-parameter]}}"""
    with open(GOLDEN) as f:
        grouped = json.load(f)
    flat = {}
    for key, faults in grouped.items():
        launch, verb = key.split("/")
        for fault, groups in faults.items():
            for families, *answer in groups:
                for family in families:
                    flat.setdefault(f"{launch}/{family or 'plain'}/{verb}", {})[fault] = answer
    return flat


_CASES = list(_cases())


def test_the_fixture_holds_exactly_the_cases(golden):
    assert {case: sorted(faults) for case, _l, _f, _v, faults in _CASES} == {case: sorted(golden[case]) for case in golden}


def test_the_table_reaches_every_family_and_both_answers(golden):
    """every family is refused and accepted at least once, and the faults of one family do not all speak with one voice"""
    for case, answers in golden.items():
        statuses = {a[0] for a in answers.values()}
        assert 0 in statuses and 2 in statuses and 3 in statuses, case
        assert len({a[1] for a in answers.values() if a[0]}) >= 15, case   # (the plain entries meet 17 refusals of the shape alone)
    assert golden["decode/sink_/launch_form"]["null_sinks"][0] == 2 and golden["prefill/sink_/launch_form"]["null_sinks"][0] == 2
    for case in ("decode/softcap_/launch_form", "prefill/softcap_/launch_form", "prefill/ragged_/launch_form", "prefill/ragged_softcap_/launch_form"):
        assert golden[case]["null_sinks"][0] == 0, "a NULL sinks block is no sinks on the ragged and soft-cap entries"


@pytest.mark.parametrize("case,launch,family,verb,faults", _CASES, ids=[c[0] for c in _CASES])
def test_entry_answers_each_fault_as_recorded(case, launch, family, verb, faults, golden):
    for fault in faults:
        assert json.loads(json.dumps(_run(launch, family, verb, fault))) == golden[case][fault], (case, fault)


if __name__ == "__main__":
    fixture = record()
    with open(GOLDEN, "w") as f:   # a fault a line
        f.write("{\n" + ",\n".join(json.dumps(key) + ":{\n" + ",\n".join(json.dumps(fault) + ":" + json.dumps(groups, separators=(",", ":"))
                                                                           for fault, groups in sorted(faults.items())) + "\n}"
                                   for key, faults in sorted(fixture.items())) + "\n}\n")
    print(f"wrote {GOLDEN}: {sum(len(g[0]) for faults in fixture.values() for groups in faults.values() for g in groups)} answers in "
          f"{sum(len(groups) for faults in fixture.values() for groups in faults.values())} groups, {os.path.getsize(GOLDEN)} bytes")
