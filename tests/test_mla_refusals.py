"""What the C entries of the MLA attention launches answer to a bad call, pinned without a GPU: for each of the nine entry families
(decode and prefill, dense and sparse, 16-bit and e4m3 caches, unsplit and cut) every verb -- `launch_form`, `workspace_size` where the
family has one, `launch` and `time` -- is called with one fault at a time, with the pairs of faults whose order decides which one
speaks, and with calls it accepts.  Per case the fixture tests/golden/mla_refusals.json holds the status, the message (an accepted
launch form: its text) and what the out-parameters hold afterwards (`out`; `*bytes` and `*pieces`): the entries zero them at different
points, and that is behaviour.  `launch` and `time` are always called with null buffers, so that a call whose params and blocks pass
is refused by the bind and nothing reaches a kernel launch.  Families that answer a fault alike share one entry.  Written by this
module's own recorder:

    PYTHONPATH=. python tests/test_mla_refusals.py        # rewrites the fixture from the sources as they are
"""
import ctypes
import json
import os

import pytest

from metal_flash_attention_amd import _abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mla_refusals.json")

FP32, FP16, BF16, E4M3, E5M2 = 0, 1, 2, _abi.MFA_KV_E4M3, _abi.MFA_KV_E5M2
LENGTHS, QLENGTHS, INDICES, TABLE, WORKSPACE, KVSCALE = 0x1000, 0x1100, 0x3000, 0x5000, 0x6000, 0x7000
UNSET_TEXT, UNSET = b"unset", 0xDEADBEEF
DK, DV = _abi.MFA_MLA_HEAD_DIMENSION, _abi.MFA_MLA_VALUE_DIMENSION

# family (mfa_attention_mla_<family>_<verb>) -> (its params, the blocks its entries take after `params`, in their order)
FAMILIES = {
    "decode": ("decode", ()),
    "decode_fp8": ("decode", ("quant",)),
    "sparse_decode": ("decode", ("sparse",)),
    "sparse_decode_fp8": ("decode", ("sparse", "quant")),
    "prefill": ("prefill", ()),
    "prefill_split": ("prefill", ("split",)),
    "prefill_fp8": ("prefill", ("quant",)),
    "prefill_fp8_split": ("prefill", ("split", "quant")),
    "prefill_sparse": ("prefill", ("sparse",)),
}
FORM, SIZE, LAUNCH, TIME = "launch_form", "workspace_size", "launch", "time"
EVERY = (FORM, SIZE, LAUNCH, TIME)


def _owns(family):
    """what a fault may ask of a family: its params, its blocks, and a workspace (decode's params name one, prefill's split block)"""
    kind, blocks = FAMILIES[family]
    return {kind, *blocks} | ({"workspace"} if kind == "decode" or "split" in blocks else set())


def _verbs(family):
    return tuple(v for v in EVERY if v != SIZE or "workspace" in _owns(family))


def _call_spec(family):
    """a call the family accepts, unsplit: the fields of its params and blocks, which a fault then changes.  `pieces`, `workspace` and
    `workspaceBytes` go where the family keeps them: decode's params, or the split block"""
    kind, _blocks = FAMILIES[family]
    rows, column, heads, batches = (2, 256, 16, 2) if kind == "decode" else (70, 256, 4, 2)
    spec = dict(rows=rows, column=column, heads=heads, batches=batches, causal=1, headDimension=DK, valueDimension=DV, precision=BF16,
                outputPrecision=BF16, scale=0.125, pageSize=0, cacheLengths=LENGTHS, queryLengths=None, blockTable=None, blockTableStride=0,
                leadingDimension=[heads * DK, DK, heads * DV], headStride=[DK, 0, DV],
                batchStride=[rows * heads * DK, column * DK, rows * heads * DV], pageStride=0,
                lHeadStride=1, lBatchStride=rows * heads, pieces=0, workspace=None, workspaceBytes=0,
                quant=dict(cachePrecision=E4M3, reserved=0, kvScale=None),
                sparse=dict(indices=INDICES, topk=64, reserved=0, indexRowStride=64, indexBatchStride=rows * 64),
                null_split=False, split_reserved=0,
                null_params=False, null_out=False, capacity=512, null_bytes=False, null_pieces=False, warmup=0, iterations=1, null_ms=False)
    return spec


def _set(**fields):
    return lambda spec: spec.update(fields)


def _at(name, index, value):
    def change(spec):
        spec[name][index] = value
    return change


def _in(block, **fields):
    return lambda spec: spec[block].update(fields)


def _both(*changes):
    def change(spec):
        for c in changes:
            c(spec)
    return change


def _paged(**fields):
    return _set(**dict(dict(pageSize=16, blockTable=TABLE, blockTableStride=16, pageStride=16 * DK), **fields))


def _long(spec):
    """few workgroups over many keys (and long lists): every plan cuts"""
    spec.update(column=8192, batchStride=[spec["batchStride"][0], 8192 * DK, spec["batchStride"][2]])
    spec["sparse"].update(topk=2048, indexRowStride=2048, indexBatchStride=spec["rows"] * 2048)


_ROOMY = _set(workspace=WORKSPACE, workspaceBytes=1 << 30)
_CUT = _both(_long, _ROOMY)
_HEAD_96 = _set(headDimension=96)
_QUANT_16BIT = _in("quant", cachePrecision=BF16)
_TOPK_0 = _in("sparse", topk=0)
_PIECES_65 = _set(pieces=65)
_KV_STRIDE_8 = _at("leadingDimension", 1, DK + 8)

# fault -> (what a family must own for the fault to be expressible, the verbs it is put to, the change)
FAULTS = {
    # accepted calls
    "nothing": ((), (FORM, SIZE), _set()),
    "accepted_cut": (("workspace",), (FORM, SIZE), _CUT),
    "accepted_no_workspace": (("workspace",), (FORM, SIZE), _long),
    "accepted_pieces_4": (("workspace",), (FORM, SIZE), _both(_set(pieces=4), _ROOMY)),
    "accepted_pieces_1": (("workspace",), (FORM, SIZE), _both(_long, _ROOMY, _set(pieces=1))),
    "accepted_paged": ((), (FORM, SIZE), _paged()),
    "accepted_paged_cut": (("workspace",), (FORM, SIZE), _both(_CUT, _paged(blockTableStride=512))),
    "accepted_fp16_out_f32": ((), (FORM, SIZE), _set(precision=FP16, outputPrecision=FP32, causal=0)),
    "accepted_kv_scale": (("quant",), (FORM, SIZE), _in("quant", kvScale=KVSCALE)),
    "accepted_query_lengths": (("prefill",), (FORM, SIZE), _set(queryLengths=QLENGTHS)),
    "accepted_rows_32": (("decode",), (FORM, SIZE), _set(rows=32)),
    "accepted_heads_70": ((), (FORM, SIZE), _set(heads=70)),
    "accepted_null_pieces_out": (("workspace",), (SIZE,), _both(_long, _set(null_pieces=True))),
    "bound_null_buffers": ((), (LAUNCH, TIME), _set()),
    "bound_null_buffers_cut": (("workspace",), (LAUNCH, TIME), _CUT),
    # the params
    "null_params": ((), EVERY, _set(null_params=True)),
    "precision_fp32": ((), EVERY, _set(precision=FP32)),
    "precision_unknown": ((), EVERY, _set(precision=9)),
    "output_precision": ((), EVERY, _set(outputPrecision=FP16)),
    "head_dimension_96": ((), EVERY, _HEAD_96),
    "value_dimension_256": ((), EVERY, _set(valueDimension=256)),
    "scale_0": ((), EVERY, _set(scale=0.0)),
    "scale_negative": ((), EVERY, _set(scale=-0.125)),
    "scale_inf": ((), EVERY, _set(scale=float("inf"))),
    "scale_nan": ((), EVERY, _set(scale=float("nan"))),
    "rows_0": ((), EVERY, _set(rows=0)),
    "column_0": ((), EVERY, _set(column=0)),
    "heads_0": ((), EVERY, _set(heads=0)),
    "batches_0": ((), EVERY, _set(batches=0)),
    "rows_33": (("decode",), EVERY, _set(rows=33)),
    "pieces_65": (("workspace",), EVERY, _PIECES_65),
    "no_cache_lengths": ((), EVERY, _set(cacheLengths=None)),
    # the layout and the grid
    "page_size_24": ((), EVERY, _paged(pageSize=24)),
    "page_size_8": ((), EVERY, _paged(pageSize=8)),
    "page_size_2048": ((), EVERY, _paged(pageSize=2048)),
    "no_block_table": ((), EVERY, _paged(blockTable=None)),
    "block_table_stride": ((), EVERY, _paged(blockTableStride=15)),
    "leading_dimension_q": ((), EVERY, _at("leadingDimension", 0, 512)),
    "leading_dimension_kv": ((), EVERY, _at("leadingDimension", 1, 512)),
    "leading_dimension_o": ((), EVERY, _at("leadingDimension", 2, 256)),
    "stride_q": ((), EVERY, _at("headStride", 0, DK + 4)),
    "stride_kv": ((), EVERY, _at("batchStride", 1, 256 * DK + 4)),
    "page_stride_kv": ((), EVERY, _paged(pageStride=16 * DK + 4)),
    "stride_o": ((), EVERY, _at("batchStride", 2, 2 * 16 * DV + 2)),
    "stride_o_4": ((), (FORM,), _at("headStride", 2, DV + 4)),   # (whole 4-element stores: accepted)
    "grid": ((), EVERY, _set(batches=1 << 20, heads=1 << 16, rows=32)),
    "grid_sparse": (("sparse",), EVERY, _set(batches=1 << 20, heads=1, rows=32)),
    "grid_sparse_prefill": (("sparse", "prefill"), EVERY, _set(batches=1 << 19, heads=1, rows=1 << 12)),
    "grid_cut": (("split",), EVERY, _both(_long, _set(batches=1 << 26, heads=64, rows=1, pieces=64, workspace=WORKSPACE, workspaceBytes=1 << 62))),
    # the sparse block
    "null_sparse": (("sparse",), EVERY, _set(sparse=None)),
    "sparse_no_indices": (("sparse",), EVERY, _in("sparse", indices=None)),
    "sparse_topk_0": (("sparse",), EVERY, _TOPK_0),
    "sparse_reserved": (("sparse",), EVERY, _in("sparse", reserved=7)),
    "sparse_index_row_stride": (("sparse",), EVERY, _in("sparse", indexRowStride=63)),
    "sparse_indices_misaligned": (("sparse",), EVERY, _in("sparse", indices=INDICES + 2)),
    # the quant block
    "null_quant": (("quant",), EVERY, _set(quant=None)),
    "quant_16bit": (("quant",), EVERY, _QUANT_16BIT),
    "quant_unknown": (("quant",), EVERY, _in("quant", cachePrecision=9)),
    "quant_e5m2": (("quant",), EVERY, _in("quant", cachePrecision=E5M2)),
    "quant_reserved": (("quant",), EVERY, _in("quant", reserved=7)),   # (refused by prefill, accepted by decode)
    "quant_kv_stride_8": (("quant",), EVERY, _KV_STRIDE_8),
    "quant_kv_page_stride_8": (("quant",), EVERY, _paged(pageStride=16 * DK + 8)),
    "quant_fp32_q": (("quant",), EVERY, _set(precision=FP32)),
    "quant_kv_scale_misaligned": (("quant",), (FORM, LAUNCH, TIME), _in("quant", kvScale=KVSCALE + 2)),
    # the split block
    "null_split": (("split",), EVERY, _set(null_split=True)),
    "split_reserved": (("split",), EVERY, _set(split_reserved=7)),
    # the workspace, while the plan cuts
    "workspace_no_bytes": (("workspace",), EVERY, _both(_long, _set(workspace=WORKSPACE))),
    "workspace_short": (("workspace",), EVERY, _both(_long, _set(workspace=WORKSPACE, workspaceBytes=4096))),
    "workspace_misaligned": (("workspace",), EVERY, _both(_long, _set(workspace=WORKSPACE + 8, workspaceBytes=1 << 30))),
    "workspace_short_pieces_2": (("workspace",), EVERY, _set(pieces=2, workspace=WORKSPACE, workspaceBytes=4096)),
    # the out-parameters and the timing arguments
    "null_out": ((), (FORM,), _set(null_out=True)),
    "capacity_0": ((), (FORM,), _set(capacity=0)),
    "capacity_8": ((), (FORM,), _set(capacity=8)),
    "null_bytes": (("workspace",), (SIZE,), _set(null_bytes=True)),
    "timing_null_milliseconds": ((), (TIME,), _set(null_ms=True)),
    "timing_iterations_0": ((), (TIME,), _set(iterations=0)),
    "timing_warmup_negative": ((), (TIME,), _set(warmup=-1)),
    # two faults: today's order decides which one speaks
    "sparse_topk_0_and_quant_16bit": (("sparse", "quant"), EVERY, _both(_TOPK_0, _QUANT_16BIT)),
    "null_sparse_and_null_quant": (("sparse", "quant"), EVERY, _set(sparse=None, quant=None)),
    "sparse_topk_0_and_head_dimension_96": (("sparse",), EVERY, _both(_TOPK_0, _HEAD_96)),
    "null_sparse_and_null_params": (("sparse",), EVERY, _set(sparse=None, null_params=True)),
    "quant_16bit_and_head_dimension_96": (("quant",), EVERY, _both(_QUANT_16BIT, _HEAD_96)),
    "null_quant_and_null_params": (("quant",), EVERY, _set(quant=None, null_params=True)),
    "quant_kv_stride_8_and_rows_0": (("quant",), EVERY, _both(_KV_STRIDE_8, _set(rows=0))),
    "quant_kv_stride_8_and_no_cache_lengths": (("quant",), EVERY, _both(_KV_STRIDE_8, _set(cacheLengths=None))),
    "quant_kv_stride_8_and_leading_dimension_q": (("quant",), EVERY, _both(_KV_STRIDE_8, _at("leadingDimension", 0, 512))),
    "split_pieces_65_and_head_dimension_96": (("split",), EVERY, _both(_PIECES_65, _HEAD_96)),
    "null_split_and_null_params": (("split",), EVERY, _set(null_split=True, null_params=True)),
    "sparse_topk_0_and_null_out": (("sparse",), (FORM,), _both(_TOPK_0, _set(null_out=True))),
    "sparse_topk_0_and_capacity_0": (("sparse",), (FORM,), _both(_TOPK_0, _set(capacity=0))),
    "quant_16bit_and_null_out": (("quant",), (FORM,), _both(_QUANT_16BIT, _set(null_out=True))),
    "split_pieces_65_and_null_out": (("split",), (FORM,), _both(_PIECES_65, _set(null_out=True))),
    "head_dimension_96_and_null_out": ((), (FORM,), _both(_HEAD_96, _set(null_out=True))),
    "null_params_and_null_out": ((), (FORM,), _set(null_params=True, null_out=True)),
    "sparse_topk_0_and_null_bytes": (("sparse", "workspace"), (SIZE,), _both(_TOPK_0, _set(null_bytes=True))),
    "quant_16bit_and_null_bytes": (("quant", "workspace"), (SIZE,), _both(_QUANT_16BIT, _set(null_bytes=True))),
    "split_pieces_65_and_null_bytes": (("split",), (SIZE,), _both(_PIECES_65, _set(null_bytes=True))),
    "head_dimension_96_and_null_bytes": (("workspace",), (SIZE,), _both(_HEAD_96, _set(null_bytes=True))),
    "null_params_and_null_bytes": (("workspace",), (SIZE,), _set(null_params=True, null_bytes=True)),
    "head_dimension_96_and_workspace_short": (("workspace",), EVERY, _both(_long, _HEAD_96, _set(workspace=WORKSPACE, workspaceBytes=4096))),
    "stride_o_and_workspace_short": (("workspace",), EVERY, _both(_long, _at("batchStride", 2, 2 * 16 * DV + 2),
                                                                   _set(workspace=WORKSPACE, workspaceBytes=4096))),
    "grid_sparse_and_workspace_short": (("sparse", "workspace"), EVERY, _both(_long, _set(batches=1 << 20, heads=1, rows=32, workspace=WORKSPACE,
                                                                                         workspaceBytes=4096))),
    "quant_16bit_and_split_pieces_65": (("quant", "split"), EVERY, _both(_QUANT_16BIT, _PIECES_65)),
    "quant_reserved_and_null_split": (("quant", "split"), EVERY, _both(_in("quant", reserved=7), _set(null_split=True))),
    "quant_kv_stride_8_and_split_reserved": (("quant", "split"), EVERY, _both(_KV_STRIDE_8, _set(split_reserved=7))),
    "timing_iterations_0_and_null_params": ((), (TIME,), _set(iterations=0, null_params=True)),
    "timing_iterations_0_and_sparse_topk_0": (("sparse",), (TIME,), _both(_TOPK_0, _set(iterations=0))),
    "timing_iterations_0_and_quant_16bit": (("quant",), (TIME,), _both(_QUANT_16BIT, _set(iterations=0))),
    "timing_iterations_0_and_null_split": (("split",), (TIME,), _set(iterations=0, null_split=True)),
}


def _struct(cls, fields):
    s = cls()
    for name, value in fields.items():
        if name not in dict(cls._fields_):
            continue
        if isinstance(value, list):
            for i, v in enumerate(value):
                getattr(s, name)[i] = v
        else:
            setattr(s, name, value)
    return s


def _cases():
    for family in FAMILIES:
        for verb in _verbs(family):
            faults = [f for f, (needs, verbs, _c) in FAULTS.items() if verb in verbs and set(needs) <= _owns(family)]
            yield f"{family}/{verb}", family, verb, faults


def _run(family, verb, fault):
    """-> [status, the message of a refusal or the text of a launch form (None: neither), the out-parameters afterwards]"""
    lib = _abi.lib()
    kind, blocks = FAMILIES[family]
    spec = _call_spec(family)
    FAULTS[fault][2](spec)
    params = _struct(_abi.mfa_mla_decode_params if kind == "decode" else _abi.mfa_mla_prefill_params, spec)
    made = {"quant": None if spec["quant"] is None else _struct(_abi.mfa_mla_quant, spec["quant"]),
            "sparse": None if spec["sparse"] is None else _struct(_abi.mfa_mla_sparse, spec["sparse"]),
            "split": None if spec["null_split"] else _struct(_abi.mfa_key_split, dict(spec, reserved=spec["split_reserved"]))}
    own = [None if made[name] is None else ctypes.byref(made[name]) for name in blocks]
    p = None if spec["null_params"] else ctypes.byref(params)
    entry = getattr(lib, f"mfa_attention_mla_{family}_{verb}")
    message = lambda status: lib.mfa_last_error_string().decode() if status else None
    if verb == SIZE:
        size, pieces = ctypes.c_uint64(UNSET), ctypes.c_uint32(UNSET)
        status = entry(p, *own, None if spec["null_bytes"] else ctypes.byref(size), None if spec["null_pieces"] else ctypes.byref(pieces))
        return [status, message(status), ["unset" if x.value == UNSET else int(x.value) for x in (size, pieces)]]
    if verb == FORM:
        out = ctypes.create_string_buffer(UNSET_TEXT, 512)
        status = entry(p, *own, None if spec["null_out"] else out, spec["capacity"])
        return [status, message(status), out.value.decode()]
    if verb == LAUNCH:   # (null buffers: nothing the params and blocks let through reaches a kernel)
        status = entry(None, None, None, None, p, *own, None)
        assert status != 0, (family, fault)
        return [status, message(status), None]
    ms = ctypes.c_float(-1.0)
    status = entry(None, None, None, None, p, *own, None, spec["warmup"], spec["iterations"], None if spec["null_ms"] else ctypes.byref(ms))
    assert status != 0 and ms.value == -1.0, (family, fault)
    return [status, message(status), None]


def record():
    """{verb: {fault: [[the families that answer alike, status, message, out-parameters], ...]}}: many faults are answered in the same
    words by every family that can express them"""
    fixture = {}
    for _case, family, verb, faults in _cases():
        for fault in faults:
            answer = json.loads(json.dumps(_run(family, verb, fault)))
            groups = fixture.setdefault(verb, {}).setdefault(fault, [])
            alike = [g for g in groups if g[1:] == answer]
            if alike:
                alike[0][0].append(family)
            else:
                groups.append([[family]] + answer)
    return fixture


@pytest.fixture(scope="module")
def golden():
    """-> {"<family>/<verb>": {fault: [status, message, out-parameters]}}"""
    with open(GOLDEN) as f:
        grouped = json.load(f)
    flat = {}
    for verb, faults in grouped.items():
        for fault, groups in faults.items():
            for families, *answer in groups:
                for family in families:
                    flat.setdefault(f"{family}/{verb}", {})[fault] = answer
    return flat


_CASES = list(_cases())


def test_the_fixture_holds_exactly_the_cases(golden):
    assert {case: sorted(faults) for case, _f, _v, faults in _CASES} == {case: sorted(golden[case]) for case in golden}


def test_the_table_reaches_every_family_and_both_answers(golden):
    """every family is accepted at least once (by the verbs that can accept without a GPU) and refused with both statuses by every verb"""
    assert {case.split("/")[0] for case in golden} == set(FAMILIES)
    for case, answers in golden.items():
        statuses = {a[0] for a in answers.values()}
        assert 2 in statuses and 3 in statuses, case
        assert (0 in statuses) == (case.split("/")[1] in (FORM, SIZE)), case
        assert len({a[1] for a in answers.values() if a[0]}) >= 15, case
    # the difference between the two quant checks that is behaviour
    assert golden["decode_fp8/launch_form"]["quant_reserved"][0] == 0 and golden["sparse_decode_fp8/launch_form"]["quant_reserved"][0] == 0
    assert golden["prefill_fp8/launch_form"]["quant_reserved"][0] == 2 and golden["prefill_fp8_split/launch_form"]["quant_reserved"][0] == 2
    # every plan that can cut does, runs unsplit without a workspace, and says how many bytes the cut needs
    for family in FAMILIES:
        if "workspace" in _owns(family):
            cut = golden[f"{family}/launch_form"]["accepted_cut"][2]
            assert " pieces" in cut and "_combine" in cut
            assert "unsplit without a workspace" in golden[f"{family}/launch_form"]["accepted_no_workspace"][2]
            size, pieces = golden[f"{family}/workspace_size"]["accepted_no_workspace"][2]
            assert pieces > 1 and size > 0
            assert golden[f"{family}/workspace_size"]["nothing"][2] == [0, 1]
        assert "paged" in golden[f"{family}/launch_form"]["accepted_paged"][2]


@pytest.mark.parametrize("case,family,verb,faults", _CASES, ids=[c[0] for c in _CASES])
def test_entry_answers_each_fault_as_recorded(case, family, verb, faults, golden):
    for fault in faults:
        assert json.loads(json.dumps(_run(family, verb, fault))) == golden[case][fault], (case, fault)


if __name__ == "__main__":
    fixture = record()
    with open(GOLDEN, "w") as f:   # a fault a line
        f.write("{\n" + ",\n".join(json.dumps(verb) + ":{\n" + ",\n".join(json.dumps(fault) + ":" + json.dumps(groups, separators=(",", ":"))
                                                                            for fault, groups in sorted(faults.items())) + "\n}"
                                   for verb, faults in sorted(fixture.items())) + "\n}\n")
    print(f"wrote {GOLDEN}: {sum(len(g[0]) for faults in fixture.values() for groups in faults.values() for g in groups)} answers in "
          f"{sum(len(groups) for faults in fixture.values() for groups in faults.values())} groups, {os.path.getsize(GOLDEN)} bytes")
