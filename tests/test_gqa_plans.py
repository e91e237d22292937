"""CPU test: the host-side plan of grouped-query launches (mfa_launch_params.headsPerKeyValue).

G = headsPerKeyValue query heads share one K / V head.  0 (what mfa_launch_params_init writes) and 1 must plan exactly what a launch
that leaves the field alone plans; forward and backwardQuery plan the same launch at any G; backwardKeyValue with G > 1 needs a
workspace for its per-query-head dK / dV slabs and ends in attn_kv_group_sum.  Device pointers are fake: planning makes no HIP call.
"""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from metal_flash_attention_amd import (  # noqa: E402
    AttentionDescriptor, AttentionKernel, AttentionKernelType, AttentionOperand, GEMMOperandPrecision, MFAError, _abi,
)
from metal_flash_attention_amd._abi import lib  # noqa: E402

T = AttentionKernelType
Op = AttentionOperand
P = GEMMOperandPrecision
WS = 0x7400000000   # a fake, 256-byte aligned device address


@pytest.fixture(scope="module", autouse=True)
def _built(built_library):
    yield


STORAGE = {"f32": (False, False, P.FP16, False), "bf16": (True, False, P.BF16, False), "f16": (True, False, P.FP16, False),
           "f16mid": (True, True, P.FP16, False), "bf16out": (True, False, P.BF16, True)}
TRANSPOSES = {"rm": (False,) * 4, "kv": (False, True, True, False), "all": (True,) * 4}


def _grid():
    grid = [(D, s, "rm") for D in (32, 64, 96, 128, 160, 256, 320, 400) for s in STORAGE]
    grid += [(D, s, t) for D in (64, 128, 256, 320) for s in ("bf16", "f32") for t in ("kv", "all")]
    return grid


def _kernels():
    for D, sname, tname in _grid():
        d = AttentionDescriptor()
        d.lowPrecisionInputs, d.lowPrecisionIntermediates, d.lowPrecisionInputType, d.lowPrecisionOutputs = STORAGE[sname]
        d.matrixDimensions, d.transposeState = (512, 512, D), TRANSPOSES[tname]
        for t in T:
            kd = d.kernelDescriptor(t)
            try:
                k = AttentionKernel(kd)
            except MFAError:   # (e.g. 16-bit outputs at D > 384: no code object)
                continue
            yield "%s/%d/%s/%s" % (t.name, D, sname, tname), kd, k


SHAPES = ((512, 512, 8, 1), (300, 520, 28, 2), (1, 4096, 8, 1), (8192, 8192, 4, 1), (77, 1000, 28, 1))


def _buffers():
    return {op: 0x100000000 * (i + 1) for i, op in enumerate(Op) if op.bufferBinding is not None}


def _params(R, C, H, B, G, workspace=None, **kw):
    arr, params, _ = AttentionKernel._marshal(_buffers(), R, C, H, B, None, None, None, None, **kw)
    params.headsPerKeyValue = G
    if workspace:
        params.workspace, params.workspaceBytes = workspace
    return arr, params


def _size(k, params):
    out = ctypes.c_uint64()
    _abi.check(lib().mfa_attention_kernel_workspace_size(k._handle, ctypes.byref(params), ctypes.byref(out)))
    return int(out.value)


def _form(k, arr, params):
    out = ctypes.create_string_buffer(1024)
    _abi.check(lib().mfa_attention_kernel_launch_form(k._handle, ctypes.byref(arr), ctypes.byref(params), out, len(out)))
    return out.value.decode()


def _plan(k, R, C, H, B, G, **kw):
    """(workspace size, form without a workspace, form with that workspace) -- or the error of each step"""
    rec = []
    arr, params = _params(R, C, H, B, G, **kw)
    for step in ("size", "bare", "ws"):
        try:
            if step == "size":
                rec.append(_size(k, params))
            elif step == "bare":
                rec.append(_form(k, arr, params))
            else:
                need = rec[0] if isinstance(rec[0], int) else 0
                arr2, params2 = _params(R, C, H, B, G, workspace=(WS, need) if need else None, **kw)
                rec.append(_form(k, arr2, params2))
        except MFAError as e:
            rec.append(("E", e.status, str(e)))
    return rec


def _copy_bytes(kd, R, C, H, B, G):
    """re-layout copies of a grouped backwardKeyValue launch: transposed Q / dO (H heads) and K / V (H / G heads), 256-byte aligned"""
    total = 0
    for op in (Op.Q, Op.K, Op.V, Op.dO):
        if kd.transposeState.get(op):
            heads = H // G if op in (Op.K, Op.V) else H
            seq = R if op in (Op.Q, Op.dO) else C
            total += (heads * B * seq * kd.headDimension * kd.memoryPrecisions[op].size + 255) & ~255
    return total


def test_field_sits_at_the_old_reserved_offset():
    header = open(os.path.join(ROOT, "include", "mfa.h")).read()
    body = header[header.index("typedef struct mfa_launch_params"):header.index("} mfa_launch_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.search(r"uint32_t causal;\s*uint32_t headsPerKeyValue;", body)
    assert _abi.mfa_launch_params.headsPerKeyValue.offset == 16 + 3 * 80 + 16 + 4
    assert _abi.mfa_launch_params.headsPerKeyValue.size == 4
    p = _abi.mfa_launch_params()
    lib().mfa_launch_params_init(ctypes.byref(p))
    assert p.headsPerKeyValue == 0


def test_zero_and_one_plan_what_an_unset_field_plans():
    for key, kd, k in _kernels():
        for R, C, H, B in SHAPES:
            for kw in ({}, {"causal": True}) if C >= R else ({},):
                unset = _plan(k, R, C, H, B, 0, **kw)
                assert _plan(k, R, C, H, B, 1, **kw) == unset, (key, R, C, H, B, kw)
        assert k.variant


def test_heads_not_a_multiple_of_the_group_are_refused():
    for key, kd, k in _kernels():
        if kd.headDimension not in (64, 128):
            continue
        arr, params = _params(512, 512, 28, 1, 8, workspace=(WS, 1 << 40))
        with pytest.raises(MFAError) as e:
            _form(k, arr, params)
        assert e.value.status == 2 and "28" in str(e.value) and "8" in str(e.value), key
        with pytest.raises(MFAError) as e:
            _size(k, params)
        assert e.value.status == 2 and "28" in str(e.value), key


@pytest.mark.parametrize("G", [2, 4, 7])
def test_grouped_backward_key_value_needs_its_slabs(G):
    seen = 0
    for key, kd, k in _kernels():
        if kd.type != T.backwardKeyValue:
            continue
        for R, C, H, B in ((512, 512, 28, 1), (300, 520, 28, 2), (8192, 8192, 28, 1), (1, 4096, 56, 1)):
            if H % G:
                continue
            D = kd.headDimension
            arr, params = _params(R, C, H, B, G)
            need = _size(k, params)
            slabs = 2 * H * B * C * D * 4
            copies = _copy_bytes(kd, R, C, H, B, G) if k.needsWorkspaceForFastPath else 0
            assert need == (((slabs + 255) & ~255) + copies if copies else slabs), (key, R, C, H, B)
            with pytest.raises(MFAError) as e:   # no workspace
                _form(k, arr, params)
            assert e.value.status == 2 and str(need) in str(e.value), key
            for bad in ((WS, need - 4), (WS + 16, need)):   # too small, misaligned
                arr2, params2 = _params(R, C, H, B, G, workspace=bad)
                with pytest.raises(MFAError) as e:
                    _form(k, arr2, params2)
                assert e.value.status == 2 and str(need) in str(e.value), key
            arr2, params2 = _params(R, C, H, B, G, workspace=(WS, need))
            form = _form(k, arr2, params2)
            assert form.endswith(" + attn_kv_group_sum x%d" % G), (key, form)
            assert "column-parallel" not in form, (key, form)   # never split, even the one-head-sized long launches
            seen += 1
    assert seen


@pytest.mark.parametrize("G", [2, 4, 7, 28])
def test_forward_and_backward_query_plan_what_g1_plans(G):
    for key, kd, k in _kernels():
        if kd.type == T.backwardKeyValue:
            continue
        for R, C, H, B in ((512, 512, 28, 1), (300, 520, 28, 2), (8192, 8192, 28, 1), (4096, 4096, 28, 1), (8192, 8192, 7, 1)):
            if H % G:
                continue
            # (transposed K / V through the re-layout workspace: their row-major copies hold the H / G K / V heads, not H)
            saved = 0
            if k.needsWorkspaceForFastPath:
                for op in (Op.K, Op.V):
                    if kd.transposeState.get(op):
                        one = lambda h: (h * B * C * kd.headDimension * kd.memoryPrecisions[op].size + 255) & ~255  # noqa: E731
                        saved += one(H) - one(H // G)
            for kw in ({}, {"causal": True}):
                got, want = _plan(k, R, C, H, B, G, **kw), _plan(k, R, C, H, B, 1, **kw)
                assert got[2] == want[2], (key, R, C, H, B, G, kw)   # the same form with the workspace
                if isinstance(want[1], str) and want[1].startswith("attn_dq16_p4_tr"):
                    # (the in-place transposed kernels do not take grouped launches: without a workspace, the general kernel)
                    assert got[1].startswith(k.fallbackVariant), (key, got[1])
                else:
                    assert got[1] == want[1], (key, R, C, H, B, G, kw)
                if isinstance(want[0], int) and want[0]:
                    assert got[0] == want[0] - saved, (key, R, C, H, B, G, kw)
                else:
                    assert got[0] == want[0], (key, R, C, H, B, G, kw)
