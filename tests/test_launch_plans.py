"""CPU test: the whole host-side plan of every kind of launch, pinned against tests/golden/launch_plans.json.xz.

For a grid of kernel descriptors (kernel types, head dimensions, storage types, transposed operands, strict block dimensions,
non-default table rows) and of launches (shapes, heads and batches, causal, per-batch lengths, block mask, workspace, alignment,
slices over the 32-bit limit), the library's C ABI reports the selected variant and its fallback, the block dimensions,
threadgroup size and LDS bytes, the effective descriptor, the workspace size and the launch form -- or the status and message of
the error.  Device pointers are fake: planning a launch makes no HIP call.

Regenerate the fixture (only when a change of routing is intended):  python tests/test_launch_plans.py --write
"""
import ctypes
import json
import lzma
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from metal_flash_attention_amd import (  # noqa: E402
    AttentionDescriptor, AttentionKernel, AttentionKernelType, AttentionOperand, GEMMOperandPrecision, MFAError, _abi,
)
from metal_flash_attention_amd._abi import lib  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plans.json.xz")
T = AttentionKernelType
Op = AttentionOperand
P = GEMMOperandPrecision
ROW_OPS = (Op.Q, Op.O, Op.dO, Op.dQ)
MATRIX_OPS = (Op.Q, Op.K, Op.V, Op.O, Op.dO, Op.dQ, Op.dK, Op.dV)
HEADS = (8, 16, 30, 32, 48, 64, 96, 100, 128, 136, 160, 192, 256, 320, 384, 1000)


def descriptors():
    """(key, AttentionKernelDescriptor or ("E", status, message)) of the descriptor grid."""
    # (name, lowPrecisionInputs, lowPrecisionIntermediates, input type, lowPrecisionOutputs); f16mid: FP16 with BF16 dO
    storage = {"f32": (False, False, P.FP16, False), "bf16": (True, False, P.BF16, False), "f16": (True, False, P.FP16, False),
               "bf16mid": (True, True, P.BF16, False), "f16mid": (True, True, P.FP16, False), "bf16out": (True, False, P.BF16, True)}
    transposes = {"rm": (False,) * 4, "kv": (False, True, True, False), "k": (False, True, False, False),
                  "v": (False, False, True, False), "all": (True,) * 4}
    grid = [(D, sname, "rm") for D in HEADS for sname in storage]
    grid += [(D, sname, tname) for D in (32, 64, 128, 160, 192, 256, 320) for sname, tnames in
             (("bf16", ("kv", "k", "v", "all")), ("f16mid", ("kv", "all")), ("f32", ("all",))) for tname in tnames]
    for D, sname, tname in grid:
        d = AttentionDescriptor()
        d.lowPrecisionInputs, d.lowPrecisionIntermediates, d.lowPrecisionInputType, d.lowPrecisionOutputs = storage[sname]
        d.matrixDimensions, d.transposeState = (512, 512, D), transposes[tname]
        for t in T:
            key = "%s/%d/%s/%s" % (t.name, D, sname, tname)
            try:
                yield key, d.kernelDescriptor(t)
            except MFAError as e:
                yield key, ("E", e.status, str(e))
                continue
            variants, rows = [], []
            if D in (64, 128, 192) and sname in ("f32", "bf16mid") and tname in ("rm", "all"):
                variants = [("/strict", dict(strictBlockDimensions=True))]
                if tname == "rm" and D != 192:   # non-default table rows: other block dimensions and cache states, strict and not
                    rows = [(64, 32, 64), (32, 64, 128), (256, 64, 128)]
                    variants.append(("/uncached", dict(cacheState="none")))
            if D in (32, 64, 96, 160, 256) and (sname, tname) == ("bf16mid", "rm"):
                # the rows that select a sibling code object of the bucket: the 32-row dQ waves and 32-key dK/dV pairs in front of
                # which a hand-placed kernel stands, the 96-wide dK/dV pairs, the eight-wave forward kernels of D <= 64.  Every
                # row goes to every kernel type: one that matches nothing pins the nearest candidate and the strict error text
                rows += [r for r in ((128, 64, D), (64, 32, D), (128, 32, 96), (256, 32, 64), (256, 64, 64)) if r not in rows]
            variants += [("/row%dx%dx%d%s" % (row + ("/strict" * s,)), dict(blockDimensions=row, strictBlockDimensions=s))
                         for row in rows for s in (False, True)]
            for suffix, change in variants:
                k = d.kernelDescriptor(t)
                for name, value in change.items():
                    setattr(k, name, {op: False for op in k.cacheState} if value == "none" else value)
                yield key + suffix, k


def launches():
    """(key, launch keyword arguments) of the launch grid; `ws` / `pointer` / `ld` are applied by _params()."""
    shapes = (("sq", 512, 512, 1, 1), ("rect", 300, 520, 1, 1), ("decode", 1, 4096, 1, 1), ("onehead", 8192, 8192, 1, 1),
              ("heads", 1024, 1024, 8, 2), ("odd", 77, 1000, 3, 1))
    mask = dict(blockMask=0x7200000, blockMaskWords=1)
    for name, R, C, H, B in shapes:
        shape = dict(row=R, column=C, heads=H, batches=B)
        extra = [("", {}), ("/causal", dict(causal=True))]
        if name in ("sq", "heads"):
            extra += [("/lengths", dict(rowLengths=0x7000000, columnLengths=0x7100000)), ("/mask", mask),
                      ("/mask/causal", dict(mask, causal=True))]
        if name in ("sq", "onehead", "rect"):
            extra += [("/ws", dict(ws=True)), ("/causal/ws", dict(causal=True, ws=True))]
        if name == "sq":   # a misaligned operand pointer, an odd leading dimension, a slice over the 32-bit limit
            extra += [("/misaligned", dict(pointer=2)), ("/oddld", dict(ld=1)), ("/huge", dict(ld=1 << 22))]
        for suffix, kw in extra:
            yield name + suffix, dict(shape, **kw)


def _buffers(extra_ptr):
    return {op: 0x100000000 * (i + 1) + (extra_ptr if op == Op.Q else 0) for i, op in enumerate(Op) if op.bufferBinding is not None}


def _params(kd, spec):
    spec = dict(spec)
    ws, ptr, ld = spec.pop("ws", False), spec.pop("pointer", 0), spec.pop("ld", 0)
    lds = None
    if ld:
        R, C, D = spec["row"], spec["column"], kd.headDimension
        lds = {op: (D + ld if not kd.transposeState.get(op) else (R if op in ROW_OPS else C) + ld) if ld < 1024 else ld
               for op in MATRIX_OPS}
    arr, params, _ = AttentionKernel._marshal(_buffers(ptr), spec.pop("row"), spec.pop("column"), spec.pop("heads"),
                                              spec.pop("batches"), lds, None, None, None, **spec)
    return arr, params, ws


def _workspace_size(k, params):
    out = ctypes.c_uint64()
    _abi.check(lib().mfa_attention_kernel_workspace_size(k._handle, ctypes.byref(params), ctypes.byref(out)))
    return int(out.value)


def _form(k, arr, params):
    out = ctypes.create_string_buffer(1024)
    _abi.check(lib().mfa_attention_kernel_launch_form(k._handle, ctypes.byref(arr), ctypes.byref(params), out, len(out)))
    return out.value.decode()


def _effective(k):
    e = k.effectiveDescriptor
    enc = lambda m: ",".join("%s=%d" % (op.name, int(v)) for op, v in sorted(m.items(), key=lambda kv: int(kv[0])))  # noqa: E731
    return "%s|%s|%s|%s" % (e.blockDimensions, enc(e.cacheState), enc(e.registerPrecisions), enc(e.memoryPrecisions))


def _launch(k, kd, spec):
    """[workspace size, form without / with a short / a misaligned / a sufficient workspace]; a form is the text or
    ["E", status, message]"""
    arr, params, ws = _params(kd, spec)
    try:
        need = _workspace_size(k, params)
    except MFAError as e:
        return ["E", e.status, str(e)]
    rec = [need]
    for w in (None,) if not (ws and need) else (None, (0x7400000000, need // 2), (0x7400000008, need + 4096), (0x7400000000, need)):
        if w:
            params.workspace, params.workspaceBytes = w
        try:
            rec.append(_form(k, arr, params))
        except MFAError as e:
            rec.append(["E", e.status, str(e)])
    return rec


def plans():
    """{descriptor key: [variant, fallback, block dimensions, threadgroup size, LDS bytes, effective descriptor, needs workspace,
    {launch key: launch record}] or ["E", status, message]}"""
    out = {}
    for key, kd in descriptors():
        if isinstance(kd, tuple):
            out[key] = list(kd)
            continue
        try:
            k = AttentionKernel(kd)
        except MFAError as e:
            out[key] = ["E", e.status, str(e)]
            continue
        out[key] = [k.variant, k.fallbackVariant, list(k.blockDimensions), k.threadgroupSize, k.threadgroupMemoryAllocation,
                    _effective(k), int(k.needsWorkspaceForFastPath), {lkey: _launch(k, kd, spec) for lkey, spec in launches()}]
    return out


@pytest.fixture(scope="module", autouse=True)
def _built(built_library):
    yield


def test_every_launch_plan_matches_the_golden_record():
    with lzma.open(GOLDEN, "rt") as f:
        want = json.load(f)
    got = json.loads(json.dumps(plans()))   # (tuples as lists, like the fixture)
    assert sorted(got) == sorted(want), "the descriptor grid changed"
    diffs = []
    for key in sorted(want):
        w, g = want[key], got[key]
        if w[0] != "E" and g[0] != "E":
            diffs += ["%s %s: %r != %r" % (key, lkey, g[-1].get(lkey), w[-1][lkey]) for lkey in w[-1] if g[-1].get(lkey) != w[-1][lkey]]
            w, g = w[:-1], g[:-1]
        if g != w:
            diffs.append("%s: %r != %r" % (key, g, w))
    assert not diffs, "%d launch plans differ:\n" % len(diffs) + "\n".join(diffs[:40])


if __name__ == "__main__":
    if sys.argv[1:2] != ["--write"]:
        sys.exit(__doc__)
    path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    with open(path, "wb") as f:
        f.write(lzma.compress(json.dumps(plans(), sort_keys=True, separators=(",", ":")).encode(), preset=9))
    print(path, os.path.getsize(path), "bytes")
