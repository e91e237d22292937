"""GPU test: every kernel family on strided operand layouts, per operand (tests/strided.py places them, tests/strided_matrix.py lists
the cases).

Each case runs forward, backwardQuery and backwardKeyValue on the same values twice -- packed, and in the layout under test, every
output allocation filled with the canary before each run, every workspace with NaN -- and checks
  - the launch form of the strided launch is the packed launch's (misaligned layouts: the general kernel's);
  - the four checks of strided.verify(): inputs untouched, every element no operand owns still canary, no new NaN, and O, L, D, dQ,
    dK, dV BIT-IDENTICAL to the packed launch: code object, grid, splits and summation order are the same, only addresses differ,
    so no tolerance applies.  (Broadcast K / V: against the launch on materialised K / V.  Misaligned layouts run another kernel
    than the packed launch: oracle only);
  - dense and causal cases against the oracle on the stored (rounded) inputs, one head per (batch, K / V group), at the unchanged
    tolerances of tests/harness.py (grouped dK / dV: x sqrt(G), as tests/test_gqa_gpu.py).
A failure names the layout, the operand, the head and the first differing (row, column).
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import harness  # noqa: E402
import strided  # noqa: E402
from metal_flash_attention_amd import AttentionKernelType  # noqa: E402
from oracle import Network, NetworkDescriptor  # noqa: E402
from strided import Op, P  # noqa: E402
from strided_matrix import BROADCAST, KINDS, MATRIX, MISALIGNED, PINNED  # noqa: E402

T = AttentionKernelType
TORCH_BITS = {np.dtype(np.uint16): torch.int16, np.dtype(np.uint32): torch.int32}
OUTPUTS_OF = {"forward": (Op.O, Op.L), "backwardQuery": (Op.dQ, Op.D), "backwardKeyValue": (Op.dK, Op.dV)}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield


def _values(problem, seed):
    rng = np.random.default_rng(seed)
    return {op: rng.uniform(-1, 1, problem.shape(op)).astype(np.float32) for op in strided.INPUTS}


def _upload(host):
    return {name: torch.from_numpy(bits.view(bits.dtype.str.replace("u", "i"))).cuda() for name, bits in host.items()}


def _download(dev, host):
    return {name: t.cpu().numpy().view(host[name].dtype) for name, t in dev.items()}


def _launch(case, kernels, placement, values):
    """one pass of the case's kernels through `placement` -> (uploaded images, images read back, launch forms)"""
    host = strided.build_allocations(placement, values)
    dev = _upload(host)
    ptrs = placement.pointers({name: t.data_ptr() for name, t in dev.items()})
    kw = strided.launch_kwargs(case, placement)
    if placement.problem.Hkv == case.Hq:
        kw["headsPerKeyValue"] = 1
    keep = []
    if case.lengths:
        keep = [torch.tensor(x, dtype=torch.int32, device="cuda") for x in case.lengths]
        kw.update(rowLengths=keep[0], columnLengths=keep[1])
    if case.mask:
        mask = torch.from_numpy(strided.pack_mask(case.mask)).cuda()
        keep.append(mask)
        kw.update(blockMask=mask, blockMaskWords=int(mask.shape[1]))
    forms = {}
    for t, k in kernels.items():
        ws = None
        if strided.wants_workspace(case, t):
            need = k.workspaceSize(row=case.R, column=case.C, heads=case.Hq, batches=case.B, headsPerKeyValue=kw["headsPerKeyValue"])
            if need:
                ws = torch.full(((need + 3) // 4,), float("nan"), dtype=torch.float32, device="cuda")   # poison
                keep.append(ws)
        forms[t.name] = k.launchForm(ptrs, workspace=ws, **kw)
        k.dispatch(ptrs, workspace=ws, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    return host, _download(dev, host), forms


def _valid(case, problem):
    """per-batch lengths: {operand: bool [B, H, seq]} of the rows / columns the kernels write"""
    if not case.lengths:
        return None
    out = {}
    for op in strided.OUTPUTS:
        n = np.asarray(case.lengths[1 if op in strided.KV_OPS else 0])
        ok = np.arange(problem.seq(op))[None, :] < n[:, None]
        out[op] = np.broadcast_to(ok[:, None, :], problem.shape(op)[:3]).copy()
    return out


def _oracle_heads(case):
    """one query head per (batch, K / V group), spread over the problem"""
    G = case.G if case.layout != "broadcast" else 1
    return [(b, j * G + (b + j) % G) for b in range(case.B) for j in range(case.Hq // G)][:: max(1, case.B * case.Hq // (6 * G))]


def _against_oracle(case, problem, values, got):
    """the gathered results against oracle.Network on the stored inputs; dK / dV only when the group is one head or fully summed here"""
    prec = problem.precisions
    G = problem.Hq // problem.Hkv
    stored = {op: strided.decode(strided.encode(values[op], prec[op]), prec[op]) for op in strided.INPUTS}
    tol = harness.TOL_FP32 if case.storage == "f32" else harness.TOL_MIXED
    out = {op: strided.decode(bits, prec[op]) for op, bits in got.items()}
    worst = {}
    for b, h in _oracle_heads(case):
        j = h // G
        members = range(j * G, (j + 1) * G) if (Op.dK in got and G > 1) else [h]
        ref_kv = {"dK": 0.0, "dV": 0.0}
        for hh in members:
            net = Network(NetworkDescriptor(case.R, case.C, case.D), seed=1)
            net.Q, net.K, net.V, net.dO = (np.ascontiguousarray(stored[op][b, x]) for op, x in ((Op.Q, hh), (Op.K, j), (Op.V, j), (Op.dO, hh)))
            net.invalidate()
            r = net.run(backward=True, causal=case.causal)
            for name in ref_kv:
                ref_kv[name] = ref_kv[name] + r[name].astype(np.float64)
            if hh == h:
                ref = r
        for name, op, head, scale in (("O", Op.O, h, 1), ("dQ", Op.dQ, h, 1), ("dK", Op.dK, j, math.sqrt(G)), ("dV", Op.dV, j, math.sqrt(G))):
            if op not in got:
                continue
            want = ref_kv[name] if name in ref_kv else ref[name]
            nbad, err = harness.check(want, out[op][b, head], tol[name] * scale)
            worst[name] = max(worst.get(name, 0.0), err)
            assert nbad == 0, "%s: %s batch %d head %d: %d elements over %g (max error %.3e)" % (case.id, name, b, head, nbad, tol[name] * scale, err)
    return worst


def _run_case(case, seed=0):
    kernels, precisions = strided.make_kernels(case)
    ops = tuple(op for t in kernels for op in OUTPUTS_OF[t.name])
    problem = strided.problem_of(case, precisions)
    values = _values(problem, seed + case.D)
    # the baseline: the same values, packed (broadcast K / V: materialised per query head)
    base_problem = strided.problem_of(case, precisions, materialised=True)
    base_values = dict(values)
    if case.layout == "broadcast":
        base_values[Op.K], base_values[Op.V] = (np.repeat(values[op], case.Hq, axis=1) for op in (Op.K, Op.V))
    packed_pl = strided.place(base_problem, "packed")
    up0, after0, forms0 = _launch(case, kernels, packed_pl, base_values)
    valid = _valid(case, base_problem)
    failures, packed = strided.verify(packed_pl, up0, after0, None, ops, valid)
    assert not failures, ("packed launch", failures, forms0)
    # the layout under test
    pl = strided.place(problem, case.layout)
    up1, after1, forms1 = _launch(case, kernels, pl, values)
    misaligned = case.layout.startswith("misaligned")
    if misaligned:
        assert all(f.startswith(("attn_generic_", "attn_paged_")) for f in forms1.values()), forms1
    elif case.id not in PINNED:
        assert forms1 == forms0, (forms0, forms1)
    same_kernel = not misaligned and case.id not in PINNED
    failures, got = strided.verify(pl, up1, after1, packed if same_kernel else None, ops, valid, bitwise=same_kernel)
    assert not failures, (case.id, failures, forms1)
    if not case.lengths and not case.mask:
        worst = _against_oracle(case, problem, values, got)
        print("max errors against the oracle", case.id, {k: "%.2e" % v for k, v in worst.items()})
    return forms1


@pytest.mark.parametrize("case", MATRIX, ids=lambda c: c.id)
def test_family_matches_packed_launch_and_oracle(case):
    _run_case(case)


@pytest.mark.parametrize("case", KINDS, ids=lambda c: c.id)
def test_launch_kind_matches_packed_launch_and_oracle(case):
    forms = _run_case(case, seed=1)
    if case.ws and case.transposed == "none" and not case.causal:
        if case.R >= 1024:
            assert "column-parallel" in forms["backwardKeyValue"] and "combine" in forms["backwardKeyValue"], forms   # (its pieces cut the rows)
        else:
            assert "column-parallel" in forms["forward"] and "column-parallel" in forms["backwardQuery"], forms
    if case.ws and case.causal:
        assert "column-parallel" in forms["backwardQuery"], forms
    if case.G > 1:
        assert forms["backwardKeyValue"].endswith("attn_kv_group_sum x%d" % case.G), forms
    if case.transposed == "all" and case.ws and case.storage != "f32":
        assert "attn_relayout" in forms["backwardQuery"] and "attn_relayout" in forms["backwardKeyValue"], forms
    if case.transposed == "all" and not case.ws:
        assert "attn_dq16_p4_tr" in forms["backwardQuery"] and "attn_dkv16_p4_tr" in forms["backwardKeyValue"], forms
    if len(case.types) == 1 and case.B * case.Hq > 64:
        assert forms["forward"].startswith(("attn_fwd16_p4p", "attn_fwd16_p6")), forms


@pytest.mark.parametrize("case", BROADCAST, ids=lambda c: c.id)
def test_broadcast_key_value_heads_match_materialised(case):
    _run_case(case, seed=2)


@pytest.mark.parametrize("case", MISALIGNED, ids=lambda c: c.id)
def test_misaligned_views_run_the_general_kernel_correctly(case):
    _run_case(case, seed=3)


# ---- offsets above 2^31 bytes --------------------------------------------------------------------------------------------------
def test_offsets_above_two_gib_match_packed_launch_and_oracle():
    """bf16, D = 128, N = 1100, one head: the eight matrix operands are column slices of one arena of 1100 rows with a row pitch of
    2^20 elements (2 MiB), so the arena is 1100 x 2 MiB = 2.15 GiB and rows 1024 .. 1099 of every operand lie beyond 2^31 bytes from
    its base.  (N + 192) x pitch x 2 bytes = 2.5 GiB stays below the 0xFF000000 slice limit, so the matrix-core kernels take the
    launch.  The arena is not canary-filled: only the slices are touched.  It is freed before the next test."""
    N, D, pitch = 1100, 128, 1 << 20
    case = strided.Case("bf16", D, "packed", Hq=1, B=1, R=N, C=N)
    kernels, precisions = strided.make_kernels(case)
    problem = strided.problem_of(case, precisions)
    values = _values(problem, 9)
    packed_pl = strided.place(problem, "packed")
    up0, after0, forms0 = _launch(case, kernels, packed_pl, values)
    packed = {op: strided.gather(packed_pl, after0, op) for op in strided.OUTPUTS}
    arena = torch.empty(N * pitch, dtype=torch.int16, device="cuda")
    try:
        rows = arena.view(N, pitch)
        column = {op: 256 * i for i, op in enumerate(strided.MATRICES)}
        for op in strided.MATRICES:
            bits = strided.encode(values[op][0, 0], P.BF16) if op in values else np.full((N, D), strided.CANARY[P.BF16], np.uint16)
            src = bits.view(np.int16) if precisions[op] != P.FP32 else None
            if precisions[op] == P.FP32:   # an FP32 output: two 16-bit columns per element
                rows[:, column[op]:column[op] + 2 * D] = torch.from_numpy(np.full((N, 2 * D), strided.CANARY[P.BF16], np.uint16).view(np.int16)).cuda()
            else:
                rows[:, column[op]:column[op] + D] = torch.from_numpy(src).cuda()
        vec = {op: torch.full((N,), float("nan"), dtype=torch.float32, device="cuda") for op in strided.VECTORS}
        ptrs, lds = {}, {}
        for op in strided.MATRICES:
            size = 4 if precisions[op] == P.FP32 else 2
            ptrs[op] = arena.data_ptr() + column[op] * 2
            lds[op] = pitch * 2 // size
        assert (N - 1) * pitch * 2 > 1 << 31
        for op in strided.VECTORS:
            ptrs[op] = vec[op].data_ptr()
        kw = dict(row=N, column=N, leadingDimensions=lds)
        forms = {}
        for t, k in kernels.items():
            forms[t.name] = k.launchForm(ptrs, **kw)
            k.dispatch(ptrs, stream=torch.cuda.current_stream().cuda_stream, **kw)
        torch.cuda.synchronize()
        assert forms == forms0 and not any(f.startswith("attn_generic") for f in forms.values()), (forms0, forms)
        got = {}
        for op in strided.OUTPUTS:
            if op in strided.VECTORS:
                got[op] = vec[op].cpu().numpy().view(np.uint32).reshape(1, 1, N)
            elif precisions[op] == P.FP32:
                got[op] = rows[:, column[op]:column[op] + 2 * D].contiguous().cpu().numpy().view(np.uint32).reshape(1, 1, N, D)
            else:
                got[op] = rows[:, column[op]:column[op] + D].contiguous().cpu().numpy().view(np.uint16).reshape(1, 1, N, D)
        for op in strided.INPUTS:
            back = rows[:, column[op]:column[op] + D].contiguous().cpu().numpy().view(np.uint16)
            assert np.array_equal(back, strided.encode(values[op][0, 0], P.BF16)), "arena: input %s was written" % op.name
    finally:
        del arena, rows
        torch.cuda.empty_cache()
    for op in strided.OUTPUTS:
        assert np.array_equal(got[op], packed[op]), "arena: %s differs from the packed launch: %s (%s)" % (
            op.name, strided.first_difference(got[op], packed[op]), forms)
    worst = _against_oracle(case, problem, values, got)
    print("max errors against the oracle, arena", {k: "%.2e" % v for k, v in worst.items()})
