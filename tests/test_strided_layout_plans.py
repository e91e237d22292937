"""CPU tests of the layout harness (tests/strided.py) and of the host-side plans of the strided GPU matrix.

  - every case of the matrix of tests/test_strided_layouts_gpu.py plans, under its layout, the launch form the packed layout plans
    (fake device addresses: planning makes no HIP call); the misaligned layouts plan the general kernel.  No aligned layout of the
    matrix may fall back to the general kernel: the GPU test would then quietly test the fallback;
  - every kernel family the `forms` section of tests/golden/variant_coverage.json names is reached by a strided case, apart from
    the families listed in NOT_REACHED with the reason;
  - the checker catches what it is for: a numpy model of attention that reads and writes through a Placement passes the four
    checks of strided.verify(), and each of six mutants of its addressing (a swapped leading dimension, a dropped base offset,
    a written pad column, a packed stride for L, a zero head stride) is flagged.  A deliberately wrong kernel is never run.
"""
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

import strided  # noqa: E402
from strided import Op, P  # noqa: E402
from strided_matrix import ALL_CASES, PINNED, family_of  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built(built_library):
    yield


GENERAL = ("attn_generic_", "attn_paged_")


@pytest.fixture(scope="module")
def plans():
    """{case id: (packed forms, strided forms)}"""
    out = {}
    for case in ALL_CASES:
        kernels, precisions = strided.make_kernels(case)
        out[case.id] = (strided.planned_forms(case, "packed", kernels, precisions), strided.planned_forms(case, None, kernels, precisions))
    return out


def test_case_ids_are_unique():
    ids = [c.id for c in ALL_CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)


def test_aligned_layouts_plan_the_packed_launch_form(plans):
    wrong = []
    for case in ALL_CASES:
        packed, own = plans[case.id]
        if case.layout.startswith("misaligned") or case.id in PINNED:
            continue
        for t in packed:
            if packed[t] != own[t]:
                wrong.append((case.id, t, packed[t], own[t]))
    assert not wrong, wrong


def test_no_aligned_case_falls_back_to_the_general_kernel(plans):
    """a case whose packed launch runs a matrix-core or FP32 production kernel must run it under its layout as well"""
    fell_back = [(case.id, t, own[t]) for case in ALL_CASES for packed, own in [plans[case.id]] for t in own
                 if not case.layout.startswith("misaligned") and own[t].startswith(GENERAL) and not packed[t].startswith(GENERAL)]
    assert len(fell_back) == 0, fell_back
    assert not PINNED, "pinned findings are listed with their reason; none is expected today"


def test_misaligned_layouts_plan_the_general_kernel(plans):
    seen = 0
    for case in ALL_CASES:
        if not case.layout.startswith("misaligned"):
            continue
        seen += 1
        packed, own = plans[case.id]
        for t in own:
            assert own[t].startswith(GENERAL), (case.id, t, own[t])
    assert seen >= 8, seen   # both positions (leading dimension, base pointer) per storage type


def test_mixed_layout_shares_no_stride_between_operands():
    for case in ALL_CASES:
        if case.layout != "mixed":
            continue
        _, precisions = strided.make_kernels(case)
        views = strided.place(strided.problem_of(case, precisions), "mixed").views
        for attr in ("ld", "headStride"):
            values = [getattr(views[op], attr) for op in strided.MATRICES]
            assert len(set(values)) == len(values), (case.id, attr, values)
        assert views[Op.L].headStride != views[Op.D].headStride and views[Op.L].headStride > case.R, case.id


# ---- family coverage ---------------------------------------------------------------------------------------------------------
# families of tests/golden/variant_coverage.json no strided case reaches, each with the reason (no wildcard: exact family names)
NOT_REACHED = {
    "attn_dkv16": "the one-wave-per-key-block dK / dV kernel: only a non-default parameter-table row selects it",
}


def test_every_recorded_family_is_reached_by_a_strided_case(plans):
    recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "variant_coverage.json")))["forms"]
    families = {family_of(name) for name in recorded}
    reached = {}
    for case in ALL_CASES:
        if case.layout in ("packed",) or case.layout.startswith("misaligned") or case.id in PINNED:
            continue
        for form in plans[case.id][1].values():
            for name in re.findall(r"attn_[A-Za-z0-9_]+", form):
                reached.setdefault(family_of(name), []).append(case.id)
    missing = sorted(f for f in families if f not in reached and f not in NOT_REACHED)
    assert not missing, missing
    stale = sorted(f for f in NOT_REACHED if f in reached or f not in families)
    assert not stale, stale
    # every reached family meets the mixed layout, and token-major or fused
    for fam, ids in reached.items():
        if fam not in families:
            continue
        layouts = {i.split("-")[2] for i in ids}
        assert "mixed" in layouts, (fam, sorted(layouts))
        assert layouts & {"token", "fused"}, (fam, sorted(layouts))


def family_table(plans):
    """family -> case ids (for the pull request's description): python tests/test_strided_layout_plans.py"""
    table = {}
    for case in ALL_CASES:
        if case.layout == "packed" or case.layout.startswith("misaligned"):
            continue
        for form in plans[case.id][1].values():
            for name in re.findall(r"attn_[A-Za-z0-9_]+", form):
                ids = table.setdefault(family_of(name), [])
                if case.id not in ids:
                    ids.append(case.id)
    return table


# ---- checker self-test: a numpy model of attention through strided views, and its mutants ---------------------------------------
def _model(placement, host, mutant=None):
    """forward + backward of softmax(Q K^T / sqrt(D)) V in float64, every operand read and written through its View"""
    p = placement.problem
    views = {op: strided.View(**vars(v)) for op, v in placement.views.items()}
    packed = strided.place(p, "packed").views
    if mutant == "k_ld_for_v":
        views[Op.V].ld = views[Op.K].ld
    elif mutant == "q_ld_for_do":
        views[Op.dO].ld = views[Op.Q].ld
    elif mutant == "no_base_offset":
        for op in (Op.K, Op.dK):
            views[op].offset = 0
    elif mutant == "packed_head_stride_for_l":
        views[Op.L].headStride = packed[Op.L].headStride
    elif mutant == "zero_head_stride":
        views[Op.K].headStride = 0
    used = strided.Placement(placement.layout, p, views, placement.allocs)

    def read(op):
        idx = np.minimum(used.indices(op), len(host[views[op].alloc]) - 1)   # (a buffer resource clamps; the model must not fault either)
        return strided.decode(host[views[op].alloc][idx], p.precisions[op]).astype(np.float64)

    def write(op, x):
        idx = used.indices(op)
        host[views[op].alloc][idx] = strided.encode(x.astype(np.float32), p.precisions[op])

    Q, K, V, dO = (read(op) for op in strided.INPUTS)
    G = p.Hq // p.Hkv
    K, V = (np.repeat(x, G, axis=1) for x in (K, V))
    S = np.einsum("bhrd,bhcd->bhrc", Q, K) / np.sqrt(p.D)
    m = S.max(-1, keepdims=True)
    e = np.exp(S - m)
    Pm = e / e.sum(-1, keepdims=True)
    O = Pm @ V
    Dv = (dO * O).sum(-1)
    dP = np.einsum("bhrd,bhcd->bhrc", dO, V)
    dS = Pm * (dP - Dv[..., None]) / np.sqrt(p.D)
    fold = lambda x: x.reshape(p.B, p.Hkv, G, p.C, p.D).sum(2)   # noqa: E731
    write(Op.O, O)
    write(Op.L, (m[..., 0] + np.log(e.sum(-1))))
    write(Op.D, Dv)
    write(Op.dQ, dS @ K)
    write(Op.dK, fold(np.einsum("bhrc,bhrd->bhcd", dS, Q)))
    write(Op.dV, fold(np.einsum("bhrc,bhrd->bhcd", Pm, dO)))
    if mutant == "writes_a_pad_column":
        v = views[Op.dQ]
        host[v.alloc][v.offset + 5 * v.ld + p.D] = 0


def _model_run(layout, mutant=None, storage=P.BF16):
    precisions = {op: storage for op in strided.MATRICES}
    precisions.update({Op.L: P.FP32, Op.D: P.FP32, Op.O: P.FP32, Op.dQ: P.FP32, Op.dK: P.FP32, Op.dV: P.FP32})
    p = strided.Problem(2, 3, 3, 40, 40, 16, precisions)
    rng = np.random.default_rng(5)
    values = {op: rng.uniform(-1, 1, p.shape(op)).astype(np.float32) for op in strided.INPUTS}
    packed_pl = strided.place(p, "packed")
    packed_host = strided.build_allocations(packed_pl, values)
    _model(packed_pl, packed_host)
    packed = {op: strided.gather(packed_pl, packed_host, op) for op in strided.OUTPUTS}
    pl = strided.place(p, layout)
    uploaded = strided.build_allocations(pl, values)
    after = {k: v.copy() for k, v in uploaded.items()}
    with np.errstate(all="ignore"):
        _model(pl, after, mutant)
    failures, got = strided.verify(pl, uploaded, after, packed)
    return failures


@pytest.mark.parametrize("layout", ["packed", "token", "fused", "padded", "mixed"])
def test_the_unmutated_model_passes_all_four_checks(layout):
    assert _model_run(layout) == []


MUTANTS = {"k_ld_for_v": "mixed", "q_ld_for_do": "mixed", "no_base_offset": "fused", "writes_a_pad_column": "padded",
           "packed_head_stride_for_l": "padded", "zero_head_stride": "mixed"}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_each_mutant_of_the_model_is_flagged(mutant):
    failures = _model_run(MUTANTS[mutant], mutant)
    assert failures, mutant
    expected = {"k_ld_for_v": ("O", "dQ"), "q_ld_for_do": ("D", "dQ"), "no_base_offset": ("O", "dK"), "writes_a_pad_column": ("dQ",),
                "packed_head_stride_for_l": ("L",), "zero_head_stride": ("O", "dK")}[mutant]
    text = " | ".join(failures)
    for name in expected:   # the failure names the operand the wrong stride spoils
        assert re.search(r"\b%s\b" % name, text), (mutant, name, failures)


def test_a_failure_names_layout_operand_head_and_element():
    failures = _model_run("mixed", "k_ld_for_v")
    assert any(re.search(r"mixed: \w+ differs from the packed launch: batch \d+ head \d+ \(row \d+, column \d+\)", f) for f in failures), failures


def test_a_swapped_stride_goes_unseen_when_every_operand_shares_one_layout():
    """why the mixed layout exists: under token-major every operand has the same strides, and the swap changes no address"""
    assert _model_run("token", "k_ld_for_v") == []


if __name__ == "__main__":
    import __graft_entry__ as entry
    entry.build()
    allplans = {}
    for c in ALL_CASES:
        ks, pr = strided.make_kernels(c)
        allplans[c.id] = (strided.planned_forms(c, "packed", ks, pr), strided.planned_forms(c, None, ks, pr))
    for fam, ids in sorted(family_table(allplans).items()):
        print("| %s | %s |" % (fam, ", ".join(ids[:3]) + (" (+%d)" % (len(ids) - 3) if len(ids) > 3 else "")))
