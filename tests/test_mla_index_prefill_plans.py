"""CPU test (no GPU call, through the built library): the host side of the prefill indexer, include/mfa_mla_index_prefill.h -- every
declared name exported and listed, the decode indexer's lists as they were, the launch form and the workspace at hand-computed shapes,
the refusals by status and words, and rows past 32 accepted by every stage: the pointers are made up."""
import os
import re

import pytest

import metal_flash_attention_amd as mfa
from metal_flash_attention_amd import AttentionMLAIndex, AttentionMLAIndexPrefill, GEMMOperandPrecision as P, MFAError, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS, NEW, WS = 0x1000, 0x2000, 0x100000   # the host reads none of them
INVALID, UNSUPPORTED = 2, 3
STAGES = ("logits", "select", "topk")
NAMES = {"mfa_mla_index_prefill_workspace_size"} | {"mfa_mla_index_prefill_%s_%s" % (s, v) for s in STAGES for v in ("launch", "launch_form", "time")}
IP = AttentionMLAIndexPrefill(P.FP16)


def shape(**over):
    return dict(dict(rows=400, column=16384, indexHeads=40, batches=2, topk=2048, cacheLengths=LENGTHS, queryLengths=NEW), **over)


def test_header_symbols_exported_and_listed_and_the_old_lists_as_they_were():
    header = open(os.path.join(ROOT, "include", "mfa_mla_index_prefill.h")).read()
    declared = set(re.findall(r"\b(mfa_\w+)\s*\(", header.split("#ifndef MFA_MLA_INDEX_PREFILL_H")[1]))
    handle = _abi.lib()
    assert declared == {s[0] for s in _abi.MLA_INDEX_PREFILL_SYMBOLS} == NAMES and len(NAMES) == 10
    for name, restype, argtypes in _abi.MLA_INDEX_PREFILL_SYMBOLS:
        fn = getattr(handle, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert int(handle.mfa_abi_version()) == 6 == _abi.EXPECTED_ABI
    assert len(_abi.MLA_INDEX_SYMBOLS) == 13 and not any("prefill" in s[0] for s in _abi.MLA_INDEX_SYMBOLS)
    assert mfa.AttentionMLAIndexPrefill is AttentionMLAIndexPrefill and issubclass(AttentionMLAIndexPrefill, AttentionMLAIndex)


def test_the_torch_ops_are_a_list_of_their_own():
    pytest.importorskip("torch")
    from metal_flash_attention_amd import torch_binding as tb
    assert [op[0] for op in tb._MLA_INDEX_OPS] == ["mla_index_logits", "mla_index_select", "mla_index_topk"]
    assert [op[0] for op in tb._MLA_INDEX_PREFILL_OPS] == ["mla_index_prefill_logits", "mla_index_prefill_select", "mla_index_prefill_topk"]
    assert [op[2:] for op in tb._MLA_INDEX_PREFILL_OPS] == [op[2:] for op in tb._MLA_INDEX_OPS] and all(op[3] == () for op in tb._MLA_INDEX_OPS)
    for name in ("mla_index_prefill_logits", "mla_index_prefill_select", "mla_index_prefill_topk"):
        assert getattr(mfa, name) is getattr(tb, name)


def test_the_launch_form_at_a_hand_computed_shape():
    # 64 tiles x 2 sequences = 128 workgroups: 4 spans bring 512, ceil(400 / 4) = 100 rows -> 128; a workspace of 300 rows holds 2 spans
    logits = "attn_mlaip_d128_f16 (grid %d = 64 tiles of 256 keys x %d spans of 128 rows x 2 sequences, 40 heads, contiguous)"
    select = "attn_mlaip_select (grid %d = %d rows x 2 sequences, topk 2048)"
    assert IP.launchForm(stage="logits", **shape()) == logits % (512, 4)
    assert IP.launchForm(stage="select", **shape()) == select % (800, 400)
    assert IP.launchForm(**shape(workspace=WS, workspaceBytes=300 * 2 * 16384 * 4)) == logits % (256, 2) + " + " + select % (512, 256) + ", 2 passes of 256 rows"
    assert IP.launchForm(**shape(workspace=WS, workspaceBytes=1 << 40)).endswith(", 1 passes of 400 rows")
    # a span is at least 32 rows and at most 256
    assert "2 tiles of 256 keys x 10 spans of 32 rows x 1 sequences" in IP.launchForm(stage="logits", **shape(rows=300, column=300, batches=1))
    assert "128 tiles of 256 keys x 16 spans of 256 rows x 8 sequences" in IP.launchForm(stage="logits", **shape(rows=4096, column=32768, batches=8))


def test_the_workspace_size_under_and_over_the_cap():
    assert IP.workspaceSize(**shape()) == 2 * 400 * 16384 * 4                      # the whole chunk: 50 MiB
    assert IP.workspaceSize(**shape(column=16382)) == 2 * 400 * 16384 * 4          # the column rounded up to 4
    # 3 x 20000 x 4 = 240000 bytes a row: 256 MiB hold 1118 rows, 4 whole spans of 256
    assert IP.workspaceSize(**shape(rows=4096, column=20000, batches=3)) == 1024 * 240000 < _abi.MFA_MLA_INDEX_PREFILL_WORKSPACE_CAP == 256 << 20


def outcome(stage, kw, op=IP):
    try:
        op.launchForm(stage=stage, **kw)
    except MFAError as e:
        return e.status, str(e).split(": ", 1)[1]
    return 0, ""


REFUSALS = [
    ("no index head", "logits", shape(indexHeads=0), INVALID, "indexHeads must be 1 .. 64, not 0"),
    ("65 index heads", "topk", shape(indexHeads=65, workspace=WS, workspaceBytes=1 << 40), INVALID, "indexHeads must be 1 .. 64, not 65"),
    ("indexDimension 64", "logits", shape(), UNSUPPORTED, "the MLA indexer is compiled for indexDimension = 128, not 64"),
    ("topk 0", "select", shape(topk=0), INVALID, "topk must be at least 1"),
    ("a logit row stride below the column", "select", shape(logitStrides=(16383, 400 * 16384)), INVALID,
     "logitRowStride must be at least column = 16384 elements, not 16383"),
    ("no workspace", "topk", shape(), INVALID, "workspace is required: mfa_mla_index_prefill_topk_launch keeps the logits of a pass of rows in it, at least 16777216 bytes"),
    ("a workspace short of one span", "topk", shape(workspace=WS, workspaceBytes=127 * 2 * 16384 * 4), INVALID,
     "workspace too small: workspaceBytes = 16646144, a pass needs one span of 128 rows per sequence, 16777216 bytes"),
]


@pytest.mark.parametrize("name,stage,kw,status,needle", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_a_refusal_names_its_requirement(name, stage, kw, status, needle):
    op = AttentionMLAIndexPrefill(P.FP16, 64) if name == "indexDimension 64" else IP
    got = outcome(stage, kw, op)
    assert got[0] == status and needle in got[1], got
    if "prefill" not in needle and "span" not in needle:   # word for word the decode indexer's text for the same mistake
        decode = {k: v for k, v in dict(kw, rows=32).items() if k != "queryLengths"}
        assert got == outcome(stage, decode, AttentionMLAIndex(P.FP16, op.indexDimension))


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("rows", [33, 4096])
def test_rows_past_32_are_accepted(stage, rows):
    assert outcome(stage, shape(rows=rows, workspace=WS, workspaceBytes=1 << 40)) == (0, "")
    assert outcome(stage, shape(rows=rows, workspace=WS, workspaceBytes=1 << 40, queryLengths=None)) == (0, "")
    with pytest.raises(MFAError, match="at most 32 rows"):   # the decode entries keep their limit
        AttentionMLAIndex(P.FP16).launchForm(stage=stage, **{k: v for k, v in shape(rows=rows, workspace=WS, workspaceBytes=1 << 40).items() if k != "queryLengths"})
