"""CPU test (no GPU call, through the built library): the host side of MLA prefill cut along the keys, include/mfa_mla_prefill_split.h --
the piece function (the very function the kernels run), the plan and the one workspace formula, the launch forms, the refusals in
words, and what must not have moved: ABI 6 and the 168 bytes of mfa_mla_prefill_params."""
import ctypes
import os
import re

import pytest

from metal_flash_attention_amd import AttentionMLAPrefill, AttentionMLAPrefillSplit, GEMMOperandPrecision as P, MFAError, _abi

ROOT = os.path.join(os.path.dirname(__file__), "..")
WS = 0x7F0000000000   # a pointer nobody follows: no entry here reaches the GPU


def shape(**kw):
    return dict(dict(rows=64, column=32832, heads=16, batches=1, scale=0.125, cacheLengths=WS), **kw)


def test_header_symbols_and_what_has_not_moved():
    header = open(os.path.join(ROOT, "include", "mfa_mla_prefill_split.h")).read()
    declared = set(re.findall(r"\b(mfa_\w+)\s*\(", header.split("#ifndef MFA_MLA_PREFILL_SPLIT_H")[1]))
    assert declared == {s[0] for s in _abi.MLA_PREFILL_SPLIT_SYMBOLS} == {
        "mfa_attention_mla_prefill_split_" + s for s in ("launch", "launch_form", "time", "workspace_size", "piece_range")}
    for name, const in (("MAX_PIECES", 64), ("TARGET", 256), ("MIN_STEPS", 16)):
        assert "MFA_MLA_PREFILL_SPLIT_%s %du" % (name, const) in header and getattr(_abi, "MFA_MLA_PREFILL_SPLIT_" + name) == const
    handle = _abi.lib()
    assert handle.mfa_abi_version() == _abi.EXPECTED_ABI == 6
    assert handle.mfa_mla_prefill_params_size() == ctypes.sizeof(_abi.mfa_mla_prefill_params) == 168
    assert not hasattr(AttentionMLAPrefill, "plannedSplit")


@pytest.mark.parametrize("pieces", [1, 2, 3, 7, 64])
def test_the_pieces_are_ordered_disjoint_cover_the_walk_and_differ_by_one_step(pieces):
    for end in range(101):
        cuts = [AttentionMLAPrefillSplit.pieceRange(end, pieces, i) for i in range(pieces)]
        assert cuts[0][0] == 0 and cuts[-1][1] == end and all(b <= e for b, e in cuts)
        assert all(cuts[i][1] == cuts[i + 1][0] for i in range(pieces - 1))
        sizes = [e - b for b, e in cuts]
        assert max(sizes) - min(sizes) <= 1, (end, pieces, cuts)


@pytest.mark.parametrize("B,H,rows,column,pieces", [(1, 16, 64, 32832, 16), (1, 16, 64, 4160, 8), (1, 16, 512, 33280, 2), (1, 128, 64, 32832, 2),
                                                    (8, 128, 64, 32832, 1), (1, 16, 64, 64, 1), (1, 1, 1, 100000, 64)])
def test_the_plan_and_the_one_workspace_formula(B, H, rows, column, pieces):
    mla = AttentionMLAPrefillSplit(P.BF16)
    need = pieces * B * H * rows * 514 * 4 if pieces > 1 else 0
    kw = shape(batches=B, heads=H, rows=rows, column=column)
    assert mla.plannedSplit(**kw) == (need, pieces)
    assert mla.plannedSplit(workspace=WS + 4, workspaceBytes=1, **kw) == (need, pieces)   # a workspace the block names is not looked at
    assert mla.plannedSplit(pieces=5, **kw) == (5 * B * H * rows * 514 * 4, 5) and mla.plannedSplit(pieces=1, **kw) == (0, 1)


def test_launch_forms():
    bf, hf = AttentionMLAPrefillSplit(P.BF16), AttentionMLAPrefillSplit(P.FP16)
    need, _ = bf.plannedSplit(**shape())
    assert bf.launchForm(**shape(workspace=WS, workspaceBytes=need)) == (
        "attn_mla16pk_d576_bf16 (grid 256 = 16 blocks x 1 sequences x 16 pieces, 1024 packed rows in blocks of 64, contiguous) + "
        "attn_mla16p_d576_bf16_combine (grid 256)")
    form = hf.launchForm(**shape(rows=3, heads=11, batches=2, pieces=5, workspace=WS, workspaceBytes=5 * 2 * 33 * 514 * 4, pageSize=16, blockTable=WS,
                                 blockTableStride=4096))
    assert form == ("attn_mla16pk_d576_f16 (grid 10 = 1 blocks x 2 sequences x 5 pieces, 33 packed rows in blocks of 64, paged) + "
                    "attn_mla16p_d576_f16_combine (grid 17)"), form
    unsplit = AttentionMLAPrefill(P.BF16).launchForm(**shape())
    assert bf.launchForm(**shape()) == unsplit[:-1] + ", unsplit without a workspace: the plan has 16 pieces)"
    assert bf.launchForm(**shape(pieces=1, workspace=WS + 2, workspaceBytes=0)) == unsplit == bf.launchForm(**shape(column=64))


def test_refusals_in_words():
    bf = AttentionMLAPrefillSplit(P.BF16)
    need, _ = bf.plannedSplit(**shape())
    for what, kw, said in (
            ("more pieces than lanes", shape(pieces=65), "mfa_key_split.pieces must be 0 (the host's plan), 1 (unsplit) or 2 .. 64"),
            ("a short workspace", shape(workspace=WS, workspaceBytes=need - 1),
             "workspace too small: %d bytes, the launch needs %d (mfa_attention_mla_prefill_split_workspace_size)" % (need - 1, need)),
            ("a misaligned workspace", shape(workspace=WS + 8, workspaceBytes=need), "workspace must be 16-byte aligned")):
        with pytest.raises(MFAError) as e:
            bf.launchForm(**kw)
        assert said in str(e.value), (what, str(e.value))
    words = []   # a params refusal comes out in the unsplit entry's words
    for host in (AttentionMLAPrefill(P.BF16), bf):
        with pytest.raises(MFAError) as e:
            host.launchForm(**shape(scale=0.0))
        words.append(str(e.value))
    assert words[0] == words[1] and "scale is required" in words[0]
    p = bf._params(**shape())[0]
    out = ctypes.create_string_buffer(64)
    assert _abi.lib().mfa_attention_mla_prefill_split_launch_form(ctypes.byref(p), None, out, len(out)) != 0
    assert "null mfa_key_split" in _abi.lib().mfa_last_error_string().decode()
