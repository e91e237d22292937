"""CPU test (fake tensors, no device): the torch binding of include/mfa_tree.h -- the tree_mask= keyword of flash_decode and
flash_prefill reaches the ops mfa::attention_decode_tree / mfa::attention_prefill_tree, registered with `tree_mask` last in their schemas
and with fake implementations that give the right shapes; None takes today's op with today's arguments; what the keyword may be is said
in words, a cap beside it too; flash_prefill_ragged has no such keyword; pack_tree_mask packs bit j of row r.  Which op every call
reaches, with which arguments, and the words of every refusal are pinned in tests/golden/tree_routing.json."""
import inspect
import json
import os

import pytest

torch = pytest.importorskip("torch")

from torch._subclasses.fake_tensor import FakeTensorMode  # noqa: E402

from metal_flash_attention_amd import torch_binding as tb  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_routing.json")
NEW_OPS = ("attention_decode_tree", "attention_prefill_tree")


@pytest.fixture(scope="module", autouse=True)
def _ops():
    if not tb._HAVE_TREE_OPS:
        pytest.skip("this torch has no torch.library.custom_op")


def operands():
    q = torch.empty((2, 8, 40, 64), dtype=torch.bfloat16, device="cuda")
    k16 = torch.empty((2, 2, 1024, 64), dtype=torch.bfloat16, device="cuda")
    k8 = torch.empty((2, 2, 1024, 64), dtype=torch.float8_e4m3fn, device="cuda")
    lens = torch.empty((2,), dtype=torch.int32, device="cuda")
    scale = torch.empty((2,), dtype=torch.float32, device="cuda")
    logits = torch.empty((8,), dtype=torch.float32, device="cuda")
    shared = torch.empty((40,), dtype=torch.int64, device="cuda")
    each = torch.empty((2, 40), dtype=torch.int64, device="cuda")
    return q, k16, k8, lens, scale, logits, shared, each


def said(x):
    if isinstance(x, torch.Tensor):
        return "Tensor%s %s" % (list(x.shape), str(x.dtype).replace("torch.", ""))
    return repr(x)


def test_the_new_ops_are_registered_and_the_old_schemas_stay():
    for name in NEW_OPS:
        schema = str(getattr(torch.ops.mfa, name).default._schema)
        assert schema.rstrip().endswith("Tensor? sink_logits, Tensor tree_mask) -> (Tensor, Tensor)"), schema
    for name, _impl, _fake, _mutates in tb._CACHE_OPS:
        if name not in NEW_OPS:
            assert "tree_mask" not in str(getattr(torch.ops.mfa, name).default._schema), name
    assert "tree_mask" not in inspect.signature(tb.flash_prefill_ragged).parameters


def test_the_fakes_give_the_right_shapes():
    with FakeTensorMode():
        q, k16, k8, lens, scale, logits, shared, each = operands()
        o, l = torch.ops.mfa.attention_decode_tree(q[:, :, :4], k16, k16, lens, None, True, None, None, 0, 0, None, shared[:4])
        assert o.shape == (2, 8, 4, 64) and o.dtype == torch.bfloat16 and l.shape == (2, 8, 4) and l.dtype == torch.float32
        o, l = torch.ops.mfa.attention_prefill_tree(q, k8, k8, lens, lens, None, True, scale, scale, 4096, 4, logits, each)
        assert o.shape == (2, 8, 40, 64) and o.dtype == torch.bfloat16 and l.shape == (2, 8, 40) and l.dtype == torch.float32
        assert tb.flash_decode(q[:, :, :4], k16, k16, lens, tree_mask=each[:, :4]).shape == (2, 8, 4, 64)
        o, lse = tb.flash_prefill(q.half(), k8, k8, lens, k_scale=scale, window=128, sink_logits=logits, tree_mask=shared, return_lse=True)
        assert o.dtype == torch.float16 and o.shape == (2, 8, 40, 64) and lse.shape == (2, 8, 40)


def outcomes(monkeypatch):
    calls = []
    real = tb._call_op

    def spy(have, name, *args):
        calls.append([name] + [said(a) for a in args])
        return real(have, name, *args)

    monkeypatch.setattr(tb, "_call_op", spy)
    out = {}
    with FakeTensorMode():
        q, k16, k8, lens, scale, logits, shared, each = operands()
        q4 = q[:, :, :4]
        cpu = torch.empty((4,), dtype=torch.int64, device="cpu")
        cases = {
            "decode none": lambda: tb.flash_decode(q4, k16, k16, lens, tree_mask=None),
            "decode window none": lambda: tb.flash_decode(q4, k16, k16, lens, window=7, tree_mask=None),
            "prefill none": lambda: tb.flash_prefill(q, k16, k16, lens, tree_mask=None),
            "decode shared": lambda: tb.flash_decode(q4, k16, k16, lens, tree_mask=shared[:4]),
            "decode per sequence, e4m3, window, sinks": lambda: tb.flash_decode(q4, k8, k8, lens, k_scale=scale, v_scale=scale, window=130, sink_tokens=4,
                                                                                 sink_logits=logits, tree_mask=each[:, :4]),
            "prefill shared": lambda: tb.flash_prefill(q, k16, k16, lens, tree_mask=shared),
            "prefill per sequence, e4m3, window of the rows": lambda: tb.flash_prefill(q, k8, k8, lens, lens, k_scale=scale, window=40, sink_logits=logits,
                                                                                       tree_mask=each),
            "decode with a cap": lambda: tb.flash_decode(q4, k16, k16, lens, softcap=50.0, tree_mask=shared[:4]),
            "prefill with a cap": lambda: tb.flash_prefill(q, k16, k16, lens, softcap=50.0, tree_mask=shared),
            "decode not causal": lambda: tb.flash_decode(q4, k16, k16, lens, causal=False, tree_mask=shared[:4]),
            "prefill window below the rows": lambda: tb.flash_prefill(q, k16, k16, lens, window=39, tree_mask=shared),
            "decode int32 masks": lambda: tb.flash_decode(q4, k16, k16, lens, tree_mask=shared[:4].int()),
            "decode masks of another length": lambda: tb.flash_decode(q4, k16, k16, lens, tree_mask=shared[:5]),
            "prefill masks [R, B]": lambda: tb.flash_prefill(q, k16, k16, lens, tree_mask=each.t()),
            "decode a list": lambda: tb.flash_decode(q4, k16, k16, lens, tree_mask=[1, 3, 7, 15]),
            "decode masks on the host": lambda: tb.flash_decode(q4, k16, k16, lens, tree_mask=cpu),
            "decode a bad window beside a tree": lambda: tb.flash_decode(q4, k16, k16, lens, window=0, tree_mask=shared[:4]),
            "prefill sink tokens without a window beside a tree": lambda: tb.flash_prefill(q, k16, k16, lens, sink_tokens=4, tree_mask=shared),
        }
        for name, call in cases.items():
            del calls[:]
            try:
                call()
                out[name] = list(calls)
            except (ValueError, RuntimeError, TypeError) as e:
                out[name] = [type(e).__name__, str(e)]
    return out


def test_which_op_every_call_reaches_and_the_words_of_every_refusal(monkeypatch):
    got = outcomes(monkeypatch)
    for name, op in (("decode none", "attention_decode"), ("decode window none", "attention_decode_window"), ("prefill none", "attention_prefill"),
                     ("decode shared", "attention_decode_tree"), ("decode per sequence, e4m3, window, sinks", "attention_decode_tree"),
                     ("prefill shared", "attention_prefill_tree"), ("prefill per sequence, e4m3, window of the rows", "attention_prefill_tree")):
        (call,) = got[name]
        assert call[0] == op and (call[-1].startswith("Tensor") and call[-1].endswith("int64")) == op.endswith("_tree"), (name, call)
    assert got["decode per sequence, e4m3, window, sinks"][0][7:] == ["Tensor[2] float32", "Tensor[2] float32", "130", "4", "Tensor[8] float32", "Tensor[2, 4] int64"]
    assert got["prefill shared"][0][-4:] == ["0", "0", "None", "Tensor[40] int64"]
    for name, kind, needle in (("decode with a cap", "ValueError", "tree_mask and softcap together have no kernel"),
                               ("prefill with a cap", "ValueError", "tree_mask and softcap together have no kernel"),
                               ("decode not causal", "ValueError", "tree_mask needs causal=True"),
                               ("prefill window below the rows", "ValueError", "window of at least R = 40"),
                               ("decode int32 masks", "ValueError", "tree_mask must be an int64 tensor [R] = [4]"),
                               ("decode masks of another length", "ValueError", "or [B, R] = [2, 4]"),
                               ("prefill masks [R, B]", "ValueError", "tree_mask must be an int64 tensor [R] = [40]"),
                               ("decode a list", "ValueError", "got list"),
                               ("decode masks on the host", "RuntimeError", "tree_mask must live on q's device"),
                               ("decode a bad window beside a tree", "ValueError", "window must be an int from 1"),
                               ("prefill sink tokens without a window beside a tree", "ValueError", "sink_tokens needs window")):
        assert got[name][0] == kind and needle in got[name][1], (name, got[name])
    assert got == json.load(open(GOLDEN)), "routing or wording moved: tests/golden/tree_routing.json"


def test_pack_tree_mask_packs_bit_j_of_row_r():
    bits = torch.zeros((3, 64, 64), dtype=torch.bool)
    g = torch.Generator().manual_seed(5)
    bits[0] = torch.rand((64, 64), generator=g) < 0.5
    bits[1] = torch.tril(torch.ones((64, 64), dtype=torch.bool))           # the chain
    bits[2, :, 63] = True                                                   # bit 63 alone: the sign of the int64
    packed = tb.pack_tree_mask(bits)
    assert packed.shape == (3, 64) and packed.dtype == torch.int64
    for t in range(3):
        for r in range(64):
            want = sum(1 << j for j in range(64) if bool(bits[t, r, j]))
            assert int(packed[t, r]) % (1 << 64) == want, (t, r)
    assert [int(x) for x in packed[1, :4]] == [1, 3, 7, 15] and int(packed[2, 0]) == -(1 << 63)
    assert tb.pack_tree_mask(bits[1, :5, :5]).tolist() == [1, 3, 7, 15, 31]
    for bad in (torch.zeros((65, 65), dtype=torch.bool), torch.zeros((4, 5), dtype=torch.bool), torch.zeros((4,), dtype=torch.bool)):
        with pytest.raises(ValueError, match="pack_tree_mask: expected bool"):
            tb.pack_tree_mask(bad)
