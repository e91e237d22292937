"""CPU test (fake tensors, no device): the torch binding of include/mfa_softcap.h -- the softcap= keyword of flash_decode, flash_prefill
and flash_prefill_ragged is validated in the style of window=, None takes today's op with today's arguments, a cap goes through the new
ops mfa::attention_decode_softcap, mfa::attention_prefill_softcap and mfa::attention_prefill_ragged_softcap, which are registered with
`softcap` last in their schemas and whose fake implementations give the right shapes; the existing ops keep their schemas."""
import pytest

torch = pytest.importorskip("torch")

from torch._subclasses.fake_tensor import FakeTensorMode  # noqa: E402

from metal_flash_attention_amd import torch_binding as tb  # noqa: E402

NEW_OPS = ("attention_decode_softcap", "attention_prefill_softcap", "attention_prefill_ragged_softcap")


@pytest.fixture(scope="module", autouse=True)
def _ops():
    if not tb._HAVE_SOFTCAP_OPS:
        pytest.skip("this torch has no torch.library.custom_op")


def operands():
    q = torch.empty((2, 8, 300, 256), dtype=torch.bfloat16, device="cuda")
    k16 = torch.empty((2, 2, 1024, 256), dtype=torch.bfloat16, device="cuda")
    k8 = torch.empty((2, 2, 1024, 256), dtype=torch.float8_e4m3fn, device="cuda")
    lens = torch.empty((2,), dtype=torch.int32, device="cuda")
    scale = torch.empty((2,), dtype=torch.float32, device="cuda")
    logits = torch.empty((8,), dtype=torch.float32, device="cuda")
    packed = torch.empty((500, 8, 256), dtype=torch.bfloat16, device="cuda")
    starts = torch.empty((3,), dtype=torch.int32, device="cuda")
    return q, k16, k8, lens, scale, logits, packed, starts


def test_the_new_ops_are_registered_and_the_old_schemas_stay():
    for name in NEW_OPS:
        schema = str(getattr(torch.ops.mfa, name).default._schema)
        assert schema.rstrip().endswith("float softcap) -> (Tensor, Tensor)"), schema
        assert "window, SymInt sink_tokens, Tensor? sink_logits, float softcap" in schema or \
            "window, int sink_tokens, Tensor? sink_logits, float softcap" in schema, schema
    for name in ("attention_decode", "attention_decode_fp8", "attention_decode_window", "attention_decode_sink", "attention_prefill",
                 "attention_prefill_window", "attention_prefill_sink", "attention_prefill_ragged"):
        assert "softcap" not in str(getattr(torch.ops.mfa, name).default._schema), name


def test_the_fakes_give_the_right_shapes():
    with FakeTensorMode():
        q, k16, k8, lens, scale, logits, packed, starts = operands()
        o, l = torch.ops.mfa.attention_decode_softcap(q[:, :, :2], k16, k16, lens, None, True, None, None, 0, 0, None, 50.0)
        assert o.shape == (2, 8, 2, 256) and o.dtype == torch.bfloat16 and l.shape == (2, 8, 2) and l.dtype == torch.float32
        o, l = torch.ops.mfa.attention_prefill_softcap(q, k8, k8, lens, lens, None, True, scale, scale, 4096, 4, logits, 30.0)
        assert o.shape == (2, 8, 300, 256) and o.dtype == torch.bfloat16 and l.shape == (2, 8, 300) and l.dtype == torch.float32
        o, l = torch.ops.mfa.attention_prefill_ragged_softcap(packed, k16, k16, lens, starts, 300, None, True, None, None, 0, 0, None, 50.0)
        assert o.shape == (500, 8, 256) and l.shape == (8, 500) and l.dtype == torch.float32
        # and through the public functions
        assert tb.flash_decode(q[:, :, :1], k16, k16, lens, softcap=50.0).shape == (2, 8, 1, 256)
        o, lse = tb.flash_decode(q[:, :, :1].half(), k8, k8, lens, k_scale=scale, window=4096, sink_logits=logits, softcap=30, return_lse=True)
        assert o.dtype == torch.float16 and o.shape == (2, 8, 1, 256) and lse.shape == (2, 8, 1)
        assert tb.flash_prefill(q, k16, k16, lens, window=65, sink_tokens=4, softcap=50.0).shape == (2, 8, 300, 256)
        o, lse = tb.flash_prefill_ragged(packed, k16, k16, lens, starts, 300, softcap=50.0, return_lse=True)
        assert o.shape == (500, 8, 256) and lse.shape == (8, 500)


def test_none_takes_todays_op_and_a_cap_the_new_one(monkeypatch):
    calls = []
    real = tb._call_op

    def spy(have, name, *args):
        calls.append((name, args))
        return real(have, name, *args)

    monkeypatch.setattr(tb, "_call_op", spy)
    with FakeTensorMode():
        q, k16, k8, lens, scale, logits, packed, starts = operands()
        q1 = q[:, :, :1]
        today = [("attention_decode", lambda **kw: tb.flash_decode(q1, k16, k16, lens, **kw)),
                 ("attention_decode_fp8", lambda **kw: tb.flash_decode(q1, k8, k8, lens, k_scale=scale, **kw)),
                 ("attention_decode_window", lambda **kw: tb.flash_decode(q1, k16, k16, lens, window=7, **kw)),
                 ("attention_decode_sink", lambda **kw: tb.flash_decode(q1, k16, k16, lens, sink_logits=logits, **kw)),
                 ("attention_prefill", lambda **kw: tb.flash_prefill(q, k16, k16, lens, **kw)),
                 ("attention_prefill_window", lambda **kw: tb.flash_prefill(q, k16, k16, lens, window=7, **kw)),
                 ("attention_prefill_sink", lambda **kw: tb.flash_prefill(q, k16, k16, lens, window=7, sink_tokens=2, **kw)),
                 ("attention_prefill_ragged", lambda **kw: tb.flash_prefill_ragged(packed, k16, k16, lens, starts, 300, window=7, **kw))]
        for name, call in today:
            del calls[:]
            call()
            (plain, plain_args), = calls
            del calls[:]
            call(softcap=None)
            (again, again_args), = calls
            assert plain == again == name and len(plain_args) == len(again_args)
            assert all(a is b or a == b for a, b in zip(plain_args, again_args)), name
            del calls[:]
            call(softcap=50)
            (capped, capped_args), = calls
            assert capped == ("attention_prefill_ragged_softcap" if "ragged" in name else name.split("_")[0] + "_" + name.split("_")[1] + "_softcap")
            assert capped_args[-1] == 50.0 and isinstance(capped_args[-1], float)


def test_the_keyword_is_validated_like_window():
    with FakeTensorMode():
        q, k16, _k8, lens, _scale, _logits, packed, starts = operands()
        calls = (lambda cap: tb.flash_decode(q[:, :, :1], k16, k16, lens, softcap=cap),
                 lambda cap: tb.flash_prefill(q, k16, k16, lens, window=7, softcap=cap),
                 lambda cap: tb.flash_prefill_ragged(packed, k16, k16, lens, starts, 300, softcap=cap))
        for who, call in zip(("flash_decode", "flash_prefill", "flash_prefill_ragged"), calls):
            for bad in (True, False, "50", [50.0], 0, 0.0, -1, -30.0, float("nan"), float("inf"), float("-inf")):
                with pytest.raises(ValueError, match=who + ": softcap must be a finite number > 0"):
                    call(bad)
            call(1)
            call(1e-3)
        # the window and the sinks beside a cap are still checked
        with pytest.raises(ValueError, match="window must be an int"):
            tb.flash_decode(q[:, :, :1], k16, k16, lens, window=0, softcap=50.0)
        with pytest.raises(ValueError, match="sink_tokens needs window"):
            tb.flash_prefill(q, k16, k16, lens, sink_tokens=4, softcap=50.0)
        with pytest.raises(ValueError, match="needs causal"):
            tb.flash_prefill_ragged(packed, k16, k16, lens, starts, 300, window=5, causal=False, softcap=50.0)
