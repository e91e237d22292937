"""Which torch op, with which arguments, the public functions over a KV cache reach -- flash_decode, flash_prefill and
flash_prefill_ragged -- pinned without a GPU: `_call_op` of torch_binding sits behind a recorder, the tensors are FakeTensorMode's.
Every rung (none, window, sinks, soft cap and their combinations) over a 16-bit cache, an e4m3 cache and a 16-bit cache that is handed
scales; for the inputs a function refuses, the exception's type and message, among them the ones where two things are wrong and the order
of the checks decides which one speaks.  The fixture tests/golden/cache_routing.json is written by this module's own recorder:

    PYTHONPATH=. python tests/test_cache_routing.py        # rewrites the fixture from the sources as they are
"""
import json
import os

import pytest

torch = pytest.importorskip("torch")
from torch._subclasses.fake_tensor import FakeTensorMode   # noqa: E402

from metal_flash_attention_amd import torch_binding as tb   # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cache_routing.json")

B, H, HKV, C, D, T = 2, 8, 2, 256, 128, 100


def _describe(v, names):
    """an argument as the fixture holds it: a tensor by the name of the operand it is (`names`: id -> name; the functions hand their
    tensors on as they are), a float in a list so that 50.0 is not 50"""
    if isinstance(v, torch.Tensor):
        return names[id(v)]
    if isinstance(v, float):
        return [v]
    assert v is None or isinstance(v, (bool, int)), v
    return v


def _operands():
    """fake tensors by name (call under FakeTensorMode)"""
    def t(shape, dtype=torch.bfloat16, device="cuda"):
        return torch.empty(shape, dtype=dtype, device=device)
    o = dict(q=t((B, H, 1, D)), q70=t((B, H, 70, D)), qp=t((T, H, D)), k=t((B, HKV, C, D)), k8=t((B, HKV, C, D), torch.float8_e4m3fn),
             lens=t((B,), torch.int32), qlens=t((B,), torch.int32), starts=t((B + 1,), torch.int32), table=t((B, 16), torch.int32),
             ks=t((HKV,), torch.float32), logits=t((H,), torch.float32), logits_h3=t((3,), torch.float32), logits_f16=t((H,), torch.float16),
             logits_cpu=t((H,), torch.float32, "cpu"), q_cpu=t((B, H, 1, D), device="cpu"), qp_cpu=t((T, H, D), device="cpu"),
             lens_cpu=t((B,), torch.int32, "cpu"))
    o["q_grad"] = t((B, H, 1, D)).requires_grad_()
    o["qp_grad"] = t((T, H, D)).requires_grad_()
    return o


# the rungs: keyword set -> keywords (operand names as strings)
RUNGS = {
    "none": {},
    "window": dict(window=7),
    "sink_tokens_window": dict(window=7, sink_tokens=2),
    "sink_logits": dict(sink_logits="logits"),
    "window_sink_tokens_sink_logits": dict(window=7, sink_tokens=2, sink_logits="logits"),
    "softcap": dict(softcap=50.0),
    "softcap_window": dict(softcap=50.0, window=7),
    "softcap_sink_tokens_window": dict(softcap=50.0, window=7, sink_tokens=2),
    "softcap_sink_logits": dict(softcap=50.0, sink_logits="logits"),
    "softcap_all": dict(softcap=50.0, window=7, sink_tokens=2, sink_logits="logits"),
}
# other spellings, over the 16-bit cache only
SPELLINGS = {
    "all_none": dict(window=None, sink_tokens=None, sink_logits=None, softcap=None),
    "softcap_int": dict(softcap=30),
    "not_causal_sink_logits_softcap": dict(causal=False, sink_logits="logits", softcap=50.0),
    "paged_lse": dict(block_table="table", return_lse=True),
}
# the caches: name -> (k_cache and v_cache, keywords)
CACHES = {"bf16": ("k", {}), "e4m3": ("k8", dict(k_scale="ks")), "bf16_with_scales": ("k", dict(v_scale="ks"))}

# what the functions refuse: keyword set -> keywords; `q` / `cache_lengths` replace the function's own operand
REFUSALS = {
    "window_0": dict(window=0),
    "window_bool": dict(window=True),
    "window_float": dict(window=7.0),
    "window_2_32": dict(window=2 ** 32),
    "window_not_causal": dict(window=7, causal=False),
    "sink_tokens_0": dict(window=7, sink_tokens=0),
    "sink_tokens_no_window": dict(sink_tokens=2),
    "sink_tokens_not_causal": dict(window=7, sink_tokens=2, causal=False),
    "sink_logits_shape": dict(sink_logits="logits_h3"),
    "sink_logits_dtype": dict(sink_logits="logits_f16"),
    "sink_logits_not_a_tensor": dict(sink_logits=1.0),
    "sink_logits_device": dict(sink_logits="logits_cpu"),
    "softcap_0": dict(softcap=0),
    "softcap_nan": dict(softcap=float("nan")),
    "softcap_bool": dict(softcap=True),
    "softcap_text": dict(softcap="50"),
    "q_cpu": dict(q="cpu"),
    "lengths_cpu": dict(cache_lengths="lens_cpu"),
    "requires_grad": dict(q="grad"),
    # two things wrong: the order of the checks decides
    "q_cpu_and_softcap_0": dict(q="cpu", softcap=0),
    "requires_grad_and_window_0": dict(q="grad", window=0),
    "softcap_0_and_window_0": dict(softcap=0, window=0),
    "softcap_0_and_sink_tokens_no_window": dict(softcap=0, sink_tokens=2),
    "window_0_and_sink_tokens_0": dict(window=0, sink_tokens=0),
    "window_not_causal_and_sink_logits_shape": dict(window=7, causal=False, sink_logits="logits_h3"),
    "sink_tokens_no_window_and_sink_logits_shape": dict(sink_tokens=2, sink_logits="logits_h3"),
    "sink_tokens_0_and_softcap_nan": dict(window=7, sink_tokens=0, softcap=float("nan")),
    "scales_16bit_and_window_0": dict(v_scale="ks", window=0),
    "scales_16bit_and_softcap_0": dict(v_scale="ks", softcap=0),
    "scales_16bit_and_q_cpu": dict(v_scale="ks", q="cpu"),
}

FUNCTIONS = {
    "flash_decode": lambda t, k, q, lens, kw: tb.flash_decode(t[q or "q"], t[k], t[k], t[lens or "lens"], **kw),
    "flash_prefill": lambda t, k, q, lens, kw: tb.flash_prefill(t[q or "q70"], t[k], t[k], t[lens or "lens"], q_lengths=t["qlens"], **kw),
    "flash_prefill_ragged": lambda t, k, q, lens, kw: tb.flash_prefill_ragged(t[q or "qp"], t[k], t[k], t[lens or "lens"], t["starts"], 70, **kw),
}


def _cases():
    for function in FUNCTIONS:
        for cache, (k, cache_kw) in CACHES.items():
            for rung, kw in dict(RUNGS, **(SPELLINGS if cache == "bf16" else {})).items():
                yield f"{function}/{cache}/{rung}", function, k, dict(cache_kw, **kw)
        for refusal, kw in REFUSALS.items():
            yield f"{function}/refused/{refusal}", function, "k", dict(kw)
    # the packed q of a ragged batch is shown to the sink checks as a [1, H, T, D] view; a q that is not packed, as it is
    yield "flash_prefill_ragged/refused/q_not_packed_sink_logits_shape", "flash_prefill_ragged", "k", dict(q="q70", sink_logits="logits_h3")
    yield "flash_prefill_ragged/bf16/q_not_packed_sink_logits", "flash_prefill_ragged", "k", dict(q="q70", sink_logits="logits")


def _run(function, k, keywords, monkeypatch):
    """-> [the one op reached, its arguments], or [the exception's type, its message]"""
    calls, names = [], {}

    def record(have, name, *args):
        assert isinstance(have, bool)
        calls.append([name, [_describe(a, names) for a in args]])
        return args[0], args[0]
    monkeypatch.setattr(tb, "_call_op", record)
    with FakeTensorMode():
        t = _operands()
        names.update((id(v), name) for name, v in t.items())
        kw = {key: t[v] if isinstance(v, str) and v in t else v for key, v in keywords.items() if key not in ("q", "cache_lengths")}
        q = keywords.get("q")
        if q in ("cpu", "grad"):
            q = ("qp_" if function == "flash_prefill_ragged" else "q_") + q
        try:
            FUNCTIONS[function](t, k, q, keywords.get("cache_lengths"), kw)
        except (ValueError, TypeError, RuntimeError) as e:
            assert not calls, "no op is reached after a refusal"
            return [type(e).__name__, str(e)]
    (call,) = calls
    return call


def record():
    mp = pytest.MonkeyPatch()
    try:
        return {case: json.loads(json.dumps(_run(function, k, kw, mp))) for case, function, k, kw in _cases()}
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


_CASES = list(_cases())


def test_the_fixture_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(case for case, *_ in _CASES)


def test_every_op_is_reached_and_every_refusal_refuses(golden):
    reached = {v[0] for v in golden.values() if isinstance(v[1], list)}
    assert reached == {"attention_decode", "attention_decode_fp8", "attention_decode_window", "attention_decode_sink", "attention_decode_softcap",
                       "attention_prefill", "attention_prefill_window", "attention_prefill_sink", "attention_prefill_softcap",
                       "attention_prefill_ragged", "attention_prefill_ragged_softcap"}
    assert all(isinstance(v[1], str) for case, v in golden.items() if "/refused/" in case), [c for c, v in golden.items() if "/refused/" in c and isinstance(v[1], list)]


@pytest.mark.parametrize("case,function,k,keywords", _CASES, ids=[c[0] for c in _CASES])
def test_public_function_reaches_the_op_with_the_arguments(case, function, k, keywords, golden, monkeypatch):
    assert json.loads(json.dumps(_run(function, k, keywords, monkeypatch))) == golden[case]


if __name__ == "__main__":
    fixture = record()
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(case) + ":" + json.dumps(fixture[case], separators=(",", ":")) for case in sorted(fixture)) + "\n}\n")   # a case a line
    print(f"wrote {GOLDEN}: {len(fixture)} cases, {os.path.getsize(GOLDEN)} bytes")
