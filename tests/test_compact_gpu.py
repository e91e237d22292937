"""GPU test: the KV-cache compaction of include/mfa_compact.h through the C ABI, byte for byte against tests/compact_model.py.  Every case
of compact_model.CASES -- six cache configurations (64 / 128 / 256, e4m3 / bf16 / f16, contiguous, token-major, pages of 16 shuffled and of 64)
crossed with sixteen paths (identity ... a negative table entry) -- compares the WHOLE K and V buffers, the whole pool with the pages no
table names, and newLengths.  The caches hold bytes that identify (sequence, head, slot, K or V).  What the list can see:
tests/test_compact_sensitivity.py, on the CPU."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402
import compact_model as cm  # noqa: E402
from metal_flash_attention_amd import GEMMOperandPrecision as P, KVCacheCompact, KVCachePrecision  # noqa: E402

PRECISION = {"e4m3": KVCachePrecision.E4M3, "bf16": P.BF16, "f16": P.FP16}
SENTINEL = 0xDEADBEEF


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def u32(values):
    """uint32 values as the int32 tensor that holds their bits, on the device"""
    return ck.dev(np.asarray(values, dtype=np.uint32).view(np.int32))


@functools.lru_cache(maxsize=None)
def expected(index):
    return cm.run(cm.CASES[index])


def launch_keywords(config, geo, path):
    """the keywords of KVCacheCompact.dispatch for a case (strides in elements), and the tensors they point to"""
    e = cm.ELEMENT_BYTES[config.element]
    strides = (geo.ld // e, geo.hs // e, 0 if geo.page else geo.outer // e)
    kw = dict(rows=path.rows, heads=cm.HKV, batches=cm.B, cacheLengths=u32(path.lens), accepted=ck.dev(path.accepted),
              acceptedStride=path.accepted.shape[1], maxAccepted=path.accepted.shape[1], acceptedCounts=u32(path.counts),
              newLengths=u32([SENTINEL] * cm.B), queryLengths=None if path.qlens is None else u32(path.qlens),
              strides=dict(kCache=strides, vCache=strides))
    if geo.page:
        kw.update(pageSize=geo.page, blockTable=ck.dev(np.ascontiguousarray(geo.table)), blockTableStride=geo.table.shape[1],
                  pageStrides=(geo.outer // e, geo.outer // e))
    else:
        kw.update(column=geo.column)
    return kw


@pytest.mark.parametrize("index", range(len(cm.CASES)), ids=[cm.case_id(case) for case in cm.CASES])
def test_the_launch_is_the_model_byte_for_byte(index):
    (config, path), (k, v, geo, (want_k, want_v, want_new)) = cm.CASES[index], expected(index)
    dk, dv = ck.dev(k.copy()), ck.dev(v.copy())
    kw = launch_keywords(config, geo, path)
    KVCacheCompact(config.D, PRECISION[config.element]).dispatch(dk, dv, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    got_k, got_v = dk.cpu().numpy(), dv.cpu().numpy()
    got_new = kw["newLengths"].cpu().numpy().view(np.uint32)
    assert np.array_equal(got_new, want_new), f"newLengths {got_new.tolist()}, the model says {want_new.tolist()}"
    for name, got, want in (("K", got_k, want_k), ("V", got_v, want_v)):
        wrong = np.flatnonzero(got != want)
        assert wrong.size == 0, f"{name}: {wrong.size} bytes differ from the model, the first at byte {int(wrong[0]) if wrong.size else -1}"
    # what the launch read is as it was: the lengths, the path, the counts, the table
    assert np.array_equal(kw["cacheLengths"].cpu().numpy().view(np.uint32), np.asarray(path.lens, dtype=np.uint32))
    assert np.array_equal(kw["accepted"].cpu().numpy(), path.accepted)
    if geo.page:
        assert np.array_equal(kw["blockTable"].cpu().numpy(), geo.table)


def test_no_newlengths_and_a_wider_accepted_stride():
    """newLengths NULL moves the same bytes; accepted rows further apart than maxAccepted are read at their stride"""
    index = next(i for i, (c, p) in enumerate(cm.CASES) if c.D == 128 and c.element == "f16" and p.name == "rotation by one")
    (config, path), (k, v, geo, (want_k, want_v, _new)) = cm.CASES[index], expected(index)
    dk, dv = ck.dev(k.copy()), ck.dev(v.copy())
    kw = launch_keywords(config, geo, path)
    wide = np.full((cm.B, path.accepted.shape[1] + 5), 3, dtype=np.int32)
    wide[:, :path.accepted.shape[1]] = path.accepted
    kw.update(newLengths=None, accepted=ck.dev(wide), acceptedStride=wide.shape[1])
    KVCacheCompact(config.D, PRECISION[config.element]).dispatch(dk, dv, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(dk.cpu().numpy(), want_k) and np.array_equal(dv.cpu().numpy(), want_v)
