"""CPU test (no GPU call): the poison of tests/cache_kit.py, which alone proves that a kernel never loads what it must not.

One batch of three sequences of 0, 37 and 128 keys in caches of 128 keys, one K / V head, D = 8, page size 16; a window-shaped mask
(keys from 20 on), a tile-shaped mask (tile 0 kept, tile 1 not) and the all-true mask; a bf16 cache (poison NaN) and an e4m3 cache
(poison 0x7f).  poisoned() keeps exactly the kept keys below each length, bit for bit, and every other key is poison; in pool_host()
every kept key lies, bit for bit, in the page its table entry names at its offset in the page, every other element of the pool is
poison, every entry without a kept key names the spare page, which is all poison, and no two entries that hold keys name the same page.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402

LENS, C, D, PAGE = (0, 37, 128), 128, 8, 16
BATCH = ck.Batch(tuple((n, 1) for n in LENS), C, 1, 1)
BELOW = np.arange(C)[None, :] < np.array(LENS)[:, None]
# name -> (the kit's mask, the same mask written out here)
MASKS = {"window": (BATCH.keep(firsts=[20] * 3), BELOW & (np.arange(C) >= 20)[None, :]),
         "tiles": (BATCH.keep(tiles=[np.array([True, False])] * 3), BELOW & (np.arange(C) < 64)[None, :]),
         "all": (BATCH.keep(), BELOW)}


def cache(fp8, seed):
    """a [3, 1, C, D] cache without a poison pattern in it, as bytes (e4m3) or 16-bit patterns (bf16), and the poison's test"""
    x = torch.rand(3, 1, C, D, generator=torch.Generator().manual_seed(seed)) * 2 - 1
    if fp8:
        return x.to(torch.float8_e4m3fn), lambda t: t.view(torch.uint8) == 0x7F
    return x.to(torch.bfloat16), torch.isnan


@pytest.mark.parametrize("mask", sorted(MASKS))
def test_the_masks_are_the_keys_below_each_length_inside_the_shape(mask):
    got, want = MASKS[mask]
    assert got.shape == (3, C) and got.dtype == bool and np.array_equal(got, want)
    assert not got[0].any() and got[2].sum() == {"window": 108, "tiles": 64, "all": 128}[mask]


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("mask", sorted(MASKS))
def test_poisoned_keeps_exactly_the_kept_keys(mask, fp8):
    keep = torch.from_numpy(MASKS[mask][1])
    t, is_poison = cache(fp8, 1)
    assert not is_poison(t).any()
    before = ck.raw(t).clone()
    out = ck.poisoned(t, MASKS[mask][0])
    assert out.dtype == t.dtype and torch.equal(ck.raw(t).view(torch.uint8), before.view(torch.uint8)), "the source was modified"
    bits = lambda x: ck.raw(x).contiguous().view(torch.uint8).reshape(3, C, -1)  # noqa: E731
    assert torch.equal(bits(out[:, 0])[keep], bits(t[:, 0])[keep]), "a kept key changed"
    assert bool(is_poison(out)[:, 0][~keep].all()), "a key that is not kept holds a value"
    assert not is_poison(out)[:, 0][keep].any()


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("mask", sorted(MASKS))
def test_the_pool_holds_the_kept_keys_in_the_named_pages_and_poison_elsewhere(mask, fp8):
    keep = MASKS[mask][1]
    (k, is_poison), (v, _) = cache(fp8, 2), cache(fp8, 3)
    pk, pv, table = ck.pool_host(k, v, PAGE, MASKS[mask][0], seed=5)
    pps = C // PAGE
    spare = pk.shape[0] - 1
    assert pk.shape == pv.shape == (3 * pps + 1, 1, PAGE, D) and pk.dtype == k.dtype and table.shape == (3, pps) and table.dtype == np.int32
    assert 0 <= table.min() and table.max() <= spare, "a table entry outside the pool"
    bits = lambda x: ck.raw(x).contiguous().view(torch.uint8).reshape(x.shape[0], x.shape[1], -1)  # noqa: E731
    for pool, src in ((pk, k), (pv, v)):
        named = torch.zeros(pool.shape[0], PAGE, dtype=torch.bool)       # the elements of the pool that hold a kept key
        for b in range(3):
            for c in np.nonzero(keep[b])[0]:
                pg, at = int(table[b, c // PAGE]), int(c % PAGE)
                assert pg != spare and not named[pg, at]
                named[pg, at] = True
                assert torch.equal(bits(pool[pg, 0])[at], bits(src[b, 0])[int(c)]), "a kept key is not where its table entry says"
        assert int(named.sum()) == int(keep.sum())
        assert bool(is_poison(pool)[:, 0][~named].all()), "an element of the pool that holds no kept key is not poison"
        assert bool(is_poison(pool[spare]).all())
    holds = keep.reshape(3, pps, PAGE).any(axis=2)
    assert (table[~holds] == spare).all(), "an entry without a kept key must name the spare page"
    assert len(set(table[holds].tolist())) == int(holds.sum()), "two entries that hold keys name the same page"


def test_the_all_true_mask_reproduces_the_keys_below_n():
    t, is_poison = cache(False, 4)
    out = ck.poisoned(t, BATCH.keep())
    for b, n in enumerate(LENS):
        assert torch.equal(out[b, :, :n].view(torch.int16), t[b, :, :n].view(torch.int16)) and bool(is_poison(out[b, :, n:]).all())
    assert np.array_equal(BATCH.keep(), BATCH.keep(firsts=[0] * 3)) and np.array_equal(BATCH.keep(), BATCH.keep(tiles=[np.ones(2, dtype=bool)] * 3))
