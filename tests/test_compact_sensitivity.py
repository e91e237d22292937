"""CPU test: what the case list of tests/test_compact_gpu.py can see.  Over the exact list that file imports (compact_model.CASES): every
wrong kernel of compact_model.MUTANTS changes at least one byte of a cache or one length in at least one case, so the byte-for-byte
comparison on the GPU would catch it; and the model itself changes nothing outside the slots [P, P + a) of each sequence and newLengths.
The condition on the list: no mutant survives it."""
import functools

import numpy as np
import pytest

import compact_model as cm


@functools.lru_cache(maxsize=None)
def expected(index):
    return cm.run(cm.CASES[index])


def differs(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a, b))


def test_the_list_crosses_every_configuration_with_every_path():
    assert len(cm.CASES) == len(cm.CONFIGS) * len(cm.PATHS) == 6 * 16
    assert len({cm.case_id(case) for case in cm.CASES}) == len(cm.CASES)
    assert {(c.D, c.element, c.layout, c.page) for c in cm.CONFIGS} == {
        (64, "e4m3", "contiguous", 0), (64, "bf16", "token-major", 0), (128, "f16", "paged", 16), (128, "e4m3", "paged", 16),
        (256, "bf16", "contiguous", 0), (256, "e4m3", "paged", 64)}
    assert all(path.rows <= 64 and path.accepted.shape == (cm.B, path.accepted.shape[1]) for path in cm.PATHS)
    # the seams the paths name: P not a multiple of a page, tree rows across a page of 16 and of 64
    for page in (16, 64):
        assert all((n - cm.ROWS) % page for n in cm.LENS)
        assert any((n - cm.ROWS) // page != (n - 1) // page for n in cm.LENS)


@pytest.mark.parametrize("mutant", cm.MUTANTS)
def test_no_mutant_survives_the_list(mutant):
    caught = [cm.case_id(case) for index, case in enumerate(cm.CASES) if differs(cm.run(case, mutant)[3], expected(index)[3])]
    print("%s: told from the model by %d of %d cases" % (mutant, len(caught), len(cm.CASES)))
    assert caught, f"the case list cannot tell the mutant {mutant} from the model"


def test_the_model_moves_something_in_every_configuration():
    for config in cm.CONFIGS:
        moved = [path.name for index, (c, path) in enumerate(cm.CASES) if c == config
                 and differs(expected(index)[3][:2], expected(index)[:2])]
        assert len(moved) >= 8, (config, moved)


@pytest.mark.parametrize("index", range(len(cm.CASES)), ids=[cm.case_id(case) for case in cm.CASES])
def test_the_model_changes_nothing_outside_the_destination_slots(index):
    (config, path), (k, v, geo, (k2, v2, new)) = cm.CASES[index], expected(index)
    inside = np.zeros(k.shape, dtype=bool)
    for b in range(cm.B):
        n, qn, P, live, a = cm.plan(geo, path.lens, path.rows, path.qlens, path.counts, path.accepted.shape[1], b)
        assert int(new[b]) == P + a <= max(n, 0) and a <= live <= path.rows
        for pos in range(P, P + a):
            slot = geo.slot(b, pos)
            for h in range(cm.HKV):
                if slot is not None:
                    inside[geo.at(slot, h):geo.at(slot, h) + geo.row_bytes] = True
    for before, after in ((k, k2), (v, v2)):
        assert np.array_equal(before[~inside], after[~inside]), "a byte outside the slots [P, P + a) changed"
    if path.name in ("identity", "a = 0"):
        assert np.array_equal(k, k2) and np.array_equal(v, v2)
