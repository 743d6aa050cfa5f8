"""The restatement of the object-class rules (tests/spec_classes.py) against hand-made cases, against its own vectorised forms,
and against the plain sweep's restatement: with one class it is tests/spec_expire.py.  No GPU needed."""
import numpy as np
import pytest

import spec_classes as spec
import spec_expire

NONE = spec.NONE


def test_setters_by_hand():
    K = np.array([9, 9, 9, 9, 9, 9], np.uint8)
    K1 = spec.set_classes(K, 2, [1, 2, 3])
    assert K1.tolist() == [9, 9, 1, 2, 3, 9] and K.tolist() == [9] * 6          # a copy: the input stays
    assert spec.set_classes(K, 6, []).tolist() == [9] * 6
    # the scatter: of several entries for one row the last wins, wherever the others stand
    K2 = spec.set_class_batch(K, [4, 0, 4, 5, 4, 0], [1, 2, 3, 255, 7, 0])
    assert K2.tolist() == [0, 9, 9, 9, 7, 255]


def test_sweep_by_hand():
    #            row  0     1     2     3     4     5     6     7
    A = np.array([3, NONE, 5, 0xFFFFFFF0, 1, 2, 2, 7], np.uint32)
    S = np.array([4, 0, 9, 0, 10, 0, 3, 0], np.uint32)
    K = np.array([0, 0, 1, 2, 1, 3, 200, 0], np.uint8)
    load = np.array([10, 20, 30, 40, 50, 60, 70, 80], np.uint32)
    cut = [5, 10, 0xFFFFFFFF, 0]       # class 3: cutoff 0 finds nothing; class 200 >= n_classes: never idle
    rows, nodes, n_idle, freed, A2, by = spec.expire_classes(A, S, K, load, 7, cut)   # n = 7: row 7 is never idle
    assert rows.tolist() == [0, 2, 3] and nodes.tolist() == [3, 5, 0xFFFFFFF0] and n_idle == 3 and freed == 80
    assert by.tolist() == [1, 1, 1, 0]
    assert A2.tolist() == [NONE, NONE, NONE, NONE, 1, 2, 2, 7]
    # S[r] == cutoff is not idle (row 4: S = 10, cutoff 10); one below is
    assert 4 not in rows
    # a page: n_idle and idle_by_class count every idle row, the listing and the freed load only the page
    rows, nodes, n_idle, freed, A2, by = spec.expire_classes(A, S, K, load, 7, cut, cap=2)
    assert rows.tolist() == [0, 2] and n_idle == 3 and freed == 40 and by.tolist() == [1, 1, 1, 0]
    assert A2.tolist() == [NONE, NONE, NONE, 0xFFFFFFF0, 1, 2, 2, 7]
    # count only
    rows, nodes, n_idle, freed, A2, by = spec.expire_classes(A, S, K, load, 7, cut, cap=0)
    assert len(rows) == 0 and n_idle == 3 and freed == 0 and np.array_equal(A2, A)
    # fewer classes: rows of class 1 and 2 are out of range now
    assert spec.expire_classes(A, S, K, load, 7, [5])[0].tolist() == [0]
    with pytest.raises(AssertionError):
        spec.expire_classes(A, S, K, load, 7, [])


def test_census_by_hand():
    A = np.array([0, 1, NONE, 1, 5, 0, 1], np.uint32)
    K = np.array([0, 1, 1, 1, 0, 7, 0], np.uint8)
    load = np.array([1, 2, 4, 8, 16, 32, 0xFFFFFFFF], np.uint32)
    assert spec.census(A, K, load, 7, 2) == ([3, 2], [1 + 16 + 0xFFFFFFFF, 10], 1)          # row 5: class 7 -> other
    assert spec.census(A, K, load, 6, 2) == ([2, 2], [17, 10], 1)                           # n = 6: row 6 is not counted
    rows, lsum, other = spec.census(A, K, load, 7, 2, m=2)
    assert rows == [[1, 0], [1, 2]] and lsum == [[1, 0], [0xFFFFFFFF, 10]] and other == 2    # row 4: node 5 >= m -> other
    assert spec.census(A, K, load, 7, 8)[2] == 0 and spec.census(A, K, load, 7, 8)[0][7] == 1


def _random(seed, n):
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 6, n).astype(np.uint32)
    A[rng.random(n) < 0.3] = NONE
    A[rng.random(n) < 0.05] = 0xFFFFFFF0
    S = rng.integers(0, 8, n).astype(np.uint32)
    K = rng.integers(0, 5, n).astype(np.uint8)
    K[rng.random(n) < 0.1] = 255
    load = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return rng, A, S, K, load


@pytest.mark.parametrize("seed", range(6))
def test_with_one_class_the_sweep_is_the_plain_sweep(seed):
    rng, A, S, K, load = _random(seed, 300)
    K[:] = 0
    for cutoff in (0, 1, 4, 8, 0xFFFFFFFF):
        for cap in (None, 0, 1, 17, 1 << 40):
            for n in (0, 1, 299, 300):
                w = spec_expire.expire(A, S, load, n, cutoff, cap)
                g = spec.expire_classes(A, S, K, load, n, [cutoff], cap)
                assert all(np.array_equal(x, y) for x, y in zip(w, g[:5]))
                assert g[5].tolist() == [w[2]]


@pytest.mark.parametrize("seed", range(6))
def test_the_vectorised_forms_are_the_restatement(seed):
    rng, A, S, K, load = _random(100 + seed, 257)
    for nc in (1, 2, 4, 37, 256):
        cut = rng.integers(0, 9, nc).astype(np.uint32)
        cut[rng.integers(0, nc)] = 0xFFFFFFFF
        for n in (0, 5, 257):
            for cap in (None, 0, 3):
                a = spec.expire_classes(A, S, K, load, n, cut, cap)
                b = spec.expire_classes_np(A, S, K, load, n, cut, cap)
                assert all(np.array_equal(x, y) for x, y in zip(a, b))
            for m in (None, 1, 4, 6):
                r, l, o = spec.census(A, K, load, n, nc, m)
                rn, ln, on = spec.census_np(A, K, load, n, nc, m)
                assert rn.tolist() == r and ln.tolist() == l and on == o
