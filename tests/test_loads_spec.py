"""The restatement of rule 10 (tests/spec_loads.py) against cases worked by hand, and at the extremes of the number formats: the
fold's expression at load = hits = gain = 2^32-1 with keep = 65536 (the largest value it can take: it must fit 64 bits), keep 0,
min_load == max_load, and the saturating sums of the hit column."""
import numpy as np

import spec_loads as spec

M = 0xFFFFFFFF


def test_fold_by_hand():
    # floor(10 * 32768 / 65536) + 3 * 4 = 5 + 12
    assert spec.fold_one(10, 3, 32768, 4, 0, M) == 17
    # floor(7 * 1 / 65536) = 0
    assert spec.fold_one(7, 0, 1, 9, 0, M) == 0
    # floor(65537 * 65535 / 65536) = 65535 (65537 * 65535 = 2^32 - 1)
    assert spec.fold_one(65537, 0, 65535, 0, 0, M) == 65535
    assert spec.fold_one(100, 2, 65536, 5, 0, 105) == 105 and spec.fold_one(100, 2, 65536, 5, 111, M) == 111
    load, H, st = spec.load_fold([10, 7, 1, 9], [3, 0, 2, 5], 3, 32768, 4, 1, 16)
    assert load.tolist() == [16, 3, 8, 9] and H.tolist() == [0, 0, 0, 5]          # the row >= n keeps both
    assert st == {"rows_changed": 3, "hits_folded": 5, "load_before": 18, "load_after": 27, "max_load_after": 16}


def test_the_largest_expression_fits_64_bits_and_clamps():
    x = (M * 65536) // 65536 + M * M
    assert x == M + M * M == 2 ** 64 - 2 ** 32 < 2 ** 64
    assert spec.fold_one(M, M, 65536, M, 0, M) == M
    assert spec.fold_one(M, M, 65536, M, 0, 12) == 12
    load, H, st = spec.load_fold([M, M], [M, 0], 2, 65536, M, 0, M)
    assert load.tolist() == [M, M] and st["rows_changed"] == 0 and st["hits_folded"] == M
    assert st["load_before"] == st["load_after"] == 2 * M and st["max_load_after"] == M


def test_keep_zero_replaces_the_load():
    load, H, st = spec.load_fold([5, 6, 7], [0, 2, M], 3, 0, 3, 0, M)
    assert load.tolist() == [0, 6, M] and not H.any()
    assert st == {"rows_changed": 2, "hits_folded": 2 + M, "load_before": 18, "load_after": 6 + M, "max_load_after": M}


def test_equal_bounds_pin_every_load():
    load, H, st = spec.load_fold([0, 4, M], [9, 0, 0], 3, 65536, 1, 4, 4)
    assert load.tolist() == [4, 4, 4] and st["rows_changed"] == 2 and st["max_load_after"] == 4


def test_no_rows():
    load, H, st = spec.load_fold([3], [2], 0, 0, 0, 0, 0)
    assert load.tolist() == [3] and H.tolist() == [2] and st["max_load_after"] == 0 and st["rows_changed"] == 0


def test_hits_sum_and_saturate():
    H = spec.hits_add(np.zeros(4, np.uint32), [1, 1, 3, 1], None)
    assert H.tolist() == [0, 3, 0, 1]
    H = spec.hits_add(H, [0, 0, 0, 2], [1 << 31, 1 << 31, 1 << 31, 0])
    assert H.tolist() == [M, 3, 0, 1]
    H = spec.hits_merge(H, [1, M - 3, 7])
    assert H.tolist() == [M, M, 7, 1]


def test_used_is_the_sum_over_placed_rows_below_n():
    A = np.array([0, 2, spec.NONE, 2, 5, 1], np.uint32)
    load = np.array([3, 4, 5, M, 7, 9], np.uint32)
    assert spec.used_of(A, load, 5, 3).tolist() == [3, 0, 4 + M]


def test_op_model_counts_only_while_tracking():
    md = spec.OpLoads()
    md.count("a")
    md.on = True
    md.count("a"); md.count("a"); md.count("b")
    assert md.fold(["a", "b", "c"], 0, 10, 1, 100) == (2, 3)
    assert md.load == {"a": 20, "b": 10, "c": 1} and md.hits == {}
