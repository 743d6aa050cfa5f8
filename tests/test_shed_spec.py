"""Rule 14 on the CPU: the sequential and the threshold form of L1 (tests/spec_shed.py) name the same surplus rows on random
tables, and hand-written tables pin each clause of L0 - L3."""
import numpy as np
import pytest

import shed_tables as tb
import spec_shed as spec

NONE, INACTIVE, NEVER = spec.NONE, spec.AFF_INACTIVE, spec.NEVER


def u32(*a):
    return np.array(a, np.uint32)


def one_node(load, S, aff=None, K=None, T=0, **kw):
    """Every row on node 0 of one live node; returns shed()'s tuple."""
    n = len(load)
    A = np.zeros(n, np.uint32)
    aff = np.zeros(n, np.uint32) if aff is None else aff
    return spec.shed(A, u32(*load), aff, u32(*S), K, n, 1, [1], [T], **kw)


@pytest.mark.parametrize("layout", list(tb.LAYOUTS))
def test_both_forms_of_the_cut_agree(layout):
    total = 0
    for seed in range(60):
        rng = np.random.default_rng(seed)
        n, m = int(rng.integers(1, 400)), int(rng.integers(1, 9))
        A, load, aff, S, K, alive, T, cutoff = tb.table(seed, n, m, layout, heavy=seed % 3 == 0, classes=seed % 2 * 3)
        cc = None if seed % 4 else [cutoff, 0, cutoff - 1, cutoff]
        imm = {1} if seed % 5 == 0 else None
        cands, pinned = spec.classify(A, load, aff, S, K, n, m, alive, cutoff, cc, imm)
        seq = spec.surplus_sequential(load, S, T, cands, pinned)
        thr = spec.thresholds(load, S, T, cands, pinned)
        assert seq == spec.surplus_threshold(S, cands, thr), seed
        for j, (sigma, cutrow, rem) in thr.items():
            assert cutrow is not None and int(S[cutrow]) == sigma and int(A[cutrow]) == j and rem >= 0
        total += len(seq)
    assert total > 200


def test_longest_idle_go_first_and_only_as_many_as_needed():
    st, rows, nodes, A2, _, used = one_node([5, 5, 5, 5], [40, 10, 30, 20], T=12, cutoff=100)
    assert rows == [1, 3] and nodes == [0, 0] and used == [10]      # stamps 40 and 30 stay: 10 <= 12; 20 would make 15
    assert st == {"surplus_rows": 2, "surplus_load": 10, "shed_rows": 2, "shed_load": 10, "nodes_over_before": 1,
                  "nodes_over_after": 0}
    assert list(A2) == [0, NONE, 0, NONE]


def test_the_first_overflow_ends_the_kept_prefix():
    # in order: stamp 9 (load 8) fits 10; stamp 8 (load 5) overflows; stamp 7 (load 1) would fit again but comes later: surplus
    st, rows, *_ = one_node([1, 5, 8], [7, 8, 9], T=10, cutoff=100)
    assert rows == [0, 1]


def test_ties_are_cut_in_row_order_with_different_loads():
    st, rows, *_ = one_node([4, 1, 3, 9, 2], [5, 5, 5, 5, 5], T=8, cutoff=6)
    assert rows == [3, 4]                                           # 4 + 1 + 3 = 8 fits; row 3 overflows, row 4 is later
    cands, pinned = spec.classify(np.zeros(5, np.uint32), u32(4, 1, 3, 9, 2), np.zeros(5, np.uint32), u32(5, 5, 5, 5, 5), None, 5,
                                  1, [1], 6)
    assert spec.thresholds(u32(4, 1, 3, 9, 2), u32(5, 5, 5, 5, 5), [8], cands, pinned) == {0: (5, 3, 8)}


def test_a_zero_load_row_is_never_shed():
    st, rows, *_ = one_node([0, 6, 0, 6], [1, 2, 1, 3], T=0, cutoff=9)
    assert rows == [1, 3] and st["surplus_rows"] == 2


def test_a_non_object_is_pinned_and_counts_against_the_target():
    aff = u32(0, INACTIVE, 0)
    st, rows, *_ = one_node([4, 4, 4], [1, 0, 2], aff=aff, T=8, cutoff=9)
    assert rows == [0]                                              # free = 8 - 4: one candidate fits, the older one goes
    assert st["nodes_over_before"] == 1 and st["nodes_over_after"] == 0


def test_the_largest_stamp_is_below_no_cutoff():
    st, rows, *_ = one_node([4, 4], [0xFFFFFFFF, 0xFFFFFFFE], T=0, cutoff=0xFFFFFFFF)
    assert rows == [1]


def test_cutoff_zero_changes_nothing():
    st, rows, nodes, A2, _, used = one_node([4, 4], [0, 0], T=0, cutoff=0)
    assert rows == [] and st["surplus_rows"] == 0 and st["nodes_over_before"] == st["nodes_over_after"] == 1
    assert list(A2) == [0, 0] and used == [8]


def test_pinned_load_alone_above_the_target_sheds_every_candidate_and_stays_over():
    st, rows, *_ = one_node([50, 3, 4], [9, 1, 2], T=20, cutoff=9)    # stamp 9 is not below 9: pinned, 50 > 20
    assert rows == [1, 2] and st["nodes_over_before"] == 1 and st["nodes_over_after"] == 1


def test_classes_from_n_classes_on_are_never_shed():
    K = np.array([0, 1, 2, 3], np.uint8)
    st, rows, *_ = one_node([5, 5, 5, 5], [1, 1, 1, 1], K=K, T=0, cutoff=0, class_cutoffs=[9, 0, 9])
    assert rows == [0, 2]                                           # class 1: cutoff 0; class 3 >= n_classes


def test_an_immovable_class_is_never_shed_in_either_form():
    K = np.array([0, 1, 0, 1], np.uint8)
    for cc in (None, [9, 9]):
        st, rows, *_ = one_node([5, 5, 5, 5], [1, 1, 1, 1], K=K, T=0, cutoff=9, class_cutoffs=cc, immovable={1})
        assert rows == [0, 2] and st["nodes_over_after"] == 1


def test_the_budget_sheds_a_row_order_prefix_of_the_surplus():
    load, S = [3] * 6, [6, 1, 5, 2, 4, 3]
    full = one_node(load, S, T=3, cutoff=9)[1]
    assert full == [1, 2, 3, 4, 5]
    for B in (0, 1, 3, 5, 9):
        st, rows, nodes, A2, _, used = one_node(load, S, T=3, cutoff=9, max_rows=B)
        assert rows == full[:B] and st["surplus_rows"] == 5 and st["shed_rows"] == min(B, 5) and used == [18 - 3 * min(B, 5)]
    st, rows, *_ = one_node(load, S, T=3, cutoff=9, max_rows=4, rows_cap=2)
    assert rows == full[:2]


def test_rows_outside_the_table_or_off_the_live_nodes_are_left_alone():
    A = u32(0, 1, 2, NONE, 0, 7)
    load, S, aff = u32(5, 5, 5, 5, 5, 5), np.zeros(6, np.uint32), np.zeros(6, np.uint32)
    st, rows, nodes, A2, aff2, used = spec.shed(A, load, aff, S, None, 5, 3, [1, 0, 1], [0, 0, NEVER], 1, lifecycle=True)
    assert rows == [0, 4] and nodes == [0, 0]                       # node 1 is dead, node 2 never over, row 5 >= n, node 7 >= m
    assert list(A2) == [NONE, 1, 2, NONE, NONE, 7] and list(aff2) == [INACTIVE, 0, 0, 0, INACTIVE, 0]
    assert st["nodes_over_before"] == 1 and st["nodes_over_after"] == 0
