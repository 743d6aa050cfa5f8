"""The load-ordered cut of the bounded rebalance (DESIGN.md section 2 rule 6, R1'): the plain restatement
(tests/spec_rebalance_order.py) against the two-tick composition of the oracle over rows permuted into (load, row) order
(tests/rebalance_order_ref.py), the threshold form against the sorted-prefix form, and the consequences the rule states."""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as hs

import rebalance_order_ref as oref
import rebalance_ref
import spec_rebalance
import spec_rebalance_order as spec

NONE = 0xFFFFFFFF
INF = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module", autouse=True)
def _oracle_built(oracle):
    return oracle


def _table(seed, n, m, kind, dead=True, pinned=True, unplaced=True, big=True, loads="small"):
    rng = np.random.default_rng(seed)
    cur, load, aff, alive, T = rebalance_ref.random_table(rng, n, m, kind, dead, pinned, unplaced, big,
                                                          max_load=int(rng.choice([1, 3, 50])))
    if loads == "skewed":
        load = oref.skewed_loads(rng, n, hi=int(rng.choice([300, 70_000, (1 << 32) - 1])))
        if kind == "tight":
            per = int(load.sum(dtype=np.uint64)) // m
            T = rng.integers(per // 2, per + per // 4 + 2, m).astype(np.uint64)
    return cur, load, aff, alive, T


def _free_and_cands(cur, load, aff, alive, T):
    m = len(alive)
    pinned, cands = spec.candidates(cur.tolist(), load.tolist(), aff.tolist(), alive.tolist(), m)
    free = [int(T[j]) - pinned[j] if int(T[j]) > pinned[j] else 0 for j in range(m)]
    return free, cands


@settings(max_examples=120, deadline=None, suppress_health_check=[HealthCheck.too_slow])
@given(seed=hs.integers(0, 2**31), n=hs.integers(0, 300), m=hs.integers(1, 12), kind=hs.sampled_from(["zero", "tight", "inf", "caps"]),
       B=hs.sampled_from([0, 1, 7, None]), rounds=hs.integers(1, 3), dead=hs.booleans(), pinned=hs.booleans(),
       unplaced=hs.booleans(), big=hs.booleans(), loads=hs.sampled_from(["small", "skewed"]))
def test_restatement_equals_the_permuted_two_tick_composition(seed, n, m, kind, B, rounds, dead, pinned, unplaced, big, loads):
    cur, load, aff, alive, T = _table(seed, n, m, "tight" if kind == "caps" else kind, dead, pinned, unplaced, big, loads)
    cap = np.random.default_rng(seed + 1).integers(0, int(load.sum(dtype=np.uint64)) // m + 10, m).astype(np.uint64)
    if kind == "caps":
        T = None
    got = spec.rebalance(cur.tolist(), load.tolist(), aff.tolist(), cap.tolist(), alive.tolist(),
                         None if T is None else T.tolist(), B, rounds, order=spec.BY_LOAD)
    want = oref.rebalance(cur, load, aff, cap, alive, T, B, rounds, order=oref.BY_LOAD)
    nxt, used, st, moves = got
    assert nxt == want[0].tolist() and used == want[1].tolist() and st == want[2]
    assert [i for i, _, _ in moves] == want[3].tolist()
    assert [a for _, a, _ in moves] == want[4].tolist()
    assert [b for _, _, b in moves] == want[5].tolist()


@pytest.mark.parametrize("loads", ["small", "skewed"])
@pytest.mark.parametrize("kind", ["tight", "zero", "inf"])
def test_threshold_form_minimality_and_the_row_order_bound(kind, loads):
    for seed in range(25):
        n, m = 40 + 23 * seed, 1 + seed % 9
        cur, load, aff, alive, T = _table(seed * 3 + 1, n, m, kind, loads=loads)
        free, cands = _free_and_cands(cur, load, aff, alive, T)
        ld = load.tolist()
        for j in range(m):
            if not alive[j]:
                continue
            sur = spec.cut_surplus(cands[j], ld, free[j], spec.BY_LOAD)
            thr = spec.threshold_form(cands[j], ld, free[j])
            tot = sum(ld[i] for i in cands[j])
            if thr is None:
                assert sur == [] and tot <= free[j]
                continue
            tau, cutrow, tsur = thr
            # the threshold form is the sorted-prefix form
            assert tau >= 1 and sorted(sur) == tsur and ld[cutrow] == tau
            # zero-load candidates are never surplus
            assert all(ld[i] > 0 for i in sur)
            # what stays fits; the surplus is the smallest set whose removal leaves <= free: the k - 1 heaviest candidates weigh
            # less than the excess
            k, excess = len(sur), tot - free[j]
            assert tot - sum(ld[i] for i in sur) <= free[j]
            heaviest = sorted((ld[i] for i in cands[j]), reverse=True)
            assert sum(heaviest[:k - 1]) < excess <= sum(heaviest[:k])
            # never more rows than the row-order cut of the same node
            assert k <= len(spec.cut_surplus(cands[j], ld, free[j], spec.ROW_ORDER))


def test_order_zero_is_the_row_order_rule():
    for seed in range(30):
        n, m = 10 * seed, 1 + seed % 7
        cur, load, aff, alive, T = _table(seed, n, m, ["tight", "zero", "inf"][seed % 3])
        cap = np.full(m, INF, np.uint64)
        B = [None, 0, 1, 9][seed % 4]
        a = spec.rebalance(cur.tolist(), load.tolist(), aff.tolist(), cap.tolist(), alive.tolist(), T.tolist(), B, 2, order=0)
        b = spec_rebalance.rebalance(cur.tolist(), load.tolist(), aff.tolist(), cap.tolist(), alive.tolist(), T.tolist(), B, 2)
        assert a == b
        c = oref.rebalance(cur, load, aff, cap, alive, T, B, 2, order=0)
        assert a[0] == c[0].tolist() and a[2] == c[2]


def test_whole_table_surplus_is_at_most_row_orders_and_zero_loads_stay():
    for seed in range(12):
        cur, load, aff, alive, T = _table(100 + seed, 600, 8, "tight", loads="skewed")
        cap = np.full(8, INF, np.uint64)
        by = oref.rebalance(cur, load, aff, cap, alive, T, None, 2, order=oref.BY_LOAD)
        ro = oref.rebalance(cur, load, aff, cap, alive, T, None, 2, order=oref.ROW_ORDER)
        assert by[2]["surplus_rows"] <= ro[2]["surplus_rows"]
        assert by[2]["nodes_over_before"] == ro[2]["nodes_over_before"]
        assert np.all(load[by[3]] > 0)   # no moved row has load 0
