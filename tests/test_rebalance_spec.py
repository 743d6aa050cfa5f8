"""The bounded rebalance ("rebalance"): the plain restatement of R0-R4 (tests/spec_rebalance.py) against
the two-tick composition of the oracle (tests/rebalance_ref.py), and the properties the rule implies."""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as hs

import rebalance_ref
import spec_rebalance

NONE = 0xFFFFFFFF
INF = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module", autouse=True)
def _oracle_built(oracle):
    return oracle


def _both(cur, load, aff, cap, alive, T, B, rounds):
    got = spec_rebalance.rebalance(cur.tolist(), load.tolist(), aff.tolist(), cap.tolist(), alive.tolist(),
                                   None if T is None else T.tolist(), B, rounds)
    want = rebalance_ref.rebalance(cur, load, aff, cap, alive, T, B, rounds)
    return got, want


def _selected(cur, load, aff, alive, T, B):
    """R0-R2 alone: the selected rows."""
    m = len(alive)
    pinned, cands = [0] * m, [[] for _ in range(m)]
    for i, c in enumerate(cur.tolist()):
        if c != NONE and c < m and alive[c]:
            if aff[i] == rebalance_ref.INACTIVE:
                pinned[c] += int(load[i])
            else:
                cands[c].append(i)
    surplus = []
    for j in range(m):
        run, free = 0, max(T[j] - pinned[j], 0)
        for i in cands[j]:
            run += int(load[i])
            if run > free:
                surplus.append(i)
    surplus.sort()
    return surplus if B is None else surplus[:B]


def _check_properties(cur, load, aff, alive, T, B, got):
    nxt, used, st, moves = got
    m = len(alive)
    nxt = np.array(nxt, np.uint64)
    cur64 = cur.astype(np.uint64)
    live_row = np.array([c != NONE and c < m and alive[c] for c in cur.tolist()], bool)
    obj = aff != rebalance_ref.INACTIVE
    # no row loses its node; rows that take no part (unplaced, dead node, node >= m) and pinned rows are unchanged
    assert np.all(nxt[cur != NONE] != NONE)
    assert np.array_equal(nxt[~(live_row & obj)], cur64[~(live_row & obj)])
    # every move lands on a live node; a node that received rows ends at used <= T, up to its own selected rows that found no
    # place and came back to it (R4: the fill places within free, the rows that stay were not counted there)
    Tl = [INF] * m if T is None else T.tolist()
    received = set()
    for i, a, b in moves:
        assert b < m and alive[b] and a != b and cur[i] == a
        received.add(b)
    moved_rows = {i for i, _, _ in moves}
    back = [0] * m
    for i in _selected(cur, load, aff, alive, Tl, B):
        if i not in moved_rows and nxt[i] == cur[i]:
            back[cur[i]] += int(load[i])
    for j in received:
        assert used[j] <= Tl[j] + back[j]
    # load is conserved; moved <= selected <= B
    before = [0] * m
    for c, l in zip(cur.tolist(), load.tolist()):
        if c != NONE and c < m:
            before[c] += l
    assert sum(used) == sum(before)
    assert st["moved_rows"] <= st["selected_rows"] <= (st["surplus_rows"] if B is None else min(B, st["surplus_rows"]))
    assert [i for i, _, _ in moves] == sorted(i for i, _, _ in moves)


@settings(max_examples=150, deadline=None, suppress_health_check=[HealthCheck.too_slow])
@given(seed=hs.integers(0, 2**31), n=hs.integers(0, 300), m=hs.integers(1, 12),
       kind=hs.sampled_from(["zero", "tight", "inf", "caps"]), B=hs.sampled_from([0, 1, 7, None]),
       rounds=hs.integers(1, 3), dead=hs.booleans(), pinned=hs.booleans(), unplaced=hs.booleans(), big=hs.booleans())
def test_restatement_equals_the_two_tick_composition(seed, n, m, kind, B, rounds, dead, pinned, unplaced, big):
    rng = np.random.default_rng(seed)
    cur, load, aff, alive, T = rebalance_ref.random_table(rng, n, m, "tight" if kind == "caps" else kind, dead, pinned,
                                                          unplaced, big)
    cap = rng.integers(0, int(load.sum()) // m + 10, m).astype(np.uint64)
    if kind == "caps":
        T = None  # the capacities are the targets
    got, want = _both(cur, load, aff, cap, alive, T, B, rounds)
    nxt, used, st, moves = got
    assert nxt == want[0].tolist()
    assert used == want[1].tolist()
    assert st == want[2]
    assert [i for i, _, _ in moves] == want[3].tolist()
    assert [a for _, a, _ in moves] == want[4].tolist()
    assert [b for _, _, b in moves] == want[5].tolist()
    _check_properties(cur, load, aff, alive, cap if T is None else T, B, got)


def test_nothing_over_target_changes_nothing():
    rng = np.random.default_rng(5)
    cur, load, aff, alive, _ = rebalance_ref.random_table(rng, 500, 8)
    T = np.full(8, INF, np.uint64)
    nxt, used, st, moves = spec_rebalance.rebalance(cur.tolist(), load.tolist(), aff.tolist(), T.tolist(), alive.tolist())
    assert nxt == cur.tolist() and moves == [] and st["surplus_rows"] == 0 and st["nodes_over_before"] == 0


def test_scale_out_spreads_onto_empty_nodes():
    """The case of the issue at a small size: loaded nodes over 1.02 x the mean come down to it, the empty nodes take the
    excess, dead nodes and pinned rows stay."""
    rng = np.random.default_rng(11)
    n, m = 4000, 16
    cur = rng.integers(0, 11, n).astype(np.uint32)     # nodes 11..14 empty, 15 dead
    cur[:300] = 15
    load = rng.integers(1, 20, n).astype(np.uint32)
    aff = cur.copy()
    aff[300:350] = rebalance_ref.INACTIVE                # 50 pinned rows
    alive = np.ones(m, np.uint8)
    alive[15] = 0
    mean = int(load[cur != 15].sum()) // 15
    T = np.full(m, mean * 102 // 100, np.uint64)
    got, want = _both(cur, load, aff, np.full(m, INF, np.uint64), alive, T, None, 2)
    nxt, used, st, moves = got
    assert nxt == want[0].tolist()
    assert all(used[j] <= T[j] for j in range(15))
    assert all(used[j] > 0 for j in range(11, 15))
    assert nxt[:300] == cur[:300].tolist() and nxt[300:350] == cur[300:350].tolist()
    assert st["nodes_over_after"] == 0 < st["nodes_over_before"]


def test_balanced_targets():
    import rio_gp
    cap = np.array([100, 100, 200, 50], np.uint64)
    used = np.array([90, 10, 100, 0], np.uint64)
    alive = np.array([1, 1, 1, 0], np.uint8)
    t = rio_gp.balanced_targets(cap, used, alive, 0)
    # utilisation 200 / 400 = 0.5 of every live capacity; the dead node never over
    assert t.tolist() == [50, 50, 100, INF]
    assert rio_gp.balanced_targets(cap, used, alive, 100).tolist() == [55, 55, 110, INF]
    assert rio_gp.balanced_targets(cap, np.array([200, 200, 400, 0], np.uint64), alive, 100).tolist() == [100, 100, 200, INF]
    inf = np.full(4, INF, np.uint64)
    assert rio_gp.balanced_targets(inf, used, alive, 0).tolist() == [67, 67, 67, INF]
