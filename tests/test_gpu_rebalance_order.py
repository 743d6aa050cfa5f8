"""The load-ordered cut of the bounded rebalance on the MI355X (rio_gp_rebalance[_dev] with order = RIO_GP_REBALANCE_BY_LOAD)
against both references, bit for bit: the two-tick composition of the oracle over rows in (load, row) order
(tests/rebalance_order_ref.py) and the plain restatement of R0-R4 with R1' (tests/spec_rebalance_order.py).  Compared are the
column, `used`, every counter and the move list.

The tables are the smallest that can still break a kernel: sizes around the 1 024-lane step and the 4 096-row tile, one and
many tiles; m on both sides of the threshold search's LDS form (at most 256 over nodes) and of its global form; loads whose
threshold is decided by every digit of the search."""
import ctypes as C

import numpy as np
import pytest

import rebalance_order_ref as oref
import rebalance_ref as ref
import rio_gp
import spec_rebalance_order as spec

pytestmark = pytest.mark.gpu
NONE = rio_gp.NONE
INF = rio_gp.CAP_INF
BY_LOAD = 1


def load_table(g, cur, load, aff, cap, alive):
    """Rows holding a node >= m are what a shrinking rio_gp_set_nodes leaves behind: placed on a bigger table first."""
    m = len(cap)
    top = int(cur[cur != NONE].max()) + 1 if (cur != NONE).any() else 0
    g.set_nodes(np.full(max(top, m), INF, np.uint64), np.ones(max(top, m), np.uint8))
    g.set_objects(len(cur), load, aff)
    g.set_assign(cur)
    g.set_nodes(cap, alive)


def recount(col, load, m):
    used = np.zeros(m, np.uint64)
    on = (col != NONE) & (col < m)
    np.add.at(used, col[on], load[on].astype(np.uint64))
    return used


def want_of(cur, load, aff, cap, alive, T, budget, rounds, order=BY_LOAD):
    """Both references; they must agree before the GPU is compared with them."""
    w = oref.rebalance(cur, load, aff, cap, alive, T, budget, rounds, order=order)
    s = spec.rebalance(cur.tolist(), load.tolist(), aff.tolist(), cap.tolist(), alive.tolist(),
                       None if T is None else T.tolist(), budget, rounds, order=order)
    assert s[0] == w[0].tolist() and s[1] == w[1].tolist() and s[2] == w[2]
    assert [i for i, _, _ in s[3]] == w[3].tolist() and [b for _, _, b in s[3]] == w[5].tolist()
    return w


def check(g, cur, load, aff, cap, alive, T=None, max_moves=None, rounds=2, moves_cap=None, list_moves=True, order=BY_LOAD):
    st, rows, frm, to = g.rebalance(T, max_moves, rounds, list_moves=list_moves, moves_cap=moves_cap, order=order)
    budget = max_moves if moves_cap is None else (moves_cap if max_moves is None else min(max_moves, moves_cap))
    nxt, used, wst, wrows, wfrom, wto = want_of(cur, load, aff, cap, alive, T, budget, rounds, order)
    assert st == wst
    if list_moves:
        assert np.array_equal(rows, wrows) and np.array_equal(frm, wfrom) and np.array_equal(to, wto)
    assert np.array_equal(g.get_assign(), nxt)
    got_used = g.get_nodes()[2]
    assert np.array_equal(got_used, used) and np.array_equal(got_used, recount(nxt, load, len(cap)))
    return nxt


@pytest.mark.parametrize("m", [1, 64, 4097])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 4097, 70_001])
def test_matches_both_references(oracle, n, m):
    rng = np.random.default_rng(n * 11 + m)
    g = rio_gp.GpuPlacement(n, m + 3)
    cap = np.full(m, INF, np.uint64)
    for kind in ("tight", "zero", "inf"):
        cur, load, aff, alive, T = ref.random_table(rng, n, m, kind)
        load = oref.skewed_loads(rng, n, hi=int(rng.choice([300, 70_000, (1 << 32) - 1])))
        if kind == "tight":   # around the mean of THESE loads; some nodes unbounded, some with nothing free
            per = int(load.sum(dtype=np.uint64)) // m
            T = rng.integers(per // 2, per + per // 4 + 2, m).astype(np.uint64)
            T[rng.random(m) < 0.05] = np.uint64(INF)
            T[rng.random(m) < 0.05] = np.uint64(0)
        load_table(g, cur, load, aff, cap, alive)
        nxt = check(g, cur, load, aff, cap, alive, T, max_moves=0)                       # the surplus is still counted
        nxt = check(g, nxt, load, aff, cap, alive, T, max_moves=1, rounds=1)
        nxt = check(g, nxt, load, aff, cap, alive, T, max_moves=max(n // 50, 2), list_moves=False)
        nxt = check(g, nxt, load, aff, cap, alive, T, max_moves=1000, moves_cap=max(n // 100, 1))
        nxt = check(g, nxt, load, aff, cap, alive, T, rounds=3)                          # unlimited
        check(g, nxt, load, aff, cap, alive, None)                                       # the capacities (INF): nothing over
    g.close()


def _one_node_table(n, loads, m=3):
    """Every row a candidate of node 1 (of m); nodes 0 and 2 are empty and unbounded."""
    cur = np.full(n, 1, np.uint32)
    aff = np.zeros(n, np.uint32)
    return cur, np.asarray(loads, np.uint32), aff, np.ones(m, np.uint8)


def _thr_of_node(cur, load, aff, alive, T, j):
    pinned, cands = spec.candidates(cur.tolist(), load.tolist(), aff.tolist(), alive.tolist(), len(alive))
    free = int(T[j]) - pinned[j] if int(T[j]) > pinned[j] else 0
    return spec.threshold_form(cands[j], load.tolist(), free)


@pytest.mark.parametrize("edge", [256, 65_536, 1 << 24])
def test_threshold_exactly_at_a_digit_boundary(oracle, edge):
    rng = np.random.default_rng(edge)
    n = 2500
    loads = rng.choice([1, 2, edge - 1, edge, edge, edge + 1, 2 * edge, 0], n)
    cur, load, aff, alive = _one_node_table(n, loads)
    g = rio_gp.GpuPlacement(n, 3)
    cap = np.full(3, INF, np.uint64)
    for want_tau in (edge, edge - 1, edge + 1):   # at the boundary, the last value below it, the first above it
        below = int(load[load < want_tau].sum(dtype=np.uint64))
        T = np.array([INF, below + 5 * want_tau + want_tau // 2, INF], np.uint64)    # five ties fit, the sixth overflows
        tau, cutrow, _ = _thr_of_node(cur, load, aff, alive, T, 1)
        assert tau == want_tau and cutrow == np.flatnonzero(load == want_tau)[5]
        load_table(g, cur, load, aff, cap, alive)
        nxt = check(g, cur, load, aff, cap, alive, T, max_moves=40)
        check(g, nxt, load, aff, cap, alive, T)
    g.close()


def test_ties_span_many_tiles_and_the_cut_falls_in_a_later_one(oracle):
    n, m = 70_001, 2
    rng = np.random.default_rng(70)
    cur, load, aff, alive, _ = ref.random_table(rng, n, m, "tight", dead=False, max_load=3)
    cap = np.full(m, INF, np.uint64)
    T = np.zeros(m, np.uint64)
    for j in range(m):
        c = (cur == j) & (aff != ref.INACTIVE)
        pin = int(load[(cur == j) & (aff == ref.INACTIVE)].sum())
        T[j] = pin + int(load[c & (load < 3)].sum()) + 3 * int(0.6 * (c & (load == 3)).sum()) + 1
        tau, cutrow, _ = _thr_of_node(cur, load, aff, alive, T, j)
        first = int(np.flatnonzero(c & (load == 3))[0])
        assert tau == 3 and cutrow > first + 8 * 4096
    g = rio_gp.GpuPlacement(n, m + 3)
    load_table(g, cur, load, aff, cap, alive)
    nxt = check(g, cur, load, aff, cap, alive, T, max_moves=5000)
    check(g, nxt, load, aff, cap, alive, T)
    g.close()


def test_equal_loads_exact_fit_and_nothing_free(oracle):
    cap = np.full(3, INF, np.uint64)
    g = rio_gp.GpuPlacement(5000, 3)
    # every candidate of the node with the same load: the cut is a pure row cut among them
    cur, load, aff, alive = _one_node_table(5000, np.full(5000, 7))
    load_table(g, cur, load, aff, cap, alive)
    T = np.array([INF, 7 * 1234 + 3, 100], np.uint64)
    assert _thr_of_node(cur, load, aff, alive, T, 1)[:2] == (7, 1234)
    check(g, cur, load, aff, cap, alive, T)
    # a prefix that fits exactly: the rows of load <= 9 fill free to the last unit; the first of load 10 is the cut
    rng = np.random.default_rng(8)
    cur, load, aff, alive = _one_node_table(5000, rng.integers(0, 21, 5000))
    load_table(g, cur, load, aff, cap, alive)
    T = np.array([INF, int(load[load <= 9].sum()), INF], np.uint64)
    assert _thr_of_node(cur, load, aff, alive, T, 1)[:2] == (10, int(np.flatnonzero(load == 10)[0]))
    check(g, cur, load, aff, cap, alive, T)
    # free = 0 (the pinned rows alone exceed the target) with zero-load candidates: they stay, every other candidate is surplus
    aff[:50] = ref.INACTIVE
    load[:50] = 100
    load_table(g, cur, load, aff, cap, alive)
    T = np.array([INF, 10, INF], np.uint64)
    nxt = check(g, cur, load, aff, cap, alive, T)
    assert np.all(nxt[(load == 0) | (aff == ref.INACTIVE)] == 1) and np.all(nxt[(load > 0) & (aff != ref.INACTIVE)] != 1)
    g.close()


@pytest.mark.parametrize("m", [64, 4097])
def test_one_node_over_and_every_node_over(oracle, m):
    n = 20_000
    rng = np.random.default_rng(m)
    cur, load, aff, alive, _ = ref.random_table(rng, n, m, "inf")
    load = oref.skewed_loads(rng, n, hi=100_000)
    cap = np.full(m, INF, np.uint64)
    g = rio_gp.GpuPlacement(n, m + 3)
    load_table(g, cur, load, aff, cap, alive)
    used = recount(cur, load, m)
    j = int(np.flatnonzero(alive)[0])
    T = np.full(m, INF, np.uint64)
    T[j] = used[j] // np.uint64(2)
    nxt = check(g, cur, load, aff, cap, alive, T)                      # one slot
    T = (recount(nxt, load, m) * np.uint64(3) // np.uint64(4)).astype(np.uint64)
    T[-1] = INF                                                        # ... with somewhere to go
    check(g, nxt, load, aff, cap, alive, T)                            # every loaded live node over
    g.close()


@pytest.mark.parametrize("n", [65, 70_001])
def test_dev_form(oracle, n):
    import torch
    m = 64
    rng = np.random.default_rng(n + 2)
    cur, load, aff, alive, T = ref.random_table(rng, n, m, "tight")
    load = oref.skewed_loads(rng, n, hi=5000)
    per = int(load.sum(dtype=np.uint64)) // m
    T = rng.integers(per // 2, per + 2, m).astype(np.uint64)
    cap = np.full(m, INF, np.uint64)
    g = rio_gp.GpuPlacement(n, m + 3)
    load_table(g, cur, load, aff, cap, alive)
    k = max(n // 3, 1)
    nxt, used, wst, wrows, wfrom, wto = want_of(cur, load, aff, cap, alive, T, k, 2)
    d = torch.full((3, k + 8), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st, nm = g.rebalance_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), k, target=T, order=BY_LOAD)
    torch.cuda.synchronize()
    h = d.cpu().numpy().view(np.uint32)
    assert st == wst and nm == len(wrows)
    assert np.array_equal(h[0, :nm], wrows) and np.array_equal(h[1, :nm], wfrom) and np.array_equal(h[2, :nm], wto)
    assert np.all(h[:, nm:] == 0xFFFFFFFF)  # nothing written past the moves
    assert np.array_equal(g.get_assign(), nxt) and np.array_equal(g.get_nodes()[2], used)
    # counts only, then a budget of 0: the surplus is counted, nothing moves
    T2 = T // np.uint64(2)
    nxt2, _, wst2, *_ = want_of(nxt, load, aff, cap, alive, T2, None, 2)
    st2, nm2 = g.rebalance_dev(target=T2, order=BY_LOAD)
    assert st2 == wst2 and nm2 == wst2["moved_rows"] and np.array_equal(g.get_assign(), nxt2)
    _, _, wst3, *_ = want_of(nxt2, load, aff, cap, alive, T // np.uint64(4), 0, 2)
    st3, nm3 = g.rebalance_dev(target=T // np.uint64(4), max_moves=0, order=BY_LOAD)
    assert st3 == wst3 and nm3 == 0 and np.array_equal(g.get_assign(), nxt2)
    g.close()


def test_never_more_surplus_rows_than_row_order(oracle):
    """What the ordering is for: per node the surplus is the smallest set that brings it under its target, so the table's
    surplus_rows is <= the row-order cut's on the same table and targets (on skewed loads: far fewer)."""
    n, m = 70_001, 64
    rng = np.random.default_rng(1)
    cur = rng.integers(0, m, n).astype(np.uint32)
    aff = cur.copy()
    load = np.minimum(rng.zipf(1.3, n), 100_000).astype(np.uint32)
    alive = np.ones(m, np.uint8)
    cap = np.full(m, INF, np.uint64)
    T = (recount(cur, load, m) * np.uint64(7) // np.uint64(10)).astype(np.uint64)
    out = {}
    for order in (0, BY_LOAD):
        g = rio_gp.GpuPlacement(n, m)
        load_table(g, cur, load, aff, cap, alive)
        out[order], *_ = g.rebalance(T, max_moves=0, order=order)
        g.close()
        assert out[order] == oref.rebalance(cur, load, aff, cap, alive, T, 0, 2, order=order)[2]
    assert 0 < out[BY_LOAD]["surplus_rows"] <= out[0]["surplus_rows"]


def test_order_zero_in_either_struct_size_is_row_order(oracle):
    n, m = 4097, 64
    rng = np.random.default_rng(9)
    cur, load, aff, alive, T = ref.random_table(rng, n, m, "tight")
    cap = np.full(m, INF, np.uint64)
    nxt, used, wst, wrows, wfrom, wto = ref.rebalance(cur, load, aff, cap, alive, T, 300, 2)
    assert rio_gp.REBALANCE_CFG_V1_SIZE == 24 and C.sizeof(rio_gp.RebalanceCfg) == 32
    for size in (24, 32):
        g = rio_gp.GpuPlacement(n, m + 3)
        load_table(g, cur, load, aff, cap, alive)
        # (with the old size the two new fields are not read: garbage in them changes nothing)
        cfg = rio_gp.RebalanceCfg(size, 2, 300, T.ctypes.data, 0 if size == 32 else 7, 0 if size == 32 else 0xDEAD)
        buf = np.empty((3, 300), np.uint32)
        rc, st, nm = g.rebalance_raw(cfg, buf[0], buf[1], buf[2], 300)
        assert rc == rio_gp.OK and st == wst and nm == len(wrows)
        assert np.array_equal(buf[0, :nm], wrows) and np.array_equal(buf[1, :nm], wfrom) and np.array_equal(buf[2, :nm], wto)
        assert np.array_equal(g.get_assign(), nxt) and np.array_equal(g.get_nodes()[2], used)
        g.close()


def test_refusals_change_nothing(oracle):
    import sharded
    import torch
    n, m = 5000, 16
    rng = np.random.default_rng(3)
    cur, load, aff, alive, T = ref.random_table(rng, n, m, "zero", dead=False)
    g = rio_gp.GpuPlacement(n, m + 3)
    load_table(g, cur, load, aff, np.full(m, INF, np.uint64), alive)
    before, used = g.get_assign(), g.get_nodes()[2]
    tgt = np.zeros(m, np.uint64)
    size = C.sizeof(rio_gp.RebalanceCfg)
    for cfg in (rio_gp.RebalanceCfg(size, 0, INF, tgt.ctypes.data, 2, 0),          # an unknown order
                rio_gp.RebalanceCfg(size, 0, INF, tgt.ctypes.data, 1, 1),          # reserved != 0
                rio_gp.RebalanceCfg(size, 0, INF, tgt.ctypes.data, 0, 1),
                rio_gp.RebalanceCfg(28, 0, INF, tgt.ctypes.data, 1, 0),            # neither the old size nor the new one
                rio_gp.RebalanceCfg(40, 0, INF, tgt.ctypes.data, 1, 0)):
        rc, _, _ = g.rebalance_raw(cfg)
        assert rc == rio_gp.EINVAL
        assert np.array_equal(g.get_assign(), before) and np.array_equal(g.get_nodes()[2], used)
    # the row-sharded protocol cuts in row order only
    L = sharded._lib()
    x = torch.zeros(2 * (m + 3) + 64, dtype=torch.int64, device="cuda")
    by_load = rio_gp.RebalanceCfg(size, 2, INF, tgt.ctypes.data, 1, 0)
    assert L.rio_gp_shard_rebalance_begin(g.handle, C.byref(by_load), 0, 1, 1, INF, C.c_void_p(x.data_ptr()), None) == rio_gp.EINVAL
    assert b"load-ordered" in rio_gp.lib().rio_gp_last_error(g.handle)
    assert np.array_equal(g.get_assign(), before) and np.array_equal(g.get_nodes()[2], used)
    g.close()


def test_a_committed_tick_after_it_equals_the_oracles(oracle):
    import pyoracle
    n, m = 70_001, 64
    rng = np.random.default_rng(17)
    load = oref.skewed_loads(rng, n, hi=2000)
    aff = rng.integers(0, m, n).astype(np.uint32)
    alive = np.ones(m, np.uint8)
    alive[::13] = 0
    cap = np.full(m, int(load.sum(dtype=np.uint64)) // m * 2, np.uint64)
    g = rio_gp.GpuPlacement(n, m)
    g.set_nodes(cap, alive)
    g.set_objects(n, load, aff)
    g.tick()
    col, used, _ = pyoracle.tick(np.full(n, NONE, np.uint32), load, aff, cap, alive)
    assert np.array_equal(g.get_assign(), col)
    T = rio_gp.balanced_targets(cap, used, alive, 5)
    col = check(g, col, load, aff, cap, alive, T, max_moves=3000)
    g.tick()
    col, used, _ = pyoracle.tick(col, load, aff, cap, alive)
    assert np.array_equal(g.get_assign(), col) and np.array_equal(g.get_nodes()[2], used)
    g.close()
