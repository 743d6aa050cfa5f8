"""The load-ordered cut (R1') of the row-sharded rebalance on the MI355X (rio_gp_shard_rebalance_begin_ordered, the threshold
passes, ShardedSolver.rebalance(order=1)): G handles on one device, bit for bit against the two-tick composition of the oracle over
rows in (load, row) order (tests/rebalance_order_ref.py) AND against the single-handle rio_gp_rebalance by load of the
concatenated table — the column, `used` on every rank, the counters, the moves.

The tables are those of tests/test_gpu_shard_rebalance.py with skewed loads: shard sizes on both sides of the 4 096-row step,
empty shards, m = 64 / 256 / 1 024 (digits of 1 to 5 bits under the record bound) and, for the histogram form without LDS, more
than 3 072 over nodes."""
import ctypes as C

import numpy as np
import pytest

import rebalance_order_ref as oref
import rebalance_ref
import rio_gp
from test_gpu_shard_rebalance import bounds_for, close, column, load_table, make_engines
from test_shard_rebalance_order_protocol import TIE_CASES, skewed_table, ties_table
from test_shard_rebalance_protocol import cut_on_rank0_table

pytestmark = pytest.mark.gpu
NONE = rio_gp.NONE
INF = rio_gp.CAP_INF
BY_LOAD = rio_gp.REBALANCE_BY_LOAD


def check(sol, engines, single, cur, load, aff, cap, alive, target=None, max_moves=None, rounds=2, list_moves=True, order=BY_LOAD):
    """One sharded rebalance against the reference and against the single handle (which is advanced too)."""
    st, rows, frm, to = sol.rebalance(target=target, max_moves=max_moves, rounds=rounds, list_moves=list_moves, order=order)
    nxt, used, wst, wrows, wfrom, wto = oref.rebalance(cur, load, aff, cap, alive, target, max_moves, rounds, order=order)
    assert st == wst
    if list_moves:
        assert np.array_equal(rows, wrows) and np.array_equal(frm, wfrom) and np.array_equal(to, wto)
    else:   # counters only: the same column and `used`, nothing listed
        assert len(rows) == 0 and len(frm) == 0 and len(to) == 0
        rows, frm, to = wrows, wfrom, wto
    assert np.array_equal(column(engines), nxt)
    for e in engines:
        assert np.array_equal(e.g.get_nodes()[2], used)
    if single is not None:
        sst, srows, sfrom, sto = single.rebalance(target, max_moves, rounds, order=order)
        assert st == sst
        assert np.array_equal(rows, srows) and np.array_equal(frm, sfrom) and np.array_equal(to, sto)
        assert np.array_equal(column(engines), single.get_assign() if single.num_objects else np.zeros(0, np.uint32))
        assert np.array_equal(single.get_nodes()[2], used)
    return nxt


def single_handle(case):
    cur, load, aff, cap, alive = case
    g = rio_gp.GpuPlacement(max(len(cur), 1), len(cap) + 3)
    load_table(g, cur, load, aff, cap, alive)
    return g


@pytest.mark.parametrize("G", [1, 2, 3, 8])
@pytest.mark.parametrize("hi", [3, 2000, (1 << 32) - 1])
@pytest.mark.parametrize("shape,n,m", [("balanced", 50_001, 256), ("ragged", 9_000, 64), ("empty", 4097, 1024)])
def test_sharded_by_load_equals_reference_and_single_handle(oracle, G, hi, shape, n, m):
    import sharded
    rng = np.random.default_rng(G * 100 + hi % 89 + len(shape))
    cur, load, aff, alive, T = skewed_table(rng, n, m, hi)
    cap = np.full(m, INF, np.uint64)
    b = bounds_for(n, G, shape, rng)
    engines = make_engines((cur, load, aff, cap, alive), b)
    single = single_handle((cur, load, aff, cap, alive))
    sol = sharded.ShardedSolver(engines, sharded.LocalExchange(G))
    T9 = np.where(T == np.uint64(INF), T, T // np.uint64(10) * np.uint64(9)).astype(np.uint64)
    col = cur
    for k, (target, max_moves, rounds) in enumerate(((T, 0, 1), (T, 1, 2), (T, max(n // 50, 2), 4), (T, None, 1), (T9, None, 8),
                                                     (np.full(m, INF, np.uint64), None, 2), (np.zeros(m, np.uint64), None, 2))):
        col = check(sol, engines, single, col, load, aff, cap, alive, target, max_moves, rounds, list_moves=k not in (2, 4))
    close(engines, single)


@pytest.mark.parametrize("case", sorted(TIE_CASES))
def test_ties_across_ranks_keep_the_first_in_global_row_order(oracle, case):
    import sharded
    ties, keep = TIE_CASES[case]
    (cur, load, aff, cap, alive, T), b, want = ties_table(ties, keep)
    engines = make_engines((cur, load, aff, cap, alive), b)
    single = single_handle((cur, load, aff, cap, alive))
    sol = sharded.ShardedSolver(engines, sharded.LocalExchange(3))
    st, rows, frm, to = sol.rebalance(target=T, max_moves=3, order=BY_LOAD)
    assert list(rows) == want[:3] and st["surplus_rows"] == len(want)
    for e, lo, hi in zip(engines, b[:-1], b[1:]):   # back to the table as it was
        e.g.set_assign(cur[lo:hi])
    nxt = check(sol, engines, single, cur, load, aff, cap, alive, T, None, 2)
    assert list(np.flatnonzero(nxt != cur)) == want
    close(engines, single)


def test_zero_load_candidates_behind_the_cut_are_never_surplus(oracle):
    """The table on which R1 makes the zero-load candidates of ranks 1 and 2 surplus (cut_on_rank0_table)."""
    import sharded
    cur, load, aff, cap, alive, b = cut_on_rank0_table()
    engines = make_engines((cur, load, aff, cap, alive), b)
    single = single_handle((cur, load, aff, cap, alive))
    sol = sharded.ShardedSolver(engines, sharded.LocalExchange(3))
    nxt = check(sol, engines, single, cur, load, aff, cap, alive, None, None, 2)
    assert list(np.flatnonzero(nxt != cur)) == [2]
    close(engines, single)


@pytest.mark.parametrize("kind", ["zero", "tenth"])
def test_more_slots_than_the_lds_histogram_holds(oracle, kind):
    """m = 4 096 nodes, nearly all over: above kShSelLdsSlots = 3 072 the histogram pass is the wave-aggregated form, and the
    record bound leaves it 1-bit digits."""
    import sharded
    rng = np.random.default_rng(71 if kind == "zero" else 72)
    n, m, G = 20_003, 4096, 3
    cur = rng.integers(0, m, n).astype(np.uint32)
    cur[:m] = np.arange(m, dtype=np.uint32)            # every node holds a candidate
    load = np.maximum(oref.skewed_loads(rng, n, 2000), 1).astype(np.uint32)
    aff = rng.integers(0, m, n).astype(np.uint32)
    alive = np.ones(m, np.uint8)
    cap = np.full(m, INF, np.uint64)
    used = np.bincount(cur, weights=load.astype(np.float64), minlength=m).astype(np.uint64)
    T = np.zeros(m, np.uint64) if kind == "zero" else used // np.uint64(10) * np.uint64(9)
    b = bounds_for(n, G, "ragged", rng)
    engines = make_engines((cur, load, aff, cap, alive), b)
    single = single_handle((cur, load, aff, cap, alive))
    sol = sharded.ShardedSolver(engines, sharded.LocalExchange(G))
    e0 = engines[0]
    nr = [e.rebalance_begin(r, G, T, INF, 2, True, x, order=BY_LOAD) for r, (e, x) in enumerate(zip(engines, sol.X))][0]
    xg = sol._gather(sol.X, out=sol.XG[0])
    over = [e.rebalance_cut(xg, y) for e, y in zip(engines, sol.Y)][0]
    # 1-bit digits, and of the 32 only those that reach into the largest load
    assert over > 3072 and e0.rebalance_threshold_plan() == (int(load.max()).bit_length(), 2 * over)
    col = check(sol, engines, single, cur, load, aff, cap, alive, T, 5000, 2)     # (begin starts over)
    check(sol, engines, single, col, load, aff, cap, alive, T, None, 1, list_moves=False)
    close(engines, single)


def test_refusals_change_nothing_and_order_zero_is_the_old_begin(oracle):
    import sharded
    rng = np.random.default_rng(43)
    n, m = 5000, 32
    cur, load, aff, alive, T = skewed_table(rng, n, m, 2000)
    cap = np.full(m, INF, np.uint64)
    e = make_engines((cur, load, aff, cap, alive), [0, n])[0]
    L, h = sharded._lib(), e.g.handle
    sol = sharded.ShardedSolver([e], sharded.LocalExchange(1))
    x, y = sol.X[0], sol.Y[0]
    vp = lambda t: C.c_void_p(t.data_ptr())
    before = (e.g.get_assign(), e.g.get_nodes()[2].copy())
    EINVAL = rio_gp.EINVAL
    row, _k0 = e.g._rebalance_cfg(T, None, 2)
    byl, _k1 = e.g._rebalance_cfg(T, None, 2, BY_LOAD)
    a, bb, p, w = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
    unchanged = lambda: np.array_equal(e.g.get_assign(), before[0])

    def host(t):   # (a record is written on the engine's stream)
        with e.ctx():
            return t.cpu().numpy()

    e._rb_R = 1    # world 1: the gathered record is the record
    # the old entry point keeps refusing the order, and says where to go
    assert L.rio_gp_shard_rebalance_begin(h, C.byref(byl), 0, 1, 1, INF, vp(x), None) == EINVAL
    msg = rio_gp.lib().rio_gp_last_error(h)
    assert b"load-ordered" in msg and b"rio_gp_shard_rebalance_begin_ordered" in msg
    # threshold_* without a session, and in a row-order session (begun through either entry point)
    assert L.rio_gp_shard_rebalance_threshold_plan(h, C.byref(p), C.byref(w)) == EINVAL
    for begin in (L.rio_gp_shard_rebalance_begin, L.rio_gp_shard_rebalance_begin_ordered):
        assert begin(h, C.byref(row), 0, 1, 1, INF, vp(x), None) == 0
        assert e.rebalance_cut(x, y) > 0
        assert L.rio_gp_shard_rebalance_threshold_plan(h, C.byref(p), C.byref(w)) == EINVAL
        assert L.rio_gp_shard_rebalance_threshold_hist(h, 0, vp(y)) == EINVAL
        assert L.rio_gp_shard_rebalance_threshold_pick(h, 0, vp(y), vp(y)) == EINVAL
        assert host(y)[0] > 0 and unchanged()               # ... and the row-order cut wrote its surplus
    # a load-ordered session: cut reports the nodes over and no surplus yet
    assert L.rio_gp_shard_rebalance_begin_ordered(h, C.byref(byl), 0, 1, 1, INF, vp(x), None) == 0
    assert L.rio_gp_shard_rebalance_threshold_plan(h, C.byref(p), C.byref(w)) == EINVAL       # before cut
    over = e.rebalance_cut(x, y)
    assert over > 0 and not host(y).any()
    passes, words = e.rebalance_threshold_plan()
    assert 2 <= passes <= 32 and words <= e.words1 and words % over == 0
    hb = e.new_buffer(words)
    assert L.rio_gp_shard_rebalance_select(h, vp(y), vp(y), C.byref(a), C.byref(bb)) == EINVAL    # before the last pick
    assert L.rio_gp_shard_rebalance_threshold_hist(h, 1, vp(hb)) == EINVAL                        # a pass ahead
    assert L.rio_gp_shard_rebalance_threshold_pick(h, 0, vp(hb), None) == EINVAL                  # a pick without its histogram
    for q in range(passes):
        e.rebalance_threshold_hist(q, hb)
        assert L.rio_gp_shard_rebalance_threshold_pick(h, q + 1, vp(hb), vp(y)) == EINVAL
        if q + 1 == passes:
            assert L.rio_gp_shard_rebalance_threshold_pick(h, q, vp(hb), None) == EINVAL          # the last pass writes S
            assert L.rio_gp_shard_rebalance_select(h, vp(y), vp(y), C.byref(a), C.byref(bb)) == EINVAL
        e.rebalance_threshold_pick(q, hb, y if q + 1 == passes else None)
    assert L.rio_gp_shard_rebalance_threshold_hist(h, passes, vp(hb)) == EINVAL                   # past the last pass
    assert host(y)[0] > 0 and unchanged()
    # a CRUD call between two passes ends the session: the next step is refused, the column is as it was
    e.rebalance_begin(0, 1, T, INF, 2, True, x, order=BY_LOAD)
    e.rebalance_cut(x, y)
    e.rebalance_threshold_plan()
    e.rebalance_threshold_hist(0, hb)
    e.rebalance_threshold_pick(0, hb)
    e.g.set_alive_all(alive)
    assert L.rio_gp_shard_rebalance_threshold_hist(h, 1, vp(hb)) == EINVAL
    assert L.rio_gp_shard_rebalance_threshold_pick(h, 1, vp(hb), vp(y)) == EINVAL
    assert unchanged() and np.array_equal(e.g.get_nodes()[2], before[1])
    # fresh runs give the references: by load, then row order right behind it (no threshold state leaks), then by load again
    col = check(sol, [e], None, cur, load, aff, cap, alive, T, 300, 2)
    col = check(sol, [e], None, col, load, aff, cap, alive, T, 200, 2, order=0)
    col = check(sol, [e], None, col, load, aff, cap, alive, T, 150, 2)
    # order = 0 through the new entry point is the row-order protocol to its end
    nr = C.c_uint32(0)
    assert L.rio_gp_shard_rebalance_begin_ordered(h, C.byref(row), 0, 1, 1, INF, vp(x), C.byref(nr)) == 0
    assert e.rebalance_cut(x, y) > 0
    assert e.rebalance_select(y, y)[1] > 0
    pend, rnd = e.rebalance_merge(y), 0
    while pend[0] and rnd < nr.value:
        e.rebalance_fill(rnd, y)
        pend, rnd = e.rebalance_merge(y), rnd + 1
    st, rows, frm, to = e.rebalance_finish(True)
    nxt, used, wst, wrows, wfrom, wto = rebalance_ref.rebalance(col, load, aff, cap, alive, T, None, 2)
    assert st == wst and np.array_equal(rows, wrows) and np.array_equal(frm, wfrom) and np.array_equal(to, wto)
    assert np.array_equal(e.g.get_assign(), nxt) and np.array_equal(e.g.get_nodes()[2], used)
    e.g.close()


def test_row_order_right_after_by_load_and_a_committed_tick(oracle):
    """No threshold state leaks into the next session, whichever entry point begins it; a committed sharded tick after a
    load-ordered rebalance equals the oracle's tick of the resulting table."""
    import sharded
    rng = np.random.default_rng(41)
    n, m, G = 60_000, 96, 3
    cur, load, aff, alive, T = skewed_table(rng, n, m, 2000)
    aff = np.where(aff == rebalance_ref.INACTIVE, rng.integers(0, m, n), aff).astype(np.uint32)   # a solve takes every row
    cur = np.where(cur >= m, NONE, cur).astype(np.uint32)
    total = int(load.sum())
    cap = np.full(m, 2 * total // m + 1, np.uint64)
    b = bounds_for(n, G, "ragged", rng)
    engines = make_engines((cur, load, aff, cap, alive), b)
    sol = sharded.ShardedSolver(engines, sharded.LocalExchange(G))
    sol.solve()                                  # not committed: the rebalance drops it
    col = check(sol, engines, None, cur, load, aff, cap, alive, T, 2000, 2)
    col = check(sol, engines, None, col, load, aff, cap, alive, T, 500, 2, order=0)
    for k in range(2):
        want, used, ost = oracle.tick(col, load, aff, cap, alive, 2)
        st = sol.tick()
        assert st == ost and np.array_equal(column(engines), want)
        for e in engines:
            assert np.array_equal(e.g.get_nodes()[2], used)
        col = check(sol, engines, None, want, load, aff, cap, alive, T, 300 * (k + 1), 1 + k)
    close(engines)
