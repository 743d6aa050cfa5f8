"""The two forms of the rebalance on ONE handle, alternating (rio_gp_rebalance and a world-1 rio_gp_shard_rebalance_* session over
the same GpuPlacement): both carve the same node scratch, reuse the same packed columns, tile counts and counters, and neither is
re-created in between, so whatever one form leaves behind is what the other starts on.  Every step is compared bit for bit with
the references (tests/rebalance_ref.py in row order, tests/rebalance_order_ref.py by load): the counters, the move list, the
column and `used`.

The steps: single by load, session in row order, single in row order, session by load, single by load with a budget of 0 (the
surplus is counted, nothing moves), single with nothing over.  The tables: 4 097 rows on 64 nodes (two tiles, the second one
ragged; one wave of nodes) and 1 025 rows on one node (nowhere to go: every selected row stays); loads 0 .. 3, so the by-load
ties of a node cross the tile boundary."""
import numpy as np
import pytest

import rebalance_order_ref as oref
import rebalance_ref as ref
import rio_gp
from test_gpu_shard_rebalance import make_engines

pytestmark = pytest.mark.gpu
INF = rio_gp.CAP_INF
ROW_ORDER, BY_LOAD = rio_gp.REBALANCE_ROW_ORDER, rio_gp.REBALANCE_BY_LOAD


def tight_targets(used, alive):
    """Three quarters of what every live node holds now: each loaded one is over; every eighth node (not node 0) is unbounded."""
    T = (used * np.uint64(3) // np.uint64(4)).astype(np.uint64)
    T[7::8] = np.uint64(INF)
    return T


@pytest.mark.parametrize("n,m", [(4097, 64), (1025, 1)])
def test_forms_alternate_on_one_handle(oracle, n, m):
    import sharded
    rng = np.random.default_rng(n + m)
    cur, load, aff, alive, _ = ref.random_table(rng, n, m, "tight", max_load=3)
    cap = np.full(m, INF, np.uint64)
    e = make_engines((cur, load, aff, cap, alive), [0, n])[0]
    g = e.g
    sol = sharded.ShardedSolver([e], sharded.LocalExchange(1))

    def single(T, max_moves, order):
        return g.rebalance(T, max_moves, 2, order=order)

    def session(T, max_moves, order):
        return sol.rebalance(target=T, max_moves=max_moves, rounds=2, order=order)

    col, used = cur, g.get_nodes()[2].copy()
    steps = [(single, BY_LOAD, n // 8), (session, ROW_ORDER, n // 8), (single, ROW_ORDER, None), (session, BY_LOAD, n // 8),
             (single, BY_LOAD, 0), (single, BY_LOAD, None)]
    for k, (form, order, max_moves) in enumerate(steps):
        last = k + 1 == len(steps)
        T = np.full(m, INF, np.uint64) if last else tight_targets(used, alive)
        want = (oref.rebalance(col, load, aff, cap, alive, T, max_moves, 2, order=order) if order == BY_LOAD
                else ref.rebalance(col, load, aff, cap, alive, T, max_moves, 2))
        nxt, used, wst, wrows, wfrom, wto = want
        assert (wst["nodes_over_before"] == 0) == last          # the tables do what the steps are there for
        if max_moves == 0:
            assert wst["surplus_rows"] > 0 and wst["nodes_over_after"] == wst["nodes_over_before"]
        st, rows, frm, to = form(T, max_moves, order)
        assert st == wst, (k, st, wst)
        assert np.array_equal(rows, wrows) and np.array_equal(frm, wfrom) and np.array_equal(to, wto), k
        assert np.array_equal(g.get_assign(), nxt), k
        assert np.array_equal(g.get_nodes()[2], used), k
        col = nxt
    g.close()
