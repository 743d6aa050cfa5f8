"""Immovable classes on the MI355X (rio_gp_set_class_movable, rio_gp_get_class_movable, rio_gp_rebalance[_dev] with the table;
DESIGN.md section 2 rule 13) against the row-by-row restatement (tests/spec_movable.py): the column, `used`, all nine counters
and the move list, in both orders of the cut.

The shapes are the smallest at which a class-aware pass (k_shedc_*) can go wrong: the quad tail of the class column (n = 1, 3,
4, 5), the 4 096-row step of a workgroup (4 095, 4 096, 4 097), a cut inside tile 1 or later (8 193, 3 * 4 096 + 1); one, two
and 33 nodes; class 255, a table shorter than 256 classes (the classes above it are movable), non-object rows and zero loads
mixed in, an immovable row exactly where the plain rule cuts, a node whose immovable load alone exceeds its target, every class
immovable; budgets 0, 1 and unlimited; the _dev form.  Then what the setter must leave alone, what the table must survive,
and the argument checks."""
import ctypes as C

import numpy as np
import pytest

import movable_tables as mt
import spec_movable as spec
import synth

pytestmark = pytest.mark.gpu
NONE = mt.NONE
INF = mt.INF
STAT_KEYS = ("surplus_rows", "surplus_load", "selected_rows", "selected_load", "moved_rows", "moved_load", "stayed_rows",
             "nodes_over_before", "nodes_over_after")


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


def load_table(g, t):
    """Rows holding a node >= m are what a shrinking rio_gp_set_nodes leaves behind: placed on a bigger table first."""
    cur, m = t["cur"], len(t["alive"])
    top = int(cur[cur != NONE].max()) + 1 if (cur != NONE).any() else 0
    g.set_nodes(np.full(max(top, m), INF, np.uint64), np.ones(max(top, m), np.uint8))
    g.set_objects(len(cur), t["load"], t["aff"])
    g.set_assign(cur)
    g.set_nodes(np.full(m, INF, np.uint64), t["alive"])
    g.set_classes(0, t["cls"])


def want_of(t, cur, budget, rounds, order, movable=None):
    m = len(t["alive"])
    return spec.rebalance(cur.tolist(), t["load"].tolist(), t["aff"].tolist(), t["cls"].tolist(),
                          (t["movable"] if movable is None else movable).tolist(), [INF] * m, t["alive"].tolist(), t["T"].tolist(),
                          budget, rounds, order)


def check(g, t, cur, budget, rounds, order, movable=None):
    """One rio_gp_rebalance against the spec; returns the next column."""
    st, rows, frm, to = g.rebalance(t["T"], budget, rounds, order=order)
    nxt, used, wst, moves = want_of(t, cur, budget, rounds, order, movable)
    assert set(st) >= set(STAT_KEYS) and {k: st[k] for k in STAT_KEYS} == wst
    assert rows.tolist() == [r for r, _, _ in moves] and frm.tolist() == [a for _, a, _ in moves]
    assert to.tolist() == [b for _, _, b in moves]
    assert g.get_assign().tolist() == nxt
    assert g.get_nodes()[2].tolist() == used
    assert np.array_equal(g.get_objects()[1], t["aff"])      # the affinity column is not written
    return np.array(nxt, np.uint32)


def test_the_directed_case(gp):
    """Rows 0-7 on node 0, 8-9 on node 1, all load 1, class 1 immovable, targets [4, 8]: the four class-0 rows of node 0 move.
    The plain rule moves rows 4-7 (and so does a build that ignores the table)."""
    t = dict(cur=np.array([0] * 8 + [1, 1], np.uint32), load=np.ones(10, np.uint32), aff=np.zeros(10, np.uint32),
             cls=np.array([1, 0, 1, 0, 1, 0, 1, 0, 0, 0], np.uint8), movable=np.array([1, 0], np.uint8),
             alive=np.ones(2, np.uint8), T=np.array([4, 8], np.uint64))
    for order in (0, 1):
        g = gp.GpuPlacement(10, 2)
        try:
            load_table(g, t)
            g.set_class_movable(t["movable"])
            st, rows, frm, to = g.rebalance(t["T"], order=order)
            assert rows.tolist() == [1, 3, 5, 7] and frm.tolist() == [0] * 4 and to.tolist() == [1] * 4
            assert st["surplus_rows"] == 4 and st["moved_rows"] == 4 and st["nodes_over_after"] == 0
            assert g.get_assign().tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 1, 1] and g.get_nodes()[2].tolist() == [4, 6]
        finally:
            g.close()


@pytest.mark.parametrize("m", [1, 2, 33])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4095, 4096, 4097, 8193, 3 * 4096 + 1])
def test_matches_the_spec_in_both_orders(gp, n, m):
    rng = np.random.default_rng(31 * n + m)
    g = gp.GpuPlacement(n, m + 3)
    try:
        for order in (0, 1):
            t = mt.random_table(rng, n, m, n_classes=200, max_load=int(rng.choice([1, 9, 70_000])))
            assert n < 100 or ((t["cls"] == 255).any() and (t["cls"] >= 200).any() and (t["load"] == 0).any()
                               and (t["aff"] == mt.INACTIVE).any() and mt.immovable_rows(t).any())
            load_table(g, t)
            g.set_class_movable(t["movable"])
            assert g.get_class_movable().tolist() == t["movable"].tolist() + [1] * 56
            cur = check(g, t, t["cur"], 0, 2, order)                  # the surplus is still counted, nothing moves
            cur = check(g, t, cur, 1, 1, order)
            cur = check(g, t, cur, None, 3, order)                    # unlimited
            # every class immovable: nothing is surplus, nothing moves
            g.set_class_movable(np.zeros(256, np.uint8))
            before = g.get_assign()
            st, rows, _, _ = g.rebalance(t["T"], order=order)
            assert st["surplus_rows"] == 0 and st["selected_rows"] == 0 and st["moved_rows"] == 0 and len(rows) == 0
            assert st["nodes_over_after"] == st["nodes_over_before"] and np.array_equal(g.get_assign(), before)
            assert np.array_equal(before, cur)
    finally:
        g.close()


@pytest.mark.parametrize("order", [0, 1])
def test_an_immovable_row_at_the_cut_and_a_node_full_of_immovable_load(gp, order):
    """One node, cut in tile 2: the row the plain rule cuts at is immovable, so its load is pinned and the cut falls on the last
    loaded candidate before it; then the immovable load alone passes the target: by load every candidate with load > 0 is
    surplus, in row order every candidate from the first with load > 0 on."""
    n, m = 3 * 4096 + 1, 3
    rng = np.random.default_rng(order)
    t = mt.random_table(rng, n, m, n_classes=256, frac_immovable=0.0, dead=False, plant=False)
    t["cur"][:] = 1
    t["aff"][:] = 0
    t["cls"][:] = 0
    t["load"][:] = 1
    t["load"][::7] = 0
    cutrow = 2 * 4096 + 6
    t["T"] = np.array([INF, int(t["load"][:cutrow].sum()), INF], np.uint64)   # the plain rule cuts node 1 at row `cutrow`
    assert t["load"][cutrow] == 1
    t["cls"][cutrow] = 255
    t["movable"][255] = 0
    g = gp.GpuPlacement(n, m)
    try:
        load_table(g, t)
        g.set_class_movable(t["movable"])
        nxt = check(g, t, t["cur"], None, 2, order)
        assert nxt[cutrow] == 1
        # free is one less: the candidates before the immovable row no longer fit, the last loaded one of them (row cutrow - 2;
        # row cutrow - 1 has load 0) is the cut in either order
        assert t["load"][cutrow - 1] == 0 and t["load"][cutrow - 2] == 1
        assert int(np.flatnonzero(nxt != 1)[0]) == cutrow - 2 and (nxt[cutrow - 1] != 1) == (order == 0)
        # a node whose immovable load alone exceeds its target
        t["load"][cutrow] = np.uint32(int(t["T"][1]) + 1)
        load_table(g, t)
        nxt = check(g, t, t["cur"], None, 2, order)
        cand = np.arange(n) != cutrow
        if order == 1:
            assert (nxt[cand & (t["load"] > 0)] != 1).all() and (nxt[cand & (t["load"] == 0)] == 1).all()
        else:
            first = int(np.flatnonzero(cand & (t["load"] > 0))[0])
            assert (nxt[:first] == 1).all() and (nxt[first:][cand[first:] & (t["load"][first:] > 0)] != 1).all()
    finally:
        g.close()


@pytest.mark.parametrize("n", [5, 8193])
def test_dev_form(gp, n):
    import torch
    m = 33
    rng = np.random.default_rng(n)
    t = mt.random_table(rng, n, m, n_classes=100)
    g = gp.GpuPlacement(n, m + 3)
    try:
        load_table(g, t)
        g.set_class_movable(t["movable"])
        k = max(n // 3, 1)
        for order in (0, 1):
            cur = g.get_assign()
            nxt, used, wst, moves = want_of(t, cur, k, 2, order)
            d = torch.full((3, k + 8), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            st, nm = g.rebalance_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), k, target=t["T"], max_moves=k, rounds=2,
                                     order=order)
            torch.cuda.synchronize()
            h = d.cpu().numpy().view(np.uint32)
            assert {key: st[key] for key in STAT_KEYS} == wst and nm == len(moves)
            assert h[0, :nm].tolist() == [r for r, _, _ in moves] and h[1, :nm].tolist() == [a for _, a, _ in moves]
            assert h[2, :nm].tolist() == [b for _, _, b in moves]
            assert np.all(h[:, nm:] == 0xFFFFFFFF)                    # nothing written past the moves
            assert g.get_assign().tolist() == nxt and g.get_nodes()[2].tolist() == used
    finally:
        g.close()


@pytest.mark.parametrize("order", [0, 1])
def test_an_all_movable_table_is_the_handle_that_never_called_the_setter(gp, order):
    n, m = 8193, 33
    rng = np.random.default_rng(77 + order)
    t = mt.random_table(rng, n, m, n_classes=256)
    out = []
    for how in ("never", "all movable", "set and reset"):
        g = gp.GpuPlacement(n, m + 3)
        try:
            load_table(g, t)
            if how == "all movable":
                g.set_class_movable(np.ones(256, np.uint8))
            elif how == "set and reset":
                g.set_class_movable(t["movable"])
                g.set_class_movable(None)
                assert g.get_class_movable().all()
            st, rows, frm, to = g.rebalance(t["T"], 500, 2, order=order)
            out.append((st, rows.tolist(), frm.tolist(), to.tolist(), g.get_assign().tolist(), g.get_nodes()[2].tolist()))
        finally:
            g.close()
    assert out[0] == out[1] == out[2] and out[0][0]["moved_rows"] > 0
    nxt, used, wst, moves = want_of(t, t["cur"], 500, 2, order, movable=np.ones(1, np.uint8))
    assert out[0][4] == nxt and out[0][5] == used and out[0][1] == [r for r, _, _ in moves]


def test_the_setter_leaves_used_an_uncommitted_solve_and_the_feed_alone(gp):
    n, m = 20_000, 16
    rng = np.random.default_rng(3)
    load = rng.integers(1, 5, n).astype(np.uint32)
    aff = rng.integers(0, m, n).astype(np.uint32)
    g = gp.GpuPlacement(n, m)
    try:
        g.set_nodes(np.full(m, int(load.sum()) * 13 // (10 * m), np.uint64), np.ones(m, np.uint8))
        g.set_objects(n, load, aff)
        g.tick()
        g.changes()                                                # the consumer knows every row
        used = g.get_nodes()[2]
        g.set_alive(1, 0)
        g.solve()
        solved = g.get_solved()
        g.set_class_movable(np.array([1, 0, 1, 0], np.uint8))
        assert g.get_class_movable().tolist() == [1, 0, 1, 0] + [1] * 252
        g.set_class_movable(None)
        g.set_class_movable(np.zeros(256, np.uint8))
        assert not g.get_class_movable().any()
        assert np.array_equal(g.get_nodes()[2], used)
        assert g.changes(cap=0)[3] == 0                            # the feed: nothing changed
        assert np.array_equal(g.get_solved(), solved)
        g.commit()                                                 # the uncommitted solve still commits
        assert np.array_equal(g.get_assign(), solved)
        assert not g.get_classes().any()                           # (the class column the call may have made: zero-filled)
    finally:
        g.close()


def test_the_setter_keeps_quiet_ticks_chained(gp):
    n = 1_000_000
    cfg = synth.config("c3", n_override=n)
    m = cfg["m"]
    g = gp.GpuPlacement(n, m, spill_rounds=2, lab=True)
    try:
        g.set_nodes(cfg["cap"], cfg["alive"], m=m)
        g.set_objects(n, cfg["load"], cfg["aff"])
        g.set_assign(synth.warm_assign(n, m))
        for _ in range(10):                                  # settle: ticks until one left every object placed
            for _ in range(3):
                g.tick_async()
            if g.tick_wait()[-1]["slow_path"] == 0:
                break
        A = g.get_assign()
        g.set_class_movable(np.ones(3, np.uint8))            # (first use: the class column is made here, outside the chain)
        for _ in range(3):
            g.tick_async()
        st0 = g.tick_wait()
        assert all(s["slow_path"] == 0 for s in st0)
        c0 = g.chained_scans()
        for _ in range(10):
            g.tick_async()
        g.set_class_movable(np.array([0, 1, 0], np.uint8))
        g.get_class_movable()
        g.set_class_movable(None)
        c1 = g.chained_scans()
        for _ in range(10):
            g.tick_async()
        st = g.tick_wait()
        c2 = g.chained_scans()
        assert c1 - c0 == 10 and c2 - c1 == 10, (c0, c1, c2)
        assert all(s == st0[-1] for s in st) and np.array_equal(g.get_assign(), A)
    finally:
        g.close()


def test_the_table_survives_remap_nodes_a_changed_row_count_and_the_rebalance(gp):
    n, m = 8193, 8
    rng = np.random.default_rng(11)
    t = mt.random_table(rng, n, m, n_classes=256, dead=False)
    t["cur"][t["cur"] >= m] = NONE
    g = gp.GpuPlacement(n, m)
    try:
        load_table(g, t)
        g.set_class_movable(t["movable"])
        want = t["movable"].tolist()
        g.rebalance(t["T"], 10)
        assert g.get_class_movable().tolist() == want
        g.set_num_objects(n // 3)
        g.set_num_objects(n)
        assert g.get_class_movable().tolist() == want
        g.remap_nodes(np.array([0, NONE, 1, 2, NONE, 3, 4, 5], np.uint32))
        assert g.get_class_movable().tolist() == want
        # and it is still honoured: the table after the removal, against the spec
        t2 = dict(t, alive=np.ones(6, np.uint8), T=np.delete(t["T"], [1, 4]))
        cur = g.get_assign()
        t2["load"], t2["aff"] = g.get_objects()[:2]
        check(g, t2, cur, None, 2, 1)
    finally:
        g.close()


def test_argument_checks_and_the_row_sharded_refusals(gp):
    import sharded
    import torch
    L = sharded._lib()
    n, m = 4097, 8
    rng = np.random.default_rng(2)
    t = mt.random_table(rng, n, m, n_classes=256, dead=False)
    t["cur"][t["cur"] >= m] = NONE
    g = gp.GpuPlacement(n, m)
    err = lambda: g._L.rio_gp_last_error(g.handle).decode()
    try:
        load_table(g, t)
        g.set_class_movable(np.array([1, 0], np.uint8))
        # RIO_GP_EINVAL with nothing changed
        assert g.set_class_movable_raw(np.ones(4, np.uint8), n_classes=257) == gp.EINVAL
        assert g.set_class_movable_raw(None, n_classes=3) == gp.EINVAL
        assert g.get_class_movable().tolist() == [1, 0] + [1] * 254
        # the sharded rebalance has no class column: refused while a class is immovable, with nothing changed
        before, used = g.get_assign(), g.get_nodes()[2]
        sol = sharded.ShardedSolver([sharded.HipShardEngine(g, 0, torch.cuda.Stream(torch.device("cuda", 0)))],
                                    sharded.LocalExchange(1))
        for order in (0, 1):    # rio_gp_shard_rebalance_begin, rio_gp_shard_rebalance_begin_ordered
            with pytest.raises(gp.ObjectPlacementError) as e:
                sol.rebalance(t["T"], 300, 2, order=order)
            assert e.value.rc == gp.EINVAL and "immovable" in e.value.text and "shard_rebalance_begin" in e.value.text
            assert ("_ordered" in e.value.text) == bool(order)
            assert np.array_equal(g.get_assign(), before) and np.array_equal(g.get_nodes()[2], used)
        # once the table is reset they behave as before: a one-rank session is the single handle's call
        g.set_class_movable(None)
        for order in (0, 1):
            twin = gp.GpuPlacement(n, m)
            try:
                load_table(twin, t)
                twin.set_assign(g.get_assign())
                wst, wrows, wfrom, wto = twin.rebalance(t["T"], 300, 2, order=order)
                st, rows, frm, to = sol.rebalance(t["T"], 300, 2, order=order)
                assert wst["moved_rows"] > 0 and {k: st[k] for k in STAT_KEYS} == {k: wst[k] for k in STAT_KEYS}
                assert np.array_equal(rows, wrows) and np.array_equal(frm, wfrom) and np.array_equal(to, wto)
                assert np.array_equal(g.get_assign(), twin.get_assign())
                assert np.array_equal(g.get_nodes()[2], twin.get_nodes()[2])
            finally:
                twin.close()
    finally:
        g.close()
    # a handle of the row-sharded solve refuses the setter
    g = gp.GpuPlacement(4096, 8)
    try:
        g.set_nodes(None, np.ones(8, np.uint8))
        g.set_objects(4096)
        h64 = (C.c_char * 64)()
        assert L.rio_gp_shard_p2p_export(g.handle, 1, h64) == gp.OK
        assert g.set_class_movable_raw(np.zeros(2, np.uint8)) == gp.EINVAL
        assert "row-sharded" in g._L.rio_gp_last_error(g.handle).decode()
        assert L.rio_gp_shard_p2p_close(g.handle) == gp.OK
        assert g.get_class_movable().all()
        assert g.set_class_movable_raw(np.zeros(2, np.uint8)) == gp.OK
    finally:
        g.close()
