"""Pressure shedding on the MI355X (rio_gp_shed_idle / _dev, rule 14): every call bit-exact against the restatement
(tests/spec_shed.py) — the column, `used` against a recount, every counter, the listing, the last-seen column unchanged, the
change feed's next read — over tables at the sizes where a pass changes its path (the compaction's tile of 1 024 rows, several
workgroups, one node, more nodes than the apply pass gathers in LDS, a slot count on each side of the selection's LDS form),
with few, equal, zero and 32-bit-wide stamps, a threshold at a digit boundary and loads up to 2^32 - 1 beside zeros; the class
form and the immovable fold, hidden rows, a renumbered node table, `used` valid and invalid on entry, ticks in flight, quiet
chained runs, an uncommitted solve, the tick after a shed, and every refusal."""
import ctypes as C

import numpy as np
import pytest

import shed_tables as tb
import spec_shed as spec
import synth

NONE, INACTIVE, NEVER = spec.NONE, spec.AFF_INACTIVE, spec.NEVER
LDS_SLOTS = 3072   # kShSelLdsSlots: up to here the selection's histogram lives in LDS


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


def load_table(g, A, load, aff, S, K, alive, m, classes=False):
    n = len(A)
    g.set_nodes(np.full(m, NEVER, np.uint64), alive, m=m)
    g.set_objects(n, load, aff)
    g.set_assign(A)
    if n:
        g.touch_merge(S)
        if classes:
            g.set_classes(0, K)


def check(g, alive, T, cutoff, max_rows=None, rows_cap=None, list_rows=True, cc=None, imm=None, life=False, dev=False,
          feed=True, stale=False):
    """One call against the restatement, everything compared; returns the spec's (stats, rows).  stale: the call finds the
    handle's `used` invalid (the column was bulk-loaded since it was last read)."""
    n, m = g.num_objects, g.num_nodes
    A = g.get_assign()
    if stale:
        g.set_assign(A)
    load, aff = g.get_objects()
    S = g.get_seen()
    K = g.get_classes() if (cc is not None or imm) else None
    if feed:
        g.changes()                                            # the consumer knows every row
    if list_rows:
        cap = int(rows_cap if rows_cap is not None else min(NEVER if max_rows is None else max_rows, n))
    else:
        cap = None
    want = spec.shed(A, load, aff, S, K, n, m, alive, T, cutoff, NEVER if max_rows is None else max_rows, cc, imm, cap, life)
    wst, wrows, wnodes, wA, waff, wused = want
    if dev:
        import torch
        d = torch.full((2, max(cap, 1)), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        st, k = g.shed_idle_dev(cutoff, d[0].data_ptr(), d[1].data_ptr(), cap, target=T, max_rows=max_rows, class_cutoffs=cc)
        out = d.cpu().numpy().view(np.uint32)
        rows, nodes = out[0, :k], out[1, :k]
        assert (out[:, k:] == 0x5A5A5A5A).all()                # nothing written past the listing
    else:
        st, rows, nodes = g.shed_idle(cutoff, target=T, max_rows=max_rows, class_cutoffs=cc, list_rows=list_rows,
                                      rows_cap=rows_cap)
    print("shed n=%d m=%d cutoff=%d B=%s cap=%s: %s" % (n, m, cutoff, max_rows, cap, st))
    assert st == wst, (st, wst)
    if list_rows:
        assert np.array_equal(rows, wrows) and np.array_equal(nodes, wnodes)
    else:
        assert len(rows) == 0
    assert np.array_equal(g.get_assign(), wA)
    l2, a2 = g.get_objects()
    assert np.array_equal(l2, load) and np.array_equal(a2, waff)
    assert np.array_equal(g.get_seen(), S)
    assert list(g.get_nodes()[2]) == wused == spec.used_of(wA, load, n, m)
    if feed:
        r, o, w, total = g.changes()
        assert total == len(wrows) and np.array_equal(r, wrows) and np.array_equal(o, wnodes) and (w == NONE).all()
    return wst, wrows


def call_sequence(g, alive, T, cutoff, **kw):
    """The calls every table gets: nothing, one row, a small listing in both forms, no listing, everything, and everything
    again."""
    n, m = g.num_objects, g.num_nodes
    st, rows = check(g, alive, T, cutoff, max_rows=0, **kw)
    assert st["shed_rows"] == 0 and st["surplus_rows"] > 0
    st, rows = check(g, alive, T, cutoff, max_rows=1, **kw)
    assert st["shed_rows"] == 1
    check(g, alive, T, cutoff, rows_cap=3, **kw)
    check(g, alive, T, cutoff, rows_cap=2, dev=True, **kw)   # the device form drops the ranks past the listing itself
    check(g, alive, T, cutoff, max_rows=5, list_rows=False, **kw)
    check(g, alive, T, cutoff, dev=True, **kw)
    used = g.get_nodes()[2]
    under = {j for j in range(m) if int(used[j]) <= int(T[j])}
    A = g.get_assign()
    st, rows = check(g, alive, T, cutoff, **kw)
    assert not under & {int(A[r]) for r in rows}
    return st


# (n, m, layout, heavy loads, nodes squeezed) — every n and m of the list, every layout, both forms of the selection
TABLES = [
    (1, 1, "spread", False, None),
    (1023, 1, "few", False, None),
    (1024, 64, "equal", False, None),
    (1025, 64, "zero", True, None),
    (4097, 64, "spread", True, None),
    (4097, 4097, "spread", False, None),
    (70_001, 1, "equal", False, None),
    (70_001, 64, "few", True, None),
    (70_001, 64, "spread", False, None),
    (70_001, 4097, "few", False, LDS_SLOTS),
    (70_001, 4097, "few", False, LDS_SLOTS + 1),
    (70_001, 4097, "zero", False, None),
]


def _table(n, m, layout, heavy, over):
    if n == 1:   # one row: a candidate of load 9 on a node with target 3
        return (np.zeros(1, np.uint32), np.array([9], np.uint32), np.zeros(1, np.uint32), np.array([77], np.uint32),
                np.zeros(1, np.uint8), np.ones(1, np.uint8), np.array([3], np.uint64), 0xFFFFFFFF)
    return tb.table(n * 31 + m, n, m, layout, heavy=heavy, over=over)


@pytest.mark.parametrize("n,m,layout,heavy,over", TABLES)
def test_the_tables_check_something(n, m, layout, heavy, over):
    """Not a GPU test: what the spec says about each table of the GPU test below, so that none of them passes vacuously."""
    A, load, aff, S, K, alive, T, cutoff = _table(n, m, layout, heavy, over)
    n_over, n_sur, mid = tb.facts(A, load, aff, S, K, n, m, alive, T, cutoff)
    assert n_over >= 1 and n_sur >= 1
    if layout in tb.TIE_LAYOUTS:
        assert mid >= 1
    if over is not None:
        assert n_over == over
    if m == 4097 and over is None and n > 4097:
        assert n_over > LDS_SLOTS


@pytest.mark.gpu
@pytest.mark.parametrize("valid", [False, True])
@pytest.mark.parametrize("n,m,layout,heavy,over", TABLES)
def test_dense_shedding_matches_the_spec(gp, n, m, layout, heavy, over, valid):
    A, load, aff, S, K, alive, T, cutoff = _table(n, m, layout, heavy, over)
    assert tb.facts(A, load, aff, S, K, n, m, alive, T, cutoff)[1] > 0
    g = gp.GpuPlacement(n + 100, m)
    try:
        load_table(g, A, load, aff, S, K, alive, m)
        call_sequence(g, alive, T, cutoff, feed=not valid, stale=not valid)
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("edge", [1 << 10, 1 << 21])
def test_threshold_exactly_at_a_digit_boundary(gp, edge):
    """One node, one slot: the digits are 11 / 11 / 10 bits of the key ~S.  sigma is made to fall on the key `edge`, the last
    key below it and the first above it."""
    rng = np.random.default_rng(edge)
    n = 2500
    keys = rng.choice(np.array([1, 2, edge - 1, edge, edge, edge + 1, 2 * edge, 0xFFFFFFF0], np.uint32), n)
    S = ~keys
    load = rng.integers(1, 9, n).astype(np.uint32)
    A, aff, K, alive = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.ones(1, np.uint8)
    for want in (edge, edge - 1, edge + 1):
        ties = np.flatnonzero(keys == want)
        T = np.array([int(load[keys < want].sum()) + int(load[ties[:5]].sum()) + int(load[ties[5]]) - 1], np.uint64)
        cands, pinned = spec.classify(A, load, aff, S, K, n, 1, alive, 0xFFFFFFFF)
        sigma, cutrow, _ = spec.thresholds(load, S, T, cands, pinned)[0]
        assert sigma == (~np.uint32(want)) and cutrow == ties[5]
        g = gp.GpuPlacement(n, 1)
        try:
            load_table(g, A, load, aff, S, K, alive, 1)
            check(g, alive, T, 0xFFFFFFFF, max_rows=40)
            check(g, alive, T, 0xFFFFFFFF)
        finally:
            g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("life", [False, True])
def test_the_class_form_and_the_movable_fold(gp, life):
    n, m = 20_011, 64
    A, load, aff, S, K, alive, T, cutoff = tb.table(5, n, m, "few", classes=4, squeeze=0.9)   # (most of the load is pinned)
    g = gp.GpuPlacement(n, m, flags=gp.CFG_ROW_LIFECYCLE if life else 0)
    try:
        load_table(g, A, load, aff, S, K, alive, m, classes=True)
        cc = [13, 0, 12, 11]                                   # classes 4 and 5 lie beyond n_classes: never shed
        assert tb.facts(A, load, aff, S, K, n, m, alive, T, cutoff, cc, None)[2] > 0
        check(g, alive, T, 0, max_rows=50, cc=cc, life=life)
        g.set_class_movable([1, 1, 0, 1])                      # class 2 immovable: cutoff 0 in both forms
        assert tb.facts(g.get_assign(), load, g.get_objects()[1], S, K, n, m, alive, T, cutoff, cc, {2})[1] > 0
        check(g, alive, T, 0, max_rows=70, cc=cc, imm={2}, life=life)
        check(g, alive, T, cutoff, max_rows=90, imm={2}, life=life)
        check(g, alive, T, 0, cc=cc, imm={2}, life=life, dev=True)
        check(g, alive, T, cutoff, imm={2}, life=life)
        g.set_class_movable(None)
        st, rows = check(g, alive, T, cutoff, life=life)
        assert st["shed_rows"] > 0 and (K[rows] == 2).any()   # what the table held back
    finally:
        g.close()


@pytest.mark.gpu
def test_hidden_rows_and_a_renumbered_node_table(gp):
    n, m = 9000, 12
    A, load, aff, S, K, alive, T, cutoff = tb.table(11, n, m, "few", dead=False)
    g = gp.GpuPlacement(n, m)
    try:
        load_table(g, A, load, aff, S, K, alive, m)
        g.set_num_objects(5000)                                # rows 5000 .. 8999 are hidden: they neither weigh nor go
        T2 = np.array([int(u * 0.5) for u in spec.used_of(A, load, 5000, m)], np.uint64)
        st, rows = check(g, alive, T2, cutoff, max_rows=300)
        assert st["shed_rows"] == 300
        g.set_num_objects(n)
        assert np.array_equal(g.get_assign()[5000:], A[5000:])
        keep = np.array([0, NONE, 1, 2, NONE, 3, 4, 5, 6, 7, 8, 9], np.uint32)   # nodes 1 and 4 removed, the rest renumbered
        g.remap_nodes(keep)
        m2 = g.num_nodes
        assert m2 == 10
        alive2 = np.ones(m2, np.uint8)
        T3 = np.array([int(u * 0.7) for u in g.get_nodes()[2]], np.uint64)
        st, rows = check(g, alive2, T3, cutoff)
        assert st["shed_rows"] > 0
        assert check(g, alive2, T3, cutoff)[0]["surplus_rows"] == 0
    finally:
        g.close()


def _settled(gp, n=1_000_000, lab=True):
    cfg = synth.config("c3", n_override=n)
    m = cfg["m"]
    g = gp.GpuPlacement(n, m, spill_rounds=2, lab=lab)
    g.set_nodes(cfg["cap"], cfg["alive"], m=m)
    g.set_objects(n, cfg["load"], cfg["aff"])
    g.set_assign(synth.warm_assign(n, m))
    for _ in range(10):                                        # settle: ticks until one left every object placed
        for _ in range(3):
            g.tick_async()
        if g.tick_wait()[-1]["slow_path"] == 0:
            break
    return g, cfg


@pytest.mark.gpu
def test_between_tick_async_and_tick_wait_and_the_tick_after(gp, oracle):
    g, cfg = _settled(gp, n=300_000, lab=False)
    n, m = cfg["n"], cfg["m"]
    try:
        rng = np.random.default_rng(3)
        g.touch_merge(rng.integers(1, 6, n).astype(np.uint32))
        cap, alive, used = g.get_nodes()
        T = np.array([int(u * 0.8) for u in used], np.uint64)
        for _ in range(4):
            g.tick_async()                                     # quiet ticks: they change nothing the call reads
        st, rows = check(g, alive, T, 6, max_rows=20_000, feed=False)
        assert st["shed_rows"] == 20_000
        assert len(g.tick_wait()) == 4
        A = g.get_assign()
        load, aff = g.get_objects()
        want, wused, wst = oracle.tick(A, load, aff, cap, alive, 2)
        got = g.tick()                                         # the shed rows are pending again: the tick places them
        assert got == wst and np.array_equal(g.get_assign(), want) and np.array_equal(g.get_nodes()[2], wused)
    finally:
        g.close()


@pytest.mark.gpu
def test_a_call_that_sheds_nothing_keeps_quiet_ticks_chained(gp):
    g, cfg = _settled(gp)
    n, m = cfg["n"], cfg["m"]
    try:
        A = g.get_assign()
        g.touch_all(5)
        for _ in range(3):                                     # quiet from here on
            g.tick_async()
        st0 = g.tick_wait()
        assert all(s["slow_path"] == 0 for s in st0)
        used = g.get_nodes()[2]
        T = np.array([int(u * 0.9) for u in used], np.uint64)
        c0 = g.chained_scans()
        for _ in range(10):
            g.tick_async()
        st, rows, nodes = g.shed_idle(9, target=T, max_rows=0)                    # over, but nothing may go
        assert st["surplus_rows"] > 0 and st["shed_rows"] == 0 and st["nodes_over_before"] == st["nodes_over_after"] > 0
        assert g.shed_idle(5, target=T)[0]["surplus_rows"] == 0                   # nothing is idle enough
        assert g.shed_idle(9, target=np.full(m, NEVER, np.uint64))[0]["nodes_over_before"] == 0   # no node is ever over
        c1 = g.chained_scans()
        for _ in range(10):
            g.tick_async()
        stq = g.tick_wait()
        c2 = g.chained_scans()
        assert c1 - c0 == 10 and c2 - c1 == 10, (c0, c1, c2)
        assert all(s == st0[-1] for s in stq) and np.array_equal(g.get_assign(), A)
        assert np.array_equal(g.get_nodes()[2], used)
        st, rows, nodes = g.shed_idle(9, target=T, max_rows=3)                    # three rows un-placed: the inputs changed
        assert st["shed_rows"] == 3
        for _ in range(10):
            g.tick_async()
        g.tick_wait()
        assert g.chained_scans() - c2 < 10
    finally:
        g.close()


@pytest.mark.gpu
def test_an_uncommitted_solve_is_dropped_only_when_something_was_shed(gp):
    g, cfg = _settled(gp, n=200_000, lab=False)
    try:
        g.touch_all(3)
        T = np.array([int(u * 0.9) for u in g.get_nodes()[2]], np.uint64)
        g.set_alive(1, 0)
        g.solve()
        solved = g.get_solved()
        assert g.shed_idle(4, target=T, max_rows=0)[0]["surplus_rows"] > 0      # count only
        assert g.shed_idle(3, target=T)[0]["shed_rows"] == 0                     # nothing idle enough
        assert np.array_equal(g.get_solved(), solved)
        g.commit()
        assert np.array_equal(g.get_assign(), solved)
        g.set_alive(2, 0)
        g.solve()
        assert g.shed_idle(4, target=T, max_rows=5)[0]["shed_rows"] == 5         # the solve no longer describes the table
        with pytest.raises(gp.ObjectPlacementError):
            g.commit()
    finally:
        g.close()


@pytest.mark.gpu
def test_every_refusal_changes_nothing(gp):
    import sharded
    n, m = 3000, 5
    A, load, aff, S, K, alive, T, cutoff = tb.table(2, n, m, "few")
    g = gp.GpuPlacement(n, m)
    try:
        load_table(g, A, load, aff, S, K, alive, m)
        used = g.get_nodes()[2]
        g.changes()
        err = lambda: g._L.rio_gp_last_error(g.handle).decode()
        buf = np.empty((2, 8), np.uint32)
        Tp = np.ascontiguousarray(T)
        cc = np.full(4, cutoff, np.uint32)

        def cfg(**kw):
            c = gp.ShedCfg(C.sizeof(gp.ShedCfg), cutoff, NEVER, Tp.ctypes.data, None, 0, 0)
            for k, v in kw.items():
                setattr(c, k, v)
            return c
        bad = [
            (None, None, None, 0),
            (cfg(struct_size=C.sizeof(gp.ShedCfg) - 8), None, None, 0),
            (cfg(struct_size=0), None, None, 0),
            (cfg(reserved=1), None, None, 0),
            (cfg(n_classes=3), None, None, 0),                                   # n_classes without the array
            (cfg(class_cutoffs=cc.ctypes.data, n_classes=0), None, None, 0),
            (cfg(class_cutoffs=cc.ctypes.data, n_classes=257), None, None, 0),
            (cfg(), buf[0], None, 8),                                            # rows without nodes
            (cfg(), None, buf[1], 8),
            (cfg(), None, None, 8),                                              # a cap without a listing
        ]
        for c, r, nd, cap in bad:
            rc, st, k = g.shed_idle_raw(c, r, nd, cap)
            assert rc == gp.EINVAL and k == 0 and st["surplus_rows"] == 0, (rc, st)
            if c is not None:
                assert "rio_gp_shed_idle" in err()
        # st and n_rows may both be NULL
        assert g._L.rio_gp_shed_idle(g.handle, C.byref(cfg(max_rows=0)), None, None, None, 0, None) == gp.OK
        h64 = (C.c_char * 64)()
        L = sharded._lib()
        assert L.rio_gp_shard_p2p_export(g.handle, 1, h64) == gp.OK             # a handle of the row-sharded solve
        assert g.shed_idle_raw(cfg())[0] == gp.EINVAL and "row-sharded" in err()
        assert L.rio_gp_shard_p2p_close(g.handle) == gp.OK
        assert np.array_equal(g.get_assign(), A) and np.array_equal(g.get_nodes()[2], used) and g.changes()[3] == 0
        assert np.array_equal(g.get_seen(), S)
        st, rows = check(g, alive, T, cutoff)
        assert st["shed_rows"] > 0
    finally:
        g.close()
