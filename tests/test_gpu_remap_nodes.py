"""Node removal on the MI355X (rio_gp_remap_nodes): every result bit for bit against the numpy restatement (tests/spec_remap.py).
Sizes around k_remap's tiles (256 rows), its wave ranges and workgroups, node counts around the bitmap words and the full LDS map
(8 192); identity, reversal, drop one, drop a random half, drop all, applied one after the other to tables with unplaced rows,
stale node ids >= m and inactive affinities, with and without the row lifecycle.  Then the feed's checkpoint, rows hidden by a
smaller n, a liveness push still pending, the ticks behind a removal against the CPU oracle, ticks in flight, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import spec_remap as spec

NONE, INACTIVE, GONE = spec.NONE, spec.AFF_INACTIVE, spec.NODE_GONE
MAX_NODES = 8192


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


class Table:
    """A handle and the numpy columns the restatement keeps beside it (every row the handle holds, hidden ones included)."""

    def __init__(self, gp, n, m, seed, lifecycle, stale=True, inactive=True, extra=0):
        rng = self.rng = np.random.default_rng(seed)
        s = min(3, MAX_NODES - m) if stale else 0          # ids m .. m+s-1 go stale when the node table shrinks to m
        self.g = gp.GpuPlacement(n + extra, m + s, flags=gp.CFG_ROW_LIFECYCLE if lifecycle else 0)
        self.lifecycle, self.n, self.m = lifecycle, n, m
        self.load = rng.integers(0, 5, n).astype(np.uint32)
        pool = np.concatenate([np.arange(m + s, dtype=np.uint32), np.array([NONE] * (1 + m // 4), np.uint32)])
        self.assign = rng.choice(pool, size=n).astype(np.uint32)
        apool = np.concatenate([pool, np.array([INACTIVE] * (1 + m // 4), np.uint32)]) if inactive else pool
        self.aff = rng.choice(apool, size=n).astype(np.uint32)
        self.cap = rng.integers(1, 1 << 40, m).astype(np.uint64)
        self.alive = (rng.random(m) < 0.8).astype(np.uint8)
        self.B = None
        g = self.g
        g.set_nodes(None, None, m=m + s)
        g.set_objects(n, self.load, self.aff)
        if n:
            g.set_assign(self.assign)
        g.set_nodes(self.cap, self.alive)

    def close(self):
        self.g.close()

    def remap(self, map):
        want = spec.remap(self.assign, self.aff, self.g.num_objects, self.m, map, self.lifecycle, B=self.B, cap=self.cap,
                          alive=self.alive)
        ev = self.g.remap_nodes(map)
        self.assign, self.aff, self.B, self.cap, self.alive = want["assign"], want["aff"], want["B"], want["cap"], want["alive"]
        self.m = len(self.cap)
        assert ev == want["evicted"]
        return ev

    def check(self):
        g, n = self.g, self.g.num_objects
        assert g.num_nodes == self.m
        assert np.array_equal(g.get_assign(), self.assign[:n])
        load, aff = g.get_objects()
        assert np.array_equal(load, self.load[:n]) and np.array_equal(aff, self.aff[:n])
        cap, alive, used = g.get_nodes()
        assert np.array_equal(cap, self.cap) and np.array_equal(alive, self.alive)
        a = self.assign[:n]
        on = a < self.m
        want_used = np.bincount(a[on], weights=self.load[:n][on].astype(np.float64), minlength=self.m).astype(np.uint64)
        assert np.array_equal(used, want_used)
        if self.m:
            off, rows = g.rows_on_nodes()
            order = np.argsort(a[on], kind="stable")
            assert np.array_equal(rows, np.flatnonzero(on)[order].astype(np.uint32))
            assert np.array_equal(off, np.concatenate([[0], np.cumsum(np.bincount(a[on], minlength=self.m))]).astype(np.uint64))


def maps_for(rng, m):
    """identity | reversal | drop one | drop a random half | drop all, each over the node count the one before left"""
    yield "identity", lambda m: np.arange(m, dtype=np.uint32)
    yield "reversal", lambda m: np.arange(m, dtype=np.uint32)[::-1].copy()
    yield "drop one", lambda m: spec.stable_map(m, [int(rng.integers(0, m))] if m else [])
    yield "drop half", lambda m: spec.stable_map(m, np.flatnonzero(rng.random(m) < 0.5))
    yield "drop all", lambda m: np.full(m, NONE, np.uint32)


SIZES = [(1, 1), (1, 8192), (255, 2), (255, 33), (256, 64), (256, 65), (257, 1024), (257, 1), (4097, 2), (4097, 8192), (4097, 65),
         (70001, 33), (70001, 1024), (70001, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("lifecycle", [False, True])
@pytest.mark.parametrize("n,m", SIZES)
def test_remap_matches_the_spec(gp, n, m, lifecycle):
    t = Table(gp, n, m, seed=n * 31 + m, lifecycle=lifecycle)
    try:
        t.check()
        for name, mk in maps_for(t.rng, m):
            before = t.assign.copy()
            ev = t.remap(mk(t.m))
            if name in ("identity", "reversal"):
                assert ev == 0
            if name == "identity":
                assert np.array_equal(t.assign, before)
            t.check()
        assert t.m == 0
    finally:
        t.close()


class Fed:
    def __init__(self, t):
        self.t = t
        t.B = np.full(len(t.assign), NONE, np.uint32)
        self.mirror = {}

    def take(self, cap=None):
        import spec_changes
        t = self.t
        n = t.g.num_objects
        wr, wo, wn, wt, wB = spec_changes.dense(t.B, t.assign, n, cap, False)
        rows, old, new, total = t.g.changes(cap=cap)
        assert total == wt and np.array_equal(rows, wr) and np.array_equal(old, wo) and np.array_equal(new, wn)
        t.B = wB
        for r, o, w in zip(rows.tolist(), old.tolist(), new.tolist()):
            if o == GONE:
                assert r in self.mirror                    # the consumer was told a node that is gone
            if w == NONE:
                self.mirror.pop(r, None)
            else:
                self.mirror[r] = w
        return rows, old, new

    def renumber(self, m, map):
        """what a consumer does with the map it removed the nodes with: its copy follows (a removed node: GONE)"""
        self.mirror = {r: (GONE if map[v] == NONE else int(map[v])) if v < m else v for r, v in self.mirror.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("lifecycle", [False, True])
def test_the_feed_checkpoint_follows_the_renumbering(gp, lifecycle):
    n, m = 5000, 33
    t = Table(gp, n, m, seed=5, lifecycle=lifecycle)
    try:
        f = Fed(t)
        f.take(cap=n // 4)                                   # the consumer knows about half of the placed rows ...
        f.take(cap=n // 4)
        perm = t.rng.permutation(m).astype(np.uint32)
        t.remap(perm)                                        # ... a pure permutation: what it knows is renumbered with the table
        f.renumber(m, perm)
        drop = np.flatnonzero(t.rng.random(m) < 0.3)
        map = spec.stable_map(m, drop)
        t.remap(map)
        f.renumber(m, map)
        rows, old, new = f.take()                            # the rest, and the rows that lost their node as (GONE, NONE)
        lost = rows[old == GONE]
        assert len(lost) and (new[old == GONE] == NONE).all()
        a = t.assign[:n]
        assert f.mirror == {int(r): int(a[r]) for r in np.flatnonzero(a != NONE)}
        assert t.g.changes(cap=0)[3] == 0
        t.check()
    finally:
        t.close()


@pytest.mark.gpu
def test_a_pure_permutation_lists_nothing_and_an_unused_feed_starts_complete(gp):
    n, m = 3000, 65
    t = Table(gp, n, m, seed=6, lifecycle=False)
    u = Table(gp, n, m, seed=6, lifecycle=False)
    try:
        f = Fed(t)
        while len(f.take(cap=700)[0]):
            pass
        t.remap(np.arange(m, dtype=np.uint32)[::-1].copy())
        assert t.g.changes(cap=0)[3] == 0                    # every told row was renumbered with its node: no change
        # a handle that never used the feed: the removal allocates nothing, the first listing is every placed row
        u.remap(spec.stable_map(m, [0, 7, 64]))
        rows, old, new, total = u.g.changes()
        placed = np.flatnonzero(u.assign[:n] != NONE)
        assert total == len(placed) and np.array_equal(rows, placed) and (old == NONE).all()
        assert np.array_equal(new, u.assign[:n][placed])
    finally:
        t.close()
        u.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lifecycle", [False, True])
def test_hidden_rows_come_back_renumbered(gp, lifecycle):
    n, m = 4097, 64
    t = Table(gp, n, m, seed=7, lifecycle=lifecycle)
    try:
        f = Fed(t)
        f.take()
        t.g.set_num_objects(1000)                            # rows 1000 .. n-1 are hidden, their contents kept
        t.g.tick_async()                                     # a column swap in between: the hidden rows go over with it
        t.g.tick_wait()
        t.assign[:1000] = t.g.get_assign()
        t.aff[:1000] = t.g.get_objects()[1]
        map = spec.stable_map(m, np.flatnonzero(t.rng.random(m) < 0.4))
        ev = t.remap(map)
        f.renumber(m, map)
        hidden_lost = int((t.assign[1000:] == NONE).sum())
        t.check()
        t.g.tick()                                           # ... and another one behind the removal
        t.assign[:1000] = t.g.get_assign()
        t.aff[:1000] = t.g.get_objects()[1]
        t.g.set_num_objects(n)
        assert hidden_lost and ev <= 1000
        t.check()                                            # the hidden rows are back, cleaned and renumbered
        f.take()
        a = t.assign[:n]
        assert f.mirror == {int(r): int(a[r]) for r in np.flatnonzero(a != NONE)}
    finally:
        t.close()


@pytest.mark.gpu
def test_a_pending_liveness_push_lands_on_the_new_id(gp):
    n, m = 257, 33
    t = Table(gp, n, m, seed=8, lifecycle=False)
    try:
        t.g.set_alive_all(np.ones(m, np.uint8))
        t.alive[:] = 1
        t.g.get_nodes()
        t.g.set_alive(20, 0)                                 # still waiting in the pinned ring
        t.alive[20] = 0
        map = spec.stable_map(m, [3, 4])
        t.remap(map)
        assert t.alive.tolist() == [1] * 18 + [0] + [1] * 12
        t.check()
        t.g.tick()                                           # the device's bitmap says the same: node 18's objects are evicted,
        got = t.g.get_assign()                               # everybody else's stay
        assert ((t.assign == 18) & (t.aff != INACTIVE)).any()
        assert not ((got == 18) & (t.aff != INACTIVE)).any()
        stay = (t.assign < t.m) & (t.assign != 18)
        assert np.array_equal(got[stay], t.assign[stay])
    finally:
        t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(4097, 33), (70001, 1024)])
def test_the_ticks_behind_a_removal_equal_the_oracle(gp, oracle, n, m):
    t = Table(gp, n, m, seed=9, lifecycle=False, stale=False, inactive=False)
    try:
        t.g.tick()
        t.assign = t.g.get_assign()
        t.remap(spec.stable_map(m, np.flatnonzero(t.rng.random(m) < 0.25)))
        t.check()
        for _ in range(2):
            want, used, ost = oracle.tick(t.assign, t.load, t.aff, t.cap, t.alive)
            st = t.g.tick()
            assert np.array_equal(t.g.get_assign(), want) and st == ost
            assert np.array_equal(t.g.get_nodes()[2], used)
            t.assign = want
    finally:
        t.close()


@pytest.mark.gpu
def test_ticks_in_flight_are_joined(gp):
    n, m = 300_000, 64                                       # big enough for the chained quiet ticks
    tabs = [Table(gp, n, m, seed=10, lifecycle=False, stale=False, inactive=False) for _ in range(2)]
    try:
        map = spec.stable_map(m, [1, 40, 63])
        for k, t in enumerate(tabs):
            t.g.set_nodes(np.full(m, 0xFFFFFFFFFFFFFFFF, np.uint64), np.ones(m, np.uint8))
            t.g.tick()
            if k == 0:
                for _ in range(3):
                    t.g.tick_async()
                ev = t.g.remap_nodes(map)
                t.g.tick_async()
                assert len(t.g.tick_wait()) == 4
            else:
                for _ in range(3):
                    t.g.tick()
                assert t.g.remap_nodes(map) == ev
                t.g.tick()
        a, b = tabs[0].g, tabs[1].g
        assert np.array_equal(a.get_assign(), b.get_assign())
        assert all(np.array_equal(x, y) for x, y in zip(a.get_nodes(), b.get_nodes()))
        assert all(np.array_equal(x, y) for x, y in zip(a.get_objects(), b.get_objects()))
        assert ev > 0 and a.num_nodes == m - 3
    finally:
        for t in tabs:
            t.close()


@pytest.mark.gpu
def test_bad_maps_change_nothing(gp):
    n, m = 1000, 8
    t = Table(gp, n, m, seed=11, lifecycle=True)
    try:
        Fed(t).take()
        bad = [(m, None), (4, [0, 1, 2, 4, NONE, NONE, NONE, NONE]), (4, [0, 1, 2, 2, NONE, NONE, NONE, NONE]),
               (4, [0, 1, 2, NONE, NONE, NONE, NONE, NONE]), (4, [0, 1, 2, 3, 3, NONE, NONE, NONE]), (m + 1, list(range(m)))]
        for m_new, map in bad:
            assert not spec.check_map(m, m_new, map)
            rc, ev = t.g.remap_nodes_raw(m_new, None if map is None else np.array(map, np.uint32))
            assert rc == gp.EINVAL and ev == 0, (m_new, map)
            assert "rio_gp_remap_nodes" in t.g._L.rio_gp_last_error(t.g.handle).decode()
            t.check()
            assert t.g.changes(cap=0)[3] == 0
        map, ev = t.g.drop_nodes([2, 5])
        assert map.tolist() == spec.stable_map(m, [2, 5]).tolist() and t.g.num_nodes == m - 2
    finally:
        t.close()


@pytest.mark.gpu
def test_row_sharded_handle_refuses(gp):
    import sharded
    L = sharded._lib()
    g = gp.GpuPlacement(4096, 8)
    try:
        g.set_nodes(None, np.ones(8, np.uint8))
        g.set_objects(4096)
        h64 = (C.c_char * 64)()
        assert L.rio_gp_shard_p2p_export(g.handle, 1, h64) == gp.OK
        rc, _ = g.remap_nodes_raw(8, np.arange(8, dtype=np.uint32))
        assert rc == gp.EINVAL and "row-sharded" in g._L.rio_gp_last_error(g.handle).decode()
        assert L.rio_gp_shard_p2p_close(g.handle) == gp.OK
        assert g.remap_nodes(np.arange(8, dtype=np.uint32)) == 0 and g.num_nodes == 8
    finally:
        g.close()
