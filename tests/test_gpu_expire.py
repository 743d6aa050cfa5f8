"""Idle expiry on the MI355X (rio_gp_touch_*, rio_gp_get_seen, rio_gp_expire / _dev): every call against the plain restatement
(tests/spec_expire.py) and against a twin handle that receives rio_gp_remove_batch of the restatement's rows instead, over
tables driven through every kind of change — touches of every form, CRUD batches, clean_servers, liveness flips and ticks,
place_pending, a rebalance, a shrinking and growing row count — at sizes around the passes' tiles (1 024 rows) and workgroups,
with and without the row lifecycle, with few and with more nodes than the apply pass gathers in LDS (4 096); the call forms;
ticks in flight, an uncommitted solve, quiet ticks that stay chained; the change feed afterwards; the row-sharded refusal;
config 3 at 10 M rows."""
import ctypes as C

import numpy as np
import pytest

import spec_expire as spec
import synth

NONE = 0xFFFFFFFF
TILE = 1024   # kChgTile
CAPS = [None, "count", 1, 7, 1 << 40]


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


class Pair:
    """The handle under test, its twin (the same calls, but rio_gp_remove_batch of the restatement's rows where the first gets
    rio_gp_expire) and the numpy last-seen column the restatement keeps."""

    def __init__(self, gp, max_objects, m, life):
        fl = gp.CFG_ROW_LIFECYCLE if life else 0
        self.g = gp.GpuPlacement(max_objects, m, flags=fl)
        self.t = gp.GpuPlacement(max_objects, m, flags=fl)
        self.S = np.zeros(max_objects, np.uint32)

    def close(self):
        self.g.close()
        self.t.close()

    def both(self, name, *a, **kw):
        r = getattr(self.g, name)(*a, **kw)
        w = getattr(self.t, name)(*a, **kw)
        return r, w

    def same_state(self):
        g, t = self.g, self.t
        assert np.array_equal(g.get_assign(), t.get_assign())
        assert np.array_equal(g.get_objects()[1], t.get_objects()[1])          # affinity: the row lifecycle
        assert np.array_equal(g.get_nodes()[2], t.get_nodes()[2])              # used
        assert g.count_placed() == t.count_placed()

    def check(self, cutoff, cap=None):
        """One rio_gp_expire against the restatement and the twin; returns (listed, n_idle)."""
        g, t = self.g, self.t
        n = g.num_objects
        A = g.get_assign()
        load = g.get_objects()[0]
        count = cap == "count"
        wr, wn, wi, wf, wA = spec.expire(A, self.S, load, n, cutoff, 0 if count else cap)
        rows, nodes, n_idle, freed = g.expire(cutoff, count_only=True) if count else g.expire(cutoff, cap=cap)
        assert n_idle == wi and freed == wf
        assert np.array_equal(rows, wr) and np.array_equal(nodes, wn)
        assert np.array_equal(g.get_assign(), wA)
        assert np.array_equal(g.get_seen(), self.S[:n])
        if len(wr):
            t.remove_batch(wr)
        self.same_state()
        return len(wr), wi


def _table(n, m, seed, headroom=1.3):
    rng = np.random.default_rng(seed)
    load = rng.integers(1, 5, max(n, 1)).astype(np.uint32)[:n]
    aff = rng.integers(0, m, max(n, 1)).astype(np.uint32)[:n]
    cap = np.full(m, int(max(1, load.sum()) * headroom / m) + 8, np.uint64)
    return rng, load, aff, cap


def _dev_u32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).cuda()


TABLES = [(n, 16) for n in (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, (1 << 20) + 17)] + [(70_000, 1), (70_000, 4097)]


@pytest.mark.gpu
@pytest.mark.parametrize("life", [False, True])
@pytest.mark.parametrize("n,m", TABLES)
def test_dense_expiry_matches_the_spec_and_the_twin(gp, n, m, life):
    import torch
    extra = 3000
    rng, load, aff, cap = _table(n, m, n + m)
    p = Pair(gp, n + extra, m, life)
    g = p.g
    try:
        p.both("set_nodes", cap, np.ones(m, np.uint8))
        p.both("set_objects", n, load, aff)
        assert p.check(5) == (0, 0)                          # nothing placed yet: nothing is idle
        a, b = p.both("tick")
        assert a == b
        epoch = 1
        for it in range(15):
            k = it % 8
            epoch += 1
            # -- a touch of some form (S is the restatement's) --
            if n and k % 4 == 0:
                idx = rng.integers(0, n, 1 + n // 3).astype(np.uint32)
                idx[-1] = idx[0]                             # a duplicate
                g.touch(idx, epoch)
                p.S = spec.touch(p.S, idx, epoch)
                g.touch(idx[: 1 + len(idx) // 2], epoch - 1)   # an older epoch lowers nothing
            elif n and k % 4 == 1:
                idx = rng.integers(0, n, 1 + n // 5).astype(np.uint32)
                d = _dev_u32(idx)
                torch.cuda.synchronize()
                g.touch_dev(d.data_ptr(), len(idx), epoch)
                p.S = spec.touch(p.S, idx, epoch)
            elif k % 4 == 2:
                rows = int(rng.integers(0, n + 1))
                st = rng.integers(0, epoch + 1, max(rows, 1)).astype(np.uint32)[:rows]
                if it % 2:
                    d = _dev_u32(st) if rows else None
                    torch.cuda.synchronize()
                    g.touch_merge_dev(d.data_ptr() if rows else None, rows)
                else:
                    g.touch_merge(st)
                p.S = spec.touch_merge(p.S, st)
            elif it == 11:
                g.touch_all(epoch - 2)
                p.S = spec.touch_all(p.S, n, epoch - 2)
            # -- a change of the table, on both handles --
            if n and k == 0:
                idx = rng.integers(0, n, 1 + n // 10).astype(np.uint32)
                node = rng.integers(0, m + 1, len(idx)).astype(np.uint32)
                node[node == m] = NONE
                p.both("update_batch", idx, node)
            elif n and k == 1:
                p.both("remove_batch", rng.integers(0, n, 1 + n // 20).astype(np.uint32))
            elif k == 2:
                a, b = p.both("clean_servers", [int(rng.integers(0, m))])
                assert a == b
            elif k == 3:
                alive = (rng.random(m) < 0.8).astype(np.uint8)
                alive[0] = 1
                p.both("set_alive_all", alive)
                a, b = p.both("tick")
                assert a == b
            elif n and k == 4:
                idx = rng.integers(0, n, 1 + n // 8).astype(np.uint32)
                req = rng.integers(0, m, len(idx)).astype(np.uint32)
                a, b = p.both("place_pending", idx, req)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            elif k == 5:
                p.both("set_alive_all", np.ones(m, np.uint8))
                a, b = p.both("tick")
                assert a == b
                a, b = p.both("rebalance", target=(cap * 2 // 3).astype(np.uint64))
                assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
            elif k == 6:
                p.both("set_num_objects", n // 2)            # rows >= n/2 are never idle and keep their S ...
                p.check(epoch, cap=[None, 3][(it // 8) % 2])
                p.both("set_num_objects", n + extra)         # ... and come back, with rows never used behind them
                p.check(epoch - 1, cap="count")
                p.both("set_num_objects", n)
            elif k == 7:
                a, b = p.both("tick")
                assert a == b
            cutoff = [epoch, 0, epoch - 1, 0xFFFFFFFF, epoch + 1, 2][it % 6]
            capv = CAPS[it % 5]
            if cutoff == 0xFFFFFFFF and capv is None:
                capv = 7                                     # (everything placed, every time, would leave little to check)
            p.check(cutoff, capv)
        a, b = p.both("tick")                                # the next tick says the same on both
        assert a == b
        p.same_state()
        pages = 0
        while p.check(0xFFFFFFFF, cap=37)[0]:                # page out everything that is placed
            pages += 1
            if pages == 6 and n > 4096:                      # (a long table: the rest in one call)
                p.check(0xFFFFFFFF)
        assert p.check(0xFFFFFFFF) == (0, 0) and g.count_placed() == 0
    finally:
        p.close()


def _settled(gp, n=200_000, m=64, seed=5, life=False, lab=False):
    rng, load, aff, cap = _table(n, m, seed)
    g = gp.GpuPlacement(n, m, flags=gp.CFG_ROW_LIFECYCLE if life else 0, lab=lab)
    g.set_nodes(cap, np.ones(m, np.uint8))
    g.set_objects(n, load, aff)
    g.tick()
    return g, rng, load, m


@pytest.mark.gpu
def test_call_forms_device_arrays_argument_checks_first_use(gp):
    import torch
    g, rng, load, m = _settled(gp)
    n = g.num_objects
    try:
        A = g.get_assign()
        placed = np.flatnonzero(A != NONE).astype(np.uint32)
        assert len(placed) > n // 2
        # first use on a fresh handle: nobody has been seen, every placed row is idle; cutoff 0 still finds nothing
        assert g.expire(1, count_only=True)[2] == len(placed) and g.expire(0, count_only=True)[2] == 0
        assert not g.get_seen().any()
        # argument checks: RIO_GP_EINVAL and nothing changed
        buf = np.empty((2, 8), np.uint32)
        for kw in (dict(out_rows=buf[0], cap=8), dict(out_node=buf[1], cap=8), dict(cap=8),
                   dict(out_rows=buf[0], out_node=buf[1], cap=8, want_n_idle=False)):
            assert g.expire_raw(1, **kw)[0] == gp.EINVAL
        assert g.touch_raw([0, n], 3) == gp.EINVAL            # one entry out of range: nothing is touched
        bad = _dev_u32([1, n + 5, 2])
        torch.cuda.synchronize()
        with pytest.raises(gp.ObjectPlacementError) as e:
            g.touch_dev(bad.data_ptr(), 3, 4)                 # the _dev form skips the invalid entry and says so
        assert e.value.rc == gp.EINVAL
        S = np.zeros(n, np.uint32)
        S[[1, 2]] = 4
        assert np.array_equal(g.get_seen(), S) and np.array_equal(g.get_assign(), A)
        with pytest.raises(gp.ObjectPlacementError):
            g.touch_merge(np.ones(n + 1, np.uint32))          # more stamps than rows
        assert np.array_equal(g.get_seen(), S)
        # the _dev form against the restatement: a page, then the rest; nothing is written past the listing
        wr, wn, wi, wf, wA = spec.expire(A, S, load, n, 4, 1000)
        d = [torch.full((1000 + 5,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        assert g.expire_dev(4, d[0].data_ptr(), d[1].data_ptr(), cap=1000) == (wi, wf)
        got = [x.cpu().numpy().view(np.uint32) for x in d]
        assert np.array_equal(got[0][:1000], wr) and np.array_equal(got[1][:1000], wn) and (got[0][1000:] == NONE).all()
        assert np.array_equal(g.get_assign(), wA)
        assert g.expire_dev(4) == (wi - 1000, 0)              # the _dev form's count only
        cap = wi + 3
        d = [torch.full((cap,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        wr2, wn2, wi2, wf2, wA2 = spec.expire(wA, S, load, n, 4, cap)
        assert g.expire_dev(4, d[0].data_ptr(), d[1].data_ptr(), cap=cap) == (wi2, wf2) and wi2 == wi - 1000
        got = [x.cpu().numpy().view(np.uint32) for x in d]
        assert np.array_equal(got[0][:wi2], wr2) and np.array_equal(got[1][:wi2], wn2) and (got[0][wi2:] == NONE).all()
        assert np.array_equal(g.get_assign(), wA2) and g.count_placed() == int((A[[1, 2]] != NONE).sum())
        assert np.array_equal(g.get_seen(), S)                # expiry leaves S alone
    finally:
        g.close()


@pytest.mark.gpu
def test_expiry_orders_itself_behind_ticks_in_flight(gp):
    n = 1 << 20
    cfg = synth.config("c3", n_override=n)
    m = cfg["m"]
    g, t = gp.GpuPlacement(n, m), gp.GpuPlacement(n, m)
    try:
        for h in (g, t):
            h.set_nodes(cfg["cap"], cfg["alive"])
            h.set_objects(n, cfg["load"], cfg["aff"])
            h.tick()
        idx = np.arange(0, n, 3, dtype=np.uint32)
        g.touch(idx, 9)
        S = spec.touch(np.zeros(n, np.uint32), idx, 9)
        for k in range(4):
            mask = synth.churn_mask(m, k + 1)
            g.set_alive_all(mask)
            g.tick_async()
            t.set_alive_all(mask)
            t.tick()
        rows, nodes, n_idle, freed = g.expire(9, cap=50_000)  # no tick_wait in between
        wr, wn, wi, wf, wA = spec.expire(t.get_assign(), S, cfg["load"], n, 9, 50_000)
        assert (n_idle, freed) == (wi, wf) and np.array_equal(rows, wr) and np.array_equal(nodes, wn)
        assert len(g.tick_wait()) == 4
        t.remove_batch(wr)
        assert np.array_equal(g.get_assign(), wA) and np.array_equal(g.get_nodes()[2], t.get_nodes()[2])
        assert g.tick() == t.tick() and np.array_equal(g.get_assign(), t.get_assign())
    finally:
        g.close()
        t.close()


@pytest.mark.gpu
def test_an_uncommitted_solve_is_dropped_only_when_something_expired(gp):
    g, rng, load, m = _settled(gp)
    n = g.num_objects
    try:
        g.touch_all(3)
        g.set_alive(1, 0)
        g.solve()
        solved = g.get_solved()
        g.touch(np.arange(10, dtype=np.uint32), 7)            # touches are no input of the solve
        buf = np.empty((2, 16), np.uint32)
        assert g.expire(7, count_only=True)[2] > 0             # count only
        assert g.expire_raw(3, buf[0], buf[1], 16) == (gp.OK, 0)   # a listing call that finds nothing
        assert g.expire_raw(7, want_n_idle=False)[0] == gp.EINVAL
        assert np.array_equal(g.get_solved(), solved)
        g.commit()
        assert np.array_equal(g.get_assign(), solved)
        g.set_alive(2, 0)
        g.solve()
        assert len(g.expire(7, cap=5)[0]) == 5                 # five rows un-placed: the solve no longer describes the table
        with pytest.raises(gp.ObjectPlacementError):
            g.commit()
    finally:
        g.close()


@pytest.mark.gpu
def test_count_only_and_zero_hit_calls_keep_quiet_ticks_chained(gp):
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
        g.touch_all(5)
        for _ in range(3):                                   # quiet from here on
            g.tick_async()
        st0 = g.tick_wait()
        assert all(s["slow_path"] == 0 for s in st0)
        c0 = g.chained_scans()
        for _ in range(10):
            g.tick_async()
        g.touch(np.arange(100, dtype=np.uint32), 6)           # a touch, a count, a listing call that finds nothing
        assert g.expire(0xFFFFFFFF, count_only=True)[2] == int((A != NONE).sum())
        assert g.expire(5)[2] == 0
        c1 = g.chained_scans()
        for _ in range(10):
            g.tick_async()
        st = g.tick_wait()
        c2 = g.chained_scans()
        assert c1 - c0 == 10 and c2 - c1 == 10, (c0, c1, c2)
        assert all(s == st0[-1] for s in st) and np.array_equal(g.get_assign(), A)
        assert g.expire(6, cap=3)[2] == int((A[100:] != NONE).sum())      # three rows un-placed: the inputs changed
        for _ in range(10):
            g.tick_async()
        g.tick_wait()
        assert g.chained_scans() - c2 < 10
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("life", [False, True])
def test_the_change_feed_lists_the_expired_rows_as_deletes(gp, life):
    g, rng, load, m = _settled(gp, n=50_000, life=life)
    n = g.num_objects
    try:
        g.changes()                                          # the consumer knows every row
        keep = rng.integers(0, n, n // 2).astype(np.uint32)
        g.touch(keep, 2)
        rows, nodes, n_idle, freed = g.expire(2, cap=4000)
        assert len(rows) == 4000 < n_idle
        r, o, w, total = g.changes()
        assert total == 4000 and np.array_equal(r, rows) and np.array_equal(o, nodes) and (w == NONE).all()
        aff = g.get_objects()[1]
        assert (aff[rows] == gp.AFF_INACTIVE).all() == life
    finally:
        g.close()


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
        err = lambda: g._L.rio_gp_last_error(g.handle).decode()
        assert g.expire_raw(1)[0] == gp.EINVAL and "row-sharded" in err()
        assert g.touch_raw([1], 1) == gp.EINVAL and "row-sharded" in err()
        for call in (lambda: g.touch_all(1), lambda: g.touch_merge(np.ones(4, np.uint32)), g.get_seen):
            with pytest.raises(gp.ObjectPlacementError) as e:
                call()
            assert e.value.rc == gp.EINVAL and "row-sharded" in e.value.text
        assert L.rio_gp_shard_p2p_close(g.handle) == gp.OK
        assert g.expire(1, count_only=True)[2] == 0
    finally:
        g.close()


@pytest.mark.gpu
def test_config3_ten_million_rows_a_tenth_seen_later(gp):
    cfg = synth.config("c3")
    n, m = cfg["n"], cfg["m"]
    g = gp.GpuPlacement(n, m)
    try:
        g.set_nodes(cfg["cap"], cfg["alive"])
        g.set_objects(n, cfg["load"], cfg["aff"])
        g.set_assign(synth.warm_assign(n, m))
        g.tick()
        A = g.get_assign()
        g.touch_all(1)
        late = np.arange(3, n, 10, dtype=np.uint32)
        g.touch(late, 2)
        S = spec.touch(spec.touch_all(np.zeros(n, np.uint32), n, 1), late, 2)
        assert g.expire(1, count_only=True)[2] == 0
        for cap in (100_000, None):
            wr, wn, wi, wf, wA = spec.expire(A, S, cfg["load"], n, 2, cap)
            rows, nodes, n_idle, freed = g.expire(2, cap=cap)
            assert (n_idle, freed) == (wi, wf) and wi > n // 2
            assert np.array_equal(rows, wr) and np.array_equal(nodes, wn)
            A = g.get_assign()
            assert np.array_equal(A, wA)
        assert g.count_placed() == int((A[late] != NONE).sum()) and g.expire(2, count_only=True)[2] == 0
        assert np.array_equal(g.get_seen(), S)
    finally:
        g.close()
