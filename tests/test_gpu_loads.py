"""Measured load on the MI355X (rio_gp_hits_add_batch / _dev, rio_gp_hits_merge / _dev, rio_gp_get_hits, rio_gp_load_fold): every
call against the restatement with Python integers (tests/spec_loads.py) and, for `used`, against a numpy k_used, at sizes around
the quads and the 256-thread workgroups and with node counts on both sides of the fold's LDS accumulators (4 096); the scatter's
saturating sum with 100 000 entries on one row; rows hidden by rio_gp_set_num_objects; the fold with `used` valid and invalid;
the tick and the rebalance that follow a fold, against the oracle and the rebalance reference over the new loads; an uncommitted
solve, ticks in flight, a chained quiet run; the feed and the last-seen column, which no call of the family touches; refusals."""
import ctypes as C

import numpy as np
import pytest

import rebalance_ref
import spec_loads as spec

NONE = 0xFFFFFFFF
M32 = 0xFFFFFFFF
EXTRA = 300
FOLDS = [(65536, 1, 0, M32), (32768, 3, 1, 40), (0, 2, 0, M32), (65535, M32, 2, M32), (65536, 0, 7, 7)]


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


def _table(n, m, seed, headroom=1.3):
    rng = np.random.default_rng(seed)
    load = rng.integers(1, 5, max(n, 1)).astype(np.uint32)[:n]
    aff = rng.integers(0, m, max(n, 1)).astype(np.uint32)[:n]
    cap = np.full(m, int(max(1, load.sum()) * headroom / m) + 8, np.uint64)
    return rng, load, aff, cap


def _dev_u32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).cuda()


class Dense:
    """A handle and what the restatement says its load and hit columns hold (all max_objects rows of both)."""

    def __init__(self, gp, n, m, seed, headroom=1.3, lab=False):
        self.rng, load, self.aff, self.cap = _table(n, m, seed, headroom)
        self.m, self.alive = m, np.ones(m, np.uint8)
        self.g = gp.GpuPlacement(n + EXTRA, m, spill_rounds=2, lab=lab)
        self.g.set_nodes(self.cap, self.alive)
        self.g.set_objects(n, load, self.aff)
        self.load = np.zeros(n + EXTRA, np.uint32)               # (rows never set hold load 0)
        self.load[:n] = load
        self.H = np.zeros(n + EXTRA, np.uint32)

    def same(self):
        """load, H and `used` are the restatement's; returns the committed column"""
        g = self.g
        n = g.num_objects
        A = g.get_assign()
        assert np.array_equal(g.get_objects()[0], self.load[:n])
        assert np.array_equal(g.get_hits(), self.H[:n])
        assert np.array_equal(g.get_nodes()[2], spec.used_of(A, self.load, n, self.m))
        return A

    def fold(self, keep, gain, lo, hi):
        n = self.g.num_objects
        self.load, self.H, want = spec.load_fold(self.load, self.H, n, keep, gain, lo, hi)
        st = self.g.load_fold(keep, gain, lo, hi)
        assert st == want
        return st


SIZES = [(n, 64) for n in (0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025)] + \
        [(4097, m) for m in (1, 64, 65, 4095, 4096, 4097, 8192)] + [(1025, 4097)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", SIZES)
def test_hits_and_folds_match_the_spec(gp, oracle, n, m):
    import torch
    d = Dense(gp, n, m, n * 13 + m)
    g, rng = d.g, d.rng
    try:
        S = np.zeros(n, np.uint32)
        S[::3] = 4
        g.touch_merge(S)                                      # a last-seen column and a feed to leave alone
        g.tick()
        g.changes()
        A0 = d.same()
        # -- the four ways into H --
        if n:
            idx = rng.integers(0, n, 1 + 2 * n).astype(np.uint32)
            idx[-1] = idx[0]
            w = rng.integers(0, 4, len(idx)).astype(np.uint32)   # weight 0 among them
            g.hits_add(idx, w)
            d.H = spec.hits_add(d.H, idx, w)
            g.hits_add(idx[: 1 + n // 2])                     # NULL weights: 1 each
            d.H = spec.hits_add(d.H, idx[: 1 + n // 2])
            di = _dev_u32(idx)
            dw = _dev_u32(w)
            torch.cuda.synchronize()
            g.hits_add_dev(di.data_ptr(), len(idx), dw.data_ptr())
            d.H = spec.hits_add(d.H, idx, w)
            g.hits_add_dev(di.data_ptr(), len(idx) // 2)
            d.H = spec.hits_add(d.H, idx[: len(idx) // 2])
        else:
            g.hits_add(np.empty(0, np.uint32))
        rows = n - n // 3                                     # rows < n (rows == n for the smallest tables)
        c = rng.integers(0, 3, max(rows, 1)).astype(np.uint32)[:rows]
        if rows:
            c[0] = M32 - 1                                    # saturates, or comes close
        g.hits_merge(c)
        d.H = spec.hits_merge(d.H, c)
        c2 = rng.integers(0, 1000, n + 1).astype(np.uint32)
        dc = _dev_u32(c2)
        torch.cuda.synchronize()
        g.hits_merge_dev(dc.data_ptr() + 4 if n else None, n)    # a pointer 4 bytes off the allocation's alignment
        d.H = spec.hits_merge(d.H, c2[1:])
        g.hits_merge_dev(dc.data_ptr() if n else None, n)        # and an aligned one
        d.H = spec.hits_merge(d.H, c2[:n])
        with pytest.raises(gp.ObjectPlacementError) as e:
            g.hits_merge(np.ones(n + 1, np.uint32))           # rows > n
        assert e.value.rc == gp.EINVAL
        assert np.array_equal(d.same(), A0)
        # -- the fold with `used` valid (a tick and get_nodes came before) --
        d.fold(*FOLDS[(n + m) % len(FOLDS)])
        assert np.array_equal(d.same(), A0)
        # -- the fold with `used` invalid --
        if n:
            idx = rng.integers(0, n, 1 + n // 4).astype(np.uint32)
            idx = np.unique(idx)
            nl = rng.integers(0, 9, len(idx)).astype(np.uint32)
            g.set_object_attrs(idx, load=nl)
            d.load[idx] = nl
            g.hits_add(idx)
            d.H = spec.hits_add(d.H, idx)
        d.fold(*FOLDS[(n + m + 1) % len(FOLDS)])
        assert np.array_equal(d.same(), A0)
        # -- rows hidden by rio_gp_set_num_objects keep load and H, and take part again --
        if n:
            every = np.arange(n, dtype=np.uint32)
            g.hits_add(every, every % 5)
            d.H = spec.hits_add(d.H, every, every % 5)
        g.set_num_objects(n // 2)
        d.fold(32768, 2, 0, 1000)
        d.same()
        g.set_num_objects(n + EXTRA)                          # ... with rows never used behind them
        assert np.array_equal(g.get_objects()[0][n:], d.load[n:])
        d.same()
        g.hits_merge(np.full(n + EXTRA, 2, np.uint32))
        d.H = spec.hits_merge(d.H, np.full(n + EXTRA, 2, np.uint32))
        g.set_num_objects(n)
        g.get_nodes()                                         # `used` valid again
        d.fold(65536, 1, 1, 50)
        A = d.same()
        # -- nothing of this touched the feed or the last-seen column --
        r, o, w_, total = g.changes(peek=True)
        assert total == int((A != A0).sum())                  # (rows un-hidden again: nothing else)
        assert np.array_equal(g.get_seen(), S)
        # -- the next tick is the oracle's over the new loads --
        st = g.tick()
        want, used, ost = oracle.tick(A, d.load[:n], d.aff, d.cap, d.alive)
        assert st == ost and np.array_equal(g.get_assign(), want)
        assert np.array_equal(g.get_nodes()[2], used[:m])
        g.set_num_objects(n + EXTRA)
        assert np.array_equal(g.get_hits()[n:], d.H[n:])      # the hidden rows' hits are still there
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dev", [False, True])
def test_one_row_named_100000_times_and_a_saturating_row(gp, dev):
    import torch
    n = 5000
    d = Dense(gp, n, 8, 1)
    g = d.g
    try:
        idx = np.full(100_000, 77, np.uint32)
        idx[::1000] = 78
        heavy = np.array([9, 9, 9, 10, 10, 11], np.uint32)
        hw = np.array([1 << 31, 1 << 31, 1 << 31, 1 << 31, (1 << 31) - 1, 0], np.uint32)
        if dev:
            a, b, c = _dev_u32(idx), _dev_u32(heavy), _dev_u32(hw)
            torch.cuda.synchronize()
            g.hits_add_dev(a.data_ptr(), len(idx))
            g.hits_add_dev(b.data_ptr(), len(heavy), c.data_ptr())
        else:
            g.hits_add(idx)
            g.hits_add(heavy, hw)
        H = g.get_hits()
        want = spec.hits_add(spec.hits_add(d.H, idx), heavy, hw)
        assert np.array_equal(H, want[:n])
        assert (H[77], H[78], H[9], H[10], H[11]) == (99_900, 100, M32, M32, 0)
        # saturated words stay where they are, whatever comes
        w2 = np.full(100_000, 3, np.uint32)
        nine = np.full(100_000, 9, np.uint32)
        if dev:
            a, b = _dev_u32(nine), _dev_u32(w2)
            torch.cuda.synchronize()
            g.hits_add_dev(a.data_ptr(), len(nine), b.data_ptr())
        else:
            g.hits_add(nine, w2)
        assert np.array_equal(g.get_hits(), want[:n])
    finally:
        g.close()


@pytest.mark.gpu
def test_dev_form_skips_invalid_entries_and_host_form_refuses_them(gp):
    import torch
    n = 1000
    d = Dense(gp, n, 8, 2)
    g = d.g
    try:
        bad = _dev_u32([1, n + 5, 2, n, 1])
        w = _dev_u32([4, 4, 0, 4, 6])
        torch.cuda.synchronize()
        with pytest.raises(gp.ObjectPlacementError) as e:
            g.hits_add_dev(bad.data_ptr(), 5, w.data_ptr())
        assert e.value.rc == gp.EINVAL
        d.H[1] = 10
        d.same()
        assert g.hits_add_raw([0, n]) == gp.EINVAL            # one entry out of range: nothing is counted
        assert g.hits_add_raw(None, n=3) == gp.EINVAL         # a NULL idx with n > 0
        d.same()
    finally:
        g.close()


@pytest.mark.gpu
def test_refusals_change_nothing(gp):
    import sharded
    L = sharded._lib()
    n = 4096
    d = Dense(gp, n, 8, 3)
    g = d.g
    try:
        g.tick()
        g.hits_add(np.arange(0, n, 7, dtype=np.uint32))
        d.H = spec.hits_add(d.H, np.arange(0, n, 7))
        A = d.same()
        err = lambda: g._L.rio_gp_last_error(g.handle).decode()
        assert g.load_fold_raw(65537, 1, 0, 10) == gp.EINVAL and "keep" in err()
        assert g.load_fold_raw(65536, 1, 11, 10) == gp.EINVAL and "min_load" in err()
        assert g.hits_add_raw(None, n=1) == gp.EINVAL
        assert np.array_equal(d.same(), A)
        h64 = (C.c_char * 64)()
        assert L.rio_gp_shard_p2p_export(g.handle, 1, h64) == gp.OK
        assert g.load_fold_raw(65536, 1, 0, 10) == gp.EINVAL and "row-sharded" in err()
        assert g.hits_add_raw([1]) == gp.EINVAL and "row-sharded" in err()
        for call in (lambda: g.hits_merge(np.ones(4, np.uint32)), g.get_hits, lambda: g.hits_merge_dev(None, 0),
                     lambda: g.hits_add_dev(None, 0)):
            with pytest.raises(gp.ObjectPlacementError) as e:
                call()
            assert e.value.rc == gp.EINVAL and "row-sharded" in e.value.text
        assert L.rio_gp_shard_p2p_close(g.handle) == gp.OK
        assert np.array_equal(d.same(), A)
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(4097, 64), (70_001, 4097)])
def test_a_rebalance_after_the_fold_moves_what_the_reference_says(gp, n, m):
    rng = np.random.default_rng(n + m)
    cur, load, aff, alive, T = rebalance_ref.random_table(rng, n, m, "tight", max_load=50)
    cap = np.full(m, gp.CAP_INF, np.uint64)
    g = gp.GpuPlacement(n, m + 3)
    try:
        top = int(cur[cur != NONE].max()) + 1 if (cur != NONE).any() else 0
        g.set_nodes(np.full(max(top, m), gp.CAP_INF, np.uint64), np.ones(max(top, m), np.uint8))
        g.set_objects(n, load, aff)
        g.set_assign(cur)
        g.set_nodes(cap, alive)
        hits = (rng.zipf(1.3, n) % 1000).astype(np.uint32)
        g.hits_merge(hits)
        st = g.load_fold(16384, 1, 1, 200)
        nl, H, want = spec.load_fold(load, hits, n, 16384, 1, 1, 200)
        assert st == want and np.array_equal(g.get_objects()[0], nl) and not g.get_hits().any()
        assert np.array_equal(g.get_nodes()[2], spec.used_of(cur, nl, n, m))
        st, rows, frm, to = g.rebalance(T, None, 2)
        nxt, used, wst, wrows, wfrom, wto = rebalance_ref.rebalance(cur, nl, aff, cap, alive, T, None, 2)
        assert st == wst and np.array_equal(rows, wrows) and np.array_equal(frm, wfrom) and np.array_equal(to, wto)
        assert np.array_equal(g.get_assign(), nxt) and np.array_equal(g.get_nodes()[2], used)
    finally:
        g.close()


@pytest.mark.gpu
def test_a_fold_drops_an_uncommitted_solve_and_hits_do_not(gp):
    d = Dense(gp, 200_000, 64, 5)
    g = d.g
    try:
        g.tick()
        g.set_alive(1, 0)
        g.solve()
        solved = g.get_solved()
        g.hits_add(np.arange(10, dtype=np.uint32))            # hits are no input of the solve
        g.hits_merge(np.ones(100, np.uint32))
        assert g.get_hits()[:12].tolist() == [2] * 10 + [1, 1]
        assert np.array_equal(g.get_solved(), solved)
        g.commit()
        assert np.array_equal(g.get_assign(), solved)
        g.set_alive(2, 0)
        g.solve()
        g.update_batch(np.array([5], np.uint32), np.array([3], np.uint32))
        with pytest.raises(gp.ObjectPlacementError) as e1:
            g.commit()
        g.solve()
        g.load_fold(65536, 1, 0, M32)                         # the loads changed: the solve no longer describes the table
        with pytest.raises(gp.ObjectPlacementError) as e2:
            g.commit()
        assert e1.value.rc == e2.value.rc and e1.value.text == e2.value.text
    finally:
        g.close()


@pytest.mark.gpu
def test_a_fold_orders_itself_behind_ticks_in_flight(gp, oracle):
    import synth
    n = 1 << 20
    cfg = synth.config("c3", n_override=n)
    m = cfg["m"]
    g = gp.GpuPlacement(n, m)
    try:
        g.set_nodes(cfg["cap"], cfg["alive"])
        g.set_objects(n, cfg["load"], cfg["aff"])
        ref, _u, _s = oracle.tick(np.full(n, NONE, np.uint32), cfg["load"], cfg["aff"], cfg["cap"], cfg["alive"])
        g.tick()
        hits = (np.arange(n, dtype=np.uint64) * 2654435761 % 7).astype(np.uint32)
        g.hits_merge(hits)
        want = []
        for k in range(4):
            mask = synth.churn_mask(m, k + 1)
            g.set_alive_all(mask)
            g.tick_async()
            ref, used, ost = oracle.tick(ref, cfg["load"], cfg["aff"], cfg["cap"], mask)
            want.append(ost)
        st = g.load_fold(32768, 5, 1, 100)                    # no tick_wait in between
        nl, H, wst = spec.load_fold(cfg["load"], hits, n, 32768, 5, 1, 100)
        assert st == wst
        assert g.tick_wait() == want
        assert np.array_equal(g.get_assign(), ref) and np.array_equal(g.get_objects()[0], nl)
        assert np.array_equal(g.get_nodes()[2], spec.used_of(ref, nl, n, m))
        nxt, used, ost = oracle.tick(ref, nl, cfg["aff"], cfg["cap"], mask)
        assert g.tick() == ost and np.array_equal(g.get_assign(), nxt) and np.array_equal(g.get_nodes()[2], used)
    finally:
        g.close()


@pytest.mark.gpu
def test_a_fold_in_the_middle_of_a_chained_quiet_run(gp, oracle):
    n, m = (1 << 18) + 3 * 1024 + 5, 64
    d = Dense(gp, n, m, 9, headroom=1.5, lab=True)
    g = d.g
    load0 = d.load[:n].copy()
    try:
        ref = np.full(n, NONE, np.uint32)
        for _ in range(10):                                   # settle: ticks until one left every object placed
            st = g.tick()
            ref, used, ost = oracle.tick(ref, load0, d.aff, d.cap, d.alive)
            assert st == ost
            if st["slow_path"] == 0 and st["evicted"] == 0:
                break
        for _ in range(3):
            g.tick_async()
        st0 = g.tick_wait()
        q, qused, qst = oracle.tick(ref, load0, d.aff, d.cap, d.alive)
        assert np.array_equal(q, ref) and all(s == qst for s in st0)
        c0 = g.chained_scans()
        for _ in range(10):
            g.tick_async()
        hits = np.zeros(n, np.uint32)
        hits[::97] = 150                                      # a few rows grow heavy: the table no longer fits its nodes
        g.hits_merge(hits)                                    # hits alone leave the run chained
        c1 = g.chained_scans()
        st = g.load_fold(65536, 1, 0, M32)
        nl, H, wst = spec.load_fold(load0, hits, n, 65536, 1, 0, M32)
        assert st == wst
        for _ in range(10):
            g.tick_async()
        got = g.tick_wait()
        c2 = g.chained_scans()
        assert c1 - c0 == 10 and c2 - c1 < 10, (c0, c1, c2)   # the tick after the fold is no link over the old loads
        want = [qst] * 10
        for _ in range(10):
            ref, used, ost = oracle.tick(ref, nl, d.aff, d.cap, d.alive)
            want.append(ost)
        assert got == want
        assert np.array_equal(g.get_assign(), ref) and np.array_equal(g.get_nodes()[2], used)
        assert np.array_equal(g.get_objects()[0], nl) and not g.get_hits().any()
    finally:
        g.close()
