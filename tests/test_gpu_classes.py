"""Object classes on the MI355X (rio_gp_set_class*, rio_gp_get_classes, rio_gp_expire_classes / _dev, rio_gp_census / _dev): every
call against the plain restatement (tests/spec_classes.py); the sweep also against a twin handle that receives
rio_gp_remove_batch of the restatement's rows instead (the Pair of tests/test_gpu_expire.py), at sizes around the passes' tiles
(1 024 rows) and workgroups, with and without the row lifecycle, with few and with more nodes than the apply pass gathers in LDS
(4 096); equality with rio_gp_expire on an all-zero class column; ticks in flight, an uncommitted solve, quiet ticks that stay
chained; the change feed afterwards; the row-sharded refusal; the class column under remap_nodes and a changing row count; the
census in each of its three forms: one slice of LDS accumulators (up to kCensusLdsCells = 4 096 cells), several slices (up to
kCensusMaxSlices = 16 of them) and global adds beyond."""
import ctypes as C

import numpy as np
import pytest

import spec_classes as spec
import spec_expire
import synth
from test_gpu_expire import CAPS, TILE, Pair, _dev_u32, _settled, _table

NONE = 0xFFFFFFFF
CENSUS_LDS_CELLS = 4096   # kCensusLdsCells: the cells one workgroup of k_census accumulates in LDS (one slice)
CENSUS_MAX_SLICES = 16    # kCensusMaxSlices: (by node ? m : 1) * n_classes up to 16 * 4 096 stays in LDS, a pass per slice
SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4096, 4097]


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


def _dev_u8(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8).copy()).cuda()


def _odd(a):
    """a copy of the uint8 array `a` that starts at an odd address"""
    buf = np.empty(len(a) + 16, np.uint8)
    off = 1 if buf.ctypes.data % 2 == 0 else 0
    out = buf[off:off + len(a)]
    out[:] = a
    assert len(a) == 0 or out.ctypes.data % 2 == 1
    return out


# ---- setters and getter ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_setters_and_getter(gp, n):
    import torch
    rng = np.random.default_rng(n)
    g = gp.GpuPlacement(n + 8, 4)
    try:
        g.set_nodes(None, np.ones(4, np.uint8))
        g.set_objects(n)
        assert not g.get_classes().any() and len(g.get_classes()) == n       # first use: zero everywhere
        K = np.zeros(n, np.uint8)
        k = 0
        for first in (0, 1, 3, 4, 5, 1021):
            for rows in (0, 1, 3, 4, 5, 1027):
                k += 1
                sent = rng.integers(1, 256, n).astype(np.uint8)              # the sentinel pattern around the range
                g.set_classes(0, sent)
                K = spec.set_classes(K, 0, sent)
                cls = _odd(rng.integers(0, 256, rows).astype(np.uint8))
                if first + rows > n:                                          # RIO_GP_EINVAL and nothing changes
                    assert g.set_classes_raw(first, cls) == gp.EINVAL
                elif k % 2:
                    assert g.set_classes_raw(first, cls) == gp.OK
                    K = spec.set_classes(K, first, cls)
                else:
                    d = _dev_u8(np.concatenate([[7], cls]))                   # the device pointer at an odd address too
                    torch.cuda.synchronize()
                    g.set_classes_dev(first, d.data_ptr() + 1, rows)
                    K = spec.set_classes(K, first, cls)
                assert np.array_equal(g.get_classes(), K), (first, rows)
        if n:
            # the scatter with duplicates: the last entry of a row wins
            for size in (1, 7, 300, 5000):
                idx = rng.integers(0, n, size).astype(np.uint32)
                idx[size // 2:] = idx[: size - size // 2][::-1]               # every row of the first half comes again
                cls = rng.integers(0, 256, size).astype(np.uint8)
                g.set_class_batch(idx, _odd(cls))
                K = spec.set_class_batch(K, idx, cls)
                assert np.array_equal(g.get_classes(), K), size
            # the host form validates first; the _dev form skips the invalid entries and says so
            assert g.set_class_batch_raw([0, n, 0], [1, 2, 3]) == gp.EINVAL
            assert np.array_equal(g.get_classes(), K)
            idx = np.array([0, n, n - 1, 0xFFFFFFFF, 0, n + 7], np.uint32)
            cls = np.array([11, 12, 13, 14, 15, 16], np.uint8)
            di, dc = _dev_u32(idx), _dev_u8(cls)
            torch.cuda.synchronize()
            assert g.set_class_batch_dev_raw(di.data_ptr(), dc.data_ptr(), len(idx)) == gp.EINVAL
            ok = idx < n
            K = spec.set_class_batch(K, idx[ok], cls[ok])
            assert np.array_equal(g.get_classes(), K)
            idx = rng.integers(0, n, 2000).astype(np.uint32)
            cls = rng.integers(0, 256, 2000).astype(np.uint8)
            di, dc = _dev_u32(idx), _dev_u8(cls)
            torch.cuda.synchronize()
            assert g.set_class_batch_dev_raw(di.data_ptr(), dc.data_ptr(), len(idx)) == gp.OK
            K = spec.set_class_batch(K, idx, cls)
            assert np.array_equal(g.get_classes(), K)
            # the election's scratch is at rest again: an update batch with duplicates still elects its last writer
            g.update_batch(np.array([0, 0, 0], np.uint32), np.array([1, 2, 3], np.uint32))
            assert g.get_assign()[0] == 3
        else:
            assert g.set_class_batch_raw([0], [1]) == gp.EINVAL
        assert g.set_class_batch_raw([], []) == gp.OK
    finally:
        g.close()


# ---- the sweep ---------------------------------------------------------------------------------------------------------------

class ClassPair(Pair):
    """tests/test_gpu_expire.py's Pair with the class column the restatement keeps."""

    def __init__(self, gp, max_objects, m, life):
        super().__init__(gp, max_objects, m, life)
        self.K = np.zeros(max_objects, np.uint8)

    def check_classes(self, cutoffs, cap=None):
        """One rio_gp_expire_classes against the restatement and the twin; returns (listed, n_idle)."""
        g, t = self.g, self.t
        n = g.num_objects
        A = g.get_assign()
        load = g.get_objects()[0]
        count = cap == "count"
        wr, wn, wi, wf, wA, wby = spec.expire_classes_np(A, self.S, self.K, load, n, cutoffs, 0 if count else cap)
        rows, nodes, n_idle, freed, by = (g.expire_classes(cutoffs, count_only=True) if count
                                          else g.expire_classes(cutoffs, cap=cap))
        assert n_idle == wi and freed == wf
        assert np.array_equal(by, wby)                                        # every idle row, listed or not
        assert np.array_equal(rows, wr) and np.array_equal(nodes, wn)
        assert np.array_equal(g.get_assign(), wA)
        assert np.array_equal(g.get_seen(), self.S[:n]) and np.array_equal(g.get_classes(), self.K[:n])
        if len(wr):
            t.remove_batch(wr)
        self.same_state()
        return len(wr), wi


TABLES = [(n, 16) for n in (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 4096, 4097, (1 << 20) + 17)] + [(70_000, 1), (70_000, 4097)]
N_CLASSES = [1, 2, 37, 256]


@pytest.mark.gpu
@pytest.mark.parametrize("life", [False, True])
@pytest.mark.parametrize("n,m", TABLES)
def test_the_per_class_sweep_matches_the_spec_and_the_twin(gp, n, m, life):
    import torch
    extra = 3000
    rng, load, aff, cap = _table(n, m, n + m + 1)
    p = ClassPair(gp, n + extra, m, life)
    g = p.g
    try:
        p.both("set_nodes", cap, np.ones(m, np.uint8))
        p.both("set_objects", n, load, aff)
        assert p.check_classes([5]) == (0, 0)                 # nothing placed yet: nothing is idle
        a, b = p.both("tick")
        assert a == b
        epoch = 1
        for it in range(12):
            k = it % 6
            epoch += 1
            nc = N_CLASSES[it % 4]
            # -- touches (S is the restatement's) and classes (K is), some of them >= n_classes --
            if n:
                idx = rng.integers(0, n, 1 + n // 3).astype(np.uint32)
                g.touch(idx, epoch)
                p.S = spec_expire.touch(p.S, idx, epoch)
            if it % 3 == 0:
                cls = rng.integers(0, min(256, nc + 3), n + extra).astype(np.uint8)   # rows >= n carry classes too
                p.both("set_num_objects", n + extra)
                g.set_classes(0, cls)
                p.both("set_num_objects", n)
                p.K = spec.set_classes(p.K, 0, cls)
            elif n:
                idx = rng.integers(0, n, 1 + n // 7).astype(np.uint32)
                cls = rng.integers(0, 256, len(idx)).astype(np.uint8)
                g.set_class_batch(idx, cls)
                p.K = spec.set_class_batch(p.K, idx, cls)
            # -- a change of the table, on both handles --
            if n and k == 0:
                idx = rng.integers(0, n, 1 + n // 10).astype(np.uint32)
                node = rng.integers(0, m + 1, len(idx)).astype(np.uint32)
                node[node == m] = NONE
                p.both("update_batch", idx, node)
            elif n and k == 1:
                p.both("remove_batch", rng.integers(0, n, 1 + n // 20).astype(np.uint32))
            elif k == 2:
                alive = (rng.random(m) < 0.8).astype(np.uint8)
                alive[0] = 1
                p.both("set_alive_all", alive)
                a, b = p.both("tick")
                assert a == b
            elif k == 3:
                p.both("set_num_objects", n // 2)            # rows >= n/2 are never idle and keep S and K ...
                p.check_classes(np.full(nc, epoch, np.uint32), cap=[None, 3][(it // 6) % 2])
                p.both("set_num_objects", n + extra)         # ... and come back, with rows never used behind them
                p.check_classes(np.full(nc, epoch - 1, np.uint32), cap="count")
                p.both("set_num_objects", n)
            elif k == 4:
                p.both("set_alive_all", np.ones(m, np.uint8))
                a, b = p.both("tick")
                assert a == b
            # -- the sweep: cutoffs among 0, a row's own stamp (epoch: not idle), one above it and 0xFFFFFFFF --
            cut = rng.choice(np.array([0, epoch - 1, epoch, epoch + 1, 0xFFFFFFFF, 2], np.uint32), nc)
            cut[it % nc] = [0xFFFFFFFF, epoch, 0][it % 3]
            capv = CAPS[it % 5]
            if capv is None and it % 2:
                capv = 7                                     # (everything idle, every time, would leave little to check)
            p.check_classes(cut, capv)
        a, b = p.both("tick")                                # the next tick says the same on both
        assert a == b
        p.same_state()
        # the _dev form against the restatement: a page; nothing is written past the listing
        A, ld = g.get_assign(), g.get_objects()[0]
        cut = np.full(256, 0xFFFFFFFF, np.uint32)
        wr, wn, wi, wf, wA, wby = spec.expire_classes_np(A, p.S, p.K, ld, n, cut, 100)
        d = [torch.full((100 + 5,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        n_idle, freed, by = g.expire_classes_dev(cut, d[0].data_ptr(), d[1].data_ptr(), cap=100)
        assert (n_idle, freed) == (wi, wf) and np.array_equal(by, wby) and wi == g.count_placed() + len(wr)
        got = [x.cpu().numpy().view(np.uint32) for x in d]
        assert np.array_equal(got[0][:len(wr)], wr) and np.array_equal(got[1][:len(wr)], wn) and (got[0][len(wr):] == NONE).all()
        assert np.array_equal(g.get_assign(), wA)
        if len(wr):
            p.t.remove_batch(wr)
        assert g.expire_classes_dev(cut)[0] == wi - len(wr)  # the _dev form's count only
        p.same_state()
        pages = 0
        while p.check_classes(cut, cap=37)[0]:               # page out everything that is placed
            pages += 1
            if pages == 4:
                p.check_classes(cut)                         # (the rest in one call)
        assert p.check_classes(cut) == (0, 0) and g.count_placed() == 0
    finally:
        p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,life", [(TILE + 1, 16, True), (70_000, 4097, False), ((1 << 20) + 17, 16, False)])
def test_with_an_all_zero_column_one_class_is_the_plain_sweep(gp, n, m, life):
    rng, load, aff, cap = _table(n, m, 3 * n + m)
    p = Pair(gp, n, m, life)                                  # g: rio_gp_expire_classes(1, {cutoff}); t: rio_gp_expire(cutoff)
    try:
        p.both("set_nodes", cap, np.ones(m, np.uint8))
        p.both("set_objects", n, load, aff)
        p.both("tick")
        p.both("touch_merge", rng.integers(0, 9, n).astype(np.uint32))
        for cutoff, capv in ((0, None), (3, "count"), (3, 1), (3, 7), (5, 1 << 40), (0xFFFFFFFF, 1000), (0xFFFFFFFF, None)):
            count = capv == "count"
            a = p.g.expire_classes([cutoff], count_only=True) if count else p.g.expire_classes([cutoff], cap=capv)
            b = p.t.expire(cutoff, count_only=True) if count else p.t.expire(cutoff, cap=capv)
            assert all(np.array_equal(x, y) for x, y in zip(a[:4], b)) and a[4].tolist() == [b[2]]
            p.same_state()
            assert np.array_equal(p.g.get_seen(), p.t.get_seen())
        assert p.g.count_placed() == 0
    finally:
        p.close()


# ---- interactions ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_call_forms_and_argument_checks(gp):
    g, rng, load, m = _settled(gp, n=20_000)
    n = g.num_objects
    try:
        A = g.get_assign()
        placed = int((A != NONE).sum())
        # first use on a fresh handle: class 0 everywhere, nobody has been seen
        assert g.expire_classes([1], count_only=True)[2] == placed and g.expire_classes([0], count_only=True)[2] == 0
        buf = np.empty((2, 8), np.uint32)
        for kw in (dict(out_rows=buf[0], cap=8), dict(out_node=buf[1], cap=8), dict(cap=8),
                   dict(out_rows=buf[0], out_node=buf[1], cap=8, want_n_idle=False)):
            assert g.expire_classes_raw(1, [1], **kw)[0] == gp.EINVAL
        assert g.expire_classes_raw(0, [1])[0] == gp.EINVAL and g.expire_classes_raw(257, np.ones(257))[0] == gp.EINVAL
        assert g.expire_classes_raw(1, None)[0] == gp.EINVAL
        assert g.expire_classes_raw(256, np.ones(256)) == (gp.OK, placed)
        assert g.census_raw(0)[0] == gp.EINVAL and g.census_raw(257)[0] == gp.EINVAL and g.census_raw(1, flags=2)[0] == gp.EINVAL
        assert np.array_equal(g.get_assign(), A)
        with pytest.raises(gp.ObjectPlacementError):
            g.set_classes(n - 1, np.ones(2, np.uint8))
        assert not g.get_classes().any()
    finally:
        g.close()


@pytest.mark.gpu
def test_sweep_and_census_order_themselves_behind_ticks_in_flight(gp):
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
        S = spec_expire.touch(np.zeros(n, np.uint32), idx, 9)
        K = (np.arange(n) % 5).astype(np.uint8)
        g.set_classes(0, K)
        for k in range(4):
            mask = synth.churn_mask(m, k + 1)
            g.set_alive_all(mask)
            g.tick_async()
            t.set_alive_all(mask)
            t.tick()
        cr, cl, co = g.census(4)                              # no tick_wait in between
        wr, wl, wo = spec.census_np(t.get_assign(), K, cfg["load"], n, 4)
        assert np.array_equal(cr, wr) and np.array_equal(cl, wl) and co == wo
        cut = [9, 0, 9, 3]
        rows, nodes, n_idle, freed, by = g.expire_classes(cut, cap=50_000)
        wr, wn, wi, wf, wA, wby = spec.expire_classes_np(t.get_assign(), S, K, cfg["load"], n, cut, 50_000)
        assert (n_idle, freed) == (wi, wf) and np.array_equal(rows, wr) and np.array_equal(nodes, wn) and np.array_equal(by, wby)
        assert len(g.tick_wait()) == 4
        t.remove_batch(wr)
        assert np.array_equal(g.get_assign(), wA) and np.array_equal(g.get_nodes()[2], t.get_nodes()[2])
        assert g.tick() == t.tick() and np.array_equal(g.get_assign(), t.get_assign())
    finally:
        g.close()
        t.close()


@pytest.mark.gpu
def test_an_uncommitted_solve_is_dropped_only_when_something_was_listed(gp):
    g, rng, load, m = _settled(gp)
    n = g.num_objects
    try:
        g.touch_all(3)
        g.set_alive(1, 0)
        g.solve()
        solved = g.get_solved()
        g.touch(np.arange(10, dtype=np.uint32), 7)
        g.set_classes(0, (np.arange(n) % 3).astype(np.uint8))     # class setters and the census are no input of the solve
        g.set_class_batch([5, 5], [2, 1])
        g.census(3, by_node=True)
        buf = np.empty((2, 16), np.uint32)
        assert g.expire_classes([7, 7, 7], count_only=True)[2] > 0                    # count only
        assert g.expire_classes_raw(3, [3, 0, 2], buf[0], buf[1], 16) == (gp.OK, 0)   # a listing call that finds nothing
        assert g.expire_classes_raw(3, [7, 7, 7], want_n_idle=False)[0] == gp.EINVAL
        assert np.array_equal(g.get_solved(), solved)
        g.commit()
        assert np.array_equal(g.get_assign(), solved)
        g.set_alive(2, 0)
        g.solve()
        assert len(g.expire_classes([0, 7, 0], cap=5)[0]) == 5   # five rows un-placed: the solve no longer describes the table
        with pytest.raises(gp.ObjectPlacementError):
            g.commit()
    finally:
        g.close()


@pytest.mark.gpu
def test_count_only_sweeps_census_calls_and_class_setters_keep_quiet_ticks_chained(gp):
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
        K = (np.arange(n) % 7).astype(np.uint8)
        g.set_classes(0, K)
        for _ in range(3):                                   # quiet from here on
            g.tick_async()
        st0 = g.tick_wait()
        assert all(s["slow_path"] == 0 for s in st0)
        c0 = g.chained_scans()
        for _ in range(10):
            g.tick_async()
        g.set_classes(10, np.full(100, 9, np.uint8))          # setters, a count, a census, a listing call that finds nothing
        g.set_class_batch([3, 4, 3], [1, 1, 2])
        K[10:110] = 9
        K[[3, 4]] = [2, 1]
        placed = A != NONE
        by = g.expire_classes(np.full(7, 0xFFFFFFFF, np.uint32), count_only=True)
        assert by[2] == int((placed & (K < 7)).sum()) and np.array_equal(by[4], np.bincount(K[placed], minlength=10)[:7])
        wr, wl, wo = spec.census_np(A, K, cfg["load"], n, 7, m)
        cr, cl, co = g.census(7, by_node=True)
        assert np.array_equal(cr, wr) and np.array_equal(cl, wl) and co == wo
        assert g.expire_classes(np.full(10, 5, np.uint32))[2] == 0
        c1 = g.chained_scans()
        for _ in range(10):
            g.tick_async()
        st = g.tick_wait()
        c2 = g.chained_scans()
        assert c1 - c0 == 10 and c2 - c1 == 10, (c0, c1, c2)
        assert all(s == st0[-1] for s in st) and np.array_equal(g.get_assign(), A)
        assert len(g.expire_classes(np.full(10, 6, np.uint32), cap=3)[0]) == 3       # three rows un-placed: the inputs changed
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
        g.set_classes(0, (np.arange(n) % 2).astype(np.uint8))
        g.touch(rng.integers(0, n, n // 2).astype(np.uint32), 2)
        rows, nodes, n_idle, freed, by = g.expire_classes([2, 0], cap=4000)
        assert len(rows) == 4000 < n_idle and not (rows % 2).any() and by.tolist() == [n_idle, 0]
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
        assert g.expire_classes_raw(1, [1])[0] == gp.EINVAL and "row-sharded" in err()
        assert g.census_raw(1)[0] == gp.EINVAL and "row-sharded" in err()
        assert g.set_classes_raw(0, np.ones(4, np.uint8)) == gp.EINVAL and "row-sharded" in err()
        assert g.set_class_batch_raw([1], [1]) == gp.EINVAL and "row-sharded" in err()
        with pytest.raises(gp.ObjectPlacementError) as e:
            g.get_classes()
        assert e.value.rc == gp.EINVAL and "row-sharded" in e.value.text
        assert L.rio_gp_shard_p2p_close(g.handle) == gp.OK
        assert g.expire_classes([1], count_only=True)[2] == 0 and not g.get_classes().any()
    finally:
        g.close()


@pytest.mark.gpu
def test_classes_survive_remap_nodes_and_a_changing_row_count(gp):
    g, rng, load, m = _settled(gp, n=30_000, m=8)
    n = g.num_objects
    try:
        K = rng.integers(0, 256, n).astype(np.uint8)
        g.set_classes(0, K)
        g.remap_nodes(np.array([0, NONE, 1, 2, NONE, 3, 4, 5], np.uint32))
        assert np.array_equal(g.get_classes(), K)
        g.set_num_objects(n // 3)
        assert np.array_equal(g.get_classes(), K[: n // 3])
        g.set_classes(1, np.array([77], np.uint8))
        K[1] = 77
        g.tick()
        g.set_num_objects(n)
        assert np.array_equal(g.get_classes(), K)
        wr, wl, wo = spec.census_np(g.get_assign(), K, g.get_objects()[0], n, 200, 6)
        cr, cl, co = g.census(200, by_node=True)
        assert np.array_equal(cr, wr) and np.array_equal(cl, wl) and co == wo
    finally:
        g.close()


# ---- the census --------------------------------------------------------------------------------------------------------------

# cells = m * n_classes by node: 1 and 592 are one slice in LDS, 4 097 and 16 384 two and four slices, 65 536 sixteen, 65 552 and
# 2^20 are added in global memory; the totals form is always one slice
CENSUS_SHAPES = [(1, 1), (16, 37), (1024, 16), (4096, 256), (241, 17), (4097, 16), (4096, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("m,nc", CENSUS_SHAPES)
def test_the_census_matches_the_spec(gp, m, nc):
    import torch
    slices = [-(-m * nc // CENSUS_LDS_CELLS) for m, nc in CENSUS_SHAPES]
    assert slices[:3] == [1, 1, 4] and slices[4] == 2 and slices[6] == CENSUS_MAX_SLICES
    assert all(x > CENSUS_MAX_SLICES for x in (slices[3], slices[5]))
    rng = np.random.default_rng(m + nc)
    for n in SIZES + [(1 << 20) + 17]:
        g = gp.GpuPlacement(n + 8, m + 4)
        try:
            g.set_nodes(m=m + 4)
            load = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
            g.set_objects(n, load, None)
            A = rng.integers(0, m, n).astype(np.uint32)
            A[rng.random(n) < 0.2] = NONE
            A[rng.random(n) < 0.05] = m + 3                  # rows on node ids >= m after a shrinking set_nodes (raw values)
            A[rng.random(n) < 0.02] = m
            if n:
                g.set_assign(A)
            g.set_nodes(m=m)
            K = rng.integers(0, min(256, nc + 2), n).astype(np.uint8)
            g.set_classes(0, K)
            for by_node in (False, True):
                wr, wl, wo = spec.census_np(A, K, load, n, nc, m if by_node else None)
                cr, cl, co = g.census(nc, by_node=by_node)
                assert np.array_equal(cr, wr) and np.array_equal(cl, wl) and co == wo, (n, by_node)
                assert int(cr.sum()) + co == g.count_placed()
            if n in (5, 4097):                               # the _dev form, and a second call adds nothing to the first
                d = [torch.full((m * nc,), -1, dtype=torch.int64, device="cuda") for _ in range(2)]
                torch.cuda.synchronize()
                assert g.census_dev(nc, d[0].data_ptr(), d[1].data_ptr(), by_node=True) == wo
                got = [x.cpu().numpy().view(np.uint64).reshape(m, nc) for x in d]
                assert np.array_equal(got[0], wr) and np.array_equal(got[1], wl)
            assert np.array_equal(g.get_assign(), A) and np.array_equal(g.get_classes(), K)
        finally:
            g.close()


@pytest.mark.gpu
def test_the_census_by_node_refuses_more_than_2_to_the_20_cells(gp):
    g = gp.GpuPlacement(64, 4097)
    try:
        g.set_nodes(None, np.ones(4097, np.uint8))
        g.set_objects(64)
        assert g.census_raw(256, by_node=True)[0] == gp.EINVAL
        assert g.census_raw(255, by_node=True)[0] == gp.OK and g.census_raw(256)[0] == gp.OK
    finally:
        g.close()
