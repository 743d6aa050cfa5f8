"""The change feed on the MI355X (rio_gp_changes / _dev / _reset, rio_op_changes): every listing against the plain restatement
(tests/spec_changes.py) over tables driven through every kind of change — CRUD batches, clean_servers, liveness flips and ticks,
place_pending, rebalance, a shrinking and growing row count — at sizes around the feed's tiles (1 024 rows) and its workgroups;
the call forms (pages, peek, counts only, device arrays, reset); ticks still in flight; quiet ticks that stay chained across a
consuming call; the row-sharded refusal; config 3 at 10 M rows; and the string layer with the write-behind bridge."""
import ctypes as C
import random
import sqlite3

import numpy as np
import pytest

import spec_changes as spec
import synth

NONE = 0xFFFFFFFF
INF = 0xFFFFFFFFFFFFFFFF
TILE = 1024   # kChgTile


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


class Fed:
    """A handle and the numpy checkpoint column the restatement keeps beside it."""

    def __init__(self, g, max_objects):
        self.g = g
        self.B = np.full(max_objects, NONE, np.uint32)

    def check(self, cap=None, peek=False):
        n = self.g.num_objects
        A = self.g.get_assign()
        wr, wo, wn, wt, wB = spec.dense(self.B, A, n, cap, peek)
        rows, old, new, total = self.g.changes(cap=cap, peek=peek)
        assert total == wt
        assert np.array_equal(rows, wr) and np.array_equal(old, wo) and np.array_equal(new, wn)
        self.B = wB
        return total


def _table(gp, n, m, seed, headroom=1.3):
    rng = np.random.default_rng(seed)
    load = rng.integers(1, 5, max(n, 1)).astype(np.uint32)[:n]
    aff = rng.integers(0, m, max(n, 1)).astype(np.uint32)[:n]
    cap = np.full(m, int(max(1, load.sum()) * headroom / m) + 8, np.uint64)
    return rng, load, aff, cap


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, (1 << 20) + 17])
def test_dense_feed_matches_the_spec(gp, n):
    m = 16
    extra = 3000
    rng, load, aff, cap = _table(gp, n, m, n)
    g = gp.GpuPlacement(n + extra, m)
    try:
        g.set_nodes(cap, np.ones(m, np.uint8))
        g.set_objects(n, load, aff)
        f = Fed(g, n + extra)
        assert f.check() == 0                    # nothing placed yet: an empty listing
        g.tick()
        f.check()                                # the first listing: every placed row
        assert f.check() == 0
        for it in range(14):
            k = it % 7
            if n and k == 0:
                idx = rng.integers(0, n, 1 + n // 10).astype(np.uint32)
                node = rng.integers(0, m + 1, len(idx)).astype(np.uint32)
                node[node == m] = NONE
                g.update_batch(idx, node)
            elif n and k == 1:
                g.remove_batch(rng.integers(0, n, 1 + n // 20).astype(np.uint32))
            elif k == 2:
                g.clean_servers([int(rng.integers(0, m))])
            elif k == 3:
                alive = (rng.random(m) < 0.8).astype(np.uint8)
                alive[0] = 1
                g.set_alive_all(alive)
                g.tick()
            elif n and k == 4:
                idx = rng.integers(0, n, 1 + n // 8).astype(np.uint32)
                g.place_pending(idx, rng.integers(0, m, len(idx)).astype(np.uint32))
            elif k == 5:
                g.set_alive_all(np.ones(m, np.uint8))
                g.tick()
                g.rebalance(target=(cap * 2 // 3).astype(np.uint64))
            elif k == 6:
                g.set_num_objects(n // 2)        # rows >= n/2 hide from the feed ...
                f.check(cap=int(rng.integers(0, 5)))
                g.set_num_objects(n + extra)     # ... and come back, with rows never used behind them
                f.check(peek=True)
                g.set_num_objects(n)
            f.check(cap=[None, 1, 7, 1 << 40][it % 4], peek=it % 5 == 4)
        while f.check(cap=37):                   # page out the rest
            pass
        assert f.check() == 0
    finally:
        g.close()


@pytest.mark.gpu
def test_rows_hidden_by_a_smaller_n_survive_the_ticks_in_between(gp):
    """rio_gp_set_num_objects keeps the contents of rows >= n, and the feed compares them as usual once n grows again.  A tick
    while they are hidden publishes the other assignment column: the hidden rows have to be in it.  (They were not: the
    operation-sequence fuzz, extended seed 41, read rows of an older column after n grew back.)"""
    n, m = 6000, 8
    g = gp.GpuPlacement(n, m)
    try:
        g.set_nodes(None, np.ones(m, np.uint8), m=m)
        g.set_objects(n)
        a = (np.arange(n) % m).astype(np.uint32)
        g.set_assign(a)
        f = Fed(g, n)
        assert f.check() == n                    # the consumer knows every row
        for k in (n // 2, 1, 0, n - 1):          # one column swap, then more of them at other sizes
            g.set_num_objects(k)
            g.tick()                             # every node alive, every row placed: the tick keeps rows < k where they are
            assert f.check() == 0
            g.set_num_objects(n)
            assert np.array_equal(g.get_assign(), a), k
            assert f.check() == 0, k             # nothing changed for the consumer either
    finally:
        g.close()


def _churned(gp, n=200_000, m=64, seed=5):
    rng, load, aff, cap = _table(gp, n, m, seed)
    g = gp.GpuPlacement(n, m)
    g.set_nodes(cap, np.ones(m, np.uint8))
    g.set_objects(n, load, aff)
    g.tick()
    return g, rng, m


@pytest.mark.gpu
def test_call_forms_pages_peek_counts_dev_reset(gp):
    import torch
    g, rng, m = _churned(gp)
    n = g.num_objects
    try:
        A = g.get_assign()
        placed = np.flatnonzero(A != NONE).astype(np.uint32)
        # counts only: nothing advances (twice the same total)
        assert g.changes(cap=0)[3] == len(placed) == g.changes(cap=0, peek=True)[3]
        # peek lists and leaves the checkpoint; consuming pages of 1 000 concatenate to the whole listing
        r, o, w, t = g.changes(peek=True)
        assert t == len(placed) and np.array_equal(r, placed) and (o == NONE).all() and np.array_equal(w, A[placed])
        pages = []
        while True:
            pr, po, pw, pt = g.changes(cap=1000)
            if pt == 0:
                break
            assert len(pr) == min(1000, pt)
            pages.append(pr)
        assert np.array_equal(np.concatenate(pages), placed)
        # a change, then the _dev form against the host form (peek both, then consume with _dev)
        g.set_alive_all((rng.random(m) < 0.9).astype(np.uint8))
        g.tick()
        hr, ho, hw, ht = g.changes(peek=True)
        assert ht > 0
        cap = ht + 5
        d = [torch.full((cap,), -1, dtype=torch.int32, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        assert g.changes_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), cap=cap, peek=True) == ht
        got = [x.cpu().numpy().view(np.uint32) for x in d]
        assert np.array_equal(got[0][:ht], hr) and np.array_equal(got[1][:ht], ho) and np.array_equal(got[2][:ht], hw)
        assert (got[0][ht:] == NONE).all()                  # nothing past the listing
        half = ht // 2
        assert g.changes_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), cap=half) == ht
        assert g.changes_dev(cap=0) == ht - half             # the _dev form's counts only
        r2, o2, w2, t2 = g.changes()
        assert t2 == ht - half and np.array_equal(r2, hr[half:]) and np.array_equal(o2, ho[half:])
        # reset: the next listing is complete again
        g.changes_reset()
        A = g.get_assign()
        r3, o3, w3, t3 = g.changes()
        assert np.array_equal(r3, np.flatnonzero(A != NONE)) and (o3 == NONE).all()
        # argument checks: nothing is listed or advanced
        buf = np.empty((3, 8), np.uint32)
        for kw in (dict(out_rows=buf[0], cap=8), dict(out_rows=buf[0], out_old=buf[1], cap=8), dict(cap=8)):
            assert g.changes_raw(0, **kw)[0] == gp.EINVAL
        assert g.changes_raw(2, buf[0], buf[1], buf[2], 8)[0] == gp.EINVAL
        assert g.changes(cap=0)[3] == 0
    finally:
        g.close()


@pytest.mark.gpu
def test_listing_reflects_ticks_still_in_flight(gp):
    n = 1 << 20
    cfg = synth.config("c3", n_override=n)
    m = cfg["m"]
    g = gp.GpuPlacement(n, m)
    try:
        g.set_nodes(cfg["cap"], cfg["alive"])
        g.set_objects(n, cfg["load"], cfg["aff"])
        g.tick()
        A0 = g.get_assign()
        g.changes()                                          # consume the first listing
        for t in range(4):
            g.set_alive_all(synth.churn_mask(m, t + 1))
            g.tick_async()
        r, o, w, total = g.changes()                         # no tick_wait in between
        A1 = g.get_assign()
        g.tick_wait()
        want = np.flatnonzero(A1 != A0).astype(np.uint32)
        assert total == len(want) > 0
        assert np.array_equal(r, want) and np.array_equal(o, A0[want]) and np.array_equal(w, A1[want])
    finally:
        g.close()


@pytest.mark.gpu
def test_consuming_call_between_quiet_ticks_keeps_them_chained(gp):
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
        g.changes()
        for _ in range(3):                                   # quiet from here on
            g.tick_async()
        st0 = g.tick_wait()
        assert all(s["slow_path"] == 0 for s in st0)
        c0 = g.chained_scans()
        for _ in range(10):
            g.tick_async()
        assert g.changes(cap=0)[3] == 0 and g.changes()[3] == 0   # counts only, then a consuming call: nothing moved
        c1 = g.chained_scans()
        for _ in range(10):
            g.tick_async()
        st = g.tick_wait()
        assert c1 - c0 == 10 and g.chained_scans() - c1 == 10, (c0, c1, g.chained_scans())
        assert all(s == st0[-1] for s in st)
        assert np.array_equal(g.get_assign(), A) and g.changes()[3] == 0
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
        rc, _ = g.changes_raw(0)
        assert rc == gp.EINVAL and "row-sharded" in g._L.rio_gp_last_error(g.handle).decode()
        assert g._L.rio_gp_changes_reset(g.handle) == gp.EINVAL
        assert L.rio_gp_shard_p2p_close(g.handle) == gp.OK
        assert g.changes(cap=0)[3] == 0
    finally:
        g.close()


@pytest.mark.gpu
def test_config3_ten_million_rows_ten_percent_flip(gp):
    cfg = synth.config("c3")
    n, m = cfg["n"], cfg["m"]
    g = gp.GpuPlacement(n, m)
    try:
        g.set_nodes(cfg["cap"], cfg["alive"])
        g.set_objects(n, cfg["load"], cfg["aff"])
        g.set_assign(synth.warm_assign(n, m))
        g.tick()
        A0 = g.get_assign()
        r, o, w, t = g.changes()
        placed = np.flatnonzero(A0 != NONE)
        assert t == len(placed) and np.array_equal(r, placed) and np.array_equal(w, A0[placed])
        g.set_alive_all(synth.churn_mask(m, 1, frac=0.10))
        g.tick()
        A1 = g.get_assign()
        r, o, w, t = g.changes()
        want = np.flatnonzero(A1 != A0)
        assert t == len(want) > n // 20
        assert np.array_equal(r, want) and np.array_equal(o, A0[want]) and np.array_equal(w, A1[want])
        assert g.changes(cap=0)[3] == 0
    finally:
        g.close()


def _chg_tpg(n):
    """Tiles per workgroup of the feed's passes (placement_kernels.hip chg_plan: at most 2 048 workgroups of four waves)."""
    nt = (n + TILE - 1) // TILE
    tpg = (nt + 2047) // 2048
    return max(4, (tpg + 3) // 4 * 4)


@pytest.mark.gpu
def test_ten_million_rows_sparse_and_paged(gp):
    """Above 8 M rows a wave walks more than one tile: tiles without a change are skipped and a page can end on a wave's second
    tile.  A few changes placed on purpose (a wave's second tile only; both of its tiles), paged with caps of 1 to 5; then one node
    flipped (~10^4 changes spread over the table, many tiles empty) paged by 1 000."""
    cfg = synth.config("c3")
    n, m = cfg["n"], cfg["m"]
    tpg = _chg_tpg(n)
    assert tpg > 4
    g = gp.GpuPlacement(n, m)
    try:
        g.set_nodes(cfg["cap"], np.ones(m, np.uint8))
        g.set_objects(n, cfg["load"], cfg["aff"])
        g.set_assign(synth.warm_assign(n, m))
        g.tick()
        f = Fed(g, n)
        f.check()
        assert f.check() == 0
        G = ((n + TILE - 1) // TILE + tpg - 1) // tpg
        rows = []
        for wg in (0, 3, 100, G // 2, G - 2):
            t0 = wg * tpg
            rows += [(t0 + 4) * TILE + 5, (t0 + 4) * TILE + 700]                          # wave 0: its second tile only
            rows += [(t0 + 1) * TILE + 9, (t0 + 1) * TILE + 10, (t0 + 5) * TILE + 3, (t0 + 5) * TILE + 1000]  # wave 1: both
            rows += [(t0 + 6) * TILE + 511]                                                # wave 2: its second tile only
        idx = np.array(sorted(r for r in rows if r < n), np.uint32)
        A = g.get_assign()
        g.update_batch(idx, ((A[idx].astype(np.int64) + 1) % m).astype(np.uint32))
        for cap in (1, 2, 3, 5, 4, 1, 3, 5, 5, 2, 3, 5, 5, 5):
            f.check(cap=cap)
        while f.check(cap=5):
            pass
        assert f.check() == 0
        alive = np.ones(m, np.uint8)
        alive[17] = 0
        g.set_alive_all(alive)
        g.tick()
        assert f.check(cap=0) > 5000
        pages = 0
        while f.check(cap=1000):
            pages += 1
        assert pages >= 5 and f.check() == 0
    finally:
        g.close()


@pytest.mark.gpu
def test_string_layer_mirror_and_sqlite_bridge(gp, tmp_path):
    import snapshot
    rng = random.Random(4)
    op = gp.GpuObjectPlacement(max_objects=48, max_nodes=8)
    try:
        addrs = ["g%d:1" % k for k in range(5)]
        for a in addrs[:4]:
            op.set_member(a)
        keys = [("T%d" % (i % 3), "o%d" % i) for i in range(70)] + [("N\0", "x\0y")]
        path = str(tmp_path / "mirror.db")
        full, ent = op.changes()
        assert full and ent == []
        mirror = {}
        for it in range(300):
            k = rng.randrange(7)
            ty, oid = rng.choice(keys)
            try:
                if k <= 2:
                    op.update(ty, oid, rng.choice(addrs))
                elif k == 3:
                    op.remove(ty, oid)
                elif k == 4:
                    op.clean_server(rng.choice(addrs))
                elif k == 5:
                    op.get_or_create_placement(ty, oid, rng.choice(addrs))
                else:
                    op.set_member(rng.choice(addrs), rng.random() < 0.7)
            except gp.ObjectPlacementError as e:     # every row held by a live object: the call changed nothing
                assert e.rc == gp.EINVAL
            if it % 10 == 9:
                full, ent = op.changes()
                mirror = spec.apply(mirror, full, ent)
                assert spec.as_set(mirror) == set(op.snapshot()), it
        # the write-behind bridge end to end (after a reset: a full rewrite first)
        op.changes_reset()
        assert snapshot.sync_sqlite(op, path)[2] is True
        for _ in range(40):
            ty, oid = rng.choice(keys)
            try:
                op.update(ty, oid, rng.choice(addrs))
            except gp.ObjectPlacementError:
                pass
        assert snapshot.sync_sqlite(op, path)[2] is False
        fresh = str(tmp_path / "fresh.db")
        snapshot.dump_sqlite(op, fresh, replace=True)
        q = "SELECT struct_name, object_id, server_address FROM object_placement ORDER BY struct_name, object_id"
        a, b = sqlite3.connect(path), sqlite3.connect(fresh)
        assert a.execute(q).fetchall() == b.execute(q).fetchall()
        a.close()
        b.close()
    finally:
        op.close()
