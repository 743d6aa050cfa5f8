"""The hot-object report on the MI355X (rio_gp_top_rows / _dev) against the plain restatement (tests/spec_top.py), bit for bit:
table sizes around the passes' tiles (1 024 rows), workgroups and the 4 096-row listing, one node, few and 1 024 nodes; key
columns that exercise each digit of the radix select (all equal, two values, keys that differ in the low 10, the middle 11 or the
top 11 bits only, 0 and 2^32-1, Zipf); tie groups at the cut across a tile boundary, a workgroup boundary, with row 0 and with
row n-1; min_key of 0, 1, exactly the threshold and above the maximum; every flag combination; hidden rows; the hit column before
any hits call, after hits and after a fold; the device form; after a node removal; ticks in flight; an uncommitted solve; that the
call changes nothing (table, used, hits, seen, the feed, quiet chained ticks); the argument checks and the row-sharded refusal."""
import ctypes as C

import numpy as np
import pytest

import spec_top as spec
import synth

NONE = 0xFFFFFFFF
TILE = 1024          # kChgTile
CAPS = [0, 1, 2, 63, 64, 65, 4095, 4096]
KINDS = ["equal", "two", "low", "mid", "top", "ends", "zipf"]


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


def keys_of(rng, n, kind):
    k = max(n, 1)
    if kind == "equal":
        K = np.full(k, 7, np.uint32)
    elif kind == "two":
        K = rng.choice(np.array([3, 0x80000001], np.uint32), k)
    elif kind == "low":          # only the low 10 bits differ
        K = (0x12345400 + rng.integers(0, 1024, k)).astype(np.uint32)
    elif kind == "mid":          # only the middle 11 bits differ
        K = (0x40000155 + (rng.integers(0, 2048, k) << 10)).astype(np.uint32)
    elif kind == "top":          # only the top 11 bits differ
        K = ((rng.integers(0, 2048, k) << 21) + 0x1ABCDE).astype(np.uint32)
    elif kind == "ends":
        K = rng.choice(np.array([0, 1, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32), k)
    else:
        K = np.minimum(rng.zipf(1.3, k), 0xFFFFFFFF).astype(np.uint32)
    return K[:n]


def assign_of(rng, n, m):
    A = rng.integers(0, m, max(n, 1)).astype(np.uint32)
    A[rng.random(len(A)) < 0.3] = NONE
    return A[:n]


def make(gp, n, m, load, A, extra=0, max_nodes=None):
    g = gp.GpuPlacement(n + extra + 1, max_nodes or m)
    g.set_nodes(None, np.ones(m, np.uint8))
    g.set_objects(n, load, np.zeros(n, np.uint32))
    if n:
        g.set_assign(A)
    return g


def check(g, A, load, H, n, flags=0, node=0, min_key=0, cap=4096):
    """one rio_gp_top_rows call against the restatement; returns the restatement's result"""
    want = spec.top_rows(A, load, H, n, flags, node, min_key, cap)
    rows, keys, nodes, nc, ks = g.top_rows(cap, by_hits=bool(flags & 1), placed=bool(flags & 2),
                                           node=node if flags & 4 else None, min_key=min_key)
    assert (nc, ks) == want[3:], (flags, node, min_key, cap, nc, ks, want[3:])
    assert np.array_equal(rows, want[0]) and np.array_equal(keys, want[1]) and np.array_equal(nodes, want[2]), (flags, node, min_key, cap)
    return want


SIZES = [0, 1, 255, 256, 257, 1023, 1024, 1025, 4097, (1 << 18) + 3, 1_000_003]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_every_size_key_column_and_cap_matches_the_spec(gp, n):
    m = 5
    rng = np.random.default_rng(n)
    A = assign_of(rng, n, m)
    big = n > 100_000
    g = make(gp, n, m, keys_of(rng, n, "equal"), A)
    try:
        for kind in (["equal", "low", "zipf", "ends"] if big else KINDS):
            load = keys_of(rng, n, kind)
            g.set_objects(n, load, np.zeros(n, np.uint32))
            if n:
                g.set_assign(A)
            for cap in ([0, 65, 4096] if big else CAPS):
                check(g, A, load, None, n, 0, 0, 0, cap)
            check(g, A, load, None, n, spec.PLACED, 0, 1, 4095 if big else 64)
            check(g, A, load, None, n, spec.PLACED | spec.ON_NODE, 3, 0, 4096 if big else 2)
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 5, 1024])
def test_every_flag_combination_and_min_key(gp, m):
    n = 3 * TILE + 77
    rng = np.random.default_rng(m)
    A = assign_of(rng, n, m)
    load = np.minimum(keys_of(rng, n, "zipf"), 1 << 30)
    H = rng.integers(0, 50, n).astype(np.uint32)
    g = make(gp, n, m, load, A)
    try:
        g.hits_merge(H)
        for flags in range(8):
            for node in sorted({0, m - 1, m // 2}):
                for cap in (0, 1, 64, 4096):
                    w = check(g, A, load, H, n, flags, node, 0, cap)
                check(g, A, load, H, n, flags, node, 1, 100)
                if len(w[1]) > 10:
                    T = int(w[1][10])
                    check(g, A, load, H, n, flags, node, T, 11)        # min_key exactly the threshold of an 11-row listing
                    check(g, A, load, H, n, flags, node, T + 1, 11)
                top = int((H if flags & 1 else load).max())
                assert check(g, A, load, H, n, flags, node, top + 1, 64)[3] == 0      # above the maximum: nothing listed
    finally:
        g.close()


@pytest.mark.gpu
def test_the_tie_group_at_the_cut_goes_to_the_lowest_rows(gp):
    n, m = 9000, 4                                  # tiles of 1 024 rows, workgroups of four tiles: rows 4 095 / 4 096
    rng = np.random.default_rng(3)
    A = assign_of(rng, n, m)
    g = make(gp, n, m, np.ones(n, np.uint32), A)
    try:
        heavy = np.array([17, 2000, 4100, 8990, 5, 7000], np.int64)
        for ties in ([1020, 1021, 1023, 1024, 1025, 1030],         # across a tile boundary
                     [4090, 4095, 4096, 4097, 8000],               # across a workgroup boundary
                     [0, 1, 2, 1023, 1024, 4096],                  # with row 0
                     [n - 3, n - 2, n - 1],                        # with row n-1
                     [0, n - 1]):
            load = np.ones(n, np.uint32)
            load[heavy] = 1000 + np.arange(len(heavy), dtype=np.uint32)
            load[np.array(ties)] = 50
            g.set_objects(n, load, np.zeros(n, np.uint32))
            g.set_assign(A)
            taken = set(ties) | set(heavy.tolist())
            rest = [r for r in range(n) if r not in taken]
            for t in range(0, len(ties) + 2):       # the cut before, inside, at the end of and behind the tie group
                w = check(g, A, load, None, n, 0, 0, 0, len(heavy) + t)
                assert w[0][len(heavy):].tolist() == (ties + rest)[:t]
                check(g, A, load, None, n, 0, 0, 50, len(heavy) + t)
        # a table of equal loads: n ties, the lowest rows are listed
        load = np.full(n, 9, np.uint32)
        g.set_objects(n, load, np.zeros(n, np.uint32))
        g.set_assign(A)
        for cap in (1, 1024, 1025, 4096):
            assert check(g, A, load, None, n, 0, 0, 0, cap)[0].tolist() == list(range(cap))
        w = check(g, A, load, None, n, spec.PLACED, 0, 0, 4096)
        assert w[0].tolist() == np.flatnonzero(A != NONE)[:4096].tolist()
    finally:
        g.close()


@pytest.mark.gpu
def test_hidden_rows_with_the_largest_keys_are_not_listed(gp):
    n, hidden, m = 2 * TILE - 5, 40, 3
    rng = np.random.default_rng(5)
    load = np.minimum(keys_of(rng, n + hidden, "zipf"), 1 << 30)
    load[n:] = 0xFFFFFFF0
    A = assign_of(rng, n + hidden, m)
    g = make(gp, n + hidden, m, load, A)
    try:
        assert check(g, A, load, None, n + hidden, 0, 0, 0, 64)[0][:hidden].min() >= n
        g.set_num_objects(n)
        w = check(g, A[:n], load[:n], None, n, 0, 0, 0, 4096)
        assert w[3] == n and w[0].max() < n
        check(g, A[:n], load[:n], None, n, spec.PLACED, 0, 0, 10)
    finally:
        g.close()


@pytest.mark.gpu
def test_by_hits_before_any_hits_call_after_hits_and_after_a_fold(gp):
    n, m = 5000, 6
    rng = np.random.default_rng(8)
    A = assign_of(rng, n, m)
    load = keys_of(rng, n, "zipf")
    g = make(gp, n, m, load, A)
    try:
        rows, keys, nodes, nc, ks = g.top_rows(100, by_hits=True)          # no hit column yet: zeros, the lowest rows first
        assert rows.tolist() == list(range(100)) and not keys.any() and (nc, ks) == (n, 0)
        assert np.array_equal(nodes, A[:100])
        assert g.top_rows(100, by_hits=True, min_key=1)[3] == 0
        idx = (rng.zipf(1.2, 40_000) % n).astype(np.uint32)
        g.hits_add(idx)
        H = np.bincount(idx, minlength=n).astype(np.uint32)
        assert np.array_equal(g.get_hits(), H)
        for flags in (1, 3, 7):
            check(g, A, load, H, n, flags, 2, 0, 64)
            check(g, A, load, H, n, flags, 2, 1, 4096)
        g.load_fold(0, 3, 1, 1000)
        load2 = g.get_objects()[0]
        assert not np.array_equal(load2, load)
        check(g, A, load2, np.zeros(n, np.uint32), n, 1, 0, 0, 10)
        w = check(g, A, load2, None, n, 0, 0, 0, 10)
        assert w[1][0] == min(1000, max(1, 3 * int(H.max())))
    finally:
        g.close()


@pytest.mark.gpu
def test_the_device_form_equals_the_host_form(gp):
    import torch
    n, m = 70_001, 9
    rng = np.random.default_rng(11)
    A = assign_of(rng, n, m)
    load = keys_of(rng, n, "zipf")
    g = make(gp, n, m, load, A)
    try:
        for flags, cap in ((0, 4096), (2, 65), (6, 1), (0, 0)):
            d = torch.full((3, max(cap, 1)), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            if cap:
                nc, ks = g.top_rows_dev(flags, 4, 1, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), cap)
            else:
                nc, ks = g.top_rows_dev(flags, 4, 1, None, None, None, 0)
            rows, keys, nodes, wnc, wks = g.top_rows(cap, placed=bool(flags & 2), node=4 if flags & 4 else None, min_key=1)
            assert (nc, ks) == (wnc, wks)
            out = d.cpu().numpy().view(np.uint32)
            L = len(rows)
            assert np.array_equal(out[0, :L], rows) and np.array_equal(out[1, :L], keys) and np.array_equal(out[2, :L], nodes)
            assert (out[:, L:] == NONE).all()                                 # entries from L on are not written
        d = torch.full((2, 8), -1, dtype=torch.int32, device="cuda")          # without d_node
        torch.cuda.synchronize()
        g.top_rows_dev(0, 0, 0, d[0].data_ptr(), d[1].data_ptr(), None, 8)
        w = spec.top_rows(A, load, None, n, 0, 0, 0, 8)
        assert np.array_equal(d.cpu().numpy().view(np.uint32)[0], w[0])
        assert g.top_rows(8, want_node=False)[2] is None
    finally:
        g.close()


@pytest.mark.gpu
def test_after_a_node_removal_has_left_m_below_max_nodes(gp):
    n, m = 3000, 8
    rng = np.random.default_rng(13)
    A = assign_of(rng, n, m)
    load = keys_of(rng, n, "zipf")
    g = make(gp, n, m, load, A)
    try:
        g.remap_nodes(np.array([0, NONE, 1, 2, NONE, 3, 4, NONE], np.uint32))
        assert g.num_nodes == 5
        A2 = g.get_assign()
        for node in range(5):
            check(g, A2, load, None, n, spec.ON_NODE | spec.PLACED, node, 0, 50)
        check(g, A2, load, None, n, spec.PLACED, 0, 0, 4096)
        assert g.top_rows_raw(spec.ON_NODE, node=5)[0] == gp.EINVAL         # m is 5 now, max_nodes 8
        assert g.top_rows_raw(0, node=5)[0] == gp.OK                        # (ignored without the flag)
    finally:
        g.close()


@pytest.mark.gpu
def test_argument_checks(gp):
    n, m = 100, 4
    rng = np.random.default_rng(1)
    g = make(gp, n, m, keys_of(rng, n, "zipf"), assign_of(rng, n, m))
    try:
        buf = np.empty((3, 4097), np.uint32)
        err = lambda: g._L.rio_gp_last_error(g.handle).decode()
        assert g.top_rows_raw(0, out_rows=buf[0], out_key=buf[1], cap=4097)[0] == gp.EINVAL and "RIO_GP_TOP_MAX" in err()
        assert g.top_rows_raw(0, out_rows=buf[0], out_key=buf[1], cap=4096) == (gp.OK, n)
        assert g.top_rows_raw(8)[0] == gp.EINVAL and "flags" in err()
        assert g.top_rows_raw(4, node=m)[0] == gp.EINVAL
        assert g.top_rows_raw(4, node=m - 1)[0] == gp.OK
        assert g.top_rows_raw(0, want_n=False)[0] == gp.EINVAL
        assert g.top_rows_raw(0, out_rows=buf[0], cap=1)[0] == gp.EINVAL       # rows without keys
        assert g.top_rows_raw(0, out_key=buf[1], cap=1)[0] == gp.EINVAL
        assert g.top_rows_raw(0, cap=1)[0] == gp.EINVAL                        # cap without a listing
        assert g.top_rows_raw(0, out_node=buf[2])[0] == gp.EINVAL              # nodes without a listing
        assert g.top_rows_raw(0) == (gp.OK, n)
    finally:
        g.close()


def _state(g):
    cap, alive, used = g.get_nodes()
    load, aff = g.get_objects()
    return [g.get_assign(), load, aff, used, g.get_hits(), g.get_seen(), np.array([g.changes(cap=0, peek=True)[3]])]


@pytest.mark.gpu
def test_the_call_changes_nothing(gp):
    n = 50_000
    cfg = synth.config("c3", n_override=n)
    m = cfg["m"]
    g = gp.GpuPlacement(n, m)
    try:
        g.set_nodes(cfg["cap"], cfg["alive"])
        g.set_objects(n, cfg["load"], cfg["aff"])
        g.tick()
        g.changes(cap=1000)                                   # the feed's checkpoint: 1 000 rows known, the rest still to list
        g.hits_add(np.arange(0, n, 7, dtype=np.uint32))
        g.touch(np.arange(0, n, 5, dtype=np.uint32), 4)
        g.set_alive(3, 0)
        g.tick()
        before = _state(g)
        for flags in range(8):
            for cap in (0, 10, 4096):
                g.top_rows(cap, by_hits=bool(flags & 1), placed=bool(flags & 2), node=1 if flags & 4 else None)
        after = _state(g)
        for b, a in zip(before, after):
            assert np.array_equal(b, a)
        assert g.changes(cap=0, peek=True)[3] > 0
    finally:
        g.close()


@pytest.mark.gpu
def test_the_call_orders_itself_behind_ticks_in_flight(gp):
    n = 1 << 18
    cfg = synth.config("c3", n_override=n)
    m = cfg["m"]
    g, t = gp.GpuPlacement(n, m), gp.GpuPlacement(n, m)
    try:
        for h in (g, t):
            h.set_nodes(cfg["cap"], cfg["alive"])
            h.set_objects(n, cfg["load"], cfg["aff"])
            h.tick()
        for k in range(4):
            mask = synth.churn_mask(m, k + 1)
            g.set_alive_all(mask)
            g.tick_async()
            t.set_alive_all(mask)
            t.tick()
        node = int(np.flatnonzero(mask)[0])
        got = g.top_rows(300, placed=True, node=node)          # no tick_wait in between
        want = spec.top_rows(t.get_assign(), cfg["load"], None, n, spec.PLACED | spec.ON_NODE, node, 0, 300)
        assert got[3:] == want[3:] and want[3] > 0
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3]))
        assert len(g.tick_wait()) == 4
        assert np.array_equal(g.get_assign(), t.get_assign())
    finally:
        g.close()
        t.close()


@pytest.mark.gpu
def test_an_uncommitted_solve_stays_committable(gp):
    n, m = 40_000, 16
    rng = np.random.default_rng(21)
    load = rng.integers(1, 9, n).astype(np.uint32)
    g = gp.GpuPlacement(n, m)
    try:
        g.set_nodes(np.full(m, int(load.sum()) * 2 // m, np.uint64), np.ones(m, np.uint8))
        g.set_objects(n, load, rng.integers(0, m, n).astype(np.uint32))
        g.tick()
        A = g.get_assign()
        g.set_alive(1, 0)
        g.solve()
        solved = g.get_solved()
        assert not np.array_equal(solved, A)
        check(g, A, load, None, n, spec.PLACED | spec.ON_NODE, 1, 0, 4096)   # the committed column, not the solved one
        check(g, A, load, None, n, 1, 0, 0, 5)
        assert g.top_rows_raw(8)[0] == gp.EINVAL
        assert np.array_equal(g.get_solved(), solved)
        g.commit()
        assert np.array_equal(g.get_assign(), solved)
        check(g, solved, load, None, n, spec.PLACED | spec.ON_NODE, 1, 0, 4096)
    finally:
        g.close()


@pytest.mark.gpu
def test_quiet_ticks_stay_chained_around_the_call(gp):
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
        for _ in range(3):                                   # quiet from here on
            g.tick_async()
        st0 = g.tick_wait()
        assert all(s["slow_path"] == 0 for s in st0)
        c0 = g.chained_scans()
        for _ in range(10):
            g.tick_async()
        got = g.top_rows(4096, placed=True)                  # a listing, a count, a filtered listing by hits
        want = spec.top_rows(A, cfg["load"], None, n, spec.PLACED, 0, 0, 4096)
        assert got[3:] == want[3:] and all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3]))
        assert g.top_rows(0)[3] == n
        g.top_rows(16, by_hits=True, node=2)
        c1 = g.chained_scans()
        for _ in range(10):
            g.tick_async()
        st = g.tick_wait()
        c2 = g.chained_scans()
        assert c1 - c0 == 10 and c2 - c1 == 10, (c0, c1, c2)
        assert all(s == st0[-1] for s in st) and np.array_equal(g.get_assign(), A)
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
        assert g.top_rows_raw(0)[0] == gp.EINVAL and "row-sharded" in err()
        with pytest.raises(gp.ObjectPlacementError) as e:
            g.top_rows(4)
        assert e.value.rc == gp.EINVAL and "row-sharded" in e.value.text
        assert L.rio_gp_shard_p2p_close(g.handle) == gp.OK
        assert g.top_rows(4)[3] == 4096
    finally:
        g.close()
