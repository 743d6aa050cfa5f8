"""Reverse placement index on the MI355X: rio_gp_rows_on_nodes (+ _dev, counts only) against numpy over the column
rio_gp_get_assign returns at the same point, and rio_op_objects_on_server against pyoracle.LocalObjectPlacement."""
import numpy as np
import pytest

import node_index_driver as drv
import rio_gp
import synth

pytestmark = pytest.mark.gpu
NONE = rio_gp.NONE


def want_index(a, m, nodes=None):
    """numpy: node j's rows ascending, nodes in order; rows holding NONE or a node >= m are listed nowhere."""
    a = np.asarray(a, np.uint32)
    sel = np.ones(m, bool) if nodes is None else np.isin(np.arange(m), np.asarray(list(nodes), np.int64))
    keep = np.flatnonzero((a < m) & sel[np.minimum(a, max(m - 1, 0))]) if m else np.zeros(0, np.int64)
    rows = keep[np.argsort(a[keep], kind="stable")].astype(np.uint32)
    off = np.zeros(m + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(a[keep], minlength=m))
    return off, rows


def check(g, nodes=None):
    a = g.get_assign()
    off, rows = g.rows_on_nodes(nodes)
    woff, wrows = want_index(a, g.num_nodes, nodes)
    assert np.array_equal(off, woff)
    assert np.array_equal(rows, wrows)
    return off, rows


def node_sets(m, rng):
    return [None, rng.choice(m, max(1, m // 3), replace=False).tolist(), [int(rng.integers(m))], [],
            [0, m + 5, m + 64, 8191 + 70] if m < 8000 else [m - 1, m + 3]]


@pytest.mark.parametrize("m", [1, 256, 8192])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097, 1023, 1024, 1025, 6 * 1024 + 1, 300_001])
def test_index_matches_numpy(n, m):
    rng = np.random.default_rng(n * 31 + m)
    g = rio_gp.GpuPlacement(max(n, 1), m)
    g.set_nodes(m=m)
    g.set_objects(n)
    a = rng.integers(0, m, n).astype(np.uint32)
    a[rng.random(n) < 0.2] = NONE
    g.set_assign(a)
    for nodes in node_sets(m, rng):
        check(g, nodes)
    if m > 1:   # rows >= m after a shrinking set_nodes
        g.set_nodes(m=max(1, m // 2))
        for nodes in node_sets(max(1, m // 2), rng):
            check(g, nodes)
    g.close()


@pytest.mark.parametrize("state", ["empty", "one_node"])
def test_nothing_placed_and_everything_on_one_node(state):
    n, m = 200_000, 1024
    g = rio_gp.GpuPlacement(n, m)
    g.set_nodes(m=m)
    g.set_objects(n)
    if state == "one_node":
        g.set_assign(np.full(n, 17, np.uint32))
    for nodes in (None, [17], [3], [17, 18]):
        off, rows = check(g, nodes)
        if state == "empty":
            assert len(rows) == 0 and not off.any()
    g.close()


def test_states_after_crud_ticks_and_requests(oracle):
    cfg = synth.config("c3", n_override=400_000)
    n, m = cfg["n"], cfg["m"]
    cap = cfg["cap"].copy()
    cap[::7] //= 2
    alive = cfg["alive"].copy()
    rng = np.random.default_rng(5)
    g = rio_gp.GpuPlacement(n, m)
    g.set_nodes(cap, alive)
    g.set_objects(n, cfg["load"], cfg["aff"])
    sets = node_sets(m, rng)
    for nodes in sets:
        check(g, nodes)                       # nothing placed
    ost = g.tick()
    want, used, wst = oracle.tick(cfg["cur"], cfg["load"], cfg["aff"], cap, alive)
    assert ost == wst and np.array_equal(g.get_assign(), want)
    for nodes in sets:
        check(g, nodes)                       # a committed tick
    g.clean_server(int(want[0]))
    check(g); check(g, [int(want[0])])        # clean_server
    alive[3::17] = 0
    g.set_alive_all(alive)
    g.tick_async(); g.tick_async()
    g.tick_wait()
    for nodes in sets:
        check(g, nodes)                       # tick_async + tick_wait
    idx = rng.choice(n, 5000, replace=False).astype(np.uint32)
    live = np.flatnonzero(alive)
    g.place_pending(idx, live[rng.integers(0, len(live), 5000)].astype(np.uint32))
    check(g); check(g, sets[1])               # place_pending
    idx = rng.choice(n, 50_000, replace=False).astype(np.uint32)
    node = rng.integers(0, m, 50_000).astype(np.uint32)
    node[::5] = NONE
    g.update_batch(idx, node)
    g.remove_batch(rng.choice(n, 20_000, replace=False).astype(np.uint32))
    for nodes in sets:
        check(g, nodes)                       # update_batch / remove_batch
    g.close()


@pytest.mark.parametrize("name,n", [("c3", None), ("c3", 40_000_000)])
def test_full_size_tables(name, n):
    """config 3 at full size (10 M x 1 024, Zipf: one node holds a large share) and a table beyond the Infinity Cache."""
    cfg = synth.config(name, n_override=n)
    g = rio_gp.GpuPlacement(cfg["n"], cfg["m"])
    g.set_nodes(cfg["cap"], cfg["alive"])
    g.set_objects(cfg["n"], cfg["load"], cfg["aff"])
    g.tick()
    a = g.get_assign()
    big = int(np.bincount(a[a < cfg["m"]], minlength=cfg["m"]).argmax())
    for nodes in (None, [big], [big, 1, 2, 900]):
        check(g, nodes)
    g.close()


def test_protocol_erange_counts_dev_and_determinism():
    import torch
    n, m = 100_000, 256
    rng = np.random.default_rng(3)
    g = rio_gp.GpuPlacement(n, m)
    g.set_nodes(m=m)
    g.set_objects(n)
    a = rng.integers(0, m, n).astype(np.uint32)
    a[::9] = NONE
    g.set_assign(a)
    woff, wrows = want_index(a, m)
    # the ERANGE sizing round: offsets and the count filled, the rows untouched
    small = np.full(len(wrows) - 1, 0xDEADBEEF, np.uint32)
    rc, off, nr = g.rows_on_nodes_try(None, small)
    assert rc == rio_gp.ERANGE and nr == len(wrows) and np.array_equal(off, woff)
    assert (small == 0xDEADBEEF).all()
    exact = np.full(len(wrows), 0xDEADBEEF, np.uint32)
    rc, off, nr = g.rows_on_nodes_try(None, exact)
    assert rc == rio_gp.OK and np.array_equal(exact, wrows)
    # counts only
    assert np.array_equal(g.count_on_nodes(), woff)
    assert np.array_equal(g.count_on_nodes([5, 7]), want_index(a, m, [5, 7])[0])
    # the _dev form into torch buffers
    d_off = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    d_rows = torch.full((len(wrows) + 8,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc, nr = g.rows_on_nodes_dev(d_off.data_ptr(), d_rows.data_ptr(), len(wrows) + 8)
    assert rc == rio_gp.OK and nr == len(wrows)
    assert np.array_equal(d_off.cpu().numpy().view(np.uint64), woff)
    got = d_rows.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:nr], wrows) and (got[nr:] == 0xFFFFFFFF).all()
    d_rows.fill_(-1)
    torch.cuda.synchronize()
    rc, nr = g.rows_on_nodes_dev(d_off.data_ptr(), d_rows.data_ptr(), len(wrows) - 1)   # too small: untouched
    assert rc == rio_gp.ERANGE and nr == len(wrows) and (d_rows.cpu().numpy() == -1).all()
    rc, nr = g.rows_on_nodes_dev(d_off.data_ptr(), 0, 0, nodes=[4])                      # counts only
    assert rc == rio_gp.OK and np.array_equal(d_off.cpu().numpy().view(np.uint64), want_index(a, m, [4])[0])
    # two calls: identical bytes
    o1, r1 = g.rows_on_nodes()
    o2, r2 = g.rows_on_nodes()
    assert o1.tobytes() == o2.tobytes() and r1.tobytes() == r2.tobytes()
    g.close()


def test_read_only(oracle):
    cfg = synth.config("c3", n_override=300_000)
    n, m = cfg["n"], cfg["m"]
    g = rio_gp.GpuPlacement(n, m)
    g.set_nodes(cfg["cap"], cfg["alive"])
    g.set_objects(n, cfg["load"], cfg["aff"])
    g.tick()
    a0, nodes0 = g.get_assign(), g.get_nodes()
    g.rows_on_nodes(); g.count_on_nodes([1]); g.rows_on_nodes([2, 3])
    assert np.array_equal(g.get_assign(), a0)
    assert all(np.array_equal(x, y) for x, y in zip(g.get_nodes(), nodes0))
    st = g.tick()
    g2 = rio_gp.GpuPlacement(n, m)   # the same history without the index calls
    g2.set_nodes(cfg["cap"], cfg["alive"]); g2.set_objects(n, cfg["load"], cfg["aff"]); g2.tick()
    assert st == g2.tick() and np.array_equal(g.get_assign(), g2.get_assign())
    g.close(); g2.close()


def test_quiet_ticks_still_chain_after_the_call():
    n, m = 1 << 18, 256
    cfg = synth.config("c2", n_override=n)
    g = rio_gp.LabPlacement(n, m)
    g.set_nodes(m=m)
    g.set_objects(n, cfg["load"], cfg["aff"])
    g.tick()
    for _ in range(40):
        g.tick_async()
    g.tick_wait()
    c0 = g.chained_scans()
    assert c0 > 0
    a = g.get_assign()
    check(g)
    for _ in range(40):
        g.tick_async()
    got = g.tick_wait()
    assert all(s["slow_path"] == 0 and s["kept"] == s["n_objects"] for s in got)
    assert g.chained_scans() >= c0 + 30
    assert np.array_equal(g.get_assign(), a)
    check(g)
    g.close()


@pytest.mark.parametrize("m,tile,geom", [(8192, 0, (2, 4)), (256, 0, (2, 8)), (8192, 70_000, (4, 4)), (256, 70_000, (4, 8)),
                                         (1, 70_000, (4, 8))])
def test_every_geometry(m, tile, geom):
    """u16 / u32 counters (a tile of more than 65 535 rows; forced by the lab knob) x 4 / 8 waves per workgroup (by the slots)."""
    n = 300_000
    rng = np.random.default_rng(m + tile)
    g = rio_gp.LabPlacement(n, m)
    g.set_nodes(m=m)
    g.set_objects(n)
    a = rng.integers(0, m, n).astype(np.uint32)
    a[rng.random(n) < 0.1] = NONE
    g.set_assign(a)
    g.set_node_index(tile)
    T, nt, cb, W = g.node_index_geometry(None)
    assert (cb, W) == geom and nt * T >= n and (tile == 0 or T >= tile)
    check(g)
    if m > 1:
        check(g, rng.choice(m, m // 2, replace=False).tolist())
        check(g, [m - 1])
    g.close()


@pytest.mark.parametrize("shadow", [True, False])
@pytest.mark.parametrize("seed", range(3))
def test_objects_on_server_equals_the_reference(oracle, seed, shadow):
    op = rio_gp.GpuObjectPlacement(max_objects=drv.MAX_OBJECTS, max_nodes=16, flags=0 if shadow else rio_gp.OP_CFG_NO_HOST_SHADOW)
    try:
        drv.run(op, oracle, seed, steps=80)
    finally:
        op.close()
