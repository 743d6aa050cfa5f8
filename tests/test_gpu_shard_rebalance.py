"""Row-sharded rebalance on the MI355X (rio_gp_shard_rebalance_*, ShardedSolver.rebalance): G handles on one device, bit for bit
against the two-tick composition of the oracle (tests/rebalance_ref.py) AND against the single-handle rio_gp_rebalance of the
concatenated table — the column, `used` on every rank, the counters, the moves."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import rebalance_ref as ref
import rio_gp
import synth

pytestmark = pytest.mark.gpu
NONE = rio_gp.NONE
INF = rio_gp.CAP_INF
HERE = os.path.dirname(os.path.abspath(__file__))


def load_table(g, cur, load, aff, cap, alive):
    """Rows holding a node >= m are what a shrinking rio_gp_set_nodes leaves behind: placed on a bigger table first."""
    m = len(cap)
    top = int(cur[cur != NONE].max()) + 1 if (cur != NONE).any() else 0
    g.set_nodes(np.full(max(top, m), INF, np.uint64), np.ones(max(top, m), np.uint8))
    g.set_objects(len(cur), load, aff)
    if len(cur):
        g.set_assign(cur)
    g.set_nodes(cap, alive)


def make_engines(case, bounds, rounds=2, extra_nodes=3):
    import torch
    import sharded
    cur, load, aff, cap, alive = case
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    engines = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        g = rio_gp.GpuPlacement(max(hi - lo, 1), len(cap) + extra_nodes, spill_rounds=rounds)
        load_table(g, cur[lo:hi], load[lo:hi], aff[lo:hi], cap, alive)
        engines.append(sharded.HipShardEngine(g, 0, stream))
    return engines


def column(engines):
    return np.concatenate([e.g.get_assign() if e.g.num_objects else np.zeros(0, np.uint32) for e in engines])


def bounds_for(n, G, kind, rng):
    if kind == "balanced":
        return [(r * n) // G for r in range(G + 1)]
    if kind == "empty":
        b = [0] * (G + 1)
        for r in range(G // 2 + 1, G + 1):
            b[r] = n
        return b
    cuts = sorted(int(c) for c in rng.integers(0, n + 1, G - 1))
    if G > 2:
        cuts[1] = cuts[0]
    return [0] + cuts + [n]


def check(sol, engines, single, cur, load, aff, cap, alive, target=None, max_moves=None, rounds=2, eff_rounds=None,
          list_moves=True):
    """One sharded rebalance against the reference and against the single handle (which is advanced too)."""
    st, rows, frm, to = sol.rebalance(target=target, max_moves=max_moves, rounds=rounds, list_moves=list_moves)
    nxt, used, wst, wrows, wfrom, wto = ref.rebalance(cur, load, aff, cap, alive, target, max_moves, eff_rounds or rounds)
    assert st == wst
    if list_moves:
        assert np.array_equal(rows, wrows) and np.array_equal(frm, wfrom) and np.array_equal(to, wto)
    else:   # counters only: the same column and `used`, nothing listed
        assert len(rows) == 0 and len(frm) == 0 and len(to) == 0
        rows, frm, to = wrows, wfrom, wto
    assert np.array_equal(column(engines), nxt)
    for e in engines:
        assert np.array_equal(e.g.get_nodes()[2], used)
    if single is not None:
        sst, srows, sfrom, sto = single.rebalance(target, max_moves, rounds)
        assert st == sst
        assert np.array_equal(rows, srows) and np.array_equal(frm, sfrom) and np.array_equal(to, sto)
        assert np.array_equal(column(engines), single.get_assign() if single.num_objects else np.zeros(0, np.uint32))
        assert np.array_equal(single.get_nodes()[2], used)
    return nxt


def close(engines, single=None):
    for e in engines:
        e.g.close()
    if single is not None:
        single.close()


@pytest.mark.parametrize("G", [1, 2, 3, 8])
@pytest.mark.parametrize("kind", ["tight", "zero", "inf"])
@pytest.mark.parametrize("shape,n,m", [("balanced", 50_001, 256), ("ragged", 9_000, 64), ("empty", 4097, 1024)])
def test_sharded_equals_reference_and_single_handle(oracle, G, kind, shape, n, m):
    import sharded
    rng = np.random.default_rng(G * 100 + len(kind) * 10 + len(shape))
    cur, load, aff, alive, T = ref.random_table(rng, n, m, kind, max_load=int(rng.choice([3, 50, 4000])))
    cap = np.full(m, INF, np.uint64)
    b = bounds_for(n, G, shape, rng)
    engines = make_engines((cur, load, aff, cap, alive), b)
    single = rio_gp.GpuPlacement(max(n, 1), m + 3)
    load_table(single, cur, load, aff, cap, alive)
    sol = sharded.ShardedSolver(engines, sharded.LocalExchange(G))
    col = cur
    T2 = T if kind != "tight" else (T * np.uint64(9) // np.uint64(10)).astype(np.uint64)
    for k, (target, max_moves, rounds) in enumerate(((T, 0, 1), (T, 1, 2), (T, max(n // 50, 2), 4), (T, None, 1),
                                                     (T2, None, 8), (np.zeros(m, np.uint64), None, 2))):
        col = check(sol, engines, single, col, load, aff, cap, alive, target, max_moves, rounds, list_moves=k not in (2, 4))
    # the capacities as the target, the handle's own rounds
    cap2 = np.where(T2 == np.uint64(INF), T2, T2 // np.uint64(2) + np.uint64(1)).astype(np.uint64)
    for g in [e.g for e in engines] + [single]:
        g.set_nodes(cap2, alive)
    check(sol, engines, single, col, load, aff, cap2, alive, None, 500, 0, eff_rounds=2)
    close(engines, single)


def test_cut_on_rank_zero_zero_load_candidates_behind_it(oracle):
    import sharded
    from test_shard_rebalance_protocol import cut_on_rank0_table
    cur, load, aff, cap, alive, b = cut_on_rank0_table()
    engines = make_engines((cur, load, aff, cap, alive), b)
    single = rio_gp.GpuPlacement(len(cur), len(cap) + 3)
    load_table(single, cur, load, aff, cap, alive)
    sol = sharded.ShardedSolver(engines, sharded.LocalExchange(3))
    st, rows, frm, to = sol.rebalance(max_moves=2)
    assert list(rows) == [2, 6] and st["surplus_rows"] == 5 and st["selected_rows"] == 2
    for e, lo, hi in zip(engines, b[:-1], b[1:]):   # back to the table as it was
        e.g.set_assign(cur[lo:hi])
    check(sol, engines, single, cur, load, aff, cap, alive, None, None, 2)
    assert np.array_equal(single.get_assign()[[2, 6, 8, 10, 13]], np.full(5, 2, np.uint32))
    close(engines, single)


def test_config3_shape_capacity_cut_and_scale_out(oracle):
    """Config-3 shape, 2 M rows over 8 shards: capacities x 0.9, then 64 empty nodes and balanced targets."""
    import sharded
    cfg = synth.config("c3w", n_override=2_000_000)
    n, m = cfg["n"], cfg["m"]
    load, aff, cap, cur = cfg["load"], cfg["aff"], cfg["cap"].copy(), cfg["cur"]
    alive = np.ones(m, np.uint8)
    b = sharded.shard_bounds(n, 8)
    engines = make_engines((cur, load, aff, cap, alive), b, extra_nodes=64)
    single = rio_gp.GpuPlacement(n, m + 64)
    load_table(single, cur, load, aff, cap, alive)
    sol = sharded.ShardedSolver(engines, sharded.LocalExchange(8))
    cap = (cap * np.uint64(9) // np.uint64(10)).astype(np.uint64)
    for g in [e.g for e in engines] + [single]:
        g.set_nodes(cap, alive)
    col = check(sol, engines, single, cur, load, aff, cap, alive)
    cap2 = np.concatenate([cap, np.full(64, int(cap.mean()), np.uint64)])
    alive2 = np.ones(m + 64, np.uint8)
    for g in [e.g for e in engines] + [single]:
        g.set_nodes(cap2, alive2)
    with pytest.raises(ValueError):          # the records grew with the node count: the old buffers are refused, nothing ran
        sol.rebalance()
    engines = [sharded.HipShardEngine(e.g, 0, e.stream) for e in engines]
    sol = sharded.ShardedSolver(engines, sharded.LocalExchange(8))
    used = ref.rebalance(col, load, aff, cap2, alive2, np.full(m + 64, INF, np.uint64), 0, 1)[1]
    T = rio_gp.balanced_targets(cap2, used, alive2, 20)
    col = check(sol, engines, single, col, load, aff, cap2, alive2, T, 10_000)
    check(sol, engines, single, col, load, aff, cap2, alive2, T)
    close(engines, single)


def test_tick_after_a_rebalance_equals_the_oracle(oracle):
    """State hygiene: a sharded solve half way is dropped by the rebalance; sharded ticks after it see the new column."""
    import sharded
    rng = np.random.default_rng(41)
    n, m, G = 60_000, 96, 3
    cur, load, aff, alive, T = ref.random_table(rng, n, m, "tight", big_nodes=False, pinned=False)
    cap = (T.astype(np.float64).clip(0, 1e12) * 1.3).astype(np.uint64)
    cap[T == np.uint64(INF)] = np.uint64(INF)
    b = bounds_for(n, G, "ragged", rng)
    engines = make_engines((cur, load, aff, cap, alive), b)
    sol = sharded.ShardedSolver(engines, sharded.LocalExchange(G))
    sol.solve()                                  # not committed: the rebalance drops it
    col = check(sol, engines, None, cur, load, aff, cap, alive, T, None, 2)
    for k in range(3):
        want, used, ost = oracle.tick(col, load, aff, cap, alive, 2)
        st = sol.tick()
        assert st == ost and np.array_equal(column(engines), want)
        for e in engines:
            assert np.array_equal(e.g.get_nodes()[2], used)
        col = want
        alive = alive.copy()
        alive[k::7] = 0
        for e in engines:
            e.g.set_alive_all(alive)
        col = check(sol, engines, None, col, load, aff, cap, alive, T, 300 * (k + 1), 1 + k)
    close(engines)


def test_invalid_calls_change_nothing(oracle):
    import ctypes as C
    import sharded
    rng = np.random.default_rng(43)
    n, m = 5000, 32
    cur, load, aff, alive, T = ref.random_table(rng, n, m, "tight")
    cap = np.full(m, INF, np.uint64)
    e = make_engines((cur, load, aff, cap, alive), [0, n])[0]
    L, h = sharded._lib(), e.g.handle
    sol = sharded.ShardedSolver([e], sharded.LocalExchange(1))
    x, y, xg = sol.X[0], sol.Y[0], sol.XG[0]
    vp = lambda t: C.c_void_p(t.data_ptr())
    before = (e.g.get_assign(), e.g.get_nodes()[2].copy())
    good, keep = e.g._rebalance_cfg(T, None, 2)
    bad_size = rio_gp.RebalanceCfg(8, 2, INF, None)
    bad_rounds = rio_gp.RebalanceCfg(C.sizeof(rio_gp.RebalanceCfg), 9, INF, None)
    EINVAL = rio_gp.EINVAL
    assert L.rio_gp_shard_rebalance_begin(h, None, 0, 1, 1, INF, vp(x), None) == EINVAL
    assert L.rio_gp_shard_rebalance_begin(h, C.byref(bad_size), 0, 1, 1, INF, vp(x), None) == EINVAL
    assert L.rio_gp_shard_rebalance_begin(h, C.byref(bad_rounds), 0, 1, 1, INF, vp(x), None) == EINVAL
    assert L.rio_gp_shard_rebalance_begin(h, C.byref(good), 1, 1, 1, INF, vp(x), None) == EINVAL      # rank >= n_ranks
    assert L.rio_gp_shard_rebalance_begin(h, C.byref(good), 3, 2, 1, INF, vp(x), None) == EINVAL
    assert L.rio_gp_shard_rebalance_begin(h, C.byref(good), 0, 1, 0, 5, vp(x), None) == EINVAL        # moves_cap, no listing
    # steps out of order
    ov, a, bb = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    st = rio_gp.RebalanceStats()
    assert L.rio_gp_shard_rebalance_cut(h, vp(xg), vp(y), C.byref(ov)) == EINVAL
    assert L.rio_gp_shard_rebalance_select(h, vp(y), vp(y), C.byref(a), C.byref(bb)) == EINVAL
    assert L.rio_gp_shard_rebalance_merge(h, vp(y), C.byref(a), C.byref(bb)) == EINVAL
    assert L.rio_gp_shard_rebalance_fill(h, 0, vp(y)) == EINVAL
    assert L.rio_gp_shard_rebalance_finish(h, C.byref(st), None, None, None, 0, None) == EINVAL
    assert np.array_equal(e.g.get_assign(), before[0]) and np.array_equal(e.g.get_nodes()[2], before[1])
    # ... and in the middle of a run: begin, then anything but cut
    assert L.rio_gp_shard_rebalance_begin(h, C.byref(good), 0, 1, 1, INF, vp(x), None) == 0
    assert L.rio_gp_shard_rebalance_select(h, vp(y), vp(y), C.byref(a), C.byref(bb)) == EINVAL
    assert L.rio_gp_shard_rebalance_fill(h, 0, vp(y)) == EINVAL
    assert L.rio_gp_shard_rebalance_finish(h, C.byref(st), None, None, None, 0, None) == EINVAL
    assert np.array_equal(e.g.get_assign(), before[0])
    # a call that changes an input between two steps ends the protocol: the next step is refused
    assert L.rio_gp_shard_rebalance_begin(h, C.byref(good), 0, 1, 1, INF, vp(x), None) == 0
    e.g.set_alive_all(alive)
    assert L.rio_gp_shard_rebalance_cut(h, vp(x), vp(y), C.byref(ov)) == EINVAL
    assert L.rio_gp_shard_rebalance_begin(h, C.byref(good), 0, 1, 1, INF, vp(x), None) == 0
    e.g.get_nodes()                       # ... and so does one that rebuilds `used`
    assert L.rio_gp_shard_rebalance_cut(h, vp(x), vp(y), C.byref(ov)) == EINVAL
    assert np.array_equal(e.g.get_assign(), before[0])

    def run_to_finish(list_moves):        # world 1: the gathered record is the record
        nr = e.rebalance_begin(0, 1, T, INF, 2, list_moves, x)
        assert e.rebalance_cut(x, y) > 0
        k_loc, total = e.rebalance_select(y, y)
        assert k_loc == total > 1
        pend, rnd = e.rebalance_merge(y), 0
        while pend[0] and rnd < nr:
            e.rebalance_fill(rnd, y)
            pend, rnd = e.rebalance_merge(y), rnd + 1
        return k_loc

    # finish's own refusals, with the protocol at its end: nothing is written, and the right call still goes through
    k = run_to_finish(True)
    buf = np.zeros((3, k), np.uint32)
    ptr = lambda a: a.ctypes.data
    nm = C.c_uint64(0)
    assert L.rio_gp_shard_rebalance_finish(h, C.byref(st), ptr(buf[0]), None, ptr(buf[2]), k, C.byref(nm)) == EINVAL   # not together
    assert L.rio_gp_shard_rebalance_finish(h, C.byref(st), None, None, None, 0, C.byref(nm)) == EINVAL       # listing was asked for
    assert L.rio_gp_shard_rebalance_finish(h, C.byref(st), ptr(buf[0]), ptr(buf[1]), ptr(buf[2]), k - 1, C.byref(nm)) == EINVAL
    assert np.array_equal(e.g.get_assign(), before[0]) and not buf.any()
    run_to_finish(False)                  # (get_assign above is harmless; begin starts over anyway)
    assert L.rio_gp_shard_rebalance_finish(h, C.byref(st), ptr(buf[0]), ptr(buf[1]), ptr(buf[2]), k, C.byref(nm)) == EINVAL  # not asked for
    assert L.rio_gp_shard_rebalance_finish(h, C.byref(st), None, None, None, 5, C.byref(nm)) == EINVAL       # moves_cap without arrays
    assert np.array_equal(e.g.get_assign(), before[0]) and not buf.any()
    # a fresh run gives the reference, with and without the listing
    col = check(sol, [e], None, cur, load, aff, cap, alive, T, 300, 2, list_moves=False)
    check(sol, [e], None, col, load, aff, cap, alive, T, None, 2)
    e.g.close()


def _world1(kind, oracle):
    import torch
    import torch.distributed as dist
    import sharded
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        rng = np.random.default_rng(47)
        n, m = 300_001, 256
        cur, load, aff, alive, T = ref.random_table(rng, n, m, "tight", big_nodes=False, pinned=False)
        cap = np.full(m, INF, np.uint64)
        e = make_engines((cur, load, aff, cap, alive), [0, n])[0]
        ex = sharded.NativeRcclExchange(e) if kind == "rccl" else sharded.P2PExchange(e)
        sol = sharded.ShardedSolver([e], ex)
        col = check(sol, [e], None, cur, load, aff, cap, alive, T, 1000, 2)
        col = check(sol, [e], None, col, load, aff, cap, alive, T, None, 4)
        # the single-handle call keeps refusing such a handle
        rc, _, _ = e.g.rebalance_raw(e.g._rebalance_cfg(T, None, 2)[0])
        assert rc == rio_gp.EINVAL and np.array_equal(e.g.get_assign(), col)
        if kind == "p2p":
            # rio_gp_shard_tick_async ticks in flight: begin is refused and changes nothing — the tick's result and `used` are
            # exactly the oracle's; after rio_gp_shard_tick_wait a rebalance goes through
            import ctypes as C
            T3 = (T * np.uint64(4) // np.uint64(5)).astype(np.uint64)
            cfg, _keep = e.g._rebalance_cfg(T3, None, 2)
            want, used, ost = oracle.tick(col, load, aff, cap, alive, 2)
            sol.tick_async()
            rc = sharded._lib().rio_gp_shard_rebalance_begin(e.g.handle, C.byref(cfg), 0, 1, 1, INF,
                                                             C.c_void_p(sol.X[0].data_ptr()), None)
            assert rc == rio_gp.EINVAL
            sts = sol.tick_wait()
            assert len(sts) == 1 and {k: sts[0][k] for k in ost} == ost
            assert np.array_equal(e.g.get_assign(), want) and np.array_equal(e.g.get_nodes()[2], used)
            check(sol, [e], None, want, load, aff, cap, alive, T3, None, 2)
        e.g.close()
    finally:
        dist.destroy_process_group()


def test_world1_rccl_rung(oracle):
    _world1("rccl", oracle)


def test_world1_p2p_rung(oracle):
    _world1("p2p", oracle)


@pytest.mark.parametrize("world,seed,max_moves,rounds", [(2, 51, -1, 2), (3, 52, 700, 4)])
def test_several_processes_one_gpu_over_gloo(oracle, tmp_path, world, seed, max_moves, rounds):
    """One process per rank on the one GPU, the records staged through the host for gloo.  Every process runs under its own
    time limit; the parent checks every exit status."""
    from shard_rebalance_gpu_worker import case
    n, m = 120_000, 80
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    worker = os.path.join(HERE, "shard_rebalance_gpu_worker.py")
    procs = [subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, worker, str(r), str(world), str(port), str(tmp_path),
                               str(seed), str(n), str(m), str(max_moves), str(rounds)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=300)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            outs.append(p.communicate()[0])
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d exited with %s\n%s" % (r, p.returncode, o[-3000:])
    cur, load, aff, cap, alive, T = case(seed, n, m)
    nxt, used, wst, wrows, wfrom, wto = ref.rebalance(cur, load, aff, cap, alive, T, None if max_moves < 0 else max_moves, rounds)
    zs = [np.load(os.path.join(str(tmp_path), "r%d.npz" % r)) for r in range(world)]
    assert np.array_equal(np.concatenate([z["a"] for z in zs]), nxt)
    for z in zs:
        assert np.array_equal(z["used"], used)
        assert [int(v) for v in z["st"]] == [wst[k] for k in sorted(wst)]
    assert np.array_equal(np.concatenate([z["rows"] for z in zs]), wrows)
    assert np.array_equal(np.concatenate([z["frm"] for z in zs]), wfrom)
    assert np.array_equal(np.concatenate([z["to"] for z in zs]), wto)
    assert wst["moved_rows"] > 0


@pytest.mark.parametrize("seed", [61, 62, 63])
def test_sequence_fuzz(oracle, seed):
    """Sharded ticks, liveness changes, capacity changes and sharded rebalances interleaved over random shard bounds; the oracle
    chain is compared after every operation."""
    import sharded
    rng = np.random.default_rng(seed)
    n, m = int(rng.integers(2000, 40_000)), int(rng.integers(3, 120))
    G = int(rng.integers(1, 6))
    cur, load, aff, alive, T = ref.random_table(rng, n, m, "tight", big_nodes=False, pinned=False)
    per = int(load.sum()) // m
    cap = rng.integers(per // 2 + 1, 2 * per + 2, m).astype(np.uint64)
    b = bounds_for(n, G, "ragged" if G > 1 else "balanced", rng)
    engines = make_engines((cur, load, aff, cap, alive), b)
    sol = sharded.ShardedSolver(engines, sharded.LocalExchange(G))
    col = cur
    for step in range(14):
        op = int(rng.integers(0, 4))
        if op == 0:
            want, used, ost = oracle.tick(col, load, aff, cap, alive, 2)
            st = sol.tick()
            assert st == ost and np.array_equal(column(engines), want), (seed, step)
            for e in engines:
                assert np.array_equal(e.g.get_nodes()[2], used)
            col = want
        elif op == 1:
            alive = (rng.random(m) > 0.2).astype(np.uint8)
            for e in engines:
                e.g.set_alive_all(alive)
        elif op == 2:
            cap = rng.integers(per // 2 + 1, 2 * per + 2, m).astype(np.uint64)
            for e in engines:
                e.g.set_nodes(cap, alive)
        else:
            target = None if rng.random() < 0.5 else rng.integers(per // 3, per + per // 2 + 2, m).astype(np.uint64)
            mm = None if rng.random() < 0.4 else int(rng.integers(0, 400))
            rounds = int(rng.integers(0, 5))
            col = check(sol, engines, None, col, load, aff, cap, alive, target, mm, rounds, eff_rounds=rounds or 2)
    close(engines)
