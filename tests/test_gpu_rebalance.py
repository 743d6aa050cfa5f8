"""Bounded rebalance on the MI355X (rio_gp_rebalance[_dev], rio_op_rebalance) against the two-tick composition of the oracle
(tests/rebalance_ref.py), byte for byte: the column, `used`, the stats and the move list."""
import numpy as np
import pytest

import rebalance_ref as ref
import rio_gp
import synth

pytestmark = pytest.mark.gpu
NONE = rio_gp.NONE
INF = rio_gp.CAP_INF


def load_table(g, cur, load, aff, cap, alive):
    """Rows holding a node >= m are what a shrinking rio_gp_set_nodes leaves behind: placed on a bigger table first."""
    m = len(cap)
    top = int(cur[cur != NONE].max()) + 1 if (cur != NONE).any() else 0
    g.set_nodes(np.full(max(top, m), INF, np.uint64), np.ones(max(top, m), np.uint8))
    g.set_objects(len(cur), load, aff)
    g.set_assign(cur)
    g.set_nodes(cap, alive)


def check(g, cur, load, aff, cap, alive, target=None, max_moves=None, rounds=2, moves_cap=None):
    st, rows, frm, to = g.rebalance(target, max_moves, rounds, moves_cap=moves_cap)
    budget = max_moves if moves_cap is None else (moves_cap if max_moves is None else min(max_moves, moves_cap))
    nxt, used, wst, wrows, wfrom, wto = ref.rebalance(cur, load, aff, cap, alive, target, budget, rounds)
    assert st == wst
    assert np.array_equal(rows, wrows) and np.array_equal(frm, wfrom) and np.array_equal(to, wto)
    assert np.array_equal(g.get_assign(), nxt)
    assert np.array_equal(g.get_nodes()[2], used)
    return nxt


@pytest.mark.parametrize("m", [1, 256, 1024, 4096])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097, 6 * 1024 + 1, 300_001, (1 << 18) - 1, (1 << 18) + 1])
def test_matches_the_composition(oracle, n, m):
    rng = np.random.default_rng(n * 7 + m)
    cur, load, aff, alive, T = ref.random_table(rng, n, m, "tight", max_load=int(rng.choice([3, 50, 4000])))
    cap = np.full(m, INF, np.uint64)
    g = rio_gp.GpuPlacement(max(n, 1), m + 3)
    load_table(g, cur, load, aff, cap, alive)
    nxt = check(g, cur, load, aff, cap, alive, T)                           # unlimited, the handle's 2 rounds
    T2 = (T * np.uint64(9) // np.uint64(10)).astype(np.uint64)
    nxt = check(g, nxt, load, aff, cap, alive, T2, max_moves=max(n // 50, 1), rounds=1)    # a budget, one round
    nxt = check(g, nxt, load, aff, cap, alive, np.zeros(m, np.uint64), rounds=3)         # every candidate surplus, nowhere to go
    # the capacities as targets; the listing smaller than max_moves
    cap2 = T2.copy()
    g.set_nodes(cap2, alive)
    check(g, nxt, load, aff, cap2, alive, None, max_moves=1000, moves_cap=max(n // 100, 1))
    g.close()


@pytest.mark.parametrize("n", [0, 65, 300_001])
def test_dev_form_counts_only_and_budget_zero(oracle, n):
    import torch
    m = 256
    rng = np.random.default_rng(n + 1)
    cur, load, aff, alive, T = ref.random_table(rng, n, m, "tight")
    cap = np.full(m, INF, np.uint64)
    g = rio_gp.GpuPlacement(max(n, 1), m + 3)
    load_table(g, cur, load, aff, cap, alive)
    nxt, used, wst, wrows, wfrom, wto = ref.rebalance(cur, load, aff, cap, alive, T, n // 3, 2)
    k = max(n // 3, 1)
    d = torch.full((3, k + 8), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st, nm = g.rebalance_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), k, target=T)
    torch.cuda.synchronize()
    h = d.cpu().numpy().view(np.uint32)
    assert st == wst and nm == len(wrows)
    assert np.array_equal(h[0, :nm], wrows) and np.array_equal(h[1, :nm], wfrom) and np.array_equal(h[2, :nm], wto)
    assert np.all(h[:, nm:] == 0xFFFFFFFF)  # nothing written past the moves
    assert np.array_equal(g.get_assign(), nxt) and np.array_equal(g.get_nodes()[2], used)
    # counts only (no listing), then a budget of 0: the surplus is counted, nothing moves
    nxt2, used2, wst2, *_ = ref.rebalance(nxt, load, aff, cap, alive, T // np.uint64(2), None, 2)
    st2, nm2 = g.rebalance_dev(target=T // np.uint64(2))
    assert st2 == wst2 and nm2 == wst2["moved_rows"]
    assert np.array_equal(g.get_assign(), nxt2)
    _, _, wst3, *_ = ref.rebalance(nxt2, load, aff, cap, alive, T // np.uint64(4), 0, 2)
    st3, _, _, _ = g.rebalance(T // np.uint64(4), max_moves=0)
    assert st3 == wst3 and st3["moved_rows"] == 0
    assert np.array_equal(g.get_assign(), nxt2)
    g.close()


def test_invalid_arguments_change_nothing(oracle):
    n, m = 5000, 16
    rng = np.random.default_rng(3)
    cur, load, aff, alive, T = ref.random_table(rng, n, m, "zero", dead=False)
    g = rio_gp.GpuPlacement(n, m + 3)
    load_table(g, cur, load, aff, np.full(m, INF, np.uint64), alive)
    before, used = g.get_assign(), g.get_nodes()[2]
    tgt = np.zeros(m, np.uint64)
    buf = np.empty((3, 64), np.uint32)
    bad = [
        (None, dict()),
        (rio_gp.RebalanceCfg(C_size() - 1, 0, INF, tgt.ctypes.data), dict()),
        (rio_gp.RebalanceCfg(C_size(), 9, INF, tgt.ctypes.data), dict()),
        (rio_gp.RebalanceCfg(C_size(), 0, INF, tgt.ctypes.data), dict(out_rows=buf[0], moves_cap=64)),   # one array of three
        (rio_gp.RebalanceCfg(C_size(), 0, INF, tgt.ctypes.data), dict(out_rows=buf[0], out_from=buf[1], moves_cap=64)),
        (rio_gp.RebalanceCfg(C_size(), 0, INF, tgt.ctypes.data), dict(moves_cap=64)),                     # a cap, no listing
    ]
    for cfg, kw in bad:
        rc, _, _ = g.rebalance_raw(cfg, **kw)
        assert rc == rio_gp.EINVAL
        assert np.array_equal(g.get_assign(), before) and np.array_equal(g.get_nodes()[2], used)
    tgt[-4:] = INF   # room on four nodes: the listing of 64 bounds the budget
    rc, st, nm = g.rebalance_raw(rio_gp.RebalanceCfg(C_size(), 0, INF, tgt.ctypes.data), buf[0], buf[1], buf[2], 64)
    _, _, wst, wrows, _, _ = ref.rebalance(cur, load, aff, np.full(m, INF, np.uint64), alive, tgt, 64, 2)
    assert rc == rio_gp.OK and st == wst and 0 < nm <= st["selected_rows"] == 64
    assert np.array_equal(buf[0, :nm], wrows)
    g.close()


def C_size():
    import ctypes
    return ctypes.sizeof(rio_gp.RebalanceCfg)


def test_ticks_after_and_between_rebalances(oracle):
    """A rebalance is a change of the inputs: the tick after it (committed, quiet, chained over 2^18+ rows) solves the new column."""
    import pyoracle
    n, m = (1 << 18) + 4097, 512
    rng = np.random.default_rng(17)
    load = rng.integers(1, 40, n).astype(np.uint32)
    aff = rng.integers(0, m, n).astype(np.uint32)
    alive = np.ones(m, np.uint8)
    alive[::37] = 0
    cap = np.full(m, int(load.sum()) // m * 2, np.uint64)
    g = rio_gp.GpuPlacement(n, m)
    g.set_nodes(cap, alive)
    g.set_objects(n, load, aff)
    col, _, _ = pyoracle.tick(np.full(n, NONE, np.uint32), load, aff, cap, alive)
    g.tick()
    assert np.array_equal(g.get_assign(), col)
    for step in range(4):
        for _ in range(3):   # quiet ticks, chained
            g.tick_async()
        g.tick_wait()
        col, _, _ = pyoracle.tick(col, load, aff, cap, alive)
        assert np.array_equal(g.get_assign(), col)
        used = pyoracle.recompute_used(col, load, m)
        T = rio_gp.balanced_targets(cap, used, alive, 10 + 20 * step)
        T[(step * 50) % m: (step * 50) % m + 40] //= np.uint64(2)
        g.tick_async()                            # in flight when the rebalance comes: it joins
        col, _, _ = pyoracle.tick(col, load, aff, cap, alive)
        st, rows, frm, to = g.rebalance(T, max_moves=[None, 5000, 1, 0][step])
        col2, used2, wst, wrows, *_ = ref.rebalance(col, load, aff, cap, alive, T, [None, 5000, 1, 0][step], 2)
        assert st == wst and np.array_equal(rows, wrows)
        g.tick_async()
        g.tick_async()
        g.tick_wait()
        col, _, _ = pyoracle.tick(col2, load, aff, cap, alive)
        col, _, _ = pyoracle.tick(col, load, aff, cap, alive)
        assert np.array_equal(g.get_assign(), col)
        g.tick()
        col, used, _ = pyoracle.tick(col, load, aff, cap, alive)
        assert np.array_equal(g.get_assign(), col) and np.array_equal(g.get_nodes()[2], used)
    g.close()


def test_config3_capacity_cut_and_scale_out(oracle):
    cfg = synth.config("c3w")
    n, m = cfg["n"], cfg["m"]
    load, aff, cap, cur = cfg["load"], cfg["aff"], cfg["cap"].copy(), cfg["cur"]
    alive = np.ones(m, np.uint8)
    g = rio_gp.GpuPlacement(n, m + 64)
    load_table(g, cur, load, aff, cap, alive)
    cap[::10] = cap[::10] * np.uint64(7) // np.uint64(10)      # 10 % of the nodes lose 30 % of their capacity
    g.set_nodes(cap, alive)
    col = check(g, cur, load, aff, cap, alive)
    # scale-out: 64 empty nodes, balanced targets
    cap2 = np.concatenate([cap, np.full(64, int(cap.mean()), np.uint64)])
    alive2 = np.ones(m + 64, np.uint8)
    g.set_nodes(cap2, alive2)
    used = g.get_nodes()[2]
    T = rio_gp.balanced_targets(cap2, used, alive2, 20)
    col = check(g, col, load, aff, cap2, alive2, T, max_moves=10_000)
    check(g, col, load, aff, cap2, alive2, T)
    g.close()


def test_string_layer_moves_and_lookups(oracle):
    p = rio_gp.GpuObjectPlacement(max_objects=1 << 14, max_nodes=16)
    addrs = ["10.0.0.%d:5000" % k for k in range(6)]
    for a in addrs:
        p.set_member(a, True, 1000)
    keys = [("Svc", "o%d" % k) for k in range(3000)]
    rng = np.random.default_rng(2)
    home = {}
    for k, key in enumerate(keys):
        a = addrs[int(rng.integers(0, 3))]          # everything on the first three servers
        p.update(key[0], key[1], a)
        home[key] = a
    p.update("Svc", "nul\0key", addrs[0])
    home[("Svc", "nul\0key")] = addrs[0]
    for a in addrs:
        p.set_member(a, True, 550)                   # lower the capacities: spread onto the three empty servers
    moves = p.rebalance()
    assert moves and all(f != t for _, _, f, t in moves)
    for ty, oid, f, t in moves:
        assert home[(ty, oid)] == f
        home[(ty, oid)] = t
    for (ty, oid), a in home.items():
        assert p.lookup(ty, oid) == a
    for a in addrs:
        assert sorted(p.objects_on_server(a)) == sorted(k for k, v in home.items() if v == a)
    p.close()
