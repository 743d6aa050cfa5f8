"""What may be in flight on a handle's pinned verdict slots, and who may start beside it (rio_gp_capi.hip: SolveRing, TickRing,
ShardSolve, RbSession, may_start).  One device, one process: a handle with the peer-to-peer windows connected at world size 1
(as test_gpu_sharded.py::test_hip_shard_p2p_world1) and one driven step by step over LocalExchange.

Every refusal that reads that state is reached once — return code, a substring of rio_gp_last_error, and the table as it was —
and every legal hand-over between the clients of the slots ends equal to the CPU oracle: column, `used`, counters.  The
argument checks of rio_gp_shard_rebalance_*, its steps called from idle and right behind _begin, and the step after
rio_gp_set_alive_all / rio_gp_get_nodes are test_gpu_shard_rebalance.py::test_invalid_calls_change_nothing's; here are the
steps one early further into the protocol.  Nothing here calls an order the library neither refuses nor documents.

Shapes: n = 5 000, m = 7 (resolve_blocks = 1: one verdict row whoever wrote it) and n = 70 000, m = 50 (seven partial rows from
k_resolve / k_resolve_xchg against k_shard_import's one), each roomy (every row kept: no fix-up) and at cap_scale 0.92 (cuts,
spill, unplaced rows: the whole fix-up)."""
import ctypes as C
import os
import socket

import numpy as np
import pytest

import rebalance_ref as ref
from test_gpu_sharded import _async_mask, make_engines
from test_sharded_protocol import random_case

pytestmark = pytest.mark.gpu

SHAPES = {"small": (5_000, 7), "big": (70_000, 50)}
KINDS = {"roomy": dict(cap_scale=6.0, warm=1.0), "tight": dict(cap_scale=0.92)}
ROUNDS = 2
RING = 64   # kRing: verdict slots in each half of the table


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


@pytest.fixture(scope="module")
def tables(oracle):
    """(case, column, used, counters) of one oracle tick per shape and kind: computed once, read-only."""
    out = {}
    for shape, (n, m) in SHAPES.items():
        for kind, kw in KINDS.items():
            case = random_case(71, n=n, m=m, **kw)
            want, used, st = oracle.tick(*case, ROUNDS)
            for a in case + (want, used):
                a.setflags(write=False)
            out[shape, kind] = (case, want, used, st)
        assert out[shape, "roomy"][3]["slow_path"] == 0 and out[shape, "tight"][3]["cut_nodes"] > 0
    return out


@pytest.fixture(scope="module")
def group():
    """The control channel P2PExchange moves its window handles over: gloo, world size 1."""
    import torch
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=0, world_size=1)
    yield dist
    dist.destroy_process_group()


def local_engine(gp, case):
    import sharded
    e = make_engines(gp, case, [0, len(case[0])], ROUNDS)[0]
    return e, sharded.ShardedSolver([e], sharded.LocalExchange(1), spill_rounds=ROUNDS)


def p2p_engine(gp, case):
    import sharded
    e = make_engines(gp, case, [0, len(case[0])], ROUNDS)[0]
    return e, sharded.ShardedSolver([e], sharded.P2PExchange(e), spill_rounds=ROUNDS)


def lib():
    import sharded
    return sharded._lib()


def vp(t):
    return C.c_void_p(t.data_ptr())


def refused(g, rc, *needles):
    import rio_gp
    assert rc == rio_gp.EINVAL, rc
    text = g._L.rio_gp_last_error(g.handle).decode()
    for s in needles:
        assert s in text, text


def snapshot(g, solved=False, nodes=True):
    return g.get_assign(), g.get_nodes()[2] if nodes else None, g.get_solved() if solved else None


def unchanged(g, snap):
    now = snapshot(g, snap[2] is not None, snap[1] is not None)
    for a, b in zip(now, snap):
        assert b is None or np.array_equal(a, b)


def committed_equals(g, want, used):
    assert np.array_equal(g.get_assign(), want)
    assert np.array_equal(g.get_nodes()[2], used)


def solve_wait_raw(gp, g):
    st, ns = gp.Stats(), C.c_uint32(0)
    return g._L.rio_gp_solve_wait(g.handle, C.byref(st), C.byref(ns))


def rebalance_begin_raw(gp, e, x):
    cfg, _keep = e.g._rebalance_cfg(None, None, 0)
    return lib().rio_gp_shard_rebalance_begin(e.g.handle, C.byref(cfg), 0, 1, 1, gp.CAP_INF, vp(x), None)


# ---- refusals -----------------------------------------------------------------------------------------------------------

def test_ticks_refused_with_solves_in_flight(gp, tables, group):
    case, want, used, ost = tables["small", "tight"]
    e, sol = p2p_engine(gp, case)
    g, L, h = e.g, lib(), e.g.handle
    g.solve_async()
    snap = snapshot(g)
    refused(g, L.rio_gp_tick_async(h), "rio_gp_tick_async", "in flight")
    refused(g, L.rio_gp_shard_tick_async(h), "rio_gp_shard_tick_async", "in flight")
    unchanged(g, snap)
    st, n_slow = g.solve_wait()
    assert st == ost and n_slow == 1 and np.array_equal(g.get_solved(), want)
    snap = snapshot(g, solved=True)
    refused(g, solve_wait_raw(gp, g), "rio_gp_solve_wait", "nothing enqueued")
    unchanged(g, snap)
    g.commit()
    committed_equals(g, want, used)
    g.close()


def test_shard_tick_refused_with_ticks_in_flight(gp, tables, group):
    case, want, used, ost = tables["small", "tight"]
    e, sol = p2p_engine(gp, case)
    g = e.g
    g.tick_async()
    snap = snapshot(g)
    refused(g, lib().rio_gp_shard_tick_async(g.handle), "rio_gp_shard_tick_async", "in flight")
    unchanged(g, snap)
    assert g.tick_wait() == [ost]
    committed_equals(g, want, used)
    g.close()


def test_refusals_with_shard_ticks_in_flight(gp, tables, group):
    case, want, used, ost = tables["big", "tight"]
    e, sol = p2p_engine(gp, case)
    g, L, h = e.g, lib(), e.g.handle
    sol.tick_async()
    snap = snapshot(g)
    refused(g, L.rio_gp_tick_async(h), "rio_gp_tick_async", "row-sharded ticks", "in flight")
    refused(g, L.rio_gp_solve_async(h), "rio_gp_solve_async", "row-sharded ticks", "in flight")
    refused(g, L.rio_gp_shard_solve_async(h), "rio_gp_shard_solve_async", "row-sharded ticks", "in flight")
    refused(g, rebalance_begin_raw(gp, e, sol.X[0]), "rio_gp_shard_rebalance_begin", "in flight")
    unchanged(g, snap)
    assert sol.tick_wait() == [ost]
    committed_equals(g, want, used)
    g.close()


def test_shard_tick_ring_full(gp, oracle, tables, group):
    case, want, used, ost = tables["small", "tight"]
    cur, load, aff, cap, alive = case
    w2, u2, o2 = oracle.tick(want, load, aff, cap, alive, ROUNDS)
    w3, u3, o3 = oracle.tick(w2, load, aff, cap, alive, ROUNDS)
    assert np.array_equal(w2, want) and np.array_equal(w3, w2) and o3 == o2   # a fixed point from the second tick on
    e, sol = p2p_engine(gp, case)
    g = e.g
    for _ in range(RING):
        sol.tick_async()
    snap = snapshot(g)
    refused(g, lib().rio_gp_shard_tick_async(g.handle), "rio_gp_shard_tick_async", "64 ticks in flight")
    unchanged(g, snap)
    assert sol.tick_wait() == [ost] + [o2] * (RING - 1)
    committed_equals(g, w2, u2)
    sol.tick_async()                       # the ring is free again
    assert sol.tick_wait() == [o2]
    g.close()


def test_whole_table_calls_refused_on_connected_handle(gp, tables, group):
    case, want, used, ost = tables["small", "tight"]
    e, sol = p2p_engine(gp, case)
    g = e.g
    assert g.solve() == ost                # an uncommitted solve: the refusals leave it as it is
    snap = snapshot(g, solved=True)
    cfg, _keep = g._rebalance_cfg(None, None, 0)
    refused(g, g.rebalance_raw(cfg)[0], "rio_gp_rebalance", "row-sharded")
    refused(g, g.changes_raw(0)[0], "rio_gp_changes", "row-sharded")
    refused(g, g._L.rio_gp_changes_reset(g.handle), "rio_gp_changes_reset", "row-sharded")
    refused(g, g.remap_nodes_raw(len(case[3]), np.arange(len(case[3]), dtype=np.uint32))[0], "rio_gp_remap_nodes", "row-sharded")
    unchanged(g, snap)
    assert sol.tick() == ost
    committed_equals(g, want, used)
    g.close()


def test_shard_steps_one_step_early(gp, tables):
    """Every rio_gp_shard_* step, asked for where the protocol is not: refused, and the solve still comes out as the oracle's."""
    import sharded
    case, want, used, ost = tables["big", "tight"]
    e, sol = local_engine(gp, case)
    g, L, h = e.g, lib(), e.g.handle
    x, y, xg = sol.X[0], sol.Y[0], sol.XG[0]
    info, ns, a, b, st = sharded.ShardInfo(), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0), gp.Stats()
    calls = {
        "resolve": lambda: L.rio_gp_shard_resolve(h, 0, 1, vp(xg), None),
        "verdict": lambda: L.rio_gp_shard_verdict(h, C.byref(info), C.byref(ns)),
        "cut": lambda: L.rio_gp_shard_cut(h, 1, vp(y)),
        "merge": lambda: L.rio_gp_shard_merge(h, vp(y), C.byref(a), C.byref(b)),
        "spill": lambda: L.rio_gp_shard_spill(h, 0, 0, vp(y)),
        "finish": lambda: L.rio_gp_shard_finish(h, C.byref(st)),
    }

    def all_refused(*names):
        for name in names:
            refused(g, calls[name](), "rio_gp_shard_" + name)

    assert g.solve() == ost                # an uncommitted solve: the refusals at idle leave it as it is
    snap = snapshot(g, solved=True)
    all_refused("resolve", "verdict", "cut", "merge", "spill", "finish")            # idle
    unchanged(g, snap)
    snap = snapshot(g)
    e.scan(x)
    all_refused("verdict", "cut", "merge", "spill", "finish")                       # scanned
    sol._gather([x], out=xg)
    e.resolve(0, 1, xg)
    all_refused("resolve", "merge", "spill")                                        # resolved
    v = e.verdict()
    assert v["cut_nodes"] == ost["cut_nodes"] and v["n_slow"] == 1
    all_refused("resolve", "merge", "spill")                                        # resolved, the verdict read: a fix-up pending
    unchanged(g, snap)
    e.cut(v["local_fixup"] > 0 and v["cut_nodes"] > 0, y)
    all_refused("resolve", "verdict", "cut", "spill", "finish")                     # cut exported
    pend, rounds_run = e.merge(sol._gather([y])), 0
    all_refused("resolve", "verdict", "cut", "merge")                               # merged
    assert pend[0] > 0
    while rounds_run < ROUNDS and pend[0]:
        e.spill(rounds_run, rounds_run + 1 == ROUNDS, y)
        all_refused("resolve", "verdict", "cut", "spill", "finish")                 # spill exported
        pend, rounds_run = e.merge(sol._gather([y])), rounds_run + 1
    local = e.finish()
    snap = snapshot(g, solved=True)
    all_refused("verdict", "cut", "merge", "spill", "finish")                       # idle again, the finished solve uncommitted
    unchanged(g, snap)
    assert rounds_run == ost["rounds_run"]
    assert {k: local[k] for k in sharded.STAT_KEYS} == {k: ost[k] for k in sharded.STAT_KEYS}   # one rank: local = global
    assert np.array_equal(g.get_solved(), want)
    g.commit()
    committed_equals(g, want, used)
    g.close()


def test_shard_cut_after_fast_verdict(gp, tables):
    case, want, used, ost = tables["big", "roomy"]
    e, sol = local_engine(gp, case)
    g = e.g
    sol.solve_async()
    v = e.verdict()
    assert v["cut_nodes"] == 0 and v["spill_rows"] == 0 and v["n_slow"] == 0
    snap = snapshot(g)
    refused(g, lib().rio_gp_shard_cut(g.handle, 0, vp(sol.Y[0])), "rio_gp_shard_cut", "no fix-up pending")
    unchanged(g, snap)
    local = e.finish()
    assert local["kept"] == ost["kept"] and np.array_equal(g.get_solved(), want)
    g.commit()
    committed_equals(g, want, used)
    g.close()


def test_shard_rebalance_steps_one_step_early(gp, oracle, tables):
    """Further into the protocol than test_gpu_shard_rebalance.py::test_invalid_calls_change_nothing goes: behind _cut, _select,
    _merge and _fill, and behind a rio_gp_set_alive that moved mut_epoch.  The capacities are the targets: one node over."""
    case, want, used, ost = tables["small", "tight"]
    cur, load, aff, cap, alive = case
    e, sol = local_engine(gp, case)
    g, L, h = e.g, lib(), e.g.handle
    x, y = sol.X[0], sol.Y[0]
    ov, a, b, st = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0), gp.RebalanceStats()
    calls = {
        "cut": lambda: L.rio_gp_shard_rebalance_cut(h, vp(x), vp(y), C.byref(ov)),
        "select": lambda: L.rio_gp_shard_rebalance_select(h, vp(y), vp(y), C.byref(a), C.byref(b)),
        "merge": lambda: L.rio_gp_shard_rebalance_merge(h, vp(y), C.byref(a), C.byref(b)),
        "fill0": lambda: L.rio_gp_shard_rebalance_fill(h, 0, vp(y)),
        "fill1": lambda: L.rio_gp_shard_rebalance_fill(h, 1, vp(y)),
        "finish": lambda: L.rio_gp_shard_rebalance_finish(h, C.byref(st), None, None, None, 0, None),
    }

    def all_refused(*names):
        for name in names:
            refused(g, calls[name](), "rio_gp_shard_rebalance_" + name.rstrip("01"))

    nr = e.rebalance_begin(0, 1, None, gp.CAP_INF, 0, True, x)
    assert nr == ROUNDS
    all_refused("merge")                                                            # begun (the other steps: the cited test)
    assert e.rebalance_cut(x, y) == 1
    all_refused("cut", "merge", "fill0", "finish")                                  # cut, a node over
    k_loc, total = e.rebalance_select(y, y)
    assert k_loc == total > 1
    all_refused("cut", "select", "fill0", "finish")                                 # selected
    pend = e.rebalance_merge(y)
    assert pend[0] > 0
    all_refused("cut", "select", "merge", "fill1", "finish")                        # merged, rows pending: round 0 is next
    e.rebalance_fill(0, y)
    all_refused("cut", "select", "fill0", "fill1", "finish")                        # round exported
    assert np.array_equal(g.get_assign(), cur)                                      # nothing is applied before _finish
    g.set_alive(0, int(alive[0]))                                                   # an input call: the session is over
    all_refused("merge", "finish")
    # a session run to its end on the same handle gives the reference, and the tick behind it the oracle's
    rst, rows, frm, to = sol.rebalance(target=None, rounds=0)
    nxt, rused, wst, wrows, wfrom, wto = ref.rebalance(cur, load, aff, cap, alive, None, None, ROUNDS)
    assert rst == wst and np.array_equal(rows, wrows) and np.array_equal(frm, wfrom) and np.array_equal(to, wto)
    committed_equals(g, nxt, rused)
    w2, u2, o2 = oracle.tick(nxt, load, aff, cap, alive, ROUNDS)
    assert sol.tick() == o2
    committed_equals(g, w2, u2)
    g.close()


# ---- legal hand-overs ---------------------------------------------------------------------------------------------------

def plain(gp, case):
    cur, load, aff, cap, alive = case
    g = gp.GpuPlacement(len(cur), len(cap), spill_rounds=ROUNDS)
    g.set_nodes(cap, alive)
    g.set_objects(len(cur), load, aff)
    g.set_assign(cur)
    return g


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_solve_ring_recycles_once(gp, tables, shape, kind):
    """65 rio_gp_solve_async: the 65th folds the first 64 verdicts into the running count and starts the ring again."""
    case, want, used, ost = tables[shape, kind]
    g = plain(gp, case)
    for _ in range(RING + 1):
        g.solve_async()
    st, n_slow = g.solve_wait()
    assert st == ost and n_slow == (RING + 1) * ost["slow_path"]
    assert np.array_equal(g.get_solved(), want)
    g.commit()
    committed_equals(g, want, used)
    g.close()


def test_synchronous_tick_abandons_solves_in_flight(gp, tables):
    case, want, used, ost = tables["big", "tight"]
    g = plain(gp, case)
    for _ in range(3):
        g.solve_async()
    assert g.tick() == ost
    snap = snapshot(g)
    refused(g, solve_wait_raw(gp, g), "rio_gp_solve_wait", "nothing enqueued")
    unchanged(g, snap)
    committed_equals(g, want, used)
    g.close()


def test_synchronous_solve_between_ticks_in_flight(gp, oracle, tables):
    """The synchronous solve uses the other half of the slot table and fx slot 0: the ticks around it keep their records."""
    case, want, used, ost = tables["big", "tight"]
    cur, load, aff, cap, alive = case
    flip = alive.copy()
    flip[[3, 11, 29]] = 0
    w2, u2, o2 = oracle.tick(want, load, aff, cap, flip, ROUNDS)
    w3, u3, o3 = oracle.tick(w2, load, aff, cap, alive, ROUNDS)
    g = plain(gp, case)
    g.tick_async()
    g.set_alive_all(flip)
    g.tick_async()
    g.set_alive_all(alive)
    assert g.solve() == o3 and np.array_equal(g.get_solved(), w3)      # uncommitted: the third tick's answer ahead of it
    g.tick_async()
    assert g.tick_wait() == [ost, o2, o3]
    committed_equals(g, w3, u3)
    g.close()


@pytest.mark.parametrize("exchange,shape,kind", [("p2p", "big", "tight"), ("local", "small", "tight"), ("p2p", "small", "roomy")])
def test_shard_solve_ring_wraps(gp, tables, group, exchange, shape, kind):
    """70 row-sharded solves before the verdict: the cursor wraps (k % 64) and n_slow counts the last 64."""
    case, want, used, ost = tables[shape, kind]
    e, sol = (p2p_engine if exchange == "p2p" else local_engine)(gp, case)
    for _ in range(RING + 6):
        sol.solve_async()
    st, n_slow = sol.solve_wait()
    assert st == ost and n_slow == RING * ost["slow_path"]
    assert np.array_equal(e.g.get_solved(), want)
    sol.commit()
    committed_equals(e.g, want, used)
    e.g.close()


@pytest.mark.parametrize("left_at", ["resolved", "merged"])
def test_rebalance_begin_drops_a_shard_solve_half_way(gp, oracle, tables, left_at):
    case, want, used, ost = tables["small", "tight"]
    cur, load, aff, cap, alive = case
    e, sol = local_engine(gp, case)
    sol.solve_async()
    if left_at == "merged":
        v = e.verdict()
        e.cut(v["local_fixup"] > 0 and v["cut_nodes"] > 0, sol.Y[0])
        assert e.merge(sol._gather(sol.Y))[0] > 0
    rst, rows, frm, to = sol.rebalance(target=None, rounds=0)
    nxt, rused, wst, wrows, wfrom, wto = ref.rebalance(cur, load, aff, cap, alive, None, None, ROUNDS)
    assert rst == wst and rst["moved_rows"] > 0
    assert np.array_equal(rows, wrows) and np.array_equal(frm, wfrom) and np.array_equal(to, wto)
    committed_equals(e.g, nxt, rused)
    w2, u2, o2 = oracle.tick(nxt, load, aff, cap, alive, ROUNDS)
    assert sol.tick() == o2
    committed_equals(e.g, w2, u2)
    e.g.close()


def test_shard_ticks_with_a_wait_in_the_middle(gp, oracle, tables, group):
    case, want, used, ost = tables["big", "tight"]
    cur, load, aff, cap, alive = case
    e, sol = p2p_engine(gp, case)
    col, osts, sts = cur, [], []
    for k in range(5):
        mask = _async_mask(len(cap), k)
        col, u, o = oracle.tick(col, load, aff, cap, mask, ROUNDS)
        osts.append(o)
        e.g.set_alive_all(mask)
        sol.tick_async()
        if k == 2:
            sts += sol.tick_wait()
    sts += sol.tick_wait()
    assert sts == osts and any(o["slow_path"] for o in osts)
    committed_equals(e.g, col, u)
    e.g.close()


def test_p2p_close_with_a_solve_resolved(gp, tables, group):
    """rio_gp_shard_p2p_close drops the solve in flight with the windows; fresh windows on the same handle solve as new."""
    import sharded
    case, want, used, ost = tables["big", "tight"]
    e, sol = p2p_engine(gp, case)
    sol.solve_async()
    sol.ex.close()
    assert lib().rio_gp_shard_p2p_ready(e.g.handle) == 0
    refused(e.g, lib().rio_gp_shard_verdict(e.g.handle, C.byref(sharded.ShardInfo()), None), "rio_gp_shard_verdict")
    sol = sharded.ShardedSolver([e], sharded.P2PExchange(e), spill_rounds=ROUNDS)
    assert sol.solve() == ost and np.array_equal(e.g.get_solved(), want)
    sol.commit()
    committed_equals(e.g, want, used)
    e.g.close()
