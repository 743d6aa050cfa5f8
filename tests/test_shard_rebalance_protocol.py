"""The row-sharded rebalance protocol on the CPU: `ShardedSolver.rebalance` drives numpy engines (tests/shard_rebalance_cpu.py)
over LocalExchange, and over gloo with one process per shard.  Column, `used` on every rank, counters and moves must equal the
whole-table rebalance of both references: tests/rebalance_ref.py (two oracle ticks) and tests/spec_rebalance.py (the rule
written out)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import rebalance_ref
import spec_rebalance
from rebalance_ref import INACTIVE, INF, NONE

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def bounds_for(n, G, kind, rng):
    """balanced | ragged (random cut points, some shards empty) | empty (all rows on one shard in the middle)"""
    if kind == "balanced":
        return [(r * n) // G for r in range(G + 1)]
    if kind == "empty":
        b = [0] * (G + 1)
        for r in range(G // 2 + 1, G + 1):
            b[r] = n
        return b
    cuts = sorted(int(c) for c in rng.integers(0, n + 1, G - 1))
    if G > 2:
        cuts[1] = cuts[0]   # an empty shard between two others
    return [0] + cuts + [n]


def run_sharded(cur, load, aff, cap, alive, b, target, max_moves, rounds, spill_rounds=2, list_moves=True):
    import sharded
    from shard_rebalance_cpu import CpuRebalanceEngine
    G = len(b) - 1
    engs = [CpuRebalanceEngine(cur[b[r]:b[r + 1]], load[b[r]:b[r + 1]], aff[b[r]:b[r + 1]], cap, alive, spill_rounds)
            for r in range(G)]
    sol = sharded.ShardedSolver(engs, sharded.LocalExchange(G), spill_rounds=spill_rounds)
    st, rows, frm, to = sol.rebalance(target=target, max_moves=max_moves, rounds=rounds, list_moves=list_moves)
    return engs, sol, st, rows, frm, to


def check_against_references(oracle, cur, load, aff, cap, alive, T, max_moves, rounds, engs, st, rows, frm, to, eff_rounds):
    want, used, wst, wrows, wfrom, wto = rebalance_ref.rebalance(cur, load, aff, cap, alive, target=T, max_moves=max_moves,
                                                                 rounds=eff_rounds)
    got = np.concatenate([e.assign for e in engs]) if engs else np.zeros(0, np.uint32)
    assert np.array_equal(got, want)
    for e in engs:
        assert np.array_equal(e.used, used)
    assert st == wst
    assert np.array_equal(rows, wrows) and np.array_equal(frm, wfrom) and np.array_equal(to, wto)
    snxt, sused, sst, smoves = spec_rebalance.rebalance([int(v) for v in cur], [int(v) for v in load], [int(v) for v in aff],
                                                        [int(v) for v in cap], [int(v) for v in alive],
                                                        target=None if T is None else [int(v) for v in T],
                                                        max_moves=max_moves, rounds=eff_rounds)
    assert [int(v) for v in got] == list(snxt)
    assert [int(v) for v in engs[0].used] == list(sused)
    assert st == sst
    assert [(int(r), int(f), int(t)) for r, f, t in zip(rows, frm, to)] == [tuple(x) for x in smoves]
    return wst


@pytest.mark.parametrize("G", [1, 2, 3, 8])
@pytest.mark.parametrize("kind", ["tight", "zero", "inf"])
@pytest.mark.parametrize("shape", ["balanced", "ragged", "empty"])
def test_sharded_rebalance_equals_the_whole_table(oracle, G, kind, shape):
    rng = np.random.default_rng(1000 * G + 10 * len(kind) + len(shape))
    n, m = 1500, 12
    cur, load, aff, alive, T = rebalance_ref.random_table(rng, n, m, target_kind=kind)
    cap = rng.integers(100, 5000, m).astype(np.uint64)
    b = bounds_for(n, G, shape, rng)
    moved = 0
    for max_moves, rounds in ((0, 1), (1, 2), (37, 4), (None, 8), (None, 1), (200, 2)):
        engs, sol, st, rows, frm, to = run_sharded(cur, load, aff, cap, alive, b, T, max_moves, rounds)
        wst = check_against_references(oracle, cur, load, aff, cap, alive, T, max_moves, rounds, engs, st, rows, frm, to, rounds)
        moved += wst["moved_rows"]
    if kind == "tight":
        assert moved > 0
    if kind == "inf":
        assert moved == 0


@pytest.mark.parametrize("G", [2, 3])
def test_default_target_is_the_capacities_and_default_rounds_the_handles(oracle, G):
    rng = np.random.default_rng(77 + G)
    n, m = 1200, 9
    cur, load, aff, alive, _ = rebalance_ref.random_table(rng, n, m)
    cap = rng.integers(int(load.sum()) // (2 * m), int(load.sum()) // m + 2, m).astype(np.uint64)
    b = bounds_for(n, G, "ragged", rng)
    for spill_rounds in (1, 3):
        engs, sol, st, rows, frm, to = run_sharded(cur, load, aff, cap, alive, b, None, None, 0, spill_rounds=spill_rounds)
        wst = check_against_references(oracle, cur, load, aff, cap, alive, None, None, 0, engs, st, rows, frm, to, spill_rounds)
        assert wst["surplus_rows"] > 0
    # without a listing: the same column and counters, no moves
    engs, sol, st, rows, frm, to = run_sharded(cur, load, aff, cap, alive, b, None, 50, 2, list_moves=False)
    want, used, wst, _, _, _ = rebalance_ref.rebalance(cur, load, aff, cap, alive, max_moves=50, rounds=2)
    assert np.array_equal(np.concatenate([e.assign for e in engs]), want) and st == wst and len(rows) == 0


def cut_on_rank0_table():
    """Node 0 (T = 10): rank 0 holds candidates of load 6, 6 (the second overflows: the cut falls on rank 0) and a zero-load
    candidate in front of the cut; ranks 1 and 2 hold only zero-load candidates of node 0 — all of them surplus.  Node 1
    (T = 10): rank 0 fills it exactly (4 + 6); the zero-load candidates of node 1 on ranks 1 and 2 are kept."""
    cur = np.array([0, 0, 0, 1, 1, 2,   0, 1, 0, 2,   0, 1, 2, 0], np.uint32)
    load = np.array([6, 0, 6, 4, 6, 1,   0, 0, 0, 1,   0, 0, 1, 0], np.uint32)
    aff = np.zeros(len(cur), np.uint32)
    cap = np.array([10, 10, 100], np.uint64)
    alive = np.ones(3, np.uint8)
    return cur, load, aff, cap, alive, [0, 6, 10, 14]


def test_cut_on_rank_zero_makes_later_zero_load_candidates_surplus(oracle):
    cur, load, aff, cap, alive, b = cut_on_rank0_table()
    engs, sol, st, rows, frm, to = run_sharded(cur, load, aff, cap, alive, b, None, None, 2)
    check_against_references(oracle, cur, load, aff, cap, alive, None, None, 2, engs, st, rows, frm, to, 2)
    # surplus: row 2 (the overflow) and the zero-load candidates of node 0 behind it on ranks 1 and 2: rows 6, 8, 10, 13
    assert st["surplus_rows"] == 5 and st["surplus_load"] == 6
    assert [int(e.rb_surplus.sum()) for e in engs] == [1, 2, 2]
    assert list(rows) == [2, 6, 8, 10, 13] and set(int(t) for t in to) == {2}
    # node 1 was an exact fit: nothing of it is surplus
    assert not any(cur[r] == 1 for r in rows)
    # a budget that ends inside rank 1
    engs, sol, st, rows, frm, to = run_sharded(cur, load, aff, cap, alive, b, None, 2, 2)
    check_against_references(oracle, cur, load, aff, cap, alive, None, 2, 2, engs, st, rows, frm, to, 2)
    assert list(rows) == [2, 6] and st["surplus_rows"] == 5 and st["selected_rows"] == 2


def test_exchange_count_is_three_plus_rounds(oracle):
    """X, the surplus record, used', one Y per round that ran — and the driver's own gather of the counters."""
    import sharded
    from shard_rebalance_cpu import CpuRebalanceEngine
    rng = np.random.default_rng(5)
    cur, load, aff, alive, T = rebalance_ref.random_table(rng, 900, 10)
    cap = np.full(10, 1000, np.uint64)

    class Counting(sharded.LocalExchange):
        calls = 0

        def all_gather(self, parts):
            Counting.calls += 1
            return super().all_gather(parts)

        def all_gather_into(self, out, parts):
            Counting.calls += 1
            return super().all_gather_into(out, parts)

    b = bounds_for(900, 3, "balanced", rng)
    for target, max_moves, rounds, most in ((T, None, 4, 3 + 4 + 1), (np.full(10, INF, np.uint64), None, 4, 1 + 1),
                                            (T, 0, 4, 2 + 1)):
        engs = [CpuRebalanceEngine(cur[b[r]:b[r + 1]], load[b[r]:b[r + 1]], aff[b[r]:b[r + 1]], cap, alive) for r in range(3)]
        sol = sharded.ShardedSolver(engs, Counting(3))
        Counting.calls = 0
        sol.rebalance(target=target, max_moves=max_moves, rounds=rounds)
        assert 2 <= Counting.calls <= most, (Counting.calls, most)


def test_hip_engine_has_one_method_per_step_and_the_library_the_symbols():
    """Fails without the feature on a machine without a GPU too: the binding and the exported entry points."""
    import rio_gp
    import sharded
    rio_gp.build()
    L = sharded._lib()
    for step in ("begin", "cut", "select", "merge", "fill", "finish"):
        assert hasattr(sharded.HipShardEngine, "rebalance_" + step)
        assert getattr(L, "rio_gp_shard_rebalance_" + step).argtypes is not None
    assert hasattr(sharded.ShardedSolver, "rebalance")


# ---- one process per shard over gloo ----

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_case(seed, n, m):
    rng = np.random.default_rng(seed)
    cur, load, aff, alive, T = rebalance_ref.random_table(rng, n, m)
    cap = rng.integers(100, 5000, m).astype(np.uint64)
    return cur, load, aff, cap, alive, T


def _worker(rank, world, port, seed, n, m, max_moves, rounds, out_dir):
    for p in (ROOT, os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "oracle"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    import sharded
    from shard_rebalance_cpu import CpuRebalanceEngine
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cur, load, aff, cap, alive, T = _gloo_case(seed, n, m)
        b = bounds_for(n, world, "ragged", np.random.default_rng(seed + 1))
        lo, hi = b[rank], b[rank + 1]
        eng = CpuRebalanceEngine(cur[lo:hi], load[lo:hi], aff[lo:hi], cap, alive)
        sol = sharded.ShardedSolver([eng], sharded.DistExchange(), spill_rounds=2)
        st, rows, frm, to = sol.rebalance(target=T, max_moves=max_moves, rounds=rounds)
        np.savez(os.path.join(out_dir, "r%d.npz" % rank), a=eng.assign, used=eng.used, rows=rows, frm=frm, to=to,
                 st=np.array([st[k] for k in sorted(st)], np.uint64))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,seed,max_moves,rounds", [(2, 31, None, 2), (3, 32, 40, 4), (3, 33, None, 1)])
def test_gloo_sharded_rebalance_equals_the_whole_table(oracle, tmp_path, world, seed, max_moves, rounds):
    n, m = 3000, 14
    port = _free_port()
    mp.spawn(_worker, args=(world, port, seed, n, m, max_moves, rounds, str(tmp_path)), nprocs=world, join=True)
    cur, load, aff, cap, alive, T = _gloo_case(seed, n, m)
    want, used, wst, wrows, wfrom, wto = rebalance_ref.rebalance(cur, load, aff, cap, alive, target=T, max_moves=max_moves,
                                                                 rounds=rounds)
    zs = [np.load(os.path.join(str(tmp_path), "r%d.npz" % r)) for r in range(world)]
    assert np.array_equal(np.concatenate([z["a"] for z in zs]), want)
    for z in zs:
        assert np.array_equal(z["used"], used)
        assert [int(v) for v in z["st"]] == [wst[k] for k in sorted(wst)]
    # every process lists the moves of its own shard with global row numbers: concatenated in rank order = the whole list
    assert np.array_equal(np.concatenate([z["rows"] for z in zs]), wrows)
    assert np.array_equal(np.concatenate([z["frm"] for z in zs]), wfrom)
    assert np.array_equal(np.concatenate([z["to"] for z in zs]), wto)
    assert wst["moved_rows"] > 0
