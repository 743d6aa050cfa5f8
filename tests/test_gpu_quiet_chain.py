"""Quiet committed ticks as one launch each: the chained k_scan adds every node's kept load into the tick's `used` buffer (a ring
of four, zeroed two links ahead) and stores the tick's verdict rows itself — no k_resolve behind it.  Runs longer than the ring of
ticks, at sizes that cover both plans (the smallest chained table, a ragged last tile, a table beyond the Infinity Cache), every
kind of change right in front of a quiet run, and two handles of one process taking turns on one device.  Every tick's counters,
the column and `used` are compared with the oracle chain."""
import time

import numpy as np
import pytest

import synth

NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


def _mk(gp, n, m, load, aff, cap, alive, cur, lab=True):
    g = gp.GpuPlacement(n, m, spill_rounds=2, lab=lab)
    g.set_nodes(cap, alive, m=m)
    g.set_objects(n, load, aff)
    g.set_assign(cur)
    return g


def _settle(g, oracle, ref, load, aff, cap, alive):
    """Ticks until one has left every object placed and its verdict has landed: what follows is quiet.  Returns the
    oracle's fixed point (table, `used`, counters of a quiet tick) and the counters of the settling ticks."""
    want = []
    for _ in range(3):
        g.tick_async()
        ref, used, ost = oracle.tick(ref, load, aff, cap, alive, 2)
        want.append(ost)
        time.sleep(0.01)
    got = g.tick_wait()
    assert got == want
    q, qused, qst = oracle.tick(ref, load, aff, cap, alive, 2)
    assert np.array_equal(q, ref) and qst["slow_path"] == 0     # (the oracle chain's fixed point)
    return ref, qused, qst


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1 << 18, 1_000_000, (1 << 22) + 12_345, 10_000_000])
def test_quiet_runs_longer_than_the_tick_ring(gp, oracle, n):
    cfg = synth.config("c3", n_override=n)
    m = cfg["m"]
    load, aff, cap = cfg["load"], cfg["aff"], cfg["cap"]
    alive = synth.churn_mask(m, 5)                       # some dead nodes: the kept rule reads the bitmap
    g = _mk(gp, n, m, load, aff, cap, alive, synth.warm_assign(n, m))
    ref, used, qst = _settle(g, oracle, synth.warm_assign(n, m), load, aff, cap, alive)
    c0 = g.chained_scans()
    for run in range(2):
        for _ in range(150):                             # past the ring of 64 ticks: harvested in the middle of the run
            g.tick_async()
        got = g.tick_wait()
        assert len(got) == 150 and all(s == qst for s in got), (run, [s for s in got if s != qst][:2], qst)
        assert np.array_equal(g.get_assign(), ref), run
        assert np.array_equal(g.get_nodes()[2], used), run
    assert g.chained_scans() - c0 >= 2 * 140, g.chained_scans() - c0
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lab", [False, True])
def test_a_quiet_run_right_behind_every_kind_of_change(gp, oracle, lab):
    cfg = synth.config("c3", n_override=600_000)
    n, m = cfg["n"], cfg["m"]
    load, aff, cap = cfg["load"].copy(), cfg["aff"].copy(), cfg["cap"]
    alive = np.ones(m, np.uint8)
    ref = synth.warm_assign(n, m)
    g = _mk(gp, n, m, load, aff, cap, alive, ref, lab=lab)
    rng = np.random.default_rng(7)
    want = []

    def ticks(k):
        nonlocal ref, used
        for _ in range(k):
            g.tick_async()
            ref, used, ost = oracle.tick(ref, load, aff, cap, alive, 2)
            want.append(ost)
            time.sleep(0.002)        # verdicts land: the quiet rule is in force when the next change arrives

    def changes():
        nonlocal ref, alive
        alive = synth.churn_mask(m, 9); g.set_alive_all(alive); yield "liveness"
        idx = rng.choice(n, 20_000, replace=False).astype(np.uint32)
        g.remove_batch(idx); ref[idx] = NONE; yield "remove"
        idx = rng.choice(n, 30_000, replace=False).astype(np.uint32)
        g.update_batch(idx, np.full(idx.size, 3, np.uint32)); ref[idx] = 3; yield "update"
        idx = rng.choice(n, 10_000, replace=False).astype(np.uint32)
        load[idx] = rng.integers(0, 500, idx.size).astype(np.uint32); aff[idx] = rng.integers(0, m, idx.size).astype(np.uint32)
        g.set_object_attrs(idx, load[idx], aff[idx]); yield "attributes"
        ref = synth.warm_assign(n, m, stream=4); ref[::9] = NONE; g.set_assign(ref); yield "set_assign"
        ev = g.clean_server(int(np.flatnonzero(alive)[0])); ref[ref == int(np.flatnonzero(alive)[0])] = NONE; assert ev > 0; yield "clean_server"
        idx = np.flatnonzero(ref == NONE)[:4000].astype(np.uint32)
        u = oracle.recompute_used(ref, load, m)
        req = np.flatnonzero(alive)[rng.integers(0, int(alive.sum()), idx.size)].astype(np.uint32)
        node, flag = g.place_pending(idx, req)
        wnode, wflag = oracle.place_pending(ref, load, cap, alive, u, idx, req)
        assert np.array_equal(node, wnode) and np.array_equal(flag, wflag); yield "place_pending"

    used = None
    ticks(3)
    for what in changes():
        ticks(3)                     # the tick that takes the change, then the first quiet ones
        ticks(20)                    # a quiet run
        assert np.array_equal(g.get_assign(), ref), what
        assert np.array_equal(g.get_nodes()[2], used), what
    got = g.tick_wait()
    assert len(got) == len(want)
    for k in range(len(want)):
        assert got[k] == want[k], (k, got[k], want[k])
    if lab:
        assert g.chained_scans() > 7 * 15, g.chained_scans()
    g.close()


@pytest.mark.gpu
def test_two_handles_take_turns_with_quiet_runs(gp, oracle):
    """One chain per process and device: a handle's run ends at its next synchronous entry; the other handle's quiet run
    then chains in its turn."""
    hs = []
    for k in range(2):
        cfg = synth.config("c3", n_override=(1 << 20) + 777 * k)
        n, m = cfg["n"], cfg["m"]
        alive = np.ones(m, np.uint8) if k == 0 else synth.churn_mask(m, 31)
        g = _mk(gp, n, m, cfg["load"], cfg["aff"], cfg["cap"], alive, synth.warm_assign(n, m, stream=k + 2))
        ref, used, qst = _settle(g, oracle, synth.warm_assign(n, m, stream=k + 2), cfg["load"], cfg["aff"], cfg["cap"], alive)
        hs.append((g, ref, used, qst))
    for turn in range(6):
        g, ref, used, qst = hs[turn % 2]
        c0 = g.chained_scans()
        for _ in range(70):
            g.tick_async()
        got = g.tick_wait()
        assert len(got) == 70 and all(s == qst for s in got), turn
        assert np.array_equal(g.get_assign(), ref) and np.array_equal(g.get_nodes()[2], used), turn
        assert g.chained_scans() - c0 >= 60, (turn, g.chained_scans() - c0)
    for g, *_ in hs:
        g.close()
