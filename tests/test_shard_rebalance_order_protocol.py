"""The load-ordered cut (R1') of the row-sharded rebalance on the CPU: `ShardedSolver.rebalance(order=1)` drives numpy engines
(tests/shard_rebalance_order_cpu.py) over LocalExchange.  Column, `used` on every rank, counters and moves must equal the
whole-table rebalance by load of both references: tests/rebalance_order_ref.py (two oracle ticks over rows in (load, row) order)
and tests/spec_rebalance_order.py (the rule written out)."""
import inspect

import numpy as np
import pytest

import rebalance_order_ref as oref
import rebalance_ref
import spec_rebalance_order as spec
from rebalance_ref import INF
from test_shard_rebalance_protocol import bounds_for, cut_on_rank0_table

BY_LOAD = oref.BY_LOAD
TIE = 5   # the load of the tied candidates of ties_table


def skewed_table(rng, n, m, hi, kind="tight"):
    """rebalance_ref.random_table's corner cases (pinned rows, dead nodes, unplaced rows, node ids >= m) with skewed loads; the
    tight targets are a random share of each node's own load, so most nodes are over and the thresholds differ."""
    cur, _, aff, alive, _ = rebalance_ref.random_table(rng, n, m, "inf")
    load = oref.skewed_loads(rng, n, hi)
    if kind == "zero":
        return cur, load, aff, alive, np.zeros(m, np.uint64)
    if kind == "inf":
        return cur, load, aff, alive, np.full(m, INF, np.uint64)
    used = np.zeros(m, np.float64)
    on = cur < m
    np.add.at(used, cur[on], load[on].astype(np.float64))
    T = (used * rng.uniform(0.2, 1.3, m)).astype(np.uint64)
    T[rng.random(m) < 0.05] = np.uint64(INF)
    return cur, load, aff, alive, T


def ties_table(ties, keep, rest=2):
    """Three shards.  Node 0 holds, on shard q, ties[q] candidates of load TIE, each followed by a lighter candidate (load 1), a
    zero-load candidate, a heavier one (load 9) and a row of node 1.  T[0] admits the lighter candidates, `keep` of the ties and
    `rest` < TIE more; node 1 takes whatever moves.  Returns the table, the shard bounds and the expected surplus rows."""
    cur, load, b, tie_rows, heavy = [], [], [0], [], []
    for k in ties:
        for _ in range(k):
            tie_rows.append(len(cur))
            heavy.append(len(cur) + 3)
            cur += [0, 0, 0, 0, 1]
            load += [TIE, 1, 0, 9, 2]
        if k == 0:   # a shard without a tie still holds lighter, zero-load and heavier candidates of the node
            heavy.append(len(cur) + 2)
            cur += [0, 0, 0, 1]
            load += [1, 0, 9, 2]
        b.append(len(cur))
    cur, load = np.array(cur, np.uint32), np.array(load, np.uint32)
    light = int(load[(cur == 0) & (load < TIE)].sum())
    T = np.array([light + TIE * keep + rest, 1 << 40], np.uint64)
    cap = np.full(2, INF, np.uint64)
    want = sorted(tie_rows[keep:] + heavy)
    return (cur, load, np.zeros(len(cur), np.uint32), cap, np.ones(2, np.uint8), T), b, want


TIE_CASES = {"inside the middle shard": ((4, 5, 3), 6), "at a shard boundary": ((4, 5, 3), 4), "allowance 0": ((4, 5, 3), 0),
             "a shard without a tie": ((3, 0, 4), 5), "only the last tie": ((2, 2, 2), 5)}


def run_sharded(cur, load, aff, cap, alive, b, target, max_moves, rounds, order=BY_LOAD, exchange=None, list_moves=True):
    import sharded
    from shard_rebalance_order_cpu import CpuOrderedRebalanceEngine
    G = len(b) - 1
    engs = [CpuOrderedRebalanceEngine(cur[b[r]:b[r + 1]], load[b[r]:b[r + 1]], aff[b[r]:b[r + 1]], cap, alive) for r in range(G)]
    sol = sharded.ShardedSolver(engs, exchange or sharded.LocalExchange(G))
    st, rows, frm, to = sol.rebalance(target=target, max_moves=max_moves, rounds=rounds, list_moves=list_moves, order=order)
    return engs, st, rows, frm, to


def check_against_references(cur, load, aff, cap, alive, T, max_moves, rounds, engs, st, rows, frm, to):
    want, used, wst, wrows, wfrom, wto = oref.rebalance(cur, load, aff, cap, alive, target=T, max_moves=max_moves, rounds=rounds,
                                                        order=BY_LOAD)
    got = np.concatenate([e.assign for e in engs])
    assert np.array_equal(got, want)
    for e in engs:
        assert np.array_equal(e.used, used)
    assert st == wst
    assert np.array_equal(rows, wrows) and np.array_equal(frm, wfrom) and np.array_equal(to, wto)
    ints = lambda a: [int(v) for v in a]
    snxt, sused, sst, smoves = spec.rebalance(ints(cur), ints(load), ints(aff), ints(cap), ints(alive), target=ints(T),
                                              max_moves=max_moves, rounds=rounds, order=spec.BY_LOAD)
    assert ints(got) == list(snxt) and ints(engs[0].used) == list(sused) and st == sst
    assert [(int(r), int(f), int(t)) for r, f, t in zip(rows, frm, to)] == [tuple(x) for x in smoves]
    return wst


@pytest.mark.parametrize("G", [1, 2, 3, 8])
@pytest.mark.parametrize("shape", ["balanced", "ragged", "empty"])
@pytest.mark.parametrize("hi", [3, 2000, (1 << 32) - 1])
def test_sharded_by_load_equals_the_whole_table(oracle, G, shape, hi):
    rng = np.random.default_rng(1000 * G + 10 * len(shape) + hi % 97)
    n, m = 1500, 12
    cur, load, aff, alive, T = skewed_table(rng, n, m, hi)
    cap = np.full(m, INF, np.uint64)
    b = bounds_for(n, G, shape, rng)
    T9 = np.where(T == np.uint64(INF), T, T // np.uint64(10) * np.uint64(9)).astype(np.uint64)
    surplus = 0
    for target, max_moves, rounds in ((T, 0, 1), (T, 1, 2), (T, n // 50, 4), (T, None, 8), (T9, None, 1),
                                      (np.zeros(m, np.uint64), None, 2), (np.full(m, INF, np.uint64), None, 2)):
        engs, st, rows, frm, to = run_sharded(cur, load, aff, cap, alive, b, target, max_moves, rounds)
        wst = check_against_references(cur, load, aff, cap, alive, target, max_moves, rounds, engs, st, rows, frm, to)
        surplus += wst["surplus_rows"]
    assert surplus > 0


@pytest.mark.parametrize("case", sorted(TIE_CASES))
def test_ties_across_ranks_keep_the_first_in_global_row_order(oracle, case):
    ties, keep = TIE_CASES[case]
    (cur, load, aff, cap, alive, T), b, want = ties_table(ties, keep)
    engs, st, rows, frm, to = run_sharded(cur, load, aff, cap, alive, b, T, None, 2)
    check_against_references(cur, load, aff, cap, alive, T, None, 2, engs, st, rows, frm, to)
    assert list(rows) == want and set(int(t) for t in to) == {1}
    assert st["surplus_rows"] == len(want) and st["nodes_over_after"] == 0
    # ... and a budget that ends among the ties
    engs, st, rows, frm, to = run_sharded(cur, load, aff, cap, alive, b, T, 3, 2)
    check_against_references(cur, load, aff, cap, alive, T, 3, 2, engs, st, rows, frm, to)
    assert list(rows) == want[:3]


def test_zero_load_candidates_behind_the_cut_are_never_surplus(oracle):
    """The table on which R1 makes the zero-load candidates of ranks 1 and 2 surplus: by load they sort in front of every cut."""
    cur, load, aff, cap, alive, b = cut_on_rank0_table()
    engs, st, rows, frm, to = run_sharded(cur, load, aff, cap, alive, b, cap, None, 2)
    check_against_references(cur, load, aff, cap, alive, cap, None, 2, engs, st, rows, frm, to)
    assert list(rows) == [2] and st["surplus_rows"] == 1 and st["surplus_load"] == 6
    assert [int(e.rb_surplus.sum()) for e in engs] == [1, 0, 0]
    engs, st, rows, frm, to = run_sharded(cur, load, aff, cap, alive, b, cap, None, 2, order=0)
    assert list(rows) == [2, 6, 8, 10, 13]


def test_order_zero_through_the_ordered_begin_is_the_row_order_protocol(oracle):
    import sharded
    from shard_rebalance_cpu import CpuRebalanceEngine
    rng = np.random.default_rng(9)
    n, m, G = 1200, 10, 3
    cur, load, aff, alive, T = skewed_table(rng, n, m, 2000)
    cap = np.full(m, INF, np.uint64)
    b = bounds_for(n, G, "ragged", rng)
    engs, st, rows, frm, to = run_sharded(cur, load, aff, cap, alive, b, T, 200, 2, order=0)
    old = [CpuRebalanceEngine(cur[b[r]:b[r + 1]], load[b[r]:b[r + 1]], aff[b[r]:b[r + 1]], cap, alive) for r in range(G)]
    ost, orows, ofrm, oto = sharded.ShardedSolver(old, sharded.LocalExchange(G)).rebalance(target=T, max_moves=200, rounds=2)
    assert st == ost and np.array_equal(rows, orows) and np.array_equal(frm, ofrm) and np.array_equal(to, oto)
    for e, o in zip(engs, old):
        assert np.array_equal(e.assign, o.assign) and np.array_equal(e.used, o.used)
    want = rebalance_ref.rebalance(cur, load, aff, cap, alive, T, 200, 2)
    assert np.array_equal(np.concatenate([e.assign for e in engs]), want[0]) and st == want[2]


def test_exchange_count_is_three_plus_rounds_plus_passes(oracle):
    """X, one H per threshold pass, the surplus record, used', one Y per round that ran — and the driver's counter gather."""
    import sharded
    rng = np.random.default_rng(5)
    cur, load, aff, alive, T = skewed_table(rng, 900, 10, 2000)
    cap = np.full(10, INF, np.uint64)

    class Counting(sharded.LocalExchange):
        calls = 0

        def all_gather(self, parts):
            Counting.calls += 1
            return super().all_gather(parts)

        def all_gather_into(self, out, parts):
            Counting.calls += 1
            return super().all_gather_into(out, parts)

    b = bounds_for(900, 3, "balanced", rng)
    for target, max_moves, rounds, fixed in ((T, None, 4, None), (np.full(10, INF, np.uint64), None, 4, 1 + 1), (T, 0, 4, 2 + 1)):
        Counting.calls = 0
        engs, st, _, _, _ = run_sharded(cur, load, aff, cap, alive, b, target, max_moves, rounds, exchange=Counting(3))
        passes = engs[0].rb_passes
        if fixed == 2:      # nothing over: X and the counters, no threshold pass
            assert passes == 0 and Counting.calls == 2
        elif fixed == 3:    # a budget of 0: the surplus is still counted, behind the thresholds
            assert passes > 0 and Counting.calls == 2 + passes + 1
        else:
            assert st["selected_rows"] > 0 and 1 <= passes <= 32
            assert 3 + passes + 1 <= Counting.calls <= 3 + rounds + passes + 1, (Counting.calls, passes)
            # the search starts at the first digit, counted from bit 32 down, that reaches into the largest load
            bits, top = engs[0].rb_bits, int(load.max()).bit_length()
            first = -(-32 // bits) - passes
            assert max(32 - (first + 1) * bits, 0) < top and (first == 0 or 32 - first * bits >= top)
        # the plan follows from the gathered X alone: the same on every shard, and the record is no longer than X
        assert len(set((e.rb_passes, e.rb_bits) for e in engs)) == 1
        assert (engs[0].rb_over << engs[0].rb_bits) <= engs[0].words1 or engs[0].rb_bits == 1


def test_steps_out_of_order_are_refused(oracle):
    from shard_rebalance_order_cpu import CpuOrderedRebalanceEngine
    rng = np.random.default_rng(3)
    cur, load, aff, alive, T = skewed_table(rng, 400, 6, 2000)
    cap = np.full(6, INF, np.uint64)
    e = CpuOrderedRebalanceEngine(cur, load, aff, cap, alive)
    x, y = e.new_buffer(e.words1), e.new_buffer(e.words2)
    e.rebalance_begin(0, 1, T, INF, 2, True, x)                       # a row-order session has no threshold passes
    assert e.rebalance_cut(x, y) > 0
    for step in (e.rebalance_threshold_plan, lambda: e.rebalance_threshold_hist(0, y), lambda: e.rebalance_threshold_pick(0, y, y)):
        with pytest.raises(ValueError):
            step()
    e.rebalance_begin(0, 1, T, INF, 2, True, x, order=BY_LOAD)
    assert e.rebalance_cut(x, y) > 0
    passes, words = e.rebalance_threshold_plan()
    h = e.new_buffer(words)
    for step in (lambda: e.rebalance_select(y, y), lambda: e.rebalance_threshold_hist(1, h),
                 lambda: e.rebalance_threshold_pick(0, h, y)):        # select before the picks, a pass ahead, a pick without its hist
        with pytest.raises(ValueError):
            step()
    for p in range(passes):
        e.rebalance_threshold_hist(p, h)
        with pytest.raises(ValueError):
            e.rebalance_threshold_hist(p + 1, h)
        e.rebalance_threshold_pick(p, h, y if p + 1 == passes else None)
    with pytest.raises(ValueError):
        e.rebalance_threshold_hist(passes, h)
    assert e.rebalance_select(y, y)[1] > 0
    assert np.array_equal(e.assign, cur)


def test_the_library_exports_the_new_steps_and_the_binding_drives_them():
    """Fails without the feature on a machine without a GPU too: the exported entry points, their binding, the driver."""
    import rio_gp
    import sharded
    rio_gp.build()
    L = sharded._lib()
    for name in ("begin_ordered", "threshold_plan", "threshold_hist", "threshold_pick"):
        assert getattr(L, "rio_gp_shard_rebalance_" + name).argtypes is not None, name
    assert len(L.rio_gp_shard_rebalance_begin_ordered.argtypes) == len(L.rio_gp_shard_rebalance_begin.argtypes)
    for step in ("threshold_plan", "threshold_hist", "threshold_pick"):
        assert hasattr(sharded.HipShardEngine, "rebalance_" + step)
    assert "order" in inspect.signature(sharded.HipShardEngine.rebalance_begin).parameters
    assert inspect.signature(sharded.ShardedSolver.rebalance).parameters["order"].default == rio_gp.REBALANCE_ROW_ORDER
