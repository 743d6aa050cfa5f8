"""Rule 13 of DESIGN.md section 2 (immovable classes): the row-by-row restatement (tests/spec_movable.py) against the
restatement of rule 6 (tests/spec_rebalance_order.py) under the equivalence the rule states — the same table with the affinity
of every immovable object row read as RIO_GP_AFF_INACTIVE — and the consequences the rule lists.  No GPU."""
import numpy as np
import pytest

import movable_tables as mt
import spec_movable as spec
import spec_rebalance_order as plain

SIZES = [(n, m) for n in (5, 63, 257, 4097, 8193) for m in (2, 3, 8, 33)]


def _lists(t):
    return (t["cur"].tolist(), t["load"].tolist(), t["aff"].tolist(), t["cls"].tolist(), t["movable"].tolist(),
            [mt.INF] * len(t["alive"]), t["alive"].tolist(), t["T"].tolist())


def _by_the_affinity_trick(t, budget, rounds, order):
    aff = t["aff"].copy()
    aff[mt.immovable_rows(t)] = mt.INACTIVE
    cur, load, _, _, _, cap, alive, T = _lists(t)
    return plain.rebalance(cur, load, aff.tolist(), cap, alive, T, budget, rounds, order=order)


def _plain(t, budget, rounds, order):
    cur, load, aff, _, _, cap, alive, T = _lists(t)
    return plain.rebalance(cur, load, aff, cap, alive, T, budget, rounds, order=order)


def _cases():
    """40 tables per size of the first three n, fewer of the large ones: 20 sizes, 800 cases with the orders and budgets"""
    for n, m in SIZES:
        for rep in range(4 if n > 1000 else 12):
            yield n, m, rep


def test_equals_rule_6_with_immovable_rows_read_as_non_objects_and_the_table_matters():
    """Random parity in both orders with budgets None, 0 and a small one; no immovable row is ever moved; and in at least a
    fifth of the cases the plain rule DOES move an immovable row, so an implementation that ignores the table cannot pass."""
    cases = planted = differs = 0
    for n, m, rep in _cases():
        rng = np.random.default_rng(1000 * n + 10 * m + rep)
        t = mt.random_table(rng, n, m)
        imm = mt.immovable_rows(t)
        cur, load, aff, cls, movable, cap, alive, T = _lists(t)
        for order in (spec.ROW_ORDER, spec.BY_LOAD):
            for budget in (None, 0, 1 + rep):
                rounds = 1 + rep % 3
                got = spec.rebalance(cur, load, aff, cls, movable, cap, alive, T, budget, rounds, order)
                want = _by_the_affinity_trick(t, budget, rounds, order)
                assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2] and got[3] == want[3], (n, m, rep, order, budget)
                assert not any(imm[r] for r, _, _ in got[3])
                nxt = np.array(got[0], np.uint32)
                assert np.array_equal(nxt[imm], t["cur"][imm])
                p = _plain(t, budget, rounds, order)
                cases += 1
                planted += any(imm[r] for r, _, _ in p[3])
                differs += p[0] != got[0]
    assert cases >= 400
    assert 5 * planted >= cases, (planted, cases)     # the floor: the plain rule moves an immovable row in >= 1/5 of the cases
    assert differs >= planted


def test_every_class_movable_is_the_plain_rule():
    for n, m, rep in _cases():
        rng = np.random.default_rng(7 * n + m + rep)
        t = mt.random_table(rng, n, m, frac_immovable=0.0)
        assert t["movable"].all()
        cur, load, aff, cls, movable, cap, alive, T = _lists(t)
        for order in (0, 1):
            for movable_arg in (movable, []):            # an all-movable table, and none at all
                got = spec.rebalance(cur, load, aff, cls, movable_arg, cap, alive, T, 2 + rep, 2, order)
                assert got == _plain(t, 2 + rep, 2, order)


def test_classes_at_or_above_n_classes_are_movable():
    rng = np.random.default_rng(5)
    t = mt.random_table(rng, 300, 4, n_classes=7)
    t["movable"][:] = 0
    cur, load, aff, cls, movable, cap, alive, T = _lists(t)
    _, _, _, moves = spec.rebalance(cur, load, aff, cls, movable, cap, alive, T)
    assert moves and all(cls[r] >= 7 for r, _, _ in moves)
    assert any(cls[r] == 255 for r, _, _ in moves)


def test_every_class_immovable_nothing_is_surplus_nothing_moves():
    rng = np.random.default_rng(6)
    t = mt.random_table(rng, 500, 5, n_classes=256)
    t["movable"][:] = 0
    cur, load, aff, cls, movable, cap, alive, T = _lists(t)
    for order in (0, 1):
        nxt, used, st, moves = spec.rebalance(cur, load, aff, cls, movable, cap, alive, T, order=order)
        assert nxt == cur and not moves and st["surplus_rows"] == 0 and st["selected_rows"] == 0
        assert st["nodes_over_after"] == st["nodes_over_before"] > 0


@pytest.mark.parametrize("order", [0, 1])
def test_immovable_load_counts_against_the_target(order):
    """A node whose immovable load alone reaches T has free = 0: in row order every candidate from the first with load > 0 on
    is surplus, by load every candidate with load > 0."""
    cur = [0] * 8 + [1]
    load = [5, 0, 1, 0, 2, 3, 0, 4, 1]
    cls = [3, 0, 0, 0, 0, 0, 0, 0, 0]
    aff = [0] * 9
    movable = [1, 1, 1, 0]
    nxt, used, st, moves = spec.rebalance(cur, load, aff, cls, movable, [mt.INF, mt.INF], [1, 1], [5, 100], order=order)
    want = [2, 3, 4, 5, 6, 7] if order == 0 else [2, 4, 5, 7]
    assert st["surplus_rows"] == len(want) and [r for r, _, _ in moves] == want
    assert nxt[0] == 0 and st["nodes_over_after"] == 0


def test_an_immovable_rows_node_is_still_a_fill_target_and_used_includes_the_row():
    cur = [0, 1, 1, 1]
    load = [3, 4, 4, 4]
    cls = [1, 0, 0, 0]
    nxt, used, st, moves = spec.rebalance(cur, load, [0] * 4, cls, [1, 0], [mt.INF] * 2, [1, 1], [8, 4])
    assert moves == [(2, 1, 0)] and used == [7, 8] and st["stayed_rows"] == 1 and nxt == [0, 1, 0, 1]


def test_the_directed_case_of_the_issue():
    cur = [0] * 8 + [1, 1]
    cls = [1, 0, 1, 0, 1, 0, 1, 0, 0, 0]
    args = (cur, [1] * 10, [0] * 10, cls)
    caps, alive, T = [mt.INF] * 2, [1, 1], [4, 8]
    assert spec.rebalance(*args, [1, 0], caps, alive, T)[3] == [(r, 0, 1) for r in (1, 3, 5, 7)]
    assert spec.rebalance(*args, [1, 1], caps, alive, T)[3] == [(r, 0, 1) for r in (4, 5, 6, 7)]
