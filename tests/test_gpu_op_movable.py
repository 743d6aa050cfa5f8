"""Immovable types through the real library on the MI355X (rio_op_set_type_movable_n over rio_gp_set_class_movable and the
class-aware passes of rio_gp_rebalance; DESIGN.md section 2 rule 13): the property end to end — a rebalance lists no key of an
immovable type, lookups answer the moved keys' new addresses and the protected keys' old ones — in the fixed cases of
tests/test_movable_host.py and in a random sequence against that file's model, whose rebalance is the row-by-row restatement of
the rule (tests/spec_movable.py)."""
import random

import pytest

from test_movable_host import Rows
from test_remove_members_host import Model

pytestmark = pytest.mark.gpu
INF = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


def _movable(p):
    d = p.dense()
    try:
        return d.get_class_movable().tolist()
    finally:
        d.close()


def _crowd(p, types, per_type):
    p.set_member("a:1", True)
    p.set_member("b:1", True)
    for t in types:
        for k in range(per_type):
            p.update(t, "o%d" % k, "a:1")
    p.set_member("a:1", True, 0)        # capacity 0: every movable key on it is surplus


@pytest.mark.parametrize("order", [0, 1])
def test_protected_keys_stay_and_lookups_answer_the_new_addresses(gp, order):
    p = gp.GpuObjectPlacement(64, 4)
    try:
        _crowd(p, ["Conn", "Plain"], 3)
        p.set_type_movable("Conn", False)
        assert p.rebalance(order=order) == [("Plain", "o%d" % k, "a:1", "b:1") for k in range(3)]
        for k in range(3):
            assert p.lookup("Conn", "o%d" % k) == "a:1" and p.lookup("Plain", "o%d" % k) == "b:1"
        assert _movable(p) == [0] + [1] * 255
        assert p.rebalance(order=order) == []
        p.set_type_movable("Conn", True)                     # movable again: the next rebalance sheds them too
        assert p.rebalance(order=order) == [("Conn", "o%d" % k, "a:1", "b:1") for k in range(3)]
        assert _movable(p) == [1] * 256
        for k in range(3):
            assert p.lookup("Conn", "o%d" % k) == "b:1"
    finally:
        p.close()


def test_a_reclaimed_row_follows_its_new_type(gp):
    p = gp.GpuObjectPlacement(4, 4)
    try:
        _crowd(p, ["A"], 4)
        p.set_type_movable("A", False)
        assert p.rebalance() == []                           # the device knows rows 0-3 as class A, immovable
        for k in range(4):
            p.remove("A", "o%d" % k)
        p.set_member("a:1", True)
        p.update("B", "n0", "a:1")                           # the table is full: the rows of the removed keys are reclaimed
        p.update("A", "n1", "a:1")
        p.update("B", "n2", "a:1")
        p.set_member("a:1", True, 0)
        assert sorted(p.rebalance()) == [("B", "n0", "a:1", "b:1"), ("B", "n2", "a:1", "b:1")]
        assert p.lookup("A", "n1") == "a:1" and p.lookup("B", "n0") == "b:1" and p.lookup("B", "n2") == "b:1"
    finally:
        p.close()


def test_three_hundred_types_and_types_with_nul_bytes(gp):
    p = gp.GpuObjectPlacement(512, 4)
    try:
        p.set_member("a:1", True)
        p.set_member("b:1", True)
        for i in range(300):
            p.update("T%d" % i, "o", "a:1")
        p.set_member("a:1", True, 0)
        for t in ("T255", "T299", "never seen"):
            with pytest.raises(gp.ObjectPlacementError) as e:
                p.set_type_movable(t, False)
            assert e.value.rc == gp.ERANGE
        for i in range(255):
            p.set_type_movable("T%d" % i, False)
        got = p.rebalance()
        assert [ty for ty, _, _, _ in got] == ["T%d" % i for i in range(255, 300)]   # the shared class is always movable
        assert p.lookup("T254", "o") == "a:1" and p.lookup("T0", "o") == "a:1" and p.lookup("T299", "o") == "b:1"
        assert _movable(p) == [0] * 255 + [1]
    finally:
        p.close()
    p = gp.GpuObjectPlacement(16, 4)
    try:
        p.set_member("a:1", True)
        p.set_member("b:1", True)
        p.update("N\0", "x\0y", "a:1")
        p.update("N", "x", "a:1")
        p.update("N\0", "z", "a:1")
        p.set_member("a:1", True, 0)
        p.set_type_movable(b"N\0", False)
        assert p.rebalance() == [("N", "x", "a:1", "b:1")]
        assert p.lookup("N\0", "x\0y") == "a:1" and p.lookup("N\0", "z") == "a:1" and p.lookup("N", "x") == "b:1"
    finally:
        p.close()


@pytest.mark.parametrize("seed", range(3))
def test_a_random_sequence_matches_the_model(gp, seed):
    rng = random.Random(900 + seed)
    p = gp.GpuObjectPlacement(6000, 8)
    md, rw = Model(8), Rows()
    addrs = ["h%d:7" % k for k in range(5)]
    keys = [("T%d" % (i % 7), "o%d" % i) for i in range(5000)] + [("N\0", "x\0y"), ("N", "x"), ("N\0", "z")]
    tnames = ["T%d" % i for i in range(7)] + ["N\0", "N", "never-a-key"]
    moved = protected = 0
    try:
        for ad in addrs:
            p.set_member(ad, True)
            md.intern(ad, up=True)
        for key in keys:                                     # more than a 4 096-row tile of keys, on three of the servers
            ad = rng.choice(addrs[:3])
            p.update(key[0], key[1], ad)
            md.update(key, ad)
            rw.know(key)
        for it in range(60):
            k = 4 if it in (3, 25, 45) else rng.randrange(10)   # (a capacity goes down at least three times)
            key = rng.choice(keys)
            ad = rng.choice(addrs[:3])
            if k <= 1:
                p.update(key[0], key[1], ad)
                md.update(key, ad)
            elif k == 2:
                p.remove(key[0], key[1])
                md.unplace(key)
            elif k == 3:
                rw.load[key] = rng.choice([0, 1, 2, 7, 400])
                p.set_object_load(key[0], key[1], rw.load[key])
            elif k == 4:
                target = rng.choice(addrs[:3])
                placed = sum(rw.load.get(x, 1) for x, v in md.where.items() if v == target)
                rw.cap[target] = rng.choice([placed // 3, placed // 2, placed, 2 * placed + 5])
                p.set_member(target, True, rw.cap[target])
            elif k <= 6:
                t = rng.choice(tnames)
                mv = rng.random() < 0.4
                want = rw.set_movable(t, mv)
                assert want == 0
                p.set_type_movable(t, mv)
            else:
                order = rng.choice([0, 1])
                budget = rng.choice([None, None, 1, 40])
                before = dict(md.where)
                want = rw.rebalance(md, order, INF if budget is None else budget)
                got = p.rebalance(budget, order=order)
                assert got == want, (it, order, budget)
                moved += len(got)
                for ty, oid, f, _ in got:
                    assert rw.key_type[(ty, oid)] not in rw.immovable and before[(ty, oid)] == f
                protected += sum(1 for x, c in rw.key_type.items() if c in rw.immovable and x in md.where)
                for x in rng.sample(keys, 60) + [(ty, oid) for ty, oid, _, _ in got[:40]]:
                    assert p.lookup(x[0], x[1]) == md.where.get(x), (it, x)
        assert {(t, i): x for t, i, x in p.snapshot()} == md.where
        assert moved > 0 and protected > 0
    finally:
        p.close()
