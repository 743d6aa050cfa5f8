"""Shedding under pressure through the string layer on the MI355X (rio_op_shed_idle over rio_gp_touch_merge, the class uploads
and rio_gp_shed_idle): the scenario of tests/test_shed_host.py — keys with stamps, loads and types of every kind on members with
small capacities, through two clones, with the host shadow on and off — against the same dict model of rule 14: keys and
addresses listed in row order, n_surplus, a type whose idle limit is IDLE_NEVER and an immovable type never listed, later
lookups "none" for the listed keys and unchanged for the rest, the change feed listing them as deletes, and the dense layer's
own state afterwards (the last-seen column uploaded, `used` within the capacities wherever a candidate was left to go)."""
import random

import numpy as np
import pytest

from test_shed_host import Model, _populate, _same

NO_HOST_SHADOW = 8   # RIO_OP_CFG_NO_HOST_SHADOW


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


class GpuOp:
    """The calls the scenario makes, over GpuObjectPlacement."""

    def __init__(self, op):
        self.op = op

    def member(self, addr, capacity):
        self.op.set_member(addr, True, capacity)

    def set_clock(self, now):
        self.op.set_clock(now)

    def try_update(self, ty, oid, addr):
        self.op.update(ty, oid, addr)
        return 0

    def set_load(self, ty, oid, load):
        self.op.set_object_load(ty, oid, load)

    def lookup(self, ty, oid):
        return self.op.lookup(ty, oid)


@pytest.mark.gpu
@pytest.mark.parametrize("shadow", [True, False])
def test_shedding_through_two_clones_matches_the_model(gp, shadow):
    rng = random.Random(17)
    a = gp.GpuObjectPlacement(max_objects=256, max_nodes=8, flags=0 if shadow else NO_HOST_SHADOW)
    b = a.clone()
    ops = [GpuOp(a), GpuOp(b)]
    md = Model()
    try:
        keys, clock = _populate(rng, ops, md)
        a.set_type_idle_limit("T1", gp.IDLE_NEVER)
        md.never.add("T1")
        a.set_type_idle_limit("T3", 2)                       # any other idle limit plays no part
        a.set_type_movable("T2", False)
        md.immovable.add("T2")
        cutoff = clock - 5
        a.changes()
        out, surplus = b.shed_idle(cutoff, 0)                # count only
        assert out == [] and surplus == len(md.surplus(cutoff)) > 3
        assert a.changes() == (False, [])
        _same(ops, md, keys)
        for cap in (3, None, None):
            want, wsur = md.shed(cutoff, cap)
            out, surplus = (a if cap else b).shed_idle(cutoff, cap)
            assert (out, surplus) == (want, wsur), cap
            assert not any(t in ("T1", "T2") for t, _, _ in out)
            _same(ops, md, keys)
            full, ch = a.changes()
            assert not full and sorted(ch) == sorted((t, o, ad, None) for t, o, ad in want)
        assert want == [] and wsur == 0                      # the second unlimited call found nothing left
        g = a.dense()
        cap_, alive, used = g.get_nodes()
        S = g.get_seen()
        assert S.max() == clock and (S > 0).sum() >= 12      # the stamps went down before the cut
        a.set_type_idle_limit("T1", 5)
        md.never.discard("T1")
        a.set_type_movable("T2", True)
        md.immovable.discard("T2")
        want, wsur = md.shed(0xFFFFFFFF)
        assert b.shed_idle(0xFFFFFFFF) == (want, wsur) and wsur > 0 and any(t in ("T1", "T2") for t, _, _ in want)
        _same(ops, md, keys)
        used = g.get_nodes()[2]
        for k, ad in enumerate(md.cap):                      # every key may go now: what is left fits, or weighs nothing less
            on = [key for key in md.order if md.where.get(key) == ad]
            assert int(used[k]) == sum(md.load.get(key, 1) for key in on)
            assert int(used[k]) <= md.cap[ad]
    finally:
        b.close()
        a.close()


@pytest.mark.gpu
def test_count_only_and_a_small_budget(gp):
    op = gp.GpuObjectPlacement(max_objects=64, max_nodes=4)
    try:
        op.set_member("x:1", True, 1)
        op.set_member("y:1", True, 100)
        for i in range(6):
            op.update("T", "o%d" % i, "x:1" if i < 4 else "y:1")
        assert op.shed_idle(0, None) == ([], 0)              # cutoff 0: nobody is idle enough
        assert op.shed_idle(7, 0) == ([], 3)
        assert op.shed_idle(7, 2) == ([("T", "o1", "x:1"), ("T", "o2", "x:1")], 3)
        assert op.shed_idle(7) == ([("T", "o3", "x:1")], 1)
        assert op.shed_idle(7) == ([], 0)
        assert [op.lookup("T", "o%d" % i) for i in range(6)] == ["x:1", None, None, None, "y:1", "y:1"]
    finally:
        op.close()
