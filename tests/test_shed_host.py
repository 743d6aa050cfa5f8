"""The string layer's shedding under pressure (rio_op_shed_idle) without a GPU: gpu_object_placement.cpp over the host-memory
stub of the dense ABI plus a host rio_gp_shed_idle (tests/stub_rio_gp_shed.cpp).  Keys with stamps, loads and types of every
kind are placed on members with small capacities; every call is compared with a dict model of rule 14 as the header words it
(include/rio_gpu_object_placement.h): the listing in row order with the address each key was on, n_surplus, a type whose idle
limit is RIO_OP_IDLE_NEVER and an immovable type never listed, later lookups "none" for the listed keys and unchanged for the
rest with the host shadow on and off, rio_op_changes listing them as deletes, what goes down to the dense call, and
RIO_GP_EUPSTREAM with nothing changed over a dense layer without the call."""
import ctypes as C
import random

import pytest

import rio_gp
from test_expire_host import ExOp
from test_remove_members_host import _build

NEVER = rio_gp.IDLE_NEVER


def _bind(L):
    rio_gp.bind_op_changes(L)
    rio_gp.bind_op_expire(L)
    rio_gp.bind_op_classes(L)
    rio_gp.bind_op_movable(L)
    rio_gp.bind_op_shed(L)
    L.rio_op_set_object_load_n.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_uint32]
    return L


@pytest.fixture(scope="module")
def shlib(tmp_path_factory):
    L = _bind(_build(tmp_path_factory.mktemp("stub_shed"), "libstub_op_shed.so", "stub_rio_gp_shed.cpp"))
    L.stub_shed_last.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_void_p]
    L.stub_shed_last.restype = None
    return L


@pytest.fixture(scope="module", params=["stub_rio_gp.cpp", "stub_rio_gp_classes.cpp"])
def lacking(request, tmp_path_factory):
    """a dense layer without rio_gp_shed_idle: the base stub (no optional call at all), and the one with expiry and classes"""
    return _bind(_build(tmp_path_factory.mktemp("stub_noshed"), "libstub_op_noshed.so", request.param))


class ShOp(ExOp):
    def clone(self):
        c = ShOp.__new__(ShOp)
        c.L, c.h = self.L, C.c_void_p(self.L.rio_op_clone(self.h))
        return c

    def member(self, addr, capacity):
        assert self.L.rio_op_set_member(self.h, addr.encode(), 1, capacity) == 0

    def set_load(self, ty, oid, load):
        t, i = ty.encode(), oid.encode()
        assert self.L.rio_op_set_object_load_n(self.h, t, len(t), i, len(i), load) == 0

    def shed(self, cutoff, max_objects=None):
        rc, out, surplus = rio_gp.op_shed_idle(self.L, self.h, cutoff, max_objects)
        assert rc == 0
        return out, surplus

    def last_cfg(self):
        cutoff, max_rows, n_classes = C.c_uint32(), C.c_uint64(), C.c_uint32()
        tab = (C.c_uint32 * 256)()
        self.L.stub_shed_last(C.byref(cutoff), C.byref(max_rows), C.byref(n_classes), tab)
        return cutoff.value, max_rows.value, n_classes.value, list(tab)


class Model:
    """Rule 14 over dicts.  Keys in row order = the order of their first interning (the table never fills here)."""

    def __init__(self):
        self.order, self.where, self.stamp, self.load, self.cap = [], {}, {}, {}, {}
        self.never, self.immovable = set(), set()

    def place(self, key, addr, clock):
        if key not in self.order:
            self.order.append(key)
        self.where[key] = addr
        if clock:
            self.stamp[key] = max(self.stamp.get(key, 0), clock)

    def surplus(self, cutoff):
        out = []
        for addr, cap in self.cap.items():
            on = [k for k in self.order if self.where.get(k) == addr]
            cand = [k for k in on if self.load.get(k, 1) >= 1 and self.stamp.get(k, 0) < cutoff and k[0] not in self.never
                    and k[0] not in self.immovable]
            pinned = sum(self.load.get(k, 1) for k in on if k not in cand)
            free = max(cap - pinned, 0)
            pre, over = 0, False
            for k in sorted(cand, key=lambda k: (-self.stamp.get(k, 0), self.order.index(k))):
                pre += self.load.get(k, 1)
                over = over or pre > free
                if over:
                    out.append(k)
        return sorted(out, key=self.order.index)

    def shed(self, cutoff, cap=None):
        sur = self.surplus(cutoff)
        listed = sur if cap is None else sur[:cap]
        out = [(k[0], k[1], self.where[k]) for k in listed]
        for k in listed:
            del self.where[k]
        return out, len(sur)


def _populate(rng, ops, md, n_keys=60):
    addrs = ["h%d:7" % k for k in range(4)]
    for k, ad in enumerate(addrs):
        md.cap[ad] = [6, 9, 4, 1 << 40][k]                  # the last member is never over
        ops[0].member(ad, md.cap[ad])
    keys = [("T%d" % (i % 5), "o%d" % i) for i in range(n_keys)] + [("N\0", "x\0y")]
    clock = 0
    for it, key in enumerate(keys):
        if it % 9 == 8:
            clock += 1
            ops[0].set_clock(clock)
        op = ops[rng.randrange(len(ops))]
        ad = rng.choice(addrs)
        assert op.try_update(key[0], key[1], ad) == 0
        md.place(key, ad, clock)
        if rng.randrange(3) == 0:
            md.load[key] = rng.choice([0, 2, 3])
            op.set_load(key[0], key[1], md.load[key])
    for key in rng.sample(keys, 12):                        # some keys are asked for again later: they are the last to go
        clock += 1
        ops[0].set_clock(clock)
        assert ops[1].lookup(key[0], key[1]) == md.where[key]
        md.stamp[key] = clock
    ops[0].set_clock(0)                                     # stamping off: the lookups that check the outcome leave no stamp
    return keys, clock


def _same(ops, md, keys):
    for key in keys:
        for op in ops:
            assert op.lookup(key[0], key[1]) == md.where.get(key), key


@pytest.mark.parametrize("shadow", [True, False])
@pytest.mark.parametrize("seed", range(4))
def test_shedding_through_two_clones_matches_the_model(shlib, seed, shadow):
    rng = random.Random(seed)
    a = ShOp(shlib, 256, 8, flags=0 if shadow else 8)      # 8: RIO_OP_CFG_NO_HOST_SHADOW
    ops = [a, a.clone()]
    md = Model()
    try:
        keys, clock = _populate(rng, ops, md)
        assert rio_gp.op_set_type_idle_limit(shlib, a.h, "T1", NEVER) == 0
        md.never.add("T1")
        assert rio_gp.op_set_type_idle_limit(shlib, a.h, "T3", 2) == 0      # any other idle limit plays no part
        assert rio_gp.op_set_type_movable(shlib, a.h, "T2", False) == 0
        md.immovable.add("T2")
        cutoff = clock - 5                                  # the keys of the last six lookups are too fresh to go
        a.changes()
        before = dict(md.where)
        out, surplus = ops[1].shed(cutoff, 0)               # count only
        assert out == [] and surplus == len(md.surplus(cutoff)) > 3
        assert md.where == before and a.changes() == (False, [])
        _same(ops, md, keys)
        for cap in (3, None, None):
            want, wsur = md.shed(cutoff, cap)
            op = ops[rng.randrange(2)]
            out, surplus = op.shed(cutoff, cap)
            assert (out, surplus) == (want, wsur), cap
            assert not any(t in ("T1", "T2") for t, _, _ in out)
            _same(ops, md, keys)
            full, ch = a.changes()
            assert not full and ch == [(t, o, ad, None) for t, o, ad in want]
        assert want == [] and wsur == 0                     # the second unlimited call found nothing left
        # the types that held their keys back let go of them
        assert rio_gp.op_set_type_idle_limit(shlib, a.h, "T1", 5) == 0
        md.never.discard("T1")
        assert rio_gp.op_set_type_movable(shlib, a.h, "T2", True) == 0
        md.immovable.discard("T2")
        want, wsur = md.shed(0xFFFFFFFF)
        assert a.shed(0xFFFFFFFF) == (want, wsur) and wsur > 0 and any(t in ("T1", "T2") for t, _, _ in want)
        _same(ops, md, keys)
    finally:
        ops[1].close()
        a.close()


def test_what_goes_down_to_the_dense_call(shlib):
    a = ShOp(shlib, 64, 4)
    try:
        a.member("x:1", 1)
        for i in range(4):
            assert a.try_update("A" if i % 2 else "B", "o%d" % i, "x:1") == 0
        out, surplus = a.shed(7, 2)
        assert len(out) == 2 and surplus == 3
        assert a.last_cfg()[:3] == (7, 2, 0)                # no type needs a table: the plain form, the budget bounded by the rows
        assert rio_gp.op_set_type_idle_limit(shlib, a.h, "A", NEVER) == 0
        out, surplus = a.shed(9)
        cutoff, max_rows, n_classes, tab = a.last_cfg()
        cls = {"B": 0, "A": 1}                              # classes in the order the types were first interned
        assert (cutoff, n_classes) == (9, 256) and tab[cls["A"]] == 0 and tab[cls["B"]] == 9 and tab[255] == 9
        assert all(t == "B" for t, _, _ in out)
    finally:
        a.close()


def test_a_dense_layer_without_the_call_answers_upstream_and_changes_nothing(lacking):
    op = ShOp(lacking, 64, 4)
    try:
        op.member("x:1", 1)
        for i in range(5):
            assert op.try_update("T", "o%d" % i, "x:1") == 0
        for cap in (None, 0):
            rc, out, surplus = rio_gp.op_shed_idle(lacking, op.h, 9, cap)
            assert rc == rio_gp.EUPSTREAM and out == [] and surplus == 0
            assert b"dense layer has no pressure shedding" in lacking.rio_op_last_error(op.h)
        for i in range(5):
            assert op.lookup("T", "o%d" % i) == "x:1"
    finally:
        op.close()
