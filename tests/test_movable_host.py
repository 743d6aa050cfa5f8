"""The string layer's immovable types (rio_op_set_type_movable_n, honoured by rio_op_rebalance / rio_op_rebalance_ordered) without
a GPU: gpu_object_placement.cpp over the host-memory stub of the dense ABI with a host double of the class column and of the
table of DESIGN.md section 2 rule 13 (tests/stub_rio_gp_movable.cpp).  A random call sequence runs through two clones of one
provider — updates, requests, removals, clean_server, capacities, types set immovable and movable again, rebalances in both
orders with and without a budget — and after every call the lookups and the snapshot, and after every rebalance its listing, are
compared with a dict model whose rebalance is the row-by-row restatement of the rule (tests/spec_movable.py) over the model's
rows.  Fixed cases: a reclaimed row that changes type, 300 types (RIO_GP_ERANGE), keys with NUL bytes, a dense layer without
the call (RIO_GP_EUPSTREAM, nothing changed), what a rebalance uploads: nothing while no type is immovable; and the
ThreadSanitizer run of the invariant "a rebalance never lists a key whose type was immovable before the call took its locks"
while other threads place keys, intern new types and flip their flags (tests/host_layer_race_driver_movable.cpp, a program of
its own)."""
import ctypes as C
import os
import random
import shutil
import subprocess

import pytest

import rio_gp
import spec_movable as spec
from test_rebalance_order_host import OrdOp
from test_remove_members_host import Model, _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 0xFFFFFFFFFFFFFFFF
OTHER = rio_gp.CLASS_OTHER


def _bind(L):
    vp, sz, cp = C.c_void_p, C.c_size_t, C.c_char_p
    rio_gp.bind_op_movable(L)
    L.rio_op_set_object_load_n.argtypes = [vp, cp, sz, cp, sz, C.c_uint32]
    outs = [C.POINTER(C.c_uint64), C.POINTER(C.POINTER(cp)), C.POINTER(C.POINTER(sz)), C.POINTER(C.POINTER(cp)),
            C.POINTER(C.POINTER(sz)), C.POINTER(C.POINTER(cp)), C.POINTER(C.POINTER(cp))]
    L.rio_op_rebalance.argtypes = [vp, C.c_uint64] + outs
    L.rio_op_rebalance_ordered.argtypes = [vp, C.c_uint32, C.c_uint64] + outs
    L.rio_op_dense.argtypes = [vp]
    L.rio_op_dense.restype = vp
    return L


@pytest.fixture(scope="module")
def mvlib(tmp_path_factory):
    L = _bind(_build(tmp_path_factory.mktemp("stub_movable"), "libstub_op_movable.so", "stub_rio_gp_movable.cpp"))
    L.stub_mv_calls.argtypes = [C.c_int]
    L.stub_mv_calls.restype = C.c_uint64
    L.rio_gp_get_class_movable.argtypes = [C.c_void_p, C.c_void_p]
    L.rio_gp_get_classes.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def plainlib(tmp_path_factory):
    """the base stub alone: none of the optional dense calls"""
    L = _build(tmp_path_factory.mktemp("stub_plain_mv"), "libstub_op_plain_mv.so", "stub_rio_gp.cpp")
    rio_gp.bind_op_movable(L)
    return L


class MvOp(OrdOp):
    def clone(self):
        c = MvOp.__new__(MvOp)
        c.L, c.h = self.L, C.c_void_p(self.L.rio_op_clone(self.h))
        return c

    def set_movable(self, ty, movable):
        return rio_gp.op_set_type_movable(self.L, self.h, ty, movable)

    def request(self, ty, oid, me):
        return self.get_or_create_placement(ty, oid, me)

    def calls(self):
        """the dense calls so far: (rio_gp_set_classes, rio_gp_set_class_batch, rio_gp_set_class_movable)"""
        return tuple(int(self.L.stub_mv_calls(k)) for k in range(3))

    def dense_movable(self):
        out = (C.c_uint8 * 256)()
        assert self.L.rio_gp_get_class_movable(self.L.rio_op_dense(self.h), out) == 0
        return list(out)


class Rows:
    """What the model needs beside the placement Model: the keys in row order (first interning; the tables here never reclaim),
    type ids as the header numbers them, the immovable types, loads and capacities."""

    def __init__(self):
        self.order, self.ids, self.key_type, self.immovable, self.load, self.cap = [], {}, {}, set(), {}, {}

    def intern(self, ty):
        if ty not in self.ids and len(self.ids) < OTHER:
            self.ids[ty] = len(self.ids)
        return self.ids.get(ty, OTHER)

    def know(self, key):
        if key not in self.key_type:
            self.order.append(key)
            self.key_type[key] = self.intern(key[0])

    def set_movable(self, ty, movable):
        c = self.intern(ty)
        if c == OTHER:
            return rio_gp.ERANGE
        (self.immovable.discard if movable else self.immovable.add)(c)
        return 0

    def rebalance(self, md, order, budget):
        """the moves of rule 13 over the model's rows: [(struct_name, object_id, from, to)]; md.where follows them"""
        node = {a: j for j, a in enumerate(md.addr)}
        cur = [node[md.where[k]] if k in md.where else spec.NONE for k in self.order]
        load = [self.load.get(k, 1) for k in self.order]
        cls = [self.key_type[k] for k in self.order]
        movable = [0 if c in self.immovable else 1 for c in range(256)]
        cap = [self.cap.get(a, INF) for a in md.addr]
        alive = [1 if md.alive[a] else 0 for a in md.addr]
        _, _, _, moves = spec.rebalance(cur, load, [0] * len(cur), cls, movable, cap, alive, None,
                                        None if budget == INF else budget, 2, order or 0)
        out = []
        for r, a, b in moves:
            k = self.order[r]
            out.append((k[0], k[1], md.addr[a], md.addr[b]))
            md.where[k] = md.addr[b]
        return out


@pytest.mark.parametrize("shadow", [True, False])
@pytest.mark.parametrize("seed", range(5))
def test_random_calls_through_two_clones_match_the_model(mvlib, seed, shadow):
    rng = random.Random(500 + seed)
    a = MvOp(mvlib, 256, 8, flags=0 if shadow else 8)   # 8: RIO_OP_CFG_NO_HOST_SHADOW
    ops = [a, a.clone()]
    md, rw = Model(8), Rows()
    addrs = ["h%d:7" % k for k in range(5)]
    keys = [("T%d" % (i % 5), "o%d" % i) for i in range(60)] + [("N\0", "x\0y"), ("N", "x"), ("N\0", "z")]
    tnames = ["T%d" % i for i in range(5)] + ["N\0", "N", "never-a-key"]
    moved_total = protected_total = 0
    try:
        for ad in addrs:
            a.member(ad, INF)
            md.intern(ad, up=True)
        for it in range(260):
            op = ops[rng.randrange(2)]
            k = rng.randrange(16)
            key = rng.choice(keys)
            ad = rng.choice(addrs[:3])                     # the objects arrive on three of the five servers
            if k <= 4:
                op.update(key[0], key[1], ad)
                md.update(key, ad)
                rw.know(key)
            elif k == 5:
                op.remove(key[0], key[1])
                md.unplace(key)
            elif k <= 7:
                got = op.request(key[0], key[1], ad)
                assert got == md.request(key, ad), it
                rw.know(key)
            elif k == 8 and it % 3 == 0:
                op.clean_server(ad)
                md.clean(ad)
            elif k == 9:
                if key in rw.key_type:                     # (a load ahead of the first use would hand out a row: not modelled)
                    rw.load[key] = rng.choice([0, 1, 2, 7, 40])
                    op.set_load(key[0], key[1], rw.load[key])
            elif k == 10:
                target = rng.choice(addrs)
                rw.cap[target] = rng.choice([0, 1, 3, 10, 30, INF])
                op.member(target, rw.cap[target])
            elif k <= 12:
                t = rng.choice(tnames)
                mv = rng.random() < 0.4
                assert op.set_movable(t, mv) == rw.set_movable(t, mv)
            elif k <= 15:
                order = rng.choice([None, 0, 1])
                budget = rng.choice([INF, INF, 1, 4])
                before = dict(md.where)
                want = rw.rebalance(md, order, budget)
                got = op.rebalance(order, budget)
                assert got == want, (it, order, budget)
                moved_total += len(got)
                for ty, oid, f, t2 in got:
                    assert rw.key_type[(ty, oid)] not in rw.immovable and before[(ty, oid)] == f
                protected_total += sum(1 for key2, c in rw.key_type.items() if c in rw.immovable and key2 in md.where)
                assert op.dense_movable() == [0 if c in rw.immovable else 1 for c in range(256)] or not rw.immovable
            for t, oid in keys:
                assert op.lookup(t, oid) == md.where.get((t, oid)), (it, t, oid)
            assert {(t, i): x for t, i, x in op.snapshot()} == md.where
        assert moved_total > 0 and protected_total > 0     # the sequence did rebalance, and with protected keys in place
    finally:
        for op in ops:
            op.close()


def _crowd(op, types, per_type, addr="a:1"):
    """per_type keys of every type on `addr` (capacity 0: everything movable is surplus) and an empty server beside it"""
    op.member(addr, INF)
    op.member("b:1", INF)
    for t in types:
        for k in range(per_type):
            op.update(t, "o%d" % k, addr)
    op.member(addr, 0)


def test_protected_keys_stay_and_lookups_answer_the_new_addresses(mvlib):
    op = MvOp(mvlib, 64, 4)
    try:
        _crowd(op, ["Conn", "Plain"], 3)
        assert op.set_movable("Conn", False) == 0
        got = op.rebalance(1)
        assert got == [("Plain", "o%d" % k, "a:1", "b:1") for k in range(3)]
        for k in range(3):
            assert op.lookup("Conn", "o%d" % k) == "a:1" and op.lookup("Plain", "o%d" % k) == "b:1"
        assert op.rebalance(0) == []
        assert op.set_movable("Conn", True) == 0            # movable again: the next rebalance sheds them too
        assert op.rebalance() == [("Conn", "o%d" % k, "a:1", "b:1") for k in range(3)]
        assert op.dense_movable() == [1] * 256
    finally:
        op.close()


def test_a_rebalance_uploads_nothing_while_no_type_is_immovable(mvlib):
    op = MvOp(mvlib, 64, 4)
    try:
        _crowd(op, ["A", "B"], 2)
        c0 = op.calls()
        assert len(op.rebalance(0, 1)) == 1 and op.calls() == c0          # the untouched path: today's dense calls only
        assert op.set_movable("A", True) == 0 and op.set_movable("never seen", True) == 0
        assert len(op.rebalance(1, 1)) == 1 and op.calls() == c0          # (setting a type movable that already was: no change)
        assert op.set_movable("A", False) == 0
        assert op.calls() == c0                                           # the setter itself makes no dense call
        got = op.rebalance(0)
        c1 = op.calls()
        assert all(ty == "B" for ty, _, _, _ in got)
        assert c1[0] == c0[0] + 1 and c1[1] == c0[1] and c1[2] == c0[2] + 1   # the classes (one range) and the table, once each
        op.update("A", "late", "a:1")
        op.update("B", "late", "a:1")
        assert op.rebalance(0) == [("B", "late", "a:1", "b:1")]
        c2 = op.calls()
        assert c2[0] == c1[0] + 1 and c2[2] == c1[2]                      # the new rows' classes; the table did not change
        assert op.set_movable("A", True) == 0
        assert op.rebalance(0) == [("A", "late", "a:1", "b:1")]           # (A's first two keys left in the budgeted calls above)
        c3 = op.calls()
        assert c3[:2] == c2[:2] and c3[2] == c2[2] + 1                    # the dense table is reset, once; no class upload
        assert op.dense_movable() == [1] * 256
        op.update("A", "later", "a:1")
        assert len(op.rebalance(0)) == 1 and op.calls() == c3             # and the path is the untouched one again
    finally:
        op.close()


def test_a_reclaimed_row_follows_its_new_type(mvlib):
    op = MvOp(mvlib, 4, 4)
    try:
        _crowd(op, ["A"], 4)
        assert op.set_movable("A", False) == 0
        assert op.rebalance() == []                          # the device knows rows 0-3 as class A, immovable
        for k in range(4):
            op.remove("A", "o%d" % k)
        op.member("a:1", INF)
        op.update("B", "n0", "a:1")                          # the table is full: the rows of the removed keys are reclaimed
        op.update("A", "n1", "a:1")
        op.update("B", "n2", "a:1")
        op.member("a:1", 0)
        assert sorted(op.rebalance()) == [("B", "n0", "a:1", "b:1"), ("B", "n2", "a:1", "b:1")]
        assert op.lookup("A", "n1") == "a:1" and op.lookup("B", "n0") == "b:1"
        assert op.set_movable("B", False) == 0 and op.set_movable("A", True) == 0
        op.update("B", "n0", "a:1")
        assert op.rebalance(1) == [("A", "n1", "a:1", "b:1")]
        assert op.lookup("B", "n0") == "a:1"
    finally:
        op.close()


def test_three_hundred_types_the_shared_class_is_always_movable(mvlib):
    op = MvOp(mvlib, 512, 4)
    try:
        op.member("a:1", INF)
        op.member("b:1", INF)
        for i in range(300):
            op.update("T%d" % i, "o", "a:1")
        op.member("a:1", 0)
        assert op.set_movable("T254", False) == 0
        for t in ("T255", "T299", "never seen"):             # (the table of types is full: a new type lands in OTHER too)
            assert op.set_movable(t, False) == rio_gp.ERANGE
            assert b"RIO_OP_CLASS_OTHER" in mvlib.rio_op_last_error(op.h)
        for i in range(254):
            assert op.set_movable("T%d" % i, False) == 0
        got = op.rebalance()
        assert [ty for ty, _, _, _ in got] == ["T%d" % i for i in range(255, 300)]   # nothing was set for the shared class
        assert op.lookup("T254", "o") == "a:1" and op.lookup("T0", "o") == "a:1" and op.lookup("T255", "o") == "b:1"
        assert op.dense_movable() == [0] * 255 + [1]
    finally:
        op.close()


def test_types_with_nul_bytes_travel_with_their_length(mvlib):
    op = MvOp(mvlib, 16, 4)
    try:
        op.member("a:1", INF)
        op.member("b:1", INF)
        op.update("N\0", "x\0y", "a:1")
        op.update("N", "x", "a:1")
        op.update("N\0", "z", "a:1")
        op.member("a:1", 0)
        assert op.set_movable(b"N\0", False) == 0
        assert op.rebalance() == [("N", "x", "a:1", "b:1")]
        assert op.lookup("N\0", "x\0y") == "a:1" and op.lookup("N\0", "z") == "a:1"
        assert op.set_movable(b"N", False) == 0 and op.set_movable(b"N\0", True) == 0
        op.update("N", "x", "a:1")
        assert op.rebalance(1) == [("N\0", "x\0y", "a:1", "b:1"), ("N\0", "z", "a:1", "b:1")]
    finally:
        op.close()


def test_without_the_dense_call_nothing_changes(plainlib):
    op = MvOp(plainlib, 32, 4)
    try:
        op.update("T", "1", "a:1")
        assert op.set_movable("T", False) == rio_gp.EUPSTREAM
        assert b"dense layer has no immovable classes" in plainlib.rio_op_last_error(op.h)
        assert op.set_movable("T", True) == rio_gp.EUPSTREAM and op.set_movable("never seen", False) == rio_gp.EUPSTREAM
        assert op.lookup("T", "1") == "a:1"
    finally:
        op.close()


def test_rebalance_with_immovable_types_under_thread_sanitizer(tmp_path):
    exe = tmp_path / "race_driver_movable"
    srcs = [os.path.join(ROOT, "rio-rs_amd", "csrc", "gpu_object_placement.cpp"), os.path.join(ROOT, "tests", "stub_rio_gp_movable.cpp"),
            os.path.join(ROOT, "tests", "host_layer_race_driver_movable.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", "-I", os.path.join(ROOT, "include")]
                   + srcs + ["-o", str(exe)], check=True)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66")
    # (ThreadSanitizer's runtime can refuse to start under address-space randomisation, before main() runs: not a finding about
    #  the code under test — the run is repeated, without randomisation when setarch is there; tests/test_host_layer_races.py)
    cmd = [str(exe)]
    if shutil.which("setarch"):
        cmd = ["setarch", os.uname().machine, "-R"] + cmd
    for attempt in range(4):
        r = subprocess.run(cmd if attempt < 2 else [str(exe)], capture_output=True, text=True, timeout=600, env=env)
        if "FATAL: ThreadSanitizer" not in r.stderr and not (r.returncode != 0 and not r.stdout and "setarch" in r.stderr):
            break
    assert "WARNING: ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert "wrong=0" in r.stdout and "protected_listed=0" in r.stdout
