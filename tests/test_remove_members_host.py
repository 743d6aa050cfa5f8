"""The string layer's node removal (rio_op_remove_members) without a GPU: gpu_object_placement.cpp over the host-memory stub of the
dense ABI plus a host rio_gp_remap_nodes (tests/stub_rio_gp_remap.cpp).  A random call sequence runs through two clones of one
provider; after every call the lookups, the snapshot, the per-server listings, the feed's mirror and rio_op_node_address of every
id are compared with a plain dict model (Model below: the stub's capacity-free policy).  Fixed cases: a full node table takes a
new address again after a removal, pointers handed out by rio_op_node_address outlive the removal, a removed address comes back
empty, and a dense layer without the call answers RIO_GP_EUPSTREAM and changes nothing."""
import ctypes as C
import os
import random
import subprocess

import pytest

import rio_gp
from test_node_index_host import StubOp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_LOCAL, FLAG_REDIRECT, FLAG_PLACED, FLAG_REPLACED = 0, 1, 2, 0x10


def _build(tmp, name, stub):
    out = tmp / name
    srcs = [os.path.join(ROOT, "rio-rs_amd", "csrc", "gpu_object_placement.cpp"), os.path.join(ROOT, "tests", stub)]
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include")] + srcs +
                   ["-o", str(out)], check=True)
    L = C.CDLL(str(out))
    vp, sz, cp = C.c_void_p, C.c_size_t, C.c_char_p
    L.rio_op_create.argtypes = [vp, C.POINTER(vp)]
    L.rio_op_clone.argtypes = [vp]
    L.rio_op_clone.restype = vp
    L.rio_op_release.argtypes = [vp]
    L.rio_op_release.restype = None
    L.rio_op_update_n.argtypes = [vp, cp, sz, cp, sz, cp]
    L.rio_op_lookup_n.argtypes = [vp, cp, sz, cp, sz, cp, sz, C.POINTER(C.c_int)]
    L.rio_op_remove_n.argtypes = [vp, cp, sz, cp, sz]
    L.rio_op_clean_server.argtypes = [vp, cp]
    L.rio_op_set_member.argtypes = [vp, cp, C.c_int, C.c_uint64]
    L.rio_op_remove_members.argtypes = [vp, C.c_uint64, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.rio_op_get_or_create_placement_n.argtypes = [vp, cp, sz, cp, sz, cp, cp, sz, C.POINTER(C.c_uint32)]
    L.rio_op_snapshot.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.POINTER(cp)), C.POINTER(C.POINTER(cp)),
                                  C.POINTER(C.POINTER(cp))]
    L.rio_op_snapshot_key_lengths.argtypes = [vp, C.POINTER(C.POINTER(sz)), C.POINTER(C.POINTER(sz))]
    L.rio_op_objects_on_server.argtypes = [vp, cp, C.POINTER(C.c_uint64), C.POINTER(C.POINTER(cp)), C.POINTER(C.POINTER(sz)),
                                           C.POINTER(C.POINTER(cp)), C.POINTER(C.POINTER(sz))]
    L.rio_op_node_address.argtypes = [vp, C.c_uint32]
    L.rio_op_node_address.restype = vp   # the raw pointer: case (b) reads it again after the removal
    L.rio_op_tick.argtypes = [vp, vp]
    L.rio_op_last_error.argtypes = [vp]
    L.rio_op_last_error.restype = cp
    return L


@pytest.fixture(scope="module")
def rmlib(tmp_path_factory):
    L = _build(tmp_path_factory.mktemp("stub_remap"), "libstub_op_remap.so", "stub_rio_gp_remap.cpp")
    rio_gp.bind_op_changes(L)
    return L


@pytest.fixture(scope="module")
def plainlib(tmp_path_factory):
    """the base stub alone: no rio_gp_remap_nodes (nor any other optional call)"""
    return _build(tmp_path_factory.mktemp("stub_plain"), "libstub_op_plain.so", "stub_rio_gp.cpp")


class Op(StubOp):
    """The stub-linked string layer; the calls return their rc where the model predicts a refusal."""

    def clone(self):
        c = Op.__new__(Op)
        c.L, c.h = self.L, C.c_void_p(self.L.rio_op_clone(self.h))
        return c

    def try_update(self, ty, oid, addr):
        t, i = ty.encode(), oid.encode()
        return self.L.rio_op_update_n(self.h, t, len(t), i, len(i), None if addr is None else addr.encode())

    def try_set_member(self, addr, active):
        return self.L.rio_op_set_member(self.h, addr.encode(), int(bool(active)), 0xFFFFFFFFFFFFFFFF)

    def try_request(self, ty, oid, me):
        t, i = ty.encode(), oid.encode()
        buf, flag = C.create_string_buffer(256), C.c_uint32(0)
        rc = self.L.rio_op_get_or_create_placement_n(self.h, t, len(t), i, len(i), me.encode(), buf, 256, C.byref(flag))
        return rc, buf.value.decode() or None, flag.value

    def lookup(self, ty, oid):
        t, i = ty.encode(), oid.encode()
        buf, found = C.create_string_buffer(256), C.c_int(0)
        assert self.L.rio_op_lookup_n(self.h, t, len(t), i, len(i), buf, 256, C.byref(found)) == 0
        return buf.value.decode() if found.value else None

    def remove_members(self, addrs):
        enc = [a.encode() for a in addrs]
        arr = (C.c_char_p * max(len(enc), 1))(*enc)
        removed, evicted = C.c_uint64(7), C.c_uint64(7)
        rc = self.L.rio_op_remove_members(self.h, len(enc), arr, C.byref(removed), C.byref(evicted))
        return rc, removed.value, evicted.value

    def node_ptr(self, node):
        return self.L.rio_op_node_address(self.h, node)

    def node_address(self, node):
        p = self.node_ptr(node)
        return None if not p else C.string_at(p).decode()

    def tick(self):
        assert self.L.rio_op_tick(self.h, None) == 0

    def changes(self):
        rc, full, out = rio_gp.op_changes(self.L, self.h)
        assert rc == 0
        return full, out


class Model:
    """What the string layer over the stub computes, in dicts: the node table in id order, who is a member, where every key is,
    and the keys that are objects without a place (a tick found no active member for them)."""

    def __init__(self, max_nodes):
        self.max_nodes = max_nodes
        self.addr = []       # node id -> address
        self.alive = {}      # address -> active member
        self.where = {}      # key -> address
        self.pending = set()

    def full_for(self, a):
        return a not in self.alive and len(self.addr) >= self.max_nodes

    def intern(self, a, up=False):
        if a not in self.alive:
            self.addr.append(a)
            self.alive[a] = up

    def unplace(self, key):
        self.where.pop(key, None)
        self.pending.discard(key)

    def update(self, key, a):
        if a is None:
            return self.unplace(key)
        self.intern(a)
        self.where[key] = a
        self.pending.discard(key)

    def clean(self, a):
        gone = [k for k, v in self.where.items() if v == a]
        for k in gone:
            del self.where[k]
        return len(gone)

    def request(self, key, me):
        self.intern(me, up=True)
        at = self.where.get(key)
        if at is not None and self.alive[at]:
            return at, FLAG_LOCAL if at == me else FLAG_REDIRECT
        rep = 0
        if at is not None:                 # service.rs:227-237: the server it sits on is not active — clean it, every object
            self.clean(at)
            rep = FLAG_REPLACED
        self.where[key] = me               # service.rs:244-252: first touch on the requester, whatever membership says
        self.pending.discard(key)
        return me, FLAG_PLACED | rep

    def tick(self):
        first = next((a for a in self.addr if self.alive[a]), None)
        for k in [k for k, v in self.where.items() if not self.alive[v]]:
            del self.where[k]
            self.pending.add(k)
        if first is not None:
            for k in self.pending:
                self.where[k] = first
            self.pending.clear()

    def remove_members(self, addrs):
        gone = [a for a in dict.fromkeys(addrs) if a in self.alive]
        ev = sum(self.clean(a) for a in gone)
        for a in gone:
            del self.alive[a]
        self.addr = [a for a in self.addr if a in self.alive]
        return len(gone), ev


def apply_listing(mirror, full, entries):
    """One rio_op_changes listing applied to {key: address}: deletes first (an old address of None on a delete: the server was
    removed), every old address that is known is the mirror's."""
    m = {} if full else dict(mirror)
    upserts = False
    for ty, oid, old, new in entries:
        key = (ty, oid)
        if new is None:
            assert not upserts and not full and key in m, (key, old)
            assert old is None or m[key] == old, (key, m[key], old)
            del m[key]
        else:
            upserts = True
            assert old is None or m.get(key) == old, (key, m.get(key), old)
            m[key] = new
    return m


def check(op, md, keys, addrs):
    for ty, oid in keys:
        assert op.lookup(ty, oid) == md.where.get((ty, oid)), (ty, oid)
    assert {(t, i): a for t, i, a in op.snapshot()} == md.where
    for k in range(md.max_nodes + 1):
        assert op.node_address(k) == (md.addr[k] if k < len(md.addr) else None), k
    for a in addrs:
        assert sorted(op.objects_on_server(a)) == sorted(k for k, v in md.where.items() if v == a), a


@pytest.mark.parametrize("shadow", [True, False])
@pytest.mark.parametrize("seed", range(5))
def test_random_calls_through_two_clones_match_the_model(rmlib, seed, shadow):
    rng = random.Random(seed)
    max_nodes = 6
    a = Op(rmlib, 256, max_nodes, flags=0 if shadow else 8)   # 8: RIO_OP_CFG_NO_HOST_SHADOW
    ops = [a, a.clone()]
    md = Model(max_nodes)
    addrs = ["h%d:7" % k for k in range(9)]                   # more addresses than ids: the table fills, removals free it
    keys = [("T%d" % (i % 3), "o%d" % i) for i in range(40)]
    mirror, fed = {}, False
    try:
        for it in range(260):
            op = ops[rng.randrange(2)]
            k = rng.randrange(12)
            key = rng.choice(keys)
            ad = rng.choice(addrs)
            if k <= 2:
                rc = op.try_update(key[0], key[1], ad)
                if md.full_for(ad):
                    assert rc == rio_gp.EINVAL
                else:
                    assert rc == 0
                    md.update(key, ad)
            elif k == 3:
                if rng.random() < 0.5:
                    assert op.try_update(key[0], key[1], None) == 0
                else:
                    op.remove(key[0], key[1])
                md.unplace(key)
            elif k <= 5:
                rc, got, flag = op.try_request(key[0], key[1], ad)
                if md.full_for(ad):
                    assert rc == rio_gp.EINVAL
                else:
                    assert rc == 0 and (got, flag) == md.request(key, ad), it
            elif k == 6:
                act = rng.random() < 0.6
                rc = op.try_set_member(ad, act)
                if md.full_for(ad):
                    assert rc == rio_gp.EINVAL
                else:
                    assert rc == 0
                    md.intern(ad)
                    md.alive[ad] = act
            elif k == 7:
                op.clean_server(ad)
                md.clean(ad)
            elif k == 8:
                assert op.remove_members([ad]) == (0,) + md.remove_members([ad])
            elif k == 9:
                some = rng.sample(addrs, rng.randrange(0, 5)) + ["never:1"]
                some += some[:1]                                  # one of them twice
                assert op.remove_members(some) == (0,) + md.remove_members(some)
            elif k == 10:
                op.tick()
                md.tick()
            else:
                full, ent = op.changes()
                assert full == (not fed)
                fed = True
                mirror = apply_listing(mirror, full, ent)
                assert mirror == md.where, it
            check(op, md, keys, addrs)
        full, ent = ops[0].changes()
        assert apply_listing(mirror, full, ent) == md.where
    finally:
        for op in ops:
            op.close()


def test_a_full_node_table_takes_a_new_address_after_a_removal(rmlib):
    op = Op(rmlib, 32, 4)
    try:
        for k in range(4):
            assert op.try_update("T", "o%d" % k, "h%d:1" % k) == 0
        assert op.try_update("T", "o4", "h4:1") == rio_gp.EINVAL
        assert b"node table full" in rmlib.rio_op_last_error(op.h)
        assert op.try_set_member("h4:1", True) == rio_gp.EINVAL
        assert op.remove_members(["h1:1"]) == (0, 1, 1)
        assert op.try_update("T", "o4", "h4:1") == 0
        assert op.lookup("T", "o4") == "h4:1" and op.lookup("T", "o1") is None and op.lookup("T", "o3") == "h3:1"
        assert [op.node_address(k) for k in range(5)] == ["h0:1", "h2:1", "h3:1", "h4:1", None]
    finally:
        op.close()


def test_address_pointers_outlive_the_removal(rmlib):
    op = Op(rmlib, 32, 8)
    try:
        for k in range(5):
            op.set_member("host-%d.example:700%d" % (k, k), True)
        before = [op.node_ptr(k) for k in range(5)]
        text = [C.string_at(p) for p in before]
        assert op.remove_members(["host-1.example:7001", "host-3.example:7003"])[:2] == (0, 2)
        for k in range(3):
            op.set_member("late-%d:1" % k, True)                  # the table grows again behind the removal
        assert [C.string_at(p) for p in before] == text           # removed ones included
        assert [op.node_ptr(k) for k in range(3)] == [before[0], before[2], before[4]]   # the kept strings did not move
    finally:
        op.close()


def test_a_removed_address_comes_back_empty_with_a_fresh_id(rmlib):
    op = Op(rmlib, 32, 8)
    try:
        op.set_member("a:1", True)
        op.set_member("b:1", True)
        for k in range(6):
            op.update("T", "o%d" % k, "a:1" if k % 2 else "b:1")
        full, ent = op.changes()
        mirror = apply_listing({}, full, ent)
        assert op.remove_members(["a:1"]) == (0, 1, 3)
        assert op.objects_on_server("a:1") == [] and op.node_address(1) is None and op.node_address(0) == "b:1"
        full, ent = op.changes()
        assert not full and sorted(ent) == [("T", "o%d" % k, None, None) for k in (1, 3, 5)]   # deletes, the old address is gone
        mirror = apply_listing(mirror, full, ent)
        assert op.get_or_create_placement("T", "o1", "a:1") == ("a:1", FLAG_PLACED)
        assert op.node_address(1) == "a:1"
        assert sorted(op.objects_on_server("a:1")) == [("T", "o1")]
        assert op.get_or_create_placement("T", "o0", "a:1") == ("b:1", FLAG_REDIRECT)      # the renumbered node still answers
        full, ent = op.changes()
        assert apply_listing(mirror, full, ent) == {(t, i): a for t, i, a in op.snapshot()}
    finally:
        op.close()


def test_without_the_dense_call_nothing_changes(plainlib):
    op = Op(plainlib, 32, 4)
    try:
        op.set_member("a:1", True)
        op.update("T", "1", "a:1")
        op.update("T", "2", "b:1")
        rc, removed, evicted = op.remove_members(["a:1"])
        assert (rc, removed, evicted) == (rio_gp.EUPSTREAM, 0, 0)
        assert b"dense layer has no node removal" in plainlib.rio_op_last_error(op.h)
        assert op.lookup("T", "1") == "a:1" and op.lookup("T", "2") == "b:1"
        assert [op.node_address(k) for k in range(3)] == ["a:1", "b:1", None]
        assert op.get_or_create_placement("T", "1", "a:1") == ("a:1", FLAG_LOCAL)
        assert op.remove_members(["never:1"])[0] == rio_gp.EUPSTREAM    # the answer does not depend on the addresses
    finally:
        op.close()
