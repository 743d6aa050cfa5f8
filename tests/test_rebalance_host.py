"""The string layer's bounded rebalance (rio_op_rebalance) without a GPU: gpu_object_placement.cpp over the host-memory stub
of the dense ABI plus a host rio_gp_rebalance (tests/stub_rio_gp_rebalance.cpp), checked against the plain restatement of the
rule (tests/spec_rebalance.py) and against what lookups and the reverse index say afterwards."""
import ctypes as C
import os
import subprocess
import threading

import pytest

import rio_gp
import spec_rebalance
from test_node_index_host import StubOp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def rblib(tmp_path_factory):
    out = tmp_path_factory.mktemp("stub_rebalance") / "libstub_op_rebalance.so"
    srcs = [os.path.join(ROOT, "rio-rs_amd", "csrc", "gpu_object_placement.cpp"),
            os.path.join(ROOT, "tests", "stub_rio_gp_rebalance.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include")] + srcs +
                   ["-o", str(out)], check=True)
    L = C.CDLL(str(out))
    vp, sz, cp = C.c_void_p, C.c_size_t, C.c_char_p
    L.rio_op_create.argtypes = [vp, C.POINTER(vp)]
    L.rio_op_release.argtypes = [vp]
    L.rio_op_release.restype = None
    L.rio_op_update_n.argtypes = [vp, cp, sz, cp, sz, cp]
    L.rio_op_remove_n.argtypes = [vp, cp, sz, cp, sz]
    L.rio_op_clean_server.argtypes = [vp, cp]
    L.rio_op_set_member.argtypes = [vp, cp, C.c_int, C.c_uint64]
    L.rio_op_get_or_create_placement_n.argtypes = [vp, cp, sz, cp, sz, cp, cp, sz, C.POINTER(C.c_uint32)]
    L.rio_op_lookup_n.argtypes = [vp, cp, sz, cp, sz, cp, sz, C.POINTER(C.c_int)]
    L.rio_op_objects_on_server.argtypes = [vp, cp, C.POINTER(C.c_uint64), C.POINTER(C.POINTER(cp)), C.POINTER(C.POINTER(sz)),
                                           C.POINTER(C.POINTER(cp)), C.POINTER(C.POINTER(sz))]
    L.rio_op_rebalance.argtypes = [vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.POINTER(cp)), C.POINTER(C.POINTER(sz)),
                                   C.POINTER(C.POINTER(cp)), C.POINTER(C.POINTER(sz)), C.POINTER(C.POINTER(cp)),
                                   C.POINTER(C.POINTER(cp))]
    return L


class RbOp(StubOp):
    def member(self, addr, cap, active=True):
        assert self.L.rio_op_set_member(self.h, addr.encode(), int(bool(active)), cap) == 0

    def lookup(self, ty, oid):
        t, i = ty.encode(), oid.encode()
        buf, found = C.create_string_buffer(256), C.c_int(0)
        assert self.L.rio_op_lookup_n(self.h, t, len(t), i, len(i), buf, 256, C.byref(found)) == 0
        return buf.value.decode() if found.value else None

    def rebalance(self, max_moves=INF):
        o = rio_gp._listing_out(2)
        assert self.L.rio_op_rebalance(self.h, max_moves, *map(C.byref, o)) == 0
        return rio_gp._listing(o)


def _fill(op, addrs, keys, rng_pick):
    home = {}
    for k, key in enumerate(keys):
        a = addrs[rng_pick(k)]
        op.update(key[0], key[1], a)
        home[key] = a
    return home


@pytest.mark.parametrize("shadow", [True, False])
@pytest.mark.parametrize("budget", [INF, 1, 25])
def test_moves_lookups_and_reverse_index(rblib, shadow, budget):
    op = RbOp(rblib, 4096, 8, flags=0 if shadow else 8)   # 8: RIO_OP_CFG_NO_HOST_SHADOW
    try:
        addrs = ["h%d:7" % k for k in range(5)]
        for a in addrs:
            op.member(a, INF)
        keys = [("T", "k%d" % k) for k in range(300)] + [("T\0x", "nul\0%d" % k) for k in range(20)]
        home = _fill(op, addrs, keys, lambda k: (k * 7) % 3)       # on the first three servers only
        for key in keys[:50]:
            assert op.lookup(*key) == home[key]                  # the host shadow holds these answers now
        caps = [90, 90, 90, 200, INF]
        for a, c in zip(addrs, caps):
            op.member(a, c)
        # the rule, row by row: rows in first-update order, nodes in membership order, load 1
        cur = [addrs.index(home[k]) for k in keys]
        nxt, _, st, want = spec_rebalance.rebalance(cur, [1] * len(keys), [0] * len(keys), caps, [1] * 5,
                                                    max_moves=None if budget == INF else budget)
        got = op.rebalance(budget)
        assert [(keys[i][0], keys[i][1], addrs[a], addrs[b]) for i, a, b in want] == got
        for ty, oid, f, t in got:
            home[(ty, oid)] = t
        for key in keys:
            assert op.lookup(*key) == home[key]
        for a in addrs:
            assert sorted(op.objects_on_server(a)) == sorted(k for k, v in home.items() if v == a)
    finally:
        op.close()


def test_dead_member_and_removed_keys_do_not_move(rblib):
    op = RbOp(rblib, 1024, 4)
    try:
        op.member("a:1", 10)
        op.member("b:1", 10)
        op.member("c:1", INF)
        keys = [("T", str(k)) for k in range(60)]
        home = _fill(op, ["a:1", "b:1"], keys, lambda k: k % 2)
        op.remove("T", "0")
        op.member("b:1", 10, active=False)
        got = op.rebalance()
        assert got and all(f == "a:1" and t == "c:1" for _, _, f, t in got)
        assert len(got) == 29 - 10   # a:1 keeps 10 of its 29 remaining objects
        assert op.lookup("T", "0") is None and op.lookup("T", "1") == "b:1"
    finally:
        op.close()


def test_concurrent_callers(rblib):
    """Lookups and updates from several threads while another rebalances: every answer is an address the key had."""
    op = RbOp(rblib, 8192, 8)
    try:
        addrs = ["s%d:1" % k for k in range(4)]
        for a in addrs:
            op.member(a, INF)
        keys = [("T", str(k)) for k in range(2000)]
        _fill(op, addrs, keys, lambda k: 0 if k % 5 else 1)
        for a, c in zip(addrs, [300, 700, 700, 700]):
            op.member(a, c)
        stop, bad = threading.Event(), []

        def reader(seed):
            k = seed
            while not stop.is_set():
                key = keys[k % len(keys)]
                if op.lookup(*key) not in addrs:
                    bad.append(key)
                k += 7

        ts = [threading.Thread(target=reader, args=(s,)) for s in range(4)]
        for t in ts:
            t.start()
        moved = []
        for _ in range(5):
            moved += op.rebalance(200)
        stop.set()
        for t in ts:
            t.join()
        assert not bad and moved
        assert len(moved) == 1000 and len(op.objects_on_server("s0:1")) == 1600 - 1000
    finally:
        op.close()
