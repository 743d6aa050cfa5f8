"""The string layer's load-ordered rebalance (rio_op_rebalance_ordered) without a GPU: gpu_object_placement.cpp over the
host-memory stub of the dense ABI plus a host rio_gp_rebalance that honours cfg.order (tests/stub_rio_gp_rebalance_order.cpp).
It must return the keys and addresses of exactly the dense moves of the rule restated in tests/spec_rebalance_order.py, for both
orders; rio_op_rebalance itself stays row order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rio_gp
import spec_rebalance_order as spec
from test_node_index_host import StubOp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def rolib(tmp_path_factory):
    out = tmp_path_factory.mktemp("stub_rebalance_order") / "libstub_op_rebalance_order.so"
    srcs = [os.path.join(ROOT, "rio-rs_amd", "csrc", "gpu_object_placement.cpp"),
            os.path.join(ROOT, "tests", "stub_rio_gp_rebalance_order.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include")] + srcs +
                   ["-o", str(out)], check=True)
    L = C.CDLL(str(out))
    vp, sz, cp = C.c_void_p, C.c_size_t, C.c_char_p
    L.rio_op_create.argtypes = [vp, C.POINTER(vp)]
    L.rio_op_release.argtypes = [vp]
    L.rio_op_release.restype = None
    L.rio_op_update_n.argtypes = [vp, cp, sz, cp, sz, cp]
    L.rio_op_remove_n.argtypes = [vp, cp, sz, cp, sz]
    L.rio_op_set_member.argtypes = [vp, cp, C.c_int, C.c_uint64]
    L.rio_op_set_object_load_n.argtypes = [vp, cp, sz, cp, sz, C.c_uint32]
    L.rio_op_lookup_n.argtypes = [vp, cp, sz, cp, sz, cp, sz, C.POINTER(C.c_int)]
    L.rio_op_objects_on_server.argtypes = [vp, cp, C.POINTER(C.c_uint64), C.POINTER(C.POINTER(cp)), C.POINTER(C.POINTER(sz)),
                                           C.POINTER(C.POINTER(cp)), C.POINTER(C.POINTER(sz))]
    outs = [C.POINTER(C.c_uint64), C.POINTER(C.POINTER(cp)), C.POINTER(C.POINTER(sz)), C.POINTER(C.POINTER(cp)),
            C.POINTER(C.POINTER(sz)), C.POINTER(C.POINTER(cp)), C.POINTER(C.POINTER(cp))]
    L.rio_op_rebalance.argtypes = [vp, C.c_uint64] + outs
    L.rio_op_rebalance_ordered.argtypes = [vp, C.c_uint32, C.c_uint64] + outs
    return L


class OrdOp(StubOp):
    def member(self, addr, cap, active=True):
        assert self.L.rio_op_set_member(self.h, addr.encode(), int(bool(active)), cap) == 0

    def set_load(self, ty, oid, load):
        t, i = ty.encode(), oid.encode()
        assert self.L.rio_op_set_object_load_n(self.h, t, len(t), i, len(i), load) == 0

    def lookup(self, ty, oid):
        t, i = ty.encode(), oid.encode()
        buf, found = C.create_string_buffer(256), C.c_int(0)
        assert self.L.rio_op_lookup_n(self.h, t, len(t), i, len(i), buf, 256, C.byref(found)) == 0
        return buf.value.decode() if found.value else None

    def rebalance(self, order=None, max_moves=INF, expect=0):
        o = rio_gp._listing_out(2)
        outs = tuple(map(C.byref, o))
        rc = (self.L.rio_op_rebalance(self.h, max_moves, *outs) if order is None
              else self.L.rio_op_rebalance_ordered(self.h, order, max_moves, *outs))
        assert rc == expect
        if rc:
            return None
        return rio_gp._listing(o)


def _setup(op, seed):
    """300 keys (some with NUL bytes) on the first three of five servers, Zipf-like loads with zeros; rows in first-update order."""
    rng = np.random.default_rng(seed)
    addrs = ["h%d:7" % k for k in range(5)]
    for a in addrs:
        op.member(a, INF)
    keys = [("T", "k%d" % k) for k in range(280)] + [("T\0x", "nul\0%d" % k) for k in range(20)]
    loads = np.minimum(rng.zipf(1.4, len(keys)), 500).astype(int)
    loads[rng.random(len(keys)) < 0.1] = 0
    home = {}
    for k, key in enumerate(keys):
        a = addrs[(k * 7) % 3]
        op.update(key[0], key[1], a)
        op.set_load(key[0], key[1], int(loads[k]))
        home[key] = a
    per = int(loads.sum()) // 3
    caps = [per * 6 // 10, per * 6 // 10, per * 9 // 10, per, INF]
    for a, c in zip(addrs, caps):
        op.member(a, c)
    return addrs, keys, loads.tolist(), home, caps


@pytest.mark.parametrize("shadow", [True, False])
@pytest.mark.parametrize("budget", [INF, 1, 25])
@pytest.mark.parametrize("order", [None, 0, 1])
def test_keys_and_addresses_of_exactly_the_dense_moves(rolib, order, budget, shadow):
    op = OrdOp(rolib, 4096, 8, flags=0 if shadow else 8)   # 8: RIO_OP_CFG_NO_HOST_SHADOW
    try:
        addrs, keys, loads, home, caps = _setup(op, 5)
        for key in keys[:50]:
            assert op.lookup(*key) == home[key]            # the host shadow holds these answers now
        cur = [addrs.index(home[k]) for k in keys]
        _, _, st, want = spec.rebalance(cur, loads, [0] * len(keys), caps, [1] * 5, max_moves=None if budget == INF else budget,
                                        order=order or 0)
        got = op.rebalance(order, budget)
        assert want and [(keys[i][0], keys[i][1], addrs[a], addrs[b]) for i, a, b in want] == got
        for ty, oid, f, t in got:
            assert home[(ty, oid)] == f
            home[(ty, oid)] = t
        for key in keys:
            assert op.lookup(*key) == home[key]
        for a in addrs:
            assert sorted(op.objects_on_server(a)) == sorted(k for k, v in home.items() if v == a)
    finally:
        op.close()


def test_by_load_moves_no_object_of_load_zero(rolib):
    moved = {}
    for order in (0, 1):
        op = OrdOp(rolib, 4096, 8)
        try:
            addrs, keys, loads, home, caps = _setup(op, 9)
            got = op.rebalance(order)
            moved[order] = got
            if order == 1:
                ld = dict(zip(keys, loads))
                assert all(ld[(ty, oid)] > 0 for ty, oid, _, _ in got)
        finally:
            op.close()
    assert moved[0] and moved[1] and moved[0] != moved[1]


def test_unknown_order_is_refused_and_changes_nothing(rolib):
    op = OrdOp(rolib, 4096, 8)
    try:
        addrs, keys, loads, home, caps = _setup(op, 2)
        assert op.rebalance(2, expect=rio_gp.EINVAL) is None
        for key in keys:
            assert op.lookup(*key) == home[key]
    finally:
        op.close()
