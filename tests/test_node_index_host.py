"""The string layer's reverse index (rio_op_objects_on_server) without a GPU: gpu_object_placement.cpp over the host-memory
stub of the dense ABI plus a host rio_gp_rows_on_nodes (tests/stub_rio_gp_index.cpp), driven against
pyoracle.LocalObjectPlacement (tests/node_index_driver.py)."""
import ctypes as C
import os
import subprocess

import pytest

import node_index_driver as drv
import rio_gp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def stublib(tmp_path_factory):
    out = tmp_path_factory.mktemp("stub_index") / "libstub_op_index.so"
    srcs = [os.path.join(ROOT, "rio-rs_amd", "csrc", "gpu_object_placement.cpp"), os.path.join(ROOT, "tests", "stub_rio_gp_index.cpp")]
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
    L.rio_op_snapshot.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.POINTER(cp)), C.POINTER(C.POINTER(cp)),
                                  C.POINTER(C.POINTER(cp))]
    L.rio_op_snapshot_key_lengths.argtypes = [vp, C.POINTER(C.POINTER(sz)), C.POINTER(C.POINTER(sz))]
    L.rio_op_objects_on_server.argtypes = [vp, cp, C.POINTER(C.c_uint64), C.POINTER(C.POINTER(cp)), C.POINTER(C.POINTER(sz)),
                                           C.POINTER(C.POINTER(cp)), C.POINTER(C.POINTER(sz))]
    return L


class _Cfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("max_objects", C.c_uint64), ("max_nodes", C.c_uint32),
                ("spill_rounds", C.c_uint32), ("flags", C.c_uint32), ("collect_ns", C.c_uint32)]


class StubOp:
    """The methods node_index_driver.run needs, over the stub-linked string layer (keys with their lengths)."""

    def __init__(self, L, max_objects, max_nodes, flags=0):
        self.L, self.h = L, C.c_void_p()
        cfg = _Cfg(C.sizeof(_Cfg), 0, max_objects, max_nodes, 0, flags, 0)
        assert L.rio_op_create(C.byref(cfg), C.byref(self.h)) == 0

    def close(self):
        self.L.rio_op_release(self.h)

    def update(self, ty, oid, addr):
        t, i = ty.encode(), oid.encode()
        assert self.L.rio_op_update_n(self.h, t, len(t), i, len(i), None if addr is None else addr.encode()) == 0

    def remove(self, ty, oid):
        t, i = ty.encode(), oid.encode()
        assert self.L.rio_op_remove_n(self.h, t, len(t), i, len(i)) == 0

    def clean_server(self, addr):
        assert self.L.rio_op_clean_server(self.h, addr.encode()) == 0

    def set_member(self, addr, active=True):
        assert self.L.rio_op_set_member(self.h, addr.encode(), int(bool(active)), INF) == 0

    def get_or_create_placement(self, ty, oid, me):
        t, i = ty.encode(), oid.encode()
        buf, flag = C.create_string_buffer(256), C.c_uint32(0)
        assert self.L.rio_op_get_or_create_placement_n(self.h, t, len(t), i, len(i), me.encode(), buf, 256, C.byref(flag)) == 0
        return buf.value.decode() or None, flag.value

    def snapshot(self):
        o = rio_gp._listing_out(1)
        n, ty, tl, oid, il, addr = map(C.byref, o)
        assert self.L.rio_op_snapshot(self.h, n, ty, oid, addr) == 0
        assert self.L.rio_op_snapshot_key_lengths(self.h, tl, il) == 0
        return rio_gp._listing(o)

    def objects_on_server(self, addr):
        o = rio_gp._listing_out(0)
        assert self.L.rio_op_objects_on_server(self.h, addr.encode(), *map(C.byref, o)) == 0
        return rio_gp._listing(o)


@pytest.mark.parametrize("shadow", [True, False])
@pytest.mark.parametrize("seed", range(6))
def test_objects_on_server_equals_the_reference(oracle, stublib, seed, shadow):
    op = StubOp(stublib, drv.MAX_OBJECTS, 16, flags=0 if shadow else 8)   # 8: RIO_OP_CFG_NO_HOST_SHADOW
    try:
        drv.run(op, oracle, seed)
    finally:
        op.close()


def test_unknown_address_and_empty_layer(stublib):
    op = StubOp(stublib, 8, 4)
    try:
        assert op.objects_on_server("nobody:1") == []
        op.update("T", "1", "x:1")
        assert op.objects_on_server("nobody:1") == []
        assert op.objects_on_server("x:1") == [("T", "1")]
    finally:
        op.close()
