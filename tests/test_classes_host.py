"""The string layer's per-type idle limits and census (rio_op_set_type_idle_limit_n / rio_op_expire_by_type / rio_op_census) without
a GPU: gpu_object_placement.cpp over the host-memory stub of the dense ABI with a host double of the object-class calls
(tests/stub_rio_gp_classes.cpp).  A random call sequence runs through two clones of one provider — every stamping call, removals,
clean_server, a moving clock, new types, limits, sweeps with and without a limit, censuses — and after every call the lookups,
the snapshot, the sweep's listing and n_idle and the census are compared with a dict model that keeps type ids, limits and stamps
as the header describes (include/rio_gpu_object_placement.h).  Fixed cases: 300 distinct types (RIO_OP_CLASS_OTHER and the
RIO_GP_ERANGE answer), a reclaimed row that changes type, keys with NUL bytes, the quirk pair ("a.b", "c") / ("a", "b.c"), the
clock at 0, RIO_OP_IDLE_NEVER, now < limit, a dense layer without the calls answering RIO_GP_EUPSTREAM with nothing changed;
and the ThreadSanitizer run of the invariant "a key stamped at or after its type's cutoff before the sweep took its locks is
never listed" while other threads intern new types and set limits (tests/host_layer_race_driver_classes.cpp, a program of its
own)."""
import ctypes as C
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import rio_gp
from test_expire_host import ExOp, Seen
from test_remove_members_host import Model, _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER = rio_gp.IDLE_NEVER
OTHER = rio_gp.CLASS_OTHER


def _bind(L):
    rio_gp.bind_op_changes(L)
    rio_gp.bind_op_expire(L)
    rio_gp.bind_op_classes(L)
    L.rio_op_dense.argtypes = [C.c_void_p]
    L.rio_op_dense.restype = C.c_void_p
    L.rio_op_try_lookup_n.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t,
                                      C.POINTER(C.c_int)]
    L.rio_op_try_get_or_create_placement_n.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p,
                                                       C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32)]
    return L


@pytest.fixture(scope="module")
def clslib(tmp_path_factory):
    L = _bind(_build(tmp_path_factory.mktemp("stub_classes"), "libstub_op_classes.so", "stub_rio_gp_classes.cpp"))
    L.rio_gp_get_classes.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def plainlib(tmp_path_factory):
    """the base stub alone: none of the optional dense calls"""
    L = _build(tmp_path_factory.mktemp("stub_plain_cls"), "libstub_op_plain_cls.so", "stub_rio_gp.cpp")
    rio_gp.bind_op_expire(L)
    rio_gp.bind_op_classes(L)
    return L


class ClsOp(ExOp):
    def clone(self):
        c = ClsOp.__new__(ClsOp)
        c.L, c.h = self.L, C.c_void_p(self.L.rio_op_clone(self.h))
        return c

    def set_limit(self, ty, max_idle):
        return rio_gp.op_set_type_idle_limit(self.L, self.h, ty, max_idle)

    def expire_by_type(self, now, default, max_objects=None):
        rc, out, idle = rio_gp.op_expire_by_type(self.L, self.h, now, default, max_objects)
        assert rc == 0
        return out, idle

    def census(self, by_server=False):
        rc, out = rio_gp.op_census(self.L, self.h, by_server)
        assert rc == 0
        return out

    def dense_classes(self, n):
        """rio_gp_get_classes on rio_op_dense(p): the device's class column as of the last upload; n = the rows handed out"""
        d = self.L.rio_op_dense(self.h)
        out = np.zeros(max(n, 1), np.uint8)
        assert self.L.rio_gp_get_classes(d, n, out.ctypes.data) == 0
        return out[:n]


class Types:
    """Type ids, limits and the sweep the header describes, beside the placement Model and the stamps of Seen."""

    def __init__(self):
        self.ids, self.limit, self.key_type = {}, {}, {}

    def intern(self, ty):
        """the class of struct_name `ty`: the next id while one is left, else OTHER (and the name is not remembered)"""
        if ty not in self.ids and len(self.ids) < OTHER:
            self.ids[ty] = len(self.ids)
        return self.ids.get(ty, OTHER)

    def know(self, key):
        """a key's type is the struct_name of its FIRST interning"""
        if key not in self.key_type:
            self.key_type[key] = self.intern(key[0])

    def set_limit(self, ty, max_idle):
        c = self.intern(ty)
        if c == OTHER:
            return rio_gp.ERANGE
        self.limit[c] = max_idle
        return 0

    def limit_of(self, key, default):
        return self.limit.get(self.key_type[key], default)      # (OTHER never has a limit of its own)

    def expire(self, md, sn, now, default, cap=None):
        idle = [k for k in sn.order if k in md.where and sn.stamp.get(k, 0) + self.limit_of(k, default) < now]
        listed = idle if cap is None else idle[:cap]
        out = [(k[0], k[1], md.where[k]) for k in listed]
        for k in listed:
            del md.where[k]
        return out, len(idle)

    def census(self, md, by_server=False):
        """[(struct_name bytes or None, address or None, rows, load)]: the stub's loads are all 1"""
        names = {c: t.encode() for t, c in self.ids.items()}
        cells = {}
        for k, ad in md.where.items():
            cell = (md.addr.index(ad) if by_server else 0, self.key_type[k])
            cells[cell] = cells.get(cell, 0) + 1
        return [(names.get(c), md.addr[j] if by_server else None, r, r) for (j, c), r in sorted(cells.items())]


@pytest.mark.parametrize("shadow", [True, False])
@pytest.mark.parametrize("seed", range(5))
def test_random_calls_through_two_clones_match_the_model(clslib, seed, shadow):
    rng = random.Random(100 + seed)
    a = ClsOp(clslib, 256, 8, flags=0 if shadow else 8)   # 8: RIO_OP_CFG_NO_HOST_SHADOW
    ops = [a, a.clone()]
    md, sn, ty = Model(8), Seen(), Types()
    addrs = ["h%d:7" % k for k in range(5)]
    keys = [("T%d" % (i % 5), "o%d" % i) for i in range(40)] + [("N\0", "x\0y"), ("N", "x")]
    tnames = ["T%d" % i for i in range(5)] + ["N\0", "N", "never-a-key"]

    def seen(key):
        sn.know(key)
        ty.know(key)
        sn.touch(key)
    try:
        for ad in addrs:
            a.set_member(ad, True)
            md.intern(ad, up=True)
        for it in range(300):
            op = ops[rng.randrange(2)]
            k = rng.randrange(14)
            key = rng.choice(keys)
            ad = rng.choice(addrs)
            if it == 40 or (it > 40 and k == 0):
                sn.clock += rng.randrange(1, 4)           # (the first 40 calls run with the clock at 0: no stamps)
                op.set_clock(sn.clock)
            elif k <= 2:
                assert op.try_update(key[0], key[1], ad) == 0
                md.update(key, ad)
                seen(key)
            elif k == 3:
                op.remove(key[0], key[1])
                md.unplace(key)
            elif k <= 5:
                rc, got, flag = op.try_request(key[0], key[1], ad)
                assert rc == 0 and (got, flag) == md.request(key, ad), it
                seen(key)
            elif k == 6:
                op.clean_server(ad)
                md.clean(ad)
            elif k == 7:
                t = rng.choice(tnames)
                lim = rng.choice([0, 1, 2, 5, NEVER, 0xFFFFFFFE])
                assert op.set_limit(t, lim) == ty.set_limit(t, lim)
            elif k <= 10:
                now = rng.choice([0, 1, sn.clock, sn.clock + 1, sn.clock + 3, 0xFFFFFFFF])
                default = rng.choice([0, 1, 3, NEVER])
                cap = rng.choice([None, 0, 1, 3, 1000])
                if cap == 0:
                    idle = len([x for x in sn.order if x in md.where and sn.stamp.get(x, 0) + ty.limit_of(x, default) < now])
                    assert op.expire_by_type(now, default, 0) == ([], idle)
                else:
                    assert op.expire_by_type(now, default, cap) == ty.expire(md, sn, now, default, cap), it
                # after every sweep the device's class column is the model's type ids, in row order
                want = [ty.key_type[x] for x in sn.order]
                assert op.dense_classes(len(want)).tolist() == want, it
            elif k == 11:
                cutoff = rng.choice([0, sn.clock, sn.clock + 1])
                assert op.expire(cutoff, None) == sn.expire(md, cutoff, None), it   # the plain sweep beside it
            for by_server in (False, True):
                assert op.census(by_server) == ty.census(md, by_server), (it, by_server)
            for t, oid in keys:                          # every lookup stamps what it finds
                got = op.lookup(t, oid)
                assert got == md.where.get((t, oid)), (it, t, oid)
                if got is not None:
                    sn.touch((t, oid))
            assert {(t, i): x for t, i, x in op.snapshot()} == md.where
        out, idle = ops[0].expire_by_type(0xFFFFFFFF, 0)
        assert (out, idle) == ty.expire(md, sn, 0xFFFFFFFF, 0)
    finally:
        for op in ops:
            op.close()


def test_three_hundred_types_share_the_other_class_past_255(clslib):
    op = ClsOp(clslib, 512, 4)
    try:
        for i in range(300):
            op.update("T%d" % i, "o", "a:1")
        assert op.set_limit("T254", 5) == 0
        assert op.set_limit("T255", 5) == rio_gp.ERANGE and op.set_limit("T299", 5) == rio_gp.ERANGE
        assert op.set_limit("never seen", 5) == rio_gp.ERANGE          # the table is full: a new type lands in OTHER too
        assert b"RIO_OP_CLASS_OTHER" in clslib.rio_op_last_error(op.h)
        cen = op.census()
        assert len(cen) == 256 and cen[:255] == [(b"T%d" % i, None, 1, 1) for i in range(255)] and cen[255] == (None, None, 45, 45)
        assert op.census(True)[255] == (None, "a:1", 45, 45)
        assert op.dense_classes(300).tolist() == list(range(255)) + [OTHER] * 45
        op.set_clock(10)
        assert op.set_limit("T0", 3) == 0
        # the clock was 0 when they were written: every stamp is 0.  T0: 0 + 3 < 10; T254: 0 + 5 < 10; the default NEVER keeps the
        # rest, OTHER included (the refused limits were not set)
        assert op.expire_by_type(10, NEVER, 0) == ([], 2)
        assert op.expire_by_type(4, NEVER) == ([("T0", "o", "a:1")], 1)
        # OTHER uses the default
        out, idle = op.expire_by_type(10, 20, 0)
        assert idle == 1
        out, idle = op.expire_by_type(10, 9)
        assert idle == 299 and [o[0] for o in out][-45:] == ["T%d" % i for i in range(255, 300)]
        assert op.census() == []
    finally:
        op.close()


def test_a_reclaimed_row_takes_its_new_keys_class(clslib):
    op = ClsOp(clslib, 4, 4)
    try:
        for k in range(4):
            op.update("A", "o%d" % k, "a:1")
        assert op.census() == [(b"A", None, 4, 4)] and op.dense_classes(4).tolist() == [0, 0, 0, 0]
        for k in range(4):
            op.remove("A", "o%d" % k)
        op.update("B", "n0", "b:1")                          # the table is full: the rows of the removed keys are reclaimed
        op.update("A", "n1", "b:1")
        op.update("B", "n2", "b:1")
        assert op.census() == [(b"A", None, 1, 1), (b"B", None, 2, 2)]
        assert sorted(op.dense_classes(4).tolist()) == [0, 0, 1, 1]   # (the fourth row still carries its old key's class)
        assert op.set_limit("B", 0) == 0
        out, idle = op.expire_by_type(1, NEVER)
        assert sorted(out) == [("B", "n0", "b:1"), ("B", "n2", "b:1")] and idle == 2
        assert op.census(True) == [(b"A", "b:1", 1, 1)]
    finally:
        op.close()


def test_keys_and_types_with_nul_bytes(clslib):
    op = ClsOp(clslib, 16, 4)
    try:
        op.update("N\0", "x\0y", "a:1")
        op.update("N", "x", "a:1")
        op.update("N\0", "z", "a:1")
        assert op.census() == [(b"N\0", None, 2, 2), (b"N", None, 1, 1)]
        assert op.set_limit(b"N\0", 0) == 0                  # the name travels with its length
        assert op.expire_by_type(1, NEVER) == ([("N\0", "x\0y", "a:1"), ("N\0", "z", "a:1")], 2)
        assert op.census() == [(b"N", None, 1, 1)]
    finally:
        op.close()


def test_the_quirk_pair_is_one_key_of_the_type_it_was_first_interned_with(clslib):
    op = ClsOp(clslib, 16, 4)
    try:
        op.update("a.b", "c", "a:1")
        op.update("a", "b.c", "b:1")                         # the same key "a.b.c": no new row, no new type
        assert op.snapshot() == [("a.b", "c", "b:1")]
        assert op.census() == [(b"a.b", None, 1, 1)] and op.dense_classes(1).tolist() == [0]
        assert op.set_limit("a", 0) == 0                     # "a" becomes a type by this call — of no key
        assert op.expire_by_type(5, NEVER) == ([], 0)
        assert op.set_limit("a.b", 0) == 0
        assert op.expire_by_type(5, NEVER) == ([("a.b", "c", "b:1")], 1)
    finally:
        op.close()


def test_clock_zero_never_and_now_below_the_limit(clslib):
    op = ClsOp(clslib, 64, 4)
    try:
        for k in range(3):
            op.update("S", "s%d" % k, "a:1")                 # the clock is 0: nothing is stamped
            op.update("D", "d%d" % k, "a:1")
        assert op.expire_by_type(0, 0, 0) == ([], 0)          # stamp 0 + 0 < 0 never holds
        assert op.expire_by_type(1, 0, 0) == ([], 6)
        assert op.expire_by_type(0xFFFFFFFF, NEVER, 0) == ([], 0)
        assert op.set_limit("S", 5) == 0 and op.set_limit("D", NEVER) == 0
        assert op.expire_by_type(5, 0, 0) == ([], 0)          # now <= limit: cutoff 0, no wrap-around; D never
        assert op.expire_by_type(3, 0, 0) == ([], 0)
        assert op.expire_by_type(6, 0, 0) == ([], 3)
        op.set_clock(100)
        assert op.lookup("S", "s1") == "a:1"                 # stamped 100
        assert op.expire_by_type(105, 0, 0) == ([], 2)        # 100 + 5 < 105 does not hold
        assert op.expire_by_type(106, 0, 0) == ([], 3)
        assert op.expire_by_type(0xFFFFFFFF, 0) == ([("S", "s%d" % k, "a:1") for k in range(3)], 3)
        assert op.census() == [(b"D", None, 3, 3)]
    finally:
        op.close()


def test_without_the_dense_calls_nothing_changes(plainlib):
    op = ClsOp(plainlib, 32, 4)
    try:
        op.update("T", "1", "a:1")
        op.set_clock(3)
        assert op.set_limit("T", 0) == 0                     # (the limit is the host's: no dense call)
        rc, out, idle = rio_gp.op_expire_by_type(plainlib, op.h, 0xFFFFFFFF, 0)
        assert rc == rio_gp.EUPSTREAM and b"dense layer has no object classes" in plainlib.rio_op_last_error(op.h)
        assert rio_gp.op_expire_by_type(plainlib, op.h, 5, 0, 0)[0] == rio_gp.EUPSTREAM
        assert rio_gp.op_census(plainlib, op.h)[0] == rio_gp.EUPSTREAM and rio_gp.op_census(plainlib, op.h, True)[0] == rio_gp.EUPSTREAM
        assert op.lookup("T", "1") == "a:1"
    finally:
        op.close()


def test_per_type_expiry_under_thread_sanitizer(tmp_path):
    exe = tmp_path / "race_driver_classes"
    srcs = [os.path.join(ROOT, "rio-rs_amd", "csrc", "gpu_object_placement.cpp"), os.path.join(ROOT, "tests", "stub_rio_gp_classes.cpp"),
            os.path.join(ROOT, "tests", "host_layer_race_driver_classes.cpp")]
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
    assert "wrong=0" in r.stdout and "hot_listed=0" in r.stdout
