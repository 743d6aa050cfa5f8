"""The string layer's idle deactivation (rio_op_set_clock / rio_op_expire) without a GPU: gpu_object_placement.cpp over the
host-memory stub of the dense ABI plus a host rio_gp_touch_merge and rio_gp_expire (tests/stub_rio_gp_expire.cpp).  A random call
sequence runs through two clones of one provider — every stamping call, removals, clean_server, a moving clock, sweeps with and
without a limit — and after every call the lookups, the snapshot and the feed's mirror are compared with a dict model that
keeps the stamps the contract describes (include/rio_gpu_object_placement.h).  Fixed cases: the clock at 0 keeps no stamps, a
table full of live objects takes new keys again after a sweep, keys with NUL bytes come back whole, a dense layer without the
calls answers RIO_GP_EUPSTREAM and changes nothing; and the ThreadSanitizer run of the invariant "a key stamped with an epoch >=
cutoff before the sweep took its locks is never listed" (tests/host_layer_race_driver_expire.cpp, a program of its own)."""
import ctypes as C
import os
import random
import shutil
import subprocess

import pytest

import rio_gp
from test_remove_members_host import Model, Op, _build, apply_listing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bind(L):
    rio_gp.bind_op_changes(L)
    rio_gp.bind_op_expire(L)
    L.rio_op_try_lookup_n.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t,
                                      C.POINTER(C.c_int)]
    L.rio_op_try_get_or_create_placement_n.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p,
                                                       C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32)]
    return L


@pytest.fixture(scope="module")
def exlib(tmp_path_factory):
    return _bind(_build(tmp_path_factory.mktemp("stub_expire"), "libstub_op_expire.so", "stub_rio_gp_expire.cpp"))


@pytest.fixture(scope="module")
def plainlib(tmp_path_factory):
    """the base stub alone: no rio_gp_touch_merge / rio_gp_expire (nor any other optional call)"""
    L = _build(tmp_path_factory.mktemp("stub_plain_ex"), "libstub_op_plain_ex.so", "stub_rio_gp.cpp")
    rio_gp.bind_op_expire(L)
    return L


class ExOp(Op):
    def clone(self):
        c = ExOp.__new__(ExOp)
        c.L, c.h = self.L, C.c_void_p(self.L.rio_op_clone(self.h))
        return c

    def set_clock(self, now):
        assert self.L.rio_op_set_clock(self.h, now) == 0

    def expire(self, cutoff, max_objects=None):
        rc, out, idle = rio_gp.op_expire(self.L, self.h, cutoff, max_objects)
        assert rc == 0
        return out, idle

    def try_lookup(self, ty, oid):
        """(answered, address): answered False = RIO_GP_EAGAIN"""
        t, i = ty.encode(), oid.encode()
        buf, found = C.create_string_buffer(256), C.c_int(0)
        rc = self.L.rio_op_try_lookup_n(self.h, t, len(t), i, len(i), buf, 256, C.byref(found))
        assert rc in (0, rio_gp.EAGAIN)
        return rc == 0, (buf.value.decode() if rc == 0 and found.value else None)

    def try_request_now(self, ty, oid, me):
        t, i = ty.encode(), oid.encode()
        buf, flag = C.create_string_buffer(256), C.c_uint32(0)
        rc = self.L.rio_op_try_get_or_create_placement_n(self.h, t, len(t), i, len(i), me.encode(), buf, 256, C.byref(flag))
        assert rc in (0, rio_gp.EAGAIN)
        return rc == 0, (buf.value.decode() if rc == 0 else None)


class Seen:
    """The stamps the contract describes, beside the placement Model: clock, {key: epoch}, and the keys in row order (the order
    in which they were first interned: the table never fills here, so no row changes hands)."""

    def __init__(self):
        self.clock, self.stamp, self.order = 0, {}, []

    def know(self, key):
        if key not in self.order:
            self.order.append(key)

    def touch(self, key):
        if self.clock:
            self.stamp[key] = max(self.stamp.get(key, 0), self.clock)

    def expire(self, md, cutoff, cap=None):
        idle = [k for k in self.order if k in md.where and self.stamp.get(k, 0) < cutoff]
        listed = idle if cap is None else idle[:cap]
        out = [(k[0], k[1], md.where[k]) for k in listed]
        for k in listed:
            del md.where[k]
        return out, len(idle)


@pytest.mark.parametrize("shadow", [True, False])
@pytest.mark.parametrize("seed", range(5))
def test_random_calls_through_two_clones_match_the_model(exlib, seed, shadow):
    rng = random.Random(seed)
    a = ExOp(exlib, 256, 8, flags=0 if shadow else 8)   # 8: RIO_OP_CFG_NO_HOST_SHADOW
    ops = [a, a.clone()]
    md, sn = Model(8), Seen()
    addrs = ["h%d:7" % k for k in range(5)]
    keys = [("T%d" % (i % 3), "o%d" % i) for i in range(40)] + [("N\0", "x\0y")]
    mirror, fed = {}, False
    try:
        for ad in addrs:
            a.set_member(ad, True)
            md.intern(ad, up=True)
        for it in range(400):
            op = ops[rng.randrange(2)]
            k = rng.randrange(14)
            key = rng.choice(keys)
            ad = rng.choice(addrs)
            if it == 60 or (it > 60 and k == 0):
                sn.clock += rng.randrange(1, 3)           # (the first 60 calls run with the clock at 0: no stamps)
                op.set_clock(sn.clock)
            elif k <= 2:
                assert op.try_update(key[0], key[1], ad) == 0
                md.update(key, ad)
                sn.know(key)
                sn.touch(key)
            elif k == 3:
                op.remove(key[0], key[1])                 # (a remove does not stamp — and interns nothing)
                md.unplace(key)
            elif k <= 5:
                rc, got, flag = op.try_request(key[0], key[1], ad)
                assert rc == 0 and (got, flag) == md.request(key, ad), it
                sn.know(key)
                sn.touch(key)
            elif k == 6:
                if op.lookup(key[0], key[1]) is not None:  # (compared with the model below)
                    sn.touch(key)
            elif k == 7:
                ok, got = op.try_lookup(key[0], key[1])
                if ok:
                    assert got == md.where.get(key)
                    if got is not None:
                        sn.touch(key)
            elif k == 8:
                ok, got = op.try_request_now(key[0], key[1], ad)
                if ok:
                    assert got == md.where.get(key)
                    sn.touch(key)
            elif k == 9:
                op.clean_server(ad)
                md.clean(ad)
            elif k == 10:
                cutoff = rng.choice([0, 1, sn.clock, sn.clock + 1, max(sn.clock - 1, 0), 0xFFFFFFFF])
                cap = rng.choice([None, 0, 1, 3, 1000])
                if cap == 0:
                    idle = len([x for x in sn.order if x in md.where and sn.stamp.get(x, 0) < cutoff])
                    assert op.expire(cutoff, 0) == ([], idle)
                else:
                    assert op.expire(cutoff, cap) == sn.expire(md, cutoff, cap), it
            elif k == 11:
                full, ent = op.changes()
                assert full == (not fed)
                fed = True
                mirror = apply_listing(mirror, full, ent)
                assert mirror == md.where, it
            for ty, oid in keys:                          # every lookup stamps what it finds
                got = op.lookup(ty, oid)
                assert got == md.where.get((ty, oid)), (it, ty, oid)
                if got is not None:
                    sn.touch((ty, oid))
            assert {(t, i): x for t, i, x in op.snapshot()} == md.where
        out, idle = ops[0].expire(0xFFFFFFFF)
        assert (out, idle) == sn.expire(md, 0xFFFFFFFF) and not md.where
        full, ent = ops[0].changes()
        assert apply_listing(mirror, full, ent) == {} or not fed
    finally:
        for op in ops:
            op.close()


def test_with_the_clock_at_zero_no_stamps_are_kept_and_everything_placed_is_idle(exlib):
    op = ExOp(exlib, 64, 4)
    try:
        for k in range(6):
            op.update("T", "o%d" % k, "a:1")
        assert op.lookup("T", "o1") == "a:1"
        op.remove("T", "o5")
        assert op.expire(0, 0) == ([], 0) and op.expire(1, 0) == ([], 5) and op.expire(0xFFFFFFFF, 0) == ([], 5)
        assert op.expire(1, 2) == ([("T", "o0", "a:1"), ("T", "o1", "a:1")], 5)
        op.set_clock(7)
        assert op.lookup("T", "o3") == "a:1"              # stamped 7
        assert op.lookup("T", "o0") is None               # a miss stamps nothing
        out, idle = op.expire(7)
        assert (out, idle) == ([("T", "o2", "a:1"), ("T", "o4", "a:1")], 2)
        assert op.expire(8) == ([("T", "o3", "a:1")], 1)
        assert op.snapshot() == []
    finally:
        op.close()


def test_a_table_full_of_live_objects_takes_new_keys_after_a_sweep(exlib):
    op = ExOp(exlib, 8, 4)
    try:
        op.set_clock(1)
        for k in range(8):
            op.update("T", "o%d" % k, "a:1")
        assert op.try_update("T", "new", "a:1") == rio_gp.EINVAL
        assert b"object table full" in exlib.rio_op_last_error(op.h)
        op.set_clock(2)
        for k in (0, 1, 2):
            assert op.lookup("T", "o%d" % k) == "a:1"
        out, idle = op.expire(2)
        assert [o[1] for o in out] == ["o%d" % k for k in range(3, 8)] and idle == 5
        for k in range(5):
            assert op.try_update("T", "new%d" % k, "b:1") == 0
        assert op.try_update("T", "new5", "b:1") == rio_gp.EINVAL
        assert {(t, i): x for t, i, x in op.snapshot()} == dict([(("T", "o%d" % k), "a:1") for k in range(3)] +
                                                                [(("T", "new%d" % k), "b:1") for k in range(5)])
    finally:
        op.close()


def test_keys_with_nul_bytes_come_back_with_their_lengths(exlib):
    op = ExOp(exlib, 16, 4)
    try:
        op.update("N\0", "x\0y", "a:1")
        op.update("N", "x", "a:1")
        assert op.expire(1) == ([("N\0", "x\0y", "a:1"), ("N", "x", "a:1")], 2)
    finally:
        op.close()


def test_without_the_dense_calls_nothing_changes(plainlib):
    op = ExOp(plainlib, 32, 4)
    try:
        op.update("T", "1", "a:1")
        op.set_clock(3)
        rc, out, idle = rio_gp.op_expire(plainlib, op.h, 0xFFFFFFFF)
        assert rc == rio_gp.EUPSTREAM and b"dense layer has no idle expiry" in plainlib.rio_op_last_error(op.h)
        assert rio_gp.op_expire(plainlib, op.h, 5, 0)[0] == rio_gp.EUPSTREAM
        assert op.lookup("T", "1") == "a:1"
    finally:
        op.close()


def test_expiry_under_thread_sanitizer(tmp_path):
    exe = tmp_path / "race_driver_expire"
    srcs = [os.path.join(ROOT, "rio-rs_amd", "csrc", "gpu_object_placement.cpp"), os.path.join(ROOT, "tests", "stub_rio_gp_expire.cpp"),
            os.path.join(ROOT, "tests", "host_layer_race_driver_expire.cpp")]
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
