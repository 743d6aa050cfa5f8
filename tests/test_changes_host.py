"""The string layer's change feed (rio_op_changes) without a GPU: gpu_object_placement.cpp over the host-memory stub of the dense
ABI plus a host rio_gp_changes (tests/stub_rio_gp_changes.cpp).  After every listing a mirror that applies it equals
rio_op_snapshot; rows are recycled by reclaim() (small max_objects), keys hold NUL bytes, a consumer thread runs beside writers,
and the write-behind bridge (snapshot.sync_sqlite / sync_postgres) keeps a file equal to a fresh dump."""
import ctypes as C
import os
import random
import sqlite3
import subprocess
import threading

import pytest

import rio_gp
import snapshot
import spec_changes as spec
from test_node_index_host import StubOp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def chlib(tmp_path_factory):
    out = tmp_path_factory.mktemp("stub_changes") / "libstub_op_changes.so"
    srcs = [os.path.join(ROOT, "rio-rs_amd", "csrc", "gpu_object_placement.cpp"), os.path.join(ROOT, "tests", "stub_rio_gp_changes.cpp")]
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
    rio_gp.bind_op_changes(L)
    return L


class ChOp(StubOp):
    """The stub-linked string layer with the calls snapshot.sync_* need: changes(), changes_reset(), snapshot()."""

    fail_next = False

    def changes(self):
        rc, full, out = rio_gp.op_changes(self.L, self.h)
        assert rc == 0
        return full, out

    def changes_reset(self):
        assert self.L.rio_op_changes_reset(self.h) == 0

    def try_update(self, ty, oid, addr):   # rc: 0, or RIO_GP_EINVAL when every row belongs to a live object
        t, i = ty.encode(), oid.encode()
        return self.L.rio_op_update_n(self.h, t, len(t), i, len(i), None if addr is None else addr.encode())

    def try_request(self, ty, oid, me):
        t, i = ty.encode(), oid.encode()
        buf, flag = C.create_string_buffer(256), C.c_uint32(0)
        return self.L.rio_op_get_or_create_placement_n(self.h, t, len(t), i, len(i), me.encode(), buf, 256, C.byref(flag))


def snap_set(op):
    return set(op.snapshot())


def step(op, rng, keys, addrs):
    """One random call: update / delete-by-update / remove / clean_server / request / membership flip."""
    k = rng.randrange(8)
    ty, oid = rng.choice(keys)
    if k <= 2:
        assert op.try_update(ty, oid, rng.choice(addrs)) in (0, rio_gp.EINVAL)
    elif k == 3:
        assert op.try_update(ty, oid, None) in (0, rio_gp.EINVAL)
    elif k == 4:
        op.remove(ty, oid)
    elif k == 5:
        op.clean_server(rng.choice(addrs))
    elif k == 6:
        assert op.try_request(ty, oid, rng.choice(addrs)) in (0, rio_gp.EINVAL)
    else:
        op.set_member(rng.choice(addrs), rng.random() < 0.7)


def keyset(rng, n, nul=False):
    keys = [("T%d" % (i % 3), "o%d" % i) for i in range(n)]
    if nul:
        keys += [("N\0%d" % i, "x\0y%d" % i) for i in range(n // 4)] + [("T0", "o1\0"), ("T0\0", "o1")]
    return keys


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("shadow", [True, False])
def test_mirror_plus_listing_is_the_snapshot(chlib, seed, shadow):
    rng = random.Random(seed)
    op = ChOp(chlib, 24, 8, flags=0 if shadow else 8)     # 24 rows for ~60 keys: reclaim() recycles rows all the time
    try:
        addrs = ["h%d:7" % k for k in range(5)]
        for a in addrs[:4]:
            op.set_member(a, True)
        keys = keyset(rng, 60, nul=seed % 2 == 1)
        full, ent = op.changes()
        assert full and ent == []
        mirror = {}
        for it in range(400):
            step(op, rng, keys, addrs)
            if rng.random() < 0.3 or it == 399:
                full, ent = op.changes()
                assert not full
                mirror = spec.apply(mirror, full, ent)
                assert spec.as_set(mirror) == snap_set(op), it
        # nothing changed: an empty listing
        assert op.changes() == (False, [])
    finally:
        op.close()


def test_full_flag_first_call_and_after_reset(chlib):
    op = ChOp(chlib, 16, 4)
    try:
        op.update("A", "1", "x:1")
        op.update("A", "2\0b", "y:2")
        full, ent = op.changes()
        assert full and sorted(ent) == [("A", "1", None, "x:1"), ("A", "2\0b", None, "y:2")]
        op.update("A", "1", "y:2")
        op.remove("A", "2\0b")
        full, ent = op.changes()
        assert not full
        assert ent == [("A", "2\0b", "y:2", None), ("A", "1", "x:1", "y:2")]      # the delete first
        op.changes_reset()
        full, ent = op.changes()
        assert full and ent == [("A", "1", None, "y:2")]
        assert op.changes() == (False, [])
    finally:
        op.close()


def test_recycled_row_gives_delete_then_upsert(chlib):
    op = ChOp(chlib, 2, 4)                                   # two rows: the third key needs a reclaimed one
    try:
        op.update("K", "a", "x:1")
        op.update("K", "b", "x:1")
        assert op.changes()[0]
        op.remove("K", "a")                                   # row of K.a: unplaced, not an object -> reclaimable
        op.update("K", "c", "x:1")                            # reclaim() hands the row to K.c, placed on the SAME node
        full, ent = op.changes()
        assert not full
        assert ent == [("K", "a", "x:1", None), ("K", "c", None, "x:1")]
        assert set(op.snapshot()) == {("K", "b", "x:1"), ("K", "c", "x:1")}
        # a key that comes back on another row after its own was recycled
        op.remove("K", "b")
        op.remove("K", "c")
        op.update("K", "d", "y:2")                            # reclaim: both rows free, K.d takes one
        op.update("K", "b", "y:2")
        full, ent = op.changes()
        mirror = spec.apply({("K", "b"): "x:1", ("K", "c"): "x:1"}, full, ent)
        assert spec.as_set(mirror) == set(op.snapshot()) == {("K", "d", "y:2"), ("K", "b", "y:2")}
    finally:
        op.close()


def test_consumer_thread_beside_writers(chlib):
    op = ChOp(chlib, 32, 8)
    addrs = ["w%d:1" % k for k in range(6)]
    for a in addrs:
        op.set_member(a, True)
    stop = threading.Event()
    errors = []
    state = {"mirror": {}, "n": 0}

    def writer(seed):
        rng = random.Random(seed)
        keys = keyset(rng, 40, nul=True)
        try:
            for _ in range(1500):
                step(op, rng, keys, addrs)
        except BaseException as e:   # (reported by the main thread)
            errors.append(e)

    def consumer():
        try:
            while not stop.is_set():
                full, ent = op.changes()
                state["mirror"] = spec.apply(state["mirror"], full, ent)
                state["n"] += 1
        except BaseException as e:
            errors.append(e)

    try:
        ws = [threading.Thread(target=writer, args=(s,)) for s in range(3)]
        c = threading.Thread(target=consumer)
        c.start()
        for w in ws:
            w.start()
        for w in ws:
            w.join()
        stop.set()
        c.join()
        assert not errors, errors
        full, ent = op.changes()
        mirror = spec.apply(state["mirror"], full, ent)
        assert spec.as_set(mirror) == snap_set(op)
        assert state["n"] > 1
    finally:
        op.close()


def _rows(path):
    db = sqlite3.connect(path)
    try:
        return db.execute("SELECT struct_name, object_id, server_address FROM object_placement ORDER BY struct_name, object_id").fetchall()
    finally:
        db.close()


def test_sync_sqlite_equals_a_fresh_dump(chlib, tmp_path):
    rng = random.Random(7)
    op = ChOp(chlib, 24, 8)
    try:
        addrs = ["s%d:9" % k for k in range(4)]
        for a in addrs:
            op.set_member(a, True)
        keys = keyset(rng, 50, nul=True)
        path = str(tmp_path / "mirror.db")
        assert snapshot.sync_sqlite(op, path)[2] is True          # the first sync is a full one
        for it in range(12):
            for _ in range(30):
                step(op, rng, keys, addrs)
            up, dl, full = snapshot.sync_sqlite(op, path)
            assert not full
            fresh = str(tmp_path / ("fresh%d.db" % it))
            snapshot.dump_sqlite(op, fresh, replace=True)
            assert _rows(path) == _rows(fresh), it
    finally:
        op.close()


def test_a_failed_write_is_followed_by_a_full_rewrite(chlib, tmp_path):
    rng = random.Random(3)
    op = ChOp(chlib, 24, 8)
    try:
        addrs = ["f%d:9" % k for k in range(4)]
        for a in addrs:
            op.set_member(a, True)
        keys = keyset(rng, 40)
        path = str(tmp_path / "mirror.db")
        for _ in range(40):
            step(op, rng, keys, addrs)
        snapshot.sync_sqlite(op, path)
        for _ in range(40):
            step(op, rng, keys, addrs)
        op.update("F", "must-arrive", addrs[0])
        db = sqlite3.connect(path)
        db.execute("CREATE TRIGGER refuse BEFORE INSERT ON object_placement BEGIN SELECT RAISE(ABORT, 'forced'); END")
        db.commit()
        db.close()
        with pytest.raises(sqlite3.DatabaseError):
            snapshot.sync_sqlite(op, path)
        db = sqlite3.connect(path)
        db.execute("DROP TRIGGER refuse")
        db.commit()
        db.close()
        up, dl, full = snapshot.sync_sqlite(op, path)
        assert full and dl == 0
        fresh = str(tmp_path / "fresh.db")
        snapshot.dump_sqlite(op, fresh, replace=True)
        assert _rows(path) == _rows(fresh)
        assert ("F", "must-arrive", addrs[0]) in _rows(path)
    finally:
        op.close()


class _FmtCursor:
    def __init__(self, db):
        self.c = db.cursor()

    def execute(self, stmt, params=()):
        self.c.execute(stmt.replace("%s", "?"), params)

    def executemany(self, stmt, rows):
        self.c.executemany(stmt.replace("%s", "?"), rows)


class _FmtConn:
    """psycopg-style connection (%s markers) over SQLite: the statements go through unchanged but for the markers."""

    def __init__(self, path):
        self.db = sqlite3.connect(path)

    def cursor(self):
        return _FmtCursor(self.db)

    def commit(self):
        self.db.commit()

    def rollback(self):
        self.db.rollback()


def test_sync_postgres_statements(chlib, tmp_path):
    rng = random.Random(11)
    op = ChOp(chlib, 24, 8)
    try:
        addrs = ["p%d:9" % k for k in range(4)]
        for a in addrs:
            op.set_member(a, True)
        keys = keyset(rng, 40)
        path = str(tmp_path / "pg.db")
        conn = _FmtConn(path)
        for it in range(6):
            for _ in range(30):
                step(op, rng, keys, addrs)
            assert snapshot.sync_postgres(op, conn)[2] == (it == 0)
            fresh = str(tmp_path / ("fresh%d.db" % it))
            snapshot.dump_sqlite(op, fresh, replace=True)
            assert _rows(path) == _rows(fresh)
        conn.db.close()
    finally:
        op.close()
