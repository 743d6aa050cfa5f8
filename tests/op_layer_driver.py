"""The string layer (rio_op_*, include/rio_gpu_object_placement.h) fuzzed as what it is: a translation.  It decides nothing — it
turns strings into rows and node ids, calls the dense layer and turns the answers back — so one random sequence of EVERY call
is checked, after every call, against a translation model over the dense layer's own CPU references.

What the driver keeps, none of it taken from the layer's internals:
  addr -> node id   learnt through rio_op_node_address, checked to be a stable injection;
  key  -> row       learnt from public listings only: rio_op_objects_on_server(a) zipped with rio_gp_rows_on_nodes of that node on
                    the rio_op_dense handle (both in row order), or the one row whose load changed for rio_op_set_object_load.  A
                    key whose row cannot be seen (it is not placed) is carried as "row unknown": unplaced, load 1.  The references
                    that take requests in array order (place_pending, update_batch) give such keys rows past the table's end;
  the documented lifetime of a key: created by update(Some) / a request / set_object_load, dropped — when the table runs full
                    and only then — if it is unplaced with affinity RIO_GP_AFF_INACTIVE and not set aside by set_object_load;
  the dense state before each call (column, load, affinity, capacity, liveness, used), read through rio_op_dense's getters,
                    which tests/test_gpu_fuzz.py holds to the oracle.
Per call the expected dense state comes from pyoracle / tests/rebalance_ref.py / tests/spec_rebalance.py / tests/spec_changes.py
with translated arguments; the column and `used`, every answer, the index, the snapshot, the feed's mirror, the shadow's answers,
what a clone sees and every refusal are compared bit for bit / string for string.  No tolerance anywhere.

Idle deactivation (rio_op_set_clock / rio_op_expire) is part of the sequence.  The model holds the clock the clones share and one
stamp per ROW (a row handed to a new key keeps its stamp) and restates the header's stamping rule in every operation that can stamp
— RIO_GP_ERANGE answers do not, every entry of a batch is judged by itself.  A sweep's listing, n_out and n_idle come from
tests/spec_expire.py over the dense state read before the call, translated through row -> key and the node table; afterwards the
column, `used` and the affinity are those of rio_gp_remove_batch of the listed rows under the row lifecycle, rio_gp_get_seen on the
rio_op_dense handle equals the model's stamps (every sweep uploads them, a count-only one too), a listed key is gone through both
clones and a key that was not listed is still answered from the shadow.

Measured load, the hot-object report, the by-load cut and the classes are part of the sequence too.  The model keeps one request
counter per ROW next to the stamp: it rises at the very sites that stamp, while tracking is on and whether or not the clock is
set, and — unlike the stamp — goes back to 0 when the row is handed to a new key.  rio_op_fold_loads is compared with
tests/spec_loads.py over the load column read before the call and those counters, row for row; before a fold the rows of the
keys no listing has shown are learnt (the one row whose load changes under rio_op_set_object_load, put back at once), so every
row without a key is a free row and must hold load 1 before and after.  rio_op_hottest_objects is tests/spec_top.py over the
placed keys in row order, rio_op_rebalance_ordered by load tests/spec_rebalance_order.py (held to tests/rebalance_order_ref.py up
to 4 096 rows).  Types are numbered in the order the header gives (a type gets its class when its first key gets its row,
whatever becomes of the call); rio_op_expire_by_type is tests/spec_classes.py under cutoffs built per class, rio_op_census its
census with 256 classes, and after each of the two rio_gp_get_classes on the dense handle equals the model's class column on
every row whose key the model knows.

Immovable types are part of the sequence as well.  The model keeps one flag per struct_name; rio_op_set_type_movable_n goes through
either clone with the type of a placed key, any known type, one never seen (it gets its class by the call, so the order of
interning follows, and the census order checks that; its first key may come with the very next call) or, past 255 types, one that
lands in RIO_OP_CLASS_OTHER (RIO_GP_ERANGE, nothing set), and a flag that repeats or takes back what the type holds.  While a type
is immovable a rebalance — made through the clone the last flag did not go through — is tests/spec_movable.py over the dense
state read before the call, the model's own class column and the table built from the model's flags (up to 4 096 rows the
vectorised reference on the affinity with RIO_GP_AFF_INACTIVE on the immovable rows must agree first); the moves are compared key
for key, and afterwards rio_gp_get_class_movable on the dense handle is the model's table, rio_gp_get_classes the model's class
column on every row whose key the model knows (the rebalance has uploaded what changed, as a per-type sweep would have: the sweep
that sometimes follows at once must agree), and the keys of the immovable types answer from their old address through both clones.
Once the last immovable type is movable again the next rebalance is the plain reference and leaves the dense table all 1.  Every
other call treats the keys as before: ticks, clean_server, the sweeps, removal and the census are compared as they always were.

The provider under test is given as make(max_objects, max_nodes, spill_rounds, flags): RealProvider.make over rio_gp (the GPU
test, tests/test_gpu_op_layer_fuzz.py) or tests/fake_rio_op.py (the driver's own test, tests/test_op_layer_driver.py).
"""
import ctypes as C

import numpy as np

import spec_changes
import spec_classes
import spec_expire
import spec_loads
import spec_top

NONE = 0xFFFFFFFF
U32 = 0xFFFFFFFF
KEEP_ONE = 65536
TOP_MAX = 4096
CLASS_OTHER = 255
ROW_ORDER, BY_LOAD = 0, 1
INF = 0xFFFFFFFFFFFFFFFF
AFF_INACTIVE = 0xFFFFFFFE
OK, EINVAL, EUPSTREAM, ENODEV, ENOMEM, ERANGE, EAGAIN = range(7)
CFG_LIVE_FIRST_TOUCH, CFG_NO_HOST_SHADOW = 4, 8
LOCAL, REDIRECT, PLACED, SPILLED, UNPLACED = range(5)
REPLACED = 0x10

FLOOR = (
    "reclaim between two feed reads",
    "rebalance moved keys of rows that had changed hands",
    "tick evicted from a member turned inactive",
    "spilled request",
    "UNPLACED request",
    "REPLACED request",
    "try_* answered from the shadow",
    "ERANGE",
    "table-full EINVAL",
    "request from an inactive requester under the default flags",
    "expire listed keys",
    "expire count only with idle keys",
    "expire capped below n_idle",
    "sweep with the clock never set listed everything placed",
    "a key stamped only by a shadow hit survived a sweep",
    "an expired key's row was handed to a new key before the next feed read",
    "a sweep judged a key by a stamp its row's previous key left",
    "expire listed a key set aside by set_object_load",
    # measured load
    "a fold saw a row that had changed hands since the last fold, with requests counted for its previous key",
    "a fold with a non-empty free list and a free-row result other than 1",
    "a fold counted requests of shadow hits",
    "a fold with the clock never set",
    "a refused fold kept its counters for the next one",
    "a fold changed no load",
    "tracking switched off between two folds",
    "get_object_load of a key never seen",
    # hot objects
    "hottest cut inside a tie group",
    "hottest on an address never seen",
    # the by-load cut
    "a by-load rebalance moved keys",
    "a by-load rebalance right after a fold",
    "an invalid order was refused",
    # classes
    "a class upload held a range and a scatter in one call",
    "a row changed hands twice between two class uploads",
    "a row changed hands before its first class upload",
    "a key of a type past 255 was swept by the default limit",
    "a type limit refused with ERANGE",
    "a per-type sweep listed keys of one type and spared older keys of another",
    "IDLE_NEVER spared an idle key",
    "a per-type sweep between two feed reads",
    "census by server with a server seen only through update",
    "census listed the shared class",
    # immovable types
    "a rebalance left a key of an immovable type on an over-capacity server and moved another",
    "a by-load rebalance with an immovable type moved keys",
    "a row changed hands to a key of an immovable type between two rebalances",
    "a rebalance did the class upload a per-type sweep would have done, and the sweep right after it agreed",
    "a type was made immovable before its first key",
    "set_type_movable refused with ERANGE",
    "the last immovable type became movable again and the next rebalance moved its keys",
    "a flag set through one clone held in a rebalance through the other",
    "tick or clean_server removed keys of an immovable type",
    "a sweep listed a key of an immovable type",
)

SIZES = ("tiny", "tiny", "edge", "tiny", "4096", "bulk")      # by seed % 6
FLAGS = (0, CFG_LIVE_FIRST_TOUCH, CFG_NO_HOST_SHADOW)            # by (seed // 6) % 3: every size meets every flag in 18 seeds


def config_of(seed):
    """(size class, provider flags) of a seed: drawn independently of each other, the whole cross product every 18 seeds."""
    return SIZES[seed % len(SIZES)], FLAGS[(seed // len(SIZES)) % 3]


class RealProvider:
    """rio_gp.GpuObjectPlacement seen as return codes and decoded listings.  `mid` is called between a listing call and the
    reading of the arrays it handed out: they belong to the calling thread until its next call of the same function."""

    def __init__(self, gp, p):
        self.gp, self.p, self.L = gp, p, gp._oplib()

    @classmethod
    def make(cls, gp):
        return lambda max_objects, max_nodes=32, spill_rounds=2, flags=0: cls(
            gp, gp.GpuObjectPlacement(max_objects=max_objects, max_nodes=max_nodes, spill_rounds=spill_rounds, flags=flags))

    def clone(self):
        return RealProvider(self.gp, self.p.clone())

    def close(self):
        self.p.close()

    def dense(self):
        return self.p.dense()

    def _rc(self, f, *a):
        try:
            return OK, f(*a)
        except self.gp.ObjectPlacementError as e:
            return e.rc, None

    def update(self, ty, oid, addr):
        return self._rc(self.p.update, ty, oid, addr)[0]

    def update_batch(self, keys, addrs):
        return self._rc(self.p.update_batch, keys, addrs)[0]

    def remove(self, ty, oid):
        return self._rc(self.p.remove, ty, oid)[0]

    def clean_server(self, addr):
        return self._rc(self.p.clean_server, addr)[0]

    def last_address_len(self):
        return int(self.L.rio_op_last_address_len(self.p._h))

    def _lookup(self, fn, ty, oid, cap):
        buf, found = C.create_string_buffer(b"\xAA" * max(cap, 1), max(cap, 1)), C.c_int(0)
        t, i = ty.encode(), oid.encode()
        rc = fn(self.p._h, t, len(t), i, len(i), buf, cap, C.byref(found))
        # (out_cap 0: the layer may not touch `out` at all — there is nothing to read)
        return rc, int(found.value), (buf.value.decode() if cap and rc in (OK, ERANGE) and found.value else "")

    def lookup(self, ty, oid, cap=512):
        return self._lookup(self.L.rio_op_lookup_n, ty, oid, cap)

    def try_lookup(self, ty, oid, cap=512):
        return self._lookup(self.L.rio_op_try_lookup_n, ty, oid, cap)

    def _request(self, fn, ty, oid, me, cap):
        buf, flag = C.create_string_buffer(b"\xAA" * max(cap, 1), max(cap, 1)), C.c_uint32(0)
        t, i = ty.encode(), oid.encode()
        rc = fn(self.p._h, t, len(t), i, len(i), me.encode(), buf, cap, C.byref(flag))
        return rc, (buf.value.decode() if cap and rc in (OK, ERANGE) else ""), int(flag.value)

    def get_or_create_placement(self, ty, oid, me, cap=512):
        return self._request(self.L.rio_op_get_or_create_placement_n, ty, oid, me, cap)

    def try_get_or_create_placement(self, ty, oid, me, cap=512):
        return self._request(self.L.rio_op_try_get_or_create_placement_n, ty, oid, me, cap)

    def _batch(self, fn, keys, *more):
        gp = self.gp
        tys, tyl, _t = gp._keys([k[0] for k in keys])
        ids, idl, _i = gp._keys([k[1] for k in keys])
        return fn(self.p._h, len(keys), tys, tyl, ids, idl, *more)

    def get_or_create_placement_batch(self, keys, mes):
        node, flag = np.empty(len(keys), np.uint32), np.empty(len(keys), np.uint32)
        rc = self._batch(self.L.rio_op_get_or_create_placement_batch_n, keys, self.gp._cstrs(mes), self.gp._ptr(node), self.gp._ptr(flag))
        return rc, [int(x) for x in node], [int(x) for x in flag]

    def lookup_batch(self, keys):
        out = np.empty(len(keys), np.uint32)
        rc = self._batch(self.L.rio_op_lookup_batch_n, keys, self.gp._ptr(out))
        return rc, [int(x) for x in out]

    def node_address(self, nid):
        return self.p.node_address(nid)

    def set_member(self, addr, active, capacity):
        return self._rc(self.p.set_member, addr, active, capacity)[0]

    def set_object_load(self, ty, oid, load):
        return self._rc(self.p.set_object_load, ty, oid, load)[0]

    def len(self):
        return self._rc(self.p.__len__)

    def tick(self):
        return self._rc(self.p.tick)

    def invalidate_cache(self):
        return self._rc(self.p.invalidate_cache)[0]

    def device_round_trips(self):
        return self.p.device_round_trips()

    def changes_reset(self):
        return self._rc(self.p.changes_reset)[0]

    @staticmethod
    def _strs(ptr, lens, n):
        v = C.cast(ptr, C.POINTER(C.c_void_p))
        return [C.string_at(v[k], lens[k]).decode() for k in range(n)]

    def snapshot(self, mid=None):
        n = C.c_uint64(0)
        ty, oid, addr = (C.POINTER(C.c_char_p)() for _ in range(3))
        tl, il = C.POINTER(C.c_size_t)(), C.POINTER(C.c_size_t)()
        rc = self.L.rio_op_snapshot(self.p._h, C.byref(n), C.byref(ty), C.byref(oid), C.byref(addr))
        if rc == OK:
            rc = self.L.rio_op_snapshot_key_lengths(self.p._h, C.byref(tl), C.byref(il))
        if rc:
            return rc, []
        if mid:
            mid()
        k = int(n.value)
        return OK, list(zip(self._strs(ty, tl, k), self._strs(oid, il, k), [addr[q].decode() for q in range(k)]))

    def objects_on_server(self, address, mid=None):
        n = C.c_uint64(0)
        ty, oid = C.POINTER(C.c_char_p)(), C.POINTER(C.c_char_p)()
        tl, il = C.POINTER(C.c_size_t)(), C.POINTER(C.c_size_t)()
        rc = self.L.rio_op_objects_on_server(self.p._h, address.encode(), C.byref(n), C.byref(ty), C.byref(tl), C.byref(oid), C.byref(il))
        if rc:
            return rc, []
        if mid:
            mid()
        k = int(n.value)
        return OK, list(zip(self._strs(ty, tl, k), self._strs(oid, il, k)))

    def rebalance(self, max_moves=None, mid=None, order=None):
        """order None: rio_op_rebalance; else rio_op_rebalance_ordered with that order (the two share the thread's arrays)."""
        n = C.c_uint64(0)
        ty, oid, fa, ta = (C.POINTER(C.c_char_p)() for _ in range(4))
        tl, il = C.POINTER(C.c_size_t)(), C.POINTER(C.c_size_t)()
        out = (C.byref(n), C.byref(ty), C.byref(tl), C.byref(oid), C.byref(il), C.byref(fa), C.byref(ta))
        B = INF if max_moves is None else int(max_moves)
        rc = self.L.rio_op_rebalance(self.p._h, B, *out) if order is None else self.L.rio_op_rebalance_ordered(self.p._h, int(order), B, *out)
        if rc:
            return rc, []
        if mid:
            mid()
        k = int(n.value)
        return OK, list(zip(self._strs(ty, tl, k), self._strs(oid, il, k), [fa[q].decode() for q in range(k)],
                            [ta[q].decode() for q in range(k)]))

    def changes(self, mid=None):
        n, full = C.c_uint64(0), C.c_int(0)
        ty, oid, oa, na = (C.POINTER(C.c_char_p)() for _ in range(4))
        tl, il = C.POINTER(C.c_size_t)(), C.POINTER(C.c_size_t)()
        rc = self.L.rio_op_changes(self.p._h, C.byref(n), C.byref(full), C.byref(ty), C.byref(tl), C.byref(oid), C.byref(il),
                                   C.byref(oa), C.byref(na))
        if rc:
            return rc, False, []
        if mid:
            mid()
        k = int(n.value)
        dec = lambda v: None if v is None else v.decode()
        return OK, bool(full.value), list(zip(self._strs(ty, tl, k), self._strs(oid, il, k), [dec(oa[q]) for q in range(k)],
                                             [dec(na[q]) for q in range(k)]))

    def set_clock(self, now):
        return int(self.L.rio_op_set_clock(self.p._h, int(now)))

    def expire(self, cutoff, max_objects=None, mid=None):
        """-> (rc, [(struct_name, object_id, address or None)], n_idle)"""
        n, idle = C.c_uint64(0), C.c_uint64(0)
        ty, oid, ad = (C.POINTER(C.c_char_p)() for _ in range(3))
        tl, il = C.POINTER(C.c_size_t)(), C.POINTER(C.c_size_t)()
        rc = self.L.rio_op_expire(self.p._h, int(cutoff), INF if max_objects is None else int(max_objects), C.byref(n), C.byref(idle),
                                  C.byref(ty), C.byref(tl), C.byref(oid), C.byref(il), C.byref(ad))
        if rc:
            return rc, [], 0
        if mid:
            mid()
        k = int(n.value)
        return OK, list(zip(self._strs(ty, tl, k), self._strs(oid, il, k),
                            [None if ad[q] is None else ad[q].decode() for q in range(k)])), int(idle.value)

    def set_load_tracking(self, on):
        return int(self.L.rio_op_set_load_tracking(self.p._h, 1 if on else 0))

    def fold_loads(self, keep, gain, min_load=0, max_load=U32):
        """-> (rc, rows_changed, hits_folded)"""
        return self.gp.op_fold_loads(self.L, self.p._h, keep, gain, min_load, max_load)

    def get_object_load(self, ty, oid):
        """-> (rc, load or None for a key never seen)"""
        return self.gp.op_get_object_load(self.L, self.p._h, ty, oid)

    def hottest_objects(self, address=None, min_load=0, max_objects=4096, mid=None):
        """-> (rc, [(struct_name, object_id, address or None, load)], n_candidates)"""
        gp = self.gp
        o, cand = gp._listing_out(1), C.c_uint64(0)
        cap = int(max_objects)
        loads = (C.c_uint32 * max(min(cap, 4096), 1))()
        rc = self.L.rio_op_hottest_objects(self.p._h, None if address is None else address.encode(), int(min_load), cap, C.byref(o[0]),
                                           C.byref(cand), *map(C.byref, o[1:]), loads)
        if rc:
            return rc, [], 0
        if mid:
            mid()
        return OK, [e + (int(loads[k]),) for k, e in enumerate(gp._listing(o))], int(cand.value)

    def set_type_idle_limit(self, ty, max_idle):
        return int(self.gp.op_set_type_idle_limit(self.L, self.p._h, ty, max_idle))

    def set_type_movable(self, ty, movable):
        return int(self.gp.op_set_type_movable(self.L, self.p._h, ty, movable))

    def expire_by_type(self, now, default_max_idle, max_objects=None, mid=None):
        """-> (rc, [(struct_name, object_id, address or None)], n_idle)"""
        gp = self.gp
        o, idle = gp._listing_out(1), C.c_uint64(0)
        rc = self.L.rio_op_expire_by_type(self.p._h, int(now), int(default_max_idle), INF if max_objects is None else int(max_objects),
                                          C.byref(o[0]), C.byref(idle), *map(C.byref, o[1:]))
        if rc:
            return rc, [], 0
        if mid:
            mid()
        return OK, gp._listing(o), int(idle.value)

    def census(self, by_server=False, mid=None):
        """-> (rc, [(struct_name as str or None for the shared class, address or None, rows, load)])"""
        n = C.c_uint64(0)
        names, addrs, lens = C.POINTER(C.c_char_p)(), C.POINTER(C.c_char_p)(), C.POINTER(C.c_size_t)()
        rows, loads = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        rc = self.L.rio_op_census(self.p._h, 1 if by_server else 0, C.byref(n), C.byref(names), C.byref(lens), C.byref(addrs),
                                  C.byref(rows), C.byref(loads))
        if rc:
            return rc, []
        if mid:
            mid()
        nv = C.cast(names, C.POINTER(C.c_void_p))
        return OK, [(C.string_at(nv[k], lens[k]).decode() if nv[k] else None, addrs[k].decode() if addrs[k] else None, int(rows[k]),
                     int(loads[k])) for k in range(n.value)]


class Key:
    """One interned key as the documentation describes its life: (ty, oid) as first handed over, its row once a listing showed
    it, whether it is set aside by set_object_load, and — while its row is unknown — whether a request has made it an object."""
    __slots__ = ("ty", "oid", "row", "keep", "obj")

    def __init__(self, ty, oid, keep):
        self.ty, self.oid, self.row, self.keep, self.obj = ty, oid, None, keep, False


class Scenario:
    OPS = (("update", 8), ("update_none", 2), ("update_batch", 3), ("remove", 5), ("clean_server", 2), ("lookup", 6),
           ("lookup_batch", 2), ("request", 10), ("request_batch", 4), ("try_lookup", 4), ("try_request", 4), ("set_member", 5),
           ("set_object_load", 3), ("tick", 3), ("rebalance", 4), ("changes", 5), ("changes_reset", 1), ("invalidate_cache", 1),
           ("objects_on_server", 2), ("snapshot", 2), ("len", 1), ("set_clock", 4), ("expire", 4),
           ("set_load_tracking", 2), ("fold_loads", 4), ("get_object_load", 2), ("hottest_objects", 3),
           ("set_type_idle_limit", 2), ("expire_by_type", 3), ("census", 2), ("set_type_movable", 4))

    def __init__(self, make, oracle, seed, steps=None):
        self.oracle, self.seed = oracle, seed
        rng = self.rng = np.random.default_rng(0x0B1A0000 + seed)
        kind, self.flags = config_of(seed)
        self.kind = kind
        self.rows_max = {"tiny": int(rng.integers(8, 49)), "edge": int(rng.choice([255, 256, 257])), "4096": 4096,
                         "bulk": 1 << 14}[kind]
        self.sa = not self.flags & CFG_LIVE_FIRST_TOUCH
        self.oflags = oracle.REF_SELF_ASSIGN if self.sa else 0
        self.rounds = int(rng.choice([1, 2, 2, 3]))
        self.max_nodes = 32
        self.steps = steps if steps is not None else {"tiny": 160, "edge": 110, "4096": 70, "bulk": 40}[kind]
        self.handles = [make(self.rows_max, self.max_nodes, self.rounds, self.flags)]
        self.handles.append(self.handles[0].clone())
        self.g = self.handles[0].dense()
        nm = int(rng.integers(3, 9))
        self.members = ["10.0.%d.%d:%d" % (seed % 200, k, 5000 + k) for k in range(nm)]
        self.odd = ["nocolon", "a-host-name-that-is-much-longer-than-thirty-two-bytes.example.org:65535"]
        self.crowd = ["10.9.0.%d:1" % k for k in range(40)] if seed % 5 == 3 else []     # more addresses than max_nodes holds
        self.upd_only = ["10.8.%d.%d:9" % (seed % 200, k) for k in range(2)]             # addresses only rio_op_update carries
        nk = {"tiny": 3 * self.rows_max, "edge": 400, "4096": 1500, "bulk": 3000}[kind]
        self.many_types = seed % 6 == 4       # one seed in six: more types than there are classes (RIO_OP_CLASS_OTHER is reached)
        tyname = (lambda k: "Y%d" % (k % 320)) if self.many_types else (lambda k: "T%d" % (k % 3))
        self.pool = [(tyname(k), str(k)) for k in range(nk)] + [("a.b", "c"), ("a", "b.c"), ("T0", ""), ("nul\0ty", "x"),
                                                               ("T1", "i\0d"), ("T1", "i")]
        if self.many_types:
            self.pool += [("", "e%d" % k) for k in range(3)] + [("Y\0%d" % k, "n") for k in range(4)]
        self.addr, self.aid, self.alive, self.cap = [], {}, [], []        # node table as documented: by id
        self.keys, self.row2key = {}, {}                                  # "ty.oid" -> Key ; row -> "ty.oid"
        self.handed = set()                                               # rows that have had more than one key
        self.dropped_since_feed = {}                                      # "ty.oid" -> row (if known) of keys reclaimed since the last read
        self.mirror, self.feed_state = {}, "first"                        # the feed's consumer
        self.ref, self.ref_on = None, True                                # LocalObjectPlacement cross-check
        self.inactive_since = set()                                       # members turned inactive that still hold objects
        self.log, self.count, self.cov = [], {}, {k: 0 for k in FLOOR}
        self.step = 0
        self.checked = 0
        # idle expiry (no draw from rng here: the earlier draws stay what they were).  The clock the clones share, 0 = stamping
        # off; one stamp per ROW (a row handed to a new key keeps its stamp): S, and S_dev = what it would be without the stamps
        # of shadow hits; rows whose present key has stamped itself; keys stamped while their row was unknown
        self.clock, self.clock_top, self.clock_ever = 0, 0, False
        self.S = np.zeros(self.rows_max, np.uint32)
        self.S_dev = np.zeros(self.rows_max, np.uint32)
        self.own = set()
        self.unknown_stamped = set()
        self.expired_since_feed = set()
        self.set_aside = set()
        # measured load: the switch the clones share; one request counter per ROW next to S (Hs: the part shadow hits counted);
        # keys counted while their row was unknown; rows whose counter a reclaim dropped since the last fold
        self.tracking, self.track_off = False, False
        self.Hc = np.zeros(self.rows_max, np.uint64)
        self.Hs = np.zeros(self.rows_max, np.uint64)
        self.unknown_hits = {}
        self.lost_hits = set()
        self.refused_fold = False
        self.last_dropped = []
        self.share = [0, 0]               # non-zero counters at a fold: on rows the model does not know, all of them
        # classes: struct_name -> class in the order of interning (at most 255 of them), its limit, the class column by row,
        # and what the next class upload will hold (the rows known to the device's class column end at cls_up)
        self.types, self.limits, self.limit_clone = {}, {}, None
        self.K = np.zeros(self.rows_max, np.uint8)
        self.cls_up, self.cls_scatter, self.cls_handed, self.cls_early = 0, set(), {}, False
        self.seen_by = {}                 # address -> the kinds of call that carried it
        # immovable types: struct_name -> immovable, the clone the last flag went through, the types flagged before their first
        # key, whether the dense table holds a flag (and of which classes), the rows handed to a new key since the last rebalance,
        # and whether the rebalance of the step before uploaded classes
        self.immovable, self.mv_clone, self.early_imm = {}, None, set()
        self.mv_dev, self.was_imm = False, set()
        self.handed_since_reb = set()
        self.reb_upload_step = None
        self.force_key = None

    # ---- small helpers ------------------------------------------------------------------------------------------------
    def fail(self, what, *more):
        raise AssertionError(("seed", self.seed, "step", self.step, what, "last ops", self.log[-6:]) + more)

    def want(self, cond, what, *more):
        self.checked += 1
        if not cond:
            self.fail(what, *more)

    def hit(self, name, on=True):
        if on:
            self.cov[name] += 1

    def h(self):
        """The clone this call goes through, and the other one."""
        k = int(self.rng.integers(2))
        return self.handles[k], self.handles[1 - k]

    def read(self):
        g = self.g
        n = g.num_objects
        col = g.get_assign() if n else np.zeros(0, np.uint32)
        load, aff = g.get_objects() if n else (np.zeros(0, np.uint32), np.zeros(0, np.uint32))
        cap, alive, used = g.get_nodes() if g.num_nodes else (np.zeros(0, np.uint64), np.zeros(0, np.uint8), np.zeros(0, np.uint64))
        return {"n": n, "col": col, "load": load, "aff": aff, "cap": cap, "alive": alive, "used": used, "m": g.num_nodes}

    def kstr(self, key):
        return key[0] + "." + key[1]

    def pick_key(self, known=0.6):
        rng = self.rng
        if self.force_key is not None:      # (the first key of a type that has just been made immovable)
            key, self.force_key = self.force_key, None
            return key
        if self.keys and rng.random() < known:
            ks = list(self.keys.values())
            k = ks[int(rng.integers(len(ks)))]
            return (k.ty, k.oid)
        return self.pool[int(rng.integers(len(self.pool)))]

    def pick_addr(self, odd=0.1):
        rng = self.rng
        r = rng.random()
        if r < odd:
            return self.odd[int(rng.integers(2))]
        if self.crowd and r < odd + 0.25:
            return self.crowd[int(rng.integers(len(self.crowd)))]
        return self.members[int(rng.integers(len(self.members)))]

    def carry(self, addrs, kind):
        """The kinds of call that have carried an address (a server may be known through rio_op_update alone)."""
        for a in addrs:
            if a is not None:
                self.seen_by.setdefault(a, set()).add(kind)

    def is_bad(self, a):
        c = a.find(":")
        return c < 0 or c == 0 or c + 1 >= len(a)

    def model_snapshot(self, st):
        """{(ty, oid): address} from the dense column and the row map."""
        out = {}
        for r in np.flatnonzero(st["col"] != NONE):
            ks = self.row2key.get(int(r))
            if ks is None:
                self.fail("a placed row has no key in the model", int(r))
            k = self.keys[ks]
            nd = int(st["col"][r])
            if nd < len(self.addr):
                out[(k.ty, k.oid)] = self.addr[nd]
        return out

    def where(self, st, key):
        """Address the model says `key` lives on (None: not placed)."""
        k = self.keys.get(self.kstr(key))
        if k is None or k.row is None:
            return None
        nd = int(st["col"][k.row])
        return None if nd == NONE else self.addr[nd]

    # ---- the documented lifetime of keys ------------------------------------------------------------------------------
    def droppable(self, st, k):
        if k.keep:
            return False
        if k.row is None:
            return not k.obj
        return st["col"][k.row] == NONE and st["aff"][k.row] == AFF_INACTIVE

    def intern(self, st, wanted):
        """`wanted`: [(key, create, use, address or None, requester)] in the call's order.  Runs the documented interning on
        the model: keys are created, the table reclaims when it is full, a second failure is the refusal.  -> True, or False when
        the call must answer EINVAL (table full of live keys, or a 33rd address); the model keeps what the call interned."""
        for attempt in range(2):
            full = False
            for key, create, use, address, up in wanted:
                ks = self.kstr(key)
                k = self.keys.get(ks)
                if k is None and create:
                    if len(self.keys) >= self.rows_max:
                        full = True
                        break
                    k = self.keys[ks] = Key(key[0], key[1], not use)
                    self.created.append(ks)
                    self.sight(key[0])    # (the type gets its class with the key's row, whatever becomes of the call)
                if k is not None and use:
                    k.keep = False
                if address is not None and address not in self.aid and address not in self.pending_addr:
                    if len(self.addr) + len(self.pending_addr) >= self.max_nodes:
                        self.refused = "33rd address"
                        return False
                    self.pending_addr[address] = 1 if up else 0
            if not full:
                return True
            gone = [ks for ks, k in self.keys.items() if self.droppable(st, k)]
            if attempt or not gone:
                self.refused = "table full"
                return False
            self.reclaims += 1
            for ks in gone:
                k = self.keys.pop(ks)
                if k.row is not None:
                    del self.row2key[k.row]
                    self.reset_rows.add(k.row)
                    self.own.discard(k.row)
                    if self.Hc[k.row]:               # the row changes hands: its counter starts again at 0, the stamp stays
                        self.lost_hits.add(k.row)
                    self.Hc[k.row] = self.Hs[k.row] = 0
                self.unknown_hits.pop(ks, None)
                self.last_dropped.append((k.ty, k.oid))
                self.unknown_stamped.discard(ks)     # (its row keeps the stamp: the next sweep's upload is compared as a whole)
                self.dropped_since_feed.setdefault(ks, k.row)
            if self.feed_state == "open":
                self.hit("reclaim between two feed reads")
        return True

    def learn_nodes(self, is_request):
        """New ids handed out by the call: addresses in the order rio_op_node_address names them."""
        h = self.handles[0]
        while True:
            a = h.node_address(len(self.addr))
            if a is None:
                break
            self.want(a not in self.aid, "two node ids for one address", a)
            self.want(a in self.pending_addr, "an address the call did not carry got an id", a)
            self.aid[a] = len(self.addr)
            self.addr.append(a)
            self.alive.append(self.pending_addr.pop(a))
            self.cap.append(INF)
        for j in (0, len(self.addr) // 2, len(self.addr) - 1):
            if 0 <= j < len(self.addr):
                self.want(h.node_address(j) == self.addr[j], "a node id changed its address", j)
        self.want(h.node_address(len(self.addr) + 3) is None, "an id nobody was given has an address")

    def learn_rows(self, before, after, nodes=None):
        """Listings of the nodes whose rows changed (or hold rows without a key): objects_on_server zipped with rows_on_nodes."""
        col = after["col"]
        if nodes is None:
            nb = before["n"]
            ch = np.flatnonzero(col[:nb] != before["col"])
            cand = set(int(x) for x in col[ch]) | set(int(x) for x in col[nb:])
            cand |= set(int(col[r]) for r in np.flatnonzero(col != NONE) if int(r) not in self.row2key)
            nodes = sorted(j for j in cand if j != NONE and j < len(self.addr))
        for j in nodes:
            rc, objs = self.handles[int(self.rng.integers(2))].objects_on_server(self.addr[j])
            self.want(rc == OK, "objects_on_server failed", rc)
            _, rows = self.g.rows_on_nodes([j])
            self.want(len(objs) == len(rows), "objects_on_server and rows_on_nodes differ in length", self.addr[j], len(objs), len(rows))
            self.want(np.array_equal(rows, np.flatnonzero(col == j)), "rows_on_nodes differs from the column", j)
            for (ty, oid), r in zip(objs, rows):
                r = int(r)
                ks = self.kstr((ty, oid))
                k = self.keys.get(ks)
                self.want(k is not None, "a listed key is not one the documented lifetime keeps", (ty, oid), r)
                self.want((k.ty, k.oid) == (ty, oid), "a key is listed under another spelling than it was created with", (ty, oid))
                if k.row is None:
                    old = self.row2key.get(r)
                    self.want(old is None, "a row changed key without a reclaim", r, old, ks)
                    self.new_row(k, ks, r)
                else:
                    self.want(k.row == r, "a key changed its row", ks, k.row, r)

    def new_row(self, k, ks, r):
        """A listing showed the row of key k.  The row keeps the stamp its previous key left (the header: "a row handed on keeps
        its stamp until its new key's first call")."""
        c = self.cls_of(k.ty)
        if r in self.ever_rows:
            self.handed.add(r)
            self.own.discard(r)
            self.hit("an expired key's row was handed to a new key before the next feed read", r in self.expired_since_feed)
            self.cls_handed[r] = self.cls_handed.get(r, 0) + 1
            self.handed_since_reb.add(r)
            if r >= self.cls_up:
                self.cls_early = True
            elif c != int(self.K[r]):
                self.cls_scatter.add(r)
        self.ever_rows.add(r)
        k.row = r
        self.row2key[r] = ks
        self.K[r] = c
        h = self.unknown_hits.pop(ks, 0)      # requests counted while the row was unknown
        self.Hc[r] = min(int(self.Hc[r]) + h, U32)

    def sight(self, ty):
        """A struct_name is interned: the first distinct one is class 0, the next class 1, ... up to 254."""
        if ty not in self.types and len(self.types) < CLASS_OTHER:
            self.types[ty] = len(self.types)

    def cls_of(self, ty):
        return self.types.get(ty, CLASS_OTHER)

    def imm_classes(self):
        """The classes of the types that are immovable now."""
        return set(self.types[ty] for ty, on in self.immovable.items() if on)

    # ---- the stamping rule (include/rio_gpu_object_placement.h, "idle deactivation") ------------------------------------------
    def stamp(self, key, shadow=False):
        """A call has answered or set an address for `key` (it returned RIO_GP_OK — an RIO_GP_ERANGE answer is a call that failed):
        with the clock non-zero the key's row is stamped, a maximum.  Called once the call's rows are learnt."""
        if not self.clock and not self.tracking:
            return
        ks = self.kstr(key)
        k = self.keys.get(ks)
        if k is None:
            self.fail("a call answered with an address for a key the model does not hold", key)
        if self.tracking:        # one request, at the very sites that stamp: whether or not the clock is set
            if k.row is None:
                self.unknown_hits[ks] = min(self.unknown_hits.get(ks, 0) + 1, U32)
            else:
                self.Hc[k.row] = min(int(self.Hc[k.row]) + 1, U32)
                if shadow:
                    self.Hs[k.row] += 1
        if not self.clock:
            return
        if k.row is None:        # (a batch that set the key's address and removed it again: see stamps_of_unknown_rows)
            self.unknown_stamped.add(ks)
            return
        r = k.row
        self.S[r] = max(int(self.S[r]), self.clock)
        if not shadow:
            self.S_dev[r] = max(int(self.S_dev[r]), self.clock)
        self.own.add(r)

    def stamps_of_unknown_rows(self, p):
        """Keys a batch stamped whose rows no listing shows (an entry set an address, a later entry of the same batch removed the
        key: every entry is judged by itself).  A count-only sweep uploads the host's stamps; the rows whose stamp rose to the
        clock — at most one per such key, none of them a row with a known key — are theirs."""
        if not self.unknown_stamped:
            return
        rc, got, _ = p.expire(0, 0)
        self.want(rc == OK and got == [], "a count-only sweep failed or listed something", rc, got[:4])
        seen = self.g.get_seen()
        diff = [int(r) for r in np.flatnonzero(seen != self.S[:len(seen)])]
        self.want(len(diff) <= len(self.unknown_stamped) and all(int(seen[r]) == self.clock and r not in self.row2key for r in diff),
                  "stamps rose that no call of the model explains", diff[:8], [int(seen[r]) for r in diff[:8]], self.clock)
        for r in diff:
            self.S[r] = self.S_dev[r] = self.clock
            self.own.add(r)
        self.unknown_stamped = set()

    def plain_lookup(self, p, st, key):
        """rio_op_lookup outside check_lookup (what fills the shadow): a found placement is stamped, shadow hit or not."""
        t0 = p.device_round_trips()
        rc, found, out = p.lookup(key[0], key[1])
        if rc == OK and found:
            self.want(out == self.where(st, key), "lookup: wrong address", out, self.where(st, key), key)
            self.stamp(key, shadow=p.device_round_trips() == t0)
        return rc, found, out

    # ---- one step: before -> call -> expected -> after ------------------------------------------------------------------
    def virtual(self, st, klist):
        """Row indices for the reference: the known row, or one past the table's end per key whose row is unknown (unplaced,
        load 1).  -> (idx, col, load, extra keys in order)"""
        extra, at, idx = [], {}, []
        for key in klist:
            k = self.keys.get(self.kstr(key))
            if k is not None and k.row is not None:
                idx.append(k.row)
            else:
                ks = self.kstr(key)
                if ks not in at:      # (the key's place in `extra`: a bulk load names 2^14 new keys)
                    at[ks] = len(extra)
                    extra.append(ks)
                idx.append(st["n"] + at[ks])
        col = np.concatenate([st["col"], np.full(len(extra), NONE, np.uint32)])
        load = np.concatenate([st["load"], np.ones(len(extra), np.uint32)])
        return np.array(idx, np.uint32), col, load, extra

    def node_arrays(self):
        return np.array(self.cap, np.uint64), np.array(self.alive, np.uint8)

    def settle(self, before, xcol, extra, what):
        """After the call: new node ids, new rows, then the whole column and `used` against the reference's."""
        after = self.read()
        self.want(after["n"] >= before["n"] and after["n"] <= self.rows_max, "the row count shrank or overflowed", after["n"])
        self.learn_rows(before, after)
        exp = np.full(after["n"], NONE, np.uint32)
        exp[:before["n"]] = xcol[:before["n"]]
        for t, ks in enumerate(extra):
            nd = xcol[before["n"] + t]
            k = self.keys.get(ks)
            if nd != NONE:
                self.want(k is not None and k.row is not None, "a key the reference placed is in no listing", ks, int(nd))
                self.want(exp[k.row] == NONE, "a new key was given a row that was placed", ks, k.row)
                exp[k.row] = nd
            if k is not None and k.row is None:
                k.obj = self.extra_obj.get(ks, k.obj)
        if what in ("tick", "clean_server") and self.imm_classes():
            nb, imm = before["n"], self.imm_classes()
            left = np.flatnonzero((before["col"] != NONE) & (after["col"][:nb] != before["col"]))
            self.hit("tick or clean_server removed keys of an immovable type", any(int(self.K[r]) in imm for r in left))
        bad = np.flatnonzero(after["col"] != exp)
        self.want(bad.size == 0, what + ": the dense column differs from the reference's", bad[:8], after["col"][bad[:8]], exp[bad[:8]])
        self.check_nodes_and_load(before, after, what)
        if self.reclaims:      # rows changed hands: no call answers a new key with what the shadow held for the row's old key
            self.probe(after, [ks for ks in dict.fromkeys(self.created) if ks in self.keys][:4])
        return after

    def check_nodes_and_load(self, before, after, what):
        m = after["m"]
        self.want(m <= len(self.addr), "the dense layer holds more nodes than ids were handed out")
        cap, alive = self.node_arrays()
        self.want(np.array_equal(after["cap"], cap[:m]) and np.array_equal(after["alive"], alive[:m]),
                  what + ": the node table differs from what set_member / the requests said", after["alive"], alive[:m])
        used = self.oracle.recompute_used(after["col"], after["load"], m) if m else np.zeros(0, np.uint64)
        self.want(np.array_equal(after["used"], used), what + ": `used` differs", after["used"], used)
        nb = before["n"]
        ch = [int(r) for r in np.flatnonzero(after["load"][:nb] != before["load"])]
        for r in ch:
            ok = (r in self.reset_rows and after["load"][r] == 1) or (self.load_row == r)
            self.want(ok, what + ": the load of a row changed that was neither reclaimed nor named", r, int(before["load"][r]), int(after["load"][r]))
        self.want((after["load"][nb:] == 1).all() or self.load_row is not None, what + ": a fresh row does not start with load 1")

    def begin(self):
        self.pending_addr, self.refused, self.reclaims, self.created = {}, None, 0, []
        self.reset_rows, self.load_row, self.extra_obj = set(), None, {}
        return self.read()

    def refused_unchanged(self, before, rc, what):
        self.want(rc == EINVAL, what + ": the refusal is not EINVAL", rc, self.refused)
        self.learn_nodes(False)
        self.pending_addr = {}
        after = self.read()
        self.want(np.array_equal(after["col"][:before["n"]], before["col"]) and (after["col"][before["n"]:] == NONE).all(),
                  what + ": a refused call changed the column")
        self.check_nodes_and_load(before, after, what)
        if self.refused == "table full":
            self.hit("table-full EINVAL")
        return after

    # ---- operations ---------------------------------------------------------------------------------------------------
    def op_update(self, addr_none=False):
        p, other = self.h()
        key = self.pick_key(0.4)
        a = None if addr_none else self.pick_addr()
        if a is not None and self.rng.random() < 0.08:      # a server no member list and no request ever names
            a = self.upd_only[int(self.rng.integers(2))]
        self.carry([a], "update")
        st = self.begin()
        ok = self.intern(st, [(key, a is not None, True, a, False)])
        rc = p.update(key[0], key[1], a)
        if not ok:
            return self.refused_unchanged(st, rc, "update")
        self.want(rc == OK, "update failed", rc)
        self.learn_nodes(False)
        idx, col, load, extra = self.virtual(st, [key])
        if a is not None or self.kstr(key) in self.keys:
            self.want(self.oracle.update_batch(col, len(self.addr), idx, [NONE if a is None else self.aid[a]]) == 0, "reference refused")
        if a is None and self.kstr(key) in self.keys and self.keys[self.kstr(key)].row is None:
            self.extra_obj[self.kstr(key)] = False      # Option::None is a remove: a key whose row is unknown is no object after it
        self.ref_key(key)
        if self.ref_on:
            self.ref[0].update(key[0], key[1], a)
        after = self.settle(st, col, extra, "update")
        if a is not None:          # an update with an address stamps; Option::None is a remove and does not
            self.stamp(key)
        return after

    def ref_key(self, key):
        """The restatement takes NUL-terminated keys: a key with a NUL byte in a writing call ends the cross-check."""
        if "\0" in key[0] + key[1]:
            self.ref_on = False

    def op_update_none(self):
        return self.op_update(True)

    def op_update_batch(self, n=None):
        p, other = self.h()
        rng = self.rng
        n = n or int(rng.choice([1, 2, 5, 40, 257]))
        keys = [self.pick_key(0.3) for _ in range(n)]
        if n > 1 and rng.random() < 0.7:          # duplicates: the last writer of a key wins
            for _ in range(max(1, n // 4)):
                keys[int(rng.integers(n))] = keys[int(rng.integers(n))]
        addrs = [None if rng.random() < 0.1 else self.pick_addr(0.03) for _ in range(n)]
        self.carry(addrs, "update")
        st = self.begin()
        ok = self.intern(st, [(k, a is not None, True, a, False) for k, a in zip(keys, addrs)])
        rc = p.update_batch(keys, addrs)
        if not ok:
            return self.refused_unchanged(st, rc, "update_batch")
        self.want(rc == OK, "update_batch failed", rc)
        self.learn_nodes(False)
        sel = [q for q in range(n) if addrs[q] is not None or self.kstr(keys[q]) in self.keys]
        idx, col, load, extra = self.virtual(st, [keys[q] for q in sel])
        nodes = [NONE if addrs[q] is None else self.aid[addrs[q]] for q in sel]
        if sel:
            self.want(self.oracle.update_batch(col, len(self.addr), idx, nodes) == 0, "reference refused")
        for q in sel:              # the last entry of a key whose row is unknown is a remove: the key is no object after the batch
            k = self.keys.get(self.kstr(keys[q]))
            if k is not None and k.row is None:
                self.extra_obj[self.kstr(keys[q])] = False if addrs[q] is None else self.extra_obj.get(self.kstr(keys[q]), k.obj)
        for k in keys:
            self.ref_key(k)
        if self.ref_on:
            for k, a in zip(keys, addrs):
                self.ref[0].update(k[0], k[1], a)
        after = self.settle(st, col, extra, "update_batch")
        for k, a in zip(keys, addrs):      # per entry: an entry with an address stamps its key, whatever a later entry does
            if a is not None:
                self.stamp(k)
        self.stamps_of_unknown_rows(p)
        return after

    def op_remove(self):
        p, other = self.h()
        key = self.pick_key(0.8)
        st = self.begin()
        self.intern(st, [(key, False, True, None, False)])
        rc = p.remove(key[0], key[1])
        self.want(rc == OK, "remove failed", rc)
        idx, col, load, extra = self.virtual(st, [key])
        k = self.keys.get(self.kstr(key))
        if k is not None:
            self.oracle.remove_batch(col, idx)
            if k.row is None:
                self.extra_obj[self.kstr(key)] = False
        self.ref_key(key)
        if self.ref_on:
            self.ref[0].remove(key[0], key[1])
        return self.settle(st, col, extra, "remove")

    def op_clean_server(self):
        p, other = self.h()
        a = self.pick_addr() if self.rng.random() < 0.9 else "10.200.0.1:9"     # sometimes an address nobody has seen
        st = self.begin()
        rc = p.clean_server(a)
        self.want(rc == OK, "clean_server failed", rc)
        col = st["col"].copy()
        if a in self.aid:
            self.oracle.clean_servers(col, len(self.addr), [self.aid[a]])
        if self.ref_on:
            self.ref[0].clean_server(a)
        after = self.settle(st, col, [], "clean_server")
        self.probe(after, [self.row2key[int(r)] for r in np.flatnonzero(st["col"] == self.aid.get(a, NONE - 1))[:3] if int(r) in self.row2key])
        return after

    def check_lookup(self, st, p, other, key, fn, what):
        want = self.where(st, key)
        cap = 512 if self.rng.random() < 0.8 or want is None else int(self.rng.integers(0, len(want) + 1))
        t0 = p.device_round_trips()
        rc, found, out = fn(key[0], key[1], cap)
        if what == "try_lookup" and rc == EAGAIN:
            return False
        if rc == OK and found:     # a lookup or try_lookup that finds a placement stamps, whoever answered; ERANGE is a failure
            self.stamp(key, shadow=p.device_round_trips() == t0)
        _, cnt = other.len()                                    # a call on the other clone, then the length this thread was left
        ln = p.last_address_len()
        self.want(cnt == int((st["col"] != NONE).sum()), "len differs from the placed rows", cnt)
        if want is None:
            self.want(rc == OK and not found and ln == 0, what + ": a key that is not placed was found", rc, found, out, key)
        elif cap < len(want.encode()) + 1:
            self.want(rc == ERANGE and found and out == "" and ln == len(want.encode()), what + ": ERANGE form", rc, found, out, ln, want)
            self.hit("ERANGE")
        else:
            self.want(rc == OK and found and out == want and ln == len(want.encode()), what + ": wrong address", rc, found, out, want, key)
        if self.ref_on and "\0" not in key[0] + key[1]:
            self.want(self.ref[0].lookup(key[0], key[1]) == want, "the reference restatement disagrees with the model", key, want)
        return True

    def op_lookup(self):
        p, other = self.h()
        st = self.begin()
        self.check_lookup(st, p, other, self.pick_key(0.8), p.lookup, "lookup")
        self.unchanged(st, "lookup")

    def op_try_lookup(self):
        p, other = self.h()
        st = self.begin()
        key = self.pick_key(0.9)
        if self.rng.random() < 0.5:
            self.plain_lookup(p, st, key)                       # (what fills the shadow)
        t0 = p.device_round_trips()
        if self.check_lookup(st, p, other, key, p.try_lookup, "try_lookup"):
            self.want(p.device_round_trips() == t0, "try_lookup went to the device")
            self.want(not self.flags & CFG_NO_HOST_SHADOW or self.kstr(key) not in self.keys, "the shadow answered although it is off")
            self.hit("try_* answered from the shadow", self.kstr(key) in self.keys)
        self.unchanged(st, "try_lookup")

    def unchanged(self, st, what):
        after = self.read()
        n = st["n"]     # (rows a refused call interned reach the device with the next call: unplaced rows past the old end)
        self.want(after["n"] >= n and np.array_equal(after["col"][:n], st["col"]) and (after["col"][n:] == NONE).all() and
                  np.array_equal(after["used"][:st["m"]], st["used"]) and not after["used"][st["m"]:].any(), what + " changed the table")

    def op_lookup_batch(self):
        p, other = self.h()
        st = self.begin()
        keys = [self.pick_key(0.7) for _ in range(int(self.rng.choice([1, 3, 50, 300])))]
        rc, ids = p.lookup_batch(keys)
        self.want(rc == OK, "lookup_batch failed", rc)
        want = [self.where(st, k) for k in keys]
        got = [None if v == NONE else self.addr[v] for v in ids]
        self.want(got == want, "lookup_batch: wrong node ids", [(k, g, w) for k, g, w in zip(keys, got, want) if g != w][:4])
        for k, v in zip(keys, ids):        # per entry: the ones that found a placement
            if v != NONE:
                self.stamp(k)
        self.unchanged(st, "lookup_batch")

    def expect_requests(self, st, keys, mes):
        """The policy for requests in array order, on the state before: the malformed-record rule, then place_pending."""
        idx, col, load, extra = self.virtual(st, keys)
        cap, alive = self.node_arrays()
        m = len(self.addr)
        if any(self.is_bad(a) for a in self.addr):
            bad = [int(i) for i in idx if col[i] != NONE and self.is_bad(self.addr[col[i]])]
            if bad:
                self.oracle.remove_batch(col, bad)
        used = self.oracle.recompute_used(col, load, m)
        req = np.array([self.aid[a] for a in mes], np.uint32)
        node, flag = self.oracle.place_pending(col, load, cap, alive, used, idx, req, self.rounds, self.oflags)
        for q, ks in enumerate(extra):
            self.extra_obj[ks] = True
        return col, extra, node, flag

    def note_flags(self, flags, mes):
        for f, me in zip(flags, mes):
            self.hit("spilled request", f & 0xF == SPILLED)
            self.hit("UNPLACED request", f & 0xF == UNPLACED)
            self.hit("REPLACED request", f & REPLACED)
            self.hit("request from an inactive requester under the default flags", self.sa and not self.alive[self.aid[me]])

    def op_request(self):
        p, other = self.h()
        key, me = self.pick_key(0.6), self.pick_addr(0.05)
        self.carry([me], "request")
        st = self.begin()
        ok = self.intern(st, [(key, True, True, me, True)])
        cap = 512 if self.rng.random() < 0.85 else 8
        t0 = p.device_round_trips()
        rc, out, flag = p.get_or_create_placement(key[0], key[1], me, cap)
        by_shadow = p.device_round_trips() == t0
        if not ok:
            return self.refused_unchanged(st, rc, "request")
        self.learn_nodes(True)
        col, extra, node, wflag = self.expect_requests(st, [key], [me])
        want = "" if node[0] == NONE else self.addr[node[0]]
        _, cnt = other.len()
        ln = p.last_address_len()
        if cap < len(want.encode()) + 1:
            self.want(rc == ERANGE and out == "", "request: ERANGE form", rc, out, want)
            self.hit("ERANGE")
        else:
            self.want(rc == OK and out == want, "request: wrong address", rc, out, want, key, me)
        self.want(ln == len(want.encode()), "request: last_address_len", ln, want)
        self.want(flag == int(wflag[0]), "request: wrong flag", flag, int(wflag[0]), key, me)
        self.note_flags([flag], [me])
        if self.ref_on:
            self.cross_request(key, me, want, flag)
        after = self.settle(st, col, extra, "request")
        if rc == OK and want:      # a request that returns an address stamps; UNPLACED and an ERANGE answer do not
            self.stamp(key, shadow=by_shadow)
        return after

    def cross_request(self, key, me, want, flag):
        """The restated get_or_create_placement of the reference, while nothing it lacks is in play."""
        if "\0" in key[0] + key[1] or self.is_bad(me) or (not self.sa and not self.alive[self.aid[me]]):
            self.ref_on = False
            return
        ip, port = me.rsplit(":", 1)
        if me not in self.ref[2]:
            self.ref[1].push(ip, port, bool(self.alive[self.aid[me]]))
            self.ref[2].add(me)
        got = self.oracle.get_or_create_placement(self.ref[0], self.ref[1], me, key[0], key[1])
        self.want(got == want, "the reference restatement places the object elsewhere", key, me, got, want)

    def op_request_batch(self):
        p, other = self.h()
        rng = self.rng
        n = int(rng.choice([2, 3, 7, 40, 256, 257]))
        keys = [self.pick_key(0.5) for _ in range(n)]
        for _ in range(n // 5):
            keys[int(rng.integers(n))] = keys[int(rng.integers(n))]
        mes = [self.pick_addr(0.02) for _ in range(n)]
        self.carry(mes, "request")
        st = self.begin()
        ok = self.intern(st, [(k, True, True, me, True) for k, me in zip(keys, mes)])
        rc, ids, flags = p.get_or_create_placement_batch(keys, mes)
        if not ok:
            return self.refused_unchanged(st, rc, "request_batch")
        self.want(rc == OK, "request_batch failed", rc)
        self.learn_nodes(True)
        col, extra, node, wflag = self.expect_requests(st, keys, mes)
        self.want(ids == [int(x) for x in node], "request_batch: wrong node ids", [(q, ids[q], int(node[q])) for q in range(n) if ids[q] != node[q]][:4])
        self.want(flags == [int(x) for x in wflag], "request_batch: wrong flags", [(q, flags[q], int(wflag[q])) for q in range(n) if flags[q] != wflag[q]][:4])
        self.note_flags(flags, mes)
        self.ref_on = False            # (a batch cleans first and places then: not the reference's order request by request)
        after = self.settle(st, col, extra, "request_batch")
        for k, nd in zip(keys, ids):       # per entry: the ones that were answered with a node
            if nd != NONE:
                self.stamp(k)
        return after

    def op_try_request(self):
        p, other = self.h()
        key, me = self.pick_key(0.95), self.pick_addr(0.0)
        st = self.begin()
        if self.rng.random() < 0.5:
            self.plain_lookup(p, st, key)
        t0 = p.device_round_trips()
        rc, out, flag = p.try_get_or_create_placement(key[0], key[1], me, 512)
        if rc != EAGAIN:
            self.stamp(key, shadow=True)   # (an EAGAIN answer does not stamp)
            want = self.where(st, key)
            self.want(rc == OK and want is not None and out == want, "try_request: wrong address", rc, out, want)
            self.want(self.alive[self.aid[want]] and not self.is_bad(want), "try_request answered for a server that is not an active member")
            self.want(flag == (LOCAL if want == me else REDIRECT), "try_request: wrong flag", flag)
            self.want(p.device_round_trips() == t0, "try_request went to the device")
            self.want(not self.flags & CFG_NO_HOST_SHADOW, "the shadow answered although it is off")
            self.hit("try_* answered from the shadow")
        self.unchanged(st, "try_request")

    def op_set_member(self):
        p, other = self.h()
        rng = self.rng
        a = self.pick_addr(0.08)
        active = bool(rng.random() < 0.65)
        self.carry([a], "member")
        st = self.begin()
        total = int(st["load"][st["col"] != NONE].sum()) if st["n"] else 0
        capv = [INF, INF, max(1, total // max(1, len(self.members))), int(rng.integers(1, 6)), 0][int(rng.integers(5))]
        ok = self.intern(st, [(("", ""), False, False, a, False)])
        rc = p.set_member(a, active, capv)
        if not ok:
            return self.refused_unchanged(st, rc, "set_member")
        self.want(rc == OK, "set_member failed", rc)
        self.learn_nodes(False)
        j = self.aid[a]
        if self.alive[j] and not active and (st["col"] == j).any():
            self.inactive_since.add(j)
        self.alive[j], self.cap[j] = int(active), capv
        if capv != INF:
            self.ref_on = False
        elif self.ref_on and not self.is_bad(a):
            ip, port = a.rsplit(":", 1)
            (self.ref[1].set_is_active if a in self.ref[2] else self.ref[1].push)(ip, port, active)
            self.ref[2].add(a)
        return self.settle(st, st["col"].copy(), [], "set_member")

    def op_set_object_load(self):
        p, other = self.h()
        rng = self.rng
        ahead = rng.random() < 0.5
        key = self.pick_key(0.1 if ahead else 0.95)
        load = int(rng.choice([0, 2, 3, 5, 9])) if self.kstr(key) not in self.keys or self.keys[self.kstr(key)].row is None \
            else int(rng.choice([0, 1, 2, 3, 5, 9]))
        st = self.begin()
        fresh = self.kstr(key) not in self.keys
        ok = self.intern(st, [(key, True, False, None, False)])
        rc = p.set_object_load(key[0], key[1], load)
        if not ok:
            return self.refused_unchanged(st, rc, "set_object_load")
        self.want(rc == OK, "set_object_load failed", rc)
        self.ref_on = False
        if fresh:
            self.set_aside.add(self.kstr(key))
        k = self.keys[self.kstr(key)]
        after = self.read()
        if k.row is None:      # the one row whose load is now `load` and was not: that is the key's row
            nb = st["n"]
            was = np.concatenate([st["load"], np.ones(after["n"] - nb, np.uint32)])
            # (a row reclaimed by this very call was reset to load 1 first: it counts as changed even where its old key's load
            #  was the same number)
            ch = [int(r) for r in np.flatnonzero(after["load"] == load) if after["load"][r] != was[r] or int(r) in self.reset_rows]
            self.want(len(ch) == 1, "set_object_load changed not exactly one row's load", ch)
            self.want(ch[0] not in self.row2key, "set_object_load of a new key wrote the row of another key", ch[0])
            self.new_row(k, self.kstr(key), ch[0])
        self.load_row = k.row
        self.want(after["load"][k.row] == load, "set_object_load: the load is not on the key's row", k.row)
        return self.settle(st, st["col"].copy(), [], "set_object_load")

    def op_tick(self):
        p, other = self.h()
        st = self.begin()
        rc, stats = p.tick()
        self.want(rc == OK, "tick failed", rc)
        self.ref_on = False
        cap, alive = self.node_arrays()
        if st["n"] and len(self.addr):
            nxt, used, ost = self.oracle.tick(st["col"], st["load"], st["aff"], cap, alive, self.rounds, 0)
            self.want(stats == ost, "tick: the counters differ", stats, ost)
        else:
            nxt = st["col"].copy()
        moved = [int(r) for r in np.flatnonzero(nxt != st["col"])]
        for j in list(self.inactive_since):
            if any(st["col"][r] == j for r in moved):
                self.hit("tick evicted from a member turned inactive")
        self.inactive_since = set()
        after = self.settle(st, nxt, [], "tick")
        self.probe(after, [self.row2key[r] for r in moved[:4] if r in self.row2key])
        return after

    def probe(self, st, kss):
        """Right after a call that moved rows the layer cannot name one by one: no call answers a moved key with its old address."""
        for ks in kss:
            k = self.keys.get(ks)
            if k is None:
                continue
            key = (k.ty, k.oid)
            for p in self.handles:
                self.check_lookup(st, p, self.handles[0], key, p.try_lookup, "try_lookup")
                self.check_lookup(st, p, self.handles[0], key, p.lookup, "lookup")

    def op_rebalance(self, order="draw"):
        """rio_op_rebalance, or rio_op_rebalance_ordered in row order, by load or with an order that does not exist."""
        import rebalance_ref
        p, other = self.h()
        if self.mv_clone is not None and self.imm_classes():     # a flag set through one clone, the rebalance through the other
            p, other = self.handles[1 - self.mv_clone], self.handles[self.mv_clone]
        rng = self.rng
        st = self.begin()
        for ks in list(self.keys)[:6]:           # (the shadow holds answers a rebalance must void)
            self.plain_lookup(p, st, (self.keys[ks].ty, self.keys[ks].oid))
        mm = (None, 0, 1, int(rng.integers(2, 6)), int(rng.integers(2, 40)))[int(rng.integers(5))]
        after_fold = order != "draw"
        if order == "draw":
            order = (None, ROW_ORDER, BY_LOAD, BY_LOAD, (2, 7, U32)[int(rng.integers(3))])[int(rng.integers(5))]
        rc, moves = p.rebalance(mm, mid=lambda: other.len(), order=order)
        if order not in (None, ROW_ORDER, BY_LOAD):
            self.want(rc == EINVAL and moves == [], "an order that does not exist was not refused", order, rc, moves[:2])
            self.hit("an invalid order was refused")
            t0 = p.device_round_trips()
            for ks in list(self.keys)[:6]:       # nothing changed: the shadow still holds the answers
                key = (self.keys[ks].ty, self.keys[ks].oid)
                self.check_lookup(st, p, other, key, p.lookup, "lookup")
            self.want(self.flags & CFG_NO_HOST_SHADOW or p.device_round_trips() == t0, "a refused rebalance voided the shadow")
            return self.unchanged(st, "rebalance with an invalid order")
        self.want(rc == OK, "rebalance failed", rc)
        self.ref_on = False
        cap, alive = self.node_arrays()
        budget = min(INF if mm is None else mm, st["n"])
        imm = self.imm_classes()
        self.check_movable_table(imm, "rebalance")      # (before the max_moves 0 call below goes through the same upload)
        if imm and st["n"] and len(self.addr):
            nxt, rows, frm, to = self.rebalance_immovable(st, imm, cap, alive, budget, order, after_fold)
        elif st["n"] and len(self.addr) and order == BY_LOAD:
            import rebalance_order_ref
            import spec_rebalance_order
            L = lambda a: [int(x) for x in a]
            s_nxt, _, _, s_moves = spec_rebalance_order.rebalance(L(st["col"]), L(st["load"]), L(st["aff"]), L(cap), L(alive), None, budget,
                                                                  self.rounds, order=BY_LOAD)
            nxt = np.array(s_nxt, np.uint32)
            rows, frm, to = ([m[q] for m in s_moves] for q in range(3))
            if st["n"] <= 4096:
                r_nxt, _, _, r_rows, r_frm, r_to = rebalance_order_ref.rebalance(st["col"], st["load"], st["aff"], cap, alive, None, budget,
                                                                                  self.rounds, order=BY_LOAD)
                self.want(s_nxt == L(r_nxt) and s_moves == [(int(r), int(f), int(t)) for r, f, t in zip(r_rows, r_frm, r_to)],
                          "the two by-load rebalance references differ")
            self.hit("a by-load rebalance moved keys", len(rows) > 0)
            self.hit("a by-load rebalance right after a fold", after_fold)
        elif st["n"] and len(self.addr):
            nxt, used, wst, rows, frm, to = rebalance_ref.rebalance(st["col"], st["load"], st["aff"], cap, alive, None, budget, self.rounds)
            if st["n"] <= 4096:
                import spec_rebalance
                L = lambda a: [int(x) for x in a]
                s_nxt, _, _, s_moves = spec_rebalance.rebalance(L(st["col"]), L(st["load"]), L(st["aff"]), L(cap), L(alive), None, budget, self.rounds)
                self.want(s_nxt == L(nxt) and s_moves == [(int(r), int(f), int(t)) for r, f, t in zip(rows, frm, to)], "the two rebalance references differ")
        else:
            nxt, rows, frm, to = st["col"].copy(), [], [], []
        want = []
        for r, f, t in zip(rows, frm, to):
            k = self.keys[self.row2key[int(r)]]
            want.append((k.ty, k.oid, self.addr[f], self.addr[t]))
            self.hit("rebalance moved keys of rows that had changed hands", int(r) in self.handed)
        self.want(moves == want, "rebalance: the moves are not the reference's, key for key in row order", order, moves[:4], want[:4])
        if order is not None:      # the two calls share the thread's arrays: the listing above was read before this call, which
            rc, none = p.rebalance(0)      # hands out an empty one and moves nothing (the column is compared below)
            self.want(rc == OK and none == [], "rebalance with max_moves 0 after an ordered one", rc, none[:2])
        after = self.settle(st, nxt, [], "rebalance")
        self.probe(after, [self.row2key[int(r)] for r in rows[:4]])
        if imm:
            # the rebalance has uploaded the classes that changed, as a per-type sweep would have; the keys of the immovable
            # types are where they were, through both clones
            self.reb_upload_step = self.step if self.g.num_objects > self.cls_up or self.cls_scatter else None
            self.class_upload("rebalance")
            held = [int(r) for r in np.flatnonzero(st["col"] != NONE) if int(self.K[r]) in imm]
            self.want(all(after["col"][r] == st["col"][r] for r in held), "rebalance moved a key of an immovable type")
            self.probe(after, [self.row2key[held[int(rng.integers(len(held)))]] for _ in range(3)] if held else [])
        elif self.was_imm:
            self.hit("the last immovable type became movable again and the next rebalance moved its keys",
                     any(int(self.K[int(r)]) in self.was_imm for r in rows))
            self.was_imm = set()
        self.check_movable_table(imm, "after rebalance")
        self.handed_since_reb = set()
        return after

    def check_movable_table(self, imm, what):
        """rio_gp_get_class_movable on the dense handle after a rebalance: the model's table while a type is immovable, all 1
        from the first rebalance after the last one became movable again (and before the first flag)."""
        got = self.g.get_class_movable()
        want = np.ones(spec_classes.MAX_CLASSES, np.uint8)
        want[sorted(imm)] = 0
        self.want(np.array_equal(got, want), what + ": the dense table of immovable classes differs from the model's",
                  np.flatnonzero(got != want)[:8], sorted(imm)[:8])
        if imm:
            self.mv_dev, self.was_imm = True, set(imm)
        else:
            self.mv_dev = False

    def rebalance_immovable(self, st, imm, cap, alive, budget, order, after_fold):
        """A rebalance while a type is immovable: tests/spec_movable.py over the dense state read before the call, the model's own
        class column and the table built from the model's flags (up to 4 096 rows the vectorised reference on the affinity with
        RIO_GP_AFF_INACTIVE on the immovable rows must agree first).  -> (next column, rows, from, to)"""
        import rebalance_order_ref
        import rebalance_ref
        import spec_movable
        n, col, load, aff = st["n"], st["col"], st["load"], st["aff"]
        L = lambda a: [int(x) for x in a]
        table = [0 if c in imm else 1 for c in range(spec_classes.MAX_CLASSES)]
        K = self.K[:n]
        o = BY_LOAD if order == BY_LOAD else ROW_ORDER
        pinned = np.array([int(c) in imm for c in K], bool)
        aff_t = np.where(pinned, np.uint32(AFF_INACTIVE), aff)
        if n <= 4096:
            if o == BY_LOAD:
                r = rebalance_order_ref.rebalance(col, load, aff_t, cap, alive, None, budget, self.rounds, order=BY_LOAD)
            else:
                r = rebalance_ref.rebalance(col, load, aff_t, cap, alive, None, budget, self.rounds)
        s_nxt, _, _, s_moves = spec_movable.rebalance(L(col), L(load), L(aff), L(K), table, L(cap), L(alive), None, budget, self.rounds, o)
        if n <= 4096:
            self.want(s_nxt == L(r[0]) and s_moves == [(int(a), int(b), int(c)) for a, b, c in zip(r[3], r[4], r[5])],
                      "the two immovable rebalance references differ")
        rows, frm, to = ([m[q] for m in s_moves] for q in range(3))
        # the same call without the table: what it would have moved (for the coverage counters only)
        plain = spec_movable.rebalance(L(col), L(load), L(aff), L(K), [1] * spec_classes.MAX_CLASSES, L(cap), L(alive), None, budget,
                                       self.rounds, o)[3]
        used = self.oracle.recompute_used(col, load, len(cap))
        placed = np.flatnonzero(col != NONE)
        over = set(j for j in range(len(cap)) if alive[j] and int(used[j]) > int(cap[j]))
        kept_on = set(int(col[r]) for r in placed if pinned[r]) & over
        self.hit("a rebalance left a key of an immovable type on an over-capacity server and moved another", any(f in kept_on for f in frm))
        self.hit("a by-load rebalance with an immovable type moved keys", o == BY_LOAD and len(rows) > 0)
        self.hit("a by-load rebalance moved keys", o == BY_LOAD and len(rows) > 0)
        self.hit("a by-load rebalance right after a fold", o == BY_LOAD and after_fold)
        self.hit("a row changed hands to a key of an immovable type between two rebalances",
                 any(pinned[r] and col[r] != NONE for r in self.handed_since_reb if r < n))
        self.hit("a type was made immovable before its first key",
                 any(pinned[r] and self.keys[self.row2key[int(r)]].ty in self.early_imm for r in placed))
        self.hit("a flag set through one clone held in a rebalance through the other",
                 self.mv_clone is not None and any(pinned[m[0]] for m in plain))
        return np.array(s_nxt, np.uint32), rows, frm, to

    def op_changes(self):
        p, other = self.h()
        st = self.begin()
        rc, full, entries = p.changes(mid=lambda: self.plain_lookup(other, st, ("T0", "0")))
        self.want(rc == OK, "changes failed", rc)
        self.want(full == (self.feed_state != "open"), "changes: `full` is 1 exactly on the first read and the first after a reset", full, self.feed_state)
        try:
            self.mirror = spec_changes.apply(self.mirror, full, entries, strict=True)
        except AssertionError as e:
            self.fail("changes: the listing does not apply to the mirror", e.args)
        snap = self.model_snapshot(st)
        self.want(self.mirror == snap, "changes: the mirror differs from the snapshot",
                  sorted(set(self.mirror.items()) ^ set(snap.items()), key=repr)[:6])
        # deletes first (apply checked it), each group in row order: by the rows the model knows
        for group in ([e for e in entries if e[3] is None], [e for e in entries if e[3] is not None]):
            rows = []
            for ty, oid, old, new in group:
                ks = self.kstr((ty, oid))
                r = self.keys[ks].row if ks in self.keys and new is not None else self.dropped_since_feed.get(ks, self.keys[ks].row if ks in self.keys else None)
                if r is not None:
                    rows.append(r)
            self.want(rows == sorted(rows), "changes: a group is not in row order", rows[:12])
        self.dropped_since_feed = {}
        self.expired_since_feed = set()
        self.feed_state = "open"
        self.unchanged(st, "changes")

    def op_changes_reset(self):
        p, other = self.h()
        self.want(p.changes_reset() == OK, "changes_reset failed")
        self.feed_state = "reset"
        self.dropped_since_feed = {}
        self.expired_since_feed = set()

    def op_invalidate_cache(self):
        p, other = self.h()
        st = self.begin()
        self.want(p.invalidate_cache() == OK, "invalidate_cache failed")
        key = self.pick_key(1.0)
        rc, found, _ = p.try_lookup(key[0], key[1], 512)
        self.want(rc == EAGAIN or self.kstr(key) not in self.keys, "try_lookup answered right after invalidate_cache", rc)
        self.want(not found, "try_lookup found a key nobody has interned", key)
        self.unchanged(st, "invalidate_cache")

    def op_objects_on_server(self, st=None):
        """The index for every known address, one address that is not a member, and one never seen."""
        p, other = self.h()
        st = st or self.begin()
        for a in list(self.addr) + ["10.250.0.1:1"]:
            rc, objs = p.objects_on_server(a, mid=lambda: other.len())
            self.want(rc == OK, "objects_on_server failed", rc)
            j = self.aid.get(a, NONE - 1)
            want = []
            for r in np.flatnonzero(st["col"] == j):
                k = self.keys[self.row2key[int(r)]]
                want.append((k.ty, k.oid))
            self.want(objs == want, "objects_on_server differs from the model", a, objs[:4], want[:4])

    def op_snapshot(self, st=None):
        p, other = self.h()
        st = st or self.begin()
        rc, snap = p.snapshot(mid=lambda: other.len())
        self.want(rc == OK, "snapshot failed", rc)
        want = self.model_snapshot(st)
        self.want(len(snap) == len(want) and {(a, b): c for a, b, c in snap} == want, "snapshot differs from the model",
                  sorted(set((a, b, c) for a, b, c in snap) ^ spec_changes.as_set(want), key=repr)[:6])

    def op_len(self):
        p, other = self.h()
        st = self.begin()
        rc, n = p.len()
        self.want(rc == OK and n == int((st["col"] != NONE).sum()), "len differs from the placed rows", rc, n)
        if self.ref_on:
            self.want(n == len(self.ref[0]), "len differs from the reference restatement's", n, len(self.ref[0]))

    def op_set_clock(self):
        """The clock the clones share, set through either: it mostly rises, sometimes repeats or falls, sometimes goes back to 0,
        which turns stamping off."""
        p, other = self.h()
        r = self.rng.random()
        if r < 0.15:
            now = 0
        elif r < 0.3:
            now = int(self.rng.integers(0, self.clock_top + 1))
        else:
            now = self.clock_top = self.clock_top + int(self.rng.integers(1, 10))
        self.want(p.set_clock(now) == OK, "set_clock failed")
        self.clock = now
        self.clock_ever = self.clock_ever or now != 0

    def check_seen(self, what):
        """Every sweep uploads the host's stamps (a count-only one too): the one place where they become visible."""
        seen = self.g.get_seen() if self.g.num_objects else np.zeros(0, np.uint32)
        bad = np.flatnonzero(seen != self.S[:len(seen)])
        self.want(bad.size == 0, what + ": the stamps on the device differ from the model's", bad[:8], seen[bad[:8]], self.S[bad[:8]])

    def op_expire(self, by_type=False):
        """rio_op_expire, or (by_type) rio_op_expire_by_type: the same sweep with a cutoff per class."""
        p, other = self.h()
        if by_type and self.limit_clone is not None:      # a limit set through one clone, the sweep through the other
            p, other = self.handles[1 - self.limit_clone], self.handles[self.limit_clone]
        rng = self.rng
        st = self.begin()
        n, col = st["n"], st["col"]
        placed = [int(r) for r in np.flatnonzero(col != NONE)]
        # a witness: a placed key looked up right before the sweep (the shadow holds its answer, and the lookup stamps it)
        wit = None
        if placed:
            k = self.keys[self.row2key[placed[int(rng.integers(len(placed)))]]]
            wit = (k.ty, k.oid)
            self.plain_lookup(p, st, wit)
        cutoff = (0, self.clock, min(self.clock + 1, 0xFFFFFFFF), int(rng.integers(0, self.clock_top + 1)), 0xFFFFFFFF)[int(rng.integers(5))]
        first = not self.clock_ever and rng.random() < 0.5      # (while the clock has never been set: any cutoff > 0, no limit)
        if first:
            cutoff = (1, 0xFFFFFFFF)[int(rng.integers(2))]
        if by_type:
            # now below, at and above the limits (and 0), a default that matters; the cutoff of a class is now - L where that is
            # positive, else 0 — L the type's own limit, or the default without one and for the shared class
            Ls = sorted(set(self.limits.values()) - {U32})
            L0 = Ls[int(rng.integers(len(Ls)))] if Ls else 0
            dflt = (0, 1, int(rng.integers(0, self.clock_top + 2)), U32, L0)[int(rng.integers(5))]
            c = self.clock
            d0 = dflt if dflt != U32 else 0
            now = (0, c, c + L0, c + L0 + 1, c + L0 + 1, max(c + L0 - 1, 0), c + d0 + 1, c + d0 + 1, int(rng.integers(0, self.clock_top + 12)),
                   U32)[int(rng.integers(10))]
            if self.many_types and rng.random() < 0.5:      # most keys are of the shared class: a sweep the default decides
                dflt = int(rng.integers(2))
                now = c + dflt + 1
            now = min(now, U32)
            cutoffs = [now - dflt if now > dflt else 0] * spec_classes.MAX_CLASSES
            for ty, cl in self.types.items():
                if ty in self.limits:
                    cutoffs[cl] = now - self.limits[ty] if now > self.limits[ty] else 0
            sweep = lambda cp: spec_classes.expire_classes(col, self.S, self.K, st["load"], n, cutoffs, cp)[:5]
            cutoff, first = (now, dflt), False
        else:
            sweep = lambda cp: spec_expire.expire(col, self.S, st["load"], n, cutoff, cp)
        idle_rows, _, n_idle, _, _ = sweep(None)
        cap = (None, 0, 1, int(rng.integers(2, 9)), max(n_idle - 1, 0), n_idle, n_idle + 1)[int(rng.integers(7))]
        if first:
            cap = None
        rows, nodes, w_idle, _, A2 = sweep(cap)
        want = []
        for r, nd in zip(rows, nodes):
            ks = self.row2key.get(int(r))
            if ks is None:
                self.fail("a placed row has no key in the model", int(r))
            want.append((self.keys[ks].ty, self.keys[ks].oid, self.addr[nd] if nd < len(self.addr) else None))
        if by_type:
            rc, got, got_idle = p.expire_by_type(now, dflt, cap, mid=lambda: other.len())
        else:
            rc, got, got_idle = p.expire(cutoff, cap, mid=lambda: other.len())
        self.want(rc == OK, "expire failed", rc)
        self.want(got == want, "expire: the listing is not the reference's, key for key in row order", cutoff, cap, got[:4], want[:4])
        self.want(got_idle == w_idle, "expire: n_idle", got_idle, w_idle)
        L = len(rows)
        imm = self.imm_classes()
        self.hit("a sweep listed a key of an immovable type", any(int(self.K[r]) in imm for r in rows))
        if by_type:
            self.hit("a rebalance did the class upload a per-type sweep would have done, and the sweep right after it agreed",
                     self.reb_upload_step is not None and self.reb_upload_step == self.step - 1)
            self.note_type_sweep(st, placed, set(int(r) for r in idle_rows), rows, cutoffs, now, dflt)
        else:
            live = [r for r in placed if int(self.S[r]) >= cutoff]
            self.hit("expire listed keys", L > 0)
            self.hit("expire count only with idle keys", cap == 0 and n_idle > 0)
            self.hit("expire capped below n_idle", 0 < L < n_idle)
            self.hit("sweep with the clock never set listed everything placed", not self.clock_ever and cutoff > 0 and L == len(placed) > 0)
            self.hit("a key stamped only by a shadow hit survived a sweep", cutoff > 0 and any(int(self.S_dev[r]) < cutoff for r in live))
            self.hit("a sweep judged a key by a stamp its row's previous key left",
                     cutoff > 0 and any(r not in self.own and self.S[r] > 0 for r in placed))
            self.hit("expire listed a key set aside by set_object_load", any(self.row2key[int(r)] in self.set_aside for r in rows))
        # the table: rio_op_remove of the listed keys, under the row lifecycle
        xcol = col.copy()
        if L:
            self.oracle.remove_batch(xcol, rows)
        self.want(np.array_equal(xcol, A2[:n]), "the two references differ")
        for ty, oid, _ in want:
            self.ref_key((ty, oid))
            if self.ref_on:
                self.ref[0].remove(ty, oid)
        after = self.settle(st, xcol, [], "expire")
        xaff = st["aff"].copy()
        xaff[rows] = AFF_INACTIVE
        self.want(np.array_equal(after["aff"][:n], xaff), "expire: the affinity column", np.flatnonzero(after["aff"][:n] != xaff)[:8])
        self.check_seen("expire")
        if by_type:
            self.class_upload("expire_by_type")
        self.expired_since_feed |= set(int(r) for r in rows)
        if L:      # (up to three of the listed keys, drawn with repetition)
            self.probe(after, list(dict.fromkeys(self.row2key[int(rows[int(rng.integers(L))])] for _ in range(3))))
        if wit is not None and wit not in [(a, b) for a, b, _ in want]:
            # a key that was not listed is answered as before — with the shadow on, without a device round trip
            t0 = p.device_round_trips()
            self.check_lookup(after, p, other, wit, p.lookup, "lookup")
            self.want(self.flags & CFG_NO_HOST_SHADOW or p.device_round_trips() == t0,
                      "expire: a key that was not listed lost its shadow entry", wit)
        return after

    # ---- classes (include/rio_gpu_object_placement.h, "per-type idle limits and a census by type") ------------------------
    def op_expire_by_type(self):
        return self.op_expire(by_type=True)

    def note_type_sweep(self, st, placed, idle, rows, cutoffs, now, dflt):
        K, S = self.K, self.S
        self.hit("a key of a type past 255 was swept by the default limit", any(int(K[r]) == CLASS_OTHER for r in rows))
        self.hit("a per-type sweep between two feed reads", len(rows) > 0 and self.feed_state == "open")
        young, old = {}, {}      # class -> the youngest stamp listed / the oldest stamp spared (idle rows past the cap are neither)
        for r in rows:
            young[int(K[r])] = max(young.get(int(K[r]), 0), int(S[r]))
        for r in placed:
            if r not in idle:
                old[int(K[r])] = min(old.get(int(K[r]), U32), int(S[r]))
        self.hit("a per-type sweep listed keys of one type and spared older keys of another",
                 any(a != b and old[b] < young[a] for a in young for b in old))
        dcut = now - dflt if now > dflt else 0
        never = set(cl for ty, cl in self.types.items() if self.limits.get(ty) == U32)
        self.hit("IDLE_NEVER spared an idle key", any(int(K[r]) in never and int(S[r]) < dcut for r in placed))
        self.hit("a sweep judged a key by a stamp its row's previous key left",
                 max(cutoffs) > 0 and any(r not in self.own and S[r] > 0 for r in placed))

    def class_upload(self, what):
        """rio_op_expire_by_type and rio_op_census upload the classes the device does not hold yet: afterwards rio_gp_get_classes
        on the dense handle is the model's class column — row for row where the model knows the row's key; a row it cannot map
        (free, or of a key no listing has shown) holds the class of some type."""
        n = self.g.num_objects
        self.hit("a class upload held a range and a scatter in one call", n > self.cls_up and bool(self.cls_scatter))
        self.hit("a row changed hands twice between two class uploads", any(v >= 2 for v in self.cls_handed.values()))
        self.hit("a row changed hands before its first class upload", self.cls_early)
        self.cls_up, self.cls_scatter, self.cls_handed, self.cls_early = n, set(), {}, False
        Kd = self.g.get_classes() if n else np.zeros(0, np.uint8)
        self.want(len(Kd) == n, what + ": the class column's length", len(Kd), n)
        rows = np.array(sorted(self.row2key), np.int64)
        self.want(rows.size == 0 or int(rows[-1]) < n, what + ": the model holds a row past the table's end")
        bad = rows[Kd[rows] != self.K[rows]]
        self.want(bad.size == 0, what + ": the device's classes differ from the model's", bad[:8], Kd[bad[:8]], self.K[bad[:8]],
                  [self.row2key[int(r)] for r in bad[:4]])
        rest = np.ones(n, bool)
        rest[rows] = False
        top = len(self.types)
        odd = np.flatnonzero(rest & (Kd >= top) & ((Kd != CLASS_OTHER) | (top < CLASS_OTHER)))
        self.want(odd.size == 0, what + ": a row holds a class no type has", odd[:8], Kd[odd[:8]], top)

    def op_set_type_idle_limit(self):
        p, other = self.h()
        rng = self.rng
        kind = 2 if self.many_types and rng.random() < 0.4 else int(rng.integers(4))      # (2: past 255 types, often a shared-class one)
        known = list(self.types)
        if kind == 0 and known:
            ty = known[int(rng.integers(len(known)))]
        elif kind == 1 and self.keys:
            ks = list(self.keys.values())
            ty = ks[int(rng.integers(len(ks)))].ty        # (the type of a key: past 255 types it may be in the shared class)
        elif kind == 2:
            ty = self.pool[int(rng.integers(len(self.pool)))][0]
            late = sorted(set(t for t, _ in self.pool if t not in self.types)) if self.many_types else []
            if late:                                      # a type of the pool that has no class yet: past 255 types it never will
                ty = late[int(rng.integers(len(late)))]
        else:
            ty = "N%d\0%d" % (self.seed, self.step) if rng.random() < 0.3 else "N%d.%d" % (self.seed, self.step)      # a new type
        L = (0, 1, U32, U32, int(rng.integers(2, 12)))[int(rng.integers(5))]
        st = self.begin()
        rc = p.set_type_idle_limit(ty, L)
        if ty in self.types or len(self.types) < CLASS_OTHER:
            self.want(rc == OK, "set_type_idle_limit failed", rc, ty)
            self.sight(ty)          # a type never seen before gets its class by this call
            self.limits[ty] = L
            self.limit_clone = self.handles.index(p)
        else:                       # the type lands in the shared class, which has no limit of its own: nothing is set
            self.want(rc == ERANGE, "set_type_idle_limit of a type in the shared class", rc, ty)
            self.hit("a type limit refused with ERANGE")
        self.unchanged(st, "set_type_idle_limit")

    def op_set_type_movable(self):
        """rio_op_set_type_movable_n through either clone: the type of a placed key, any known type, one never seen (it gets its
        class by this call) or — past 255 types — one that lands in the shared class (RIO_GP_ERANGE, nothing set); the flag is drawn,
        repeats included.  The call only notes the flag: the table, the feed and the node table are as they were."""
        p, other = self.h()
        rng = self.rng
        kind = 2 if self.many_types and rng.random() < 0.4 else int(rng.integers(4))
        st = self.begin()
        placed = [int(r) for r in np.flatnonzero(st["col"] != NONE)]
        known = list(self.types)
        if kind == 0 and placed:
            ty = self.keys[self.row2key[placed[int(rng.integers(len(placed)))]]].ty
        elif kind == 1 and known:
            ty = known[int(rng.integers(len(known)))]
        elif kind == 2:
            ty = self.pool[int(rng.integers(len(self.pool)))][0]
            late = sorted(set(t for t, _ in self.pool if t not in self.types)) if self.many_types else []
            if late:                                      # a type of the pool that has no class yet: past 255 types it never will
                ty = late[int(rng.integers(len(late)))]
        else:
            ty = "M%d\0%d" % (self.seed, self.step) if rng.random() < 0.3 else "M%d.%d" % (self.seed, self.step)      # a new type
            unseen = [k for k in self.pool if k[0] not in self.types]
            if unseen and rng.random() < 0.6:             # ... or one of the pool's, whose first key comes with the next call
                self.force_key = unseen[int(rng.integers(len(unseen)))]
                ty = self.force_key[0]
        if self.immovable and rng.random() < 0.25:       # a flag some type holds already, given again or taken back
            ty, self.force_key = list(self.immovable)[int(rng.integers(len(self.immovable)))], None
        movable = bool(rng.random() < (0.6 if self.immovable.get(ty) else 0.45))
        now = [t for t, on in self.immovable.items() if on]
        if self.mv_dev and len(now) == 1 and rng.random() < 0.4:      # the last immovable type becomes movable again
            ty, movable, self.force_key = now[0], True, None
        if movable:
            self.force_key = None
        rc = p.set_type_movable(ty, movable)
        if ty in self.types or len(self.types) < CLASS_OTHER:
            self.want(rc == OK, "set_type_movable failed", rc, ty)
            if ty not in self.types and not movable:
                self.early_imm.add(ty)
            self.sight(ty)          # a type never seen before gets its class by this call
            self.immovable[ty] = not movable
            self.mv_clone = self.handles.index(p)
        else:                       # the type lands in the shared class, which is always movable: nothing is set
            self.want(rc == ERANGE, "set_type_movable of a type in the shared class", rc, ty)
            self.hit("set_type_movable refused with ERANGE")
        self.unchanged(st, "set_type_movable")

    def feed_peek(self):
        """What the dense feed would list, the checkpoint left where it is."""
        if not self.g.num_objects:
            return None
        rows, old, new, total = self.g.changes(peek=True)
        return rows.tolist(), old.tolist(), new.tolist(), int(total)

    def witness(self, p, st):
        """A placed key looked up right before a call that must leave the shadow alone."""
        placed = np.flatnonzero(st["col"] != NONE)
        if not placed.size:
            return None
        k = self.keys[self.row2key[int(placed[int(self.rng.integers(placed.size))])]]
        self.plain_lookup(p, st, (k.ty, k.oid))
        return (k.ty, k.oid)

    def still_in_shadow(self, p, other, st, wit, what):
        if wit is None:
            return
        t0 = p.device_round_trips()
        self.check_lookup(st, p, other, wit, p.lookup, "lookup")
        self.want(self.flags & CFG_NO_HOST_SHADOW or p.device_round_trips() == t0, what + ": a key lost its shadow entry", wit)

    def op_census(self):
        p, other = self.h()
        st = self.begin()
        by = bool(self.rng.random() < 0.6)
        wit = self.witness(p, st)
        feed = self.feed_peek()
        rc, got = p.census(by, mid=lambda: other.len())
        self.want(rc == OK, "census failed", rc)
        n, m = st["n"], len(self.addr)
        name = {cl: ty for ty, cl in self.types.items()}      # (the shared class has no name)
        if by:
            rows, lsum, _ = spec_classes.census(st["col"], self.K, st["load"], n, spec_classes.MAX_CLASSES, m)
            want = [(name.get(c), self.addr[j], rows[j][c], lsum[j][c]) for j in range(m) for c in range(spec_classes.MAX_CLASSES) if rows[j][c]]
        else:
            rows, lsum, _ = spec_classes.census(st["col"], self.K, st["load"], n, spec_classes.MAX_CLASSES)
            want = [(name.get(c), None, rows[c], lsum[c]) for c in range(spec_classes.MAX_CLASSES) if rows[c]]
        self.want(got == want, "census: the entries are not the reference's, in server and class order", by,
                  [(g, w) for g, w in zip(got, want) if g != w][:3], len(got), len(want))
        self.want(sum(e[2] for e in got) == int((st["col"] != NONE).sum()), "census: the rows do not sum to the placed keys")
        self.hit("census listed the shared class", any(e[0] is None for e in got))
        self.hit("census by server with a server seen only through update", by and any(self.seen_by.get(e[1]) == {"update"} for e in got))
        # read-only: the table, the feed and the shadow as they were (nothing stamped or counted: the model did neither, and the
        # next sweep and the next fold compare the stamps and the counters as a whole)
        self.unchanged(st, "census")
        self.want(self.feed_peek() == feed, "census changed the feed")
        self.still_in_shadow(p, other, st, wit, "census")
        self.class_upload("census")

    # ---- measured load (include/rio_gpu_object_placement.h, "measured load") ---------------------------------------------
    def op_set_load_tracking(self):
        p, other = self.h()
        on = bool(self.rng.random() < 0.75)
        self.want(p.set_load_tracking(on) == OK, "set_load_tracking failed")
        self.tracking = on
        self.track_off = self.track_off or not on

    def op_get_object_load(self):
        p, other = self.h()
        rng = self.rng
        st = self.begin()
        kind = int(rng.integers(5))
        if kind == 0:
            key = ("never", "%d.%d" % (self.seed, self.step))
        elif kind == 1 and self.last_dropped:
            key = self.last_dropped[-1 - int(rng.integers(min(4, len(self.last_dropped))))]       # a key whose row was reclaimed
        elif kind == 2:
            key = (("a.b", "c"), ("a", "b.c"))[int(rng.integers(2))]
        else:
            key = self.pick_key(0.9)
        rc, load = p.get_object_load(key[0], key[1])
        self.want(rc == OK, "get_object_load failed", rc)
        k = self.keys.get(self.kstr(key))
        want = None if k is None else 1 if k.row is None or k.row >= st["n"] else int(st["load"][k.row])
        self.want(load == want, "get_object_load: not the dense column's load at the key's row", key, load, want)
        self.hit("get_object_load of a key never seen", k is None)
        self.unchanged(st, "get_object_load")      # (it stamps and counts nothing: the next sweep and the next fold compare both)

    def learn_unplaced_rows(self, p):
        """The rows of the keys no listing has shown (they are not placed), so that a fold is compared key for key: the one row
        whose load changes under rio_op_set_object_load, which is put back at once.  Such a key holds load 1 (a fresh or a
        recycled row, and every earlier fold was preceded by this), and the requests counted for it move to its row."""
        for ks, k in list(self.keys.items()):
            if k.row is not None:
                continue
            rc, old = p.get_object_load(k.ty, k.oid)
            self.want(rc == OK and old == 1, "get_object_load of a key that was never placed or loaded", ks, rc, old)
            l0 = self.g.get_objects()[0]
            self.want(p.set_object_load(k.ty, k.oid, 0) == OK, "set_object_load failed", ks)
            l1 = self.g.get_objects()[0]
            ch = [int(r) for r in np.flatnonzero(l1 != l0)] if len(l1) == len(l0) else []
            self.want(len(ch) == 1 and ch[0] not in self.row2key, "set_object_load changed not exactly one row's load, a row without a key", ks, ch[:4])
            self.want(p.set_object_load(k.ty, k.oid, 1) == OK, "set_object_load failed", ks)
            self.new_row(k, ks, ch[0])

    def op_fold_loads(self):
        p, other = self.h()
        rng = self.rng
        self.learn_unplaced_rows(p)
        st = self.begin()
        wit = self.witness(p, st)
        r = rng.random()
        keeps, gains = (0, 1, 32768, 65535, KEEP_ONE), (0, 1, 7, U32)
        if r < 0.3:
            par = (KEEP_ONE, 1, 0, U32)          # every counter visible as load + requests
        elif r < 0.42:
            par = ((KEEP_ONE + 1, 1, 0, U32), (U32, 0, 0, U32), (KEEP_ONE, 1, 5, 4), (0, 7, U32, 0))[int(rng.integers(4))]
        elif r < 0.7:
            par = (keeps[int(rng.integers(5))], gains[int(rng.integers(4))], 0, U32)
        else:                                    # clamps that bite from either side, and min_load == max_load
            lo, hi = ((0, 3), (5, U32), (2, 2), (1, 1), (0, 0), (3, 9))[int(rng.integers(6))]
            par = (keeps[int(rng.integers(5))], gains[int(rng.integers(4))], lo, hi)
        keep, gain, lo, hi = par
        self.want(not self.unknown_hits, "requests are left for keys without a row", list(self.unknown_hits)[:4])
        total = int(self.Hc.sum())
        seen0 = self.g.get_seen() if st["n"] else None
        feed = self.feed_peek()
        rc, changed, folded = p.fold_loads(keep, gain, lo, hi)
        after = self.read()
        n = after["n"]      # (rows a refused call interned reach the device with this call: fresh rows, load 1)
        before = np.concatenate([st["load"], np.ones(n - st["n"], np.uint32)])
        hits = self.g.get_hits() if n else np.zeros(0, np.uint32)
        if keep > KEEP_ONE or lo > hi:
            self.want(rc == EINVAL and (changed, folded) == (0, 0), "a fold that must be refused", par, rc, changed, folded)
            self.want(np.array_equal(after["load"], before) and not hits.any(), "a refused fold changed the loads or the device's counters")
            self.unchanged(st, "a refused fold")
            self.refused_fold = self.refused_fold or total > 0      # (the counters stand: the next legal fold finds them)
            if rng.random() < 0.5:
                self.log.append("fold_loads (after a refusal)")
                self.op_fold_loads()
            return
        self.want(rc == OK, "fold_loads failed", rc, par)
        H = np.minimum(self.Hc[:n], U32).astype(np.uint32)
        new, _, _ = spec_loads.load_fold(before, H, n, keep, gain, lo, hi)
        mapped = np.array(sorted(self.row2key), np.int64)
        self.want(mapped.size == 0 or int(mapped[-1]) < n, "the model holds a row past the table's end")
        bad = mapped[after["load"][mapped] != new[mapped]]
        self.want(bad.size == 0, "fold_loads: the loads are not load_fold's over the model's counters", par, bad[:8],
                  before[bad[:8]], H[bad[:8]], after["load"][bad[:8]], new[bad[:8]])
        # rows the model cannot map to a key belong to none (learn_unplaced_rows above): free rows, load 1 before and after,
        # whatever keep and the clamps are
        rest = np.ones(n, bool)
        rest[mapped] = False
        free = int(rest.sum())
        self.want((before[rest] == 1).all() and (after["load"][rest] == 1).all(), "fold_loads: a row that belongs to no key does not hold load 1",
                  par, np.flatnonzero(rest & ((before != 1) | (after["load"] != 1)))[:8], before[rest][:8], after["load"][rest][:8])
        w_changed = int((new[mapped] != before[mapped]).sum())
        self.want(changed == w_changed, "fold_loads: rows_changed counts the keys whose load differs", par, changed, w_changed, free)
        self.want(folded == total, "fold_loads: hits_folded is not the requests the model counted", folded, total)
        self.want(not hits.any(), "fold_loads left counters on the device", np.flatnonzero(hits)[:8])
        used = spec_loads.used_of(after["col"], after["load"], n, after["m"]) if after["m"] else np.zeros(0, np.uint64)
        self.want(np.array_equal(after["used"], used), "fold_loads: `used` differs", after["used"], used)
        self.want(np.array_equal(after["col"][:st["n"]], st["col"]) and (after["col"][st["n"]:] == NONE).all() and
                  np.array_equal(after["aff"][:st["n"]], st["aff"]), "fold_loads changed the column or the affinity")
        self.want(seen0 is None or np.array_equal(self.g.get_seen()[:st["n"]], seen0), "fold_loads changed the stamps")
        self.want(self.feed_peek() == feed, "fold_loads changed the feed")
        self.share[1] += int((self.Hc[:n] != 0).sum())      # (share[0]: counters on rows the model does not know — none, see above)
        free_load = max(lo, min(hi, 1 if keep == KEEP_ONE else 0))
        self.hit("a fold saw a row that had changed hands since the last fold, with requests counted for its previous key",
                 any(r in self.row2key for r in self.lost_hits))
        self.hit("a fold with a non-empty free list and a free-row result other than 1", free > 0 and free_load != 1)
        self.hit("a fold counted requests of shadow hits", bool(self.Hs.any()))
        self.hit("a fold with the clock never set", not self.clock_ever and total > 0)
        self.hit("a refused fold kept its counters for the next one", self.refused_fold)
        self.hit("a fold changed no load", changed == 0)
        self.hit("tracking switched off between two folds", self.track_off and self.count.get("fold_loads", 0) > 1)
        self.Hc[:] = 0
        self.Hs[:] = 0
        self.unknown_hits, self.lost_hits, self.refused_fold, self.track_off = {}, set(), False, False
        self.still_in_shadow(p, other, after, wit, "fold_loads")      # (a request of the next period)
        if rng.random() < 0.25:      # the call to make after a fold: the loads are skewed now
            self.log.append("rebalance (after fold)")
            self.op_rebalance(order=BY_LOAD)

    # ---- hot objects (include/rio_gpu_object_placement.h, "hot objects") ---------------------------------------------------
    def op_hottest_objects(self):
        p, other = self.h()
        rng = self.rng
        st = self.begin()
        n, col, load = st["n"], st["col"], st["load"]
        placed = [int(r) for r in np.flatnonzero(col != NONE)]
        wit = self.witness(p, st)
        only_update = [a for a in self.addr if self.seen_by.get(a) == {"update"}]
        kind = int(rng.integers(10))
        if kind < 4:
            a = None                                        # every server
        elif kind == 4 and only_update:
            a = only_update[int(rng.integers(len(only_update)))]
        elif kind == 5:
            a = "10.251.%d.1:1" % (self.seed % 200)         # an address never seen
        elif kind == 6:
            a = self.odd[int(rng.integers(2))]              # a malformed one (a server like any other once it is known)
        else:
            a = self.members[int(rng.integers(len(self.members)))]
        x = int(load[placed[int(rng.integers(len(placed)))]]) if placed else 1
        min_load = (0, 1, x, min(x + 1, U32), U32)[int(rng.integers(5))]
        keys, where, ld = [], {}, {}
        for r in placed:
            k = self.keys[self.row2key[r]]
            keys.append((k.ty, k.oid))
            where[(k.ty, k.oid)] = self.addr[col[r]] if col[r] < len(self.addr) else None
            ld[(k.ty, k.oid)] = int(load[r])
        if a is None:
            full, nc = spec_top.op_hottest(keys, where, ld, None, min_load, len(keys) + 1)
        else:          # (spec_top selects by address: an address nobody was given an id for holds nothing)
            full, nc = spec_top.op_hottest(keys, where, ld, a, min_load, len(keys) + 1) if a in self.aid else ([], 0)
        ties = [i for i in range(1, len(full)) if full[i - 1][3] == full[i][3] and i <= TOP_MAX]
        tie = ties[int(rng.integers(len(ties)))] if ties else 1
        cap = (0, 1, tie, tie, max(nc - 1, 0), nc, nc + 1, TOP_MAX, TOP_MAX + 1)[int(rng.integers(9))]
        if cap != TOP_MAX + 1:
            cap = min(cap, TOP_MAX)
        rc, got, got_nc = p.hottest_objects(a, min_load, cap, mid=lambda: other.len())
        if cap > TOP_MAX:
            self.want(rc == EINVAL, "hottest_objects above RIO_GP_TOP_MAX was not refused", rc)
            return self.unchanged(st, "a refused hottest_objects")
        self.want(rc == OK, "hottest_objects failed", rc)
        self.want(got == full[:cap], "hottest_objects: the listing is not the reference's (load descending, ties in row order)",
                  a, min_load, cap, got[:4], full[:4])
        self.want(got_nc == nc, "hottest_objects: n_candidates", got_nc, nc)
        # ... and the dense layer's own restatement over the dense state
        flags = spec_top.PLACED | (spec_top.ON_NODE if a is not None else 0)
        if a is None or a in self.aid:
            rows, kk, nodes, d_nc, _ = spec_top.top_rows(col, load, None, n, flags, self.aid.get(a, 0), min_load, cap)
            dense = [(self.keys[self.row2key[int(r)]].ty, self.keys[self.row2key[int(r)]].oid,
                      self.addr[nd] if nd < len(self.addr) else None, int(v)) for r, v, nd in zip(rows, kk, nodes)]
            self.want(got == dense and got_nc == d_nc, "hottest_objects disagrees with top_rows over the dense state", got[:4], dense[:4])
        self.hit("hottest cut inside a tie group", 0 < cap < nc and full[cap - 1][3] == full[cap][3])
        self.hit("hottest on an address never seen", a is not None and a not in self.aid)
        self.unchanged(st, "hottest_objects")       # read-only: nothing stamped or counted (the model did neither), the shadow intact
        self.still_in_shadow(p, other, st, wit, "hottest_objects")

    # ---- the run ------------------------------------------------------------------------------------------------------
    def setup(self):
        rng = self.rng
        self.ever_rows = set()
        self.ref = (self.oracle.LocalObjectPlacement(), self.oracle.LocalStorage(), set())
        self.begin()
        caps = int(rng.integers(3))      # 0: unbounded for a while (the reference cross-check), 1: tight from the start, 2: mixed
        for a in self.members:
            self.log.append("set_member")
            self.carry([a], "member")
            st = self.begin()
            self.intern(st, [(("", ""), False, False, a, False)])
            capv = INF if caps == 0 else int(rng.integers(1, 5)) if caps == 1 else [INF, 3, 0][int(rng.integers(3))]
            self.want(self.handles[0].set_member(a, True, capv) == OK, "set_member failed")
            self.learn_nodes(False)
            self.alive[self.aid[a]], self.cap[self.aid[a]] = 1, capv
            ip, port = a.rsplit(":", 1)
            self.ref[1].push(ip, port, True)
            self.ref[2].add(a)
            if capv != INF:
                self.ref_on = False
            self.settle(st, st["col"].copy(), [], "set_member")
        if self.kind == "bulk":          # the table loaded in one update_batch, as a snapshot is
            n = self.rows_max - 200
            keys = [("B", str(k)) for k in range(n)]
            addrs = [self.members[k % len(self.members)] for k in range(n)]
            self.log.append("update_batch (bulk)")
            st = self.begin()
            self.intern(st, [(k, True, True, a, False) for k, a in zip(keys, addrs)])
            self.want(self.handles[0].update_batch(keys, addrs) == OK, "bulk update_batch failed")
            idx, col, load, extra = self.virtual(st, keys)
            self.oracle.update_batch(col, len(self.addr), idx, [self.aid[a] for a in addrs])
            for k, a in zip(keys, addrs):
                self.ref[0].update(k[0], k[1], a)
            self.settle(st, col, extra, "update_batch (bulk)")
        if self.many_types:              # 280 keys of as many types in one batch: 255 numbered classes and the shared one
            keys = self.pool[:280]
            addrs = [self.members[k % len(self.members)] for k in range(len(keys))]
            self.log.append("update_batch (types)")
            st = self.begin()
            self.intern(st, [(k, True, True, a, False) for k, a in zip(keys, addrs)])
            self.want(self.handles[1].update_batch(keys, addrs) == OK, "the types' update_batch failed")
            idx, col, load, extra = self.virtual(st, keys)
            self.oracle.update_batch(col, len(self.addr), idx, [self.aid[a] for a in addrs])
            for k, a in zip(keys, addrs):
                self.ref[0].update(k[0], k[1], a)
            self.settle(st, col, extra, "update_batch (types)")

    def run(self):
        names = [a for a, w in self.OPS for _ in range(w)]
        try:
            self.setup()
            for self.step in range(self.steps):
                op = names[int(self.rng.integers(len(names)))]
                if self.reb_upload_step is not None and self.reb_upload_step == self.step - 1 and self.rng.random() < 0.5:
                    op = "expire_by_type"      # the sweep right behind a rebalance that did the class upload
                elif self.force_key is not None:
                    op = "update"              # the first key of a type that was made immovable before it
                elif self.mv_dev and not self.imm_classes() and self.rng.random() < 0.5:
                    op = "rebalance"           # the rebalance that resets the dense table
                self.log.append(op)
                self.count[op] = self.count.get(op, 0) + 1
                getattr(self, "op_" + op)()
                if self.kind == "tiny" or self.step % 8 == 7:
                    st = self.read()
                    self.op_objects_on_server(st)
                    self.op_snapshot(st)
            st = self.read()
            self.op_objects_on_server(st)
            self.op_snapshot(st)
            rc, got, _ = self.handles[0].expire(0, 0)       # the stamps of the whole run, uploaded by a count-only sweep
            self.want(rc == OK and got == [], "a count-only sweep failed or listed something", rc, got[:4])
            self.check_seen("the end")
            self.op_changes()
        finally:
            for h in self.handles[::-1]:
                h.close()
        return self.steps


def run_seed(make, oracle, seed, steps=None):
    sc = Scenario(make, oracle, seed, steps)
    sc.run()
    return sc
