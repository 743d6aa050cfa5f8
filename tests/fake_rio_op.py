"""A plain-Python stand-in for the string layer (rio_op_*, rio-rs_amd/csrc/gpu_object_placement.cpp), FOR TESTS ONLY: what
include/rio_gpu_object_placement.h documents, over a row-lifecycle dense table built on tests/fake_rio_gp.py — a dict interner,
lazy reclaim when the table runs full, rows kept for rio_op_set_object_load, a host shadow by stamp, the feed's retired rows,
the flags of immovable types and their lazy upload ahead of a rebalance.
It lets tests/op_layer_driver.py be tested without a GPU (tests/test_op_layer_driver.py): `fault=` makes exactly one behaviour
wrong, and the driver must notice.  It is not a CPU backend: nothing under rio-rs_amd/ imports it.

It offers the surface the driver's adapter offers (op_layer_driver.RealProvider): return codes instead of exceptions, and
`mid` callbacks where the real adapter reads thread-owned arrays after an intervening call.
"""
import numpy as np

import fake_rio_gp
from fake_rio_gp import AFF_INACTIVE, CAP_INF, EAGAIN, EINVAL, ERANGE, NONE, OK, TOP_MAX

U32 = 0xFFFFFFFF

CFG_LIVE_FIRST_TOUCH, CFG_NO_HOST_SHADOW = 4, 8
FLAG_REPLACED = 0x10

FAULTS = (
    "spill_wrong_node",            # a request whose first choice is full spills to another node than the solver says
    "rebalance_key_order",         # rebalance lists its moves in key order, not row order
    "rebalance_keeps_shadow",      # rebalance does not invalidate the host shadow
    "feed_forgets_retired",        # a reclaimed row's old key is not deleted in the feed
    "index_lists_reclaimed",       # objects_on_server names the key a reused row had before it was reclaimed
    "kept_row_recycled",           # a row set aside by set_object_load is recycled
    "update_batch_first_wins",     # update_batch applies duplicates in the wrong order
    "reset_not_full",              # `full` is not raised after changes_reset
    "expire_keeps_shadow_entry",   # a sweep leaves the shadow's answer for the keys it listed
    "expire_drops_whole_shadow",   # a sweep that listed keys voids every shadow entry, not only theirs
    "shadow_hit_does_not_stamp",   # a lookup or request the shadow answers does not stamp
    "remove_stamps",               # a remove stamps the key
    "clone_has_its_own_clock",     # set_clock through one clone does not reach the calls made through the other
    "reclaim_resets_stamp",        # a reclaimed row's stamp goes back to 0
    "expire_cutoff_inclusive",     # a key stamped exactly at the cutoff is idle
    "expire_listing_not_in_row_order",   # the listing comes out in reverse
    "stamps_not_uploaded_on_count_only",  # a count-only sweep does not hand the stamps to the dense layer
    # measured load
    "reclaim_keeps_counter",       # a reclaimed row keeps the requests counted for its previous key
    "shadow_hit_not_counted",      # a lookup or request the shadow answers counts no request
    "remove_counts_request",       # a remove counts a request
    "tracking_per_clone",          # set_load_tracking through one clone does not reach the calls made through the other
    "fold_leaves_free_rows",       # a fold leaves the rows on the free list at the folded value
    "rows_changed_counts_free_rows",   # rows_changed counts rows that belong to no key
    "refused_fold_drops_counters",  # a refused fold forgets the requests counted so far
    "hits_folded_after_clamp",     # hits_folded is worked out from the clamped loads
    "get_object_load_stamps",      # get_object_load stamps and counts like a lookup
    # hot objects
    "hottest_ties_by_key",         # keys of equal load come in key order, not row order
    "hottest_ignores_min_load_per_server",   # min_load is ignored when an address is given
    "hottest_lists_unplaced",      # keys that are not placed are listed
    # the by-load cut
    "by_load_runs_row_order",      # RIO_GP_REBALANCE_BY_LOAD is silently run as row order
    "invalid_order_runs_row_order",  # an invalid order is not refused
    # classes
    "reclaimed_row_keeps_class",   # a row handed to a key of another type keeps its old key's class
    "class_range_starts_late",     # the upload of the new rows' classes starts one row late
    "class_from_current_spelling",  # a key's class follows the struct_name of the call, not the one it was first interned with
    "type_256_gets_a_limit",       # a type in the shared class is given a limit of its own (it becomes the shared class's)
    "type_cutoff_wraps",           # now - L wraps around where now < L
    "idle_never_is_zero",          # RIO_OP_IDLE_NEVER is taken as a limit of 0
    "census_lists_empty_cells",    # census by server lists the empty cells of the types a server does not hold
    "census_names_shared_class",   # the shared class comes with a name
    "expire_by_type_keeps_shadow_entry",   # a per-type sweep leaves the shadow's answer for the keys it listed
    # immovable types
    "movable_classes_not_uploaded",   # a rebalance with an immovable type sends the table, the classes that changed it does not
    "movable_table_uploaded_once",    # the table goes to the dense layer the first time only: later changes of a flag stay on the host
    "movable_never_reset",         # after the last immovable type became movable again the dense table is left as it was
    "movable_flag_per_clone",      # a flag set through one clone does not reach a rebalance made through the other
    "movable_other_class_accepted",   # a type in the shared class is accepted: the shared class becomes immovable
    "movable_unseen_type_not_numbered",   # the call does not number a type never seen before (and drops its flag)
    "movable_ordered_call_ignores",   # rio_op_rebalance_ordered runs without the table
    "movable_upload_clears_sweep_state",   # after a rebalance's class upload the next per-type sweep runs on the classes of before it
)


def _oracle():
    import pyoracle
    return pyoracle


class LifeDense(fake_rio_gp.GpuPlacement):
    """fake_rio_gp.GpuPlacement under RIO_GP_CFG_ROW_LIFECYCLE: the CRUD calls keep the affinity column (include/rio_gpu_placement.h)."""

    def __init__(self, max_objects, max_nodes, spill_rounds, self_assign, fault=None):
        super().__init__(max_objects, max_nodes, spill_rounds=spill_rounds, flags=fake_rio_gp.CFG_REF_SELF_ASSIGN if self_assign else 0)
        self._op_fault = fault
        self._aff[:] = AFF_INACTIVE
        self._col[:] = NONE

    def set_self_assign(self, on):
        self._oflags = _oracle().REF_SELF_ASSIGN if on else 0

    def update_batch(self, idx, node):
        idx, node = np.asarray(idx, np.uint32), np.asarray(node, np.uint32)
        super().update_batch(idx, node)
        for i, nd in zip(idx, node):
            self._aff[i] = AFF_INACTIVE if nd == NONE else nd

    def remove_batch(self, idx):
        super().remove_batch(idx)
        self._aff[np.asarray(idx, np.uint32)] = AFF_INACTIVE

    def clean_server(self, node):
        hit = np.flatnonzero(self._col[:self._n] == np.uint32(node))
        self._aff[hit] = AFF_INACTIVE
        return super().clean_server(node)

    def place_pending(self, idx, requester):
        idx, requester = np.asarray(idx, np.uint32), np.asarray(requester, np.uint32)
        col = self._col[:self._n]
        before = col.copy()
        node, flag = super().place_pending(idx, requester)
        if self._op_fault == "spill_wrong_node":
            live = np.flatnonzero(self._alive)
            for k in range(len(idx)):
                if flag[k] & 0xF == 3 and len(live) > 1:
                    other = int(live[(int(np.searchsorted(live, node[k])) + 1) % len(live)])
                    col[idx[k]] = other
                    for q in range(len(idx)):
                        if idx[q] == idx[k]:
                            node[q] = other
        dead = set()
        seen = set()
        for k in range(len(idx)):
            c = before[idx[k]]
            if c != NONE and c < self._m and not self._alive[c]:
                dead.add(int(c))
        if dead:
            self._aff[:self._n][np.isin(before, list(dead))] = AFF_INACTIVE
        for k in range(len(idx)):
            i = int(idx[k])
            if i in seen:
                continue
            seen.add(i)
            c = before[i]
            if c == NONE or int(c) in dead:
                self._aff[i] = requester[k]
        return node, flag

    def get_objects(self):
        return self._load[:self._n].copy(), self._aff[:self._n].copy()

    def _expire(self, cutoff, cap):
        out = super()._expire(cutoff, cap)
        self._aff[out[0]] = AFF_INACTIVE      # an expired row is no longer an object
        return out

    def _expire_classes(self, cutoffs, cap):
        out = super()._expire_classes(cutoffs, cap)
        self._aff[out[0]] = AFF_INACTIVE
        return out

    def count_placed(self):
        return int((self._col[:self._n] != NONE).sum())


class _State:
    pass


class FakeObjectPlacement:
    def __init__(self, max_objects, max_nodes=32, spill_rounds=2, flags=0, fault=None, _s=None):
        if _s is not None:
            self.s = _s
            self.own_now, self.own_track, self.own_imm = 0, False, {}
            return
        assert fault is None or fault in FAULTS, fault
        s = self.s = _State()
        s.fault = fault
        s.max_objects, s.max_nodes = int(max_objects), int(max_nodes)
        s.self_assign = not flags & CFG_LIVE_FIRST_TOUCH
        s.shadow_on = not flags & CFG_NO_HOST_SHADOW
        s.g = LifeDense(max_objects, max_nodes, spill_rounds or 2, s.self_assign, fault)
        s.g.set_nodes(np.zeros(0, np.uint64), np.zeros(0, np.uint8), m=0)
        s.g.set_num_objects(0)
        s.rows, s.row_key, s.row_live, s.row_keep, s.free, s.stale_key = {}, [], [], [], [], []
        s.nodes, s.addr, s.alive, s.cap, s.bad = {}, [], [], [], []
        s.pushed = (0, 0)
        s.shadow, s.clock, s.base, s.clean_stamp = {}, 1, 1, {}
        s.feed_on, s.feed_full, s.retired = False, True, {}
        s.trips = [0, 0]
        s.last_len = 0
        s.now, s.stamps = 0, np.zeros(s.max_objects, np.uint32)     # the clock every clone stamps with; one stamp per row
        s.track, s.hits = False, np.zeros(s.max_objects, np.uint64)  # the tracking switch the clones share; one counter per row
        # struct_name -> class in the order of interning, limit by class, the class of every row, and what the device holds of it
        s.types, s.type_names, s.type_limit, s.row_class, s.cls_uploaded, s.cls_dirty = {}, [], {}, [], 0, []
        # immovable types: the flag by class, whether the table changed since its last upload, whether the dense layer holds one
        s.type_imm, s.mv_dirty, s.mv_on_device, s.mv_sent, s.stale_cls = {}, False, False, False, None
        self.own_now, self.own_track, self.own_imm = 0, False, {}

    def clone(self):
        return FakeObjectPlacement(0, _s=self.s)

    def close(self):
        pass

    def dense(self):
        return self.s.g

    # ---- tables
    @staticmethod
    def _key(ty, oid):
        return ty + "." + oid

    def _sync(self):
        s = self.s
        if s.pushed != (len(s.addr), tuple(s.alive), tuple(s.cap)):
            s.g.set_nodes(np.array(s.cap, np.uint64), np.array(s.alive, np.uint8), m=len(s.addr))
            s.pushed = (len(s.addr), tuple(s.alive), tuple(s.cap))
        if s.g.num_objects != len(s.row_key):
            s.g.set_num_objects(len(s.row_key))

    def _node(self, a, create, up=False):
        s = self.s
        if a in s.nodes:
            return s.nodes[a]
        if not create:
            return NONE
        if len(s.addr) >= s.max_nodes:
            return EINVAL - 100
        s.nodes[a] = len(s.addr)
        s.addr.append(a)
        s.alive.append(1 if up else 0)
        s.cap.append(CAP_INF)
        c = a.find(":")
        s.bad.append(c < 0 or c == 0 or c + 1 >= len(a))
        return s.nodes[a]

    def _row(self, ty, oid, create, use=False):
        """-> row, NONE (unknown, not created) or "full"."""
        s = self.s
        k = self._key(ty, oid)
        if k in s.rows:
            r = s.rows[k]
            if use:
                s.row_keep[r] = 0
            if s.fault == "class_from_current_spelling" and create:
                self._set_class(r, self._type(ty))
            return r
        if not create:
            return NONE
        if s.free:
            r = s.free.pop()
        elif len(s.row_key) < s.max_objects:
            r = len(s.row_key)
            s.row_key.append(None)
            s.row_live.append(0)
            s.row_keep.append(0)
            s.row_class.append(0)
            s.stale_key.append((ty, oid))
        else:
            return "full"
        c = self._type(ty)
        if not (s.fault == "reclaimed_row_keeps_class" and r < s.cls_uploaded):
            self._set_class(r, c)
        s.rows[k] = r
        s.row_key[r] = (ty, oid)
        s.row_live[r] = 1
        s.row_keep[r] = 0 if use else 1
        return r

    # ---- classes
    def _type(self, ty):
        """The class of a struct_name: the next number when it is new and one is left, else the shared class."""
        s = self.s
        if ty not in s.types:
            if len(s.type_names) >= 255:
                return 255
            s.types[ty] = len(s.type_names)
            s.type_names.append(ty)
        return s.types[ty]

    def _set_class(self, r, c):
        s = self.s
        if s.row_class[r] != c:
            s.row_class[r] = c
            if r < s.cls_uploaded:
                s.cls_dirty.append(r)

    def _sync_classes(self):
        """A range for the rows handed out since the last upload, a scatter for the rows that changed hands."""
        s = self.s
        n = len(s.row_key)
        if n > s.cls_uploaded:
            first = s.cls_uploaded + (1 if s.fault == "class_range_starts_late" else 0)
            if n > first:
                s.g.set_classes(first, np.array(s.row_class[first:n], np.uint8))
            s.cls_uploaded = n
        if s.cls_dirty:
            s.g.set_class_batch(s.cls_dirty, [s.row_class[r] for r in s.cls_dirty])
            s.cls_dirty = []

    # ---- immovable types
    def set_type_movable(self, ty, movable):
        s = self.s
        if s.fault == "movable_unseen_type_not_numbered" and ty not in s.types:
            return OK
        c = self._type(ty)
        if c == 255 and s.fault != "movable_other_class_accepted":
            return ERANGE
        flags = self.own_imm if s.fault == "movable_flag_per_clone" else s.type_imm
        imm = not movable
        if bool(flags.get(c, False)) != imm:
            flags[c] = imm
            s.mv_dirty = True
        return OK

    def _sync_movable(self, ordered):
        """Ahead of a dense rebalance: with an immovable type the classes that changed and, if it changed, the table; without
        one nothing, except the one reset after the last immovable type became movable again."""
        s = self.s
        flags = self.own_imm if s.fault == "movable_flag_per_clone" else s.type_imm
        imm = sorted(c for c, on in flags.items() if on)
        if s.fault == "movable_flag_per_clone":
            s.mv_dirty = True          # (each clone sends its own table)
        if ordered and s.fault == "movable_ordered_call_ignores":
            imm, s.mv_dirty = [], True
        if imm:
            before = s.g.get_classes() if s.fault == "movable_upload_clears_sweep_state" else None
            if s.fault != "movable_classes_not_uploaded":
                self._sync_classes()
            if before is not None and not np.array_equal(before, s.g.get_classes()[:len(before)]):
                s.stale_cls = before
            if s.mv_dirty and not (s.fault == "movable_table_uploaded_once" and s.mv_sent):
                table = np.ones(256, np.uint8)
                table[imm] = 0
                s.g.set_class_movable(table)
                s.mv_dirty, s.mv_on_device, s.mv_sent = False, True, True
        elif s.mv_on_device:
            if s.fault != "movable_never_reset":
                s.g.set_class_movable(None)
            s.mv_on_device = False
            s.mv_dirty = s.mv_dirty and s.fault == "movable_ordered_call_ignores"

    def set_type_idle_limit(self, ty, max_idle):
        s = self.s
        c = self._type(ty)
        if c == 255 and s.fault != "type_256_gets_a_limit":
            return ERANGE
        s.type_limit[c] = int(max_idle)
        return OK

    def expire_by_type(self, now, default_max_idle, max_objects=None, mid=None):
        """-> (rc, [(struct_name, object_id, address or None)], n_idle)"""
        s = self.s
        cut = []
        for c in range(256):
            L = s.type_limit.get(c, int(default_max_idle))
            if L == U32 and s.fault == "idle_never_is_zero":
                L = 0
            cut.append((now - L) & U32 if s.fault == "type_cutoff_wraps" else now - L if now > L else 0)
        return self._sweep(lambda cap: s.g.expire_classes(cut, cap, count_only=cap == 0)[:3], max_objects, mid, True)

    def census(self, by_server=False, mid=None):
        """-> (rc, [(struct_name or None, address or None, rows, load)])"""
        s = self.s
        self._sync()
        self._sync_classes()
        rows, load, _ = s.g.census(256, by_node=bool(by_server))
        rows, load = rows.reshape(-1, 256), load.reshape(-1, 256)
        out = []
        for j in range(min(len(s.addr), len(rows)) if by_server else 1):
            held = rows[j].any()
            for c in range(256):
                empty = s.fault == "census_lists_empty_cells" and by_server and held and c < len(s.type_names)
                if rows[j][c] or empty:
                    name = s.type_names[c] if c < len(s.type_names) else "other" if s.fault == "census_names_shared_class" else None
                    out.append((name, s.addr[j] if by_server else None, int(rows[j][c]), int(load[j][c])))
        if mid:
            mid()
        return OK, out

    def _reclaim(self):
        s = self.s
        self._sync()
        col, (load, aff) = s.g.get_assign(), s.g.get_objects()
        gone = []
        for r in range(len(s.row_key)):
            keep = s.row_keep[r] and s.fault != "kept_row_recycled"
            if s.row_live[r] and not keep and col[r] == NONE and aff[r] == AFF_INACTIVE:
                if s.feed_on and s.fault != "feed_forgets_retired":
                    s.retired.setdefault(r, s.row_key[r])
                del s.rows[self._key(*s.row_key[r])]
                s.row_key[r], s.row_live[r], s.row_keep[r] = None, 0, 0
                s.shadow.pop(r, None)
                if s.fault == "reclaim_resets_stamp":
                    s.stamps[r] = 0
                if s.fault != "reclaim_keeps_counter":
                    s.hits[r] = 0
                s.free.append(r)
                gone.append(r)
        if gone:
            s.g.set_object_attrs(gone, load=np.ones(len(gone), np.uint32))
        return bool(gone)

    def _with_reclaim(self, body):
        rc = body()
        if rc == "full":
            if not self._reclaim():
                return EINVAL
            rc = body()
        return EINVAL if rc == "full" else rc

    # ---- last-seen stamps
    def set_clock(self, now):
        self.own_now = int(now)
        if self.s.fault != "clone_has_its_own_clock":
            self.s.now = int(now)
        return OK

    def _stamp(self, row, by_shadow=False):
        s = self.s
        self._count(row, by_shadow)
        t = self.own_now if s.fault == "clone_has_its_own_clock" else s.now
        if t and not (by_shadow and s.fault == "shadow_hit_does_not_stamp"):
            s.stamps[row] = max(int(s.stamps[row]), t)

    # ---- request counters (measured load)
    def _count(self, row, by_shadow=False):
        """One request for the row's key, at every site that stamps: whether or not the clock is set."""
        s = self.s
        on = self.own_track if s.fault == "tracking_per_clone" else s.track
        if on and not (by_shadow and s.fault == "shadow_hit_not_counted"):
            s.hits[row] = min(int(s.hits[row]) + 1, U32)

    def set_load_tracking(self, on):
        self.own_track = bool(on)
        if self.s.fault != "tracking_per_clone":
            self.s.track = bool(on)
        return OK

    def fold_loads(self, keep, gain, min_load=0, max_load=U32):
        """-> (rc, rows_changed, hits_folded)"""
        s = self.s
        if keep > 65536 or min_load > max_load:
            if s.fault == "refused_fold_drops_counters":
                s.hits[:] = 0
            return EINVAL, 0, 0
        self._sync()
        n = len(s.row_key)
        if s.hits[:n].any():
            s.g.hits_merge(s.hits[:n].astype(np.uint32))
        s.hits[:] = 0
        before, hits = s.g.get_objects()[0], s.g.get_hits()
        st = s.g.load_fold(keep, gain, min_load, max_load)
        changed, folded = st["rows_changed"], st["hits_folded"]
        if s.fault == "hits_folded_after_clamp":
            after = s.g.get_objects()[0]
            folded = sum((int(a) - (int(b) * keep >> 16)) // gain for a, b, h in zip(after, before, hits)
                         if h and gain and int(a) >= int(b) * keep >> 16)
        # rows on the free list belong to no key: they leave the count and go back to load 1
        free_load = max(min_load, min(max_load, 1 if keep == 65536 else 0))
        if s.free and free_load != 1:
            if s.fault != "rows_changed_counts_free_rows":
                changed -= len(s.free)
            if s.fault != "fold_leaves_free_rows":
                s.g.set_object_attrs(s.free, load=np.ones(len(s.free), np.uint32))
        return OK, changed, folded

    def get_object_load(self, ty, oid):
        """-> (rc, load or None)"""
        s = self.s
        r = s.rows.get(self._key(ty, oid))
        if r is None:
            return OK, None
        self._sync()
        if s.fault == "get_object_load_stamps":
            self._stamp(r)
        return OK, int(s.g.get_objects()[0][r])

    def hottest_objects(self, address=None, min_load=0, max_objects=TOP_MAX, mid=None):
        """-> (rc, [(struct_name, object_id, address or None, load)], n_candidates)"""
        s = self.s
        cap = int(max_objects)
        if cap > TOP_MAX:
            return EINVAL, [], 0
        self._sync()
        node = None
        if address is not None:
            if address not in s.nodes:
                return OK, [], 0
            node = s.nodes[address]
        mk = 0 if s.fault == "hottest_ignores_min_load_per_server" and node is not None else int(min_load)
        placed = s.fault != "hottest_lists_unplaced"
        rows, keys, nodes, nc, _ = s.g.top_rows(cap, placed=placed, node=node, min_key=mk)
        if s.fault == "hottest_ties_by_key":
            rows, keys, nodes, _, _ = s.g.top_rows(TOP_MAX, placed=placed, node=node, min_key=mk)
            order = sorted(range(len(rows)), key=lambda i: (-int(keys[i]), s.row_key[rows[i]] or ("", "")))[:cap]
            rows, keys, nodes = rows[order], keys[order], nodes[order]
        out = [s.row_key[r] + (s.addr[nd] if nd < len(s.addr) else None, int(k)) for r, k, nd in zip(rows, keys, nodes) if s.row_live[r]]
        if mid:
            mid()
        return OK, out, nc

    def expire(self, cutoff, max_objects=None, mid=None):
        """-> (rc, [(struct_name, object_id, address or None)], n_idle)"""
        s = self.s
        if s.fault == "expire_cutoff_inclusive":
            cutoff = min(int(cutoff) + 1, 0xFFFFFFFF)
        return self._sweep(lambda cap: s.g.expire(cutoff, cap, count_only=cap == 0)[:3], max_objects, mid, False)

    def _sweep(self, dense, max_objects, mid, by_type):
        """rio_op_expire and rio_op_expire_by_type: dense(cap) -> (rows, nodes, n_idle) is the dense call."""
        s = self.s
        self._sync()
        if by_type:
            self._sync_classes()
            if s.stale_cls is not None:      # (fault movable_upload_clears_sweep_state)
                s.g.set_classes(0, s.stale_cls)
                s.stale_cls = None
        n = len(s.row_key)
        cap = n if max_objects is None else min(int(max_objects), n)
        if s.stamps.any() and not (cap == 0 and s.fault == "stamps_not_uploaded_on_count_only"):
            s.g.touch_merge(s.stamps[:n])
        rows, nodes, n_idle = dense(cap)
        out = []
        for r, nd in zip(rows, nodes):
            if s.fault != ("expire_by_type_keeps_shadow_entry" if by_type else "expire_keeps_shadow_entry"):
                self._put(r, NONE)
            if s.row_live[r]:
                out.append(s.row_key[r] + (s.addr[nd] if nd < len(s.addr) else None,))
        if len(rows) and s.fault == "expire_drops_whole_shadow":
            self._invalidate()
        if s.fault == "expire_listing_not_in_row_order":
            out.reverse()
        if mid:
            mid()
        return OK, out, n_idle

    # ---- shadow
    def _put(self, row, node):
        if self.s.shadow_on:
            self.s.shadow[int(row)] = (self.s.clock, int(node))

    def _get(self, row):
        s = self.s
        e = s.shadow.get(int(row)) if s.shadow_on else None
        if e is None or e[0] < s.base or (e[1] != NONE and e[0] < s.clean_stamp.get(e[1], 0)):
            return None
        return e[1]

    def _invalidate(self):
        self.s.clock += 1
        self.s.base = self.s.clock

    def invalidate_cache(self):
        self._invalidate()
        return OK

    def device_round_trips(self):
        return tuple(self.s.trips)

    def _trip(self):
        self.s.trips[0] += 1
        self.s.trips[1] += 1

    def _out(self, addr, cap):
        self.s.last_len = len(addr.encode())
        return (ERANGE, "") if cap < self.s.last_len + 1 else (OK, addr)

    def last_address_len(self):
        return self.s.last_len

    # ---- the trait
    def update(self, ty, oid, addr):
        s = self.s
        res = {}

        def body():
            if addr is None:
                r = self._row(ty, oid, False, True)
                res["v"] = None if r == NONE else (r, NONE)
                return OK
            r = self._row(ty, oid, True, True)
            if r == "full":
                return r
            nd = self._node(addr, True)
            if nd < 0:
                return EINVAL
            res["v"] = (r, nd)
            return OK
        rc = self._with_reclaim(body)
        if rc or res.get("v") is None:
            return rc
        self._sync()
        self._trip()
        r, nd = res["v"]
        s.g.update_batch([r], [nd])
        self._put(r, nd)
        if nd != NONE:
            self._stamp(r)
        return OK

    def update_batch(self, keys, addrs):
        s = self.s
        out = {}

        def body():
            rows, nodes = [], []
            for (ty, oid), a in zip(keys, addrs):
                if a is None:
                    r = self._row(ty, oid, False, True)
                    if r == NONE:
                        continue
                    nd = NONE
                else:
                    r = self._row(ty, oid, True, True)
                    if r == "full":
                        return r
                    nd = self._node(a, True)
                    if nd < 0:
                        return EINVAL
                rows.append(r)
                nodes.append(nd)
            out["v"] = (rows, nodes)
            return OK
        rc = self._with_reclaim(body)
        if rc:
            return rc
        self._sync()
        rows, nodes = out["v"]
        if rows:
            if s.fault == "update_batch_first_wins":
                rows, nodes = rows[::-1], nodes[::-1]
            s.g.update_batch(rows, nodes)
            for r, nd in zip(rows, nodes):
                self._put(r, nd)
                if nd != NONE:         # per entry, whatever a later entry does to the key
                    self._stamp(r)
        return OK

    def remove(self, ty, oid):
        r = self._row(ty, oid, False, True)
        if r == NONE:
            return OK
        self._sync()
        self._trip()
        self.s.g.remove_batch([r])
        self._put(r, NONE)
        if self.s.fault == "remove_stamps":
            self._stamp(r)
        if self.s.fault == "remove_counts_request":
            self._count(r)
        return OK

    def clean_server(self, addr):
        s = self.s
        nd = s.nodes.get(addr)
        if nd is None:
            return OK
        self._sync()
        s.g.clean_server(nd)
        s.clock += 1
        s.clean_stamp[nd] = s.clock
        return OK

    def lookup(self, ty, oid, cap=512):
        """-> (rc, found, address)"""
        s = self.s
        s.last_len = 0
        r = self._row(ty, oid, False)
        if r == NONE:
            return OK, 0, ""
        nd = self._get(r)
        hit = nd is not None
        if nd is None:
            self._sync()
            self._trip()
            nd = int(s.g.lookup_batch([r])[0])
            self._put(r, nd)
        if nd == NONE:
            return OK, 0, ""
        rc, a = self._out(s.addr[nd], cap)
        if rc == OK:                   # (an ERANGE answer is a call that failed: no stamp)
            self._stamp(r, hit)
        return rc, 1, a

    def try_lookup(self, ty, oid, cap=512):
        s = self.s
        s.last_len = 0
        r = s.rows.get(self._key(ty, oid))
        if r is None:
            return OK, 0, ""
        nd = self._get(r)
        if nd is None:
            return EAGAIN, 0, ""
        if nd == NONE:
            return OK, 0, ""
        rc, a = self._out(s.addr[nd], cap)
        if rc == OK:
            self._stamp(r, True)
        return rc, 1, a

    def _sticky(self, r, me):
        s = self.s
        nd = self._get(r)
        if nd is None or nd == NONE or not s.alive[nd] or s.bad[nd]:
            return None
        return nd, (0 if nd == me else 1)

    def try_get_or_create_placement(self, ty, oid, me, cap=512):
        """-> (rc, address, flag)"""
        s = self.s
        s.last_len = 0
        r = s.rows.get(self._key(ty, oid))
        if r is None or s.row_keep[r] or me not in s.nodes:
            return EAGAIN, "", 0
        hit = self._sticky(r, s.nodes[me])
        if hit is None:
            return EAGAIN, "", 0
        rc, a = self._out(s.addr[hit[0]], cap)
        if rc == OK:
            self._stamp(r, True)
        return rc, a, hit[1]

    def _policy(self, rows, reqs):
        s = self.s
        if any(s.bad):
            cur = s.g.lookup_batch(rows)
            bad = [r for r, c in zip(rows, cur) if c != NONE and s.bad[c]]
            if bad:
                s.g.remove_batch(bad)
        node, flag = s.g.place_pending(rows, reqs)
        cleaned = any(int(f) & FLAG_REPLACED for f in flag)
        if cleaned:
            self._invalidate()
        for r, nd in zip(rows, node):
            if not cleaned or nd == NONE or s.alive[nd]:
                self._put(r, nd)
        return node, flag

    def get_or_create_placement(self, ty, oid, me, cap=512):
        """-> (rc, address, flag)"""
        s = self.s
        s.last_len = 0
        res = {}

        def body():
            r = self._row(ty, oid, True, True)
            if r == "full":
                return r
            nd = self._node(me, True, up=True)
            if nd < 0:
                return EINVAL
            res["v"] = (r, nd)
            return OK
        rc = self._with_reclaim(body)
        if rc:
            return rc, "", 0
        r, q = res["v"]
        hit = self._sticky(r, q)
        if hit is not None:
            rc, a = self._out(s.addr[hit[0]], cap)
            if rc == OK:
                self._stamp(r, True)
            return rc, a, hit[1]
        self._sync()
        self._trip()
        node, flag = self._policy([r], [q])
        rc, a = self._out("" if node[0] == NONE else s.addr[node[0]], cap)
        if rc == OK and node[0] != NONE:
            self._stamp(r)
        return rc, a, int(flag[0])

    def get_or_create_placement_batch(self, keys, mes):
        """-> (rc, node ids, flags)"""
        out = {}

        def body():
            rows, reqs = [], []
            for (ty, oid), me in zip(keys, mes):
                r = self._row(ty, oid, True, True)
                if r == "full":
                    return r
                nd = self._node(me, True, up=True)
                if nd < 0:
                    return EINVAL
                rows.append(r)
                reqs.append(nd)
            out["v"] = (rows, reqs)
            return OK
        rc = self._with_reclaim(body)
        if rc:
            return rc, [], []
        self._sync()
        rows, reqs = out["v"]
        if not rows:
            return OK, [], []
        node, flag = self._policy(rows, reqs)
        for r, nd in zip(rows, node):
            if nd != NONE:
                self._stamp(r)
        return OK, [int(x) for x in node], [int(x) for x in flag]

    def lookup_batch(self, keys):
        s = self.s
        rows = [self._row(ty, oid, False) for ty, oid in keys]
        self._sync()
        out = []
        for r in rows:
            if r == NONE:
                out.append(NONE)
            else:
                nd = int(s.g.lookup_batch([r])[0])
                self._put(r, nd)
                if nd != NONE:
                    self._stamp(r)
                out.append(nd)
        return OK, out

    def node_address(self, nid):
        return self.s.addr[nid] if nid < len(self.s.addr) else None

    def set_member(self, addr, active, capacity):
        s = self.s
        nd = self._node(addr, True)
        if nd < 0:
            return EINVAL
        s.alive[nd] = 1 if active else 0
        s.cap[nd] = int(capacity)
        self._sync()
        return OK

    def set_object_load(self, ty, oid, load):
        res = {}

        def body():
            r = self._row(ty, oid, True, False)
            res["r"] = r
            return r if r == "full" else OK
        rc = self._with_reclaim(body)
        if rc:
            return rc
        self._sync()
        self.s.g.set_object_attrs([res["r"]], load=[load])
        return OK

    def len(self):
        self._sync()
        return OK, self.s.g.count_placed()

    def tick(self):
        s = self.s
        self._sync()
        s.g.set_self_assign(False)
        st = s.g.tick()
        s.g.set_self_assign(s.self_assign)
        self._invalidate()
        return OK, st

    # ---- listings (mid: called between the call and the reading of its arrays)
    def snapshot(self, mid=None):
        s = self.s
        self._sync()
        col = s.g.get_assign()
        out = [(s.row_key[r][0], s.row_key[r][1], s.addr[col[r]]) for r in range(len(col))
               if s.row_live[r] and col[r] != NONE and col[r] < len(s.addr)]
        if mid:
            mid()
        return OK, out

    def objects_on_server(self, addr, mid=None):
        s = self.s
        self._sync()
        out = []
        if addr in s.nodes:
            _, rows = s.g.rows_on_nodes([s.nodes[addr]])
            names = s.stale_key if s.fault == "index_lists_reclaimed" else s.row_key
            out = [names[r] for r in rows if s.row_live[r]]
        if mid:
            mid()
        return OK, out

    def rebalance(self, max_moves=None, mid=None, order=None):
        """order None: rio_op_rebalance; else rio_op_rebalance_ordered with that order."""
        s = self.s
        ordered = order is not None
        order = 0 if order is None else int(order)
        if order not in (0, 1):
            if s.fault != "invalid_order_runs_row_order":
                return EINVAL, []
            order = 0
        if s.fault == "by_load_runs_row_order":
            order = 0
        self._sync()
        self._sync_movable(ordered)
        cap = min(CAP_INF if max_moves is None else int(max_moves), len(s.row_key))
        _, rows, frm, to = s.g.rebalance(None, cap, 0, moves_cap=cap, order=order)
        if s.fault != "rebalance_keeps_shadow":
            self._invalidate()
        out = [(s.row_key[r][0], s.row_key[r][1], s.addr[f], s.addr[t]) for r, f, t in zip(rows, frm, to) if s.row_live[r]]
        if s.fault == "rebalance_key_order":
            out.sort()
        if mid:
            mid()
        return OK, out

    def changes(self, mid=None):
        s = self.s
        self._sync()
        s.feed_on = True
        rows, old, new, _ = s.g.changes(cap=None)
        listed = {int(r): (int(o), int(n)) for r, o, n in zip(rows, old, new)}
        for r in s.retired:
            if r not in listed:
                c = int(s.g.lookup_batch([r])[0])
                listed[r] = (c, c)
        dels, ups = [], []
        A = lambda nd: s.addr[nd] if nd < len(s.addr) else None
        for r in sorted(listed):
            a0, a1 = A(listed[r][0]), A(listed[r][1])
            if r in s.retired:
                if a0:
                    dels.append(s.retired[r] + (a0, None))
                if a1 and s.row_live[r]:
                    ups.append(s.row_key[r] + (None, a1))
                continue
            if not s.row_live[r]:
                continue
            if a1:
                ups.append(s.row_key[r] + (a0, a1))
            elif a0:
                dels.append(s.row_key[r] + (a0, None))
        s.retired = {}
        full, s.feed_full = s.feed_full, False
        if mid:
            mid()
        return OK, bool(full), dels + ups

    def changes_reset(self):
        s = self.s
        s.g.changes_reset()
        s.retired = {}
        s.feed_full = s.fault != "reset_not_full"
        return OK


def module(fault=None):
    """What the driver is given: make(max_objects, max_nodes, spill_rounds, flags) -> a provider."""
    def make(max_objects, max_nodes=32, spill_rounds=2, flags=0):
        return FakeObjectPlacement(max_objects, max_nodes, spill_rounds, flags, fault)
    return make
