"""A CPU stand-in for the rio_gp binding, FOR TESTS ONLY: the surface tests/test_gpu_fuzz.py's scenarios use, implemented over
the CPU oracle (oracle/pyoracle.py), tests/rebalance_ref.py, tests/rebalance_order_ref.py, tests/spec_changes.py, tests/spec_remap.py
and tests/spec_top.py; idle expiry and measured load (the hit column and the fold, in uint64: the scenarios hold them against
tests/spec_loads.py's Python integers) and object classes (the class column, the per-class sweep and the census, which the scenarios
hold against tests/spec_classes.py) are restated here in plain numpy; the table of immovable classes goes into the rebalance through
the equivalence rule 13 states (the affinity of the immovable rows read as RIO_GP_AFF_INACTIVE).  It lets the fuzz driver itself be tested
without a GPU (tests/test_fuzz_driver.py): its bookkeeping (n, the feed's checkpoint, the mirror, the uncommitted solve) and its
sensitivity — `fault=` makes exactly one behaviour of the handle wrong, and the scenarios must notice.

It is not a CPU backend: nothing under rio-rs_amd/ imports it, and the product has no fallback.

"Device" buffers are host arrays whose address stands for the device pointer, so pointer arithmetic on `.ptr` works as it does
with tools/hipbuf.DevBuf.
"""
import ctypes as C
import types

import numpy as np

import rebalance_order_ref
import rebalance_ref
import spec_changes
import spec_remap
import spec_top

NONE = 0xFFFFFFFF
CAP_INF = 0xFFFFFFFFFFFFFFFF
AFF_INACTIVE = 0xFFFFFFFE
CFG_REF_SELF_ASSIGN = 2
CHANGES_PEEK = 1
TOP_BY_HITS, TOP_PLACED, TOP_ON_NODE, TOP_MAX = 1, 2, 4, 4096
REBALANCE_ROW_ORDER, REBALANCE_BY_LOAD = 0, 1
CENSUS_BY_NODE, MAX_CLASSES = 1, 256
U32 = 0xFFFFFFFF
OK, EINVAL, EUPSTREAM, ENODEV, ENOMEM, ERANGE, EAGAIN = range(7)

FAULTS = (
    "feed_keeps_last_row",         # a consuming listing does not advance the checkpoint for its last listed row
    "feed_lists_hidden_rows",      # the feed lists rows >= n
    "rebalance_stale_alive",       # the rebalance uses the liveness of before the last set_alive*
    "rebalance_stale_used",        # the rebalance leaves `used` of the old column
    "rebalance_keeps_solve",       # the rebalance keeps an uncommitted solve committable
    "index_drops_last_row",        # the index drops the last row of a node's range
    "index_reads_solved",          # the index reads the uncommitted column
    "num_objects_stale_used",      # set_num_objects leaves `used` as it was
    "remap_keeps_solve",           # a node removal keeps an uncommitted solve committable
    "remap_skips_hidden_rows",     # a node removal leaves the rows >= n as they were
    "remap_counts_hidden_rows",    # a node removal counts the rows >= n it un-places as evicted
    "remap_checkpoint_none_not_gone",   # a checkpoint naming a removed node becomes NONE, not RIO_GP_NODE_GONE
    "remap_stale_node_table",      # a node removal leaves cap and alive at their old ids
    "remap_affinity_not_renumbered",    # the synchronous committed ticks read the affinity of before the removal (the getter does not)
    "expire_cutoff_inclusive",     # a row stamped exactly at the cutoff is idle
    "expire_unplaces_past_cap",    # a sweep un-places every idle row, not only the listed ones
    "expire_lists_hidden_rows",    # a sweep finds rows >= n idle
    "expire_freed_counts_unlisted",     # load_freed sums every idle row's load
    "expire_stale_used",           # a sweep leaves `used` of the old column
    "expire_keeps_solve",          # a sweep that un-placed rows keeps an uncommitted solve committable
    "expire_zero_hit_drops_solve",      # a sweep that un-placed nothing drops an uncommitted solve
    "expire_count_only_writes",    # a count-only sweep un-places the idle rows
    "touch_overwrites",            # a touch stores the epoch instead of the maximum
    "touch_all_past_n",            # touch_all stamps the rows >= n too
    "touch_dev_stops_at_invalid",  # the _dev batch stops at its first invalid entry instead of skipping it
    "touch_drops_solve",           # a touch drops an uncommitted solve
    "remap_moves_seen",            # a node removal clears the stamps of the rows < n
    "hits_add_wraps",              # the hit counters wrap at 2^32 instead of saturating
    "hits_dev_stops_at_invalid",   # the _dev hits batch stops at its first invalid entry instead of skipping it
    "hits_merge_past_rows",        # a merge of `rows` counters also counts for the rest of the quad behind `rows`
    "hits_drop_solve",             # a hits call drops an uncommitted solve
    "fold_past_n",                 # the fold rewrites the loads and zeroes the hits of the rows >= n too
    "fold_keeps_hits",             # the fold leaves H as it was
    "fold_clamps_before_gain",     # the fold clamps the decayed load and adds H * gain afterwards
    "fold_stale_used",             # the fold leaves `used` of the old loads
    "fold_keeps_solve",            # the fold keeps an uncommitted solve committable
    "fold_refused_still_zeroes_hits",   # a refused fold zeroes H[:n]
    "top_ties_to_highest_rows",    # the report orders equal keys by descending row
    "top_lists_hidden_rows",       # rows >= n are candidates of the report
    "top_key_sum_of_listed_only",  # key_sum covers the listed candidates only
    "top_reads_solved",            # the report reads the uncommitted column
    "top_writes_past_listing",     # the report writes one entry behind its listing
    "top_drops_solve",             # the report drops an uncommitted solve
    "top_hits_key_ignores_flag",   # under RIO_GP_TOP_BY_HITS the key is still the load
    "by_load_is_row_order",        # cfg.order is ignored: the cut is R1
    "by_load_ties_shed_first_rows",     # among candidates of equal load the cut sheds the lowest rows, not the highest
    "by_load_sheds_zero_load",     # zero-load candidates are cut behind the loaded ones, so an over node sheds them
    "classes_batch_first_wins",    # of several batch entries for one row the first wins
    "classes_dev_batch_stops_at_invalid",   # the _dev class batch stops at its first invalid entry instead of skipping it
    "classes_range_writes_past_end",    # the range setter writes one byte behind its last row
    "classes_drop_solve",          # a class setter drops an uncommitted solve
    "classes_batch_dirty_pos",     # a class batch leaves its rows marked in the position scratch: the next update batch skips them
    "num_objects_clears_classes",  # set_num_objects zeroes the class column
    "remap_clears_classes",        # a node removal zeroes the classes of the rows < n
    "expc_cutoff_inclusive",       # class sweep: a row stamped exactly at its class's cutoff is idle
    "expc_high_class_is_class_0",  # class sweep: a row of a class >= n_classes is swept under class 0's cutoff
    "expc_by_class_listed_only",   # idle_by_class counts the listed rows only
    "expc_by_class_accumulates",   # idle_by_class adds to what the sweep before left
    "expc_unplaces_past_cap",      # a class sweep un-places every idle row, not only the listed ones
    "expc_lists_hidden_rows",      # a class sweep finds rows >= n idle
    "expc_keeps_solve",            # a class sweep that un-placed rows keeps an uncommitted solve committable
    "expc_count_only_writes",      # a count-only class sweep un-places the idle rows
    "census_counts_hidden_rows",   # the census counts rows >= n
    "census_reads_solved",         # the census reads the uncommitted column
    "census_uses_max_nodes",       # by node the census works on max_nodes nodes, not on m
    "census_other_per_slice",      # between 4 097 and 65 536 cells a row that is counted in n_other is counted once per 4 096 cells
    "census_dev_adds",             # the _dev census adds to what the arrays held
    "census_drops_solve",          # the census drops an uncommitted solve
    "census_skips_zero_load_rows", # a row of load 0 is left out of out_rows
    "movable_ignored",             # the rebalance does not consult the table of immovable classes
    "movable_pinned_load_not_counted",  # immovable rows are no candidates, but their load does not count against the target
    "movable_counts_as_surplus",   # immovable rows are never moved, but surplus_rows / surplus_load count them
    "movable_class_255_always_movable",      # the rebalance treats class 255 as movable whatever the table says
    "movable_stale_classes",       # the rebalance reads the class column as it was at the last rio_gp_set_class_movable
    "movable_writes_affinity",     # the rebalance leaves RIO_GP_AFF_INACTIVE in the affinity column of the immovable rows
    "movable_hidden_quad",         # the immovable rows of the quad behind n count as pinned load of their node
    "rebalance_resets_movable",    # a rebalance under a table resets it
    "movable_short_table_keeps_old_flags",   # a table of n_classes flags leaves the classes >= n_classes as they were
    "movable_refused_still_sets",  # a refused rio_gp_set_class_movable writes the table all the same
    "movable_drops_solve",         # rio_gp_set_class_movable drops an uncommitted solve
    "remap_resets_movable",        # a node removal resets the table of immovable classes
    "num_objects_resets_movable",  # set_num_objects resets the table of immovable classes
)


class ObjectPlacementError(Exception):
    def __init__(self, kind, text, rc):
        super().__init__("%s(%s)" % (kind, text))
        self.kind, self.text, self.rc = kind, text, rc


def _einval(text):
    return ObjectPlacementError("Unknown", text, EINVAL)


def _oracle():
    import pyoracle
    return pyoracle


def build(*a, **k):
    return None


def balanced_targets(cap, used, alive, slack_permille=0):
    """rio_gp.balanced_targets restated (integers throughout)."""
    cap = np.asarray(cap, np.uint64)
    used = np.asarray(used, np.uint64)
    live = np.asarray(alive, np.uint8) != 0
    t = np.full(len(cap), CAP_INF, np.uint64)
    if not live.any():
        return t
    total = sum(int(u) for u in used[live])
    caps = [int(c) for c in cap[live]]
    scale = 1000 + int(slack_permille)
    if any(c == CAP_INF for c in caps):
        per = -(-total * scale // (1000 * len(caps)))
        t[live] = np.uint64(min(per, CAP_INF))
        return t
    sc = sum(caps)
    t[live] = np.array([min(-(-c * total * scale // (sc * 1000)) if sc else 0, c) for c in caps], np.uint64)
    return t


class DevBuf:
    """tools/hipbuf.DevBuf over host memory."""

    def __init__(self, arr=None, nbytes=None):
        self.nbytes = int(arr.nbytes if arr is not None else nbytes)
        self._mem = np.zeros(max(self.nbytes, 16), np.uint8)
        if arr is not None:
            self._mem[:self.nbytes] = np.ascontiguousarray(arr).view(np.uint8).ravel()

    @property
    def ptr(self):
        return self._mem.ctypes.data

    def to_host(self, dtype=np.uint32):
        return self._mem[:self.nbytes - self.nbytes % np.dtype(dtype).itemsize].view(dtype).copy()

    def free(self):
        self._mem = None


def _at(ptr, count, dtype=np.uint32):
    """The `count` entries at "device" address ptr, as a writable array."""
    if not count:
        return np.zeros(0, dtype)
    ct = {np.uint8: C.c_uint8, np.uint32: C.c_uint32, np.uint64: C.c_uint64}[dtype]
    return np.ctypeslib.as_array((ct * int(count)).from_address(int(ptr)))


class GpuPlacement:
    def __init__(self, max_objects, max_nodes, device=0, spill_rounds=2, flags=0, lab=False, fault=None):
        assert fault is None or fault in FAULTS, fault
        self._fault = fault
        self._lab = bool(lab)
        self._cap_rows, self._cap_nodes = int(max_objects), int(max_nodes)
        self._rounds = int(spill_rounds)
        self._oflags = _oracle().REF_SELF_ASSIGN if flags & CFG_REF_SELF_ASSIGN else 0
        self._n, self._m = 0, 0
        self._col = np.full(self._cap_rows, NONE, np.uint32)
        self._load = np.ones(self._cap_rows, np.uint32)
        self._aff = np.full(self._cap_rows, NONE, np.uint32)
        self._cap = np.zeros(0, np.uint64)
        self._alive = np.zeros(0, np.uint8)
        self._alive_seen = self._alive.copy()   # the liveness the "device" has consumed (a set_alive* only pushes)
        self._B = np.full(self._cap_rows, NONE, np.uint32)
        self._S = np.zeros(self._cap_rows, np.uint32)
        self._H = np.zeros(self._cap_rows, np.uint32)
        self._K = np.zeros(self._cap_rows, np.uint8)
        self._I = np.ones(MAX_CLASSES, np.uint8)  # rule 13: 1 = the rebalance may move the class's objects
        self._K_at_I = self._K.copy()             # (fault movable_stale_classes: the column at the last set_class_movable)
        self._by_acc = np.zeros(256, np.uint64)  # (fault expc_by_class_accumulates: what the sweeps so far counted)
        self._pos_dirty = None                    # (fault classes_batch_dirty_pos: the rows the last class batch named)
        self._chain_ok, self._chained = False, 0  # lab: nothing a tick reads has changed since the last tick_async; links so far
        self._solved = None
        self._stale_used = None
        self._stale_aff = None
        self._done = []

    # ---- helpers
    def _view(self):
        n = self._n
        return self._col[:n], self._load[:n], self._aff[:n]

    def _changed(self):
        """Every call that changes an input of the solve: the uncommitted solve is dropped."""
        self._solved = None
        self._stale_used = None
        self._chain_ok = False

    def _sync_alive(self):
        self._alive_seen = self._alive.copy()

    def close(self):
        self._col = None

    @property
    def num_objects(self):
        return self._n

    @property
    def num_nodes(self):
        return self._m

    # ---- tables
    def set_nodes(self, cap=None, alive=None, m=None):
        if m is None:
            m = len(cap) if cap is not None else len(alive)
        if m > self._cap_nodes:
            raise _einval("m exceeds max_nodes")
        self._cap = np.full(m, CAP_INF, np.uint64) if cap is None else np.array(cap, np.uint64)[:m].copy()
        self._alive = np.ones(m, np.uint8) if alive is None else (np.asarray(alive)[:m] != 0).astype(np.uint8)
        self._m = m
        self._sync_alive()
        self._changed()

    def set_alive(self, node, alive):
        if node >= self._m:
            raise _einval("node out of range")
        self._alive[node] = 1 if alive else 0
        self._changed()

    def set_alive_all(self, alive):
        if len(alive) != self._m:
            raise _einval("m differs")
        self._alive = (np.asarray(alive) != 0).astype(np.uint8)
        self._changed()

    def get_nodes(self):
        col, load, _ = self._view()
        used = self._stale_used if self._stale_used is not None else _oracle().recompute_used(col, load, self._m)
        return self._cap.copy(), self._alive.copy(), used.copy()

    def set_objects(self, n, load=None, aff=None):
        if n > self._cap_rows:
            raise _einval("n exceeds max_objects")
        self._load[:n] = 1 if load is None else np.asarray(load, np.uint32)[:n]
        self._aff[:n] = NONE if aff is None else np.asarray(aff, np.uint32)[:n]
        self._col[:] = NONE
        self._n = int(n)
        self._changed()

    def set_object_attrs(self, idx, load=None, aff=None):
        idx = np.asarray(idx, np.uint32)
        if len(idx) and int(idx.max()) >= self._n:
            raise _einval("object index out of range")
        if load is not None:
            self._load[idx] = np.asarray(load, np.uint32)
        if aff is not None:
            self._aff[idx] = np.asarray(aff, np.uint32)
            if self._stale_aff is not None:
                self._stale_aff[idx] = np.asarray(aff, np.uint32)
        self._changed()

    def get_objects(self):
        return self._load[:self._n].copy(), self._aff[:self._n].copy()

    def set_num_objects(self, n):
        if n > self._cap_rows:
            raise _einval("n exceeds max_objects")
        before = self.get_nodes()[2]
        self._n = int(n)
        self._changed()
        if self._fault == "num_objects_clears_classes":
            self._K[:] = 0
        if self._fault == "num_objects_resets_movable":
            self._I[:] = 1
        if self._fault == "num_objects_stale_used":
            self._stale_used = before

    def set_assign(self, assign):
        assign = np.asarray(assign, np.uint32)
        if len(assign) != self._n:
            raise _einval("n differs from the object table")
        self._col[:self._n] = assign
        self._changed()

    def get_assign(self):
        return self._col[:self._n].copy()

    def get_solved(self):
        if self._solved is None or len(self._solved) != self._n:
            raise _einval("no solve / size mismatch")
        return self._solved.copy()

    # ---- CRUD
    def lookup_batch(self, idx):
        return _oracle().lookup_batch(self._view()[0], idx)

    def update_batch(self, idx, node):
        if self._pos_dirty is not None:
            idx, node = np.asarray(idx, np.uint32), np.asarray(node, np.uint32)
            keep = ~np.isin(idx, self._pos_dirty)
            idx, node, self._pos_dirty = idx[keep], node[keep], None
        if _oracle().update_batch(self._view()[0], self._m, idx, node):
            raise _einval("update_batch")
        self._changed()

    def remove_batch(self, idx):
        if _oracle().remove_batch(self._view()[0], idx):
            raise _einval("remove_batch")
        self._changed()

    def clean_server(self, node):
        col = self._view()[0]
        hit = col == np.uint32(node)
        col[hit] = NONE
        self._changed()
        return int(hit.sum())

    def clean_servers(self, dead_nodes):
        ev = _oracle().clean_servers(self._view()[0], self._m, [int(j) for j in dead_nodes])
        self._changed()
        return ev

    # ---- policy
    def place_pending(self, idx, requester):
        col, load, _ = self._view()
        used = _oracle().recompute_used(col, load, self._m)
        out = _oracle().place_pending(col, load, self._cap, self._alive, used, idx, requester, self._rounds, self._oflags)
        self._sync_alive()
        self._changed()
        return out

    def place_pending_dev(self, n, d_idx, d_requester, d_out_node, d_out_flag=None):
        node, flag = self.place_pending(_at(d_idx, n).copy(), _at(d_requester, n).copy())
        _at(d_out_node, n)[:] = node
        if d_out_flag:
            _at(d_out_flag, n)[:] = flag
        return None

    def mixed_batch(self, update=None, remove=None, lookup=None, place=None):
        e = np.empty(0, np.uint32)
        lo, pn, pf = e, e, e
        if update is not None:
            self.update_batch(update[0], update[1])
        if remove is not None:
            self.remove_batch(remove)
        if lookup is not None:
            lo = self.lookup_batch(lookup)
        if place is not None:
            pn, pf = self.place_pending(place[0], place[1])
        return [0, 0, 0, 0], lo, pn, pf

    # ---- solves
    def _tick(self):
        col, load, aff = self._view()
        self._sync_alive()
        return _oracle().tick(col, load, aff, self._cap, self._alive, self._rounds, self._oflags)

    def solve(self):
        nxt, _, st = self._tick()
        self._stale_used = None
        self._solved = nxt
        return st

    def commit(self):
        if self._solved is None or len(self._solved) != self._n:
            raise _einval("rio_gp_commit: no solve to commit")
        self._col[:self._n] = self._solved
        self._solved = None
        self._stale_used = None

    def tick(self):
        aff = self._aff
        if self._stale_aff is not None:
            self._aff = self._stale_aff
        try:
            st = self.solve()
        finally:
            self._aff = aff
        self.commit()
        return st

    def tick_async(self):
        # a quiet tick behind a quiet tick is a link of a chain (the lab build chains whatever the table's size): the stand-in
        # has no verdicts to wait for, so every tick_async behind one with nothing changed in between counts
        self._chained += int(self._lab and self._chain_ok)
        st = self.solve()      # (not tick(): the fault remap_affinity_not_renumbered is one of the synchronous tick alone)
        self.commit()
        self._done.append(st)
        self._chain_ok = True

    def tick_wait(self, cap=4096):
        out, self._done = self._done[-cap:], []
        return out

    # ---- node removal
    def remap_nodes_raw(self, m_new, map):
        m, n, f = self._m, self._n, self._fault
        if not spec_remap.check_map(m, m_new, map):
            return EINVAL, 0
        map = np.asarray(map, np.uint32)
        rows = n if f == "remap_skips_hidden_rows" else self._cap_rows
        solved, old_aff = self._solved, self._aff.copy()
        out = spec_remap.remap(self._col[:rows], self._aff[:rows], self._cap_rows if f == "remap_counts_hidden_rows" else n, m, map,
                               False, B=self._B[:rows], cap=self._cap, alive=self._alive)
        self._col[:rows], self._aff[:rows], self._B[:rows] = out["assign"], out["aff"], out["B"]
        if f == "remap_checkpoint_none_not_gone":
            self._B[self._B == spec_remap.NODE_GONE] = NONE
        if f == "remap_stale_node_table":
            self._cap, self._alive = self._cap[:m_new].copy(), self._alive[:m_new].copy()
        else:
            self._cap, self._alive = out["cap"].copy(), out["alive"].copy()
        self._m = int(m_new)
        self._sync_alive()
        self._changed()
        if f == "remap_keeps_solve":
            self._solved = solved
        if f == "remap_affinity_not_renumbered":
            self._stale_aff = old_aff if self._stale_aff is None else self._stale_aff
        if f == "remap_moves_seen":
            self._S[:n] = 0
        if f == "remap_clears_classes":
            self._K[:n] = 0
        if f == "remap_resets_movable":
            self._I[:] = 1
        return OK, out["evicted"]

    def remap_nodes(self, map):
        map = np.asarray(map, np.uint32)
        rc, ev = self.remap_nodes_raw(int(np.count_nonzero(map != NONE)), map)
        if rc != OK:
            raise _einval("rio_gp_remap_nodes: not a legal map")
        return ev

    # ---- reverse index
    def _index(self, nodes):
        m = self._m
        a = self._col[:self._n]
        if self._fault == "index_reads_solved" and self._solved is not None and len(self._solved) == self._n:
            a = self._solved
        sel = np.ones(m, bool)
        if nodes is not None:
            sel[:] = False
            ids = np.asarray(list(nodes), np.int64)
            sel[ids[ids < m]] = True
        parts, off = [], np.zeros(m + 1, np.uint64)
        on = a < m
        order = np.flatnonzero(on)
        order = order[np.argsort(a[order], kind="stable")]
        cnt = np.bincount(a[on], minlength=m) if m else np.zeros(0, np.int64)
        start = np.concatenate([[0], np.cumsum(cnt)])
        for j in np.flatnonzero(sel & (cnt > 0)) if m else []:
            r = order[start[j]:start[j + 1]]
            if self._fault == "index_drops_last_row":
                r = r[:-1]
            parts.append(r)
            off[j + 1] = len(r)
        off = np.cumsum(off).astype(np.uint64)
        rows = np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)
        return off, rows

    def rows_on_nodes(self, nodes=None, _cap=None):
        return self._index(nodes)

    def rows_on_nodes_try(self, nodes, rows):
        off, r = self._index(nodes)
        if len(r) > len(rows):
            return ERANGE, off, len(r)
        rows[:len(r)] = r
        return OK, off, len(r)

    def count_on_nodes(self, nodes=None):
        return self._index(nodes)[0]

    def rows_on_nodes_dev(self, d_offsets, d_rows, rows_cap, nodes=None):
        off, r = self._index(nodes)
        _at(d_offsets, self._m + 1, np.uint64)[:] = off
        if d_rows and len(r) > rows_cap:
            return ERANGE, len(r)
        if d_rows:
            _at(d_rows, len(r))[:] = r
        return OK, len(r)

    # ---- bounded rebalance
    def _rebalance(self, target, budget, rounds, order=REBALANCE_ROW_ORDER):
        if order not in (REBALANCE_ROW_ORDER, REBALANCE_BY_LOAD):
            raise _einval("rio_gp_rebalance: cfg.order")
        col, load, aff = self._view()
        f = self._fault
        alive = self._alive_seen if f == "rebalance_stale_alive" and len(self._alive_seen) == self._m else self._alive
        before = self.get_nodes()[2]
        solved = self._solved
        n, m = self._n, self._m
        # rule 13 through the equivalence it states: rule 6 with the affinity of every immovable object row read as INACTIVE
        I = self._I.copy()
        if f == "movable_class_255_always_movable":
            I[255] = 1
        K = self._K_at_I if f == "movable_stale_classes" else self._K
        imm = (I[K[:n]] == 0) & (f != "movable_ignored")
        tabled = bool(imm.any())
        if tabled:
            aff = np.where(imm, np.uint32(AFF_INACTIVE), aff)
        if f == "movable_pinned_load_not_counted" and tabled:
            on = imm & (col < m)
            extra = np.zeros(m, np.uint64)
            np.add.at(extra, col[on].astype(np.int64), load[on].astype(np.uint64))
            T = np.array(self._cap if target is None else target, np.uint64)
            target = np.where(T > np.uint64(CAP_INF) - extra, np.uint64(CAP_INF), T + extra)
        n4 = min(-(-n // 4) * 4, self._cap_rows)
        if f == "movable_hidden_quad" and n4 > n and (I[self._K[n:n4]] == 0).any():
            # the rows of the quad behind n: the immovable ones are pinned load, the others take no part
            hid = I[self._K[n:n4]] == 0
            col = np.concatenate([col, np.where(hid, self._col[n:n4], np.uint32(NONE))])
            load = np.concatenate([load, self._load[n:n4]])
            aff = np.concatenate([aff, np.full(n4 - n, AFF_INACTIVE, np.uint32)])

        def run(col, aff, budget):
            if order == REBALANCE_BY_LOAD and f != "by_load_is_row_order":
                r, perm = np.arange(len(col)), None
                if f == "by_load_ties_shed_first_rows":
                    perm = np.lexsort((-r, load))
                elif f == "by_load_sheds_zero_load":
                    perm = np.lexsort((r, load, load == 0))
                return rebalance_order_ref.rebalance(col, load, aff, self._cap, alive, target, budget, rounds or self._rounds,
                                                     order=order, perm=perm)
            return rebalance_ref.rebalance(col, load, aff, self._cap, alive, target, budget, rounds or self._rounds)

        nxt, used, st, rows, frm, to = run(col, aff, budget)
        if f == "movable_counts_as_surplus" and tabled:
            st0 = run(col, self._aff[:n], 0)[2]
            st = dict(st, surplus_rows=st0["surplus_rows"], surplus_load=st0["surplus_load"])
        if f == "movable_writes_affinity" and tabled:
            self._aff[:n] = aff[:n]
        if f == "rebalance_resets_movable":
            self._I[:] = 1
        nxt, col = nxt[:n], self._col[:n]
        col[:] = nxt
        self._changed()
        if self._fault == "rebalance_keeps_solve":
            self._solved = solved
        if self._fault == "rebalance_stale_used":
            self._stale_used = before
        return st, rows, frm, to

    def rebalance(self, target=None, max_moves=None, rounds=0, list_moves=True, moves_cap=None, order=REBALANCE_ROW_ORDER):
        if list_moves:
            mm = CAP_INF if max_moves is None else int(max_moves)
            cap = int(moves_cap if moves_cap is not None else min(mm, self._n))
            return self._rebalance(target, min(mm, cap), rounds, order)
        st, _, _, _ = self._rebalance(target, max_moves, rounds, order)
        e = np.empty(0, np.uint32)
        return st, e, e, e

    def rebalance_dev(self, d_rows=None, d_from=None, d_to=None, moves_cap=0, target=None, max_moves=None, rounds=0,
                      order=REBALANCE_ROW_ORDER):
        if bool(d_rows) != bool(d_from) or bool(d_rows) != bool(d_to) or (not d_rows and moves_cap):
            raise _einval("rio_gp_rebalance: the output rule")
        mm = CAP_INF if max_moves is None else int(max_moves)
        budget = min(mm, int(moves_cap)) if d_rows else (None if max_moves is None else mm)
        st, rows, frm, to = self._rebalance(target, budget, rounds, order)
        if d_rows:
            _at(d_rows, len(rows))[:] = rows
            _at(d_from, len(rows))[:] = frm
            _at(d_to, len(rows))[:] = to
        return st, len(rows)

    # ---- change feed
    def _changes(self, cap, peek):
        n = self._cap_rows if self._fault == "feed_lists_hidden_rows" else self._n
        rows, old, new, total, B = spec_changes.dense(self._B, self._col, n, cap, peek)
        if self._fault == "feed_keeps_last_row" and not peek and len(rows):
            B[rows[-1]] = self._B[rows[-1]]
        self._B = B
        return rows, old, new, total

    def changes(self, cap=None, peek=False):
        if cap is not None:
            cap = min(int(cap), self._n)
        return self._changes(cap, peek)

    def changes_dev(self, d_rows=None, d_old=None, d_new=None, cap=0, peek=False):
        if bool(d_rows) != bool(d_old) or bool(d_rows) != bool(d_new) or (not d_rows and cap):
            raise _einval("rio_gp_changes: the output rule")
        rows, old, new, total = self._changes(int(cap), peek)
        if d_rows:
            _at(d_rows, len(rows))[:] = rows
            _at(d_old, len(rows))[:] = old
            _at(d_new, len(rows))[:] = new
        return total

    def changes_reset(self):
        self._B[:] = NONE

    # ---- idle expiry
    def _touch(self, idx, epoch):
        if self._fault == "touch_overwrites":
            self._S[idx] = np.uint32(epoch)
        else:
            np.maximum.at(self._S, np.asarray(idx, np.int64), np.uint32(epoch))
        if self._fault == "touch_drops_solve":
            self._changed()

    def touch_raw(self, idx, epoch):
        idx = np.asarray(idx, np.uint32)
        if len(idx) and int(idx.max()) >= self._n:
            return EINVAL
        self._touch(idx, epoch)
        return OK

    def touch(self, idx, epoch):
        if self.touch_raw(idx, epoch) != OK:
            raise _einval("rio_gp_touch_batch: object index out of range")

    def touch_dev(self, d_idx, n, epoch):
        idx = _at(d_idx, n).copy()
        bad = idx >= self._n
        if self._fault == "touch_dev_stops_at_invalid" and bad.any():
            self._touch(idx[:int(np.argmax(bad))], epoch)
        else:
            self._touch(idx[~bad], epoch)
        if bad.any():
            raise _einval("rio_gp_touch_batch: invalid entries were skipped")

    def touch_all(self, epoch):
        rows = self._cap_rows if self._fault == "touch_all_past_n" else self._n
        self._touch(np.arange(rows), epoch)

    def touch_merge(self, stamps):
        stamps = np.asarray(stamps, np.uint32)
        rows = len(stamps)
        if rows > self._n:
            raise _einval("rio_gp_touch_merge: rows exceeds the object table")
        self._S[:rows] = np.maximum(self._S[:rows], stamps)
        if self._fault == "touch_drops_solve":
            self._changed()

    def touch_merge_dev(self, d_stamps, rows):
        if rows > self._n:
            raise _einval("rio_gp_touch_merge: rows exceeds the object table")
        self.touch_merge(_at(d_stamps, rows).copy())

    def get_seen(self):
        return self._S[:self._n].copy()

    def _expire(self, cutoff, cap):
        """cap None: count only.  -> rows, nodes, n_idle, load_freed"""
        f = self._fault
        n = self._cap_rows if f == "expire_lists_hidden_rows" else self._n
        col = self._col
        lim = int(cutoff) + (1 if f == "expire_cutoff_inclusive" else 0)
        idle = np.flatnonzero((col[:n] != NONE) & (self._S[:n].astype(np.int64) < lim)).astype(np.uint32)
        before, solved = self.get_nodes()[2], self._solved
        e = np.empty(0, np.uint32)
        if cap is None:
            listed, gone = e, (idle if f == "expire_count_only_writes" else e)
        else:
            listed = idle[:int(cap)]
            gone = idle if f == "expire_unplaces_past_cap" else listed
        nodes = col[listed].copy()
        freed = int(self._load[idle if f == "expire_freed_counts_unlisted" and cap is not None else listed].astype(np.uint64).sum())
        col[gone] = NONE
        if len(listed):        # as rio_gp_remove_batch of the listed rows
            self._changed()
            if f == "expire_keeps_solve":
                self._solved = solved
            if f == "expire_stale_used":
                self._stale_used = before
        elif f == "expire_zero_hit_drops_solve":
            self._changed()
        return listed, nodes, len(idle), freed

    def expire(self, cutoff, cap=None, count_only=False):
        cap = self._n if cap is None else min(int(cap), self._n)
        if count_only or cap == 0:
            return self._expire(cutoff, None)[:3] + (0,)
        return self._expire(cutoff, cap)

    def expire_dev(self, cutoff, d_rows=None, d_node=None, cap=0):
        if bool(d_rows) != bool(d_node) or (not d_rows and cap):
            raise _einval("rio_gp_expire: the output rule")
        rows, nodes, n_idle, freed = self._expire(cutoff, int(cap) if d_rows and cap else None)
        if len(rows):
            _at(d_rows, len(rows))[:] = rows
            _at(d_node, len(rows))[:] = nodes
        return n_idle, freed

    def expire_raw(self, cutoff, out_rows=None, out_node=None, cap=0, want_n_idle=True):
        if not want_n_idle or (out_rows is None) != (out_node is None) or (out_rows is None and cap):
            return EINVAL, 0
        rows, nodes, n_idle, _ = self._expire(cutoff, int(cap) if out_rows is not None and cap else None)
        if len(rows):
            out_rows[:len(rows)] = rows
            out_node[:len(rows)] = nodes
        return OK, n_idle

    # ---- object classes
    def _classes_written(self):
        if self._fault == "classes_drop_solve":
            self._changed()

    def set_classes_raw(self, first_row, cls, rows=None):
        cls = np.asarray(cls, np.uint8)
        rows = len(cls) if rows is None else int(rows)
        if first_row > self._n or rows > self._n - first_row:
            return EINVAL
        self._K[first_row:first_row + rows] = cls[:rows]
        if self._fault == "classes_range_writes_past_end" and rows and first_row + rows < self._cap_rows:
            self._K[first_row + rows] = cls[rows - 1]
        self._classes_written()
        return OK

    def set_classes(self, first_row, cls):
        if self.set_classes_raw(first_row, cls) != OK:
            raise _einval("rio_gp_set_classes: the range exceeds the object table")

    def set_classes_dev(self, first_row, d_cls, rows):
        if first_row > self._n or rows > self._n - first_row:
            raise _einval("rio_gp_set_classes: the range exceeds the object table")
        self.set_classes(first_row, _at(d_cls, rows, np.uint8).copy())

    def _class_batch(self, idx, cls):
        idx, cls = np.asarray(idx, np.int64), np.asarray(cls, np.uint8)
        if self._fault == "classes_batch_first_wins":
            idx, cls = idx[::-1], cls[::-1]
        self._K[idx] = cls        # (numpy assigns in order: of a repeated index the last value stays)
        if self._fault == "classes_batch_dirty_pos" and len(idx):
            self._pos_dirty = np.unique(idx).astype(np.uint32)
        self._classes_written()

    def set_class_batch_raw(self, idx, cls):
        idx = np.asarray(idx, np.uint32)
        if len(idx) and int(idx.max()) >= self._n:
            return EINVAL
        self._class_batch(idx, cls)
        return OK

    def set_class_batch(self, idx, cls):
        if self.set_class_batch_raw(idx, cls) != OK:
            raise _einval("rio_gp_set_class_batch: object index out of range")

    def set_class_batch_dev_raw(self, d_idx, d_cls, n):
        idx, cls = _at(d_idx, n).copy(), _at(d_cls, n, np.uint8).copy()
        bad = idx >= self._n
        ok = ~bad
        if self._fault == "classes_dev_batch_stops_at_invalid" and bad.any():
            ok[int(np.argmax(bad)):] = False
        self._class_batch(idx[ok], cls[ok])
        return EINVAL if bad.any() else OK

    def get_classes(self):
        return self._K[:self._n].copy()

    # ---- immovable classes (rule 13)
    def set_class_movable_raw(self, movable, n_classes=None):
        mv = None if movable is None or not len(movable) else np.asarray(movable, np.uint8)
        k = (0 if mv is None else len(mv)) if n_classes is None else int(n_classes)
        f = self._fault
        if k > MAX_CLASSES or (k and mv is None):
            if f == "movable_refused_still_sets":
                self._I[:] = 1
                if mv is not None:
                    self._I[:] = mv[:MAX_CLASSES] != 0
            return EINVAL
        if f != "movable_short_table_keeps_old_flags":
            self._I[:] = 1
        if k:
            self._I[:k] = mv[:k] != 0
        self._K_at_I = self._K.copy()
        if f == "movable_drops_solve":
            self._changed()
        return OK

    def set_class_movable(self, movable=None):
        if self.set_class_movable_raw(movable) != OK:
            raise _einval("rio_gp_set_class_movable")

    def get_class_movable_raw(self):
        return OK, self._I.copy()

    def get_class_movable(self):
        return self._I.copy()

    def _expire_classes(self, cutoffs, cap):
        """cap None: count only.  -> rows, nodes, n_idle, load_freed, idle_by_class"""
        f = self._fault
        cut = np.asarray(cutoffs, np.uint32).astype(np.int64)
        nc = len(cut)
        if not 1 <= nc <= 256:
            raise _einval("rio_gp_expire_classes: 1 .. RIO_GP_MAX_CLASSES cutoffs are needed")
        n = self._cap_rows if f == "expc_lists_hidden_rows" else self._n
        col, k = self._col, self._K[:n].astype(np.int64)
        if f == "expc_high_class_is_class_0":
            k = np.where(k >= nc, 0, k)
        if f == "expc_cutoff_inclusive":
            cut = cut + 1
        limit = np.concatenate([cut, np.zeros(256 - nc, np.int64)])     # behind the given classes: nothing is older than 0
        idle = np.flatnonzero((col[:n] != NONE) & (self._S[:n] < limit[k])).astype(np.uint32)
        before, solved = self.get_nodes()[2], self._solved
        e = np.empty(0, np.uint32)
        if cap is None:
            listed, gone = e, (idle if f == "expc_count_only_writes" else e)
        else:
            listed = idle[:int(cap)]
            gone = idle if f == "expc_unplaces_past_cap" else listed
        by = np.bincount(k[listed if f == "expc_by_class_listed_only" else idle], minlength=256)[:nc].astype(np.uint64)
        if f == "expc_by_class_accumulates":
            self._by_acc[:nc] += by
            by = self._by_acc[:nc].copy()
        nodes = col[listed].copy()
        freed = int(self._load[listed].astype(np.uint64).sum())
        col[gone] = NONE
        if len(listed):        # as rio_gp_remove_batch of the listed rows
            self._changed()
            if f == "expc_keeps_solve":
                self._solved = solved
        return listed, nodes, len(idle), freed, by

    def expire_classes(self, cutoffs, cap=None, count_only=False):
        cap = self._n if cap is None else min(int(cap), self._n)
        if count_only or cap == 0:
            r = self._expire_classes(cutoffs, None)
            return r[:3] + (0, r[4])
        return self._expire_classes(cutoffs, cap)

    def expire_classes_dev(self, cutoffs, d_rows=None, d_node=None, cap=0):
        if bool(d_rows) != bool(d_node) or (not d_rows and cap):
            raise _einval("rio_gp_expire: the output rule")
        rows, nodes, n_idle, freed, by = self._expire_classes(cutoffs, int(cap) if d_rows and cap else None)
        if len(rows):
            _at(d_rows, len(rows))[:] = rows
            _at(d_node, len(rows))[:] = nodes
        return n_idle, freed, by

    def expire_classes_raw(self, n_classes, cutoffs, out_rows=None, out_node=None, cap=0, want_n_idle=True):
        if not 1 <= n_classes <= 256 or cutoffs is None:
            return EINVAL, 0
        if not want_n_idle or (out_rows is None) != (out_node is None) or (out_rows is None and cap):
            return EINVAL, 0
        rows, nodes, n_idle, _, _ = self._expire_classes(np.asarray(cutoffs, np.uint32)[:n_classes],
                                                         int(cap) if out_rows is not None and cap else None)
        if len(rows):
            out_rows[:len(rows)] = rows
            out_node[:len(rows)] = nodes
        return OK, n_idle

    def _census(self, flags, nc):
        """-> rc, rows, load (flat uint64, node-major), n_other"""
        f = self._fault
        by_node = bool(flags & CENSUS_BY_NODE)
        m = (self._cap_nodes if f == "census_uses_max_nodes" else self._m) if by_node else 1
        if flags & ~CENSUS_BY_NODE or not 1 <= nc <= 256 or m * nc > 1 << 20:
            return EINVAL, None, None, 0
        n = self._cap_rows if f == "census_counts_hidden_rows" else self._n
        A = self._col[:n]
        if f == "census_reads_solved" and self._solved is not None and len(self._solved) == n:
            A = self._solved
        cells = m * nc
        rows, load, other = np.zeros(cells, np.uint64), np.zeros(cells, np.uint64), 0
        r = np.flatnonzero(A != NONE)
        a, c = A[r].astype(np.int64), self._K[r].astype(np.int64)
        out = (c >= nc) | (a >= m if by_node else False)
        other = int(out.sum())
        r, cell = r[~out], ((a * nc if by_node else 0) + c)[~out]
        if len(r):             # the rows sorted by cell: each cell is one run, counted and summed in uint64
            order = np.argsort(cell, kind="stable")
            w = self._load[r[order]].astype(np.uint64)
            u, start = np.unique(cell[order], return_index=True)
            one = (w != 0) if f == "census_skips_zero_load_rows" else np.ones(len(w), bool)
            rows[u] = np.add.reduceat(one.astype(np.uint64), start)
            load[u] = np.add.reduceat(w, start)
        if f == "census_other_per_slice" and 4096 < cells <= 65536:
            other *= -(-cells // 4096)
        if f == "census_drops_solve":
            self._changed()
        return OK, rows, load, other

    def census_raw(self, n_classes, by_node=False, flags=None):
        fl = (CENSUS_BY_NODE if by_node else 0) if flags is None else int(flags)
        rc, rows, load, other = self._census(fl, int(n_classes))
        if rc != OK:
            e = np.zeros(0, np.uint64)
            return rc, e, e, 0
        shape = (len(rows) // int(n_classes), int(n_classes)) if by_node else (int(n_classes),)
        return rc, rows.reshape(shape), load.reshape(shape), other

    def census(self, n_classes, by_node=False):
        rc, rows, load, other = self.census_raw(n_classes, by_node)
        if rc != OK:
            raise _einval("rio_gp_census")
        return rows, load, other

    def census_dev(self, n_classes, d_rows, d_load, by_node=False):
        rc, rows, load, other = self._census(CENSUS_BY_NODE if by_node else 0, int(n_classes))
        if rc != OK or not d_rows or not d_load:
            raise _einval("rio_gp_census")
        cells = (self._m if by_node else 1) * int(n_classes)     # (the caller's arrays hold m * n_classes cells)
        for p, v in ((d_rows, rows), (d_load, load)):
            out = _at(p, cells, np.uint64)
            out[:] = (out + v[:cells]) if self._fault == "census_dev_adds" else v[:cells]
        return other

    # ---- measured load
    def _hits_add(self, idx, w):
        """H[idx[k]] += w[k], saturating: the sums in uint64 (fewer than 2^31 entries of less than 2^32 each)."""
        idx = np.asarray(idx, np.int64)
        w = np.ones(len(idx), np.uint64) if w is None else np.asarray(w, np.uint32).astype(np.uint64)
        s = self._H.astype(np.uint64)
        np.add.at(s, idx, w)
        self._H = (s & np.uint64(U32) if self._fault == "hits_add_wraps" else np.minimum(s, np.uint64(U32))).astype(np.uint32)
        if self._fault == "hits_drop_solve":
            self._changed()

    def hits_add_raw(self, idx, n=None, weight=None):
        idx = np.asarray(idx, np.uint32)
        if len(idx) and int(idx.max()) >= self._n:
            return EINVAL
        self._hits_add(idx, weight)
        return OK

    def hits_add(self, idx, weight=None):
        if self.hits_add_raw(idx, weight=weight) != OK:
            raise _einval("rio_gp_hits_add_batch: object index out of range")

    def hits_add_dev(self, d_idx, n, d_weight=None):
        idx = _at(d_idx, n).copy()
        w = _at(d_weight, n).copy() if d_weight else np.ones(n, np.uint32)
        bad = idx >= self._n
        ok = ~bad
        if self._fault == "hits_dev_stops_at_invalid" and bad.any():
            ok[int(np.argmax(bad)):] = False
        self._hits_add(idx[ok], w[ok])
        if bad.any():
            raise _einval("rio_gp_hits_add_batch: invalid entries were skipped")

    def hits_merge(self, counts):
        counts = np.asarray(counts, np.uint32)
        rows = len(counts)
        if rows > self._n:
            raise _einval("rio_gp_hits_merge: rows exceeds the object table")
        self._hits_add(np.arange(rows), counts)
        if self._fault == "hits_merge_past_rows" and rows % 4:
            self._hits_add(np.arange(rows, min(rows + 4 - rows % 4, self._cap_rows)), None)

    def hits_merge_dev(self, d_counts, rows):
        if rows > self._n:
            raise _einval("rio_gp_hits_merge: rows exceeds the object table")
        self.hits_merge(_at(d_counts, rows).copy())

    def get_hits(self):
        return self._H[:self._n].copy()

    def load_fold_raw(self, keep, gain, min_load, max_load, _stats=None):
        f, n = self._fault, self._n
        if keep > 65536 or min_load > max_load:
            if f == "fold_refused_still_zeroes_hits":
                self._H[:n] = 0
            return EINVAL
        rows = self._cap_rows if f == "fold_past_n" else n
        old, h = self._load[:rows].astype(np.uint64), self._H[:rows].astype(np.uint64)
        lo, hi = np.uint64(min_load), np.uint64(max_load)
        x = (old * np.uint64(keep)) >> np.uint64(16)
        if f == "fold_clamps_before_gain":
            new = np.minimum(np.clip(x, lo, hi) + h * np.uint64(gain), np.uint64(U32))
        else:
            new = np.clip(x + h * np.uint64(gain), lo, hi)
        if _stats is not None:
            _stats.update(rows_changed=int((old[:n] != new[:n]).sum()), hits_folded=int(h[:n].sum()), load_before=int(old[:n].sum()),
                          load_after=int(new[:n].sum()), max_load_after=int(new[:n].max()) if n else 0)
        before, solved = self.get_nodes()[2], self._solved
        self._load[:rows] = new.astype(np.uint32)
        if f != "fold_keeps_hits":
            self._H[:rows] = 0
        self._changed()
        if f == "fold_keeps_solve":
            self._solved = solved
        if f == "fold_stale_used":
            self._stale_used = before
        return OK

    def load_fold(self, keep, gain, min_load=0, max_load=U32):
        st = {}
        if self.load_fold_raw(keep, gain, min_load, max_load, st) != OK:
            raise _einval("rio_gp_load_fold: keep > 65536 or min_load > max_load")
        return st

    # ---- hot-object report
    def _top(self, flags, node, min_key, cap):
        """-> rc, rows, keys, nodes, n_candidates, key_sum"""
        f, e = self._fault, np.empty(0, np.uint32)
        if cap > TOP_MAX or flags & ~(TOP_BY_HITS | TOP_PLACED | TOP_ON_NODE) or (flags & TOP_ON_NODE and node >= self._m):
            return EINVAL, e, e, e, 0, 0
        A, n = self._col, self._n
        if f == "top_reads_solved" and self._solved is not None and len(self._solved) == n:
            A = self._solved
        if f == "top_lists_hidden_rows":
            n = self._cap_rows
        kflags = flags & ~TOP_BY_HITS if f == "top_hits_key_ignores_flag" else flags
        rows, keys, nodes, nc, ks = spec_top.top_rows(A, self._load, self._H, n, kflags, node, min_key, cap)
        if f == "top_ties_to_highest_rows":
            r, k, _, _, _ = spec_top.top_rows(A, self._load, self._H, n, kflags, node, min_key, n)
            rows = r[np.lexsort((-r.astype(np.int64), -k.astype(np.int64)))][:int(cap)]
            keys, nodes = (self._H if kflags & TOP_BY_HITS else self._load)[rows], A[rows]
        if f == "top_key_sum_of_listed_only":
            ks = int(keys.astype(np.uint64).sum())
        if f == "top_drops_solve":
            self._changed()
        return OK, rows, keys, nodes, nc, ks

    def _top_out(self, arrays, values, cap):
        """The listing into the caller's arrays of cap entries (a missing one is skipped)."""
        L = len(values[0])
        for out, v in zip(arrays, values):
            if out is not None:
                out[:L] = v
                if self._fault == "top_writes_past_listing" and L < len(out):
                    out[L] = 0

    def top_rows(self, cap, by_hits=False, placed=False, node=None, min_key=0, want_node=True):
        flags = (TOP_BY_HITS if by_hits else 0) | (TOP_PLACED if placed else 0) | (TOP_ON_NODE if node is not None else 0)
        rc, rows, keys, nodes, nc, ks = self._top(flags, int(node or 0), int(min_key), int(cap))
        if rc != OK:
            raise _einval("rio_gp_top_rows")
        return rows, keys, (nodes if want_node else None), nc, ks

    def top_rows_dev(self, flags, node, min_key, d_rows, d_key, d_node, cap):
        if bool(d_rows) != bool(d_key) or (not d_rows and (cap or d_node)):
            raise _einval("rio_gp_top_rows: the output rule")
        rc, rows, keys, nodes, nc, ks = self._top(int(flags), int(node), int(min_key), int(cap))
        if rc != OK:
            raise _einval("rio_gp_top_rows")
        if d_rows:    # (a "device" array of cap entries: the scenario's buffers are longer, as the host's are)
            self._top_out([_at(p, cap + 1) if p else None for p in (d_rows, d_key, d_node)], (rows, keys, nodes), cap)
        return nc, ks

    def top_rows_raw(self, flags, node=0, min_key=0, out_rows=None, out_key=None, out_node=None, cap=0, want_n=True):
        if not want_n or (out_rows is None) != (out_key is None) or (out_rows is None and (cap or out_node is not None)):
            return EINVAL, 0
        rc, rows, keys, nodes, nc, _ = self._top(int(flags), int(node), int(min_key), int(cap))
        if rc == OK:
            self._top_out((out_rows, out_key, out_node), (rows, keys, nodes), cap)
        return rc, nc

    # ---- lab calls: no-ops
    def set_compact(self, *a, **k):
        return None

    def set_speculate(self, *a, **k):
        return None

    def chained_scans(self):
        return self._chained


def module(fault=None):
    """The surface of this module with every handle created under `fault` (one of FAULTS, or None)."""
    def make(*a, **k):
        k.setdefault("fault", fault)
        return GpuPlacement(*a, **k)
    return types.SimpleNamespace(GpuPlacement=make, CFG_REF_SELF_ASSIGN=CFG_REF_SELF_ASSIGN, balanced_targets=balanced_targets,
                                 DevBuf=DevBuf, ObjectPlacementError=ObjectPlacementError, build=build, NONE=NONE,
                                 CAP_INF=CAP_INF, OK=OK, EINVAL=EINVAL, ERANGE=ERANGE, fault=fault)
