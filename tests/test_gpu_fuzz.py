"""Randomised operation sequences through the C ABI against the CPU oracle, bit for bit after EVERY operation.

One scenario = a random table (sizes drawn around the kernels' thresholds: tile, workgroup and batch-size boundaries), random
capacities (unbounded / tight / zero), loads, affinities (nodes, NONE, RIO_GP_AFF_INACTIVE), liveness, the reference's
self-assignment switch on or off — then 12-30 operations drawn from everything the dense layer offers: committed and
uncommitted solves (synchronous, asynchronous streams), liveness flips, update / remove / lookup batches, clean_server(s),
place_pending at every batch-size regime (one workgroup, three launches, plain kernels, window-sorted), new loads /
affinities / capacities.  A second kind of scenario drives the ROW-SHARDED solve (G handles on the one device, random shard
boundaries with empty shards, streams of committed ticks with liveness changes) against the whole-table oracle.  The fix-up policies the product picks adaptively are also forced through the lab build's knobs, by
seed.  The seeds are fixed: a failure names the seed and the operation.

A second family of scenarios ("extended": Scenario(..., ext=True), seeds and generator of its own) draws from OPS_EXT: the old
operations plus the reverse index (rio_gp_rows_on_nodes[_dev], every call form), the bounded rebalance (rio_gp_rebalance[_dev],
against tests/rebalance_ref.py and, up to 4 096 rows, tests/spec_rebalance.py), the change feed (rio_gp_changes[_dev] / _reset
against tests/spec_changes.py, plus a mirror fed by the consuming listings that must equal the column at the end) and
rio_gp_set_num_objects.  It also checks that calls which promise to change nothing leave an uncommitted solve as it was (and
committable), that every other call drops it, that the index and the feed leave quiet ticks chained while a rebalance ends the
chain, and calls all three between rio_gp_tick_async and rio_gp_tick_wait.  The old family's tables, operations and draws are
untouched (tests/test_fuzz_driver.py replays them against a CPU stand-in and a recorded log).

Node removal (rio_gp_remap_nodes, against tests/spec_remap.py over every row the model holds, the hidden ones included) is one of
the extended operations: the identity, a permutation, a swap, one node, several nodes with stable compaction or with the survivors
shuffled, exactly the dead nodes, the node most rows are on — at least one node is kept, and a third of the removals end on a node
count at which a kernel changes its per-node form, on a handle that keeps its larger max_nodes.  After a legal map: the evicted
count (rows < n), num_nodes, cap and alive at their new ids, the renumbered affinity, the column and `used`; an uncommitted solve
is gone; the consumer's mirror is renumbered by the scenario (RIO_GP_NODE_GONE for a removed node), so the feed's old nodes stay
checked; rows hidden at the time are compared when n grows again and at the end.  About one map in ten is illegal (a duplicate, a
kept value >= m_new, too few kept entries, m_new > m): RIO_GP_EINVAL and nothing changed, an uncommitted solve included.  It is
also called between tick_async and tick_wait and in the middle of a chained quiet run, where the tick after it must not chain.

Idle expiry (tests/spec_expire.py) is fuzzed the same way: the scenario keeps a model S of the last-seen column over every row the
handle holds and a clock of its own (epochs mostly rise, some repeat or fall, 0 and 0xFFFFFFFF now and then).  `touch` draws one of
the family's writers — the host batch (and one refused for an index >= n), the _dev batch (sometimes not 16-byte aligned; with
invalid entries it applies the rest and reports RIO_GP_EINVAL), touch_all, touch_merge host and _dev (rows 0, n, a boundary size,
any; stamps below, at and above what S holds) and a merge of n + 1 rows, refused — and rio_gp_get_seen must equal S[:n] after each,
an uncommitted solve still there.  `expire` draws a cutoff (0, a placed row's own stamp, one above the largest, 0xFFFFFFFF), a cap
(none, 0, 1, small, n_idle - 1 / n_idle / n_idle + 1, one that ends the listing inside a tile of 1 024 rows) and a form (host,
the call as given into sentinel-filled arrays, _dev, count-only host and _dev): rows, nodes, n_idle and load_freed are exact,
nothing is written past the listing, the column and `used` follow, S does not change; a sweep that listed rows drops an
uncommitted solve and ends a chained run, one that listed nothing (or only counted) leaves both alone.  Both are also called
between tick_async and tick_wait and in the middle of chained quiet runs; S is compared again when hidden rows come back and after
every node removal (S names no node).

Measured load, the hot-object report and the load-ordered rebalance cut are fuzzed the same way.  The scenario keeps a model H of the hit column over every row the handle holds.  `hits`
draws one of the family's writers (tests/spec_loads.py) — the host batch with and without weights, duplicates included (and one
refused for an index >= n), the _dev batch (sometimes not 16-byte aligned; with invalid entries it applies the rest and reports
RIO_GP_EINVAL), the merge host and _dev (rows 0, n, a boundary size, any, so every rows % 4; the _dev array sometimes behind 1-3
words of padding) and a merge of n + 1 rows, refused; about one call in ten carries values that fill a counter exactly, miss
0xFFFFFFFF by one, overshoot it, and plain 0xFFFFFFFF — and rio_gp_get_hits must equal H[:n] after each, an uncommitted solve
still there.  `fold` draws (keep, gain, min_load, max_load) by kind (identity, replace, decay, one value for every row, a small
max_load, a gain that takes H * gain past 2^32); the five statistics, the loads, H zero on [:n] and `used` of the new loads are
exact, and every legal fold — the identity too — drops an uncommitted solve and ends a chained run; about one in ten is refused
(keep 65537, min_load > max_load) and changes nothing.  A quarter of the folds call rio_gp_set_num_objects themselves right
before, with nothing in between, so that `used` is not valid when the fold picks its kernel (the scenario's own check after every
operation makes it valid again), sometimes onto a row that holds hits in the middle of its quad.  `top` draws all eight flag
sets, a node (any, the fullest, an empty one, one >= m: refused under ON_NODE and ignored without), min_key (0, a key that occurs,
the largest, one above, 0xFFFFFFFF), a cap (0, 1, small, n_candidates - 1 / n_candidates / n_candidates + 1, 4 096, one that cuts
inside a group of equal keys lying in more than one tile of 1 024 rows) and a form (host with and without out_node, the call as
given into sentinel-filled arrays, _dev with and without d_node, count-only host and _dev) against tests/spec_top.py, whose H is
None until a call of the hits section has been made; cap 4 097 and an unknown flag bit are refused; rows, keys, nodes,
n_candidates and key_sum are exact, nothing is written behind the listing, H and an uncommitted solve are as they were.
`rebalance` draws its order: by load it goes through tests/rebalance_order_ref.py and, up to 4 096 rows, through
tests/spec_rebalance_order.py, which must agree first; on more than 3 072 nodes half of those calls take all-zero targets, and while
more than 3 072 live nodes hold load four rebalances in five go by load and all of those take them.  All
three new calls are also made between tick_async and tick_wait and in the middle of chained quiet runs (hits and top leave the
run chained, a fold ends it), right behind an uncommitted solve, and — the report — right behind a sweep that listed rows and
between two pages of the feed; H is compared again after every node removal and sweep, and H and the loads when hidden rows come
back and, over every row, at the end.

Object classes are fuzzed the same way.  The scenario keeps a model K of the class column
over every row the handle holds; only the setters change it.  `classes` draws one call of the setter family (tests/spec_classes.py) — the host range (start and end each at 0, n, a boundary
size or any row, on every residue mod 4, the source 0-3 bytes into its buffer), the _dev range (the array behind 0-3 bytes of
padding), a range reaching n + 1 (refused), the host batch (sizes from _BATCHES, half the time its second half naming the rows of
the first again with classes of its own: the last entry wins), one with an index >= n (refused), the _dev batch (with invalid
entries it applies the rest and reports RIO_GP_EINVAL) and a batch of 0 entries; the classes are all one, a few small ones, uniform
over 0 .. 255, small ones with 255 and values beyond the n_classes later calls pass, or four different ones in every quad of rows —
and rio_gp_get_classes must equal K[:n] after each, `used` and an uncommitted solve as they were.  About one batch in four is
followed at once by an update batch over some of its rows: the election borrows rio_gp_update_batch's position scratch.
`expire_classes` is op_expire with a cutoff per class (spec_classes.expire_classes_np; up to 4 096 rows the Python-integer
expire_classes must agree first): n_classes from 1, 2, 3, 8, 64, 255, 256 and the largest class present (whose rows are then never
idle), each cutoff 0, a placed row's own stamp, one above the largest stamp or 0xFFFFFFFF — per class, one value for every class,
or 0 for all but one class — op_expire's caps and forms, idle_by_class given or NULL: rows, nodes, n_idle, load_freed and
idle_by_class (every idle row, listed or not: it sums to n_idle) are exact, nothing is written past the listing, S and K do not
change; under one cutoff for all 256 classes the count equals rio_gp_expire's, and on an all-zero column one cutoff lists what
tests/spec_expire.py lists; n_classes 0 and 257 are refused.  `census` draws totals or RIO_GP_CENSUS_BY_NODE, host or _dev (into
sentinel-filled arrays: the call overwrites), n_classes from 1, 2, 16, 17, 255, 256 or, by node, so that m * n_classes lies on
and next to the boundaries of the kernel's forms (4 096, 65 536 and 2^20 cells, the first value past 2^20 refused) against
spec_classes.census_np (up to 4 096 rows the Python-integer census must agree first): out_rows, out_load (uint64) and n_other are
exact and sum to the placed rows and their load, and K, H, the column, `used` and an uncommitted solve are as they were; an unknown
flag bit and n_classes 0 and 257 are refused.  All three are also called between tick_async and tick_wait and in the middle of
chained quiet runs (only a class sweep that un-placed a row ends the chain), right behind an uncommitted solve, and — the sweep —
right behind a report, behind another class sweep with a different n_classes and between two pages of the feed; a sweep or a census
comes right behind a setter and a census right behind a fold now and then.  K is compared again after every node removal (on a
handle no call of the section has touched it must come back all 0), sweep and change of n and, over every row, at the end; once
per row-sharded scenario a setter, a sweep and a census on a shard handle are refused.

Immovable classes (DESIGN.md section 2 rule 13) are fuzzed the same way.  The scenario keeps a model I of the handle's 256 flags, all
movable to begin with; only a legal rio_gp_set_class_movable changes it.  `movable` draws one such call: a reset (NULL, or n_classes 0
beside an array that is not read), or n_classes from 1, 2, 3, 8, 64, 255, 256 with every class movable, every class immovable, about
half of them, only class 255, only the class most placed rows below n hold, only classes no row below n holds, or a table that ends
below the largest class present, so that the classes from there on are movable again (a movable class's flag is any nonzero byte, and
the array is sometimes longer than n_classes) — through the checked and the raw form; about one call in ten is refused (n_classes 257
with an array that would change the table, a NULL array with n_classes > 0): RIO_GP_EINVAL and I as it was.  After every call
rio_gp_get_class_movable equals I, the class column is the model's (the call may be the one that allocates it, all 0), and the column,
`used` and an uncommitted solve are as they were; in the middle of a chained quiet run the ticks after it stay chained.  `rebalance`
under a table that names an immovable class is compared with the same vectorised references on aff' — the affinity with
RIO_GP_AFF_INACTIVE on every row below n whose class is immovable, the equivalence the rule states — and, up to 4 096 rows and within a
bound on its cost (live nodes x selected rows x rounds <= 4 000 000: its R3 walks the nodes once per waiting row), with
tests/spec_movable.py, which takes K[:n] and I themselves and must agree first; afterwards the affinity column is what it was, the table
is I and no listed row is of an immovable class.  A third of the rebalances set a table themselves right before the call, with only
the table's getter in between; the one in the middle of a quiet run and every one that sends the by-load cut to its histograms in
global memory (more than 3 072 over nodes) always do.  A rebalance comes right behind a `movable`, right behind a setter that changed
the class of a placed row and right behind a class sweep that listed rows now and then, and `movable` is among the calls made right
behind an uncommitted solve, between tick_async and tick_wait and in the middle of quiet runs.  I is compared again after every change
of n, after every legal and every refused node removal and at the end; once per row-sharded scenario the call is refused on a shard
handle, whose table stays all 1.

    python tests/test_gpu_fuzz.py <seconds> [first_seed]     # a longer campaign: old and extended scenarios alternate
"""
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
AFF_INACTIVE = 0xFFFFFFFE
INF = 0xFFFFFFFFFFFFFFFF

_SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 65536, 262143, 262144, 262145)
_BATCHES = (1, 2, 4, 5, 255, 256, 257, 1000, 1024, 1025, 4095, 4096, 4097, 20000, 65535, 65536, 65537, 131072)
# the node counts a scenario draws its m from (Scenario.__init__ keeps its own literal: the old family's draws stay as recorded)
_NODES = (1, 2, 3, 7, 31, 32, 33, 64, 100, 255, 256, 257, 1000, 1024, 1025, 4096, 5000, 8191, 8192)


def _pick(rng, table, hi):
    """A size: half the time one of the boundary values (below hi), else log-uniform in [1, hi]."""
    if rng.random() < 0.5:
        c = [v for v in table if v <= hi]
        return int(c[rng.integers(len(c))])
    return int(np.exp(rng.uniform(0, np.log(hi))))


class Scenario:
    def __init__(self, gp, oracle, seed, big=False, ext=False):
        """ext: the operations are drawn from OPS_EXT (the reverse index, the rebalance, the change feed and set_num_objects beside
        the old ones), from a generator of its own, and the scenario keeps what their checks need (see "extended scenarios")."""
        self.gp, self.oracle, self.seed, self.ext = gp, oracle, seed, bool(ext)
        rng = self.rng = np.random.default_rng((0xE87E0000 if ext else 0x5EED0000) + seed)
        self.n = n = _pick(rng, _SIZES + (524288, 1_000_000), 2_000_000 if big else 300_000)
        if big and rng.random() < 0.3:   # a campaign spends a third of its scenarios on tables of 10^5 .. 2 x 10^6 rows
            self.n = n = int(np.exp(rng.uniform(np.log(100_000), np.log(2_000_000))))
        self.m = m = int(rng.choice([1, 2, 3, 7, 31, 32, 33, 64, 100, 255, 256, 257, 1000, 1024, 1025, 4096, 5000, 8191, 8192]))
        self.rounds = int(rng.choice([1, 2, 2, 2, 3]))
        self.sa = bool(rng.random() < 0.25)
        self.flags = gp.CFG_REF_SELF_ASSIGN if self.sa else 0
        self.oflags = oracle.REF_SELF_ASSIGN if self.sa else 0
        kind = rng.integers(4)
        self.load = {0: lambda: rng.integers(0, 30, n), 1: lambda: np.ones(n), 2: lambda: rng.zipf(1.3, n).clip(0, 60000),
                     3: lambda: rng.integers(0, 2, n) * rng.integers(0, 1000, n)}[int(kind)]().astype(np.uint32)
        self.aff = rng.integers(0, m, n).astype(np.uint32)
        r = rng.random(n)
        self.aff[r < 0.08] = NONE
        self.aff[(r >= 0.08) & (r < 0.11)] = AFF_INACTIVE
        if rng.random() < 0.3:      # a hot affinity node
            self.aff[rng.random(n) < 0.4] = int(rng.integers(m))
        self.cap = self._caps()
        self.alive = (rng.random(m) > rng.choice([0.0, 0.1, 0.5])).astype(np.uint8)
        start = rng.integers(3)
        if start == 0:
            self.ref = np.full(n, NONE, np.uint32)
        else:
            self.ref = rng.integers(0, m, n).astype(np.uint32)
            self.ref[rng.random(n) < (0.02 if start == 1 else 0.5)] = NONE
        self.lab = seed % 3 == 2
        # half of the lab scenarios: the quiet asynchronous ticks overlap / chain whatever the table's size (the product's rule
        # needs 2^22 rows) — their scans alternate between two streams and hand the rows over wave range by wave range
        self.chain_small = self.lab and (seed // 3) % 2 == 1
        if self.chain_small:
            os.environ["RIO_GP_OVERLAP_MIN_ROWS"] = "1"
        try:
            g = self.g = gp.GpuPlacement(n, m, spill_rounds=self.rounds, flags=self.flags, lab=self.lab)
        finally:
            os.environ.pop("RIO_GP_OVERLAP_MIN_ROWS", None)
        g.set_nodes(self.cap, self.alive, m=m)
        g.set_objects(n, self.load, self.aff)
        g.set_assign(self.ref)
        if self.lab:
            k = (seed // 3) % 6
            g.set_compact(("never", "always", "never", "always", "auto", "auto")[k], cut_pack=("never", "never", "always", "never", "auto", "auto")[k],
                          inc=("auto", "always", "never", "never", "always", "never")[k],
                          cut_apply=("auto", "never", "always")[(seed // 54) % 3])   # (the one-pass / the two-pass whole-table fix-up)
            g.set_speculate(("never", "always", "auto")[(seed // 18) % 3])
        self.log = []
        self.count = {}
        # extended scenarios: the handle's max_objects (n shrinks and grows below it: the arrays keep their full length, every
        # operation works on [:n]); the feed's checkpoint column and a mirror fed by consuming listings only; the expected column
        # of an uncommitted solve (None: there is none); whether liveness changed with no tick since; the coverage-floor counters
        self.nmax = n
        self.B = np.full(n, NONE, np.uint32)
        self.mirror = np.full(n, NONE, np.uint32)
        self.pending = None
        self.fresh_flip = False
        self.in_flight = False
        self.page_open = self.page_writer = False
        self.paging_out = self.mixed_wrote = False
        self.m0 = m                # the handle's max_nodes: a removal leaves m below it
        self.remapped = self.remap_refused = False
        # idle expiry: the model of the last-seen column (rows >= n keep their value), the scenario's own clock for epochs,
        # whether a call of the family has been made (the first one allocates S), whether the last sweep un-placed anything
        self.S = np.zeros(n, np.uint32)
        self.clock = 0
        self.seen_used = self.expire_listed = False
        self.mids = 0              # quiet runs so far (op_async: which call goes into the middle of the next one)
        self.behind = 0            # calls sent right behind an uncommitted solve so far (run(): which call is next)
        self.flights = 0           # streams with a call between tick_async and tick_wait so far (op_async: which call is next)
        # measured load: the model of the hit column (rows >= n keep their value), whether a call of the section has been made
        # (the first one allocates H: until then the report's model has none), whether the last fold was refused, whether the
        # last legal fold left every load equal; mark / after: what the last operation left behind for the one right after it
        # ("expire listed": the sweep has just used the scratch the report shares)
        self.H = np.zeros(n, np.uint32)
        self.hits_used = self.fold_refused = self.fold_equal = False
        self.mark = self.after = None
        # object classes: the model of the class column (rows >= n keep their value), whether a call of the section has been made
        # (the first one allocates K, all 0), the n_classes of the last class sweep, whether the last one un-placed anything;
        # in_mid: the operation runs in the middle of a chained quiet run (op_classes adds no writer of its own there)
        self.K = np.zeros(n, np.uint8)
        self.cls_used = self.expc_listed = self.in_mid = False
        self.last_nc = None
        # immovable classes: the model of the table (1: movable), the n_classes of the last legal call, the classes that were
        # immovable at the last rebalance under a table (until the first plain rebalance after it)
        self.I = np.ones(256, np.uint8)
        self.mv_nc = 0
        self.was_imm = np.zeros(256, bool)
        self.cov = {}

    def _caps(self):
        rng, m = self.rng, self.m
        total = int(self.load[:self.n].sum())
        k = rng.integers(4)
        if k == 0:
            return np.full(m, INF, np.uint64)
        if k == 1:
            return rng.integers(0, total // m + 5, m).astype(np.uint64)            # tight: about half fits
        if k == 2:
            c = rng.integers(0, 3 * (total // m) + 5, m).astype(np.uint64)          # roomy, some zero, some unbounded
            c[rng.random(m) < 0.1] = 0
            c[rng.random(m) < 0.1] = INF
            return c
        return np.full(m, (total * 5 // 4) // m + 1, np.uint64)                     # BASELINE's 1.25x

    # ---- checks -------------------------------------------------------------------------------------------------------
    def check_table(self, what):
        if self.in_flight:     # (the first look at the table since the ticks were enqueued: what they did wrong shows here)
            what = "%s, behind tick_async" % what
        got, ref = self.g.get_assign(), self.ref[:self.n]
        assert np.array_equal(got, ref), (self.seed, what, self.log[-6:], np.flatnonzero(got != ref)[:8])
        used = self.oracle.recompute_used(ref, self.load[:self.n], self.m)
        gu = self.g.get_nodes()[2]
        assert np.array_equal(gu, used), (self.seed, what, self.log[-6:], np.flatnonzero(gu != used)[:8])

    def otick(self):
        n = self.n
        return self.oracle.tick(self.ref[:n], self.load[:n], self.aff[:n], self.cap, self.alive, self.rounds, self.oflags)

    def _set_col(self, want):
        """The model's column after a commit: rows >= n keep what they hold."""
        if len(want) == len(self.ref):
            self.ref = want
        else:
            self.ref[:self.n] = want

    # ---- operations ---------------------------------------------------------------------------------------------------
    def op_tick(self):
        st = self.g.tick()
        want, used, ost = self.otick()
        self._set_col(want)
        self.pending, self.fresh_flip = None, False
        assert st == ost, (self.seed, "tick", self.log[-6:], st, ost)

    def op_solve(self):
        st = self.g.solve()
        want, used, ost = self.otick()
        got = self.g.get_solved()
        assert st == ost, (self.seed, "solve", self.log[-6:], st, ost)
        assert np.array_equal(got, want), (self.seed, "solve", self.log[-6:], np.flatnonzero(got != want)[:8])
        self.fresh_flip = False
        if self.rng.random() < (0.3 if self.ext else 0.5):   # (extended scenarios: more of the calls meet an uncommitted solve)
            self.g.commit()
            self._set_col(want)
            self.pending = None
        else:
            self.pending = want

    def op_async(self):
        k = int(self.rng.integers(1, 5))
        # a longer stream without changes: verdicts land, the ticks chain (extended scenarios: more often, for the calls in its middle)
        # (the first asynchronous stream of such an extended scenario always is one, and run() makes sure there is a stream: the
        # default seeds hold more of these scenarios than there are calls to put into the middle of a run)
        quiet_run = self.chain_small and (self.rng.random() < (0.75 if self.ext else 0.5) or (self.ext and self.mids == 0))
        if quiet_run:
            k += 6
        last_chained = False
        want_st = []
        # extended scenarios, a quiet run: a call in the middle of it (see _mid_call); any run: a call between the last tick_async
        # and tick_wait, whose answer reflects every enqueued tick
        # (the calls take turns, from a start the seed sets: eighteen of the default seeds have such runs, one start each, and MID
        #  holds sixteen entries, so each call gets one)
        mid = "none"
        if self.ext and quiet_run:
            mid = self.MID[(self.seed // 6 + self.mids) % len(self.MID)]
            self.mids += 1
        watch = None
        self.after = None          # (the ticks below come between the operation before and the calls in flight)
        for i in range(k):
            if i and not quiet_run and self.rng.random() < 0.5:
                self.op_flip()
            if mid != "none" and i == k - 4:
                watch = self._mid_call(mid, last_chained)
            c0 = self.g.chained_scans() if self.lab and mid != "none" else 0
            self.g.tick_async()
            want, used, ost = self.otick()
            self._set_col(want)
            self.pending, self.fresh_flip = None, False
            want_st.append(ost)
            if self.lab and mid != "none":
                last_chained = self.g.chained_scans() - c0 == 1
                if watch is not None and watch[0] in self.ENDS_CHAIN and i == k - 4:
                    # a rebalance, a node removal (the identity map too), a fold (the identity fold too) and a sweep that
                    # un-placed a row change the inputs: the tick after does not chain
                    assert not last_chained, (self.seed, watch[0], "the tick after a %s chained" % watch[0], self.log[-6:])
            if self.rng.random() < 0.3 or (quiet_run and i < 3):
                time.sleep(0.002)
        if watch is not None and watch[0] not in self.ENDS_CHAIN and watch[1]:
            # the tick before the call was a link of a chain and nothing has changed since: the 4 ticks after it are links too,
            # as they are in the same run without the call
            c = self.g.chained_scans() - watch[2]
            assert c == 4, (self.seed, watch[0], "quiet ticks after the call did not stay chained", c, self.log[-6:])
            self.cov["chained across a call"] = self.cov.get("chained across a call", 0) + 1
            self._hit("chained across a census", watch[0] == "census")
            self._hit("chained across a movable", watch[0] == "movable")
        self.mark = None           # (a call in the middle of the run is not "right before" what follows the ticks after it)
        if self.ext and self.rng.random() < 0.7:
            self.in_flight = True
            try:
                # (the calls take turns, from a start the seed sets: each of them gets a few of the default seeds' streams)
                what = self.IN_FLIGHT[(self.seed + self.flights) % len(self.IN_FLIGHT)]
                self.flights += 1
                self.log.append("in flight: " + what)
                self.count["in flight: " + what] = self.count.get("in flight: " + what, 0) + 1
                getattr(self, "op_" + what)()
            finally:
                self.in_flight = False
        got = self.g.tick_wait()
        assert got == want_st, (self.seed, "tick_async", self.log[-6:], got, want_st)

    def _mid_call(self, what, last_chained):
        """A call between the quiet asynchronous ticks of a run (lab build, every tick may chain).  The index and a consuming feed
        call change nothing a tick reads: if the tick before was a link of a chain, the ticks after are.  A rebalance ends the
        chain, and so does a node removal.  A touch, a count-only sweep and a sweep that lists nothing change nothing either; a
        sweep that un-placed a row ends the chain ("expire" comes back as "expire count" when it listed nothing).  The hits calls
        and the report change nothing; a legal fold ends the chain whatever it folds.  The class setters, the census, a count-only
        class sweep and one that lists nothing change nothing; a class sweep that un-placed a row ends the chain.
        -> (what, the tick before chained, chained_scans() after the call)"""
        self.log.append("mid run: " + what)
        self.count["mid run: " + what] = self.count.get("mid run: " + what, 0) + 1
        self.in_mid = True
        try:
            what = self._mid_op(what)
        finally:
            self.in_mid = False
        return what, last_chained, self.g.chained_scans() if self.lab else 0

    def _mid_op(self, what):
        if what == "index":
            self.op_index()
        elif what == "changes":
            self._feed(None if self.rng.random() < 0.5 else int(self.rng.integers(1, 50)), False, False)
        elif what == "rebalance":
            self.op_rebalance()
        elif what == "touch":
            self.op_touch()
        elif what == "hits":
            self.op_hits()
        elif what == "top":
            self.op_top()
        elif what == "fold":
            self.op_fold(legal=True)      # (a refused fold changes nothing: only a legal one must end the chain)
        elif what == "expire count":
            self.op_expire(hit=False)
        elif what == "expire":
            if not self.op_expire(hit=True):
                what = "expire count"
        elif what == "classes":
            self.op_classes()
        elif what == "census":
            self.op_census()
        elif what == "expire_classes count":
            self.op_expire_classes(hit=False)
        elif what == "expire_classes":
            if not self.op_expire_classes(hit=True):
                what = "expire_classes count"
        elif what == "movable":
            self.op_movable()
        else:
            self.op_remap(legal=True)     # (a refused map changes nothing: only a legal one must end the chain)
        return what

    def op_flip(self):
        rng, m = self.rng, self.m
        self.pending, self.fresh_flip = None, True   # (a liveness push is a change of the inputs: an uncommitted solve is dropped)
        k = rng.integers(3)
        if k == 0:
            j = int(rng.integers(m))
            self.alive[j] ^= 1
            self.g.set_alive(j, int(self.alive[j]))
        elif k == 1:
            self.alive = (rng.random(m) > 0.1).astype(np.uint8)
            self.g.set_alive_all(self.alive)
        else:
            self.alive = np.ones(m, np.uint8)
            self.g.set_alive_all(self.alive)

    def _idx(self, k=None, big_ok=True):
        rng, n = self.rng, self.n
        if k is None:
            k = _pick(rng, _BATCHES, 140000 if n >= 20000 else 20000)
            if big_ok and n >= 20000 and rng.random() < 0.2:
                k = int(rng.integers(262144, 600000))     # the window-sorted forms
                self.count["batches >= 2^18"] = self.count.get("batches >= 2^18", 0) + 1
        mode = rng.integers(3)
        if mode == 0:
            return rng.integers(0, n, k).astype(np.uint32)
        if mode == 1:                                     # a narrow range: many duplicates
            lo = int(rng.integers(n))
            return (lo + rng.integers(0, max(1, min(n - lo, k // 2 + 1)), k)).astype(np.uint32)
        return (np.arange(k, dtype=np.uint64) * 7 % n).astype(np.uint32)

    def op_update(self):
        idx = self._idx()
        node = self.rng.integers(0, self.m, idx.size).astype(np.uint32)
        node[self.rng.random(idx.size) < 0.05] = NONE      # Option::None deletes (local.rs:36-37)
        self.g.update_batch(idx, node)
        self.oracle.update_batch(self.ref[:self.n], self.m, idx, node)

    def op_remove(self):
        idx = self._idx()
        self.g.remove_batch(idx)
        self.oracle.remove_batch(self.ref[:self.n], idx)

    def op_lookup(self):
        idx = self._idx()
        got = self.g.lookup_batch(idx)
        assert np.array_equal(got, self.oracle.lookup_batch(self.ref[:self.n], idx)), (self.seed, "lookup", self.log[-6:])

    def op_clean(self):
        rng, m = self.rng, self.m
        if rng.random() < 0.5:
            j = int(rng.integers(m))
            ev = self.g.clean_server(j)
            a = self.ref[:self.n]
            want = int((a == j).sum())
            a[a == j] = NONE
        else:
            dead = sorted(set(int(x) for x in rng.integers(0, m, int(rng.integers(1, 8)))))
            ev = self.g.clean_servers(dead)
            want = self.oracle.clean_servers(self.ref[:self.n], m, dead)
        assert ev == want, (self.seed, "clean", self.log[-6:], ev, want)

    def op_place(self):
        idx = self._idx()
        req = self.rng.integers(0, self.m, idx.size).astype(np.uint32)
        if self.rng.random() < 0.3:
            req[:] = int(self.rng.integers(self.m))
        n = self.n
        used = self.oracle.recompute_used(self.ref[:n], self.load[:n], self.m)
        if self.rng.random() < 0.3:   # the same call over device-resident arrays (validated on the device; sometimes not 16-byte aligned)
            DevBuf = self._devbuf()
            off = int(self.rng.integers(0, 2)) * int(self.rng.integers(1, 4))
            pad = np.zeros(off, np.uint32)
            d_idx, d_req = DevBuf(np.concatenate([pad, idx])), DevBuf(np.concatenate([pad, req]))
            d_node, d_flag = DevBuf(nbytes=4 * (idx.size + off)), DevBuf(nbytes=4 * (idx.size + off))
            self.g.place_pending_dev(idx.size, d_idx.ptr + 4 * off, d_req.ptr + 4 * off, d_node.ptr + 4 * off, d_flag.ptr + 4 * off)
            node, flag = d_node.to_host()[off:], d_flag.to_host()[off:]
            for x in (d_idx, d_req, d_node, d_flag):
                x.free()
            self.count["place_dev"] = self.count.get("place_dev", 0) + 1
        else:
            node, flag = self.g.place_pending(idx, req)
        wnode, wflag = self.oracle.place_pending(self.ref[:n], self.load[:n], self.cap, self.alive, used, idx, req, self.rounds, self.oflags)
        self.fresh_flip = False   # (a request batch delivers a pushed liveness bitmap to the device)
        self._hit("place_pending on a handle whose m is below max_nodes", self.m < self.m0)
        bad = np.flatnonzero((node != wnode) | (flag != wflag))
        assert bad.size == 0, (self.seed, "place_pending", self.log[-6:], idx.size, bad[:8], node[bad[:8]], wnode[bad[:8]], flag[bad[:8]], wflag[bad[:8]])

    def op_mixed(self):
        """rio_gp_mixed_batch: up to 256 entries of each kind, one round trip — against the oracle's four calls in order."""
        rng = self.rng
        def some():
            return self._idx(k=int(_pick(rng, (1, 2, 4, 5, 31, 64, 200, 256), 256)), big_ok=False) if rng.random() < 0.7 else None
        ui, ri, li, pi = some(), some(), some(), some()
        un = pr = None
        if ui is not None:
            un = rng.integers(0, self.m, ui.size).astype(np.uint32)
            un[rng.random(ui.size) < 0.05] = NONE
        if pi is not None:
            pr = rng.integers(0, self.m, pi.size).astype(np.uint32)
        rc, lo, pn, pf = self.g.mixed_batch(update=None if ui is None else (ui, un), remove=ri, lookup=li,
                                            place=None if pi is None else (pi, pr))
        assert rc == [0, 0, 0, 0], (self.seed, "mixed rc", rc)
        self.mixed_wrote = ui is not None or ri is not None or pi is not None   # (lookups alone are a lookup: nothing changes)
        if ui is not None:
            self.oracle.update_batch(self.ref[:self.n], self.m, ui, un)
        if ri is not None:
            self.oracle.remove_batch(self.ref[:self.n], ri)
        if li is not None:
            assert np.array_equal(lo, self.oracle.lookup_batch(self.ref[:self.n], li)), (self.seed, "mixed lookup", self.log[-6:])
        if pi is not None:
            n = self.n
            used = self.oracle.recompute_used(self.ref[:n], self.load[:n], self.m)
            wnode, wflag = self.oracle.place_pending(self.ref[:n], self.load[:n], self.cap, self.alive, used, pi, pr, self.rounds, self.oflags)
            self.fresh_flip = False
            bad = np.flatnonzero((pn != wnode) | (pf != wflag))
            assert bad.size == 0, (self.seed, "mixed place_pending", self.log[-6:], pi.size, bad[:8], pn[bad[:8]], wnode[bad[:8]])

    def op_attrs(self):
        idx = np.unique(self._idx(big_ok=False))
        load = self.rng.integers(0, 500, idx.size).astype(np.uint32)
        aff = self.rng.integers(0, self.m, idx.size).astype(np.uint32)
        aff[self.rng.random(idx.size) < 0.1] = NONE
        self.load[idx] = load
        self.aff[idx] = aff
        self.g.set_object_attrs(idx, load, aff)

    def op_caps(self):
        self.cap = self._caps()
        self.g.set_nodes(self.cap, self.alive, m=self.m)
        self.fresh_flip = False   # (the node table is uploaded whole, liveness included)


    # ---- extended scenarios: the reverse index, the bounded rebalance, the change feed, set_num_objects ---------------------
    def _devbuf(self):
        """The device-buffer class of the binding module the scenario was given (a stand-in brings its own), else tools/hipbuf's."""
        DevBuf = getattr(self.gp, "DevBuf", None)
        if DevBuf is None:
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
            from hipbuf import DevBuf
        return DevBuf

    def _hit(self, key, on=True):
        self.cov[key] = self.cov.get(key, 0) + int(bool(on))

    def _read_only(self, what):
        """After a call that promises to change nothing: an uncommitted solve is still there, byte for byte, and can still be
        committed (sometimes it is, and the model follows)."""
        if self.pending is None:
            return
        try:
            got = self.g.get_solved()
        except self.gp.ObjectPlacementError as e:
            raise AssertionError((self.seed, what, "the uncommitted solve is gone", self.log[-6:], str(e)))
        assert np.array_equal(got, self.pending), (self.seed, what, "the uncommitted solve changed", self.log[-6:],
                                                   np.flatnonzero(got != self.pending)[:8])
        if not self.paging_out and self.rng.random() < 0.3:
            self.g.commit()
            self._set_col(self.pending)
            self.pending = None
            self.check_table(what + " + commit")

    def _dropped(self, what):
        """After a call that changes an input of the solve: the solve that was uncommitted is gone, commit() has nothing to publish."""
        try:
            self.g.commit()
        except self.gp.ObjectPlacementError:
            return
        raise AssertionError((self.seed, what, "an uncommitted solve was still committable after the call", self.log[-6:]))

    def _want_index(self, nodes):
        a, m = self.ref[:self.n], self.m
        sel = np.ones(m, bool)
        if nodes is not None:
            ids = np.asarray(list(nodes), np.int64)
            sel[:] = False
            sel[ids[ids < m]] = True
        if nodes is not None and len(nodes) <= 8:   # the definition, node by node
            parts = [np.flatnonzero(a == j) if sel[j] else np.zeros(0, np.int64) for j in range(m)] if m <= 64 else None
            if parts is not None:
                off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint64)
                return off, np.concatenate(parts).astype(np.uint32)
        keep = np.flatnonzero((a < m) & sel[np.minimum(a, m - 1)])
        rows = keep[np.argsort(a[keep], kind="stable")].astype(np.uint32)
        off = np.zeros(m + 1, np.uint64)
        off[1:] = np.cumsum(np.bincount(a[keep], minlength=m))
        return off, rows

    def op_index(self):
        rng, m, g = self.rng, self.m, self.g
        k = int(rng.integers(5))
        if k == 0:
            nodes = None
        elif k == 1:
            nodes = [int(rng.integers(m))]
        elif k == 2:
            nodes = sorted(set(int(x) for x in rng.integers(0, m, int(rng.integers(2, 9)))))
        elif k == 3:
            nodes = list(range(m))
        else:      # ids >= m among them: ignored
            nodes = sorted(set(int(x) for x in rng.integers(0, m + 70, int(rng.integers(1, 9))))) + [m, m + 64 + int(rng.integers(100))]
        woff, wrows = self._want_index(nodes)
        total = len(wrows)
        form = ("host", "count", "try", "dev")[int(rng.integers(4))]
        tag = (self.seed, "index", form, nodes if nodes is None or len(nodes) < 12 else len(nodes), self.log[-6:])
        self._hit("index while a solve is uncommitted", self.pending is not None)
        if form == "host":
            off, rows = g.rows_on_nodes(nodes)
            assert np.array_equal(off, woff) and np.array_equal(rows, wrows), tag
        elif form == "count":
            assert np.array_equal(g.count_on_nodes(nodes), woff), tag
        elif form == "try":
            short = total > 0           # one entry too small: ERANGE, the buffer untouched, the offsets right
            buf = np.full(total - 1 if short else total, 0xDEADBEEF, np.uint32)
            rc, off, nr = g.rows_on_nodes_try(nodes, buf)
            assert nr == total and np.array_equal(off, woff), tag
            if short:
                assert rc == self.gp.ERANGE and (buf == 0xDEADBEEF).all(), tag + (rc,)
                self._hit("index answered with ERANGE")
            else:
                assert rc == self.gp.OK, tag + (rc,)
        else:
            DevBuf = self._devbuf()
            pad = int(rng.integers(0, 4))
            d_off = DevBuf(np.full(m + 1, 0xDEADBEEFDEADBEEF, np.uint64))
            d_rows = DevBuf(np.full(total + pad + 1, 0xDEADBEEF, np.uint32))
            rc, nr = g.rows_on_nodes_dev(d_off.ptr, d_rows.ptr, total + pad, nodes)
            off, rows = d_off.to_host(np.uint64), d_rows.to_host()
            d_off.free()
            d_rows.free()
            assert rc == self.gp.OK and nr == total and np.array_equal(off, woff), tag + (rc, nr, total)
            assert np.array_equal(rows[:total], wrows) and (rows[total:] == 0xDEADBEEF).all(), tag
        self._read_only("index")

    def _targets(self):
        rng, m, n = self.rng, self.m, self.n
        kind = ("capacities", "balanced", "tight", "zero", "inf")[int(rng.integers(5))]
        if kind == "capacities":
            return kind, None
        if kind == "balanced":
            used = self.oracle.recompute_used(self.ref[:n], self.load[:n], m)
            return kind, self.gp.balanced_targets(self.cap, used, self.alive, int(rng.integers(0, 300)))
        if kind == "tight":    # around the mean load, some nodes unbounded (as tests/rebalance_ref.random_table draws them)
            per = int(self.load[:n].sum()) // max(m, 1)
            T = rng.integers(max(per // 2, 0), per + per // 4 + 2, m).astype(np.uint64)
            T[rng.random(m) < 0.05] = np.uint64(INF)
            return kind, T
        return kind, (np.zeros(m, np.uint64) if kind == "zero" else np.full(m, INF, np.uint64))

    def op_rebalance(self):
        import rebalance_order_ref
        import rebalance_ref
        rng, m, n, g = self.rng, self.m, self.n, self.g
        kind, T = self._targets()
        order = (rebalance_order_ref.ROW_ORDER, rebalance_order_ref.BY_LOAD)[int(rng.random() < (0.7 if self.in_flight else 0.5))]
        # more than 3 072 live nodes hold load (few of the default seeds' tables do, and not for long): mostly by load, and then
        # always under all-zero targets
        wide = m > 3072 and int(np.count_nonzero((self.alive != 0) & (self.oracle.recompute_used(self.ref[:n], self.load[:n], m) > 0))) > 3072
        if wide and rng.random() < 0.8:
            order = rebalance_order_ref.BY_LOAD
        by_load = order == rebalance_order_ref.BY_LOAD
        hist = False
        if by_load and m > 3072 and (wide or rng.random() < 0.5):   # every node that holds load is over: the cut's histograms in global memory
            kind, T, hist = "zero", np.zeros(m, np.uint64), True
        max_moves = (None, 0, 1, max(1, n * int(rng.integers(1, 6)) // 100))[int(rng.integers(4))]
        rounds = int(rng.integers(0, 4))
        form = ("host", "dev", "count", "dev count")[int(rng.integers(4))]
        listing = form in ("host", "dev")
        moves_cap = None
        if listing and rng.random() < 0.3:      # a listing smaller than max_moves: B = min(max_moves, moves_cap)
            moves_cap = int(rng.integers(0, 1 + (max_moves if max_moves is not None else max(n // 50, 1))))
        budget = max_moves
        if listing:
            cap = moves_cap if moves_cap is not None else min(INF if max_moves is None else max_moves, n)
            budget = cap if max_moves is None else min(max_moves, cap)
        # a third of the draws, and every draw that sends the cut to its histograms in global memory: the table of immovable
        # classes is set right before the rebalance, with nothing but the table's own getter in between
        # (and the one rebalance the default seeds put into the middle of a quiet run)
        if rng.random() < 1 / 3 or hist or self.in_mid:
            self.op_movable(inner=True, want_imm=hist or self.in_mid)
        had_solve, dead_unticked = self.pending is not None, self.fresh_flip and not self.alive.all()
        cur, load, aff = self.ref[:n], self.load[:n], self.aff[:n]
        tag = (self.seed, "rebalance", "by load" if by_load else "row order", kind, form, max_moves, moves_cap, rounds, self.log[-6:])
        # rule 13: with an immovable class the result is that of rule 6 on aff', the affinity of every object row of an immovable
        # class read as RIO_GP_AFF_INACTIVE
        tabled = bool((self.I == 0).any())
        imm = self.I[self.K[:n]] == 0
        aff_t = np.where(imm, np.uint32(AFF_INACTIVE), aff) if tabled else aff

        def reference(a):
            if by_load:      # R1': the two-tick composition over the rows in (load, row) order
                return rebalance_order_ref.rebalance(cur, load, a, self.cap, self.alive, T, budget, rounds or self.rounds, order=order)
            return rebalance_ref.rebalance(cur, load, a, self.cap, self.alive, T, budget, rounds or self.rounds)

        nxt, used, wst, wrows, wfrom, wto = reference(aff_t)
        agreed = False
        if tabled and n <= 4096:
            # tests/spec_movable.py, which takes the class column and the table themselves; its R3 walks the nodes once per waiting
            # row, so it is consulted within a bound on that cost only (tests/test_fuzz_driver.py holds the share that is skipped)
            import spec_movable
            cost = int(np.count_nonzero(self.alive)) * wst["selected_rows"] * (rounds or self.rounds)
            self._hit("immovable rebalance of at most 4 096 rows")
            self._hit("immovable rebalance of at most 4 096 rows without the row-by-row restatement", cost > 4_000_000)
            if cost <= 4_000_000:
                s_nxt, s_used, s_st, s_moves = spec_movable.rebalance(
                    [int(x) for x in cur], [int(x) for x in load], [int(x) for x in aff], [int(x) for x in self.K[:n]],
                    [int(x) for x in self.I], [int(x) for x in self.cap], [int(x) for x in self.alive],
                    None if T is None else [int(x) for x in T], budget, rounds or self.rounds, order)
                assert s_st == wst and [int(x) for x in nxt] == s_nxt and [int(x) for x in used] == s_used, tag + ("the two references differ",)
                assert s_moves == [(int(r), int(f), int(t)) for r, f, t in zip(wrows, wfrom, wto)], tag + ("the two references differ",)
                agreed = True
        elif n <= 4096:    # the row-by-row restatement as well
            ints = ([int(x) for x in cur], [int(x) for x in load], [int(x) for x in aff], [int(x) for x in self.cap],
                    [int(x) for x in self.alive], None if T is None else [int(x) for x in T], budget, rounds or self.rounds)
            if by_load:
                import spec_rebalance_order
                s_nxt, s_used, s_st, s_moves = spec_rebalance_order.rebalance(*ints, order=order)
            else:
                import spec_rebalance
                s_nxt, s_used, s_st, s_moves = spec_rebalance.rebalance(*ints)
            assert s_st == wst and [int(x) for x in nxt] == s_nxt and [int(x) for x in used] == s_used, tag + ("the two references differ",)
            assert s_moves == [(int(r), int(f), int(t)) for r, f, t in zip(wrows, wfrom, wto)], tag + ("the two references differ",)
        if form == "host":
            st, rows, frm, to = g.rebalance(T, max_moves, rounds, moves_cap=moves_cap, order=order)
        elif form == "count":
            st, rows, frm, to = g.rebalance(T, max_moves, rounds, list_moves=False, order=order)
        elif form == "dev count":
            st, nm = g.rebalance_dev(target=T, max_moves=max_moves, rounds=rounds, order=order)
            assert nm == len(wrows), tag + (nm, len(wrows))
        else:
            DevBuf = self._devbuf()
            cap = int(cap)
            d = [DevBuf(np.full(cap + 2, 0xDEADBEEF, np.uint32)) for _ in range(3)]
            st, nm = g.rebalance_dev(d[0].ptr, d[1].ptr, d[2].ptr, cap, target=T, max_moves=max_moves, rounds=rounds, order=order)
            rows, frm, to = (x.to_host() for x in d)
            for x in d:
                x.free()
            assert nm == len(wrows), tag + (nm, len(wrows))
            assert all((x[nm:] == 0xDEADBEEF).all() for x in (rows, frm, to)), tag + ("written past the moves",)
            rows, frm, to = rows[:nm], frm[:nm], to[:nm]
        assert st == wst, tag + (st, wst)
        if listing:
            assert np.array_equal(rows, wrows) and np.array_equal(frm, wfrom) and np.array_equal(to, wto), tag + (rows[:8], wrows[:8])
        if listing:          # no listed row is of an immovable class
            assert not imm[rows].any(), tag + ("a row of an immovable class was moved", rows[imm[rows]][:8])
        self.ref[:n] = nxt
        self.pending = None
        if tabled or self.cls_used:
            got = g.get_objects()[1]         # the rule reads the affinity as inactive: the column is not written
            assert np.array_equal(got, aff), tag + ("the rebalance wrote the affinity column", np.flatnonzero(got != aff)[:8])
        self._mv_check(tag)
        if had_solve:
            self._dropped("rebalance")
        if tabled:
            self._hit_movable(cur, load, aff, imm, T, wst, wrows, wto, by_load, had_solve, agreed, reference)
            self.was_imm = self.I == 0      # the classes the last rebalance under a table held in place
        elif self.was_imm.any():
            # the first rebalance since: every class is movable again, and rows of those classes move
            self._hit("plain rebalance after a reset moved rows of a class that had been immovable",
                      bool(self.was_imm[self.K[:n][wrows]].any()))
            self.was_imm = np.zeros(256, bool)
        self._hit("rebalance moved rows", wst["moved_rows"] > 0)
        self._hit("rebalance selected rows that all stayed", wst["selected_rows"] > 0 and wst["moved_rows"] == 0)
        self._hit("rebalance with max_moves 0 and a surplus", budget == 0 and wst["surplus_rows"] > 0)
        self._hit("rebalance with dead nodes right after a flip", dead_unticked)
        self._hit("rebalance under self-assign", self.sa)
        self._hit("rebalance while a solve is uncommitted", had_solve)
        self._hit("rebalance between tick_async and tick_wait", self.in_flight)
        self._hit("rebalance on a handle whose m is below max_nodes", self.m < self.m0)
        if by_load:
            Tn = self.cap if T is None else np.asarray(T, np.uint64)
            over = (self.alive != 0) & (self.oracle.recompute_used(cur, load, m) > Tn)
            on = cur < m
            zero = on & (load == 0) & (aff != AFF_INACTIVE)
            zero[on] &= over[cur[on]]
            self._hit("by-load cut moved rows", wst["moved_rows"] > 0)
            self._hit("by-load cut after a fold made every load equal",
                      self.fold_equal and n > 1 and bool((load == load[0]).all()) and wst["surplus_rows"] > 0)
            self._hit("by-load cut with more than 3 072 over nodes", wst["nodes_over_before"] > 3072)
            self._hit("by-load cut with zero-load candidates on an over node", bool(zero.any()))
            self._hit("by-load cut between tick_async and tick_wait", self.in_flight)
            self._hit("by-load cut on a handle whose m is below max_nodes", self.m < self.m0)

    def _hit_movable(self, cur, load, aff, imm, T, wst, wrows, wto, by_load, had_solve, agreed, reference):
        """The coverage counters of a rebalance under a table that names an immovable class."""
        n, m = self.n, self.m
        Tn = self.cap if T is None else np.asarray(T, np.uint64)
        on = imm & (aff != AFF_INACTIVE) & (cur < m)
        pinned = np.zeros(m, np.uint64)
        np.add.at(pinned, cur[on].astype(np.int64), load[on].astype(np.uint64))
        plain = reference(aff)           # the same call without the table: for this counter only
        n4 = min(-(-n // 4) * 4, self.nmax)
        objects = aff != AFF_INACTIVE
        self._hit("immovable rebalance moved rows", wst["moved_rows"] > 0)
        self._hit("the table changed the moves", not (np.array_equal(plain[3], wrows) and np.array_equal(plain[5], wto)))
        self._hit("immovable rebalance with a node whose pinned load alone exceeds its target",
                  bool(((self.alive != 0) & (pinned > Tn)).any()))
        self._hit("every class immovable with a node over target (surplus 0)",
                  bool(objects.any() and imm[objects].all() and wst["nodes_over_before"] > 0 and wst["surplus_rows"] == 0))
        self._hit("immovable by-load cut moved rows", by_load and wst["moved_rows"] > 0)
        self._hit("immovable by-load cut with more than 3 072 over nodes", by_load and wst["nodes_over_before"] > 3072)
        self._hit("immovable rebalance on more than 65 536 rows", n > 65536)
        self._hit("immovable rebalance on more than 1 024 nodes", m > 1024)
        self._hit("immovable rebalance with n not a multiple of 4 and an immovable class in the quad behind n",
                  n4 > n and bool((self.I[self.K[n:n4]] == 0).any()))
        self._hit("immovable rebalance with hidden placed rows of an immovable class",
                  bool(((self.ref[n:] != NONE) & (self.I[self.K[n:]] == 0)).any()))
        self._hit("immovable rebalance with a table shorter than a class present", n > 0 and int(self.K[:n].max()) >= self.mv_nc)
        self._hit("immovable rebalance on a handle whose m is below max_nodes", m < self.m0)
        self._hit("immovable rebalance while a solve is uncommitted", had_solve)
        self._hit("immovable rebalance between tick_async and tick_wait", self.in_flight)
        self._hit("immovable rebalance in the middle of a quiet run", self.in_mid)
        self._hit("immovable rebalance right behind a setter that changed a placed row's class", self.after == "classes placed")
        self._hit("immovable rebalance right behind a class sweep that listed rows", self.after == "class sweep listed")
        self._hit("immovable rebalance right behind a movable", self.after == "movable")
        self._hit("the row-by-row restatement agreed on an immovable rebalance that moved rows", agreed and wst["moved_rows"] > 0)

    def _feed(self, cap, peek, dev):
        import spec_changes
        g, n = self.g, self.n
        self._hit("paged feed with a writer before the next page", self.page_open and self.page_writer)
        self._hit("feed with hidden rows that differ from the checkpoint", n < self.nmax and (self.ref[n:] != self.B[n:]).any())
        wr, wo, wn, wt, wB = spec_changes.dense(self.B, self.ref, n, cap, peek)
        tag = (self.seed, "changes", cap, peek, dev, n, self.log[-6:])
        if dev:
            DevBuf = self._devbuf()
            c = n + 5 if cap is None else int(cap)
            if c == 0:
                total = g.changes_dev(cap=0, peek=peek)
                rows = old = new = np.zeros(0, np.uint32)
            else:
                size = min(c, n) + 2     # (a listing never holds more than n rows)
                d = [DevBuf(np.full(size, 0xDEADBEEF, np.uint32)) for _ in range(3)]
                total = g.changes_dev(d[0].ptr, d[1].ptr, d[2].ptr, cap=min(c, size - 1), peek=peek)
                rows, old, new = (x.to_host() for x in d)
                for x in d:
                    x.free()
                k = min(total, c)
                assert all((x[k:] == 0xDEADBEEF).all() for x in (rows, old, new)), tag + ("written past the listing",)
                rows, old, new = rows[:k], old[:k], new[:k]
        else:
            rows, old, new, total = g.changes(cap=cap, peek=peek)
        assert total == wt, tag + (total, wt)
        assert np.array_equal(rows, wr) and np.array_equal(old, wo) and np.array_equal(new, wn), tag + (rows[:8], wr[:8])
        self.B = wB
        consuming = not peek and cap != 0
        if consuming:
            assert np.array_equal(self.mirror[rows], old), tag + ("the listing's old nodes are not what the mirror holds",)
            self.mirror[rows] = new
            self.page_open, self.page_writer = len(rows) < total, False
        self._read_only("changes")    # (consuming or not: the feed's checkpoint is no input of a solve)
        return total

    def op_changes(self):
        rng, n = self.rng, self.n
        cap = (None, 0, 1, int(rng.integers(2, 60)), n + 1 + int(rng.integers(1000)))[int(rng.integers(5))]
        peek = bool(rng.random() < 0.3)
        self._feed(cap, peek, bool(rng.random() < 0.3))

    def op_changes_reset(self):
        self.g.changes_reset()
        self.B[:] = NONE
        self.mirror[:] = NONE
        self.page_open = False
        self._hit("feed reset")

    def op_num_objects(self):
        rng = self.rng
        k = rng.random()
        if k < 0.1:
            n = 0
        elif k < 0.45:
            n = self.nmax
        elif k < 0.7:
            n = _pick(rng, _SIZES, self.nmax)
        else:
            n = int(rng.integers(0, self.nmax + 1))
        self._set_n(n)

    def _set_n(self, n):
        grew = n > self.n
        self.g.set_num_objects(n)
        self.n = n
        if grew and self.remapped:     # rows a removal found hidden are back: cleaned and renumbered, in both columns
            tag = (self.seed, "num_objects", "hidden rows after a remap", self.log[-6:])
            got, aff = self.g.get_assign(), self.g.get_objects()[1]
            assert np.array_equal(got, self.ref[:n]), tag + ("assignment", np.flatnonzero(got != self.ref[:n])[:8])
            assert np.array_equal(aff, self.aff[:n]), tag + ("affinity", np.flatnonzero(aff != self.aff[:n])[:8])
        if grew and self.seen_used:    # the stamps of the rows that were hidden: no touch, sweep or remap in between moved them
            self._seen_check((self.seed, "num_objects", "the stamps of rows that were hidden", self.log[-6:]))
        if grew and self.hits_used:    # their hits and loads: no hits call and no fold reaches a hidden row
            self._hits_check((self.seed, "num_objects", "the hits and loads of rows that were hidden", self.log[-6:]), loads=True)
        if self.cls_used:              # K is per row of max_objects: a changing n leaves it alone, going down and coming back
            self._cls_check((self.seed, "num_objects", "the classes of the rows below n", self.log[-6:]))
        self._mv_check((self.seed, "num_objects", self.log[-6:]))      # nor the table of immovable classes

    def _remap_draw(self):
        """A legal map for rio_gp_remap_nodes, at least one node kept: identity | permutation | swap | drop one | drop several
        (stable) | drop several (survivors shuffled) | drop exactly the dead nodes | drop the node most rows are on.  Where the
        count is free, half the time it is chosen so that m_new is the nearest smaller entry of _NODES (about a third of the
        removals): the kernels pick their per-node forms there, and the handle keeps its larger max_nodes."""
        import spec_remap
        rng, m = self.rng, self.m
        ident = np.arange(m, dtype=np.uint32)
        kind = ("identity", "permutation", "swap", "drop one", "drop several", "drop and shuffle", "drop the dead",
                "drop the fullest")[int(rng.integers(8))]
        if kind == "identity" or m == 1:
            return "identity", ident
        if kind == "permutation":
            return kind, rng.permutation(m).astype(np.uint32)
        if kind == "swap":
            a, b = (int(x) for x in rng.choice(m, 2, replace=False))
            ident[[a, b]] = ident[[b, a]]
            return kind, ident
        below = [v for v in _NODES if v < m]
        if kind == "drop one":
            gone = [int(rng.integers(m))]
        elif kind == "drop the dead":
            gone = np.flatnonzero(self.alive == 0)
            if len(gone) == 0:
                return "identity", ident
            gone = gone[:m - 1]
        else:
            if rng.random() < (0.5 if kind != "drop the fullest" else 1 / 3):
                count = m - below[-1]
            else:
                count = int(rng.integers(1, max(2, m // 3 + 1)))
            count = min(count, m - 1)
            first = []
            if kind == "drop the fullest":
                a = self.ref[:self.n]
                first = [int(np.bincount(a[a < m], minlength=m).argmax())]
                count -= 1
            rest = np.setdiff1d(np.arange(m), first)
            gone = first + [int(x) for x in rng.choice(rest, count, replace=False)]
        map = spec_remap.stable_map(m, gone)
        if kind == "drop and shuffle":
            kept = map != NONE
            map[kept] = rng.permutation(int(kept.sum())).astype(np.uint32)
        return kind, map

    def _remap_refused(self):
        """The four kinds of illegal map: RIO_GP_EINVAL, and nothing changed — an uncommitted solve included."""
        import spec_remap
        rng, m = self.rng, self.m
        _, map = self._remap_draw()
        m_new = int((map != NONE).sum())
        kept = np.flatnonzero(map != NONE)
        kind = ("duplicate", "kept value >= m_new", "fewer than m_new kept", "m_new > m")[int(rng.integers(4))]
        if kind == "duplicate" and m_new < 2:
            kind = "m_new > m"
        if kind == "duplicate":
            a, b = (int(x) for x in rng.choice(kept, 2, replace=False))
            map[a] = map[b]
        elif kind == "kept value >= m_new":
            map[int(rng.choice(kept))] = m_new + int(rng.integers(0, 3))
        elif kind == "fewer than m_new kept":
            map[int(rng.choice(kept))] = NONE
        else:
            map, m_new = np.arange(m, dtype=np.uint32), m + 1 + int(rng.integers(0, 3))
        tag = (self.seed, "remap", "refused", kind, m, m_new, self.log[-6:])
        assert not spec_remap.check_map(m, m_new, map), tag
        rc, ev = self.g.remap_nodes_raw(m_new, map)
        assert rc == self.gp.EINVAL and ev == 0, tag + (rc, ev)
        assert self.g.num_nodes == m, tag + (self.g.num_nodes,)
        self.remap_refused = True
        self._hit("remap refused with a solve uncommitted", self.pending is not None)
        self._mv_check(tag)
        self._read_only("remap refused")
        self.check_table("remap refused")

    def op_remap(self, legal=False):
        """rio_gp_remap_nodes against tests/spec_remap.py over every row the model holds (the hidden ones too); the consumer's
        mirror is renumbered by the scenario, as the header asks of whoever holds node ids from before the call."""
        import spec_remap
        self.remap_refused = False
        if not legal and self.rng.random() < (1 / 3 if self.pending is not None else 0.1):   # (about 10 % of all draws)
            return self._remap_refused()
        m, n, g = self.m, self.n, self.g
        kind, map = self._remap_draw()
        m_new = int((map != NONE).sum())
        assert spec_remap.check_map(m, m_new, map), (self.seed, "remap", kind, "the draw is not a legal map")
        had_solve = self.pending is not None
        removed = np.zeros(m + 1, bool)
        removed[:m] = map == NONE
        on_removed = lambda col: removed[np.minimum(col, m)]
        self._hit("remap pure permutation", m_new == m and kind != "identity")
        self._hit("remap while a solve is uncommitted", had_solve)
        self._hit("remap between tick_async and tick_wait", self.in_flight)
        self._hit("remap with a checkpoint naming a removed node", on_removed(self.B).any())
        self._hit("remap with hidden rows on a removed node", on_removed(self.ref[n:]).any())
        self._hit("remap right after a flip", self.fresh_flip)
        self._hit("remap down to a kernel's node-count boundary", m_new < m and m_new in _NODES)
        want = spec_remap.remap(self.ref, self.aff, n, m, map, False, B=self.B, cap=self.cap, alive=self.alive)
        ev = g.remap_nodes(map)
        self.ref, self.aff, self.B, self.cap, self.alive = want["assign"], want["aff"], want["B"], want["cap"], want["alive"]
        self.m = m_new
        self.pending, self.fresh_flip, self.remapped = None, False, True   # (the call writes the liveness bitmap whole)
        known = self.mirror < m                 # the consumer's duty: ids handed out before the call are void
        v = map[self.mirror[known]]
        v[v == NONE] = spec_remap.NODE_GONE
        self.mirror[known] = v
        tag = (self.seed, "remap", kind, m, m_new, self.log[-6:])
        assert ev == want["evicted"], tag + ("evicted", ev, want["evicted"])
        assert g.num_nodes == m_new, tag + ("num_nodes", g.num_nodes)
        cap, alive, _ = g.get_nodes()
        assert np.array_equal(cap, self.cap) and np.array_equal(alive, self.alive), tag + ("the node table did not move with the ids",)
        load, aff = g.get_objects()
        assert np.array_equal(load, self.load[:n]), tag + ("load changed",)
        assert np.array_equal(aff, self.aff[:n]), tag + ("affinity", np.flatnonzero(aff != self.aff[:n])[:8])
        self.check_table("remap")
        if self.seen_used:             # S names no node: it does not move with them
            self._seen_check(tag + ("the last-seen column changed",))
        if self.hits_used:             # nor does H
            self._hits_check(tag + ("the hit column changed",))
        # nor does K (asked every time: on a handle no call of the section has touched, this is its first and returns zeros)
        self._cls_check(tag + ("the class column changed",))
        self._mv_check(tag)            # the table is per class: it names no node
        if had_solve:
            self._dropped("remap")
        self._hit("remap removed nodes that held rows", ev > 0)

    # ---- idle expiry: the touch calls and rio_gp_expire against tests/spec_expire.py ---------------------------------------
    def _seen_check(self, tag):
        got = self.g.get_seen()
        self.seen_used = True
        assert np.array_equal(got, self.S[:self.n]), tag + ("get_seen differs from the model", np.flatnonzero(got != self.S[:self.n])[:8])

    def _epoch(self):
        """The scenario's clock: most epochs rise; some repeat or fall (the calls are maxima); now and then 0 and 0xFFFFFFFF."""
        rng, k = self.rng, self.rng.random()
        if k < 0.06:
            return 0
        if k < 0.10:
            return 0xFFFFFFFF
        if k < 0.30:
            return int(rng.integers(0, self.clock + 1))
        self.clock += int(rng.integers(1, 40))
        return self.clock

    def _beyond_n(self):
        """A row index a call must refuse: n, n + 1, max_objects, NONE."""
        n = self.n
        return int((n, n + 1, max(self.nmax, n), NONE)[int(self.rng.integers(4))])

    def _dev_offset(self, arr):
        """arr on the device, sometimes behind 1 .. 3 words of padding so that it is not 16-byte aligned -> (buffer, address)."""
        off = int(self.rng.integers(0, 2)) * int(self.rng.integers(1, 4))
        d = self._devbuf()(np.concatenate([np.zeros(off, np.uint32), np.asarray(arr, np.uint32)]))
        return d, d.ptr + 4 * off

    def _refused(self, call, tag):
        try:
            call()
        except self.gp.ObjectPlacementError as e:
            assert e.rc == self.gp.EINVAL, tag + ("refused with", e.rc)
            return
        raise AssertionError(tag + ("the call was not refused",))

    def op_touch(self):
        import spec_expire
        rng, n, g = self.rng, self.n, self.g
        form = ("host", "host refused", "dev", "dev invalid", "all", "merge", "merge dev", "merge refused")[int(rng.integers(8))]
        epoch = self._epoch()
        tag = (self.seed, "touch", form, epoch, n, self.log[-6:])
        self._hit("touch while a solve is uncommitted", self.pending is not None)
        self._hit("touch with hidden rows", n < self.nmax)
        self._hit("touch between tick_async and tick_wait", self.in_flight)
        idx = self._idx(big_ok=False) if n else np.zeros(0, np.uint32)
        bufs = []
        if form == "host":
            g.touch(idx, epoch)
            self.S = spec_expire.touch(self.S, idx, epoch)
        elif form == "host refused":          # validated first: one index >= n, nothing changes
            bad = np.append(idx, np.uint32(0))
            bad[int(rng.integers(bad.size))] = self._beyond_n()
            rc = g.touch_raw(bad, epoch)
            assert rc == self.gp.EINVAL, tag + (rc,)
        elif form == "dev":
            d, ptr = self._dev_offset(idx)
            bufs.append(d)
            g.touch_dev(ptr, idx.size, epoch)
            self.S = spec_expire.touch(self.S, idx, epoch)
        elif form == "dev invalid":           # the valid entries are applied, the call reports RIO_GP_EINVAL
            bad = np.append(idx, np.uint32(0))
            for k in rng.integers(0, bad.size, int(rng.integers(1, 5))):
                bad[int(k)] = self._beyond_n()
            d, ptr = self._dev_offset(bad)
            bufs.append(d)
            self._refused(lambda: g.touch_dev(ptr, bad.size, epoch), tag)
            self.S = spec_expire.touch(self.S, bad[bad < n], epoch)
            self._hit("touch_dev skipped invalid entries")
        elif form == "all":
            g.touch_all(epoch)
            self.S = spec_expire.touch_all(self.S, n, epoch)
        elif form == "merge refused":         # rows = n + 1
            stamps = np.full(n + 1, epoch, np.uint32)
            if rng.random() < 0.5:
                self._refused(lambda: g.touch_merge(stamps), tag)
            else:
                d, ptr = self._dev_offset(stamps)
                bufs.append(d)
                self._refused(lambda: g.touch_merge_dev(ptr, n + 1), tag)
        else:
            rows = (0, n, _pick(rng, _SIZES, n) if n else 0, int(rng.integers(0, n + 1)))[int(rng.integers(4))]
            # per row: 0 | below | equal to | above what S holds | 0xFFFFFFFF (rare: it ends the row's part in every later sweep)
            have = self.S[:rows].astype(np.int64)
            kind = rng.choice(5, rows, p=[0.15, 0.25, 0.2, 0.38, 0.02])
            step = rng.integers(1, 40, rows)
            stamps = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [0, have - step, have, have + step], 0xFFFFFFFF)
            stamps = np.clip(stamps, 0, 0xFFFFFFFF).astype(np.uint32)
            if rows and epoch in (0, 0xFFFFFFFF):
                stamps[int(rng.integers(rows))] = epoch
            if form == "merge":
                g.touch_merge(stamps)
            else:
                d, ptr = self._dev_offset(stamps)
                bufs.append(d)
                g.touch_merge_dev(ptr, rows)
            self.S = spec_expire.touch_merge(self.S, stamps)
        self._seen_check(tag)      # (it waits: rio_gp_touch_all and rio_gp_touch_merge_dev do not, and their buffer is freed below)
        for d in bufs:
            d.free()
        self._read_only("touch")
        self.check_table("touch")

    def _expire_cap(self, idle, n_idle):
        """None | 0 | 1 | a small number | n_idle - 1, n_idle, n_idle + 1 | a cap that ends the listing inside a tile of 1 024 rows
        that holds more idle rows."""
        rng = self.rng
        k = int(rng.integers(8))
        if k < 4:
            return (None, 0, 1, int(rng.integers(2, 60)))[k]
        if k < 7:
            return max(n_idle + k - 5, 0)
        _, first, count = np.unique(idle // 1024, return_index=True, return_counts=True)
        many = np.flatnonzero(count >= 2)
        if len(many) == 0:
            return max(n_idle - 1, 0)
        t = int(many[rng.integers(len(many))])
        return int(first[t]) + int(rng.integers(1, count[t]))

    def op_expire(self, hit=None):
        """rio_gp_expire[_dev] against spec_expire.expire over the model's column, stamps and loads.  hit: None — cutoff, cap and
        form are drawn; True — a listing that un-places at least one row when any placed row can be idle; False — a count-only
        call or cutoff 0.  -> rows un-placed."""
        import spec_expire
        rng, n, g = self.rng, self.n, self.g
        S, A = self.S, self.ref
        placed = np.flatnonzero(A[:n] != NONE)
        first, had_solve = not self.seen_used, self.pending is not None
        form = ("host", "dev", "host", "dev", "count", "dev count")[int(rng.integers(6))]
        if hit is None and had_solve and rng.random() < 0.5:
            hit = True                 # (a sweep that must drop the solve, not one of the many that list nothing)
        if hit is True:
            form = form if form in ("host", "dev") else ("host", "dev")[int(rng.integers(2))]
            lo = int(S[placed].min()) if len(placed) else 0
            cutoff = (min(lo + 1, 0xFFFFFFFF), min(int(S[placed].max()) + 1 if len(placed) else 1, 0xFFFFFFFF), 0xFFFFFFFF)[int(rng.integers(3))]
        elif hit is False and rng.random() < 0.5:
            cutoff = 0
        else:
            k = int(rng.integers(4))
            if k == 0:
                cutoff = 0
            elif k == 1:      # a placed row's own stamp: the strict < decides that row
                cutoff = int(S[placed[rng.integers(len(placed))]]) if len(placed) else int(S[:n].max()) if n else 0
            elif k == 2:
                cutoff = min(int(S[:n].max()) + 1 if n else 1, 0xFFFFFFFF)
            else:
                cutoff = 0xFFFFFFFF
        if hit is False and cutoff != 0:
            form = form if form in ("count", "dev count") else ("count", "dev count")[int(rng.integers(2))]
        listing = form in ("host", "dev")
        idle, _, n_idle, _, _ = spec_expire.expire(A, S, self.load, n, cutoff, None)
        cap = self._expire_cap(idle, n_idle) if listing else None
        if hit is True and cap == 0:
            cap = 1
        want_cap = cap if listing else 0
        wrows, wnodes, w_idle, wfreed, A2 = spec_expire.expire(A, S, self.load, n, cutoff, want_cap)
        L = len(wrows)
        tag = (self.seed, "expire", form, cutoff, cap, n, self.log[-6:])
        self._hit("expire un-placed rows", L > 0)
        self._hit("expire capped below n_idle", 0 < L < n_idle)
        self._hit("expire with a placed row stamped exactly at the cutoff", cutoff > 0 and bool((S[placed] == cutoff).any()))
        self._hit("expire as the first call of the family", first)
        self._hit("expire listed rows while a solve was uncommitted", had_solve and L > 0)
        self._hit("expire hit nothing while a solve was uncommitted", had_solve and L == 0)
        self._hit("expire between tick_async and tick_wait", self.in_flight)
        self._hit("expire with hidden placed rows older than the cutoff", bool(((A[n:] != NONE) & (S[n:] < cutoff)).any()))
        self._hit("expire at n == 0", n == 0)
        self._hit("expire on a handle whose m is below max_nodes", self.m < self.m0)
        self._hit("expire between two pages of the feed", self.page_open)
        self.seen_used = True
        if form == "count":
            rows, nodes, got_idle, freed = g.expire(cutoff, count_only=True)
        elif form == "dev count":
            got_idle, freed = g.expire_dev(cutoff)
            rows = nodes = np.zeros(0, np.uint32)
        elif form == "host" and (cap is None or rng.random() < 0.5):
            rows, nodes, got_idle, freed = g.expire(cutoff, cap)
        elif form == "host":   # the call as given, into sentinel-filled arrays of cap + 2, without load_freed
            out = [np.full(cap + 2, 0xDEADBEEF, np.uint32) for _ in range(2)]
            rc, got_idle = g.expire_raw(cutoff, out[0], out[1], cap)
            assert rc == self.gp.OK, tag + (rc,)
            assert all((x[L:] == 0xDEADBEEF).all() for x in out), tag + ("written past the listing",)
            rows, nodes, freed = out[0][:L], out[1][:L], wfreed
        else:
            c = n if cap is None else int(cap)
            d = [self._devbuf()(np.full(c + 2, 0xDEADBEEF, np.uint32)) for _ in range(2)]
            got_idle, freed = g.expire_dev(cutoff, d[0].ptr, d[1].ptr, c)
            rows, nodes = (x.to_host() for x in d)
            for x in d:
                x.free()
            assert all((x[L:] == 0xDEADBEEF).all() for x in (rows, nodes)), tag + ("written past the listing",)
            rows, nodes = rows[:L], nodes[:L]
        assert got_idle == w_idle == n_idle, tag + ("n_idle", got_idle, w_idle)
        assert np.array_equal(rows, wrows) and np.array_equal(nodes, wnodes), tag + (rows[:8], wrows[:8], nodes[:8], wnodes[:8])
        assert freed == wfreed, tag + ("load_freed", freed, wfreed)
        self.ref = A2
        self.expire_listed = L > 0
        self._seen_check(tag)          # a sweep reads S and never writes it
        if self.hits_used:             # and H is no business of its
            self._hits_check(tag)
        if self.cls_used:              # nor is K
            self._cls_check(tag)
        if L > 0:
            self.mark = "expire listed"
            self.pending = None
            if had_solve:
                self._dropped("expire")
        else:
            self._read_only("expire")
        self.check_table("expire")
        return L

    # ---- measured load and the hot-object report: tests/spec_loads.py and tests/spec_top.py --------------------------------
    def _hits_check(self, tag, loads=False):
        got = self.g.get_hits()
        self.hits_used = True
        assert np.array_equal(got, self.H[:self.n]), tag + ("get_hits differs from the model", np.flatnonzero(got != self.H[:self.n])[:8])
        if loads:
            got = self.g.get_objects()[0]
            assert np.array_equal(got, self.load[:self.n]), tag + ("load differs from the model", np.flatnonzero(got != self.load[:self.n])[:8])

    def _hit_values(self, rows, at):
        """Weights or counts for the rows `rows` (distinct, or every other entry of a repeated row carries 0): mostly small, some
        0; in about one call in ten up to four of them are what fills the row's counter exactly (0xFFFFFFFF - H), misses by one,
        overshoots by one, and plain 0xFFFFFFFF.  at: the entries that may carry one.  -> (values, one filled its row exactly)"""
        rng = self.rng
        w = rng.integers(0, 6, len(rows)).astype(np.uint32)
        if rng.random() < 0.3:
            w[rng.random(len(rows)) < 0.2] = rng.integers(0, 100000)
        exact = False
        if len(at) and rng.random() < 0.12:
            at = rng.permutation(at)[:4]
            for j, k in enumerate(at):
                room = 0xFFFFFFFF - int(self.H[rows[k]])
                w[k] = (room, max(room - 1, 0), min(room + 1, 0xFFFFFFFF), 0xFFFFFFFF)[j]
            exact = True
        return w, exact

    def op_hits(self):
        """One call of the hits family against spec_loads.hits_add / hits_merge; rio_gp_get_hits must equal H[:n] after each, an
        uncommitted solve still there."""
        import spec_loads
        rng, n, g = self.rng, self.n, self.g
        form = ("host", "host weights", "host refused", "dev", "dev invalid", "merge", "merge dev", "merge refused")[int(rng.integers(8))]
        tag = (self.seed, "hits", form, n, self.log[-6:])
        self._hit("hits while a solve is uncommitted", self.pending is not None)
        self._hit("hits with hidden rows holding hits", bool(self.H[n:].any()))
        self._hit("hits between tick_async and tick_wait", self.in_flight)
        bufs, exact = [], False

        def batch(idx):
            """weights for a batch (None: 1 each); the entries of a row that gets a filling weight are its only ones that count"""
            if form == "host" or (form != "host weights" and rng.random() < 0.4):
                return None, False
            _, first = np.unique(idx, return_index=True)
            w, ex = self._hit_values(idx, first)
            if ex:
                again = np.ones(len(idx), bool)
                again[first] = False
                w[again] = 0
            return w, ex

        if form in ("host", "host weights", "dev"):
            idx = self._idx(big_ok=False) if n else np.zeros(0, np.uint32)
            w, exact = batch(idx)
            if form == "dev":
                d, ptr = self._dev_offset(idx)
                dw, wptr = self._dev_offset(w) if w is not None else (None, None)
                bufs += [d] + ([dw] if dw is not None else [])
                g.hits_add_dev(ptr, idx.size, wptr)
            else:
                g.hits_add(idx, w)
            self.H = spec_loads.hits_add(self.H, idx, w)
        elif form == "host refused":          # validated first: one index >= n, nothing changes
            bad = np.append(self._idx(big_ok=False) if n else np.zeros(0, np.uint32), np.uint32(0))
            bad[int(rng.integers(bad.size))] = self._beyond_n()
            rc = g.hits_add_raw(bad, weight=None if rng.random() < 0.5 else np.ones(bad.size, np.uint32))
            assert rc == self.gp.EINVAL, tag + (rc,)
        elif form == "dev invalid":           # the valid entries are applied, the call reports RIO_GP_EINVAL
            bad = np.append(self._idx(big_ok=False) if n else np.zeros(0, np.uint32), np.uint32(0))
            for k in rng.integers(0, bad.size, int(rng.integers(1, 5))):
                bad[int(k)] = self._beyond_n()
            ok = bad < n
            w, exact = batch(np.where(ok, bad, 0).astype(np.uint32))
            exact = False                     # (a filling weight may sit on an invalid entry)
            d, ptr = self._dev_offset(bad)
            dw, wptr = self._dev_offset(w) if w is not None else (None, None)
            bufs += [d] + ([dw] if dw is not None else [])
            self._refused(lambda: g.hits_add_dev(ptr, bad.size, wptr), tag)
            self.H = spec_loads.hits_add(self.H, bad[ok], None if w is None else w[ok])
            self._hit("hits_dev skipped invalid entries")
        elif form == "merge refused":         # rows = n + 1
            counts = np.ones(n + 1, np.uint32)
            if rng.random() < 0.5:
                self._refused(lambda: g.hits_merge(counts), tag)
            else:
                d, ptr = self._dev_offset(counts)
                bufs.append(d)
                self._refused(lambda: g.hits_merge_dev(ptr, n + 1), tag)
        else:
            rows = (0, n, n, _pick(rng, _SIZES, n) if n else 0, int(rng.integers(0, n + 1)))[int(rng.integers(5))]
            counts, exact = self._hit_values(np.arange(rows), np.arange(rows))
            self._hit("hits merge of rows not a multiple of 4", rows % 4 != 0)
            if form == "merge":
                g.hits_merge(counts)
            else:
                d, ptr = self._dev_offset(counts)
                bufs.append(d)
                self._hit("hits merge from an unaligned device array", ptr != d.ptr)
                g.hits_merge_dev(ptr, rows)
            self.H = spec_loads.hits_merge(self.H, counts)
        self._hit("hits saturated exactly at 0xFFFFFFFF", exact)
        self._hits_check(tag)      # (it waits: rio_gp_hits_merge_dev does not, and its buffer is freed below)
        for d in bufs:
            d.free()
        self.mark = "hits"
        self._read_only("hits")
        self.check_table("hits")

    def _fold_draw(self):
        """(kind, keep, gain, min_load, max_load) of a legal fold."""
        rng = self.rng
        kind = ("identity", "replace", "decay", "one value", "small max", "large gain")[int(rng.integers(6))]
        small = int(rng.integers(0, 4))
        if kind == "identity":
            return kind, 65536, 0, 0, 0xFFFFFFFF
        if kind == "replace":
            lo = int(rng.integers(0, 3))
            return kind, 0, int(rng.integers(0, 50)), lo, (0xFFFFFFFF, lo + int(rng.integers(0, 1000)))[int(rng.integers(2))]
        if kind == "decay":
            return kind, (32768, 1, 65535)[int(rng.integers(3))], small, 0, 0xFFFFFFFF
        if kind == "one value":
            v = (0, 1, 255, 256, 65535, 65536, 1 << 24, 0xFFFFFFFF)[int(rng.integers(8))]
            return kind, (0, 32768, 65536)[int(rng.integers(3))], small, v, v
        if kind == "small max":
            return kind, (32768, 65536)[int(rng.integers(2))], small, 0, int(rng.integers(0, 8))
        return kind, (0, 32768, 65536)[int(rng.integers(3))], int(rng.integers(1 << 16, 1 << 32)), 0, 0xFFFFFFFF

    def op_fold(self, legal=False):
        """rio_gp_load_fold against spec_loads.load_fold over the model's loads and hits: the five statistics, the loads, H zero on
        [:n], `used` of the new loads; every legal fold drops an uncommitted solve, a refused one changes nothing."""
        import spec_loads
        rng, n, g = self.rng, self.n, self.g
        kind, keep, gain, lo, hi = self._fold_draw()
        had_solve = self.pending is not None
        self.fold_refused = not legal and rng.random() < (0.4 if had_solve else 0.1)
        if self.fold_refused:
            if rng.random() < 0.5 or hi == 0:
                keep = 65537 + int(rng.integers(0, 2)) * int(rng.integers(0, 1 << 20))
            else:
                lo, hi = hi, int(rng.integers(0, hi))
            tag = (self.seed, "fold", "refused", keep, gain, lo, hi, n, self.log[-6:])
            rc = g.load_fold_raw(keep, gain, lo, hi)
            assert rc == self.gp.EINVAL, tag + (rc,)
            self._hit("fold refused with a solve uncommitted", had_solve)
            self._hits_check(tag, loads=True)
            self._read_only("fold refused")
            self.check_table("fold refused")
            return
        fresh_n = False
        behind_hits = self.after == "hits"      # (run() sends a fold right behind a hits call now and then: H is not all zero)
        if not legal and not self.in_flight and not had_solve and (rng.random() < 0.25 or behind_hits):
            # rio_gp_set_num_objects right before it, and nothing in between: `used` is not valid when the fold picks its form
            # (after an operation of its own the scenario's check_table has made it valid again)
            n = (self.nmax, _pick(rng, _SIZES, self.nmax), int(rng.integers(0, self.nmax + 1)), -1)[int(rng.integers(4))]
            if n < 0 or behind_hits:      # a row that holds hits and is not the first of its quad becomes the first hidden one
                held = np.flatnonzero(self.H)
                held = held[held % 4 != 0]
                n = int(held[rng.integers(len(held))]) if len(held) else self.nmax
            fresh_n = n != self.n
            self._set_n(n)
            self.page_writer = self.page_writer or fresh_n
        tag = (self.seed, "fold", kind, keep, gain, lo, hi, n, fresh_n, self.log[-6:])
        self._hit("fold with used not valid", fresh_n)
        self._hit("fold on more than 4 096 nodes", self.m > 4096)
        self._hit("fold on a handle whose m is below max_nodes", self.m < self.m0)
        self._hit("fold with n not a multiple of 4 and hits in the quad behind n", n % 4 != 0 and bool(self.H[n:(n | 3) + 1].any()))
        self._hit("fold while a solve is uncommitted", had_solve)
        self._hit("fold between tick_async and tick_wait", self.in_flight)
        self.load, self.H, want = spec_loads.load_fold(self.load, self.H, n, keep, gain, lo, hi)
        st = g.load_fold(keep, gain, lo, hi)
        self.pending = None
        self.fold_equal = n > 1 and bool((self.load[:n] == self.load[0]).all())
        self._hit("fold changed no load", want["rows_changed"] == 0)
        self._hit("fold clamped every load to one value", self.fold_equal)
        assert st == want, tag + ("statistics", st, want)
        self.mark = "fold"         # (run() sends a census right behind now and then: it sums the loads the fold has just written)
        self._hits_check(tag, loads=True)     # (H is zero on [:n], the loads are the model's)
        self.check_table("fold")              # (`used` is that of the new loads)
        if had_solve:
            self._dropped("fold")

    def _top_cap(self, keys_all, rows_all):
        """0 (count only) | 1 | a small number | n_cand - 1, n_cand, n_cand + 1 | 4 096 | a cap that cuts inside a group of equal
        keys whose rows lie in more than one tile of 1 024 rows -> (cap, it is such a cut)"""
        import spec_top
        rng, nc = self.rng, len(rows_all)
        k = int(rng.integers(9))
        if k < 7:
            return min(max((0, 1, int(rng.integers(2, 60)), nc - 1, nc, nc + 1, spec_top.TOP_MAX)[k], 0), spec_top.TOP_MAX), False
        start = np.flatnonzero(np.concatenate([[True], keys_all[1:] != keys_all[:-1]])) if nc else np.zeros(0, np.int64)
        end = np.append(start[1:], nc)
        ok = np.flatnonzero((start + 1 <= np.minimum(end - 1, spec_top.TOP_MAX)) &
                            (rows_all[start] // 1024 != rows_all[np.maximum(end - 1, 0)] // 1024)) if nc else start
        if len(ok) == 0:
            return spec_top.TOP_MAX, False
        t = int(ok[rng.integers(len(ok))])
        return int(rng.integers(start[t] + 1, min(end[t] - 1, spec_top.TOP_MAX) + 1)), True

    def op_top(self):
        """rio_gp_top_rows[_dev] against spec_top.top_rows over the model's column, loads and hits (none before the first call
        of the hits section): rows, keys, nodes, n_candidates and key_sum exact, nothing written behind the listing, nothing
        changed."""
        import spec_top
        rng, n, m, g = self.rng, self.n, self.m, self.g
        flags = int(rng.integers(8))
        H = self.H if self.hits_used else None
        K = (self.H if flags & spec_top.BY_HITS else self.load)[:n]
        A = self.ref[:n]
        on = A[A < m]
        count = np.bincount(on, minlength=m)
        k = int(rng.integers(4))
        if k == 0:
            node = int(rng.integers(m))
        elif k == 1:      # the node most rows are on
            node = int(count.argmax())
        elif k == 2:      # one that holds no row, if there is one
            empty = np.flatnonzero(count == 0)
            node = int(empty[rng.integers(len(empty))]) if len(empty) else int(rng.integers(m))
        else:             # no node: refused under ON_NODE, ignored without it
            node = int((m, m + 1, self.m0, NONE)[int(rng.integers(4))])
        k = int(rng.choice(5, p=[0.4, 0.3, 0.1, 0.1, 0.1]))
        top = int(K.max()) if n else 0
        min_key = (0, int(K[rng.integers(n)]) if n else 0, top, min(top + 1, 0xFFFFFFFF), 0xFFFFFFFF)[k]
        form = ("host", "host no node", "raw", "dev", "count", "dev count")[int(rng.integers(6))]
        bad = (None, None, None, None, None, None, "cap", "flag")[int(rng.integers(8))]
        if flags & spec_top.ON_NODE and node >= m:
            bad = "node"
        rows_all, keys_all, _, n_cand, _ = spec_top.top_rows(self.ref, self.load, H, n, flags, node, min_key, n)
        cap, in_tie = self._top_cap(keys_all, rows_all)
        if form in ("count", "dev count"):
            cap = 0
        wrows, wkeys, wnodes, wn, wsum = spec_top.top_rows(self.ref, self.load, H, n, flags, node, min_key, cap)
        L = len(wrows)
        assert wn == n_cand and L == min(n_cand, cap)
        tag = (self.seed, "top", form, flags, node, min_key, cap, n, bad, self.log[-6:])
        if bad is not None:      # cap above RIO_GP_TOP_MAX | an unknown flag bit | ON_NODE with a node >= m: refused
            bflags = flags | (8, 16, 1 << 31)[int(rng.integers(3))] if bad == "flag" else flags
            bcap = spec_top.TOP_MAX + 1 + int(rng.integers(0, 2)) * int(rng.integers(0, 5000)) if bad == "cap" else max(cap, 1)
            if form in ("dev", "dev count"):
                d = [self._devbuf()(np.full(bcap + 2, 0xDEADBEEF, np.uint32)) for _ in range(3)]
                self._refused(lambda: g.top_rows_dev(bflags, node, min_key, d[0].ptr, d[1].ptr, d[2].ptr, bcap), tag)
                for x in d:
                    x.free()
            else:
                out = [np.full(bcap + 2, 0xDEADBEEF, np.uint32) for _ in range(3)]
                rc, _ = g.top_rows_raw(bflags, node, min_key, out[0], out[1], out[2], bcap)
                assert rc == self.gp.EINVAL, tag + (rc,)
            self._read_only("top refused")
            self.check_table("top refused")
            return
        self._hit("top by hits before any hits call", bool(flags & spec_top.BY_HITS) and not self.hits_used)
        self._hit("top cut inside a tie group spanning tiles", in_tie and cap > 0)
        self._hit("top listed all 4 096", L == spec_top.TOP_MAX)
        self._hit("top with cap above n_candidates", cap > n_cand)
        self._hit("top between two pages of the feed", self.page_open)
        self._hit("top right after an expire that listed rows", self.after == "expire listed")
        self._hit("top right after a class sweep that listed rows", self.after == "class sweep listed")
        self.mark = "top"          # (the class sweep shares the report's scratch as well: run() sends one right behind)
        self._hit("top while a solve is uncommitted", self.pending is not None)
        self._hit("top between tick_async and tick_wait", self.in_flight)
        self._hit("top on a handle whose m is below max_nodes", self.m < self.m0)
        self._hit("top at n == 0", n == 0)
        by_hits, placed = bool(flags & spec_top.BY_HITS), bool(flags & spec_top.PLACED)
        on_node = node if flags & spec_top.ON_NODE else None
        nodes = key_sum = None
        if form in ("host", "count"):
            rows, keys, nodes, got_n, key_sum = g.top_rows(cap, by_hits, placed, on_node, min_key)
        elif form == "host no node":
            rows, keys, none, got_n, key_sum = g.top_rows(cap, by_hits, placed, on_node, min_key, want_node=False)
            assert none is None, tag
        elif form == "raw" and cap == 0:
            rc, got_n = g.top_rows_raw(flags, node, min_key)
            assert rc == self.gp.OK, tag + (rc,)
            rows = keys = nodes = np.zeros(0, np.uint32)
        elif form == "raw":       # the call as given, into sentinel-filled arrays of cap + 2, without key_sum
            out = [np.full(cap + 2, 0xDEADBEEF, np.uint32) for _ in range(3)]
            rc, got_n = g.top_rows_raw(flags, node, min_key, out[0], out[1], out[2], cap)
            assert rc == self.gp.OK, tag + (rc,)
            assert all((x[L:] == 0xDEADBEEF).all() for x in out), tag + ("written past the listing",)
            rows, keys, nodes = (x[:L] for x in out)
        elif cap == 0:
            got_n, key_sum = g.top_rows_dev(flags, node, min_key, None, None, None, 0)
            rows = keys = nodes = np.zeros(0, np.uint32)
        else:
            with_node = bool(rng.random() < 0.7)
            d = [self._devbuf()(np.full(cap + 2, 0xDEADBEEF, np.uint32)) for _ in range(3)]
            got_n, key_sum = g.top_rows_dev(flags, node, min_key, d[0].ptr, d[1].ptr, d[2].ptr if with_node else None, cap)
            out = [x.to_host() for x in d]
            for x in d:
                x.free()
            assert all((x[L:] == 0xDEADBEEF).all() for x in out), tag + ("written past the listing",)
            assert with_node or (out[2] == 0xDEADBEEF).all(), tag + ("a node array that was not given was written",)
            rows, keys, nodes = out[0][:L], out[1][:L], (out[2][:L] if with_node else None)
        assert got_n == wn, tag + ("n_candidates", got_n, wn)
        assert np.array_equal(rows, wrows) and np.array_equal(keys, wkeys), tag + (rows[:8], wrows[:8], keys[:8], wkeys[:8])
        assert nodes is None or np.array_equal(nodes, wnodes), tag + ("nodes", nodes[:8], wnodes[:8])
        assert key_sum is None or key_sum == wsum, tag + ("key_sum", key_sum, wsum)
        if self.hits_used:
            self._hits_check(tag)
        self._read_only("top")
        self.check_table("top")

    # ---- object classes: the setters, rio_gp_expire_classes and rio_gp_census against tests/spec_classes.py ---------------------
    def _cls_check(self, tag):
        got = self.g.get_classes()
        if not self.cls_used and not self.K.any():      # no setter has run: this call, or the one before, allocated K, all 0
            assert not got.any(), tag + ("the class column of an untouched handle is not zero", np.flatnonzero(got)[:8])
        self.cls_used = True
        assert np.array_equal(got, self.K[:self.n]), tag + ("get_classes differs from the model", np.flatnonzero(got != self.K[:self.n])[:8])

    def _cls_values(self, rows):
        """One class per entry of `rows` (the row each value goes to): all one class | a few small classes | uniform over
        0 .. 255 | small ones, 255 and values beyond the n_classes later calls pass | four different classes in every quad of rows."""
        rng, k = self.rng, len(rows)
        kind = int(rng.integers(5))
        if kind == 0:
            return np.full(k, int(rng.integers(256)), np.uint8)
        if kind == 1:
            return rng.integers(0, 4, k).astype(np.uint8)
        if kind == 2:
            return rng.integers(0, 256, k).astype(np.uint8)
        if kind == 3:
            return rng.choice(np.array([0, 1, 2, 3, 7, 8, 15, 16, 17, 63, 64, 200, 254, 255], np.uint8), k)
        base = rng.choice(256, 4, replace=False).astype(np.uint8)
        return base[np.asarray(rows, np.int64) % 4]

    def _row_edge(self):
        """Where a range starts or ends: 0 | n | a boundary size | any row — half the time up to 3 rows beside it, so that every
        residue mod 4 occurs at each of them."""
        rng, n = self.rng, self.n
        v = (0, n, _pick(rng, _SIZES, n) if n else 0, int(rng.integers(0, n + 1)))[int(rng.integers(4))]
        if rng.random() < 0.5:
            v += int(rng.integers(-3, 4))
        return min(max(v, 0), n)

    def op_classes(self):
        """One call of the setter family against spec_classes.set_classes / set_class_batch; rio_gp_get_classes must equal K[:n]
        after each, `used` and an uncommitted solve as they were.  About one batch in four is followed at once by an update batch
        over some of its rows: the election borrows rio_gp_update_batch's position scratch and has to hand it back all ones."""
        import spec_classes
        rng, n, g = self.rng, self.n, self.g
        form = ("range", "range", "range dev", "range refused", "batch", "batch", "batch refused", "batch dev", "batch dev",
                "batch empty")[int(rng.integers(10))]
        tag = (self.seed, "classes", form, n, self.log[-6:])
        had_solve = self.pending is not None
        self._hit("classes with hidden rows holding classes", bool(self.K[n:].any()))
        self._hit("classes while a solve is uncommitted", had_solve)
        self._hit("classes between tick_async and tick_wait", self.in_flight)
        bufs, unaligned, dup, skipped, updated = [], False, False, False, False
        K0, on0 = self.K, self.ref[:n] != NONE      # (the model functions return a new column)
        if form in ("range", "range dev"):
            a, b = sorted((self._row_edge(), self._row_edge()))
            cls = self._cls_values(np.arange(a, b))
            off = int(rng.integers(0, 4))            # the source 0 .. 3 bytes into its buffer
            src = np.zeros(b - a + 3, np.uint8)
            src[off:off + b - a] = cls
            unaligned = a % 4 != 0 and b % 4 != 0 and b > a
            if form == "range":
                rc = g.set_classes_raw(a, src[off:off + b - a])
                assert rc == self.gp.OK, tag + (a, b, rc)
            else:
                d = self._devbuf()(src)
                bufs.append(d)
                g.set_classes_dev(a, d.ptr + off, b - a)
            self.K = spec_classes.set_classes(self.K, a, cls)
        elif form == "range refused":         # first_row + rows = n + 1: nothing changes
            a = int(rng.integers(0, n + 1))
            cls = np.full(n + 1 - a, 1 + int(rng.integers(255)), np.uint8)
            if rng.random() < 0.5:
                rc = g.set_classes_raw(a, cls)
                assert rc == self.gp.EINVAL, tag + (a, rc)
            else:
                d = self._devbuf()(cls)
                bufs.append(d)
                self._refused(lambda: g.set_classes_dev(a, d.ptr, len(cls)), tag)
        elif form == "batch empty":
            if rng.random() < 0.5:
                rc = g.set_class_batch_raw(np.zeros(0, np.uint32), np.zeros(0, np.uint8))
            else:
                rc = g.set_class_batch_dev_raw(None, None, 0)
            assert rc == self.gp.OK, tag + (rc,)
        else:
            idx = self._idx(big_ok=False) if n else np.zeros(0, np.uint32)
            if idx.size > 1 and rng.random() < 0.5:      # the second half names the rows of the first again, with classes of its own
                h = idx.size // 2
                idx[idx.size - h:] = idx[:h]
            cls = self._cls_values(idx)
            if form == "batch refused":       # validated first: one index >= n, nothing changes
                bad = np.append(idx, np.uint32(0))
                bad[int(rng.integers(bad.size))] = self._beyond_n()
                rc = g.set_class_batch_raw(bad, np.append(cls, np.uint8(1)))
                assert rc == self.gp.EINVAL, tag + (rc,)
            else:
                if form == "batch dev":       # invalid entries among them: the rest is applied, the call reports RIO_GP_EINVAL
                    if rng.random() < 0.7:
                        idx, cls = np.append(idx, np.uint32(0)), np.append(cls, np.uint8(rng.integers(256)))
                        for k in rng.integers(0, idx.size, int(rng.integers(1, 5))):
                            idx[int(k)] = self._beyond_n()
                    d, ptr = self._dev_offset(idx)
                    off = int(rng.integers(0, 4))
                    dc = self._devbuf()(np.concatenate([np.zeros(off, np.uint8), cls]))
                    bufs += [d, dc]
                    rc = g.set_class_batch_dev_raw(ptr, dc.ptr + off, idx.size)
                    ok = idx < n
                    skipped = not ok.all()
                    assert rc == (self.gp.EINVAL if skipped else self.gp.OK), tag + (rc, skipped)
                    idx, cls = idx[ok], cls[ok]
                else:
                    rc = g.set_class_batch_raw(idx, cls)
                    assert rc == self.gp.OK, tag + (rc,)
                K2 = spec_classes.set_class_batch(self.K, idx, cls)
                if idx.size:                  # is there a row whose first entry carries another class than its last?
                    first = np.zeros(self.nmax, np.uint8)
                    first[idx[::-1]] = cls[::-1]
                    u = np.unique(idx)
                    dup = bool((first[u] != K2[u]).any())
                self.K = K2
                if idx.size and not (had_solve or self.in_flight or self.in_mid) and rng.random() < 0.3:
                    # an update batch over some of the same rows, and nothing in between
                    sub = idx[rng.random(idx.size) < 0.5]
                    sub = sub if sub.size else idx[:1]
                    node = rng.integers(0, self.m, sub.size).astype(np.uint32)
                    node[rng.random(sub.size) < 0.05] = NONE
                    g.update_batch(sub, node)
                    self.oracle.update_batch(self.ref[:n], self.m, sub, node)
                    self.page_writer = updated = True
        self._hit("classes range with unaligned start and end", unaligned)
        self._hit("classes batch with duplicates of one row", dup)
        self._hit("classes_dev batch skipped invalid entries", skipped)
        self._hit("classes batch right before an update batch of the same rows", updated)
        # (a rebalance under a table comes right behind a setter that changed the class of a placed row now and then)
        self.mark = "classes placed" if (K0 is not self.K and bool(((K0[:n] != self.K[:n]) & on0).any())) else "classes"
        self._cls_check(tag)       # (it waits: rio_gp_set_classes_dev does not, and its buffer is freed below)
        for d in bufs:
            d.free()
        self._read_only("classes")
        self.check_table("classes" + (" + update" if updated else ""))

    # ---- immovable classes: rio_gp_set_class_movable / rio_gp_get_class_movable; the rebalance under the table is op_rebalance's ----
    def _mv_check(self, tag):
        got = self.g.get_class_movable()
        assert got.shape == (256,) and np.array_equal(got, self.I), tag + ("get_class_movable differs from the model",
                                                                            np.flatnonzero(got != self.I)[:8])

    def _movable_draw(self, want_imm=False):
        """One table for rio_gp_set_class_movable -> (kind, n_classes, flags or None): a reset | n_classes from 1, 2, 3, 8, 64, 255,
        256 with every class movable, every class immovable, about half of them, only class 255 (n_classes 256), only the class
        most placed rows below n hold (n_classes at least that class + 1), only classes no row below n holds | a table shorter
        than the largest class present, so that the classes from there on are movable again.  A movable class's flag is any
        nonzero byte.  want_imm: one of the kinds that leave rows immovable."""
        rng, n = self.rng, self.n
        K = self.K[:n]
        kinds = ("reset", "all movable", "all immovable", "half", "only 255", "the commonest class", "absent classes", "short")
        kind = kinds[int(rng.integers(8))] if not want_imm else ("half", "half", "the commonest class", "short")[int(rng.integers(4))]
        nc = int(rng.choice([1, 2, 3, 8, 64, 255, 256]))
        if kind == "short":
            nc = int(K.max()) if n else 0
        if (kind == "reset" or nc == 0) and not want_imm:
            return "reset", 0, None
        if nc == 0:
            return "all immovable", 256, np.zeros(256, np.uint8)
        mv = rng.choice(np.array([1, 1, 2, 255], np.uint8), nc)
        if kind == "all immovable":
            mv[:] = 0
        elif kind in ("half", "short"):
            mv[rng.random(nc) < (0.5 if kind == "half" else 0.7)] = 0
        elif kind == "only 255":
            nc, mv = 256, rng.choice(np.array([1, 1, 2, 255], np.uint8), 256)
            mv[255] = 0
        elif kind == "the commonest class":
            held = K[self.ref[:n] != NONE]
            c = int(np.bincount(held, minlength=256).argmax()) if len(held) else 0
            nc = max(nc, c + 1)
            mv = rng.choice(np.array([1, 1, 2, 255], np.uint8), nc)
            mv[c] = 0
        elif kind == "absent classes":
            here = np.zeros(256, bool)
            here[K] = True
            mv[~here[:nc]] = 0
        if want_imm and not (mv[K[K < nc]] == 0).any():      # no row below n would be immovable: every class is
            return "all immovable", 256, np.zeros(256, np.uint8)
        return kind, nc, mv

    def op_movable(self, inner=False, want_imm=False):
        """One rio_gp_set_class_movable call: afterwards rio_gp_get_class_movable equals the model I, and the class column (which
        the call may have allocated, all 0), the column, `used` and an uncommitted solve are as they were.  About one call in
        ten is refused (n_classes 257, a NULL array with n_classes > 0): RIO_GP_EINVAL, I unchanged.  inner: op_rebalance's own
        call right before its rebalance — the setter and the table's getter only."""
        rng, g = self.rng, self.g
        had_solve, first = self.pending is not None, not self.cls_used
        if not inner and rng.random() < 0.1:
            if rng.random() < 0.5:      # (an array that would change the table if it were read)
                kind, rc = "n_classes 257", g.set_class_movable_raw((self.I[np.arange(257) % 256] == 0).astype(np.uint8), n_classes=257)
            else:
                kind, rc = "no array", g.set_class_movable_raw(None, n_classes=int(rng.choice([1, 8, 256])))
            tag = (self.seed, "movable", "refused", kind, self.log[-6:])
            assert rc == self.gp.EINVAL, tag + (rc,)
            self._hit("movable refused")
        else:
            kind, nc, mv = self._movable_draw(want_imm)
            tag = (self.seed, "movable", kind, nc, self.log[-6:])
            k = int(rng.integers(3))
            if k == 0 or (mv is None and k == 1):      # the checked form: n_classes is the array's length
                g.set_class_movable(mv)
            elif mv is None:                            # n_classes 0 with an array: it is not read
                rc = g.set_class_movable_raw(np.zeros(4, np.uint8), n_classes=0)
                assert rc == self.gp.OK, tag + (rc,)
            else:                                       # the array longer than n_classes: the flags behind them are not read
                rc = g.set_class_movable_raw(np.concatenate([mv, np.zeros(3, np.uint8)]), n_classes=nc)
                assert rc == self.gp.OK, tag + (rc,)
            self.I = np.ones(256, np.uint8)
            if nc:
                self.I[:nc] = mv != 0
            self.mv_nc = nc
        self._mv_check(tag)
        if inner:
            return
        self._hit("movable as the first call of the section", first)
        self._hit("movable while a solve is uncommitted", had_solve)
        self._hit("movable between tick_async and tick_wait", self.in_flight)
        self.mark = "movable"
        self._cls_check(tag)
        self._read_only("movable")
        self.check_table("movable")

    def _class_cutoffs(self, nc, placed, hit):
        """One cutoff per class -> (kind, cutoffs).  Each is 0 | the stamp of a placed row of the class (the comparison is
        strict) | one above the largest stamp | 0xFFFFFFFF: drawn per class, or one value for every class, or 0 for every class
        but one.  hit True: every class above every stamp but 0xFFFFFFFF."""
        rng, n, S, K = self.rng, self.n, self.S, self.K
        top = min(int(S[:n].max()) + 1 if n else 1, 0xFFFFFFFF)
        if hit is True:
            return "all idle", rng.choice(np.array([top, 0xFFFFFFFF], np.uint32), nc)
        own = np.zeros(nc, np.uint32)
        if len(placed):
            p = placed[rng.integers(0, len(placed), min(len(placed), 2048))]
            own[:] = S[p[0]]
            sel = K[p] < nc
            own[K[p][sel]] = S[p][sel]
        kind = ("per class", "all equal", "one class")[int(rng.integers(3))]
        if kind == "all equal":
            return kind, np.full(nc, (0, int(own[rng.integers(nc)]), top, 0xFFFFFFFF)[int(rng.integers(4))], np.uint32)
        if kind == "one class":
            cut = np.zeros(nc, np.uint32)
            here = np.unique(K[placed])
            here = here[here < nc]
            c = int(here[rng.integers(len(here))]) if len(here) else int(rng.integers(nc))
            cut[c] = (top, 0xFFFFFFFF, max(int(own[c]), 1))[int(rng.integers(3))]
            return kind, cut
        pick = rng.integers(0, 4, nc)
        return kind, np.array([0, 0, top, 0xFFFFFFFF], np.uint32)[pick] + own * (pick == 1).astype(np.uint32)

    def op_expire_classes(self, hit=None):
        """rio_gp_expire_classes[_dev] against spec_classes.expire_classes_np (up to 4 096 rows the Python-integer expire_classes
        must agree with it first) over the model's column, stamps, classes and loads; the bookkeeping is op_expire's.  hit: None —
        everything is drawn; True — a listing that un-places a row when any placed row can be idle; False — a count-only call or
        every cutoff 0.  -> rows un-placed."""
        import spec_classes
        import spec_expire
        rng, n, g = self.rng, self.n, self.g
        S, A, K = self.S, self.ref, self.K
        had_solve = self.pending is not None
        if hit is None and rng.random() < (0.3 if had_solve else 0.1):      # n_classes 0 | 257: refused, nothing changes
            nc = (0, 257)[int(rng.integers(2))]
            tag = (self.seed, "expire_classes", "refused", nc, n, self.log[-6:])
            out = [np.full(6, 0xDEADBEEF, np.uint32) for _ in range(2)]
            if rng.random() < 0.5:
                rc, _ = g.expire_classes_raw(nc, np.full(257, 0xFFFFFFFF, np.uint32))
            else:
                rc, _ = g.expire_classes_raw(nc, np.full(257, 0xFFFFFFFF, np.uint32), out[0], out[1], 4)
            assert rc == self.gp.EINVAL and all((x == 0xDEADBEEF).all() for x in out), tag + (rc,)
            self._hit("class sweep refused with a solve uncommitted", had_solve)
            self.expc_listed = False
            if self.cls_used:
                self._cls_check(tag)
            self._read_only("expire_classes refused")
            self.check_table("expire_classes refused")
            return 0
        placed = np.flatnonzero(A[:n] != NONE)
        first, zero = not self.cls_used, not K[:n].any()
        nc = int((1, 2, 3, 8, 64, 255, 256, max(int(K[:n].max()) if n else 0, 1))[int(rng.integers(8))])
        form = ("host", "dev", "host", "dev", "count", "dev count")[int(rng.integers(6))]
        if hit is None and had_solve and rng.random() < 0.5:
            hit = True                 # (a sweep that must drop the solve, not one of the many that list nothing)
        behind = self.after in ("class sweep", "class sweep listed")
        if hit is True:
            form = form if form in ("host", "dev") else ("host", "dev")[int(rng.integers(2))]
            nc = 256 if not behind or self.last_nc != 256 else 255
        elif behind and nc == self.last_nc:   # right behind another sweep: a different n_classes, so that copies of the
            nc = 256 if nc != 256 else 3      # per-class counts the sweep before did not zero are added to this one's
        plain = hit is None and zero and rng.random() < 0.25
        if plain:                      # every class is 0: one cutoff is rio_gp_expire's
            nc = 1
        kind, cut = self._class_cutoffs(nc, placed, hit)
        if kind == "all equal" and not plain and rng.random() < 0.5:
            nc, cut = 256, np.full(256, cut[0], np.uint32)
        if hit is False:
            if rng.random() < 0.5:
                cut[:] = 0
            else:
                form = form if form in ("count", "dev count") else ("count", "dev count")[int(rng.integers(2))]
        listing = form in ("host", "dev")
        idle, _, n_idle, _, _, by_all = spec_classes.expire_classes_np(A, S, K, self.load, n, cut, None)
        cap = self._expire_cap(idle, n_idle) if listing else None
        if hit is True and cap == 0:
            cap = 1
        want_cap = cap if listing else 0
        wrows, wnodes, w_idle, wfreed, A2, wby = spec_classes.expire_classes_np(A, S, K, self.load, n, cut, want_cap)
        L = len(wrows)
        tag = (self.seed, "expire_classes", form, nc, kind, cap, n, self.log[-6:])
        assert w_idle == n_idle and np.array_equal(wby, by_all) and int(wby.sum()) == n_idle, tag + ("the reference counts by cap",)
        if n <= 4096:      # the row-by-row restatement as well
            p = spec_classes.expire_classes(A, S, K, self.load, n, [int(x) for x in cut], want_cap)
            assert (np.array_equal(p[0], wrows) and np.array_equal(p[1], wnodes) and p[2:4] == (w_idle, wfreed) and
                    np.array_equal(p[4], A2) and np.array_equal(p[5], wby)), tag + ("the two references differ",)
        if nc == 1 and zero:           # ... and rio_gp_expire's own restatement
            e = spec_expire.expire(A, S, self.load, n, int(cut[0]), want_cap)
            assert (np.array_equal(e[0], wrows) and np.array_equal(e[1], wnodes) and tuple(e[2:4]) == (w_idle, wfreed) and
                    np.array_equal(e[4], A2)), tag + ("spec_expire lists something else on an all-zero class column",)
        Kp, Sp = K[placed], S[placed]
        inside = Kp < nc
        self._hit("class sweep un-placed rows", L > 0)
        self._hit("class sweep capped below n_idle", 0 < L < n_idle)
        self._hit("class sweep with rows of a class >= n_classes", bool((~inside).any()))
        self._hit("class sweep with a placed row stamped exactly at its class's cutoff",
                  bool(((cut[Kp[inside]] > 0) & (Sp[inside] == cut[Kp[inside]])).any()))
        self._hit("class sweep as the first call of the section", first)
        self._hit("class sweep right behind a class sweep", behind and self.last_nc != nc)
        self._hit("class sweep right behind a top", self.after == "top")
        self._hit("class sweep listed rows while a solve was uncommitted", had_solve and L > 0)
        self._hit("class sweep hit nothing while a solve was uncommitted", had_solve and L == 0)
        self._hit("class sweep between two pages of the feed", self.page_open)
        self._hit("class sweep on a handle whose m is below max_nodes", self.m < self.m0)
        self._hit("class sweep between tick_async and tick_wait", self.in_flight)
        self._hit("class sweep with hidden placed rows older than their cutoff",
                  bool(((A[n:] != NONE) & (K[n:] < nc) & (S[n:] < cut[np.minimum(K[n:], nc - 1)])).any()))
        self._hit("class sweep with one cutoff on an all-zero class column", nc == 1 and zero)
        if kind == "all equal" and nc == 256:
            # every class under one cutoff c: as many idle rows as rio_gp_expire(c) counts (two count-only calls: nothing changes)
            a = g.expire(int(cut[0]), count_only=True)[2]
            b = g.expire_classes(cut, count_only=True)[2]
            assert a == b == n_idle, tag + ("count-only rio_gp_expire and the class sweep under one cutoff differ", a, b, n_idle)
            self._hit("class sweep under one cutoff against rio_gp_expire's count")
        by = None
        if form == "count":
            rows, nodes, got_idle, freed, by = g.expire_classes(cut, count_only=True)
        elif form == "dev count":
            got_idle, freed, by = g.expire_classes_dev(cut)
            rows = nodes = np.zeros(0, np.uint32)
        elif form == "host" and (cap is None or rng.random() < 0.5):
            rows, nodes, got_idle, freed, by = g.expire_classes(cut, cap)
        elif form == "host":   # the call as given, into sentinel-filled arrays of cap + 2, without load_freed and idle_by_class
            out = [np.full(cap + 2, 0xDEADBEEF, np.uint32) for _ in range(2)]
            rc, got_idle = g.expire_classes_raw(nc, cut, out[0], out[1], cap)
            assert rc == self.gp.OK, tag + (rc,)
            assert all((x[L:] == 0xDEADBEEF).all() for x in out), tag + ("written past the listing",)
            rows, nodes, freed = out[0][:L], out[1][:L], wfreed
        else:
            c = n if cap is None else int(cap)
            d = [self._devbuf()(np.full(c + 2, 0xDEADBEEF, np.uint32)) for _ in range(2)]
            got_idle, freed, by = g.expire_classes_dev(cut, d[0].ptr, d[1].ptr, c)
            rows, nodes = (x.to_host() for x in d)
            for x in d:
                x.free()
            assert all((x[L:] == 0xDEADBEEF).all() for x in (rows, nodes)), tag + ("written past the listing",)
            rows, nodes = rows[:L], nodes[:L]
        assert got_idle == n_idle, tag + ("n_idle", got_idle, n_idle)
        assert np.array_equal(rows, wrows) and np.array_equal(nodes, wnodes), tag + (rows[:8], wrows[:8], nodes[:8], wnodes[:8])
        assert freed == wfreed, tag + ("load_freed", freed, wfreed)
        if by is not None:             # every idle row of the class, listed or not
            assert len(by) == nc and np.array_equal(by, wby), tag + ("idle_by_class", np.flatnonzero(by != wby)[:8], by[:8], wby[:8])
            assert int(by.sum()) == got_idle, tag + ("idle_by_class does not sum to n_idle", int(by.sum()), got_idle)
        self.ref = A2
        self.expc_listed, self.last_nc = L > 0, nc
        self._seen_check(tag)          # a sweep reads S and K and never writes them (it is a call of the touch section too: S exists)
        self._cls_check(tag)
        if self.hits_used:
            self._hits_check(tag)
        if L > 0:
            self.mark = "class sweep listed"
            self.pending = None
            if had_solve:
                self._dropped("expire_classes")
        else:
            self.mark = "class sweep"
            self._read_only("expire_classes")
        self.check_table("expire_classes")
        return L

    def _census_classes(self, by_node):
        """n_classes of a census: totals — 1, 2, 16, 17, 255, 256; by node — the last value on this side of each boundary of the
        kernel's forms (4 096, 65 536 and 2^20 cells) and the first beyond it, as far as m leaves them inside 1 .. 256, or any."""
        rng, m = self.rng, self.m
        if not by_node:
            return int((1, 2, 16, 17, 255, 256)[int(rng.integers(6))])
        if (1 << 20) % m == 0 and (1 << 20) // m <= 256 and rng.random() < 0.3:
            return (1 << 20) // m      # exactly 2^20 cells: the most the call takes
        c = {int(rng.integers(1, 257))}
        for lim in (4096, 65536, 1 << 20):
            c.update((lim // m, lim // m + 1))
        c = sorted(v for v in c if 1 <= v <= 256)
        return int(c[rng.integers(len(c))])

    def op_census(self):
        """rio_gp_census[_dev] against spec_classes.census_np (up to 4 096 rows the Python-integer census must agree with it
        first): out_rows, out_load and n_other exact, the _dev arrays overwritten, nothing changed."""
        import spec_classes
        rng, n, m, g = self.rng, self.n, self.m, self.g
        A, K = self.ref, self.K
        by_node, dev = bool(rng.random() < 0.6), bool(rng.random() < 0.4)
        nc = self._census_classes(by_node)
        if self.after == "fold" and rng.random() < 0.6:
            # right behind a fold, which is what takes loads to 2^24 and beyond: few cells, so that one of them passes 2^32
            by_node, nc = False, int(rng.integers(1, 3))
        bad =("flag", "n_classes 0", "n_classes 257")[int(rng.integers(3))] if rng.random() < 0.12 else None
        nc = {"n_classes 0": 0, "n_classes 257": 257}.get(bad, nc)
        if bad is None and by_node and m * nc > 1 << 20:
            bad = "cells"
        cells = (m if by_node else 1) * nc
        shape = (m, nc) if by_node else (nc,)
        had_solve = self.pending is not None
        tag = (self.seed, "census", "by node" if by_node else "totals", "dev" if dev else "host", nc, m, n, bad, self.log[-6:])
        SENT = 0xDEADBEEFDEADBEEF
        if bad is not None:      # an unknown flag bit | n_classes 0 or 257 | more than 2^20 cells: refused, nothing changes
            if dev and bad != "flag":
                d = [self._devbuf()(np.full(cells + 1, SENT, np.uint64)) for _ in range(2)]
                self._refused(lambda: g.census_dev(nc, d[0].ptr, d[1].ptr, by_node), tag)
                out = [x.to_host(np.uint64) for x in d]
                for x in d:
                    x.free()
                assert all((x == SENT).all() for x in out), tag + ("a refused census wrote",)
            else:
                flags = int(by_node) | ((2, 4, 1 << 31)[int(rng.integers(3))] if bad == "flag" else 0)
                rc = g.census_raw(nc, by_node, flags)[0]
                assert rc == self.gp.EINVAL, tag + (rc,)
            self._hit("census refused for more than 2^20 cells", bad == "cells")
            self._read_only("census refused")
            self.check_table("census refused")
            return
        wrows, wload, wother = spec_classes.census_np(A, K, self.load, n, nc, m if by_node else None)
        if n <= 4096:      # the row-by-row restatement as well
            p = spec_classes.census(A, K, self.load, n, nc, m if by_node else None)
            assert p[0] == wrows.tolist() and p[1] == wload.tolist() and p[2] == wother, tag + ("the two references differ",)
        on = A[:n] != NONE
        counted = on & (K[:n] < nc)
        self._hit("census by node in one slice", by_node and cells <= 4096)
        self._hit("census by node in several slices", by_node and 4096 < cells <= 65536)
        self._hit("census by node beyond 65 536 cells", by_node and cells > 65536)
        self._hit("census by node of exactly 2^20 cells", by_node and cells == 1 << 20)
        self._hit("census with n_other > 0 by class", not by_node and wother > 0)
        self._hit("census with n_other > 0 by node", by_node and wother > 0)
        self._hit("census at n == 0", n == 0)
        self._hit("census with n not a multiple of 4 and a placed row in the quad behind n",
                  n % 4 != 0 and bool((A[n:(n | 3) + 1] != NONE).any()))
        self._hit("census with a cell whose load exceeds 2^32", bool(wload.size) and int(wload.max()) > 1 << 32)
        self._hit("census as the first call of the section", not self.cls_used)
        self._hit("census between two pages of the feed", self.page_open)
        self._hit("census on a handle whose m is below max_nodes", m < self.m0)
        self._hit("census while a solve is uncommitted", had_solve)
        self._hit("census between tick_async and tick_wait", self.in_flight)
        if dev:            # into arrays that hold a sentinel: the call overwrites every cell and nothing behind them
            d = [self._devbuf()(np.full(cells + 1, SENT, np.uint64)) for _ in range(2)]
            other = g.census_dev(nc, d[0].ptr, d[1].ptr, by_node)
            rows, lsum = (x.to_host(np.uint64) for x in d)
            for x in d:
                x.free()
            assert rows[cells] == SENT and lsum[cells] == SENT, tag + ("written past the cells",)
            rows, lsum = rows[:cells].reshape(shape), lsum[:cells].reshape(shape)
        else:
            rc, rows, lsum, other = g.census_raw(nc, by_node)
            assert rc == self.gp.OK, tag + (rc,)
            assert rows.shape == shape and lsum.shape == shape, tag + ("the arrays are not [m][n_classes]", rows.shape, shape)
        assert other == wother, tag + ("n_other", other, wother)
        assert np.array_equal(rows, wrows), tag + ("out_rows", np.flatnonzero(rows.ravel() != wrows.ravel())[:8])
        assert np.array_equal(lsum, wload), tag + ("out_load", np.flatnonzero(lsum.ravel() != wload.ravel())[:8])
        assert int(rows.sum()) + other == int(on.sum()), tag + ("out_rows and n_other do not sum to the placed rows",)
        assert int(lsum.sum()) == int(self.load[:n][counted].astype(np.uint64).sum()), tag + ("out_load does not sum to the counted rows' load",)
        self._cls_check(tag)       # read-only: K, H, the column, `used` and an uncommitted solve are as they were
        if self.hits_used:
            self._hits_check(tag)
        self._read_only("census")
        self.check_table("census")

    def finish_feed(self):
        """The end of an extended scenario: the rest of the feed is paged out — three small pages, then pages of a third of what
        is left, so that a table of 10^5 changed rows does not take 10^4 calls — and the mirror equals the column on rows < n."""
        pages = 0
        self.paging_out = True     # (no commit from here on: the column the mirror is compared with stays)
        while True:
            left = self._feed(0, True, False)
            if left == 0:
                break
            self._feed(37 if pages < 3 else max(37, -(-left // 3)), False, False)
            pages += 1
        got = self.g.get_assign()
        assert np.array_equal(self.mirror[:self.n], got), (self.seed, "changes", "the mirror differs from the column at the end",
                                                           self.log[-6:], np.flatnonzero(self.mirror[:self.n] != got)[:8])

    NEED_ROWS = ("update", "remove", "lookup", "place", "mixed", "attrs")                       # skipped while n == 0
    WRITERS = ("tick", "solve", "async", "update", "remove", "clean", "place", "mixed", "rebalance", "num_objects", "remap", "expire",
               "expire_classes")
    DROPS_SOLVE = ("tick", "rebalance", "update", "remove", "clean", "place", "mixed", "attrs", "caps", "num_objects", "remap", "expire",
                   "fold", "expire_classes")   # (the fold rewrites loads, not the column: it drops the solve and is no writer of the feed)
    MID = ("none", "index", "changes", "rebalance", "remap", "touch", "expire count", "expire", "hits", "top", "fold",
           "classes", "census", "expire_classes count", "expire_classes", "movable")   # op_async: a call in a quiet run
    # ... after which the next tick must not chain (an "expire" or an "expire_classes" un-placed a row)
    ENDS_CHAIN = ("rebalance", "remap", "expire", "fold", "expire_classes")
    # op_async: the calls that take turns between the last tick_async and tick_wait
    IN_FLIGHT = ("index", "changes", "rebalance", "remap", "touch", "expire", "hits", "fold", "top", "classes", "expire_classes", "census",
                 "movable")

    # run(): the calls that come right behind an uncommitted solve
    BEHIND_SOLVE = ("index", "remap", "rebalance", "remap", "touch", "expire", "expire", "hits", "top", "top", "fold", "fold", "fold",
                    "classes", "classes", "expire_classes", "expire_classes", "census", "census", "movable")

    OPS = (("tick", 5), ("solve", 2), ("async", 3), ("flip", 4), ("update", 2), ("remove", 2), ("lookup", 1), ("clean", 2),
           ("place", 4), ("mixed", 3), ("attrs", 1), ("caps", 1))

    OPS_EXT = OPS + (("index", 3), ("rebalance", 6), ("changes", 5), ("changes_reset", 1), ("num_objects", 2), ("remap", 3),
                     ("touch", 4), ("expire", 4), ("hits", 4), ("fold", 3), ("top", 4), ("classes", 6), ("expire_classes", 4),
                     ("census", 4), ("movable", 3))

    def run(self):
        names = [a for a, w in (self.OPS_EXT if self.ext else self.OPS) for _ in range(w)]
        k = int(self.rng.integers(12, 31))
        try:
            for i in range(k):
                op = names[int(self.rng.integers(len(names)))]
                if self.ext and self.chain_small and self.mids == 0 and i == k - 1:
                    op = "async"       # (no quiet run yet: see op_async)
                elif self.ext and self.pending is not None and self.rng.random() < 0.75:
                    # an uncommitted solve lives until the next writer: three times in four the calls that must keep it, or must drop
                    # it themselves, come right behind it (the table's weights alone bring them there a few times in the default seeds)
                    # (the calls take turns, from a start the seed sets, as MID's and IN_FLIGHT's do)
                    op = self.BEHIND_SOLVE[(7 * self.seed + self.behind) % len(self.BEHIND_SOLVE)]
                    self.behind += 1
                elif self.ext and self.mark is not None and self.rng.random() < 0.3:
                    # the report on the scratch a sweep has just used, right behind the sweep; a class sweep right behind the
                    # report, and right behind another class sweep (the copies of the per-class counts it was to leave zero);
                    # a sweep or a census right behind a setter, while the column is not all one class
                    # a rebalance right behind a call that set the table, behind a setter that changed the class of a placed row and
                    # behind a class sweep that listed rows
                    j = int(self.rng.integers(2))
                    op = {"expire listed": "top", "class sweep listed": ("top", "expire_classes")[j],
                          "class sweep": "expire_classes", "top": "expire_classes", "fold": "census",
                          "classes": ("expire_classes", "census")[j], "classes placed": ("rebalance", "census")[j],
                          "movable": "rebalance", "hits": "fold"}[self.mark]
                    if self.mark == "class sweep listed" and (self.I == 0).any() and self.rng.random() < 0.5:
                        op = "rebalance"
                self.after, self.mark = self.mark, None
                if self.ext and self.n == 0 and op in self.NEED_ROWS:
                    self.log.append("skipped: " + op)
                    continue
                self.log.append(op)
                self.count[op] = self.count.get(op, 0) + 1
                had_solve = self.pending is not None
                getattr(self, "op_" + op)()
                if self.ext:
                    # (a sweep that listed nothing is treated as a refused remap is: it wrote nothing and drops nothing)
                    did = ((op != "mixed" or self.mixed_wrote) and (op != "remap" or not self.remap_refused) and
                           (op != "expire" or self.expire_listed) and (op != "fold" or not self.fold_refused) and
                           (op != "expire_classes" or self.expc_listed))
                    if op in self.WRITERS and (op not in ("remap", "expire", "expire_classes") or did):
                        self.page_writer = True
                    if op in self.DROPS_SOLVE and did:
                        self.pending = None
                        if had_solve and op not in ("rebalance", "remap", "expire", "fold", "expire_classes"):    # (those have asked already)
                            self._dropped(op)
                    elif op in ("mixed", "lookup"):
                        self._read_only(op)
                self.check_table(op)
            if self.ext:
                self.finish_feed()
                self.check_table("the end")
                if (self.remapped or self.seen_used or self.hits_used or self.cls_used) and self.n < self.nmax:
                    # the rows still hidden come back as the removals left them, with the stamps, hits, loads and classes they had
                    self._set_n(self.nmax)
                    self.check_table("the end, every row back (num_objects)")
                if self.hits_used:
                    self._hits_check((self.seed, "the end", "hits and loads over every row", self.log[-6:]), loads=True)
                if self.cls_used:
                    self._cls_check((self.seed, "the end", "classes over every row", self.log[-6:]))
                self._mv_check((self.seed, "the end", "the table of immovable classes", self.log[-6:]))
            self.chained = self.g.chained_scans() if self.lab else 0
        finally:
            self.g.close()
        return k


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


@pytest.mark.parametrize("seed", range(int(os.environ.get("RIO_FUZZ_SEEDS", "36"))))
def test_random_operation_sequences(gp, oracle, seed):
    Scenario(gp, oracle, seed).run()


EXT_SEEDS = int(os.environ.get("RIO_FUZZ_EXT_SEEDS", "120"))


@pytest.mark.parametrize("seed", range(EXT_SEEDS))
def test_random_sequences_with_index_rebalance_and_feed(gp, oracle, seed):
    Scenario(gp, oracle, seed, ext=True).run()


def _sharded_scenario(gp, oracle, seed):
    """The row-sharded solve as G handles on the one device, sequenced by the ShardedSolver the multi-GPU
    bench uses: random shard boundaries (empty and one-row shards included), a stream of committed ticks with liveness
    changes between them, every tick against the WHOLE-table oracle (rows, the global `used` on every rank, the counters)."""
    import sharded
    import torch
    rng = np.random.default_rng(0x5A4D0000 + seed)
    n = _pick(rng, _SIZES, 200_000)
    m = int(rng.choice([1, 2, 7, 33, 64, 257, 1024, 3000, 8192]))
    rounds = int(rng.choice([1, 2, 2, 3]))
    G = int(rng.choice([1, 2, 3, 5, 8]))
    load = (rng.integers(0, 30, n) if rng.random() < 0.5 else rng.zipf(1.3, n).clip(0, 60000)).astype(np.uint32)
    aff = rng.integers(0, m, n).astype(np.uint32)
    aff[rng.random(n) < 0.1] = NONE
    if rng.random() < 0.3:
        aff[rng.random(n) < 0.4] = int(rng.integers(m))
    total = int(load.sum())
    cap = [np.full(m, INF, np.uint64), rng.integers(0, total // m + 5, m).astype(np.uint64),
           np.full(m, (total * 5 // 4) // m + 1, np.uint64)][int(rng.integers(3))]
    alive = (rng.random(m) > rng.choice([0.0, 0.1, 0.5])).astype(np.uint8)
    ref = rng.integers(0, m, n).astype(np.uint32)
    ref[rng.random(n) < rng.choice([0.02, 0.5, 1.0])] = NONE
    cuts = sorted(int(x) for x in rng.integers(0, n + 1, G - 1))
    bounds = [0] + cuts + [n]
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    engines = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        g = gp.GpuPlacement(max(hi - lo, 1), m, spill_rounds=rounds)
        g.set_nodes(cap, alive, m=m)
        g.set_objects(hi - lo, load[lo:hi], aff[lo:hi])
        if hi > lo:
            g.set_assign(ref[lo:hi])
        engines.append(sharded.HipShardEngine(g, 0, stream))
    sol = sharded.ShardedSolver(engines, sharded.LocalExchange(G), spill_rounds=rounds)
    try:
        for step in range(int(rng.integers(3, 7))):
            if step:
                k = rng.integers(3)
                if k == 0:
                    alive = (rng.random(m) > 0.1).astype(np.uint8)
                elif k == 1:
                    alive = np.ones(m, np.uint8)
                else:
                    alive[int(rng.integers(m))] ^= 1
                for e in engines:
                    e.g.set_alive_all(alive)
            if step == 1:
                # once per scenario, between two ticks: a handle of the row-sharded solve (one that has exported its exchange
                # window) refuses the class calls before any launch, and the ticks after it are what they are without them
                import ctypes
                g = engines[int(rng.integers(G))].g
                L, h64 = sharded._lib(), (ctypes.c_char * 64)()
                assert L.rio_gp_shard_p2p_export(g.handle, 1, h64) == gp.OK, (seed, "classes on a shard handle: export")
                try:
                    rc = (g.set_classes_raw(0, np.ones(1, np.uint8)) if rng.random() < 0.5 else g.set_class_batch_raw([0], [1]),
                          g.expire_classes_raw(1, [0xFFFFFFFF])[0], g.census_raw(int(rng.integers(1, 257)), bool(rng.integers(2)))[0],
                          g.set_class_movable_raw(np.zeros(int(rng.choice([1, 8, 256])), np.uint8)))
                finally:
                    assert L.rio_gp_shard_p2p_close(g.handle) == gp.OK, (seed, "classes on a shard handle: close")
                assert rc == (gp.EINVAL,) * 4, (seed, "classes on a shard handle", rc)
                assert g.get_class_movable().all(), (seed, "a refused set_class_movable on a shard handle changed the table")
            st = sol.tick()
            ref, used, ost = oracle.tick(ref, load, aff, cap, alive, rounds)
            got = np.concatenate([e.g.get_assign() if e.g.num_objects else np.zeros(0, np.uint32) for e in engines])
            assert np.array_equal(got, ref), (seed, step, bounds, np.flatnonzero(got != ref)[:8])
            assert st == ost, (seed, step, st, ost)
            for e in engines:
                assert np.array_equal(e.g.get_nodes()[2], used), (seed, step)
    finally:
        for e in engines:
            e.g.close()


@pytest.mark.parametrize("seed", range(int(os.environ.get("RIO_FUZZ_SHARD_SEEDS", "24"))))
def test_random_sharded_tick_streams(gp, oracle, seed):
    _sharded_scenario(gp, oracle, seed)


if __name__ == "__main__":
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (ROOT, os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import json
    try:   # (two HIP runtimes in the process: torch's has to come up first — see tests/conftest.py)
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        pass
    import pyoracle
    import rio_gp
    rio_gp.build()
    pyoracle.build()
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    t0, ops, first, cov = time.time(), 0, seed, {}
    while time.time() - t0 < budget:
        if seed % 10 == 9:   # every tenth scenario: a row-sharded tick stream (G handles on the device)
            _sharded_scenario(rio_gp, pyoracle, seed)
            cov["row-sharded tick streams"] = cov.get("row-sharded tick streams", 0) + 1
            seed += 1
            continue
        sc = Scenario(rio_gp, pyoracle, seed, big=True, ext=seed % 2 == 1)   # old and extended scenarios alternate
        ops += sc.run()
        cov["extended scenarios"] = cov.get("extended scenarios", 0) + int(sc.ext)
        for k, v in list(sc.count.items()) + list(sc.cov.items()):
            cov[k] = cov.get(k, 0) + v
        for k, on in (("tables >= 10^5 rows", sc.n >= 100_000), ("tables >= 2^19 rows", sc.n >= 524288), ("self-assign", sc.sa),
                      ("forced policies (lab build)", sc.lab), ("scenarios with chained quiet ticks", sc.chained > 0)):
            cov[k] = cov.get(k, 0) + int(on)
        cov["chained scans"] = cov.get("chained scans", 0) + sc.chained
        seed += 1
    print(json.dumps({"scenarios": seed - first, "first_seed": first, "operations_checked": ops, "seconds": round(time.time() - t0, 1),
                      "mismatches": 0, "coverage": cov}))
