"""numpy engine of the row-sharded rebalance with the load-ordered cut — TEST INFRASTRUCTURE ONLY.

tests/shard_rebalance_cpu.py::CpuRebalanceEngine plus the steps of a load-ordered session (rebalance_begin(order=1),
rebalance_threshold_plan / _hist / _pick), written out from the protocol text in include/rio_gpu_placement.h ("row-sharded
rebalance": the H record, R1' on rank r), so that `ShardedSolver.rebalance(order=1)` can be checked against the whole-table
references without a GPU.  Never imported by the product package.
"""
import numpy as np

from shard_engine_cpu import _u64
from shard_rebalance_cpu import INACTIVE, CpuRebalanceEngine

BY_LOAD = 1
MAX_DIGIT_BITS = 11


class CpuOrderedRebalanceEngine(CpuRebalanceEngine):
    def rebalance_begin(self, rank, n_ranks, target, max_moves, rounds, list_moves, x, order=0):
        if order not in (0, BY_LOAD):
            raise ValueError("bad arguments")
        nr = super().rebalance_begin(rank, n_ranks, target, max_moves, rounds, list_moves, x)
        self.rb_order = order
        if order == BY_LOAD:   # word 2m of X: the largest load among this rank's object rows on a node < m
            rows = (self.assign < self.m) & (self.aff != INACTIVE)
            _u64(x)[2 * self.m] = int(self.load[rows].max()) if rows.any() else 0
        self.rb_pass = self.rb_passes = self.rb_skip = 0
        self.rb_hist_out = False
        return nr

    def _by_load(self):
        return getattr(self, "rb_order", 0) == BY_LOAD

    def rebalance_cut(self, xg, s):
        if not self._by_load():
            return super().rebalance_cut(xg, s)
        self._need(self.rb_state == 1)
        m, T = self.m, self.rb_T
        X = _u64(xg).reshape(self.rb_R, self.words1)
        P = X[:, :m].sum(axis=0, dtype=np.uint64)
        ctot = X[:, m:2 * m].sum(axis=0, dtype=np.uint64)
        self.used = P + ctot
        fr = np.where(self.alive & (T > P), T - P, 0).astype(np.uint64)
        over = self.alive & (ctot > fr)
        self.rb_over_before = int((self.alive & (self.used > T)).sum())
        # every globally over node is a slot on every rank, in ascending node order
        self.rb_slot_node = np.flatnonzero(over)
        self.rb_slot_of = np.full(m, -1, np.int64)
        self.rb_slot_of[self.rb_slot_node] = np.arange(len(self.rb_slot_node))
        self.rb_rem = [int(fr[j]) for j in self.rb_slot_node]      # what is left of the GLOBAL free_j
        self.rb_pre = [0] * len(self.rb_slot_node)                  # the digits chosen so far
        self.rb_surplus = np.zeros(self.n, bool)
        _u64(s)[:] = 0                                              # the surplus is not known yet
        self.rb_over = int(over.sum())
        # the digit: 11 bits at most, narrowed until the record is no longer than X
        bits = MAX_DIGIT_BITS
        while bits > 1 and (self.rb_over << bits) > self.words1:
            bits -= 1
        self.rb_bits = bits
        # the passes of the whole search, from bit 32 down, without those whose digit lies wholly above the largest load
        top = int(X[:, 2 * m].max()).bit_length() or 32
        whole = -(-32 // bits)
        self.rb_skip = 0
        while self.rb_skip + 1 < whole and max(32 - (self.rb_skip + 1) * bits, 0) >= top:
            self.rb_skip += 1
        self.rb_passes = whole - self.rb_skip if self.rb_over else 0
        self.rb_pass = 0
        self.rb_hist_out = False
        self.rb_state = 2
        return self.rb_over

    def _digit(self, p):
        hi = 32 - (p + self.rb_skip) * self.rb_bits
        lo = max(hi - self.rb_bits, 0)
        return hi, lo, 1 << (hi - lo)

    def _pending(self):
        return self._by_load() and self.rb_over > 0 and self.rb_pass < self.rb_passes

    def rebalance_threshold_plan(self):
        self._need(self.rb_state == 2 and self._by_load() and self.rb_over > 0)
        return self.rb_passes, self.rb_over << self.rb_bits

    def rebalance_threshold_hist(self, p, hist):
        self._need(self.rb_state == 2 and self._pending() and p == self.rb_pass)
        hi, lo, bins = self._digit(p)
        stride = 1 << self.rb_bits
        H = _u64(hist)
        if len(H) != self.rb_over << self.rb_bits:
            raise ValueError("histogram buffer of %d words" % len(H))
        H[:] = 0
        rows = np.flatnonzero(self.rb_cand & (self.load > 0))
        if len(rows):
            sl = self.rb_slot_of[self.assign[rows]]
            rows, sl = rows[sl >= 0], sl[sl >= 0]
            l = self.load[rows].astype(np.uint64)
            pre = np.array(self.rb_pre, np.uint64)[sl] if len(sl) else np.zeros(0, np.uint64)
            agree = (l >> np.uint64(hi)) == (pre >> np.uint64(hi)) if hi < 32 else np.ones(len(rows), bool)
            d = (l >> np.uint64(lo)) & np.uint64(bins - 1)
            np.add.at(H, (sl[agree] * stride + d[agree].astype(np.int64)), l[agree])
        self.rb_hist_out = True

    def rebalance_threshold_pick(self, p, hg, s=None):
        self._need(self.rb_state == 2 and self._pending() and p == self.rb_pass and self.rb_hist_out)
        last = p + 1 == self.rb_passes
        if last and s is None:
            raise ValueError("the last pass writes the S record")
        hi, lo, bins = self._digit(p)
        stride, r = 1 << self.rb_bits, self.rb_rank
        Hg = _u64(hg).reshape(self.rb_R, self.rb_over << self.rb_bits)
        tot = Hg.sum(axis=0, dtype=np.uint64)                       # (integer sums: the rank order changes nothing)
        keep = {}
        for k, j in enumerate(self.rb_slot_node):
            run, rem = 0, self.rb_rem[k]
            for d in range(bins):
                v = int(tot[k * stride + d])
                if run + v > rem:                                    # the first digit whose inclusive sum passes rem
                    break
                run += v
            else:
                raise AssertionError("an over node's candidates weigh more than free")
            self.rb_rem[k] = rem - run
            self.rb_pre[k] |= d << lo
            if last:
                tau = self.rb_pre[k]
                ties = [int(Hg[q, k * stride + d]) // tau for q in range(self.rb_R)]
                c = self.rb_rem[k] // tau
                keep[int(j)] = (tau, min(max(c - sum(ties[:r]), 0), ties[r]))
        if last:
            surplus = np.zeros(self.n, bool)
            seen = {}
            for i in np.flatnonzero(self.rb_cand):                   # row order
                j = int(self.assign[i])
                if j not in keep:
                    continue
                tau, mine = keep[j]
                l = int(self.load[i])
                if l > tau:
                    surplus[i] = True
                elif l == tau:
                    seen[j] = seen.get(j, 0) + 1
                    surplus[i] = seen[j] > mine
            self.rb_surplus = surplus
            S = _u64(s)
            S[:] = 0
            S[0] = int(surplus.sum())
            S[1] = int(self.load[surplus].sum(dtype=np.uint64))
        self.rb_hist_out = False
        self.rb_pass += 1

    def rebalance_select(self, sg, y):
        self._need(not self._pending())
        return super().rebalance_select(sg, y)
