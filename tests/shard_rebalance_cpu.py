"""numpy engine of the row-sharded rebalance — TEST INFRASTRUCTURE ONLY.

The step methods of rio-rs_amd/sharded.py::HipShardEngine.rebalance_*, written out from the protocol in
include/rio_gpu_placement.h ("row-sharded rebalance") on top of tests/shard_engine_cpu.py, so that `ShardedSolver.rebalance`
(what is all-gathered, how the records are reduced in rank order, when the rounds stop) can be checked against the whole-table
references (tests/rebalance_ref.py, tests/spec_rebalance.py) without a GPU.  Never imported by the product package.
"""
import numpy as np

import spec_tick
from shard_engine_cpu import CpuShardEngine, _u64

NONE = 0xFFFFFFFF
INACTIVE = 0xFFFFFFFE
U64MAX = (1 << 64) - 1
SUM_KEYS = ("surplus_rows", "surplus_load", "selected_rows", "selected_load", "moved_rows", "moved_load", "stayed_rows")


class CpuRebalanceEngine(CpuShardEngine):
    def __init__(self, cur, load, aff, cap, alive, spill_rounds=2):
        super().__init__(cur, load, aff, cap, alive)
        self.spill_rounds = spill_rounds
        self.rb_state = 0

    @property
    def num_rows(self):
        return self.n

    def _need(self, ok):
        if not ok:
            raise ValueError("rebalance step out of order")

    def rebalance_begin(self, rank, n_ranks, target, max_moves, rounds, list_moves, x):
        if rounds > 8 or rank >= n_ranks:
            raise ValueError("bad arguments")
        m, c, l = self.m, self.assign, self.load.astype(np.uint64)
        self.rb_rank, self.rb_R = rank, n_ranks
        self.rb_T = self.cap.copy() if target is None else np.ascontiguousarray(target, np.uint64)[:m].copy()
        self.rb_B = int(max_moves)
        self.rb_rounds = rounds if rounds else self.spill_rounds
        on = c < m
        obj = self.aff != INACTIVE
        live = on.copy()
        live[on] = self.alive[c[on]]
        self.rb_cand = live & obj
        pin, lu = np.zeros(m, np.uint64), np.zeros(m, np.uint64)
        np.add.at(lu, c[on], l[on])
        np.add.at(pin, c[on & ~obj], l[on & ~obj])
        self.rb_lu = lu
        X = _u64(x)
        X[:] = 0
        X[:m] = pin
        X[m:2 * m] = lu - pin
        X[2 * m + 7] = 1
        self.rb_fills = 0
        self.rb_surplus = np.zeros(self.n, bool)
        self.rb_sel = np.zeros(0, np.int64)
        self.rb_node = np.zeros(0, np.uint32)
        self.rb_over = self.rb_total = self.rb_pending = 0
        self.rb_state = 1
        return self.rb_rounds

    def rebalance_cut(self, xg, s):
        self._need(self.rb_state == 1)
        m, r, T = self.m, self.rb_rank, self.rb_T
        X = _u64(xg).reshape(self.rb_R, self.words1)
        P = X[:, :m].sum(axis=0, dtype=np.uint64)
        cpre = X[:r, m:2 * m].sum(axis=0, dtype=np.uint64) if r else np.zeros(m, np.uint64)
        ctot = X[:, m:2 * m].sum(axis=0, dtype=np.uint64)
        self.used = P + ctot
        fr = np.where(self.alive & (T > P), T - P, 0).astype(np.uint64)
        over = self.alive & (ctot > fr)
        self.rb_over_before = int((self.alive & (self.used > T)).sum())
        forced = over & (cpre > fr)
        left = np.where(forced, 0, fr - np.minimum(cpre, fr)).astype(np.uint64)
        surplus = np.zeros(self.n, bool)
        run = {}
        cutdone = set()
        for i in np.flatnonzero(self.rb_cand):     # row order; strict prefix cut per over node
            j = int(self.assign[i])
            if not over[j]:
                continue
            if forced[j] or j in cutdone:
                surplus[i] = True
                continue
            q = run.get(j, 0) + int(self.load[i])
            if q > int(left[j]):
                cutdone.add(j)
                surplus[i] = True
            else:
                run[j] = q
        self.rb_surplus = surplus
        S = _u64(s)
        S[:] = 0
        S[0] = int(surplus.sum())
        S[1] = int(self.load[surplus].sum(dtype=np.uint64))
        self.rb_over = int(over.sum())
        self.rb_state = 2
        return self.rb_over

    def rebalance_select(self, sg, y):
        self._need(self.rb_state == 2 and self.rb_over > 0)
        m, r = self.m, self.rb_rank
        S = _u64(sg).reshape(self.rb_R, self.words2)
        pre, tot, mine = int(S[:r, 0].sum(dtype=np.uint64)), int(S[:, 0].sum(dtype=np.uint64)), int(S[r, 0])
        K = min(max(self.rb_B - pre, 0), mine)
        self.rb_sel = np.flatnonzero(self.rb_surplus)[:K]
        self.rb_node = np.full(K, NONE, np.uint32)
        l = self.load[self.rb_sel].astype(np.uint64)
        np.subtract.at(self.rb_lu, self.assign[self.rb_sel], l)
        Y = _u64(y)
        Y[:m] = self.rb_lu
        Y[m] = int(l.sum(dtype=np.uint64))
        Y[m + 1] = K
        self.rb_total = min(self.rb_B, tot)
        self.rb_first = True
        self.rb_state = 3
        return K, self.rb_total

    def rebalance_merge(self, yg):
        self._need((self.rb_state == 3 and self.rb_total > 0) or self.rb_state == 5)
        m, r = self.m, self.rb_rank
        Y = _u64(yg).reshape(self.rb_R, self.words2)
        add = Y[:, :m].sum(axis=0, dtype=np.uint64)
        self.used = add if self.rb_first else self.used + add
        self.rb_first = False
        self.rb_base = int(Y[:r, m].sum(dtype=np.uint64)) if r else 0
        self.rb_pending = int(Y[:, m + 1].sum(dtype=np.uint64))
        self.rb_state = 4
        return self.rb_pending, int(Y[:, m].sum(dtype=np.uint64))

    def rebalance_fill(self, rnd, y):
        self._need(self.rb_state == 4 and rnd == self.rb_fills and rnd < self.rb_rounds and self.rb_pending > 0)
        m, T = self.m, self.rb_T
        last = rnd + 1 == self.rb_rounds
        fre = np.where(self.alive & (T > self.used), T - self.used, 0).astype(np.uint64)
        nz = np.flatnonzero(fre > 0)
        order = sorted(nz.tolist(), key=lambda j: (-spec_tick.capacity_class(int(fre[j])), j))
        Cs = [0]
        for j in order:
            Cs.append(min(Cs[-1] + int(fre[j]), U64MAX))
        adm = np.zeros(m, np.uint64)
        Q = self.rb_base
        left_rows = left_load = 0
        for k in np.flatnonzero(self.rb_node == NONE):
            l = int(self.load[self.rb_sel[k]])
            node = NONE
            if order and Q < Cs[-1]:
                lo = _last_le(Cs, Q)
                if Q + l <= Cs[lo + 1]:
                    node = order[lo]
            Q += l
            if node != NONE:
                self.rb_node[k] = node
                adm[node] += np.uint64(l)
            else:
                left_rows += 1
                left_load += l
                if last:   # R4: the load stays on the row's own node
                    adm[self.assign[self.rb_sel[k]]] += np.uint64(l)
        Y = _u64(y)
        Y[:m] = adm
        Y[m] = left_load
        Y[m + 1] = left_rows
        self.rb_fills += 1
        self.rb_state = 5

    def rebalance_finish(self, list_moves):
        done = ((self.rb_state == 2 and self.rb_over == 0) or (self.rb_state == 3 and self.rb_total == 0) or
                (self.rb_state == 4 and (self.rb_pending == 0 or self.rb_fills == self.rb_rounds)))
        self._need(done)
        ran = self.rb_state == 4
        sel, node = (self.rb_sel, self.rb_node) if ran else (np.zeros(0, np.int64), np.zeros(0, np.uint32))
        frm = self.assign[sel]
        mv = (node != NONE) & (node != frm)
        rows = sel[mv].astype(np.uint32)
        st = dict(surplus_rows=int(self.rb_surplus.sum()), surplus_load=int(self.load[self.rb_surplus].sum(dtype=np.uint64)),
                  selected_rows=len(self.rb_sel) if self.rb_state >= 3 else 0,
                  selected_load=int(self.load[self.rb_sel].sum(dtype=np.uint64)) if self.rb_state >= 3 else 0,
                  moved_rows=int(mv.sum()), moved_load=int(self.load[rows].sum(dtype=np.uint64)),
                  stayed_rows=int((node == NONE).sum()), nodes_over_before=self.rb_over_before,
                  nodes_over_after=int((self.alive & (self.used > self.rb_T)).sum()))
        f, t = frm[mv].copy(), node[mv].copy()
        self.assign[rows] = t
        self.rb_state = 0
        if not list_moves:
            e = np.empty(0, np.uint32)
            return st, e, e, e
        return st, rows, f, t


def _last_le(Cs, Q):
    """largest k with Cs[k] <= Q (Cs ascending, Cs[0] = 0)"""
    lo, hi = 0, len(Cs) - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if Cs[mid] <= Q:
            lo = mid
        else:
            hi = mid
    return lo
