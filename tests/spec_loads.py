"""Measured load restated with Python integers (include/rio_gpu_placement.h "measured load"; DESIGN.md section 2 rule 10): the hit
column H under rio_gp_hits_add_batch and rio_gp_hits_merge, and what rio_gp_load_fold makes of load and H.  Every sum is taken
in Python integers (no wrap) and cut to a u32 at the end, so the restatement shares no arithmetic with the kernels; the merge and
the fold evaluate their row rule once per distinct (load, hits) pair, which keeps a table of 10^5 rows a matter of milliseconds.  `used` is
k_used in numpy.  String layer: which calls count a request, as a dict model keeps them."""
import numpy as np

NONE = 0xFFFFFFFF
U32 = 0xFFFFFFFF
KEEP_ONE = 65536


def _per_pair(a, b, f):
    """[f(a[r], b[r]) for every row r] as uint32, f called with Python integers once per DISTINCT pair: a table of 10^5 rows has
    few of them, and the arithmetic stays f's.  (The pairs are packed into one u64 to find the distinct ones; f sees them unpacked.)"""
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    if len(a) == 0:
        return np.zeros(0, np.uint32)
    uniq, inv = np.unique((a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64), return_inverse=True)
    return np.array([f(k >> 32, k & U32) for k in uniq.tolist()], np.uint32)[inv.ravel()]


def hits_add(H, idx, weight=None):
    """rio_gp_hits_add_batch -> H': H[idx[k]] = min(H[idx[k]] + w[k], 2^32-1); duplicates sum; the order does not matter."""
    out = np.array(H, np.uint32, copy=True)
    idx = np.asarray(idx, np.int64).tolist()
    w = [1] * len(idx) if weight is None else np.asarray(weight, np.uint32).tolist()
    add = {}     # row -> the sum of its weights (Python integers), so that only the rows the batch names are walked
    for i, x in zip(idx, w):
        add[i] = add.get(i, 0) + x
    for i, x in add.items():
        out[i] = min(int(out[i]) + x, U32)
    return out


def hits_merge(H, counts):
    """rio_gp_hits_merge -> H': H[r] = min(H[r] + counts[r], 2^32-1) for r < len(counts)."""
    H = np.array(H, np.uint32, copy=True)
    k = len(counts)
    H[:k] = _per_pair(H[:k], counts, lambda h, c: min(h + c, U32))
    return H


def fold_one(load, hits, keep, gain, min_load, max_load):
    """One row of rio_gp_load_fold: clamp(floor(load * keep / 65536) + hits * gain, min_load, max_load)."""
    assert 0 <= keep <= KEEP_ONE and min_load <= max_load
    x = (int(load) * int(keep)) // KEEP_ONE + int(hits) * int(gain)
    return max(int(min_load), min(int(max_load), x))


def load_fold(load, H, n, keep, gain, min_load, max_load):
    """rio_gp_load_fold -> (load', H', stats): rows r < n are folded and their H zeroed; rows >= n keep both."""
    load = np.array(load, np.uint32, copy=True)
    H = np.array(H, np.uint32, copy=True)
    folded = _per_pair(load[:n], H[:n], lambda l, h: fold_one(l, h, keep, gain, min_load, max_load))
    old, hits, new = load[:n].tolist(), H[:n].tolist(), folded.tolist()    # (Python integers)
    st = {"rows_changed": int(np.count_nonzero(folded != load[:n])), "hits_folded": sum(hits),
          "load_before": sum(old), "load_after": sum(new), "max_load_after": max(new) if new else 0}
    load[:n] = folded
    H[:n] = 0
    return load, H, st


def used_of(assign, load, n, m):
    """k_used: used[j] = the sum of load over the rows r < n with assign[r] == j < m (uint64)."""
    a = np.asarray(assign, np.uint32)[:n].astype(np.int64)
    ok = a < m
    out = np.zeros(m, np.uint64)
    np.add.at(out, a[ok], np.asarray(load, np.uint32)[:n][ok].astype(np.uint64))
    return out


class OpLoads:
    """The string layer's request counters as the contract describes them: {key: requests since the last fold} while tracking is
    on, {key: load} (absent: 1) for every key that has a row."""

    def __init__(self):
        self.on, self.hits, self.load = False, {}, {}

    def count(self, key):
        """a call answered or set an address for `key`"""
        if self.on:
            self.hits[key] = min(self.hits.get(key, 0) + 1, U32)

    def fold(self, keys, keep, gain, min_load, max_load):
        """rio_op_fold_loads over `keys` (every key that has a row) -> (rows_changed, hits_folded)"""
        changed, folded = 0, 0
        for k in keys:
            old = self.load.get(k, 1)
            new = fold_one(old, self.hits.get(k, 0), keep, gain, min_load, max_load)
            changed += new != old
            folded += self.hits.get(k, 0)
            self.load[k] = new
        self.hits = {}
        return changed, folded

    def forget(self, key):
        """the key's row changes hands: load 1 and no requests for whoever gets it"""
        self.load.pop(key, None)
        self.hits.pop(key, None)
