"""Idle expiry restated in plain numpy (include/rio_gpu_placement.h "idle expiry"; DESIGN.md section 2 rule 9): the last-seen
column S under the touch calls, and what rio_gp_expire lists and un-places.  String layer: which keys a sweep lists, from the
stamps a model of the host keeps."""
import numpy as np

NONE = 0xFFFFFFFF
AFF_INACTIVE = 0xFFFFFFFE


def touch(S, idx, epoch):
    """rio_gp_touch_batch -> S': S[idx[k]] = max(S[idx[k]], epoch); duplicates and order do not matter."""
    S = np.array(S, np.uint32, copy=True)
    idx = np.asarray(idx, np.int64)
    np.maximum.at(S, idx, np.uint32(epoch))
    return S


def touch_all(S, n, epoch):
    """rio_gp_touch_all -> S': rows < n are seen at `epoch` at the least; rows >= n keep their S."""
    S = np.array(S, np.uint32, copy=True)
    S[:n] = np.maximum(S[:n], np.uint32(epoch))
    return S


def touch_merge(S, stamps):
    """rio_gp_touch_merge -> S': S[r] = max(S[r], stamps[r]) for r < len(stamps)."""
    S = np.array(S, np.uint32, copy=True)
    stamps = np.asarray(stamps, np.uint32)
    S[:len(stamps)] = np.maximum(S[:len(stamps)], stamps)
    return S


def expire(A, S, load, n, cutoff, cap=None):
    """-> (rows, nodes, n_idle, load_freed, A'): row r < n is idle iff A[r] != NONE and S[r] < cutoff (raw values); the listing is
    the first min(n_idle, cap) idle rows, ascending, with their nodes; A' = A with exactly the listed rows un-placed; load_freed =
    the sum of their loads.  cap None: no limit.  S and rows >= n are never changed."""
    A = np.array(A, np.uint32, copy=True)
    S = np.asarray(S, np.uint32)
    idle = np.flatnonzero((A[:n] != NONE) & (S[:n] < np.uint32(cutoff))).astype(np.uint32) if cutoff > 0 else np.empty(0, np.uint32)
    n_idle = int(len(idle))
    k = idle if cap is None else idle[:int(cap)]
    nodes = A[k].copy()
    freed = int(np.asarray(load, np.uint64)[k].sum())
    A[k] = NONE
    return k, nodes, n_idle, freed, A


def op_expire(placed, stamps, cutoff, cap=None):
    """String layer: placed {key: address} in row order (a dict keeps insertion order only by accident: pass rows = [(row, key)]
    where order matters), stamps {key: epoch} (absent: never stamped) -> the keys a sweep with `cutoff` lists, as a set."""
    idle = [k for k in placed if stamps.get(k, 0) < cutoff]
    return set(idle if cap is None else idle[:cap])
