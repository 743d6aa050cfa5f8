"""Object classes restated in plain numpy and Python integers (include/rio_gpu_placement.h "object classes"; DESIGN.md section 2
rule 12): the class column K under its setters, what rio_gp_expire_classes lists and un-places, and what rio_gp_census counts."""
import numpy as np

NONE = 0xFFFFFFFF
MAX_CLASSES = 256


def set_classes(K, first_row, cls):
    """rio_gp_set_classes -> K': K[first_row + k] = cls[k]; nothing else changes."""
    K = np.array(K, np.uint8, copy=True)
    cls = np.asarray(cls, np.uint8)
    K[first_row:first_row + len(cls)] = cls
    return K


def set_class_batch(K, idx, cls):
    """rio_gp_set_class_batch -> K': the entries applied one after the other in batch order, so the last entry of a row wins."""
    K = np.array(K, np.uint8, copy=True)
    for i, c in zip(np.asarray(idx, np.int64).tolist(), np.asarray(cls, np.uint8).tolist()):
        K[i] = c
    return K


def expire_classes(A, S, K, load, n, cutoffs, cap=None):
    """-> (rows, nodes, n_idle, load_freed, A', idle_by_class): row r < n is idle iff A[r] != NONE and K[r] < len(cutoffs) and
    S[r] < cutoffs[K[r]] (raw values); the listing is the first min(n_idle, cap) idle rows, ascending, with their nodes; A' = A
    with exactly the listed rows un-placed; load_freed = the sum of their loads; idle_by_class[c] = every idle row of class c,
    listed or not.  cap None: no limit.  S, K and rows >= n are never changed."""
    A = np.array(A, np.uint32, copy=True)
    assert 1 <= len(cutoffs) <= MAX_CLASSES
    idle, by = [], [0] * len(cutoffs)
    for r in range(n):
        c = int(K[r])
        if int(A[r]) != NONE and c < len(cutoffs) and int(S[r]) < int(cutoffs[c]):
            idle.append(r)
            by[c] += 1
    k = np.array(idle if cap is None else idle[:int(cap)], np.uint32)
    nodes = A[k].copy()
    freed = sum(int(load[r]) for r in k.tolist())
    A[k] = NONE
    return k, nodes, len(idle), freed, A, np.array(by, np.uint64)


def expire_classes_np(A, S, K, load, n, cutoffs, cap=None):
    """expire_classes vectorised, for the long tables of the device tests (tests/test_classes_spec.py holds the two together)."""
    A = np.array(A, np.uint32, copy=True)
    K = np.asarray(K, np.uint8)[:n].astype(np.int64)
    nc = len(cutoffs)
    assert 1 <= nc <= MAX_CLASSES
    table = np.zeros(MAX_CLASSES, np.uint32)            # 0 behind the given cutoffs: S < 0 never holds
    table[:nc] = np.asarray(cutoffs, np.uint32)
    idle = np.flatnonzero((A[:n] != NONE) & (np.asarray(S, np.uint32)[:n] < table[K])).astype(np.uint32)
    by = np.bincount(K[idle], minlength=MAX_CLASSES)[:nc].astype(np.uint64)
    k = idle if cap is None else idle[:int(cap)]
    nodes = A[k].copy()
    freed = int(np.asarray(load, np.uint64)[k].sum())
    A[k] = NONE
    return k, nodes, int(len(idle)), freed, A, by


def census(A, K, load, n, n_classes, m=None):
    """rio_gp_census -> (rows, load, n_other) as Python-int lists: m None: [n_classes]; else RIO_GP_CENSUS_BY_NODE over m nodes:
    [m][n_classes].  A placed row of a class >= n_classes (by node: or on a node id >= m) is counted in n_other only."""
    assert 1 <= n_classes <= MAX_CLASSES
    by_node = m is not None
    rows = [[0] * n_classes for _ in range(m if by_node else 1)]
    lsum = [[0] * n_classes for _ in range(m if by_node else 1)]
    other = 0
    for r in range(n):
        a, c = int(A[r]), int(K[r])
        if a == NONE:
            continue
        if c >= n_classes or (by_node and a >= m):
            other += 1
            continue
        j = a if by_node else 0
        rows[j][c] += 1
        lsum[j][c] += int(load[r])
    return (rows, lsum, other) if by_node else (rows[0], lsum[0], other)


def census_np(A, K, load, n, n_classes, m=None):
    """census vectorised (uint64 arrays), for the long tables of the device tests."""
    A = np.asarray(A, np.uint32)[:n].astype(np.int64)
    K = np.asarray(K, np.uint8)[:n].astype(np.int64)
    load = np.asarray(load, np.uint32)[:n].astype(np.int64)
    by_node = m is not None
    placed = A != NONE
    ok = placed & (K < n_classes) & ((A < m) if by_node else True)
    cell = (A[ok] * n_classes if by_node else 0) + K[ok]
    cells = (m if by_node else 1) * n_classes
    rows = np.bincount(cell, minlength=cells).astype(np.uint64)
    # the load sums as two weighted counts of 16-bit halves: every partial sum stays below 2^53, so float64 holds it exactly
    # (fewer than 2^37 rows); one pass each, where np.add.at walks the rows one by one
    w = load[ok]
    lo = np.bincount(cell, weights=w & 0xFFFF, minlength=cells).astype(np.uint64)
    hi = np.bincount(cell, weights=w >> 16, minlength=cells).astype(np.uint64)
    lsum = lo + (hi << np.uint64(16))
    shape = (m, n_classes) if by_node else (n_classes,)
    return rows.reshape(shape), lsum.reshape(shape), int(placed.sum() - ok.sum())
