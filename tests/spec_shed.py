"""Rule 14 (pressure shedding) restated with Python integers, twice: L1 in its sequential form (a node's
candidates walked in (S descending, row ascending) order against free_j) and in its threshold form (sigma_j, cutrow_j), then
L2 / L3 with `used`, the counters and the listing.  No numpy arithmetic decides anything here: the arrays are read into ints."""

NONE = 0xFFFFFFFF
AFF_INACTIVE = 0xFFFFFFFE
NEVER = 0xFFFFFFFFFFFFFFFF
MAX_CLASSES = 256


def cutoff_of(k, cutoff, class_cutoffs, immovable):
    """L0: the effective cutoff of a row of class k."""
    if immovable is not None and k in immovable:
        return 0
    if class_cutoffs is None:
        return int(cutoff)
    return int(class_cutoffs[k]) if k < len(class_cutoffs) else 0


def classify(A, load, aff, S, K, n, m, alive, cutoff, class_cutoffs=None, immovable=None):
    """L0: (cands, pinned) — per node the candidate rows (ascending) and the pinned load; dead nodes and nodes >= m: absent."""
    cands = {j: [] for j in range(m) if alive[j]}
    pinned = {j: 0 for j in cands}
    for r in range(n):
        j = int(A[r])
        if j >= m or j not in cands:
            continue
        k = int(K[r]) if K is not None else 0
        c = cutoff_of(k, cutoff, class_cutoffs, immovable)
        if int(aff[r]) != AFF_INACTIVE and int(load[r]) >= 1 and int(S[r]) < c:
            cands[j].append(r)
        else:
            pinned[j] += int(load[r])
    return cands, pinned


def _free(T, j, pinned):
    t = int(T[j])
    return t - pinned[j] if t > pinned[j] else 0


def surplus_sequential(load, S, T, cands, pinned):
    """L1, sequential form: the set of surplus rows."""
    out = set()
    for j, rows in cands.items():
        free = _free(T, j, pinned)
        pre, over = 0, False
        for r in sorted(rows, key=lambda r: (-int(S[r]), r)):
            pre += int(load[r])
            over = over or pre > free
            if over:
                out.add(r)
    return out


def thresholds(load, S, T, cands, pinned):
    """L1, threshold form: {j: (sigma_j, cutrow_j, rem_j)} for the over nodes (those with more candidate load than free_j)."""
    out = {}
    for j, rows in cands.items():
        free = _free(T, j, pinned)
        if sum(int(load[r]) for r in rows) <= free:
            continue
        by_stamp = {}
        for r in rows:
            by_stamp[int(S[r])] = by_stamp.get(int(S[r]), 0) + int(load[r])
        above = 0
        for sigma in sorted(by_stamp, reverse=True):
            if above + by_stamp[sigma] > free:
                break
            above += by_stamp[sigma]
        rem = free - above
        pre, cutrow = 0, None
        for r in rows:                      # (ascending rows)
            if int(S[r]) != sigma:
                continue
            pre += int(load[r])
            if pre > rem:
                cutrow = r
                break
        out[j] = (sigma, cutrow, rem)
    return out


def surplus_threshold(S, cands, thr):
    out = set()
    for j, (sigma, cutrow, _rem) in thr.items():
        for r in cands[j]:
            if int(S[r]) < sigma or (int(S[r]) == sigma and r >= cutrow):
                out.add(r)
    return out


def used_of(A, load, n, m):
    u = [0] * m
    for r in range(n):
        if int(A[r]) < m:
            u[int(A[r])] += int(load[r])
    return u


def shed(A, load, aff, S, K, n, m, alive, T, cutoff, max_rows=NEVER, class_cutoffs=None, immovable=None, rows_cap=None,
         lifecycle=False):
    """One call.  Returns (stats, rows, nodes, A_new, aff_new, used_new); the inputs are left alone.  rows_cap None: no listing
    (rows / nodes come back all the same: they are what a listing would hold)."""
    cands, pinned = classify(A, load, aff, S, K, n, m, alive, cutoff, class_cutoffs, immovable)
    sur = sorted(surplus_sequential(load, S, T, cands, pinned))
    B = int(max_rows) if rows_cap is None else min(int(max_rows), int(rows_cap))
    sel = sur[:B]
    used = used_of(A, load, n, m)
    st = {"surplus_rows": len(sur), "surplus_load": sum(int(load[r]) for r in sur), "shed_rows": len(sel),
          "shed_load": sum(int(load[r]) for r in sel),
          "nodes_over_before": sum(1 for j in range(m) if alive[j] and used[j] > int(T[j]))}
    A2, aff2 = A.copy(), aff.copy()
    nodes = [int(A[r]) for r in sel]
    for r in sel:
        used[int(A[r])] -= int(load[r])
        A2[r] = NONE
        if lifecycle:
            aff2[r] = AFF_INACTIVE
    st["nodes_over_after"] = sum(1 for j in range(m) if alive[j] and used[j] > int(T[j]))
    return st, sel, nodes, A2, aff2, used
