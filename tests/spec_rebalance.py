"""The bounded rebalance of DESIGN.md section 2 ("rebalance", R0-R4), restated row by row in plain Python from the text.

It shares no code with the oracle (oracle/placement_oracle.c) or with tests/spec_tick.py: the tests check it against the
two-tick composition of the oracle (tests/rebalance_ref.py) and the GPU against both.
"""
NONE = 0xFFFFFFFF
INACTIVE = 0xFFFFFFFE
INF = 0xFFFFFFFFFFFFFFFF


def capacity_class(f):
    """f > 0 rounded down to three significant bits, as an ordinal: 4 * floor(log2 f) + the two bits below the leading one."""
    e = f.bit_length() - 1
    mant = (f >> (e - 2)) & 3 if e >= 2 else (f << (2 - e)) & 3
    return 4 * e + mant


def rebalance(cur, load, aff, cap, alive, target=None, max_moves=None, rounds=2):
    """Returns (next column, used of it, stats dict, moves [(row, from, to)] in row order)."""
    n, m = len(cur), len(cap)
    T = list(cap) if target is None else list(target)

    def live(j):
        return j < m and alive[j]

    # R0: candidates (objects on a live node) per node in row order; pinned load (non-objects on a live node)
    pinned = [0] * m
    cands = [[] for _ in range(m)]
    for i in range(n):
        c = cur[i]
        if c != NONE and live(c):
            if aff[i] == INACTIVE:
                pinned[c] += load[i]
            else:
                cands[c].append(i)
    # R1: strict prefix cut against free = T -sat pinned
    surplus = []
    for j in range(m):
        if not live(j):
            continue
        free = T[j] - pinned[j] if T[j] > pinned[j] else 0
        run, over = 0, False
        for i in cands[j]:
            run += load[i]
            if over or run > free:
                over = True
                surplus.append(i)
    surplus.sort()
    # R2: the first B in row order
    selected = surplus if max_moves is None else surplus[:max_moves]
    chosen = set(selected)
    # R3: water-fill against free = T -sat used' (used' = the load of every row that is not selected), live nodes only
    used2 = [0] * m
    for i in range(n):
        if cur[i] != NONE and cur[i] < m and i not in chosen:
            used2[cur[i]] += load[i]
    nxt = list(cur)
    pending = list(selected)
    for _ in range(rounds):
        if not pending:
            break
        free = {j: T[j] - used2[j] for j in range(m) if live(j) and T[j] > used2[j]}
        order = sorted(free, key=lambda j: (-capacity_class(free[j]), j))
        bounds = [0]
        for j in order:
            bounds.append(min(bounds[-1] + free[j], INF))
        q, left = 0, []
        for i in pending:
            target_node = None
            if order and q < bounds[-1]:
                k = 0
                while k + 1 < len(order) and bounds[k + 1] <= q:
                    k += 1
                if q + load[i] <= bounds[k + 1]:
                    target_node = order[k]
            q += load[i]
            if target_node is None:
                left.append(i)
            else:
                nxt[i] = target_node
                used2[target_node] += load[i]  # counts from the next round on: `free` of this round is fixed
        pending = left
    # R4: what found no node keeps its node (nxt[i] == cur[i] already)
    used = [0] * m
    before = [0] * m
    for i in range(n):
        if nxt[i] != NONE and nxt[i] < m:
            used[nxt[i]] += load[i]
        if cur[i] != NONE and cur[i] < m:
            before[cur[i]] += load[i]
    moves = [(i, cur[i], nxt[i]) for i in range(n) if nxt[i] != cur[i]]
    st = {
        "surplus_rows": len(surplus), "surplus_load": sum(load[i] for i in surplus),
        "selected_rows": len(selected), "selected_load": sum(load[i] for i in selected),
        "moved_rows": len(moves), "moved_load": sum(load[i] for i, _, _ in moves),
        "stayed_rows": len(pending),
        "nodes_over_before": sum(1 for j in range(m) if live(j) and before[j] > T[j]),
        "nodes_over_after": sum(1 for j in range(m) if live(j) and used[j] > T[j]),
    }
    return nxt, used, st, moves
