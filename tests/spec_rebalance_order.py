"""The bounded rebalance of DESIGN.md section 2 ("rebalance") with the ordering of its cut as a parameter: R0-R4 with R1
(order = 0, row order) or R1' (order = 1, by load), restated row by row in plain Python from the text.

It shares no code with the oracle, with tests/spec_rebalance.py or with tests/rebalance_order_ref.py: the tests check it
against the two-tick composition of the oracle (tests/rebalance_order_ref.py) and the GPU against both.  `threshold_form`
restates the (tau, cutrow) form of R1' that the kernels evaluate; `cut_surplus` is the sorted-prefix definition.
"""
import bisect

NONE = 0xFFFFFFFF
INACTIVE = 0xFFFFFFFE
INF = 0xFFFFFFFFFFFFFFFF
ROW_ORDER, BY_LOAD = 0, 1


def capacity_class(f):
    """f > 0 rounded down to three significant bits, as an ordinal: 4 * floor(log2 f) + the two bits below the leading one."""
    e = f.bit_length() - 1
    mant = (f >> (e - 2)) & 3 if e >= 2 else (f << (2 - e)) & 3
    return 4 * e + mant


def candidates(cur, load, aff, alive, m):
    """R0: (pinned load per node, candidate rows per node in row order) over the live nodes."""
    pinned = [0] * m
    cands = [[] for _ in range(m)]
    for i in range(len(cur)):
        c = cur[i]
        if c != NONE and c < m and alive[c]:
            if aff[i] == INACTIVE:
                pinned[c] += load[i]
            else:
                cands[c].append(i)
    return pinned, cands


def cut_surplus(rows, load, free, order):
    """R1 / R1' for one node: its candidates `rows` (row order) in the order of the rule, kept while the inclusive prefix of
    their loads is <= free; the first that overflows and every later one in that order are surplus."""
    seq = list(rows) if order == ROW_ORDER else sorted(rows, key=lambda i: (load[i], i))
    run, over, out = 0, False, []
    for i in seq:
        run += load[i]
        if over or run > free:
            over = True
            out.append(i)
    return out


def threshold_form(rows, load, free):
    """The (tau, cutrow) pair of R1' for one node whose candidates weigh more than free, and the surplus it defines:
    tau = the load of the first overflowing candidate, rem = free - the load of the candidates below tau, c = rem // tau,
    cutrow = the row of the (c + 1)-th candidate of load tau in row order; surplus iff load > tau or (load == tau and
    row >= cutrow).  None where nothing overflows."""
    if sum(load[i] for i in rows) <= free:
        return None
    tau = None
    for v in sorted(set(load[i] for i in rows)):
        if v and sum(load[i] for i in rows if load[i] <= v) > free:
            tau = v
            break
    rem = free - sum(load[i] for i in rows if load[i] < tau)
    c = rem // tau
    ties = [i for i in rows if load[i] == tau]
    cutrow = ties[c]
    surplus = [i for i in rows if load[i] > tau or (load[i] == tau and i >= cutrow)]
    return tau, cutrow, surplus


def rebalance(cur, load, aff, cap, alive, target=None, max_moves=None, rounds=2, order=ROW_ORDER):
    """Returns (next column, used of it, stats dict, moves [(row, from, to)] in row order)."""
    n, m = len(cur), len(cap)
    T = list(cap) if target is None else list(target)

    def live(j):
        return j < m and alive[j]

    pinned, cands = candidates(cur, load, aff, alive, m)
    # R1 / R1': the cut per live node against free = T -sat pinned
    surplus = []
    for j in range(m):
        if live(j):
            surplus += cut_surplus(cands[j], load, T[j] - pinned[j] if T[j] > pinned[j] else 0, order)
    surplus.sort()
    # R2: the first B in row order
    selected = surplus if max_moves is None else surplus[:max_moves]
    chosen = set(selected)
    # R3: water-fill in row order against free = T -sat used' (used' = the load of every row that is not selected)
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
        nodes = sorted(free, key=lambda j: (-capacity_class(free[j]), j))
        bounds = [0]
        for j in nodes:
            bounds.append(min(bounds[-1] + free[j], INF))
        q, left, admitted = 0, [], []
        for i in pending:
            to = None
            if nodes and q < bounds[-1]:
                k = bisect.bisect_right(bounds, q) - 1   # the last k with bounds[k] <= q (q < bounds[-1]: k < len(nodes))
                if q + load[i] <= bounds[k + 1]:
                    to = nodes[k]
            q += load[i]
            if to is None:
                left.append(i)
            else:
                nxt[i] = to
                admitted.append((to, load[i]))
        for to, l in admitted:   # counts from the next round on: `free` of this round is fixed
            used2[to] += l
        pending = left
    # R4: what found no node keeps its node (nxt[i] == cur[i] already)
    used, before = [0] * m, [0] * m
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
