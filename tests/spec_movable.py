"""Rule 13 of DESIGN.md section 2 (immovable classes) restated row by row in plain Python from the text: the bounded rebalance
of rule 6 in which a row placed on a live node is PINNED iff it is not an object or its class is immovable.

It shares no code with tests/spec_rebalance_order.py (nor with spec_rebalance.py or the oracle): tests/test_movable_spec.py
checks it against that restatement under the equivalence the rule states — the same table with the affinity of every immovable
object row read as RIO_GP_AFF_INACTIVE — and the GPU is checked against this one.

    rebalance(cur, load, aff, cls, movable, cap, alive, target, max_moves, rounds, order)
        cur / load / aff / cls   per row: node (NONE: unplaced), load, affinity (INACTIVE: not an object), class 0..255
        movable                  flags of the classes 0 .. len(movable) - 1; a class beyond them is movable
        -> (next column, used per node, the nine counters, moves [(row, from, to)] ascending)
"""
NONE = 0xFFFFFFFF
INACTIVE = 0xFFFFFFFE
U64 = (1 << 64) - 1
ROW_ORDER, BY_LOAD = 0, 1


def is_immovable(movable, c):
    return c < len(movable) and not movable[c]


def _three_bit_class(f):
    """free capacity f >= 1 rounded down to three significant bits, as an ordinal (rule 3)"""
    top = f.bit_length() - 1
    below = (f >> (top - 2)) if top >= 2 else (f << (2 - top))
    return 4 * top + (below & 3)


def _surplus_of_node(rows, load, free, order):
    """R1 (row order) or R1' (load ascending, then row) over one node's candidates, given in row order"""
    walk = rows if order == ROW_ORDER else sorted(rows, key=lambda r: (load[r], r))
    out, prefix = [], 0
    for k, r in enumerate(walk):
        prefix += load[r]
        if prefix > free:           # the first that overflows and every later one in that order
            out = list(walk[k:])
            break
    return out


def rebalance(cur, load, aff, cls, movable, cap, alive, target=None, max_moves=None, rounds=2, order=ROW_ORDER):
    n, m = len(cur), len(cap)
    T = [int(t) for t in (cap if target is None else target)]
    live = [j for j in range(m) if alive[j]]
    is_live = [bool(alive[j]) for j in range(m)]

    # R0 with rule 13: pinned iff not an object OR of an immovable class
    pinned_load = [0] * m
    cand = {j: [] for j in live}
    for r in range(n):
        j = cur[r]
        if j == NONE or j >= m or not is_live[j]:
            continue                # unplaced, on a node >= m, on a dead node: takes no part
        if aff[r] == INACTIVE or is_immovable(movable, cls[r]):
            pinned_load[j] += load[r]
        else:
            cand[j].append(r)

    # R1 / R1'
    surplus = []
    for j in live:
        free = max(T[j] - pinned_load[j], 0)
        surplus.extend(_surplus_of_node(cand[j], load, free, order))
    surplus.sort()

    # R2
    selected = surplus if max_moves is None else surplus[:max_moves]
    sel = set(selected)

    # R3: used' = the load of every row that is not selected (the immovable rows among them)
    used = [0] * m
    before = [0] * m
    for r in range(n):
        j = cur[r]
        if j != NONE and j < m:
            before[j] += load[r]
            if r not in sel:
                used[j] += load[r]
    nxt = list(cur)
    waiting = list(selected)
    for _ in range(rounds):
        if not waiting:
            break
        free = [(T[j] - used[j]) if is_live[j] and T[j] > used[j] else 0 for j in range(m)]
        order_nodes = sorted((j for j in range(m) if free[j] > 0), key=lambda j: (-_three_bit_class(free[j]), j))
        C = [0]
        for j in order_nodes:
            C.append(min(C[-1] + free[j], U64))
        Q, still, gains = 0, [], [0] * m
        for r in waiting:
            took = None
            for k in range(len(order_nodes)):       # the interval [C[k], C[k+1]) that contains Q
                if C[k] <= Q < C[k + 1]:
                    if Q + load[r] <= C[k + 1]:
                        took = order_nodes[k]
                    break
            Q += load[r]
            if took is None:
                still.append(r)
            else:
                nxt[r] = took
                gains[took] += load[r]
        for j in range(m):
            used[j] += gains[j]
        waiting = still

    # R4: what found no node keeps its node
    for r in waiting:
        used[cur[r]] += load[r]
    moves = [(r, cur[r], nxt[r]) for r in selected if nxt[r] != cur[r]]
    stats = {
        "surplus_rows": len(surplus), "surplus_load": sum(load[r] for r in surplus),
        "selected_rows": len(selected), "selected_load": sum(load[r] for r in selected),
        "moved_rows": len(moves), "moved_load": sum(load[r] for r, _, _ in moves),
        "stayed_rows": len(waiting),
        "nodes_over_before": sum(1 for j in live if before[j] > T[j]),
        "nodes_over_after": sum(1 for j in live if used[j] > T[j]),
    }
    return nxt, used, stats, moves
