"""The bounded rebalance ("rebalance") as two ticks of the existing oracle with cap = T, and the random
tables the rebalance tests draw.  Shared by the CPU and the GPU tests; needs pyoracle built (the `oracle` fixture)."""
import numpy as np

NONE = 0xFFFFFFFF
INACTIVE = 0xFFFFFFFE
INF = 0xFFFFFFFFFFFFFFFF


def rebalance(cur, load, aff, cap, alive, target=None, max_moves=None, rounds=2):
    """Returns (next column uint32, used uint64 [m], stats dict, rows, from, to) — moves in row order."""
    import pyoracle
    cur = np.asarray(cur, np.uint32)
    load = np.asarray(load, np.uint32)
    aff = np.asarray(aff, np.uint32)
    cap = np.asarray(cap, np.uint64)
    alive = np.asarray(alive, np.uint8)
    m = len(cap)
    T = cap if target is None else np.asarray(target, np.uint64)
    on = (cur != NONE) & (cur < m)
    live = on.copy()
    live[on] = alive[cur[on]] != 0
    obj = aff != INACTIVE
    pinned, cand = live & ~obj, live & obj
    # tick A: pinned rows kept, candidates claim their own node, no spill round: the candidates left NONE are the surplus
    cur_a = np.where(pinned, cur, NONE).astype(np.uint32)
    aff_a = np.where(cand, cur, INACTIVE).astype(np.uint32)
    nxt_a, _, _ = pyoracle.tick(cur_a, load, aff_a, T, alive, rounds=0, flags=0)
    surplus = cand & (nxt_a == NONE)
    idx = np.flatnonzero(surplus)
    sel = np.zeros(len(cur), bool)
    sel[idx if max_moves is None else idx[:max_moves]] = True
    # tick B: every other row on a live node kept, the selected rows spill only
    cur_b = np.where(live & ~sel, cur, NONE).astype(np.uint32)
    aff_b = np.where(sel, NONE, INACTIVE).astype(np.uint32)
    nxt_b, _, _ = pyoracle.tick(cur_b, load, aff_b, T, alive, rounds=rounds, flags=0)
    nxt = cur.copy()
    placed = sel & (nxt_b != NONE)
    nxt[placed] = nxt_b[placed]  # R4: the others keep their node
    used = pyoracle.recompute_used(nxt, load, m)
    before = pyoracle.recompute_used(cur, load, m)
    moved = np.flatnonzero(nxt != cur)
    lv = alive.astype(bool)
    st = {
        "surplus_rows": int(surplus.sum()), "surplus_load": int(load[surplus].sum(dtype=np.uint64)),
        "selected_rows": int(sel.sum()), "selected_load": int(load[sel].sum(dtype=np.uint64)),
        "moved_rows": len(moved), "moved_load": int(load[moved].sum(dtype=np.uint64)),
        "stayed_rows": int((sel & (nxt_b == NONE)).sum()),
        "nodes_over_before": int((lv & (before > T)).sum()), "nodes_over_after": int((lv & (used > T)).sum()),
    }
    return nxt, used, st, moved.astype(np.uint32), cur[moved], nxt[moved]


def random_table(rng, n, m, target_kind="tight", dead=True, pinned=True, unplaced=True, big_nodes=True, max_load=50):
    """A placed table with the corner cases of R0: pinned rows, dead nodes, unplaced rows, node ids >= m; and a target."""
    cur = rng.integers(0, m, n).astype(np.uint32)
    if big_nodes and n:
        cur[rng.random(n) < 0.03] = np.uint32(m + int(rng.integers(0, 3)))
    if unplaced:
        cur[rng.random(n) < 0.1] = NONE
    load = rng.integers(0, max_load + 1, n).astype(np.uint32)
    aff = rng.integers(0, m, n).astype(np.uint32)
    if pinned:
        aff[rng.random(n) < 0.1] = INACTIVE
    aff[rng.random(n) < 0.03] = NONE
    alive = np.ones(m, np.uint8)
    if dead and m > 1:
        alive[rng.random(m) < 0.15] = 0
    per = int(load.sum()) // max(m, 1)
    if target_kind == "zero":
        T = np.zeros(m, np.uint64)
    elif target_kind == "inf":
        T = np.full(m, INF, np.uint64)
    else:  # tight: around the mean, some nodes well below, some unbounded
        T = rng.integers(max(per // 2, 0), per + per // 4 + 2, m).astype(np.uint64)
        T[rng.random(m) < 0.05] = np.uint64(INF)
    return cur, load, aff, alive, T
