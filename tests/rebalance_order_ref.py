"""The bounded rebalance with a load-ordered cut (rule 6, R1') as two ticks of the existing oracle with
cap = T.  Tick A — every candidate claims its own node, no spill round — runs over the rows permuted into (load, row) order and
is un-permuted afterwards: the oracle admits claims in row order, so the claim order per node is then (load, row), and the
candidates it leaves without a node are the surplus of R1'.  Tick B and R4 are those of tests/rebalance_ref.py.  order = 0 is
tests/rebalance_ref.py itself.  Shared by the CPU and the GPU tests; needs pyoracle built (the `oracle` fixture)."""
import numpy as np

import rebalance_ref

NONE = 0xFFFFFFFF
INACTIVE = 0xFFFFFFFE
INF = 0xFFFFFFFFFFFFFFFF
ROW_ORDER, BY_LOAD = 0, 1


def surplus_mask(cur, load, aff, T, alive, order=BY_LOAD, perm=None):
    """(surplus, live, pinned, cand) boolean row masks: tick A.  perm: the claim order of tick A from a caller that wants a
    wrong one (the faults of tests/fake_rio_gp.py); None: the order of the rule."""
    import pyoracle
    m = len(T)
    on = (cur != NONE) & (cur < m)
    live = on.copy()
    live[on] = alive[cur[on]] != 0
    obj = aff != INACTIVE
    pinned, cand = live & ~obj, live & obj
    n = len(cur)
    if perm is None:
        perm = np.lexsort((np.arange(n), load)) if order == BY_LOAD else np.arange(n)
    cur_a = np.where(pinned, cur, NONE).astype(np.uint32)
    aff_a = np.where(cand, cur, INACTIVE).astype(np.uint32)
    nxt_p, _, _ = pyoracle.tick(np.ascontiguousarray(cur_a[perm]), np.ascontiguousarray(load[perm]),
                                np.ascontiguousarray(aff_a[perm]), T, alive, rounds=0, flags=0)
    nxt_a = np.empty(n, np.uint32)
    nxt_a[perm] = nxt_p
    return cand & (nxt_a == NONE), live, pinned, cand


def rebalance(cur, load, aff, cap, alive, target=None, max_moves=None, rounds=2, order=BY_LOAD, perm=None):
    """Returns (next column uint32, used uint64 [m], stats dict, rows, from, to) — moves in row order.  perm: see surplus_mask."""
    import pyoracle
    if order == ROW_ORDER:
        return rebalance_ref.rebalance(cur, load, aff, cap, alive, target, max_moves, rounds)
    cur = np.asarray(cur, np.uint32)
    load = np.asarray(load, np.uint32)
    aff = np.asarray(aff, np.uint32)
    cap = np.asarray(cap, np.uint64)
    alive = np.asarray(alive, np.uint8)
    m = len(cap)
    T = cap if target is None else np.asarray(target, np.uint64)
    surplus, live, _, _ = surplus_mask(cur, load, aff, T, alive, order, perm)
    idx = np.flatnonzero(surplus)
    sel = np.zeros(len(cur), bool)
    sel[idx if max_moves is None else idx[:max_moves]] = True
    # tick B: every other row on a live node kept, the selected rows spill only (row order)
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


def skewed_loads(rng, n, hi=(1 << 32) - 1, a=1.3):
    """Zipf-like u32 loads clipped at `hi`, with zeros: every digit of a threshold search decides somewhere."""
    l = np.minimum(rng.zipf(a, n).astype(np.float64), float(hi)).astype(np.uint64)
    l[rng.random(n) < 0.1] = 0
    if n:
        big = rng.random(n) < 0.02
        l[big] = rng.integers(min(1 << 16, hi), hi, int(big.sum()), dtype=np.uint64, endpoint=True)
    return l.astype(np.uint32)
