"""Random tables for the tests of rule 13 (immovable classes): tests/test_movable_spec.py, tests/test_gpu_movable.py.

Every table mixes what the rule distinguishes: objects of movable and of immovable classes (class 255 among them, and classes
at or above the table's n_classes, which are movable whatever the array would say), non-object rows, unplaced rows, zero loads,
dead nodes, rows on a node id >= m, and targets around the mean load so that most nodes are over.  `plant` puts an immovable
row exactly where the plain rule cuts a node, and gives one node immovable load beyond its target."""
import numpy as np

NONE = 0xFFFFFFFF
INACTIVE = 0xFFFFFFFE
INF = 0xFFFFFFFFFFFFFFFF


def random_table(rng, n, m, frac_immovable=0.3, n_classes=None, max_load=9, dead=True, plant=True):
    """-> dict(cur, load, aff, cls, movable, alive, T) as numpy arrays (movable: n_classes uint8 flags)."""
    n_classes = int(rng.integers(1, 257)) if n_classes is None else n_classes
    used_classes = np.unique(np.concatenate([rng.integers(0, 256, 12), [0, 255, min(n_classes, 255), max(n_classes - 1, 0)]]))
    cls = rng.choice(used_classes, n).astype(np.uint8)
    movable = (rng.random(n_classes) >= frac_immovable).astype(np.uint8)
    cur = rng.integers(0, m, n).astype(np.uint32)
    cur[rng.random(n) < 0.05] = NONE
    if n > 8:
        cur[rng.random(n) < 0.01] = m + 1            # left behind by a smaller node table
    aff = rng.integers(0, m, n).astype(np.uint32)
    aff[rng.random(n) < 0.1] = INACTIVE              # non-object rows mixed in
    load = rng.integers(0, max_load + 1, n).astype(np.uint32)
    load[rng.random(n) < 0.1] = 0
    alive = np.ones(m, np.uint8)
    if dead and m > 2:
        alive[rng.integers(0, m)] = 0
    per = max(int(load.sum(dtype=np.uint64)) // m, 1)
    T = rng.integers(per // 2, per + per // 2 + 1, m).astype(np.uint64)   # 0.5 .. 1.5 times the mean
    if m > 3:
        T[rng.integers(0, m)] = INF
    t = dict(cur=cur, load=load, aff=aff, cls=cls, movable=movable, alive=alive, T=T)
    if plant and n >= 5:
        _plant(rng, t, m)
    return t


def immovable_rows(t):
    """mask of the rows whose class is immovable under t's table"""
    k = t["cls"].astype(np.int64)
    mv = np.ones(256, np.uint8)
    mv[:len(t["movable"])] = t["movable"]
    return mv[k] == 0


def _plant(rng, t, m):
    cur, load, aff, cls, movable, alive, T = (t[k] for k in ("cur", "load", "aff", "cls", "movable", "alive", "T"))
    imm = np.flatnonzero(movable == 0)
    if not len(imm):
        return
    c = int(imm[0])
    live = np.flatnonzero(alive)
    # an immovable row exactly at the position of the plain rule's row-order cut of one node
    j = int(live[0])
    rows = np.flatnonzero((cur == j) & (aff != INACTIVE))
    pin = int(load[(cur == j) & (aff == INACTIVE)].sum())
    if T[j] != INF and len(rows):
        run = np.cumsum(load[rows].astype(np.int64))
        over = np.flatnonzero(run > max(int(T[j]) - pin, 0))
        if len(over):
            r = rows[over[0]]
            cls[r] = c
            load[r] = max(int(load[r]), 1)
    # a node whose immovable load alone exceeds its target
    if len(live) > 1:
        j = int(live[-1])
        rows = np.flatnonzero((cur == j) & (aff != INACTIVE))
        if len(rows) >= 2 and T[j] != INF:
            cls[rows[0]] = c
            load[rows[0]] = np.uint32(min(int(T[j]) + 1, 0xFFFFFFFF))
