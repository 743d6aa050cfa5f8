"""Tables for the pressure-shedding tests (rule 14): one generator for the CPU and the GPU tests, and the conditions under which
a table checks something (an over node, a surplus, a cut in the middle of a tie group)."""
import numpy as np

import spec_shed as spec

NONE = spec.NONE
INACTIVE = spec.AFF_INACTIVE
NEVER = spec.NEVER

# layout -> (stamps drawn from, cutoff): few distinct epochs (large tie groups, one of them at the cutoff: pinned), all equal
# (a pure row-order cut), all 0 (never seen), spread over all 32 bits (every digit decides; 0xFFFFFFFF is below no cutoff)
LAYOUTS = {
    "few": ([10, 11, 12, 13], 13),
    "equal": ([7], 8),
    "zero": ([0], 1),
    "spread": (None, 0xFFFFFFFF),
}
TIE_LAYOUTS = ("few", "equal", "zero")


def table(seed, n, m, layout, heavy=False, dead=True, classes=0, squeeze=0.6, over=None):
    """A, load, aff, S, K, alive, T, cutoff.  squeeze: T = squeeze * used on the nodes meant to be over, ~0 on every fourth of
    the others, used + 5 on the rest; every seventh over node gets T = 1: there the pinned load alone may exceed it.
    over: at most that many nodes are squeezed (the live nodes of the lowest ids that hold a candidate)."""
    rng = np.random.default_rng(seed)
    A = rng.integers(0, m, n).astype(np.uint32)
    A[rng.random(n) < 0.05] = NONE
    if heavy:
        load = rng.choice(np.array([0, 1, 7, 1000, 0xFFFFFFFF], np.uint32), n)
    else:
        load = rng.integers(0, 40, n).astype(np.uint32)
    aff = rng.integers(0, m, n).astype(np.uint32)
    aff[rng.random(n) < 0.05] = INACTIVE
    vals, cutoff = LAYOUTS[layout]
    if vals is None:
        S = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        S[rng.random(n) < 0.02] = 0xFFFFFFFF
    else:
        S = rng.choice(np.array(vals, np.uint32), n)
    K = rng.integers(0, classes + 2, n).astype(np.uint8) if classes else np.zeros(n, np.uint8)
    alive = np.ones(m, np.uint8)
    if dead and m >= 3:
        alive[m // 2] = 0
    used = spec.used_of(A, load, n, m)
    has_cand = np.zeros(m, bool)
    c = (A < m) & (aff != INACTIVE) & (load >= 1) & (S < cutoff)
    has_cand[A[c]] = True
    T = np.empty(m, np.uint64)
    k = 0
    for j in range(m):
        if has_cand[j] and alive[j] and (over is None or k < over):
            T[j] = 1 if k % 7 == 6 else int(used[j] * squeeze)
            k += 1
        else:
            T[j] = NEVER if j % 4 == 0 else used[j] + 5
    return A, load, aff, S, K, alive, T, cutoff


def facts(A, load, aff, S, K, n, m, alive, T, cutoff, class_cutoffs=None, immovable=None):
    """What the spec says about a table before anything is compared with it: (over nodes, surplus rows, nodes whose cut row is
    neither the first of its ties nor absent)."""
    cands, pinned = spec.classify(A, load, aff, S, K, n, m, alive, cutoff, class_cutoffs, immovable)
    thr = spec.thresholds(load, S, T, cands, pinned)
    sur = spec.surplus_threshold(S, cands, thr)
    mid = 0
    for j, (sigma, cutrow, _rem) in thr.items():
        ties = [r for r in cands[j] if int(S[r]) == sigma]
        mid += cutrow is not None and cutrow != ties[0] and cutrow <= ties[-1]
    return len(thr), len(sur), mid
