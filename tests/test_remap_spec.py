"""tests/spec_remap.py held to its definition: "the existing clean-servers reference over the removed set, then renumber", on
random tables with hidden rows, stale node ids >= m, with and without the row lifecycle; and every illegal shape of the map."""
import numpy as np
import pytest

import spec_remap as spec

NONE, INACTIVE, GONE = spec.NONE, spec.AFF_INACTIVE, spec.NODE_GONE


def table(rng, rows, m, stale=True):
    pool = list(range(m)) + [NONE] + ([m, m + 3, 70000] if stale else [])
    assign = rng.choice(np.array(pool, np.uint32), size=rows)
    aff = rng.choice(np.array(pool + [INACTIVE], np.uint32), size=rows)
    B = rng.choice(np.array(pool + [GONE], np.uint32), size=rows)
    return assign.astype(np.uint32), aff.astype(np.uint32), B.astype(np.uint32)


def random_map(rng, m):
    removed = [j for j in range(m) if rng.random() < 0.4]
    perm = rng.permutation(m - len(removed)).astype(np.uint32)
    map = np.full(m, NONE, np.uint32)
    map[[j for j in range(m) if j not in removed]] = perm
    return map, removed


@pytest.mark.parametrize("lifecycle", [False, True])
@pytest.mark.parametrize("seed", range(8))
def test_remap_is_clean_servers_then_renumber(oracle, seed, lifecycle):
    rng = np.random.default_rng(seed)
    m = int(rng.integers(1, 40))
    rows = int(rng.integers(1, 300))
    n = int(rng.integers(0, rows + 1))
    assign, aff, B = table(rng, rows, m)
    cap = rng.integers(0, 1 << 40, size=m).astype(np.uint64)
    alive = rng.integers(0, 2, size=m).astype(np.uint8)
    map, removed = random_map(rng, m)
    got = spec.remap(assign, aff, n, m, map, lifecycle, B=B, cap=cap, alive=alive)
    # the reference: clean_servers over the visible rows (its count is `evicted`) and over the hidden ones ...
    ref = assign.copy()
    vis, hid = np.ascontiguousarray(ref[:n]), np.ascontiguousarray(ref[n:])
    ev = oracle.clean_servers(vis, m, removed) if n else 0
    if rows > n:
        oracle.clean_servers(hid, m, removed)
    ref = np.concatenate([vis, hid])
    dropped = (ref != assign)
    want_aff = aff.copy()
    if lifecycle:
        want_aff[dropped] = INACTIVE
    # ... then the renumbering, value by value
    def ren(v, gone):
        return int(v) if v >= m else (gone if map[v] == NONE else int(map[v]))
    assert got["evicted"] == ev
    assert got["assign"].tolist() == [ren(v, NONE) for v in ref]
    assert got["aff"].tolist() == [ren(v, NONE) for v in want_aff]
    assert got["B"].tolist() == [ren(v, GONE) for v in B]
    for j in range(m):
        if map[j] != NONE:
            assert got["cap"][map[j]] == cap[j] and got["alive"][map[j]] == alive[j]
    assert len(got["cap"]) == m - len(removed)
    # the feed: a row that only had its node renumbered is as changed or unchanged as before; a row that lost its node is a
    # change (GONE or another old node, NONE) unless the consumer was never told it was placed
    same = (assign == B)
    assert np.array_equal((got["assign"] == got["B"]), (same & ~dropped) | (dropped & (B == NONE)))


def test_stable_map_keeps_the_order():
    assert spec.stable_map(6, [1, 4, 4]).tolist() == [0, NONE, 1, 2, NONE, 3]
    assert spec.stable_map(2, [0, 1]).tolist() == [NONE, NONE]
    assert spec.check_map(6, 4, spec.stable_map(6, [1, 4]))


def test_every_illegal_map_is_refused():
    assert spec.check_map(3, 3, [2, 0, 1]) and spec.check_map(3, 0, [NONE] * 3) and spec.check_map(0, 0, [])
    assert not spec.check_map(3, 2, None)
    assert not spec.check_map(3, 2, [0, 2, NONE])       # a kept value >= m_new
    assert not spec.check_map(3, 2, [0, 0, NONE])       # a value twice
    assert not spec.check_map(3, 2, [0, NONE, NONE])    # fewer than m_new kept
    assert not spec.check_map(3, 2, [0, 1, 1])          # more kept than m_new (a value twice)
    assert not spec.check_map(3, 4, [0, 1, 2])          # m_new > m
    assert not spec.check_map(3, 2, [0, 1])             # not m entries
