"""Node removal restated in plain numpy (include/rio_gpu_placement.h rio_gp_remap_nodes; DESIGN.md section 2 rule 8): exactly
rio_gp_clean_servers over the removed nodes, then a renumbering, over every row the handle holds."""
import numpy as np

NONE = 0xFFFFFFFF
AFF_INACTIVE = 0xFFFFFFFE
NODE_GONE = 0xFFFFFFFC


def check_map(m, m_new, map):
    """True when `map` (m entries) is a legal argument: the kept entries (!= NONE) hit every value of 0 .. m_new-1 exactly once."""
    if map is None or len(map) != m or m_new > m:
        return False
    kept = np.asarray(map, np.uint32)
    kept = kept[kept != NONE]
    return len(kept) == m_new and bool(np.array_equal(np.sort(kept), np.arange(m_new, dtype=np.uint32)))


def stable_map(m, removed):
    """The map that drops `removed` and keeps the other nodes in their order."""
    keep = np.ones(m, bool)
    keep[np.asarray(sorted(set(removed)), np.int64)] = False
    map = np.full(m, NONE, np.uint32)
    map[keep] = np.arange(int(keep.sum()), dtype=np.uint32)
    return map


def _renumber(col, m, map, gone_value):
    col = np.array(col, np.uint32, copy=True)
    known = col < m
    new = np.asarray(map, np.uint32)[col[known]]
    new[new == NONE] = gone_value
    col[known] = new
    return col


def remap(assign, aff, n, m, map, lifecycle, B=None, cap=None, alive=None):
    """assign / aff / B: every row the handle holds (rows >= n are the hidden ones).  -> dict(assign, aff, B, cap, alive,
    evicted): the columns after the call, the node table moved to the new ids, the rows < n that lost their node."""
    map = np.asarray(map, np.uint32)
    assign = np.asarray(assign, np.uint32)
    aff = np.asarray(aff, np.uint32)
    lost = np.zeros(len(assign), bool)
    known = assign < m
    lost[known] = map[assign[known]] == NONE
    out = {"evicted": int(lost[:n].sum())}
    out["assign"] = _renumber(assign, m, map, NONE)
    a2 = _renumber(aff, m, map, NONE)
    if lifecycle:
        a2[lost] = AFF_INACTIVE
    out["aff"] = a2
    out["B"] = None if B is None else _renumber(B, m, map, NODE_GONE)
    kept = np.flatnonzero(map != NONE)
    order = kept[np.argsort(map[kept], kind="stable")]   # old id of new id 0, 1, ...
    out["cap"] = None if cap is None else np.asarray(cap, np.uint64)[order]
    out["alive"] = None if alive is None else np.asarray(alive, np.uint8)[order]
    return out
