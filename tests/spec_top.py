"""The hot-object report restated in plain numpy (include/rio_gpu_placement.h "hot-object report"; DESIGN.md section 2 rule 11,
frozen): which rows rio_gp_top_rows counts and which it lists, in which order.  String layer: which keys
rio_op_hottest_objects lists, from a model's placements and loads."""
import numpy as np

NONE = 0xFFFFFFFF
BY_HITS, PLACED, ON_NODE = 1, 2, 4
TOP_MAX = 4096


def top_rows(A, load, H, n, flags=0, node=0, min_key=0, cap=TOP_MAX):
    """-> (rows, keys, nodes, n_candidates, key_sum).  K = H under BY_HITS (None: all zero), else load.  Row r is a candidate iff
    r < n, K[r] >= min_key, A[r] != NONE under PLACED (raw values) and A[r] == node under ON_NODE.  The listing is the first
    min(n_candidates, cap) candidates in the order (K descending, r ascending); n_candidates and key_sum cover every candidate."""
    A = np.asarray(A, np.uint32)[:n]
    if flags & BY_HITS:
        K = np.zeros(n, np.uint32) if H is None else np.asarray(H, np.uint32)[:n]
    else:
        K = np.asarray(load, np.uint32)[:n]
    cand = K >= np.uint32(min_key)
    if flags & PLACED:
        cand &= A != np.uint32(NONE)
    if flags & ON_NODE:
        cand &= A == np.uint32(node)
    r = np.flatnonzero(cand)
    # np.lexsort: the LAST key is the primary one — descending K (ascending of its negation in int64), then ascending r
    order = np.lexsort((r, -K[r].astype(np.int64)))
    rows = r[order][:int(cap)].astype(np.uint32)
    return rows, K[rows].copy(), A[rows].copy(), int(len(r)), int(K[r].astype(np.uint64).sum())


def op_hottest(rows, where, load, address=None, min_load=0, cap=TOP_MAX):
    """String layer: rows = the keys in row order (the order in which they first reached the table), where {key: address} of
    the placed ones, load {key: load} -> ([(struct_name, object_id, address, load)], n_candidates): the placed keys (on `address`
    if given) with load >= min_load, load descending, keys of equal load in row order."""
    sel = [(k, where[k], load[k]) for k in rows if k in where and (address is None or where[k] == address) and load[k] >= min_load]
    order = sorted(range(len(sel)), key=lambda i: (-sel[i][2], i))
    return [(sel[i][0][0], sel[i][0][1], sel[i][1], sel[i][2]) for i in order[:cap]], len(sel)
