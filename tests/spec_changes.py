"""The change feed restated in plain numpy / dicts (include/rio_gpu_placement.h "change feed"; include/rio_gpu_object_placement.h
rio_op_changes).  Dense layer: a checkpoint column B, the column A the call sees, n rows, a cap and the peek flag give the
listing and the new B.  String layer: how a mirror of rio_op_snapshot applies one listing."""
import numpy as np

NONE = 0xFFFFFFFF


def dense(B, A, n, cap=None, peek=False):
    """-> (rows, old, new, total, B'): the first min(total, cap) rows r < n with A[r] != B[r], ascending, with B[r] and A[r];
    total = every such row; B' = B advanced for exactly the listed rows (unchanged under peek).  Rows >= n keep their B."""
    A = np.asarray(A, np.uint32)
    B = np.array(B, np.uint32, copy=True)
    rows = np.flatnonzero(A[:n] != B[:n]).astype(np.uint32)
    total = int(len(rows))
    k = rows if cap is None else rows[:int(cap)]
    old, new = B[k].copy(), A[k].copy()
    if not peek:
        B[k] = A[k]
    return k, old, new, total, B


def apply(mirror, full, entries, strict=True):
    """One rio_op_changes listing applied to a mirror {(struct_name, object_id): address}; returns the new mirror.  strict: every
    entry's old address is what the mirror holds for the key (None: absent), deletes come before upserts, and a full listing
    holds no delete."""
    m = {} if full else dict(mirror)
    seen_upsert = False
    for ty, oid, old, new in entries:
        key = (ty, oid)
        if strict:
            assert m.get(key) == old, (key, m.get(key), old, new)
            if new is None:
                assert not seen_upsert, "a delete after an upsert"
                assert not full, "a delete in a full listing"
        if new is None:
            assert old is not None
            m.pop(key, None)
        else:
            seen_upsert = True
            m[key] = new
    return m


def as_set(mirror):
    return {(k[0], k[1], v) for k, v in mirror.items()}
