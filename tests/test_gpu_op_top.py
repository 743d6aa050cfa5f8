"""The hot-object report through the string layer on the MI355X (rio_op_hottest_objects over rio_gp_top_rows), 600 keys on 6
members: every report — per address and over all addresses, with a floor and a limit — against what rio_op_snapshot and
rio_op_get_object_load say of the same provider, ordered by the model (tests/spec_top.py, op_hottest); after set_object_load, after
a tracked fold, after an expiry and after clean_server."""
import numpy as np
import pytest

import spec_top as spec


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


def check_all(op, keys, addrs):
    """every report against snapshot + get_object_load; returns the number of placed keys"""
    where = {(t, i): a for t, i, a in op.snapshot()}
    load = {k: op.get_object_load(*k) for k in keys}
    assert all(v is not None for v in load.values())
    for address in [None] + addrs + ["10.9.9.9:1"]:
        for lo, cap in ((0, 4096), (0, 7), (2, 50), (0, 0), (1 << 20, 10)):
            want = spec.op_hottest(keys, where, load, address, lo, cap)
            assert op.hottest_objects(address, lo, cap) == want, (address, lo, cap)
    return len(where)


@pytest.mark.gpu
def test_reports_follow_loads_folds_expiry_and_clean_server(gp):
    n, m = 600, 6
    op = gp.GpuObjectPlacement(max_objects=2048, max_nodes=8)
    try:
        addrs = ["10.0.0.%d:5000" % k for k in range(m)]
        for a in addrs:
            op.set_member(a, True)
        keys = [("Svc%d" % (k % 3), "o%d" % k) for k in range(n - 1)] + [("N\0", "x\0y")]     # (row order: the order of arrival)
        op.update_batch(keys, [addrs[(k * 7) % m] for k in range(n)])
        assert op.hottest_objects(max_objects=3) == ([(t, i, addrs[(k * 7) % m], 1) for k, (t, i) in enumerate(keys[:3])], n)
        assert check_all(op, keys, addrs) == n
        # -- after set_object_load: a few heavy keys, many ties --
        rng = np.random.default_rng(2)
        for k in rng.permutation(n)[:120]:
            op.set_object_load(*keys[k], int(rng.choice([0, 2, 2, 5, 900, 70_000])))
        op.set_object_load(*keys[-1], 4_000_000_000)
        assert op.hottest_objects(max_objects=1)[0] == [("N\0", "x\0y", addrs[((n - 1) * 7) % m], 4_000_000_000)]
        assert check_all(op, keys, addrs) == n
        # -- after a tracked fold: requests become loads --
        op.set_load_tracking(True)
        hot = (rng.zipf(1.3, 4000) - 1) % n
        op.lookup_batch([keys[i] for i in hot])
        op.set_load_tracking(False)
        changed, folded = op.fold_loads(32768, 3, 1, 1_000_000)
        assert folded == 4000 and changed > 0
        assert check_all(op, keys, addrs) == n
        # -- after an expiry: the expired keys are no longer placed, so no longer reported --
        op.set_clock(5)
        op.lookup_batch(keys[::2])
        out, idle = op.expire(5, 100)
        assert len(out) == 100 and idle == n // 2
        gone = {(t, i) for t, i, a in out}
        placed = check_all(op, keys, addrs)
        assert placed == n - 100
        assert not gone & {(t, i) for t, i, a, l in op.hottest_objects()[0]}
        # -- after clean_server: the server reports nothing, the others are as they were --
        op.clean_server(addrs[2])
        assert op.hottest_objects(addrs[2]) == ([], 0)
        assert check_all(op, keys, addrs) < placed
        with pytest.raises(gp.ObjectPlacementError) as e:
            op.hottest_objects(max_objects=4097)
        assert e.value.rc == gp.EINVAL
    finally:
        op.close()
