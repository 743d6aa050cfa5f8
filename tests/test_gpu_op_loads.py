"""Measured load through the string layer on the MI355X (rio_op_set_load_tracking / rio_op_fold_loads / rio_op_get_object_load
over rio_gp_hits_merge and rio_gp_load_fold), 2 000 keys on 8 members: skewed requests of every counting form, then a fold —
every key's load is the model's (tests/spec_loads.py); then rio_op_rebalance moves exactly what the rebalance reference
(tests/rebalance_ref.py) moves over those loads; the host shadow answered lookups all along, and answers them after the fold."""
import numpy as np
import pytest

import rebalance_ref
import spec_loads as spec

NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


@pytest.mark.gpu
def test_skewed_requests_fold_into_loads_and_the_rebalance_acts_on_them(gp):
    n, m = 2000, 8
    op = gp.GpuObjectPlacement(max_objects=4096, max_nodes=16)
    try:
        addrs = ["10.0.0.%d:5000" % k for k in range(m)]
        for a in addrs:
            op.set_member(a, True, 40_000)
        keys = [("Svc%d" % (k % 3), "o%d" % k) for k in range(n - 1)] + [("N\0", "x\0y")]
        home = {key: addrs[k % 3] for k, key in enumerate(keys)}         # everything on the first three servers
        op.update_batch(keys, [home[k] for k in keys])
        md = spec.OpLoads()
        assert op.fold_loads(65536, 1) == (0, 0)                         # tracking is off: nothing was counted
        op.set_load_tracking(True)
        md.on = True
        rng = np.random.default_rng(4)
        hot = (rng.zipf(1.2, 30_000) - 1) % n                            # skewed: a few keys take most requests
        for lo in range(0, len(hot), 5000):                              # the batch form, per entry
            part = [keys[i] for i in hot[lo:lo + 5000]] + [("Svc0", "nobody")]
            got = op.lookup_batch(part)
            assert got[:-1] == [home[k] for k in part[:-1]] and got[-1] is None
            for k in part[:-1]:
                md.count(k)
        b0 = op.device_round_trips()[0]
        for i in hot[:3000]:                                             # the single form, from the host shadow
            assert op.lookup(*keys[i]) == home[keys[i]]
            md.count(keys[i])
        assert op.device_round_trips()[0] == b0
        for i in range(0, n, 50):
            assert op.get_or_create_placement(*keys[i], addrs[5])[0] == home[keys[i]]
            md.count(keys[i])
            ok, got = op.try_lookup(*keys[i])
            assert ok and got == home[keys[i]]
            md.count(keys[i])
        assert op.lookup("Svc0", "nobody") is None                       # counts nothing
        want = md.fold(keys, 0, 1, 1, 1_000_000)
        assert op.fold_loads(0, 1, 1, 1_000_000) == want and want[1] == 30_000 + 3000 + 2 * (n // 50)
        for key in keys:
            assert op.get_object_load(*key) == md.load[key], key
        assert op.get_object_load("Svc0", "nobody") is None
        g = op.dense()
        loads = np.array([md.load[k] for k in keys], np.uint32)
        assert np.array_equal(g.get_objects()[0][:n], loads) and not g.get_hits().any()
        # the shadow still answers: no address changed
        b0 = op.device_round_trips()[0]
        for key in keys[:200]:
            assert op.lookup(*key) == home[key]
        assert op.device_round_trips()[0] == b0
        op.set_load_tracking(False)
        # the rebalance acts on the measured loads: capacities the first three servers now exceed
        for a in addrs:
            op.set_member(a, True, 6000)
        assert op.get_object_load(*keys[0]) == md.load[keys[0]]          # (a call that brings the device's node table up to date)
        nrows = g.num_objects
        cur = g.get_assign()
        load, aff = g.get_objects()
        cap, alive, used = g.get_nodes()
        assert np.array_equal(used, spec.used_of(cur, load, nrows, len(cap)))
        nxt, wused, wst, wrows, wfrom, wto = rebalance_ref.rebalance(cur, load, aff, cap, alive, None, None, 2)
        moves = op.rebalance()
        assert len(wrows) > 0
        assert moves == [(keys[r][0], keys[r][1], addrs[f], addrs[t]) for r, f, t in zip(wrows, wfrom, wto)]
        assert np.array_equal(g.get_assign(), nxt) and np.array_equal(g.get_nodes()[2], wused)
        for ty, oid, f, t in moves:
            home[(ty, oid)] = t
        for key in keys[::7]:
            assert op.lookup(*key) == home[key]
    finally:
        op.close()
