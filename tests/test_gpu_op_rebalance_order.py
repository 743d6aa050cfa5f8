"""The string layer's load-ordered rebalance on the MI355X: rio_op_rebalance_ordered returns the keys and addresses of exactly
the dense moves of the rule (tests/spec_rebalance_order.py, rows in first-update order, nodes in membership order), lookups and
the reverse index follow, and rio_op_rebalance stays row order."""
import numpy as np
import pytest

import rio_gp
import spec_rebalance_order as spec

pytestmark = pytest.mark.gpu
INF = rio_gp.CAP_INF


def _setup(p, seed, n_keys=3000):
    rng = np.random.default_rng(seed)
    addrs = ["10.0.0.%d:5000" % k for k in range(6)]
    for a in addrs:
        p.set_member(a, True, INF)
    keys = [("Svc", "o%d" % k) for k in range(n_keys)] + [("Svc", "nul\0key"), ("S\0vc", "x")]
    loads = np.minimum(rng.zipf(1.3, len(keys)), 100_000).astype(np.int64)
    loads[rng.random(len(keys)) < 0.1] = 0
    home = {}
    for k, key in enumerate(keys):
        a = addrs[int(rng.integers(0, 3))]          # everything on the first three servers
        p.update(key[0], key[1], a)
        p.set_object_load(key[0], key[1], int(loads[k]))
        home[key] = a
    per = int(loads.sum()) // 3
    caps = [per * 6 // 10, per * 7 // 10, per * 9 // 10, per, per, INF]
    for a, c in zip(addrs, caps):
        p.set_member(a, True, c)
    return addrs, keys, loads.tolist(), home, caps


@pytest.mark.parametrize("budget", [None, 1, 40])
@pytest.mark.parametrize("order", [0, 1])
def test_keys_and_addresses_of_exactly_the_dense_moves(oracle, order, budget):
    p = rio_gp.GpuObjectPlacement(max_objects=1 << 14, max_nodes=16)
    addrs, keys, loads, home, caps = _setup(p, 2)
    cur = [addrs.index(home[k]) for k in keys]
    _, _, st, want = spec.rebalance(cur, loads, [0] * len(keys), caps, [1] * len(addrs), max_moves=budget, order=order)
    moves = p.rebalance(budget, order=order)
    assert want and moves == [(keys[i][0], keys[i][1], addrs[a], addrs[b]) for i, a, b in want]
    if order == 1:
        ld = dict(zip(keys, loads))
        assert all(ld[(ty, oid)] > 0 for ty, oid, _, _ in moves)
    for ty, oid, f, t in moves:
        assert home[(ty, oid)] == f
        home[(ty, oid)] = t
    for (ty, oid), a in home.items():
        assert p.lookup(ty, oid) == a
    for a in addrs:
        assert sorted(p.objects_on_server(a)) == sorted(k for k, v in home.items() if v == a)
    p.close()


def test_unknown_order_is_refused(oracle):
    p = rio_gp.GpuObjectPlacement(max_objects=1 << 10, max_nodes=8)
    addrs, keys, loads, home, caps = _setup(p, 3, n_keys=200)
    with pytest.raises(rio_gp.ObjectPlacementError) as e:
        p.rebalance(order=2)
    assert e.value.rc == rio_gp.EINVAL
    for (ty, oid), a in home.items():
        assert p.lookup(ty, oid) == a
    p.close()
