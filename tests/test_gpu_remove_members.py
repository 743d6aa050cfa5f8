"""rio_op_remove_members on the MI355X, end to end: the string layer over the real dense layer, about a thousand keys on about
forty addresses, driven through two clones against the dict model of tests/test_remove_members_host.py (its request policy is the
reference's, which the device computes with unbounded capacities; whole-table ticks are left out: the device's is a capacity
solve, not the stub's)."""
import random

import pytest

from test_remove_members_host import Model, apply_listing


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


def refused(gp, fn, *a):
    with pytest.raises(gp.ObjectPlacementError) as e:
        fn(*a)
    assert e.value.rc == gp.EINVAL and "node table full" in e.value.text


def check(op, md, keys, addrs, sample):
    for ty, oid in sample:
        assert op.lookup(ty, oid) == md.where.get((ty, oid)), (ty, oid)
    for k in range(md.max_nodes + 1):
        assert op.node_address(k) == (md.addr[k] if k < len(md.addr) else None), k


@pytest.mark.gpu
@pytest.mark.parametrize("shadow", [True, False])
def test_random_calls_on_the_device_match_the_model(gp, shadow):
    rng = random.Random(3 + shadow)
    max_nodes = 32
    a = gp.GpuObjectPlacement(max_objects=4096, max_nodes=max_nodes, flags=0 if shadow else gp.OP_CFG_NO_HOST_SHADOW)
    ops = [a, a.clone()]
    md = Model(max_nodes)
    addrs = ["10.0.%d.%d:50%02d" % (k // 8, k % 8, k) for k in range(40)]   # more addresses than ids
    keys = [("T%d" % (i % 5), "obj-%d" % i) for i in range(1000)]
    mirror, fed = {}, False
    try:
        for ad in addrs[:24]:
            a.set_member(ad, True)
            md.intern(ad)
            md.alive[ad] = True
        a.update_batch(keys[:600], [addrs[i % 24] for i in range(600)])
        for i in range(600):
            md.update(keys[i], addrs[i % 24])
        for it in range(300):
            op = ops[rng.randrange(2)]
            k = rng.randrange(11)
            key, ad = rng.choice(keys), rng.choice(addrs)
            if k <= 1:
                if md.full_for(ad):
                    refused(gp, op.update, key[0], key[1], ad)
                else:
                    op.update(key[0], key[1], ad)
                    md.update(key, ad)
            elif k == 2:
                op.remove(key[0], key[1]) if rng.random() < 0.5 else op.update(key[0], key[1], None)
                md.unplace(key)
            elif k <= 5:
                if md.full_for(ad):
                    refused(gp, op.get_or_create_placement, key[0], key[1], ad)
                else:
                    assert op.get_or_create_placement(key[0], key[1], ad) == md.request(key, ad), it
            elif k == 6:
                act = rng.random() < 0.6
                if md.full_for(ad):
                    refused(gp, op.set_member, ad, act)
                else:
                    op.set_member(ad, act)
                    md.intern(ad)
                    md.alive[ad] = act
            elif k == 7:
                op.clean_server(ad)
                md.clean(ad)
            elif k <= 9:
                some = rng.sample(addrs, rng.randrange(1, 6)) + ["never:1"]
                some += some[:1]
                assert op.remove_members(some) == md.remove_members(some), it
            else:
                full, ent = op.changes()
                assert full == (not fed)
                fed = True
                mirror = apply_listing(mirror, full, ent)
                assert mirror == md.where, it
            check(op, md, keys, addrs, rng.sample(keys, 25) + [key])
            if it % 25 == 0:
                assert {(t, i): v for t, i, v in op.snapshot()} == md.where
                for x in rng.sample(addrs, 4):
                    assert sorted(op.objects_on_server(x)) == sorted(kk for kk, v in md.where.items() if v == x)
        assert {(t, i): v for t, i, v in ops[1].snapshot()} == md.where
        full, ent = ops[0].changes()
        assert apply_listing(mirror, full, ent) == md.where
        assert len(a) == len(md.where)
    finally:
        for op in ops:
            op.close()


@pytest.mark.gpu
def test_a_full_node_table_takes_a_new_address_after_a_removal(gp):
    op = gp.GpuObjectPlacement(max_objects=64, max_nodes=4)
    try:
        for k in range(4):
            op.update("T", "o%d" % k, "h%d:1" % k)
        refused(gp, op.update, "T", "o4", "h4:1")
        assert op.remove_members(["h1:1"]) == (1, 1)
        op.update("T", "o4", "h4:1")
        assert op.lookup("T", "o4") == "h4:1" and op.lookup("T", "o1") is None and op.lookup("T", "o3") == "h3:1"
        assert [op.node_address(k) for k in range(5)] == ["h0:1", "h2:1", "h3:1", "h4:1", None]
        assert sorted(op.snapshot()) == sorted([("T", "o0", "h0:1"), ("T", "o2", "h2:1"), ("T", "o3", "h3:1"), ("T", "o4", "h4:1")])
    finally:
        op.close()
