"""Idle deactivation through the string layer on the MI355X (rio_op_set_clock / rio_op_expire over rio_gp_touch_merge and
rio_gp_expire): with the clock at 0 no stamps are kept and every placed key is idle; with the clock running, every stamping call
(lookup on the device and from the host shadow, try_lookup, update, get_or_create_placement and its try form, the batch forms)
keeps its key out of a sweep whose cutoff lies between two clock values, and nothing else does; the expired keys answer "none"
afterwards while the kept ones are still answered from the host shadow; the change feed lists them as deletes; a table full of
live objects takes new keys again; keys with NUL bytes come back whole."""
import pytest

import spec_changes


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


@pytest.mark.gpu
def test_clock_at_zero_keeps_no_stamps_and_lists_everything_placed(gp):
    op = gp.GpuObjectPlacement(max_objects=64, max_nodes=8)
    try:
        op.set_member("a:1")
        keys = [("T", "o%d" % k) for k in range(10)]
        for ty, oid in keys:
            op.update(ty, oid, "a:1")
        assert op.lookup("T", "o3") == "a:1"
        op.remove("T", "o9")
        g = op.dense()
        assert op.expire(0, 0) == ([], 0) and op.expire(1, 0) == ([], 9)       # count only: nothing changes
        assert not g.get_seen().any()                                           # no stamp was kept
        assert op.expire(1, 4) == ([("T", "o%d" % k, "a:1") for k in range(4)], 9)
        out, idle = op.expire(0xFFFFFFFF)
        assert out == [("T", "o%d" % k, "a:1") for k in range(4, 9)] and idle == 5
        assert op.snapshot() == [] and len(op) == 0
    finally:
        op.close()


@pytest.mark.gpu
def test_every_stamping_call_keeps_its_key_and_the_shadow_is_corrected_precisely(gp):
    op = gp.GpuObjectPlacement(max_objects=256, max_nodes=8)
    try:
        for a in ("a:1", "b:1"):
            op.set_member(a)
        keys = [("T%d" % (k % 3), "o%d" % k) for k in range(60)] + [("N\0", "x\0y"), ("N", "x")]
        full, ent = op.changes()
        mirror = spec_changes.apply({}, full, ent)
        op.set_clock(1)
        op.update_batch(keys, ["a:1" if k % 2 else "b:1" for k in range(len(keys))])   # stamped 1, and in the shadow
        where = {key: ("a:1" if k % 2 else "b:1") for k, key in enumerate(keys)}
        op.set_clock(5)
        kept = set()

        def keep(key):
            kept.add(key)
            return key
        # one key (or a few) per stamping call
        assert op.lookup(*keep(keys[0])) == where[keys[0]]                          # a shadow hit
        ok, got = op.try_lookup(*keep(keys[1]))
        assert ok and got == where[keys[1]]
        ok, got, fl = op.try_get_or_create_placement(*keep(keys[2]), "a:1")
        assert ok and got == where[keys[2]]
        assert op.get_or_create_placement(*keep(keys[3]), "b:1")[0] == where[keys[3]]   # sticky, from the shadow
        op.update(*keep(keys[4]), "b:1")
        where[keys[4]] = "b:1"
        op.invalidate_cache()                                                        # from here on the device answers
        assert op.lookup(*keep(keys[5])) == where[keys[5]]
        assert op.get_or_create_placement(*keep(keys[6]), "a:1")[0] == where[keys[6]]
        assert op.lookup_batch([keep(keys[7]), keep(keys[8]), ("T", "nobody")]) == [where[keys[7]], where[keys[8]], None]
        op.update_batch([keep(keys[9]), keys[10]], ["a:1", None])                    # an address stamps, a removal does not
        where[keys[9]] = "a:1"
        del where[keys[10]]
        got, _fl = op.get_or_create_placement_batch([keep(keys[11]), keep(keys[12])], ["a:1", "b:1"])
        assert got == [where[keys[11]], where[keys[12]]]
        assert op.lookup(*keep(keys[60])) == where[keys[60]]                         # the key with NUL bytes
        # calls that do not stamp
        op.set_object_load(*keys[20], 3)
        assert op.lookup("T", "nobody") is None
        op.remove(*keys[21])
        del where[keys[21]]
        for key in keys[30:40]:                                                      # these answer from the shadow later
            assert op.lookup(*key) == where[key]
            kept.add(key)
        op.set_clock(9)
        want = [(k[0], k[1], where[k]) for k in keys if k in where and k not in kept]   # row order = the order of the batch
        assert op.expire(3, 0) == ([], len(want))
        out, idle = op.expire(3)                                                     # 1 < 3 <= 5
        assert idle == len(want) and out == want
        assert ("N", "x", where[("N", "x")]) in out                                  # (and its twin with the NUL bytes is kept)
        for t, i, _a in out:
            del where[(t, i)]
        # the shadow: expired keys answer none, kept keys are still hits (no device round trip)
        b0 = op.device_round_trips()[0]
        for key in keys[30:40]:
            assert op.lookup(*key) == where[key]
        assert op.device_round_trips()[0] == b0
        for t, i, _a in out[:10]:
            assert op.lookup(t, i) is None
            ok, got = op.try_lookup(t, i)
            assert ok and got is None
        assert op.device_round_trips()[0] == b0                                      # "none" is the shadow's answer as well
        # the feed lists exactly what happened; applied to the mirror it yields the snapshot
        full, ent = op.changes()
        mirror = spec_changes.apply(mirror, full, ent)
        assert spec_changes.as_set(mirror) == set(op.snapshot()) == {(k[0], k[1], a) for k, a in where.items()}
        assert op.expire(3) == ([], 0)
        out2, _ = op.expire(10)                                                      # everything that is left goes now
        assert {(t, i) for t, i, _a in out2} == set(where)
        full, ent = op.changes()
        assert all(new is None for _t, _i, _old, new in ent)
        assert spec_changes.apply(mirror, full, ent) == {} and op.snapshot() == []
    finally:
        op.close()


@pytest.mark.gpu
def test_a_table_full_of_live_objects_takes_new_keys_after_a_sweep(gp):
    op = gp.GpuObjectPlacement(max_objects=32, max_nodes=4)
    try:
        op.set_member("a:1")
        op.set_clock(1)
        for k in range(32):
            op.update("T", "o%d" % k, "a:1")
        with pytest.raises(gp.ObjectPlacementError) as e:
            op.update("T", "new", "a:1")
        assert "object table full" in e.value.text
        op.set_clock(2)
        for k in range(8):
            assert op.get_or_create_placement("T", "o%d" % k, "a:1")[0] == "a:1"
        out, idle = op.expire(2, 20)
        assert idle == 24 and [o[1] for o in out] == ["o%d" % k for k in range(8, 28)]
        for k in range(20):
            op.update("T", "new%d" % k, "a:1")
        with pytest.raises(gp.ObjectPlacementError):
            op.update("T", "new20", "a:1")
        assert len(op) == 32
        assert {s[1] for s in op.snapshot()} == ({"o%d" % k for k in range(8)} | {"o%d" % k for k in range(28, 32)} |
                                                 {"new%d" % k for k in range(20)})
    finally:
        op.close()
