"""Per-type idle limits and the census through the real library on the MI355X (rio_op_set_type_idle_limit_n,
rio_op_expire_by_type, rio_op_census over rio_gp_set_classes / _set_class_batch / _expire_classes / _census): the fixed cases of
tests/test_classes_host.py — 300 types with RIO_OP_CLASS_OTHER and RIO_GP_ERANGE, a reclaimed row that changes type, keys with
NUL bytes, the quirk pair, the clock at 0, RIO_OP_IDLE_NEVER, now below the limit — and a random sequence against that file's
model; after every sweep rio_gp_get_classes on rio_op_dense(p) equals the model's type ids."""
import random

import pytest

from test_classes_host import Types
from test_expire_host import Seen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


def _classes(p):
    d = p.dense()
    try:
        return d.get_classes().tolist()
    finally:
        d.close()


def test_three_hundred_types_share_the_other_class_past_255(gp):
    NEVER = gp.IDLE_NEVER
    p = gp.GpuObjectPlacement(512, 4)
    for i in range(300):
        p.update("T%d" % i, "o", "a:1")
    p.set_type_idle_limit("T254", 5)
    for t in ("T255", "T299", "never seen"):
        with pytest.raises(gp.ObjectPlacementError) as e:
            p.set_type_idle_limit(t, 5)
        assert e.value.rc == gp.ERANGE
    cen = p.census()
    assert len(cen) == 256 and cen[:255] == [(b"T%d" % i, None, 1, 1) for i in range(255)] and cen[255] == (None, None, 45, 45)
    assert p.census(True)[255] == (None, "a:1", 45, 45)
    assert _classes(p) == list(range(255)) + [gp.CLASS_OTHER] * 45
    p.set_clock(10)
    p.set_type_idle_limit("T0", 3)
    assert p.expire_by_type(10, NEVER, 0) == ([], 2)          # every stamp is 0: T0 0 + 3 < 10, T254 0 + 5 < 10
    assert p.expire_by_type(4, NEVER) == ([("T0", "o", "a:1")], 1)
    assert p.expire_by_type(10, 20, 0) == ([], 1)             # OTHER uses the default
    out, idle = p.expire_by_type(10, 9)
    assert idle == 299 and [o[0] for o in out][-45:] == ["T%d" % i for i in range(255, 300)]
    assert p.census() == [] and p.snapshot() == []
    assert _classes(p) == list(range(255)) + [gp.CLASS_OTHER] * 45   # the sweep leaves the class column alone


def test_a_reclaimed_row_takes_its_new_keys_class(gp):
    p = gp.GpuObjectPlacement(4, 4)
    for k in range(4):
        p.update("A", "o%d" % k, "a:1")
    assert p.census() == [(b"A", None, 4, 4)] and _classes(p) == [0, 0, 0, 0]
    for k in range(4):
        p.remove("A", "o%d" % k)
    p.update("B", "n0", "b:1")                               # the table is full: the rows of the removed keys are reclaimed
    p.update("A", "n1", "b:1")
    p.update("B", "n2", "b:1")
    assert p.census() == [(b"A", None, 1, 1), (b"B", None, 2, 2)]
    assert sorted(_classes(p)) == [0, 0, 1, 1]                # (the fourth row still carries its old key's class)
    p.set_type_idle_limit("B", 0)
    out, idle = p.expire_by_type(1, gp.IDLE_NEVER)
    assert sorted(out) == [("B", "n0", "b:1"), ("B", "n2", "b:1")] and idle == 2
    assert p.census(True) == [(b"A", "b:1", 1, 1)]


def test_nul_bytes_the_quirk_pair_clock_zero_never_and_now_below_the_limit(gp):
    NEVER = gp.IDLE_NEVER
    p = gp.GpuObjectPlacement(64, 4)
    p.update("N\0", "x\0y", "a:1")
    p.update("N", "x", "a:1")
    p.update("a.b", "c", "a:1")
    p.update("a", "b.c", "b:1")                              # the same key "a.b.c": no new row, no new type
    assert p.census() == [(b"N\0", None, 1, 1), (b"N", None, 1, 1), (b"a.b", None, 1, 1)]
    assert p.census(True) == [(b"N\0", "a:1", 1, 1), (b"N", "a:1", 1, 1), (b"a.b", "b:1", 1, 1)]
    assert _classes(p) == [0, 1, 2]
    p.set_type_idle_limit("a", 0)                            # "a" becomes a type by this call — of no key
    assert p.expire_by_type(0, 0, 0) == ([], 0) and p.expire_by_type(1, 0, 0) == ([], 3)    # the clock is 0: every stamp is 0
    assert p.expire_by_type(0xFFFFFFFF, NEVER, 0) == ([], 0)
    p.set_type_idle_limit(b"N\0", 5)
    p.set_type_idle_limit("N", NEVER)
    assert p.expire_by_type(5, NEVER, 0) == ([], 0) and p.expire_by_type(3, NEVER, 0) == ([], 0)   # now <= limit: no wrap-around
    assert p.expire_by_type(6, NEVER) == ([("N\0", "x\0y", "a:1")], 1)
    p.set_clock(100)
    assert p.lookup("a.b", "c") == "b:1"                     # stamped 100
    p.set_type_idle_limit("a.b", 5)
    assert p.expire_by_type(105, 0, 0) == ([], 0) and p.expire_by_type(106, 0, 0) == ([], 1)
    assert p.expire_by_type(0xFFFFFFFF, 0) == ([("a.b", "c", "b:1")], 1)
    assert p.census() == [(b"N", None, 1, 1)] and _classes(p) == [0, 1, 2]


class _Where:
    """the placement half of the model: what a table with unbounded capacities and live servers does"""

    def __init__(self, addrs):
        self.addr, self.where = list(addrs), {}


@pytest.mark.parametrize("seed", range(3))
def test_random_calls_match_the_model(gp, seed):
    rng = random.Random(seed)
    p = gp.GpuObjectPlacement(256, 8)
    addrs = ["h%d:7" % k for k in range(5)]
    for ad in addrs:
        p.set_member(ad, True)
    md, sn, ty = _Where(addrs), Seen(), Types()
    keys = [("T%d" % (i % 5), "o%d" % i) for i in range(40)] + [("N\0", "x\0y"), ("N", "x")]
    tnames = ["T%d" % i for i in range(5)] + ["N\0", "N", "never-a-key"]
    for it in range(150):
        k = rng.randrange(10)
        key, ad = rng.choice(keys), rng.choice(addrs)
        if it == 20 or (it > 20 and k == 0):
            sn.clock += rng.randrange(1, 4)
            p.set_clock(sn.clock)
        elif k <= 3:
            p.update(key[0], key[1], ad)
            md.where[key] = ad
            sn.know(key)
            ty.know(key)
            sn.touch(key)
        elif k == 4:
            p.remove(key[0], key[1])
            md.where.pop(key, None)
        elif k == 5:
            t, lim = rng.choice(tnames), rng.choice([0, 1, 2, 5, gp.IDLE_NEVER])
            p.set_type_idle_limit(t, lim)
            assert ty.set_limit(t, lim) == 0
        elif k <= 8:
            now = rng.choice([0, 1, sn.clock, sn.clock + 1, sn.clock + 3, 0xFFFFFFFF])
            default = rng.choice([0, 1, 3, gp.IDLE_NEVER])
            cap = rng.choice([None, 1, 3, 1000])
            assert p.expire_by_type(now, default, cap) == ty.expire(md, sn, now, default, cap), it
            assert _classes(p) == [ty.key_type[x] for x in sn.order], it
        else:
            if p.lookup(key[0], key[1]) is not None:
                sn.touch(key)
        for by_server in (False, True):
            assert p.census(by_server) == ty.census(md, by_server), (it, by_server)
        assert {(t, i): x for t, i, x in p.snapshot()} == md.where
