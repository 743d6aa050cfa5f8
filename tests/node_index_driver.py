"""Differential driver of rio_op_objects_on_server (the reverse index of the string layer), shared by the host-stub test
(tests/test_node_index_host.py) and the GPU test (tests/test_gpu_node_index.py).

A random sequence of update / remove / clean_server / get_or_create_placement / membership flips runs against the layer under
test and against pyoracle.LocalObjectPlacement (+ Service::get_or_create_placement restated); the table is kept small so that
keys are reclaimed.  After every step, for every address: objects_on_server equals, as a set of "{struct_name}.{object_id}"
keys without repeats, the entries the oracle holds for that address, and snapshot() filtered by that address."""
import random

ADDRS = ["10.0.0.1:5000", "10.0.0.2:5000", "h3:1", "a-rather-long-host-name-that-does-not-fit-thirty-two-bytes.example:65535"]
OFF_MEMBERS = ["10.9.9.9:1"]   # update()d onto, never a member (LocalObjectPlacement stores any address: local.rs:22-40)
UNKNOWN = "never.seen:1"
# ("a.b","c") and ("a","b.c") are one object (local.rs:26-29); ("N\0ul", "z") holds a NUL byte (the oracle, which takes C
# strings, knows it as "N.z": no other key is that)
KEYS = [("T", str(k)) for k in range(8)] + [("a.b", "c"), ("a", "b.c"), ("U", ""), ("N\0ul", "z"), ("V", "x\0y")]
MAX_OBJECTS = 8   # fewer rows than keys: new keys reuse the rows of removed ones (reclaim)


def joined(ty, oid):
    return "%s.%s" % (ty, oid)


def _oracle_key(ty, oid):   # what the oracle's C-string entry points see
    return joined(ty.split("\0")[0], oid.split("\0")[0])


def expected(ref):
    """address -> set of joined keys the oracle holds there (keys that collide count once)."""
    out = {}
    for ty, oid in KEYS:
        a = ref.lookup(ty, oid)
        if a is not None:
            out.setdefault(a, set()).add(joined(ty, oid))
    return out


def check(op, ref):
    want = expected(ref)
    snap = {}
    for ty, oid, a in op.snapshot():
        snap.setdefault(a, []).append(joined(ty, oid))
    for a in ADDRS + OFF_MEMBERS + [UNKNOWN]:
        got = [joined(ty, oid) for ty, oid in op.objects_on_server(a)]
        assert len(got) == len(set(got)), (a, got)
        assert sorted(got) == sorted(want.get(a, set())), (a, got, want.get(a))
        assert sorted(got) == sorted(snap.get(a, [])), (a, got, snap.get(a))


def live_count(ref):
    return len({_oracle_key(*k) for k in KEYS if ref.lookup(*k) is not None})


def run(op, oracle, seed, steps=120):
    """op: the layer under test, with update / remove / clean_server / get_or_create_placement / set_member / snapshot /
    objects_on_server as rio_gp.GpuObjectPlacement has them."""
    rnd = random.Random(seed)
    ref, members = oracle.LocalObjectPlacement(), oracle.LocalStorage()
    for a in ADDRS:
        ip, port = a.rsplit(":", 1)
        members.push(ip, port, True)
        op.set_member(a, True)
    check(op, ref)
    for _ in range(steps):
        kind = rnd.choice(["update", "update", "update", "remove", "clean", "request", "request", "active"])
        ty, oid = rnd.choice(KEYS)
        placed = ref.lookup(ty, oid) is not None
        if kind in ("update", "request") and not placed and live_count(ref) >= MAX_OBJECTS - 1:
            kind = "remove"     # (keep the live objects within the table: the reference has no such limit)
        if kind == "update":
            a = rnd.choice(ADDRS + OFF_MEMBERS + [None])
            op.update(ty, oid, a)
            ref.update(ty, oid, a)
        elif kind == "remove":
            op.remove(ty, oid)
            ref.remove(ty, oid)
        elif kind == "clean":
            a = rnd.choice(ADDRS + OFF_MEMBERS)
            op.clean_server(a)
            ref.clean_server(a)
        elif kind == "active":
            a = rnd.choice(ADDRS)
            on = rnd.random() < 0.6
            ip, port = a.rsplit(":", 1)
            members.set_is_active(ip, port, on)
            op.set_member(a, on)
        else:
            me = rnd.choice(ADDRS)
            got = op.get_or_create_placement(ty, oid, me)[0]
            assert got == oracle.get_or_create_placement(ref, members, me, ty.split("\0")[0], oid.split("\0")[0])
        check(op, ref)
