#!/usr/bin/env python3
"""The string layer's six key-listing calls on a table of 8 192 keys (every eighth with a NUL byte) on four servers, each call
listing a few thousand entries: wall clock per call, median and min-max of `reps` runs, every run from the same state (what a
call changes is put back, untimed, before the next run).
  snapshot             8 192 entries
  objects_on_server    the 4 096 keys of one server
  rebalance            that server's capacity lowered to 1 024: 3 072 moves
  changes              4 096 keys moved to another server since the last listing
  expire               4 096 keys last stamped before the cutoff
  hottest_objects      max_objects = RIO_GP_TOP_MAX = 4 096, over all servers
`lib_us` is the library call alone (rio_op_* through the GpuObjectPlacement's handle, the out-parameters made beforehand);
`method_us` is the GpuObjectPlacement method, which decodes every entry into Python strings as well.  RIO_GP_LIB selects another
build of the library (tools/ab_lib.sh does the same for bench.py).  Prints one JSON line.
Usage: listing_probe.py [reps] [--out profiles/listing_probe.json]"""
import ctypes as C
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rio-rs_amd")):
    sys.path.insert(0, p)
import numpy as np
import rio_gp

N, INF = 8192, rio_gp.CAP_INF
KEYS = [("T", ("k\0%d" if k % 8 == 0 else "k%d") % k) for k in range(N)]
SERVERS = ["10.0.0.%d:7000" % j for j in range(4)]
HOME = [SERVERS[k % 2] for k in range(N)]                      # 4 096 keys on each of the first two servers


def stat(ts):
    return {"us": float(np.median(ts)) * 1e6, "us_min": float(np.min(ts)) * 1e6, "us_max": float(np.max(ts)) * 1e6}


def main(reps):
    L = rio_gp._oplib()
    op = rio_gp.GpuObjectPlacement(max_objects=N, max_nodes=16)
    for a in SERVERS:
        op.set_member(a, True, INF)
    for k in range(1, N, 64):                                     # (odd keys: on the server the rebalance leaves alone)
        op.set_object_load(*KEYS[k], 2 + k % 97)
    state = {"clock": 10}

    def home():                                                   # every key on its server, stamped with a fresh clock
        state["clock"] += 10
        op.set_clock(state["clock"])
        op.update_batch(KEYS, HOME)

    def lib_call(name, k, *args):
        o = rio_gp._listing_out(k)
        refs = [C.byref(v) for v in o]
        fn = getattr(L, name)
        t0 = time.perf_counter()
        rc = fn(op._h, *args, *refs)
        dt = time.perf_counter() - t0
        assert rc == rio_gp.OK, (name, rc)
        return dt, int(o[0].value)

    def lib_snapshot():
        o = rio_gp._listing_out(1)
        n, ty, tl, oid, il, addr = [C.byref(v) for v in o]
        t0 = time.perf_counter()
        rc = L.rio_op_snapshot(op._h, n, ty, oid, addr) or L.rio_op_snapshot_key_lengths(op._h, tl, il)
        dt = time.perf_counter() - t0
        assert rc == rio_gp.OK
        return dt, int(o[0].value)

    def lib_changes():
        o, full = rio_gp._listing_out(2), C.c_int(0)
        refs = [C.byref(v) for v in o]
        t0 = time.perf_counter()
        rc = L.rio_op_changes(op._h, refs[0], C.byref(full), *refs[1:])
        dt = time.perf_counter() - t0
        assert rc == rio_gp.OK
        return dt, int(o[0].value)

    def lib_expire(cutoff):
        o, idle = rio_gp._listing_out(1), C.c_uint64(0)
        refs = [C.byref(v) for v in o]
        t0 = time.perf_counter()
        rc = L.rio_op_expire(op._h, cutoff, 4096, refs[0], C.byref(idle), *refs[1:])
        dt = time.perf_counter() - t0
        assert rc == rio_gp.OK
        return dt, int(o[0].value)

    def lib_hottest():
        o, cand = rio_gp._listing_out(1), C.c_uint64(0)
        refs = [C.byref(v) for v in o]
        loads = (C.c_uint32 * rio_gp.TOP_MAX)()
        t0 = time.perf_counter()
        rc = L.rio_op_hottest_objects(op._h, None, 0, rio_gp.TOP_MAX, refs[0], C.byref(cand), *refs[1:], loads)
        dt = time.perf_counter() - t0
        assert rc == rio_gp.OK
        return dt, int(o[0].value)

    def method(fn):
        t0 = time.perf_counter()
        got = fn()
        return time.perf_counter() - t0, len(got)

    # before: what puts the table into the state the call is timed from (untimed)
    def before_rebalance():
        home()
        op.set_member(SERVERS[0], True, 1024)

    def after_rebalance():
        op.set_member(SERVERS[0], True, INF)

    def before_changes():
        home()
        op.changes()
        op.update_batch(KEYS[:4096], [SERVERS[2 + k % 2] for k in range(4096)])

    def before_expire():
        home()                                                    # all stamped with the clock ...
        state["clock"] += 10
        op.set_clock(state["clock"])
        op.lookup_batch(KEYS[4096:])                              # ... and the upper half with a later one

    cases = {
        "snapshot": (home, None, lib_snapshot, lambda: method(op.snapshot), N),
        "objects_on_server": (home, None, lambda: lib_call("rio_op_objects_on_server", 0, SERVERS[0].encode()),
                              lambda: method(lambda: op.objects_on_server(SERVERS[0])), 4096),
        "rebalance": (before_rebalance, after_rebalance, lambda: lib_call("rio_op_rebalance", 2, INF),
                      lambda: method(op.rebalance), 3072),
        "changes": (before_changes, None, lib_changes, lambda: method(lambda: op.changes()[1]), 4096),
        "expire": (before_expire, None, lambda: lib_expire(state["clock"]),
                   lambda: method(lambda: op.expire(state["clock"], 4096)[0]), 4096),
        "hottest_objects": (home, None, lib_hottest, lambda: method(lambda: op.hottest_objects()[0]), 4096),
    }
    out = {"keys": N, "reps": reps, "lib": os.path.basename(os.environ.get("RIO_GP_LIB", rio_gp.LIB_PATH))}
    for name, (before, after, lib_fn, method_fn, want) in cases.items():
        res = {}
        for kind, fn in (("lib_us", lib_fn), ("method_us", method_fn)):
            ts = []
            for _ in range(reps + 2):
                before()
                dt, n = fn()
                assert n == want, (name, kind, n, want)
                ts.append(dt)
                if after:
                    after()
            res[kind] = stat(ts[2:])
        res["entries"] = want
        out[name] = res
    op.close()
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    res = main(int(args[0]) if args else 15)
    line = json.dumps(res)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    print(line)
