#!/usr/bin/env python3
"""The hot-object report on config 3 (10 M x 1 024, the warm table of synth.py after one tick, Zipf(1.3) loads): wall clock per
rio_gp_top_rows call (host-pointer form: every pass, the copy of the listing and the one stream wait), median and min-max of
`reps` runs, every run from the same state (the call changes nothing).
  load_cap16 / load_cap4096                 by load, no filter
  placed_cap16 / placed_cap4096             the same under RIO_GP_TOP_PLACED (the committed column is read as well)
  hot_node_cap16 / hot_node_cap4096         RIO_GP_TOP_PLACED | RIO_GP_TOP_ON_NODE for the node with the largest load
  equal_loads_cap4096                       every load equal: 10 M ties at the cut, the lowest 4 096 rows
  count_only                                cap 0: the first histogram pass alone
  host_baseline_cap16 / host_baseline_cap4096   what a host does without the call, in the same run: rio_gp_get_objects and
                                            rio_gp_get_assign to the host, numpy.argpartition of the placed rows' loads, a sort of
                                            the k it kept
  count_placed                              yardstick, an existing pass: 4 B per row
For each device case: us, algorithmic bytes per row (4 B per pass over the key column, 4 B more per pass under a filter flag:
three histogram passes and the collecting pass; the tie pass re-reads only the tiles that hold a listed tie) and TB/s.
Prints one JSON line.  Usage: top_probe.py [reps] [--out profiles/top_probe.json]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import rio_gp, synth
import spec_top as spec

NONE = 0xFFFFFFFF


def stat(ts, n, bytes_per_row):
    us = float(np.median(ts)) * 1e6
    return {"us": us, "us_min": float(np.min(ts)) * 1e6, "us_max": float(np.max(ts)) * 1e6,
            "bytes_per_row": round(float(bytes_per_row), 3), "tb_per_s": n * float(bytes_per_row) / us / 1e6}


def timed(fn, reps):
    ts, last = [], None
    for _ in range(reps + 2):
        t0 = time.perf_counter()
        last = fn()
        ts.append(time.perf_counter() - t0)
    return ts[2:], last


def main(reps):
    cfg = synth.config("c3")
    n, m = cfg["n"], cfg["m"]
    rng = np.random.default_rng(17)
    load = np.minimum(rng.zipf(1.3, n), 100_000).astype(np.uint32)
    g = rio_gp.GpuPlacement(n, m)
    g.set_nodes(np.full(m, int(load.sum()) * 5 // (4 * m), np.uint64), np.ones(m, np.uint8))
    g.set_objects(n, load, cfg["aff"])
    g.set_assign(synth.warm_assign(n, m))
    g.tick()
    A = g.get_assign()
    used = g.get_nodes()[2]
    hot = int(np.argmax(used))
    out = {"n": n, "m": m, "reps": reps, "placed": int((A != NONE).sum()), "hot_node": hot, "rows_on_hot_node": int((A == hot).sum()),
           "max_load": int(load.max())}

    def case(name, cap, passes, filt, **kw):
        ts, got = timed(lambda: g.top_rows(cap, **kw), reps)
        flags = (spec.PLACED if kw.get("placed") else 0) | (spec.ON_NODE if kw.get("node") is not None else 0)
        want = spec.top_rows(A, g.get_objects()[0], None, n, flags, kw.get("node") or 0, 0, cap)
        assert got[3:] == want[3:] and all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])), name
        out[name] = dict(stat(ts, n, passes * (8 if filt else 4)), n_candidates=got[3], listed=len(got[0]))

    case("load_cap16", 16, 4, False)
    case("load_cap4096", 4096, 4, False)
    case("placed_cap16", 16, 4, True, placed=True)
    case("placed_cap4096", 4096, 4, True, placed=True)
    case("hot_node_cap16", 16, 4, True, placed=True, node=hot)
    case("hot_node_cap4096", 4096, 4, True, placed=True, node=hot)
    case("count_only", 0, 1, False)

    def host(k):
        ld = g.get_objects()[0]
        a = g.get_assign()
        r = np.flatnonzero(a != NONE)
        part = r[np.argpartition(ld[r], len(r) - k)[len(r) - k:]]
        return part[np.lexsort((part, -ld[part].astype(np.int64)))]
    for k in (16, 4096):
        ts, rows = timed(lambda: host(k), reps)
        out["host_baseline_cap%d" % k] = stat(ts, n, 8)
        # (argpartition breaks ties at the cut as it likes: the keys are the listing's, the rows need not be)
        assert np.array_equal(load[rows], g.top_rows(k, placed=True)[1])
    ts, _ = timed(g.count_placed, reps)
    out["count_placed"] = stat(ts, n, 4)

    g.set_objects(n, np.full(n, 7, np.uint32), cfg["aff"])
    g.set_assign(A)
    case("equal_loads_cap4096", 4096, 4, False)
    for k in ("cap16", "cap4096"):
        out["host_baseline_over_placed_" + k] = out["host_baseline_" + k]["us"] / out["placed_" + k]["us"]
    g.close()
    return out


if __name__ == "__main__":
    argv = sys.argv[1:]
    dest = os.environ.get("PROBE_OUT")
    if "--out" in argv:
        k = argv.index("--out")
        dest = argv[k + 1]
        del argv[k:k + 2]
    res = {"top_rows": main(int(argv[0]) if argv else 15)}
    print(json.dumps(res))
    if dest:
        with open(dest, "w") as f:
            json.dump(res, f, indent=1)
