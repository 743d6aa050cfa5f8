#!/usr/bin/env python3
"""Object classes on config 3 (10 M x 1 024, the warm table of synth.py after one tick): wall clock per call, median and min-max
of `reps` runs, every run from the same restored table (the assignment column is put back from a device copy and `used` rebuilt
before each run, not timed; S and K are never changed by a sweep or a census).  S is laid out by row as in expire_probe.py: r %
100 == 0 was last seen at epoch 1, 1 <= r % 100 < 10 at epoch 2, the rest at epoch 3; K[r] = (r / 100) % 8 (and % 64 for the
64-class census): every class holds the same share of each, so cutoffs of 2 for every class find 1 % of the rows idle and cutoffs
of 3 find 10 %.
  expire_count_only / expire_1pct / expire_10pct      rio_gp_expire_dev, the parent's call: the yardstick
  classes_count_only / classes_1pct / classes_10pct   rio_gp_expire_classes_dev with 8 cutoffs on the same table in the same run
  count_placed                    rio_gp_count_placed: one pass over A (4 B per row), the census's yardstick
  census_totals_8 / _64           rio_gp_census_dev, [n_classes] cells (LDS accumulators)
  census_by_node_8 / _64          rio_gp_census_dev, [1 024][n_classes] cells: 8 192 cells run as two LDS slices (two passes over
                                  the columns), 65 536 cells are past kCensusMaxSlices slices (global adds per row)
  census_by_node_4                [1 024][4]: 4 096 cells, the largest shape that accumulates in LDS (over the 64-class column:
                                  the rows of a class >= 4 are counted in n_other)
  host_route_8                    what a host does without the call: rio_gp_get_assign + rio_gp_get_objects + numpy.bincount
                                  over its own class column (totals and by node)
Prints one JSON line.  Usage: classes_probe.py [reps]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np
import rio_gp, synth

NONE = 0xFFFFFFFF


def stat(ts):
    return {"us": float(np.median(ts)) * 1e6, "us_min": float(np.min(ts)) * 1e6, "us_max": float(np.max(ts)) * 1e6}


def main(reps):
    import torch
    cfg = synth.config("c3")
    n, m = cfg["n"], cfg["m"]
    g = rio_gp.GpuPlacement(n, m)
    g.set_nodes(cfg["cap"], np.ones(m, np.uint8))
    g.set_objects(n, cfg["load"], cfg["aff"])
    g.set_assign(synth.warm_assign(n, m))
    g.tick()
    A0 = g.get_assign()
    dA = torch.from_numpy(A0.view(np.int32).copy()).cuda()
    S = np.full(n, 3, np.uint32)
    r100 = np.arange(n) % 100
    S[r100 < 10] = 2
    S[r100 == 0] = 1
    g.touch_merge(S)
    K8 = ((np.arange(n) // 100) % 8).astype(np.uint8)
    K64 = ((np.arange(n) // 100) % 64).astype(np.uint8)
    g.set_classes(0, K8)
    g.changes()
    d = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2)]
    cells = [torch.empty(m * 64, dtype=torch.int64, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    dp = [x.data_ptr() for x in d]
    cp = [x.data_ptr() for x in cells]
    out = {"n": n, "m": m, "reps": reps, "placed": int((A0 != NONE).sum())}

    def restore():
        g.set_assign_dev(n, dA.data_ptr())
        g.get_nodes()                             # `used` valid again: the sweep keeps it current
        g.changes()

    def timed(fn):
        ts, last = [], None
        for _ in range(reps + 1):
            restore()
            t0 = time.perf_counter()
            last = fn()
            ts.append(time.perf_counter() - t0)
        return ts[1:], last

    for name, cutoff, listing in (("count_only", 3, False), ("1pct", 2, True), ("10pct", 3, True)):
        a = (dp[0], dp[1], n) if listing else (None, None, 0)
        ts, r = timed(lambda: g.expire_dev(cutoff, a[0], a[1], cap=a[2]))
        out["expire_" + name] = dict(stat(ts), n_idle=r[0], load_freed=r[1])
        ts, r = timed(lambda: g.expire_classes_dev([cutoff] * 8, a[0], a[1], cap=a[2]))
        out["classes_" + name] = dict(stat(ts), n_idle=r[0], load_freed=r[1], idle_by_class=[int(x) for x in r[2]])
        assert r[0] == out["expire_" + name]["n_idle"] and r[1] == out["expire_" + name]["load_freed"]
        out["classes_over_expire_" + name] = out["classes_" + name]["us"] / out["expire_" + name]["us"]

    ts, r = timed(g.count_placed)
    out["count_placed"] = dict(stat(ts), placed=r)
    for nc, K in ((8, K8), (64, K64), (4, None)):
        if K is not None:
            g.set_classes(0, K)
        if nc != 4:
            ts, r = timed(lambda: g.census_dev(nc, cp[0], cp[1]))
            out["census_totals_%d" % nc] = dict(stat(ts), n_other=int(r))
        ts, r = timed(lambda: g.census_dev(nc, cp[0], cp[1], by_node=True))
        out["census_by_node_%d" % nc] = dict(stat(ts), n_other=int(r), cells=m * nc)

    def host_route():
        A = g.get_assign()
        load = g.get_objects()[0]
        ok = A != NONE
        tot = (np.bincount(K8[ok], minlength=8), np.bincount(K8[ok], weights=load[ok], minlength=8))
        okn = ok & (A < m)
        cell = A[okn].astype(np.int64) * 8 + K8[okn]
        by = (np.bincount(cell, minlength=m * 8), np.bincount(cell, weights=load[okn], minlength=m * 8))
        return int(tot[0].sum()), int(by[0].sum())
    g.set_classes(0, K8)
    ts, r = timed(host_route)
    out["host_route_8"] = dict(stat(ts), rows=r[0])
    out["census_by_node_8_over_host_route"] = out["census_by_node_8"]["us"] / out["host_route_8"]["us"]
    out["census_totals_8_over_count_placed"] = out["census_totals_8"]["us"] / out["count_placed"]["us"]
    g.close()
    return out


if __name__ == "__main__":
    res = {"classes": main(int(sys.argv[1]) if len(sys.argv) > 1 else 7)}
    print(json.dumps(res))
    if os.environ.get("PROBE_OUT"):
        with open(os.environ["PROBE_OUT"], "w") as f:
            json.dump(res, f, indent=1)
