#!/usr/bin/env python3
"""rio_gp_changes on config 3 (10 M x 1 024, the warm table of synth.py after one tick): wall clock per call of the _dev form
(device arrays, one wait) and of the host form (a count pass and a wait, then the listing and its copy to the host) in four
cases: nothing changed (counts only, and a whole call); one node flipped dead + a tick (~10^4 changes); 10 % of the nodes
flipped + a tick (~10^6 changes); the first, complete listing of every placed row (~10^7).  The changes are made before each
call and not timed.  Baseline: what a consumer does without the feed — rio_gp_get_assign and a numpy diff against its previous
copy.  Bytes: the count pass reads A and B (8 B/row); the listing re-reads the tiles with a change and writes 12 B per listed
row plus B.  Prints one JSON line.  Usage: changes_probe.py [reps]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np
import rio_gp, synth


def med(ts):
    return {"us": float(np.median(ts)) * 1e6, "us_min": float(np.min(ts)) * 1e6}


def main(reps):
    import torch
    cfg = synth.config("c3")
    n, m = cfg["n"], cfg["m"]
    g = rio_gp.GpuPlacement(n, m)
    g.set_nodes(cfg["cap"], np.ones(m, np.uint8))
    g.set_objects(n, cfg["load"], cfg["aff"])
    g.set_assign(synth.warm_assign(n, m))
    g.tick()
    d = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    dp = [x.data_ptr() for x in d]
    out = {"n": n, "m": m, "reps": reps}

    def dev_call(cap=n):
        t0 = time.perf_counter()
        total = g.changes_dev(*dp, cap=cap) if cap else g.changes_dev(cap=0)
        return time.perf_counter() - t0, total

    def host_call():
        t0 = time.perf_counter()
        r = g.changes(cap=n)
        return time.perf_counter() - t0, r[3]

    # the first, complete listing (the checkpoint reset before each call, not timed)
    for form, fn in (("dev", dev_call), ("host", host_call)):
        ts, tot = [], 0
        for _ in range(reps + 1):
            g.changes_reset()
            t, tot = fn()
            ts.append(t)
        out["first_listing_" + form] = dict(med(ts[1:]), changes=tot)
    # nothing changed
    ts_c, ts_d, ts_h = [], [], []
    for _ in range(reps + 1):
        ts_c.append(dev_call(0)[0]); ts_d.append(dev_call()[0]); ts_h.append(host_call()[0])
    out["nothing_count_only_dev"] = med(ts_c[1:])
    out["nothing_dev"] = med(ts_d[1:])
    out["nothing_host"] = med(ts_h[1:])
    # one node flipped dead + a tick; 10 % of the nodes flipped + a tick (a different set each call)
    rng = np.random.default_rng(1)
    for name, frac in (("one_node", None), ("ten_percent", 0.10)):
        for form, fn in (("dev", dev_call), ("host", host_call)):
            ts, tots = [], []
            for k in range(reps + 1):
                alive = np.ones(m, np.uint8)
                if frac is None:
                    alive[int(rng.integers(0, m))] = 0
                else:
                    alive[rng.choice(m, int(m * frac), replace=False)] = 0
                g.set_alive_all(alive)
                g.tick()
                t, tot = fn()
                ts.append(t); tots.append(tot)
            out[name + "_" + form] = dict(med(ts[1:]), changes=int(np.median(tots[1:])))
    # baseline: the column to the host and a numpy diff against the previous copy
    prev = g.get_assign()
    ts, td = [], []
    for _ in range(reps + 1):
        alive = np.ones(m, np.uint8)
        alive[rng.choice(m, m // 10, replace=False)] = 0
        g.set_alive_all(alive)
        g.tick()
        t0 = time.perf_counter()
        cur = g.get_assign()
        t1 = time.perf_counter()
        rows = np.flatnonzero(cur != prev)
        old, new = prev[rows], cur[rows]
        t2 = time.perf_counter()
        ts.append(t2 - t0); td.append(t1 - t0)
        prev = cur
    out["baseline_get_assign_diff"] = dict(med(ts[1:]), get_assign_us=float(np.median(td[1:])) * 1e6, changes=int(len(rows)))
    g.changes()   # (drain)
    g.close()
    return out


if __name__ == "__main__":
    res = {"changes": main(int(sys.argv[1]) if len(sys.argv) > 1 else 10)}
    print(json.dumps(res))
    if os.environ.get("PROBE_OUT"):
        with open(os.environ["PROBE_OUT"], "w") as f:
            json.dump(res, f, indent=1)
