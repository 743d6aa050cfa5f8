#!/usr/bin/env python3
"""rio_gp_rebalance on config 3 (10 M x 1 024, Zipf loads, the warm table of synth.py) in three scenarios: (1) nothing over
target, (2) 10 % of the nodes lose 30 % of their capacity, (3) scale-out: 64 empty nodes join, balanced targets, max_moves 10^4
and unlimited.  Wall clock per call (the table is put back between calls: the copy is not timed), the moves made, and the
fraction of the 8 TB/s roofline against 12 B per row read + 4 B per moved row written.  Prints one JSON line.
Usage: rebalance_probe.py [reps]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np
import rio_gp, synth


def timed_calls(g, col, reps, reset, **kw):
    ts, st = [], None
    for _ in range(reps + 1):
        if reset:
            g.set_assign(col)
            g.get_nodes()   # (rebuilds `used` outside the timed call)
        t0 = time.perf_counter()
        st, *_ = g.rebalance(list_moves=False, **kw)
        ts.append(time.perf_counter() - t0)
    ts = ts[1:]  # the first call allocates the scratch
    return float(np.median(ts)) * 1e6, float(np.min(ts)) * 1e6, st


def row(n, us, us_min, st):
    b = 12 * n + 4 * st["moved_rows"]
    return {"call_us": us, "call_us_min": us_min, "moved_rows": st["moved_rows"], "selected_rows": st["selected_rows"],
            "surplus_rows": st["surplus_rows"], "stayed_rows": st["stayed_rows"], "nodes_over_before": st["nodes_over_before"],
            "nodes_over_after": st["nodes_over_after"], "bytes": b, "frac_of_8TBps": b / (us_min * 1e-6) / 8e12}


def main(reps):
    cfg = synth.config("c3w")
    n, m = cfg["n"], cfg["m"]
    cap, alive, col = cfg["cap"].copy(), np.ones(m, np.uint8), cfg["cur"]
    g = rio_gp.GpuPlacement(n, m + 64)
    g.set_nodes(cap, alive)
    g.set_objects(n, cfg["load"], cfg["aff"])
    g.set_assign(col)
    out = {"n": n, "m": m, "reps": reps}
    inf = np.full(m, rio_gp.CAP_INF, np.uint64)
    out["nothing_over"] = row(n, *timed_calls(g, col, reps, False, target=inf))
    out["nothing_over_caps"] = row(n, *timed_calls(g, col, reps, False))
    cut = cap.copy()
    cut[::10] = cut[::10] * np.uint64(7) // np.uint64(10)
    g.set_nodes(cut, alive)
    out["capacity_cut"] = row(n, *timed_calls(g, col, reps, True))
    cap2 = np.concatenate([cut, np.full(64, int(cap.mean()), np.uint64)])
    alive2 = np.ones(m + 64, np.uint8)
    g.set_nodes(cap2, alive2)
    g.set_assign(col)
    T = rio_gp.balanced_targets(cap2, g.get_nodes()[2], alive2, 20)
    out["scale_out_1e4"] = row(n, *timed_calls(g, col, reps, True, target=T, max_moves=10_000))
    out["scale_out_all"] = row(n, *timed_calls(g, col, reps, True, target=T))
    # what the host route costs before it decides anything: the column to the host
    g.set_assign(col)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); g.get_assign(); ts.append(time.perf_counter() - t0)
    out["get_assign_us"] = float(np.median(ts)) * 1e6
    g.close()
    return out


if __name__ == "__main__":
    print(json.dumps({"rebalance": main(int(sys.argv[1]) if len(sys.argv) > 1 else 10)}))
