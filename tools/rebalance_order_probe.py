#!/usr/bin/env python3
"""rio_gp_rebalance in row order and by load (cfg.order) on config 3 (10 M x 1 024), warm after a tick, after a fold of 10^7
Zipf requests into the loads (so that they are skewed as a measured load is): the same two scenarios as
tools/rebalance_probe.py — (1) 10 % of the capacities cut by 30 %, (2) scale-out onto 64 empty nodes with balanced targets
(slack 20 per mille), unlimited moves.  The capacities are synth.uniform_cap of the FOLDED loads.

Both orders run on the same restored table in the same session, alternating, `reps` (>= 7) timed calls each after one untimed
call (the first call of a scenario allocates scratch): wall clock around the whole call, which ends with a stream wait; the
column is put back and `used` rebuilt outside the timed region.  Per order: median, min, max of the call, and surplus_rows,
moved_rows, stayed_rows, nodes_over_after.  The yardstick for the load-ordered call is the row-order call of the same run plus
one streaming pass of 12 B/row per digit of the threshold search; `tile_pass_us` (= the `nothing over` call: one such pass
with the call's fixed part) is measured here as well.
Prints one JSON line.  Usage: rebalance_order_probe.py [reps] [--out profiles/rebalance_order_probe.json]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np
import rio_gp, synth

ORDERS = (("row_order", rio_gp.REBALANCE_ROW_ORDER), ("by_load", rio_gp.REBALANCE_BY_LOAD))


def scenario(g, col, reps, **kw):
    ts = {name: [] for name, _ in ORDERS}
    st = {}
    for it in range(reps + 1):
        for name, order in ORDERS:      # alternating: drift of the machine hits both alike
            g.set_assign(col)
            g.get_nodes()               # (rebuilds `used` outside the timed call)
            g.sync()
            t0 = time.perf_counter()
            st[name], *_ = g.rebalance(list_moves=False, order=order, **kw)
            if it:
                ts[name].append(time.perf_counter() - t0)
    out = {}
    for name, _ in ORDERS:
        t, s = np.array(ts[name]) * 1e6, st[name]
        out[name] = {"call_us": float(np.median(t)), "call_us_min": float(t.min()), "call_us_max": float(t.max()),
                     "surplus_rows": s["surplus_rows"], "surplus_load": s["surplus_load"], "selected_rows": s["selected_rows"],
                     "moved_rows": s["moved_rows"], "moved_load": s["moved_load"], "stayed_rows": s["stayed_rows"],
                     "nodes_over_before": s["nodes_over_before"], "nodes_over_after": s["nodes_over_after"]}
    out["by_load_over_row_order"] = out["by_load"]["call_us"] / out["row_order"]["call_us"]
    out["moved_rows_ratio"] = out["row_order"]["moved_rows"] / max(out["by_load"]["moved_rows"], 1)
    return out


def main(reps):
    cfg = synth.config("c3")
    n, m = cfg["n"], cfg["m"]
    g = rio_gp.GpuPlacement(n, m + 64)
    alive = np.ones(m, np.uint8)
    g.set_nodes(np.full(m, rio_gp.CAP_INF, np.uint64), alive)
    g.set_objects(n, cfg["load"], cfg["aff"])
    rng = np.random.default_rng(11)
    hits = np.bincount(((rng.zipf(1.1, n) - 1) % n).astype(np.uint32), minlength=n).astype(np.uint32)
    g.hits_merge(hits)
    KEEP, GAIN, LO, HI = 32768, 1, 1, 1_000_000
    fold = g.load_fold(KEEP, GAIN, LO, HI)
    load = g.get_objects()[0] if hasattr(g, "get_objects") else None
    if load is None:
        load = np.clip((cfg["load"].astype(np.uint64) * KEEP >> 16) + hits.astype(np.uint64) * GAIN, LO, HI).astype(np.uint32)
    cap = synth.uniform_cap(load, m)
    g.set_nodes(cap, alive)
    g.set_assign(synth.warm_assign(n, m))
    g.tick()                               # warm: the committed column of the folded loads
    col = g.get_assign()
    out = {"n": n, "m": m, "reps": reps, "fold": dict(fold, keep=KEEP, gain=GAIN, min_load=LO, max_load=HI),
           "load_max": int(load.max()), "load_mean": float(load.mean()), "cap": int(cap[0])}
    # one table pass with the call's fixed part: nothing over target ends after k_shed_hist
    inf, ts = np.full(m, rio_gp.CAP_INF, np.uint64), []
    for it in range(reps + 1):
        g.sync()
        t0 = time.perf_counter()
        g.rebalance(target=inf, list_moves=False)
        if it:
            ts.append(time.perf_counter() - t0)
    out["tile_pass_us"] = float(np.median(ts)) * 1e6
    cut = cap.copy()
    cut[::10] = cut[::10] * np.uint64(7) // np.uint64(10)
    g.set_nodes(cut, alive)
    out["capacity_cut"] = scenario(g, col, reps)
    cap2 = np.concatenate([cut, np.full(64, int(cap.mean()), np.uint64)])
    alive2 = np.ones(m + 64, np.uint8)
    g.set_nodes(cap2, alive2)
    g.set_assign(col)
    T = rio_gp.balanced_targets(cap2, g.get_nodes()[2], alive2, 20)
    out["scale_out_all"] = scenario(g, col, reps, target=T)
    g.close()
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    path = None
    if "--out" in args:
        k = args.index("--out")
        path = args[k + 1]
        del args[k:k + 2]
    res = {"rebalance_order": main(max(int(args[0]) if args else 7, 7))}
    line = json.dumps(res)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
    print(line)
