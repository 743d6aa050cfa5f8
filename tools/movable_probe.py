#!/usr/bin/env python3
"""rio_gp_rebalance with immovable classes (rio_gp_set_class_movable, DESIGN.md section 2 rule 13) on the table of
tools/rebalance_order_probe.py: config 3 (10 M x 1 024), warm after a tick, loads folded from 10^7 Zipf requests, 10 % of the
capacities cut by 30 %, unlimited moves.  Every row carries class row % 8.

Three tables of flags — no immovable class (the setter never called: the kernels without the class column), 1 of 8 classes
immovable, 4 of 8 — in both orders of the cut, all on the same restored column in the same session, alternating, `reps`
(>= 20) timed calls each after one untimed call: wall clock around the whole call, which ends with a stream wait; the column is
put back and `used` rebuilt outside the timed region.  Per case: median, min, max of the call, its ratio to the no-immovable
call of the same order and run, and surplus_rows, moved_rows, stayed_rows, nodes_over_after (fewer candidates change the work
as well as the bytes: the class-aware passes read 13 B per row instead of 12).
Prints one JSON line.  Usage: movable_probe.py [reps] [--out profiles/movable_probe.json] [--only none|1_of_8|4_of_8]
--only runs one table of flags alone (no ratios): the form for a kernel trace, whose per-kernel sums then belong to one case."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np
import rio_gp, synth

ORDERS = (("row_order", rio_gp.REBALANCE_ROW_ORDER), ("by_load", rio_gp.REBALANCE_BY_LOAD))
TABLES = (("none", None), ("1_of_8", [1, 1, 1, 0, 1, 1, 1, 1]), ("4_of_8", [0, 1, 0, 1, 0, 1, 0, 1]))


def main(reps, only=None):
    tables = [t for t in TABLES if only in (None, t[0])]
    cfg = synth.config("c3")
    n, m = cfg["n"], cfg["m"]
    g = rio_gp.GpuPlacement(n, m)
    alive = np.ones(m, np.uint8)
    g.set_nodes(np.full(m, rio_gp.CAP_INF, np.uint64), alive)
    g.set_objects(n, cfg["load"], cfg["aff"])
    rng = np.random.default_rng(11)
    hits = np.bincount(((rng.zipf(1.1, n) - 1) % n).astype(np.uint32), minlength=n).astype(np.uint32)
    g.hits_merge(hits)
    g.load_fold(32768, 1, 1, 1_000_000)
    load = g.get_objects()[0]
    cap = synth.uniform_cap(load, m)
    g.set_nodes(cap, alive)
    g.set_assign(synth.warm_assign(n, m))
    g.tick()
    col = g.get_assign()
    cut = cap.copy()
    cut[::10] = cut[::10] * np.uint64(7) // np.uint64(10)
    g.set_nodes(cut, alive)
    ts = {(t, o): [] for t, _ in tables for o, _ in ORDERS}
    st = {}
    classes_set = False
    for it in range(reps + 1):
        for tname, flags in tables:         # alternating: drift of the machine hits every case alike
            if flags is not None and not classes_set:
                g.set_classes(0, (np.arange(n) % 8).astype(np.uint8))
                classes_set = True
            if it or flags is not None:     # (the first `none` round runs on a handle that never called the setter)
                g.set_class_movable(flags)
            for oname, order in ORDERS:
                g.set_assign(col)
                g.get_nodes()               # (rebuilds `used` outside the timed call)
                g.sync()
                t0 = time.perf_counter()
                st[tname, oname], *_ = g.rebalance(list_moves=False, order=order)
                if it:
                    ts[tname, oname].append(time.perf_counter() - t0)
    out = {"n": n, "m": m, "reps": reps, "load_max": int(load.max()), "load_mean": float(load.mean()), "cap": int(cap[0])}
    for (tname, oname), v in ts.items():
        t, s = np.array(v) * 1e6, st[tname, oname]
        out.setdefault(tname, {})[oname] = {
            "call_us": float(np.median(t)), "call_us_min": float(t.min()), "call_us_max": float(t.max()),
            "surplus_rows": s["surplus_rows"], "selected_rows": s["selected_rows"], "moved_rows": s["moved_rows"],
            "stayed_rows": s["stayed_rows"], "nodes_over_before": s["nodes_over_before"], "nodes_over_after": s["nodes_over_after"]}
    for tname, _ in ([] if only else TABLES[1:]):
        for oname, _ in ORDERS:
            out[tname][oname]["over_none"] = out[tname][oname]["call_us"] / out["none"][oname]["call_us"]
    g.close()
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    path = None
    if "--out" in args:
        k = args.index("--out")
        path = args[k + 1]
        del args[k:k + 2]
    only = None
    if "--only" in args:
        k = args.index("--only")
        only = args[k + 1]
        del args[k:k + 2]
    res = {"movable": main(max(int(args[0]) if args else 20, 20), only)}
    line = json.dumps(res)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
    print(line)
