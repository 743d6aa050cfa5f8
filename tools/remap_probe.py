"""rio_gp_remap_nodes on config 3 (10 M rows x 1 024 nodes, warm, after a tick): drop one node, drop 10 % of the nodes, a pure
reversal (and one node dropped with the last node moved into its id), each with the change feed in use and without it — and, in the same run, what a host has to do for the same effect
without the call (get_assign + get_objects + numpy + set_assign + set_object_attrs + set_nodes).  Per case: warm-up runs, then
REPS timed runs from the same restored table; median, min and max of the call's wall time and of the device time between two HIP
events around it, the bytes the rule says must move (8 B read per row, 12 B with the feed's checkpoint, plus 1 KiB per column
and tile of 256 rows in which a value changes) and the rate that makes.

    python tools/remap_probe.py [--n ROWS] [--reps 7] [--out profiles/remap_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import rio_gp  # noqa: E402
import spec_remap as spec  # noqa: E402
import synth  # noqa: E402

NONE = 0xFFFFFFFF


def summary(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def changed_tiles(a, b):
    n = len(a) // 256 * 256
    d = (a != b)
    return int(d[:n].reshape(-1, 256).any(axis=1).sum()) + int(d[n:].any())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remap_probe.json"))
    a = ap.parse_args()
    cfg = synth.config("c3", n_override=a.n) if a.n else synth.config("c3")
    n, m = cfg["n"], cfg["m"]
    g = rio_gp.GpuPlacement(n, m)
    g.set_nodes(cfg["cap"], cfg["alive"])
    g.set_objects(n, cfg["load"], cfg["aff"])
    g.tick()
    assign0 = g.get_assign()
    rng = np.random.default_rng(1)
    swap = np.arange(m, dtype=np.uint32)     # the last node takes the freed id: only the rows of those two nodes change
    swap[m // 3], swap[m - 1] = NONE, m // 3
    maps = {"drop_one": spec.stable_map(m, [m // 3]), "drop_one_last_into_hole": swap,
            "drop_10pct": spec.stable_map(m, rng.choice(m, m // 10, replace=False)),
            "reversal": np.arange(m, dtype=np.uint32)[::-1].copy()}
    out = {"rows": n, "nodes": m, "reps": a.reps, "cases": {}}

    def restore(feed):
        g.set_nodes(cfg["cap"], cfg["alive"])
        g.set_objects(n, cfg["load"], cfg["aff"])
        g.set_assign(assign0)
        g.get_nodes()
        if feed:
            g.changes_dev(cap=0)       # (allocates B) ...
            while g.changes(cap=n)[3]:  # ... and consumes everything: B == A
                pass

    for feed in (False, True):
        for name, mp in maps.items():
            want = spec.remap(assign0, cfg["aff"], n, m, mp, False, B=assign0 if feed else None)
            wall, dev = [], []
            for r in range(a.warmup + a.reps):
                restore(feed)
                g.sync()
                g.timer_begin()
                t0 = time.perf_counter()
                ev = g.remap_nodes(mp)
                t1 = time.perf_counter()
                ms = g.timer_end()
                assert ev == want["evicted"]
                if r >= a.warmup:
                    wall.append((t1 - t0) * 1e6)
                    dev.append(ms * 1e3)
            assert np.array_equal(g.get_assign(), want["assign"])
            tiles = changed_tiles(assign0, want["assign"]) + changed_tiles(cfg["aff"], want["aff"])
            if feed:
                tiles += changed_tiles(assign0, want["B"])
            rd = n * (12 if feed else 8)
            byt = rd + tiles * 1024
            out["cases"]["%s%s" % (name, "_feed" if feed else "")] = {
                "evicted": ev, "wall_us": summary(wall), "device_us": summary(dev), "bytes_read": rd, "bytes_written": tiles * 1024,
                "bytes_per_row": round(byt / n, 2), "GBps_at_device_median": round(byt / statistics.median(dev) / 1e3, 1)}
            print(name, "feed" if feed else "no feed", out["cases"]["%s%s" % (name, "_feed" if feed else "")], flush=True)
    # the same effect through the calls a host had before: whole columns over PCIe, both ways
    host = []
    mp = maps["drop_one"]
    for r in range(3):
        restore(False)
        g.sync()
        t0 = time.perf_counter()
        asg = g.get_assign()
        load, aff = g.get_objects()
        cap, alive, _ = g.get_nodes()
        w = spec.remap(asg, aff, n, m, mp, False, cap=cap, alive=alive)
        g.set_assign(w["assign"])
        idx = np.flatnonzero(w["aff"] != aff).astype(np.uint32)
        if len(idx):
            g.set_object_attrs(idx, aff=w["aff"][idx])
        g.set_nodes(w["cap"], w["alive"])
        host.append((time.perf_counter() - t0) * 1e3)
    out["host_route_drop_one_ms"] = summary(host)
    out["ratio_host_route_to_call"] = round(statistics.median(host) * 1e3 / out["cases"]["drop_one"]["wall_us"]["median"], 1)
    print("host route (ms)", out["host_route_drop_one_ms"], "ratio", out["ratio_host_route_to_call"], flush=True)
    g.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
