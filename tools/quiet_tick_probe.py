#!/usr/bin/env python3
"""Quiet committed ticks of config 3 (one launch each: the chained k_scan adds the kept loads into `used` and stores the verdict
rows itself) with the adds spread over R replicas of the `used` buffer (lab knob RIO_GP_CHAIN_REPS; 0 = no adds at all, a
timing run whose `used` is wrong), alternating in ONE run; final table, `used` and counters compared between the runs that add.
Usage: quiet_tick_probe.py [ticks=400] [config=c3|c4|c2] [reps,reps,...]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np
import rio_gp, synth
if os.environ.get("PROBE_LAB"):  # another lab build of the same sources (A/B of a compile-time variant)
    rio_gp.LAB_PATH = os.environ["PROBE_LAB"]
ticks = int(sys.argv[1]) if len(sys.argv) > 1 else 400
cfg = synth.config(sys.argv[2] if len(sys.argv) > 2 else "c3")
reps = [int(x) for x in (sys.argv[3] if len(sys.argv) > 3 else "1,4,8,16,32,0").split(",")]
n, m = cfg["n"], cfg["m"]
out = {"n": n, "m": m, "ticks": ticks, "runs": []}
final = {}
for rnd in range(2):
    for r in reps:
        os.environ["RIO_GP_CHAIN_REPS"] = str(r)
        g = rio_gp.LabPlacement(n, m)
        g.set_nodes(cfg["cap"], cfg["alive"])
        g.set_objects(n, cfg["load"], cfg["aff"])
        g.set_assign(cfg["cur"])
        for _ in range(20):
            g.tick_async()
        g.tick_wait(); g.sync()
        c0 = g.chained_scans()
        t0 = time.perf_counter()
        ts = []
        for _ in range(ticks):
            ta = time.perf_counter()
            g.tick_async()
            ts.append(time.perf_counter() - ta)
        t1 = time.perf_counter()
        sts = g.tick_wait()
        t2 = time.perf_counter()
        us = (t2 - t0) / ticks * 1e6
        out["runs"].append({"reps": r, "round": rnd, "us_per_tick": round(us, 2), "host_enqueue_us_per_tick": round((t1 - t0) / ticks * 1e6, 2),
                            "tick_async_median_us": round(float(np.median(ts)) * 1e6, 2),
                            "chained": g.chained_scans() - c0, "slow_path_ticks": sum(x["slow_path"] for x in sts)})
        if r:
            final[(r, rnd)] = (g.get_assign(), g.get_nodes()[2], sts[-1])
        g.close()
        print(json.dumps(out["runs"][-1]), flush=True)
a0 = next(iter(final.values()))
out["equal"] = all(np.array_equal(a0[0], v[0]) and np.array_equal(a0[1], v[1]) and a0[2] == v[2] for v in final.values())
print(json.dumps(out))
