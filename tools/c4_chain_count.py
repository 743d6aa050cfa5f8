#!/usr/bin/env python3
"""Does a quiet tick of config 4 on one GPU (100 M rows x 4 096 nodes) chain?  40 quiet ticks through the lab build: chained
scans counted, us per tick."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import rio_gp, synth
cfg = synth.config("c4")
g = rio_gp.LabPlacement(cfg["n"], cfg["m"])
g.set_nodes(cfg["cap"], cfg["alive"])
g.set_objects(cfg["n"], cfg["load"], cfg["aff"])
g.set_assign(cfg["cur"])
for _ in range(3):
    g.tick_async()
    time.sleep(0.05)
g.tick_wait()
c0 = g.chained_scans()
t0 = time.perf_counter()
for _ in range(40):
    g.tick_async()
sts = g.tick_wait()
us = (time.perf_counter() - t0) / 40 * 1e6
print(json.dumps({"n": cfg["n"], "m": cfg["m"], "chained": g.chained_scans() - c0, "us_per_tick": round(us, 1),
                  "slow_path_ticks": sum(s["slow_path"] for s in sts)}))
g.close()
