#!/usr/bin/env python3
"""Workload for the PMC passes over QUIET committed ticks: config 3 settled by a few ticks, then 30 quiet asynchronous ticks
(the chained scan per tick, and whatever else the build runs for one), then the stream probes that calibrate FETCH_SIZE /
WRITE_SIZE (tools/pmc_traffic.py).  PROBE_LAB: another lab build of the library (before / after).  Usage: pmc_quiet_workload.py [ticks]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import rio_gp, synth
if os.environ.get("PROBE_LAB"):
    rio_gp.LAB_PATH = os.environ["PROBE_LAB"]
ticks = int(sys.argv[1]) if len(sys.argv) > 1 else 30
cfg = synth.config("c3")
g = rio_gp.LabPlacement(cfg["n"], cfg["m"])
g.set_nodes(cfg["cap"], cfg["alive"])
g.set_objects(cfg["n"], cfg["load"], cfg["aff"])
g.set_assign(cfg["cur"])
for _ in range(3):
    g.tick_async()
    time.sleep(0.01)
g.tick_wait()
for _ in range(ticks):
    g.tick_async()
g.tick_wait()
for mode in (4, 0, 3):
    g.stream_probe(mode, 10)
g.close()
