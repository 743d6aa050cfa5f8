#!/usr/bin/env python3
"""The row-sharded rebalance (rio_gp_shard_rebalance_*, ShardedSolver.rebalance) beside the single-handle rio_gp_rebalance, in
the same run, on the same warm config-3 table (10 M x 1 024, Zipf loads) and the three scenarios of tools/rebalance_probe.py:
(1) nothing over target, (2) 10 % of the nodes lose 30 % of their capacity, (3) scale-out: 64 empty nodes join, balanced
targets, max_moves 10^4 and unlimited.  Legs: (a) rio_gp_rebalance on one handle; (b) the protocol with G = 1 handle; (c) G = 8
handles on the ONE device, driven by one process over LocalExchange (the "all-gather" is a concatenation on the device: nothing
here crosses xGMI).  Wall clock per call without a move listing, median and minimum over `reps` calls after one warm-up call
(it allocates the scratch); the table is put back between calls outside the timed region.  The legs are interleaved scenario by
scenario so that they see the same clocks.  Prints one JSON line.
Usage: shard_rebalance_probe.py [reps] [rows]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np
import torch
import rio_gp, sharded, synth


class Leg:
    def __init__(self, cfg, bounds, sharded_route):
        self.n, self.m = cfg["n"], cfg["m"]
        self.b = bounds
        self.col = cfg["cur"]
        stream = torch.cuda.Stream(torch.device("cuda", 0))
        self.gs = []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            g = rio_gp.GpuPlacement(hi - lo, self.m + 64)
            g.set_nodes(cfg["cap"], np.ones(self.m, np.uint8))
            g.set_objects(hi - lo, cfg["load"][lo:hi], cfg["aff"][lo:hi])
            g.set_assign(self.col[lo:hi])
            self.gs.append(g)
        self.stream, self.sharded_route, self.sol = stream, sharded_route, None
        self.make_solver()

    def make_solver(self):   # (the record buffers are sized by the node count: made again when it changes)
        if self.sharded_route:
            engines = [sharded.HipShardEngine(g, 0, self.stream) for g in self.gs]
            self.sol = sharded.ShardedSolver(engines, sharded.LocalExchange(len(engines)))

    def set_nodes(self, cap, alive):
        for g in self.gs:
            g.set_nodes(cap, alive)
        self.make_solver()

    def reset(self):
        for g, lo, hi in zip(self.gs, self.b[:-1], self.b[1:]):
            g.set_assign(self.col[lo:hi])
            g.get_nodes()   # (rebuilds `used` outside the timed call)

    def call(self, **kw):
        if self.sol is None:
            return self.gs[0].rebalance(list_moves=False, **kw)[0]
        return self.sol.rebalance(list_moves=False, **kw)[0]

    def timed(self, reps, reset, **kw):
        ts, st = [], None
        for _ in range(reps + 1):
            if reset:
                self.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = self.call(**kw)
            ts.append(time.perf_counter() - t0)
        ts = ts[1:]
        return {"call_us": float(np.median(ts)) * 1e6, "call_us_min": float(np.min(ts)) * 1e6, "moved_rows": st["moved_rows"],
                "selected_rows": st["selected_rows"], "surplus_rows": st["surplus_rows"], "stayed_rows": st["stayed_rows"],
                "nodes_over_before": st["nodes_over_before"], "nodes_over_after": st["nodes_over_after"]}

    def close(self):
        for g in self.gs:
            g.close()


def main(reps, rows):
    cfg = synth.config("c3w", n_override=rows)
    n, m = cfg["n"], cfg["m"]
    cap, alive = cfg["cap"].copy(), np.ones(m, np.uint8)
    legs = {"single": Leg(cfg, [0, n], False), "sharded_g1": Leg(cfg, [0, n], True),
            "sharded_g8": Leg(cfg, sharded.shard_bounds(n, 8), True)}
    out = {"n": n, "m": m, "reps": reps, "legs": list(legs)}

    def scenario(name, reset, **kw):
        out[name] = {k: leg.timed(reps, reset, **kw) for k, leg in legs.items()}
        ref = out[name]["single"]
        for k in legs:   # the legs computed the same thing
            assert all(out[name][k][f] == ref[f] for f in ref if not f.startswith("call_us")), (name, k)

    inf = np.full(m, rio_gp.CAP_INF, np.uint64)
    scenario("nothing_over", False, target=inf)
    cut = cap.copy()
    cut[::10] = cut[::10] * np.uint64(7) // np.uint64(10)
    for leg in legs.values():
        leg.set_nodes(cut, alive)
    scenario("capacity_cut", True)
    cap2 = np.concatenate([cut, np.full(64, int(cap.mean()), np.uint64)])
    alive2 = np.ones(m + 64, np.uint8)
    for leg in legs.values():
        leg.set_nodes(cap2, alive2)
        leg.reset()
    T = rio_gp.balanced_targets(cap2, legs["single"].gs[0].get_nodes()[2], alive2, 20)
    scenario("scale_out_1e4", True, target=T, max_moves=10_000)
    scenario("scale_out_all", True, target=T)
    for leg in legs.values():
        leg.close()
    return out


if __name__ == "__main__":
    print(json.dumps({"shard_rebalance": main(int(sys.argv[1]) if len(sys.argv) > 1 else 10,
                                              int(sys.argv[2]) if len(sys.argv) > 2 else None)}))
