#!/usr/bin/env python3
"""The load-ordered cut of the row-sharded rebalance (rio_gp_shard_rebalance_begin_ordered + the threshold passes,
ShardedSolver.rebalance(order=1)) on config 3 (10 M x 1 024) after a fold of 10^7 Zipf requests into the loads — the table of
tools/rebalance_order_probe.py — over 8 shards on ONE device, driven by one process over LocalExchange (the "all-gather" is a
concatenation on the device: nothing here crosses xGMI).  Scenarios: (1) 10 % of the capacities cut by 30 %, (2) scale-out onto
64 empty nodes with balanced targets (slack 20 per mille), unlimited moves.

In the same run, alternating, on the same restored table: the sharded protocol in row order (the protocol as it was) and by load,
and the single-handle rio_gp_rebalance in both orders on the whole table.  `reps` (>= 7) timed calls each after one untimed call
(it allocates scratch): wall clock around the whole call without a move listing, which ends with a stream wait; the column is put
back and `used` rebuilt outside the timed region.  The legs must report the same counters per order (asserted).

`steps` drives the load-ordered protocol by hand with a device synchronise after every step, so each figure includes one: the
sum is above the call's time.  `pass_us` = one histogram pass on the 8 shards + the exchange of its record + the 8 picks.
Prints one JSON line.  Usage: shard_rebalance_order_probe.py [reps] [--out profiles/shard_rebalance_order_probe.json]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np
import torch
import rio_gp, sharded, synth

G = 8
ORDERS = (("row_order", rio_gp.REBALANCE_ROW_ORDER), ("by_load", rio_gp.REBALANCE_BY_LOAD))
KEYS = ("surplus_rows", "surplus_load", "selected_rows", "moved_rows", "moved_load", "stayed_rows", "nodes_over_before",
        "nodes_over_after")


class Leg:
    """The table on one handle (bounds = [0, n]: rio_gp_rebalance) or on the handles of its shards (the protocol)."""

    def __init__(self, n, m, load, aff, cap, col, bounds, protocol):
        self.b, self.col = bounds, col
        self.stream = torch.cuda.Stream(torch.device("cuda", 0))
        self.gs = []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            g = rio_gp.GpuPlacement(hi - lo, m + 64)
            g.set_nodes(cap, np.ones(m, np.uint8))
            g.set_objects(hi - lo, load[lo:hi], aff[lo:hi])
            g.set_assign(col[lo:hi])
            self.gs.append(g)
        self.protocol, self.sol = protocol, None
        self.make_solver()

    def make_solver(self):   # (the record buffers are sized by the node count: made again when it changes)
        if self.protocol:
            self.engines = [sharded.HipShardEngine(g, 0, self.stream) for g in self.gs]
            self.sol = sharded.ShardedSolver(self.engines, sharded.LocalExchange(len(self.engines)))

    def set_nodes(self, cap, alive):
        for g in self.gs:
            g.set_nodes(cap, alive)
        self.make_solver()

    def reset(self):
        for g, lo, hi in zip(self.gs, self.b[:-1], self.b[1:]):
            g.set_assign(self.col[lo:hi])
            g.get_nodes()   # (rebuilds `used` outside the timed call)
        torch.cuda.synchronize()

    def call(self, order, **kw):
        if self.sol is None:
            return self.gs[0].rebalance(list_moves=False, order=order, **kw)[0]
        return self.sol.rebalance(list_moves=False, order=order, **kw)[0]

    def close(self):
        for g in self.gs:
            g.close()


def stepwise(leg, reps, target=None, whole_search=False):
    """The load-ordered protocol step by step (a synchronise after each): median microseconds per step over `reps` runs.
    whole_search: the gathered X is made to report a largest load of 2^32 - 1, so every pass from bit 32 down runs — the
    protocol without the start at the largest load, for the same result."""
    sol, E = leg.sol, leg.engines
    R, m = len(E), leg.gs[0].num_nodes
    rec, timed = {}, [False]

    def step(name, fn):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if timed[0]:
            rec.setdefault(name, []).append(time.perf_counter() - t0)
        return out

    info = {}
    for it in range(reps + 1):
        leg.reset()
        timed[0] = it > 0   # (the first run is the warm-up: its times are dropped)
        nr = step("begin", lambda: [e.rebalance_begin(r, R, target, rio_gp.CAP_INF, 0, False, x, order=rio_gp.REBALANCE_BY_LOAD)
                                    for r, (e, x) in enumerate(zip(E, sol.X))][0])
        xg = step("gather_x", lambda: sol._gather(sol.X, out=sol.XG[0]))
        if whole_search:
            with E[0].ctx():
                xg.view(R, -1)[:, 2 * m] = 0xFFFFFFFF
            torch.cuda.synchronize()
        over = step("cut", lambda: [e.rebalance_cut(xg, y) for e, y in zip(E, sol.Y)][0])
        passes, words = [e.rebalance_threshold_plan() for e in E][0]
        H = [e.new_buffer(words) for e in E]
        torch.cuda.synchronize()
        t_pass = 0.0
        for p in range(passes):
            t0 = time.perf_counter()
            step("hist", lambda: [e.rebalance_threshold_hist(p, hb) for e, hb in zip(E, H)])
            hg = step("gather_h", lambda: sol._gather(H))
            step("pick_last" if p + 1 == passes else "pick",
                 lambda: [e.rebalance_threshold_pick(p, hg, y if p + 1 == passes else None) for e, y in zip(E, sol.Y)])
            t_pass += time.perf_counter() - t0
        if timed[0]:
            rec.setdefault("passes_total", []).append(t_pass)
        sg = step("gather_s", lambda: sol._gather(sol.Y))
        total = step("select", lambda: [e.rebalance_select(sg, y) for e, y in zip(E, sol.Y)][0][1])
        rounds = 0
        if total:
            yg = step("gather_y", lambda: sol._gather(sol.Y))
            pend = step("merge", lambda: [e.rebalance_merge(yg) for e in E][0])
            while pend[0] and rounds < nr:
                step("fill", lambda: [e.rebalance_fill(rounds, y) for e, y in zip(E, sol.Y)])
                yg = step("gather_y", lambda: sol._gather(sol.Y))
                pend = step("merge", lambda: [e.rebalance_merge(yg) for e in E][0])
                rounds += 1
        local = step("finish", lambda: [e.rebalance_finish(False) for e in E])
        info = {"nodes_over": over, "passes": passes, "record_words": words, "digit_bits": (words // over).bit_length() - 1,
                "rounds_run": rounds, "moved_rows": sum(l[0]["moved_rows"] for l in local)}
    med = lambda name: float(np.median(rec[name])) * 1e6 if name in rec else 0.0
    per_call = lambda name: med(name) * (len(rec[name]) / reps) if name in rec else 0.0   # steps that run several times a call
    out = dict(info)
    out["step_us"] = {k: med(k) for k in ("begin", "gather_x", "cut", "hist", "gather_h", "pick", "pick_last", "gather_s", "select",
                                         "gather_y", "merge", "fill", "finish")}
    out["passes_total_us"] = med("passes_total")
    out["pass_us"] = out["passes_total_us"] / max(info["passes"], 1)
    out["other_steps_us"] = sum(per_call(k) for k in ("begin", "gather_x", "cut", "gather_s", "select", "gather_y", "merge", "fill",
                                                      "finish"))
    return out


def scenario(legs, reps, **kw):
    ts = {(k, name): [] for k in legs for name, _ in ORDERS}
    st = {}
    for it in range(reps + 1):
        for k, leg in legs.items():           # alternating: drift of the machine hits every leg and order alike
            for name, order in ORDERS:
                leg.reset()
                t0 = time.perf_counter()
                st[k, name] = leg.call(order, **kw)
                if it:
                    ts[k, name].append(time.perf_counter() - t0)
    out = {}
    for k in legs:
        out[k] = {}
        for name, _ in ORDERS:
            t, s = np.array(ts[k, name]) * 1e6, st[k, name]
            assert all(s[f] == st["single", name][f] for f in KEYS), (k, name, s, st["single", name])
            out[k][name] = dict({"call_us": float(np.median(t)), "call_us_min": float(t.min()), "call_us_max": float(t.max())},
                                **{f: s[f] for f in KEYS})
        out[k]["by_load_over_row_order"] = out[k]["by_load"]["call_us"] / out[k]["row_order"]["call_us"]
        out[k]["moved_rows_ratio"] = out[k]["row_order"]["moved_rows"] / max(out[k]["by_load"]["moved_rows"], 1)
    out["sharded_over_single_by_load"] = out["sharded"]["by_load"]["call_us"] / out["single"]["by_load"]["call_us"]
    out["steps"] = stepwise(legs["sharded"], reps, **kw)
    out["steps_whole_search"] = stepwise(legs["sharded"], reps, whole_search=True, **kw)
    for k in ("steps", "steps_whole_search"):   # the same cut, wherever the search starts
        assert out[k]["moved_rows"] == out["sharded"]["by_load"]["moved_rows"], (k, out[k])
    return out


def main(reps):
    cfg = synth.config("c3")
    n, m = cfg["n"], cfg["m"]
    alive = np.ones(m, np.uint8)
    g = rio_gp.GpuPlacement(n, m + 64)
    g.set_nodes(np.full(m, rio_gp.CAP_INF, np.uint64), alive)
    g.set_objects(n, cfg["load"], cfg["aff"])
    rng = np.random.default_rng(11)
    hits = np.bincount(((rng.zipf(1.1, n) - 1) % n).astype(np.uint32), minlength=n).astype(np.uint32)
    g.hits_merge(hits)
    KEEP, GAIN, LO, HI = 32768, 1, 1, 1_000_000
    fold = g.load_fold(KEEP, GAIN, LO, HI)
    load = g.get_objects()[0]              # the folded loads, for the shards' handles
    cap = synth.uniform_cap(load, m)
    g.set_nodes(cap, alive)
    g.set_assign(synth.warm_assign(n, m))
    g.tick()                               # warm: the committed column of the folded loads
    col = g.get_assign()
    g.close()
    legs = {"single": Leg(n, m, load, cfg["aff"], cap, col, [0, n], False),
            "sharded": Leg(n, m, load, cfg["aff"], cap, col, sharded.shard_bounds(n, G), True)}
    out = {"n": n, "m": m, "shards": G, "reps": reps, "fold": dict(fold, keep=KEEP, gain=GAIN, min_load=LO, max_load=HI),
           "load_max": int(load.max()), "load_mean": float(load.mean()), "cap": int(cap[0])}
    cut = cap.copy()
    cut[::10] = cut[::10] * np.uint64(7) // np.uint64(10)
    for leg in legs.values():
        leg.set_nodes(cut, alive)
    out["capacity_cut"] = scenario(legs, reps)
    cap2 = np.concatenate([cut, np.full(64, int(cap.mean()), np.uint64)])
    alive2 = np.ones(m + 64, np.uint8)
    for leg in legs.values():
        leg.set_nodes(cap2, alive2)
        leg.reset()
    T = rio_gp.balanced_targets(cap2, legs["single"].gs[0].get_nodes()[2], alive2, 20)
    out["scale_out_all"] = scenario(legs, reps, target=T)
    for leg in legs.values():
        leg.close()
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    path = None
    if "--out" in args:
        k = args.index("--out")
        path = args[k + 1]
        del args[k:k + 2]
    res = {"shard_rebalance_order": main(max(int(args[0]) if args else 7, 7))}
    line = json.dumps(res)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
    print(line)
