#!/usr/bin/env python3
"""rio_gp_rows_on_nodes on config 3 (10 M x 1 024, Zipf) and on a table beyond the Infinity Cache (40 M x 1 024): wall clock of
the full index (_dev, into torch buffers), a one-node query (the node that holds most rows, and a typical one), counts only, and
the baseline they replace: rio_gp_get_assign + the numpy filter.  Prints one JSON line with the byte counts of each pass (column
reads, matrix traffic, listed rows) so that a kernel trace of the same run (rocprofv3 --kernel-trace --stats) can be read against
them.  Usage: node_index_probe.py [n ...]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np
import torch
import rio_gp, synth

REPS = 20


def timed(fn, reps=REPS):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e6, float(np.min(ts)) * 1e6


def matrix_entries(n, s):   # NiPlan (placement_kernels.hip: ni_plan) without a lab knob
    nt = max(1, min((n + 1023) // 1024, max(1, min(8192, (1 << 21) // s))))
    T = ((n + nt - 1) // nt + 255) // 256 * 256
    return s * ((n + T - 1) // T), T


def probe(n):
    cfg = synth.config("c3", n_override=n)
    m = cfg["m"]
    g = rio_gp.GpuPlacement(n, m)
    g.set_nodes(cfg["cap"], cfg["alive"])
    g.set_objects(n, cfg["load"], cfg["aff"])
    g.tick()
    a = g.get_assign()
    cnt = np.bincount(a[a < m], minlength=m)
    big, typ = int(cnt.argmax()), int(np.argsort(cnt)[m // 2])
    d_off = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    d_rows = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    out = {"n": n, "m": m, "placed": int(cnt.sum()), "rows_on_biggest": int(cnt[big]), "rows_on_typical": int(cnt[typ])}
    for name, nodes, listed in (("full", None, int(cnt.sum())), ("one_node_biggest", [big], int(cnt[big])),
                                ("one_node_typical", [typ], int(cnt[typ]))):
        s = m if nodes is None else 1
        E, T = matrix_entries(n, s)
        us, us_min = timed(lambda: g.rows_on_nodes_dev(d_off.data_ptr(), d_rows.data_ptr(), n, nodes))
        cus, cus_min = timed(lambda: g.rows_on_nodes_dev(d_off.data_ptr(), 0, 0, nodes))
        # bytes: count = column + matrix write; scan = matrix read (reduce) + read + write (apply); scatter = column + matrix
        # read + listed rows
        b = {"count": 4 * n + 4 * E, "scan": 12 * E, "scatter": 4 * n + 4 * E + 4 * listed}
        total = sum(b.values())
        out[name] = {"call_us": us, "call_us_min": us_min, "counts_only_us": cus, "counts_only_us_min": cus_min, "listed": listed,
                     "matrix_entries": E, "tile_rows": T, "bytes": b, "frac_of_8TBps": total / (us_min * 1e-6) / 8e12}
    # baseline: the whole column to the host, then numpy (the full index: a stable argsort; one node: a filter)
    def base_full():
        x = g.get_assign()
        k = np.flatnonzero(x < m)
        return k[np.argsort(x[k], kind="stable")]
    out["baseline_get_assign_us"] = timed(lambda: g.get_assign(), 10)[0]
    out["baseline_full_us"] = timed(base_full, 5)[0]
    out["baseline_one_node_us"] = timed(lambda: np.flatnonzero(g.get_assign() == big), 10)[0]
    g.close()
    return out


if __name__ == "__main__":
    sizes = [int(x) for x in sys.argv[1:]] or [10_000_000, 40_000_000]
    print(json.dumps({"node_index": [probe(n) for n in sizes]}))
