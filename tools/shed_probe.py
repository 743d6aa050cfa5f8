#!/usr/bin/env python3
"""rio_gp_shed_idle on config 3 (10 M x 1 024), warm after a tick, with the expiry probe's last-seen layout (row r was last seen
at epoch 1 where r % 100 == 0, at epoch 2 where 1 <= r % 100 < 10, at epoch 3 elsewhere) and the rebalance probes' pressure:
10 % of the capacities cut by 30 %.  Every call runs from the same restored table (the assignment column is put back from a
device copy and `used` rebuilt before each run, not timed), the calls of one repetition alternating, `reps` (>= 7) timed runs
each after one untimed run (the first call allocates scratch): wall clock around the whole call, which ends with a stream wait.
  shed_dev              rio_gp_shed_idle_dev, cutoff 4 (every object may go), listing into device arrays, no limit
  shed_dev_cutoff_3     the same with cutoff 3: only the 10 % of the rows seen before epoch 3 may go, the nodes stay over
  shed_count_only       max_rows = 0: the node pass, the selection, the tie walk and the count pass; nothing changes
  nothing_over          targets ~0: the node pass and the call's fixed part
  rebalance_by_load     rio_gp_rebalance, order = by load, no move listing, on the same table: the call whose pass structure this
                        one shares (here the cut capacities leave room elsewhere: its rows move)
  expire_count_only     rio_gp_expire_dev without arrays, cutoff 3
  host_route            what a host does without the call: rio_gp_get_assign + rio_gp_get_seen + rio_gp_get_objects, one numpy
                        lexsort by (node, stamp descending, row) with a segmented prefix sum, rio_gp_remove_batch of the surplus
selection_passes: the histogram passes the call launches for this table, from the plan the library uses (digit width from the
slot count; the passes above the highest bit in which two candidate stamps differ are skipped).
Prints one JSON line.  Usage: shed_probe.py [reps] [--out profiles/shed_probe.json]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np
import rio_gp, synth

NONE = 0xFFFFFFFF


def stat(ts):
    t = np.array(ts) * 1e6
    return {"call_us": float(np.median(t)), "call_us_min": float(t.min()), "call_us_max": float(t.max())}


def selection_passes(slots, stamps):
    """sh_sel_plan + launch_ish_select's skip (rio-rs_amd/csrc/placement_kernels.hip), restated: (digit bits, passes launched)"""
    lds = slots <= 3072
    room = min(96 * 1024 // 8 if lds else 1 << 22, 1 << 22)
    bits = 1
    while bits < 11 and (max(slots, 1) << (bits + 1)) <= room:
        bits += 1
    passes = -(-32 // bits)
    keys = (~np.asarray(stamps, np.uint32)).astype(np.uint32)
    x = int(keys.min()) ^ int(keys.max())
    hb = x.bit_length() - 1 if x else 0
    first = 0
    while max(32 - first * bits - bits, 0) > hb:
        first += 1
    return bits, passes - first, passes


def host_route(g, m, T, cutoff):
    A, S = g.get_assign(), g.get_seen()
    load, aff = g.get_objects()
    on = A < m
    used = np.bincount(A[on], weights=load[on], minlength=m).astype(np.int64)
    cand = on & (aff != rio_gp.AFF_INACTIVE) & (load >= 1) & (S < cutoff)
    cl = np.bincount(A[cand], weights=load[cand], minlength=m).astype(np.int64)
    free = np.maximum(T.astype(np.int64) - (used - cl), 0)
    over = cl > free
    rows = np.flatnonzero(cand)
    rows = rows[over[A[rows]]]
    order = np.lexsort((rows, ~S[rows], A[rows]))          # node, then stamp descending, then row
    r = rows[order]
    nd, l = A[r], load[r].astype(np.int64)
    cs = np.cumsum(l)
    first = np.r_[True, nd[1:] != nd[:-1]]
    base = (cs - l)[first]
    pre = cs - base[np.cumsum(first) - 1]
    sur = np.sort(r[pre > free[nd]]).astype(np.uint32)
    g.remove_batch(sur)
    return len(sur)


def main(reps):
    import torch
    cfg = synth.config("c3")
    n, m = cfg["n"], cfg["m"]
    alive = np.ones(m, np.uint8)
    g = rio_gp.GpuPlacement(n, m)
    g.set_nodes(cfg["cap"], alive)
    g.set_objects(n, cfg["load"], cfg["aff"])
    g.set_assign(synth.warm_assign(n, m))
    g.tick()
    A0 = g.get_assign()
    dA = torch.from_numpy(A0.view(np.int32).copy()).cuda()
    S = np.full(n, 3, np.uint32)
    r100 = np.arange(n) % 100
    S[r100 < 10] = 2
    S[r100 == 0] = 1
    g.touch_merge(S)
    cut = cfg["cap"].copy()
    cut[::10] = cut[::10] * np.uint64(7) // np.uint64(10)
    g.set_nodes(cut, alive)
    never = np.full(m, rio_gp.CAP_INF, np.uint64)
    d = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    dp = [x.data_ptr() for x in d]
    calls = (
        ("shed_dev", lambda: g.shed_idle_dev(4, dp[0], dp[1], n)[0]),
        ("shed_dev_cutoff_3", lambda: g.shed_idle_dev(3, dp[0], dp[1], n)[0]),
        ("shed_count_only", lambda: g.shed_idle_dev(4, max_rows=0)[0]),
        ("nothing_over", lambda: g.shed_idle_dev(4, target=never)[0]),
        ("rebalance_by_load", lambda: g.rebalance(list_moves=False, order=rio_gp.REBALANCE_BY_LOAD)[0]),
        ("expire_count_only", lambda: {"n_idle": g.expire_dev(3)[0]}),
        ("host_route", lambda: {"removed": host_route(g, m, cut, 4)}),
    )
    ts, last = {name: [] for name, _ in calls}, {}
    for it in range(reps + 1):
        for name, fn in calls:                    # alternating: drift of the machine hits all alike
            g.set_assign_dev(n, dA.data_ptr())
            g.get_nodes()                         # `used` valid again, outside the timed call
            g.sync()
            t0 = time.perf_counter()
            last[name] = fn()
            if it:
                ts[name].append(time.perf_counter() - t0)
    out = {"n": n, "m": m, "reps": reps, "placed": int((A0 != NONE).sum())}
    for name, _ in calls:
        out[name] = dict(stat(ts[name]), **last[name])
    assert out["host_route"]["removed"] == out["shed_dev"]["surplus_rows"] == out["shed_dev"]["shed_rows"]
    slots = out["shed_dev"]["nodes_over_before"]
    bits, launched, planned = selection_passes(slots, S)
    out["selection"] = {"slots": slots, "digit_bits": bits, "passes_launched": launched, "passes_of_the_plan": planned}
    out["shed_dev_over_rebalance_by_load"] = out["shed_dev"]["call_us"] / out["rebalance_by_load"]["call_us"]
    out["shed_dev_over_host_route"] = out["shed_dev"]["call_us"] / out["host_route"]["call_us"]
    g.close()
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    path = None
    if "--out" in args:
        k = args.index("--out")
        path = args[k + 1]
        del args[k:k + 2]
    res = {"shed": main(max(int(args[0]) if args else 7, 7))}
    line = json.dumps(res)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
    print(line)
