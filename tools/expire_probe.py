#!/usr/bin/env python3
"""Idle expiry on config 3 (10 M x 1 024, the warm table of synth.py after one tick): wall clock per call, median and min-max of
`reps` runs, every run from the same restored table (the assignment column is put back from a device copy and `used` rebuilt
before each run, not timed; S is never changed by an expiry).  S is laid out by row: r % 100 == 0 was last seen at epoch 1,
1 <= r % 100 < 10 at epoch 2, the rest at epoch 3 — a cutoff of 2 finds 1 % of the rows idle, a cutoff of 3 finds 10 %.
  count_only            rio_gp_expire_dev without arrays: the count pass (8 B per row), the scan, one wait
  changes_count_only    rio_gp_changes_dev without arrays on the same table in the same session: the yardstick (same bytes, same
                        launches)
  idle_1pct / idle_10pct   the _dev form, no limit: + the apply pass over the tiles with a hit, 8 B per listed row out
  idle_10pct_cap_1e4    the same with cap = 10^4: the apply pass ends after the first workgroups
  idle_10pct_host       the host-pointer form: a wait after the count, the listing staged and copied out
  touch_batch_dev_1e6   10^6 random rows, rising epochs (every entry an atomic maximum)
  touch_batch_host_16 / _1e5   rio_gp_touch_batch from a host array: the index check, the staging copy, the scatter, one wait
  touch_all             every row, rising epochs (4 B read + 4 B written per row), timed with the stream wait behind it
  host_route            what a host does without the calls: rio_gp_get_assign, a numpy pass over the column and its own stamps,
                        rio_gp_remove_batch of the idle rows (10 %)
Prints one JSON line.  Usage: expire_probe.py [reps]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np
import rio_gp, synth

NONE = 0xFFFFFFFF


def stat(ts):
    return {"us": float(np.median(ts)) * 1e6, "us_min": float(np.min(ts)) * 1e6, "us_max": float(np.max(ts)) * 1e6}


def main(reps):
    import torch
    cfg = synth.config("c3")
    n, m = cfg["n"], cfg["m"]
    g = rio_gp.GpuPlacement(n, m)
    g.set_nodes(cfg["cap"], np.ones(m, np.uint8))
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
    g.changes()                                   # the feed's checkpoint: allocated, and level with the table
    d = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    dp = [x.data_ptr() for x in d]
    out = {"n": n, "m": m, "reps": reps, "placed": int((A0 != NONE).sum())}

    def restore():
        g.set_assign_dev(n, dA.data_ptr())
        g.get_nodes()                             # `used` valid again: the expiry keeps it current
        g.changes()

    def timed(fn):
        ts, last = [], None
        for _ in range(reps + 1):
            restore()
            t0 = time.perf_counter()
            last = fn()
            ts.append(time.perf_counter() - t0)
        return ts[1:], last

    ts, r = timed(lambda: g.expire_dev(3))
    out["count_only"] = dict(stat(ts), n_idle=r[0])
    ts, r = timed(lambda: g.changes_dev(cap=0))
    out["changes_count_only"] = dict(stat(ts), changes=r)
    ts, r = timed(lambda: g.expire_dev(2, dp[0], dp[1], cap=n))
    out["idle_1pct"] = dict(stat(ts), n_idle=r[0], load_freed=r[1])
    ts, r = timed(lambda: g.expire_dev(3, dp[0], dp[1], cap=n))
    out["idle_10pct"] = dict(stat(ts), n_idle=r[0], load_freed=r[1])
    ts, r = timed(lambda: g.expire_dev(3, dp[0], dp[1], cap=10_000))
    out["idle_10pct_cap_1e4"] = dict(stat(ts), n_idle=r[0], load_freed=r[1])
    ts, r = timed(lambda: g.expire(3, cap=n))
    out["idle_10pct_host"] = dict(stat(ts), n_idle=r[2], listed=int(len(r[0])))

    def host_route():
        A = g.get_assign()
        rows = np.flatnonzero((A != NONE) & (S < 3)).astype(np.uint32)
        g.remove_batch(rows)
        return len(rows)
    ts, r = timed(host_route)
    out["host_route"] = dict(stat(ts), removed=r)

    rng = np.random.default_rng(3)
    idx = torch.from_numpy(rng.integers(0, n, 1_000_000).astype(np.int32)).cuda()
    torch.cuda.synchronize()
    ts = []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        g.touch_dev(idx.data_ptr(), 1_000_000, 10 + k)
        ts.append(time.perf_counter() - t0)
    out["touch_batch_dev_1e6"] = stat(ts[1:])
    for name, cnt in (("touch_batch_host_16", 16), ("touch_batch_host_1e5", 100_000)):
        hidx = rng.integers(0, n, cnt).astype(np.uint32)
        ts = []
        for k in range(reps + 1):
            t0 = time.perf_counter()
            g.touch(hidx, 50 + k)
            ts.append(time.perf_counter() - t0)
        out[name] = stat(ts[1:])
    ts = []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        g.touch_all(100 + k)
        g.sync()
        ts.append(time.perf_counter() - t0)
    out["touch_all"] = stat(ts[1:])
    out["count_only_over_changes_count_only"] = out["count_only"]["us"] / out["changes_count_only"]["us"]
    g.close()
    return out


if __name__ == "__main__":
    res = {"expire": main(int(sys.argv[1]) if len(sys.argv) > 1 else 7)}
    print(json.dumps(res))
    if os.environ.get("PROBE_OUT"):
        with open(os.environ["PROBE_OUT"], "w") as f:
            json.dump(res, f, indent=1)
