#!/usr/bin/env python3
"""Measured load on config 3 (10 M x 1 024, the warm table of synth.py after one tick): wall clock per call around work that ends
in a stream wait, median and min-max of `reps` runs, every run from the same restored state (the hit column is filled again from
a device copy and the loads put back before each run, not timed).  The hits are those of 10 M Zipf-distributed requests.
  fold_used_valid        rio_gp_load_fold (keep 1/2, gain 1, loads 1 .. 10^6) with `used` valid: load, H and the committed column
                         read, `used` kept in step inside the pass
  fold_used_invalid      the same with `used` invalid: load and H only
  fold_invalid_then_used the same followed by rio_gp_get_nodes: what a separate k_used pass costs on top (the A/B of the in-pass
                         update: fold_used_valid against this)
  fold_nothing_to_do     keep 65536 with H all zero: 8 B per row read, nothing written
  hits_merge_dev         rio_gp_hits_merge_dev of a device column of counters + the stream wait
  hits_add_batch_dev     10 M Zipf indices, weights NULL (one atomic add each, the hot rows contended)
  touch_merge_dev        yardstick, an existing pass: 8 B per row (+ 4 B written where a stamp rises: rising stamps every run)
  count_placed           yardstick, an existing pass: 4 B per row
For each: us, algorithmic bytes per row (counted from the columns: a quad of 16 B is written only where it changes) and TB/s.
Prints one JSON line.  Usage: load_fold_probe.py [reps] [--out profiles/load_fold_probe.json]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np
import rio_gp, synth


def stat(ts, n, bytes_per_row):
    us = float(np.median(ts)) * 1e6
    return {"us": us, "us_min": float(np.min(ts)) * 1e6, "us_max": float(np.max(ts)) * 1e6,
            "bytes_per_row": round(float(bytes_per_row), 3), "tb_per_s": n * float(bytes_per_row) / us / 1e6}


def quads_changed(before, after):
    """fraction of the 16-byte quads in which some word differs"""
    k = len(before) // 4 * 4
    return float((before[:k] != after[:k]).reshape(-1, 4).any(axis=1).mean())


def main(reps):
    import torch
    cfg = synth.config("c3")
    n, m = cfg["n"], cfg["m"]
    g = rio_gp.GpuPlacement(n, m)
    g.set_nodes(cfg["cap"], np.ones(m, np.uint8))
    g.set_objects(n, cfg["load"], cfg["aff"])
    g.set_assign(synth.warm_assign(n, m))
    g.tick()
    rng = np.random.default_rng(11)
    idx = ((rng.zipf(1.1, n) - 1) % n).astype(np.uint32)
    hits = np.bincount(idx, minlength=n).astype(np.uint32)
    load0 = cfg["load"].astype(np.uint32)
    d_idx = torch.from_numpy(idx.view(np.int32).copy()).cuda()
    d_hits = torch.from_numpy(hits.view(np.int32).copy()).cuda()
    d_load = torch.from_numpy(load0.view(np.int32).copy()).cuda()
    d_aff = torch.from_numpy(cfg["aff"].astype(np.uint32).view(np.int32).copy()).cuda()
    d_A = torch.from_numpy(g.get_assign().view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    KEEP, GAIN, LO, HI = 32768, 1, 1, 1_000_000
    new = np.clip((load0.astype(np.uint64) * KEEP >> 16) + hits.astype(np.uint64) * GAIN, LO, HI).astype(np.uint32)
    fold_bytes = 8 + 16 * quads_changed(load0, new) / 4 + 16 * quads_changed(hits, np.zeros_like(hits)) / 4
    out = {"n": n, "m": m, "reps": reps, "requests": int(hits.sum()), "rows_with_hits": int((hits != 0).sum()),
           "fold": {"keep": KEEP, "gain": GAIN, "min_load": LO, "max_load": HI, "rows_changed": int((new != load0).sum())}}

    def restore(used_valid, with_hits=True):
        g.set_objects_dev(n, d_load.data_ptr(), d_aff.data_ptr())   # the loads back (and the column cleared) ...
        g.set_assign_dev(n, d_A.data_ptr())                         # ... and the column back
        g.load_fold(65536, 0)                                       # H := 0
        if with_hits:
            g.hits_merge_dev(d_hits.data_ptr(), n)
        if used_valid:
            g.get_nodes()
        else:
            g.set_object_attrs([0], load=[int(load0[0])])           # the same load again: `used` counts as invalid
        g.sync()

    def timed(fn, used_valid, with_hits=True):
        ts, last = [], None
        for _ in range(reps + 2):
            restore(used_valid, with_hits)
            t0 = time.perf_counter()
            last = fn()
            ts.append(time.perf_counter() - t0)
        return ts[2:], last

    ts, st = timed(lambda: g.load_fold(KEEP, GAIN, LO, HI), True)
    out["fold_used_valid"] = dict(stat(ts, n, fold_bytes + 4), stats=st)
    used_a = g.get_nodes()[2]
    ts, st = timed(lambda: g.load_fold(KEEP, GAIN, LO, HI), False)
    out["fold_used_invalid"] = dict(stat(ts, n, fold_bytes), stats=st)
    assert np.array_equal(g.get_objects()[0], new) and np.array_equal(g.get_nodes()[2], used_a)
    ts, _ = timed(lambda: (g.load_fold(KEEP, GAIN, LO, HI), g.get_nodes()), False)
    out["fold_invalid_then_used"] = stat(ts, n, fold_bytes + 8)
    ts, st = timed(lambda: g.load_fold(65536, 1), False, with_hits=False)
    out["fold_nothing_to_do"] = dict(stat(ts, n, 8), stats=st)

    def merge():
        g.hits_merge_dev(d_hits.data_ptr(), n)
        g.sync()
    ts, _ = timed(merge, True, with_hits=False)
    out["hits_merge_dev"] = stat(ts, n, 8 + 16 * quads_changed(hits, np.zeros_like(hits)) / 4)
    ts, _ = timed(lambda: g.hits_add_dev(d_idx.data_ptr(), n), True, with_hits=False)
    out["hits_add_batch_dev"] = stat(ts, n, 4 + 8)                  # the index read; the word read and written by the atomic
    assert np.array_equal(g.get_hits(), hits)

    # the yardsticks: two passes of the library as it was before this feature, in the same session
    stamps = torch.ones(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g.touch_merge_dev(stamps.data_ptr(), n)
    g.sync()
    ts = []
    for k in range(reps + 2):
        stamps.add_(1)                                              # rising stamps: every quad is written, as in the fold
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.touch_merge_dev(stamps.data_ptr(), n)
        g.sync()
        ts.append(time.perf_counter() - t0)
    out["touch_merge_dev"] = stat(ts[2:], n, 12)
    ts = []
    for k in range(reps + 2):
        t0 = time.perf_counter()
        g.touch_merge_dev(stamps.data_ptr(), n)                     # nothing rises: 8 B per row read, nothing written
        g.sync()
        ts.append(time.perf_counter() - t0)
    out["touch_merge_dev_nothing_rises"] = stat(ts[2:], n, 8)
    ts = []
    for k in range(reps + 2):
        t0 = time.perf_counter()
        g.count_placed()
        ts.append(time.perf_counter() - t0)
    out["count_placed"] = stat(ts[2:], n, 4)
    out["fold_used_valid_over_fold_invalid_then_used"] = out["fold_used_valid"]["us"] / out["fold_invalid_then_used"]["us"]
    out["fold_used_invalid_over_touch_merge_dev"] = out["fold_used_invalid"]["us"] / out["touch_merge_dev"]["us"]
    g.close()
    return out


if __name__ == "__main__":
    argv = sys.argv[1:]
    dest = os.environ.get("PROBE_OUT")
    if "--out" in argv:
        k = argv.index("--out")
        dest = argv[k + 1]
        del argv[k:k + 2]
    res = {"load_fold": main(int(argv[0]) if argv else 15)}
    print(json.dumps(res))
    if dest:
        with open(dest, "w") as f:
            json.dump(res, f, indent=1)
