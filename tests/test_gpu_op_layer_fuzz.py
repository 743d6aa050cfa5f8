"""The whole string layer (rio_op_*) on the GPU under tests/op_layer_driver.py: every call of the layer in one random sequence,
two clones used alternately, each call checked against the translation model over the dense layer's CPU references (see the
driver).  The seeds are the ones tests/test_op_layer_driver.py holds to the coverage floor on the CPU stand-in.

Each seed ends with a short concurrent phase on a provider of its own: up to 8 threads, each with its own clone, its own keys and
its own active requester with unbounded capacity — so the final table does not depend on the interleaving — beside one thread
that alternates changes / objects_on_server / rebalance(max_moves=0) / tick / fold_loads(65536, 1) / a count-only
hottest_objects.  At quiescence the model built per key from each thread's own log equals the snapshot, the feed's mirror equals
the snapshot, and every listed change's old address was what the mirror held (spec_changes.apply, strict).  Load tracking is on
from before the threads start and each worker logs, per key, its calls that answered or set an address: after one final fold
the hits_folded of all folds sum to the logged total and every key's load is 1 + its logged count — the header's "none is lost
and none is counted twice" — and the census by type equals the snapshot's.

    python tests/test_gpu_op_layer_fuzz.py <seconds> [first_seed]     # a longer campaign; one JSON line
"""
import os
import sys
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEEDS = int(os.environ.get("RIO_OP_FUZZ_SEEDS", "42"))


def concurrent_phase(gp, seed, threads=6, steps=120):
    import op_layer_driver as drv
    import spec_changes
    rng = np.random.default_rng(0xC0C00000 + seed)
    flags = drv.FLAGS[seed % 3]
    rows_max = int(rng.choice([64 * threads, 4096]))
    p = drv.RealProvider.make(gp)(rows_max, 32, 2, flags)
    addrs = ["10.7.%d.%d:7000" % (seed % 200, t) for t in range(threads)]
    for a in addrs:
        assert p.set_member(a, True, drv.INF) == drv.OK
    assert p.set_load_tracking(True) == drv.OK
    final = [dict() for _ in range(threads)]
    counted = [dict() for _ in range(threads)]     # per worker: key -> its calls that answered or set an address
    folded = []
    errors = []
    stop = threading.Event()

    def worker(t):
        mine, r, me, model, cnt = p.clone(), np.random.default_rng(seed * 100 + t), addrs[t], final[t], counted[t]
        try:
            for _ in range(steps):
                key = ("C%d" % t, str(int(r.integers(40))))
                k = r.random()
                if k < 0.45:
                    rc, out, flag = mine.get_or_create_placement(key[0], key[1], me, 64)
                    want = model.get(key, me)
                    assert rc == drv.OK and out == want, ("request", key, rc, out, want)
                    assert flag & 0xF == (drv.PLACED if key not in model else drv.LOCAL if want == me else drv.REDIRECT), ("flag", key, flag)
                    model[key] = want
                    cnt[key] = cnt.get(key, 0) + 1
                elif k < 0.6:
                    to = addrs[int(r.integers(threads))]
                    assert mine.update(key[0], key[1], to) == drv.OK
                    model[key] = to
                    cnt[key] = cnt.get(key, 0) + 1
                elif k < 0.75:
                    assert mine.remove(key[0], key[1]) == drv.OK
                    model.pop(key, None)
                else:
                    fn = mine.lookup if r.random() < 0.5 else mine.try_lookup
                    rc, found, out = fn(key[0], key[1], 64)
                    if rc != drv.EAGAIN:
                        assert rc == drv.OK and (out if found else None) == model.get(key), ("lookup", key, rc, found, out, model.get(key))
                        if found:
                            cnt[key] = cnt.get(key, 0) + 1
        except BaseException as e:
            errors.append((t, e))
        finally:
            mine.close()

    mirror = [{}]
    first = [True]

    def reader():
        mine = p.clone()
        try:
            k = 0
            while not stop.is_set():
                k += 1
                if k % 6 == 4:
                    rc, _, hf = mine.fold_loads(65536, 1)
                    assert rc == drv.OK, ("fold_loads", rc)
                    folded.append(hf)
                elif k % 6 == 5:
                    rc, objs, nc = mine.hottest_objects(None, 0, 0)
                    assert rc == drv.OK and objs == [] and nc <= 40 * threads, ("hottest_objects", rc, nc)
                elif k % 4 == 0:
                    rc, full, entries = mine.changes()
                    assert rc == drv.OK and full == first[0], ("changes", rc, full)
                    first[0] = False
                    mirror[0] = spec_changes.apply(mirror[0], full, entries, strict=True)
                elif k % 4 == 1:
                    a = addrs[k % threads]
                    rc, objs = mine.objects_on_server(a)
                    assert rc == drv.OK and all(ty[0] == "C" for ty, _ in objs), ("objects_on_server", rc)
                elif k % 4 == 2:
                    rc, moves = mine.rebalance(0)
                    assert rc == drv.OK and moves == [], ("rebalance", rc, moves)
                else:
                    rc, st = mine.tick()
                    assert rc == drv.OK and st["evicted"] == 0, ("tick", rc, st)
        except BaseException as e:
            errors.append(("reader", e))
        finally:
            mine.close()

    ths = [threading.Thread(target=worker, args=(t,)) for t in range(threads)]
    rd = threading.Thread(target=reader)
    rd.start()
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    stop.set()
    rd.join()
    try:
        assert not errors, (seed, "concurrent phase", errors[:2])
        want = {}
        for m in final:
            want.update(m)
        rc, snap = p.snapshot()
        assert rc == drv.OK and {(a, b): c for a, b, c in snap} == want and len(snap) == len(want), (seed, "the snapshot at quiescence differs")
        rc, full, entries = p.changes()
        assert rc == drv.OK and full == first[0], (seed, "changes at quiescence", rc, full)
        mirror[0] = spec_changes.apply(mirror[0], full, entries, strict=True)
        assert mirror[0] == want, (seed, "the feed's mirror differs from the snapshot at quiescence")
        # measured load: one final fold, then every request the workers logged is in exactly one fold and on its own key
        rc, _, hf = p.fold_loads(65536, 1)
        assert rc == drv.OK, (seed, "the final fold", rc)
        total = {}
        for c in counted:
            total.update(c)        # (every worker has keys of its own)
        assert sum(folded) + hf == sum(total.values()), (seed, "hits_folded over all folds", sum(folded) + hf, sum(total.values()))
        created = set(total)       # (a key exists from its first request or update: both are logged)
        assert len(created) <= rows_max and p.dense().num_objects == len(created), (seed, "the table of this phase never reclaims",
                                                                                     len(created), rows_max, p.dense().num_objects)
        for key in sorted(created):
            rc, load = p.get_object_load(key[0], key[1])
            assert rc == drv.OK and load == 1 + total[key], (seed, "a key's load is not 1 + its logged requests", key, load, total[key])
        rc, cen = p.census()
        by_rows, by_load = {}, {}
        for (ty, _), a in want.items():
            by_rows[ty] = by_rows.get(ty, 0) + 1
        for key in want:
            by_load[key[0]] = by_load.get(key[0], 0) + 1 + total[key]
        # (class order is the order in which the workers' types were first interned: whichever thread came first)
        assert rc == drv.OK and len(cen) == len(by_rows) and sorted(cen) == sorted((ty, None, by_rows[ty], by_load[ty]) for ty in by_rows), \
            (seed, "the census by type differs from the snapshot's", cen, by_rows, by_load)
    finally:
        p.close()
    return threads * steps


@pytest.fixture(scope="module")
def gp():
    import rio_gp
    rio_gp.build()
    return rio_gp


@pytest.mark.parametrize("seed", range(SEEDS))
def test_random_string_layer_sequences(gp, oracle, seed):
    import op_layer_driver as drv
    drv.run_seed(drv.RealProvider.make(gp), oracle, seed)
    concurrent_phase(gp, seed)


if __name__ == "__main__":
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for q in (ROOT, os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, q)
    import json
    try:   # (two HIP runtimes in the process: torch's has to come up first — see tests/conftest.py)
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        pass
    import op_layer_driver as drv
    import pyoracle
    import rio_gp
    rio_gp.build()
    pyoracle.build()
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed = first = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    t0, ops, checked, conc, cov, mismatches = time.time(), 0, 0, 0, {}, []
    while time.time() - t0 < budget:
        try:
            sc = drv.run_seed(drv.RealProvider.make(rio_gp), pyoracle, seed)
            ops += sc.steps
            checked += sc.checked
            for k, v in list(sc.cov.items()) + list(sc.count.items()) + [("%s table, flags %d" % (sc.kind, sc.flags), 1)]:
                cov[k] = cov.get(k, 0) + v
            conc += concurrent_phase(rio_gp, seed)
        except AssertionError as e:
            mismatches.append(repr(e.args)[:600])
        seed += 1
    print(json.dumps({"scenarios": seed - first, "first_seed": first, "operations_checked": ops, "assertions": checked,
                      "concurrent_calls": conc, "seconds": round(time.time() - t0, 1), "mismatches": len(mismatches),
                      "first_mismatches": mismatches[:3], "coverage": cov}))
    sys.exit(1 if mismatches else 0)
