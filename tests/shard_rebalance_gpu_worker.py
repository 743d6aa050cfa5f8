"""One rank of a several-process row-sharded rebalance on one GPU — TEST INFRASTRUCTURE ONLY (tests/test_gpu_shard_rebalance.py
starts one of these per rank, each under its own time limit, and checks every exit status).

usage: shard_rebalance_gpu_worker.py RANK WORLD PORT OUT_DIR SEED N M MAX_MOVES ROUNDS   (MAX_MOVES -1 = no limit)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "rio-rs_amd"), os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def case(seed, n, m):
    import rebalance_ref
    rng = np.random.default_rng(seed)
    cur, load, aff, alive, T = rebalance_ref.random_table(rng, n, m)
    cap = rng.integers(100, 5000, m).astype(np.uint64)
    return cur, load, aff, cap, alive, T


def bounds(n, world, seed):
    cuts = sorted(int(c) for c in np.random.default_rng(seed + 1).integers(0, n + 1, world - 1))
    return [0] + cuts + [n]


def main():
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    out_dir = sys.argv[4]
    seed, n, m, max_moves, rounds = (int(v) for v in sys.argv[5:10])
    import torch
    import torch.distributed as dist
    import rio_gp
    import sharded
    from test_gpu_shard_rebalance import make_engines
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        cur, load, aff, cap, alive, T = case(seed, n, m)
        b = bounds(n, world, seed)
        eng = make_engines((cur, load, aff, cap, alive), [b[rank], b[rank + 1]])[0]
        sol = sharded.ShardedSolver([eng], sharded.DistExchange(stage_through_host=True))
        st, rows, frm, to = sol.rebalance(target=T, max_moves=None if max_moves < 0 else max_moves, rounds=rounds)
        np.savez(os.path.join(out_dir, "r%d.npz" % rank), a=eng.g.get_assign() if eng.g.num_objects else np.zeros(0, np.uint32),
                 used=eng.g.get_nodes()[2], rows=rows, frm=frm, to=to, st=np.array([st[k] for k in sorted(st)], np.uint64))
        eng.g.close()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
