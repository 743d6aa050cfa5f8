"""bench.py --gpus N cannot print a line for fewer GPUs than it names (round-4 verdict, item 2): started without a launcher it
becomes the launcher; with fewer visible devices than N it refuses with exit code 2 and an empty stdout."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_refuses_more_gpus_than_are_visible():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode == 2 and r.stdout.strip() == "" and "refusing to run" in r.stderr


def test_bench_refuses_a_launcher_with_another_rank_count():
    env = dict(os.environ, WORLD_SIZE="4", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode != 0 and r.stdout.strip() == "" and "must equal WORLD_SIZE" in r.stderr


def test_bench_full_and_dump_outputs_options(tmp_path):
    """--full and --dump-outputs DIR are options of the line; the dump is of a single-GPU line and is refused before any rank
    starts otherwise."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "d")], capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode != 0 and r.stdout.strip() == "" and "--dump-outputs" in r.stderr
    assert not (tmp_path / "d").exists()


class _Handle:
    """The two read-backs dump_outputs makes of a placement handle."""

    def __init__(self, assign, used):
        self.assign, self.used = assign, used

    def get_assign(self):
        return self.assign.copy()

    def get_nodes(self):
        return None, None, self.used


def test_dump_outputs_samples_a_large_table_at_fixed_rows(tmp_path, monkeypatch):
    """Above DUMP_MAX_ROWS the column is written at the rows synth.r(i, 7) % n, i < DUMP_MAX_ROWS, deduplicated, in row
    order: the same rows on every run, the values of exactly those rows."""
    import numpy as np
    sys.path[:0] = [ROOT, os.path.join(ROOT, "rio-rs_amd")]
    had = "HSA_ENABLE_IPC_MODE_LEGACY" in os.environ
    import bench
    if not had:   # (set by bench.py for its own runs)
        os.environ.pop("HSA_ENABLE_IPC_MODE_LEGACY", None)
    import rio_gp
    import synth
    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", 5000)
    n = 40_000
    col = (np.arange(n, dtype=np.uint32) * 7) % 1021
    col[::13] = 0xFFFFFFFF
    keys = [k for k, _ in rio_gp.Stats._fields_ if k != "reserved"]
    st = {k: i * 1000 for i, k in enumerate(keys)}
    used = np.arange(1021, dtype=np.uint64) * 3
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), _Handle(col, used), st)
    a = np.load(tmp_path / "a" / "assign.npy")
    rows = np.unique(synth.r(np.arange(5000, dtype=np.uint64), 7) % np.uint64(n)).astype(np.int64)
    assert a.dtype == np.float32 and 4000 < len(a) <= 5000 and len(a) == len(rows)
    assert np.array_equal(a, col[rows].astype(np.float32)) and np.array_equal(a, np.load(tmp_path / "b" / "assign.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "used.npy"), used.astype(np.float64))
    assert np.load(tmp_path / "a" / "stats.npy").tolist() == [float(st[k]) for k in keys]
    small = tmp_path / "small"
    bench.dump_outputs(str(small), _Handle(col[:5000], used), st)     # at the limit: the whole column
    assert np.array_equal(np.load(small / "assign.npy"), col[:5000].astype(np.float32))
