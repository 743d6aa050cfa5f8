"""What the compiler reports for every kernel of placement_kernels.hip (-Rpass-analysis=kernel-resource-usage), for the
tests/test_kernel_resources*.py: one compile per process and compile line, shared by every module that asks.  No GPU needed."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "rio-rs_amd", "csrc", "placement_kernels.hip")
_cache = {}


def records(source=SOURCE, extra=()):
    """kernel (mangled name) -> {remark: value}.  `extra`: further compiler arguments; they are part of the cache's key."""
    line = ("hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-c", source,
            "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage") + tuple(extra)
    if line not in _cache:
        with tempfile.TemporaryDirectory(prefix="kres") as d:
            r = subprocess.run(list(line) + ["-o", os.path.join(d, "pk.o")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        recs, cur = {}, None
        for text in r.stderr.splitlines():
            m = re.search(r"remark: Function Name: (\S+)", text)
            if m:
                cur = recs.setdefault(m.group(1), {})
                continue
            m = re.search(r"remark:\s+([A-Za-z /\[\]]+?): (\d+)", text)
            if m and cur is not None:
                cur[m.group(1).strip()] = int(m.group(2))
        _cache[line] = recs
    return _cache[line]
