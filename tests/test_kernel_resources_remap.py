"""What the compiler made of the node-removal kernel (k_remap), from its own resource remarks: no GPU needed.

The kernel streams two or three columns with dwordx4 loads, one tile ahead, and keeps the node map in 32 KiB of LDS: it must
spill nothing to scratch and stay within 64 vector registers, so that two of its 1 024-thread workgroups fit a CU (8 waves per
SIMD) and the loads of one cover the LDS lookups of the other."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recs(tmp_path_factory):
    """kernel (mangled name) -> {remark: value} from -Rpass-analysis=kernel-resource-usage"""
    src = os.path.join(ROOT, "rio-rs_amd", "csrc", "placement_kernels.hip")
    out = tmp_path_factory.mktemp("kres") / "pk.o"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-c", src,
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    recs, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = recs.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+?): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return recs


def test_the_remap_kernel_uses_no_scratch_and_keeps_full_occupancy(recs):
    mine = {k: v for k, v in recs.items() if re.match(r"_ZN5riogp7k_remapE", k)}
    assert len(mine) == 1, sorted(k for k in recs if "remap" in k)
    for name, u in mine.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 64 and u["Occupancy [waves/SIMD]"] == 8, (name, u)
        assert u["LDS Size [bytes/block]"] <= 33 * 1024, (name, u)   # the map (8 192 x 4 B) and a counter: two workgroups per CU
