"""What the compiler made of the row-sharded rebalance's kernels (k_shrb_*), from its own resource remarks: no GPU needed.

The record kernels are one workgroup over the nodes and the fill round walks the packed rows, four per lane, with a binary
search over C[] in registers: none may spill to scratch, and the fill — the only one launched over many workgroups — keeps full
occupancy so that the rounds of several ranks sharing a device do not crowd each other out."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_shrb_export_x", "k_shrb_import_x", "k_shrb_export_y", "k_shrb_merge", "k_shrb_fill")


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


def test_the_sharded_rebalance_kernels_use_no_scratch(recs):
    mine = {k: v for k, v in recs.items() if re.match(r"_ZN5riogp\d+(%s)E" % "|".join(KERNELS), k)}
    assert len(mine) == len(KERNELS), sorted(k for k in recs if "shrb" in k)
    for name, u in mine.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 64 and u["Occupancy [waves/SIMD]"] == 8, (name, u)
    # the scan that starts at a rank's base is the same kernel as the single-handle route's
    scans = [k for k in recs if re.match(r"_ZN5riogp11k_shed_scanI[jmy]EE", k)]
    assert len(scans) == 2, scans
    for k in scans:
        assert recs[k]["ScratchSize [bytes/lane]"] == 0, (k, recs[k])
