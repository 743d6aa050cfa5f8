"""What the compiler made of the kernels the row-sharded load-ordered cut adds (k_shrb_import_slots, k_shrb_sel_pick), from its
own resource remarks: no GPU needed.

Both are record kernels — one workgroup over the nodes, one workgroup per over node over the gathered histograms — and stay
within what tests/test_kernel_resources_shard_rebalance.py sets for k_shrb_*: nothing in scratch, at most 64 registers a lane,
8 waves per SIMD.  The histogram pass itself is k_shed_sel_hist, reused as it is: both of its forms are still the only two, and
still spill nothing."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_shrb_import_slots", "k_shrb_sel_pick")


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


def test_the_new_record_kernels_use_no_scratch_and_keep_full_occupancy(recs):
    mine = {k: v for k, v in recs.items() if re.match(r"_ZN5riogp\d+(%s)E" % "|".join(KERNELS), k)}
    assert len(mine) == len(KERNELS), sorted(k for k in recs if "shrb" in k)
    for name, u in mine.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 64 and u["Occupancy [waves/SIMD]"] == 8, (name, u)


def test_the_histogram_pass_is_the_single_handles_kernel_and_spills_nothing(recs):
    hist = {k: v for k, v in recs.items() if "sel_hist" in k}
    assert len(hist) == 2, sorted(hist)   # the LDS form and the wave-aggregated one: no third, sharded form
    for name, u in hist.items():
        assert re.match(r"_ZN5riogp15k_shed_sel_histILb[01]EEE", name), name
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
