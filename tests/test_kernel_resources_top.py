"""What the compiler made of the hot-object report's kernels (k_top_hist in its six forms, k_top_select, k_top_collect, k_top_ties,
k_top_sort), from its own resource remarks: no GPU needed.

The histogram, collect and tie passes stream one quad per lane, column and step with dwordx4 loads: they must spill nothing to
scratch and stay within 64 vector registers, so that the 256-thread workgroups fill every SIMD's eight wave slots.  The histogram
pass keeps 2 048 bins in LDS (8 KiB), the sort 4 096 composites (32 KiB of the CU's 160); neither uses scratch."""
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


def test_the_streaming_passes_use_no_scratch_and_at_most_64_registers(recs):
    mine = {k: v for k, v in recs.items()
            if re.match(r"_ZN5riogp(10k_top_histILb[01]ELi[012]EE|13k_top_collectILb[01]EE|10k_top_tiesILb[01]EE)", k)}
    assert len(mine) == 10, sorted(k for k in recs if "k_top" in k)
    for name, u in mine.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 64 and u["Occupancy [waves/SIMD]"] == 8, (name, u)
        assert u["LDS Size [bytes/block]"] <= 8192 + 64, (name, u)


def test_the_selection_and_the_sort_use_no_scratch(recs):
    mine = {k: v for k, v in recs.items() if re.match(r"_ZN5riogp(12k_top_select|10k_top_sort)E", k)}
    assert len(mine) == 2, sorted(k for k in recs if "k_top" in k)
    for name, u in mine.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
    sort = next(v for k, v in mine.items() if "k_top_sort" in k)
    assert sort["LDS Size [bytes/block]"] == 32768, sort
