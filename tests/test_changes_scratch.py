"""The change feed's kernels (k_chg_count, k_chg_scan, k_chg_list): the two passes stream two columns with dwordx4 loads and keep
them in registers, the scan holds eight sums per thread; none may spill to scratch, all keep full occupancy.  The compiler's resource report, without a GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_feed_kernels_use_no_scratch(tmp_path):
    src = os.path.join(ROOT, "rio-rs_amd", "csrc", "placement_kernels.hip")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-c", src,
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "pk.o")],
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
    feed = {k: v for k, v in recs.items() if re.match(r"_ZN5riogp(11k_chg_count|10k_chg_scan|10k_chg_list)E", k)}
    assert len(feed) == 3, sorted(recs)[:5]
    for name, u in feed.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 64 and u["Occupancy [waves/SIMD]"] == 8, (name, u)
