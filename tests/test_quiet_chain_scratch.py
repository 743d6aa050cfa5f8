"""The chained scan is the whole quiet tick (k_scan<..., CHAIN>: the kept-load adds into `used` and the verdict rows are part of
it): the form the product launches — one tile per wave-iteration, every ALLALIVE x NT instantiation — must keep its registers
and spill nothing to scratch.  The compiler's resource report, without a GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_quiet_tick_kernel_uses_no_scratch(tmp_path):
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
    quiet = {k: v for k, v in recs.items() if re.match(r"_ZN5riogp6k_scanILb0ELb[01]ELi1ELi0ELb[01]ELb1EEE", k)}
    assert len(quiet) == 4, sorted(recs)[:5]
    for name, u in quiet.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 64 and u["Occupancy [waves/SIMD]"] == 8, (name, u)
