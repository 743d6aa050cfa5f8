"""What the compiler made of the row-sharded rebalance's kernels (k_shrb_*), from its own resource remarks: no GPU needed.

The record kernels are one workgroup over the nodes and the fill round walks the packed rows, four per lane, with a binary
search over C[] in registers: none may spill to scratch, and the fill — the only one launched over many workgroups — keeps full
occupancy so that the rounds of several ranks sharing a device do not crowd each other out."""
import re

import pytest

import kernel_resource_usage

KERNELS = ("k_shrb_export_x", "k_shrb_import_x", "k_shrb_export_y", "k_shrb_merge", "k_shrb_fill")


@pytest.fixture(scope="module")
def recs():
    """kernel (mangled name) -> {remark: value} from -Rpass-analysis=kernel-resource-usage"""
    return kernel_resource_usage.records()


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
