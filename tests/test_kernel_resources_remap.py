"""What the compiler made of the node-removal kernel (k_remap), from its own resource remarks: no GPU needed.

The kernel streams two or three columns with dwordx4 loads, one tile ahead, and keeps the node map in 32 KiB of LDS: it must
spill nothing to scratch and stay within 64 vector registers, so that two of its 1 024-thread workgroups fit a CU (8 waves per
SIMD) and the loads of one cover the LDS lookups of the other."""
import re

import pytest

import kernel_resource_usage


@pytest.fixture(scope="module")
def recs():
    """kernel (mangled name) -> {remark: value} from -Rpass-analysis=kernel-resource-usage"""
    return kernel_resource_usage.records()


def test_the_remap_kernel_uses_no_scratch_and_keeps_full_occupancy(recs):
    mine = {k: v for k, v in recs.items() if re.match(r"_ZN5riogp7k_remapE", k)}
    assert len(mine) == 1, sorted(k for k in recs if "remap" in k)
    for name, u in mine.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 64 and u["Occupancy [waves/SIMD]"] == 8, (name, u)
        assert u["LDS Size [bytes/block]"] <= 33 * 1024, (name, u)   # the map (8 192 x 4 B) and a counter: two workgroups per CU
