"""What the compiler made of the measured-load kernels (k_hits_add, k_hits_merge, k_load_fold in its three forms), from its own
resource remarks: no GPU needed.

The merge and the fold stream one quad per lane and column with dwordx4 loads and do their arithmetic in 64 bits: they must spill
nothing to scratch and stay within 64 vector registers, so that the 256-thread workgroups fill every SIMD's eight wave slots.
The scatter is an atomic add with a fix-up: no scratch either."""
import re

import pytest

import kernel_resource_usage


@pytest.fixture(scope="module")
def recs():
    """kernel (mangled name) -> {remark: value} from -Rpass-analysis=kernel-resource-usage"""
    return kernel_resource_usage.records()


def test_the_fold_and_merge_passes_use_no_scratch_and_at_most_64_registers(recs):
    mine = {k: v for k, v in recs.items() if re.match(r"_ZN5riogp(11k_load_foldILi[012]EE|12k_hits_mergeE)", k)}
    assert len(mine) == 4, sorted(k for k in recs if "fold" in k or "hits" in k)
    for name, u in mine.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 64 and u["Occupancy [waves/SIMD]"] == 8, (name, u)
        assert u["LDS Size [bytes/block]"] <= 64, (name, u)   # static: four sums and a maximum (the per-node words are dynamic)


def test_the_scatter_uses_no_scratch(recs):
    mine = {k: v for k, v in recs.items() if re.match(r"_ZN5riogp10k_hits_addE", k)}
    assert len(mine) == 1, sorted(k for k in recs if "hits" in k)
    for name, u in mine.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
