"""What the compiler made of the hot-object report's kernels (k_top_hist in its six forms, k_top_select, k_top_collect, k_top_ties,
k_top_sort), from its own resource remarks: no GPU needed.

The histogram, collect and tie passes stream one quad per lane, column and step with dwordx4 loads: they must spill nothing to
scratch and stay within 64 vector registers, so that the 256-thread workgroups fill every SIMD's eight wave slots.  The histogram
pass keeps 2 048 bins in LDS (8 KiB), the sort 4 096 composites (32 KiB of the CU's 160); neither uses scratch."""
import re

import pytest

import kernel_resource_usage


@pytest.fixture(scope="module")
def recs():
    """kernel (mangled name) -> {remark: value} from -Rpass-analysis=kernel-resource-usage"""
    return kernel_resource_usage.records()


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
