"""What the compiler made of the object-class kernels (k_expc_count, k_expc_apply, k_census, k_cls_elect, k_cls_apply), from its
own resource remarks: no GPU needed.

The per-class sweep holds to the plain sweep's bar (tests/test_kernel_resources_expire.py): no scratch and at most 64 vector
registers, so that the 256-thread workgroups fill every SIMD's eight wave slots.  On top of the plain passes' static LDS the
count pass keeps the cutoff table and the per-class histogram (1 KiB each), the apply pass the cutoff table.  The census streams
three columns with one quad per lane and 1 024-thread workgroups: no scratch and at most 64 vector registers either (its
accumulators are dynamic LDS, at most kCensusLdsCells x 12 B).  The scatter's two kernels spill nothing."""
import re

import pytest

import kernel_resource_usage


@pytest.fixture(scope="module")
def recs():
    """kernel (mangled name) -> {remark: value} from -Rpass-analysis=kernel-resource-usage"""
    return kernel_resource_usage.records()


def test_the_per_class_sweep_uses_no_scratch_and_keeps_full_occupancy(recs):
    mine = {k: v for k, v in recs.items() if re.match(r"_ZN5riogp12k_expc_(count|apply)E", k)}
    assert len(mine) == 2, sorted(k for k in recs if "expc" in k)
    for name, u in mine.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 64 and u["Occupancy [waves/SIMD]"] == 8, (name, u)
        # static: the plain pass's (tile offsets, the scan's words, the freed sum) plus the cutoff table and the histogram
        assert u["LDS Size [bytes/block]"] <= 4096 + 64 + 2048, (name, u)


def test_the_census_uses_no_scratch(recs):
    mine = {k: v for k, v in recs.items() if "k_census" in k}
    assert len(mine) == 3, sorted(mine)   # totals in LDS; by node in LDS and in global memory
    for name, u in mine.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 64, (name, u)


def test_the_class_scatter_uses_no_scratch(recs):
    mine = {k: v for k, v in recs.items() if re.match(r"_ZN5riogp11k_cls_(elect|apply)E", k)}
    assert len(mine) == 2, sorted(k for k in recs if "cls" in k)
    for name, u in mine.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
