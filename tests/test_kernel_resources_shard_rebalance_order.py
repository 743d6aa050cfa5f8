"""What the compiler made of the kernels the row-sharded load-ordered cut adds (k_shrb_import_slots, k_shrb_sel_pick), from its
own resource remarks: no GPU needed.

Both are record kernels — one workgroup over the nodes, one workgroup per over node over the gathered histograms — and stay
within what tests/test_kernel_resources_shard_rebalance.py sets for k_shrb_*: nothing in scratch, at most 64 registers a lane,
8 waves per SIMD.  The histogram pass itself is k_shed_sel_hist, reused as it is: both of its forms are still the only two, and
still spill nothing."""
import re

import pytest

import kernel_resource_usage

KERNELS = ("k_shrb_import_slots", "k_shrb_sel_pick")


@pytest.fixture(scope="module")
def recs():
    """kernel (mangled name) -> {remark: value} from -Rpass-analysis=kernel-resource-usage"""
    return kernel_resource_usage.records()


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
