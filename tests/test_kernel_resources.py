"""The compiler's own resource report of the kernels whose registers and scratch the design depends on, without a GPU
(placement_kernels.hip compiled once for all the resource modules: tests/kernel_resource_usage.py).

The chained scan of quiet ticks (k_scan<..., CHAIN>) waits, resident, for waves of the launch before it: that is free of deadlock
only while TWO of its 1 024-thread workgroups fit a CU — 8 waves per SIMD, i.e. at most 64 vector registers and at most 80
scalar registers per wave (800 per SIMD, allocated in sixteens plus sixteen: MI355X_MICROARCH.md "Residency").  The library
asks the occupancy query again when a handle is created and every in-kernel wait is bounded.  The chained scan is also the
whole quiet tick (the kept-load adds into `used` and the verdict rows are part of it): it must spill nothing to scratch.
The committed tick's in-place scan (k_inc_scan) has one form, two tiles per wave-iteration, and spills nothing either.
The change feed's kernels (k_chg_count, k_chg_scan, k_chg_list): the two passes stream two columns with dwordx4 loads and keep
them in registers, the scan holds eight sums per thread; none may spill to scratch, all keep full occupancy."""
import re

import pytest

import kernel_resource_usage


@pytest.fixture(scope="module")
def recs():
    """kernel (mangled name) -> {remark: value} from -Rpass-analysis=kernel-resource-usage"""
    return kernel_resource_usage.records()


def test_every_chained_scan_fits_twice_on_a_cu(recs):
    # k_scan<VIRT, ALLALIVE, TPI, COMPACT, NT, CHAIN = true>: one tile per wave-iteration, ALLALIVE x NT
    chained = {k: v for k, v in recs.items() if re.match(r"_ZN5riogp6k_scanILb0ELb[01]ELi\d+ELi0ELb[01]ELb1EEE", k)}
    assert len(chained) == 4, sorted(chained)
    for name, u in chained.items():
        assert "ELi1ELi0" in name, name
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 64, (name, u)
        assert u["TotalSGPRs"] <= 80, (name, u)
        assert u["Occupancy [waves/SIMD]"] == 8, (name, u)
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)


def test_the_inc_scan_has_one_form_and_uses_no_scratch(recs):
    # k_inc_scan<TPI, NT>: two tiles per wave-iteration, NT either way
    inc = {k: v for k, v in recs.items() if k.startswith("_ZN5riogp10k_inc_scanI")}
    assert len(inc) == 2, sorted(inc)
    for name, u in inc.items():
        assert re.match(r"_ZN5riogp10k_inc_scanILi2ELb[01]EEE", name), name
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)


def test_the_feed_kernels_use_no_scratch(recs):
    feed = {k: v for k, v in recs.items() if re.match(r"_ZN5riogp(11k_chg_count|10k_chg_scan|10k_chg_list)E", k)}
    assert len(feed) == 3, sorted(recs)[:5]
    for name, u in feed.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 64 and u["Occupancy [waves/SIMD]"] == 8, (name, u)
