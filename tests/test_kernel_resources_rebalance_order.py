"""What the compiler made of the load-ordered cut's kernels (k_shed_sel_hist in its two forms, k_shed_sel_pick) and of the four
k_shed_* kernels that took the optional threshold (k_shed_tile, k_shed_cut, k_shed_count, k_shed_pack), from its own resource
remarks: no GPU needed.

The streaming passes read one quad per lane and column with dwordx4 loads and must spill nothing to scratch.  Their histograms,
node maps and thresholds live in DYNAMIC LDS sized by the launch, so the static LDS the compiler reports
is only what the design states: nothing for the histogram passes and k_shed_tile, the 16 wave partials of the block scan (128 B)
plus a few words for k_shed_sel_pick, k_shed_cut and k_shed_pack, two counters for k_shed_count."""
import re

import pytest

import kernel_resource_usage


@pytest.fixture(scope="module")
def recs():
    """kernel (mangled name) -> {remark: value} from -Rpass-analysis=kernel-resource-usage"""
    return kernel_resource_usage.records()


def _pick(recs, pattern, count):
    mine = {k: v for k, v in recs.items() if re.match(pattern, k)}
    assert len(mine) == count, sorted(k for k in recs if "k_shed" in k)
    return mine


def test_the_histogram_passes_stream_without_scratch_or_static_lds(recs):
    for name, u in _pick(recs, r"_ZN5riogp15k_shed_sel_histILb[01]EEE", 2).items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["LDS Size [bytes/block]"] == 0, (name, u)           # map | prefixes | histogram: dynamic
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 128, (name, u)      # 1 024-thread workgroups: at most 128 registers a lane


def test_the_pick_uses_no_scratch_and_the_scan_partials_only(recs):
    (name, u), = _pick(recs, r"_ZN5riogp15k_shed_sel_pickE", 1).items()
    assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
    assert u["LDS Size [bytes/block]"] == 128, (name, u)


def test_the_four_changed_kernels_use_no_scratch_and_the_static_lds_they_had(recs):
    want_lds = {"11k_shed_tile": 0, "10k_shed_cut": 128 + 8 + 8, "12k_shed_count": 8 + 8, "11k_shed_pack": 128}
    for key, lds in want_lds.items():
        (name, u), = _pick(recs, r"_ZN5riogp%sE" % key, 1).items()
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["LDS Size [bytes/block]"] == lds, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 128, (name, u)
