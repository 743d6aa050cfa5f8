"""What the compiler made of the class-aware table passes of the rebalance (DESIGN.md section 2 rule 13: k_shedc_hist,
k_shedc_selhist, k_shedc_tile, k_shedc_cut, k_shedc_count, k_shedc_pack), from its own resource remarks: no GPU needed.

Each is the body of the kernel it stems from with the class test added: the quad of K beside the three dwordx4 loads and the 8
words of the immovable-class bitmask in DYNAMIC LDS.  So they must spill nothing to scratch (a bitmask indexed per lane in a
by-value array would), stay within 128 registers a lane (1 024-thread workgroups) and report the static LDS of their
originals.  That the originals are still there under their names and unchanged is what the resource tests of the rebalance
check (tests/test_kernel_resources_rebalance_order.py, tests/test_kernel_resources_shard_rebalance_order.py)."""
import re

import pytest

import kernel_resource_usage


@pytest.fixture(scope="module")
def recs():
    return kernel_resource_usage.records()


def _pick(recs, pattern, count):
    mine = {k: v for k, v in recs.items() if re.match(pattern, k)}
    assert len(mine) == count, sorted(k for k in recs if "k_shed" in k)
    return mine


# kernel -> (instantiations, static LDS of the kernel it stems from)
KERNELS = {
    r"_ZN5riogp12k_shedc_histILb[01]EEE": (2, None),      # (MAX adds one word)
    r"_ZN5riogp15k_shedc_selhistILb[01]EEE": (2, 0),
    r"_ZN5riogp12k_shedc_tileE": (1, 0),
    r"_ZN5riogp11k_shedc_cutE": (1, 128 + 8 + 8),
    r"_ZN5riogp13k_shedc_countE": (1, 8 + 8),
    r"_ZN5riogp12k_shedc_packE": (1, 128),
}


@pytest.mark.parametrize("pattern", sorted(KERNELS))
def test_no_scratch_at_most_128_registers_and_the_static_lds_of_the_original(recs, pattern):
    count, lds = KERNELS[pattern]
    for name, u in _pick(recs, pattern, count).items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 128, (name, u)
        if lds is not None:
            assert u["LDS Size [bytes/block]"] == lds, (name, u)


def test_the_class_aware_hist_has_the_static_lds_of_the_plain_one(recs):
    plain = _pick(recs, r"_ZN5riogp11k_shed_histILb[01]EEE", 2)
    aware = _pick(recs, r"_ZN5riogp12k_shedc_histILb[01]EEE", 2)
    for name, u in plain.items():
        form = re.search(r"histILb([01])E", name).group(1)
        (twin,) = [v for k, v in aware.items() if "histILb%sE" % form in k]
        assert twin["LDS Size [bytes/block]"] == u["LDS Size [bytes/block]"], (name, u, twin)
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
