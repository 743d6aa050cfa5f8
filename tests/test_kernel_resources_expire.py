"""What the compiler made of the idle-expiry kernels (k_exp_count, k_exp_apply, k_touch, k_seen_merge), from its own resource
remarks: no GPU needed.

The count and apply passes stream two columns with dwordx4 loads and keep a tile of both in registers, as the change feed's
passes do: they must spill nothing to scratch and stay within 64 vector registers, so that the 256-thread workgroups fill every
SIMD's eight wave slots.  The apply pass keeps its tile offsets and two small words in static LDS (the per-node histogram is
dynamic: at most 4 096 x 8 B on top).  The touch kernels are a scatter and a one-quad-per-lane stream: no scratch either."""
import re

import pytest

import kernel_resource_usage


@pytest.fixture(scope="module")
def recs():
    """kernel (mangled name) -> {remark: value} from -Rpass-analysis=kernel-resource-usage"""
    return kernel_resource_usage.records()


def test_the_count_and_apply_passes_use_no_scratch_and_keep_full_occupancy(recs):
    mine = {k: v for k, v in recs.items() if re.match(r"_ZN5riogp11k_exp_(count|apply)E", k)}
    assert len(mine) == 2, sorted(k for k in recs if "exp" in k)
    for name, u in mine.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 64 and u["Occupancy [waves/SIMD]"] == 8, (name, u)
        assert u["LDS Size [bytes/block]"] <= 4096 + 64, (name, u)   # static: the tile offsets, the scan's words, the freed sum


def test_the_touch_kernels_use_no_scratch(recs):
    mine = {k: v for k, v in recs.items() if re.match(r"_ZN5riogp(7k_touch|12k_seen_merge)E", k)}
    assert len(mine) == 2, sorted(k for k in recs if "touch" in k or "seen" in k)
    for name, u in mine.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
