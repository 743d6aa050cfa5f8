"""What the compiler made of the pressure-shedding kernels (k_ish_* and their class forms k_ishc_*), from its own resource
remarks: no GPU needed.

The node pass, the selection's histogram pass in both forms, the tie-walk's tile pass and the count pass stream one quad per
lane and column with dwordx4 loads: they must spill nothing to scratch and stay within 64 vector registers, so that every
SIMD's eight wave slots fill.  The cut and the apply pass (a re-read of the few tiles that hold a listed row, the expiries'
apply body) must not spill either; the apply pass keeps the tile offsets of its workgroup in 4 KiB of LDS.  The class forms
keep the cutoff table in 1 KiB of static LDS on top of their plain form's."""
import re

import pytest

import kernel_resource_usage

STREAMING = r"_ZN5riogp(10k_ish_hist|11k_ishc_hist|14k_ish_key_histILb[01]EE|15k_ishc_key_histILb[01]EE|10k_ish_tile|11k_ishc_tile|" \
            r"11k_ish_count|12k_ishc_count)E"
REST = r"_ZN5riogp(9k_ish_cut|10k_ishc_cut|11k_ish_apply|12k_ishc_apply)E"


@pytest.fixture(scope="module")
def recs():
    """kernel (mangled name) -> {remark: value} from -Rpass-analysis=kernel-resource-usage"""
    return kernel_resource_usage.records()


def test_the_streaming_passes_use_no_scratch_and_at_most_64_registers(recs):
    mine = {k: v for k, v in recs.items() if re.match(STREAMING, k)}
    assert len(mine) == 10, sorted(k for k in recs if "k_ish" in k)
    for name, u in mine.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 64 and u["Occupancy [waves/SIMD]"] == 8, (name, u)
        # static LDS: a few words of reduction state, and the class forms' cutoff table
        assert u["LDS Size [bytes/block]"] <= (1024 if "k_ishc" in name else 0) + 64, (name, u)


def test_the_cut_and_the_apply_pass_use_no_scratch(recs):
    mine = {k: v for k, v in recs.items() if re.match(REST, k)}
    assert len(mine) == 4, sorted(k for k in recs if "k_ish" in k)
    for name, u in mine.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 96, (name, u)
        cls = 1024 if "k_ishc" in name else 0
        if "apply" in name:
            assert u["LDS Size [bytes/block]"] <= 4096 + 64 + cls, (name, u)     # toff[kChgMaxTpg] and the scan's words
        else:
            assert u["LDS Size [bytes/block]"] <= 256 + cls, (name, u)


def test_no_other_shedding_kernel_exists_unpinned(recs):
    mine = [k for k in recs if "k_ish" in k]
    assert len(mine) == 14 and all(re.match(STREAMING, k) or re.match(REST, k) for k in mine), sorted(mine)
