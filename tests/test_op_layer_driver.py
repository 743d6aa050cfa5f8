"""The string-layer fuzz driver itself (tests/op_layer_driver.py), without a GPU: it runs against a plain-Python stand-in for
the string layer (tests/fake_rio_op.py, over tests/fake_rio_gp.py).

  - the committed seeds run clean: the model's own bookkeeping (rows, nodes, the lifetime of keys, the mirror) holds;
  - the coverage floor: what the driver exists for does happen in the committed seeds;
  - sensitivity: with exactly one behaviour of the stand-in made wrong, some committed seed fails.
"""
import pytest

import fake_rio_op
import op_layer_driver as drv

SEEDS = 42     # (tests/test_gpu_op_layer_fuzz.py runs the same seeds on the GPU)


@pytest.fixture(scope="module")
def clean_run(oracle):
    cov, count, checked, share = {}, {}, 0, [0, 0]
    for seed in range(SEEDS):
        sc = drv.run_seed(fake_rio_op.module(), oracle, seed)
        checked += sc.checked
        share = [share[0] + sc.share[0], share[1] + sc.share[1]]
        for k, v in sc.cov.items():
            cov[k] = cov.get(k, 0) + v
        for k, v in sc.count.items():
            count[k] = count.get(k, 0) + v
    return cov, count, checked, share


def test_committed_seeds_run_clean_and_use_every_operation(clean_run):
    cov, count, checked, _ = clean_run
    assert checked > 10000
    for op, _ in drv.Scenario.OPS:
        assert count.get(op, 0) > 0, (op, count)


def test_coverage_floor(clean_run):
    cov, count, _, _ = clean_run
    missing = [k for k in drv.FLOOR if cov.get(k, 0) < 1]
    assert not missing, (missing, cov, count)


def test_folds_are_compared_key_for_key(clean_run):
    """Of the non-zero request counters present at a fold at most 1 in 20 may sit on a row the model cannot map to a key (the
    driver learns the rows of unplaced keys before it folds: none does)."""
    unknown, present = clean_run[3]
    assert present > 500 and unknown * 20 <= present, (unknown, present)


def test_every_size_meets_every_flag():
    """Size and flags are drawn independently: the whole cross product occurs in the committed seeds — the default flags (what a
    host binds) on the 255 / 256 / 257, 4 096 and 2^14-row tables and RIO_OP_CFG_NO_HOST_SHADOW on a tiny one among them."""
    seen = {drv.config_of(s) for s in range(SEEDS)}
    assert seen == {(k, f) for k in ("tiny", "edge", "4096", "bulk") for f in drv.FLAGS}


@pytest.mark.parametrize("fault", fake_rio_op.FAULTS)
def test_a_wrong_string_layer_is_noticed(oracle, fault):
    for seed in range(SEEDS):
        try:
            drv.run_seed(fake_rio_op.module(fault), oracle, seed)
        except AssertionError as e:
            assert "seed" in repr(e.args) and "last ops" in repr(e.args), e.args
            return
    pytest.fail("no committed seed noticed the fault %r" % fault)
