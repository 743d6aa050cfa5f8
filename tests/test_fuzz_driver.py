"""The fuzz driver itself (tests/test_gpu_fuzz.py's Scenario), without a GPU: the scenarios run against a CPU stand-in for the
handle (tests/fake_rio_gp.py).

  - replay: the old family's seeds draw the tables and operations they drew before the extended op table existed
    (tests/golden/fuzz_old_family_ops.json, recorded from the earlier Scenario against the same stand-in);
  - the extended seeds run clean: the model's own bookkeeping (n, the feed's checkpoint, the mirror, the uncommitted solve, the
    stamps, the hits, the classes and the table of immovable classes) holds;
  - the coverage floor: what the extended family exists for does happen in its default seeds;
  - sensitivity: with exactly one behaviour of the stand-in made wrong, the default extended seeds fail, naming the operation.
"""
import json
import os

import pytest

import fake_rio_gp
import test_gpu_fuzz as fuzz

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuzz_old_family_ops.json")

FLOOR = (
    "rebalance moved rows",
    "rebalance selected rows that all stayed",
    "rebalance with max_moves 0 and a surplus",
    "rebalance with dead nodes right after a flip",
    "rebalance under self-assign",
    "rebalance while a solve is uncommitted",
    "rebalance between tick_async and tick_wait",
    "paged feed with a writer before the next page",
    "feed with hidden rows that differ from the checkpoint",
    "feed reset",
    "index answered with ERANGE",
    "index while a solve is uncommitted",
    "remap removed nodes that held rows",
    "remap pure permutation",
    "remap while a solve is uncommitted",
    "remap refused with a solve uncommitted",
    "remap between tick_async and tick_wait",
    "remap with a checkpoint naming a removed node",
    "remap with hidden rows on a removed node",
    "remap right after a flip",
    "remap down to a kernel's node-count boundary",
    "rebalance on a handle whose m is below max_nodes",
    "place_pending on a handle whose m is below max_nodes",
    "expire un-placed rows",
    "expire capped below n_idle",
    "expire with a placed row stamped exactly at the cutoff",
    "expire as the first call of the family",
    "expire listed rows while a solve was uncommitted",
    "expire hit nothing while a solve was uncommitted",
    "expire between tick_async and tick_wait",
    "expire with hidden placed rows older than the cutoff",
    "expire at n == 0",
    "expire on a handle whose m is below max_nodes",
    "expire between two pages of the feed",
    "touch while a solve is uncommitted",
    "touch with hidden rows",
    "touch_dev skipped invalid entries",
    "touch between tick_async and tick_wait",
    "hits saturated exactly at 0xFFFFFFFF",
    "hits_dev skipped invalid entries",
    "hits merge from an unaligned device array",
    "hits merge of rows not a multiple of 4",
    "hits while a solve is uncommitted",
    "hits with hidden rows holding hits",
    "hits between tick_async and tick_wait",
    "fold with used not valid",
    "fold on more than 4 096 nodes",
    "fold on a handle whose m is below max_nodes",
    "fold with n not a multiple of 4 and hits in the quad behind n",
    "fold changed no load",
    "fold clamped every load to one value",
    "fold while a solve is uncommitted",
    "fold between tick_async and tick_wait",
    "fold refused with a solve uncommitted",
    "top by hits before any hits call",
    "top cut inside a tie group spanning tiles",
    "top listed all 4 096",
    "top with cap above n_candidates",
    "top between two pages of the feed",
    "top right after an expire that listed rows",
    "top while a solve is uncommitted",
    "top between tick_async and tick_wait",
    "top on a handle whose m is below max_nodes",
    "top at n == 0",
    "by-load cut moved rows",
    "by-load cut after a fold made every load equal",
    "by-load cut with more than 3 072 over nodes",
    "by-load cut with zero-load candidates on an over node",
    "by-load cut between tick_async and tick_wait",
    "by-load cut on a handle whose m is below max_nodes",
    "classes batch with duplicates of one row",
    "classes range with unaligned start and end",
    "classes with hidden rows holding classes",
    "classes while a solve is uncommitted",
    "classes between tick_async and tick_wait",
    "classes batch right before an update batch of the same rows",
    "classes_dev batch skipped invalid entries",
    "class sweep un-placed rows",
    "class sweep capped below n_idle",
    "class sweep with rows of a class >= n_classes",
    "class sweep with a placed row stamped exactly at its class's cutoff",
    "class sweep as the first call of the section",
    "class sweep right behind a class sweep",
    "class sweep right behind a top",
    "class sweep listed rows while a solve was uncommitted",
    "class sweep hit nothing while a solve was uncommitted",
    "class sweep between two pages of the feed",
    "class sweep on a handle whose m is below max_nodes",
    "class sweep between tick_async and tick_wait",
    "class sweep with hidden placed rows older than their cutoff",
    "class sweep with one cutoff on an all-zero class column",
    "class sweep under one cutoff against rio_gp_expire's count",
    "top right after a class sweep that listed rows",
    "census by node in one slice",
    "census by node in several slices",
    "census by node beyond 65 536 cells",
    "census with n_other > 0 by class",
    "census with n_other > 0 by node",
    "census at n == 0",
    "census with n not a multiple of 4 and a placed row in the quad behind n",
    "census with a cell whose load exceeds 2^32",
    "census between two pages of the feed",
    "census on a handle whose m is below max_nodes",
    "census while a solve is uncommitted",
    "census between tick_async and tick_wait",
    "chained across a census",
    "immovable rebalance moved rows",
    "the table changed the moves",
    "immovable rebalance with a node whose pinned load alone exceeds its target",
    "every class immovable with a node over target (surplus 0)",
    "immovable by-load cut moved rows",
    "immovable by-load cut with more than 3 072 over nodes",
    "immovable rebalance on more than 65 536 rows",
    "immovable rebalance on more than 1 024 nodes",
    "immovable rebalance with n not a multiple of 4 and an immovable class in the quad behind n",
    "immovable rebalance with hidden placed rows of an immovable class",
    "immovable rebalance with a table shorter than a class present",
    "immovable rebalance on a handle whose m is below max_nodes",
    "immovable rebalance while a solve is uncommitted",
    "immovable rebalance between tick_async and tick_wait",
    "immovable rebalance in the middle of a quiet run",
    "immovable rebalance right behind a setter that changed a placed row's class",
    "immovable rebalance right behind a class sweep that listed rows",
    "immovable rebalance right behind a movable",
    "plain rebalance after a reset moved rows of a class that had been immovable",
    "the row-by-row restatement agreed on an immovable rebalance that moved rows",
    "movable refused",
    "movable as the first call of the section",
    "movable while a solve is uncommitted",
    "movable between tick_async and tick_wait",
    "chained across a movable",
)

# fault of the stand-in -> the operation the failure must name
FAULTS = {
    "feed_keeps_last_row": "changes",
    "feed_lists_hidden_rows": "changes",
    "rebalance_stale_alive": "rebalance",
    "rebalance_stale_used": "rebalance",
    "rebalance_keeps_solve": "rebalance",
    "index_drops_last_row": "index",
    "index_reads_solved": "index",
    "num_objects_stale_used": "num_objects",
    "remap_keeps_solve": "remap",
    "remap_skips_hidden_rows": "remap",
    "remap_counts_hidden_rows": "remap",
    "remap_checkpoint_none_not_gone": "changes",
    "remap_stale_node_table": "remap",
    "remap_affinity_not_renumbered": "tick",
    "expire_cutoff_inclusive": "expire",
    "expire_unplaces_past_cap": "expire",
    "expire_lists_hidden_rows": "expire",
    "expire_freed_counts_unlisted": "expire",
    "expire_stale_used": "expire",
    "expire_keeps_solve": "expire",
    "expire_zero_hit_drops_solve": "expire",
    "expire_count_only_writes": "expire",
    "touch_overwrites": "touch",
    "touch_all_past_n": "num_objects",
    "touch_dev_stops_at_invalid": "touch",
    "touch_drops_solve": "touch",
    "remap_moves_seen": "remap",
    "hits_add_wraps": "hits",
    "hits_dev_stops_at_invalid": "hits",
    "hits_merge_past_rows": "hits",
    "hits_drop_solve": "hits",
    "fold_past_n": "num_objects",
    "fold_keeps_hits": "fold",
    "fold_clamps_before_gain": "fold",
    "fold_stale_used": "fold",
    "fold_keeps_solve": "fold",
    "fold_refused_still_zeroes_hits": "fold",
    "top_ties_to_highest_rows": "top",
    "top_lists_hidden_rows": "top",
    "top_key_sum_of_listed_only": "top",
    "top_reads_solved": "top",
    "top_writes_past_listing": "top",
    "top_drops_solve": "top",
    "top_hits_key_ignores_flag": "top",
    "by_load_is_row_order": "rebalance",
    "by_load_ties_shed_first_rows": "rebalance",
    "by_load_sheds_zero_load": "rebalance",
    "classes_batch_first_wins": "classes",
    "classes_dev_batch_stops_at_invalid": "classes",
    "classes_range_writes_past_end": "classes",
    "classes_drop_solve": "classes",
    "classes_batch_dirty_pos": "classes",
    "num_objects_clears_classes": "num_objects",
    "remap_clears_classes": "remap",
    "expc_cutoff_inclusive": "expire_classes",
    "expc_high_class_is_class_0": "expire_classes",
    "expc_by_class_listed_only": "expire_classes",
    "expc_by_class_accumulates": "expire_classes",
    "expc_unplaces_past_cap": "expire_classes",
    "expc_lists_hidden_rows": "expire_classes",
    "expc_keeps_solve": "expire_classes",
    "expc_count_only_writes": "expire_classes",
    "census_counts_hidden_rows": "census",
    "census_reads_solved": "census",
    "census_uses_max_nodes": "census",
    "census_other_per_slice": "census",
    "census_dev_adds": "census",
    "census_drops_solve": "census",
    "census_skips_zero_load_rows": "census",
    "movable_ignored": "rebalance",
    "movable_pinned_load_not_counted": "rebalance",
    "movable_counts_as_surplus": "rebalance",
    "movable_class_255_always_movable": "rebalance",
    "movable_stale_classes": "rebalance",
    "movable_writes_affinity": "rebalance",
    "movable_hidden_quad": "rebalance",
    "rebalance_resets_movable": "rebalance",
    "movable_short_table_keeps_old_flags": "movable",
    "movable_refused_still_sets": "movable",
    "movable_drops_solve": "movable",
    "remap_resets_movable": "remap",
    "num_objects_resets_movable": "num_objects",
}


def test_old_family_replays_its_recorded_operations(oracle):
    want = json.load(open(GOLDEN))
    assert sorted(int(k) for k in want) == list(range(36))
    for seed in range(36):
        sc = fuzz.Scenario(fake_rio_gp.module(), oracle, seed)
        sc.run()
        assert {"n": sc.n, "m": sc.m, "ops": sc.log} == want[str(seed)], seed


def test_op_tables():
    """The old table is what it was; the extended one is the old entries plus the new operations."""
    assert fuzz.Scenario.OPS == (("tick", 5), ("solve", 2), ("async", 3), ("flip", 4), ("update", 2), ("remove", 2), ("lookup", 1),
                                 ("clean", 2), ("place", 4), ("mixed", 3), ("attrs", 1), ("caps", 1))
    assert fuzz.Scenario.OPS_EXT[:len(fuzz.Scenario.OPS)] == fuzz.Scenario.OPS
    assert [a for a, _ in fuzz.Scenario.OPS_EXT[len(fuzz.Scenario.OPS):]] == ["index", "rebalance", "changes", "changes_reset",
                                                                            "num_objects", "remap", "touch", "expire", "hits", "fold", "top",
                                                                            "classes", "expire_classes", "census", "movable"]


@pytest.fixture(scope="module")
def clean_run(oracle):
    """The default extended seeds against the stand-in: (coverage counters, operation counts)."""
    cov, count = {}, {}
    for seed in range(fuzz.EXT_SEEDS):
        sc = fuzz.Scenario(fake_rio_gp.module(), oracle, seed, ext=True)
        sc.run()
        for k, v in sc.cov.items():
            cov[k] = cov.get(k, 0) + v
        for k, v in sc.count.items():
            count[k] = count.get(k, 0) + v
    return cov, count


def test_extended_seeds_run_clean_and_use_every_new_operation(clean_run):
    cov, count = clean_run
    for op in ("index", "rebalance", "changes", "changes_reset", "num_objects", "remap", "touch", "expire", "in flight: index",
               "in flight: changes", "in flight: rebalance", "in flight: remap", "in flight: touch", "in flight: expire",
               "mid run: touch", "mid run: expire count", "mid run: expire", "hits", "fold", "top", "in flight: hits",
               "in flight: fold", "in flight: top", "mid run: hits", "mid run: fold", "mid run: top", "classes", "expire_classes",
               "census", "in flight: classes", "in flight: expire_classes", "in flight: census", "mid run: classes",
               "mid run: expire_classes count", "mid run: expire_classes", "mid run: census", "movable", "in flight: movable",
               "mid run: movable"):
        assert count.get(op, 0) > 0, (op, count)


def test_coverage_floor(clean_run):
    cov, count = clean_run
    missing = [k for k in FLOOR if cov.get(k, 0) < 1]
    assert not missing, (missing, cov, count)


def test_immovable_rebalances_meet_the_row_by_row_restatement(clean_run):
    """tests/spec_movable.py is consulted under a bound on its cost (live nodes x selected rows x rounds <= 4 000 000: all 128 plain
    rebalances of at most 4 096 rows in the default seeds before the table existed lay below 2 500 000), so at most 1 in 20 of the
    rebalances under a table on at most 4 096 rows may go without it."""
    cov, count = clean_run
    total = cov.get("immovable rebalance of at most 4 096 rows", 0)
    skipped = cov.get("immovable rebalance of at most 4 096 rows without the row-by-row restatement", 0)
    assert total >= 20 and 20 * skipped <= total, (skipped, total)


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_a_wrong_handle_is_noticed(oracle, fault):
    assert set(FAULTS) == set(fake_rio_gp.FAULTS)
    for seed in range(fuzz.EXT_SEEDS):
        sc = fuzz.Scenario(fake_rio_gp.module(fault), oracle, seed, ext=True)
        try:
            sc.run()
        except AssertionError as e:
            assert FAULTS[fault] in repr(e.args), (fault, seed, e.args)
            return
    pytest.fail("no default extended seed noticed the fault %r" % fault)
