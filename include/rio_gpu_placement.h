/*
 * rio_gpu_placement.h — C ABI of the MI355X batched object-placement solver.
 *
 * This is the drop-in boundary for rio-rs' `object_placement::*` hot path.  Nothing like it
 * exists in the reference (pure Rust, static dispatch); these are the entry points an FFI
 * binding for that path would call.  Every entry point cites the reference interface it
 * replaces (paths relative to /root/reference):
 *
 *   trait ObjectPlacement            rio-rs/src/object_placement/mod.rs:38-56
 *   LocalObjectPlacement (semantics) rio-rs/src/object_placement/local.rs:22-68
 *   placement policy                 rio-rs/src/service.rs:193-298
 *   error convention                 rio-rs/src/errors.rs:135-142
 *
 * Two layers are exported from the same shared library (librio_gp.so):
 *
 *   rio_gp_*  dense-index layer.  Objects are rows 0..n-1, nodes are 0..m-1, the table
 *             (object: cur/load/aff) x (node: cap/alive/used) lives in HBM.  Plain
 *             uint32_t/uint64_t arrays, caller-owned, copied in/out.  `_dev` variants take
 *             device pointers (inputs already resident in HBM).
 *   rio_op_*  string layer (rio_gpu_object_placement.h): (struct_name, object_id) and
 *             "ip:port" strings, i.e. exactly the ObjectPlacement trait; interns strings
 *             to dense ids on the host and calls the rio_gp_* layer.
 *
 * Conventions
 *   - Every call returns int: 0 = ok.  Non-zero HIP status -> RIO_GP_EUPSTREAM
 *     (ObjectPlacementError::Upstream); bad argument/index -> RIO_GP_EINVAL
 *     (ObjectPlacementError::Unknown).  A lookup miss is RIO_GP_NONE in the output with
 *     rc 0, never an error (local.rs:48).  Nothing throws or aborts across the ABI.
 *   - A handle is internally synchronized (one mutex + one HIP stream per handle); calls
 *     are synchronous on return unless the name ends in `_async`.
 *     "Synchronous" means the results are in the caller's buffers and every effect is
 *     ordered before the handle's next call; the library waits on completion words its
 *     kernels store into mapped pinned memory (the calling thread spins for the length of
 *     the call — call from a blocking pool, not from an async executor thread) and asks
 *     the HIP stream only when a word does not arrive (a device fault surfaces there).
 *   - There is NO CPU fallback: rio_gp_create fails with RIO_GP_ENODEV without a gfx950
 *     device.
 */
#ifndef RIO_GPU_PLACEMENT_H
#define RIO_GPU_PLACEMENT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: rio_op_cfg.flags == 0 means the reference's first touch (round 5 flipped the default: RIO_OP_CFG_LIVE_FIRST_TOUCH opts out),
 * rio_op_cfg.reserved became collect_ns, rio_gp_mixed_batch and the rio_op_*_batch_n / rio_op_try_* calls exist, RIO_GP_EAGAIN.
 * A client built against version 1 that passes flags = 0 gets another placement policy: compare rio_gp_abi_version() with the
 * header it was built against. */
#define RIO_GP_ABI_VERSION 2u

/* "not placed": Option::None of lookup (object_placement/mod.rs:50). */
#define RIO_GP_NONE 0xFFFFFFFFu
/* hard limits of the solver */
#define RIO_GP_MAX_NODES 8192u
#define RIO_GP_MAX_OBJECTS 0x7FFFF000ull
/* capacity value meaning "unbounded" (the reference has no capacity at all) */
#define RIO_GP_CAP_INF 0xFFFFFFFFFFFFFFFFull
/* Affinity value of a row that is NOT an object: the dense twin of "no entry in the map" (a key that was never
 * inserted, or was removed: local.rs:36-37,60-68, or dropped by clean_server: local.rs:51-58).  A whole-table solve
 * keeps such a row where it is if it happens to be placed on a live node and never places it otherwise; it is not
 * counted in rio_gp_stats.n_objects.  Any other affinity >= the node count (RIO_GP_NONE included) means "an object
 * without a preferred node": it goes to the water-fill. */
#define RIO_GP_AFF_INACTIVE 0xFFFFFFFEu
/* rio_gp_cfg.flags */
/* Row lifecycle (what the string layer uses): rows start as non-objects (affinity RIO_GP_AFF_INACTIVE) and the CRUD
 * calls maintain that column — update(i, node) and the first place_pending request of a pending row make row i an
 * object (affinity = the node / the requester), update(i, NONE), remove and clean_server make it a non-object again.
 * Without the flag the affinity column is only ever written by rio_gp_set_objects / rio_gp_set_object_attrs. */
#define RIO_GP_CFG_ROW_LIFECYCLE 1u
/* Reference-faithful first touch.  By default a node (a requester) that membership marks inactive is not a placement target:
 * a pending object whose affinity node / requester is not alive goes to the water-fill.  The reference has no such test —
 * Service::get_or_create_placement updates the object onto self.address whatever the membership says about self
 * (service.rs:244-252), and evicts it again on the next touch (service.rs:227-237).  With this flag the solver does the
 * same: a pending row claims its affinity node (a place_pending request: its requester) whether or not that node is alive,
 * against the node's whole capacity; rows on nodes that are not alive are still evicted, and the water-fill still places
 * on live nodes only.  With unbounded capacities rio_gp_tick / rio_gp_place_pending then equal the reference request by
 * request for ANY membership (tests/test_gpu_object_placement.py).  Single-GPU handles only: the rio_gp_shard_* calls
 * return RIO_GP_EINVAL on a handle created with it. */
#define RIO_GP_CFG_REF_SELF_ASSIGN 2u

/* return codes */
#define RIO_GP_OK 0
#define RIO_GP_EINVAL 1    /* -> ObjectPlacementError::Unknown  (errors.rs:140-141) */
#define RIO_GP_EUPSTREAM 2 /* -> ObjectPlacementError::Upstream (errors.rs:137-138) */
#define RIO_GP_ENODEV 3    /* no HIP device / not gfx950: the product path fails loudly */
#define RIO_GP_ENOMEM 4
#define RIO_GP_ERANGE 5    /* string layer, and rio_gp_rows_on_nodes: the caller's output buffer is too small (nothing is
                            * truncated; the sizes needed are reported) */
#define RIO_GP_EAGAIN 6    /* string layer, rio_op_try_*: the host shadow cannot answer without the device (or without a lock a device
                            * call may hold): nothing was done, make the blocking call */

/* per-request outcome of rio_gp_place_pending (service.rs:193-298 folded into one code) */
#define RIO_GP_FLAG_LOCAL 0u      /* already placed on the requester (sticky hit, service.rs:241-242,262-264) */
#define RIO_GP_FLAG_REDIRECT 1u   /* already placed on another live node (ResponseError::Redirect, service.rs:286-289) */
#define RIO_GP_FLAG_PLACED 2u     /* was unplaced/evicted, now first-touch placed on the requester (service.rs:244-252) */
#define RIO_GP_FLAG_SPILLED 3u    /* requester full: placed on another node (capacity extension; caller redirects) */
#define RIO_GP_FLAG_UNPLACED 4u   /* no capacity anywhere: stays RIO_GP_NONE */
/* OR-ed onto PLACED / SPILLED / UNPLACED of the request that found its object on a server that is not alive: that server
 * was cleaned (clean_server, service.rs:227-237) and the object re-placed by this call — check_address_mismatch's
 * "placed elsewhere, but there is dead" branch (service.rs:268-285).  Later requests for the same object in the same batch
 * observe the new placement (LOCAL / REDIRECT). */
#define RIO_GP_FLAG_REPLACED 0x10u
#define RIO_GP_FLAG_MASK 0x0Fu    /* the five outcomes above */

typedef struct rio_gp rio_gp_t;

typedef struct rio_gp_cfg {
    uint32_t struct_size;  /* = sizeof(rio_gp_cfg); ABI guard */
    int32_t device;        /* HIP device ordinal */
    uint64_t max_objects;  /* row capacity of the object table (<= RIO_GP_MAX_OBJECTS) */
    uint32_t max_nodes;    /* row capacity of the node table (<= RIO_GP_MAX_NODES) */
    uint32_t spill_rounds; /* water-fill rounds for objects their affinity node rejects; 0 -> default 2 */
    uint32_t flags;        /* RIO_GP_CFG_* bits, 0 = none */
    uint32_t reserved;
} rio_gp_cfg;

/* Counters of one whole-table solve (rio_gp_tick / rio_gp_solve). */
typedef struct rio_gp_stats {
    uint64_t n_objects; /* rows that are objects = kept + claimed + spilled + unplaced */
    uint64_t kept;      /* sticky: placed on a live node (service.rs:241-242) */
    uint64_t evicted;   /* were placed on a dead node (clean_server, service.rs:227-237) */
    uint64_t claimed;   /* pending, admitted on their affinity node (first touch, service.rs:244-252) */
    uint64_t spilled;   /* pending, placed on another node by the water-fill */
    uint64_t unplaced;  /* pending, no room: stay RIO_GP_NONE */
    uint64_t load_kept, load_claimed, load_spilled, load_unplaced;
    uint32_t cut_nodes;   /* nodes whose claimants exceeded their free capacity */
    uint32_t slow_path;   /* 0 = single-pass fast path, 1 = cut/spill fix-up ran */
    uint32_t rounds_run;  /* spill rounds executed */
    uint32_t reserved;
} rio_gp_stats;

/* ---- lifetime -------------------------------------------------------------------------- */

/* ObjectPlacement::prepare (mod.rs:42-44; SQL migrations sqlite.rs:58-66): allocate the HBM
 * tables, create the stream.  `*out` is NULL on failure; rio_gp_last_error(NULL) has the text. */
int rio_gp_create(const rio_gp_cfg* cfg, rio_gp_t** out);
void rio_gp_destroy(rio_gp_t* h);
/* Text of the last failure on this handle (or of the last failed create when h == NULL).
 * The Rust adapter wraps it as ObjectPlacementError::{Upstream,Unknown}(text). */
const char* rio_gp_last_error(rio_gp_t* h);
/* Change RIO_GP_CFG_REF_SELF_ASSIGN after creation (the only bit that may change; every other bit of `flags` must equal the
 * handle's).  The string layer uses it around rio_op_tick: a whole-table solve has no requester that vouches for itself, so it
 * places on active members only even when requests self-assign.  Counts as a change of the solve's inputs. */
int rio_gp_set_flags(rio_gp_t* h, uint32_t flags);
/* "hip:gfx950" — there is no other backend. */
const char* rio_gp_backend(rio_gp_t* h);
uint32_t rio_gp_abi_version(void);
/* hipStreamSynchronize on the handle's stream. */
int rio_gp_sync(rio_gp_t* h);

/* ---- node table: the "node" side, fed by MembershipStorage (cluster/storage/mod.rs:70-121) */

/* Replace the node table: m nodes, capacity (load units) and liveness (Member.active,
 * cluster/storage/mod.rs:20-58).  cap == NULL -> all RIO_GP_CAP_INF; alive == NULL -> all 1. */
int rio_gp_set_nodes(rio_gp_t* h, uint32_t m, const uint64_t* cap, const uint8_t* alive);
/* MembershipStorage::set_is_active (cluster/storage/mod.rs:80) pushed instead of polled
 * (is_active, mod.rs:102-110).  A push costs no device work of its own: the bitmap waits in mapped pinned memory and
 * reaches the device with the next whole-table solve or tick (whose scan reads it from there), or with one tiny kernel
 * when a request batch needs it first.  Every later call sees the new liveness. */
int rio_gp_set_alive(rio_gp_t* h, uint32_t node, uint8_t alive);
int rio_gp_set_alive_all(rio_gp_t* h, uint32_t m, const uint8_t* alive);
int rio_gp_get_nodes(rio_gp_t* h, uint32_t m, uint64_t* cap, uint8_t* alive, uint64_t* used);

/* ---- object table ---------------------------------------------------------------------- */

/* Define rows 0..n-1: per-object load and affinity (= the requesting server `self.address`
 * of service.rs:244).  All rows start unplaced.  load == NULL -> 1; aff == NULL -> RIO_GP_NONE
 * (RIO_GP_AFF_INACTIVE under RIO_GP_CFG_ROW_LIFECYCLE). */
int rio_gp_set_objects(rio_gp_t* h, uint64_t n, const uint32_t* load, const uint32_t* aff);
int rio_gp_set_objects_dev(rio_gp_t* h, uint64_t n, const uint32_t* d_load, const uint32_t* d_aff);
/* Bulk-load / dump the whole assignment column (warm start, snapshot; the on-disk twin is
 * object_placement(struct_name, object_id, server_address), migrations/0001-sqlite-init.sql:1-9). */
int rio_gp_set_assign(rio_gp_t* h, uint64_t n, const uint32_t* assign);
int rio_gp_set_assign_dev(rio_gp_t* h, uint64_t n, const uint32_t* d_assign);
int rio_gp_get_assign(rio_gp_t* h, uint64_t n, uint32_t* out_assign);
/* Read the load and/or affinity columns back (either may be NULL). */
int rio_gp_get_objects(rio_gp_t* h, uint64_t n, uint32_t* out_load, uint32_t* out_aff);
/* Change load and/or affinity of individual rows (either array may be NULL = leave as is). */
int rio_gp_set_object_attrs(rio_gp_t* h, uint64_t n, const uint32_t* idx, const uint32_t* load,
                            const uint32_t* aff);
/* Change how many rows take part (0 <= n <= max_objects) WITHOUT touching their contents: rows >= n are neither
 * solved nor valid indices until n grows again.  A host that hands out rows one by one (the string layer's interning)
 * keeps n at its high-water mark so that a solve streams the rows in use, not the table's capacity. */
int rio_gp_set_num_objects(rio_gp_t* h, uint64_t n);
/* Number of placed rows (HashMap::len of local.rs:12): one 4 B/row pass. */
int rio_gp_count_placed(rio_gp_t* h, uint64_t* out);
/* Device pointer of the live assignment column (valid until the next tick/commit). */
const uint32_t* rio_gp_assign_dev(rio_gp_t* h);
uint64_t rio_gp_num_objects(rio_gp_t* h);
uint32_t rio_gp_num_nodes(rio_gp_t* h);

/* ---- the ObjectPlacement CRUD, batched -------------------------------------------------- */

/* ObjectPlacement::lookup (mod.rs:50; local.rs:42-49): out_node[k] = node of idx[k] or
 * RIO_GP_NONE.  idx[k] >= n is RIO_GP_EINVAL. */
int rio_gp_lookup_batch(rio_gp_t* h, uint64_t n, const uint32_t* idx, uint32_t* out_node);
int rio_gp_lookup_batch_dev(rio_gp_t* h, uint64_t n, const uint32_t* d_idx, uint32_t* d_out_node);
/* ObjectPlacement::update (mod.rs:46-49; local.rs:22-40): upsert idx[k] -> node[k];
 * node[k] == RIO_GP_NONE deletes (local.rs:36-37).  Duplicate idx in one batch resolve as the
 * sequential loop would: the highest batch position wins. */
int rio_gp_update_batch(rio_gp_t* h, uint64_t n, const uint32_t* idx, const uint32_t* node);
int rio_gp_update_batch_dev(rio_gp_t* h, uint64_t n, const uint32_t* d_idx, const uint32_t* d_node);
/* ObjectPlacement::remove (mod.rs:55; local.rs:60-68): un-place; absent is a no-op. */
int rio_gp_remove_batch(rio_gp_t* h, uint64_t n, const uint32_t* idx);
int rio_gp_remove_batch_dev(rio_gp_t* h, uint64_t n, const uint32_t* d_idx);
/* ObjectPlacement::clean_server (mod.rs:52; local.rs:51-58): un-place EVERY object whose
 * node == `node` (one coalesced pass over the assignment column). */
int rio_gp_clean_server(rio_gp_t* h, uint32_t node, uint64_t* evicted);
/* Same for any number of failed nodes in ONE pass: bit j of dead_bitmap (ceil(m/64) words). */
int rio_gp_clean_servers(rio_gp_t* h, const uint64_t* dead_bitmap, uint64_t* evicted);

/* ---- node removal: renumber the node table and every column that names a node --------------- */

/* change feed only: out_old of a row whose last-told node has since been removed */
#define RIO_GP_NODE_GONE 0xFFFFFFFCu

/* MembershipStorage::remove (rio-rs/src/cluster/storage/mod.rs:77, next to push :74 and set_is_active :80) for the dense
 * table: node ids are handed back.  m = rio_gp_num_nodes(h); map has m entries: map[j] = the new id of node j, or RIO_GP_NONE
 * when node j is removed.  The kept entries hit every value of 0 .. m_new-1 exactly once (so m_new <= m; m_new == m is a pure
 * permutation).  The rule (DESIGN.md section 2 rule 8) is exactly rio_gp_clean_servers over the removed nodes, then a
 * renumbering, over every row the handle holds — the rows >= n that rio_gp_set_num_objects hides included:
 *   - assignment: a value v < m becomes map[v]; a row on a removed node becomes RIO_GP_NONE (and, under
 *     RIO_GP_CFG_ROW_LIFECYCLE, a non-object, as clean_server makes it: local.rs:51-58); values >= m (RIO_GP_NONE, ids a
 *     shrinking rio_gp_set_nodes left behind) stay.  *evicted (may be NULL) = the rows < n un-placed this way: what
 *     rio_gp_clean_servers would report.
 *   - affinity: v < m becomes map[v], an affinity naming a removed node becomes RIO_GP_NONE ("no preferred node");
 *     RIO_GP_AFF_INACTIVE and every other value >= m stay.
 *   - the feed's checkpoint B (only if the feed has been used; nothing is allocated otherwise): v < m becomes map[v], a
 *     removed node becomes RIO_GP_NODE_GONE.  A row last told "on j" and now un-placed is listed by the next rio_gp_changes
 *     as (r, RIO_GP_NODE_GONE, RIO_GP_NONE); a row whose node was only renumbered is not listed.
 *   - node table: cap and alive of node j move to map[j] (a rio_gp_set_alive* push still waiting is applied first); the node
 *     count becomes m_new; `used` is the one of the new column on return.
 *   - Like rio_gp_update_batch: it joins rio_gp_tick_async work in flight, drops an uncommitted rio_gp_solve and counts as a
 *     change of the inputs.  Load, n, the counters and the index scratch are untouched.  Node ids handed out before the call
 *     (lookups, listings) are void after it.
 *   - RIO_GP_EINVAL, nothing changed: map == NULL, a kept value >= m_new, a value that appears twice, fewer than m_new kept
 *     entries, or a handle of the row-sharded solve.
 *   - Cost: one streaming pass, 8 B read per row (12 B with the feed in use); a column's tile of 256 rows is written only
 *     where one of its values changes. */
int rio_gp_remap_nodes(rio_gp_t* h, uint32_t m_new, const uint32_t* map, uint64_t* evicted);

/* ---- reverse index: the rows on given nodes ------------------------------------------------ */

/* Reverse index of the assignment column: the object_placement(server_address) index (idx_object_placement_server_address,
 * rio-rs/src/object_placement/migrations/0001-sqlite-init.sql:9) and the Redis backend's reverse set per address
 * (rio-rs/src/object_placement/redis.rs:46-52,68-72), built on demand.  For every node j < m selected by node_bitmap (bit j of
 * word j/64; NULL = every node; bits >= m are ignored, as rio_gp_clean_servers does) the rows whose assignment is j, ascending,
 * concatenated in node order: node j's rows are out_rows[out_offsets[j] .. out_offsets[j+1]).  out_offsets has m + 1 entries
 * (an unselected node: an empty range); *n_rows = out_offsets[m].
 *   - The index of exactly the column rio_gp_get_assign returns at the same point: rows 0 .. n-1 whatever their affinity or
 *     lifecycle state; a row holding RIO_GP_NONE, or any node id >= m (rows a shrinking rio_gp_set_nodes left behind), is listed
 *     nowhere.  The output is one fixed byte string for a given column.
 *   - Read-only: no table, counter, `used` vector or pending solve changes.
 *   - out_rows == NULL with rows_cap == 0: counts only (the offsets).  *n_rows > rows_cap: RIO_GP_ERANGE with the offsets and
 *     *n_rows filled, out_rows untouched.
 *   - Scratch, allocated with the first call and kept until rio_gp_destroy: 8 MiB + 100 KiB of device memory and 64 KiB of
 *     mapped pinned host memory for every (n, m) up to RIO_GP_MAX_OBJECTS x RIO_GP_MAX_NODES; the host-pointer form also
 *     stages its listing in device memory (4 B per listed row, kept at the largest answer so far).
 * The _dev form takes device pointers (d_offsets: m + 1 u64, d_rows: rows_cap u32) and waits once. */
int rio_gp_rows_on_nodes(rio_gp_t* h, const uint64_t* node_bitmap, uint64_t* out_offsets, uint32_t* out_rows,
                         uint64_t rows_cap, uint64_t* n_rows);
int rio_gp_rows_on_nodes_dev(rio_gp_t* h, const uint64_t* node_bitmap, uint64_t* d_offsets, uint32_t* d_rows,
                             uint64_t rows_cap, uint64_t* n_rows);

/* ---- bounded rebalance: move objects off nodes over their load target ------------------------ */

#define RIO_GP_REBALANCE_ROW_ORDER 0u /* R1: a node's candidates are cut in row order */
#define RIO_GP_REBALANCE_BY_LOAD 1u   /* R1': in (load, row) order: the heaviest are shed first */

typedef struct rio_gp_rebalance_cfg {
    uint32_t struct_size;    /* = sizeof(rio_gp_rebalance_cfg); ABI guard.  24 (the struct up to `target`, as it was before
                                `order` existed) is accepted too and means row order: the fields behind it are not read.  Every
                                other size: RIO_GP_EINVAL */
    uint32_t rounds;         /* water-fill rounds; 0 = the handle's spill_rounds; <= 8 */
    uint64_t max_moves;      /* B: rows selected at most; ~0 = no limit */
    const uint64_t* target;  /* host array of m u64 (T[j]; ~0 = never over); NULL = the capacities */
    uint32_t order;          /* RIO_GP_REBALANCE_ROW_ORDER / RIO_GP_REBALANCE_BY_LOAD; anything else: RIO_GP_EINVAL */
    uint32_t reserved;       /* 0 (RIO_GP_EINVAL otherwise) */
} rio_gp_rebalance_cfg;

typedef struct rio_gp_rebalance_stats {
    uint64_t surplus_rows, surplus_load;          /* R1: candidates beyond the cut of their node */
    uint64_t selected_rows, selected_load;        /* R2: the first B of them */
    uint64_t moved_rows, moved_load;              /* rows whose node changed */
    uint64_t stayed_rows;                         /* selected, no place found: kept where they were (R4) */
    uint32_t nodes_over_before, nodes_over_after; /* live nodes j with used[j] > T[j] */
} rio_gp_rebalance_stats;

/* Bounded rebalance of the COMMITTED column ("rebalance"): the rule is the sticky rule's missing half —
 * capacity is enforced on objects already placed.  A row on a live node is a candidate (an object) or pinned (a non-object,
 * affinity RIO_GP_AFF_INACTIVE); every other row (unplaced, on a dead node, on a node >= m) is left exactly as it is.
 *   R1  per live node j, free_j = T[j] -sat (pinned load on j); j's candidates in row order are kept while the inclusive prefix
 *       of their loads stays <= free_j; the first that overflows and every later one are surplus.
 *   R1' (cfg->order = RIO_GP_REBALANCE_BY_LOAD, in place of R1) j's candidates are taken in the order (load ascending, then
 *       row ascending) and kept while the inclusive prefix of their loads stays <= free_j; the first that overflows and every
 *       later one in that order are surplus: the heaviest rows are shed, and a node's surplus is the SMALLEST set of its
 *       candidates whose removal leaves <= free_j.  Per node surplus_rows is therefore <= what R1 gives on the same table
 *       (surplus_load may be larger: the heavy tail can overshoot), and a candidate of load 0 is never surplus.  As a
 *       threshold: per over node a pair (tau_j >= 1, cutrow_j); candidate i is surplus iff load[i] > tau_j, or load[i] ==
 *       tau_j and i >= cutrow_j.  tau_j is the load of the first overflowing candidate; with rem_j = free_j - (the load of
 *       j's candidates below tau_j) and c_j = floor(rem_j / tau_j), cutrow_j is the row of the (c_j + 1)-th candidate of j
 *       with load tau_j, in row order.  R1 is the case in which every key is 0.  R2, R3 and R4 do not change: the budget is
 *       still the first B surplus rows in row order, and the fill runs in row order.
 *   R2  the first B surplus rows in row order are selected.
 *   R3  the selected rows are water-filled in row order exactly as in rule 3, with free = T -sat used' on live nodes (used' =
 *       the load of every row that is not selected) in place of cap - used, `rounds` rounds; a row's own node is a legal target.
 *   R4  a selected row that finds no node keeps its node.
 * Nothing else changes (load, affinity, row lifecycle, n); `used` is the one of the new column on return.  It never places,
 * evicts or cleans: that is the tick's and clean_server's work.
 *   - out_rows / out_from / out_to: the moves (rows whose node changed), ascending by row, with the old and the new node; the
 *     three are given together or not at all (RIO_GP_EINVAL).  With them B = min(max_moves, moves_cap), so the listing always
 *     fits; without them moves_cap must be 0.  *n_moves (may be NULL) = the number of moves.  st may be NULL.
 *   - RIO_GP_EINVAL (nothing changed): bad cfg / struct_size, an unknown order, reserved != 0, rounds > 8, the output rule
 *     above, or a handle of the row-sharded
 *     solve (rio_gp_shard_comm_init / _p2p_connect / _tick_async: a row-sharded table is rebalanced through
 *     rio_gp_shard_rebalance_*, below).
 *   - Like rio_gp_update_batch: it joins rio_gp_tick_async work in flight, drops an uncommitted rio_gp_solve, and counts as a
 *     change of the inputs (the next tick takes neither the quiet nor the chained form over the old column).
 *   - Cost: one streaming pass over the column, load and affinity when no live node is over its target; otherwise three more
 *     passes over the table and a few over the selected rows.  By load, one more pass over the table per digit of the
 *     threshold search (3 to 7: the digit is as wide as the over nodes' histograms allow).  Scratch grows with the first
 *     calls and is kept until rio_gp_destroy.
 * The _dev form takes device pointers for the three move arrays. */
int rio_gp_rebalance(rio_gp_t* h, const rio_gp_rebalance_cfg* cfg, rio_gp_rebalance_stats* st, uint32_t* out_rows,
                     uint32_t* out_from, uint32_t* out_to, uint64_t moves_cap, uint64_t* n_moves);
int rio_gp_rebalance_dev(rio_gp_t* h, const rio_gp_rebalance_cfg* cfg, rio_gp_rebalance_stats* st, uint32_t* d_rows,
                         uint32_t* d_from, uint32_t* d_to, uint64_t moves_cap, uint64_t* n_moves);

/* ---- change feed: the placements changed since the last read ---------------------------------- */

#define RIO_GP_CHANGES_PEEK 1u

/* The rows whose node changed since the consumer last looked: what a write-behind mirror of the table (the object_placement
 * rows of rio-rs/src/object_placement/sqlite.rs:68-85, or a Redis / Postgres copy) needs to stay in step without reading the
 * whole column.  The handle keeps a checkpoint column B, one u32 per row: the node the consumer was last told for that row.  B
 * starts as RIO_GP_NONE everywhere, so the first listing holds every placed row.  A = the column rio_gp_get_assign returns at
 * the point of the call (raw values: node ids >= m count like any other).
 *   - A change is a row r < n with A[r] != B[r].  The listing is the first min(total, cap) changes in ascending row order:
 *     out_rows[k] = r, out_old[k] = B[r], out_new[k] = A[r].  *n_changes = total, every change, listed or not.
 *   - Unless flags has RIO_GP_CHANGES_PEEK, B[r] := A[r] for exactly the listed rows.  A small cap therefore pages through the
 *     changes (every page a prefix, never RIO_GP_ERANGE), and a mirror that applies the pages in order stays consistent.
 *   - The three arrays are given together or not at all (RIO_GP_EINVAL); without them cap must be 0: count only, nothing is
 *     advanced.
 *   - Nothing else changes: the table, `used`, the quiet and chained tick state, the counters and an uncommitted solve stay as
 *     they were; B is not an input of any solve (a quiet tick before a consuming call is still quiet and chained after it).
 *   - Like rio_gp_rows_on_nodes it orders itself behind the work in flight: the listing reflects every tick enqueued before
 *     it, rio_gp_tick_async ticks that have not been waited for included.
 *   - Rows >= n are not listed and keep their B.  Shrinking n (rio_gp_set_num_objects) therefore HIDES rows from the feed until
 *     n grows again; then they are compared as usual.
 *   - RIO_GP_EINVAL on a handle of the row-sharded solve (rio_gp_shard_*, rio_gp_p2p_*): a per-shard feed is not implemented.
 *   - out_old may be RIO_GP_NODE_GONE: the node the consumer was last told for that row has since been removed
 *     (rio_gp_remap_nodes) and has no id any more; a mirror treats it as "was placed, on a node that is gone".  Checkpoints
 *     naming a node that was merely renumbered follow the renumbering: such a row is not listed.
 *   - Memory: B takes 4 B per row of max_objects, allocated (filled with RIO_GP_NONE) by the first feed call and kept until
 *     rio_gp_destroy, plus 4 B per 1 024 rows of tile counts; a handle that never calls the feed pays nothing.  The host-pointer
 *     form also stages its listing in device memory (12 B per listed row, kept at the largest listing so far).
 *   - Cost: one streaming pass over A and B (8 B per row) to count; a listing re-reads only the tiles of 1 024 rows that hold a
 *     change and writes 12 B per listed row (and B for them).
 * The _dev form writes into device arrays of cap entries and waits once.  rio_gp_changes_reset sets B := RIO_GP_NONE for every
 * row: the next listing is complete again (a consumer that lost its mirror). */
int rio_gp_changes(rio_gp_t* h, uint32_t flags, uint32_t* out_rows, uint32_t* out_old, uint32_t* out_new, uint64_t cap,
                   uint64_t* n_changes);
int rio_gp_changes_dev(rio_gp_t* h, uint32_t flags, uint32_t* d_rows, uint32_t* d_old, uint32_t* d_new, uint64_t cap,
                       uint64_t* n_changes);
int rio_gp_changes_reset(rio_gp_t* h);

/* ---- idle expiry: last-seen stamps, and un-placing the rows nobody has asked for -------------- */

/* ObjectPlacementItem's "TODO: ttl" and "TODO: last_seen" (rio-rs/src/object_placement/mod.rs:23-24) for the dense table.  The
 * handle keeps a last-seen column S, one u32 per row of max_objects: the caller's epoch at which the row was last touched, 0 =
 * never seen.  Epochs are the caller's numbers; the library reads no clock.  S is written by the touch calls only: ticks, the
 * CRUD calls, rio_gp_place_pending, rio_gp_set_objects, rio_gp_set_num_objects and rio_gp_remap_nodes leave it alone (S names
 * no node).
 *   - rio_gp_touch_batch: S[idx[k]] = max(S[idx[k]], epoch).  A maximum: duplicates and ordering do not matter.  The host form
 *     validates first (an idx[k] >= n is RIO_GP_EINVAL, nothing changes); the _dev form skips invalid entries and reports
 *     RIO_GP_EINVAL, as rio_gp_remove_batch_dev does.
 *   - rio_gp_touch_all: the same for every row r < n.
 *   - rio_gp_touch_merge: S[r] = max(S[r], stamps[r]) for r < rows, rows <= n (RIO_GP_EINVAL otherwise): a host that keeps
 *     stamps of its own hands them over in one streaming pass.
 *   - rio_gp_get_seen: S[0 .. n-1]; n must be the row count, as for rio_gp_get_assign.
 *   - Touch calls are no inputs of any solve: `used`, an uncommitted rio_gp_solve and the quiet and chained tick state stay as
 *     they were.  They order themselves on the handle's stream; rio_gp_touch_all and rio_gp_touch_merge_dev do not wait.
 *
 * rio_gp_expire (DESIGN.md section 2 rule 9).  A = the column rio_gp_get_assign returns at the point of the call.  Row r < n is
 * IDLE iff A[r] != RIO_GP_NONE and S[r] < cutoff (raw values: node ids >= m count as placed; affinity is not consulted).
 *   - *n_idle = every idle row, listed or not.  The listing is the first L = min(n_idle, cap) idle rows in ascending row order:
 *     out_rows[k] = r, out_node[k] = A[r].
 *   - Exactly the listed rows are un-placed as rio_gp_remove_batch of those rows would do it: A[r] := RIO_GP_NONE; under
 *     RIO_GP_CFG_ROW_LIFECYCLE the row becomes a non-object (affinity RIO_GP_AFF_INACTIVE); load and S stay.  `used` follows the
 *     writes when it is valid, as the remove kernels keep it (it stays invalid otherwise and is rebuilt before its next use).
 *     The change feed lists them as (r, old, RIO_GP_NONE) with no extra work.
 *   - *load_freed (may be NULL) = the sum of the listed rows' loads.
 *   - A small cap pages by prefix and bounds the work per sweep: a listed row is no longer idle.  Never RIO_GP_ERANGE.
 *   - The two arrays are given together or not at all; without them cap must be 0: count only, nothing changes at all (the
 *     quiet and chained tick state included, like the feed's count).  cutoff == 0 finds nothing.
 *   - Like the feed it orders itself behind rio_gp_tick_async work in flight.  With L > 0 it behaves like rio_gp_remove_batch:
 *     it drops an uncommitted rio_gp_solve and counts as a change of the inputs.  With L == 0 it changes nothing.
 *   - Rows >= n are never idle and keep their S.
 *   - RIO_GP_EINVAL, nothing changed: n_idle == NULL; the array rule; a handle of the row-sharded solve (rio_gp_shard_*,
 *     rio_gp_p2p_*: a per-shard expiry is not implemented) — the touch calls and rio_gp_get_seen refuse the same way.
 *   - Memory: S takes 4 B per row of max_objects, allocated (zero-filled) by the first call of this section and kept until
 *     rio_gp_destroy, plus the feed's 4 B per 1 024 rows of tile counts; a handle that calls none of them pays nothing.  The
 *     host-pointer form stages its listing in device memory (8 B per listed row).
 *   - Cost: one streaming pass over A and S (8 B per row) to count; the apply pass re-reads only the tiles of 1 024 rows that
 *     hold a listed row.
 * The _dev form writes into device arrays of cap entries and waits once. */
int rio_gp_touch_batch(rio_gp_t* h, uint64_t n, const uint32_t* idx, uint32_t epoch);
int rio_gp_touch_batch_dev(rio_gp_t* h, uint64_t n, const uint32_t* d_idx, uint32_t epoch);
int rio_gp_touch_all(rio_gp_t* h, uint32_t epoch);
int rio_gp_touch_merge(rio_gp_t* h, uint64_t rows, const uint32_t* stamps);
int rio_gp_touch_merge_dev(rio_gp_t* h, uint64_t rows, const uint32_t* d_stamps);
int rio_gp_get_seen(rio_gp_t* h, uint64_t n, uint32_t* out);
int rio_gp_expire(rio_gp_t* h, uint32_t cutoff, uint32_t* out_rows, uint32_t* out_node, uint64_t cap, uint64_t* n_idle,
                  uint64_t* load_freed);
int rio_gp_expire_dev(rio_gp_t* h, uint32_t cutoff, uint32_t* d_rows, uint32_t* d_node, uint64_t cap, uint64_t* n_idle,
                      uint64_t* load_freed);

/* ---- measured load: per-row hit counters, and the fold that turns them into loads ------------- */

/* The reference has no load at all (ObjectPlacementItem, rio-rs/src/object_placement/mod.rs:23-24, carries an id and an address;
 * local.rs keeps a map of the two): like capacity, load is this library's extension, and so is measuring it.  The handle keeps a
 * hit column H, one u32 per row of max_objects: requests counted for the row since the last fold.  H names no node and is
 * written by the calls of this section only: ticks, the CRUD calls, rio_gp_place_pending, rio_gp_set_objects,
 * rio_gp_set_num_objects, rio_gp_remap_nodes and rio_gp_expire leave it alone (a row handed to another object keeps its hits
 * unless its owner folds or the row is hidden: the string layer zeroes its own counters, see rio_op_fold_loads).
 * DESIGN.md section 2 rule 10 (frozen):
 *   - rio_gp_hits_add_batch: H[idx[k]] = min(H[idx[k]] + w[k], 0xFFFFFFFF) for every k, w[k] = 1 when weight is NULL.
 *     Duplicates sum; a saturating sum of non-negative numbers does not depend on the order, so the result is one fixed column.
 *     The host form validates first (an idx[k] >= n is RIO_GP_EINVAL, nothing changes); the _dev form skips invalid entries and
 *     reports RIO_GP_EINVAL, as rio_gp_touch_batch_dev does.
 *   - rio_gp_hits_merge: H[r] = min(H[r] + counts[r], 0xFFFFFFFF) for r < rows, rows <= n (RIO_GP_EINVAL otherwise): a host that
 *     counts for itself hands its counters over in one streaming pass.  d_counts may have any 4-byte alignment.
 *   - rio_gp_get_hits: H[0 .. n-1]; n must be the row count, as for rio_gp_get_seen.
 *   - The hits calls are no inputs of any solve: `used`, an uncommitted rio_gp_solve and the quiet and chained tick state stay as
 *     they were.  They order themselves on the handle's stream; rio_gp_hits_merge_dev does not wait.
 *   - rio_gp_load_fold, for every row r < n (affinity, lifecycle state and placement are not consulted), exact in u64:
 *         x = floor(load[r] * keep / 65536) + H[r] * gain;   load[r] := clamp(x, min_load, max_load);   H[r] := 0
 *     keep <= 65536 (65536 keeps the old load whole, 0 replaces it) and min_load <= max_load, else RIO_GP_EINVAL and nothing
 *     changes.  x cannot overflow: load * keep <= (2^32-1) * 2^16 < 2^48, so the quotient is below 2^32; H * gain <= (2^32-1)^2 =
 *     2^64 - 2^33 + 1; their sum is below 2^64 - 2^32.  Rows >= n keep both load and H.
 *   - Statistics, over rows < n: rows_changed = rows whose load differs afterwards; hits_folded = the sum of H before;
 *     load_before / load_after = the sums of load; max_load_after = the largest load afterwards (0 for n == 0).
 *   - `used` is that of the new loads on return: rio_gp_get_nodes equals the sum of load over the rows r < n with
 *     assign[r] == j < m.  When `used` is valid before the call the pass keeps it in step itself (it then reads the committed
 *     column as well, 4 B per row more); when it is not, it stays invalid and is rebuilt before its next use.
 *   - The fold behaves like rio_gp_set_object_attrs with loads: it orders itself behind rio_gp_tick_async work in flight, drops
 *     an uncommitted rio_gp_solve and counts as a change of the inputs (no tick after it is quiet or chained over the old loads).
 *     The change feed, S and the node index scratch are untouched.
 *   - RIO_GP_EINVAL, nothing changed: a handle of the row-sharded solve (rio_gp_shard_*, rio_gp_p2p_*: a per-shard hit column
 *     is not implemented), for every call of the section.
 *   - Memory: H takes 4 B per row of max_objects, allocated (zero-filled) by the first call of this section and kept until
 *     rio_gp_destroy; a handle that calls none of them pays nothing.
 *   - Cost: the merge streams 8 B per row and writes only the quads that change; the fold streams load and H (8 B per row, 12
 *     with `used` valid) and writes load where it differs and H where it held a hit. */
typedef struct rio_gp_load_fold_stats {
    uint64_t rows_changed, hits_folded, load_before, load_after;
    uint32_t max_load_after, reserved;
} rio_gp_load_fold_stats;
int rio_gp_hits_add_batch(rio_gp_t* h, uint64_t n, const uint32_t* idx, const uint32_t* weight /* NULL = 1 each */);
int rio_gp_hits_add_batch_dev(rio_gp_t* h, uint64_t n, const uint32_t* d_idx, const uint32_t* d_weight);
int rio_gp_hits_merge(rio_gp_t* h, uint64_t rows, const uint32_t* counts);
int rio_gp_hits_merge_dev(rio_gp_t* h, uint64_t rows, const uint32_t* d_counts);
int rio_gp_get_hits(rio_gp_t* h, uint64_t n, uint32_t* out);
int rio_gp_load_fold(rio_gp_t* h, uint32_t keep, uint32_t gain, uint32_t min_load, uint32_t max_load,
                     rio_gp_load_fold_stats* st /* may be NULL */);

/* ---- hot-object report: the k heaviest rows ---------------------------------------------------- */

/* "What makes node X hot", "which objects are the hottest": the ORDER BY load DESC LIMIT k that every store the reference can sit
 * on answers (its ObjectPlacementItem, rio-rs/src/object_placement/mod.rs:23-24, has no load to order by: load is this library's
 * extension, and so is this report).  DESIGN.md section 2 rule 11 (frozen; tests/spec_top.py restates it):
 *   - A is the column rio_gp_get_assign returns at the point of the call; K[r] = load[r], or H[r] (the hit column of
 *     rio_gp_hits_*) under RIO_GP_TOP_BY_HITS.  On a handle that never called the hits family H is all zero, and this call does
 *     not allocate it.
 *   - Row r is a CANDIDATE iff r < n and K[r] >= min_key and, under RIO_GP_TOP_PLACED, A[r] != RIO_GP_NONE (raw values: ids >= m
 *     count as placed, as in rule 9) and, under RIO_GP_TOP_ON_NODE, A[r] == node.  Affinity and lifecycle state are not
 *     consulted; rows >= n are never candidates.
 *   - *n_candidates = every candidate, listed or not; *key_sum = the sum of K over all candidates (fewer than 2^31 rows times
 *     2^32: it cannot overflow).
 *   - The listing is the first L = min(*n_candidates, cap) candidates in the total order (K descending, then r ascending):
 *     out_rows[k] = r, out_key[k] = K[r], out_node[k] = A[r].  One fixed listing: ties at the cut go to the lowest rows.  Entries
 *     from L on are not written.
 *   - out_rows and out_key are given together or not at all; without them cap must be 0 (count only) and out_node NULL.
 *   - RIO_GP_EINVAL: cap > RIO_GP_TOP_MAX, an unknown flag bit, RIO_GP_TOP_ON_NODE with node >= m (node is ignored without the
 *     flag), n_candidates == NULL, a handle of the row-sharded solve (rio_gp_shard_*, rio_gp_p2p_*).
 *   - Read-only: the table, `used`, H, S, the change feed's checkpoint, an uncommitted rio_gp_solve (it stays committable) and
 *     the quiet and chained tick state are as they were.  Like rio_gp_changes it orders itself behind rio_gp_tick_async work in
 *     flight.
 *   - Memory: about 100 KB of device scratch (histograms, the selected rows, the listing), 48 KB of pinned host memory and the
 *     change feed's per-tile counts (4 B per 1 024 rows), allocated by the first call; a handle that never calls pays nothing.
 *   - Cost: an exact radix select on the device: three histogram passes over K (11 / 11 / 10 bits; the second and third are
 *     skipped when everything fits the listing), one collecting pass and a pass over the tiles that hold a tie at the cut, each
 *     4 B per row (8 B under a filter flag, which reads A too); then at most 4 096 rows are sorted and come back.  The _dev form
 *     takes device arrays of cap entries; both forms wait once. */
#define RIO_GP_TOP_BY_HITS 1u /* key = H[r]; without it key = load[r] */
#define RIO_GP_TOP_PLACED 2u  /* only rows with A[r] != RIO_GP_NONE */
#define RIO_GP_TOP_ON_NODE 4u /* only rows with A[r] == node */
#define RIO_GP_TOP_MAX 4096u
int rio_gp_top_rows(rio_gp_t* h, uint32_t flags, uint32_t node, uint32_t min_key, uint32_t* out_rows, uint32_t* out_key,
                    uint32_t* out_node /* may be NULL */, uint64_t cap, uint64_t* n_candidates, uint64_t* key_sum /* may be NULL */);
int rio_gp_top_rows_dev(rio_gp_t* h, uint32_t flags, uint32_t node, uint32_t min_key, uint32_t* d_rows, uint32_t* d_key,
                        uint32_t* d_node /* may be NULL */, uint64_t cap, uint64_t* n_candidates, uint64_t* key_sum /* may be NULL */);

/* ---- object classes: per-class idle limits and a census by class ------------------------------ */

/* Every object of the reference has a type: its key is ObjectId(struct_name, object_id) (rio-rs/src/object_placement/mod.rs:23-24
 * keeps both in ObjectPlacementItem), and the SQL backends store struct_name in a column of its own.  The handle keeps a class
 * column K, one uint8_t per row of max_objects: the caller's number for the row's type, 0 to begin with.  K names no node and is
 * written by the class setters only: ticks, the CRUD calls, rio_gp_place_pending, rio_gp_set_objects, rio_gp_set_num_objects,
 * rio_gp_remap_nodes, the rebalance, rio_gp_expire and the load calls leave it alone.  DESIGN.md section 2 rule 12 (frozen;
 * tests/spec_classes.py restates it):
 *   - rio_gp_set_classes: K[first_row + k] = cls[k] for k < rows.  first_row + rows <= n, else RIO_GP_EINVAL and nothing changes.
 *     Any alignment of first_row, rows and the pointer; no byte outside the range changes.
 *   - rio_gp_set_class_batch: K[idx[k]] = cls[k], processed as if in batch order: of several entries for one row the LAST
 *     wins (the election of rio_gp_update_batch).  The host form validates first (an idx[k] >= n is RIO_GP_EINVAL, nothing
 *     changes); the _dev form skips invalid entries and reports RIO_GP_EINVAL, as rio_gp_touch_batch_dev does.
 *   - rio_gp_get_classes: K[0 .. n-1]; n must be the row count, as for rio_gp_get_seen.
 *   - The class setters are no inputs of any solve: `used`, an uncommitted rio_gp_solve and the quiet and chained tick state stay
 *     as they were.  They order themselves on the handle's stream; rio_gp_set_classes_dev does not wait.
 *
 * rio_gp_expire_classes: rio_gp_expire with a cutoff per class.  Row r < n is IDLE iff A[r] != RIO_GP_NONE and K[r] < n_classes
 * and S[r] < cutoffs[K[r]] (S: the last-seen column of the touch calls).  A row whose class is >= n_classes is never idle; a
 * cutoff of 0 finds nothing in its class.  cutoffs is a HOST array of n_classes entries in both forms, 1 <= n_classes <=
 * RIO_GP_MAX_CLASSES (else RIO_GP_EINVAL).  Everything else is rio_gp_expire's contract: the listing (ascending rows, paged by
 * cap, never RIO_GP_ERANGE), *n_idle (every idle row, listed or not), the count-only form (no arrays, cap 0: nothing changes
 * at all), *load_freed, the un-placing as rio_gp_remove_batch would do it (row lifecycle, `used`), the order behind
 * rio_gp_tick_async work in flight, the uncommitted solve dropped only when a row was listed, the change feed, the refusal on a
 * handle of the row-sharded solve.  idle_by_class (host, n_classes entries, may be NULL): [c] = every idle row of class c,
 * listed or not.  On a handle whose classes are all 0, rio_gp_expire_classes(1, {cutoff}) is rio_gp_expire(cutoff).
 *
 * rio_gp_census: the placed rows by class.  A = the column rio_gp_get_assign returns at the point of the call.  For every
 * r < n with A[r] != RIO_GP_NONE (raw values; affinity and lifecycle state are not consulted):
 *   - K[r] >= n_classes: the row is counted in *n_other only;
 *   - otherwise out_rows[K[r]] += 1 and out_load[K[r]] += load[r]; the arrays hold n_classes entries;
 *   - under RIO_GP_CENSUS_BY_NODE the arrays are [m][n_classes], node-major, the row lands in cell (A[r], K[r]), and a placed
 *     row whose node id is >= m is counted in *n_other only.  m * n_classes <= 2^20, else RIO_GP_EINVAL.
 *   - RIO_GP_EINVAL: an unknown flag, n_classes outside 1 .. RIO_GP_MAX_CLASSES, a NULL among out_rows / out_load / n_other, a
 *     handle of the row-sharded solve.
 *   - Read-only: the table, `used`, K, an uncommitted rio_gp_solve (it stays committable) and the quiet and chained tick state
 *     are as they were.  Like rio_gp_changes it orders itself behind rio_gp_tick_async work in flight.
 *   - The _dev form takes the two arrays in device memory (n_other stays a host word); both forms wait once.
 *   - Memory: K takes 1 B per row of max_objects, allocated (zero-filled) by the first call of this section and kept until
 *     rio_gp_destroy, plus 3 KiB of tables; the host-pointer census stages its cells in device memory (16 B per cell).  A handle
 *     that calls none of them pays nothing.
 *   - Cost: the sweep's count pass streams A, S and K (9 B per row); the census streams A, K and load (9 B per row), once
 *     for up to 4 096 cells and beyond 65 536, once per 4 096 cells in between. */
#define RIO_GP_MAX_CLASSES 256u
#define RIO_GP_CENSUS_BY_NODE 1u /* cells (node, class) instead of (class) */
int rio_gp_set_classes(rio_gp_t* h, uint64_t first_row, uint64_t rows, const uint8_t* cls);
int rio_gp_set_classes_dev(rio_gp_t* h, uint64_t first_row, uint64_t rows, const uint8_t* d_cls);
int rio_gp_set_class_batch(rio_gp_t* h, uint64_t n, const uint32_t* idx, const uint8_t* cls);
int rio_gp_set_class_batch_dev(rio_gp_t* h, uint64_t n, const uint32_t* d_idx, const uint8_t* d_cls);
int rio_gp_get_classes(rio_gp_t* h, uint64_t n, uint8_t* out);
int rio_gp_expire_classes(rio_gp_t* h, uint32_t n_classes, const uint32_t* cutoffs, uint32_t* out_rows, uint32_t* out_node,
                          uint64_t cap, uint64_t* n_idle, uint64_t* load_freed, uint64_t* idle_by_class /* may be NULL */);
int rio_gp_expire_classes_dev(rio_gp_t* h, uint32_t n_classes, const uint32_t* cutoffs, uint32_t* d_rows, uint32_t* d_node,
                              uint64_t cap, uint64_t* n_idle, uint64_t* load_freed, uint64_t* idle_by_class /* may be NULL */);
int rio_gp_census(rio_gp_t* h, uint32_t flags, uint32_t n_classes, uint64_t* out_rows, uint64_t* out_load, uint64_t* n_other);
int rio_gp_census_dev(rio_gp_t* h, uint32_t flags, uint32_t n_classes, uint64_t* d_rows, uint64_t* d_load, uint64_t* n_other);

/* Immovable classes (DESIGN.md section 2 rule 13): the rebalance leaves the objects of chosen types where they are — what
 * Orleans' [Immovable] attribute asks of its rebalancer.  The handle keeps a table I[RIO_GP_MAX_CLASSES] of flags, all
 * "movable" to begin with.  In R0 of rio_gp_rebalance[_dev] a row r < n on a live node j < m is PINNED iff
 * aff[r] == RIO_GP_AFF_INACTIVE or I[K[r]] says immovable (K: the class column above); otherwise it is a candidate.  Everything
 * downstream is rule 6 verbatim: an immovable row's load counts against its node's target as a non-object's does, the row is
 * never surplus, never selected, never moved and never listed, its node may still be a fill target, and the result is that of
 * rule 6 on the same table with the affinity of every immovable object row read as RIO_GP_AFF_INACTIVE (the affinity column
 * itself is not written).  With every class movable the call is the rebalance without the table, launch for launch.
 *   - rio_gp_set_class_movable: movable[c] == 0 makes class c immovable for c < n_classes; the classes >= n_classes become
 *     movable (n_classes = 0, movable = NULL: the table is reset).  RIO_GP_EINVAL, nothing changed: n_classes >
 *     RIO_GP_MAX_CLASSES, a NULL array with n_classes > 0, a handle of the row-sharded solve.  Like the class setters it is no
 *     input of any solve (`used`, an uncommitted rio_gp_solve, the quiet and chained tick state and the change feed stay as
 *     they were) and it may allocate K, zero-filled.  rio_gp_remap_nodes, rio_gp_set_num_objects and the rebalance leave the
 *     table alone.
 *   - rio_gp_get_class_movable: out256[c] = 1 where class c is movable, 0 where it is not, for all RIO_GP_MAX_CLASSES classes.
 *   - Only the rebalance and rio_gp_shed_idle (below: it never sheds such a row) consult the table: ticks, rio_gp_clean_server, node removal, expiry and the CRUD calls treat the rows
 *     as before (a dead node's immovable objects are evicted like any others).
 *   - rio_gp_shard_rebalance_begin[_ordered] on a handle whose table names an immovable class is RIO_GP_EINVAL: a rank's table
 *     has no class column.
 *   - Cost: with an immovable class the table passes of the rebalance read K too, 13 B per row instead of 12. */
int rio_gp_set_class_movable(rio_gp_t* h, uint32_t n_classes, const uint8_t* movable);
int rio_gp_get_class_movable(rio_gp_t* h, uint8_t* out256);

/* Pressure shedding (DESIGN.md section 2 rule 14): on every over-target node, un-place the objects nobody has asked for the
 * longest, and only as many as bring the node back to its target — Orleans' activation shedding under memory pressure.  It is
 * the answer where rio_gp_rebalance leaves stayed_rows (the cluster as a whole is over: nothing can move) and rio_gp_expire's
 * cluster-wide cutoff relieves nothing.  A = the column rio_gp_get_assign returns at the point of the call, S = the last-seen
 * column (rule 9), K = the class column (rule 12), T[j] = cfg->target[j] (NULL: the capacities; ~0: never over).  Only rows
 * r < n with A[r] = j < m and alive[j] take part; every other row (unplaced, on a dead node, on a node id >= m, r >= n) is left
 * exactly as it is.
 *   L0  candidates and pinned rows.  A participating row has an effective cutoff c(r): cfg->cutoff without class_cutoffs; with
 *       them class_cutoffs[K[r]] for K[r] < n_classes and 0 for the classes from n_classes on (as rio_gp_expire_classes treats
 *       them); and 0 for a row of an immovable class (rio_gp_set_class_movable) in either form: shedding deactivates, and rule
 *       13's types are the ones that must not be.  The row is a CANDIDATE iff aff[r] != RIO_GP_AFF_INACTIVE, load[r] >= 1 and
 *       S[r] < c(r); otherwise it is PINNED: its load counts against T[j] and it is never touched.
 *   L1  the cut.  Per live node j: free_j = T[j] -sat (pinned load on j).  j's candidates are taken in the order (S descending,
 *       then row ascending) and kept while the inclusive prefix of their loads stays <= free_j; the first that overflows and
 *       every later one in that order are SURPLUS: the most recently seen stay, the longest idle go.  As a threshold, per over
 *       node (sigma_j, cutrow_j): candidate i is surplus iff S[i] < sigma_j, or S[i] == sigma_j and i >= cutrow_j; sigma_j is the
 *       stamp of the first overflowing candidate, rem_j = free_j - (load of j's candidates with S > sigma_j), and cutrow_j is
 *       the first candidate of j with stamp sigma_j, in row order, whose inclusive load prefix among those ties exceeds rem_j
 *       (rule R1 restricted to the ties).
 *   L2  the budget.  The first B surplus rows in ascending row order are selected: B = cfg->max_rows, or min(max_rows,
 *       rows_cap) with a listing — the listing always fits and the call never answers RIO_GP_ERANGE.  A budget below the
 *       surplus sheds a row-order prefix of it (R2's caveat); the next call cuts afresh.
 *   L3  the outcome.  Exactly the selected rows are un-placed as rio_gp_expire un-places its listed rows: A[r] := RIO_GP_NONE,
 *       under RIO_GP_CFG_ROW_LIFECYCLE the row becomes a non-object, load, S and K stay; `used` follows; the change feed
 *       lists them as (r, old, NONE).  out_rows[k] = r, out_node[k] = A_old[r], ascending by row; *n_rows = shed_rows.
 *   Counters: surplus_rows / surplus_load (L1), shed_rows / shed_load (L3), nodes_over_before / nodes_over_after = the live
 *       nodes with used[j] > T[j] on the old / the new column, as the rebalance counts them.
 *   With shed_rows == 0 (nothing over, B == 0, cutoff 0) nothing changes at all: the column, `used`, S, the feed's checkpoint,
 *       an uncommitted rio_gp_solve, the quiet and chained tick state.  With shed_rows > 0 the call behaves like
 *       rio_gp_remove_batch: it drops an uncommitted solve and counts as a change of the inputs.  Either way it orders itself
 *       behind rio_gp_tick_async work in flight.
 *   RIO_GP_EINVAL, nothing changed or allocated: cfg NULL, struct_size != sizeof(rio_gp_shed_cfg), reserved != 0; n_classes
 *       outside 1 .. RIO_GP_MAX_CLASSES with class_cutoffs, or non-zero without; out_rows / out_node not given together,
 *       rows_cap != 0 without them; a handle of the row-sharded solve.  st and n_rows may both be NULL.
 *   rio_gp_shed_idle_dev: out_rows / out_node are device arrays of rows_cap entries; the call waits for the node pass (the
 *       host picks the over nodes) and once more at its end.  The host-pointer form also waits for the surplus count.
 *   Cost: one pass over A, load, aff and S (16 B a row, 17 with classes) for the node pass, each digit of the selection (the
 *       digits every candidate stamp shares are skipped), the tie walk and the count; nothing past the node pass when no
 *       node is over. */
typedef struct rio_gp_shed_cfg {
    uint32_t struct_size;          /* = sizeof(rio_gp_shed_cfg) */
    uint32_t cutoff;               /* a row may be shed only if S[r] < cutoff */
    uint64_t max_rows;             /* B; ~0 = no limit; 0 = count the surplus, change nothing */
    const uint64_t* target;        /* m u64, NULL = the capacities, ~0 = never over */
    const uint32_t* class_cutoffs; /* NULL, or n_classes u32 in place of cutoff (rule L0) */
    uint32_t n_classes;
    uint32_t reserved;             /* 0 */
} rio_gp_shed_cfg;
typedef struct rio_gp_shed_stats {
    uint64_t surplus_rows, surplus_load, shed_rows, shed_load;
    uint32_t nodes_over_before, nodes_over_after;
} rio_gp_shed_stats;
int rio_gp_shed_idle(rio_gp_t* h, const rio_gp_shed_cfg* cfg, rio_gp_shed_stats* st, uint32_t* out_rows, uint32_t* out_node,
                     uint64_t rows_cap, uint64_t* n_rows);
int rio_gp_shed_idle_dev(rio_gp_t* h, const rio_gp_shed_cfg* cfg, rio_gp_shed_stats* st, uint32_t* d_rows, uint32_t* d_node,
                         uint64_t rows_cap, uint64_t* n_rows);

/* ---- the placement policy, batched ------------------------------------------------------ */

/* Service::get_or_create_placement + check_address_mismatch (service.rs:193-298) for a batch
 * of requests, processed as if sequentially in batch order: request k asks for object idx[k]
 * on server requester[k].
 *   - object placed on a node that is not alive -> clean_server(that node) (all of its objects
 *     are un-placed, service.rs:233-237), the object becomes pending;
 *   - still placed -> sticky: out_node = that node, flag LOCAL / REDIRECT;
 *   - pending -> first touch on requester[k] (service.rs:244-252), admitted while the
 *     requester's free capacity lasts (index-ordered prefix rule), else
 *     water-filled onto the emptiest nodes, else left RIO_GP_NONE.
 * With every capacity = RIO_GP_CAP_INF this is exactly the reference policy.  out_flag may
 * be NULL. */
int rio_gp_place_pending(rio_gp_t* h, uint64_t n, const uint32_t* idx, const uint32_t* requester,
                         uint32_t* out_node, uint32_t* out_flag);
/* The same with request and result arrays already resident in HBM (device pointers; d_out_flag may be NULL).  The
 * entries are checked on the device BEFORE anything is changed: an out-of-range index or requester fails the whole call
 * with RIO_GP_EINVAL and leaves the table as it was. */
int rio_gp_place_pending_dev(rio_gp_t* h, uint64_t n, const uint32_t* d_idx, const uint32_t* d_requester,
                             uint32_t* d_out_node, uint32_t* d_out_flag);

/* Up to 256 entries of EACH of update / remove / lookup / place_pending in one call: exactly rio_gp_update_batch, then
 * rio_gp_remove_batch, then rio_gp_lookup_batch, then rio_gp_place_pending over the given arrays (a count of 0 skips the
 * kind) — but ONE launch and ONE host wait for all of them (one workgroup runs the parts one after the other).
 * This is what the connections of one reference Server ask for at the same moment (lookups, first touches and removals
 * mixed: service.rs:193-254, server.rs:292-304; local.rs:22-68); the string layer's combiner sends one such call per
 * generation of concurrent callers.  rc[k] = what the k-th of those calls would have returned (0 update, 1 remove, 2 lookup,
 * 3 place_pending): a kind with an out-of-range entry changes nothing and reports RIO_GP_EINVAL there, the other kinds still
 * run.  The return value is about the call as a whole (arguments, device). */
typedef struct rio_gp_mixed {
    uint32_t struct_size; /* sizeof(rio_gp_mixed) */
    uint32_t n_update;
    const uint32_t* update_idx;
    const uint32_t* update_node;
    uint32_t n_remove;
    uint32_t n_lookup;
    const uint32_t* remove_idx;
    const uint32_t* lookup_idx;
    uint32_t* lookup_out;
    uint32_t n_place;
    uint32_t reserved;
    const uint32_t* place_idx;
    const uint32_t* place_requester;
    uint32_t* place_node;
    uint32_t* place_flag; /* may be NULL */
    int32_t rc[4];
} rio_gp_mixed;
int rio_gp_mixed_batch(rio_gp_t* h, rio_gp_mixed* ops);

/* Whole-table solve: every row gets a decision in one call (the eager form of the lazy
 * per-request path of service.rs:193-254 + the clean_server stream of SURVEY §3.2):
 * keep if alive (sticky) | claim affinity node by index-ordered prefix | water-fill | NONE.
 *   rio_gp_solve   computes the new assignment column and `used`, does not publish it;
 *   rio_gp_commit  publishes the last solve (pointer swap);
 *   rio_gp_tick    = solve + commit. */
int rio_gp_solve(rio_gp_t* h, rio_gp_stats* stats);
int rio_gp_commit(rio_gp_t* h);
int rio_gp_tick(rio_gp_t* h, rio_gp_stats* stats);
/* The committed tick without a host wait: rio_gp_tick_async enqueues solve + fix-up + commit of one tick on the handle's
 * stream and returns; ticks enqueued back to back each consume the previous one's commit on the device (and any
 * rio_gp_set_alive* pushed in between, in stream order).  rio_gp_tick_wait waits for all of them and hands out their
 * counters, oldest first: *n_out = ticks completed since the last wait, out[0..min(cap, *n_out)) = the most recent ones.
 * The tables are exactly what the same sequence of rio_gp_tick calls produces; only the counters arrive later.  (A
 * server that pushes a membership change and rebalances has no use for the counters before the next push.)
 * On the handle's OWN stream a tick that cannot need the fix-up (nothing has changed since a tick that left every object
 * placed) enqueues no fix-up, and on tables of 2^18 rows and more (up to 1 024 nodes) it is one launch, its scan, which
 * does the resolve step itself: the scans of such ticks alternate between the handle's stream and a second internal one, each
 * wave starting as soon as the same wave of the previous tick's scan has finished its rows (a dependency per row
 * range instead of per launch: the data dependency between two ticks is exactly that).  Every other call of the handle
 * orders itself behind all of it.  On a caller's stream (rio_gp_set_stream) everything stays on that one stream. */
int rio_gp_tick_async(rio_gp_t* h);
int rio_gp_tick_wait(rio_gp_t* h, rio_gp_stats* out, uint32_t cap, uint32_t* n_out);
/* Enqueue one solve on the handle's stream without waiting.  rio_gp_solve_wait drains the
 * stream, runs the cut/spill fix-up for the LAST enqueued solve if it needed one, and
 * returns its stats.  *n_slow = how many of the solves enqueued since the last wait took
 * the fix-up path on the device. */
int rio_gp_solve_async(rio_gp_t* h);
int rio_gp_solve_wait(rio_gp_t* h, rio_gp_stats* stats, uint32_t* n_slow);
/* Device pointer of the column the last solve produced (before commit). */
const uint32_t* rio_gp_solved_dev(rio_gp_t* h);
int rio_gp_get_solved(rio_gp_t* h, uint64_t n, uint32_t* out_assign);

/* ---- row-sharded solve across the GPUs of one node ----------------------- */
/*
 * Rank r (one process, one GPU, one handle) owns the contiguous rows [off_r, off_r + n_r) of the
 * object table; shard order = index order; the node table is replicated.  Rows couple only through
 * the per-node load vectors, so the only cross-rank data are two small records, all-gathered by
 * the CALLER between the calls below (RCCL over xGMI from the Rust/Python host; the library itself
 * never talks to another rank):
 *   X (rio_gp_shard_words1 = 2m+8 u64): local kept load[m] | local claim load[m] | 8 counters
 *   Y (rio_gp_shard_words2 =  m+2 u64): locally admitted load[m] | pending spill load | pending rows
 * Every cross-rank reduction is an integer sum taken in rank order, so the sharded solve equals the
 * unsharded rio_gp_solve of the concatenated table bit for bit.
 *
 *   fast path (nothing cut, nothing spills):   scan -> [all-gather X] -> resolve -> verdict -> finish
 *   fix-up:   ... verdict -> cut -> [all-gather Y] -> merge
 *                 -> { spill(round) -> [all-gather Y] -> merge } while rows are pending -> finish
 * then rio_gp_commit publishes as usual.  d_* are DEVICE pointers owned by the caller.
 */
typedef struct rio_gp_shard_info {
    uint64_t cut_nodes;    /* nodes whose global claim load exceeds their free capacity */
    uint64_t spill_rows;   /* rows (all ranks) whose affinity node is unusable: go to the water-fill */
    uint64_t local_fixup;  /* != 0: THIS rank has claimants to re-mark (pass it to rio_gp_shard_cut) */
    uint64_t kept, evicted, claimants, load_kept, load_claim; /* global row/load counters */
} rio_gp_shard_info;
/* Enqueue every later call of this handle on the caller's HIP stream (hipStream_t as void*; NULL = back
 * to the handle's own stream), e.g. the stream the host's RCCL all-gather is ordered against. */
int rio_gp_set_stream(rio_gp_t* h, void* hip_stream);
uint32_t rio_gp_shard_words1(rio_gp_t* h);
uint32_t rio_gp_shard_words2(rio_gp_t* h);
/* k_scan + local column sums; d_x[words1] = this rank's X record.  Asynchronous. */
int rio_gp_shard_scan(rio_gp_t* h, uint64_t* d_x);
/* d_xg[n_ranks][words1] = the all-gathered X records.  Asynchronous.  on_stream (hipStream_t, may be NULL = the
 * handle's stream): a host that pipelines independent solves runs the exchange and this step on a second stream,
 * ordered after rio_gp_shard_scan by its own event, so the all-gather overlaps the next solve's scan. */
int rio_gp_shard_resolve(rio_gp_t* h, uint32_t rank, uint32_t n_ranks, const uint64_t* d_xg, void* on_stream);
/* Waits for the stream; global verdict of the LAST resolve; *n_slow = how many of the resolves enqueued
 * since the last verdict need the fix-up. */
int rio_gp_shard_verdict(rio_gp_t* h, rio_gp_shard_info* out, uint32_t* n_slow);
/* Fix-up step 1 (only if cut_nodes or spill_rows): exact cut on this rank, d_y[words2] = Y record. */
int rio_gp_shard_cut(rio_gp_t* h, int run_local_fixup, uint64_t* d_y);
/* d_yg[n_ranks][words2] = all-gathered Y records -> global `used`, this rank's spill base.  Synchronous;
 * returns the rows / load still waiting for the water-fill on all ranks. */
int rio_gp_shard_merge(rio_gp_t* h, const uint64_t* d_yg, uint64_t* pending_rows, uint64_t* pending_load);
/* One water-fill round over this rank's pending rows; d_y[words2] = Y record of the round. */
int rio_gp_shard_spill(rio_gp_t* h, uint32_t round, int last, uint64_t* d_y);
/* Local counters of this rank's rows (sum them over ranks; cut_nodes/slow_path/rounds_run are global
 * quantities the caller already holds).  After this, rio_gp_commit / rio_gp_get_solved work as usual. */
int rio_gp_shard_finish(rio_gp_t* h, rio_gp_stats* local_stats);

/* Preferred on one node: peer-to-peer exchange over xGMI with no collective call at all.  Every rank exports an
 * uncached window (rio_gp_shard_p2p_export -> 64-byte hipIpcMemHandle_t), the host all-gathers the handles over its
 * control channel, every rank maps its peers' windows (rio_gp_shard_p2p_connect; ends with a handshake and fails
 * with RIO_GP_EUPSTREAM if a peer's store does not become visible within 3 s — fall back to RCCL then).  After that
 * rio_gp_shard_solve_async is two launches on one stream, no host involvement: the scan, then one kernel in which every
 * workgroup stores its eight nodes' sums straight into the peers' HBM as data-tagged 8-byte words, polls the same words of
 * every rank and resolves its nodes (no flag, no collective).  rio_gp_shard_exchange (fix-up records) stores the raw
 * record and a sequence flag; the consuming kernel waits on the flags.  All ranks must call export/connect/solve/exchange
 * collectively and in the same order. */
int rio_gp_shard_p2p_export(rio_gp_t* h, uint32_t n_ranks, void* out_handle64);
int rio_gp_shard_p2p_connect(rio_gp_t* h, uint32_t rank, uint32_t n_ranks, const void* handles /* [n_ranks][64] */);
int rio_gp_shard_p2p_ready(rio_gp_t* h);
/* Unmap the peers' windows and free ours (e.g. to fall back to RCCL after a time-out). */
int rio_gp_shard_p2p_close(rio_gp_t* h);

/* One COMMITTED tick of the row-sharded table with nothing waiting on the host (peer-to-peer windows only; the sharded twin
 * of rio_gp_tick_async): the scan and the one-launch exchange, then the whole fix-up chain — exact cut on this rank, Y
 * record out, everyone's in, one water-fill round per spill round, each followed by its exchange — every step guarded on the
 * device, so a tick that needs none of it pays a handful of short launches, and the publication (two pointer swaps).  The
 * result is what the synchronous sequence above computes.  All ranks must enqueue the same ticks in the same order; at most
 * 64 may be in flight.  rio_gp_shard_tick_wait waits for them and returns the records of the last `cap` (oldest first),
 * *n_out = how many had been enqueued: this rank's counters (sum them over the ranks) and the global verdict of each tick. */
typedef struct rio_gp_shard_tick_info {
    rio_gp_stats local;   /* this rank's rows (cut_nodes / slow_path / rounds_run of it: the global values below) */
    uint64_t cut_nodes;   /* global */
    uint64_t spill_rows;  /* global: rows that went to the water-fill before any cut */
    uint32_t slow_path;   /* the tick needed the fix-up (on any rank) */
    uint32_t rounds_run;  /* water-fill rounds that had rows pending */
} rio_gp_shard_tick_info;
int rio_gp_shard_tick_async(rio_gp_t* h);
int rio_gp_shard_tick_wait(rio_gp_t* h, rio_gp_shard_tick_info* out, uint32_t cap, uint32_t* n_out);

/* Optional: let the library issue the all-gathers itself through RCCL (resolved at run time with dlopen — the
 * copy already in the process, else librccl.so.1; `rccl_path` may name one, NULL = default search).  The host only
 * moves the 128-byte ncclUniqueId from rank 0 to the other ranks over its own control channel:
 *   rank 0: rio_gp_shard_comm_unique_id(id);  all ranks: rio_gp_shard_comm_init(h, rank, n_ranks, id).
 * rio_gp_shard_solve_async = scan -> all-gather X -> resolve in ONE call, the exchange on a second stream so that
 * back-to-back independent solves overlap it with the next scan; follow with rio_gp_shard_verdict / _finish (or the
 * fix-up calls, using rio_gp_shard_exchange for the Y records) exactly as above. */
int rio_gp_shard_comm_unique_id(void* out128, const char* rccl_path);
int rio_gp_shard_comm_init(rio_gp_t* h, uint32_t rank, uint32_t n_ranks, const void* id128, const char* rccl_path);
uint32_t rio_gp_shard_comm_ranks(rio_gp_t* h);
int rio_gp_shard_solve_async(rio_gp_t* h);
int rio_gp_shard_exchange(rio_gp_t* h, const uint64_t* d_in, uint64_t* d_out, uint64_t words_per_rank);

/* ---- row-sharded rebalance --------------------------------------------------------------- */
/*
 * rio_gp_rebalance of the CONCATENATED table (DESIGN.md section 2 rule 6 is stated over it), computed by the ranks of the
 * row-sharded solve: rank r owns the rows [off_r, off_r + n_r), the node table, the targets and liveness are replicated, cfg is
 * the same on every rank (max_moves and moves_cap are GLOBAL).  As above the library never talks to a peer: the caller
 * all-gathers one small record between the steps, and every rank calls the same steps in the same order.  All reductions are
 * integer sums in rank order, so the column, `used`, the counters and the moves equal the single-handle call's bit for bit.
 *
 *   begin -> [all-gather X] -> cut -> nodes_over == 0 ? finish
 *         :  [all-gather S] -> select -> selected_total == 0 ? finish
 *         :  [all-gather Y] -> merge -> { fill(round) -> [all-gather Y] -> merge } while rows are pending and round < rounds
 *         -> finish
 *
 *   X (rio_gp_shard_words1 = 2m+8 u64): pinned load[m] | candidate load[m] of this rank's rows | 8 words (unused)
 *   S (rio_gp_shard_words2 =  m+2 u64): this rank's surplus rows | their load | m words (zero)
 *   Y (rio_gp_shard_words2) after select: used'_r[m] (the load of this rank's rows that are not selected) | selected load |
 *       selected rows;  after fill: load admitted this round[m] | load still pending | rows still pending (the last round's
 *       record also carries, per node, the load of the rows that found no node and keep theirs: R4)
 *
 *   R1 on rank r cuts the candidates of node j against free_j - (candidate load of j on ranks < r), free_j = T[j] -sat the pinned
 *   load of all ranks; where the lower ranks' candidates alone exceed free_j every candidate of j on rank r is surplus, the
 *   zero-load ones included.  R2: rank r selects its first clamp(B - surplus rows of ranks < r, 0, its own) surplus rows.  R3:
 *   every round is one water-fill round over this rank's selected rows whose prefix starts at the pending load of the ranks
 *   < r; `used` is rebuilt from the summed records between rounds.
 *
 * The load-ordered cut (cfg->order = RIO_GP_REBALANCE_BY_LOAD, rule R1') is started with rio_gp_shard_rebalance_begin_ordered.
 * A node's threshold tau_j depends on its candidates on every rank, so R1 becomes a radix selection whose histograms are summed
 * over the ranks; R0, R2, R3 and R4 are as above:
 *
 *   begin_ordered -> [all-gather X] -> cut -> nodes_over == 0 ? finish
 *         :  threshold_plan -> { threshold_hist(p) -> [all-gather H] -> threshold_pick(p) } for p = 0 .. passes - 1
 *         -> [all-gather S] -> select -> ... as above
 *
 *   H (`words` u64 of rio_gp_shard_rebalance_threshold_plan): per over node, in ascending node order on every rank, the load of
 *       this rank's candidates by the digit of the pass, among those that agree with the digits chosen so far.  words =
 *       (nodes over) << (digit bits) <= rio_gp_shard_words1: the digit (11 bits at most) is narrowed until the record is no
 *       longer than X, so whatever carries X carries H (a window row of rio_gp_shard_exchange included).  The digits are those
 *       of ceil(32 / digit bits) passes from bit 32 down; the passes whose digit lies wholly above the largest load are not run.
 *       For that, word 2m of X (the first of the eight) carries, in a load-ordered session, the largest load among this rank's
 *       object rows on a node < m (0 without one; the row-order protocol leaves the word 0).  Digit, passes and words follow
 *       from the gathered X alone: every rank derives the same plan.
 *
 *   R1' on rank r: every globally over node is searched on every rank (a rank without a candidate of it, or without rows, adds
 *   zeros).  The pick sums the gathered histograms in rank order and takes the first digit whose inclusive sum passes what is
 *   left of the GLOBAL free_j.  After the last pass the bin of tau_j in rank q's histogram is tau_j * ties_q[j], and with c_j =
 *   floor(what is left / tau_j) rank r keeps its first clamp(c_j - ties of the ranks < r, 0, ties_r[j]) candidates of load tau_j
 *   in row order; its other candidates of that load and every heavier one are surplus, every lighter one (the zero-load ones
 *   included, on every rank) is kept.
 *
 * Handle state changes as in rio_gp_rebalance (joins rio_gp_tick_async work, drops an uncommitted solve, counts as a change of
 * the inputs); `used` is the GLOBAL one of the new column on every rank after finish.  RIO_GP_EINVAL, nothing changed: bad cfg /
 * struct_size, rounds > 8, rank >= n_ranks, moves_cap without list_moves, rio_gp_shard_tick_async ticks in flight, a step
 * called out of order (a threshold pass out of order, threshold_* in a row-order session and select before the last pick of a
 * load-ordered one included), or cfg->order != RIO_GP_REBALANCE_ROW_ORDER in rio_gp_shard_rebalance_begin.  begin and
 * begin_ordered may be called at any step: they start over.  Between begin and finish the handle belongs to the
 * protocol: a call that changes an input of the solve (nodes, liveness, objects, CRUD, a solve, a tick, rio_gp_rebalance) or
 * reads `used` (rio_gp_get_nodes) ends it, and the next step answers RIO_GP_EINVAL (the column is written by finish alone, so it
 * is as it was).  d_* are DEVICE pointers owned by the caller.
 */
/* R0 over this rank's rows; d_x[words1] = X.  list_moves != 0: finish lists the moves and B = min(max_moves, moves_cap);
 * *rounds_out (may be NULL) = the rounds that will run at most (cfg->rounds, 0 = the handle's spill_rounds).  Asynchronous. */
int rio_gp_shard_rebalance_begin(rio_gp_t* h, const rio_gp_rebalance_cfg* cfg, uint32_t rank, uint32_t n_ranks, int list_moves,
                                 uint64_t moves_cap, uint64_t* d_x, uint32_t* rounds_out);
/* rio_gp_shard_rebalance_begin that also takes cfg->order = RIO_GP_REBALANCE_BY_LOAD; with RIO_GP_REBALANCE_ROW_ORDER it is
 * rio_gp_shard_rebalance_begin itself. */
int rio_gp_shard_rebalance_begin_ordered(rio_gp_t* h, const rio_gp_rebalance_cfg* cfg, uint32_t rank, uint32_t n_ranks,
                                         int list_moves, uint64_t moves_cap, uint64_t* d_x, uint32_t* rounds_out);
/* d_xg[n_ranks][words1] gathered -> the global `used`, the cuts that fall on this rank, its surplus; d_s[words2] = S.
 * *nodes_over = live nodes holding more candidate load than free_j, on all ranks: 0 ends the protocol (finish).  In a
 * load-ordered session the surplus is not known yet: d_s is zeroed, and with nodes over the threshold passes come next. */
int rio_gp_shard_rebalance_cut(rio_gp_t* h, const uint64_t* d_xg, uint64_t* d_s, uint32_t* nodes_over);
/* Load-ordered sessions, after cut reported nodes over: the number of threshold passes and the u64 words of one rank's
 * histogram record (the same on every rank; words <= rio_gp_shard_words1). */
int rio_gp_shard_rebalance_threshold_plan(rio_gp_t* h, uint32_t* passes, uint64_t* words);
/* Pass `pass` (0, 1, ... in order): d_h[words] = this rank's histogram.  Asynchronous. */
int rio_gp_shard_rebalance_threshold_hist(rio_gp_t* h, uint32_t pass, uint64_t* d_h);
/* d_hg[n_ranks][words] = the gathered histograms of `pass` -> its digit of every threshold.  The last pass also places this
 * rank's cuts and writes d_s[words2] = S as cut does in a row-order session (d_s may be NULL on the earlier passes).
 * Asynchronous. */
int rio_gp_shard_rebalance_threshold_pick(rio_gp_t* h, uint32_t pass, const uint64_t* d_hg, uint64_t* d_s);
/* d_sg[n_ranks][words2] gathered -> R2, the selected rows packed; d_y[words2] = Y.  *selected_local sizes the move arrays of
 * finish; *selected_total = min(B, surplus rows of all ranks): 0 ends the protocol (finish). */
int rio_gp_shard_rebalance_select(rio_gp_t* h, const uint64_t* d_sg, uint64_t* d_y, uint64_t* selected_local,
                                  uint64_t* selected_total);
/* d_yg[n_ranks][words2] gathered -> the global `used`, this rank's prefix base; the rows / load pending on all ranks. */
int rio_gp_shard_rebalance_merge(rio_gp_t* h, const uint64_t* d_yg, uint64_t* pending_rows, uint64_t* pending_load);
/* Round `round` (0, 1, ... in order, while rows are pending and round < rounds) over this rank's selected rows; d_y = Y. */
int rio_gp_shard_rebalance_fill(rio_gp_t* h, uint32_t round, uint64_t* d_y);
/* R4, this rank's part of the column, its moves (HOST arrays of moves_cap >= *selected_local entries, given iff list_moves):
 * ascending, with rank-LOCAL row numbers; add off_r and concatenate in rank order.  local_stats: surplus_*, selected_*, moved_*
 * and stayed_rows of this rank's rows (sum them over the ranks); nodes_over_before / _after are global. */
int rio_gp_shard_rebalance_finish(rio_gp_t* h, rio_gp_rebalance_stats* local_stats, uint32_t* out_rows, uint32_t* out_from,
                                  uint32_t* out_to, uint64_t moves_cap, uint64_t* n_moves);

/* ---- measurement hooks (HIP events on the handle's own stream) -------------------------- */
int rio_gp_timer_begin(rio_gp_t* h);
/* rio_gp_timer_stop records the closing event behind the work enqueued so far and returns at once; rio_gp_timer_end waits
 * for the closing event (recording it first when nobody has) and reports the milliseconds between the two. */
int rio_gp_timer_stop(rio_gp_t* h);
int rio_gp_timer_end(rio_gp_t* h, float* ms);
/* One fast-path solve with a HIP-event pair around EACH kernel launch (so the durations are
 * per-launch, not host-paired): scan_ms = the streaming kernel k_scan (16 algorithmic B/row),
 * resolve_ms = k_resolve.  Does not publish; fails with RIO_GP_EINVAL if the solve needs the
 * cut/spill fix-up (use rio_gp_solve then). */
int rio_gp_solve_profiled(rio_gp_t* h, float* scan_ms, float* resolve_ms);
/* A/B knobs, phase traces and the streaming probes are not part of the boundary: rio_gpu_placement_debug.h. */

#ifdef __cplusplus
}
#endif
#endif /* RIO_GPU_PLACEMENT_H */
