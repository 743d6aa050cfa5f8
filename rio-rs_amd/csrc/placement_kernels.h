// placement_kernels.h — launch interface between the C ABI (rio_gp_capi.hip) and the gfx950
// kernels (placement_kernels.hip).  Internal; the public boundary is include/rio_gpu_placement.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace riogp {

typedef uint32_t u32;
typedef unsigned long long u64;

constexpr u32 kNone = 0xFFFFFFFFu;       // unplaced (RIO_GP_NONE)
constexpr u32 kSpillMark = 0xFFFFFFFEu;  // pending, waiting for the water-fill (never survives a solve)
constexpr u32 kSkipMark = 0xFFFFFFFDu;   // virtual-table row that is a duplicate request (place_pending)
constexpr u32 kAffInactive = 0xFFFFFFFEu;  // AFFINITY of a row that is not an object (RIO_GP_AFF_INACTIVE): never placed
constexpr u32 kFlagReplaced = 0x10u;  // RIO_GP_FLAG_REPLACED (rio_gpu_placement.h)
constexpr u32 kNoCut = 0xFFFFFFFFu;

constexpr int kWaves = 16;           // waves per workgroup of the streaming kernels
constexpr int kBlock = kWaves * 64;  // 1024 threads: ONE workgroup per CU owns one LDS histogram
constexpr int kTile = 256;           // objects per wave-iteration: 64 lanes x dwordx4
constexpr u32 kMaxBlocks = 256;      // = CUs; rows of the per-block histogram table
constexpr u32 kMaxSubs = 256;
constexpr int kMidBatch = 16384;     // lookups of up to this many entries go through mapped pinned memory and a completion word
constexpr int kReqBatch = 131072;    // place_pending batches from host buffers of up to this many requests: mapped pinned memory the kernels
                                     // read and write over PCIe themselves; bigger ones: the caller's arrays registered for the call, DMA copies
                                     // (measured per size, profiles/round6_pp_sizes.txt: 65 536 requests 125 us through the pinned rows against
                                     //  137-182 through registered arrays; 262 143: 398 against 249-373)
constexpr int kSmallBatch = 256;     // place_pending / lookup micro-batches served by one workgroup and one launch        // sub-chunks per block for the exact-cut refinement

// Work decomposition of a table of n rows.  Index order is the only order that matters:
// the table is `tiles` tiles of kTile rows; wave `gw` (of nw = G*kWaves) owns the contiguous tiles
// [gw*tiles/nw, (gw+1)*tiles/nw) (balanced to +-1 tile), block b owns kWaves consecutive wave
// ranges, sub-chunk t of block b is [block_row_lo(b) + t*sub, +sub).
struct Plan {
    u64 n;       // rows
    u64 tiles;   // ceil(n / kTile)
    u64 tq;      // tiles / nw   } the balanced split without a division on the device
    u64 div_magic;  // ceil(2^38 / nw)
    u32 tr;      // tiles % nw
    u32 nw;      // wave ranges = G * kWaves
    u32 G;       // blocks (<= kMaxBlocks)
    u32 sub;     // rows per sub-chunk (multiple of kTile)
    u32 subs;    // sub-chunks per block (<= kMaxSubs)
    u32 m;       // nodes
    u32 mwords;  // ceil(m/32)
    u32 trace;   // lab build: phase traces of the fix-up kernels (0 in the product)
    u32 sa;      // RIO_GP_CFG_REF_SELF_ASSIGN: a pending row claims its affinity node (a request: its requester) whether or not
                 // membership marks that node active, against the node's whole capacity (service.rs:244-252 self-assigns
                 // unconditionally); the water-fill still places on live nodes only.  0: a claim needs a live node
    u64 mark;    // what k_resolve stores in column 7 of its partial rows ("row present"): 1, or the sequence number the
                 // host spins on instead of waiting for the stream
    // packed fix-up (see PackOut): when set, wave gw's rows are only the first wcnt[gw] positions of its range
    const u32* wcnt;
    // k_scan only (launch_scan sets it from NodeTab::alive_src): the liveness bitmap the kernel was given is a fresh one in
    // mapped host memory; workgroup 0 copies it here, the device array the kernels behind the scan read
    u32* alive_dst;
};
Plan make_plan(u64 n, u32 m, u32 max_blocks);
u64 plan_wave_row_lo(u64 n, u32 m, u32 gw, u32* nw_out);  // first row of wave range gw, as the device computes it (debug / tests)

// Accumulators of one solve, device resident (all 64-bit so they can be atomically added).
struct DevStats {
    u64 kept, evicted, claimants, spillcand;            // k_scan   (rows)
    u64 load_kept, load_claim_tot, n_cut;               // k_resolve
    u64 rejected, load_rejected;                        // k_apply_cut
    u64 spilled, load_spilled, unplaced, load_unplaced; // k_spill_apply
    u64 rounds_run;                                     // k_spill_rank
    u64 evicted_clean;                                  // k_clean
    u64 err;                                            // invalid entries seen by batch kernels
    u64 local_fixup;                                    // row-sharded solve: nodes whose claimants of THIS rank need re-marking (k_resolve_xchg)
    u64 global_slow;                                    // row-sharded solve: != 0 iff the solve needs the fix-up on ANY rank (the same
                                                        // value on every rank: it is computed from the all-gathered sums)
};

// Per-workgroup rows of the fix-up counters (a whole-table solve whose counters the host wants): workgroup b of the
// streaming grid owns row b of `dev` across the kernels of one solve — k_scan zeroes it, the cut pass and every water-fill
// round add to it with plain stores, and each round also stores the row into `host` (pinned, mapped): the host folds the
// rows when it reads the verdict.  No contended atomics on eight global words (a 255-to-1 fan-in is ~3 us at the tail of
// three kernels per tick) and no copy kernel for the totals.  Both nullptr: the kernels add into DevStats atomically
// (row-sharded solve, place_pending).
// row = { rejected rows, rejected load, spilled rows, spilled load, unplaced rows, unplaced load, rounds run (row 0), - }
struct FxRows {
    u64* dev = nullptr;   // [kMaxBlocks][8]
    u64* host = nullptr;  // [kMaxBlocks][8], device address of pinned host memory
    u64 seq = 0;          // != 0: the LAST water-fill round stores it in word 7 of every row (also when the round is a
                          // no-op): the host spins on the pinned rows instead of waiting for the stream
};

// Scratch of one solve over one table (real table or the virtual table of place_pending).
struct SolveBufs {
    u64* H;          // [ceil(m/8)][G][16] per-block load histograms, node-group major: kept-by-cur x8 | claim-by-aff x8
                     //   (one 128-byte line per (group of 8 nodes, block): k_resolve reads G contiguous lines per workgroup)
    u64* partial;    // [ceil(m/8)][8] k_resolve per-workgroup partial counters (device copy)
    u64* blkstat;    // [G][4]   kept, evicted, claimants rows per block
    u64* wsp_sum[2]; // [G*kWaves] spill-candidate load per wave range (ping-pong over rounds)
    u32* wsp_cnt[2]; // [G*kWaves]
    u64* bsp_sum[2]; // [G] the same per workgroup (what k_spill_apply's prologue folds: G words instead of G*kWaves)
    u32* bsp_cnt[2]; // [G]
    u64* used_kept;  // [m] load of kept rows (+ used_base for the virtual table)
    u64* used_cur;   // [m] used_kept + admitted claims + admitted spills
    u64* claim_tot;  // [m]
    u32* cutblk;     // [m] block containing the cut or kNoCut
    u64* budget;     // [m] free capacity left at the start of the cut block
    u64* admpre;     // [m] claim load admitted before the cut block
    u32* cutidx;     // [m] row index of the first rejected claimant or kNoCut
    // row-sharded solve only (nullptr otherwise): nodes whose claim prefix overflowed on a lower rank, and the
    // spill load pending on lower ranks
    u32* forced_bits;        // [mwords]
    u64* rank_base;          // [1]
    const u64* pending_global;  // [1] rows still pending on ALL ranks (k_shard_import_delta), nullptr = local count
    const u64* run_if = nullptr;  // the re-marking pass (k_fill<APPLY> without FILL) returns at once when *run_if == 0
                                  // (asynchronous row-sharded tick: DevStats::local_fixup; nullptr = always run)
    // The claim load the cuts reject, for the ordered spill prefix of k_fill's round 0 (no pass over rows):
    u64* RP;         // [node groups][G] by node group, in the blocks BEFORE block b: k_scan zeroes, a k_resolve workgroup that owns
                     //   cut nodes stores its row (plain stores, whole lines); nullptr: not maintained
    u64* R;          // [G] correction of the cut blocks themselves (what a cut block admits of its nodes), as a negative
                     //   number: k_scan zeroes, k_cut_find adds (k_resolve<SEARCH> folds it into RP instead)
    u64* D;          // [kFillRounds][m] load admitted per water-fill round, kept apart from used_cur so that no round reads
                     //   and writes the same vector: k_resolve zeroes it, round r of k_fill orders the nodes by
                     //   used_cur + D[0..r) and adds into D[r]; the committed `used` is used_cur + sum D (launch_used_fold).
                     //   nullptr (row-sharded solve): the rounds read used_snap and add straight into used_cur
    const u64* used_snap;  // row-sharded solve: the global `used` vector as the last exchange left it (nobody writes it during a round)
    u64* Tg = nullptr;     // [m][16] k_cut_apply's per-wave claim sums of the undecided rows: k_resolve zeroes the rows of the nodes
                           //   it finds a cut for (nullptr: the solve's fix-up does not use k_cut_apply)
    DevStats* stats;
    FxRows fx;
};
constexpr u32 kFillRounds = 8;  // rows of SolveBufs::D = the largest number of water-fill rounds per solve

// Packed pending rows (k_scan<COMPACT>): wave gw copies its PENDING rows, in index order, to the front of its own
// row range in these scratch columns and records how many (wcnt[gw]).  The fix-up kernels then run unchanged over
// {cur = an all-NONE column, load, aff, next} with Plan::wcnt set, so their passes cost O(pending rows) instead of
// O(rows); k_pk_scatter writes the decisions back through `idx`.  Index order is preserved: (wave, packed position).
struct PackOut {
    u32* idx;
    u32* load;
    u32* aff;
    u32* next;
    u32* wcnt;  // [G*kWaves]
};

// table columns; for the real table cur/next are the ping-pong assignment columns
struct Table {
    const u32* cur;
    const u32* load;
    const u32* aff;
    u32* next;
    // packed fix-up only (else nullptr): the water-fill also writes each decision to real_next[pk_idx[position]],
    // which makes the separate k_pk_scatter launch unnecessary when at least one spill round runs
    const u32* pk_idx = nullptr;
    u32* real_next = nullptr;
    // the packing pass has already stored NONE into the real row of every packed row (k_cut_apply_rank<PACK>): the last
    // round then writes only the rows it places, not one scattered NONE per row it could not place
    bool none_prewritten = false;
    // virtual table of a window-sorted request batch (k_pp_win_gather): its rows arrive as 8-byte answer records {node | flag |
    // later, load} — the scan reads them and leaves cur / load as columns for the kernels behind it — and the alive requesters' first touches
    // are already in the real column (the scan stores only those whose requester is not alive: RIO_GP_CFG_REF_SELF_ASSIGN)
    const uint2* vrec = nullptr;
    bool prewritten = false;
    // plain virtual table (general request path): when *skip_if != 0 the batch held an invalid entry and the table was not
    // built — the scan solves an empty one
    const u32* skip_if = nullptr;
};

struct NodeTab {
    const u64* cap;         // [m]
    const u32* alive_bits;  // [mwords]
    const u64* used_base;   // [m] or nullptr (virtual table: the committed `used`)
    // A liveness push that has not reached alive_bits yet (else nullptr): the bitmap in mapped pinned host memory.  The
    // scan of the next solve reads it from there and brings alive_bits up to date on its way — the push costs no launch.
    const u32* alive_src = nullptr;
};

// Chained quiet ticks (rio_gp_tick_async over a table nothing has changed in): the scans of consecutive ticks alternate between
// two streams and hand their rows over wave range by wave range — wave range w of tick k + 1 reads what wave range w of tick k
// wrote (and writes what it read), so it waits for THAT wave's flag instead of for the whole launch; the ramp-down of
// one scan and the ramp-up of the next overlap.  flags[w] = `set` of the last chained scan whose wave range w is through.
// The chained scan is the whole tick: no claim can occur and kept rows are never cut, so every workgroup adds its kept loads
// into the tick's `used` buffer and stores its own verdict row (no k_resolve behind it).  The buffers rotate through a ring of
// four: link k adds into buffer k and zeroes buffer k + 2, which link k - 2 — finished before link k started, on the same
// stream — added into last; the host zeroes the first two links' buffers in front of the run.
constexpr u32 kChainReps = 16;  // replicas of a chained tick's `used` buffer (8, 16 and 32 measured within 0.5 us per tick)
struct ScanChain {
    u32* flags = nullptr;   // [kMaxBlocks * kWaves] one per wave range; device memory
    u32* err = nullptr;     // one word of mapped host memory: raised when a wait gave up (the tables are then stale)
    u32 wait = 0;     // sequence number of the scan to wait for (0: none — the stream orders this scan behind what it depends on)
    u32 set = 0;      // this scan's sequence number
    u64* used = nullptr;       // [kChainReps][m] this tick's `used` as replicas (zero before the first add): workgroup b adds into
                               // replica b % kChainReps, the committed vector is their sum (the host folds replicas 1.. into replica 0 later)
    u64* used_zero = nullptr;  // [kChainReps][m] the buffer of the link two ahead: each workgroup zeroes its slice
    u64* rows = nullptr;       // [G][8] pinned verdict rows, word 7 = Plan::mark: {load_kept, 0, 0, kept, evicted, claimants,
                               // spill candidates + claimants (rows the tick cannot settle), mark}
};

bool scan_chain_fits(u32 m);  // two workgroups of the chained scan per CU (what makes the in-kernel wait deadlock-free)

// --- solve pipeline ---
void launch_scan(const Plan& p, const Table& t, const NodeTab& nt, const SolveBufs& b, bool virt, bool all_alive,
                 hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr, const PackOut* pack = nullptr,
                 const ScanChain* chain = nullptr);
// host_partial: pinned host rows [resolve_blocks(m)][8] = load_kept, load_claim_tot, n_cut, kept, evicted,
// claimants, spillcand, present — the caller adds the rows up (no atomics / copy kernel on the stream).
// search (with p.wcnt set): the packed pending rows — k_resolve also finds the exact cut rows (no k_cut_find launch).
// fold_into: the committed `used` vector still waiting for the D rows of the previous committed solve (folded in before
// b.D is zeroed), fold_rounds = that solve's rounds.
// kept_from: the scan built no kept histogram (launch_inc_scan) — the kept load of a node is the committed vector's entry
// where the node is alive (read after the fold when it is fold_into itself).
// fold_from: where those rows are (nullptr: b.D).
void launch_resolve(const Plan& p, const NodeTab& nt, const SolveBufs& b, u64* host_partial, hipStream_t s,
                    hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr, const PackOut* search = nullptr,
                    u64* fold_into = nullptr, u32 fold_rounds = 0, const u64* kept_from = nullptr, const u64* fold_from = nullptr);
// The scan of a COMMITTED tick over a mostly-placed table (k_inc_scan): cur / load / aff are streamed like k_scan does, the
// assignment column is updated in place and only where a row's value changes, no histogram is built; the pending rows ->
// pack (per wave range of p).  launch_rebal deals them out evenly over rebal_plan(p) into `dst` and builds the fix-up's
// per-block histograms and spill totals there.
bool inc_scan_fits(u32 m);
void launch_inc_scan(const Plan& p, u32* assign, const u32* load, const u32* aff, const NodeTab& nt, const SolveBufs& b,
                     const PackOut& pack, hipStream_t s);
Plan rebal_plan(const Plan& p);
u64 rebal_rows(u64 n);  // rows of the balanced columns for a table of n rows (+ the usual padding)
void launch_rebal(const Plan& p, const Plan& pv, const PackOut& src, const NodeTab& nt, const PackOut& dst, const SolveBufs& b,
                  hipStream_t s);
unsigned resolve_blocks(u32 m);
void set_scan_nt(int mode);  // 0 by table size | 1 always | 2 never: non-temporal column streams in k_scan
// The exact cut search as a launch of its own (k_cut_find; guards itself on the device).  have_cutblk: launch_resolve of
// the same solve (same bufs) has already written cutblk / budget / admpre — else k_cutblk runs first (row-sharded path).
void launch_cut_find(const Plan& p, const Table& t, const NodeTab& nt, const SolveBufs& b, bool virt, hipStream_t s,
                     bool have_cutblk);
// One launch of k_fill: apply = re-mark the rejected claimants (+ pack: copy the rows that go on to the water-fill into the
// pack columns, per-wave counts in pack->wcnt; real table only), fill = one water-fill round.  apply && fill is round 0
// of a solve, fill alone a later round, apply alone the row-sharded solve's cut step.  The workgroups order the nodes
// themselves (by capacity class, in LDS): there is no ranking launch.
void launch_fill(const Plan& p, const Table& t, const NodeTab& nt, const SolveBufs& b, bool virt, bool apply, bool fill,
                 int round, bool last, hipStream_t s, const PackOut* pack = nullptr);
bool fill_can_pack(u32 m);
// k_cut_apply (real table of one GPU, whole-table solves): the exact cut search and the re-marking pass as ONE pass over the
// rows — replaces launch_cut_find + the apply half of round 0; the rounds behind it are launch_fill(apply = false) from round 0
// on, over pk (pack: Plan::wcnt = pk.wcnt, Table::none_prewritten) or over the table (pk is scratch for the undecided rows)
bool cut_apply_fits(u32 m);
void launch_cut_apply(const Plan& p, const Table& t, const NodeTab& nt, const SolveBufs& b, const PackOut& pk, const PackOut& ul,
                      u64* Tg, bool pack, bool all_alive, hipStream_t s);
// used[j] += D[0][j] + ... + D[rounds-1][j]
void launch_used_fold(u64* used, const u64* D, u32 m, u32 rounds, hipStream_t s);
#ifdef RIO_GP_LAB
int ktrace_enable(int on);
int ktrace_read(int table, u64* out /*[kMaxBlocks*8]*/);  // 0 k_resolve<search> | 1 k_fill round 0 | 2 k_fill later rounds
float sync_probe(int mode, int reps, hipStream_t s);  // host round-trip probes (stream_probe.hip)
float stream_probe(int mode, const u32* a, const u32* b, const u32* c, u32* o, u64 n, int reps, hipStream_t s,
                   hipEvent_t e0, hipEvent_t e1);
#endif

// --- CRUD over the assignment column ---
// the requests of a call of at most 4 entries, passed in the kernel arguments (a = object indices, b = nodes / requesters)
struct SmallInline { u32 a[4]; u32 b[4]; };
void launch_lookup_small(const u32* assign, u64 n_obj, const u32* idx, u32 n, u32* out, DevStats* st, hipStream_t s,
                         u32* done, u32 seq, const SmallInline* inl = nullptr);
// done / seq (lookup, update_small, remove, pp_small): when the call is ONE workgroup, its last act is to store seq into
// *done (mapped pinned memory) — the host spins on the word instead of waiting for the stream; nullptr = no word
void launch_lookup(const u32* assign, u64 n_obj, const u32* idx, u64 n, u32* out, DevStats* st, hipStream_t s,
                   u32* done = nullptr, u32 seq = 0, unsigned int* ticket = nullptr);  // ticket (device word, 0 between calls):
                   // several workgroups may share the completion word — the last one to finish stores it
// aff_life (every CRUD launcher below): the affinity column when the handle tracks the row lifecycle (rows that are
// written become objects, rows that are removed / deleted / dropped by clean_server stop being objects), else nullptr
// used / load != nullptr (medium batches): the per-node load vector follows the writes (a few global atomics)
void launch_update(u32* assign, u64 n_obj, u32 m, const u32* idx, const u32* node, u64 n, u32* pos_scratch,
                   DevStats* st, hipStream_t s, u32* aff_life = nullptr, unsigned int* ticket = nullptr, u32* done = nullptr,
                   u32 seq = 0, u64* used = nullptr, const u32* load = nullptr);
// n <= kSmallBatch validated entries (may be mapped host memory): last writer wins inside the batch, one launch
void launch_update_small(u32* assign, const u32* idx, const u32* node, u32 n, hipStream_t s, u32* aff_life = nullptr,
                         u32* done = nullptr, u32 seq = 0, const SmallInline* inl = nullptr, u64* used = nullptr,
                         const u32* load = nullptr, u32 m = 0);
// n <= kSmallBatch validated entries (may be mapped host memory / kernel arguments): one small workgroup
void launch_remove_small(u32* assign, u32 m, const u32* load, const u32* idx, u32 n, u64* used_or_null, hipStream_t s,
                         u32* aff_life, u32* done, u32 seq, const SmallInline* inl);
void launch_remove(u32* assign, u64 n_obj, u32 m, const u32* load, const u32* idx, u64 n, u64* used_or_null,
                   DevStats* st, hipStream_t s, u32* aff_life = nullptr, u32* done = nullptr, u32 seq = 0,
                   const SmallInline* inl = nullptr, unsigned int* ticket = nullptr);
// big random batches, partitioned by row window first (k_part_bin ...): part_applicable says whether a batch qualifies,
// scratch = part_scratch_words(n_obj, n) u32 words of device memory
bool part_applicable(u64 n_obj, u64 n, const void* idx, const void* node_or_null);
size_t part_scratch_words(u64 n_obj, u64 n);
// end of a synchronous call: the error counter (as 0 / 1) into a mapped host word, then the completion word (the host spins on it)
void launch_finish_err(const DevStats* st, u32* host_err, u32* done, u32 seq, hipStream_t s);
void set_part_shift(int shift);  // rows per window = 1 << shift, 12..14 (A/B runs)
void launch_update_part(u32* assign, u64 n_obj, u32 m, const u32* idx, const u32* node, u64 n, u32* scratch, DevStats* st,
                        hipStream_t s, u32* aff_life = nullptr);
void launch_remove_part(u32* assign, u64 n_obj, u32 m, const u32* load, const u32* idx, u64 n, u32* scratch,
                        u64* used_or_null, DevStats* st, hipStream_t s, u32* aff_life = nullptr);
// counter == nullptr: accumulate into st->evicted_clean.  ticket/host_out: self-resetting counter + total written to
// mapped host memory by the last workgroup (dead_bits may itself be mapped host memory).
void launch_clean(u32* assign, u64 n_obj, u32 m, const u32* dead_bits, u64* used_or_null, DevStats* st, hipStream_t s,
                  u64* counter = nullptr, unsigned int* ticket = nullptr, u64* host_out = nullptr, u32* aff_life = nullptr,
                  u32 seq = 0 /* != 0: *host_out = total | seq << 40, the word the host spins on */,
                  const u32* skip_if = nullptr /* asynchronous form: do nothing when *skip_if != 0 */);
void launch_recompute_used(const u32* assign, const u32* load, u64 n_obj, u32 m, u64* used, hipStream_t s);
void launch_fill_u32(u32* p, u64 n, u32 v, hipStream_t s);
void launch_set_attrs(u32* load, u32* aff, u64 n_obj, const u32* idx, const u32* nload, const u32* naff, u64 n,
                      DevStats* st, hipStream_t s);
void launch_count_placed(const u32* assign, u64 n_obj, DevStats* st, hipStream_t s);
void launch_pack_alive(const uint8_t* alive_bytes, u32 m, u32* alive_bits, hipStream_t s);
struct WordPack { u32 w[256]; };  // 8 192 bits = RIO_GP_MAX_NODES, passed by value as a kernel argument
void launch_store_words(const WordPack& pack, u32 nwords, u32* dst, hipStream_t s);

// --- place_pending, batches of up to kOneBatch requests: ONE workgroup, one launch; idx/req/out_* may be mapped host
//     memory; *status = 1 means "needs the general path", nothing was changed ---
constexpr int kOneBatch = 4096;
// stage + ticket (device memory: pp_stage_bytes() of scratch, one zeroed word): batches of more than kPpStagedFrom requests
// from HOST buffers (host_io; device-resident batches: more than 1 024) go through three launches — requests and their rows
// gathered by many workgroups, the decision in one, results and table stores by many again (k_pp_stage / k_pp_decide /
// k_pp_apply) — instead of one workgroup doing all of it
constexpr int kPpStagedFrom = 256;
inline size_t pp_stage_bytes() { return (size_t)kOneBatch * (16 + 16 + 8) + 64; }
// the update / remove / lookup parts of a mixed micro-batch (<= kSmallBatch validated entries each; *_inl: n <= 4 entries in
// the kernel arguments): run by the one workgroup of k_pp_one<kSmallBatch, 1> in front of the requests, or alone
struct CrudSmallArgs {
    u32 nu = 0, nr = 0, nl = 0;
    const u32 *u_idx = nullptr, *u_node = nullptr, *r_idx = nullptr, *l_idx = nullptr;
    u32* l_out = nullptr;
    const SmallInline *u_inl = nullptr, *r_inl = nullptr, *l_inl = nullptr;
    u64 n_obj = 0;
    DevStats* st = nullptr;
};
void launch_pp_one(u32* assign, const u32* load, u32 m, const u64* cap, const u32* alive_bits, u64* used,
                   const u32* idx, const u32* req, u32 n, u32* out_node, u32* out_flag, u32* status, hipStream_t s,
                   u32* aff_life = nullptr, u32* done = nullptr, u32 seq = 0, const SmallInline* inl = nullptr, u32 n_obj_chk = 0,
                   void* stage = nullptr, unsigned int* ticket = nullptr, u32 sa = 0, bool host_io = false,
                   const CrudSmallArgs* crud = nullptr);
void launch_crud_small(const CrudSmallArgs& c, u32* assign, const u32* load, u32 m, u64* used_or_null, u32* aff_life, u32* done,
                       u32 seq, hipStream_t s);
// --- place_pending, the general request path (k_ppm_first / k_ppm_gather / solve of the virtual table / k_ppm_output) ---
// bad: device word, 0 between calls (raised by k_ppm_first on an invalid entry, put back by k_ppm_output's last workgroup);
// s_idx / s_req: the library's padded device copies of the requests, written on the way (use THEM afterwards: idx / req may be
// mapped host memory, or a caller's exact-size device arrays the solve's tile-wide reads must not run past);
// dead_bits / vflag != nullptr: some node is not alive — nodes that requests run into are marked, REPLACED bits per request
void launch_ppm_first(const u32* assign, u64 n_obj, u32 m, const u32* alive_bits, const u32* idx, const u32* req, u64 n,
                      u32* pos_scratch, u32* s_idx, u32* s_req, u32* dead_bits, u32* vflag, u32* bad, hipStream_t s);
void launch_ppm_gather(const u32* assign, const u32* load, const u32* idx, u64 n, const u32* pos_scratch, u32* vcur, u32* vload,
                       u32* vfirst, const u32* bad, hipStream_t s);
// *status (mapped host memory): 0 done | 1 the solve needs the fix-up and it was not enqueued (fixup_done == false): nothing
// was changed, enqueue it and launch this again with fixup_done | 3 invalid entry: nothing was changed.  Ends with the
// several-workgroup completion word (ticket / done / seq).
void launch_ppm_output(u32* assign, u64 n_obj, const u32* idx, const u32* req, u64 n, const u32* vcur, const u32* vnext,
                       const u32* vfirst, const u32* vflag, u32* pos_scratch, const u32* alive_bits, const SolveBufs& b,
                       const Plan& vp, u32* out_node, u32* out_flag, u32* aff_life, u32* bad, bool fixup_done, u32* status,
                       unsigned int* ticket, u32* done, u32 seq, hipStream_t s);

// place_pending over a window-sorted batch (big batches): see k_pp_win_gather.  scratch = part_scratch_words(n_obj, n) words.
bool pp_win_applicable(u64 n_obj, u64 n, const void* idx, const void* req);
// claim_fast: [m + 1] u64 of device memory — the load the batch's first touches put on every requester + the count of requests
// the window kernel could not answer by itself; cleared by launch_pp_bin, filled by launch_pp_win_gather, judged by
// launch_pp_win_verdict (*verdict: 1 every answer is final, `used` has taken the claims | 2 the batch needs the solve over the
// records, nothing else was changed | 3 invalid entry), handed out by launch_pp_win_unsort
void launch_pp_bin(u64 n_obj, u32 m, const u32* idx, const u32* req, u64 n, u32* scratch, DevStats* st, u32* host_err, hipStream_t s,
                   u32* dead_bits, u64* claim_fast);  // (clears the two)
// ans0 / ans1: the answer records' two words, [n] each, in the SORTED order of launch_pp_bin's records (launch_pp_win_unsort
// carries them back to batch order: the caller's columns on verdict 1, vrec on verdict 2)
void launch_pp_win_gather(u32* assign, const u32* load, u64 n_obj, u32 m, const u32* alive_bits, u64 n, const u32* scratch,
                          u32* ans0, u32* ans1, u32* dead_bits, u32* aff_life, const DevStats* st, u64* claim_fast, hipStream_t s);
void launch_pp_win_unsort(u64 n_obj, const u32* scratch, const u32* ans0, const u32* ans1, u64 n, uint2* vrec, u32* out_node, u32* out_flag,
                          const u32* verdict, hipStream_t s);
void launch_pp_win_verdict(u32 m, const u64* cap, const u32* alive_bits, u64* used, const u64* claim_fast, const DevStats* st,
                           u32* verdict_dev, u32* verdict_host, hipStream_t s);
void launch_pp_win_output(const u32* idx, const u32* req, u64 n, const u32* vcur, const u32* vload, const u32* vnext,
                          const u32* alive_bits, const u32* cutidx, u32 m, u32* out_node, u32* out_flag, u32* aff_life,
                          const DevStats* st, hipStream_t s, u32 sa, const uint2* vrec);

size_t scan_lds_bytes(u32 m);

// --- row-sharded solve: records exchanged between ranks ---
inline size_t shard_words1(u32 m) { return 2 * (size_t)m + 8; }  // X = [kept_local[m] | claim_local[m] | 8 counters]
inline size_t shard_words2(u32 m) { return (size_t)m + 2; }      // Y = [delta[m] | spill load | spill rows]
void launch_shard_pack1(const Plan& p, const SolveBufs& b, u64* X, hipStream_t s);
// Xg[R][shard_words1(m)] = the all-gathered X records (RCCL paths)
void launch_shard_import(const Plan& p, const NodeTab& nt, const SolveBufs& b, const u64* Xg, u32 rank, u32 R,
                         u64* gprev, u64* gfinal, u64* verdict_dev, u64* verdict_host, hipStream_t s);
// peer-to-peer exchange over xGMI (windows IPC-mapped by every rank, R <= 32)
// the whole fast-path exchange in one launch (k_resolve_xchg): window rows of shard_xchg_words(m) words; host_partial =
// pinned rows [resolve_blocks(m)][8] of partial verdicts (the caller adds them up)
inline size_t shard_xchg_words(u32 m) { return 2 * (2 * (size_t)m + 8 * (size_t)((m + 7) / 8)); }  // two tagged words per value
void launch_resolve_xchg(const Plan& p, const NodeTab& nt, const SolveBufs& b, u64* const* d_peers, u32 R, u32 rank,
                         size_t my_row_off, const u64* win_rows, size_t W, u64 seq, u64* p2p_err, u64* gprev, u64* gfinal,
                         u64* host_partial, u32 co_resident, hipStream_t s);
void launch_p2p_put(const u64* src, u32 words, u64* const* d_peers, u32 R, size_t data_off, size_t flag_off, u64 seq,
                    hipStream_t s);
void launch_p2p_wait_copy(const u64* win_slot, size_t W, u32 R, u32 words, const u64* flags, u64 seq, u64* err, u64* out,
                          hipStream_t s);
void launch_shard_export_delta(const Plan& p, const SolveBufs& b, const u64* base, int wsp_sel, u64* Y, hipStream_t s);
// asynchronous row-sharded tick: one exchange of the fix-up record in two launches (export + put | wait + import), both
// no-ops — no store to a peer, no wait for one — when the solve needs no fix-up anywhere (DevStats::global_slow)
void launch_shard_export_put(const Plan& p, const SolveBufs& b, const u64* base, int wsp_sel, u64* const* d_peers, u32 R,
                             size_t data_off, size_t flag_off, u64 seq, hipStream_t s);
void launch_shard_wait_import(const Plan& p, const SolveBufs& b, const u64* win_slot, size_t W, const u64* flags, u64 seq,
                              u64* err, u32 rank, u32 R, u64* gprev, const u64* gfinal, u64* verdict_dev, u64* verdict_host,
                              hipStream_t s);
void launch_shard_tick_stats(const Plan& p, const SolveBufs& b, u64* out_host, u64 mark, hipStream_t s);
void launch_shard_import_delta(const Plan& p, const SolveBufs& b, const u64* Yg, u32 rank, u32 R, u64* gprev,
                               u64* verdict_dev, u64* verdict_host, hipStream_t s);

// --- reverse placement index (rio_gp_rows_on_nodes): count -> scan -> scatter, each pass its own launch ---
constexpr u32 kNiIdentity = 0, kNiSingle = 1, kNiMap = 2;  // node -> slot: every node selected | one node | map[node] (kNone: not)
constexpr int kNiMaxWaves = 8;                   // waves per workgroup of the count / scatter passes (NiPlan::W is 4 or 8)
constexpr u32 kNiChunk = 4096;                   // matrix entries per workgroup of the scan
constexpr u64 kNiMaxEntries = (u64)1 << 21;      // slots x tiles: the matrix is at most 8 MiB of u32
constexpr u64 kNiMaxTiles = 8192;
constexpr u32 kNiMaxParts = (u32)(kNiMaxEntries / kNiChunk);  // chunk sums (+ 1 word: the total)
struct NiPlan {
    u64 n;     // rows considered: 0 .. n-1
    u64 T;     // rows per tile (a multiple of 256; one tile per wave)
    u32 m;     // nodes
    u32 s;     // selected nodes = slots
    u32 mode;  // kNi*
    u32 node;  // kNiSingle: the one node
    u32 nt;    // tiles (<= kNiMaxEntries / s)
    u32 nb;    // bits of a slot id (0 .. 13): ballots per position to rank equal slots
    u32 cb;    // bytes per LDS counter of the count pass: 2 while T <= 65 535, else 4
    u32 W;     // waves per workgroup
};
NiPlan ni_plan(u64 n, u32 m, u32 s, u32 mode, u32 node, u32 force_tile /* 0: by size */);
// cnt: kNiMaxEntries u32; map: kNiMap only, m words in device memory
void launch_ni_count(const u32* assign, const NiPlan& p, const u32* map, u32* cnt, hipStream_t s);
// part: kNiMaxParts + 1 u32; rank: kNiMap only, m + 1 words in device memory; off: m + 1 u64 (device)
void launch_ni_scan(u32* cnt, const NiPlan& p, u32* part, const u32* rank, u64* off, hipStream_t s);
const u32* ni_total(const NiPlan& p, const u32* part);  // device word: rows listed
// nothing is written when *ni_total > cap
void launch_ni_scatter(const u32* assign, const NiPlan& p, const u32* map, const u32* cnt, const u32* part, u64 cap, u32* rows,
                       hipStream_t s);

// --- bounded rebalance (rio_gp_rebalance): shed the candidates beyond a node's target, water-fill them (kernels: k_shed_*) ---
constexpr u32 kShChunk = 4 * kBlock;          // rows (packed rows) per workgroup step: 1 024 lanes x 4
constexpr u64 kShMaxEntries = (u64)1 << 22;   // (over node x tile) matrix of candidate loads: at most 32 MiB of u64
constexpr int kShAccSurplusRows = 0, kShAccSurplusLoad = 1, kShAccSelectedLoad = 2, kShAccMovedRows = 3, kShAccMovedLoad = 4,
              kShAccStayed = 5, kShAcc = 8;  // device counters of one call (u64 [kShAcc])
struct ShPlan {
    u64 n;   // rows
    u64 T;   // rows per tile (a multiple of kShChunk; one workgroup per tile)
    u32 nt;  // tiles (s * nt <= kShMaxEntries)
    u32 m;   // nodes
    u32 s;   // over-target nodes = slots of the matrix
};
ShPlan sh_plan(u64 n, u32 m, u32 s);
size_t shed_order_lds(u32 m);
// `cls` in the launches of the table passes below (rule 13; nullptr = no immovable class, the kernels without the table): the
// class column and the immovable classes, one bit each.  With it a row of an immovable class counts as a pinned row in every
// pass (kernels k_shedc_*: the quad of K beside the three columns, the bits in kShClsLds more bytes of dynamic LDS).
struct ShCls {
    const unsigned char* K;  // the class column, readable in whole quads up to the rows rounded up to 4
    u32 imm[8];              // bit c: class c is immovable (8 x 32 = RIO_GP_MAX_CLASSES)
};
constexpr size_t kShClsLds = sizeof(ShCls::imm);
// used, pin: m u64 each (zeroed here): the load of every row on node j, the load of the non-object rows on it; maxl (may be
// nullptr): one u32 -> the largest load of an object row on a node < m
void launch_shed_hist(const u32* assign, const u32* load, const u32* aff, u64 n, u32 m, u64* used, u64* pin, hipStream_t s,
                      u32* maxl = nullptr, const ShCls* cls = nullptr);
// map: node -> slot (kNone: not over); slot_node / slot_free: per slot; mat: s * nt u64; cut: m u32 (kNone where nothing is cut).
// thr (m u32, or nullptr = row order) in the four launches below: the load-ordered cut's threshold per node (kNone on a node
// that is not over).  With it the cut walks only the candidates whose load == thr[node] — slot_free is then what
// launch_shed_select left — and a candidate is surplus iff load > thr[node] || (load == thr[node] && row >= cut[node]).
// fill_cut: cut starts as kNone on every node (false: k_shrb_import_x / k_shrb_import_slots wrote it).  No slot or no row: no pass.
void launch_shed_cut(const u32* assign, const u32* load, const u32* aff, const ShPlan& p, const u32* map, const u32* slot_node,
                     const u64* slot_free, u64* mat, u32* cut, const u32* thr, bool fill_cut, hipStream_t s,
                     const ShCls* cls = nullptr);
// tcnt: nt u32 -> the exclusive scan of the per-tile surplus counts; acc[kShAccSurplusRows / SurplusLoad]
void launch_shed_count(const u32* assign, const u32* load, const u32* aff, const ShPlan& p, const u32* cut, const u32* thr,
                       u32* tcnt, u64* acc, hipStream_t s, const ShCls* cls = nullptr);
// the first `budget` surplus rows into pk_* (row, load, node = kNone); used[j] -= their load; acc[kShAccSelectedLoad]
void launch_shed_pack(const u32* assign, const u32* load, const u32* aff, const ShPlan& p, const u32* cut, const u32* thr,
                      const u32* toff, u64 budget, u32* pk_row, u32* pk_load, u32* pk_node, u64* used, u64* acc, hipStream_t s,
                      const ShCls* cls = nullptr);
// The load-ordered cut (RIO_GP_REBALANCE_BY_LOAD; kernels: k_shed_sel_hist, k_shed_sel_pick): a segmented, weighted radix
// selection, most significant digit first.  Per over node (slot) it finds the smallest load tau whose candidates, together with
// every lighter one, weigh more than slot_free: thr[slot_node] = tau, slot_free[slot] -= the load of the candidates below tau.
// The digit is `bits` wide (the last one may be narrower); the histogram is s << bits u64.
constexpr u32 kShSelLdsBytes = 96 * 1024;        // LDS for a pass's histogram (k_shed_sel_hist<true>), beside the node map (4 B a
                                                 // node) and the slots' prefixes (4 B a slot): 141 KiB of the CU's 160 at most
constexpr u32 kShSelLdsSlots = kShSelLdsBytes / (4 * sizeof(u64));  // = 3 072: up to here a digit of >= 2 bits fits there
struct ShSelPlan {
    u32 bits;    // digit width
    u32 passes;  // ceil(32 / bits)
    bool lds;    // per-workgroup LDS histogram, flushed once (else: one global atomic per wave and distinct bin)
};
ShSelPlan sh_sel_plan(u32 s);
// pre: s u32 of scratch; hist: (s << bits) u64 of scratch; thr: m u32 (kNone where the node is not over)
void launch_shed_select(const u32* assign, const u32* load, const u32* aff, u64 n, u32 m, u32 s, const u32* map,
                        const u32* slot_node, u64* slot_free, u32* pre, u64* hist, u32* thr, hipStream_t st,
                        const ShCls* cls = nullptr);
// one water-fill round over the K packed rows against free = tgt -sat used; csum: ceil(K / kShChunk) u64; C: m + 1 u64; ord: m u32
void launch_shed_round(u64 K, const u32* pk_load, u32* pk_node, const u64* tgt, u32 m, u64* used, u64* csum, u64* C, u32* ord,
                       u32* cntp, hipStream_t s);
// R4 + the column + the move list (out_rows NULL: counts only); mc: ceil(K / kShChunk) u32
void launch_shed_finish(u64 K, const u32* pk_row, const u32* pk_load, const u32* pk_node, u32* assign, u64* used, u32* mc,
                        u64* acc, u32* out_rows, u32* out_from, u32* out_to, hipStream_t s);

// --- row-sharded rebalance (rio_gp_shard_rebalance_*): the k_shed_* passes over one rank's rows; k_shrb_* carry the rank offsets ---
constexpr int kShrbOver = 0, kShrbSlots = 1, kShrbForced = 2, kShrbOverBefore = 3, kShrbInfo = 4;  // u32 counters of k_shrb_import_x
constexpr int kShrbMaxLoad = kShrbInfo;  // one more word, written by k_shrb_import_slots alone: the largest load on any rank
struct ShrbImport {
    const u64* Xg;     // [R][2m + 8] gathered X records: pinned load | candidate load | counters
    u32 rank, R, m;
    const u64* T;      // [m] targets
    const u32* live;   // [m] 0 / 1
    u64* used;         // -> [m] global load per node
    u64* tgt;          // -> [m] T on live nodes, 0 elsewhere
    u32* map;          // -> [m] node -> slot where the cut falls on THIS rank (kNone elsewhere)
    u32* slot_node;    // -> per slot
    u64* slot_free;    // -> per slot: what the lower ranks' candidates left of free_j
    u32* cut;          // -> [m] 0 where the cut fell on a lower rank (every candidate here is surplus), kNone elsewhere; the
                       //    slots' nodes are filled in by k_shed_cut
    u32* info;         // -> [kShrbInfo] (k_shrb_import_slots: [kShrbInfo + 1])
};
// X = pin | used - pin | 8 words: *maxl (nullptr: 0), five zeros, 1 (as in the solve's record)
void launch_shrb_export_x(const u64* used, const u64* pin, u32 m, const u32* maxl, u64* X, hipStream_t s);
void launch_shrb_import_x(const ShrbImport& a, hipStream_t s);
// The load-ordered cut, sharded (kernels: k_shrb_import_slots, k_shed_sel_hist, k_shrb_sel_pick).  The slots are the globally
// over nodes in ascending node order, the same on every rank; the plan depends on (S, m) alone and its histogram record,
// S << bits u64, is never longer than an X record (shard_words1(m)): the digit is narrowed until it fits.
ShSelPlan shrb_sel_plan(u32 S, u32 m);
// the first pass of plan q that can pick a digit other than 0 when no load exceeds max_load (0: unknown, pass 0)
u32 shrb_sel_first_pass(const ShSelPlan& q, u32 max_load);
// launch_shrb_import_x for the load-ordered cut: info[kShrbSlots] = info[kShrbOver], info[kShrbMaxLoad] = the largest word 2m of
// the gathered X records, slot_free = the global free_j, pre[slot] = 0, cut = thr = kNone on every node
void launch_shrb_import_slots(const ShrbImport& a, u32* pre, u32* thr, hipStream_t s);
// H (S << bits u64, zeroed here) = this rank's histogram of pass `pass`
void launch_shrb_sel_hist(const u32* assign, const u32* load, const u32* aff, u64 n, u32 m, u32 S, const u32* map, const u32* pre,
                          const ShSelPlan& q, u32 pass, u64* H, hipStream_t s);
// Hg[R][S << bits] gathered -> the digit of every slot: pre, slot_free as launch_shed_select's passes leave them.  The last pass
// sets thr[slot_node] and turns slot_free into the load of the ties THIS rank keeps (launch_shed_cut with thr places the cut).
void launch_shrb_sel_pick(const u64* Hg, u32 rank, u32 R, u32 S, const ShSelPlan& q, u32 pass, const u32* slot_node,
                          u64* slot_free, u32* pre, u32* thr, hipStream_t s);
// Y = v[m] | *a | b
void launch_shrb_export_y(const u64* v, u32 m, const u64* a, u64 b, u64* Y, hipStream_t s);
// used = (first ? 0 : used) + sum of the gathered Y[q][0..m) in rank order; *base = sum of Y[q][m] over q < rank;
// pend[0] = rows, pend[1] = load pending on all ranks
void launch_shrb_merge(const u64* Yg, u32 rank, u32 R, u32 m, bool first, u64* used, u64* base, u64* pend, hipStream_t s);
// launch_shed_round with the prefix starting at *base and the admissions going into Y (zeroed here) instead of `used`: Y =
// admitted load[m] | load still pending | rows still pending.  last: the rows left without a node give their load back to their
// own node in Y (R4), so that the sum over the ranks is the `used` of the new column.
void launch_shrb_round(u64 K, const u32* pk_row, const u32* pk_load, u32* pk_node, const u32* assign, const u64* tgt, u32 m,
                       const u64* used, const u64* base, bool last, u64* csum, u64* C, u32* ord, u32* cntp, u64* Y, hipStream_t s);

// --- change feed (rio_gp_changes): count A != B per tile, then list the changed rows of the tiles that hold one ---
constexpr u32 kChgTile = 1024;       // rows per tile: one wave, four steps of 256 rows (lane l: rows 4l .. 4l+3 of a step)
constexpr u32 kChgWaves = 4;         // waves per workgroup; a workgroup owns `tpg` consecutive tiles, its waves take every 4th
constexpr u32 kChgMaxGroups = 2048;  // workgroups of a pass (k_chg_scan scans their sums)
constexpr u32 kChgMaxTpg = 1024;     // tiles per workgroup at RIO_GP_MAX_OBJECTS rows
struct ChgPlan {
    u64 n;    // rows compared: 0 .. n-1
    u32 nt;   // tiles
    u32 tpg;  // tiles per workgroup (a multiple of kChgWaves)
    u32 G;    // workgroups
};
ChgPlan chg_plan(u64 n);
// cnt: nt u32 (per-tile counts); gsum: kChgMaxGroups + 1 u32 -> the exclusive prefix of the workgroup sums, gsum[G] = total;
// total: a word of mapped pinned memory (the host reads it after the wait).  Two launches: the count pass, a one-workgroup scan.
void launch_chg_count(const u32* A, const u32* B, const ChgPlan& p, u32* cnt, u32* gsum, u32* total, hipStream_t s);
// the first `cap` changes as (row, B[row], A[row]); consume: B[row] := A[row] for the listed rows
void launch_chg_list(const u32* A, u32* B, const ChgPlan& p, const u32* cnt, const u32* gsum, u64 cap, bool consume, u32* rows,
                     u32* old_node, u32* new_node, hipStream_t s);

// --- node removal (rio_gp_remap_nodes): clean the removed nodes' rows and renumber the kept nodes, one pass (k_remap) ---
constexpr u32 kRemapMaxNodes = 8192;     // = RIO_GP_MAX_NODES: the map's LDS image
constexpr u32 kNodeGone = 0xFFFFFFFCu;   // RIO_GP_NODE_GONE: checkpoint of a row whose last-told node has been removed
// map: m u32 in device memory (new id, kNone = removed).  Rows 0 .. rows-1 of assign / aff / B (B may be nullptr) are rewritten
// where a value changes; life: a row that loses its node also becomes a non-object.  blk: [G][4] u64, workgroup b stores
// {0, rows < n_count it un-placed, 0, 0}; returns G.
u32 launch_remap(u32* assign, u32* aff, u32* B, u64 rows, u64 n_count, u32 m, const u32* map, bool life, u64* blk, hipStream_t s);

// --- idle expiry (rio_gp_touch_*, rio_gp_expire): a last-seen column S; the placed rows with S < cutoff are listed and un-placed ---
constexpr u32 kExpLdsNodes = 4096;  // node counts up to which k_exp_apply gathers the released load per workgroup in LDS (32 KiB)
// the feed's plan, per-tile counts, workgroup sums and mapped total word (launch_chg_count), with the idle predicate over
// (A, S, cutoff); *freed (device memory) is zeroed for launch_exp_apply
void launch_exp_count(const u32* A, const u32* S, const ChgPlan& p, u32 cutoff, u32* cnt, u32* gsum, u32* total, u64* freed,
                      hipStream_t s);
// the first `cap` idle rows as (row, A[row]); each of them: A[row] := kNone, aff_life[row] := kAffInactive (aff_life != nullptr),
// *freed += load[row], used[A[row]] -= load[row] (used != nullptr and A[row] < m)
void launch_exp_apply(u32* A, const u32* S, const ChgPlan& p, u32 cutoff, const u32* cnt, const u32* gsum, u64 cap, u32* rows,
                      u32* node, u32* aff_life, const u32* load, u32 m, u64* used, u64* freed, hipStream_t s);
// S[idx[k]] = max(S[idx[k]], epoch) for k < n; entries >= n_obj are skipped and counted in st->err
void launch_touch(u32* S, u64 n_obj, const u32* idx, u64 n, u32 epoch, DevStats* st, hipStream_t s);
// S[r] = max(S[r], stamps ? stamps[r] : epoch) for r < rows (S is padded: whole quads are read and written)
void launch_seen_merge(u32* S, const u32* stamps, u32 epoch, u64 rows, hipStream_t s);

// --- measured load (rio_gp_hits_*, rio_gp_load_fold): a hit column H; the fold turns hits into loads, `used` following ---
// H[idx[k]] = min(H[idx[k]] + (weight ? weight[k] : 1), 2^32-1) for k < n; entries >= n_obj are skipped and counted in st->err
void launch_hits_add(u32* H, u64 n_obj, const u32* idx, const u32* weight, u64 n, DevStats* st, hipStream_t s);
// H[r] = min(H[r] + counts[r], 2^32-1) for r < rows (H is padded: whole quads are read and written; counts: any alignment)
void launch_hits_merge(u32* H, const u32* counts, u64 rows, hipStream_t s);
// load[r] := clamp(floor(load[r] * keep / 65536) + H[r] * gain, lo, hi), H[r] := 0 for r < n; used != nullptr: used[A[r]] +=
// new - old for A[r] < m (LDS accumulators for m <= kExpLdsNodes); the pass ADDS into st (5 u64 of device memory, zeroed by the
// caller) = { rows changed, hits folded, load before, load after, largest load after }
void launch_load_fold(u32* load, u32* H, const u32* A, u64 n, u32 keep, u32 gain, u32 lo, u32 hi, u32 m, u64* used, u64* st,
                      hipStream_t s);

// --- hot-object report (rio_gp_top_rows): the first `cap` candidates by (K descending, row ascending), an exact radix select ---
constexpr u32 kTopMax = 4096;   // = RIO_GP_TOP_MAX: rows of one listing (their composites sort in 32 KiB of LDS)
constexpr u32 kTopBins = 2048;  // bins of one digit's histogram (11 / 11 / 10 bits from the top)
constexpr u32 kTopPlaced = 2u, kTopOnNode = 4u;  // = RIO_GP_TOP_PLACED / RIO_GP_TOP_ON_NODE (the key column is the caller's choice)
// The call's device state, one allocation.  Everything in front of `pairs` is zeroed by every call.
struct TopScratch {
    u64 n_cand, key_sum;                             // pass 0: the candidates and the sum of their keys
    u32 prefix, want, all, cursor, tie_total, pad[3];  // the digits chosen so far (at the end: T) / the rank left (at the end: t)
    u32 hist[3][kTopBins];
    u64 pairs[kTopMax];     // (K << 32) | ~row of the rows to list, unordered
    u64 hdr[2];             // what the host reads back: n_candidates, key_sum ...
    u32 out[3 * kTopMax];   // ... and, in the host-pointer form, rows | keys | nodes of `cap` entries each right behind them
};
constexpr u64 kTopZeroWords = 4 + 8 + 3 * (u64)kTopBins;
static_assert(kTopZeroWords * sizeof(u32) == offsetof(TopScratch, pairs), "TopScratch: the zeroed head ends where pairs begins");
// K: the key column (nullptr: every key is 0), A: the committed column; filt: kTopPlaced | kTopOnNode; cnt / gsum: the feed's
// per-tile counts and workgroup sums (launch_chg_count's).  rows / key: cap entries; nodes: cap entries or nullptr.  sc->hdr holds
// n_candidates and key_sum when the stream has run.
void launch_top_rows(const u32* K, const u32* A, u64 n, u32 min_key, u32 filt, u32 node, u32 cap, TopScratch* sc, u32* cnt,
                     u32* gsum, u32* rows, u32* key, u32* nodes, hipStream_t s);

// --- object classes (rio_gp_set_class*, rio_gp_expire_classes, rio_gp_census): a class column K, one byte per row ---
constexpr u32 kClsMax = 256;           // = RIO_GP_MAX_CLASSES: the cutoff table and the per-class histogram, 1 KiB of LDS each
static_assert(sizeof(ShCls::imm) * 8 == kClsMax, "rule 13: one bit per class");
constexpr u32 kClsSlots = 32;          // copies of the sweep's per-class counts the workgroups of k_expc_count spread their adds over
constexpr u32 kCensusLdsCells = 4096;  // cells one workgroup of k_census accumulates in LDS (12 B a cell: 48 KiB): one slice
constexpr u32 kCensusMaxSlices = 16;   // slices (passes over the columns) up to which the census stays in LDS; beyond: global adds
struct ClsCutoffs {
    u32 v[kClsMax];  // cutoff per class, 0 from n_classes on (a kernel argument: 1 KiB)
};
// K[idx[k]] = cls[k] for k < n, the last entry of a row wins; entries >= n_obj are skipped and counted in st->err.  pos: the
// handle's all-ones position scratch (launch_update's), all-ones again afterwards.  n < 2^32 - 1.
void launch_set_class_batch(unsigned char* K, u64 n_obj, const u32* idx, const unsigned char* cls, u64 n, u32* pos, DevStats* st,
                            hipStream_t s);
// launch_exp_count / launch_exp_apply with the idle predicate A[r] != kNone && S[r] < cutoffs.v[K[r]].  by_class: kClsSlots *
// kClsMax u64 of device memory, zero between the calls (the caller zeroes them once); host_by_class: kClsMax u64 of mapped pinned
// memory = the idle rows of every class when the stream has run
void launch_expc_count(const u32* A, const u32* S, const unsigned char* K, const ChgPlan& p, const ClsCutoffs& cutoffs, u32* cnt,
                       u32* gsum, u32* total, u64* by_class, u64* host_by_class, u64* freed, hipStream_t s);
void launch_expc_apply(u32* A, const u32* S, const unsigned char* K, const ChgPlan& p, const ClsCutoffs& cutoffs, const u32* cnt, const u32* gsum, u64 cap, u32* rows, u32* node, u32* aff_life, const u32* load, u32 m,
                       u64* used, u64* freed, hipStream_t s);
// The placed rows r < n by class (by_node: by (A[r], K[r]), node-major): out_rows / out_load: (by_node ? m : 1) * n_classes u64
// each, *other = the placed rows with K[r] >= n_classes (by_node: or A[r] >= m); all three in device memory, zeroed here.
// Up to kCensusMaxSlices * kCensusLdsCells cells: LDS accumulators per workgroup, one pass over the columns per slice of
// kCensusLdsCells cells; beyond: one pass, global adds per row.
void launch_census(const u32* A, const unsigned char* K, const u32* load, u64 n, u32 m, u32 n_classes, bool by_node,
                   u64* out_rows, u64* out_load, u64* other, hipStream_t s);

// --- pressure shedding (rio_gp_shed_idle): un-place the longest-idle candidates of the over-target nodes (kernels: k_ish_*) ---
// The columns a pass reads and the rule that names a candidate: an object of load >= 1 on a node < m with S < cutoff, or, with
// cls, S < cls->v[K[row]] (kernels k_ishc_*; the caller folds "never shed" classes in as cutoff 0).
struct IshCols {
    const u32 *A, *load, *aff, *S;
    u32 cutoff;
    const unsigned char* K;  // with cls only: the class column, readable in whole quads
    const ClsCutoffs* cls;   // nullptr: the plain form
};
// used, cand: m u64 each (zeroed here): the load of every row on node j, the load of its candidates; kmm: 2 u32 -> the smallest
// and the largest key ~S of a candidate (kNone, 0 without one)
void launch_ish_hist(const IshCols& c, u64 n, u32 m, u64* used, u64* cand, u32* kmm, hipStream_t s);
// launch_shed_select with the key ~S and the weight load: thr[slot_node] = the smallest key under which the candidates up to and
// including it weigh more than slot_free; slot_free -= the load of the candidates of a smaller key.  kmin / kmax: kmm as read
// back; the passes over digits every candidate shares are skipped.  Returns the histogram passes it launched.
u32 launch_ish_select(const IshCols& c, u64 n, u32 m, u32 s, const u32* map, const u32* slot_node, u64* slot_free, u32* pre,
                      u64* hist, u32* thr, u32 kmin, u32 kmax, hipStream_t st);
// the tie walk: cut[slot_node] = the first candidate of key thr[node], in row order, whose inclusive load prefix among those
// passes slot_free (kNone on the other nodes); mat: s * nt u64
void launch_ish_cut(const IshCols& c, const ShPlan& p, const u32* map, const u32* slot_node, const u64* slot_free, u64* mat,
                    u32* cut, const u32* thr, hipStream_t s);
// launch_exp_count / launch_exp_apply over the surplus predicate key > thr[node] || (key == thr[node] && row >= cut[node]);
// acc[kShAccSurplusLoad] += the surplus rows' load (the caller zeroes acc)
void launch_ish_count(const IshCols& c, const ChgPlan& p, u32 m, const u32* thr, const u32* cut, u32* cnt, u32* gsum, u32* total,
                      u64* acc, u64* freed, hipStream_t s);
void launch_ish_apply(u32* A, const IshCols& c, const ChgPlan& p, u32 m, const u32* thr, const u32* cut, const u32* cnt,
                      const u32* gsum, u64 cap, u32* rows, u32* node, u32* aff_life, u64* used, u64* freed, hipStream_t s);

}  // namespace riogp
