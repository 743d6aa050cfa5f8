// rio_gp_capi.hip — host side of the C ABI (include/rio_gpu_placement.h): handle, HBM tables,
// stream, and the kernel sequences behind every entry point.  No torch, no CPU fallback.
//
// Reference interfaces replaced (relative to /root/reference):
//   trait ObjectPlacement            rio-rs/src/object_placement/mod.rs:38-56
//   LocalObjectPlacement             rio-rs/src/object_placement/local.rs:22-68
//   Service::get_or_create_placement rio-rs/src/service.rs:193-254 (+ check_address_mismatch :261-298)
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <algorithm>
#include <atomic>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rio_gpu_placement.h"
#ifdef RIO_GP_LAB
#include "../../include/rio_gpu_placement_debug.h"
#endif
#include "placement_kernels.h"

using namespace riogp;

namespace {

thread_local std::string g_create_error;
struct RioGpNcclId { char internal[128]; };  // ncclUniqueId, passed BY VALUE to ncclCommInitRank
constexpr int kRing = 64;  // in-flight async solves whose verdicts we keep
constexpr u32 kUsedRing = 4;  // `used` buffers (rio_gp::used_ring): two chained ticks in flight, the buffers they add into and zero

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};
// A column of cap_rows u32 that a feature allocates and fills on its first use (lazy_fill).  It reads as nullptr until the fill
// is enqueued: a call after a failed allocation or fill allocates only what is still missing.
struct LazyColumn {
    u32* mem = nullptr;  // allocated
    bool filled = false;
    operator u32*() const { return filled ? mem : nullptr; }
};

}  // namespace

// RCCL, resolved at run time (dlopen of the copy already in the process, else librccl.so.1): the library has
// no link-time dependency on it, and a host that never shards never loads it.  Only the four entry points
// the data path needs; types restated from rccl.h (ncclUniqueId = 128 opaque bytes, ncclUint64 = 5).
struct RcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, RioGpNcclId, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
constexpr int kNcclUint64 = 5;
constexpr int kShardRing = 4;

struct ShardComm {
    RcclApi api;
    void* comm = nullptr;
    u32 rank = 0, R = 1;
    hipStream_t side = nullptr;  // exchange + global resolve of solve k run here, overlapping solve k+1's scan
    hipEvent_t ready[kShardRing] = {}, done[kShardRing] = {};
    bool done_valid[kShardRing] = {};
    u64* X[kShardRing] = {};
    u64* XG[kShardRing] = {};
    u32 k = 0;
};

// Peer-to-peer exchange windows (rio_gp_shard_p2p_*): one uncached window per rank, IPC-mapped by every peer.
//   xdata [kP2PSlots][R][Wx]  k_resolve_xchg's data-tagged words of rank r (a region of its own: a raw record word whose
//                             upper half happened to equal a step's tag would be taken for that step's data)
//   data  [kP2PSlots][R][W]   raw record of rank r for the step using that slot (fix-up exchanges)
//   flags [kP2PSlots][R][8]   sequence number of the step whose raw record is complete (one 64 B line each)
//   hello [R][8]              set-up handshake
constexpr int kP2PSlots = 4;
struct P2P {
    u32 rank = 0, R = 1;
    size_t W = 0;                 // u64 words per raw record row
    size_t Wx = 0;                // u64 words per tagged row (shard_xchg_words)
    u64* win = nullptr;           // this rank's window
    std::vector<void*> opened;    // peers' windows as mapped here (nullptr for our own)
    u64** d_peers = nullptr;      // device array [R] of window bases (ours included)
    u64* d_err = nullptr;         // set by a waiting kernel that timed out
    u64* scratch = nullptr;       // [W] staging of the local record
    u64 seq = 0;
    // Window slots rotate per KIND of exchange (tagged one-launch exchange | raw fix-up records), not with the sequence number:
    // a tick takes 1 + (1 + rounds) sequence numbers, and when that is a multiple of kP2PSlots every tick's tagged exchange
    // would land in the same slot — a rank that is through a churn-free tick (no further wait on its peers) would overwrite
    // the words a slower rank has not read yet, which then waits for a tag that is gone.  With slots of their own two
    // consecutive exchanges of a kind never share one, and no rank is ever more than one exchange ahead of another.
    u64 xslot_n = 0, yslot_n = 0;
    // A call that has taken sequence numbers / window slots and then fails (a launch error) leaves this rank's counters ahead
    // of what its peers will ever see: every later exchange would wait for, or overwrite, the wrong record.  The session is
    // marked and every later call on it fails with RIO_GP_EUPSTREAM until the windows are connected afresh.
    bool out_of_step = false;
    u32 co_resident = 1;          // ranks whose kernels run on THIS device, ours included (learnt at the handshake)
    size_t xdata_off(u32 slot, u32 r) const { return ((size_t)slot * R + r) * Wx; }
    size_t xwords() const { return (size_t)kP2PSlots * R * Wx; }
    size_t data_off(u32 slot, u32 r) const { return xwords() + ((size_t)slot * R + r) * W; }
    size_t flag_off(u32 slot, u32 r) const { return xwords() + (size_t)kP2PSlots * R * W + ((size_t)slot * R + r) * 8; }
    size_t hello_off(u32 r) const { return xwords() + (size_t)kP2PSlots * R * W + (size_t)kP2PSlots * R * 8 + (size_t)r * 8; }
    size_t total_words() const { return xwords() + (size_t)kP2PSlots * R * W + (size_t)kP2PSlots * R * 8 + (size_t)R * 8; }
};

struct StepGuard {  // see P2P::out_of_step
    P2P* q;
    bool done = false;
    ~StepGuard() { if (q && !done) q->out_of_step = true; }
};
static const char* const kOutOfStep = "the peer-to-peer session lost step with its peers in an earlier failed call: close it on every rank "
                                      "(rio_gp_shard_p2p_close), then export and connect fresh windows";

// How one solve of the REAL table is enqueued (solve_form computes it; the enqueue functions take it and keep nothing).
struct SolveForm {
    bool compact = false;    // the scan packs the pending rows per wave, the fix-up runs over the packed rows only
    bool cutpack = false;    // whole-table fix-up: the cut pass packs the rows that go on to the water-fill
    int inc = 0;             // 0 k_scan | 2 k_inc_scan + k_rebal: the scan and its fix-up write the committed column itself
    bool cut_apply = false;  // the whole-table fix-up is k_cut_apply (cuts + re-marking in one pass)
    bool resolve_searches = false;  // k_resolve searches the cuts of the packed rows itself (no k_cut_find launch)
    Plan fix_plan{};         // the plan of the table the fix-up runs over: the real one, or the packed rows'
    const PackOut* pkx = nullptr;  // where the fix-up finds the packed rows: the scan's pack columns | the balanced ones (k_rebal)
};
// The solve that waits for its commit.  commit_enqueue consumes it; a change of the solve's inputs drops it.
struct PendingSolve {
    bool have = false;
    bool inplace = false;  // it wrote its decisions into the committed column itself: the commit swaps no columns
    bool used_D = false;   // it ran with sb.D set: what its water-fill rounds admitted is in the D rows
    u64* used = nullptr;   // it built its `used` here instead of in sb.used_cur (a chained tick)
};

// The committed per-node load vector `used`.  Water-fill rounds keep what they admit apart from the solve's vector (the D rows,
// SolveBufs::D) and a chained tick adds into kChainReps replicas, so the committed vector is its first vector PLUS `rounds` rows
// of `parts` until somebody folds them in: the next solve's k_resolve for free (take_parts_for_resolve), or live() / ensure()
// when somebody needs the vector first.  Nothing outside this class reads or writes that state; the call sites say what they mean:
//   invalidate()   the column no longer matches: rebuild before the next use (pending parts are dropped with it)
//   live()         the pointer for a kernel that updates `used` in place, parts folded in; nullptr while it is invalid
//   ensure()       the pointer for a reader: folded, or rebuilt from the committed column (k_recompute_used)
//   fold_pending() the fold alone, for a solve about to zero the D rows or to publish without them
//   publish(...)   a solve's vector becomes the committed one: the only place where that happens
//   rebuilt()      the caller has just written the vector of the committed column into storage() itself
//   borrow()       storage() holds something else until the next rebuilt() / publish() / ensure() (the row-sharded rebalance)
struct rio_gp;
class UsedVec {
  public:
    struct Parts { u64* into; u32 rounds; const u64* src; };
    void init(rio_gp* owner, u64* first) { h = owner; vec = first; }
    u64* storage() const { return vec; }  // the first vector, whatever it holds (its writers; readers behind an ensure())
    bool valid() const { return state == kValid; }
    bool borrowed() const { return state == kBorrowed; }
    void invalidate() { if (state == kValid) state = kInvalid; pending = false; }
    void rebuilt() { state = kValid; pending = false; }
    void borrow() { state = kBorrowed; pending = false; }
    void fold_pending();  // pending parts in now (before something overwrites their source, or drops them)
    u64* live();
    u64* ensure();
    Parts take_parts_for_resolve();  // what launch_resolve folds (into == nullptr: nothing); they are no longer pending
    void publish(const PendingSolve& ps);  // a whole-table solve: its vector + its D rows | a chained tick's ring slot + its replicas
    void publish_request(bool vslow);      // a request-path solve: its vector, + its D rows when it took the fix-up

  private:
    enum State { kInvalid, kValid, kBorrowed };
    void swap_in(bool parts_in_D);
    rio_gp* h = nullptr;
    u64* vec = nullptr;
    State state = kValid;
    bool pending = false;        // `rounds` rows of `parts` are still to be added
    u32 rounds = 0;
    const u64* parts = nullptr;  // the handle's D rows | replicas 1.. of a chained tick's buffer
};

// What the last solves said, for the heuristics that choose the next one's form (solve_form: pending, fix_rows) and decide
// whether its fix-up is enqueued speculatively (solve_locked: slow).
struct SolveStats {
    u64 pending = 0;   // rows the previous solve found pending (claimants + spill candidates)
    bool pending_valid = false;
    u64 fix_rows = 0;  // rows it sent to the water-fill (spill candidates + rejected claimants)
    bool fix_valid = false;
    bool slow = false;
    // sync: the call read the fix-up's counters on the host (rio_gp_solve, rio_gp_tick): only those keep fix_rows current
    void record(const DevStats& v, bool slow_, bool sync) {
        pending = v.claimants + v.spillcand;
        pending_valid = true;
        if (sync) { fix_rows = v.spillcand + (slow_ ? v.rejected : 0); fix_valid = true; }
        slow = slow_;
    }
    void forget_pending() { pending_valid = false; }  // the table changed size or node ids
    void forget() { pending_valid = false; fix_valid = false; }  // an in-place solve was abandoned: the table is not what they describe
};

// One asynchronous committed tick in flight (rio_gp_tick_async fills it, rio_gp_tick_wait harvests it)
struct TickSlot {
    u32 G = 0;       // workgroups of its streaming grid (how many fix-up counter rows to fold)
    u32 rows = 0;    // its verdict rows: resolve_blocks(m), or G (a chained quiet tick: a row per workgroup)
    u64 mark = 0;    // column 7 of those rows
    u64 epoch = 0;   // mut_epoch it was enqueued under
    bool quiet = false;  // it was enqueued without its fix-up (checked against its verdict when harvested)
};

// host-side fold of the per-workgroup partial rows k_resolve (or a chained scan) stored into a pinned slot; mark != 0: every row
// must carry it (*bad is set where one does not)
static DevStats reduce_rows(const u64* rows, u32 nrows, u64 mark = 0, bool* bad = nullptr) {
    DevStats d;
    memset(&d, 0, sizeof d);
    for (u32 r = 0; r < nrows; ++r) {
        const u64* x = rows + (size_t)r * 8;
        if (mark && x[7] != mark && bad) *bad = true;
        d.load_kept += x[0]; d.load_claim_tot += x[1]; d.n_cut += x[2];
        d.kept += x[3]; d.evicted += x[4]; d.claimants += x[5]; d.spillcand += x[6];
    }
    return d;
}
static bool needs_fixup(const DevStats& v) { return v.n_cut > 0 || v.spillcand > 0; }

// What is in flight on the pinned verdict slots (h_slots / d_slots: 2 kRing slots of slot_rows rows of 8 words).  The table has two
// halves, each with ONE cursor, and the fix-up counter rows (h_fx) have a slot per half-slot that needs one:
//
//   client                                        verdict slots              counter rows (fx)    cursor
//   rio_gp_solve, _tick, _solve_profiled, the     0                          0                    none: they abandon() the solve
//     request path (synchronous: they wait)                                                        half; whatever it held is lost
//   rio_gp_solve_async                            [0, kRing), n % kRing      0 (rio_gp_solve_wait) SolveRing, Owner::solves
//   rio_gp_shard_resolve, _shard_solve_async      [0, kRing), n % kRing      none (DevStats)      SolveRing, Owner::shard
//     (rio_gp_shard_merge: slot 0, read at once)
//   rio_gp_tick_async                             kRing + k                  1 + k                TickRing, Owner::ticks
//   rio_gp_shard_tick_async                       kRing + k                  1 + k (its record)   TickRing, Owner::shard_ticks
//
// Who may start while what is in flight (may_start; every refusal is RIO_GP_EINVAL and changes nothing):
//   * The two owners of the tick half exclude each other: the same slots, the same counter rows.  rio_gp_tick_async harvests
//     its own ring when it is full; rio_gp_shard_tick_async refuses at kRing in flight (a harvest would need its peers).
//   * A tick of either kind does not start while the solve half's cursor is off 0: it publishes (the columns swap), and the
//     solves in flight still have their fix-up and their commit to come (rio_gp_solve_wait, rio_gp_shard_cut ... _finish).
//   * Row-sharded ticks in flight keep out the calls that start another asynchronous solve or reset the row-sharded
//     protocol: rio_gp_solve_async, rio_gp_shard_solve_async, rio_gp_shard_rebalance_begin.
//   * Everything else coexists.  Synchronous solves and rio_gp_solve_async run beside ticks in flight: they use the other
//     half and fx slot 0, and stream order puts them behind the ticks.  A synchronous solve abandons asynchronous solves in
//     flight (their verdicts are never read); rio_gp_tick_async ticks stay in flight across any other call until harvested.
//   * Not decided here, and not refused today: the two owners of the solve half advance the one cursor (rio_gp_solve_async with
//     a row-sharded solve at "resolved", and the other way round); rio_gp_shard_scan / _resolve with ticks in flight.
struct SolveRing {
    enum class Owner { none, solves, shard };
    // rio_gp_solve_async:
    SolveForm form{};           // the form of the last one: rio_gp_solve_wait enqueues its fix-up
    PendingSolve last{};        // ... and what it becomes once rio_gp_solve_wait has finished it (in flight, not yet pending)

    void init(const u64* host_slots, size_t slot_words) { host = host_slots; words = slot_words; }
    Owner owned_by() const { return owner; }
    bool in_flight() const { return n != 0; }
    bool any_solves() const { return any; }
    bool full() const { return n >= (u32)kRing; }            // rio_gp_solve_async recycles; row-sharded enqueues wrap
    u32 next_slot() const { return n % kRing; }               // where the next enqueue stores its verdict rows
    const u64* rows_host(u32 k) const { return host + (size_t)(k % kRing) * words; }
    void pushed(Owner o) { owner = o; ++n; if (o == Owner::solves) any = true; }
    void pushed_shard(u32 rows) { sh_slot = n; sh_rows = rows; pushed(Owner::shard); }
    // the ring is full: the verdicts of the solves in it are folded into the running count before their slots are overwritten
    void recycle(u32 nrows) {
        for (u32 k = 0; k < n; ++k) slow += needs_fixup(verdict(k, nrows));
        n = 0;
    }
    // The synchronous solves: whatever was in flight is never waited for.
    void abandon() { rewind(); slow = 0; any = false; }
    // The cursor alone (row-sharded protocol resets, rio_gp_shard_verdict): a rio_gp_solve_async count survives it, as it always has.
    void rewind() { n = 0; owner = Owner::none; }
    // rio_gp_solve_wait, after the stream: the last solve's verdict + how many of ALL the solves since the last wait took the fix-up
    // path.  (n == 0 with solves enqueued: only behind a rewind(); the last slot is read, as it always has been.)
    DevStats fold(u32 nrows, uint32_t* n_slow) {
        DevStats v;
        memset(&v, 0, sizeof v);
        if (n == 0) v = verdict(kRing - 1, nrows);
        for (u32 k = 0; k < n; ++k) {
            v = verdict(k, nrows);
            slow += needs_fixup(v);
        }
        *n_slow = slow;
        slow = 0;
        any = false;
        return v;
    }
    PendingSolve finish() { rewind(); return last; }  // the last solve of the ring is finished: it waits for its commit
    // rio_gp_shard_verdict, after the streams: x = the column sums of the last resolve's rows (0: cut nodes, 1: spill rows); returns
    // how many of the (at most kRing) resolves since the last verdict need the fix-up.  Ends with the cursor at 0.
    uint32_t shard_fold(u64 x[8]) {
        uint32_t cnt = 0;
        for (u32 k = n > (u32)kRing ? n - kRing : 0; k < n; ++k) {
            shard_sums(k, x);
            cnt += (x[0] > 0 || x[1] > 0);
        }
        shard_sums(sh_slot, x);
        rewind();
        return cnt;
    }

  private:
    DevStats verdict(u32 k, u32 nrows) const { return reduce_rows(rows_host(k), nrows); }
    void shard_sums(u32 k, u64 x[8]) const {  // one verdict row (k_shard_import) or one partial row per workgroup (k_resolve_xchg)
        for (int c = 0; c < 8; ++c) x[c] = 0;
        for (u32 r = 0; r < sh_rows; ++r)
            for (int c = 0; c < 8; ++c) x[c] += rows_host(k)[(size_t)r * 8 + c];
    }
    const u64* host = nullptr;  // h_slots
    size_t words = 0;           // u64 words per slot
    Owner owner = Owner::none;  // whose enqueue moved the cursor last (none: the cursor is at 0)
    u32 n = 0;                  // the cursor: the next enqueue stores its verdict rows into slot n % kRing
    u32 sh_slot = 0;            // row-sharded solves: verdict slot of the last resolve
    u32 sh_rows = 1;            // ... and its verdict rows there: 1 (k_shard_import) | resolve_blocks(m) (k_resolve_xchg)
    u32 slow = 0;      // fix-up verdicts among the rio_gp_solve_async solves whose ring slots were recycled
    bool any = false;  // a rio_gp_solve_async solve has been enqueued since the last rio_gp_solve_wait / abandon()
};

struct TickRing {
    enum class Owner { none, ticks, shard_ticks };
    u32 peeked = 0;             // Owner::ticks: ticks [0, peeked) have had their verdicts looked at (peek_ticks)
    TickSlot slot[kRing];       // Owner::ticks
    u64 shard_mark[kRing] = {}; // Owner::shard_ticks: word 15 of tick k's record (k_shard_tick_stats)
    std::vector<rio_gp_stats> done;  // harvested rio_gp_tick_async ticks rio_gp_tick_wait has not handed out yet

    void init(u64* host_slots, u64* dev_slots, size_t slot_words) {
        host = host_slots + (size_t)kRing * slot_words;
        dev = dev_slots + (size_t)kRing * slot_words;
        words = slot_words;
    }
    u32 count(Owner o) const { return owner == o ? n : 0; }  // ticks of that owner in flight: [0, count)
    bool full() const { return n == (u32)kRing; }
    u32 next_slot() const { return n; }                       // the tick the next enqueue becomes
    void pushed(Owner o) { owner = o; ++n; }
    void clear() { owner = Owner::none; n = 0; peeked = 0; }
    static u32 fx_slot(u32 k) { return 1 + k; }
    u64* rows_dev(u32 k) const { return dev + (size_t)(k % kRing) * words; }
    const u64* rows_host(u32 k) const { return host + (size_t)(k % kRing) * words; }
    DevStats reduce(u32 k, bool* bad) const { return reduce_rows(rows_host(k), slot[k % kRing].rows, slot[k % kRing].mark, bad); }

  private:
    u64 *host = nullptr, *dev = nullptr;  // the tick half of h_slots / d_slots
    size_t words = 0;
    Owner owner = Owner::none;  // none <=> n == 0
    u32 n = 0;                  // in flight: ticks [0, n), tick k in verdict slot kRing + k and fx slot fx_slot(k)
};

// The row-sharded solve (rio_gp_shard_*): the step the protocol is at and what travels with it.
enum class ShStep { idle, scanned, resolved, cut_exported, merged, spill_exported };
struct ShardSolve {
    ShStep step = ShStep::idle;
    bool slow = false;   // the solve in flight took the fix-up path (rio_gp_shard_verdict)
    u32 rank = 0, R = 1;
    hipStream_t side = nullptr;  // stream the last resolve ran on, when not the handle's
    bool at(ShStep s) const { return step == s; }
    void bind(u32 rank_, u32 R_, hipStream_t side_) { rank = rank_; R = R_; side = side_; }  // what the next resolve runs as
};

// The row-sharded rebalance (rio_gp_shard_rebalance_*): the step, what the gathered records said, the host's copies of the
// targets and the live flags (they outlive the calls that upload them).  rio_gp_shard_rebalance_begin assigns a fresh one.
enum class RbStep { idle, begun /* X out */, cut /* surplus record out */, selected /* Y out */, merged, round_exported };
struct RbSession {
    RbStep step = RbStep::idle;
    u32 rank = 0, R = 1, rounds = 0, fills = 0;
    bool list = false, first = false;
    u64 budget = 0, K = 0, sel_total = 0, pending = 0;
    u32 over = 0, over_before = 0;
    u64 epoch = 0;  // mut_epoch as rio_gp_shard_rebalance_begin left it: any other change of the inputs ends the protocol
    ShPlan plan{};
    // the load-ordered cut (rio_gp_shard_rebalance_begin_ordered, order = RIO_GP_REBALANCE_BY_LOAD): between cut and select the
    // threshold passes run in order, a histogram and then its pick
    u32 order = 0, slots = 0, sel_first = 0, sel_pass = 0;  // (passes sel_first .. sel.passes - 1 of the plan run)
    bool sel_hist_out = false;  // the histogram of pass sel_pass is out, its pick has not run
    ShSelPlan sel{};
    bool thresholds_pending() const { return order != 0 && over != 0 && sel_pass < sel.passes; }
    std::vector<u64> T;
    std::vector<u32> live;
    // A step continues the protocol only on the handle as begin left it: no call that changes an input of the solve (they all
    // count in mut_epoch) and none that rebuilt or republished `used` (which holds the protocol's vectors) came between.
    bool at(const rio_gp* h, RbStep s);
    bool finished() const {
        return (step == RbStep::cut && !over) || (step == RbStep::selected && !sel_total) ||
               (step == RbStep::merged && (!pending || fills == rounds));
    }
    u64 listed_rows() const { return step == RbStep::merged ? K : 0; }    // rows whose moves _finish applies and lists
    u64 selected_rows() const { return step == RbStep::selected || step == RbStep::merged || step == RbStep::round_exported ? K : 0; }
};

struct rio_gp {
    ShardComm* sc = nullptr;
    P2P* p2p = nullptr;
    std::mutex mu;
    std::string err;
    int device = 0;
    bool lifecycle = false;            // RIO_GP_CFG_ROW_LIFECYCLE: the affinity column also says which rows are objects
    u32 sa = 0;                        // RIO_GP_CFG_REF_SELF_ASSIGN: claims / first touches do not need a live node (Plan::sa)
    hipStream_t stream = nullptr;      // the stream every call of this handle is enqueued on
    hipStream_t own_stream = nullptr;  // created by rio_gp_create (rio_gp_set_stream may point `stream` elsewhere)
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    u64 cap_obj = 0, cap_rows = 0;
    u32 cap_nodes = 0, rounds = 2;
    u64 n = 0;
    u64 n_hi = 0;  // the largest n since creation: rows >= n_hi hold RIO_GP_NONE in both assignment columns (see commit_enqueue)
    u32 m = 0;
    // object table (HBM): two assignment columns (ping-pong), load, affinity, position scratch
    u32* assign[2] = {nullptr, nullptr};
    int cur = 0;
    u32 *load = nullptr, *aff = nullptr, *pos = nullptr;
    // node table
    u64* cap = nullptr;
    UsedVec used;  // the committed per-node loads (above)
    u32 *alive_bits = nullptr, *dead_bits = nullptr;
    // A liveness push is a bitmap written into a ring slot of mapped pinned memory (no launch).  It reaches alive_bits with
    // the next whole-table scan, which reads it from the slot (scan_nodes), or through flush_alive when something else
    // needs the device array first.
    u32 *h_alive_ring = nullptr, *d_alive_ring = nullptr;
    u32 alive_slot_words = 0, alive_slot = 0;
    bool alive_dirty = false;
    uint8_t* alive_bytes = nullptr;
    std::vector<uint8_t> h_alive;
    u64* D = nullptr;  // [kFillRounds][max_nodes] what a solve's water-fill rounds admit (SolveBufs::D; UsedVec folds them in)
    // solve scratch
    SolveBufs sb{};
    DevStats* dstats = nullptr;
    DevStats* h_stats = nullptr;  // pinned scratch for D2H copies of the device accumulators ([0]) + verdicts
    u64* h_slots = nullptr;       // pinned+mapped, kRing slots x slot_rows x 8: k_resolve partial counters
    u64* d_slots = nullptr;       // the same memory as the device sees it
    size_t slot_rows = 0;
    bool all_alive = true;
    Plan plan{};
    PendingSolve pending{};
    // what is in flight on the two halves of the slot table (above): asynchronous / row-sharded solves, ticks of either kind
    SolveRing solves;
    TickRing ticks;
    // fix-up counters as per-workgroup rows (FxRows, placement_kernels.h): device rows + pinned slots [1 + kRing][kMaxBlocks][8]
    // (slot 0: synchronous solves, slots 1..kRing: asynchronous ticks)
    u64* fx_dev = nullptr;
    u64* h_fx = nullptr;
    u64* d_fx = nullptr;
    // row-sharded solve (rio_gp_shard_*): global `used` snapshots, forced-node bitmap, spill base, verdict words
    u64 *sh_gprev = nullptr, *sh_gfinal = nullptr, *sh_rank_base = nullptr, *sh_verdict = nullptr;
    u32* sh_forced = nullptr;
    // outputs of the LOCAL column sums (k_resolve in shard mode): kept apart from the solver's arrays, which the
    // global resolve of the PREVIOUS solve may still be writing on the exchange stream
    u64 *sh_lkept = nullptr, *sh_lclaim = nullptr, *sh_lcur = nullptr;
    u32 *sh_lcutblk = nullptr, *sh_lcutidx = nullptr;
    ShardSolve sh;  // ... and the protocol's step
    // packed fix-up (PackOut, placement_kernels.h): scratch columns + per-wave counts; chosen adaptively per tick
    PackOut pk{};
    SolveStats last{};
    // A tick that took the fast path leaves every object placed; until the next call that changes an input of the solve
    // (mut_epoch counts those) every further tick keeps every row where it is, and rio_gp_tick_async enqueues no speculative
    // fix-up behind it: two launches a tick instead of five.  quiet_epoch = the mut_epoch such a tick was enqueued under.
    u64 mut_epoch = 0, quiet_epoch = ~0ull;
    int compact_mode = 0;  // 0 auto | 1 always | 2 never (rio_gp_debug_set_compact)
    // A committed tick over a mostly-placed table updates the assignment column in place and builds no kept histogram
    // (k_inc_scan), then k_rebal deals the pending rows out evenly to the fix-up's workgroups: 0 auto | 2 never (bits 7-8
    // of rio_gp_debug_set_compact; A/B runs, parity tests)
    int inc_mode = 0;
    PackOut pk2{};              // the balanced pack columns (k_rebal); the undecided rows' lists of k_cut_apply
    u64* Tg = nullptr;          // [max_nodes][16] k_cut_apply's wave sums of the undecided rows (placement_kernels.h, SolveBufs::Tg)
    int cutpack_mode = 0;  // the same for packing at the cut pass of whole-table solves (bits 5-6 of rio_gp_debug_set_compact)
    // Quiet ticks CHAIN (ScanChain, placement_kernels.h): a tick that cannot need the fix-up is one launch of the chained k_scan,
    // which adds the per-node kept loads into the tick's `used` buffer and stores its verdict rows itself.  The scans of a run of
    // quiet ticks alternate between the main stream and `scan2` and hand their rows over wave range by wave range (a flag per
    // wave), so the ramp-down of one scan and the ramp-up of the next overlap.  A run starts on the main stream (which orders it
    // behind everything else) and ends with the first chain_join (in the Locked guard every entry takes): the main stream waits
    // for `scan2`, and the last scan's waves have waited for every earlier one.
    hipStream_t scan2 = nullptr;
    u32* chain_flags = nullptr;                       // [kMaxBlocks * kWaves] one per wave range
    u32 *h_chain_err = nullptr, *d_chain_err = nullptr;  // mapped host word: a chained wait gave up
    u32 chain_seq = 0, chain_prev = 0, chain_pos = 0;  // last sequence number handed out | the run's last scan (0: no run) | its length
    hipEvent_t ev_run = nullptr;  // recorded on the main stream in front of a run's first scan: the run's first scan on `scan2` waits for
                                  // it, so that nothing but the two scans of the chain competes for the chip while one of them waits
    u64 overlap_min_rows = (u64)1 << 18;  // quiet ticks of smaller tables: k_scan + k_resolve on the main stream (lab builds,
                                          //  RIO_GP_OVERLAP_MIN_ROWS: the parity tests run the chained ticks on small tables)
    hipEvent_t ev_join = nullptr;
    // The `used` buffers: the committed one (h->used) and the solve's (sb.used_cur) are the first vectors of two of the kUsedRing slots of
    // used_ring; link c of a chained run adds into slot used_base + c and zeroes slot used_base + c + 2 (mod kUsedRing:
    // ScanChain), kChainReps replicas of m words each
    u64* used_ring = nullptr;
    size_t used_slot_words = 0;  // kChainReps * cap_nodes where the chain can run, cap_nodes elsewhere
    u32 used_base = 0;
    int chain_diag = 0;           // lab builds, RIO_GP_CHAIN_DIAG: 1 = the chained kernel on the main stream, no waits (PMC passes: the
                                  // profiler serialises dispatches) | 3 = every link waits for a sequence number nobody will ever
                                  // store (the bounded spin and the error path under test)
    bool chain_ok = false;        // two workgroups of the chained scan fit a CU (scan_chain_fits at the table's node count)
    u64 chain_total = 0;   // chained scans enqueued so far (lab builds: rio_gp_debug_chained_scans)
    int chain_mode = 0;    // 0 on | 2 never (lab builds: bit 12 of rio_gp_debug_set_compact)
    int cutapply_mode = 0; // whole-table fix-up by k_cut_apply (cuts + re-marking in one pass): 0 when the solve packs at the cut pass
                           // | 1 always | 2 never (k_cut_find + k_fill<APPLY>) (bits 9-10 of rio_gp_debug_set_compact)
    int spec_mode = 0;     // speculative fix-up enqueue: 0 auto (after a solve that needed it) | 1 always | 2 never
    int part_mode = 0;     // partitioned CRUD batches: 0 when the batch qualifies | 2 never (rio_gp_debug_set_compact bit 4)
    // clean_server(s): dead bitmap + evicted count in mapped pinned memory, self-resetting device counter + ticket
    u32* h_cs = nullptr;
    u32* d_cs = nullptr;
    size_t cs_words = 0;
    u64* cs_cnt = nullptr;
    unsigned int* cs_ticket = nullptr;
    // micro-batch staging: pinned host memory mapped into the device, [6][kSmallBatch] u32 = idx | req | node | flag | status | completion word
    u32* h_small = nullptr;
    u32* d_small = nullptr;
    u64 wait_seq = 1;       // sequence numbers of the synchronous solves (spin_rows): never 0 or 1
    u32* h_mid = nullptr;   // medium batches (<= kMidBatch), mapped pinned memory, [4][kMidBatch] u32: lookup idx | out; place_pending idx | req | out | flag
    u32* d_mid = nullptr;
    unsigned int* mid_ticket = nullptr;  // device word of the several-workgroup completion protocol
    u32* h_req = nullptr;   // request batches of up to kReqBatch entries from host buffers, mapped pinned memory, [4][kReqBatch] u32: idx | req | out | flag
    u32* d_req = nullptr;
    u32* pp_bad = nullptr;  // device word of the general request path: != 0 while a batch with an invalid entry is in flight
                            // ([1]: the window-sorted path's verdict word)
    u64* pp_claim = nullptr;  // [max_nodes + 1] window-sorted request path: claim load per requester + its "needs the solve" counter
    bool pp_last_slow = false;  // the last general-path request batch needed the cut / water-fill: the next one enqueues it speculatively
    DevBuf rq[4];           // staging of bigger host-buffer request batches (the general path's own scratch is vt / stage)
    void* pp_stage = nullptr;            // staging table of the three-launch request path (k_pp_stage / _decide / _apply)
    u32 small_seq = 0;      // sequence number of the last micro-batch call; its completion word is row 5, word 0
    // virtual table (place_pending) and staging for host-pointer calls
    DevBuf vt[4], stage[4];
    DevBuf vrec;  // big place_pending batches: virtual-table records {cur | load}, 8 bytes per request
    DevBuf part;  // scratch of the partitioned update / remove batches (records + fragment tables)
    bool timer_stopped = false;  // rio_gp_timer_stop has recorded the closing event of the measurement in progress
    // reverse placement index (rio_gp_rows_on_nodes), allocated on first use: the (slot x tile) matrix, chunk sums + total, the
    // node -> slot map on the device, the offsets of the host-pointer form; the map and the ranks are built in mapped pinned memory
    u32 *ni_cnt = nullptr, *ni_part = nullptr, *ni_map = nullptr;
    u64* ni_off = nullptr;
    u32 *h_ni = nullptr, *d_ni = nullptr;  // [RIO_GP_MAX_NODES] map | [RIO_GP_MAX_NODES + 1] ranks | [1] total read back
    DevBuf ni_rows;                        // the host-pointer form's listing (grows to the largest answer: 4 B per listed row)
    u32 ni_force_tile = 0;                 // lab builds: rows per tile (rio_gp_debug_set_node_index)
    // bounded rebalance (rio_gp_rebalance), grown on use: per-node arrays + counters, the (over node x tile) matrix, per-tile and
    // per-chunk counts, the packed rows (row | load | node), the host-pointer form's move listing (row | from | to)
    // ... and the load-ordered cut's (slot x digit) histogram
    DevBuf sh_nodes, sh_mat, sh_tile, sh_chunk, sh_pk, sh_mv, sh_sel;
    RbSession rb;  // row-sharded rebalance (rio_gp_shard_rebalance_*)
    // change feed (rio_gp_changes), allocated on first use: the checkpoint column B (cap_rows u32, RIO_GP_NONE to begin with), the
    // per-tile counts, the workgroup sums + total, a mapped word the total arrives in; the host-pointer form's staged listing
    // (row | old | new, grows to the largest listing)
    LazyColumn chg_B;
    u32 *chg_cnt = nullptr, *chg_gsum = nullptr;
    u32 *h_chg = nullptr, *d_chg = nullptr;
    DevBuf chg_stage;
    // idle expiry (rio_gp_touch_*, rio_gp_expire), allocated on first use: the last-seen column S (cap_rows u32, 0 to begin with)
    // and the freed-load word; the passes use the feed's counts, sums and mapped words (no two calls overlap on the stream)
    LazyColumn exp_S;
    u64* exp_freed = nullptr;
    // measured load (rio_gp_hits_*, rio_gp_load_fold), allocated on first use: the hit column H (cap_rows u32, 0 to begin with)
    LazyColumn hits_H;
    // hot-object report (rio_gp_top_rows), allocated on first use: the selection's device state, and pinned host memory for the
    // two sums and the host-pointer form's listing (16 + 12 * RIO_GP_TOP_MAX bytes); the per-tile counts are the feed's
    TopScratch* top_sc = nullptr;
    unsigned char* h_top = nullptr;
    // object classes (rio_gp_set_class*, rio_gp_expire_classes, rio_gp_census), allocated on first use: the class column K
    // (cap_rows bytes, 0 to begin with; cls_ready: the fills are enqueued), the sweep's per-class idle counts (kClsSlots copies of
    // kClsMax u64, zero between the calls) and the mapped pinned words their sum arrives in, and the host-pointer census's cells
    // (rows | load | other, grown on use)
    unsigned char* cls_K = nullptr;
    u64 *cls_tab = nullptr, *h_cls = nullptr, *d_cls = nullptr;
    bool cls_ready = false;
    // rule 13: the immovable classes, one bit per class (rio_gp_set_class_movable); only the rebalance reads them
    u32 cls_imm[kClsMax / 32] = {};
    bool cls_any_imm = false;
    bool cls_tab_stale = false;  // a sweep failed where nobody can tell whether k_cls_publish ran: the copies are zeroed on next use
    DevBuf cls_cells;
    std::vector<void*> allocs;
};

void UsedVec::fold_pending() {
    if (!pending) return;
    launch_used_fold(vec, parts, h->m, rounds, h->stream);
    pending = false;
}
u64* UsedVec::live() {
    if (state != kValid) return nullptr;
    fold_pending();
    return vec;
}
u64* UsedVec::ensure() {
    if (state == kValid) { fold_pending(); return vec; }
    launch_recompute_used(h->assign[h->cur], h->load, h->n, h->m, vec, h->stream);
    rebuilt();  // from the assignment column: nothing to fold
    return vec;
}
UsedVec::Parts UsedVec::take_parts_for_resolve() {
    const Parts p{pending ? vec : nullptr, rounds, parts ? parts : h->D};  // (parts: nullptr until the first publication)
    pending = false;
    return p;
}
// the solve's vector (sb.used_cur) becomes the committed one and the last committed one the next solve's scratch: no copy
void UsedVec::swap_in(bool parts_in_D) {
    std::swap(vec, h->sb.used_cur);
    state = kValid;
    pending = parts_in_D;  // + what its water-fill rounds admitted (D rows), folded in later
    rounds = h->rounds;
    parts = h->D;
}
void UsedVec::publish(const PendingSolve& ps) {
    if (!ps.used) return swap_in(ps.used_D);
    h->sb.used_cur = vec;  // a chained tick: its buffer of the ring is the new vector
    vec = ps.used;
    state = kValid;
    pending = true;  // + its other replicas, folded in later
    rounds = kChainReps - 1;
    parts = vec + h->m;
}
void UsedVec::publish_request(bool vslow) { swap_in(vslow); }

bool RbSession::at(const rio_gp* h, RbStep s) {
    if (step != RbStep::idle && (h->mut_epoch != epoch || !h->used.borrowed())) step = RbStep::idle;
    return step == s;
}

namespace {

#define HIPCHK(h, call)                                                                       \
    do {                                                                                      \
        hipError_t e__ = (call);                                                              \
        if (e__ != hipSuccess) {                                                              \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e__);                     \
            return RIO_GP_EUPSTREAM;                                                          \
        }                                                                                     \
    } while (0)

void p2p_free(rio_gp* h) {
    P2P* q = h->p2p;
    if (!q) return;
    for (void* o : q->opened) if (o) (void)hipIpcCloseMemHandle(o);
    if (q->d_peers) (void)hipFree(q->d_peers);
    if (q->d_err) (void)hipFree(q->d_err);
    if (q->scratch) (void)hipFree(q->scratch);
    if (q->win) (void)hipFree(q->win);
    delete q;
    h->p2p = nullptr;
}

void shard_comm_free(rio_gp* h) {
    p2p_free(h);
    ShardComm* sc = h->sc;
    if (!sc) return;
    if (sc->side) (void)hipStreamSynchronize(sc->side);
    if (sc->comm && sc->api.CommDestroy) (void)sc->api.CommDestroy(sc->comm);
    for (int q = 0; q < kShardRing; ++q) {
        if (sc->ready[q]) (void)hipEventDestroy(sc->ready[q]);
        if (sc->done[q]) (void)hipEventDestroy(sc->done[q]);
        if (sc->X[q]) (void)hipFree(sc->X[q]);
        if (sc->XG[q]) (void)hipFree(sc->XG[q]);
    }
    if (sc->side) (void)hipStreamDestroy(sc->side);
    delete sc;
    h->sc = nullptr;
}

int fail(rio_gp* h, int rc, const std::string& msg) {
    h->err = msg;
    return rc;
}

template <typename T>
int dalloc(rio_gp* h, T** out, size_t count) {
    void* p = nullptr;
    if (count == 0) count = 1;
    hipError_t e = hipMalloc(&p, count * sizeof(T));
    if (e != hipSuccess) {
        h->err = std::string("hipMalloc: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? RIO_GP_ENOMEM : RIO_GP_EUPSTREAM;
    }
    h->allocs.push_back(p);
    *out = static_cast<T*>(p);
    return RIO_GP_OK;
}

int ensure(rio_gp* h, DevBuf& b, size_t bytes) {
    bytes = (bytes + 4095) & ~(size_t)4095;
    bytes += 8 * kTile * sizeof(u32);  // k_scan prefetches up to 4 tiles past n
    if (b.bytes >= bytes) return RIO_GP_OK;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) return fail(h, e == hipErrorOutOfMemory ? RIO_GP_ENOMEM : RIO_GP_EUPSTREAM,
                                      std::string("hipMalloc(staging): ") + hipGetErrorString(e));
    b.bytes = bytes;
    return RIO_GP_OK;
}

// first use of a lazily filled column: allocate (once), fill with `value`, publish
int lazy_fill(rio_gp* h, LazyColumn& c, u32 value) {
    if (c.filled) return RIO_GP_OK;
    int rc;
    if (!c.mem && (rc = dalloc(h, &c.mem, h->cap_rows))) return rc;
    launch_fill_u32(c.mem, h->cap_rows, value, h->stream);
    HIPCHK(h, hipGetLastError());
    c.filled = true;  // (last: it is what says the column is complete)
    return RIO_GP_OK;
}

// The host-pointer form of a listing: the first L words of each of the k arrays staged at d, d + stride, ... go into the
// caller's k arrays; k async copies, one wait.
int read_listing(rio_gp* h, const u32* d, u64 stride, u64 L, std::initializer_list<u32*> out) {
    for (u32* o : out) {
        HIPCHK(h, hipMemcpyAsync(o, d, L * sizeof(u32), hipMemcpyDeviceToHost, h->stream));
        d += stride;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RIO_GP_OK;
}

void fill_stats(const DevStats& d, u64 n, rio_gp_stats* s) {
    if (!s) return;
    memset(s, 0, sizeof *s);
    (void)n;
    s->n_objects = d.kept + d.claimants + d.spillcand;  // = rows, minus the rows that are not objects (RIO_GP_AFF_INACTIVE)
    s->kept = d.kept;
    s->evicted = d.evicted;
    s->claimed = d.claimants - d.rejected;
    s->spilled = d.spilled;
    s->unplaced = d.unplaced;
    s->load_kept = d.load_kept;
    s->load_claimed = d.load_claim_tot - d.load_rejected;
    s->load_spilled = d.load_spilled;
    s->load_unplaced = d.load_unplaced;
    s->cut_nodes = (uint32_t)d.n_cut;
    s->slow_path = needs_fixup(d) ? 1u : 0u;
    s->rounds_run = (uint32_t)d.rounds_run;
}

u32* aff_life(rio_gp* h) { return h->lifecycle ? h->aff : nullptr; }
Plan hplan(rio_gp* h, u64 n) {  // the decomposition of a table of n rows under this handle's policy flags
    Plan p = make_plan(n, h->m, 0);
    p.sa = h->sa;
    return p;
}
Table real_table(rio_gp* h) { return Table{h->assign[h->cur], h->load, h->aff, h->assign[h->cur ^ 1]}; }
constexpr u64 kSearchMaxBlockRows = 1u << 17;  // rows per block up to which k_resolve searches the cuts itself
constexpr u32 kAliveSlots = 2 * kRing + 4;  // every slot handed to a scan belongs to a solve or tick of a ring of kRing
void launch_alive_words(rio_gp* h) {
    WordPack pk;
    const u32 words = (h->m + 31) / 32;
    memcpy(pk.w, h->h_alive_ring + (size_t)h->alive_slot * h->alive_slot_words, sizeof(u32) * (words ? words : 1));
    launch_store_words(pk, words, h->alive_bits, h->stream);
}
// the device's liveness bitmap is up to date after this (one tiny kernel if a push is pending)
void flush_alive(rio_gp* h) {
    if (!h->alive_dirty) return;
    h->alive_dirty = false;
    launch_alive_words(h);
}
NodeTab real_nodes(rio_gp* h) { flush_alive(h); return NodeTab{h->cap, h->alive_bits, nullptr}; }
// the node tables for a whole-table solve that starts with k_scan: a pending liveness push rides in that launch
NodeTab scan_nodes(rio_gp* h) {
    NodeTab nt{h->cap, h->alive_bits, nullptr};
    if (h->alive_dirty) {
        h->alive_dirty = false;
        nt.alive_src = h->d_alive_ring + (size_t)h->alive_slot * h->alive_slot_words;
    }
    return nt;
}

// One run of chained scans per process and DEVICE at a time: the chain's progress argument counts the workgroup slots of ONE pair
// of launches (two per CU); a second handle's pair on the same device could hold the slots the first one's earlier launch needs.
// (A host that drives one handle per GPU from one process chains on every one of them.)
constexpr int kChainDevices = 64;
std::atomic<rio_gp*> g_chain_owner[kChainDevices];
std::atomic<rio_gp*>& chain_owner(rio_gp* h) { return g_chain_owner[(unsigned)h->device % kChainDevices]; }
bool chain_begin(rio_gp* h) {
    if (h->chain_prev) return true;  // (a run in progress is this handle's)
    rio_gp* none = nullptr;
    return chain_owner(h).compare_exchange_strong(none, h, std::memory_order_acq_rel) || none == h;
}
void chain_end(rio_gp* h) {
    h->chain_prev = 0;
    h->chain_pos = 0;
    rio_gp* me = h;
    (void)chain_owner(h).compare_exchange_strong(me, nullptr, std::memory_order_acq_rel);
}
// the main stream waits for the chained run in progress: what of it is not on the main stream is on `scan2` (no-op without a run)
void chain_join(rio_gp* h) {
    if (!h->chain_prev) return;
    (void)hipSetDevice(h->device);
    if (h->chain_pos >= 2 &&
        (hipEventRecord(h->ev_join, h->scan2) != hipSuccess || hipStreamWaitEvent(h->stream, h->ev_join, 0) != hipSuccess)) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(h->scan2);
    }
    chain_end(h);  // (the run of chained scans ends here: the next one starts on the main stream, behind this wait)
}
// what every entry point holds: the handle's mutex, with the chained run joined (rio_gp_tick_async joins only when it must)
struct Locked {
    std::unique_lock<std::mutex> l;
    explicit Locked(rio_gp* h, bool join = true) : l(h->mu) { if (join) chain_join(h); }
};
// a change of the solve's inputs: the solve waiting for its commit no longer describes them, and no tick is quiet any more
void inputs_changed(rio_gp* h) {
    h->pending = PendingSolve{};
    ++h->mut_epoch;
}

// The form of one solve of the real table (h->plan is that table's, mark included), from the handle's knobs and statistics and
// from what the caller knows:
//   commit   the solve is published in this call (a tick)
//   sync     this call reads the verdict on the host (rio_gp_solve, rio_gp_tick): only those calls keep last.fix_rows current
//   quiet    nothing has changed since a tick that left every object placed: no fix-up can be needed
//   chained  ... and the tick is the chained k_scan alone, a link of a run
// This is the only place where compact_mode, cutpack_mode, inc_mode, cutapply_mode, last.pending and last.fix_rows choose a form.
// spec_mode and chain_mode stay with their readers: spec_mode decides WHEN solve_locked enqueues the fix-up, which shapes that
// function's host waits and nothing of the form; chain_mode is one of tick_async_locked's conditions for a link of a run, next
// to the stream's and the table's, and must be decided before the run is joined — `chained` is its outcome.
SolveForm solve_form(const rio_gp* h, bool commit, bool sync, bool quiet = false, bool chained = false) {
    SolveForm f;
    f.fix_plan = h->plan;
    f.pkx = &h->pk;
    if (chained) return f;  // (nothing packs, nothing searches, k_scan maintains no rejected-load tables)
    // Adaptive packed fix-up: when the previous solve left few rows pending — but some: a stream without churn keeps the
    // plain scan, two tiles in flight — (a churn stream: most rows are kept),
    // k_scan also packs this solve's pending rows per wave, and — if the verdict then asks for the fix-up — the cut
    // and water-fill kernels run over the packed rows only (O(pending) passes instead of O(rows)); results identical.
    // (A solve that is neither published nor waited for here — rio_gp_solve_async — gets its fix-up from a later call, over
    // the table as it is then: it packs nothing.)
    f.compact = !quiet && (commit || sync) &&
                (h->compact_mode == 1 ||
                 (h->compact_mode == 0 && h->last.pending_valid && h->last.pending > 0 && h->last.pending * 4 <= h->n && h->n >= 65536));
    // Packing at the cut pass: a whole-table solve (nothing known to be kept) whose previous solve sent few rows to the
    // water-fill — a contended table re-solved: ~10 % of the rows — lets round 0 of k_fill pack those rows on its way, and
    // the later rounds run over them instead of streaming the table again.  Results identical.
    f.cutpack = sync && !f.compact && h->rounds >= 1 && fill_can_pack(h->m) &&
                (h->cutpack_mode == 1 || (h->cutpack_mode == 0 && h->last.fix_valid && h->last.fix_rows * 4 <= h->n && h->n >= 65536));
    // ... and when the tick is committed and the library's `used` vector is valid, the scan streams the assignment column
    // alone and works in place (k_inc_scan + k_rebal).  Only a COMMITTED tick may work in place, only a
    // valid `used` vector can stand in for the kept histogram, and the rings of pending rows must fit the LDS next to the
    // liveness bitmap.
    // (Tables whose blocks are beyond the in-resolve cut search — config 4 on one GPU, 390 K rows a block — take this path too:
    // 100 M x 4 096, three boxes, same-run A/B: 700-720 us pipelined against 734-797 with k_scan<COMPACT>; round 0 of the
    // water-fill alone is 60-90 us shorter over the balanced rows.  The cut search stays k_cut_find's launch there.)
    if (f.compact && commit && h->used.valid() && h->inc_mode != 2 && inc_scan_fits(h->m) && h->m != 0) {
        f.inc = 2;
        f.fix_plan = rebal_plan(h->plan);
        f.pkx = &h->pk2;
    }
    f.fix_plan.wcnt = f.compact ? f.pkx->wcnt : nullptr;
    // The whole-table fix-up is k_cut_apply when the solve packs at the cut pass (few rows go on to the water-fill: the ranges
    // with work are a fraction of the table and k_cut_apply deals them out over the chip); a solve that re-marks most of the
    // table keeps the two-pass form.  Never over packed rows (f.inc implies f.compact).
    f.cut_apply = !f.compact && h->cutapply_mode != 2 && !h->sb.forced_bits && cut_apply_fits(h->m) && (h->cutapply_mode == 1 || f.cutpack);
    // The exact cut search rides in k_resolve when a block's packed rows are few enough for a wave pair per node to stream
    // (config 3: 39 K rows a block, 18 us against 6 + 14 for a resolve and a search launch of their own); on big blocks
    // (config 4 on one GPU: 390 K rows, ~39 K packed) a wave pair per node takes 91 us where k_cut_find's (block, node slice)
    // work items spread over the chip take 36: there the search stays a launch of its own.
    f.resolve_searches = f.compact && h->plan.G && h->n / h->plan.G <= kSearchMaxBlockRows;
    return f;
}

// The fix-up of a solve whose fast path said it needs one (or may need one: every kernel here guards itself on the
// device, so the sequence can be enqueued before the host has read the verdict):
//   the exact cut search — k_cut_find, unless launch_resolve already searched (packed pending rows: f.resolve_searches);
//   round 0 = k_fill<APPLY, FILL> (re-mark + water-fill; cutpack: it also packs the rows that go on to the water-fill, and
//   the later rounds run over those rows only); rounds 1.. = k_fill<FILL>.
// A virtual table (the request path) runs the plain form: SolveForm{}.
void enqueue_slow(rio_gp* h, const SolveForm& f, const Plan& p, const Table& t, const NodeTab& nt, bool virt) {
    const bool cutpack = f.cutpack && !virt && !p.wcnt;
    // Whole-table solve of the real table: ONE pass finds the exact cuts, re-marks and (cutpack) packs — k_cut_apply — and
    // every round, the first included, is a plain water-fill round (over the packed rows / over the table).
    if (!virt && !f.resolve_searches && !p.wcnt && f.cut_apply) {
        launch_cut_apply(p, t, nt, h->sb, h->pk, h->pk2, h->Tg, cutpack, h->all_alive, h->stream);
        if (cutpack) {
            Plan pp = p;
            pp.wcnt = h->pk.wcnt;
            Table vt{h->pos /* all-NONE column: every packed row is pending */, h->pk.load, h->pk.aff, h->pk.next};
            vt.pk_idx = h->pk.idx;
            vt.real_next = t.next;
            vt.none_prewritten = true;
            for (u32 r = 0; r < h->rounds; ++r) launch_fill(pp, vt, nt, h->sb, true, false, true, (int)r, r + 1 == h->rounds, h->stream);
        } else {
            for (u32 r = 0; r < h->rounds; ++r) launch_fill(p, t, nt, h->sb, false, false, true, (int)r, r + 1 == h->rounds, h->stream);
        }
        return;
    }
    if (!f.resolve_searches) launch_cut_find(p, t, nt, h->sb, virt, h->stream, true);
    launch_fill(p, t, nt, h->sb, virt, true, true, 0, h->rounds == 1, h->stream, cutpack ? &h->pk : nullptr);
    if (cutpack) {
        Plan pp = p;
        pp.wcnt = h->pk.wcnt;
        Table vt{h->pos /* all-NONE column: every packed row is pending */, h->pk.load, h->pk.aff, h->pk.next};
        vt.pk_idx = h->pk.idx;
        vt.real_next = t.next;
        vt.none_prewritten = true;
        for (u32 r = 1; r < h->rounds; ++r) launch_fill(pp, vt, nt, h->sb, true, false, true, (int)r, r + 1 == h->rounds, h->stream);
        return;
    }
    for (u32 r = 1; r < h->rounds; ++r) launch_fill(p, t, nt, h->sb, virt, false, true, (int)r, r + 1 == h->rounds, h->stream);
}

// scan + resolve of one solve over the REAL table: the packed pending rows' cuts are searched inside k_resolve, the previous
// committed solve's D rows are folded into the committed vector before k_resolve zeroes them.  Returns what the solve is once
// it waits for its commit; the enqueue functions keep nothing of a solve on the handle themselves.
PendingSolve enqueue_scan_resolve(rio_gp* h, const SolveForm& f, const Table& t, const NodeTab& nt, u64* host_rows) {
    h->sb.D = h->D;
    // a whole-table fix-up by k_cut_apply takes its ordered spill totals from its own pass: k_scan / k_resolve need not
    // maintain the rejected-load tables R / RP (k_resolve: one prefix over the blocks per node group that owns a cut)
    SolveBufs rb = h->sb;
    if (f.cut_apply) { rb.R = nullptr; rb.RP = nullptr; rb.Tg = h->Tg; }
    if (f.inc) {
        // (t.cur is read AND written: the tick is committed, nobody is promised the table as it was)
        launch_inc_scan(h->plan, h->assign[h->cur], h->load, h->aff, nt, h->sb, h->pk, h->stream);
        launch_rebal(h->plan, f.fix_plan, h->pk, nt, h->pk2, h->sb, h->stream);
    } else {
        launch_scan(h->plan, t, nt, rb, false, h->all_alive, h->stream, nullptr, nullptr, f.compact ? &h->pk : nullptr);
    }
    Plan rp = f.fix_plan;
    if (!f.resolve_searches) rp.wcnt = nullptr;
    const UsedVec::Parts fold = h->used.take_parts_for_resolve();
    launch_resolve(rp, nt, rb, host_rows, h->stream, nullptr, nullptr, f.resolve_searches ? f.pkx : nullptr,
                   fold.into, fold.rounds, f.inc ? h->used.storage() : nullptr, fold.src);
    return PendingSolve{true, f.inc != 0, h->sb.D != nullptr, nullptr};
}
u64* used_slot(rio_gp* h, u32 q) { return h->used_ring + (size_t)(q % kUsedRing) * h->used_slot_words; }
// A quiet tick as one link of a chained run: the chained k_scan alone (ScanChain, placement_kernels.h) — its workgroups add the
// kept loads into this link's `used` buffer and store the tick's verdict rows (`rows`, one per workgroup) themselves.  Nothing of
// the fix-up's scratch is written; the vector it builds replaces the committed one whole (commit_enqueue: its replicas 1.. are
// folded into replica 0 later, like a solve's D rows — whatever D rows were pending are superseded).
PendingSolve enqueue_chained(rio_gp* h, const Table& t, const NodeTab& nt, u64* rows) {
    hipStream_t ss = h->stream;
    ScanChain ch{h->chain_flags, h->d_chain_err};
    if (!h->chain_prev) {
        // the run's buffers start behind the committed one; its first two links add into buffers nothing zeroes inside the run
        h->used_base = (u32)((h->used.storage() - h->used_ring) / h->used_slot_words) + 1;
        const size_t zb = (size_t)kChainReps * h->m * sizeof(u64);
        (void)hipMemsetAsync(used_slot(h, h->used_base), 0, zb, h->stream);
        (void)hipMemsetAsync(used_slot(h, h->used_base + 1), 0, zb, h->stream);
        (void)hipEventRecord(h->ev_run, h->stream);
    } else if ((h->chain_pos & 1u) && h->chain_diag != 1) {
        ss = h->scan2;
        if (h->chain_pos == 1) (void)hipStreamWaitEvent(ss, h->ev_run, 0);
    }
    ch.wait = !h->chain_prev || h->chain_diag == 1 ? 0 : h->chain_diag == 3 ? h->chain_prev + 1000u : h->chain_prev;  // (3: a predecessor that never comes)
    ch.set = ++h->chain_seq;
    ch.used = used_slot(h, h->used_base + h->chain_pos);
    ch.used_zero = used_slot(h, h->used_base + h->chain_pos + 2);
    ch.rows = rows;
    ++h->chain_total;
    h->chain_prev = ch.set;
    ++h->chain_pos;
    SolveBufs rb = h->sb;
    rb.R = nullptr; rb.RP = nullptr; rb.Tg = nullptr;
    launch_scan(h->plan, t, nt, rb, false, h->all_alive, ss, nullptr, nullptr, nullptr, &ch);
    return PendingSolve{true, false, false, ch.used};
}
// the fix-up over the rows the scan packed (compact): the water-fill writes every decision through the packed rows' indices
// into the real column itself — the other assignment column, or (k_inc_scan) the committed one
void enqueue_slow_packed(rio_gp* h, const SolveForm& f, const NodeTab& nt) {
    const PackOut& pkx = *f.pkx;
    Table vt{h->pos /* all-NONE column: every packed row is pending */, pkx.load, pkx.aff, pkx.next};
    vt.pk_idx = pkx.idx;
    vt.real_next = f.inc ? h->assign[h->cur] : h->assign[h->cur ^ 1];
    enqueue_slow(h, f, f.fix_plan, vt, nt, true);
}

u64* slot_dev(rio_gp* h, u32 k) { return h->d_slots + (size_t)(k % kRing) * h->slot_rows * 8; }  // solve half
DevStats reduce_slot(rio_gp* h, u32 k, u32 m) { return reduce_rows(h->solves.rows_host(k), resolve_blocks(m)); }

// May `who` start now?  The one place that decides it, and that words the refusals (the table above SolveRing says why).
enum class Client { tick_async, solve_async, shard_solve_async, shard_tick_async, shard_rebalance_begin };
int may_start(rio_gp* h, Client who) {
    static const char* const name[] = {"rio_gp_tick_async", "rio_gp_solve_async", "rio_gp_shard_solve_async", "rio_gp_shard_tick_async",
                                       "rio_gp_shard_rebalance_begin"};
    const bool tick = who == Client::tick_async || who == Client::shard_tick_async;
    const char* why = nullptr;
    if (tick && h->solves.in_flight())
        why = h->solves.owned_by() == SolveRing::Owner::shard ? "a row-sharded solve is in flight (finish it: rio_gp_shard_verdict ... rio_gp_shard_finish)"
                                                         : "rio_gp_solve_async solves are in flight (call rio_gp_solve_wait)";
    else if (who != Client::shard_tick_async && h->ticks.count(TickRing::Owner::shard_ticks))
        why = "row-sharded ticks are in flight (call rio_gp_shard_tick_wait)";
    else if (who == Client::shard_tick_async && h->ticks.count(TickRing::Owner::ticks))
        why = "rio_gp_tick_async ticks are in flight (call rio_gp_tick_wait)";
    else if (who == Client::shard_tick_async && h->ticks.full())
        why = "64 ticks in flight (call rio_gp_shard_tick_wait)";
    return why ? fail(h, RIO_GP_EINVAL, std::string(name[(int)who]) + ": " + why) : RIO_GP_OK;
}
bool row_sharded(const rio_gp* h) { return h->sc || h->p2p || h->ticks.count(TickRing::Owner::shard_ticks); }
// The rebalance, the change feed, node removal, idle expiry, measured load and the hot-object report work on a whole table, not
// on one rank's rows: `who` is refused on a handle of the row-sharded solve.
int refuse_row_sharded(rio_gp* h, const char* who) {
    if (!row_sharded(h)) return RIO_GP_OK;
    return fail(h, RIO_GP_EINVAL, std::string(who) + ": not implemented on a handle of the row-sharded solve");
}

// the fix-up kernels of the next solve write their per-workgroup counter rows into pinned slot `slot` (0: synchronous
// solves, 1 + k: asynchronous tick k)
void use_fx_slot(rio_gp* h, u32 slot) {
    h->sb.fx.dev = h->fx_dev;
    h->sb.fx.host = h->d_fx + (size_t)slot * kMaxBlocks * 8;
    h->sb.fx.seq = 0;
}
// Waiting without the runtime: the kernels of a synchronous solve store the solve's sequence number into word 7 of every
// row they write into mapped pinned memory (k_resolve's partial rows, the last water-fill round's counter rows); the host
// spins until every row carries it.  launch + hipStreamSynchronize costs 12.6 us, launch + spin 7.3 us
// (tools/sync_probe.py).  false: not there after 50 ms — the caller asks the stream (a dead kernel shows up there).
bool spin_rows(const u64* rows, u32 nrows, u64 seq) {
    const volatile u64* r = rows;
    const auto t0 = std::chrono::steady_clock::now();
    u32 spins = 0;
    for (u32 i = 0; i < nrows;) {
        if (r[(size_t)i * 8 + 7] == seq) { ++i; continue; }
        __builtin_ia32_pause();
        if ((++spins & 0xFFFu) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) return false;
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return true;
}
// fold those rows into a fast-path verdict (after the stream has been waited for)
void fold_fx(rio_gp* h, u32 slot, u32 G, DevStats* v) {
    const u64* rows = h->h_fx + (size_t)slot * kMaxBlocks * 8;
    u64 x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (u32 b = 0; b < G; ++b)
        for (int c = 0; c < 8; ++c) x[c] += rows[(size_t)b * 8 + c];
    v->rejected = x[0]; v->load_rejected = x[1];
    v->spilled = x[2]; v->load_spilled = x[3];
    v->unplaced = x[4]; v->load_unplaced = x[5];
    v->rounds_run = x[6];
}
int merge_slow(rio_gp* h, DevStats* v) {
    if (!(h->sb.fx.seq && spin_rows(h->h_fx, h->plan.G, h->sb.fx.seq))) HIPCHK(h, hipStreamSynchronize(h->stream));
    fold_fx(h, 0, h->plan.G, v);
    return RIO_GP_OK;
}

// A solve that works in place (k_inc_scan) has rewritten part of the committed column by the time anything behind it can
// fail.  If the call does not reach its end, the solve is abandoned, and the table is no longer what the `used` vector and
// the pending-row statistics describe: the next tick re-solves it from scratch (plain k_scan: the kept histogram is rebuilt
// from the rows).
struct InplaceGuard {
    rio_gp* h;
    bool ok = false;
    ~InplaceGuard() {
        if (ok) return;
        if (h->pending.inplace) { h->used.invalidate(); h->last.forget(); }
        h->pending = PendingSolve{};
    }
};

int commit_enqueue(rio_gp* h) {
    const PendingSolve ps = h->pending;
    if (!ps.have) return fail(h, RIO_GP_EINVAL, "rio_gp_commit: no solve to commit");
    if (!ps.inplace) {  // (k_inc_scan and its fix-up wrote the committed column itself)
        // rows >= n keep their contents (rio_gp_set_num_objects), and a solve writes rows < n of the other column only: the rows
        // above n that were ever in use go over with the swap.  Nothing to copy while n is at its high-water mark (the string
        // layer, every table that does not shrink).
        if (h->n < h->n_hi)
            HIPCHK(h, hipMemcpyAsync(h->assign[h->cur ^ 1] + h->n, h->assign[h->cur] + h->n, (size_t)(h->n_hi - h->n) * sizeof(u32),
                                     hipMemcpyDeviceToDevice, h->stream));
        h->cur ^= 1;
    }
    h->used.publish(ps);  // publication = two pointer swaps: the columns' above, the `used` vectors' in there
    h->pending = PendingSolve{};  // (consumed; not an input change: mut_epoch stays)
    return RIO_GP_OK;
}

// One whole-table solve; with `commit` the publication (two pointer swaps) happens before the last wait.
// Host waits: verdict + completion when the fix-up is needed, verdict only on the fast path — and ONE wait when the
// fix-up was enqueued speculatively (below).
int solve_locked(rio_gp* h, rio_gp_stats* stats, bool commit = false) {
    InplaceGuard ipg{h};
    h->plan = hplan(h, h->n);
    h->solves.abandon();
    use_fx_slot(h, 0);
    const u64 seq = ++h->wait_seq;
    h->plan.mark = seq;  // k_resolve's partial rows carry it ...
    // ... and so do the counter rows of the last water-fill round, when that round is the solve's last kernel
    const bool fx_last = h->rounds >= 1;
    if (fx_last) h->sb.fx.seq = seq;
    const Table t = real_table(h);
    const NodeTab nt = scan_nodes(h);
    // Speculative fix-up: when the previous solve needed the fix-up (a churn stream needs it every tick), its kernels
    // are enqueued right behind k_resolve instead of after a host round trip for the verdict.  Every fix-up kernel
    // guards itself on device (the cut search: stats->n_cut; the water-fill rounds: pending-row count), so a solve that
    // turns out not to need them pays a few no-op launches and gets the same result.
    const bool spec = h->spec_mode != 2 && (h->spec_mode == 1 || h->last.slow);
    const SolveForm f = solve_form(h, commit, true);
    h->pending = enqueue_scan_resolve(h, f, t, nt, slot_dev(h, 0));  // (a call that fails from here on abandons it: InplaceGuard)
    DevStats v;
    bool slow = false;
    const u64* vrows = h->h_slots;  // slot 0 of the solve ring
    if (!spec) {
        if (!spin_rows(vrows, resolve_blocks(h->m), seq)) HIPCHK(h, hipStreamSynchronize(h->stream));
        v = reduce_slot(h, 0, h->m);
        slow = needs_fixup(v);
    }
    if (spec || slow) {
        if (f.compact) enqueue_slow_packed(h, f, nt);
        else enqueue_slow(h, f, h->plan, t, nt, false);
    }
    h->solves.abandon();
    if (commit) {
        int rc = commit_enqueue(h);
        if (rc) return rc;
    }
    if (spec) {
        if (!(fx_last && spin_rows(h->h_fx, h->plan.G, seq))) HIPCHK(h, hipStreamSynchronize(h->stream));
        v = reduce_slot(h, 0, h->m);
        slow = needs_fixup(v);
        if (slow) fold_fx(h, 0, h->plan.G, &v);  // the water-fill rounds stored every workgroup's row into the pinned slot
    } else if (slow) {
        int rc = merge_slow(h, &v);  // waits for the last round's rows (or the stream)
        if (rc) return rc;
    }  // (fast path: k_resolve was the last kernel and its rows are here; the publication is two host-side swaps)
    HIPCHK(h, hipGetLastError());
    h->last.record(v, slow, true);
    fill_stats(v, h->n, stats);
    ipg.ok = true;
    return RIO_GP_OK;
}

// wait for the asynchronous ticks in flight and turn their verdict slots + device-stats copies into rio_gp_stats
// verdicts of enqueued ticks that have already landed in their pinned slots (every row carries the tick's mark): no wait
void peek_ticks(rio_gp* h) {
    TickRing& tr = h->ticks;
    for (const u32 n = tr.count(TickRing::Owner::ticks); tr.peeked < n; ++tr.peeked) {
        const u32 k = tr.peeked;
        const TickSlot& tk = tr.slot[k];
        if (tk.quiet) continue;  // (a quiet tick was enqueued under the quiet rule already: its verdict cannot start it)
        const volatile u64* rows = tr.rows_host(k);
        for (u32 r = 0; r < tk.rows; ++r)
            if (rows[(size_t)r * 8 + 7] != tk.mark) return;
        std::atomic_thread_fence(std::memory_order_acquire);
        if (!needs_fixup(tr.reduce(k, nullptr)) && tk.epoch == h->mut_epoch) h->quiet_epoch = h->mut_epoch;
    }
}

int harvest_ticks(rio_gp* h) {
    TickRing& tr = h->ticks;
    const u32 n = tr.count(TickRing::Owner::ticks);
    if (!n) return RIO_GP_OK;
    chain_join(h);
    // When the last tick in flight is a quiet one, the verdict rows are the last thing every tick writes (a chained scan's
    // workgroups store theirs behind their adds; the k_resolve of a quiet tick on the main stream is its tick's last kernel) and
    // the last tick's kernels ran behind everything older: spin on the rows of EVERY tick in flight in mapped memory instead of
    // asking the runtime (launch + hipStreamSynchronize 12.6 us, launch + spin 7.3: tools/sync_probe.py) — the rows of two chained
    // links land in any order.  Not there after 50 ms: the stream is asked.
    bool landed = tr.slot[n - 1].quiet;
    for (u32 k = 0; landed && k < n; ++k) landed = spin_rows(tr.rows_host(k), tr.slot[k].rows, tr.slot[k].mark);
    if (!landed) HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (h->h_chain_err && *reinterpret_cast<volatile u32*>(h->h_chain_err)) {  // never seen; must not pass silently if it happens
        *h->h_chain_err = 0;
        tr.clear();
        return fail(h, RIO_GP_EUPSTREAM, "rio_gp_tick_wait: a chained scan gave up waiting for the previous tick's rows (tables are stale: reload them)");
    }
    for (u32 k = 0; k < n; ++k) {
        bool bad = false;
        DevStats v = tr.reduce(k, &bad);
        if (bad) {  // a verdict row without its tick's mark after the stream is done: never seen; must not pass silently
            tr.clear();
            return fail(h, RIO_GP_EUPSTREAM, "rio_gp_tick_wait: a tick's verdict rows are incomplete (tables are stale: reload them)");
        }
        const bool slow = needs_fixup(v);
        if (slow && tr.slot[k].quiet) {  // cannot happen (see mut_epoch); if it ever does it must not pass silently
            tr.clear();
            return fail(h, RIO_GP_EUPSTREAM, "rio_gp_tick_wait: a tick that was enqueued without its fix-up needed one (tables are stale: reload them)");
        }
        if (!slow && tr.slot[k].epoch == h->mut_epoch) h->quiet_epoch = h->mut_epoch;
        if (slow) fold_fx(h, TickRing::fx_slot(k), tr.slot[k].G, &v);
        rio_gp_stats st;
        fill_stats(v, h->n, &st);
        tr.done.push_back(st);
        h->last.record(v, slow, false);
    }
    tr.clear();
    return RIO_GP_OK;
}

// One committed tick, nothing waits on the host: k_scan (packing when the last known solve left few rows pending),
// k_resolve into this tick's verdict slot, the whole fix-up behind it (every fix-up kernel guards itself on the device),
// the publication (two pointer swaps, host side) and an asynchronous copy of the device accumulators into this tick's
// pinned record.  The result is the one rio_gp_tick computes; only the counters arrive later (rio_gp_tick_wait).
int tick_async_locked(rio_gp* h) {
    int rc = may_start(h, Client::tick_async);
    if (rc) return rc;
    if (h->ticks.full() && (rc = harvest_ticks(h))) return rc;
    peek_ticks(h);
    // nothing has changed since a tick that left every object placed: this one keeps every row, no fix-up can be needed
    // (lab builds: rio_gp_debug_set_speculate(always) keeps the launches)
    const bool quiet = h->quiet_epoch == h->mut_epoch && h->spec_mode != 1;
    // ... and it is one launch of the chained scan, a link of a run, on tables from overlap_min_rows rows on (below, the plain
    // k_scan + k_resolve on the main stream)
    const bool ov_can = quiet && h->stream == h->own_stream && h->n >= h->overlap_min_rows;
    if (ov_can && h->chain_seq >= 0x70000000u) {  // (sequence numbers compare by signed difference: start over long before they wrap)
        chain_join(h);
        (void)hipMemsetAsync(h->chain_flags, 0, (size_t)kMaxBlocks * kWaves * sizeof(u32), h->stream);
        h->chain_seq = 0;
    }
    // (chained: a pushed liveness bitmap rides in a scan that nothing behind it may overtake — a quiet tick has none; the chained
    //  scan addresses its columns by 32-bit byte offsets: tables below 2^30 rows, 4 GiB a column.  Not under
    //  RIO_GP_CFG_REF_SELF_ASSIGN: there a row whose affinity node is dead claims it again every tick — a quiet tick has
    //  claimants, and their cut needs k_resolve)
    const bool chained = ov_can && h->chain_mode != 2 && h->scan2 && h->chain_ok && !h->alive_dirty && h->cap_rows < ((size_t)1 << 30) &&
                         !h->sa && chain_begin(h);
    if (!chained) chain_join(h);
    InplaceGuard ipg{h};
    h->plan = hplan(h, h->n);
    const Table t = real_table(h);
    const NodeTab nt = scan_nodes(h);
    const u32 k = h->ticks.next_slot();
    use_fx_slot(h, TickRing::fx_slot(k));
    h->plan.mark = (1ull << 40) | ++h->wait_seq;  // column 7 of the verdict rows: peek_ticks knows them by it
    h->ticks.slot[k] = TickSlot{h->plan.G, chained ? h->plan.G : resolve_blocks(h->m), h->plan.mark, h->mut_epoch, quiet};
    u64* const rows = h->ticks.rows_dev(k);
    const SolveForm f = solve_form(h, true, false, quiet, chained);
    h->pending = chained ? enqueue_chained(h, t, nt, rows) : enqueue_scan_resolve(h, f, t, nt, rows);
    if (quiet) {
        // (the chained scan, or k_scan + k_resolve)
    } else if (f.compact) {
        enqueue_slow_packed(h, f, nt);
    } else {
        enqueue_slow(h, f, h->plan, t, nt, false);
    }
    if ((rc = commit_enqueue(h))) return rc;
    HIPCHK(h, hipGetLastError());
    h->ticks.pushed(TickRing::Owner::ticks);
    ipg.ok = true;
    return RIO_GP_OK;
}

// Micro-batch calls (one workgroup) end by storing their sequence number into a word of mapped pinned memory
// (signal_done, placement_kernels.hip); the host spins on it — launch + hipStreamSynchronize measured 12.6 us, launch +
// spin 7.3 us (tools/sync_probe.py).  A kernel that dies never writes the word: after ~50 ms the stream is asked.
u32 small_begin(rio_gp* h) {
    if (++h->small_seq == 0) h->small_seq = 1;
    return h->small_seq;
}
u32* small_done_dev(rio_gp* h) { return h->d_small + 5 * kSmallBatch; }
bool small_inline(SmallInline* inl, uint64_t n, const uint32_t* a, const uint32_t* b) {
    if (n > 4) return false;
    for (uint64_t k = 0; k < 4; ++k) {
        inl->a[k] = k < n ? a[k] : 0u;
        inl->b[k] = (k < n && b) ? b[k] : 0u;
    }
    return true;
}
int small_wait(rio_gp* h, u32 seq, volatile u32* w = nullptr) {
    if (!w) w = h->h_small + 5 * kSmallBatch;
    const auto t0 = std::chrono::steady_clock::now();
    for (u32 spins = 1; *w != seq; ++spins) {
        __builtin_ia32_pause();
        if ((spins & 0xFFFu) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) break;
    }
    if (*w == seq) {
        std::atomic_thread_fence(std::memory_order_acquire);
        return RIO_GP_OK;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (*w != seq) return fail(h, RIO_GP_EUPSTREAM, "micro-batch kernel left no completion word");
    return RIO_GP_OK;
}

int zero_stats(rio_gp* h) {
    HIPCHK(h, hipMemsetAsync(h->dstats, 0, sizeof(DevStats), h->stream));
    return RIO_GP_OK;
}

int read_stats(rio_gp* h) {
    HIPCHK(h, hipMemcpyAsync(h->h_stats, h->dstats, sizeof(DevStats), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    return RIO_GP_OK;
}

// A `_dev` batch of a per-row column writer: its kernel skips the entries it cannot take and counts them in dstats.
template <class Launch>
int dev_batch(rio_gp* h, const char* who, Launch&& launch) {
    int rc;
    if ((rc = zero_stats(h))) return rc;
    launch();
    if ((rc = read_stats(h))) return rc;
    if (h->h_stats[0].err) return fail(h, RIO_GP_EINVAL, std::string(who) + ": invalid entries were skipped");
    return RIO_GP_OK;
}

// A host batch of a per-row column writer on its way to the device: `first` (n words) into stage[0] and, if given, `second` (n
// elements of `elem` bytes) into stage[1]; d = the device pointers (null for n = 0: nothing is staged).  An index batch names
// its family's `begin`, and the order is the rule: a row-sharded handle is refused, then every index is checked against h->n,
// then the first-use allocation runs, so that a rejected call allocates nothing.  (A whole column, the merges', passes no
// `begin`: its caller has checked its rows and begun.)  staged_done is the other end.
struct Staged {
    const u32* first;
    const void* second;
};
int stage_batch(rio_gp* h, const char* who, int (*begin)(rio_gp*, const char*), uint64_t n, const uint32_t* first,
                const void* second, size_t elem, Staged& d) {
    int rc;
    d = {nullptr, nullptr};
    if (begin) {
        if ((rc = refuse_row_sharded(h, who))) return rc;
        for (uint64_t k = 0; k < n; ++k)
            if (first[k] >= h->n) return fail(h, RIO_GP_EINVAL, std::string(who) + ": object index out of range");
        if ((rc = begin(h, who))) return rc;
    }
    if (!n) return RIO_GP_OK;
    if ((rc = ensure(h, h->stage[0], n * sizeof(u32))) || (second && (rc = ensure(h, h->stage[1], n * elem)))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->stage[0].p, first, n * sizeof(u32), hipMemcpyHostToDevice, h->stream));
    if (second) HIPCHK(h, hipMemcpyAsync(h->stage[1].p, second, n * elem, hipMemcpyHostToDevice, h->stream));
    d = {(const u32*)h->stage[0].p, second ? h->stage[1].p : nullptr};
    return RIO_GP_OK;
}
int staged_done(rio_gp* h) {
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));  // the caller's arrays are read until here
    return RIO_GP_OK;
}

}  // namespace

extern "C" {

uint32_t rio_gp_abi_version(void) { return RIO_GP_ABI_VERSION; }

const char* rio_gp_last_error(rio_gp_t* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

const char* rio_gp_backend(rio_gp_t*) { return "hip:gfx950"; }

int rio_gp_create(const rio_gp_cfg* cfg, rio_gp_t** out) {
    if (out) *out = nullptr;
    if (!cfg || !out || cfg->struct_size != sizeof(rio_gp_cfg)) {
        g_create_error = "rio_gp_create: bad cfg (struct_size mismatch)";
        return RIO_GP_EINVAL;
    }
    if (cfg->max_objects > RIO_GP_MAX_OBJECTS || cfg->max_nodes > RIO_GP_MAX_NODES) {
        g_create_error = "rio_gp_create: max_objects/max_nodes above the solver limits";
        return RIO_GP_EINVAL;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) {
        g_create_error = std::string("rio_gp_create: no usable HIP device (") +
                         (e != hipSuccess ? hipGetErrorString(e) : "device ordinal out of range") +
                         "); there is no CPU fallback";
        return RIO_GP_ENODEV;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_error = std::string("rio_gp_create: device is not gfx950 (MI355X): ") + prop.gcnArchName;
        return RIO_GP_ENODEV;
    }
    rio_gp* h = new rio_gp();
    h->device = cfg->device;
    h->lifecycle = (cfg->flags & RIO_GP_CFG_ROW_LIFECYCLE) != 0;
    h->sa = (cfg->flags & RIO_GP_CFG_REF_SELF_ASSIGN) ? 1u : 0u;
    h->cap_obj = cfg->max_objects;
    h->cap_rows = ((cfg->max_objects + kTile - 1) / kTile) * kTile + 8 * kTile;  // k_scan prefetches past the end
    h->cap_nodes = cfg->max_nodes ? cfg->max_nodes : 1;
    h->rounds = cfg->spill_rounds ? cfg->spill_rounds : 2;
    if (h->rounds > kFillRounds) {
        g_create_error = "rio_gp_create: spill_rounds above the solver limit (8)";
        delete h;
        return RIO_GP_EINVAL;
    }
    int rc = RIO_GP_OK;
    auto bail = [&](int code) {
        g_create_error = h->err;
        rio_gp_destroy(h);
        return code;
    };
    if (hipSetDevice(h->device) != hipSuccess) { h->err = "hipSetDevice failed"; return bail(RIO_GP_EUPSTREAM); }
    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess || !(h->stream = h->own_stream) ||
        hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) {
        h->err = "stream/event creation failed";
        return bail(RIO_GP_EUPSTREAM);
    }
    if (hipStreamCreateWithFlags(&h->scan2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_run, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        if (h->scan2) (void)hipStreamDestroy(h->scan2);
        h->scan2 = nullptr;  // (no chain: everything else works)
    }
    h->chain_ok = h->scan2 && scan_chain_fits((u32)h->cap_nodes);
#ifdef RIO_GP_LAB
    if (const char* e = getenv("RIO_GP_CHAIN_DIAG")) h->chain_diag = atoi(e);  // (1: PMC passes only — the waits are what makes the chain correct)
    if (const char* e = getenv("RIO_GP_OVERLAP_MIN_ROWS")) h->overlap_min_rows = strtoull(e, nullptr, 10);
#endif
    const size_t R = h->cap_rows, M = h->cap_nodes, W = (size_t)kMaxBlocks * kWaves;
    // the balanced pack columns (k_rebal) have uniform wave ranges: up to a tile per wave range more than the table; the
    // all-NONE column stands in for their `cur` column as well
    const size_t R2 = std::max((size_t)rebal_rows(h->cap_obj) + 8 * kTile, R);
#define A(ptr, cnt) if ((rc = dalloc(h, &(ptr), (cnt))) != RIO_GP_OK) return bail(rc)
    A(h->assign[0], R); A(h->assign[1], R); A(h->load, R); A(h->aff, R); A(h->pos, R2);
    h->used_slot_words = (h->chain_ok ? (size_t)kChainReps : 1) * M;
    A(h->cap, M); A(h->used_ring, kUsedRing * h->used_slot_words); A(h->alive_bits, (M + 31) / 32 + 4); A(h->dead_bits, (M + 31) / 32 + 4);
    A(h->alive_bytes, M);
    A(h->sb.H, (size_t)((M + 7) / 8) * kMaxBlocks * 16); A(h->sb.blkstat, (size_t)kMaxBlocks * 4);
    A(h->sb.partial, (size_t)resolve_blocks((u32)M) * 8 + 8);
    A(h->sb.wsp_sum[0], W); A(h->sb.wsp_sum[1], W); A(h->sb.wsp_cnt[0], W); A(h->sb.wsp_cnt[1], W);
    A(h->sb.bsp_sum[0], (size_t)kMaxBlocks); A(h->sb.bsp_sum[1], (size_t)kMaxBlocks); A(h->sb.bsp_cnt[0], (size_t)kMaxBlocks); A(h->sb.bsp_cnt[1], (size_t)kMaxBlocks);
    A(h->sb.used_kept, M); A(h->sb.claim_tot, M); A(h->sb.cutblk, M); A(h->sb.budget, M);
    A(h->sb.admpre, M); A(h->sb.cutidx, M); A(h->dstats, 1); A(h->fx_dev, (size_t)kMaxBlocks * 8);
    A(h->sb.R, (size_t)kMaxBlocks); A(h->sb.RP, (size_t)kMaxBlocks * resolve_blocks((u32)M)); A(h->D, (size_t)kFillRounds * M);
    A(h->pk.idx, R); A(h->pk.load, R); A(h->pk.aff, R); A(h->pk.next, R); A(h->pk.wcnt, W);
    A(h->pk2.idx, R2); A(h->pk2.load, R2); A(h->pk2.aff, R2); A(h->pk2.next, R2); A(h->pk2.wcnt, W);
    A(h->Tg, M * kWaves);
    A(h->chain_flags, W);
    A(h->sh_lkept, M); A(h->sh_lclaim, M); A(h->sh_lcur, M); A(h->sh_lcutblk, M); A(h->sh_lcutidx, M);
    A(h->sh_gprev, M); A(h->sh_gfinal, M); A(h->sh_rank_base, 2); A(h->sh_verdict, 8); A(h->sh_forced, (M + 31) / 32 + 4);
#undef A
    h->used.init(h, h->used_ring);
    h->sb.used_cur = h->used_ring + h->used_slot_words;
    h->sb.stats = h->dstats;
    if (hipHostMalloc(reinterpret_cast<void**>(&h->h_stats), sizeof(DevStats) * kRing, hipHostMallocMapped) !=
        hipSuccess) {
        h->err = "hipHostMalloc failed";
        return bail(RIO_GP_ENOMEM);
    }
    if (hipHostMalloc(reinterpret_cast<void**>(&h->h_chain_err), 64, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_chain_err), h->h_chain_err, 0) != hipSuccess) {
        h->err = "hipHostMalloc(chain error word) failed";
        return bail(RIO_GP_ENOMEM);
    }
    memset(h->h_chain_err, 0, 64);
    h->slot_rows = std::max<size_t>(resolve_blocks(h->cap_nodes), kMaxBlocks);  // (k_resolve's rows, or a chained scan's: one per workgroup)
    if (hipHostMalloc(reinterpret_cast<void**>(&h->h_slots), (size_t)2 * kRing * h->slot_rows * 8 * sizeof(u64),
                      hipHostMallocMapped) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&h->h_fx), (size_t)(1 + kRing) * kMaxBlocks * 8 * sizeof(u64), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_fx), h->h_fx, 0) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_slots), h->h_slots, 0) != hipSuccess) {
        h->err = "hipHostMalloc(mapped verdict slots) failed";
        return bail(RIO_GP_ENOMEM);
    }
    memset(h->h_slots, 0, (size_t)2 * kRing * h->slot_rows * 8 * sizeof(u64));
    h->solves.init(h->h_slots, h->slot_rows * 8);
    h->ticks.init(h->h_slots, h->d_slots, h->slot_rows * 8);
    memset(h->h_fx, 0, (size_t)(1 + kRing) * kMaxBlocks * 8 * sizeof(u64));
    h->cs_words = (((size_t)h->cap_nodes + 31) / 32 + 8 + 1) & ~(size_t)1;  // bitmap words, then the u64 count (8 B aligned)
    if (hipHostMalloc(reinterpret_cast<void**>(&h->h_cs), (h->cs_words + 4) * sizeof(u32), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_cs), h->h_cs, 0) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&h->cs_cnt), 9 * 16 * sizeof(u64)) != hipSuccess ||  // k_clean: total + 8 group counters, a line each
        hipMalloc(reinterpret_cast<void**>(&h->cs_ticket), sizeof(unsigned int)) != hipSuccess ||
        hipMemset(h->cs_cnt, 0, 9 * 16 * sizeof(u64)) != hipSuccess || hipMemset(h->cs_ticket, 0, sizeof(unsigned int)) != hipSuccess) {
        h->err = "clean_server staging allocation failed";
        return bail(RIO_GP_ENOMEM);
    }
    h->allocs.push_back(h->cs_cnt);
    h->allocs.push_back(h->cs_ticket);
    h->alive_slot_words = (((u32)h->cap_nodes + 31) / 32 + 4 + 31) & ~31u;
    if (hipHostMalloc(reinterpret_cast<void**>(&h->h_alive_ring), (size_t)kAliveSlots * h->alive_slot_words * sizeof(u32),
                      hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_alive_ring), h->h_alive_ring, 0) != hipSuccess) {
        h->err = "hipHostMalloc(mapped liveness ring) failed";
        (void)hipGetLastError();
        rio_gp_destroy(h);
        return RIO_GP_EUPSTREAM;
    }
    if (hipHostMalloc(reinterpret_cast<void**>(&h->h_small), (size_t)6 * kSmallBatch * sizeof(u32), hipHostMallocMapped) !=
            hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_small), h->h_small, 0) != hipSuccess) {
        h->err = "hipHostMalloc(mapped micro-batch staging) failed";
        return bail(RIO_GP_ENOMEM);
    }
    memset(h->h_small, 0, (size_t)6 * kSmallBatch * sizeof(u32));  // completion word: 0 = no call yet (sequence numbers start at 1)
    if (hipHostMalloc(reinterpret_cast<void**>(&h->h_mid), (size_t)4 * kMidBatch * sizeof(u32), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_mid), h->h_mid, 0) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&h->mid_ticket), sizeof(unsigned int)) != hipSuccess ||
        hipMemset(h->mid_ticket, 0, sizeof(unsigned int)) != hipSuccess) {
        h->err = "hipHostMalloc(mapped medium-batch staging) failed";
        return bail(RIO_GP_ENOMEM);
    }
    h->allocs.push_back(h->mid_ticket);
    if (hipHostMalloc(reinterpret_cast<void**>(&h->h_req), (size_t)4 * kReqBatch * sizeof(u32), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_req), h->h_req, 0) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&h->pp_bad), 64) != hipSuccess || hipMemset(h->pp_bad, 0, 64) != hipSuccess) {
        h->err = "hipHostMalloc(mapped request staging) failed";
        return bail(RIO_GP_ENOMEM);
    }
    h->allocs.push_back(h->pp_bad);
    if ((rc = dalloc(h, &h->pp_claim, (size_t)h->cap_nodes + 1)) != RIO_GP_OK) return bail(rc);
    if (hipMalloc(&h->pp_stage, pp_stage_bytes()) != hipSuccess || hipMemset(h->pp_stage, 0, pp_stage_bytes()) != hipSuccess) {
        h->err = "request staging allocation failed";
        return bail(RIO_GP_ENOMEM);
    }
    h->allocs.push_back(h->pp_stage);
    // every row starts unplaced; the position scratch is all-ones between calls
    launch_fill_u32(h->assign[0], R, kNone, h->stream);
    launch_fill_u32(h->assign[1], R, kNone, h->stream);
    launch_fill_u32(h->pos, R2, kNone, h->stream);
    launch_fill_u32(h->load, R, 0, h->stream);
    launch_fill_u32(h->aff, R, kNone, h->stream);
    (void)hipMemsetAsync(h->used_ring, 0, kUsedRing * h->used_slot_words * sizeof(u64), h->stream);
    (void)hipMemsetAsync(h->alive_bits, 0, ((M + 31) / 32 + 4) * sizeof(u32), h->stream);
    (void)hipMemsetAsync(h->dstats, 0, sizeof(DevStats), h->stream);
    (void)hipMemsetAsync(h->D, 0, (size_t)kFillRounds * M * sizeof(u64), h->stream);
    (void)hipMemsetAsync(h->sb.R, 0, (size_t)kMaxBlocks * sizeof(u64), h->stream);
    (void)hipMemsetAsync(h->chain_flags, 0, W * sizeof(u32), h->stream);
    if (hipStreamSynchronize(h->stream) != hipSuccess || hipGetLastError() != hipSuccess) {
        h->err = "initial fill failed (no gfx950 code object loaded?)";
        return bail(RIO_GP_EUPSTREAM);
    }
    *out = h;
    return RIO_GP_OK;
}

void rio_gp_destroy(rio_gp_t* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->own_stream && h->own_stream != h->stream) (void)hipStreamSynchronize(h->own_stream);
    if (h->scan2) (void)hipStreamSynchronize(h->scan2);  // (a chained run's links on the second stream, before anything is freed)
    shard_comm_free(h);
    for (void* p : h->allocs) (void)hipFree(p);
    for (auto& b : h->vt) if (b.p) (void)hipFree(b.p);
    for (auto& b : h->stage) if (b.p) (void)hipFree(b.p);
    for (auto& b : h->rq) if (b.p) (void)hipFree(b.p);
    if (h->vrec.p) (void)hipFree(h->vrec.p);
    if (h->part.p) (void)hipFree(h->part.p);
    if (h->ni_rows.p) (void)hipFree(h->ni_rows.p);
    for (DevBuf* b : {&h->sh_nodes, &h->sh_mat, &h->sh_tile, &h->sh_chunk, &h->sh_pk, &h->sh_mv, &h->sh_sel})
        if (b->p) (void)hipFree(b->p);
    if (h->chg_stage.p) (void)hipFree(h->chg_stage.p);
    if (h->cls_cells.p) (void)hipFree(h->cls_cells.p);
    if (h->h_cls) (void)hipHostFree(h->h_cls);
    if (h->h_ni) (void)hipHostFree(h->h_ni);
    if (h->h_chg) (void)hipHostFree(h->h_chg);
    if (h->h_top) (void)hipHostFree(h->h_top);
    if (h->h_stats) (void)hipHostFree(h->h_stats);
    if (h->h_chain_err) (void)hipHostFree(h->h_chain_err);
    if (h->h_slots) (void)hipHostFree(h->h_slots);
    if (h->h_fx) (void)hipHostFree(h->h_fx);
    if (h->h_small) (void)hipHostFree(h->h_small);
    if (h->h_mid) (void)hipHostFree(h->h_mid);
    if (h->h_req) (void)hipHostFree(h->h_req);
    if (h->h_cs) (void)hipHostFree(h->h_cs);
    if (h->h_alive_ring) (void)hipHostFree(h->h_alive_ring);
    chain_end(h);
    if (h->scan2) { (void)hipStreamSynchronize(h->scan2); (void)hipStreamDestroy(h->scan2); }
    if (h->ev_run) (void)hipEventDestroy(h->ev_run);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->ev2) (void)hipEventDestroy(h->ev2);
    if (h->ev3) (void)hipEventDestroy(h->ev3);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
}

int rio_gp_set_flags(rio_gp_t* h, uint32_t flags) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    const uint32_t fixed = h->lifecycle ? RIO_GP_CFG_ROW_LIFECYCLE : 0u;
    if ((flags & ~RIO_GP_CFG_REF_SELF_ASSIGN) != fixed) return fail(h, RIO_GP_EINVAL, "rio_gp_set_flags: only RIO_GP_CFG_REF_SELF_ASSIGN may change");
    const u32 sa = (flags & RIO_GP_CFG_REF_SELF_ASSIGN) ? 1u : 0u;
    if (sa && (h->p2p || h->sc)) return fail(h, RIO_GP_EINVAL, "rio_gp_set_flags: row-sharded handles do not implement RIO_GP_CFG_REF_SELF_ASSIGN");
    if (sa != h->sa) { h->sa = sa; inputs_changed(h); }
    return RIO_GP_OK;
}

int rio_gp_sync(rio_gp_t* h) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RIO_GP_OK;
}

uint64_t rio_gp_num_objects(rio_gp_t* h) { return h ? h->n : 0; }
uint32_t rio_gp_num_nodes(rio_gp_t* h) { return h ? h->m : 0; }

// ---- node table ---------------------------------------------------------------------------

int rio_gp_set_nodes(rio_gp_t* h, uint32_t m, const uint64_t* cap, const uint8_t* alive) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    if (m > h->cap_nodes) return fail(h, RIO_GP_EINVAL, "rio_gp_set_nodes: m exceeds max_nodes");
    HIPCHK(h, hipSetDevice(h->device));
    std::vector<u64> c(m ? m : 1, RIO_GP_CAP_INF);
    if (cap) memcpy(c.data(), cap, (size_t)m * sizeof(u64));
    h->h_alive.assign(m, 1);
    if (alive) for (uint32_t j = 0; j < m; ++j) h->h_alive[j] = alive[j] ? 1 : 0;
    if (m) {
        HIPCHK(h, hipMemcpyAsync(h->cap, c.data(), (size_t)m * sizeof(u64), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->alive_bytes, h->h_alive.data(), m, hipMemcpyHostToDevice, h->stream));
    }
    launch_pack_alive(h->alive_bytes, m, h->alive_bits, h->stream);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->alive_dirty = false;
    h->all_alive = true;
    for (uint32_t j = 0; j < m; ++j) h->all_alive = h->all_alive && h->h_alive[j];
    if (m != h->m) h->used.invalidate();
    h->m = m;
    inputs_changed(h);
    return RIO_GP_OK;
}

// Liveness push without a host wait and without a launch: the bitmap is packed into a ring slot of mapped pinned memory;
// the next whole-table scan reads it from there (scan_nodes), anything else that needs the device array first makes
// flush_alive deliver it in the arguments of one tiny kernel.
static int push_alive_bits(rio_gp* h) {
    static_assert(RIO_GP_MAX_NODES <= 256 * 32, "WordPack holds RIO_GP_MAX_NODES bits");
    const u32 words = (h->m + 31) / 32;
    if (!h->alive_dirty) h->alive_slot = (h->alive_slot + 1) % kAliveSlots;  // (an unconsumed push is simply overwritten)
    u32* w = h->h_alive_ring + (size_t)h->alive_slot * h->alive_slot_words;
    memset(w, 0, sizeof(u32) * (words ? words : 1));
    h->all_alive = true;
    for (uint32_t j = 0; j < h->m; ++j) {
        if (h->h_alive[j]) w[j >> 5] |= 1u << (j & 31);
        else h->all_alive = false;
    }
    std::atomic_thread_fence(std::memory_order_release);
    h->alive_dirty = true;
    inputs_changed(h);
    return RIO_GP_OK;
}

int rio_gp_set_alive_all(rio_gp_t* h, uint32_t m, const uint8_t* alive) {
    if (!h || !alive) return RIO_GP_EINVAL;
    Locked g(h);
    if (m != h->m) return fail(h, RIO_GP_EINVAL, "rio_gp_set_alive_all: m differs from the node table");
    HIPCHK(h, hipSetDevice(h->device));
    for (uint32_t j = 0; j < m; ++j) h->h_alive[j] = alive[j] ? 1 : 0;
    return push_alive_bits(h);
}

int rio_gp_set_alive(rio_gp_t* h, uint32_t node, uint8_t alive) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    if (node >= h->m) return fail(h, RIO_GP_EINVAL, "rio_gp_set_alive: node out of range");
    HIPCHK(h, hipSetDevice(h->device));
    h->h_alive[node] = alive ? 1 : 0;
    return push_alive_bits(h);
}

int rio_gp_get_nodes(rio_gp_t* h, uint32_t m, uint64_t* cap, uint8_t* alive, uint64_t* used) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    if (m != h->m) return fail(h, RIO_GP_EINVAL, "rio_gp_get_nodes: m differs from the node table");
    HIPCHK(h, hipSetDevice(h->device));
    const u64* const d_used = used ? h->used.ensure() : nullptr;
    if (cap && m) HIPCHK(h, hipMemcpyAsync(cap, h->cap, (size_t)m * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    if (used && m) HIPCHK(h, hipMemcpyAsync(used, d_used, (size_t)m * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (alive) memcpy(alive, h->h_alive.data(), m);
    return RIO_GP_OK;
}

// ---- object table -------------------------------------------------------------------------

static int set_objects_impl(rio_gp_t* h, uint64_t n, const uint32_t* load, const uint32_t* aff, hipMemcpyKind kind) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    if (n > h->cap_obj) return fail(h, RIO_GP_EINVAL, "rio_gp_set_objects: n exceeds max_objects");
    HIPCHK(h, hipSetDevice(h->device));
    if (load) { if (n) HIPCHK(h, hipMemcpyAsync(h->load, load, n * sizeof(u32), kind, h->stream)); }
    else launch_fill_u32(h->load, n, 1u, h->stream);
    if (aff) { if (n) HIPCHK(h, hipMemcpyAsync(h->aff, aff, n * sizeof(u32), kind, h->stream)); }
    else launch_fill_u32(h->aff, n, h->lifecycle ? kAffInactive : kNone, h->stream);
    launch_fill_u32(h->assign[h->cur], h->cap_rows, kNone, h->stream);
    HIPCHK(h, hipMemsetAsync(h->used.storage(), 0, (size_t)h->cap_nodes * sizeof(u64), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->n = n;
    h->n_hi = std::max<u64>(h->n_hi, n);
    h->used.rebuilt();  // (all zero: no row is placed)
    inputs_changed(h);
    return RIO_GP_OK;
}
int rio_gp_set_objects(rio_gp_t* h, uint64_t n, const uint32_t* load, const uint32_t* aff) {
    return set_objects_impl(h, n, load, aff, hipMemcpyHostToDevice);
}
int rio_gp_set_objects_dev(rio_gp_t* h, uint64_t n, const uint32_t* d_load, const uint32_t* d_aff) {
    return set_objects_impl(h, n, d_load, d_aff, hipMemcpyDeviceToDevice);
}

static int set_assign_impl(rio_gp_t* h, uint64_t n, const uint32_t* assign, hipMemcpyKind kind) {
    if (!h || !assign) return RIO_GP_EINVAL;
    Locked g(h);
    if (n != h->n) return fail(h, RIO_GP_EINVAL, "rio_gp_set_assign: n differs from the object table");
    if (kind == hipMemcpyHostToDevice)
        for (uint64_t i = 0; i < n; ++i)
            if (assign[i] != RIO_GP_NONE && assign[i] >= h->m)
                return fail(h, RIO_GP_EINVAL, "rio_gp_set_assign: node id out of range");
    HIPCHK(h, hipSetDevice(h->device));
    if (n) HIPCHK(h, hipMemcpyAsync(h->assign[h->cur], assign, n * sizeof(u32), kind, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->used.invalidate();
    inputs_changed(h);
    return RIO_GP_OK;
}
int rio_gp_set_assign(rio_gp_t* h, uint64_t n, const uint32_t* a) { return set_assign_impl(h, n, a, hipMemcpyHostToDevice); }
int rio_gp_set_assign_dev(rio_gp_t* h, uint64_t n, const uint32_t* a) { return set_assign_impl(h, n, a, hipMemcpyDeviceToDevice); }

int rio_gp_get_assign(rio_gp_t* h, uint64_t n, uint32_t* out) {
    if (!h || !out) return RIO_GP_EINVAL;
    Locked g(h);
    if (n != h->n) return fail(h, RIO_GP_EINVAL, "rio_gp_get_assign: n differs from the object table");
    HIPCHK(h, hipSetDevice(h->device));
    if (n) HIPCHK(h, hipMemcpyAsync(out, h->assign[h->cur], n * sizeof(u32), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RIO_GP_OK;
}
int rio_gp_get_solved(rio_gp_t* h, uint64_t n, uint32_t* out) {
    if (!h || !out) return RIO_GP_EINVAL;
    Locked g(h);
    if (n != h->n || !h->pending.have) return fail(h, RIO_GP_EINVAL, "rio_gp_get_solved: no solve / size mismatch");
    HIPCHK(h, hipSetDevice(h->device));
    if (n) HIPCHK(h, hipMemcpyAsync(out, h->assign[h->cur ^ 1], n * sizeof(u32), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RIO_GP_OK;
}
int rio_gp_get_objects(rio_gp_t* h, uint64_t n, uint32_t* out_load, uint32_t* out_aff) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    if (n != h->n) return fail(h, RIO_GP_EINVAL, "rio_gp_get_objects: n differs from the object table");
    HIPCHK(h, hipSetDevice(h->device));
    if (n && out_load) HIPCHK(h, hipMemcpyAsync(out_load, h->load, n * sizeof(u32), hipMemcpyDeviceToHost, h->stream));
    if (n && out_aff) HIPCHK(h, hipMemcpyAsync(out_aff, h->aff, n * sizeof(u32), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RIO_GP_OK;
}
int rio_gp_set_object_attrs(rio_gp_t* h, uint64_t n, const uint32_t* idx, const uint32_t* load, const uint32_t* aff) {
    if (!h || (n && !idx)) return RIO_GP_EINVAL;
    Locked g(h);
    for (uint64_t k = 0; k < n; ++k)
        if (idx[k] >= h->n) return fail(h, RIO_GP_EINVAL, "rio_gp_set_object_attrs: object index out of range");
    if (!n || (!load && !aff)) return RIO_GP_OK;
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    for (int q = 0; q < 3; ++q)
        if ((rc = ensure(h, h->stage[q], n * sizeof(u32)))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->stage[0].p, idx, n * sizeof(u32), hipMemcpyHostToDevice, h->stream));
    if (load) HIPCHK(h, hipMemcpyAsync(h->stage[1].p, load, n * sizeof(u32), hipMemcpyHostToDevice, h->stream));
    if (aff) HIPCHK(h, hipMemcpyAsync(h->stage[2].p, aff, n * sizeof(u32), hipMemcpyHostToDevice, h->stream));
    if ((rc = zero_stats(h))) return rc;
    launch_set_attrs(h->load, h->aff, h->n, (const u32*)h->stage[0].p, load ? (const u32*)h->stage[1].p : nullptr,
                     aff ? (const u32*)h->stage[2].p : nullptr, n, h->dstats, h->stream);
    if (load) h->used.invalidate();
    inputs_changed(h);
    return read_stats(h);
}

int rio_gp_count_placed(rio_gp_t* h, uint64_t* out) {
    if (!h || !out) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipSetDevice(h->device));
    int rc = zero_stats(h);
    if (rc) return rc;
    launch_count_placed(h->assign[h->cur], h->n, h->dstats, h->stream);
    if ((rc = read_stats(h))) return rc;
    *out = h->h_stats[0].evicted_clean;
    return RIO_GP_OK;
}

// ---- reverse placement index --------------------------------------------------------------

// The scratch of rio_gp_rows_on_nodes, on first use: kNiMaxEntries u32 of matrix (8 MiB), kNiMaxParts + 1 chunk sums, the map (32 KiB),
// RIO_GP_MAX_NODES + 1 offsets (64 KiB), and 2 * RIO_GP_MAX_NODES + 2 words of mapped pinned memory.  Fixed sizes: they hold for every (n, m).
static int ni_scratch(rio_gp* h) {
    if (h->ni_cnt) return RIO_GP_OK;
    int rc;
    if ((rc = dalloc(h, &h->ni_part, kNiMaxParts + 1)) || (rc = dalloc(h, &h->ni_map, RIO_GP_MAX_NODES)) ||
        (rc = dalloc(h, &h->ni_off, RIO_GP_MAX_NODES + 1)))
        return rc;
    if (!h->h_ni) {
        if (hipHostMalloc(reinterpret_cast<void**>(&h->h_ni), (2 * RIO_GP_MAX_NODES + 2) * sizeof(u32), hipHostMallocMapped) !=
                hipSuccess ||
            hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_ni), h->h_ni, 0) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, RIO_GP_ENOMEM, "hipHostMalloc(node index map) failed");
        }
    }
    if ((rc = dalloc(h, &h->ni_cnt, kNiMaxEntries))) return rc;  // (last: it is what says the scratch is complete)
    if (!h->ni_part || !h->ni_map || !h->ni_off || !h->d_ni) {
        h->ni_cnt = nullptr;
        return fail(h, RIO_GP_ENOMEM, "rio_gp_rows_on_nodes: scratch allocation failed");
    }
    return RIO_GP_OK;
}

// Count (and scan) the selected rows of the committed column; offsets into `off` (device).  Leaves the plan in *p (p->s == 0 or
// p->n == 0: nothing was launched, the offsets are zeros).
// (the scratch must exist: ni_scratch first — `off` may be h->ni_off)
static int ni_count_scan(rio_gp* h, const uint64_t* node_bitmap, u64* off, NiPlan* p) {
    const u32 m = h->m;
    u32* map = h->h_ni;
    u32* rank = h->h_ni + RIO_GP_MAX_NODES;
    u32 s = 0, single = 0;
    for (u32 j = 0; j < m; ++j) {
        rank[j] = s;
        const bool sel = !node_bitmap || ((node_bitmap[j >> 6] >> (j & 63)) & 1ull);
        map[j] = sel ? s : kNone;
        if (sel) { single = j; ++s; }
    }
    rank[m] = s;
    const u32 mode = s == m ? kNiIdentity : s == 1 ? kNiSingle : kNiMap;
    *p = ni_plan(h->n, m, s, mode, single, h->ni_force_tile);
    if (s == 0 || h->n == 0) {  // nothing to list: the offsets are zeros
        p->s = 0;
        launch_fill_u32(reinterpret_cast<u32*>(off), 2 * ((u64)m + 1), 0, h->stream);
        HIPCHK(h, hipGetLastError());
        return RIO_GP_OK;
    }
    if (mode == kNiMap) HIPCHK(h, hipMemcpyAsync(h->ni_map, map, (size_t)m * sizeof(u32), hipMemcpyHostToDevice, h->stream));
    launch_ni_count(h->assign[h->cur], *p, h->ni_map, h->ni_cnt, h->stream);
    launch_ni_scan(h->ni_cnt, *p, h->ni_part, h->d_ni + RIO_GP_MAX_NODES, off, h->stream);
    HIPCHK(h, hipGetLastError());
    return RIO_GP_OK;
}

static int ni_erange(rio_gp* h, u64 total, u64 cap) {
    return fail(h, RIO_GP_ERANGE, "rio_gp_rows_on_nodes: " + std::to_string(total) + " rows do not fit rows_cap = " + std::to_string(cap));
}

// Read-only: nothing here changes the tables, the epochs, `used` or the chain; it reads the column rio_gp_get_assign reads.
int rio_gp_rows_on_nodes(rio_gp_t* h, const uint64_t* node_bitmap, uint64_t* out_offsets, uint32_t* out_rows, uint64_t rows_cap,
                         uint64_t* n_rows) {
    if (!h || !out_offsets || !n_rows || (!out_rows && rows_cap)) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipSetDevice(h->device));
    NiPlan p;
    int rc;
    if ((rc = ni_scratch(h)) || (rc = ni_count_scan(h, node_bitmap, h->ni_off, &p))) return rc;
    const u32 m = h->m;
    HIPCHK(h, hipMemcpyAsync(out_offsets, h->ni_off, (size_t)(m + 1) * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const u64 total = out_offsets[m];
    *n_rows = total;
    if (!out_rows || total == 0) return RIO_GP_OK;  // counts only (or nothing to list)
    if (total > rows_cap) return ni_erange(h, total, rows_cap);
    if ((rc = ensure(h, h->ni_rows, total * sizeof(u32)))) return rc;
    launch_ni_scatter(h->assign[h->cur], p, h->ni_map, h->ni_cnt, h->ni_part, total, (u32*)h->ni_rows.p, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out_rows, h->ni_rows.p, total * sizeof(u32), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RIO_GP_OK;
}

int rio_gp_rows_on_nodes_dev(rio_gp_t* h, const uint64_t* node_bitmap, uint64_t* d_offsets, uint32_t* d_rows, uint64_t rows_cap,
                             uint64_t* n_rows) {
    if (!h || !d_offsets || !n_rows || (!d_rows && rows_cap)) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipSetDevice(h->device));
    NiPlan p;
    int rc;
    if ((rc = ni_scratch(h)) || (rc = ni_count_scan(h, node_bitmap, reinterpret_cast<u64*>(d_offsets), &p))) return rc;
    u32* h_total = h->h_ni + 2 * RIO_GP_MAX_NODES + 1;
    *h_total = 0;
    if (p.s) {
        // the scatter checks the total against rows_cap on the device: one wait for the whole call
        if (d_rows) launch_ni_scatter(h->assign[h->cur], p, h->ni_map, h->ni_cnt, h->ni_part, rows_cap, d_rows, h->stream);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(h_total, ni_total(p, h->ni_part), sizeof(u32), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const u64 total = *h_total;
    *n_rows = total;
    if (d_rows && total > rows_cap) return ni_erange(h, total, rows_cap);
    return RIO_GP_OK;
}

// ---- bounded rebalance ----------------------------------------------------------------------

// struct_size is the ABI guard of rio_gp_rebalance_cfg: the struct as it was before `order` (up to `target`) means row order and
// its later fields are not read; the whole struct carries an order.  NULL, or what is wrong with the cfg.
constexpr size_t kRebalanceCfgV1 = offsetof(rio_gp_rebalance_cfg, order);
static const char* rebalance_cfg_order(const rio_gp_rebalance_cfg* cfg, u32* order) {
    *order = RIO_GP_REBALANCE_ROW_ORDER;
    if (!cfg) return "cfg missing";
    if (cfg->struct_size == kRebalanceCfgV1) return nullptr;
    if (cfg->struct_size != sizeof(rio_gp_rebalance_cfg)) return "struct_size differs";
    if (cfg->order != RIO_GP_REBALANCE_ROW_ORDER && cfg->order != RIO_GP_REBALANCE_BY_LOAD) return "unknown order";
    if (cfg->reserved != 0) return "reserved is not 0";
    *order = cfg->order;
    return nullptr;
}

// rio_gp_rebalance[_dev] (rebalance_locked) and the rio_gp_shard_rebalance_* session sequence the same phases, each written
// once: rb_cfg (the cfg checks; rounds and budget), rb_surplus (R1: the cuts and the surplus per tile), rb_pack (R2, into an
// RbPacked), rb_finish (R4, the column, the moves, the read-back, the stats).  R0 and a round of R3 are one launcher call each.

// The node scratch of both forms: the only carving of h->sh_nodes.  Every array is rewritten by the call or session that reads
// it, so the two forms may alternate on one handle.  lu, tdev, base, live, info and maxl are the session's alone: the single
// form keeps its `used` in h->used.storage() and decides on the host what k_shrb_import_* decides from the others.
namespace {
struct RbBufs {
    u64 *pin, *tgt, *slot_free, *C, *acc, *lu, *tdev, *base;
    u32 *map, *slot_node, *cut, *ord, *cntp, *live, *info, *maxl, *thr, *pre;
};
constexpr int kRbPend = 6;  // acc[6], acc[7]: rows / load pending on all ranks (k_shrb_merge)
RbBufs rb_bufs(rio_gp* h) {
    const size_t M = h->cap_nodes;
    RbBufs b;
    b.pin = (u64*)h->sh_nodes.p;
    b.tgt = b.pin + M;  // (0 on dead nodes)
    b.slot_free = b.tgt + M;
    b.C = b.slot_free + M;
    b.acc = b.C + M + 1;
    b.lu = b.acc + kShAcc;
    b.tdev = b.lu + M;
    b.base = b.tdev + M;
    b.map = (u32*)(b.base + 1);
    b.slot_node = b.map + M;
    b.cut = b.slot_node + M;
    b.ord = b.cut + M;
    b.cntp = b.ord + M;
    b.live = b.cntp + 4;
    b.info = b.live + M;
    // the load-ordered cut: info has one more word (kShrbMaxLoad); this rank's largest load, the threshold per node, the digits
    // chosen so far per slot
    b.maxl = b.info + kShrbInfo + 1;
    b.thr = b.maxl + 1;
    b.pre = b.thr + M;
    return b;
}
int rb_ensure(rio_gp* h) {
    const size_t M = h->cap_nodes;
    return ensure(h, h->sh_nodes, (6 * M + 2 + kShAcc) * sizeof(u64) + (7 * M + 4 + kShrbInfo + 2) * sizeof(u32));
}
// the K packed rows of a call or session (h->sh_pk as rb_pack sized it): row | load | node
struct RbPacked { u32 *row, *load, *node; };
RbPacked rb_packed(rio_gp* h, u64 K) {
    u32* const row = (u32*)h->sh_pk.p;
    return {row, row + K, row + 2 * K};
}
}  // namespace

// What both forms ask of a cfg; `who` keeps every message's text.  own: the calling form's complaint about its other arguments
// (or NULL), reported where that form always reported it.  listing: the moves are listed, into at most `cap` entries.
enum class RbForm { single, shard, shard_ordered };
struct RbCfg { u32 order, rounds; u64 budget; };
static int rb_cfg(rio_gp* h, const char* who, RbForm form, const rio_gp_rebalance_cfg* cfg, const char* own, bool listing, u64 cap,
                  RbCfg* c) {
    const std::string me = std::string(who) + ": ";
    if (const char* why = rebalance_cfg_order(cfg, &c->order))
        return fail(h, RIO_GP_EINVAL, me + (form == RbForm::single ? why : "cfg missing or struct_size differs"));
    if (c->order != RIO_GP_REBALANCE_ROW_ORDER && form == RbForm::shard)
        return fail(h, RIO_GP_EINVAL, me + "the load-ordered cut (order = RIO_GP_REBALANCE_BY_LOAD) of a row-sharded table has "
                                           "threshold passes between cut and select: start it with "
                                           "rio_gp_shard_rebalance_begin_ordered");
    if (cfg->rounds > 8) return fail(h, RIO_GP_EINVAL, me + "rounds above the solver limit (8)");
    if (own) return fail(h, RIO_GP_EINVAL, me + own);
    if (!listing && cap) return fail(h, RIO_GP_EINVAL, me + "moves_cap without a move listing");
    c->rounds = cfg->rounds ? cfg->rounds : h->rounds;
    c->budget = listing ? std::min<u64>(cfg->max_moves, cap) : cfg->max_moves;
    return RIO_GP_OK;
}

// the (slot x tile) matrix and the per-tile counts of a plan (a plan without slots still has one row: a forced pass)
static int rb_plan_ensure(rio_gp* h, const ShPlan& p) {
    if (int rc = ensure(h, h->sh_mat, (size_t)std::max<u32>(p.s, 1) * p.nt * sizeof(u64))) return rc;
    return ensure(h, h->sh_tile, (size_t)p.nt * sizeof(u32));
}

// R1 behind map / slot_node / slot_free (and, by load, thr): the cut of every slot, the surplus per tile, acc's two surplus
// words.  fill_cut: cut[] starts as kNone everywhere (the single form; in the session k_shrb_import_* wrote it).
// cls (here and in rb_pack): the immovable classes of rule 13, or nullptr (none; the session of the row-sharded table always)
static int rb_surplus(rio_gp* h, const ShPlan& p, const RbBufs& b, const u32* thr, bool fill_cut, const ShCls* cls = nullptr) {
    if (int rc = rb_plan_ensure(h, p)) return rc;
    launch_shed_cut(h->assign[h->cur], h->load, h->aff, p, b.map, b.slot_node, b.slot_free, (u64*)h->sh_mat.p, b.cut, thr, fill_cut,
                    h->stream, cls);
    launch_shed_count(h->assign[h->cur], h->load, h->aff, p, b.cut, thr, (u32*)h->sh_tile.p, b.acc, h->stream, cls);
    HIPCHK(h, hipGetLastError());
    return RIO_GP_OK;
}

// R2: the first K > 0 surplus rows into the packed columns, in row order; used[] -= their load, acc[kShAccSelectedLoad]
static int rb_pack(rio_gp* h, const ShPlan& p, const RbBufs& b, const u32* thr, u64 K, u64* used, const ShCls* cls = nullptr) {
    const u64 nc = (K + kShChunk - 1) / kShChunk;
    int rc;
    if ((rc = ensure(h, h->sh_pk, 3 * K * sizeof(u32))) || (rc = ensure(h, h->sh_chunk, nc * sizeof(u64)))) return rc;
    const RbPacked pk = rb_packed(h, K);
    launch_shed_pack(h->assign[h->cur], h->load, h->aff, p, b.cut, thr, (const u32*)h->sh_tile.p, K, pk.row, pk.load, pk.node, used,
                     b.acc, h->stream, cls);
    return RIO_GP_OK;
}

// acc as the passes so far left it -> the counters of the stats; moved_* and stayed_rows only behind a finish pass that ran
static void rb_counters(const u64* a, bool finished, rio_gp_rebalance_stats* s) {
    s->surplus_rows = a[kShAccSurplusRows];
    s->surplus_load = a[kShAccSurplusLoad];
    s->selected_load = a[kShAccSelectedLoad];
    if (!finished) return;
    s->moved_rows = a[kShAccMovedRows];
    s->moved_load = a[kShAccMovedLoad];
    s->stayed_rows = a[kShAccStayed];
}

// R4 + the column + the moves of the K packed rows (K == 0: nothing to launch), then acc and the global `used` behind one wait:
// the counters of *s and nodes_over_after against the targets T.  own_used: where the rows left without a node give their load
// back, the vector rb_pack took it from; what is read back is h->used.storage(), the same vector in the single form, the sum
// over the ranks in the session.  d_rows / d_from / d_to: K entries each, or NULL.
static int rb_finish(rio_gp* h, const RbBufs& b, u64 K, u64* own_used, const u64* T, u32* d_rows, u32* d_from, u32* d_to,
                     rio_gp_rebalance_stats* s) {
    const u32 m = h->m;
    if (K) {
        const RbPacked pk = rb_packed(h, K);
        launch_shed_finish(K, pk.row, pk.load, pk.node, h->assign[h->cur], own_used, (u32*)h->sh_chunk.p, b.acc, d_rows, d_from, d_to,
                           h->stream);
        HIPCHK(h, hipGetLastError());
    }
    u64 a[kShAcc];
    std::vector<u64> used(m ? m : 1);
    HIPCHK(h, hipMemcpyAsync(a, b.acc, sizeof a, hipMemcpyDeviceToHost, h->stream));
    if (m) HIPCHK(h, hipMemcpyAsync(used.data(), h->used.storage(), (size_t)m * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    rb_counters(a, K != 0, s);
    s->nodes_over_after = 0;
    for (u32 j = 0; j < m; ++j) s->nodes_over_after += h->h_alive[j] && used[j] > T[j];
    return RIO_GP_OK;
}

// The device-side work of rio_gp_rebalance[_dev] (validated, locked).  d_rows / d_from / d_to: device arrays of at least
// `budget` entries, or all NULL.  Three host waits at the most, each the end of a phase: R0 (`used` and pin, from which the
// host picks the slots), rb_surplus (acc: K), rb_finish.  The session of the row-sharded table (further down) ends the same
// phases where its records leave for the other ranks.
static int rebalance_locked(rio_gp* h, const rio_gp_rebalance_cfg* cfg, const RbCfg& c, rio_gp_rebalance_stats* st, u32* d_rows,
                            u32* d_from, u32* d_to, uint64_t* n_moves) {
    rio_gp_rebalance_stats s{};
    if (n_moves) *n_moves = 0;
    HIPCHK(h, hipSetDevice(h->device));
    // a change of the inputs, like every CRUD call: an uncommitted solve is dropped, the next tick is neither quiet nor chained
    inputs_changed(h);
    const u32 m = h->m;
    const u64 n = h->n;
    int rc;
    if ((rc = rb_ensure(h))) return rc;
    const RbBufs b = rb_bufs(h);
    const u32* const thr = c.order == RIO_GP_REBALANCE_BY_LOAD ? b.thr : nullptr;  // (nullptr: the k_shed_* kernels cut in row order)
    // rule 13: with an immovable class every table pass runs in its class-aware form (k_shedc_*); without one, as ever
    ShCls cs{};
    if (h->cls_any_imm) {
        cs.K = h->cls_K;  // (rio_gp_set_class_movable made the column)
        memcpy(cs.imm, h->cls_imm, sizeof cs.imm);
    }
    const ShCls* const cls = h->cls_any_imm ? &cs : nullptr;
    // the targets (the capacities by default) and the live nodes
    std::vector<u64> T(m ? m : 1), used(m ? m : 1), pn(m ? m : 1);
    if (cfg->target) memcpy(T.data(), cfg->target, (size_t)m * sizeof(u64));
    else if (m) HIPCHK(h, hipMemcpyAsync(T.data(), h->cap, (size_t)m * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    // R0: one pass — every node's load (the `used` vector of this column, rebuilt: nothing left to fold) and its pinned load
    u64* const d_used = h->used.storage();
    launch_shed_hist(h->assign[h->cur], h->load, h->aff, n, m, d_used, b.pin, h->stream, nullptr, cls);
    HIPCHK(h, hipGetLastError());
    h->used.rebuilt();
    if (m) {
        HIPCHK(h, hipMemcpyAsync(used.data(), d_used, (size_t)m * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(pn.data(), b.pin, (size_t)m * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // R1 on the host's side: which live nodes hold more candidate load than T -sat pinned
    std::vector<u32> hmap(m ? m : 1, kNone), snode;
    std::vector<u64> sfree, tl(m ? m : 1, 0);
    for (u32 j = 0; j < m; ++j) {
        if (!h->h_alive[j]) continue;
        tl[j] = T[j];
        s.nodes_over_before += used[j] > T[j];
        const u64 fr = T[j] > pn[j] ? T[j] - pn[j] : 0, cand = used[j] - pn[j];
        if (cand > fr) { hmap[j] = (u32)snode.size(); snode.push_back(j); sfree.push_back(fr); }
    }
    const u32 S = (u32)snode.size();
    const ShPlan p = sh_plan(n, m, S);
    if (S) {
        // R1 on the device: the exact cut of every over node; the surplus per tile (counted under a budget of 0 too; the
        // targets are for the rounds)
        HIPCHK(h, hipMemcpyAsync(b.map, hmap.data(), (size_t)m * sizeof(u32), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(b.slot_node, snode.data(), (size_t)S * sizeof(u32), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(b.slot_free, sfree.data(), (size_t)S * sizeof(u64), hipMemcpyHostToDevice, h->stream));
        if (c.budget) HIPCHK(h, hipMemcpyAsync(b.tgt, tl.data(), (size_t)m * sizeof(u64), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemsetAsync(b.acc, 0, kShAcc * sizeof(u64), h->stream));
        if (thr) {  // R1' first finds every over node's threshold (slot_free: what is left for the candidates of exactly that
                    // load): the cut below then falls among those
            if ((rc = ensure(h, h->sh_sel, ((size_t)S << sh_sel_plan(S).bits) * sizeof(u64)))) return rc;
            launch_shed_select(h->assign[h->cur], h->load, h->aff, n, m, S, b.map, b.slot_node, b.slot_free, b.pre, (u64*)h->sh_sel.p,
                               b.thr, h->stream, cls);
        }
        if ((rc = rb_surplus(h, p, b, thr, true, cls))) return rc;
        u64 a[kShAcc];
        HIPCHK(h, hipMemcpyAsync(a, b.acc, sizeof a, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        rb_counters(a, false, &s);
    }
    const u64 K = std::min<u64>(s.surplus_rows, c.budget);
    s.selected_rows = K;
    if (!K) {  // nothing over target, or nothing may move: nothing changed, and `used` is R0's
        s.nodes_over_after = s.nodes_over_before;
        if (st) *st = s;
        return RIO_GP_OK;
    }
    // R2: the first K surplus rows, packed in row order; R3: the water-fill rounds; R4 + the column + the moves
    if ((rc = rb_pack(h, p, b, thr, K, d_used, cls))) return rc;
    const RbPacked pk = rb_packed(h, K);
    for (u32 r = 0; r < c.rounds; ++r)
        launch_shed_round(K, pk.load, pk.node, b.tgt, m, d_used, (u64*)h->sh_chunk.p, b.C, b.ord, b.cntp, h->stream);
    if ((rc = rb_finish(h, b, K, d_used, T.data(), d_rows, d_from, d_to, &s))) return rc;
    if (n_moves) *n_moves = s.moved_rows;
    if (st) *st = s;
    return RIO_GP_OK;
}

// the checks of both entry points: nothing is changed before they pass
static int rebalance_args(rio_gp* h, const rio_gp_rebalance_cfg* cfg, const void* r, const void* f, const void* t, uint64_t cap,
                          RbCfg* c) {
    const bool together = (r != nullptr) == (f != nullptr) && (r != nullptr) == (t != nullptr);
    const char* own = together ? nullptr : "out_rows / out_from / out_to are given together or not at all";
    if (int rc = rb_cfg(h, "rio_gp_rebalance", RbForm::single, cfg, own, r != nullptr, cap, c)) return rc;
    return refuse_row_sharded(h, "rio_gp_rebalance");
}

int rio_gp_rebalance(rio_gp_t* h, const rio_gp_rebalance_cfg* cfg, rio_gp_rebalance_stats* st, uint32_t* out_rows,
                     uint32_t* out_from, uint32_t* out_to, uint64_t moves_cap, uint64_t* n_moves) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    RbCfg c;
    int rc;
    if ((rc = rebalance_args(h, cfg, out_rows, out_from, out_to, moves_cap, &c))) return rc;
    // the listing is staged on the device (moves <= selected <= budget <= min(n, moves_cap))
    u32* d = nullptr;
    u64 stage = 0;
    if (out_rows) {
        stage = std::min<u64>(c.budget, h->n);
        if ((rc = ensure(h, h->sh_mv, 3 * std::max<u64>(stage, 1) * sizeof(u32)))) return rc;
        d = (u32*)h->sh_mv.p;
    }
    uint64_t nm = 0;
    if ((rc = rebalance_locked(h, cfg, c, st, d, d ? d + stage : nullptr, d ? d + 2 * stage : nullptr, &nm))) return rc;
    if (n_moves) *n_moves = nm;
    if (out_rows && nm) return read_listing(h, d, stage, nm, {out_rows, out_from, out_to});
    return RIO_GP_OK;
}

int rio_gp_rebalance_dev(rio_gp_t* h, const rio_gp_rebalance_cfg* cfg, rio_gp_rebalance_stats* st, uint32_t* d_rows,
                         uint32_t* d_from, uint32_t* d_to, uint64_t moves_cap, uint64_t* n_moves) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    RbCfg c;
    if (int rc = rebalance_args(h, cfg, d_rows, d_from, d_to, moves_cap, &c)) return rc;
    return rebalance_locked(h, cfg, c, st, d_rows, d_from, d_to, n_moves);
}

// ---- change feed -----------------------------------------------------------------------------

// The feed's state, on first use: B (RIO_GP_NONE everywhere: the first listing is complete), 4 B per tile of counts, the
// workgroup sums and one mapped pinned line (chg_counters: idle expiry counts with them too).
static int chg_counters(rio_gp* h) {
    const u64 tiles = (h->cap_rows + kChgTile - 1) / kChgTile;
    int rc;
    // (each piece once: a call after a failed allocation or fill allocates only what is still missing)
    if (!h->chg_cnt && (rc = dalloc(h, &h->chg_cnt, tiles))) return rc;
    if (!h->chg_gsum && (rc = dalloc(h, &h->chg_gsum, kChgMaxGroups + 1))) return rc;
    if (!h->h_chg) {
        if (hipHostMalloc(reinterpret_cast<void**>(&h->h_chg), 64, hipHostMallocMapped) != hipSuccess ||
            hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_chg), h->h_chg, 0) != hipSuccess) {
            (void)hipGetLastError();
            if (h->h_chg) (void)hipHostFree(h->h_chg);
            h->h_chg = nullptr;
            return fail(h, RIO_GP_ENOMEM, "hipHostMalloc(change feed word) failed");
        }
    }
    return RIO_GP_OK;
}
static int chg_scratch(rio_gp* h) {
    if (h->chg_B) return RIO_GP_OK;
    int rc;
    if ((rc = chg_counters(h))) return rc;
    return lazy_fill(h, h->chg_B, kNone);
}

// checks shared by both forms: nothing is changed before they pass
static int chg_args(rio_gp* h, uint32_t flags, const void* r, const void* o, const void* w, uint64_t cap, const uint64_t* n_changes) {
    if (flags & ~RIO_GP_CHANGES_PEEK) return fail(h, RIO_GP_EINVAL, "rio_gp_changes: unknown flags");
    if (!n_changes) return fail(h, RIO_GP_EINVAL, "rio_gp_changes: n_changes is NULL");
    if ((r != nullptr) != (o != nullptr) || (r != nullptr) != (w != nullptr))
        return fail(h, RIO_GP_EINVAL, "rio_gp_changes: out_rows / out_old / out_new are given together or not at all");
    if (!r && cap) return fail(h, RIO_GP_EINVAL, "rio_gp_changes: cap without a listing");
    return refuse_row_sharded(h, "rio_gp_changes");
}

// The count pass over the committed column and B (rows 0 .. n-1); the total lands in the mapped word.  Nothing here touches the
// table, `used`, the epochs or the chain: B is the feed's own.
static int chg_count(rio_gp* h, const ChgPlan& p) {
    *h->h_chg = 0;
    launch_chg_count(h->assign[h->cur], h->chg_B, p, h->chg_cnt, h->chg_gsum, h->d_chg, h->stream);
    HIPCHK(h, hipGetLastError());
    return RIO_GP_OK;
}

int rio_gp_changes(rio_gp_t* h, uint32_t flags, uint32_t* out_rows, uint32_t* out_old, uint32_t* out_new, uint64_t cap,
                   uint64_t* n_changes) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    int rc;
    if ((rc = chg_args(h, flags, out_rows, out_old, out_new, cap, n_changes))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = chg_scratch(h))) return rc;
    const ChgPlan p = chg_plan(h->n);
    if ((rc = chg_count(h, p))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const u64 total = p.G ? *h->h_chg : 0;
    *n_changes = total;
    const u64 L = std::min<u64>(total, cap);
    if (!out_rows || L == 0) return RIO_GP_OK;
    if ((rc = ensure(h, h->chg_stage, 3 * L * sizeof(u32)))) return rc;
    u32* d = (u32*)h->chg_stage.p;
    launch_chg_list(h->assign[h->cur], h->chg_B, p, h->chg_cnt, h->chg_gsum, L, !(flags & RIO_GP_CHANGES_PEEK), d, d + L, d + 2 * L,
                    h->stream);
    HIPCHK(h, hipGetLastError());
    return read_listing(h, d, L, L, {out_rows, out_old, out_new});
}

int rio_gp_changes_dev(rio_gp_t* h, uint32_t flags, uint32_t* d_rows, uint32_t* d_old, uint32_t* d_new, uint64_t cap,
                       uint64_t* n_changes) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    int rc;
    if ((rc = chg_args(h, flags, d_rows, d_old, d_new, cap, n_changes))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = chg_scratch(h))) return rc;
    const ChgPlan p = chg_plan(h->n);
    if ((rc = chg_count(h, p))) return rc;
    // the list pass reads the prefix the count pass left on the device and drops ranks >= cap itself: one wait for the call
    if (d_rows) launch_chg_list(h->assign[h->cur], h->chg_B, p, h->chg_cnt, h->chg_gsum, cap, !(flags & RIO_GP_CHANGES_PEEK), d_rows,
                                d_old, d_new, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *n_changes = p.G ? *h->h_chg : 0;
    return RIO_GP_OK;
}

int rio_gp_changes_reset(rio_gp_t* h) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    if (int rc = refuse_row_sharded(h, "rio_gp_changes_reset")) return rc;
    if (!h->chg_B) return RIO_GP_OK;  // (never used: the first listing is complete anyway)
    HIPCHK(h, hipSetDevice(h->device));
    launch_fill_u32(h->chg_B, h->cap_rows, kNone, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RIO_GP_OK;
}

// ---- idle expiry ------------------------------------------------------------------------------

// The last-seen column on first use (0 everywhere: never seen), the freed-load word and the feed's counters.
static int exp_scratch(rio_gp* h) {
    if (h->exp_S) return RIO_GP_OK;
    int rc;
    if ((rc = chg_counters(h))) return rc;
    if (!h->exp_freed && (rc = dalloc(h, &h->exp_freed, 1))) return rc;
    return lazy_fill(h, h->exp_S, 0u);
}
// what every call of the family does first (one rule: no last-seen column on a handle of the row-sharded solve)
static int exp_begin(rio_gp* h, const char* who) {
    if (int rc = refuse_row_sharded(h, who)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    return exp_scratch(h);
}

// Touch calls write S and nothing else: no inputs_changed, `used` and the solve in flight stay as they are.
int rio_gp_touch_batch_dev(rio_gp_t* h, uint64_t n, const uint32_t* d_idx, uint32_t epoch) {
    if (!h || (n && !d_idx)) return RIO_GP_EINVAL;
    Locked g(h);
    int rc;
    if ((rc = exp_begin(h, "rio_gp_touch_batch"))) return rc;
    if (!n) return RIO_GP_OK;
    return dev_batch(h, "rio_gp_touch_batch", [&] { launch_touch(h->exp_S, h->n, d_idx, n, epoch, h->dstats, h->stream); });
}

int rio_gp_touch_batch(rio_gp_t* h, uint64_t n, const uint32_t* idx, uint32_t epoch) {
    if (!h || (n && !idx)) return RIO_GP_EINVAL;
    Locked g(h);
    int rc;
    Staged d;
    if ((rc = stage_batch(h, "rio_gp_touch_batch", exp_begin, n, idx, nullptr, 0, d)) || !n) return rc;
    launch_touch(h->exp_S, h->n, d.first, n, epoch, h->dstats, h->stream);  // (validated: nothing is counted)
    return staged_done(h);
}

int rio_gp_touch_all(rio_gp_t* h, uint32_t epoch) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    int rc;
    if ((rc = exp_begin(h, "rio_gp_touch_all"))) return rc;
    launch_seen_merge(h->exp_S, nullptr, epoch, h->n, h->stream);
    HIPCHK(h, hipGetLastError());
    return RIO_GP_OK;
}

int rio_gp_touch_merge_dev(rio_gp_t* h, uint64_t rows, const uint32_t* d_stamps) {
    if (!h || (rows && !d_stamps)) return RIO_GP_EINVAL;
    Locked g(h);
    if (rows > h->n) return fail(h, RIO_GP_EINVAL, "rio_gp_touch_merge: rows exceeds the object table");
    int rc;
    if ((rc = exp_begin(h, "rio_gp_touch_merge"))) return rc;
    launch_seen_merge(h->exp_S, d_stamps, 0u, rows, h->stream);
    HIPCHK(h, hipGetLastError());
    return RIO_GP_OK;
}

int rio_gp_touch_merge(rio_gp_t* h, uint64_t rows, const uint32_t* stamps) {
    if (!h || (rows && !stamps)) return RIO_GP_EINVAL;
    Locked g(h);
    if (rows > h->n) return fail(h, RIO_GP_EINVAL, "rio_gp_touch_merge: rows exceeds the object table");
    int rc;
    if ((rc = exp_begin(h, "rio_gp_touch_merge"))) return rc;
    Staged d;
    if ((rc = stage_batch(h, "rio_gp_touch_merge", nullptr, rows, stamps, nullptr, 0, d)) || !rows) return rc;
    launch_seen_merge(h->exp_S, d.first, 0u, rows, h->stream);
    return staged_done(h);
}

int rio_gp_get_seen(rio_gp_t* h, uint64_t n, uint32_t* out) {
    if (!h || !out) return RIO_GP_EINVAL;
    Locked g(h);
    if (n != h->n) return fail(h, RIO_GP_EINVAL, "rio_gp_get_seen: n differs from the object table");
    int rc;
    if ((rc = exp_begin(h, "rio_gp_get_seen"))) return rc;
    if (n) HIPCHK(h, hipMemcpyAsync(out, h->exp_S, n * sizeof(u32), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RIO_GP_OK;
}

// The idle sweep (rio_gp_expire*, rio_gp_expire_classes*): one driver behind the four calls.  What a call names idle:
struct Sweep {
    bool classes;             // false: S < cutoff for every row; the plain sweep never touches cls_*
    u32 cutoff;
    u32 n_classes;            // true: S < cutoffs[K[row]], K < n_classes (a row of a class from n_classes on is never idle) ...
    const uint32_t* cutoffs;
    uint64_t* idle_by_class;  // ... and the idle rows of every class are counted into here (may be NULL)
};
static int cls_begin(rio_gp* h, const char* who);  // (object classes, below)

// The copies of the per-class counts are zero between the calls because k_cls_publish, the last launch of the count pass, leaves
// them so.  A call that cannot tell whether that launch ran (a launch error, a failed wait) has the next call of the section
// fill them again: a sweep after a failed one must not add to what the failed one left.
static int expc_failed(rio_gp* h, const char* msg) {
    h->cls_tab_stale = true;  // (cls_begin zeroes the copies before the next call of the section runs)
    return fail(h, RIO_GP_EUPSTREAM, msg);
}
// The count pass over the committed column and S (and K); the total lands in the mapped word, the per-class counts in h->h_cls
// (mapped too: complete after the next wait).  It changes nothing of the table.
static int sweep_count(rio_gp* h, const ChgPlan& p, const Sweep& w, const ClsCutoffs& ct) {
    *h->h_chg = 0;
    if (w.classes) {
        launch_expc_count(h->assign[h->cur], h->exp_S, h->cls_K, p, ct, h->chg_cnt, h->chg_gsum, h->d_chg, h->cls_tab, h->d_cls,
                          h->exp_freed, h->stream);
        if (hipGetLastError() != hipSuccess) return expc_failed(h, "rio_gp_expire_classes: a launch of the count pass failed");
        return RIO_GP_OK;
    }
    launch_exp_count(h->assign[h->cur], h->exp_S, p, w.cutoff, h->chg_cnt, h->chg_gsum, h->d_chg, h->exp_freed, h->stream);
    HIPCHK(h, hipGetLastError());
    return RIO_GP_OK;
}
// The apply pass for the first `cap` idle rows, and the freed load into the mapped line's second u64.  `used` follows the writes
// when it is valid, as the remove kernels keep it.  The caller has not waited yet.
static int sweep_apply(rio_gp* h, const ChgPlan& p, const Sweep& w, const ClsCutoffs& ct, u64 cap, u32* d_rows, u32* d_node) {
    u64* const used = h->used.live();
    if (w.classes)
        launch_expc_apply(h->assign[h->cur], h->exp_S, h->cls_K, p, ct, h->chg_cnt, h->chg_gsum, cap, d_rows, d_node, aff_life(h),
                          h->load, h->m, used, h->exp_freed, h->stream);
    else
        launch_exp_apply(h->assign[h->cur], h->exp_S, p, w.cutoff, h->chg_cnt, h->chg_gsum, cap, d_rows, d_node, aff_life(h),
                         h->load, h->m, used, h->exp_freed, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(reinterpret_cast<u64*>(h->h_chg) + 1, h->exp_freed, sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    return RIO_GP_OK;
}

// Both forms.  to_host: rows / node are the caller's host arrays: count, wait, clamp to cap, apply into chg_stage, read the
// listing back.  Otherwise they are device arrays: the apply pass reads the prefix the count pass left on the device and drops
// ranks >= cap itself, one wait for the call.
static int sweep(rio_gp* h, const Sweep& w, bool to_host, uint32_t* rows, uint32_t* node, uint64_t cap, uint64_t* n_idle,
                 uint64_t* load_freed) {
    // the checks: nothing is allocated, launched or changed before they pass
    if (w.classes && (w.n_classes < 1 || w.n_classes > RIO_GP_MAX_CLASSES || !w.cutoffs))
        return fail(h, RIO_GP_EINVAL, "rio_gp_expire_classes: 1 .. RIO_GP_MAX_CLASSES cutoffs are needed");
    if (!n_idle) return fail(h, RIO_GP_EINVAL, "rio_gp_expire: n_idle is NULL");
    if ((rows != nullptr) != (node != nullptr))
        return fail(h, RIO_GP_EINVAL, "rio_gp_expire: out_rows / out_node are given together or not at all");
    if (!rows && cap) return fail(h, RIO_GP_EINVAL, "rio_gp_expire: cap without a listing");
    int rc;
    ClsCutoffs ct;  // (the class form's: 0 from n_classes on)
    if ((rc = exp_begin(h, w.classes ? "rio_gp_expire_classes" : "rio_gp_expire"))) return rc;
    if (w.classes) {
        if ((rc = cls_begin(h, "rio_gp_expire_classes"))) return rc;
        std::fill(std::copy(w.cutoffs, w.cutoffs + w.n_classes, ct.v), ct.v + kClsMax, 0u);
    }
    const ChgPlan p = chg_plan(h->n);
    if ((rc = sweep_count(h, p, w, ct))) return rc;
    u64* const freed = reinterpret_cast<u64*>(h->h_chg) + 1;
    const bool apply = !to_host && rows && cap && p.G;  // (the host form's apply comes behind the wait)
    if (!to_host) *freed = 0;
    if (apply && (rc = sweep_apply(h, p, w, ct, cap, rows, node))) {
        inputs_changed(h);
        return rc;
    }
    const hipError_t e = hipStreamSynchronize(h->stream);
    const u64 total = p.G ? *h->h_chg : 0;
    if (apply && (e != hipSuccess || total)) inputs_changed(h);  // something was un-placed (or nobody can tell)
    if (e != hipSuccess && w.classes) {
        if (to_host) return expc_failed(h, "rio_gp_expire_classes: the count pass failed");
        h->cls_tab_stale = true;
    }
    HIPCHK(h, e);
    *n_idle = total;
    if (w.classes && w.idle_by_class) std::copy(h->h_cls, h->h_cls + w.n_classes, w.idle_by_class);
    if (load_freed) *load_freed = apply ? *freed : 0;
    const u64 L = std::min<u64>(total, cap);
    if (!to_host || !rows || L == 0) return RIO_GP_OK;  // (a count-only call or no idle row: no inputs_changed)
    if ((rc = ensure(h, h->chg_stage, 2 * L * sizeof(u32)))) return rc;
    u32* d = (u32*)h->chg_stage.p;
    inputs_changed(h);  // from here on it is a rio_gp_remove_batch of the listed rows
    if ((rc = sweep_apply(h, p, w, ct, L, d, d + L))) return rc;
    if ((rc = read_listing(h, d, L, L, {rows, node}))) return rc;
    if (load_freed) *load_freed = *freed;
    return RIO_GP_OK;
}

int rio_gp_expire(rio_gp_t* h, uint32_t cutoff, uint32_t* out_rows, uint32_t* out_node, uint64_t cap, uint64_t* n_idle,
                  uint64_t* load_freed) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    return sweep(h, Sweep{false, cutoff, 0, nullptr, nullptr}, true, out_rows, out_node, cap, n_idle, load_freed);
}

int rio_gp_expire_dev(rio_gp_t* h, uint32_t cutoff, uint32_t* d_rows, uint32_t* d_node, uint64_t cap, uint64_t* n_idle,
                      uint64_t* load_freed) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    return sweep(h, Sweep{false, cutoff, 0, nullptr, nullptr}, false, d_rows, d_node, cap, n_idle, load_freed);
}

// ---- object classes ---------------------------------------------------------------------------

static_assert(RIO_GP_MAX_CLASSES == kClsMax, "object classes: the header's constant is the kernels'");

// what every call of the family does first (one rule: no class column on a handle of the row-sharded solve): the class column
// on first use, 0 everywhere, and the sweep's small tables
static int cls_begin(rio_gp* h, const char* who) {
    if (int rc = refuse_row_sharded(h, who)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if (h->cls_ready && h->cls_tab_stale) {
        HIPCHK(h, hipMemsetAsync(h->cls_tab, 0, (size_t)kClsSlots * kClsMax * sizeof(u64), h->stream));
        h->cls_tab_stale = false;
    }
    if (h->cls_ready) return RIO_GP_OK;
    int rc;
    if (!h->cls_K && (rc = dalloc(h, &h->cls_K, h->cap_rows))) return rc;
    if (!h->cls_tab && (rc = dalloc(h, &h->cls_tab, (size_t)kClsSlots * kClsMax))) return rc;
    if (!h->h_cls) {
        if (hipHostMalloc(reinterpret_cast<void**>(&h->h_cls), kClsMax * sizeof(u64), hipHostMallocMapped) != hipSuccess ||
            hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_cls), h->h_cls, 0) != hipSuccess) {
            (void)hipGetLastError();
            if (h->h_cls) (void)hipHostFree(h->h_cls);
            h->h_cls = nullptr;
            return fail(h, RIO_GP_ENOMEM, "hipHostMalloc(per-class counts) failed");
        }
    }
    HIPCHK(h, hipMemsetAsync(h->cls_K, 0, h->cap_rows, h->stream));
    HIPCHK(h, hipMemsetAsync(h->cls_tab, 0, (size_t)kClsSlots * kClsMax * sizeof(u64), h->stream));
    h->cls_ready = true;  // (last: it is what says the column is complete)
    return RIO_GP_OK;
}

// The class setters write K and nothing else: no inputs_changed, `used` and the solve in flight stay as they are.
static int cls_set_range(rio_gp* h, uint64_t first_row, uint64_t rows, const uint8_t* cls, bool dev) {
    if (!h || (rows && !cls)) return RIO_GP_EINVAL;
    Locked g(h);
    int rc;
    if ((rc = refuse_row_sharded(h, "rio_gp_set_classes"))) return rc;
    if (first_row > h->n || rows > h->n - first_row) return fail(h, RIO_GP_EINVAL, "rio_gp_set_classes: the range exceeds the object table");
    if ((rc = cls_begin(h, "rio_gp_set_classes"))) return rc;
    if (!rows) return RIO_GP_OK;
    HIPCHK(h, hipMemcpyAsync(h->cls_K + first_row, cls, rows, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    if (!dev) HIPCHK(h, hipStreamSynchronize(h->stream));  // the caller's array is read until here
    return RIO_GP_OK;
}
int rio_gp_set_classes(rio_gp_t* h, uint64_t first_row, uint64_t rows, const uint8_t* cls) {
    return cls_set_range(h, first_row, rows, cls, false);
}
int rio_gp_set_classes_dev(rio_gp_t* h, uint64_t first_row, uint64_t rows, const uint8_t* d_cls) {
    return cls_set_range(h, first_row, rows, d_cls, true);
}

int rio_gp_set_class_batch_dev(rio_gp_t* h, uint64_t n, const uint32_t* d_idx, const uint8_t* d_cls) {
    if (!h || (n && (!d_idx || !d_cls))) return RIO_GP_EINVAL;
    Locked g(h);
    if (n >= 0xFFFFFFFFull) return fail(h, RIO_GP_EINVAL, "rio_gp_set_class_batch: too many entries");
    int rc;
    if ((rc = cls_begin(h, "rio_gp_set_class_batch"))) return rc;
    if (!n) return RIO_GP_OK;
    return dev_batch(h, "rio_gp_set_class_batch",
                     [&] { launch_set_class_batch(h->cls_K, h->n, d_idx, d_cls, n, h->pos, h->dstats, h->stream); });
}

int rio_gp_set_class_batch(rio_gp_t* h, uint64_t n, const uint32_t* idx, const uint8_t* cls) {
    if (!h || (n && (!idx || !cls))) return RIO_GP_EINVAL;
    Locked g(h);
    if (n >= 0xFFFFFFFFull) return fail(h, RIO_GP_EINVAL, "rio_gp_set_class_batch: too many entries");
    int rc;
    Staged d;
    if ((rc = stage_batch(h, "rio_gp_set_class_batch", cls_begin, n, idx, cls, 1, d)) || !n) return rc;
    launch_set_class_batch(h->cls_K, h->n, d.first, (const unsigned char*)d.second, n, h->pos, h->dstats,
                           h->stream);  // (validated: nothing is counted)
    return staged_done(h);
}

int rio_gp_get_classes(rio_gp_t* h, uint64_t n, uint8_t* out) {
    if (!h || !out) return RIO_GP_EINVAL;
    Locked g(h);
    int rc;
    if ((rc = refuse_row_sharded(h, "rio_gp_get_classes"))) return rc;
    if (n != h->n) return fail(h, RIO_GP_EINVAL, "rio_gp_get_classes: n differs from the object table");
    if ((rc = cls_begin(h, "rio_gp_get_classes"))) return rc;
    if (n) HIPCHK(h, hipMemcpyAsync(out, h->cls_K, n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RIO_GP_OK;
}

// Rule 13.  Like the class setters no input of any solve: no inputs_changed; the rebalance alone reads the table.
int rio_gp_set_class_movable(rio_gp_t* h, uint32_t n_classes, const uint8_t* movable) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    if (n_classes > RIO_GP_MAX_CLASSES) return fail(h, RIO_GP_EINVAL, "rio_gp_set_class_movable: n_classes out of range");
    if (n_classes && !movable) return fail(h, RIO_GP_EINVAL, "rio_gp_set_class_movable: no array");
    if (int rc = cls_begin(h, "rio_gp_set_class_movable")) return rc;  // (refuses the row-sharded solve; the column, 0 everywhere)
    u32 imm[kClsMax / 32] = {};
    bool any = false;
    for (u32 c = 0; c < n_classes; ++c)
        if (!movable[c]) { imm[c >> 5] |= 1u << (c & 31); any = true; }
    memcpy(h->cls_imm, imm, sizeof imm);
    h->cls_any_imm = any;
    return RIO_GP_OK;
}

int rio_gp_get_class_movable(rio_gp_t* h, uint8_t* out256) {
    if (!h || !out256) return RIO_GP_EINVAL;
    Locked g(h);
    for (u32 c = 0; c < kClsMax; ++c) out256[c] = !((h->cls_imm[c >> 5] >> (c & 31)) & 1u);
    return RIO_GP_OK;
}

int rio_gp_expire_classes(rio_gp_t* h, uint32_t n_classes, const uint32_t* cutoffs, uint32_t* out_rows, uint32_t* out_node,
                          uint64_t cap, uint64_t* n_idle, uint64_t* load_freed, uint64_t* idle_by_class) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    return sweep(h, Sweep{true, 0, n_classes, cutoffs, idle_by_class}, true, out_rows, out_node, cap, n_idle, load_freed);
}

int rio_gp_expire_classes_dev(rio_gp_t* h, uint32_t n_classes, const uint32_t* cutoffs, uint32_t* d_rows, uint32_t* d_node,
                              uint64_t cap, uint64_t* n_idle, uint64_t* load_freed, uint64_t* idle_by_class) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    return sweep(h, Sweep{true, 0, n_classes, cutoffs, idle_by_class}, false, d_rows, d_node, cap, n_idle, load_freed);
}

// ---- pressure shedding (rule 14) ---------------------------------------------------------------

// the checks of both entry points: nothing is allocated, launched or changed before they pass
static int shed_args(rio_gp* h, const rio_gp_shed_cfg* cfg, const void* r, const void* nd, uint64_t cap) {
    const char* why = nullptr;
    if (!cfg) why = "cfg is NULL";
    else if (cfg->struct_size != sizeof(rio_gp_shed_cfg)) why = "struct_size differs";
    else if (cfg->reserved != 0) why = "reserved is not 0";
    else if (cfg->class_cutoffs && (cfg->n_classes < 1 || cfg->n_classes > RIO_GP_MAX_CLASSES))
        why = "1 .. RIO_GP_MAX_CLASSES class cutoffs are needed";
    else if (!cfg->class_cutoffs && cfg->n_classes) why = "n_classes without class_cutoffs";
    else if ((r != nullptr) != (nd != nullptr)) why = "out_rows / out_node are given together or not at all";
    else if (!r && cap) why = "rows_cap without a listing";
    if (why) return fail(h, RIO_GP_EINVAL, std::string("rio_gp_shed_idle: ") + why);
    return refuse_row_sharded(h, "rio_gp_shed_idle");
}

// Both forms, validated and locked.  to_host: rows / node are the caller's host arrays.  The phases are the rebalance's (R0 and
// the host's slot pick behind a first wait, the cuts, the surplus per tile) with the expiries' apply pass in place of R2 - R4.
// The node pass writes the call's own scratch (RbBufs::lu / pin), not the handle's `used`: a call that sheds nothing leaves
// the committed vector, its pending parts and its validity exactly as they were.
static int shed_locked(rio_gp* h, const rio_gp_shed_cfg* cfg, bool to_host, rio_gp_shed_stats* st, uint32_t* rows, uint32_t* node,
                       uint64_t cap, uint64_t* n_rows) {
    rio_gp_shed_stats s{};
    int rc;
    if ((rc = exp_begin(h, "rio_gp_shed_idle"))) return rc;
    const bool classes = cfg->class_cutoffs || h->cls_any_imm;
    ClsCutoffs ct;
    if (classes) {  // L0 as one table: the caller's cutoffs (or the one cutoff for every class), 0 where a class is immovable
        if ((rc = cls_begin(h, "rio_gp_shed_idle"))) return rc;
        for (u32 c = 0; c < kClsMax; ++c) {
            const u32 v = cfg->class_cutoffs ? (c < cfg->n_classes ? cfg->class_cutoffs[c] : 0u) : cfg->cutoff;
            ct.v[c] = ((h->cls_imm[c >> 5] >> (c & 31)) & 1u) ? 0u : v;
        }
    }
    if ((rc = rb_ensure(h))) return rc;
    const RbBufs b = rb_bufs(h);
    const u32 m = h->m;
    const u64 n = h->n;
    const u64 B = rows ? std::min<u64>(cfg->max_rows, cap) : cfg->max_rows;
    const IshCols cols{h->assign[h->cur], h->load, h->aff, h->exp_S, cfg->cutoff, classes ? h->cls_K : nullptr,
                       classes ? &ct : nullptr};
    if (n_rows) *n_rows = 0;
    std::vector<u64> T(m ? m : 1), used(m ? m : 1), cand(m ? m : 1);
    if (cfg->target) memcpy(T.data(), cfg->target, (size_t)m * sizeof(u64));
    else if (m) HIPCHK(h, hipMemcpyAsync(T.data(), h->cap, (size_t)m * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    // the node pass: every node's load and its candidates' load; the range of the candidates' keys
    u32 kmm[2] = {kNone, 0};
    launch_ish_hist(cols, n, m, b.lu, b.pin, b.info, h->stream);
    HIPCHK(h, hipGetLastError());
    if (m) {
        HIPCHK(h, hipMemcpyAsync(used.data(), b.lu, (size_t)m * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(cand.data(), b.pin, (size_t)m * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(kmm, b.info, sizeof kmm, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // L1 on the host's side: the live nodes whose candidates weigh more than T -sat pinned
    std::vector<u32> hmap(m ? m : 1, kNone), snode;
    std::vector<u64> sfree;
    for (u32 j = 0; j < m; ++j) {
        if (!h->h_alive[j]) continue;
        s.nodes_over_before += used[j] > T[j];
        const u64 pinned = used[j] - cand[j], fr = T[j] > pinned ? T[j] - pinned : 0;
        if (cand[j] > fr) { hmap[j] = (u32)snode.size(); snode.push_back(j); sfree.push_back(fr); }
    }
    s.nodes_over_after = s.nodes_over_before;
    const u32 S = (u32)snode.size();
    const ChgPlan cp = chg_plan(n);
    if (!S || !cp.G) {  // no node has anything to shed: nothing was changed
        if (st) *st = s;
        return RIO_GP_OK;
    }
    const ShPlan p = sh_plan(n, m, S);
    if ((rc = rb_plan_ensure(h, p)) || (rc = ensure(h, h->sh_sel, ((size_t)S << sh_sel_plan(S).bits) * sizeof(u64)))) return rc;
    HIPCHK(h, hipMemcpyAsync(b.map, hmap.data(), (size_t)m * sizeof(u32), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(b.slot_node, snode.data(), (size_t)S * sizeof(u32), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(b.slot_free, sfree.data(), (size_t)S * sizeof(u64), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(b.acc, 0, kShAcc * sizeof(u64), h->stream));
    // L1 on the device: sigma_j (as the key ~sigma_j in thr) and rem_j, then cutrow_j among the ties; the surplus per tile
    (void)launch_ish_select(cols, n, m, S, b.map, b.slot_node, b.slot_free, b.pre, (u64*)h->sh_sel.p, b.thr, kmm[0], kmm[1],
                            h->stream);
    launch_ish_cut(cols, p, b.map, b.slot_node, b.slot_free, (u64*)h->sh_mat.p, b.cut, b.thr, h->stream);
    *h->h_chg = 0;
    launch_ish_count(cols, cp, m, b.thr, b.cut, h->chg_cnt, h->chg_gsum, h->d_chg, b.acc, h->exp_freed, h->stream);
    HIPCHK(h, hipGetLastError());
    u64 a[kShAcc] = {};
    HIPCHK(h, hipMemcpyAsync(a, b.acc, sizeof a, hipMemcpyDeviceToHost, h->stream));
    // L2 / L3.  The device form's apply pass reads the prefix the count pass left on the device and drops ranks >= B itself;
    // the host form waits for the count first and stages exactly the listing.
    u32 *d_rows = rows, *d_node = node;
    u64 K = B;
    if (to_host || !rows) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        K = std::min<u64>(*h->h_chg, B);
        if (K) {  // (without a listing the ranks still need somewhere to go)
            if ((rc = ensure(h, h->chg_stage, 2 * K * sizeof(u32)))) return rc;
            d_rows = (u32*)h->chg_stage.p;
            d_node = d_rows + K;
        }
    }
    u64 freed = 0;
    if (K) {
        // the recount of the node pass follows the writes; it becomes the committed vector below if a row was shed
        launch_ish_apply(h->assign[h->cur], cols, cp, m, b.thr, b.cut, h->chg_cnt, h->chg_gsum, K, d_rows, d_node, aff_life(h), b.lu,
                         h->exp_freed, h->stream);
        if (hipGetLastError() != hipSuccess) {
            inputs_changed(h);  // (nobody can tell what ran)
            h->used.invalidate();
            return fail(h, RIO_GP_EUPSTREAM, "rio_gp_shed_idle: the launch of the apply pass failed");
        }
        const hipError_t e1 = hipMemcpyAsync(&freed, h->exp_freed, sizeof freed, hipMemcpyDeviceToHost, h->stream);
        const hipError_t e2 = m ? hipMemcpyAsync(used.data(), b.lu, (size_t)m * sizeof(u64), hipMemcpyDeviceToHost, h->stream) : hipSuccess;
        const hipError_t e3 = hipStreamSynchronize(h->stream);
        if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
            inputs_changed(h);
            h->used.invalidate();
            HIPCHK(h, e1 != hipSuccess ? e1 : e2 != hipSuccess ? e2 : e3);
        }
    } else {
        HIPCHK(h, hipStreamSynchronize(h->stream));  // (the counters; nothing was changed)
    }
    s.surplus_rows = *h->h_chg;
    s.surplus_load = a[kShAccSurplusLoad];
    s.shed_rows = std::min<u64>(s.surplus_rows, K);
    s.shed_load = freed;
    if (s.shed_rows) {
        // from here on it is a rio_gp_remove_batch of the listed rows; `used` is the node pass's recount less what they weighed
        inputs_changed(h);
        h->used.invalidate();
        if (m) HIPCHK(h, hipMemcpyAsync(h->used.storage(), b.lu, (size_t)m * sizeof(u64), hipMemcpyDeviceToDevice, h->stream));
        h->used.rebuilt();
        s.nodes_over_after = 0;
        for (u32 j = 0; j < m; ++j) s.nodes_over_after += h->h_alive[j] && used[j] > T[j];
        if (to_host && rows && (rc = read_listing(h, d_rows, K, s.shed_rows, {rows, node}))) return rc;
    }
    if (n_rows) *n_rows = s.shed_rows;
    if (st) *st = s;
    return RIO_GP_OK;
}

int rio_gp_shed_idle(rio_gp_t* h, const rio_gp_shed_cfg* cfg, rio_gp_shed_stats* st, uint32_t* out_rows, uint32_t* out_node,
                     uint64_t rows_cap, uint64_t* n_rows) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    if (int rc = shed_args(h, cfg, out_rows, out_node, rows_cap)) return rc;
    return shed_locked(h, cfg, true, st, out_rows, out_node, rows_cap, n_rows);
}

int rio_gp_shed_idle_dev(rio_gp_t* h, const rio_gp_shed_cfg* cfg, rio_gp_shed_stats* st, uint32_t* d_rows, uint32_t* d_node,
                         uint64_t rows_cap, uint64_t* n_rows) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    if (int rc = shed_args(h, cfg, d_rows, d_node, rows_cap)) return rc;
    return shed_locked(h, cfg, false, st, d_rows, d_node, rows_cap, n_rows);
}

// Read-only, like rio_gp_count_placed: the committed column, K and load; no inputs_changed.
static int census_begin(rio_gp* h, uint32_t flags, uint32_t n_classes, const void* r, const void* l, const void* o) {
    if (flags & ~RIO_GP_CENSUS_BY_NODE) return fail(h, RIO_GP_EINVAL, "rio_gp_census: unknown flags");
    if (n_classes < 1 || n_classes > RIO_GP_MAX_CLASSES) return fail(h, RIO_GP_EINVAL, "rio_gp_census: n_classes out of range");
    if (!r || !l || !o) return fail(h, RIO_GP_EINVAL, "rio_gp_census: out_rows, out_load and n_other are needed");
    if ((flags & RIO_GP_CENSUS_BY_NODE) && (u64)h->m * n_classes > (1ull << 20))
        return fail(h, RIO_GP_EINVAL, "rio_gp_census: more than 2^20 cells");
    return cls_begin(h, "rio_gp_census");
}

int rio_gp_census(rio_gp_t* h, uint32_t flags, uint32_t n_classes, uint64_t* out_rows, uint64_t* out_load, uint64_t* n_other) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    int rc;
    if ((rc = census_begin(h, flags, n_classes, out_rows, out_load, n_other))) return rc;
    const bool by_node = flags & RIO_GP_CENSUS_BY_NODE;
    const u64 cells = (u64)(by_node ? h->m : 1u) * n_classes;
    if ((rc = ensure(h, h->cls_cells, (2 * cells + 1) * sizeof(u64)))) return rc;
    u64* const d = (u64*)h->cls_cells.p;
    launch_census(h->assign[h->cur], h->cls_K, h->load, h->n, h->m, n_classes, by_node, d, d + cells, d + 2 * cells, h->stream);
    HIPCHK(h, hipGetLastError());
    if (cells) {
        HIPCHK(h, hipMemcpyAsync(out_rows, d, cells * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(out_load, d + cells, cells * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(n_other, d + 2 * cells, sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RIO_GP_OK;
}

int rio_gp_census_dev(rio_gp_t* h, uint32_t flags, uint32_t n_classes, uint64_t* d_rows, uint64_t* d_load, uint64_t* n_other) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    int rc;
    if ((rc = census_begin(h, flags, n_classes, d_rows, d_load, n_other))) return rc;
    if ((rc = ensure(h, h->cls_cells, sizeof(u64)))) return rc;
    u64* const d = (u64*)h->cls_cells.p;
    launch_census(h->assign[h->cur], h->cls_K, h->load, h->n, h->m, n_classes, flags & RIO_GP_CENSUS_BY_NODE, reinterpret_cast<u64*>(d_rows),
                  reinterpret_cast<u64*>(d_load), d,
                  h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(n_other, d, sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RIO_GP_OK;
}

// ---- measured load ----------------------------------------------------------------------------

// what every call of the family does first (one rule: no hit column on a handle of the row-sharded solve): the hit column on
// first use, 0 everywhere
static int hits_begin(rio_gp* h, const char* who) {
    if (int rc = refuse_row_sharded(h, who)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    return lazy_fill(h, h->hits_H, 0u);
}

// The hits calls write H and nothing else: no inputs_changed, `used` and the solve in flight stay as they are.
int rio_gp_hits_add_batch_dev(rio_gp_t* h, uint64_t n, const uint32_t* d_idx, const uint32_t* d_weight) {
    if (!h || (n && !d_idx)) return RIO_GP_EINVAL;
    Locked g(h);
    int rc;
    if ((rc = hits_begin(h, "rio_gp_hits_add_batch"))) return rc;
    if (!n) return RIO_GP_OK;
    return dev_batch(h, "rio_gp_hits_add_batch", [&] { launch_hits_add(h->hits_H, h->n, d_idx, d_weight, n, h->dstats, h->stream); });
}

int rio_gp_hits_add_batch(rio_gp_t* h, uint64_t n, const uint32_t* idx, const uint32_t* weight) {
    if (!h || (n && !idx)) return RIO_GP_EINVAL;
    Locked g(h);
    int rc;
    Staged d;
    if ((rc = stage_batch(h, "rio_gp_hits_add_batch", hits_begin, n, idx, weight, sizeof(u32), d)) || !n) return rc;
    launch_hits_add(h->hits_H, h->n, d.first, (const u32*)d.second, n, h->dstats, h->stream);  // (validated: nothing is counted)
    return staged_done(h);
}

int rio_gp_hits_merge_dev(rio_gp_t* h, uint64_t rows, const uint32_t* d_counts) {
    if (!h || (rows && !d_counts)) return RIO_GP_EINVAL;
    Locked g(h);
    int rc;
    if ((rc = hits_begin(h, "rio_gp_hits_merge"))) return rc;
    if (rows > h->n) return fail(h, RIO_GP_EINVAL, "rio_gp_hits_merge: rows exceeds the object table");
    launch_hits_merge(h->hits_H, d_counts, rows, h->stream);
    HIPCHK(h, hipGetLastError());
    return RIO_GP_OK;
}

int rio_gp_hits_merge(rio_gp_t* h, uint64_t rows, const uint32_t* counts) {
    if (!h || (rows && !counts)) return RIO_GP_EINVAL;
    Locked g(h);
    int rc;
    if ((rc = hits_begin(h, "rio_gp_hits_merge"))) return rc;
    if (rows > h->n) return fail(h, RIO_GP_EINVAL, "rio_gp_hits_merge: rows exceeds the object table");
    Staged d;
    if ((rc = stage_batch(h, "rio_gp_hits_merge", nullptr, rows, counts, nullptr, 0, d)) || !rows) return rc;
    launch_hits_merge(h->hits_H, d.first, rows, h->stream);
    return staged_done(h);
}

int rio_gp_get_hits(rio_gp_t* h, uint64_t n, uint32_t* out) {
    if (!h || !out) return RIO_GP_EINVAL;
    Locked g(h);
    int rc;
    if ((rc = hits_begin(h, "rio_gp_get_hits"))) return rc;
    if (n != h->n) return fail(h, RIO_GP_EINVAL, "rio_gp_get_hits: n differs from the object table");
    if (n) HIPCHK(h, hipMemcpyAsync(out, h->hits_H, n * sizeof(u32), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RIO_GP_OK;
}

// The fold is a rio_gp_set_object_attrs of every row's load: it drops an uncommitted solve and counts as a change of the inputs.
// `used` follows inside the pass when it is valid (the pass then reads the committed column too); it stays invalid otherwise.
int rio_gp_load_fold(rio_gp_t* h, uint32_t keep, uint32_t gain, uint32_t min_load, uint32_t max_load, rio_gp_load_fold_stats* st) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    int rc;
    if ((rc = hits_begin(h, "rio_gp_load_fold"))) return rc;
    if (keep > 65536u) return fail(h, RIO_GP_EINVAL, "rio_gp_load_fold: keep above 65536");
    if (min_load > max_load) return fail(h, RIO_GP_EINVAL, "rio_gp_load_fold: min_load above max_load");
    u64* const used = h->used.live();
    // the five statistics words are the first five of the handle's accumulators (zeroed here, read back into pinned memory)
    if ((rc = zero_stats(h))) return rc;
    inputs_changed(h);
    launch_load_fold(h->load, h->hits_H, h->assign[h->cur], h->n, keep, gain, min_load, max_load, h->m, used,
                     reinterpret_cast<u64*>(h->dstats), h->stream);
    if ((rc = read_stats(h))) return rc;
    const u64* const w = reinterpret_cast<const u64*>(h->h_stats);
    if (st) {
        st->rows_changed = w[0];
        st->hits_folded = w[1];
        st->load_before = w[2];
        st->load_after = w[3];
        st->max_load_after = (uint32_t)w[4];
        st->reserved = 0;
    }
    return RIO_GP_OK;
}

// ---- hot-object report --------------------------------------------------------------------------

constexpr size_t kTopHostBytes = 2 * sizeof(u64) + 3 * (size_t)RIO_GP_TOP_MAX * sizeof(u32);
static_assert(RIO_GP_TOP_MAX == kTopMax && RIO_GP_TOP_PLACED == kTopPlaced && RIO_GP_TOP_ON_NODE == kTopOnNode,
              "rio_gp_top_rows: the header's constants are the kernels'");

// The selection's scratch on first use: the feed's per-tile counts and workgroup sums, the device state, the pinned read-back.
static int top_scratch(rio_gp* h) {
    int rc;
    if ((rc = chg_counters(h))) return rc;
    if (!h->h_top && hipHostMalloc(reinterpret_cast<void**>(&h->h_top), kTopHostBytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        h->h_top = nullptr;
        return fail(h, RIO_GP_ENOMEM, "hipHostMalloc(hot-object report) failed");
    }
    if (!h->top_sc) {
        unsigned char* mem = nullptr;
        if ((rc = dalloc(h, &mem, sizeof(TopScratch)))) return rc;
        // (once: `pairs` is read only where a pass of the same call wrote it, and the sort guards the rows it gathers anyway)
        launch_fill_u32(reinterpret_cast<u32*>(mem), sizeof(TopScratch) / sizeof(u32), 0u, h->stream);
        HIPCHK(h, hipGetLastError());
        h->top_sc = reinterpret_cast<TopScratch*>(mem);
    }
    return RIO_GP_OK;
}

// checks shared by both forms: nothing is allocated or launched before they pass
static int top_args(rio_gp* h, uint32_t flags, uint32_t node, const void* r, const void* k, const void* o, uint64_t cap,
                    const uint64_t* n_candidates) {
    if (flags & ~(RIO_GP_TOP_BY_HITS | RIO_GP_TOP_PLACED | RIO_GP_TOP_ON_NODE)) return fail(h, RIO_GP_EINVAL, "rio_gp_top_rows: unknown flags");
    if (!n_candidates) return fail(h, RIO_GP_EINVAL, "rio_gp_top_rows: n_candidates is NULL");
    if (cap > RIO_GP_TOP_MAX) return fail(h, RIO_GP_EINVAL, "rio_gp_top_rows: cap above RIO_GP_TOP_MAX");
    if ((r != nullptr) != (k != nullptr)) return fail(h, RIO_GP_EINVAL, "rio_gp_top_rows: out_rows / out_key are given together or not at all");
    if (!r && (cap || o)) return fail(h, RIO_GP_EINVAL, "rio_gp_top_rows: cap or out_node without a listing");
    if ((flags & RIO_GP_TOP_ON_NODE) && node >= h->m) return fail(h, RIO_GP_EINVAL, "rio_gp_top_rows: node out of range");
    return refuse_row_sharded(h, "rio_gp_top_rows");
}

// Both forms: every pass enqueued behind whatever the handle has in flight, the two sums (and, for the host form, the listing
// behind them) copied into pinned memory, one wait.  Reads load or H and the committed column; writes its own scratch only.
static int top_rows(rio_gp* h, uint32_t flags, uint32_t node, uint32_t min_key, u32* d_rows, u32* d_key, u32* d_node, bool to_host,
                    uint32_t* out_rows, uint32_t* out_key, uint32_t* out_node, uint64_t cap, uint64_t* n_candidates, uint64_t* key_sum) {
    int rc;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = top_scratch(h))) return rc;
    TopScratch* const sc = h->top_sc;
    const u32 c = (u32)cap;
    if (to_host) {
        d_rows = sc->out;
        d_key = sc->out + c;
        d_node = out_node ? sc->out + 2 * (size_t)c : nullptr;
    }
    // (a handle that never counted a hit has no H: every key is 0, and none is allocated for the question)
    const u32* const K = (flags & RIO_GP_TOP_BY_HITS) ? h->hits_H : h->load;
    launch_top_rows(K, h->assign[h->cur], h->n, min_key, flags & (RIO_GP_TOP_PLACED | RIO_GP_TOP_ON_NODE), node, c, sc, h->chg_cnt,
                    h->chg_gsum, d_rows, d_key, d_node, h->stream);
    HIPCHK(h, hipGetLastError());
    const size_t bytes = 2 * sizeof(u64) + (to_host ? (out_node ? 3 : 2) * (size_t)c * sizeof(u32) : 0);
    HIPCHK(h, hipMemcpyAsync(h->h_top, sc->hdr, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    u64 hdr[2];
    memcpy(hdr, h->h_top, sizeof hdr);
    *n_candidates = hdr[0];
    if (key_sum) *key_sum = hdr[1];
    const size_t L = (size_t)std::min<u64>(hdr[0], cap);
    if (to_host && L) {
        const u32* const o = reinterpret_cast<const u32*>(h->h_top + sizeof hdr);
        memcpy(out_rows, o, L * sizeof(u32));
        memcpy(out_key, o + c, L * sizeof(u32));
        if (out_node) memcpy(out_node, o + 2 * (size_t)c, L * sizeof(u32));
    }
    return RIO_GP_OK;
}

int rio_gp_top_rows(rio_gp_t* h, uint32_t flags, uint32_t node, uint32_t min_key, uint32_t* out_rows, uint32_t* out_key,
                    uint32_t* out_node, uint64_t cap, uint64_t* n_candidates, uint64_t* key_sum) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    int rc;
    if ((rc = top_args(h, flags, node, out_rows, out_key, out_node, cap, n_candidates))) return rc;
    return top_rows(h, flags, node, min_key, nullptr, nullptr, nullptr, true, out_rows, out_key, out_node, cap, n_candidates, key_sum);
}

int rio_gp_top_rows_dev(rio_gp_t* h, uint32_t flags, uint32_t node, uint32_t min_key, uint32_t* d_rows, uint32_t* d_key,
                        uint32_t* d_node, uint64_t cap, uint64_t* n_candidates, uint64_t* key_sum) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    int rc;
    if ((rc = top_args(h, flags, node, d_rows, d_key, d_node, cap, n_candidates))) return rc;
    return top_rows(h, flags, node, min_key, d_rows, d_key, d_node, false, nullptr, nullptr, nullptr, cap, n_candidates, key_sum);
}

int rio_gp_set_num_objects(rio_gp_t* h, uint64_t n) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    if (n > h->cap_obj) return fail(h, RIO_GP_EINVAL, "rio_gp_set_num_objects: n exceeds max_objects");
    // rows keep their contents: rows >= n simply take no part (and are rejected as indices) until n grows again — but a
    // placed row that drops out (or comes back) changes what `used` must count, so the vector is rebuilt before its next use
    if (n != h->n) h->used.invalidate();
    h->n = n;
    h->n_hi = std::max<u64>(h->n_hi, n);
    inputs_changed(h);
    h->last.forget_pending();
    return RIO_GP_OK;
}

const uint32_t* rio_gp_assign_dev(rio_gp_t* h) { return h ? h->assign[h->cur] : nullptr; }
const uint32_t* rio_gp_solved_dev(rio_gp_t* h) { return h ? h->assign[h->cur ^ 1] : nullptr; }

// ---- CRUD ---------------------------------------------------------------------------------

int rio_gp_lookup_batch_dev(rio_gp_t* h, uint64_t n, const uint32_t* d_idx, uint32_t* d_out) {
    if (!h || (n && (!d_idx || !d_out))) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipSetDevice(h->device));
    int rc = zero_stats(h);
    if (rc) return rc;
    launch_lookup(h->assign[h->cur], h->n, d_idx, n, d_out, h->dstats, h->stream);
    if ((rc = read_stats(h))) return rc;
    if (h->h_stats[0].err) return fail(h, RIO_GP_EINVAL, "rio_gp_lookup_batch: object index out of range");
    return RIO_GP_OK;
}

int rio_gp_lookup_batch(rio_gp_t* h, uint64_t n, const uint32_t* idx, uint32_t* out_node) {
    if (!h || (n && (!idx || !out_node))) return RIO_GP_EINVAL;
    Locked g(h);
    for (uint64_t k = 0; k < n; ++k)
        if (idx[k] >= h->n) return fail(h, RIO_GP_EINVAL, "rio_gp_lookup_batch: object index out of range");
    if (!n) return RIO_GP_OK;
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if (n <= (uint64_t)kSmallBatch) {  // micro-batch: the gather reads and writes mapped pinned memory, one launch + wait
        SmallInline inl;
        const bool in_args = small_inline(&inl, n, idx, nullptr);  // n <= 4: the requests ride in the kernel arguments
        if (!in_args) memcpy(h->h_small, idx, n * sizeof(u32));
        const u32 seq = small_begin(h);
        launch_lookup_small(h->assign[h->cur], h->n, h->d_small, (u32)n, h->d_small + 2 * kSmallBatch, h->dstats, h->stream,
                            small_done_dev(h), seq, in_args ? &inl : nullptr);
        if ((rc = small_wait(h, seq))) return rc;
        memcpy(out_node, h->h_small + 2 * kSmallBatch, n * sizeof(u32));
        return RIO_GP_OK;
    }
    if (n <= (uint64_t)kMidBatch) {
        // medium batch: indices and results in mapped pinned memory, a few workgroups, the last one stores the completion
        // word — no staging copies through the runtime, no stream wait (1 000 lookups: 29.5 -> ~13 us per call)
        memcpy(h->h_mid, idx, n * sizeof(u32));
        const u32 seq = small_begin(h);
        launch_lookup(h->assign[h->cur], h->n, h->d_mid, n, h->d_mid + kMidBatch, h->dstats, h->stream, small_done_dev(h), seq,
                      h->mid_ticket);
        if ((rc = small_wait(h, seq))) return rc;
        memcpy(out_node, h->h_mid + kMidBatch, n * sizeof(u32));
        return RIO_GP_OK;
    }
    if ((rc = ensure(h, h->stage[0], n * sizeof(u32))) || (rc = ensure(h, h->stage[1], n * sizeof(u32)))) return rc;
    u32 *d_idx = (u32*)h->stage[0].p, *d_out = (u32*)h->stage[1].p;
    HIPCHK(h, hipMemcpyAsync(d_idx, idx, n * sizeof(u32), hipMemcpyHostToDevice, h->stream));
    launch_lookup(h->assign[h->cur], h->n, d_idx, n, d_out, h->dstats, h->stream);
    HIPCHK(h, hipMemcpyAsync(out_node, d_out, n * sizeof(u32), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    return RIO_GP_OK;
}

// End of a synchronous call of the window-partitioned kernels: the error counter and the completion word arrive in mapped host
// memory (k_finish_err); no counter copy-back, no hipStreamSynchronize.
static int finish_err(rio_gp* h, const char* what) {
    const u32 seq = small_begin(h);
    h->h_small[4 * kSmallBatch] = 0;
    launch_finish_err(h->dstats, h->d_small + 4 * kSmallBatch, small_done_dev(h), seq, h->stream);
    int rc = small_wait(h, seq);
    if (rc) return rc;
    if (h->h_small[4 * kSmallBatch]) return fail(h, RIO_GP_EINVAL, what);
    return RIO_GP_OK;
}

static int update_dev_locked(rio_gp* h, uint64_t n, const uint32_t* d_idx, const uint32_t* d_node) {
    int rc = zero_stats(h);
    if (rc) return rc;
    if (h->part_mode != 2 && part_applicable(h->n, n, d_idx, d_node)) {  // big batch: binned by row window, elected in LDS, written densely
        if ((rc = ensure(h, h->part, part_scratch_words(h->n, n) * sizeof(u32)))) return rc;
        launch_update_part(h->assign[h->cur], h->n, h->m, d_idx, d_node, n, (u32*)h->part.p, h->dstats, h->stream, aff_life(h));
        h->used.invalidate();
        inputs_changed(h);
        return finish_err(h, "rio_gp_update_batch: invalid entries were skipped");
    } else {
        launch_update(h->assign[h->cur], h->n, h->m, d_idx, d_node, n, h->pos, h->dstats, h->stream, aff_life(h));
    }
    h->used.invalidate();
    inputs_changed(h);
    if ((rc = read_stats(h))) return rc;
    if (h->h_stats[0].err) return fail(h, RIO_GP_EINVAL, "rio_gp_update_batch: invalid entries were skipped");
    return RIO_GP_OK;
}

int rio_gp_update_batch_dev(rio_gp_t* h, uint64_t n, const uint32_t* d_idx, const uint32_t* d_node) {
    if (!h || (n && (!d_idx || !d_node))) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipSetDevice(h->device));
    return update_dev_locked(h, n, d_idx, d_node);
}

int rio_gp_update_batch(rio_gp_t* h, uint64_t n, const uint32_t* idx, const uint32_t* node) {
    if (!h || (n && (!idx || !node))) return RIO_GP_EINVAL;
    Locked g(h);
    for (uint64_t k = 0; k < n; ++k)
        if (idx[k] >= h->n || (node[k] != RIO_GP_NONE && node[k] >= h->m))
            return fail(h, RIO_GP_EINVAL, "rio_gp_update_batch: index or node out of range");
    if (!n) return RIO_GP_OK;
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if (n <= (uint64_t)kSmallBatch) {
        // micro-batch (one first-touch update per activation in the reference flow, service.rs:244-252): the entries were
        // validated above, so the kernels read them from mapped pinned memory and nothing is copied, zeroed or read back
        SmallInline inl;
        const bool in_args = small_inline(&inl, n, idx, node);
        if (!in_args) {
            memcpy(h->h_small, idx, n * sizeof(u32));
            memcpy(h->h_small + kSmallBatch, node, n * sizeof(u32));
        }
        const u32 seq = small_begin(h);
        // `used` follows the writes when it is valid (k_remove_small does the same): a server that mixes single updates with
        // policy calls does not re-stream the whole table before every place_pending
        u64* const used = h->used.live();
        launch_update_small(h->assign[h->cur], h->d_small, h->d_small + kSmallBatch, (u32)n, h->stream, aff_life(h),
                            small_done_dev(h), seq, in_args ? &inl : nullptr, used, h->load, h->m);
        inputs_changed(h);
        return small_wait(h, seq);
    }
    if (n <= (uint64_t)kMidBatch) {
        // medium batch, validated above: the election and the apply kernel read the entries from mapped pinned memory, the
        // apply kernel's last workgroup stores the completion word — no staging copies, no counter read-back, no stream wait
        memcpy(h->h_mid, idx, n * sizeof(u32));
        memcpy(h->h_mid + kMidBatch, node, n * sizeof(u32));
        const u32 seq = small_begin(h);
        u64* const used = h->used.live();
        launch_update(h->assign[h->cur], h->n, h->m, h->d_mid, h->d_mid + kMidBatch, n, h->pos, h->dstats, h->stream, aff_life(h),
                      h->mid_ticket, small_done_dev(h), seq, used, h->load);
        inputs_changed(h);
        return small_wait(h, seq);
    }
    if ((rc = ensure(h, h->stage[0], n * sizeof(u32))) || (rc = ensure(h, h->stage[1], n * sizeof(u32)))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->stage[0].p, idx, n * sizeof(u32), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->stage[1].p, node, n * sizeof(u32), hipMemcpyHostToDevice, h->stream));
    return update_dev_locked(h, n, (const u32*)h->stage[0].p, (const u32*)h->stage[1].p);
}

static int remove_dev_locked(rio_gp* h, uint64_t n, const uint32_t* d_idx) {
    int rc = zero_stats(h);
    if (rc) return rc;
    u64* const used = h->used.live();
    if (h->part_mode != 2 && part_applicable(h->n, n, d_idx, nullptr)) {
        if ((rc = ensure(h, h->part, part_scratch_words(h->n, n) * sizeof(u32)))) return rc;
        launch_remove_part(h->assign[h->cur], h->n, h->m, h->load, d_idx, n, (u32*)h->part.p, used,
                           h->dstats, h->stream, aff_life(h));
        inputs_changed(h);
        return finish_err(h, "rio_gp_remove_batch: invalid entries were skipped");
    } else {
        launch_remove(h->assign[h->cur], h->n, h->m, h->load, d_idx, n, used, h->dstats,
                      h->stream, aff_life(h));
    }
    inputs_changed(h);
    if ((rc = read_stats(h))) return rc;
    if (h->h_stats[0].err) return fail(h, RIO_GP_EINVAL, "rio_gp_remove_batch: invalid entries were skipped");
    return RIO_GP_OK;
}

int rio_gp_remove_batch_dev(rio_gp_t* h, uint64_t n, const uint32_t* d_idx) {
    if (!h || (n && !d_idx)) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipSetDevice(h->device));
    return remove_dev_locked(h, n, d_idx);
}

int rio_gp_remove_batch(rio_gp_t* h, uint64_t n, const uint32_t* idx) {
    if (!h || (n && !idx)) return RIO_GP_EINVAL;
    Locked g(h);
    for (uint64_t k = 0; k < n; ++k)
        if (idx[k] >= h->n) return fail(h, RIO_GP_EINVAL, "rio_gp_remove_batch: object index out of range");
    if (!n) return RIO_GP_OK;
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if (n <= (uint64_t)kSmallBatch) {  // micro-batch: validated above, read from mapped pinned memory, one launch + one wait
        SmallInline inl;
        const bool in_args = small_inline(&inl, n, idx, nullptr);
        if (!in_args) memcpy(h->h_small, idx, n * sizeof(u32));
        const u32 seq = small_begin(h);
        u64* const used = h->used.live();
        launch_remove_small(h->assign[h->cur], h->m, h->load, h->d_small, (u32)n, used, h->stream,
                            aff_life(h), small_done_dev(h), seq, in_args ? &inl : nullptr);
        inputs_changed(h);
        return small_wait(h, seq);
    }
    if (n <= (uint64_t)kMidBatch) {  // medium batch, validated above: as update_batch
        memcpy(h->h_mid, idx, n * sizeof(u32));
        const u32 seq = small_begin(h);
        u64* const used = h->used.live();
        launch_remove(h->assign[h->cur], h->n, h->m, h->load, h->d_mid, n, used, h->dstats,
                      h->stream, aff_life(h), small_done_dev(h), seq, nullptr, h->mid_ticket);
        inputs_changed(h);
        return small_wait(h, seq);
    }
    if ((rc = ensure(h, h->stage[0], n * sizeof(u32)))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->stage[0].p, idx, n * sizeof(u32), hipMemcpyHostToDevice, h->stream));
    return remove_dev_locked(h, n, (const u32*)h->stage[0].p);
}

int rio_gp_clean_servers(rio_gp_t* h, const uint64_t* dead_bitmap, uint64_t* evicted) {
    if (!h || !dead_bitmap) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipSetDevice(h->device));
    // one launch + one wait: the kernel reads the bitmap from mapped pinned memory and its last workgroup writes the
    // evicted count back into it (no staging copy, no counter memset, no copy-back)
    const u32 words32 = (h->m + 31) / 32;
    u64* h_count = reinterpret_cast<u64*>(h->h_cs + h->cs_words);
    *h_count = 0;
    if (evicted) *evicted = 0;
    if (!words32) return RIO_GP_OK;
    bool any = false;
    for (u32 w = 0; w < words32; ++w) h->h_cs[w] = 0;
    for (u32 j = 0; j < h->m; ++j)
        if ((dead_bitmap[j >> 6] >> (j & 63)) & 1ull) { h->h_cs[j >> 5] |= 1u << (j & 31); any = true; }
    inputs_changed(h);
    if (!any || h->n == 0) return RIO_GP_OK;  // retain() with a predicate nothing matches, or over an empty map
    const u32 seq = (small_begin(h) & 0xFFFFFFu) | 0x800000u;  // 24 bits, never 0
    u64* const used = h->used.live();  // (k_clean zeroes the dead nodes' entries: what the last solve's rounds admitted there must be in first)
    launch_clean(h->assign[h->cur], h->n, h->m, h->d_cs, used, h->dstats, h->stream,
                 h->cs_cnt, h->cs_ticket, reinterpret_cast<u64*>(h->d_cs + h->cs_words), aff_life(h), seq);
    {   // the last workgroup stores total | seq << 40 into mapped pinned memory: spin on the tag, ask the stream after 50 ms
        volatile u64* w = h_count;
        const auto t0 = std::chrono::steady_clock::now();
        u32 spins = 0;
        while ((*w >> 40) != seq) {
            __builtin_ia32_pause();
            if ((++spins & 0xFFFu) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) break;
        }
        if ((*w >> 40) != seq) {
            HIPCHK(h, hipStreamSynchronize(h->stream));
            HIPCHK(h, hipGetLastError());
            if ((*w >> 40) != seq) return fail(h, RIO_GP_EUPSTREAM, "rio_gp_clean_servers: the kernel left no total");
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (evicted) *evicted = *h_count & ((1ull << 40) - 1);
    return RIO_GP_OK;
}

int rio_gp_clean_server(rio_gp_t* h, uint32_t node, uint64_t* evicted) {
    if (!h) return RIO_GP_EINVAL;
    u32 m;
    {
        Locked g(h);
        m = h->m;
        if (node >= m) {  // an address nothing was ever placed on: retain() removes nothing (local.rs:56)
            if (evicted) *evicted = 0;
            return RIO_GP_OK;
        }
    }
    std::vector<uint64_t> bm((m + 63) / 64 + 1, 0);
    bm[node >> 6] |= 1ull << (node & 63);
    return rio_gp_clean_servers(h, bm.data(), evicted);
}

// MembershipStorage::remove (cluster/storage/mod.rs:77) for the dense table: DESIGN.md section 2 rule 8.  The map is checked on
// the host (at most RIO_GP_MAX_NODES entries) before anything changes; then one launch of k_remap over the committed column, the
// affinity column and the feed's checkpoint, rows 0 .. n_hi-1.  The other assignment column needs no pass: the solve it may hold
// is dropped, a later solve writes its rows < n, and commit_enqueue copies the rows [n, n_hi) over from the committed column
// before it swaps.
int rio_gp_remap_nodes(rio_gp_t* h, uint32_t m_new, const uint32_t* map, uint64_t* evicted) {
    static_assert(kRemapMaxNodes == RIO_GP_MAX_NODES && kNodeGone == RIO_GP_NODE_GONE, "k_remap's constants follow the header");
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    if (!map) return fail(h, RIO_GP_EINVAL, "rio_gp_remap_nodes: map is NULL");
    if (int rc = refuse_row_sharded(h, "rio_gp_remap_nodes")) return rc;
    const u32 m = h->m;
    if (m_new > m) return fail(h, RIO_GP_EINVAL, "rio_gp_remap_nodes: m_new exceeds the node count");
    std::vector<u32> from(m_new ? m_new : 1, kNone);  // new id -> old id
    u32 kept = 0;
    for (u32 j = 0; j < m; ++j) {
        if (map[j] == RIO_GP_NONE) continue;
        if (map[j] >= m_new) return fail(h, RIO_GP_EINVAL, "rio_gp_remap_nodes: a kept node's new id is not below m_new");
        if (from[map[j]] != kNone) return fail(h, RIO_GP_EINVAL, "rio_gp_remap_nodes: two nodes map to the same id");
        from[map[j]] = j;
        ++kept;
    }
    if (kept != m_new) return fail(h, RIO_GP_EINVAL, "rio_gp_remap_nodes: fewer than m_new nodes are kept");
    HIPCHK(h, hipSetDevice(h->device));
    if (evicted) *evicted = 0;
    // a change of the inputs, like every CRUD call: an uncommitted solve is dropped, the next tick is neither quiet nor chained
    inputs_changed(h);
    h->last.forget_pending();
    int rc;
    u32 G = 0;
    if (m && h->n_hi) {
        if ((rc = ensure(h, h->stage[0], (size_t)m * sizeof(u32)))) return rc;
        HIPCHK(h, hipMemcpyAsync(h->stage[0].p, map, (size_t)m * sizeof(u32), hipMemcpyHostToDevice, h->stream));
        G = launch_remap(h->assign[h->cur], h->aff, h->chg_B, h->n_hi, h->n, m, (const u32*)h->stage[0].p, h->lifecycle,
                         h->sb.blkstat, h->stream);
        HIPCHK(h, hipGetLastError());
        // `used` is the one of the new column: rebuilt from it before its next use (nothing left to fold)
        h->used.invalidate();
    }
    // the node table: cap and alive of node j move to map[j]; h_alive already holds every liveness push, delivered or not, so
    // the device bitmap is written whole from it
    std::vector<u64> cap(m ? m : 1), cap2(m_new ? m_new : 1);
    std::vector<u64> blk((size_t)(G ? G : 1) * 4, 0);
    if (m) HIPCHK(h, hipMemcpyAsync(cap.data(), h->cap, (size_t)m * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    if (G) HIPCHK(h, hipMemcpyAsync(blk.data(), h->sb.blkstat, (size_t)G * 4 * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<uint8_t> alive2(m_new);
    h->all_alive = true;
    for (u32 k = 0; k < m_new; ++k) {
        cap2[k] = cap[from[k]];
        alive2[k] = h->h_alive[from[k]];
        h->all_alive = h->all_alive && alive2[k];
    }
    h->h_alive.swap(alive2);
    h->m = m_new;
    h->alive_dirty = false;
    if (m_new) {
        HIPCHK(h, hipMemcpyAsync(h->cap, cap2.data(), (size_t)m_new * sizeof(u64), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->alive_bytes, h->h_alive.data(), m_new, hipMemcpyHostToDevice, h->stream));
    }
    launch_pack_alive(h->alive_bytes, m_new, h->alive_bits, h->stream);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (m_new != m) h->used.invalidate();
    u64 ev = 0;
    for (u32 b = 0; b < G; ++b) ev += blk[(size_t)b * 4 + 1];
    if (evicted) *evicted = ev;
    return RIO_GP_OK;
}

// ---- policy -------------------------------------------------------------------------------

// The general path of place_pending (any batch the one-workgroup kernels do not finish): the window-sorted form for big dense
// batches, else k_ppm_first -> [k_clean] -> k_ppm_gather -> solve of the virtual table against the committed `used` (same
// kernels, VIRT) -> [fix-up] -> k_ppm_output, with nothing waiting on the host in between (placement_kernels.hip).
// d_idx / d_req / d_out / d_flag: device-resident arrays, or (host_io) rows of mapped pinned host memory — then the first
// kernel leaves device copies of the requests for the kernels behind it and the last one writes the results over PCIe.
// Synchronous: returns when the results are in d_out / d_flag.  dev_api: the entries were NOT validated on the host.
static int place_pending_general(rio_gp* h, uint64_t n, const u32* d_idx, const u32* d_req, u32* d_out, u32* d_flag,
                                 bool host_io, bool dev_api) {
    flush_alive(h);  // the request kernels read the device's liveness bitmap
    int rc;
    const size_t bytes = n * sizeof(u32);
    for (int q = 0; q < 4; ++q)
        if ((rc = ensure(h, h->vt[q], bytes))) return rc;
    u32 *vcur = (u32*)h->vt[0].p, *vload = (u32*)h->vt[1].p, *vaff = (u32*)h->vt[2].p, *vnext = (u32*)h->vt[3].p;
    u32* assign = h->assign[h->cur];
    h->sb.fx = FxRows{};  // nobody reads the fix-up counters of the virtual-table solve: plain DevStats atomics, no pinned slot touched
    u64* const used = h->used.ensure();
    const char* const who = dev_api ? "rio_gp_place_pending_dev" : "rio_gp_place_pending";
    if (h->part_mode != 2 && !host_io && pp_win_applicable(h->n, n, d_idx, d_req) &&
        (((uintptr_t)d_out | (uintptr_t)d_flag) & 15u) == 0) {  // (its output kernels store whole vectors)
        // Big batch: sorted by row window once, the row-side step out of LDS (k_pp_win_gather), the decisions written into the
        // real column by the solve itself: two random accesses per request instead of nine.  The entries are validated by the
        // binning kernel, which changes nothing.
        if ((rc = ensure(h, h->part, part_scratch_words(h->n, n) * sizeof(u32))) || (rc = ensure(h, h->vrec, n * sizeof(uint2)))) return rc;
        // An invalid entry makes the call fail with nothing changed, and nobody waits to find out: the binning kernel raises a
        // flag in mapped host memory and a device counter, every kernel enqueued behind it looks at the counter and does
        // nothing (k_scan solves an empty table), and the host reads the flag when it picks up the verdict.
        if ((rc = zero_stats(h))) return rc;
        u32* const h_bad = h->h_cs + h->cs_words + 2;
        *h_bad = 0;
        u32* const h_status = h->h_small + 4 * kSmallBatch;
        *h_status = 0;
        launch_pp_bin(h->n, h->m, d_idx, d_req, n, (u32*)h->part.p, h->dstats, h->d_cs + h->cs_words + 2, h->stream, h->dead_bits,
                      h->pp_claim);
        // The window kernel answers every request it can by itself — sticky hits, first touches on requesters that are active
        // members, later requests of an object — and records what the first touches ask of every requester; when every total
        // fits (k_pp_win_verdict) the answers are final and k_pp_win_split hands them out: no virtual table, no solve.
        launch_pp_win_gather(assign, h->load, h->n, h->m, h->alive_bits, n, (const u32*)h->part.p, vaff, vnext, h->dead_bits,
                             aff_life(h), h->dstats, h->pp_claim, h->stream);
        if (!h->all_alive)  // service.rs:227-237: every object of a dead node a request ran into is un-placed
            launch_clean(assign, h->n, h->m, h->dead_bits, used, h->dstats, h->stream, nullptr, nullptr, nullptr, aff_life(h));
        launch_pp_win_verdict(h->m, h->cap, h->alive_bits, used, h->pp_claim, h->dstats, h->pp_bad + 1, h->d_small + 4 * kSmallBatch,
                              h->stream);
        // (the answers' two words sit in vaff / vnext, in the sorted order, until here: the solve below writes vnext afterwards)
        launch_pp_win_unsort(h->n, (const u32*)h->part.p, vaff, vnext, n, (uint2*)h->vrec.p, d_out, d_flag, h->pp_bad + 1, h->stream);
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipGetLastError());
        if (*h_bad || *h_status == 3) return fail(h, RIO_GP_EINVAL, std::string(who) + ": object index or requester out of range (nothing was changed)");
        if (*h_status == 1) {  // final: `used` has taken the claims in place
            inputs_changed(h);
            return RIO_GP_OK;
        }
        if (*h_status != 2) return fail(h, RIO_GP_EUPSTREAM, std::string(who) + ": the window kernels left no verdict");
        // The batch needs the solve (a requester would run full, a dead node was in the way, a requester is not an active
        // member): over the same records, the window kernel's placements standing as the optimistic ones.  The solve's kernels
        // read whole tiles of the object and requester columns: they get padded copies (the caller's arrays end where they end).
        if ((rc = ensure(h, h->stage[0], bytes)) || (rc = ensure(h, h->stage[1], bytes))) return rc;
        HIPCHK(h, hipMemcpyAsync(h->stage[0].p, d_idx, bytes, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->stage[1].p, d_req, bytes, hipMemcpyDeviceToDevice, h->stream));
        d_idx = (const u32*)h->stage[0].p;
        d_req = (const u32*)h->stage[1].p;
        Plan vp = hplan(h, n);
        const u64 seq = ++h->wait_seq;
        vp.mark = seq;
        Table vtab{vcur, vload, d_req /* the requesters ARE the affinity column of the virtual table */, vnext};
        vtab.pk_idx = d_idx;      // virtual row -> real row: every decision of the solve also goes to assign[d_idx[k]]
        vtab.real_next = assign;  // (in place: the rows that change are pending, nothing else reads them before the outputs)
        vtab.vrec = (const uint2*)h->vrec.p;  // the scan reads the records and writes vcur / vload for the kernels behind it
        vtab.prewritten = true;               // k_pp_win_gather has put the alive requesters' first touches into the column
        const NodeTab vnt{h->cap, h->alive_bits, used};
        h->sb.D = h->D;
        launch_scan(vp, vtab, vnt, h->sb, true, h->all_alive, h->stream);
        launch_resolve(vp, vnt, h->sb, slot_dev(h, 0), h->stream);
        enqueue_slow(h, SolveForm{}, vp, vtab, vnt, true);  // ahead of the verdict: its kernels guard themselves on the device
        launch_pp_win_output(d_idx, d_req, n, vcur, vload, vnext, h->alive_bits, h->sb.cutidx, h->m, d_out, d_flag, aff_life(h), h->dstats,
                             h->stream, h->sa, (const uint2*)h->vrec.p);
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipGetLastError());
        const DevStats v = reduce_slot(h, 0, h->m);
        const bool vslow = needs_fixup(v);
        h->used.publish_request(vslow);
        inputs_changed(h);
        return RIO_GP_OK;
    }
    // The library's own (padded) copies of the requests, made by the first kernel on its way: requests in mapped host memory
    // are read over PCIe once — and a caller's device arrays end where they end, while the solve's kernels read whole tiles
    // (the requesters are the affinity column of the virtual table): past the end of an exact-size array that is somebody
    // else's page (found by the fuzz: a memory access fault at sizes a few hundred bytes short of a page).
    u32 *s_idx = nullptr, *s_req = nullptr, *vflag = nullptr;
    if ((rc = ensure(h, h->stage[0], bytes)) || (rc = ensure(h, h->stage[1], bytes))) return rc;
    s_idx = (u32*)h->stage[0].p; s_req = (u32*)h->stage[1].p;
    const bool mark = !h->all_alive;  // (1) service.rs:227-237 — requested rows on dead nodes trigger clean_server of those nodes
    if (mark) {
        if ((rc = ensure(h, h->stage[2], bytes))) return rc;
        vflag = (u32*)h->stage[2].p;
    }
    u32* const h_status = h->h_small + 4 * kSmallBatch;
    u32* const d_status = h->d_small + 4 * kSmallBatch;
    *h_status = 2;  // neither 0, 1 nor 3: the output kernel must write it
    launch_ppm_first(assign, h->n, h->m, h->alive_bits, d_idx, d_req, n, h->pos, s_idx, s_req, mark ? h->dead_bits : nullptr, vflag,
                     h->pp_bad, h->stream);
    const u32* const k_idx = s_idx;
    const u32* const k_req = s_req;
    (void)host_io;
    if (mark) launch_clean(assign, h->n, h->m, h->dead_bits, used, h->dstats, h->stream, nullptr, nullptr, nullptr, aff_life(h), 0, h->pp_bad);
    // (2)(3) the virtual table (rows = requests): the first request per row decides
    launch_ppm_gather(assign, h->load, k_idx, n, h->pos, vcur, vload, vaff /* position of the row's first request */, h->pp_bad, h->stream);
    // (4) solve it against the committed `used`
    Plan vp = hplan(h, n);
    const u64 mk = ++h->wait_seq;
    vp.mark = mk;
    Table vtab{vcur, vload, k_req /* the requesters ARE the affinity column of the virtual table */, vnext};
    vtab.skip_if = h->pp_bad;
    const NodeTab vnt{h->cap, h->alive_bits, used};  // (ensure() above folded whatever the last solve's rounds had left)
    h->sb.D = h->D;
    launch_scan(vp, vtab, vnt, h->sb, true, h->all_alive, h->stream);
    launch_resolve(vp, vnt, h->sb, slot_dev(h, 0), h->stream);
    // the fix-up ahead of the verdict when the last batch needed it (its kernels guard themselves on the device); otherwise the
    // output kernel finds out on the device and hands back status 1 having changed nothing
    bool fixed = h->spec_mode != 2 && (h->spec_mode == 1 || h->pp_last_slow);
    if (fixed) enqueue_slow(h, SolveForm{}, vp, vtab, vnt, true);
    // (5) publish, outputs, scratch reset, completion word
    u32 seq = small_begin(h);
    launch_ppm_output(assign, h->n, k_idx, k_req, n, vcur, vnext, vaff, vflag, h->pos, h->alive_bits, h->sb, vp, d_out, d_flag,
                      aff_life(h), h->pp_bad, fixed, d_status, h->mid_ticket, small_done_dev(h), seq, h->stream);
    if ((rc = small_wait(h, seq))) return rc;
    if (*h_status == 1 && !fixed) {
        enqueue_slow(h, SolveForm{}, vp, vtab, vnt, true);
        fixed = true;
        *h_status = 2;
        seq = small_begin(h);
        launch_ppm_output(assign, h->n, k_idx, k_req, n, vcur, vnext, vaff, vflag, h->pos, h->alive_bits, h->sb, vp, d_out, d_flag,
                          aff_life(h), h->pp_bad, true, d_status, h->mid_ticket, small_done_dev(h), seq, h->stream);
        if ((rc = small_wait(h, seq))) return rc;
    }
    HIPCHK(h, hipGetLastError());
    if (*h_status == 3) return fail(h, RIO_GP_EINVAL, std::string(who) + ": object index or requester out of range (nothing was changed)");
    if (*h_status != 0) return fail(h, RIO_GP_EUPSTREAM, std::string(who) + ": the output kernel left no status");
    const DevStats v = reduce_slot(h, 0, h->m);  // (k_resolve's pinned rows landed before the completion word)
    const bool vslow = needs_fixup(v);
    h->pp_last_slow = vslow;
    h->used.publish_request(vslow);
    inputs_changed(h);
    return RIO_GP_OK;
}

// One pass over a caller's array: copy it into the mapped pinned row the kernels read, and find its largest entry on the way
// (a branch-free loop the compiler vectorises: the validation of a request batch costs no pass of its own and no early-exit
// branch per entry — 262 143 requests: a scalar check-then-memcpy was most of the call's host time).
static inline u32 copy_max(u32* __restrict__ dst, const u32* __restrict__ src, size_t n) {
    u32 mx = 0;
    for (size_t k = 0; k < n; ++k) {
        const u32 v = src[k];
        dst[k] = v;
        mx = v > mx ? v : mx;
    }
    return mx;
}
static inline u32 max_of(const u32* __restrict__ src, size_t n) {
    u32 mx = 0;
    for (size_t k = 0; k < n; ++k) mx = src[k] > mx ? src[k] : mx;
    return mx;
}

// rio_gp_place_pending with the handle locked; the entries are validated here (on their way into the pinned rows) unless
// `validated` says the caller has; micro_tried: the one-workgroup kernel has already run over this batch and handed it over
// untouched (rio_gp_mixed_batch)
static int place_pending_host_locked(rio_gp* h, uint64_t n, const uint32_t* idx, const uint32_t* requester, uint32_t* out_node,
                                     uint32_t* out_flag, bool micro_tried, bool validated = true) {
    static const char* const kRange = "rio_gp_place_pending: object index or requester out of range";
    flush_alive(h);
    int rc;
    if (!validated && n <= (uint64_t)kSmallBatch) {
        if (max_of(idx, n) >= h->n || max_of(requester, n) >= h->m) return fail(h, RIO_GP_EINVAL, kRange);
        validated = true;
    }
    if (n <= (uint64_t)kSmallBatch && !micro_tried) {
        // micro-batch: one workgroup, one launch, request/result arrays in mapped pinned memory (no staging copies)
        u64* const used = h->used.ensure();
        u32 *hs = h->h_small, *ds = h->d_small;
        SmallInline inl;
        const bool in_args = small_inline(&inl, n, idx, requester);
        if (!in_args) {
            memcpy(hs, idx, n * sizeof(u32));
            memcpy(hs + kSmallBatch, requester, n * sizeof(u32));
        }
        hs[4 * kSmallBatch] = 2;  // neither 0 nor 1: the kernel must write it
        const u32 seq = small_begin(h);
        launch_pp_one(h->assign[h->cur], h->load, h->m, h->cap, h->alive_bits, used, ds, ds + kSmallBatch,
                      (u32)n, ds + 2 * kSmallBatch, ds + 3 * kSmallBatch, ds + 4 * kSmallBatch, h->stream, aff_life(h),
                      small_done_dev(h), seq, in_args ? &inl : nullptr, 0, nullptr, nullptr, h->sa);
        if ((rc = small_wait(h, seq))) return rc;
        const u32 status = hs[4 * kSmallBatch];
        if (status == 0) {
            memcpy(out_node, hs + 2 * kSmallBatch, n * sizeof(u32));
            if (out_flag) memcpy(out_flag, hs + 3 * kSmallBatch, n * sizeof(u32));
            inputs_changed(h);
            return RIO_GP_OK;
        }
        if (status != 1) return fail(h, RIO_GP_EUPSTREAM, "rio_gp_place_pending: micro-batch kernel left no status");
        // status 1: a dead node / dead or full requester is involved — nothing was changed, take the general path
    }
    const size_t bytes = n * sizeof(u32);
    if (n <= (uint64_t)kMidBatch / 4) {
        // medium batch (<= 4 096 requests): requests and results in mapped pinned memory, the last kernel's last workgroup
        // stores the completion word: no staging copies, no stream wait
        u32* hm = h->h_mid;
        u32* dm = h->d_mid;
        const u32 mi = copy_max(hm, idx, n), mr = copy_max(hm + kMidBatch, requester, n);
        if (!validated && (mi >= h->n || mr >= h->m)) return fail(h, RIO_GP_EINVAL, kRange);
        if (n > (uint64_t)kSmallBatch) {
            // first the one-workgroup kernel (k_pp_one, 1024 threads x 4 requests): sticky hits and first touches that fit —
            // the whole call is ONE launch and one wait (4 096 requests: 46 -> ~15 us); anything heavier hands over untouched
            u64* const used = h->used.ensure();
            h->h_small[4 * kSmallBatch] = 2;
            const u32 seq1 = small_begin(h);
            launch_pp_one(h->assign[h->cur], h->load, h->m, h->cap, h->alive_bits, used, dm, dm + kMidBatch, (u32)n,
                          dm + 2 * kMidBatch, dm + 3 * kMidBatch, h->d_small + 4 * kSmallBatch, h->stream, aff_life(h),
                          small_done_dev(h), seq1, nullptr, 0, h->pp_stage, h->mid_ticket, h->sa, true);
            if ((rc = small_wait(h, seq1))) return rc;
            const u32 status = h->h_small[4 * kSmallBatch];
            if (status == 0) {
                memcpy(out_node, hm + 2 * kMidBatch, bytes);
                if (out_flag) memcpy(out_flag, hm + 3 * kMidBatch, bytes);
                inputs_changed(h);
                return RIO_GP_OK;
            }
            if (status != 1) return fail(h, RIO_GP_EUPSTREAM, "rio_gp_place_pending: one-workgroup kernel left no status");
        }
        if ((rc = place_pending_general(h, n, dm, dm + kMidBatch, dm + 2 * kMidBatch, dm + 3 * kMidBatch, true, false))) return rc;
        memcpy(out_node, hm + 2 * kMidBatch, bytes);
        if (out_flag) memcpy(out_flag, hm + 3 * kMidBatch, bytes);
        return RIO_GP_OK;
    }
    if (n <= (uint64_t)kReqBatch) {
        // up to 65 536 requests: requests and results in mapped pinned memory — the first kernel of the general path reads them
        // over PCIe once (and leaves device copies), the last one writes the results back; no staging copies through the runtime
        u32* hq = h->h_req;
        u32* dq = h->d_req;
        const u32 mi = copy_max(hq, idx, n), mr = copy_max(hq + kReqBatch, requester, n);
        if (!validated && (mi >= h->n || mr >= h->m)) return fail(h, RIO_GP_EINVAL, kRange);
        if ((rc = place_pending_general(h, n, dq, dq + kReqBatch, dq + 2 * kReqBatch, dq + 3 * kReqBatch, true, false))) return rc;
        memcpy(out_node, hq + 2 * kReqBatch, bytes);
        if (out_flag) memcpy(out_flag, hq + 3 * kReqBatch, bytes);
        return RIO_GP_OK;
    }
    // Bigger batches: the runtime's copies out of and into the caller's pageable arrays (staged through its own pinned buffers:
    // ~106 us per MB and direction on this driver, tools/reg_probe.py).  The entries are validated on the DEVICE (the first kernel
    // raises a word every later kernel looks at: an invalid entry changes nothing) — no pass of the host over 2 MB.
    // Round 6 registered the caller's four arrays for the duration of the call instead (hipHostRegister / hipHostUnregister:
    // 55 us per MB, 262 143 requests 249 us instead of ~370) — and two of eight processes of the parity test aborted inside a LATER,
    // unrelated hipMemcpy into a fresh numpy array (none of eight without the registration): the runtime does not survive user pages
    // that are registered, unregistered, freed and mapped again at the same address.  Removed (docs/LESSONS.md 39); a caller that
    // wants the copy engine's rate hands over device arrays (rio_gp_place_pending_dev) or its own pinned ones.
    for (int q = 0; q < 2; ++q)
        if ((rc = ensure(h, h->rq[q], bytes)) || (rc = ensure(h, h->rq[2 + q], bytes))) return rc;
    u32 *d_idx = (u32*)h->rq[0].p, *d_req = (u32*)h->rq[1].p, *d_out = (u32*)h->rq[2].p, *d_flag = (u32*)h->rq[3].p;
    HIPCHK(h, hipMemcpyAsync(d_idx, idx, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_req, requester, bytes, hipMemcpyHostToDevice, h->stream));
    if ((rc = place_pending_general(h, n, d_idx, d_req, d_out, d_flag, false, false))) return rc;
    HIPCHK(h, hipMemcpyAsync(out_node, d_out, bytes, hipMemcpyDeviceToHost, h->stream));
    if (out_flag) HIPCHK(h, hipMemcpyAsync(out_flag, d_flag, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    return RIO_GP_OK;
}

int rio_gp_place_pending(rio_gp_t* h, uint64_t n, const uint32_t* idx, const uint32_t* requester,
                         uint32_t* out_node, uint32_t* out_flag) {
    if (!h || (n && (!idx || !requester || !out_node))) return RIO_GP_EINVAL;
    Locked g(h);
    if (!n) return RIO_GP_OK;
    if (n > 0x7FFFF000ull) return fail(h, RIO_GP_EINVAL, "rio_gp_place_pending: batch too large");
    HIPCHK(h, hipSetDevice(h->device));
    // (validated on the way into the pinned rows, before anything is enqueued: an invalid entry changes nothing)
    return place_pending_host_locked(h, n, idx, requester, out_node, out_flag, false, false);
}

// Up to kSmallBatch entries of EACH of update / remove / lookup / place_pending, executed in that order, as ONE launch and ONE
// host wait: one workgroup runs the parts one after the other (k_pp_one<256, 1> with the other parts in front of the requests,
// k_crud_small when there are no requests), a device-scope fence and a barrier between them, one completion word.  What the string layer's combiner sends when the callers of one generation
// asked for different things (a server's connections mix lookups, first touches and removals: service.rs:193-254,
// server.rs:292-304): one round trip instead of one per kind.
int rio_gp_mixed_batch(rio_gp_t* h, rio_gp_mixed* ops) {
    if (!h || !ops || ops->struct_size < sizeof(rio_gp_mixed)) return RIO_GP_EINVAL;
    const uint32_t nu = ops->n_update, nr = ops->n_remove, nl = ops->n_lookup, np = ops->n_place;
    if ((nu && (!ops->update_idx || !ops->update_node)) || (nr && !ops->remove_idx) ||
        (nl && (!ops->lookup_idx || !ops->lookup_out)) || (np && (!ops->place_idx || !ops->place_requester || !ops->place_node)))
        return RIO_GP_EINVAL;
    Locked g(h);
    if (nu > (uint32_t)kSmallBatch || nr > (uint32_t)kSmallBatch || nl > (uint32_t)kSmallBatch || np > (uint32_t)kSmallBatch)
        return fail(h, RIO_GP_EINVAL, "rio_gp_mixed_batch: at most 256 entries of each kind");
    // every kind is validated before anything is enqueued; a kind with an invalid entry is skipped as a whole (its own call
    // would have changed nothing either) and says so in rc[], the others run
    bool run[4] = {nu != 0, nr != 0, nl != 0, np != 0};
    for (int k = 0; k < 4; ++k) ops->rc[k] = RIO_GP_OK;
    for (uint32_t k = 0; k < nu && run[0]; ++k)
        if (ops->update_idx[k] >= h->n || (ops->update_node[k] != RIO_GP_NONE && ops->update_node[k] >= h->m)) {
            ops->rc[0] = fail(h, RIO_GP_EINVAL, "rio_gp_update_batch: index or node out of range");
            run[0] = false;
        }
    for (uint32_t k = 0; k < nr && run[1]; ++k)
        if (ops->remove_idx[k] >= h->n) {
            ops->rc[1] = fail(h, RIO_GP_EINVAL, "rio_gp_remove_batch: object index out of range");
            run[1] = false;
        }
    for (uint32_t k = 0; k < nl && run[2]; ++k)
        if (ops->lookup_idx[k] >= h->n) {
            ops->rc[2] = fail(h, RIO_GP_EINVAL, "rio_gp_lookup_batch: object index out of range");
            run[2] = false;
        }
    for (uint32_t k = 0; k < np && run[3]; ++k)
        if (ops->place_idx[k] >= h->n || ops->place_requester[k] >= h->m) {
            ops->rc[3] = fail(h, RIO_GP_EINVAL, "rio_gp_place_pending: object index or requester out of range");
            run[3] = false;
        }
    const int kinds = (int)run[0] + (int)run[1] + (int)run[2] + (int)run[3];
    if (!kinds) return RIO_GP_OK;
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    // staging: the place_pending entries where its own call has them (h_small); update / remove / lookup in the first row of the
    // medium-batch area (mapped pinned memory as well) — [0] update idx | [1] update node | [2] remove idx | [3] lookup idx |
    // [4] lookup out
    u32 *hm = h->h_mid, *dm = h->d_mid;
    u32 *hs = h->h_small, *ds = h->d_small;
    const u32 seq = small_begin(h);
    if (kinds >= 2) {
        // ONE launch: the update / remove / lookup parts run in front of the requests inside the one-workgroup request kernel
        // (k_pp_one<256, 1>), or alone (k_crud_small) when nobody asked for a placement
        SmallInline iu, ir, il, ip;
        CrudSmallArgs c;
        c.n_obj = h->n; c.st = h->dstats;
        if (run[3]) flush_alive(h);
        u64* const used = run[3] ? h->used.ensure() : h->used.live();  // (the request kernel reads it; the others update it)
        if (run[0]) {
            c.nu = nu; c.u_idx = dm; c.u_node = dm + kSmallBatch;
            if (small_inline(&iu, nu, ops->update_idx, ops->update_node)) c.u_inl = &iu;
            else {
                memcpy(hm, ops->update_idx, nu * sizeof(u32));
                memcpy(hm + kSmallBatch, ops->update_node, nu * sizeof(u32));
            }
        }
        if (run[1]) {
            c.nr = nr; c.r_idx = dm + 2 * kSmallBatch;
            if (small_inline(&ir, nr, ops->remove_idx, nullptr)) c.r_inl = &ir;
            else memcpy(hm + 2 * kSmallBatch, ops->remove_idx, nr * sizeof(u32));
        }
        if (run[2]) {
            c.nl = nl; c.l_idx = dm + 3 * kSmallBatch; c.l_out = dm + 4 * kSmallBatch;
            if (small_inline(&il, nl, ops->lookup_idx, nullptr)) c.l_inl = &il;
            else memcpy(hm + 3 * kSmallBatch, ops->lookup_idx, nl * sizeof(u32));
        }
        if (run[0] || run[1] || run[3]) { inputs_changed(h); }
        if (run[3]) {
            const bool in_args = small_inline(&ip, np, ops->place_idx, ops->place_requester);
            if (!in_args) {
                memcpy(hs, ops->place_idx, np * sizeof(u32));
                memcpy(hs + kSmallBatch, ops->place_requester, np * sizeof(u32));
            }
            hs[4 * kSmallBatch] = 2;  // neither 0 nor 1: the kernel must write it
            launch_pp_one(h->assign[h->cur], h->load, h->m, h->cap, h->alive_bits, used, ds, ds + kSmallBatch, np,
                          ds + 2 * kSmallBatch, ds + 3 * kSmallBatch, ds + 4 * kSmallBatch, h->stream, aff_life(h), small_done_dev(h), seq,
                          in_args ? &ip : nullptr, 0, nullptr, nullptr, h->sa, false, &c);
        } else {
            launch_crud_small(c, h->assign[h->cur], h->load, h->m, used, aff_life(h), small_done_dev(h), seq,
                              h->stream);
        }
    } else {
    SmallInline inl;
    if (run[0]) {
        const bool in_args = small_inline(&inl, nu, ops->update_idx, ops->update_node);
        if (!in_args) {
            memcpy(hm, ops->update_idx, nu * sizeof(u32));
            memcpy(hm + kSmallBatch, ops->update_node, nu * sizeof(u32));
        }
        u64* const used = h->used.live();
        launch_update_small(h->assign[h->cur], dm, dm + kSmallBatch, nu, h->stream, aff_life(h), small_done_dev(h),
                            seq, in_args ? &inl : nullptr, used, h->load, h->m);
        inputs_changed(h);
    }
    if (run[1]) {
        const bool in_args = small_inline(&inl, nr, ops->remove_idx, nullptr);
        if (!in_args) memcpy(hm + 2 * kSmallBatch, ops->remove_idx, nr * sizeof(u32));
        u64* const used = h->used.live();
        launch_remove_small(h->assign[h->cur], h->m, h->load, dm + 2 * kSmallBatch, nr, used, h->stream,
                            aff_life(h), small_done_dev(h), seq, in_args ? &inl : nullptr);
        inputs_changed(h);
    }
    if (run[2]) {
        const bool in_args = small_inline(&inl, nl, ops->lookup_idx, nullptr);
        if (!in_args) memcpy(hm + 3 * kSmallBatch, ops->lookup_idx, nl * sizeof(u32));
        launch_lookup_small(h->assign[h->cur], h->n, dm + 3 * kSmallBatch, nl, dm + 4 * kSmallBatch, h->dstats, h->stream,
                            small_done_dev(h), seq, in_args ? &inl : nullptr);
    }
    if (run[3]) {
        flush_alive(h);
        u64* const used = h->used.ensure();
        const bool in_args = small_inline(&inl, np, ops->place_idx, ops->place_requester);
        if (!in_args) {
            memcpy(hs, ops->place_idx, np * sizeof(u32));
            memcpy(hs + kSmallBatch, ops->place_requester, np * sizeof(u32));
        }
        hs[4 * kSmallBatch] = 2;  // neither 0 nor 1: the kernel must write it
        launch_pp_one(h->assign[h->cur], h->load, h->m, h->cap, h->alive_bits, used, ds, ds + kSmallBatch, np,
                      ds + 2 * kSmallBatch, ds + 3 * kSmallBatch, ds + 4 * kSmallBatch, h->stream, aff_life(h), small_done_dev(h), seq,
                      in_args ? &inl : nullptr, 0, nullptr, nullptr, h->sa);
    }
    }
    if ((rc = small_wait(h, seq))) return rc;
    if (run[2]) memcpy(ops->lookup_out, hm + 4 * kSmallBatch, nl * sizeof(u32));  // (stored by the kernel whose fence precedes the word)
    if (run[3]) {
        const u32 status = hs[4 * kSmallBatch];
        if (status == 0) {
            memcpy(ops->place_node, hs + 2 * kSmallBatch, np * sizeof(u32));
            if (ops->place_flag) memcpy(ops->place_flag, hs + 3 * kSmallBatch, np * sizeof(u32));
            inputs_changed(h);
        } else if (status == 1) {
            // a dead node / a dead or full requester is involved: nothing of the place_pending part was changed, the general path
            ops->rc[3] = place_pending_host_locked(h, np, ops->place_idx, ops->place_requester, ops->place_node, ops->place_flag, true);
        } else {
            return fail(h, RIO_GP_EUPSTREAM, "rio_gp_mixed_batch: micro-batch kernel left no status");
        }
    }
    return RIO_GP_OK;
}

int rio_gp_place_pending_dev(rio_gp_t* h, uint64_t n, const uint32_t* d_idx, const uint32_t* d_requester,
                             uint32_t* d_out_node, uint32_t* d_out_flag) {
    if (!h || (n && (!d_idx || !d_requester || !d_out_node))) return RIO_GP_EINVAL;
    Locked g(h);
    if (!n) return RIO_GP_OK;
    if (n > 0x7FFFF000ull) return fail(h, RIO_GP_EINVAL, "rio_gp_place_pending_dev: batch too large");
    // an empty table (or no nodes): every entry is out of range, and the one-workgroup kernel's "0 rows = the host has
    // validated the entries" convention must not be reached with entries nobody has looked at
    if (h->n == 0 || h->m == 0)
        return fail(h, RIO_GP_EINVAL, "rio_gp_place_pending_dev: object index or requester out of range (nothing was changed)");
    HIPCHK(h, hipSetDevice(h->device));
    flush_alive(h);
    int rc;
    if (n <= (uint64_t)kMidBatch / 4 && h->n < (1ull << 31) &&
        (((uintptr_t)d_idx | (uintptr_t)d_requester | (uintptr_t)d_out_node | (uintptr_t)d_out_flag) & 15u) == 0) {
        // up to 4 096 requests: the one-workgroup kernel first, reading the caller's device arrays in place (it validates the
        // entries itself) — ONE launch and one wait when the batch is sticky hits and first touches that fit
        u64* const used = h->used.ensure();
        h->h_small[4 * kSmallBatch] = 2;
        const u32 seq = small_begin(h);
        launch_pp_one(h->assign[h->cur], h->load, h->m, h->cap, h->alive_bits, used, d_idx, d_requester, (u32)n, d_out_node,
                      d_out_flag ? d_out_flag : h->d_mid + 3 * kMidBatch, h->d_small + 4 * kSmallBatch, h->stream, aff_life(h),
                      small_done_dev(h), seq, nullptr, (u32)h->n, h->pp_stage, h->mid_ticket, h->sa);
        if ((rc = small_wait(h, seq))) return rc;
        const u32 status = h->h_small[4 * kSmallBatch];
        if (status == 0) {
            inputs_changed(h);
            return RIO_GP_OK;
        }
        if (status == 3)
            return fail(h, RIO_GP_EINVAL, "rio_gp_place_pending_dev: object index or requester out of range (nothing was changed)");
        if (status != 1) return fail(h, RIO_GP_EUPSTREAM, "rio_gp_place_pending_dev: one-workgroup kernel left no status");
    }
    return place_pending_general(h, n, d_idx, d_requester, d_out_node, d_out_flag, false, true);
}

int rio_gp_solve(rio_gp_t* h, rio_gp_stats* stats) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipSetDevice(h->device));
    return solve_locked(h, stats);
}

int rio_gp_commit(rio_gp_t* h) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipSetDevice(h->device));
    int rc = commit_enqueue(h);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RIO_GP_OK;
}

int rio_gp_tick(rio_gp_t* h, rio_gp_stats* stats) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipSetDevice(h->device));
    return solve_locked(h, stats, true);
}

int rio_gp_tick_async(rio_gp_t* h) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h, false);  // (a quiet tick does not wait for the previous tick's k_resolve: tick_async_locked)
    HIPCHK(h, hipSetDevice(h->device));
    return tick_async_locked(h);
}

int rio_gp_tick_wait(rio_gp_t* h, rio_gp_stats* out, uint32_t cap, uint32_t* n_out) {
    if (!h || !n_out || (cap && !out)) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipSetDevice(h->device));
    int rc = harvest_ticks(h);
    if (rc) return rc;
    std::vector<rio_gp_stats>& done = h->ticks.done;
    const size_t n = done.size();
    const size_t take = n < cap ? n : cap;
    for (size_t k = 0; k < take; ++k) out[k] = done[n - take + k];  // the most recent `take`, oldest first
    *n_out = (uint32_t)n;
    done.clear();
    return RIO_GP_OK;
}

int rio_gp_solve_async(rio_gp_t* h) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipSetDevice(h->device));  // a host with several handles (one per GPU) calls from any thread
    SolveRing& ring = h->solves;
    int rc = may_start(h, Client::solve_async);
    if (rc) return rc;
    // the verdict ring holds kRing solves: fold their verdicts into the running count before the slots are overwritten
    // (rio_gp_solve_wait reports how many of ALL the solves since the last wait took the fix-up path)
    if (ring.full()) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        ring.recycle(resolve_blocks(h->m));
    }
    h->plan = hplan(h, h->n);
    use_fx_slot(h, 0);
    ring.form = solve_form(h, false, false);
    ring.last = enqueue_scan_resolve(h, ring.form, real_table(h), scan_nodes(h), slot_dev(h, ring.next_slot()));
    HIPCHK(h, hipGetLastError());
    ring.pushed(SolveRing::Owner::solves);
    inputs_changed(h);
    return RIO_GP_OK;
}

int rio_gp_solve_wait(rio_gp_t* h, rio_gp_stats* stats, uint32_t* n_slow) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (!h->solves.any_solves()) return fail(h, RIO_GP_EINVAL, "rio_gp_solve_wait: nothing enqueued");
    uint32_t slow = 0;
    DevStats last = h->solves.fold(resolve_blocks(h->m), &slow);
    if (needs_fixup(last)) {
        enqueue_slow(h, h->solves.form, h->plan, real_table(h), real_nodes(h), false);
        int rc = merge_slow(h, &last);
        if (rc) return rc;
        HIPCHK(h, hipGetLastError());
    }
    fill_stats(last, h->n, stats);
    if (n_slow) *n_slow = slow;
    h->pending = h->solves.finish();
    return RIO_GP_OK;
}

int rio_gp_solve_profiled(rio_gp_t* h, float* scan_ms, float* resolve_ms) {
    if (!h || !scan_ms || !resolve_ms) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->ev2) { HIPCHK(h, hipEventCreate(&h->ev2)); HIPCHK(h, hipEventCreate(&h->ev3)); }
    h->plan = hplan(h, h->n);
    use_fx_slot(h, 0);
    const Table t = real_table(h);
    const NodeTab nt = scan_nodes(h);
    // hipExtLaunchKernelGGL start/stop events = the dispatch's own begin/end timestamps
    h->used.fold_pending();  // (before k_resolve zeroes the D rows)
    h->sb.D = h->D;
    launch_scan(h->plan, t, nt, h->sb, false, h->all_alive, h->stream, h->ev0, h->ev1);
    launch_resolve(h->plan, nt, h->sb, slot_dev(h, 0), h->stream, h->ev2, h->ev3);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventElapsedTime(scan_ms, h->ev0, h->ev1));
    HIPCHK(h, hipEventElapsedTime(resolve_ms, h->ev2, h->ev3));
    inputs_changed(h);
    h->solves.abandon();
    const DevStats v = reduce_slot(h, 0, h->m);
    if (needs_fixup(v))
        return fail(h, RIO_GP_EINVAL, "rio_gp_solve_profiled: this table needs the cut/spill fix-up");
    return RIO_GP_OK;
}

// ---- row-sharded solve across GPUs ------------------------------------------

static int p2p_check(rio_gp* h);

int rio_gp_set_stream(rio_gp_t* h, void* hip_stream) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : h->own_stream;
    return RIO_GP_OK;
}

uint32_t rio_gp_shard_words1(rio_gp_t* h) { return h ? (uint32_t)shard_words1(h->m) : 0; }
uint32_t rio_gp_shard_words2(rio_gp_t* h) { return h ? (uint32_t)shard_words2(h->m) : 0; }

static SolveBufs local_bufs(rio_gp* h) {  // where the local sums of a shard scan go
    SolveBufs b = h->sb;
    b.RP = nullptr;
    b.R = nullptr;  // the row-sharded solve keeps the cut step and the rounds apart (the Y exchange sits between them):
    b.D = nullptr;  // no per-block rejected loads, admitted load straight into used_cur, a ranking launch per round
    b.used_kept = h->sh_lkept;
    b.claim_tot = h->sh_lclaim;
    b.used_cur = h->sh_lcur;
    b.cutblk = h->sh_lcutblk;
    b.cutidx = h->sh_lcutidx;
    return b;
}

static SolveBufs shard_bufs(rio_gp* h) {
    SolveBufs b = h->sb;
    b.RP = nullptr;
    b.R = nullptr;
    b.D = nullptr;
    b.used_snap = h->sh_gprev;  // the global `used` as the last exchange left it: what a round orders the nodes by
    b.forced_bits = h->sh_forced;
    b.rank_base = h->sh_rank_base;
    b.pending_global = h->sh_verdict;  // [0] = rows pending on all ranks, written by k_shard_import_delta
    return b;
}

// What every row-sharded solve starts with: the plan, the committed `used` whole, k_scan over this rank's rows.  Such a solve
// never works in place and never runs with sb.D (local_bufs / shard_bufs): once finished it is a plain PendingSolve{true}.
struct ShardScan { Table t; NodeTab nt; };
static ShardScan shard_scan_begin(rio_gp* h) {
    h->plan = hplan(h, h->n);
    h->sb.fx = FxRows{};  // row-sharded solve: the fix-up counters are summed in DevStats (rio_gp_shard_finish reads them)
    h->used.fold_pending();  // (nothing stays pending over a solve that publishes without D rows)
    const ShardScan s{real_table(h), real_nodes(h)};
    launch_scan(h->plan, s.t, s.nt, h->sb, false, h->all_alive, h->stream);
    return s;
}

int rio_gp_shard_scan(rio_gp_t* h, uint64_t* d_x) {
    if (!h || !d_x) return RIO_GP_EINVAL;
    Locked g(h);
    if (h->sa) return fail(h, RIO_GP_EINVAL, "row-sharded solves do not implement RIO_GP_CFG_REF_SELF_ASSIGN (single-GPU handles only)");
    const NodeTab nt = shard_scan_begin(h).nt;
    const SolveBufs lb = local_bufs(h);
    launch_resolve(h->plan, nt, lb, nullptr, h->stream);  // used_base = nullptr: purely local sums
    launch_shard_pack1(h->plan, lb, reinterpret_cast<u64*>(d_x), h->stream);
    inputs_changed(h);
    h->sh.step = ShStep::scanned;
    return RIO_GP_OK;
}

int rio_gp_shard_resolve(rio_gp_t* h, uint32_t rank, uint32_t n_ranks, const uint64_t* d_xg, void* on_stream) {
    if (!h || !d_xg || n_ranks == 0 || rank >= n_ranks) return RIO_GP_EINVAL;
    Locked g(h);
    if (!h->sh.at(ShStep::scanned)) return fail(h, RIO_GP_EINVAL, "rio_gp_shard_resolve: call rio_gp_shard_scan first");
    hipStream_t st = on_stream ? static_cast<hipStream_t>(on_stream) : h->stream;
    h->sh.bind(rank, n_ranks, on_stream ? st : nullptr);
    launch_shard_import(h->plan, real_nodes(h), shard_bufs(h), reinterpret_cast<const u64*>(d_xg), rank, n_ranks,
                        h->sh_gprev, h->sh_gfinal, h->sh_verdict, slot_dev(h, h->solves.next_slot()), st);
    h->solves.pushed_shard(1);
    h->sh.step = ShStep::resolved;
    return RIO_GP_OK;
}

int rio_gp_shard_verdict(rio_gp_t* h, rio_gp_shard_info* out, uint32_t* n_slow) {
    if (!h || !out) return RIO_GP_EINVAL;
    Locked g(h);
    if (!h->sh.at(ShStep::resolved)) return fail(h, RIO_GP_EINVAL, "rio_gp_shard_verdict: call rio_gp_shard_resolve first");
    HIPCHK(h, hipSetDevice(h->device));
    if (h->sh.side) HIPCHK(h, hipStreamSynchronize(h->sh.side));  // the exchange stream of a pipelined caller
    h->sh.side = nullptr;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->p2p && h->p2p->d_peers) { int rc = p2p_check(h); if (rc) return rc; }
    HIPCHK(h, hipGetLastError());
    u64 x[8];
    const uint32_t slow = h->solves.shard_fold(x);
    out->cut_nodes = x[0]; out->spill_rows = x[1]; out->local_fixup = x[2]; out->kept = x[3];
    out->evicted = x[4]; out->claimants = x[5]; out->load_kept = x[6]; out->load_claim = x[7];
    if (n_slow) *n_slow = slow;
    h->sh.slow = (x[0] > 0 || x[1] > 0);
    if (!h->sh.slow)  // fast path: the committed `used` is the global kept + claimed load
        HIPCHK(h, hipMemcpyAsync(h->sb.used_cur, h->sh_gfinal, (size_t)(h->m ? h->m : 1) * sizeof(u64),
                                 hipMemcpyDeviceToDevice, h->stream));
    return RIO_GP_OK;
}

int rio_gp_shard_cut(rio_gp_t* h, int run_local_fixup, uint64_t* d_y) {
    if (!h || !d_y) return RIO_GP_EINVAL;
    Locked g(h);
    if (!h->sh.at(ShStep::resolved) || !h->sh.slow) return fail(h, RIO_GP_EINVAL, "rio_gp_shard_cut: no fix-up pending");
    HIPCHK(h, hipSetDevice(h->device));
    const SolveBufs b = shard_bufs(h);
    if (run_local_fixup) {
        launch_cut_find(h->plan, real_table(h), real_nodes(h), b, false, h->stream, false);
        launch_fill(h->plan, real_table(h), real_nodes(h), b, false, true, false, 0, false, h->stream);
    }
    launch_shard_export_delta(h->plan, b, h->sb.used_kept, 0, reinterpret_cast<u64*>(d_y), h->stream);
    h->sh.step = ShStep::cut_exported;
    return RIO_GP_OK;
}

int rio_gp_shard_merge(rio_gp_t* h, const uint64_t* d_yg, uint64_t* pending_rows, uint64_t* pending_load) {
    if (!h || !d_yg) return RIO_GP_EINVAL;
    Locked g(h);
    if (!h->sh.at(ShStep::cut_exported) && !h->sh.at(ShStep::spill_exported)) return fail(h, RIO_GP_EINVAL, "rio_gp_shard_merge: nothing exported");
    HIPCHK(h, hipSetDevice(h->device));
    launch_shard_import_delta(h->plan, shard_bufs(h), reinterpret_cast<const u64*>(d_yg), h->sh.rank, h->sh.R,
                              h->sh_gprev, h->sh_verdict, slot_dev(h, 0), h->stream);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    const u64* x = h->h_slots;
    if (pending_rows) *pending_rows = x[0];
    if (pending_load) *pending_load = x[1];
    h->sh.step = ShStep::merged;
    return RIO_GP_OK;
}

int rio_gp_shard_spill(rio_gp_t* h, uint32_t round, int last, uint64_t* d_y) {
    if (!h || !d_y) return RIO_GP_EINVAL;
    Locked g(h);
    if (!h->sh.at(ShStep::merged)) return fail(h, RIO_GP_EINVAL, "rio_gp_shard_spill: call rio_gp_shard_merge first");
    HIPCHK(h, hipSetDevice(h->device));
    const SolveBufs b = shard_bufs(h);
    launch_fill(h->plan, real_table(h), real_nodes(h), b, false, false, true, (int)round, last != 0, h->stream);
    launch_shard_export_delta(h->plan, b, h->sh_gprev, (int)((round & 1) ^ 1), reinterpret_cast<u64*>(d_y), h->stream);
    h->sh.step = ShStep::spill_exported;
    return RIO_GP_OK;
}

int rio_gp_shard_finish(rio_gp_t* h, rio_gp_stats* local_stats) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    if (!h->sh.at(ShStep::resolved) && !h->sh.at(ShStep::merged))
        return fail(h, RIO_GP_EINVAL, "rio_gp_shard_finish: solve not resolved / last exchange not merged");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(h->h_stats, h->dstats, sizeof(DevStats), hipMemcpyDeviceToHost, h->stream));
    // local row counters of this shard: fold k_resolve's per-workgroup partial rows on the host
    std::vector<u64> part((size_t)resolve_blocks(h->m) * 8);
    HIPCHK(h, hipMemcpyAsync(part.data(), h->sb.partial, part.size() * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    DevStats v;
    memset(&v, 0, sizeof v);
    for (size_t r = 0; r < part.size() / 8; ++r) {
        const u64* x = part.data() + r * 8;
        v.load_kept += x[0]; v.load_claim_tot += x[1];
        v.kept += x[3]; v.evicted += x[4]; v.claimants += x[5]; v.spillcand += x[6];
    }
    if (h->sh.slow) {
        const DevStats& d = h->h_stats[0];
        v.rejected = d.rejected; v.load_rejected = d.load_rejected;
        v.spilled = d.spilled; v.load_spilled = d.load_spilled;
        v.unplaced = d.unplaced; v.load_unplaced = d.load_unplaced;
    }
    fill_stats(v, h->n, local_stats);  // cut_nodes / slow_path / rounds_run are global: the caller has them
    h->pending = PendingSolve{true};
    h->solves.rewind();
    h->sh.step = ShStep::idle;
    return RIO_GP_OK;
}

// ---- row-sharded rebalance -------------------------------------------------------------------
// The phases of rebalance_locked (the helpers above it: rb_cfg, rb_surplus, rb_pack, rb_finish over the one RbBufs carving) over
// one rank's rows, cut at the points where the single-handle call waits for the device: what the host decided there from `used`
// and `pin` is decided here from the gathered records, on the device (k_shrb_import_x / k_shrb_merge), in rank order.
//   _begin          rb_cfg, R0 into lu; the X record leaves (rebalance_locked: its first wait; the host picks the slots)
//   _cut            k_shrb_import_* pick the slots; waits for info.  Row order: rb_surplus, the S record leaves
//   _threshold_*    by load only: a histogram leaves per pass; the last pick runs rb_surplus, S leaves (launch_shed_select)
//   _select         waits for the gathered S: K (rebalance_locked: its second wait, for acc); rb_pack against lu, Y leaves
//   _merge / _fill  the global `used` from the gathered Y; _merge waits for the pending counts; a round per _fill
//   _finish         rb_finish against lu, the global `used` read back: the last wait of either form; read_listing

// rio_gp_shard_rebalance_begin (row order only: its protocol has no threshold passes) and rio_gp_shard_rebalance_begin_ordered
static int shard_rebalance_begin(rio_gp* h, const char* who, bool ordered, const rio_gp_rebalance_cfg* cfg, uint32_t rank,
                                 uint32_t n_ranks, int list_moves, uint64_t moves_cap, uint64_t* d_x, uint32_t* rounds_out) {
    RbCfg c;
    int rc = rb_cfg(h, who, ordered ? RbForm::shard_ordered : RbForm::shard, cfg,
                    !d_x || n_ranks == 0 || rank >= n_ranks ? "rank >= n_ranks, or no record" : nullptr, list_moves != 0, moves_cap, &c);
    if (rc || (rc = may_start(h, Client::shard_rebalance_begin))) return rc;
    // rule 13: a rank's table has no class column, and moving a protected row is the one wrong answer
    if (h->cls_any_imm)
        return fail(h, RIO_GP_EINVAL, std::string(who) + ": the handle names an immovable class (rio_gp_set_class_movable) and the "
                                                         "row-sharded rebalance has no class column: reset the table first");
    const u32 order = c.order;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = rb_ensure(h))) return rc;
    const RbBufs b = rb_bufs(h);
    const u32 m = h->m;
    // a change of the inputs, like rio_gp_rebalance: an uncommitted solve (a sharded one half way included) is dropped
    inputs_changed(h);
    h->sh.step = ShStep::idle;
    h->solves.rewind();
    h->used.borrow();  // until rio_gp_shard_rebalance_finish: its storage holds the protocol's intermediate vectors
    RbSession fresh;
    fresh.T = std::move(h->rb.T);  // (in the last session's host arrays: a copy it enqueued may still be on its way into them)
    fresh.live = std::move(h->rb.live);
    fresh.rank = rank; fresh.R = n_ranks;
    fresh.order = order;
    fresh.rounds = c.rounds;
    fresh.list = list_moves != 0;
    fresh.budget = c.budget;
    fresh.T.assign(m ? m : 1, 0);
    fresh.live.assign(m ? m : 1, 0);
    for (u32 j = 0; j < m; ++j) fresh.live[j] = h->h_alive[j] ? 1u : 0u;
    RbSession& rb = h->rb = std::move(fresh);
    if (cfg->target) {
        memcpy(rb.T.data(), cfg->target, (size_t)m * sizeof(u64));
        if (m) HIPCHK(h, hipMemcpyAsync(b.tdev, rb.T.data(), (size_t)m * sizeof(u64), hipMemcpyHostToDevice, h->stream));
    } else if (m) {  // (read by the host in _finish, behind the waits of the steps between)
        HIPCHK(h, hipMemcpyAsync(rb.T.data(), h->cap, (size_t)m * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(b.tdev, h->cap, (size_t)m * sizeof(u64), hipMemcpyDeviceToDevice, h->stream));
    }
    if (m) HIPCHK(h, hipMemcpyAsync(b.live, rb.live.data(), (size_t)m * sizeof(u32), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(b.acc, 0, kShAcc * sizeof(u64), h->stream));
    // R0 over this rank's rows: the load per node (kept in lu: it becomes used'_r in _select) and the pinned load
    u32* const maxl = order ? b.maxl : nullptr;  // (by load: X also carries this rank's largest load, where the search starts)
    launch_shed_hist(h->assign[h->cur], h->load, h->aff, h->n, m, b.lu, b.pin, h->stream, maxl);
    launch_shrb_export_x(b.lu, b.pin, m, maxl, reinterpret_cast<u64*>(d_x), h->stream);
    HIPCHK(h, hipGetLastError());
    if (rounds_out) *rounds_out = rb.rounds;
    rb.epoch = h->mut_epoch;
    rb.step = RbStep::begun;
    return RIO_GP_OK;
}

int rio_gp_shard_rebalance_begin(rio_gp_t* h, const rio_gp_rebalance_cfg* cfg, uint32_t rank, uint32_t n_ranks, int list_moves,
                                 uint64_t moves_cap, uint64_t* d_x, uint32_t* rounds_out) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    return shard_rebalance_begin(h, "rio_gp_shard_rebalance_begin", false, cfg, rank, n_ranks, list_moves, moves_cap, d_x, rounds_out);
}

int rio_gp_shard_rebalance_begin_ordered(rio_gp_t* h, const rio_gp_rebalance_cfg* cfg, uint32_t rank, uint32_t n_ranks,
                                         int list_moves, uint64_t moves_cap, uint64_t* d_x, uint32_t* rounds_out) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    return shard_rebalance_begin(h, "rio_gp_shard_rebalance_begin_ordered", true, cfg, rank, n_ranks, list_moves, moves_cap, d_x,
                                 rounds_out);
}

// R1 over this rank's rows behind the slots' free loads (and, by load, thresholds): the cut rows that fall here, the surplus per
// tile; S = surplus rows | load | zeros
static int shard_rebalance_surplus(rio_gp* h, const RbSession& rb, const RbBufs& b, bool forced, uint64_t* d_s) {
    const ShPlan& p = rb.plan;
    const u32* const thr = rb.order ? b.thr : nullptr;
    HIPCHK(h, hipMemsetAsync(d_s, 0, ((size_t)h->m + 2) * sizeof(u64), h->stream));
    if (!h->n || !(p.s || forced)) return RIO_GP_OK;
    if (int rc = rb_surplus(h, p, b, thr, false)) return rc;
    HIPCHK(h, hipMemcpyAsync(d_s, b.acc, 2 * sizeof(u64), hipMemcpyDeviceToDevice, h->stream));  // surplus rows | load
    return RIO_GP_OK;
}

int rio_gp_shard_rebalance_cut(rio_gp_t* h, const uint64_t* d_xg, uint64_t* d_s, uint32_t* nodes_over) {
    if (!h || !d_xg || !d_s) return RIO_GP_EINVAL;
    Locked g(h);
    RbSession& rb = h->rb;
    if (!rb.at(h, RbStep::begun)) return fail(h, RIO_GP_EINVAL, "rio_gp_shard_rebalance_cut: call rio_gp_shard_rebalance_begin first");
    HIPCHK(h, hipSetDevice(h->device));
    const RbBufs b = rb_bufs(h);
    const u32 m = h->m;
    ShrbImport a{};
    a.Xg = reinterpret_cast<const u64*>(d_xg);
    a.rank = rb.rank; a.R = rb.R; a.m = m;
    a.T = b.tdev; a.live = b.live;
    a.used = h->used.storage(); a.tgt = b.tgt; a.map = b.map; a.slot_node = b.slot_node; a.slot_free = b.slot_free; a.cut = b.cut;
    a.info = b.info;
    if (rb.order) launch_shrb_import_slots(a, b.pre, b.thr, h->stream);
    else launch_shrb_import_x(a, h->stream);
    HIPCHK(h, hipGetLastError());
    u32 info[kShrbInfo + 1] = {};
    HIPCHK(h, hipMemcpyAsync(info, b.info, (kShrbInfo + (rb.order ? 1 : 0)) * sizeof(u32), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    rb.over = info[kShrbOver];
    rb.over_before = info[kShrbOverBefore];
    const u32 S = info[kShrbSlots];
    rb.plan = sh_plan(h->n, m, S);
    if (rb.order) {  // the surplus is known behind the thresholds: rio_gp_shard_rebalance_threshold_pick's last pass writes S
        rb.slots = S;
        rb.sel = shrb_sel_plan(S, m);
        rb.sel_first = shrb_sel_first_pass(rb.sel, info[kShrbMaxLoad]);
        rb.sel_pass = rb.sel_first;
        rb.sel_hist_out = false;
        int rc;  // (what the last pick's rb_surplus needs, here: a pick that has run is not taken back)
        if (S && h->n && (rc = rb_plan_ensure(h, rb.plan))) return rc;
        HIPCHK(h, hipMemsetAsync(d_s, 0, ((size_t)m + 2) * sizeof(u64), h->stream));
    } else if (int rc = shard_rebalance_surplus(h, rb, b, info[kShrbForced] != 0, d_s)) {
        return rc;
    }
    if (nodes_over) *nodes_over = rb.over;
    rb.step = RbStep::cut;
    return RIO_GP_OK;
}

int rio_gp_shard_rebalance_threshold_plan(rio_gp_t* h, uint32_t* passes, uint64_t* words) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    RbSession& rb = h->rb;
    if (!rb.at(h, RbStep::cut) || !rb.order || !rb.over)
        return fail(h, RIO_GP_EINVAL, "rio_gp_shard_rebalance_threshold_plan: a load-ordered session behind rio_gp_shard_rebalance_cut "
                                      "with nodes over only (rio_gp_shard_rebalance_begin_ordered)");
    if (passes) *passes = rb.sel.passes - rb.sel_first;
    if (words) *words = (u64)rb.slots << rb.sel.bits;
    return RIO_GP_OK;
}

int rio_gp_shard_rebalance_threshold_hist(rio_gp_t* h, uint32_t pass, uint64_t* d_h) {
    if (!h || !d_h) return RIO_GP_EINVAL;
    Locked g(h);
    RbSession& rb = h->rb;
    if (!rb.at(h, RbStep::cut) || !rb.thresholds_pending() || pass != rb.sel_pass - rb.sel_first)
        return fail(h, RIO_GP_EINVAL, "rio_gp_shard_rebalance_threshold_hist: the passes of a load-ordered session run in order, "
                                      "between rio_gp_shard_rebalance_cut (with nodes over) and rio_gp_shard_rebalance_select");
    HIPCHK(h, hipSetDevice(h->device));
    const RbBufs b = rb_bufs(h);
    launch_shrb_sel_hist(h->assign[h->cur], h->load, h->aff, h->n, h->m, rb.slots, b.map, b.pre, rb.sel, rb.sel_pass,
                         reinterpret_cast<u64*>(d_h), h->stream);
    HIPCHK(h, hipGetLastError());
    rb.sel_hist_out = true;
    return RIO_GP_OK;
}

int rio_gp_shard_rebalance_threshold_pick(rio_gp_t* h, uint32_t pass, const uint64_t* d_hg, uint64_t* d_s) {
    if (!h || !d_hg) return RIO_GP_EINVAL;
    Locked g(h);
    RbSession& rb = h->rb;
    if (!rb.at(h, RbStep::cut) || !rb.thresholds_pending() || pass != rb.sel_pass - rb.sel_first || !rb.sel_hist_out)
        return fail(h, RIO_GP_EINVAL, "rio_gp_shard_rebalance_threshold_pick: call rio_gp_shard_rebalance_threshold_hist of the same "
                                      "pass first; the passes run in order");
    const bool last = rb.sel_pass + 1 == rb.sel.passes;
    if (last && !d_s) return fail(h, RIO_GP_EINVAL, "rio_gp_shard_rebalance_threshold_pick: the last pass writes the S record");
    HIPCHK(h, hipSetDevice(h->device));
    const RbBufs b = rb_bufs(h);
    launch_shrb_sel_pick(reinterpret_cast<const u64*>(d_hg), rb.rank, rb.R, rb.slots, rb.sel, rb.sel_pass, b.slot_node, b.slot_free, b.pre,
                         b.thr, h->stream);
    HIPCHK(h, hipGetLastError());
    if (last)
        if (int rc = shard_rebalance_surplus(h, rb, b, false, d_s)) return rc;
    rb.sel_hist_out = false;
    ++rb.sel_pass;
    return RIO_GP_OK;
}

int rio_gp_shard_rebalance_select(rio_gp_t* h, const uint64_t* d_sg, uint64_t* d_y, uint64_t* selected_local,
                                  uint64_t* selected_total) {
    if (!h || !d_sg || !d_y) return RIO_GP_EINVAL;
    Locked g(h);
    RbSession& rb = h->rb;
    if (!rb.at(h, RbStep::cut) || !rb.over)
        return fail(h, RIO_GP_EINVAL, "rio_gp_shard_rebalance_select: call rio_gp_shard_rebalance_cut first (and only when it reports nodes over)");
    if (rb.thresholds_pending())
        return fail(h, RIO_GP_EINVAL, "rio_gp_shard_rebalance_select: the threshold passes of the load-ordered cut come first "
                                      "(rio_gp_shard_rebalance_threshold_plan / _hist / _pick)");
    HIPCHK(h, hipSetDevice(h->device));
    const RbBufs b = rb_bufs(h);
    const u32 m = h->m, R = rb.R;
    const size_t W = (size_t)m + 2;
    std::vector<u64> sg(2 * (size_t)R);
    HIPCHK(h, hipMemcpy2DAsync(sg.data(), 2 * sizeof(u64), d_sg, W * sizeof(u64), 2 * sizeof(u64), R, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    u64 pre = 0, tot = 0;
    for (u32 q = 0; q < R; ++q) {
        if (q < rb.rank) pre += sg[2 * q];
        tot += sg[2 * q];
    }
    const u64 mine = sg[2 * (size_t)rb.rank], B = rb.budget;
    const u64 K = B > pre ? std::min<u64>(B - pre, mine) : 0;  // R2: this rank's share of the first B surplus rows
    rb.K = K;
    rb.sel_total = std::min<u64>(B, tot);
    if (K)
        if (int rc = rb_pack(h, rb.plan, b, rb.order ? b.thr : nullptr, K, b.lu)) return rc;
    launch_shrb_export_y(b.lu, m, b.acc + kShAccSelectedLoad, K, reinterpret_cast<u64*>(d_y), h->stream);
    HIPCHK(h, hipGetLastError());
    if (selected_local) *selected_local = K;
    if (selected_total) *selected_total = rb.sel_total;
    rb.first = true;
    rb.step = RbStep::selected;
    return RIO_GP_OK;
}

int rio_gp_shard_rebalance_merge(rio_gp_t* h, const uint64_t* d_yg, uint64_t* pending_rows, uint64_t* pending_load) {
    if (!h || !d_yg) return RIO_GP_EINVAL;
    Locked g(h);
    RbSession& rb = h->rb;
    if ((!rb.at(h, RbStep::selected) || !rb.sel_total) && !rb.at(h, RbStep::round_exported))
        return fail(h, RIO_GP_EINVAL, "rio_gp_shard_rebalance_merge: nothing exported (rio_gp_shard_rebalance_select with rows selected, or _fill, first)");
    HIPCHK(h, hipSetDevice(h->device));
    const RbBufs b = rb_bufs(h);
    launch_shrb_merge(reinterpret_cast<const u64*>(d_yg), rb.rank, rb.R, h->m, rb.first, h->used.storage(), b.base, b.acc + kRbPend,
                      h->stream);
    HIPCHK(h, hipGetLastError());
    u64 pend[2];
    HIPCHK(h, hipMemcpyAsync(pend, b.acc + kRbPend, sizeof pend, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    rb.first = false;
    rb.pending = pend[0];
    if (pending_rows) *pending_rows = pend[0];
    if (pending_load) *pending_load = pend[1];
    rb.step = RbStep::merged;
    return RIO_GP_OK;
}

int rio_gp_shard_rebalance_fill(rio_gp_t* h, uint32_t round, uint64_t* d_y) {
    if (!h || !d_y) return RIO_GP_EINVAL;
    Locked g(h);
    RbSession& rb = h->rb;
    if (!rb.at(h, RbStep::merged) || round != rb.fills || round >= rb.rounds || !rb.pending)
        return fail(h, RIO_GP_EINVAL, "rio_gp_shard_rebalance_fill: call rio_gp_shard_rebalance_merge first; rounds run in order while rows are pending");
    HIPCHK(h, hipSetDevice(h->device));
    const RbBufs b = rb_bufs(h);
    const u64 K = rb.K;
    const RbPacked pk = rb_packed(h, K);
    launch_shrb_round(K, pk.row, pk.load, pk.node, h->assign[h->cur], b.tgt, h->m, h->used.storage(), b.base,
                      round + 1 == rb.rounds, (u64*)h->sh_chunk.p, b.C, b.ord, b.cntp, reinterpret_cast<u64*>(d_y), h->stream);
    HIPCHK(h, hipGetLastError());
    ++rb.fills;
    rb.step = RbStep::round_exported;
    return RIO_GP_OK;
}

int rio_gp_shard_rebalance_finish(rio_gp_t* h, rio_gp_rebalance_stats* local_stats, uint32_t* out_rows, uint32_t* out_from,
                                  uint32_t* out_to, uint64_t moves_cap, uint64_t* n_moves) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    RbSession& rb = h->rb;
    (void)rb.at(h, RbStep::idle);  // (a session whose inputs moved is over)
    if (!rb.finished()) return fail(h, RIO_GP_EINVAL, "rio_gp_shard_rebalance_finish: the protocol has not reached its end");
    if ((out_rows != nullptr) != (out_from != nullptr) || (out_rows != nullptr) != (out_to != nullptr))
        return fail(h, RIO_GP_EINVAL, "rio_gp_shard_rebalance_finish: out_rows / out_from / out_to are given together or not at all");
    if ((out_rows != nullptr) != rb.list)
        return fail(h, RIO_GP_EINVAL, "rio_gp_shard_rebalance_finish: the move listing is asked for in rio_gp_shard_rebalance_begin");
    const u64 K = rb.listed_rows();
    if (out_rows ? moves_cap < K : moves_cap != 0)
        return fail(h, RIO_GP_EINVAL, "rio_gp_shard_rebalance_finish: moves_cap below this rank's selected rows (rio_gp_shard_rebalance_select)");
    HIPCHK(h, hipSetDevice(h->device));
    const RbBufs b = rb_bufs(h);
    rio_gp_rebalance_stats s{};
    int rc;
    u32* d = nullptr;
    if (K && out_rows) {
        if ((rc = ensure(h, h->sh_mv, 3 * K * sizeof(u32)))) return rc;
        d = (u32*)h->sh_mv.p;
    }
    s.selected_rows = rb.selected_rows();
    s.nodes_over_before = rb.over_before;
    // (the rows left without a node gave their load back in the last round's record: k_shed_mcount's returns go to lu, scratch now)
    if ((rc = rb_finish(h, b, K, b.lu, rb.T.data(), d, d ? d + K : nullptr, d ? d + 2 * K : nullptr, &s))) return rc;
    if (out_rows && s.moved_rows && (rc = read_listing(h, d, K, s.moved_rows, {out_rows, out_from, out_to}))) return rc;
    if (n_moves) *n_moves = s.moved_rows;
    if (local_stats) *local_stats = s;
    h->used.rebuilt();  // the global `used` of the new column, on every rank
    rb.step = RbStep::idle;
    return RIO_GP_OK;
}

// ---- peer-to-peer exchange over xGMI (preferred): no collective call on the data path at all ----

int rio_gp_shard_p2p_export(rio_gp_t* h, uint32_t n_ranks, void* out_handle64) {
    if (!h || !out_handle64 || n_ranks == 0 || n_ranks > 32) return RIO_GP_EINVAL;
    Locked g(h);
    if (h->p2p) return fail(h, RIO_GP_EINVAL, "rio_gp_shard_p2p_export: window already exported");
    HIPCHK(h, hipSetDevice(h->device));
    P2P* q = new P2P();
    q->R = n_ranks;
    q->W = (shard_words1(h->cap_nodes) + 7) & ~(size_t)7;
    q->Wx = (shard_xchg_words(h->cap_nodes) + 7) & ~(size_t)7;
    const size_t bytes = q->total_words() * sizeof(u64);
    void* w = nullptr;
    // uncached first (what RCCL uses for its own flag/LL buffers on gfx94x/95x), fine-grained second; ordinary cached
    // device memory is NOT acceptable: a peer's store would sit behind this GPU's stale L2 lines
    if (hipExtMallocWithFlags(&w, bytes, hipDeviceMallocUncached) != hipSuccess) {
        (void)hipGetLastError();
        w = nullptr;
        if (hipExtMallocWithFlags(&w, bytes, hipDeviceMallocFinegrained) != hipSuccess) {
            (void)hipGetLastError();
            delete q;
            return fail(h, RIO_GP_EUPSTREAM, "rio_gp_shard_p2p_export: no uncached / fine-grained device memory");
        }
    }
    q->win = static_cast<u64*>(w);
    h->p2p = q;
    HIPCHK(h, hipMemsetAsync(q->win, 0, bytes, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    hipIpcMemHandle_t ih;
    HIPCHK(h, hipIpcGetMemHandle(&ih, q->win));
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle size");
    memcpy(out_handle64, &ih, 64);
    return RIO_GP_OK;
}

int rio_gp_shard_p2p_connect(rio_gp_t* h, uint32_t rank, uint32_t n_ranks, const void* handles) {
    if (!h || !handles || n_ranks == 0 || rank >= n_ranks) return RIO_GP_EINVAL;
    Locked g(h);
    P2P* q = h->p2p;
    if (!q || q->R != n_ranks || q->d_peers) return fail(h, RIO_GP_EINVAL, "rio_gp_shard_p2p_connect: export first / rank count differs");
    HIPCHK(h, hipSetDevice(h->device));
    q->rank = rank;
    q->opened.assign(n_ranks, nullptr);
    std::vector<u64*> bases(n_ranks, nullptr);
    for (uint32_t r = 0; r < n_ranks; ++r) {
        if (r == rank) { bases[r] = q->win; continue; }
        hipIpcMemHandle_t ih;
        memcpy(&ih, static_cast<const char*>(handles) + (size_t)r * 64, 64);
        void* o = nullptr;
        hipError_t e = hipIpcOpenMemHandle(&o, ih, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, RIO_GP_EUPSTREAM, std::string("hipIpcOpenMemHandle: ") + hipGetErrorString(e));
        }
        q->opened[r] = o;
        bases[r] = static_cast<u64*>(o);
    }
    HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&q->d_peers), n_ranks * sizeof(u64*)));
    HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&q->d_err), sizeof(u64)));
    HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&q->scratch), q->W * sizeof(u64)));
    HIPCHK(h, hipMemcpy(q->d_peers, bases.data(), n_ranks * sizeof(u64*), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemset(q->d_err, 0, sizeof(u64)));
    // handshake: every rank stores a token into every peer's hello line and waits for all of theirs (3 s limit).  Next to
    // the token travels the identity of the device the rank runs on (hash of its PCI bus id): ranks that share a GPU — a test
    // box, or a deployment that packs several shards on one device — must keep their spinning exchange kernels small enough
    // to be co-resident (launch_resolve_xchg).
    const u64 token = 0xC0FFEE0000000001ull;
    u64 devid = 1469598103934665603ull;
    {
        char bus[64] = {0};
        if (hipDeviceGetPCIBusId(bus, (int)sizeof bus - 1, h->device) != hipSuccess) {
            (void)hipGetLastError();
            snprintf(bus, sizeof bus, "device-%d", h->device);
        }
        for (const char* c = bus; *c; ++c) devid = (devid ^ (u64)(unsigned char)*c) * 1099511628211ull;
        devid |= 1ull;
    }
    HIPCHK(h, hipMemcpyAsync(q->scratch, &devid, sizeof devid, hipMemcpyHostToDevice, h->stream));
    launch_p2p_put(q->scratch, 1, q->d_peers, n_ranks, q->hello_off(rank) + 1, q->hello_off(rank), token, h->stream);
    launch_p2p_wait_copy(q->win, q->W, n_ranks, 0, q->win + q->hello_off(0), token, q->d_err, nullptr, h->stream);
    u64 err = 0;
    std::vector<u64> hello((size_t)n_ranks * 8, 0);
    HIPCHK(h, hipMemcpyAsync(&err, q->d_err, sizeof err, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(hello.data(), q->win + q->hello_off(0), hello.size() * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (err) return fail(h, RIO_GP_EUPSTREAM, "rio_gp_shard_p2p_connect: a peer's handshake store never became visible");
    q->co_resident = 0;
    for (uint32_t r = 0; r < n_ranks; ++r) q->co_resident += hello[(size_t)r * 8 + 1] == devid;
    if (q->co_resident == 0) q->co_resident = 1;
    return RIO_GP_OK;
}

int rio_gp_shard_p2p_ready(rio_gp_t* h) { return h && h->p2p && h->p2p->d_peers ? 1 : 0; }

int rio_gp_shard_p2p_close(rio_gp_t* h) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    (void)hipGetLastError();
    p2p_free(h);
    h->sh.step = ShStep::idle;
    h->solves.rewind();
    return RIO_GP_OK;
}

static int p2p_check(rio_gp* h) {  // after a wait on the stream: did any in-kernel wait time out?
    u64 err = 0;
    HIPCHK(h, hipMemcpyAsync(&err, h->p2p->d_err, sizeof err, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (err) {
        // a peer never delivered (it is gone, or minutes behind): whatever was enqueued behind the wait ran on records that are
        // not there, and this rank's sequence numbers are ahead of anything the peers will see — the session is over
        h->p2p->out_of_step = true;
        return fail(h, RIO_GP_EUPSTREAM, "peer-to-peer exchange timed out waiting for a rank's record (the session is out of step: "
                                         "rio_gp_shard_p2p_close, then fresh windows or another exchange path)");
    }
    return RIO_GP_OK;
}

// ---- native RCCL exchange (optional): the library issues the all-gathers itself --------------

static bool rccl_load(RcclApi* a, const char* path, std::string* err) {
    const char* cands[] = {path, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (int pass = 0; pass < 2 && !a->lib; ++pass)      // pass 0: a copy already in the process (torch's), pass 1: load
        for (const char* c : cands)
            if (c && *c && (a->lib = dlopen(c, RTLD_NOW | RTLD_GLOBAL | (pass == 0 ? RTLD_NOLOAD : 0)))) break;
    if (!a->lib) { *err = std::string("dlopen(librccl) failed: ") + (dlerror() ? dlerror() : "?"); return false; }
    a->GetUniqueId = reinterpret_cast<int (*)(void*)>(dlsym(a->lib, "ncclGetUniqueId"));
    a->CommInitRank = reinterpret_cast<int (*)(void**, int, RioGpNcclId, int)>(dlsym(a->lib, "ncclCommInitRank"));
    a->CommDestroy = reinterpret_cast<int (*)(void*)>(dlsym(a->lib, "ncclCommDestroy"));
    a->AllGather = reinterpret_cast<int (*)(const void*, void*, size_t, int, void*, hipStream_t)>(dlsym(a->lib, "ncclAllGather"));
    a->GetErrorString = reinterpret_cast<const char* (*)(int)>(dlsym(a->lib, "ncclGetErrorString"));
    if (!a->GetUniqueId || !a->CommInitRank || !a->CommDestroy || !a->AllGather) { *err = "librccl lacks a required symbol"; return false; }
    return true;
}

int rio_gp_shard_comm_unique_id(void* out128, const char* rccl_path) {
    if (!out128) return RIO_GP_EINVAL;
    RcclApi a;
    std::string err;
    if (!rccl_load(&a, rccl_path, &err)) { g_create_error = err; return RIO_GP_EUPSTREAM; }
    RioGpNcclId id;
    memset(&id, 0, sizeof id);
    const int rc = a.GetUniqueId(&id);
    if (rc != 0) { g_create_error = "ncclGetUniqueId failed"; return RIO_GP_EUPSTREAM; }
    memcpy(out128, &id, sizeof id);
    return RIO_GP_OK;
}

int rio_gp_shard_comm_init(rio_gp_t* h, uint32_t rank, uint32_t n_ranks, const void* id128, const char* rccl_path) {
    if (!h || !id128 || n_ranks == 0 || rank >= n_ranks) return RIO_GP_EINVAL;
    Locked g(h);
    if (h->sc) return fail(h, RIO_GP_EINVAL, "rio_gp_shard_comm_init: communicator already set up");
    HIPCHK(h, hipSetDevice(h->device));
    ShardComm* sc = new ShardComm();
    std::string err;
    if (!rccl_load(&sc->api, rccl_path, &err)) { delete sc; return fail(h, RIO_GP_EUPSTREAM, err); }
    RioGpNcclId id;
    memcpy(&id, id128, sizeof id);
    const int rc = sc->api.CommInitRank(&sc->comm, (int)n_ranks, id, (int)rank);
    if (rc != 0) {
        const std::string m = std::string("ncclCommInitRank: ") + (sc->api.GetErrorString ? sc->api.GetErrorString(rc) : "failed");
        delete sc;
        return fail(h, RIO_GP_EUPSTREAM, m);
    }
    sc->rank = rank;
    sc->R = n_ranks;
    h->sc = sc;  // from here on rio_gp_destroy releases whatever was created
    HIPCHK(h, hipStreamCreateWithFlags(&sc->side, hipStreamNonBlocking));
    const size_t w1 = shard_words1(h->cap_nodes);
    for (int q = 0; q < kShardRing; ++q) {
        HIPCHK(h, hipEventCreateWithFlags(&sc->ready[q], hipEventDisableTiming));
        HIPCHK(h, hipEventCreateWithFlags(&sc->done[q], hipEventDisableTiming));
        HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&sc->X[q]), w1 * sizeof(u64)));
        HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&sc->XG[q]), w1 * n_ranks * sizeof(u64)));
    }
    return RIO_GP_OK;
}

uint32_t rio_gp_shard_comm_ranks(rio_gp_t* h) { return h && h->sc ? h->sc->R : 0; }

// One whole fast-path step of the row-sharded solve, nothing waits on the host:
//   stream:      k_scan, k_resolve (local sums), pack X      -> event
//   side stream: ncclAllGather(X) over xGMI, k_shard_import  -> event (frees the ring slot)
// Back-to-back calls overlap solve k's exchange with solve k+1's scan.
int rio_gp_shard_solve_async(rio_gp_t* h) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    if (h->sa) return fail(h, RIO_GP_EINVAL, "row-sharded solves do not implement RIO_GP_CFG_REF_SELF_ASSIGN (single-GPU handles only)");
    if (int rc = may_start(h, Client::shard_solve_async)) return rc;
    if (h->p2p && h->p2p->d_peers) {
        // peer-to-peer, ONE stream, two launches, no collective call and no host wait: k_scan -> k_resolve_xchg.
        // Stream order is the flow control: a rank's record j+1 leaves only after it consumed everyone's record j,
        // so none of the 4 window slots (P2P::xslot_n) is overwritten while its owner still reads it.  (Running the exchange on a
        // second stream under the next scan was measured SLOWER on gfx950: two event records + two stream waits per
        // solve cost more than the 5 us they hide.)
        P2P* q = h->p2p;
        if (q->out_of_step) return fail(h, RIO_GP_EUPSTREAM, kOutOfStep);
        StepGuard step{q};
        const u64 seq = ++q->seq;
        const u32 slot = (u32)(q->xslot_n++ % kP2PSlots);
        const NodeTab nt = shard_scan_begin(h).nt;
        h->sh.bind(q->rank, q->R, nullptr);
        // ONE launch behind the scan: every workgroup exchanges and resolves its own node group (k_resolve_xchg);
        // the verdict arrives as resolve_blocks(m) partial rows in the pinned slot
        SolveBufs xb = shard_bufs(h);
        xb.H = h->sb.H;
        xb.blkstat = h->sb.blkstat;
        launch_resolve_xchg(h->plan, nt, xb, q->d_peers, q->R, q->rank, q->xdata_off(slot, q->rank),
                            q->win + q->xdata_off(slot, 0), q->Wx, seq, q->d_err, h->sh_gprev, h->sh_gfinal,
                            slot_dev(h, h->solves.next_slot()), q->co_resident, h->stream);
        h->solves.pushed_shard(resolve_blocks(h->m));
        inputs_changed(h);
        h->sh.step = ShStep::resolved;
        HIPCHK(h, hipGetLastError());
        step.done = true;
        return RIO_GP_OK;
    }
    ShardComm* sc = h->sc;
    if (!sc) return fail(h, RIO_GP_EINVAL, "rio_gp_shard_solve_async: set up rio_gp_shard_p2p_connect or rio_gp_shard_comm_init first");
    const int q = (int)(sc->k++ % kShardRing);
    if (sc->done_valid[q]) HIPCHK(h, hipStreamWaitEvent(h->stream, sc->done[q], 0));
    const NodeTab nt = shard_scan_begin(h).nt;
    const SolveBufs lb = local_bufs(h);
    launch_resolve(h->plan, nt, lb, nullptr, h->stream);
    launch_shard_pack1(h->plan, lb, sc->X[q], h->stream);
    HIPCHK(h, hipEventRecord(sc->ready[q], h->stream));
    HIPCHK(h, hipStreamWaitEvent(sc->side, sc->ready[q], 0));
    const int rc = sc->api.AllGather(sc->X[q], sc->XG[q], shard_words1(h->m), kNcclUint64, sc->comm, sc->side);
    if (rc != 0) return fail(h, RIO_GP_EUPSTREAM, std::string("ncclAllGather: ") + (sc->api.GetErrorString ? sc->api.GetErrorString(rc) : "failed"));
    h->sh.bind(sc->rank, sc->R, sc->side);
    launch_shard_import(h->plan, nt, shard_bufs(h), sc->XG[q], sc->rank, sc->R, h->sh_gprev, h->sh_gfinal, h->sh_verdict,
                        slot_dev(h, h->solves.next_slot()), sc->side);
    HIPCHK(h, hipEventRecord(sc->done[q], sc->side));
    sc->done_valid[q] = true;
    h->solves.pushed_shard(1);
    inputs_changed(h);
    h->sh.step = ShStep::resolved;
    return RIO_GP_OK;
}

// ---- asynchronous committed tick of the row-sharded table (peer-to-peer windows) ----
// Record of tick k in pinned memory: k_resolve_xchg's partial verdict rows in the tick ring's slot k (d_slots), and in slot
// 1 + k of the fix-up counter rows (h_fx; the row-sharded solve does not use them otherwise): rows 0-1 = this rank's counters
// (k_shard_tick_stats, 16 words), row 2 + e = {rows, load} pending on all ranks after exchange e (k_shard_import_delta).
static void shard_exchange_y(rio_gp* h, const SolveBufs& b, const u64* base, int wsp_sel, u64* verdict_host) {
    P2P* q = h->p2p;
    const u64 seq = ++q->seq;
    const u32 slot = (u32)(q->yslot_n++ % kP2PSlots);
    launch_shard_export_put(h->plan, b, base, wsp_sel, q->d_peers, q->R, q->data_off(slot, q->rank), q->flag_off(slot, q->rank), seq,
                            h->stream);
    launch_shard_wait_import(h->plan, b, q->win + q->data_off(slot, 0), q->W, q->win + q->flag_off(slot, 0), seq, q->d_err,
                             h->sh.rank, h->sh.R, h->sh_gprev, h->sh_gfinal, h->sh_verdict, verdict_host, h->stream);
}

int rio_gp_shard_tick_async(rio_gp_t* h) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    if (h->sa) return fail(h, RIO_GP_EINVAL, "row-sharded solves do not implement RIO_GP_CFG_REF_SELF_ASSIGN (single-GPU handles only)");
    P2P* q = h->p2p;
    if (!q || !q->d_peers) return fail(h, RIO_GP_EINVAL, "rio_gp_shard_tick_async: peer-to-peer windows only (rio_gp_shard_p2p_connect first)");
    int rc = may_start(h, Client::shard_tick_async);
    if (rc) return rc;
    if (q->out_of_step) return fail(h, RIO_GP_EUPSTREAM, kOutOfStep);
    HIPCHK(h, hipSetDevice(h->device));
    const u32 k = h->ticks.next_slot();
    // (1) the fast path: k_scan -> k_resolve_xchg, verdict rows into this tick's slot of the tick ring
    StepGuard step{q};  // (every sequence number this tick takes — its own and its exchanges' — is taken before any check below)
    const u64 seq = ++q->seq;
    const u32 slot = (u32)(q->xslot_n++ % kP2PSlots);
    const ShardScan sc0 = shard_scan_begin(h);
    const Table& t = sc0.t;
    const NodeTab& nt = sc0.nt;
    h->sh.bind(q->rank, q->R, nullptr);
    SolveBufs b = shard_bufs(h);
    b.H = h->sb.H;
    b.blkstat = h->sb.blkstat;
    u64* rows = h->ticks.rows_dev(k);
    u64* rec = h->d_fx + (size_t)TickRing::fx_slot(k) * kMaxBlocks * 8;
    launch_resolve_xchg(h->plan, nt, b, q->d_peers, q->R, q->rank, q->xdata_off(slot, q->rank), q->win + q->xdata_off(slot, 0),
                        q->Wx, seq, q->d_err, h->sh_gprev, h->sh_gfinal, rows, q->co_resident, h->stream);
    // (2) exact cut on this rank: k_cutblk + k_cut_find guard themselves on the cut flag, the re-marking pass on the number
    //     of nodes k_resolve_xchg found to need it here
    b.run_if = &h->dstats->local_fixup;
    launch_cut_find(h->plan, t, nt, b, false, h->stream, false);
    launch_fill(h->plan, t, nt, b, false, true, false, 0, false, h->stream);
    // (3) what this rank admitted, everyone's, the global `used`, this rank's spill base
    shard_exchange_y(h, b, h->sb.used_kept, 0, rec + 16);
    // (4) one water-fill round per spill round (a no-op on the device when nothing is pending anywhere), each with its exchange
    for (u32 r = 0; r < h->rounds; ++r) {
        launch_fill(h->plan, t, nt, b, false, false, true, (int)r, r + 1 == h->rounds, h->stream);
        shard_exchange_y(h, b, h->sh_gprev, (int)((r & 1) ^ 1), rec + 8 * (size_t)(3 + r));
    }
    // (5) this rank's counters, (6) publication
    h->ticks.shard_mark[k] = (1ull << 41) | ++h->wait_seq;
    launch_shard_tick_stats(h->plan, b, rec, h->ticks.shard_mark[k], h->stream);
    HIPCHK(h, hipGetLastError());
    h->pending = PendingSolve{true};
    if ((rc = commit_enqueue(h))) return rc;
    h->ticks.pushed(TickRing::Owner::shard_ticks);
    h->sh.step = ShStep::idle;
    step.done = true;
    return RIO_GP_OK;
}

int rio_gp_shard_tick_wait(rio_gp_t* h, rio_gp_shard_tick_info* out, uint32_t cap, uint32_t* n_out) {
    if (!h || !n_out || (cap && !out)) return RIO_GP_EINVAL;
    Locked g(h);
    *n_out = 0;
    const u32 n = h->ticks.count(TickRing::Owner::shard_ticks);
    if (!n) return RIO_GP_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    h->ticks.clear();
    if (h->p2p && h->p2p->d_peers) { int rc = p2p_check(h); if (rc) return rc; }
    const u32 nb = resolve_blocks(h->m);
    const u32 take = n < cap ? n : cap;
    for (u32 k = n - take; k < n; ++k) {
        rio_gp_shard_tick_info& o = out[k - (n - take)];
        const u64* rows = h->ticks.rows_host(k);
        const u64* rec = h->h_fx + (size_t)TickRing::fx_slot(k) * kMaxBlocks * 8;
        if (rec[15] != h->ticks.shard_mark[k]) return fail(h, RIO_GP_EUPSTREAM, "rio_gp_shard_tick_wait: a tick left no record");
        u64 x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (u32 r = 0; r < nb; ++r)
            for (int c = 0; c < 8; ++c) x[c] += rows[(size_t)r * 8 + c];
        DevStats v;
        memset(&v, 0, sizeof v);
        v.load_kept = rec[0]; v.load_claim_tot = rec[1];
        v.kept = rec[3]; v.evicted = rec[4]; v.claimants = rec[5]; v.spillcand = rec[6];
        const bool slow = x[0] > 0 || x[1] > 0;
        if (slow) {
            v.rejected = rec[8]; v.load_rejected = rec[9];
            v.spilled = rec[10]; v.load_spilled = rec[11];
            v.unplaced = rec[12]; v.load_unplaced = rec[13];
        }
        fill_stats(v, h->n, &o.local);
        o.cut_nodes = x[0];
        o.spill_rows = x[1];
        o.slow_path = slow ? 1u : 0u;
        o.rounds_run = 0;
        for (u32 r = 0; slow && r < h->rounds; ++r) o.rounds_run += rec[8 * (size_t)(2 + r)] > 0;  // rows pending BEFORE round r
    }
    *n_out = n;
    return RIO_GP_OK;
}

// all-gather of `words` u64 per rank on the handle's stream (the Y records of the fix-up path, counters)
int rio_gp_shard_exchange(rio_gp_t* h, const uint64_t* d_in, uint64_t* d_out, uint64_t words) {
    if (!h || !d_in || !d_out) return RIO_GP_EINVAL;
    Locked g(h);
    if (h->p2p && h->p2p->d_peers) {
        P2P* q = h->p2p;
        if (words > q->W) return fail(h, RIO_GP_EINVAL, "rio_gp_shard_exchange: record larger than the window row");
        if (q->out_of_step) return fail(h, RIO_GP_EUPSTREAM, kOutOfStep);
        StepGuard step{q};  // (a failure behind the sequence number / slot taken here leaves the ranks out of step: marked)
        const u64 seq = ++q->seq;
        const u32 slot = (u32)(q->yslot_n++ % kP2PSlots);
        launch_p2p_put(reinterpret_cast<const u64*>(d_in), (u32)words, q->d_peers, q->R, q->data_off(slot, q->rank),
                       q->flag_off(slot, q->rank), seq, h->stream);
        launch_p2p_wait_copy(q->win + q->data_off(slot, 0), q->W, q->R, (u32)words, q->win + q->flag_off(slot, 0), seq,
                             q->d_err, reinterpret_cast<u64*>(d_out), h->stream);
        const int rc = p2p_check(h);
        step.done = rc == RIO_GP_OK;
        return rc;
    }
    if (!h->sc) return fail(h, RIO_GP_EINVAL, "rio_gp_shard_exchange: call rio_gp_shard_comm_init first");
    const int rc = h->sc->api.AllGather(d_in, d_out, (size_t)words, kNcclUint64, h->sc->comm, h->stream);
    if (rc != 0) return fail(h, RIO_GP_EUPSTREAM, "ncclAllGather failed");
    return RIO_GP_OK;
}

#ifdef RIO_GP_LAB
// ---- lab build only (librio_gp_lab.so, include/rio_gpu_placement_debug.h): policy knobs for the parity tests and A/B
//      runs, the streaming / host round-trip probes.  None of it is in the product library.
void rio_gp_debug_set_scan_nt(int mode) { set_scan_nt(mode); }
void rio_gp_debug_set_part_shift(int shift) { set_part_shift(shift); }
uint64_t rio_gp_debug_wave_row_lo(uint64_t n_objects, uint32_t n_nodes, uint32_t wave, uint32_t* n_waves) {
    return plan_wave_row_lo(n_objects, n_nodes, wave, n_waves);
}

int rio_gp_debug_set_compact(rio_gp_t* h, int mode) {
    if (!h || mode < 0 || mode >= 8192 || (mode & 2048) || (mode & 15) > 2 || ((mode >> 5) & 3) == 3) return RIO_GP_EINVAL;  // nothing is changed
    Locked g(h);
    h->part_mode = (mode & 16) ? 2 : 0;  // bit 4: big update / remove batches through the plain kernels (A/B runs, parity tests)
    h->cutpack_mode = (mode >> 5) & 3;   // bits 5-6: packing at the cut pass of whole-table solves, 0 auto | 1 always | 2 never
    h->compact_mode = mode & 15;
    h->inc_mode = (mode >> 7) & 3;       // bits 7-8: in-place scan of committed ticks, 0 auto | 1 whatever the table's size | 2 never
    if (h->inc_mode == 3) h->inc_mode = 0;
    h->cutapply_mode = (mode >> 9) & 3;  // bits 9-10: 0 = k_cut_apply when the solve packs at the cut pass | 1 = always | 2 = never
    if (h->cutapply_mode == 3) h->cutapply_mode = 0;
    h->chain_mode = (mode & 4096) ? 2 : 0;  // bit 12: quiet ticks are not chained (k_scan + k_resolve on the main stream)
    return RIO_GP_OK;
}

uint64_t rio_gp_debug_chained_scans(rio_gp_t* h) {
    if (!h) return 0;
    Locked g(h);
    return h->chain_total;
}

int rio_gp_debug_set_node_index(rio_gp_t* h, uint32_t tile_rows) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    h->ni_force_tile = tile_rows;
    return RIO_GP_OK;
}
int rio_gp_debug_node_index_geometry(rio_gp_t* h, const uint64_t* node_bitmap, uint32_t* out4) {
    if (!h || !out4) return RIO_GP_EINVAL;
    Locked g(h);
    u32 s = 0;
    for (u32 j = 0; j < h->m; ++j) s += !node_bitmap || ((node_bitmap[j >> 6] >> (j & 63)) & 1ull);
    const NiPlan p = ni_plan(h->n, h->m, s, 0, 0, h->ni_force_tile);
    out4[0] = (u32)p.T; out4[1] = p.nt; out4[2] = p.cb; out4[3] = p.W;
    return RIO_GP_OK;
}
int rio_gp_debug_set_speculate(rio_gp_t* h, int speculate) {
    if (!h || speculate < 0 || speculate > 2) return RIO_GP_EINVAL;
    Locked g(h);
    h->spec_mode = speculate;
    return RIO_GP_OK;
}

int rio_gp_debug_ktrace(rio_gp_t* h, int enable, int table, uint64_t* out2048) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (out2048 && ktrace_read(table, reinterpret_cast<u64*>(out2048)) != 0) return fail(h, RIO_GP_EUPSTREAM, "ktrace read failed");
    ktrace_enable(enable);
    return RIO_GP_OK;
}

int rio_gp_debug_stream_probe(rio_gp_t* h, int mode, int reps, float* ms) {
    if (!h || !ms || reps < 1) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipSetDevice(h->device));
    if (mode >= 20 && mode <= 23) {  // host round-trip probes: microseconds per call / 1000
        *ms = sync_probe(mode, reps, h->stream);
        if (*ms < 0) return fail(h, RIO_GP_EUPSTREAM, "sync probe failed");
        return RIO_GP_OK;
    }
    // same columns the solve streams: cur/load/aff in, the ping-pong column out (an uncommitted solve is lost)
    *ms = stream_probe(mode, h->assign[h->cur], h->load, h->aff, h->assign[h->cur ^ 1], h->n, reps, h->stream, h->ev0,
                       h->ev1);
    inputs_changed(h);
    if (*ms < 0) return fail(h, RIO_GP_EUPSTREAM, "stream probe failed");
    return RIO_GP_OK;
}
#endif  // RIO_GP_LAB

int rio_gp_timer_begin(rio_gp_t* h) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    h->timer_stopped = false;
    return RIO_GP_OK;
}

int rio_gp_timer_stop(rio_gp_t* h) {
    if (!h) return RIO_GP_EINVAL;
    Locked g(h);
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    h->timer_stopped = true;
    return RIO_GP_OK;
}

int rio_gp_timer_end(rio_gp_t* h, float* ms) {
    if (!h || !ms) return RIO_GP_EINVAL;
    Locked g(h);
    if (!h->timer_stopped) HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    h->timer_stopped = false;
    HIPCHK(h, hipEventSynchronize(h->ev1));
    HIPCHK(h, hipEventElapsedTime(ms, h->ev0, h->ev1));
    return RIO_GP_OK;
}

}  // extern "C"
