// gpu_object_placement.cpp — host-side mirror of the reference's ObjectPlacement interface
// (include/rio_gpu_object_placement.h) on top of the dense C ABI.  Pure host C++: interning of
// (struct_name, object_id) and "ip:port" strings, the malformed-record rule of the policy, reference
// counting for Clone, and a combining front-end for the single-object calls (concurrent callers share one device
// round trip).  Every placement fact lives in HBM; this file never mirrors the assignment.
//
// Mirrors (relative to /root/reference):
//   LocalObjectPlacement              rio-rs/src/object_placement/local.rs:12-68
//   Service::get_or_create_placement  rio-rs/src/service.rs:193-254
//
// Which rows are objects is a DEVICE fact too (RIO_GP_CFG_ROW_LIFECYCLE): a key that was never inserted, was removed
// (local.rs:36-37,60-68) or was dropped by clean_server (local.rs:51-58) has no entry in the reference's map; here its
// row carries the affinity RIO_GP_AFF_INACTIVE, which keeps it out of every whole-table solve (rio_op_tick), and the
// table's row count on the device is the high-water mark of the rows handed out, not max_objects.  Keys of such rows
// are reclaimed lazily, when the table runs full (reclaim()).
//
// Locks (always taken in this order): mu — compound operations and every device call sequence; imu — the interning
// tables, a reader-writer lock: calls whose key and address are already interned (every lookup, every sticky request) take it
// shared.  Single-object calls that need the device publish themselves on a lock-free list; whoever gets mu next serves
// everything published (flat combining, run_combined).  What the device knows of the host tables (node table, row count)
// is brought up to date under mu by sync_device() BEFORE any device call that may carry a new id, by whichever thread
// issues that call: an id can therefore never reach the device ahead of the table entry it refers to, whoever interned it.
//
// Host shadow of the assignment column (Shadow below).  The reference calls lookup / get_or_create_placement once per request
// from one task per connection (server.rs:292-304), and LocalObjectPlacement answers a hit from a hash map in ~100 ns
// (local.rs:42-49); a device round trip per call is 8-11 us however well it is shared.  So every answer the device gives
// for a row is remembered on the host — node + a stamp — and a later lookup / sticky request of that row is answered from
// there, under the shared table lock, without the device.  The shadow is a cache of DEVICE decisions, never a decision of
// its own: first touches, evictions, capacity and ticks all run on the GPU, and every call that changes rows it cannot
// name (clean_server, a tick, a request batch that cleaned a dead node, reclaimed keys) invalidates by stamp.
// rio_op_cfg.flags & RIO_OP_CFG_NO_HOST_SHADOW switches it off (A/B runs: examples/c_host_threads.c measures both).
#include <linux/futex.h>
#include <sched.h>
#include <sys/syscall.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/rio_gpu_object_placement.h"

// Weak: the dense layer's reverse index is optional to this file — the host-memory stubs the string layer is tested against
// without a GPU need not define it (rio_op_objects_on_server reports RIO_GP_EUPSTREAM then).
extern "C" int rio_gp_rows_on_nodes(rio_gp_t* h, const uint64_t* node_bitmap, uint64_t* out_offsets, uint32_t* out_rows,
                                    uint64_t rows_cap, uint64_t* n_rows) __attribute__((weak));
// Weak for the same reason: the bounded rebalance (rio_op_rebalance reports RIO_GP_EUPSTREAM without it).
extern "C" int rio_gp_rebalance(rio_gp_t* h, const rio_gp_rebalance_cfg* cfg, rio_gp_rebalance_stats* st, uint32_t* out_rows,
                                uint32_t* out_from, uint32_t* out_to, uint64_t moves_cap, uint64_t* n_moves) __attribute__((weak));
// Weak for the same reason: the change feed (rio_op_changes reports RIO_GP_EUPSTREAM without it).
extern "C" int rio_gp_changes(rio_gp_t* h, uint32_t flags, uint32_t* out_rows, uint32_t* out_old, uint32_t* out_new, uint64_t cap,
                              uint64_t* n_changes) __attribute__((weak));
extern "C" int rio_gp_changes_reset(rio_gp_t* h) __attribute__((weak));
// Weak for the same reason: node removal (rio_op_remove_members reports RIO_GP_EUPSTREAM without it).
extern "C" int rio_gp_remap_nodes(rio_gp_t* h, uint32_t m_new, const uint32_t* map, uint64_t* evicted) __attribute__((weak));
// Weak for the same reason: idle expiry (rio_op_expire reports RIO_GP_EUPSTREAM without them).
extern "C" int rio_gp_touch_merge(rio_gp_t* h, uint64_t rows, const uint32_t* stamps) __attribute__((weak));
extern "C" int rio_gp_expire(rio_gp_t* h, uint32_t cutoff, uint32_t* out_rows, uint32_t* out_node, uint64_t cap, uint64_t* n_idle,
                             uint64_t* load_freed) __attribute__((weak));
// Weak for the same reason: measured load (rio_op_fold_loads reports RIO_GP_EUPSTREAM without them).
extern "C" int rio_gp_hits_merge(rio_gp_t* h, uint64_t rows, const uint32_t* counts) __attribute__((weak));
extern "C" int rio_gp_load_fold(rio_gp_t* h, uint32_t keep, uint32_t gain, uint32_t min_load, uint32_t max_load,
                                rio_gp_load_fold_stats* st) __attribute__((weak));
// Weak for the same reason: the hot-object report (rio_op_hottest_objects reports RIO_GP_EUPSTREAM without it).
extern "C" int rio_gp_top_rows(rio_gp_t* h, uint32_t flags, uint32_t node, uint32_t min_key, uint32_t* out_rows, uint32_t* out_key,
                               uint32_t* out_node, uint64_t cap, uint64_t* n_candidates, uint64_t* key_sum) __attribute__((weak));

// Weak for the same reason: object classes (rio_op_expire_by_type and rio_op_census report RIO_GP_EUPSTREAM without them).
extern "C" int rio_gp_set_classes(rio_gp_t* h, uint64_t first_row, uint64_t rows, const uint8_t* cls) __attribute__((weak));
extern "C" int rio_gp_set_class_batch(rio_gp_t* h, uint64_t n, const uint32_t* idx, const uint8_t* cls) __attribute__((weak));
extern "C" int rio_gp_expire_classes(rio_gp_t* h, uint32_t n_classes, const uint32_t* cutoffs, uint32_t* out_rows,
                                     uint32_t* out_node, uint64_t cap, uint64_t* n_idle, uint64_t* load_freed,
                                     uint64_t* idle_by_class) __attribute__((weak));
extern "C" int rio_gp_census(rio_gp_t* h, uint32_t flags, uint32_t n_classes, uint64_t* out_rows, uint64_t* out_load,
                             uint64_t* n_other) __attribute__((weak));
// Weak for the same reason: immovable classes (rio_op_set_type_movable_n reports RIO_GP_EUPSTREAM without it).
extern "C" int rio_gp_set_class_movable(rio_gp_t* h, uint32_t n_classes, const uint8_t* movable) __attribute__((weak));
// Weak for the same reason: pressure shedding (rio_op_shed_idle reports RIO_GP_EUPSTREAM without it).
extern "C" int rio_gp_shed_idle(rio_gp_t* h, const rio_gp_shed_cfg* cfg, rio_gp_shed_stats* st, uint32_t* out_rows, uint32_t* out_node,
                                uint64_t rows_cap, uint64_t* n_rows) __attribute__((weak));

namespace {

// one spin-wait step that tells the core (and its sibling thread) that this is one
#if defined(__x86_64__) || defined(__i386__)
static inline void cpu_relax() { __builtin_ia32_pause(); }
#elif defined(__aarch64__)
static inline void cpu_relax() { __asm__ __volatile__("yield" ::: "memory"); }
#else
static inline void cpu_relax() { __asm__ __volatile__("" ::: "memory"); }
#endif
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ != __ORDER_LITTLE_ENDIAN__
#error "Req::futex_word takes the upper half of a 64-bit word as the word at offset 4: little-endian hosts only"
#endif

constexpr int kFull = -1000;  // internal: the object table has no free row (reclaim, then retry)
constexpr int kNoop = -1001;  // internal: nothing to do on the device (an unknown key looked up / removed / deleted)
constexpr int kUpgrade = -1002;  // internal: the call has to change the interning tables — again, under the exclusive lock
constexpr int kHit = -1003;      // internal: answered from the host shadow, no device round trip

// Text of the calling thread's last failed call (rio_op_last_error): a failure is reported to the thread that made
// the call, so its text is that thread's too — no lock, no race with other callers' failures.
thread_local std::string t_err;
// length of the address the calling thread's last rio_op_lookup / rio_op_get_or_create_placement produced
// (rio_op_last_address_len): what a caller whose buffer was too small (RIO_GP_ERANGE) allocates before it asks again
thread_local size_t t_addr_len = 0;
// rio_op_expire's stamps and rio_op_fold_loads' counters on their way to the device, and rio_op_get_object_load's copy of the
// load column
thread_local std::vector<uint32_t> t_ex_stamps, t_ld_hits, t_ld_col;

// One single-object call waiting for its device round trip (see run_combined).
// One single-object call waiting for its device round trip (see run_combined).  The struct is a cache line of its own: its
// caller spins on `result` while every other waiter spins on theirs.  The serving thread reads the inputs once and answers
// with ONE store — node, flag, return code and the "done" bit packed into a word: with the answer spread over four fields the
// waiter's polling pulled the line back between the server's stores, four or five transfers per request, 40 us of a 64-request
// batch (measured).
struct alignas(64) Req {
    int kind;                 // 0 lookup | 1 get_or_create_placement | 2 update | 3 remove
    uint32_t row, req;        // dense ids (req: requester node for kind 1, new node or NONE for kind 2)
    std::atomic<uint64_t> result{0};  // kDone | rc << 40 | flag << 32 | node: stored LAST, and once, by the serving thread (the
                                      // request lives on its caller's stack)
    std::string err;          // text of ITS failure (a request that fails does not fail its batch-mates): written before `result`
    // the caller's view of the answer, unpacked by the caller itself
    uint32_t node = RIO_GP_NONE, flag = 0;
    int rc = RIO_GP_OK;
    static constexpr uint64_t kDone = 1ull << 63;
    static constexpr uint64_t kSleep = 1ull << 62;  // set by the caller before it sleeps on the word's upper half (a futex)
    uint32_t* futex_word() { return reinterpret_cast<uint32_t*>(&result) + 1; }  // little-endian: bits 32..63
    static uint64_t pack(int rc, uint32_t node, uint32_t flag) {
        return kDone | ((uint64_t)(uint8_t)rc << 40) | ((uint64_t)(flag & 0xFFu) << 32) | node;
    }
    void unpack(uint64_t w) { node = (uint32_t)w; flag = (uint32_t)(w >> 32) & 0xFFu; rc = (int)((w >> 40) & 0xFFu); }
};

// Where a caller leaves its request for the serving thread: 32 bytes, filled by the caller (in parallel with every other caller),
// read by the server as an array — a linked list through the callers' own stack frames cost the server a dependent cache miss
// per request (25 us for 28 requests, measured at 64 callers over two sockets).
constexpr uint32_t kSlots = 512;
struct alignas(32) Slot {
    std::atomic<uint64_t> tag{0};  // (generation + 1) << 8 | kind: stored LAST by the caller; the server waits for its generation's tag
    uint32_t row = 0, req = 0;
    Req* r = nullptr;
};

// Host shadow of the assignment column: entry = stamp << 16 | node (0xFFFF = not placed), one atomic u64 per row, in chunks of
// 65 536 rows allocated as rows are handed out.  Writers hold State::mu (the order of the device calls IS the order of the
// writes); readers hold nothing but the shared table lock that keeps their row id theirs.
//   valid(entry) = stamp >= base  &&  (node == none || stamp >= clean_stamp[node])
//   clean_server(j): clean_stamp[j] = ++clock  (the rows that sat on j are gone; every other row's entry stays good)
//   tick / a request batch that ran into a dead node / anything that moves rows it cannot name: base = ++clock
struct Shadow {
    static constexpr uint32_t kBits = 16, kNoneNode = 0xFFFFu;
    bool enabled = true;
    size_t nchunks = 0;
    std::unique_ptr<std::atomic<std::atomic<uint64_t>*>[]> chunks;
    std::unique_ptr<std::atomic<uint64_t>[]> clean_stamp;
    std::atomic<uint64_t> clock{1}, base{1};
    void init(uint64_t max_objects, uint32_t max_nodes, bool on) {
        enabled = on;
        nchunks = (size_t)((max_objects + (1u << kBits) - 1) >> kBits);
        chunks.reset(new std::atomic<std::atomic<uint64_t>*>[nchunks ? nchunks : 1]);
        for (size_t c = 0; c < (nchunks ? nchunks : 1); ++c) chunks[c].store(nullptr, std::memory_order_relaxed);
        clean_stamp.reset(new std::atomic<uint64_t>[max_nodes ? max_nodes : 1]);
        for (uint32_t j = 0; j < (max_nodes ? max_nodes : 1); ++j) clean_stamp[j].store(0, std::memory_order_relaxed);
    }
    ~Shadow() {
        for (size_t c = 0; c < nchunks; ++c) delete[] chunks[c].load(std::memory_order_relaxed);
    }
    bool get(uint32_t row, uint32_t* node) const {  // (any thread; the caller's row id is pinned by the shared table lock)
        if (!enabled) return false;
        const std::atomic<uint64_t>* ch = chunks[row >> kBits].load(std::memory_order_acquire);
        if (!ch) return false;
        const uint64_t e = ch[row & ((1u << kBits) - 1)].load(std::memory_order_acquire);
        const uint64_t stamp = e >> 16;
        const uint32_t nd = (uint32_t)(e & 0xFFFFu);
        if (stamp < base.load(std::memory_order_acquire)) return false;
        if (nd != kNoneNode && stamp < clean_stamp[nd].load(std::memory_order_acquire)) return false;
        *node = nd == kNoneNode ? RIO_GP_NONE : nd;
        return true;
    }
    void put(uint32_t row, uint32_t node) {  // mu held: what the device just said (or was just told) about the row
        if (!enabled) return;
        std::atomic<uint64_t>* ch = chunks[row >> kBits].load(std::memory_order_relaxed);
        if (!ch) {
            ch = new std::atomic<uint64_t>[1u << kBits];
            for (uint32_t k = 0; k < (1u << kBits); ++k) ch[k].store(0, std::memory_order_relaxed);
            chunks[row >> kBits].store(ch, std::memory_order_release);
        }
        const uint64_t nd = node == RIO_GP_NONE ? kNoneNode : (node & 0xFFFFu);
        ch[row & ((1u << kBits) - 1)].store((clock.load(std::memory_order_relaxed) << 16) | nd, std::memory_order_release);
    }
    void erase(uint32_t row) {  // mu + exclusive table lock held: the row changes hands (reclaim)
        std::atomic<uint64_t>* ch = chunks[row >> kBits].load(std::memory_order_relaxed);
        if (ch) ch[row & ((1u << kBits) - 1)].store(0, std::memory_order_release);
    }
    void clean(uint32_t node) { clean_stamp[node].store(clock.fetch_add(1, std::memory_order_acq_rel) + 1, std::memory_order_release); }
    void invalidate_all() { base.store(clock.fetch_add(1, std::memory_order_acq_rel) + 1, std::memory_order_release); }
};

// Last-seen stamps (rio_op_set_clock / rio_op_expire): the host's clock value at which a call last answered or set an address
// for the row's key, one atomic u32 per row in chunks of 65 536 rows allocated by whoever stamps first (any thread: the chunk
// pointer is installed with a compare-exchange).  While the clock is 0 a call pays one relaxed load of it and nothing more.  A
// stamp is a maximum and is written only when the word is lower than the clock: a hot row costs one read-modify-write per clock
// value, not one per call.  Stampers hold the shared side of the table lock, or count as in flight (their row id is theirs);
// rio_op_expire reads the words under the exclusive side.  A row that reclaim() hands to another key keeps its stamp: stamps
// only rise, on the host as on the device, so a recycled row counts as seen when its previous key was, until its own first call.
//
// Request counters (rio_op_set_load_tracking / rio_op_fold_loads) sit next to the stamps, in chunks installed the same way: the
// sites that stamp a key are the sites that count a request for it, so stamp() does both and each is off behind one relaxed load.
// A counter saturates at 2^32-1.  rio_op_fold_loads takes each word with an exchange: a request counted by a call in flight
// (which holds no lock) lands in this fold or in the next one, never in both and never in neither.
struct Stamps {
    static constexpr uint32_t kBits = 16;
    typedef std::atomic<std::atomic<uint32_t>*> Slot;
    // the clock (low half; 0: stamping off) and the tracking switch (bit 32) in ONE word: with both off a call pays one relaxed
    // load of it and nothing more, exactly what it paid for the clock alone
    static constexpr uint64_t kTrack = 1ull << 32;
    std::atomic<uint64_t> ctl{0};
    void set_clock(uint32_t now) {
        uint64_t c = ctl.load(std::memory_order_relaxed);
        while (!ctl.compare_exchange_weak(c, (c & kTrack) | now, std::memory_order_relaxed)) {}
    }
    void set_tracking(bool on) {
        if (on) ctl.fetch_or(kTrack, std::memory_order_relaxed);
        else ctl.fetch_and(~kTrack, std::memory_order_relaxed);
    }
    size_t nchunks = 0;
    std::unique_ptr<Slot[]> chunks, hit_chunks;
    void init(uint64_t max_objects) {
        nchunks = (size_t)((max_objects + (1u << kBits) - 1) >> kBits);
        chunks.reset(new Slot[nchunks ? nchunks : 1]);
        hit_chunks.reset(new Slot[nchunks ? nchunks : 1]);
        for (size_t c = 0; c < (nchunks ? nchunks : 1); ++c) {
            chunks[c].store(nullptr, std::memory_order_relaxed);
            hit_chunks[c].store(nullptr, std::memory_order_relaxed);
        }
    }
    ~Stamps() {
        for (size_t c = 0; c < nchunks; ++c) {
            delete[] chunks[c].load(std::memory_order_relaxed);
            delete[] hit_chunks[c].load(std::memory_order_relaxed);
        }
    }
    // the row's word of a column of chunks, its chunk installed (zero-filled) by whoever gets there first
    static std::atomic<uint32_t>& word(Slot* col, uint32_t row) {
        Slot& slot = col[row >> kBits];
        std::atomic<uint32_t>* ch = slot.load(std::memory_order_acquire);
        if (!ch) {
            std::atomic<uint32_t>* fresh = new std::atomic<uint32_t>[1u << kBits];
            for (uint32_t k = 0; k < (1u << kBits); ++k) fresh[k].store(0, std::memory_order_relaxed);
            if (slot.compare_exchange_strong(ch, fresh, std::memory_order_acq_rel, std::memory_order_acquire)) ch = fresh;
            else delete[] fresh;  // (somebody else's chunk is in: ch holds it)
        }
        return ch[row & ((1u << kBits) - 1)];
    }
    // a call answered or set an address for the row's key: one request counted (tracking on), the clock stamped (clock set)
    void stamp(uint32_t row) {
        const uint64_t c = ctl.load(std::memory_order_relaxed);
        if (!c) return;
        if (c & kTrack) {
            std::atomic<uint32_t>& hc = word(hit_chunks.get(), row);
            uint32_t cur = hc.load(std::memory_order_relaxed);
            while (cur != 0xFFFFFFFFu && !hc.compare_exchange_weak(cur, cur + 1, std::memory_order_relaxed)) {}
        }
        const uint32_t t = (uint32_t)c;
        if (!t) return;
        std::atomic<uint32_t>& w = word(chunks.get(), row);
        uint32_t cur = w.load(std::memory_order_relaxed);
        while (cur < t && !w.compare_exchange_weak(cur, t, std::memory_order_relaxed)) {}
    }
    // the request counters of rows 0 .. n-1, each taken and left at 0; false: none was non-zero (out is not to be used)
    bool take_hits(uint64_t n, std::vector<uint32_t>& out) {
        bool any = false;
        out.assign(n, 0u);
        for (uint64_t r0 = 0; r0 < n; r0 += (1u << kBits)) {
            std::atomic<uint32_t>* ch = hit_chunks[r0 >> kBits].load(std::memory_order_acquire);
            if (!ch) continue;
            const uint64_t k1 = std::min<uint64_t>(n - r0, 1u << kBits);
            for (uint64_t k = 0; k < k1; ++k) {
                if (!ch[k].load(std::memory_order_relaxed)) continue;
                out[r0 + k] = ch[k].exchange(0u, std::memory_order_relaxed);
                any = any || out[r0 + k] != 0;
            }
        }
        return any;
    }
    // put counters taken by take_hits back (the device refused them): saturating, next to whatever was counted since
    void give_back(const std::vector<uint32_t>& v) {
        for (uint64_t r = 0; r < v.size(); ++r) {
            if (!v[r]) continue;
            std::atomic<uint32_t>& c = word(hit_chunks.get(), (uint32_t)r);
            uint32_t cur = c.load(std::memory_order_relaxed);
            while (!c.compare_exchange_weak(cur, cur + v[r] < cur ? 0xFFFFFFFFu : cur + v[r], std::memory_order_relaxed)) {}
        }
    }
    // a row that changes hands starts at 0 requests
    void clear_hits(uint32_t row) {
        std::atomic<uint32_t>* ch = hit_chunks[row >> kBits].load(std::memory_order_acquire);
        if (ch) ch[row & ((1u << kBits) - 1)].store(0u, std::memory_order_relaxed);
    }
    // the stamps of rows 0 .. n-1 (0: never stamped); false: nothing has ever been stamped (out is not written)
    bool gather(uint64_t n, std::vector<uint32_t>& out) const {
        bool any = false;
        for (size_t c = 0; c < nchunks && !any; ++c) any = chunks[c].load(std::memory_order_acquire) != nullptr;
        if (!any) return false;
        out.assign(n, 0u);
        for (uint64_t r0 = 0; r0 < n; r0 += (1u << kBits)) {
            const std::atomic<uint32_t>* ch = chunks[r0 >> kBits].load(std::memory_order_acquire);
            if (!ch) continue;
            const uint64_t k1 = std::min<uint64_t>(n - r0, 1u << kBits);
            for (uint64_t k = 0; k < k1; ++k) out[r0 + k] = ch[k].load(std::memory_order_relaxed);
        }
        return true;
    }
};

// The table lock: readers are every single-object call (a shadow hit holds it for ~0.3 us and touches nothing else that is
// shared), writers are rare (a key or an address nobody has seen, a reclaim, the batched calls' interning).  std::shared_mutex
// keeps ONE reader count: two read-modify-writes of one cache line per call, 16 callers on two sockets spent most of a hit
// waiting for that line (1.6e6 hits/s from one thread, 4.4e6 from 16).  Here every thread counts itself in on a line of its
// own group (32 groups, threads dealt round robin); a writer raises its flag, then waits for every group to drain (Dekker's
// handshake: both sides sequentially consistent).  Writer-preferring: a reader that sees the flag steps back until it is gone.
class TableLock {
    static constexpr uint32_t kGroups = 32;
    struct alignas(64) Group { std::atomic<uint32_t> readers{0}; };
    Group groups_[kGroups];
    alignas(64) std::atomic<uint32_t> writer_{0};
    std::mutex wmu_;  // one writer at a time; writers queue here, asleep
    static uint32_t my_group() {
        static std::atomic<uint32_t> next{0};
        static thread_local uint32_t mine = next.fetch_add(1, std::memory_order_relaxed) % kGroups;
        return mine;
    }
    static void backoff(unsigned spin) {
        if (spin < 256) { cpu_relax(); return; }
        if (spin < 512) { sched_yield(); return; }
        const timespec ts{0, 50000};  // a reclaim or a big batch's interning holds the lock for milliseconds: do not burn a CPU on it
        nanosleep(&ts, nullptr);
    }

 public:
    void lock_shared() {
        std::atomic<uint32_t>& r = groups_[my_group()].readers;
        for (unsigned spin = 0;;) {
            r.fetch_add(1, std::memory_order_seq_cst);
            if (!writer_.load(std::memory_order_seq_cst)) return;
            r.fetch_sub(1, std::memory_order_seq_cst);
            while (writer_.load(std::memory_order_acquire)) backoff(spin++);
        }
    }
    bool try_lock_shared() {  // never waits: false while a writer holds or wants the lock
        std::atomic<uint32_t>& r = groups_[my_group()].readers;
        r.fetch_add(1, std::memory_order_seq_cst);
        if (!writer_.load(std::memory_order_seq_cst)) return true;
        r.fetch_sub(1, std::memory_order_seq_cst);
        return false;
    }
    void unlock_shared() { groups_[my_group()].readers.fetch_sub(1, std::memory_order_release); }
    void lock() {
        wmu_.lock();
        writer_.store(1, std::memory_order_seq_cst);
        for (Group& g : groups_)
            for (unsigned spin = 0; g.readers.load(std::memory_order_seq_cst) != 0;) backoff(spin++);
    }
    void unlock() {
        writer_.store(0, std::memory_order_release);
        wmu_.unlock();
    }
};

// node id -> address.  The strings live in `store`, which never moves or frees one: rio_op_node_address and rio_op_changes hand
// out their c_str(), valid until rio_op_release.  Removing nodes (rio_op_remove_members) rebuilds the id table only; the strings
// of removed nodes stay behind in `store` (the graveyard), and an address that comes back gets a new string with its new id.
struct NodeAddrs {
    std::deque<std::string> store;
    std::vector<const std::string*> by_id;
    size_t size() const { return by_id.size(); }
    const std::string& operator[](size_t id) const { return *by_id[id]; }
    void push_back(const std::string& a) {
        store.push_back(a);
        by_id.push_back(&store.back());
    }
};

struct State {
    // (the words many threads hammer at once sit on cache lines of their own: 64 waiters trying the device lock on the line the
    //  publishers' list head and the table lock's reader count live on cost 50 us per combined batch, measured)
    alignas(64) std::mutex mu;    // compound operations and their device call sequences (taken first)
    alignas(64) std::atomic<int> busy{0};  // somebody holds mu: waiters look at this (a shared read) before they try the lock
    alignas(64) TableLock imu;          // the interning tables below (taken second, or alone by the single-object calls, which must
                            // be able to intern and publish while the serving thread waits for the device); shared: read-only use
    // Published single-object calls: tickets of the current generation (generation << 32 | requests so far) and two slot arrays
    // (generation & 1).  A caller takes a ticket, fills its slot and tags it; ticket 0 of a generation serves that generation.
    alignas(64) std::atomic<uint64_t> ticket{0};
    alignas(64) Slot slots[2][kSlots];
    alignas(64) std::vector<Req*> batch;  // (under mu) the requests the serving thread took off the list, oldest first
    std::vector<uint64_t> results;        // (under mu) their packed answers
    std::vector<int> sv_kind;             // (under mu) serve()'s scratch: no allocation per batch
    std::vector<uint32_t> sv_row, sv_req;
    struct KindBuf { std::vector<uint32_t> rows, reqs, res, fl, who; } sv_kb[4];  // the batch split by kind
    Shadow shadow;
    Stamps seen;
    uint64_t dev_batches = 0, dev_requests = 0;  // (under mu) device round trips of combined batches / requests they carried
    size_t last_batch = 0, prev_batch = 0;       // (under mu) requests of the last two combined batches
    uint32_t collect_ns = 0;                     // rio_op_cfg.collect_ns
    uint32_t cpus = 1;                           // CPUs this process may use at once (affinity mask, cgroup quota)
    std::atomic<uint32_t> spin_ns{30000};        // how long a waiting caller spins before it sleeps (set by the servers)
    bool self_assign = true;                     // requests first-touch their requester whatever membership says (the default)
    rio_gp_t* gp = nullptr;
    uint64_t max_objects = 0;
    uint32_t max_nodes = 0;
    // --- under imu ---
    std::unordered_map<std::string, uint32_t> rows;   // "{type}.{id}" -> dense row (local.rs:26-29)
    std::deque<std::pair<std::string, std::string>> row_key;  // row -> the (struct_name, object_id) it is interned as
    std::vector<uint8_t> row_live;                    // row currently has a key
    std::vector<uint8_t> row_keep;                    // key created by rio_op_set_object_load and not used since: its load is
                                                      // what the caller set, so reclaim() must not recycle (and reset) the row
    std::vector<uint32_t> free_rows;                  // reclaimed rows, ready for new keys
    // object classes: the first distinct struct_name interned is class 0, the next 1, ... up to 254; every further one shares
    // RIO_OP_CLASS_OTHER and is not remembered.  The table never shrinks (a deque: the strings never move, rio_op_census hands
    // out pointers into them).  A row's class is that of row_key[row].first, set when the row is handed to a key.
    std::unordered_map<std::string, uint8_t> type_id;
    std::deque<std::string> type_name;
    std::vector<uint32_t> type_limit;                 // rio_op_set_type_idle_limit_n, per type id
    std::vector<uint8_t> type_has_limit;
    // rio_op_set_type_movable_n, per type id: 1 = the rebalance leaves the type's keys where they are.  n_immovable: how many
    // are; mv_dirty: the table changed since the dense layer last got it (read by the rebalance under mu + imu exclusive);
    // mv_on_device: the dense table names an immovable class
    std::vector<uint8_t> type_immovable;
    uint32_t n_immovable = 0;
    bool mv_dirty = false, mv_on_device = false;
    std::vector<uint8_t> row_class;                   // row -> class
    // (written under imu exclusive, read by the uploads under mu + imu exclusive) what the device's class column holds: rows
    // [0, cls_uploaded) as of the last upload, except the rows in cls_dirty, which were handed to a key of another class since
    uint64_t cls_uploaded = 0;
    std::vector<uint32_t> cls_dirty;
    std::atomic<uint64_t> hi_rows{0};                 // rows ever handed out: every row id is < hi_rows (atomic: sync_device looks
                                                      // at it and at the two versions below without the table lock)
    std::unordered_map<std::string, uint32_t> nodes;  // address -> node id
    NodeAddrs node_addr;                              // the strings never move (rio_op_node_address)
    std::vector<uint8_t> node_alive, node_malformed;
    std::vector<uint64_t> node_cap;
    uint32_t n_malformed = 0;
    std::atomic<uint64_t> node_version{1};            // bumped on every change of the node table
    std::atomic<uint64_t> shape_version{1};           // bumped when a node is added or a capacity changes (not on liveness flips)
    bool reclaiming = false;                          // single-object calls wait (rcv) while keys are being reclaimed, or nodes
                                                      // removed (rio_op_remove_members: the node ids they carry are renumbered)
    std::condition_variable_any rcv;
    // --- under mu ---
    uint64_t pushed_version = 0;                      // node_version the device holds
    uint64_t pushed_shape = 0;
    uint32_t pushed_nodes = 0;
    uint64_t pushed_rows = 0;                         // row count the device holds (rio_gp_set_num_objects)
    // change feed (rio_op_changes): on from its first call; `full` until a listing after creation or a reset; `retired`: for
    // every row reclaim() handed back since the last listing, the key the consumer's mirror knows for it — the FIRST key retired
    // from the row (a later one never reached the mirror)
    bool feed_on = false, feed_full = true;
    std::unordered_map<uint32_t, std::pair<std::string, std::string>> retired;
    // ---
    std::atomic<int> inflight{0};                     // single-object calls between their intern and their return
    std::atomic<int> refs{1};
};

// A key part as the caller handed it over: NUL-terminated (len < 0) or with its length (the _n entry points: a Rust
// String may hold a NUL byte, service_object.rs:19-26).
struct Part {
    const char* p;
    ptrdiff_t len;
    Part(const char* c) : p(c ? c : ""), len(-1) {}
    Part(const char* c, size_t n) : p(c ? c : ""), len((ptrdiff_t)(c ? n : 0)) {}
    Part(const std::string& str) : p(str.data()), len((ptrdiff_t)str.size()) {}
    std::string str() const { return len < 0 ? std::string(p) : std::string(p, (size_t)len); }
};
// the keys of a batched call: NUL-terminated arrays, or arrays with lengths (the _batch_n entry points)
struct Keys {
    const char* const* tys; const size_t* tyl;
    const char* const* ids; const size_t* idl;
    Part ty(uint64_t k) const { return tyl ? Part(tys[k], tyl[k]) : Part(tys[k]); }
    Part id(uint64_t k) const { return idl ? Part(ids[k], idl[k]) : Part(ids[k]); }
};
std::string key_of(const Part& ty, const Part& id) {  // local.rs:26-29,43,61
    std::string k = ty.str();
    k += '.';
    k += id.str();
    return k;
}

// service.rs:204-213: splitn(2, ":"), a record is bad when ip or port is empty
bool malformed(const std::string& a) {
    const size_t c = a.find(':');
    return c == std::string::npos || c == 0 || c + 1 >= a.size();
}

int fail(int rc, const std::string& m) {
    t_err = m;
    return rc;
}
// mu for a compound call: taken blocking, and marked busy so that single-object callers wait on the flag, not on the lock word
struct DevLock {
    State* s;
    explicit DevLock(State* st) : s(st) { s->mu.lock(); s->busy.store(1, std::memory_order_relaxed); }
    ~DevLock() { s->busy.store(0, std::memory_order_release); s->mu.unlock(); }
    DevLock(const DevLock&) = delete;
    DevLock& operator=(const DevLock&) = delete;
};
int gp_fail(State* s, int rc) {  // only directly after the failing rio_gp_* call, under mu (nobody else calls the handle)
    const char* e = rio_gp_last_error(s->gp);
    t_err = e ? e : "";
    return rc;
}

// What a key-listing call hands out: entry k is (ty[k], tylen[k], id[k], idlen[k]) and up to two addresses.  The keys are
// copies in `store` (two strings per entry): a key can be reclaimed as soon as the locks are released.  The addresses point into
// the node table, whose strings stay until rio_op_release (NodeAddrs).  Every listing function has ONE instance per thread, so
// its arrays are the calling thread's until its next call of that same function, whatever else the thread calls meanwhile.
struct KeyListing {
    std::vector<std::string> store;
    std::vector<const char*> ty, id, a0, a1;
    std::vector<size_t> tylen, idlen;
    std::vector<uint32_t> rows, c1, c2;  // scratch the dense call fills: clear() leaves it, the next call sizes its first try from it
    void clear() {
        store.clear();
        ty.clear(); id.clear(); a0.clear(); a1.clear(); tylen.clear(); idlen.clear();
    }
    void add(const std::pair<std::string, std::string>& key, const char* x0 = nullptr, const char* x1 = nullptr) {
        store.push_back(key.first);
        store.push_back(key.second);
        a0.push_back(x0);
        a1.push_back(x1);
    }
    // the key of a row the dense layer listed (imu held); false: the row has no key at the moment and is left out
    bool add(const State* s, uint32_t row, const char* x0 = nullptr, const char* x1 = nullptr) {
        if (row >= s->row_live.size() || !s->row_live[row]) return false;
        add(s->row_key[row], x0, x1);
        return true;
    }
    // After the locks are released, and only once `store` is complete (a string's bytes may move while it grows): the pointer
    // and length arrays, and the caller's out-parameters (those it has).
    void publish(uint64_t* n, const char* const** tys, const size_t** tyl, const char* const** ids, const size_t** idl,
                 const char* const** x0 = nullptr, const char* const** x1 = nullptr) {
        for (size_t k = 0; k + 1 < store.size(); k += 2) {
            ty.push_back(store[k].c_str());
            tylen.push_back(store[k].size());
            id.push_back(store[k + 1].c_str());
            idlen.push_back(store[k + 1].size());
        }
        *n = ty.size();
        *tys = ty.data();
        *ids = id.data();
        if (tyl) *tyl = tylen.data();
        if (idl) *idl = idlen.data();
        if (x0) *x0 = a0.data();
        if (x1) *x1 = a1.data();
    }
};
thread_local KeyListing t_snap, t_on, t_rb, t_ch, t_ex, t_hot;

// the address of a node id as the listings hand it out: into the node table, `none` for an id without an address
const char* addr_of(const State* s, uint32_t nd, const char* none = nullptr) {
    return nd < s->node_addr.size() ? s->node_addr[nd].c_str() : none;
}

// Bring the device's copy of the host tables up to date: the node table (any new address, liveness or capacity change)
// and the row count.  Requires mu; imu is taken here unless the caller already holds it.
int sync_device(State* s, bool imu_held) {
    // (the common case — nothing new since the last device call — takes no lock: with 64 callers interning, the serving thread
    //  queued 20 us per batch for a reader slot of the table lock here)
    if (s->node_version.load(std::memory_order_acquire) == s->pushed_version &&
        s->hi_rows.load(std::memory_order_acquire) == s->pushed_rows) return RIO_GP_OK;
    std::vector<uint64_t> cap;
    std::vector<uint8_t> alive;
    uint64_t version, shape, nrows;
    uint32_t m;
    {
        std::shared_lock<TableLock> li(s->imu, std::defer_lock);
        if (!imu_held) li.lock();
        version = s->node_version;
        shape = s->shape_version;
        m = (uint32_t)s->node_addr.size();
        nrows = s->hi_rows;
        if (version != s->pushed_version) {
            cap = s->node_cap;
            alive = s->node_alive;
        }
    }
    if (version != s->pushed_version) {
        // a liveness flip alone is one small asynchronous kernel (MembershipStorage::set_is_active pushed, not polled);
        // a new address or a capacity change replaces the node table
        const int rc = (shape == s->pushed_shape && m == s->pushed_nodes && m > 0)
                           ? rio_gp_set_alive_all(s->gp, m, alive.data())
                           : rio_gp_set_nodes(s->gp, m, cap.data(), alive.data());
        if (rc) return gp_fail(s, rc);
        s->pushed_version = version;
        s->pushed_shape = shape;
        s->pushed_nodes = m;
    }
    if (nrows != s->pushed_rows) {
        const int rc = rio_gp_set_num_objects(s->gp, nrows);
        if (rc) return gp_fail(s, rc);
        s->pushed_rows = nrows;
    }
    return RIO_GP_OK;
}

// find or create the node id of an address (imu held; excl: exclusively — a shared holder that would have to create gets kUpgrade)
int intern_node(State* s, const std::string& addr, bool create, uint32_t* out, bool mark_up = false, bool excl = true) {
    auto it = s->nodes.find(addr);
    if (it != s->nodes.end()) {
        *out = it->second;
        return RIO_GP_OK;
    }
    if (!create) {
        *out = RIO_GP_NONE;
        return RIO_GP_OK;
    }
    if (!excl) return kUpgrade;
    if (s->node_addr.size() >= s->max_nodes) return fail(RIO_GP_EINVAL, "node table full (max_nodes)");
    const uint32_t id = (uint32_t)s->node_addr.size();
    s->nodes.emplace(addr, id);
    s->node_addr.push_back(addr);
    // not a member until rio_op_set_member says so (is_active == false) — except a server that answers requests itself
    s->node_alive.push_back(mark_up ? 1 : 0);
    s->node_cap.push_back(RIO_GP_CAP_INF);
    const bool bad = malformed(addr);
    s->node_malformed.push_back(bad ? 1 : 0);
    s->n_malformed += bad;
    ++s->node_version;
    ++s->shape_version;
    *out = id;
    return RIO_GP_OK;
}

// the class of a struct_name, giving it the next id when it is new and one is left (imu held exclusively)
uint8_t intern_type(State* s, const std::string& ty) {
    auto it = s->type_id.find(ty);
    if (it != s->type_id.end()) return it->second;
    if (s->type_name.size() >= RIO_OP_CLASS_OTHER) return RIO_OP_CLASS_OTHER;
    const uint8_t c = (uint8_t)s->type_name.size();
    s->type_name.push_back(ty);
    s->type_limit.push_back(0);
    s->type_has_limit.push_back(0);
    s->type_immovable.push_back(0);
    s->type_id.emplace(ty, c);
    return c;
}

// find or create the row of a key (imu held).  kFull: no free row — the caller releases its locks, runs reclaim() and retries.
// use: the call makes (or unmakes) an object of the key — update, get_or_create_placement, remove; a key whose row is
// held for a load set ahead of its first use (row_keep) is an ordinary key from then on
int intern_row(State* s, const Part& ty, const Part& id, bool create, uint32_t* out, bool use = false, bool excl = true) {
    const std::string key = key_of(ty, id);
    auto it = s->rows.find(key);
    if (it != s->rows.end()) {
        *out = it->second;
        if (use && s->row_keep[it->second]) {
            if (!excl) return kUpgrade;
            s->row_keep[it->second] = 0;
        }
        return RIO_GP_OK;
    }
    if (!create) {
        *out = RIO_GP_NONE;
        return RIO_GP_OK;
    }
    if (!excl) return kUpgrade;
    uint32_t row;
    if (!s->free_rows.empty()) {
        row = s->free_rows.back();
        s->free_rows.pop_back();
    } else if (s->hi_rows < s->max_objects) {
        row = (uint32_t)s->hi_rows.fetch_add(1, std::memory_order_acq_rel);
        s->row_key.emplace_back();
        s->row_live.push_back(0);
        s->row_keep.push_back(0);
        s->row_class.push_back(0);
    } else {
        return kFull;
    }
    s->rows.emplace(key, row);
    s->row_key[row] = std::make_pair(ty.str(), id.str());
    const uint8_t cls = intern_type(s, s->row_key[row].first);
    if (cls != s->row_class[row]) {
        s->row_class[row] = cls;
        if (row < s->cls_uploaded) s->cls_dirty.push_back(row);  // (a reclaimed row: the device still holds its old key's class)
    }
    s->row_live[row] = 1;
    s->row_keep[row] = use ? 0 : 1;  // created without a use: rio_op_set_object_load ahead of the first update / request
    *out = row;
    return RIO_GP_OK;
}

// The table is full: give the rows of keys that are no longer objects (unplaced AND affinity RIO_GP_AFF_INACTIVE on the
// device: removed, deleted, dropped by clean_server and not touched since) back to the free list and forget their keys —
// what HashMap::remove / retain do at once in the reference (local.rs:36-37,51-68).  Row ids live in single-object calls
// between their intern and their return, so those are drained first and held off meanwhile; compound calls are excluded
// by mu.  EINVAL when every row belongs to a live object.
int reclaim(State* s) {
    {
        std::unique_lock<TableLock> li(s->imu);
        while (s->reclaiming) s->rcv.wait(li);  // someone else is at it: wait, then let the caller retry
        if (!s->free_rows.empty() || s->hi_rows < s->max_objects) return RIO_GP_OK;
        s->reclaiming = true;
    }
    while (s->inflight.load(std::memory_order_acquire) != 0) sched_yield();
    int rc = RIO_GP_OK;
    size_t got = 0;
    {
        DevLock g(s);
        std::lock_guard<TableLock> gi(s->imu);
        const uint64_t n = s->hi_rows;
        std::vector<uint32_t> assign(n ? n : 1), aff(n ? n : 1), gone, ones;
        if ((rc = sync_device(s, true)) == RIO_GP_OK) {
            if ((rc = rio_gp_get_assign(s->gp, n, assign.data())) || (rc = rio_gp_get_objects(s->gp, n, nullptr, aff.data())))
                rc = gp_fail(s, rc);
        }
        if (rc == RIO_GP_OK) {
            for (uint64_t r = 0; r < n; ++r)
                if (s->row_live[r] && !s->row_keep[r] && assign[r] == RIO_GP_NONE && aff[r] == RIO_GP_AFF_INACTIVE) {
                    if (s->feed_on) s->retired.emplace((uint32_t)r, s->row_key[r]);  // (kept if the row was retired before)
                    s->rows.erase(key_of(s->row_key[r].first, s->row_key[r].second));
                    s->row_key[r] = std::pair<std::string, std::string>();
                    s->row_live[r] = 0;
                    s->shadow.erase((uint32_t)r);  // the row changes hands: what the shadow knew of it belonged to the old key
                    s->seen.clear_hits((uint32_t)r);  // ... and so did the requests counted for it
                    s->free_rows.push_back((uint32_t)r);
                    gone.push_back((uint32_t)r);
                }
            got = gone.size();
            if (got) {  // a recycled row starts like a fresh one: load 1
                ones.assign(got, 1u);
                if ((rc = rio_gp_set_object_attrs(s->gp, got, gone.data(), ones.data(), nullptr))) rc = gp_fail(s, rc);
            }
        }
        s->reclaiming = false;
    }
    s->rcv.notify_all();
    if (rc) return rc;
    if (!got) return fail(RIO_GP_EINVAL, "object table full (max_objects live objects)");
    return RIO_GP_OK;
}

// The address into the caller's buffer, whole or not at all: the reference returns an owned String of any length
// (local.rs:42-49), so nothing is ever truncated.  RIO_GP_ERANGE: the buffer is too small — out holds "" and
// rio_op_last_address_len() says how many bytes (without the NUL) the address has.
int copy_out(const std::string& v, char* out, size_t cap) {
    t_addr_len = v.size();
    if (out && cap) out[0] = 0;
    if (!out || cap < v.size() + 1)
        return fail(RIO_GP_ERANGE, "address of " + std::to_string(v.size()) + " bytes does not fit the output buffer");
    memcpy(out, v.data(), v.size());
    out[v.size()] = 0;
    return RIO_GP_OK;
}

// the whole policy for a batch of (row, requester) pairs; rows/reqs are dense ids (mu held, device tables in sync)
int policy_batch(State* s, std::vector<uint32_t>& rows, std::vector<uint32_t>& reqs, uint32_t* out_node,
                 uint32_t* out_flag, bool tables_locked = true) {
    const uint64_t n = rows.size();
    bool any_malformed;
    {
        std::shared_lock<TableLock> li(s->imu, std::defer_lock);
        if (!tables_locked) li.lock();
        any_malformed = s->n_malformed != 0;
    }
    if (any_malformed) {
        // service.rs:213-223: a record whose address has no ip or no port is removed (only that record)
        std::vector<uint32_t> cur(n), bad;
        int rc = rio_gp_lookup_batch(s->gp, n, rows.data(), cur.data());
        if (rc) return gp_fail(s, rc);
        {
            std::shared_lock<TableLock> li(s->imu, std::defer_lock);
            if (!tables_locked) li.lock();
            for (uint64_t k = 0; k < n; ++k)
                if (cur[k] != RIO_GP_NONE && s->node_malformed[cur[k]]) bad.push_back(rows[k]);
        }
        if (!bad.empty() && (rc = rio_gp_remove_batch(s->gp, bad.size(), bad.data()))) return gp_fail(s, rc);
    }
    int rc = rio_gp_place_pending(s->gp, n, rows.data(), reqs.data(), out_node, out_flag);
    if (rc) return gp_fail(s, rc);
    // the shadow follows: a request that found its object on a dead node had that node cleaned (every object of it: rows this
    // batch does not name), so everything older than this batch is dropped first; then every requested row is where the
    // device just said it is
    bool cleaned = false;
    for (uint64_t k = 0; k < n && !cleaned && out_flag; ++k) cleaned = (out_flag[k] & RIO_GP_FLAG_REPLACED) != 0;
    if (cleaned || !out_flag) s->shadow.invalidate_all();
    // (a batch that cleaned a server: the device cleans first and places then — a first touch onto a requester that is not an
    //  active member survives there, where the reference's request order might wipe it again — so such answers are not cached:
    //  the next call about that row asks the device)
    std::shared_lock<TableLock> li(s->imu, std::defer_lock);
    if (cleaned && !tables_locked) li.lock();
    for (uint64_t k = 0; k < n; ++k)
        if (!cleaned || out_node[k] == RIO_GP_NONE || (out_node[k] < s->node_alive.size() && s->node_alive[out_node[k]]))
            s->shadow.put(rows[k], out_node[k]);
    return RIO_GP_OK;
}

// Combining front-end for the single-object calls that need the device (a lookup the shadow cannot answer, a first touch,
// update, remove): the reference is called from one tokio task per connection (server.rs:292-304), and one device round trip
// per call (8-11 us behind a mutex) would cap a provider at ~1e5 calls/s however many tasks call it.  Flat combining, with the
// roles settled at publication: a caller interns its key, takes a TICKET of the current generation, fills the slot the ticket
// names (32 bytes, in parallel with every other caller) and tags it.  Ticket 0 serves its generation: it waits for `mu`,
// closes the generation (later tickets belong to the next one, whose ticket 0 is already waiting for the lock), reads the
// slots as an array, makes ONE device round trip (rio_gp_mixed_batch: one launch runs the kinds that were asked for one after
// the other, one wait), answers every caller with one exchange on that caller's own cache line and releases the lock.
// Everybody else waits for its answer on a line nobody else touches — spinning at first, asleep on it after that.  Tenure is exactly one batch, so a server always returns to its own
// caller (round-2 advisor finding).  A lone caller pays exactly what it paid before; N concurrent callers share a round trip.
// Requests of one batch keep their arrival (ticket) order: the first request for an object decides, as in
// rio_gp_place_pending.  What this replaced, measured at 64 callers on the 2-socket host: round 4's queue + condition variable
// (1.1e5 lookups/s: every waiter fought for the queue's mutex), then a lock-free list with every waiter trying the device lock
// (the lock lay free for 33 us per batch, or was stormed), a linked list through the callers' stack frames (a dependent cache
// miss per request: 25 us per batch) and answers spread over four fields of a line the caller polls (40 us per batch).  Tried on
// top and dropped: the answers as ONE array + ONE "generation answered" word every caller polls, instead of a store into each
// caller's own line — no faster at 16 / 64 callers and 7x slower at 256 (every hardware thread polling one line).

// one batched device call for the requests `who` of one kind; t_err holds the text when it fails
int run_kind(State* s, int kind, std::vector<uint32_t>& rows, std::vector<uint32_t>& reqs, uint32_t* res, uint32_t* fl) {
    int rc;
    const size_t n = rows.size();
    if (kind == 0) {
        if ((rc = rio_gp_lookup_batch(s->gp, n, rows.data(), res))) gp_fail(s, rc);
        else for (size_t k = 0; k < n; ++k) s->shadow.put(rows[k], res[k]);
    } else if (kind == 1) {
        rc = policy_batch(s, rows, reqs, res, fl, false);
    } else if (kind == 2) {
        if ((rc = rio_gp_update_batch(s->gp, n, rows.data(), reqs.data()))) gp_fail(s, rc);
        else for (size_t k = 0; k < n; ++k) s->shadow.put(rows[k], reqs[k]);  // (in order: the last writer of a row wins here too)
    } else {
        if ((rc = rio_gp_remove_batch(s->gp, n, rows.data()))) gp_fail(s, rc);
        else for (size_t k = 0; k < n; ++k) s->shadow.put(rows[k], RIO_GP_NONE);
    }
    return rc;
}

// results[i] = the packed answer of batch[i] (Req::pack); error texts go into the requests themselves
void serve(State* s, std::vector<Req*>& batch, std::vector<uint64_t>& results) {  // mu held (NOT imu: callers keep interning and
                                                                                  // publishing during the round trip)
    results.assign(batch.size(), 0);
    // every id in this batch was interned before its request was published: whatever the device does not know yet of the
    // node table or the row count goes there now, ahead of the requests (the serving thread may not be the one that
    // interned the new address)
    const int src = sync_device(s, false);
    if (src) {
        for (size_t i = 0; i < batch.size(); ++i) { batch[i]->err = t_err; results[i] = Req::pack(src, RIO_GP_NONE, 0); }
        return;
    }
    ++s->dev_batches;
    s->dev_requests += batch.size();
    // (the requests' inputs were copied out of the slots by the caller: sv_kind / sv_row / sv_req)
    std::vector<int>& kinds = s->sv_kind;
    std::vector<uint32_t>&arow = s->sv_row, &areq = s->sv_req;
    State::KindBuf* kb = s->sv_kb;
    int present = 0;
    bool micro = true;
    for (int kind = 0; kind < 4; ++kind) { kb[kind].rows.clear(); kb[kind].reqs.clear(); kb[kind].who.clear(); }
    for (size_t i = 0; i < batch.size(); ++i) {
        State::KindBuf& b = kb[kinds[i]];
        b.rows.push_back(arow[i]); b.reqs.push_back(areq[i]); b.who.push_back((uint32_t)i);
    }
    for (int kind = 0; kind < 4; ++kind) {
        kb[kind].res.assign(kb[kind].who.size(), RIO_GP_NONE);
        kb[kind].fl.assign(kb[kind].who.size(), 0);
        present += !kb[kind].who.empty();
        micro = micro && kb[kind].who.size() <= 256;
    }
    auto answer = [&](int kind, int rc) {
        const State::KindBuf& b = kb[kind];
        for (size_t k = 0; k < b.who.size(); ++k) {
            if (rc) batch[b.who[k]]->err = t_err;
            results[b.who[k]] = Req::pack(rc, b.res[k], b.fl[k]);
        }
    };
    bool done[4] = {false, false, false, false};
    // writes first, in arrival order (sequential last-writer-wins, local.rs:22-40), then the reads and the policy calls:
    // a caller only returns after the batch, so any order inside it is a valid linearisation of concurrent calls
    static const int kOrder[4] = {2, 3, 0, 1};
    if (present >= 2 && micro) {
        // The callers of this generation asked for different things (a server's connections mix lookups, first touches and
        // removals): ONE device round trip for all of it — rio_gp_mixed_batch runs the four kinds in exactly this order in
        // one launch — instead of one per kind.
        bool any_malformed;
        {
            std::shared_lock<TableLock> li(s->imu);
            any_malformed = s->n_malformed != 0;  // (rare: policy_batch's own pre-pass handles those records)
        }
        if (!any_malformed) {
            rio_gp_mixed m;
            memset(&m, 0, sizeof m);
            m.struct_size = (uint32_t)sizeof m;
            m.n_update = (uint32_t)kb[2].who.size(); m.update_idx = kb[2].rows.data(); m.update_node = kb[2].reqs.data();
            m.n_remove = (uint32_t)kb[3].who.size(); m.remove_idx = kb[3].rows.data();
            m.n_lookup = (uint32_t)kb[0].who.size(); m.lookup_idx = kb[0].rows.data(); m.lookup_out = kb[0].res.data();
            m.n_place = (uint32_t)kb[1].who.size(); m.place_idx = kb[1].rows.data(); m.place_requester = kb[1].reqs.data();
            m.place_node = kb[1].res.data(); m.place_flag = kb[1].fl.data();
            if (rio_gp_mixed_batch(s->gp, &m) == RIO_GP_OK) {
                static const int kRcOf[4] = {2, 3, 0, 1};  // kind -> index into rio_gp_mixed.rc (update, remove, lookup, place)
                for (int kind : kOrder) {  // the shadow follows in the order the device applied them
                    const State::KindBuf& b = kb[kind];
                    if (b.who.empty() || m.rc[kRcOf[kind]] != RIO_GP_OK) continue;  // a refused kind changed nothing: one by one below
                    bool cleaned = false;
                    if (kind == 1) {
                        for (size_t k = 0; k < b.who.size() && !cleaned; ++k) cleaned = (b.fl[k] & RIO_GP_FLAG_REPLACED) != 0;
                        if (cleaned) s->shadow.invalidate_all();
                    }
                    std::shared_lock<TableLock> lk(s->imu, std::defer_lock);
                    if (cleaned) lk.lock();  // (policy_batch's rule: after a clean, answers on servers that are not active are not cached)
                    for (size_t k = 0; k < b.who.size(); ++k) {
                        const uint32_t v = kind == 2 ? b.reqs[k] : kind == 3 ? RIO_GP_NONE : b.res[k];
                        if (!cleaned || v == RIO_GP_NONE || (v < s->node_alive.size() && s->node_alive[v])) s->shadow.put(b.rows[k], v);
                    }
                    answer(kind, RIO_GP_OK);
                    done[kind] = true;
                }
            }
        }
    }
    for (int kind : kOrder) {
        State::KindBuf& b = kb[kind];
        if (b.who.empty() || done[kind]) continue;
        int rc = run_kind(s, kind, b.rows, b.reqs, b.res.data(), b.fl.data());
        if (rc == RIO_GP_OK || b.who.size() == 1) {
            answer(kind, rc);
            continue;
        }
        // The batched call was refused (the dense layer validates before it mutates): run the requests one by one, in
        // order, so that only the offender sees the error — its batch-mates are other callers' requests.
        std::vector<uint32_t> r1(1), q1(1);
        for (size_t k = 0; k < b.who.size(); ++k) {
            r1[0] = b.rows[k]; q1[0] = b.reqs[k];
            uint32_t nd = RIO_GP_NONE, f = 0;
            rc = run_kind(s, kind, r1, q1, &nd, &f);
            if (rc) batch[b.who[k]]->err = t_err;
            results[b.who[k]] = Req::pack(rc, nd, f);
        }
    }
}

// how long a waiter has been at it, in nanoseconds (steady clock: a pause is 10-40 ns depending on the core, so iteration
// counts say nothing about time)
static inline long long waited_ns(const std::chrono::steady_clock::time_point t0) {
    return (long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
}
// A device round trip is 8-15 us, and a caller waits for one to three of them: spin (a futex sleep + wake costs more than the
// wait); give the core away when it takes longer than `spin_ns` (more callers than cores; a compound call holds the device),
// sleep in earnest when it takes much longer (a snapshot, a reclaim, a big batched call).
static inline void wait_step(unsigned spin, const std::chrono::steady_clock::time_point t0, long long spin_ns) {
    if (spin < 64) { cpu_relax(); return; }
    for (int q = 0; q < 4; ++q) cpu_relax();
    if ((spin & 63u) != 0) return;
    const long long ns = waited_ns(t0);
    if (ns > 20 * spin_ns) { const timespec ts{0, 50000}; nanosleep(&ts, nullptr); }
    else if (ns > spin_ns) sched_yield();
}

static inline void futex_wait32(uint32_t* addr, uint32_t expect, long timeout_ns) {
    const timespec ts{0, timeout_ns};
    (void)syscall(SYS_futex, addr, FUTEX_WAIT_PRIVATE, expect, &ts, nullptr, 0);
}
static inline void futex_wake32(uint32_t* addr) { (void)syscall(SYS_futex, addr, FUTEX_WAKE_PRIVATE, 1, nullptr, nullptr, 0); }

// CPUs the process may keep busy: the affinity mask, cut by a cgroup CPU quota (v2 cpu.max, v1 cfs_quota_us / cfs_period_us)
static uint32_t usable_cpus() {
    long n = sysconf(_SC_NPROCESSORS_ONLN);
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0 && CPU_COUNT(&set) > 0) n = CPU_COUNT(&set);
    if (n < 1) n = 1;
    long long quota = -1, period = 0;
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = {0};
        if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atoll(q);
        fclose(f);
    } else {
        FILE* fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r");
        FILE* fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r");
        if (fq && fp && (fscanf(fq, "%lld", &quota) != 1 || fscanf(fp, "%lld", &period) != 1)) quota = -1;
        if (fq) fclose(fq);
        if (fp) fclose(fp);
    }
    if (quota > 0 && period > 0) n = std::min<long>(n, std::max<long>(1, (long)((quota + period - 1) / period)));
    return (uint32_t)n;
}

int run_combined(State* s, Req* mine) {
    // publish: a ticket of the current generation, then the slot it names
    uint64_t gen;
    uint32_t idx;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spin = 0;; ++spin) {
        const uint64_t t = s->ticket.fetch_add(1, std::memory_order_acq_rel);
        gen = t >> 32;
        idx = (uint32_t)t;
        if (idx < kSlots) break;
        // the generation is full (more callers than slots): wait until its server closes it, then take a ticket of the next one
        while ((s->ticket.load(std::memory_order_acquire) >> 32) == gen) wait_step(spin++, t0, 300000);
    }
    Slot& mys = s->slots[gen & 1][idx];
    mys.row = mine->row;
    mys.req = mine->req;
    mys.r = mine;
    mys.tag.store(((gen + 1) << 8) | (uint64_t)mine->kind, std::memory_order_release);
    if (idx != 0) {
        // Somebody took ticket 0 of this generation: THAT caller serves it, our request included.  We only wait for our result,
        // on a cache line nobody else touches: no lock word, no shared flag (64 waiters trying the lock left it free for 33 us per
        // batch — everyone was asleep or yielding when it was released — and stormed it when it was not).
        // Spin for about as long as the answer usually takes, then sleep on the word itself (a futex; the server wakes exactly
        // the callers that said they sleep).  How long "usually" is depends on how many CPUs the callers may burn: 64 callers
        // spinning inside a 16-CPU quota are throttled as a group — the server with them (measured on the GPU box: 102 of 109
        // scheduler periods throttled, 4.7e5 calls/s) — so the servers shorten the spin when a batch carries more callers than
        // there are CPUs (spin_ns).
        uint64_t w;
        const long long budget = s->spin_ns.load(std::memory_order_relaxed);
        for (unsigned spin = 1;; ++spin) {
            if ((w = mine->result.load(std::memory_order_acquire)) & Req::kDone) break;
            cpu_relax();
            if ((spin & 15u) != 0 || waited_ns(t0) < budget) continue;
            w = mine->result.fetch_or(Req::kSleep, std::memory_order_acq_rel);
            if (w & Req::kDone) break;
            // (bounded: a wake-up that got lost would cost a millisecond, not the call)
            while (!((w = mine->result.load(std::memory_order_acquire)) & Req::kDone))
                futex_wait32(mine->futex_word(), (uint32_t)(Req::kSleep >> 32), 1000000);
            break;
        }
        mine->unpack(w);
        return mine->rc;
    }
    // Ticket 0: the server of everything published in this generation, from now until we close it.  (One spinning thread per
    // generation: it may spin long — the lock is handed over within a device round trip unless a compound call holds it.)
    for (unsigned spin = 0;; ++spin) {
        if (!s->busy.load(std::memory_order_relaxed) && s->mu.try_lock()) break;
        wait_step(spin, t0, 5000000);
    }
    s->busy.store(1, std::memory_order_relaxed);
    if (s->collect_ns > 1 && s->last_batch + s->prev_batch > 1) {
        // Other callers are active: the ones the last batch served are on their way back with their next request.  Closed-loop
        // callers otherwise alternate between two cohorts, each batch carrying half of them and every call waiting two round
        // trips; the server waits — at most collect_ns — until about as many callers have published as the last two batches
        // carried together: "half, then the other half" becomes "everyone" per round trip (16 callers: 2 023 batches for 32 000
        // requests instead of 3 900, 7.1e5 against 5.2e5 calls/s, measured).
        const uint32_t want = (uint32_t)(s->last_batch + s->prev_batch) - 1u;
        const auto c0 = std::chrono::steady_clock::now();
        // (wait_step: a window that outlasts its bound by much — the quota throttled the process — yields instead of burning on)
        for (unsigned spin = 0; (uint32_t)s->ticket.load(std::memory_order_relaxed) < want &&
                                std::chrono::steady_clock::now() - c0 < std::chrono::nanoseconds(s->collect_ns); ++spin)
            wait_step(spin, c0, (long long)s->collect_ns);
    }
    // close the generation: whoever takes a ticket from now on belongs to the next one (and its ticket 0 waits for this lock)
    const uint64_t closed = s->ticket.exchange((gen + 1) << 32, std::memory_order_acq_rel);
    const uint32_t n = (uint32_t)closed < kSlots ? (uint32_t)closed : kSlots;
    std::vector<Req*>& batch = s->batch;
    batch.resize(n);
    s->sv_kind.resize(n); s->sv_row.resize(n); s->sv_req.resize(n);
    Slot* sl = s->slots[gen & 1];
    for (uint32_t i = 0; i < n; ++i) {  // arrival (ticket) order; a caller between its ticket and its tag is waited for
        uint64_t tag;
        // (a publisher preempted between its ticket and its tag — 64-256 callers inside a 16-CPU quota — must get a CPU to finish:
        //  pause, then yield, then sleep, instead of burning the quantum it is waiting for)
        const auto w0 = std::chrono::steady_clock::now();
        for (unsigned spin = 0; ((tag = sl[i].tag.load(std::memory_order_acquire)) >> 8) != gen + 1; ++spin) wait_step(spin, w0, 20000);
        s->sv_kind[i] = (int)(tag & 0xFFu);
        s->sv_row[i] = sl[i].row;
        s->sv_req[i] = sl[i].req;
        batch[i] = sl[i].r;
    }
    s->prev_batch = s->last_batch;
    s->last_batch = n;
    serve(s, batch, s->results);
    uint32_t* asleep[kSlots];
    uint32_t n_asleep = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (batch[i] == mine) { mine->unpack(s->results[i]); continue; }
        uint32_t* const fw = batch[i]->futex_word();
        // last touch of that request: it lives on its caller's stack
        if (batch[i]->result.exchange(s->results[i], std::memory_order_acq_rel) & Req::kSleep) asleep[n_asleep++] = fw;
    }
    // the next batch's callers spin about two of this batch's round trips when there is a CPU for each of them, less when not
    {
        const uint32_t callers = std::max<uint32_t>(1u, std::max<uint32_t>(n, (uint32_t)s->prev_batch));
        const uint64_t ns = 30000ull * s->cpus / callers;
        s->spin_ns.store((uint32_t)std::min<uint64_t>(30000, std::max<uint64_t>(2000, ns)), std::memory_order_relaxed);
    }
    s->busy.store(0, std::memory_order_release);
    s->mu.unlock();
    // wake the sleepers after the lock is gone: the next server is already at work (the word may belong to a later call of the
    // same thread by now — a spurious wake-up, which every sleeper tolerates)
    for (uint32_t i = 0; i < n_asleep; ++i) futex_wake32(asleep[i]);
    return mine->rc;
}

// A single-object call: intern under imu — shared first: a key and an address that are already known change nothing, and
// such a call may be answered from the host shadow right there (kHit); exclusively when something has to be created —
// (held off while keys are being reclaimed), count as in flight while its row id is on its way to the device (reclaim()
// waits for that count to drain before it forgets any key).
// `intern(excl)` fills the request and returns RIO_GP_OK, kFull, an error, kNoop = "nothing to do" (e.g. lookup of an unknown
// key), kHit = answered, or (excl == false only) kUpgrade.
// `done(rc)` runs after the round trip and BEFORE the call stops counting as in flight: what still needs the node id the device
// answered with (its address) happens there — rio_op_remove_members renumbers the ids only once nothing is in flight.
struct NoDone { int operator()(int rc) const { return rc; } };
template <typename F, typename D = NoDone>
int single_call(State* s, Req* r, F intern, D done = D()) {
    for (int attempt = 0;; ++attempt) {
        int rc;
        {
            std::shared_lock<TableLock> li(s->imu);
            while (s->reclaiming) s->rcv.wait(li);
            rc = intern(false);
            if (rc == RIO_GP_OK) s->inflight.fetch_add(1, std::memory_order_acq_rel);
        }
        if (rc == kUpgrade) {
            std::unique_lock<TableLock> li(s->imu);
            while (s->reclaiming) s->rcv.wait(li);
            rc = intern(true);
            if (rc == RIO_GP_OK) s->inflight.fetch_add(1, std::memory_order_acq_rel);
        }
        if (rc == kFull && attempt == 0) {
            if ((rc = reclaim(s))) return rc;
            continue;
        }
        if (rc == kFull) return fail(RIO_GP_EINVAL, "object table full (max_objects live objects)");
        if (rc != RIO_GP_OK) return rc;
        rc = run_combined(s, r);
        if (rc) t_err = r->err;
        rc = done(rc);
        s->inflight.fetch_sub(1, std::memory_order_acq_rel);
        return rc;
    }
}

// compound (mu + imu for the whole call) operations: run `body`, reclaim and retry once when the table is full
template <typename F>
int compound_call(State* s, F body) {
    for (int attempt = 0;; ++attempt) {
        int rc;
        {
            DevLock g(s);
            std::lock_guard<TableLock> gi(s->imu);
            rc = body();
        }
        if (rc == kFull && attempt == 0) {
            if ((rc = reclaim(s))) return rc;
            continue;
        }
        if (rc == kFull) return fail(RIO_GP_EINVAL, "object table full (max_objects live objects)");
        return rc;
    }
}

}  // namespace

struct rio_op {
    State* s;
};

extern "C" {

int rio_op_create(const rio_op_cfg* cfg, rio_op_t** out) {
    if (out) *out = nullptr;
    if (!cfg || !out || cfg->struct_size != sizeof(rio_op_cfg) || cfg->max_objects == 0 || cfg->max_nodes == 0)
        return fail(RIO_GP_EINVAL, "rio_op_create: bad cfg");
    if (cfg->collect_ns > RIO_OP_MAX_COLLECT_NS)  // (the field was `reserved` in ABI version 1: a client that never set it)
        return fail(RIO_GP_EINVAL, "rio_op_create: collect_ns above RIO_OP_MAX_COLLECT_NS (1 ms)");
    rio_gp_cfg g;
    memset(&g, 0, sizeof g);
    g.struct_size = sizeof g;
    g.device = cfg->device;
    g.max_objects = cfg->max_objects;
    g.max_nodes = cfg->max_nodes;
    g.spill_rounds = cfg->spill_rounds;
    // reference-faithful unless the caller opts out: get_or_create_placement first-touches the requester whatever membership
    // says about it (service.rs:244-252)
    g.flags = RIO_GP_CFG_ROW_LIFECYCLE | ((cfg->flags & RIO_OP_CFG_LIVE_FIRST_TOUCH) ? 0u : RIO_GP_CFG_REF_SELF_ASSIGN);
    rio_gp_t* gp = nullptr;
    int rc = rio_gp_create(&g, &gp);
    if (rc) {
        const char* e = rio_gp_last_error(nullptr);
        return fail(rc, e ? e : "");
    }
    // every potential row is initialised (unplaced, load 1, not an object); none takes part until it is handed out
    if ((rc = rio_gp_set_objects(gp, cfg->max_objects, nullptr, nullptr)) || (rc = rio_gp_set_num_objects(gp, 0)) ||
        (rc = rio_gp_set_nodes(gp, 0, nullptr, nullptr))) {
        const char* e = rio_gp_last_error(gp);
        t_err = e ? e : "";
        rio_gp_destroy(gp);
        return rc;
    }
    State* s = new State();
    s->gp = gp;
    s->max_objects = cfg->max_objects;
    s->max_nodes = cfg->max_nodes;
    s->pushed_version = s->node_version.load();  // the empty node table is on the device
    s->pushed_shape = s->shape_version.load();
    s->shadow.init(cfg->max_objects, cfg->max_nodes, (cfg->flags & RIO_OP_CFG_NO_HOST_SHADOW) == 0);
    s->seen.init(cfg->max_objects);
    s->collect_ns = cfg->collect_ns ? cfg->collect_ns : RIO_OP_DEFAULT_COLLECT_NS;
    s->cpus = usable_cpus();
    s->self_assign = (cfg->flags & RIO_OP_CFG_LIVE_FIRST_TOUCH) == 0;
    *out = new rio_op{s};
    return RIO_GP_OK;
}

rio_op_t* rio_op_clone(rio_op_t* p) {
    if (!p) return nullptr;
    p->s->refs.fetch_add(1);
    return new rio_op{p->s};
}

void rio_op_release(rio_op_t* p) {
    if (!p) return;
    State* s = p->s;
    delete p;
    if (s->refs.fetch_sub(1) == 1) {
        rio_gp_destroy(s->gp);
        delete s;
    }
}

int rio_op_prepare(rio_op_t* p) { return p ? RIO_GP_OK : RIO_GP_EINVAL; }

const char* rio_op_last_error(rio_op_t*) { return t_err.c_str(); }

rio_gp_t* rio_op_dense(rio_op_t* p) { return p ? p->s->gp : nullptr; }

const char* rio_op_node_address(rio_op_t* p, uint32_t node_id) {
    if (!p) return nullptr;
    std::shared_lock<TableLock> gi(p->s->imu);
    // the strings are never modified, moved or freed (NodeAddrs): the pointer stays valid for the life of the provider
    return node_id < p->s->node_addr.size() ? p->s->node_addr[node_id].c_str() : nullptr;
}

static int op_update_batch(rio_op_t* p, uint64_t n, const Keys& ks, const char* const* addrs) {
    if (!p || (n && (!ks.tys || !ks.ids || !addrs))) return RIO_GP_EINVAL;
    State* s = p->s;
    return compound_call(s, [&]() -> int {
        std::vector<uint32_t> rows, nodes;
        rows.reserve(n);
        nodes.reserve(n);
        for (uint64_t k = 0; k < n; ++k) {
            uint32_t row = RIO_GP_NONE, node = RIO_GP_NONE;
            int rc;
            if (addrs[k]) {  // Some(address): entry(key) = address
                if ((rc = intern_row(s, ks.ty(k), ks.id(k), true, &row, true))) return rc;
                if ((rc = intern_node(s, addrs[k], true, &node))) return rc;
            } else {         // None: remove(key) (local.rs:36-37) — an unknown key stays unknown
                if ((rc = intern_row(s, ks.ty(k), ks.id(k), false, &row, true))) return rc;
                if (row == RIO_GP_NONE) continue;
            }
            rows.push_back(row);
            nodes.push_back(node);
        }
        int rc;
        if ((rc = sync_device(s, true))) return rc;
        if (rows.empty()) return RIO_GP_OK;
        rc = rio_gp_update_batch(s->gp, rows.size(), rows.data(), nodes.data());
        if (rc) return gp_fail(s, rc);
        for (size_t k = 0; k < rows.size(); ++k) {  // (in order: the last writer of a row wins)
            s->shadow.put(rows[k], nodes[k]);
            if (nodes[k] != RIO_GP_NONE) s->seen.stamp(rows[k]);
        }
        return RIO_GP_OK;
    });
}

int rio_op_update_batch(rio_op_t* p, uint64_t n, const char* const* tys, const char* const* ids, const char* const* addrs) {
    return op_update_batch(p, n, Keys{tys, nullptr, ids, nullptr}, addrs);
}
int rio_op_update_batch_n(rio_op_t* p, uint64_t n, const char* const* tys, const size_t* tyl, const char* const* ids, const size_t* idl,
                          const char* const* addrs) {
    if (n && (!tyl || !idl)) return RIO_GP_EINVAL;
    return op_update_batch(p, n, Keys{tys, tyl, ids, idl}, addrs);
}

static int op_update(rio_op_t* p, const Part& ty, const Part& id, const char* addr) {
    if (!p) return RIO_GP_EINVAL;
    State* s = p->s;
    Req r;
    r.kind = 2;
    r.req = RIO_GP_NONE;
    const int rc = single_call(s, &r, [&](bool excl) -> int {
        int rc;
        if (addr) {  // Some(address): entry(key) = address
            if ((rc = intern_row(s, ty, id, true, &r.row, true, excl))) return rc;
            return intern_node(s, addr, true, &r.req, false, excl);
        }
        // None: remove(key) (local.rs:36-37) — an unknown key stays unknown
        if ((rc = intern_row(s, ty, id, false, &r.row, true, excl))) return rc;
        return r.row == RIO_GP_NONE ? kNoop : RIO_GP_OK;
    }, [&](int rc) -> int {  // (still in flight: the row is this key's)
        if (!rc && addr) s->seen.stamp(r.row);
        return rc;
    });
    return rc == kNoop ? RIO_GP_OK : rc;
}

static int op_lookup_batch(rio_op_t* p, uint64_t n, const Keys& ks, uint32_t* out) {
    if (!p || (n && (!ks.tys || !ks.ids || !out))) return RIO_GP_EINVAL;
    State* s = p->s;
    DevLock g(s);
    std::shared_lock<TableLock> gi(s->imu);
    std::vector<uint32_t> rows, where;
    for (uint64_t k = 0; k < n; ++k) {
        uint32_t row;
        int rc = intern_row(s, ks.ty(k), ks.id(k), false, &row);
        if (rc) return rc;
        out[k] = RIO_GP_NONE;  // unknown key: Ok(None)
        if (row != RIO_GP_NONE) {
            rows.push_back(row);
            where.push_back((uint32_t)k);
        }
    }
    if (rows.empty()) return RIO_GP_OK;
    int rc;
    if ((rc = sync_device(s, true))) return rc;
    std::vector<uint32_t> res(rows.size());
    rc = rio_gp_lookup_batch(s->gp, rows.size(), rows.data(), res.data());
    if (rc) return gp_fail(s, rc);
    for (size_t q = 0; q < rows.size(); ++q) {
        out[where[q]] = res[q];
        s->shadow.put(rows[q], res[q]);
        if (res[q] != RIO_GP_NONE) s->seen.stamp(rows[q]);
    }
    return RIO_GP_OK;
}

int rio_op_lookup_batch(rio_op_t* p, uint64_t n, const char* const* tys, const char* const* ids, uint32_t* out) {
    return op_lookup_batch(p, n, Keys{tys, nullptr, ids, nullptr}, out);
}
int rio_op_lookup_batch_n(rio_op_t* p, uint64_t n, const char* const* tys, const size_t* tyl, const char* const* ids, const size_t* idl,
                          uint32_t* out) {
    if (n && (!tyl || !idl)) return RIO_GP_EINVAL;
    return op_lookup_batch(p, n, Keys{tys, tyl, ids, idl}, out);
}

int rio_op_update(rio_op_t* p, const char* ty, const char* id, const char* addr) { return op_update(p, Part(ty), Part(id), addr); }
int rio_op_update_n(rio_op_t* p, const char* ty, size_t ty_len, const char* id, size_t id_len, const char* addr) {
    return op_update(p, Part(ty, ty_len), Part(id, id_len), addr);
}

static int op_lookup(rio_op_t* p, const Part& ty, const Part& id, char* out, size_t cap, int* found) {
    if (!p || !found) return RIO_GP_EINVAL;
    State* s = p->s;
    Req r;
    r.kind = 0;
    r.req = RIO_GP_NONE;
    *found = 0;
    t_addr_len = 0;
    int hit_rc = RIO_GP_OK;
    const int rc = single_call(s, &r, [&](bool) -> int {
        const int rc = intern_row(s, ty, id, false, &r.row);
        if (rc) return rc;
        if (r.row == RIO_GP_NONE) return kNoop;  // unknown key: Ok(None), no device work
        // what the device last said about this row, if nothing has happened since that could have moved it: the answer
        // (local.rs:42-49 is a hash-map read; so is this).  The address is copied out here, under the table lock.
        if (s->shadow.get(r.row, &r.node)) {
            *found = r.node != RIO_GP_NONE;
            if (*found && !(hit_rc = copy_out(s->node_addr[r.node], out, cap))) s->seen.stamp(r.row);
            return kHit;
        }
        return RIO_GP_OK;
    }, [&](int rc) -> int {  // (still in flight: the node id is the one the address table knows)
        if (rc) return rc;
        *found = r.node != RIO_GP_NONE;
        t_addr_len = 0;
        if (*found) {
            std::shared_lock<TableLock> gi(s->imu);
            const int crc = copy_out(s->node_addr[r.node], out, cap);  // RIO_GP_ERANGE: *found is set, nothing was copied
            if (!crc) s->seen.stamp(r.row);
            return crc;
        }
        return RIO_GP_OK;
    });
    if (rc == kNoop) return RIO_GP_OK;
    if (rc == kHit) return hit_rc;
    return rc;
}

int rio_op_lookup(rio_op_t* p, const char* ty, const char* id, char* out, size_t cap, int* found) {
    return op_lookup(p, Part(ty), Part(id), out, cap, found);
}
int rio_op_lookup_n(rio_op_t* p, const char* ty, size_t ty_len, const char* id, size_t id_len, char* out, size_t cap, int* found) {
    return op_lookup(p, Part(ty, ty_len), Part(id, id_len), out, cap, found);
}

size_t rio_op_last_address_len(rio_op_t*) { return t_addr_len; }

// rio_op_try_*: the host shadow or RIO_GP_EAGAIN.  Nothing here takes State::mu, waits for the table lock (a batched call holds
// it exclusively across its device calls), interns a key or an address, or counts as in flight: a pure read of the interning
// tables and one shadow word, under the shared side of the table lock when it is free right now.
namespace {
struct TrySharedLock {
    TableLock& l;
    bool held;
    explicit TrySharedLock(TableLock& l_) : l(l_), held(l_.try_lock_shared()) {}
    ~TrySharedLock() { if (held) l.unlock_shared(); }
};
}  // namespace

int rio_op_try_lookup_n(rio_op_t* p, const char* ty, size_t ty_len, const char* id, size_t id_len, char* out, size_t cap, int* found) {
    if (!p || !found || (!ty && ty_len) || (!id && id_len)) return RIO_GP_EINVAL;
    State* s = p->s;
    *found = 0;
    t_addr_len = 0;
    TrySharedLock li(s->imu);
    if (!li.held || s->reclaiming) return RIO_GP_EAGAIN;
    const auto it = s->rows.find(key_of(Part(ty, ty_len), Part(id, id_len)));
    if (it == s->rows.end()) return RIO_GP_OK;  // a key nobody has interned: Ok(None), as rio_op_lookup says without the device
    uint32_t node;
    if (!s->shadow.get(it->second, &node)) return RIO_GP_EAGAIN;
    *found = node != RIO_GP_NONE;
    if (!*found) return RIO_GP_OK;
    const int rc = copy_out(s->node_addr[node], out, cap);
    if (!rc) s->seen.stamp(it->second);
    return rc;
}

int rio_op_try_get_or_create_placement_n(rio_op_t* p, const char* ty, size_t ty_len, const char* id, size_t id_len,
                                         const char* self_address, char* out, size_t cap, uint32_t* flag) {
    if (!p || !self_address || (!ty && ty_len) || (!id && id_len)) return RIO_GP_EINVAL;
    State* s = p->s;
    t_addr_len = 0;
    TrySharedLock li(s->imu);
    if (!li.held || s->reclaiming) return RIO_GP_EAGAIN;
    const auto it = s->rows.find(key_of(Part(ty, ty_len), Part(id, id_len)));
    if (it == s->rows.end() || s->row_keep[it->second]) return RIO_GP_EAGAIN;  // a first touch: the device's
    const auto rq = s->nodes.find(self_address);
    if (rq == s->nodes.end()) return RIO_GP_EAGAIN;                             // a requester nobody has seen: interned by the call
    // the sticky path of service.rs:199-242, exactly as op_get_or_create answers it from the shadow
    uint32_t nd;
    if (!s->shadow.get(it->second, &nd) || nd == RIO_GP_NONE || nd >= s->node_alive.size() || !s->node_alive[nd] || s->node_malformed[nd])
        return RIO_GP_EAGAIN;
    if (flag) *flag = nd == rq->second ? RIO_GP_FLAG_LOCAL : RIO_GP_FLAG_REDIRECT;
    const int rc = copy_out(s->node_addr[nd], out, cap);
    if (!rc) s->seen.stamp(it->second);
    return rc;
}

int rio_op_clean_server(rio_op_t* p, const char* address) {
    if (!p || !address) return RIO_GP_EINVAL;
    State* s = p->s;
    DevLock g(s);
    std::shared_lock<TableLock> gi(s->imu);
    uint32_t node;
    int rc = intern_node(s, address, false, &node);
    if (rc) return rc;
    if (node == RIO_GP_NONE) return RIO_GP_OK;  // nothing was ever placed there: retain() removes nothing
    if ((rc = sync_device(s, true))) return rc;
    rc = rio_gp_clean_server(s->gp, node, nullptr);
    if (rc) return gp_fail(s, rc);
    s->shadow.clean(node);  // whatever the shadow held for rows of that node is void; every other row's entry stands
    return RIO_GP_OK;
}

static int op_remove(rio_op_t* p, const Part& ty, const Part& id) {
    if (!p) return RIO_GP_EINVAL;
    State* s = p->s;
    Req r;
    r.kind = 3;
    r.req = RIO_GP_NONE;
    const int rc = single_call(s, &r, [&](bool excl) -> int {
        const int rc = intern_row(s, ty, id, false, &r.row, true, excl);
        if (rc) return rc;
        return r.row == RIO_GP_NONE ? kNoop : RIO_GP_OK;  // absent: no-op (local.rs:60-68)
    });
    return rc == kNoop ? RIO_GP_OK : rc;
}

int rio_op_remove(rio_op_t* p, const char* ty, const char* id) { return op_remove(p, Part(ty), Part(id)); }
int rio_op_remove_n(rio_op_t* p, const char* ty, size_t ty_len, const char* id, size_t id_len) {
    return op_remove(p, Part(ty, ty_len), Part(id, id_len));
}

int rio_op_len(rio_op_t* p, uint64_t* out) {
    if (!p || !out) return RIO_GP_EINVAL;
    State* s = p->s;
    DevLock g(s);
    int rc;
    if ((rc = sync_device(s, false))) return rc;
    rc = rio_gp_count_placed(s->gp, out);
    return rc ? gp_fail(s, rc) : RIO_GP_OK;
}

int rio_op_set_member(rio_op_t* p, const char* address, int active, uint64_t capacity) {
    if (!p || !address) return RIO_GP_EINVAL;
    State* s = p->s;
    DevLock g(s);
    std::lock_guard<TableLock> gi(s->imu);
    uint32_t node;
    int rc = intern_node(s, address, true, &node);
    if (rc) return rc;
    s->node_alive[node] = active ? 1 : 0;
    if (s->node_cap[node] != capacity) {
        s->node_cap[node] = capacity;
        ++s->shape_version;
    }
    ++s->node_version;
    return sync_device(s, true);
}

// MembershipStorage::remove (cluster/storage/mod.rs:77), mu + the write side of the table lock held, nothing in flight
static int remove_members_locked(State* s, uint64_t n, const char* const* addresses, uint64_t* removed, uint64_t* evicted) {
    if (!rio_gp_remap_nodes) return fail(RIO_GP_EUPSTREAM, "dense layer has no node removal");
    const uint32_t m = (uint32_t)s->node_addr.size();
    std::vector<uint32_t> map(m ? m : 1, 0);
    uint32_t gone = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const auto it = s->nodes.find(addresses[k]);
        if (it == s->nodes.end() || map[it->second] == RIO_GP_NONE) continue;  // never seen, or given twice
        map[it->second] = RIO_GP_NONE;
        ++gone;
    }
    if (!gone) return RIO_GP_OK;
    // stable compaction: the surviving nodes keep their relative order
    uint32_t m_new = 0;
    for (uint32_t j = 0; j < m; ++j)
        if (map[j] != RIO_GP_NONE) map[j] = m_new++;
    // the device holds the table as it is (no rio_gp_set_nodes of the old shape may follow the renumbering), then renumbers
    int rc;
    if ((rc = sync_device(s, true))) return rc;
    uint64_t ev = 0;
    if ((rc = rio_gp_remap_nodes(s->gp, m_new, map.data(), &ev))) return gp_fail(s, rc);
    std::vector<const std::string*> by_id(m_new);
    std::vector<uint8_t> alive(m_new), bad(m_new);
    std::vector<uint64_t> cap(m_new), stamp(m_new);
    s->n_malformed = 0;
    for (uint32_t j = 0; j < m; ++j) {
        const uint32_t k = map[j];
        if (k == RIO_GP_NONE) { s->nodes.erase(s->node_addr[j]); continue; }
        s->nodes[s->node_addr[j]] = k;
        by_id[k] = s->node_addr.by_id[j];
        alive[k] = s->node_alive[j];
        bad[k] = s->node_malformed[j];
        cap[k] = s->node_cap[j];
        stamp[k] = s->shadow.clean_stamp[j].load(std::memory_order_relaxed);
        s->n_malformed += bad[k];
    }
    s->node_addr.by_id.swap(by_id);
    s->node_alive.swap(alive);
    s->node_malformed.swap(bad);
    s->node_cap.swap(cap);
    // the shadow's entries name old ids: all of them are void (as after a tick); the per-node stamps follow their nodes
    for (uint32_t k = 0; k < m; ++k) s->shadow.clean_stamp[k].store(k < m_new ? stamp[k] : 0, std::memory_order_relaxed);
    s->shadow.invalidate_all();
    // the device already holds this table
    s->pushed_version = ++s->node_version;
    s->pushed_shape = ++s->shape_version;
    s->pushed_nodes = m_new;
    if (removed) *removed = gone;
    if (evicted) *evicted = ev;
    return RIO_GP_OK;
}

int rio_op_remove_members(rio_op_t* p, uint64_t n, const char* const* addresses, uint64_t* removed, uint64_t* evicted) {
    if (!p || (n && !addresses)) return RIO_GP_EINVAL;
    for (uint64_t k = 0; k < n; ++k)
        if (!addresses[k]) return RIO_GP_EINVAL;
    if (removed) *removed = 0;
    if (evicted) *evicted = 0;
    State* s = p->s;
    // node ids live in single-object calls between their intern and their return: hold new ones off and drain those in flight,
    // as reclaim() does for row ids
    {
        std::unique_lock<TableLock> li(s->imu);
        while (s->reclaiming) s->rcv.wait(li);
        s->reclaiming = true;
    }
    while (s->inflight.load(std::memory_order_acquire) != 0) sched_yield();
    int rc;
    {
        DevLock g(s);
        std::lock_guard<TableLock> gi(s->imu);
        rc = remove_members_locked(s, n, addresses, removed, evicted);
        s->reclaiming = false;
    }
    s->rcv.notify_all();
    return rc;
}

static int op_set_object_load(rio_op_t* p, const Part& ty, const Part& id, uint32_t load) {
    if (!p) return RIO_GP_EINVAL;
    State* s = p->s;
    return compound_call(s, [&]() -> int {
        uint32_t row;
        int rc = intern_row(s, ty, id, true, &row);
        if (rc) return rc;
        if ((rc = sync_device(s, true))) return rc;
        // the load only: the key does not become an object before its first update / request
        rc = rio_gp_set_object_attrs(s->gp, 1, &row, &load, nullptr);
        return rc ? gp_fail(s, rc) : RIO_GP_OK;
    });
}

int rio_op_set_object_load(rio_op_t* p, const char* ty, const char* id, uint32_t load) { return op_set_object_load(p, Part(ty), Part(id), load); }
int rio_op_set_object_load_n(rio_op_t* p, const char* ty, size_t ty_len, const char* id, size_t id_len, uint32_t load) {
    return op_set_object_load(p, Part(ty, ty_len), Part(id, id_len), load);
}

static int op_get_or_create_batch(rio_op_t* p, uint64_t n, const Keys& ks, const char* const* selfs, uint32_t* out_node,
                                  uint32_t* out_flag) {
    if (!p || (n && (!ks.tys || !ks.ids || !selfs || !out_node))) return RIO_GP_EINVAL;
    State* s = p->s;
    return compound_call(s, [&]() -> int {
        std::vector<uint32_t> rows(n), reqs(n);
        for (uint64_t k = 0; k < n; ++k) {
            int rc;
            if ((rc = intern_row(s, ks.ty(k), ks.id(k), true, &rows[k], true))) return rc;
            if ((rc = intern_node(s, selfs[k], true, &reqs[k], true))) return rc;  // a server answering requests is up
        }
        int rc;
        if ((rc = sync_device(s, true))) return rc;
        if ((rc = policy_batch(s, rows, reqs, out_node, out_flag))) return rc;
        for (uint64_t k = 0; k < n; ++k)
            if (out_node[k] != RIO_GP_NONE) s->seen.stamp(rows[k]);
        return RIO_GP_OK;
    });
}

int rio_op_get_or_create_placement_batch(rio_op_t* p, uint64_t n, const char* const* tys, const char* const* ids,
                                         const char* const* selfs, uint32_t* out_node, uint32_t* out_flag) {
    return op_get_or_create_batch(p, n, Keys{tys, nullptr, ids, nullptr}, selfs, out_node, out_flag);
}
int rio_op_get_or_create_placement_batch_n(rio_op_t* p, uint64_t n, const char* const* tys, const size_t* tyl, const char* const* ids,
                                           const size_t* idl, const char* const* selfs, uint32_t* out_node, uint32_t* out_flag) {
    if (n && (!tyl || !idl)) return RIO_GP_EINVAL;
    return op_get_or_create_batch(p, n, Keys{tys, tyl, ids, idl}, selfs, out_node, out_flag);
}

static int op_get_or_create(rio_op_t* p, const Part& ty, const Part& id, const char* self_address, char* out, size_t cap,
                            uint32_t* flag) {
    if (!p || !self_address) return RIO_GP_EINVAL;
    State* s = p->s;
    Req r;
    r.kind = 1;
    t_addr_len = 0;
    int hit_rc = RIO_GP_OK;
    const int rc = single_call(s, &r, [&](bool excl) -> int {
        int rc;
        if ((rc = intern_row(s, ty, id, true, &r.row, true, excl))) return rc;
        if ((rc = intern_node(s, self_address, true, &r.req, true, excl))) return rc;  // a server answering requests is up
        // The sticky path of service.rs:199-242 — lookup, the server it names is an active member, return it — from the host
        // shadow: the object is where the device last put it, nothing has happened since that could have moved it, and that
        // server is up and well-formed.  Anything else (pending, on a server that is not active, malformed) is the device's.
        uint32_t nd;
        if (s->shadow.get(r.row, &nd) && nd != RIO_GP_NONE && nd < s->node_alive.size() && s->node_alive[nd] && !s->node_malformed[nd]) {
            r.node = nd;
            r.flag = nd == r.req ? RIO_GP_FLAG_LOCAL : RIO_GP_FLAG_REDIRECT;
            if (flag) *flag = r.flag;
            if (!(hit_rc = copy_out(s->node_addr[nd], out, cap))) s->seen.stamp(r.row);
            return kHit;
        }
        return RIO_GP_OK;
    }, [&](int rc) -> int {  // (still in flight: the node id is the one the address table knows)
        if (rc) return rc;
        if (flag) *flag = r.flag;
        std::shared_lock<TableLock> gi(s->imu);
        // RIO_GP_ERANGE: the decision is made and *flag is set; the address is one rio_op_lookup away (a pure read)
        const int crc = copy_out(r.node == RIO_GP_NONE ? std::string() : s->node_addr[r.node], out, cap);
        if (!crc && r.node != RIO_GP_NONE) s->seen.stamp(r.row);
        return crc;
    });
    if (rc == kHit) return hit_rc;
    return rc;
}

int rio_op_get_or_create_placement(rio_op_t* p, const char* ty, const char* id, const char* self_address, char* out,
                                   size_t cap, uint32_t* flag) {
    return op_get_or_create(p, Part(ty), Part(id), self_address, out, cap, flag);
}
int rio_op_get_or_create_placement_n(rio_op_t* p, const char* ty, size_t ty_len, const char* id, size_t id_len,
                                     const char* self_address, char* out, size_t cap, uint32_t* flag) {
    return op_get_or_create(p, Part(ty, ty_len), Part(id, id_len), self_address, out, cap, flag);
}

int rio_op_snapshot_key_lengths(rio_op_t* p, const size_t** struct_name_lens, const size_t** object_id_lens) {
    if (!p || !struct_name_lens || !object_id_lens) return RIO_GP_EINVAL;
    *struct_name_lens = t_snap.tylen.data();
    *object_id_lens = t_snap.idlen.data();
    return RIO_GP_OK;
}

int rio_op_snapshot(rio_op_t* p, uint64_t* n_out, const char* const** struct_names, const char* const** object_ids,
                    const char* const** server_addresses) {
    if (!p || !n_out || !struct_names || !object_ids || !server_addresses) return RIO_GP_EINVAL;
    State* s = p->s;
    t_snap.clear();
    {
        DevLock g(s);
        std::shared_lock<TableLock> gi(s->imu);
        int rc;
        if ((rc = sync_device(s, true))) return rc;
        const uint64_t n = s->hi_rows;
        std::vector<uint32_t> assign(n ? n : 1);
        if ((rc = rio_gp_get_assign(s->gp, n, assign.data()))) return gp_fail(s, rc);
        for (uint64_t row = 0; row < n; ++row)
            if (const char* a = addr_of(s, assign[row])) t_snap.add(s, (uint32_t)row, a);  // (RIO_GP_NONE is no node id either)
    }
    t_snap.publish(n_out, struct_names, nullptr, object_ids, nullptr, server_addresses);  // (lengths: rio_op_snapshot_key_lengths)
    return RIO_GP_OK;
}

int rio_op_objects_on_server(rio_op_t* p, const char* address, uint64_t* n_out, const char* const** struct_names,
                             const size_t** struct_name_lens, const char* const** object_ids, const size_t** object_id_lens) {
    if (!p || !address || !n_out || !struct_names || !struct_name_lens || !object_ids || !object_id_lens) return RIO_GP_EINVAL;
    State* s = p->s;
    t_on.clear();
    {
        DevLock g(s);
        std::shared_lock<TableLock> gi(s->imu);
        int rc;
        if ((rc = sync_device(s, true))) return rc;
        const auto it = s->nodes.find(address);
        if (it != s->nodes.end()) {  // (an address never seen holds nothing: 0 objects)
            if (!rio_gp_rows_on_nodes) return fail(RIO_GP_EUPSTREAM, "dense layer has no reverse index");
            const uint32_t node = it->second, m = (uint32_t)s->node_addr.size();
            std::vector<uint64_t> bitmap((m + 63) / 64 + 1, 0), off(m + 1);
            bitmap[node >> 6] |= 1ull << (node & 63);
            uint64_t n = 0;
            // the thread's buffer from its last call first (an empty one: counts only); one more round with the exact size when
            // it is too small
            std::vector<uint32_t>& rows = t_on.rows;
            rc = rio_gp_rows_on_nodes(s->gp, bitmap.data(), off.data(), rows.empty() ? nullptr : rows.data(), rows.size(), &n);
            if (rc == RIO_GP_ERANGE || (rc == RIO_GP_OK && n > rows.size())) {
                rows.resize(n);
                rc = rio_gp_rows_on_nodes(s->gp, bitmap.data(), off.data(), rows.data(), rows.size(), &n);
            }
            if (rc) return gp_fail(s, rc);
            for (uint64_t k = 0; k < n; ++k) t_on.add(s, rows[k]);
        }
    }
    t_on.publish(n_out, struct_names, struct_name_lens, object_ids, object_id_lens);
    return RIO_GP_OK;
}

// Immovable types ahead of a dense rebalance (mu + imu exclusive held, sync_device done).  With one: the class column follows the
// host's, then the table where it changed.  Without one nothing is called — except once after the last one became movable
// again, when the dense table is reset.
static int sync_classes(State* s);
static int sync_movable(State* s) {
    int rc;
    if (s->n_immovable) {
        if ((rc = sync_classes(s))) return rc;
        if (s->mv_dirty) {
            uint8_t movable[RIO_GP_MAX_CLASSES];
            for (uint32_t c = 0; c < RIO_GP_MAX_CLASSES; ++c) movable[c] = !(c < s->type_immovable.size() && s->type_immovable[c]);
            if ((rc = rio_gp_set_class_movable(s->gp, RIO_GP_MAX_CLASSES, movable))) return gp_fail(s, rc);
            s->mv_dirty = false;
            s->mv_on_device = true;
        }
    } else if (s->mv_on_device) {
        if ((rc = rio_gp_set_class_movable(s->gp, 0, nullptr))) return gp_fail(s, rc);
        s->mv_dirty = false;
        s->mv_on_device = false;
    }
    return RIO_GP_OK;
}

int rio_op_set_type_movable_n(rio_op_t* p, const char* struct_name, size_t len, int movable) {
    if (!p || (!struct_name && len)) return RIO_GP_EINVAL;
    if (!rio_gp_set_class_movable || !rio_gp_set_classes || !rio_gp_set_class_batch)
        return fail(RIO_GP_EUPSTREAM, "dense layer has no immovable classes");
    State* s = p->s;
    std::lock_guard<TableLock> gi(s->imu);
    const uint8_t c = intern_type(s, std::string(struct_name ? struct_name : "", len));
    if (c == RIO_OP_CLASS_OTHER) return fail(RIO_GP_ERANGE, "rio_op_set_type_movable_n: the type shares RIO_OP_CLASS_OTHER, which is always movable");
    const uint8_t imm = movable ? 0 : 1;
    if (s->type_immovable[c] != imm) {
        s->type_immovable[c] = imm;
        if (imm) ++s->n_immovable; else --s->n_immovable;
        s->mv_dirty = true;
    }
    return RIO_GP_OK;
}

int rio_op_rebalance(rio_op_t* p, uint64_t max_moves, uint64_t* n_out, const char* const** struct_names,
                     const size_t** struct_name_lens, const char* const** object_ids, const size_t** object_id_lens,
                     const char* const** from_addresses, const char* const** to_addresses) {
    return rio_op_rebalance_ordered(p, RIO_GP_REBALANCE_ROW_ORDER, max_moves, n_out, struct_names, struct_name_lens, object_ids,
                                    object_id_lens, from_addresses, to_addresses);
}

int rio_op_rebalance_ordered(rio_op_t* p, uint32_t order, uint64_t max_moves, uint64_t* n_out, const char* const** struct_names,
                             const size_t** struct_name_lens, const char* const** object_ids, const size_t** object_id_lens,
                             const char* const** from_addresses, const char* const** to_addresses) {
    if (!p || !n_out || !struct_names || !struct_name_lens || !object_ids || !object_id_lens || !from_addresses || !to_addresses)
        return RIO_GP_EINVAL;
    if (order != RIO_GP_REBALANCE_ROW_ORDER && order != RIO_GP_REBALANCE_BY_LOAD)
        return fail(RIO_GP_EINVAL, "rio_op_rebalance_ordered: unknown order");
    State* s = p->s;
    t_rb.clear();
    {
        DevLock g(s);
        std::lock_guard<TableLock> gi(s->imu);  // the write side: no lookup is answered while keys change their address
        int rc;
        if ((rc = sync_device(s, true))) return rc;
        if (!rio_gp_rebalance) return fail(RIO_GP_EUPSTREAM, "dense layer has no rebalance");
        if ((rc = sync_movable(s))) return rc;
        // a move is a row that is handed out: at most as many as rows were ever interned
        const uint64_t cap = std::min<uint64_t>(max_moves, s->row_key.size());
        std::vector<uint32_t> &rows = t_rb.rows, &src = t_rb.c1, &dst = t_rb.c2;
        rows.resize(cap ? cap : 1); src.resize(cap ? cap : 1); dst.resize(cap ? cap : 1);
        rio_gp_rebalance_cfg cfg{};
        cfg.struct_size = sizeof cfg;
        cfg.max_moves = cap;  // targets: the capacities of rio_op_set_member
        cfg.order = order;
        uint64_t n = 0;
        rc = rio_gp_rebalance(s->gp, &cfg, nullptr, rows.data(), src.data(), dst.data(), cap, &n);
        s->shadow.invalidate_all();  // moved rows must not be answered from their old address (also when the call failed)
        if (rc) return gp_fail(s, rc);
        for (uint64_t k = 0; k < n; ++k) t_rb.add(s, rows[k], addr_of(s, src[k], ""), addr_of(s, dst[k], ""));
    }
    t_rb.publish(n_out, struct_names, struct_name_lens, object_ids, object_id_lens, from_addresses, to_addresses);
    return RIO_GP_OK;
}

int rio_op_set_clock(rio_op_t* p, uint32_t now) {
    if (!p) return RIO_GP_EINVAL;
    p->s->seen.set_clock(now);
    return RIO_GP_OK;
}

// The device's class column follows the host's: a range for the rows handed out since the last upload, a scatter for the rows
// that changed hands to a key of another class (mu + imu exclusive held, sync_device done: the device knows hi_rows rows).
static int sync_classes(State* s) {
    const uint64_t n = s->hi_rows;
    int rc;
    if (n > s->cls_uploaded) {
        if ((rc = rio_gp_set_classes(s->gp, s->cls_uploaded, n - s->cls_uploaded, s->row_class.data() + s->cls_uploaded)))
            return gp_fail(s, rc);
        s->cls_uploaded = n;
    }
    if (!s->cls_dirty.empty()) {
        std::vector<uint8_t> cls(s->cls_dirty.size());
        for (size_t k = 0; k < cls.size(); ++k) cls[k] = s->row_class[s->cls_dirty[k]];  // (the row's class now: duplicates agree)
        if ((rc = rio_gp_set_class_batch(s->gp, cls.size(), s->cls_dirty.data(), cls.data()))) return gp_fail(s, rc);
        s->cls_dirty.clear();
    }
    return RIO_GP_OK;
}

// rio_op_expire and rio_op_expire_by_type: `sweep(rows, node, cap, &idle)` is the dense call, `ready()` what it needs on the
// device first (it answers RIO_GP_EUPSTREAM before anything changes on a dense layer without the calls).
extern "C++" {
template <class Ready, class Sweep>
static int expire_impl(rio_op_t* p, uint64_t max_objects_out, uint64_t* n_out, uint64_t* n_idle, const char* const** struct_names,
                       const size_t** struct_name_lens, const char* const** object_ids, const size_t** object_id_lens,
                       const char* const** addresses, Ready&& ready, Sweep&& sweep) {
    if (!p || !n_out || !struct_names || !struct_name_lens || !object_ids || !object_id_lens || !addresses) return RIO_GP_EINVAL;
    State* s = p->s;
    t_ex.clear();
    *n_out = 0;
    if (n_idle) *n_idle = 0;
    {
        // mu keeps every device change out; the write side of the table lock keeps every stamper out: a stamp of an epoch >=
        // cutoff that was written before this lock was taken is in the upload below, so its key cannot be listed
        DevLock g(s);
        std::lock_guard<TableLock> gi(s->imu);
        int rc;
        if ((rc = sync_device(s, true))) return rc;
        if ((rc = ready(s))) return rc;
        const uint64_t n = s->hi_rows;
        if (s->seen.gather(n, t_ex_stamps) && (rc = rio_gp_touch_merge(s->gp, n, t_ex_stamps.data()))) return gp_fail(s, rc);
        const uint64_t cap = std::min<uint64_t>(max_objects_out, n);  // a listed row is a row that is handed out
        uint64_t idle = 0;
        if (!cap) {  // count only: nothing changes
            if ((rc = sweep(s, nullptr, nullptr, 0, &idle))) return gp_fail(s, rc);
            if (n_idle) *n_idle = idle;
        } else {
            std::vector<uint32_t> &rows = t_ex.rows, &node = t_ex.c1;
            rows.resize(cap); node.resize(cap);
            if ((rc = sweep(s, rows.data(), node.data(), cap, &idle))) {
                s->shadow.invalidate_all();  // (nobody can tell which rows it un-placed before it failed)
                return gp_fail(s, rc);
            }
            if (n_idle) *n_idle = idle;
            const uint64_t got = std::min(idle, cap);
            // the shadow follows precisely: exactly the listed rows are un-placed; every other row's entry stands
            for (uint64_t k = 0; k < got; ++k) {
                s->shadow.put(rows[k], RIO_GP_NONE);
                t_ex.add(s, rows[k], addr_of(s, node[k]));
            }
        }
    }
    t_ex.publish(n_out, struct_names, struct_name_lens, object_ids, object_id_lens, addresses);
    return RIO_GP_OK;
}
}  // extern "C++"

int rio_op_expire(rio_op_t* p, uint32_t cutoff, uint64_t max_objects_out, uint64_t* n_out, uint64_t* n_idle,
                  const char* const** struct_names, const size_t** struct_name_lens, const char* const** object_ids,
                  const size_t** object_id_lens, const char* const** addresses) {
    return expire_impl(
        p, max_objects_out, n_out, n_idle, struct_names, struct_name_lens, object_ids, object_id_lens, addresses,
        [](State*) { return !rio_gp_touch_merge || !rio_gp_expire ? fail(RIO_GP_EUPSTREAM, "dense layer has no idle expiry") : RIO_GP_OK; },
        [&](State* s, uint32_t* rows, uint32_t* node, uint64_t cap, uint64_t* idle) {
            return rio_gp_expire(s->gp, cutoff, rows, node, cap, idle, nullptr);
        });
}

static bool has_classes() { return rio_gp_touch_merge && rio_gp_set_classes && rio_gp_set_class_batch && rio_gp_expire_classes && rio_gp_census; }

int rio_op_set_type_idle_limit_n(rio_op_t* p, const char* struct_name, size_t len, uint32_t max_idle) {
    if (!p || (!struct_name && len)) return RIO_GP_EINVAL;
    State* s = p->s;
    std::lock_guard<TableLock> gi(s->imu);
    const uint8_t c = intern_type(s, std::string(struct_name ? struct_name : "", len));
    if (c == RIO_OP_CLASS_OTHER) return fail(RIO_GP_ERANGE, "rio_op_set_type_idle_limit_n: the type shares RIO_OP_CLASS_OTHER, which has no limit of its own");
    s->type_limit[c] = max_idle;
    s->type_has_limit[c] = 1;
    return RIO_GP_OK;
}

int rio_op_expire_by_type(rio_op_t* p, uint32_t now, uint32_t default_max_idle, uint64_t max_objects_out, uint64_t* n_out,
                          uint64_t* n_idle, const char* const** struct_names, const size_t** struct_name_lens,
                          const char* const** object_ids, const size_t** object_id_lens, const char* const** addresses) {
    uint32_t cutoffs[RIO_GP_MAX_CLASSES];
    return expire_impl(
        p, max_objects_out, n_out, n_idle, struct_names, struct_name_lens, object_ids, object_id_lens, addresses,
        [&](State* s) {
            if (!has_classes()) return fail(RIO_GP_EUPSTREAM, "dense layer has no object classes");
            // a key is idle iff stamp + L < now, without wrap-around: cutoff = now - L where that is positive, else 0 (nothing);
            // RIO_OP_IDLE_NEVER >= every now.  Types seen later than this call are not idle by it: they have the default too.
            for (uint32_t c = 0; c < RIO_GP_MAX_CLASSES; ++c) {
                const uint32_t L = c < s->type_has_limit.size() && s->type_has_limit[c] ? s->type_limit[c] : default_max_idle;
                cutoffs[c] = now > L ? now - L : 0u;
            }
            return sync_classes(s);
        },
        [&](State* s, uint32_t* rows, uint32_t* node, uint64_t cap, uint64_t* idle) {
            return rio_gp_expire_classes(s->gp, RIO_GP_MAX_CLASSES, cutoffs, rows, node, cap, idle, nullptr, nullptr);
        });
}

// Rule 14 over the members' capacities.  rio_op_expire's body with another dense call: the surplus takes the place of the idle
// count, and the rows the call un-placed are its first min(surplus, cap).  Types that must never be deactivated go down as a
// class-cutoff table (cutoff 0 for RIO_OP_IDLE_NEVER); immovable types follow from the dense rule once the table is uploaded.
int rio_op_shed_idle(rio_op_t* p, uint32_t cutoff, uint64_t max_objects_out, uint64_t* n_out, uint64_t* n_surplus,
                     const char* const** struct_names, const size_t** struct_name_lens, const char* const** object_ids,
                     const size_t** object_id_lens, const char* const** addresses) {
    uint32_t cutoffs[RIO_GP_MAX_CLASSES];
    bool by_class = false;
    return expire_impl(
        p, max_objects_out, n_out, n_surplus, struct_names, struct_name_lens, object_ids, object_id_lens, addresses,
        [&](State* s) {
            if (!rio_gp_touch_merge || !rio_gp_shed_idle) return fail(RIO_GP_EUPSTREAM, "dense layer has no pressure shedding");
            for (uint32_t c = 0; c < RIO_GP_MAX_CLASSES; ++c) {
                const bool never = c < s->type_has_limit.size() && s->type_has_limit[c] && s->type_limit[c] == RIO_OP_IDLE_NEVER;
                cutoffs[c] = never ? 0u : cutoff;
                by_class = by_class || never;
            }
            const bool movable_table = s->n_immovable || s->mv_on_device;
            if ((by_class || movable_table) && !has_classes()) return fail(RIO_GP_EUPSTREAM, "dense layer has no object classes");
            if (movable_table && !rio_gp_set_class_movable) return fail(RIO_GP_EUPSTREAM, "dense layer has no immovable classes");
            int rc;
            if (by_class && (rc = sync_classes(s))) return rc;
            return movable_table ? sync_movable(s) : RIO_GP_OK;
        },
        [&](State* s, uint32_t* rows, uint32_t* node, uint64_t cap, uint64_t* surplus) {
            rio_gp_shed_cfg cfg{};
            cfg.struct_size = sizeof cfg;
            cfg.cutoff = cutoff;
            cfg.max_rows = cap;  // targets: the capacities of rio_op_set_member
            cfg.class_cutoffs = by_class ? cutoffs : nullptr;
            cfg.n_classes = by_class ? RIO_GP_MAX_CLASSES : 0u;
            rio_gp_shed_stats st{};
            const int rc = rio_gp_shed_idle(s->gp, &cfg, &st, rows, node, cap, nullptr);
            *surplus = st.surplus_rows;
            return rc;
        });
}

// rio_op_census's listing: the calling thread's until its next call
struct CensusListing {
    std::vector<const char*> names, addrs;
    std::vector<size_t> lens;
    std::vector<uint64_t> rows, loads, cell_rows, cell_loads;
};
static thread_local CensusListing t_census;

int rio_op_census(rio_op_t* p, int by_server, uint64_t* n_out, const char* const** struct_names, const size_t** struct_name_lens,
                  const char* const** addresses, const uint64_t** rows, const uint64_t** loads) {
    if (!p || !n_out || !struct_names || !struct_name_lens || !addresses || !rows || !loads) return RIO_GP_EINVAL;
    State* s = p->s;
    CensusListing& t = t_census;
    t.names.clear(); t.addrs.clear(); t.lens.clear(); t.rows.clear(); t.loads.clear();
    *n_out = 0;
    {
        // the locks of rio_op_expire: the class upload changes what the layer knows about the device
        DevLock g(s);
        std::lock_guard<TableLock> gi(s->imu);
        int rc;
        if ((rc = sync_device(s, true))) return rc;
        if (!has_classes()) return fail(RIO_GP_EUPSTREAM, "dense layer has no object classes");
        if ((rc = sync_classes(s))) return rc;
        const uint32_t m = by_server ? (uint32_t)s->node_addr.size() : 1u;
        const uint32_t dm = by_server ? s->pushed_nodes : 1u;  // (the device's node count: the cells it writes)
        t.cell_rows.assign((size_t)std::max(m, dm) * RIO_GP_MAX_CLASSES + 1, 0);
        t.cell_loads.assign((size_t)std::max(m, dm) * RIO_GP_MAX_CLASSES + 1, 0);
        uint64_t other = 0;
        if ((rc = rio_gp_census(s->gp, by_server ? RIO_GP_CENSUS_BY_NODE : 0u, RIO_GP_MAX_CLASSES, t.cell_rows.data(),
                                t.cell_loads.data(), &other)))
            return gp_fail(s, rc);
        for (uint32_t j = 0; j < std::min(m, dm); ++j)
            for (uint32_t c = 0; c < RIO_GP_MAX_CLASSES; ++c) {
                const size_t cell = (size_t)j * RIO_GP_MAX_CLASSES + c;
                if (!t.cell_rows[cell]) continue;
                const bool named = c < s->type_name.size();
                t.names.push_back(named ? s->type_name[c].data() : nullptr);
                t.lens.push_back(named ? s->type_name[c].size() : 0);
                t.addrs.push_back(by_server ? addr_of(s, j) : nullptr);
                t.rows.push_back(t.cell_rows[cell]);
                t.loads.push_back(t.cell_loads[cell]);
            }
    }
    *n_out = t.rows.size();
    *struct_names = t.names.data();
    *struct_name_lens = t.lens.data();
    *addresses = t.addrs.data();
    *rows = t.rows.data();
    *loads = t.loads.data();
    return RIO_GP_OK;
}

int rio_op_set_load_tracking(rio_op_t* p, int on) {
    if (!p) return RIO_GP_EINVAL;
    p->s->seen.set_tracking(on != 0);
    return RIO_GP_OK;
}

int rio_op_fold_loads(rio_op_t* p, uint32_t keep, uint32_t gain, uint32_t min_load, uint32_t max_load, uint64_t* rows_changed,
                      uint64_t* hits_folded) {
    if (!p) return RIO_GP_EINVAL;
    if (rows_changed) *rows_changed = 0;
    if (hits_folded) *hits_folded = 0;
    if (keep > 65536u || min_load > max_load) return fail(RIO_GP_EINVAL, "rio_op_fold_loads: keep above 65536 or min_load above max_load");
    State* s = p->s;
    // mu keeps every device change out; the write side of the table lock keeps the stampers that hold the shared side out.  A
    // call in flight counts without a lock: take_hits takes each word with an exchange, so its request is in this fold or the next.
    DevLock g(s);
    std::lock_guard<TableLock> gi(s->imu);
    int rc;
    if ((rc = sync_device(s, true))) return rc;
    if (!rio_gp_hits_merge || !rio_gp_load_fold) return fail(RIO_GP_EUPSTREAM, "dense layer has no measured load");
    const uint64_t n = s->hi_rows;
    if (s->seen.take_hits(n, t_ld_hits) && (rc = rio_gp_hits_merge(s->gp, n, t_ld_hits.data()))) {
        s->seen.give_back(t_ld_hits);  // (nothing reached the device: the requests wait for the next fold)
        return gp_fail(s, rc);
    }
    rio_gp_load_fold_stats st{};
    if ((rc = rio_gp_load_fold(s->gp, keep, gain, min_load, max_load, &st))) return gp_fail(s, rc);
    // Rows waiting on the free list belong to no key.  Each held load 1 and no request (reclaim() and this function leave them
    // so), so the fold made clamp(keep == 65536 ? 1 : 0) of every one of them: where that is not 1 they are no key's change —
    // they leave the count — and are put back to 1, what whoever gets one expects to find.
    const uint32_t kept = keep == 65536u ? 1u : 0u;
    const uint32_t free_load = kept < min_load ? min_load : (kept > max_load ? max_load : kept);
    const uint64_t n_free = free_load != 1u ? s->free_rows.size() : 0;
    if (rows_changed) *rows_changed = st.rows_changed - std::min<uint64_t>(n_free, st.rows_changed);
    if (hits_folded) *hits_folded = st.hits_folded;
    if (n_free) {  // (the fold has happened and is reported, whatever becomes of this call)
        const std::vector<uint32_t> ones(n_free, 1u);
        if ((rc = rio_gp_set_object_attrs(s->gp, n_free, s->free_rows.data(), ones.data(), nullptr))) return gp_fail(s, rc);
    }
    return RIO_GP_OK;  // (no address changed: the host shadow stands)
}

int rio_op_get_object_load(rio_op_t* p, const char* struct_name, size_t struct_name_len, const char* object_id,
                           size_t object_id_len, uint32_t* load, int* found) {
    if (!p || !struct_name || !object_id || !load || !found) return RIO_GP_EINVAL;
    State* s = p->s;
    *found = 0;
    *load = 0;
    DevLock g(s);
    std::lock_guard<TableLock> gi(s->imu);
    const auto it = s->rows.find(key_of(Part(struct_name, struct_name_len), Part(object_id, object_id_len)));
    if (it == s->rows.end()) return RIO_GP_OK;
    int rc;
    if ((rc = sync_device(s, true))) return rc;
    const uint64_t n = s->hi_rows;
    t_ld_col.resize(n ? n : 1);
    if ((rc = rio_gp_get_objects(s->gp, n, t_ld_col.data(), nullptr))) return gp_fail(s, rc);
    *load = t_ld_col[it->second];
    *found = 1;
    if (t_ld_col.capacity() > (1u << 16)) std::vector<uint32_t>().swap(t_ld_col);  // (a big table's column does not stay with the thread)
    return RIO_GP_OK;
}

int rio_op_hottest_objects(rio_op_t* p, const char* address, uint32_t min_load, uint64_t max_objects_out, uint64_t* n_out,
                           uint64_t* n_candidates, const char* const** struct_names, const size_t** struct_name_lens,
                           const char* const** object_ids, const size_t** object_id_lens, const char* const** addresses,
                           uint32_t* loads) {
    if (!p || !n_out || !struct_names || !struct_name_lens || !object_ids || !object_id_lens || !addresses) return RIO_GP_EINVAL;
    if (max_objects_out && !loads) return RIO_GP_EINVAL;
    State* s = p->s;
    t_hot.clear();
    *n_out = 0;
    if (n_candidates) *n_candidates = 0;
    if (max_objects_out > RIO_GP_TOP_MAX) return fail(RIO_GP_EINVAL, "rio_op_hottest_objects: max_objects_out above RIO_GP_TOP_MAX");
    uint64_t listed = 0;
    {
        // rio_op_objects_on_server's locks: mu keeps every device change out and the shared side of the table lock keeps the
        // rows with their keys, so no row changes hands between the dense call and the translation.  Nothing is stamped or
        // counted, and the host shadow is not consulted: the loads are the device's.
        DevLock g(s);
        std::shared_lock<TableLock> gi(s->imu);
        int rc;
        if ((rc = sync_device(s, true))) return rc;
        if (!rio_gp_top_rows) return fail(RIO_GP_EUPSTREAM, "dense layer has no hot-object report");
        uint32_t flags = RIO_GP_TOP_PLACED, node = 0;
        bool known = true;
        if (address) {
            const auto it = s->nodes.find(address);
            known = it != s->nodes.end();  // (an address never seen holds nothing: 0 objects)
            if (known) {
                flags |= RIO_GP_TOP_ON_NODE;
                node = it->second;
            }
        }
        if (known) {
            const uint64_t cap = max_objects_out;
            uint64_t cand = 0;
            std::vector<uint32_t> &rows = t_hot.rows, &key = t_hot.c1, &on = t_hot.c2;
            if (!cap) {
                rc = rio_gp_top_rows(s->gp, flags, node, min_load, nullptr, nullptr, nullptr, 0, &cand, nullptr);
            } else {
                rows.resize(cap); key.resize(cap); on.resize(cap);
                rc = rio_gp_top_rows(s->gp, flags, node, min_load, rows.data(), key.data(), on.data(), cap, &cand, nullptr);
            }
            if (rc) return gp_fail(s, rc);
            if (n_candidates) *n_candidates = cand;
            const uint64_t got = std::min(cand, cap);
            // (a placed row has a key: rows on the free list are un-placed.  Were one ever not to, it is left out of the
            //  listing, which then falls short of min(*n_candidates, max_objects_out).)
            for (uint64_t k = 0; k < got; ++k)
                if (t_hot.add(s, rows[k], addr_of(s, on[k]))) loads[listed++] = key[k];
        }
    }
    t_hot.publish(n_out, struct_names, struct_name_lens, object_ids, object_id_lens, addresses);  // (*n_out == listed)
    return RIO_GP_OK;
}

int rio_op_changes(rio_op_t* p, uint64_t* n_out, int* full, const char* const** struct_names, const size_t** struct_name_lens,
                   const char* const** object_ids, const size_t** object_id_lens, const char* const** old_addresses,
                   const char* const** new_addresses) {
    if (!p || !n_out || !full || !struct_names || !struct_name_lens || !object_ids || !object_id_lens || !old_addresses ||
        !new_addresses)
        return RIO_GP_EINVAL;
    State* s = p->s;
    t_ch.clear();
    {
        // mu keeps every device change (and reclaim()) out until the listing is matched with its keys; the shared table lock keeps
        // the keys and the node table as they are
        DevLock g(s);
        std::shared_lock<TableLock> gi(s->imu);
        int rc;
        if ((rc = sync_device(s, true))) return rc;
        if (!rio_gp_changes || !rio_gp_changes_reset) return fail(RIO_GP_EUPSTREAM, "dense layer has no change feed");
        s->feed_on = true;
        // a listing the caller does not get must not stay consumed: the next call is a full one instead
        auto lost = [&](int code) {
            (void)rio_gp_changes_reset(s->gp);
            s->retired.clear();
            s->feed_full = true;
            return gp_fail(s, code);
        };
        // every change, consumed: into the thread's buffers from its last call first, the rest (a second page) with the exact size
        std::vector<uint32_t> &rows = t_ch.rows, &src = t_ch.c1, &dst = t_ch.c2;
        uint64_t total = 0, rest = 0;
        uint64_t cap = std::max<uint64_t>(rows.size(), 4096);
        rows.resize(cap); src.resize(cap); dst.resize(cap);
        if ((rc = rio_gp_changes(s->gp, 0, rows.data(), src.data(), dst.data(), cap, &total))) return lost(rc);
        uint64_t got = std::min(total, cap);
        if (total > got) {
            rows.resize(total); src.resize(total); dst.resize(total);
            if ((rc = rio_gp_changes(s->gp, 0, rows.data() + got, src.data() + got, dst.data() + got, total - got, &rest)))
                return lost(rc);
            got += std::min(rest, total - got);
        }
        // retired rows the listing does not hold have B == A: their node now is their old node as well
        std::vector<uint32_t> rr, rr_node;
        for (const auto& kv : s->retired) rr.push_back(kv.first);
        std::sort(rr.begin(), rr.end());
        {
            std::vector<uint32_t> miss;
            for (uint32_t r : rr)
                if (!std::binary_search(rows.begin(), rows.begin() + got, r)) miss.push_back(r);
            rr_node.assign(miss.size(), RIO_GP_NONE);
            if (!miss.empty() && (rc = rio_gp_lookup_batch(s->gp, miss.size(), miss.data(), rr_node.data()))) return lost(rc);
            rr.swap(miss);
        }
        // one row: a retired row deletes the mirror's key and upserts its new key; any other row upserts or deletes its key.
        // The listing takes the deletes in one pass over the rows and the upserts in a second one (ups).
        auto row = [&](uint32_t r, uint32_t from, uint32_t to, bool ups) {
            const char* a0 = addr_of(s, from);
            const char* a1 = addr_of(s, to);
            // (RIO_GP_NODE_GONE: the mirror holds the key on an address that has been removed — placed, address no longer known)
            const bool was = a0 || from == RIO_GP_NODE_GONE;
            const auto it = s->retired.find(r);
            if (it != s->retired.end()) {
                if (!ups && was) t_ch.add(it->second, a0);
                if (ups && a1) t_ch.add(s, r, nullptr, a1);
                return;
            }
            // (a row without a key here is a free row that was never the mirror's: unplaced on both sides)
            if (ups ? a1 != nullptr : (!a1 && was)) t_ch.add(s, r, a0, a1);
        };
        // deletes first, then upserts, both in row order
        for (int ups = 0; ups < 2; ++ups) {
            size_t k = 0;
            for (uint64_t i = 0; i < got; ++i) {
                for (; k < rr.size() && rr[k] < rows[i]; ++k) row(rr[k], rr_node[k], rr_node[k], ups);
                row(rows[i], src[i], dst[i], ups);
            }
            for (; k < rr.size(); ++k) row(rr[k], rr_node[k], rr_node[k], ups);
        }
        s->retired.clear();
        *full = s->feed_full ? 1 : 0;
        s->feed_full = false;
    }
    t_ch.publish(n_out, struct_names, struct_name_lens, object_ids, object_id_lens, old_addresses, new_addresses);
    return RIO_GP_OK;
}

int rio_op_changes_reset(rio_op_t* p) {
    if (!p) return RIO_GP_EINVAL;
    State* s = p->s;
    DevLock g(s);
    if (!rio_gp_changes_reset) return fail(RIO_GP_EUPSTREAM, "dense layer has no change feed");
    const int rc = rio_gp_changes_reset(s->gp);
    s->retired.clear();
    s->feed_full = true;
    return rc ? gp_fail(s, rc) : RIO_GP_OK;
}

int rio_op_tick(rio_op_t* p, rio_gp_stats* stats) {
    if (!p) return RIO_GP_EINVAL;
    State* s = p->s;
    DevLock g(s);
    int rc;
    if ((rc = sync_device(s, false))) return rc;
    // A whole-table solve has no requester that vouches for itself: it places on servers that are active members only, also when
    // requests first-touch their requester whatever membership says (the default: service.rs:244-252) — an object evicted from a
    // dead server would otherwise claim that same server, its home, again.
    if (s->self_assign && (rc = rio_gp_set_flags(s->gp, RIO_GP_CFG_ROW_LIFECYCLE))) return gp_fail(s, rc);
    rc = rio_gp_tick(s->gp, stats);
    if (rc) gp_fail(s, rc);
    s->shadow.invalidate_all();  // a whole-table solve may move any pending or evicted row (also when it failed half-way)
    if (s->self_assign) {
        const int rc2 = rio_gp_set_flags(s->gp, RIO_GP_CFG_ROW_LIFECYCLE | RIO_GP_CFG_REF_SELF_ASSIGN);
        if (rc2 && !rc) return gp_fail(s, rc2);
    }
    return rc;
}

int rio_op_invalidate_cache(rio_op_t* p) {
    if (!p) return RIO_GP_EINVAL;
    DevLock g(p->s);
    p->s->shadow.invalidate_all();
    return RIO_GP_OK;
}

int rio_op_device_round_trips(rio_op_t* p, uint64_t* batches, uint64_t* requests) {
    if (!p) return RIO_GP_EINVAL;
    DevLock g(p->s);
    if (batches) *batches = p->s->dev_batches;
    if (requests) *requests = p->s->dev_requests;
    return RIO_GP_OK;
}

}  // extern "C"
