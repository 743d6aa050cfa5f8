// host_layer_race_driver_classes.cpp — TEST INFRASTRUCTURE ONLY: the string layer (gpu_object_placement.cpp) over the host-memory
// stub with object classes (stub_rio_gp_classes.cpp), built with ThreadSanitizer.  Caller threads loop lookup / try_lookup /
// get_or_create_placement / try_get_or_create_placement over the HOT keys (type "T", idle limit 1) while the main thread advances
// the clock and sweeps with rio_op_expire_by_type, and a further thread interns new types (keys of types "X0", "X1", ...: more than
// 255 of them, so the RIO_OP_CLASS_OTHER path runs too) and sets limits on them.  The invariant
// (include/rio_gpu_object_placement.h): a key stamped at or after its type's cutoff before the sweep took its locks is never
// listed.  Every round the main thread sets the clock to e, waits until every caller has finished two whole passes over the hot
// keys (so every hot key carries a stamp >= e), and sweeps with now = e + 1 — the cutoff of "T" and "C" is e — while the callers
// keep calling: no hot key may be listed.  The cold keys (type "C", limit 1) are placed once per round and never asked for: the
// sweep lists all of them.  The "X" keys have limits that never let them be idle (the default is RIO_OP_IDLE_NEVER).
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../include/rio_gpu_object_placement.h"

static std::atomic<int> g_stop{0};
static std::atomic<long> g_wrong{0}, g_calls{0};
constexpr int kHot = 48, kCold = 40, kCallers = 6, kRounds = 60;
static std::atomic<long> g_pass[kCallers];  // whole passes over the hot keys a caller has FINISHED

static void caller(rio_op_t* p, int me_idx) {
    char buf[64];
    const std::string me = "s" + std::to_string(me_idx % 3) + ":1";
    for (long pass = 0; !g_stop.load(std::memory_order_acquire); ++pass) {
        for (int key = 0; key < kHot; ++key) {
            const std::string id = "h" + std::to_string(key);
            int found = 0;
            uint32_t flag = 0;
            int rc;
            // every hot key gets an address answered in every pass: a form that may decline (try_*) is followed by one that may not
            switch ((key + pass + me_idx) & 3) {
                case 0: rc = rio_op_get_or_create_placement(p, "T", id.c_str(), me.c_str(), buf, sizeof buf, &flag); break;
                case 1: rc = rio_op_try_lookup_n(p, "T", 1, id.data(), id.size(), buf, sizeof buf, &found);
                        if (rc == RIO_GP_EAGAIN || (rc == RIO_GP_OK && !found))
                            rc = rio_op_get_or_create_placement(p, "T", id.c_str(), me.c_str(), buf, sizeof buf, &flag);
                        break;
                case 2: rc = rio_op_lookup(p, "T", id.c_str(), buf, sizeof buf, &found);
                        if (rc == RIO_GP_OK && !found)
                            rc = rio_op_get_or_create_placement(p, "T", id.c_str(), me.c_str(), buf, sizeof buf, &flag);
                        break;
                default: rc = rio_op_try_get_or_create_placement_n(p, "T", 1, id.data(), id.size(), me.c_str(), buf, sizeof buf, &flag);
                         if (rc == RIO_GP_EAGAIN)
                             rc = rio_op_get_or_create_placement(p, "T", id.c_str(), me.c_str(), buf, sizeof buf, &flag);
            }
            if (rc != RIO_GP_OK) g_wrong.fetch_add(1);
            g_calls.fetch_add(1);
        }
        g_pass[me_idx].fetch_add(1, std::memory_order_release);
    }
}

static void churner(rio_op_t* p) {
    long wrong = 0;
    for (int i = 0; !g_stop.load(std::memory_order_acquire); ++i) {
        const std::string ty = "X" + std::to_string(i % 400);
        const int rc = rio_op_set_type_idle_limit_n(p, ty.data(), ty.size(), (i & 1) ? RIO_OP_IDLE_NEVER : (1u << 30));
        wrong += rc != RIO_GP_OK && rc != RIO_GP_ERANGE;  // (past 255 types: RIO_OP_CLASS_OTHER has no limit of its own)
        wrong += rio_op_update_n(p, ty.data(), ty.size(), "k", 1, "s1:1") != RIO_GP_OK;
        if ((i & 63) == 0) {
            uint64_t n = 0;
            const char* const* a; const char* const* b; const size_t* l; const uint64_t* r; const uint64_t* w;
            wrong += rio_op_census(p, i & 64 ? 1 : 0, &n, &a, &l, &b, &r, &w) != RIO_GP_OK;
        }
        std::this_thread::yield();
    }
    if (wrong) g_wrong.fetch_add(wrong);
}

int main() {
    rio_op_cfg cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = (uint32_t)sizeof cfg;
    cfg.max_objects = 4096;
    cfg.max_nodes = 8;
    rio_op_t* p = nullptr;
    if (rio_op_create(&cfg, &p) != RIO_GP_OK) return 2;
    for (int f = 0; f < 3; ++f)
        if (rio_op_set_member(p, ("s" + std::to_string(f) + ":1").c_str(), 1, RIO_GP_CAP_INF)) return 3;
    if (rio_op_set_clock(p, 1)) return 4;
    if (rio_op_set_type_idle_limit_n(p, "T", 1, 1) || rio_op_set_type_idle_limit_n(p, "C", 1, 1)) return 5;
    std::vector<std::thread> th;
    std::vector<rio_op_t*> clones;
    for (int t = 0; t < kCallers; ++t) {
        clones.push_back(rio_op_clone(p));
        th.emplace_back(caller, clones.back(), t);
    }
    clones.push_back(rio_op_clone(p));
    th.emplace_back(churner, clones.back());
    long wrong = 0, hot_listed = 0, cold_listed = 0;
    for (uint32_t e = 2; e < 2 + (uint32_t)kRounds; ++e) {
        for (int c = 0; c < kCold; ++c)  // stamped with e - 1
            wrong += rio_op_update(p, "C", ("c" + std::to_string(c)).c_str(), "s0:1") != RIO_GP_OK;
        wrong += rio_op_set_clock(p, e) != RIO_GP_OK;
        long seen[kCallers];
        for (int t = 0; t < kCallers; ++t) seen[t] = g_pass[t].load(std::memory_order_acquire);
        // a pass that was under way when the clock moved may have stamped its first keys with e - 1: wait for TWO to finish
        for (int t = 0; t < kCallers; ++t)
            while (g_pass[t].load(std::memory_order_acquire) < seen[t] + 2) std::this_thread::yield();
        uint64_t n = 0, idle = 0;
        const char* const* ty; const char* const* id; const char* const* ad;
        const size_t* tl; const size_t* il;
        const uint64_t cap = (e & 1) ? ~0ull : 25;  // every other sweep in pages
        for (;;) {
            wrong += rio_op_expire_by_type(p, e + 1, RIO_OP_IDLE_NEVER, cap, &n, &idle, &ty, &tl, &id, &il, &ad) != RIO_GP_OK;
            for (uint64_t k = 0; k < n; ++k) {
                if (tl[k] == 1 && ty[k][0] == 'T') ++hot_listed;
                else ++cold_listed;
                wrong += ad[k] == nullptr;
            }
            if (idle <= n) break;
        }
    }
    g_stop.store(1, std::memory_order_release);
    for (std::thread& t : th) t.join();
    for (rio_op_t* c : clones) rio_op_release(c);
    rio_op_release(p);
    wrong += hot_listed + (cold_listed != (long)kCold * kRounds);
    printf("calls=%ld hot_listed=%ld cold_listed=%ld wrong=%ld\n", g_calls.load(), hot_listed, cold_listed, wrong + g_wrong.load());
    return wrong + g_wrong.load() ? 1 : 0;
}
