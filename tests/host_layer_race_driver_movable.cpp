// host_layer_race_driver_movable.cpp — TEST INFRASTRUCTURE ONLY: the string layer (gpu_object_placement.cpp) over the host-memory
// stub with immovable classes (stub_rio_gp_movable.cpp), built with ThreadSanitizer.  Caller threads loop update / lookup /
// get_or_create_placement over keys of the types "P" (immovable from the start), "Q" (see below) and "M" (movable), always towards
// the crowded server s0, while a further thread interns new types ("X0", "X1", ...: more than 255 of them, so the
// RIO_OP_CLASS_OTHER answer runs too) and flips their flags, and the main thread rebalances in both orders, with and without a
// budget.  The invariant (include/rio_gpu_object_placement.h): a rebalance never lists a key whose type was immovable before the
// call took its locks.  "P" is immovable throughout; "Q" is made immovable by the main thread right before every other rebalance
// and movable again after it, so in those calls no "Q" key may be listed either, and in the others some are (the flag does come
// off).  "M" keys are listed all along: the rebalances do move things.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../include/rio_gpu_object_placement.h"

static std::atomic<int> g_stop{0};
static std::atomic<long> g_wrong{0}, g_calls{0};
constexpr int kKeys = 40, kCallers = 5, kRounds = 120;

static void caller(rio_op_t* p, int me_idx) {
    char buf[64];
    const char* types[3] = {"P", "Q", "M"};
    for (long pass = 0; !g_stop.load(std::memory_order_acquire); ++pass) {
        for (int key = 0; key < kKeys; ++key) {
            const std::string id = "k" + std::to_string(key);
            const char* ty = types[(key + me_idx) % 3];
            int found = 0, rc;
            uint32_t flag = 0;
            switch ((key + pass + me_idx) & 3) {
                case 0: rc = rio_op_update(p, ty, id.c_str(), "s0:1"); break;   // back onto the crowded server
                case 1: rc = rio_op_lookup(p, ty, id.c_str(), buf, sizeof buf, &found); break;
                case 2: rc = rio_op_get_or_create_placement(p, ty, id.c_str(), "s0:1", buf, sizeof buf, &flag); break;
                default: rc = rio_op_try_lookup_n(p, ty, 1, id.data(), id.size(), buf, sizeof buf, &found);
                         if (rc == RIO_GP_EAGAIN) rc = RIO_GP_OK;
            }
            if (rc != RIO_GP_OK) g_wrong.fetch_add(1);
            g_calls.fetch_add(1);
        }
    }
}

static void churner(rio_op_t* p) {
    long wrong = 0;
    for (int i = 0; !g_stop.load(std::memory_order_acquire); ++i) {
        const std::string ty = "X" + std::to_string(i % 400);
        const int rc = rio_op_set_type_movable_n(p, ty.data(), ty.size(), (i / 400) & 1);
        wrong += rc != RIO_GP_OK && rc != RIO_GP_ERANGE;  // (past 255 types: RIO_OP_CLASS_OTHER is always movable)
        wrong += rio_op_update_n(p, ty.data(), ty.size(), "k", 1, "s0:1") != RIO_GP_OK;
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
    if (rio_op_set_member(p, "s0:1", 1, 10)) return 3;                    // far below what the callers put on it
    if (rio_op_set_member(p, "s1:1", 1, RIO_GP_CAP_INF) || rio_op_set_member(p, "s2:1", 1, RIO_GP_CAP_INF)) return 3;
    if (rio_op_set_type_movable_n(p, "P", 1, 0)) return 4;
    std::vector<std::thread> th;
    std::vector<rio_op_t*> clones;
    for (int t = 0; t < kCallers; ++t) {
        clones.push_back(rio_op_clone(p));
        th.emplace_back(caller, clones.back(), t);
    }
    clones.push_back(rio_op_clone(p));
    th.emplace_back(churner, clones.back());
    long wrong = 0, p_listed = 0, q_listed_protected = 0, q_listed_free = 0, m_listed = 0;
    for (int r = 0; r < kRounds; ++r) {
        const bool protect_q = r & 1;
        if (protect_q) wrong += rio_op_set_type_movable_n(p, "Q", 1, 0) != RIO_GP_OK;
        uint64_t n = 0;
        const char* const* ty; const char* const* id; const char* const* from; const char* const* to;
        const size_t* tl; const size_t* il;
        const uint64_t budget = (r & 2) ? ~0ull : 7;
        const int rc = (r & 4) ? rio_op_rebalance_ordered(p, RIO_GP_REBALANCE_BY_LOAD, budget, &n, &ty, &tl, &id, &il, &from, &to)
                               : rio_op_rebalance(p, budget, &n, &ty, &tl, &id, &il, &from, &to);
        wrong += rc != RIO_GP_OK;
        for (uint64_t k = 0; rc == RIO_GP_OK && k < n; ++k) {
            if (tl[k] == 1 && ty[k][0] == 'P') ++p_listed;
            else if (tl[k] == 1 && ty[k][0] == 'Q') ++(protect_q ? q_listed_protected : q_listed_free);
            else if (tl[k] == 1 && ty[k][0] == 'M') ++m_listed;
            wrong += from[k] == nullptr || to[k] == nullptr;
        }
        if (protect_q) wrong += rio_op_set_type_movable_n(p, "Q", 1, 1) != RIO_GP_OK;
        for (int y = 0; y < 50; ++y) std::this_thread::yield();
    }
    g_stop.store(1, std::memory_order_release);
    for (std::thread& t : th) t.join();
    for (rio_op_t* c : clones) rio_op_release(c);
    rio_op_release(p);
    wrong += p_listed + q_listed_protected + (m_listed == 0) + (q_listed_free == 0);
    printf("calls=%ld protected_listed=%ld q_listed_free=%ld m_listed=%ld wrong=%ld\n", g_calls.load(), p_listed + q_listed_protected,
           q_listed_free, m_listed, wrong + g_wrong.load());
    return wrong + g_wrong.load() ? 1 : 0;
}
