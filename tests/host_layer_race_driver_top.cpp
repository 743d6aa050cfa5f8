// host_layer_race_driver_top.cpp — TEST INFRASTRUCTURE ONLY: the string layer (gpu_object_placement.cpp) over the host-memory
// stub with the hot-object report (stub_rio_gp_top.cpp), built with ThreadSanitizer.  Caller threads loop update /
// get_or_create_placement / lookup over a fixed set of keys on clones while reporter threads call rio_op_hottest_objects, per
// address and over all addresses.  Every report must be well formed whatever runs beside it: at most the number asked for, loads
// descending, every key one of the set with its own length, every address one of the members (include/rio_gpu_object_placement.h:
// the report holds the device lock and the shared side of the table lock, so no row changes hands under it).
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../include/rio_gpu_object_placement.h"

static std::atomic<int> g_stop{0};
static std::atomic<long> g_wrong{0}, g_reports{0};
constexpr int kKeys = 48, kCallers = 4, kReporters = 2, kReports = 150;

static void caller(rio_op_t* p, int me_idx) {
    char buf[64];
    const std::string me = "s" + std::to_string(me_idx % 3) + ":1";
    for (long pass = 0; !g_stop.load(std::memory_order_acquire); ++pass) {
        for (int key = 0; key < kKeys; ++key) {
            const std::string id = "h" + std::to_string(key);
            int found = 0;
            uint32_t flag = 0;
            int rc;
            switch ((key + pass + me_idx) % 3) {
                case 0: rc = rio_op_update(p, "T", id.c_str(), ("s" + std::to_string((key + pass) % 3) + ":1").c_str()); break;
                case 1: rc = rio_op_get_or_create_placement(p, "T", id.c_str(), me.c_str(), buf, sizeof buf, &flag); break;
                default: rc = rio_op_lookup(p, "T", id.c_str(), buf, sizeof buf, &found);
            }
            if (rc != RIO_GP_OK) g_wrong.fetch_add(1);
        }
    }
}

static void reporter(rio_op_t* p, int idx) {
    std::vector<uint32_t> loads(16);
    for (int k = 0; k < kReports; ++k) {
        const std::string addr = "s" + std::to_string((k + idx) % 3) + ":1";
        const uint64_t want = 1 + (uint64_t)(k % 16);
        uint64_t n = 0, cand = 0;
        const char* const* ty = nullptr;
        const char* const* id = nullptr;
        const char* const* ad = nullptr;
        const size_t* tl = nullptr;
        const size_t* il = nullptr;
        const int rc = rio_op_hottest_objects(p, k % 3 ? addr.c_str() : nullptr, 0, want, &n, &cand, &ty, &tl, &id, &il, &ad, loads.data());
        long bad = rc != RIO_GP_OK || n > want || n > cand || cand > (uint64_t)kKeys;
        for (uint64_t q = 0; !bad && q < n; ++q) {
            bad += tl[q] != 1 || ty[q][0] != 'T' || il[q] < 2 || il[q] > 3 || id[q][0] != 'h';
            bad += !ad[q] || (k % 3 && addr != ad[q]);
            bad += q && loads[q] > loads[q - 1];
        }
        if (bad) g_wrong.fetch_add(1);
        g_reports.fetch_add(1);
        std::this_thread::yield();
    }
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
    for (int key = 0; key < kKeys; ++key) {
        const std::string id = "h" + std::to_string(key);
        if (rio_op_update(p, "T", id.c_str(), "s0:1")) return 4;
        if (rio_op_set_object_load(p, "T", id.c_str(), 1 + (uint32_t)(key % 7))) return 5;
    }
    std::vector<std::thread> callers, reporters;
    std::vector<rio_op_t*> clones;
    for (int t = 0; t < kCallers + kReporters; ++t) clones.push_back(rio_op_clone(p));
    for (int t = 0; t < kCallers; ++t) callers.emplace_back(caller, clones[t], t);
    for (int t = 0; t < kReporters; ++t) reporters.emplace_back(reporter, clones[kCallers + t], t);
    long wrong = 0;
    for (int k = 0; k < 20; ++k) {
        if (k % 5 == 0) wrong += rio_op_invalidate_cache(p) != RIO_GP_OK;  // some calls go to the "device" again
        std::this_thread::yield();
    }
    for (std::thread& t : reporters) t.join();
    g_stop.store(1, std::memory_order_release);
    for (std::thread& t : callers) t.join();
    for (rio_op_t* c : clones) rio_op_release(c);
    rio_op_release(p);
    printf("reports=%ld wrong=%ld\n", g_reports.load(), wrong + g_wrong.load());
    return wrong + g_wrong.load() ? 1 : 0;
}
