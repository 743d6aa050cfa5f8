// host_layer_race_driver_remove_members.cpp — TEST INFRASTRUCTURE ONLY: the string layer (gpu_object_placement.cpp) over the
// host-memory stub with node removal (stub_rio_gp_remap.cpp), built with ThreadSanitizer.  Caller threads loop lookup /
// get_or_create_placement / the try_ forms over a fixed key set while one thread adds members, places keys on them and removes
// them again.  Node ids are renumbered under the callers' feet: every address a caller is handed must be one that exists in this
// run's address set (a renumbered id read against the old table would be another node's address — still in the set — so each
// key is only ever placed on ITS OWN addresses: key k on "n<k % 4>-<g>:1"; an answer outside that family is wrong).
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../include/rio_gpu_object_placement.h"

static std::atomic<int> g_stop{0};
static std::atomic<long> g_wrong{0}, g_calls{0};
constexpr int kKeys = 64, kFamilies = 4, kCallers = 6, kRounds = 120;

static bool own(int key, const char* addr) {  // "n<f>-<g>:1" with f == key % kFamilies
    return addr[0] == 'n' && addr[1] == (char)('0' + key % kFamilies) && addr[2] == '-';
}

static void caller(rio_op_t* p, int seed) {
    char buf[64];
    unsigned x = 12345u + (unsigned)seed * 977u;
    while (!g_stop.load(std::memory_order_acquire)) {
        x = x * 1664525u + 1013904223u;
        const int key = (int)((x >> 8) % kKeys);
        const std::string id = "k" + std::to_string(key);
        int found = 0;
        uint32_t flag = 0;
        int rc;
        switch ((x >> 4) & 3u) {
            case 0: rc = rio_op_lookup(p, "T", id.c_str(), buf, sizeof buf, &found); break;
            case 1: rc = rio_op_try_lookup_n(p, "T", 1, id.data(), id.size(), buf, sizeof buf, &found);
                    if (rc == RIO_GP_EAGAIN) { rc = RIO_GP_OK; found = 0; }
                    break;
            case 2: {  // a request arriving at a server of the key's own family that is never removed
                const std::string me = "n" + std::to_string(key % kFamilies) + "-home:1";
                rc = rio_op_get_or_create_placement(p, "T", id.c_str(), me.c_str(), buf, sizeof buf, &flag);
                found = rc == RIO_GP_OK && buf[0] != 0;
                break;
            }
            default: {
                const std::string me = "n" + std::to_string(key % kFamilies) + "-home:1";
                rc = rio_op_try_get_or_create_placement_n(p, "T", 1, id.data(), id.size(), me.c_str(), buf, sizeof buf, &flag);
                found = rc == RIO_GP_OK;
                if (rc == RIO_GP_EAGAIN) rc = RIO_GP_OK;
            }
        }
        if (rc != RIO_GP_OK || (found && !own(key, buf))) g_wrong.fetch_add(1);
        g_calls.fetch_add(1);
    }
}

int main() {
    rio_op_cfg cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = (uint32_t)sizeof cfg;
    cfg.max_objects = 1024;
    cfg.max_nodes = 12;  // 4 home servers + at most 8 short-lived ones: the table only holds them because ids come back
    rio_op_t* p = nullptr;
    if (rio_op_create(&cfg, &p) != RIO_GP_OK) return 2;
    for (int f = 0; f < kFamilies; ++f)
        if (rio_op_set_member(p, ("n" + std::to_string(f) + "-home:1").c_str(), 1, RIO_GP_CAP_INF)) return 3;
    std::vector<std::thread> th;
    std::vector<rio_op_t*> clones;
    for (int t = 0; t < kCallers; ++t) {
        clones.push_back(rio_op_clone(p));
        th.emplace_back(caller, clones.back(), t);
    }
    long wrong = 0;
    for (int g = 0; g < kRounds; ++g) {  // members come (two per family), take keys, and go — under new names every round
        std::vector<std::string> names;
        for (int f = 0; f < kFamilies; ++f)
            for (int q = 0; q < 2; ++q) names.push_back("n" + std::to_string(f) + "-" + std::to_string(2 * g + q) + ":1");
        for (const std::string& a : names) wrong += rio_op_set_member(p, a.c_str(), 1, RIO_GP_CAP_INF) != RIO_GP_OK;
        for (int key = g % 3; key < kKeys; key += 3) {
            const std::string id = "k" + std::to_string(key);
            wrong += rio_op_update(p, "T", id.c_str(), names[(size_t)(key % kFamilies) * 2 + (size_t)(key & 1)].c_str()) != RIO_GP_OK;
        }
        std::vector<const char*> ptrs;
        for (const std::string& a : names) ptrs.push_back(a.c_str());
        uint64_t removed = 0, evicted = 0;
        wrong += rio_op_remove_members(p, ptrs.size(), ptrs.data(), &removed, &evicted) != RIO_GP_OK;
        wrong += removed != names.size();
        if (g % 16 == 0) wrong += rio_op_tick(p, nullptr) != RIO_GP_OK;
    }
    g_stop.store(1, std::memory_order_release);
    for (std::thread& t : th) t.join();
    for (rio_op_t* c : clones) rio_op_release(c);
    // the table is what the home servers hold: every short-lived address is gone, ids 0 .. 3 are the homes
    for (uint32_t k = 0; k < 6; ++k) {
        const char* a = rio_op_node_address(p, k);
        wrong += k < (uint32_t)kFamilies ? !(a && strstr(a, "-home:1")) : a != nullptr;
    }
    rio_op_release(p);
    printf("calls=%ld wrong=%ld\n", g_calls.load(), wrong + g_wrong.load());
    return wrong + g_wrong.load() ? 1 : 0;
}
