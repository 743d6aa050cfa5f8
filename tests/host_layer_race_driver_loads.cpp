// host_layer_race_driver_loads.cpp — TEST INFRASTRUCTURE ONLY: the string layer (gpu_object_placement.cpp) over the host-memory
// stub with measured load (stub_rio_gp_loads.cpp), built with ThreadSanitizer.  Caller threads loop lookup / try_lookup /
// get_or_create_placement / try_get_or_create_placement over keys that are placed, with load tracking on, and count every call
// that answered an address; the main thread folds all the while.  The invariant (include/rio_gpu_object_placement.h): a request
// counted before a fold took its locks is in that fold, one counted after them is in the next — none is lost and none is
// counted twice.  So the requests folded by every fold, plus those of one last fold after the callers have stopped, are exactly
// the calls the callers counted.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../include/rio_gpu_object_placement.h"

static std::atomic<int> g_stop{0};
static std::atomic<long> g_wrong{0}, g_counted{0};
constexpr int kKeys = 48, kCallers = 6, kFolds = 200;

static void caller(rio_op_t* p, int me_idx) {
    char buf[64];
    const std::string me = "s" + std::to_string(me_idx % 3) + ":1";
    long mine = 0;
    for (long pass = 0; !g_stop.load(std::memory_order_acquire); ++pass) {
        for (int key = 0; key < kKeys; ++key) {
            const std::string id = "h" + std::to_string(key);
            int found = 0;
            uint32_t flag = 0;
            int rc;
            switch ((key + pass + me_idx) & 3) {
                case 0: rc = rio_op_get_or_create_placement(p, "T", id.c_str(), me.c_str(), buf, sizeof buf, &flag);
                        mine += rc == RIO_GP_OK;
                        break;
                case 1: rc = rio_op_try_lookup_n(p, "T", 1, id.data(), id.size(), buf, sizeof buf, &found);
                        mine += rc == RIO_GP_OK && found;
                        if (rc == RIO_GP_EAGAIN) rc = RIO_GP_OK;
                        break;
                case 2: rc = rio_op_lookup(p, "T", id.c_str(), buf, sizeof buf, &found);
                        mine += rc == RIO_GP_OK && found;
                        break;
                default: rc = rio_op_try_get_or_create_placement_n(p, "T", 1, id.data(), id.size(), me.c_str(), buf, sizeof buf, &flag);
                         mine += rc == RIO_GP_OK;
                         if (rc == RIO_GP_EAGAIN) rc = RIO_GP_OK;
            }
            if (rc != RIO_GP_OK) g_wrong.fetch_add(1);
        }
    }
    g_counted.fetch_add(mine);
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
    for (int key = 0; key < kKeys; ++key)  // placed before tracking is on: not counted
        if (rio_op_update(p, "T", ("h" + std::to_string(key)).c_str(), "s0:1")) return 4;
    if (rio_op_set_load_tracking(p, 1)) return 5;
    std::vector<std::thread> th;
    std::vector<rio_op_t*> clones;
    for (int t = 0; t < kCallers; ++t) {
        clones.push_back(rio_op_clone(p));
        th.emplace_back(caller, clones.back(), t);
    }
    long wrong = 0;
    uint64_t folded = 0;
    for (int k = 0; k < kFolds; ++k) {
        uint64_t changed = 0, hits = 0;
        wrong += rio_op_fold_loads(p, (k & 1) ? 65536u : 32768u, 1, 1, 1000000u, &changed, &hits) != RIO_GP_OK;
        folded += hits;
        if (k % 7 == 0) wrong += rio_op_invalidate_cache(p) != RIO_GP_OK;  // some calls go to the "device" again
        std::this_thread::yield();
    }
    g_stop.store(1, std::memory_order_release);
    for (std::thread& t : th) t.join();
    uint64_t changed = 0, hits = 0;
    wrong += rio_op_fold_loads(p, 65536u, 1, 1, 1000000u, &changed, &hits) != RIO_GP_OK;
    folded += hits;
    wrong += rio_op_fold_loads(p, 65536u, 1, 1, 1000000u, &changed, &hits) != RIO_GP_OK;  // nothing is left
    wrong += hits != 0;
    for (rio_op_t* c : clones) rio_op_release(c);
    rio_op_release(p);
    const long counted = g_counted.load();
    wrong += (long)folded != counted;
    printf("counted=%ld folded=%llu wrong=%ld\n", counted, (unsigned long long)folded, wrong + g_wrong.load());
    return wrong + g_wrong.load() ? 1 : 0;
}
