// stub_rio_gp_loads.cpp — TEST INFRASTRUCTURE ONLY: the host-memory stub of the dense C ABI (stub_rio_gp.cpp, which already has
// rio_gp_get_objects) plus a host rio_gp_hits_merge and rio_gp_load_fold, so that the string layer's rio_op_set_load_tracking /
// rio_op_fold_loads / rio_op_get_object_load run without a GPU (tests/test_loads_host.py, the ThreadSanitizer driver
// tests/host_layer_race_driver_loads.cpp).  Same contract as the library's (include/rio_gpu_placement.h, DESIGN.md section 2
// rule 10): a hit column H per handle, 0 to begin with; the merge is a saturating sum; the fold is exact in 64 bits over the rows
// r < n and zeroes their H.  The stub's struct has no room for H: it lives in a side map, which rio_gp_create (wrapped here)
// clears for the address it hands out.
#define rio_gp_create stub_base_create
#include "stub_rio_gp.cpp"
#undef rio_gp_create
#include <map>

static std::mutex g_hits_mu;
static std::map<const rio_gp*, std::vector<uint32_t>> g_hits;

extern "C" int rio_gp_create(const rio_gp_cfg* cfg, rio_gp_t** out) {
    const int rc = stub_base_create(cfg, out);
    if (rc == RIO_GP_OK) {
        std::lock_guard<std::mutex> g(g_hits_mu);
        g_hits.erase(*out);  // (a handle freed earlier lived at this address)
    }
    return rc;
}

static std::vector<uint32_t>& hits_of(rio_gp* h) {  // (g_hits_mu held)
    std::vector<uint32_t>& v = g_hits[h];
    if (v.size() != h->assign.size()) v.assign(h->assign.size(), 0u);
    return v;
}

extern "C" int rio_gp_hits_merge(rio_gp_t* h, uint64_t rows, const uint32_t* counts) {
    if (!h || (rows && !counts)) return RIO_GP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (rows > h->n) return h->fail("stub: rows exceeds the object table");
    std::lock_guard<std::mutex> gs(g_hits_mu);
    std::vector<uint32_t>& H = hits_of(h);
    for (uint64_t r = 0; r < rows; ++r) {
        const uint64_t s = (uint64_t)H[r] + counts[r];
        H[r] = s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s;
    }
    return RIO_GP_OK;
}

extern "C" int rio_gp_load_fold(rio_gp_t* h, uint32_t keep, uint32_t gain, uint32_t min_load, uint32_t max_load,
                                rio_gp_load_fold_stats* st) {
    if (!h) return RIO_GP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (keep > 65536u || min_load > max_load) return h->fail("stub: keep above 65536 or min_load above max_load");
    std::lock_guard<std::mutex> gs(g_hits_mu);
    std::vector<uint32_t>& H = hits_of(h);
    rio_gp_load_fold_stats s;
    memset(&s, 0, sizeof s);
    for (uint64_t r = 0; r < h->n; ++r) {
        const uint64_t x = (((uint64_t)h->load[r] * keep) >> 16) + (uint64_t)H[r] * gain;
        const uint32_t nl = x < min_load ? min_load : (x > max_load ? max_load : (uint32_t)x);
        s.rows_changed += nl != h->load[r];
        s.hits_folded += H[r];
        s.load_before += h->load[r];
        s.load_after += nl;
        if (nl > s.max_load_after) s.max_load_after = nl;
        h->load[r] = nl;
        H[r] = 0;
    }
    if (st) *st = s;
    return RIO_GP_OK;
}
