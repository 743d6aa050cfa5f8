// stub_rio_gp_expire.cpp — TEST INFRASTRUCTURE ONLY: the host-memory stub of the dense C ABI with its optional calls (reverse
// index, rebalance, change feed, node removal: included as stub_rio_gp_remap.cpp includes them) plus a host rio_gp_touch_merge and
// rio_gp_expire, so that the string layer's rio_op_set_clock / rio_op_expire run without a GPU (tests/test_expire_host.py, the
// ThreadSanitizer driver tests/host_layer_race_driver_expire.cpp).  Same contract as the library's (include/rio_gpu_placement.h,
// DESIGN.md section 2 rule 9): a last-seen column S per handle, 0 to begin with; row r < n is idle iff assign[r] != RIO_GP_NONE
// and S[r] < cutoff; the first min(n_idle, cap) idle rows are listed in row order and un-placed (the stub always keeps the row
// lifecycle: their affinity becomes RIO_GP_AFF_INACTIVE).  The stub's struct has no room for S: it lives in a side map, which
// rio_gp_create (wrapped here) clears for the address it hands out.
#define rio_gp_create stub_base_create
#define rio_gp_destroy stub_base_destroy
#define rio_gp_set_nodes stub_base_set_nodes
#include "stub_rio_gp.cpp"
#undef rio_gp_create
#undef rio_gp_destroy
#undef rio_gp_set_nodes
#include "stub_rio_gp_remap.cpp"

static std::mutex g_seen_mu;
static std::map<const rio_gp*, std::vector<uint32_t>> g_seen;

extern "C" int rio_gp_create(const rio_gp_cfg* cfg, rio_gp_t** out) {
    const int rc = stub_base_create(cfg, out);
    if (rc == RIO_GP_OK) {
        std::lock_guard<std::mutex> g(g_seen_mu);
        g_seen.erase(*out);  // (a handle freed earlier lived at this address)
    }
    return rc;
}

static std::vector<uint32_t>& seen_of(rio_gp* h) {  // (g_seen_mu held)
    std::vector<uint32_t>& s = g_seen[h];
    if (s.size() != h->assign.size()) s.assign(h->assign.size(), 0u);
    return s;
}

extern "C" int rio_gp_touch_merge(rio_gp_t* h, uint64_t rows, const uint32_t* stamps) {
    if (!h || (rows && !stamps)) return RIO_GP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (rows > h->n) return h->fail("stub: rows exceeds the object table");
    std::lock_guard<std::mutex> gs(g_seen_mu);
    std::vector<uint32_t>& S = seen_of(h);
    for (uint64_t r = 0; r < rows; ++r)
        if (stamps[r] > S[r]) S[r] = stamps[r];
    return RIO_GP_OK;
}

extern "C" int rio_gp_expire(rio_gp_t* h, uint32_t cutoff, uint32_t* out_rows, uint32_t* out_node, uint64_t cap, uint64_t* n_idle,
                             uint64_t* load_freed) {
    if (!h) return RIO_GP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (!n_idle) return h->fail("stub: n_idle is NULL");
    if ((out_rows != nullptr) != (out_node != nullptr) || (!out_rows && cap))
        return h->fail("stub: out_rows / out_node are given together or not at all");
    std::lock_guard<std::mutex> gs(g_seen_mu);
    const std::vector<uint32_t>& S = seen_of(h);
    uint64_t total = 0, freed = 0;
    for (uint64_t r = 0; r < h->n; ++r) {
        if (h->assign[r] == RIO_GP_NONE || S[r] >= cutoff) continue;
        if (total < cap) {
            out_rows[total] = (uint32_t)r;
            out_node[total] = h->assign[r];
            freed += h->load[r];
            h->assign[r] = RIO_GP_NONE;
            h->aff[r] = RIO_GP_AFF_INACTIVE;
        }
        ++total;
    }
    *n_idle = total;
    if (load_freed) *load_freed = freed;
    return RIO_GP_OK;
}
