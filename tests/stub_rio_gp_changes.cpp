// stub_rio_gp_changes.cpp — TEST INFRASTRUCTURE ONLY: the host-memory stub of the dense C ABI (stub_rio_gp.cpp, included as it
// is) plus a host-memory change feed (rio_gp_changes / rio_gp_changes_reset), so that the string layer's rio_op_changes runs
// without a GPU (tests/test_changes_host.py).  Same contract as the library's (include/rio_gpu_placement.h): a checkpoint column B
// per handle, RIO_GP_NONE to begin with; the changes are the rows r < n with assign[r] != B[r], listed in row order up to cap, and
// B advances for exactly the listed rows unless RIO_GP_CHANGES_PEEK.  The stub's struct has no room for B: it lives in a side map,
// which rio_gp_destroy (wrapped here) clears.
#include <map>

#define rio_gp_destroy stub_base_destroy
#include "stub_rio_gp.cpp"
#undef rio_gp_destroy

static std::mutex g_feed_mu;
static std::map<const rio_gp*, std::vector<uint32_t>> g_feed;

extern "C" void rio_gp_destroy(rio_gp_t* h) {
    {
        std::lock_guard<std::mutex> g(g_feed_mu);
        g_feed.erase(h);
    }
    stub_base_destroy(h);
}

static std::vector<uint32_t>& feed_of(rio_gp* h) {  // (g_feed_mu held)
    std::vector<uint32_t>& b = g_feed[h];
    if (b.size() != h->assign.size()) b.assign(h->assign.size(), RIO_GP_NONE);
    return b;
}

extern "C" int rio_gp_changes(rio_gp_t* h, uint32_t flags, uint32_t* out_rows, uint32_t* out_old, uint32_t* out_new, uint64_t cap,
                              uint64_t* n_changes) {
    if (!h || !n_changes || (flags & ~RIO_GP_CHANGES_PEEK)) return RIO_GP_EINVAL;
    if ((out_rows != nullptr) != (out_old != nullptr) || (out_rows != nullptr) != (out_new != nullptr) || (!out_rows && cap))
        return h->fail("stub: out_rows / out_old / out_new are given together or not at all");
    std::lock_guard<std::mutex> g(h->mu);
    std::lock_guard<std::mutex> gf(g_feed_mu);
    std::vector<uint32_t>& B = feed_of(h);
    uint64_t total = 0;
    for (uint64_t r = 0; r < h->n; ++r) {
        if (h->assign[r] == B[r]) continue;
        if (total < cap) {
            out_rows[total] = (uint32_t)r;
            out_old[total] = B[r];
            out_new[total] = h->assign[r];
            if (!(flags & RIO_GP_CHANGES_PEEK)) B[r] = h->assign[r];
        }
        ++total;
    }
    *n_changes = total;
    return RIO_GP_OK;
}

extern "C" int rio_gp_changes_reset(rio_gp_t* h) {
    if (!h) return RIO_GP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    std::lock_guard<std::mutex> gf(g_feed_mu);
    feed_of(h).assign(h->assign.size(), RIO_GP_NONE);
    return RIO_GP_OK;
}
