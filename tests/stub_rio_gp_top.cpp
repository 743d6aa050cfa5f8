// stub_rio_gp_top.cpp — TEST INFRASTRUCTURE ONLY: the host-memory stub of the dense C ABI (stub_rio_gp.cpp, which already has
// the load column, rio_gp_set_object_attrs and rio_gp_get_objects) plus a host rio_gp_top_rows, so that the string layer's
// rio_op_hottest_objects runs without a GPU (tests/test_top_host.py, the ThreadSanitizer driver
// tests/host_layer_race_driver_top.cpp).  Same contract as the library's (include/rio_gpu_placement.h, DESIGN.md section 2
// rule 11): candidates by key, PLACED and ON_NODE over the rows r < n, the first `cap` of them by (key descending, row
// ascending), every candidate counted.  The stub keeps no hit column: under RIO_GP_TOP_BY_HITS every key is 0, as on a handle that
// never counted a hit.
#include "stub_rio_gp.cpp"
#include <algorithm>
#include <utility>

extern "C" int rio_gp_top_rows(rio_gp_t* h, uint32_t flags, uint32_t node, uint32_t min_key, uint32_t* out_rows, uint32_t* out_key,
                               uint32_t* out_node, uint64_t cap, uint64_t* n_candidates, uint64_t* key_sum) {
    if (!h) return RIO_GP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (flags & ~(RIO_GP_TOP_BY_HITS | RIO_GP_TOP_PLACED | RIO_GP_TOP_ON_NODE)) return h->fail("stub: unknown flags");
    if (!n_candidates) return h->fail("stub: n_candidates is NULL");
    if (cap > RIO_GP_TOP_MAX) return h->fail("stub: cap above RIO_GP_TOP_MAX");
    if ((out_rows != nullptr) != (out_key != nullptr) || (!out_rows && (cap || out_node))) return h->fail("stub: listing arrays");
    if ((flags & RIO_GP_TOP_ON_NODE) && node >= h->alive.size()) return h->fail("stub: node out of range");
    std::vector<std::pair<uint32_t, uint32_t>> cand;  // (key, row)
    uint64_t sum = 0;
    for (uint64_t r = 0; r < h->n; ++r) {
        const uint32_t k = (flags & RIO_GP_TOP_BY_HITS) ? 0u : h->load[r];
        if (k < min_key) continue;
        if ((flags & RIO_GP_TOP_PLACED) && h->assign[r] == RIO_GP_NONE) continue;
        if ((flags & RIO_GP_TOP_ON_NODE) && h->assign[r] != node) continue;
        cand.emplace_back(k, (uint32_t)r);
        sum += k;
    }
    std::stable_sort(cand.begin(), cand.end(),
                     [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) { return a.first > b.first; });
    *n_candidates = cand.size();
    if (key_sum) *key_sum = sum;
    for (uint64_t k = 0; k < std::min<uint64_t>(cap, cand.size()); ++k) {
        out_rows[k] = cand[k].second;
        out_key[k] = cand[k].first;
        if (out_node) out_node[k] = h->assign[cand[k].second];
    }
    return RIO_GP_OK;
}
