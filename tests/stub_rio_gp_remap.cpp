// stub_rio_gp_remap.cpp — TEST INFRASTRUCTURE ONLY: the host-memory stub of the dense C ABI with its optional calls (reverse
// index, rebalance, change feed: included as stub_rio_gp_all.cpp includes them) plus a host rio_gp_remap_nodes, so that the string
// layer's rio_op_remove_members runs without a GPU (tests/test_remove_members_host.py, the ThreadSanitizer run of
// tests/test_host_layer_races_remove_members.py).  Same contract as the library's (include/rio_gpu_placement.h, DESIGN.md section 2
// rule 8): the map is validated before anything changes; every row the handle holds is cleaned of the removed nodes (the stub
// always keeps the row lifecycle) and renumbered, the affinity column and — if the feed has been used — the checkpoint B as well
// (a removed node: RIO_GP_NODE_GONE); liveness and capacities move with their nodes.
#define rio_gp_destroy stub_base_destroy
#define rio_gp_set_nodes stub_base_set_nodes
#include "stub_rio_gp.cpp"
#undef rio_gp_destroy
#undef rio_gp_set_nodes
#include "stub_rio_gp_rebalance.cpp"
#include "stub_rio_gp_changes.cpp"

extern "C" int rio_gp_remap_nodes(rio_gp_t* h, uint32_t m_new, const uint32_t* map, uint64_t* evicted) {
    if (!h) return RIO_GP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (!map) return h->fail("stub: map is NULL");
    const uint32_t m = (uint32_t)h->alive.size();
    if (m_new > m) return h->fail("stub: m_new exceeds the node count");
    std::vector<uint32_t> from(m_new ? m_new : 1, RIO_GP_NONE);
    uint32_t kept = 0;
    for (uint32_t j = 0; j < m; ++j) {
        if (map[j] == RIO_GP_NONE) continue;
        if (map[j] >= m_new || from[map[j]] != RIO_GP_NONE) return h->fail("stub: the kept ids are not 0 .. m_new-1, each once");
        from[map[j]] = j;
        ++kept;
    }
    if (kept != m_new) return h->fail("stub: fewer than m_new nodes are kept");
    uint64_t ev = 0;
    for (size_t r = 0; r < h->assign.size(); ++r) {
        uint32_t& a = h->assign[r];
        uint32_t& f = h->aff[r];
        const bool gone = a < m && map[a] == RIO_GP_NONE;
        if (a < m) a = map[a];
        if (gone) { f = RIO_GP_AFF_INACTIVE; ev += r < h->n; }
        else if (f < m) f = map[f];
    }
    {
        std::lock_guard<std::mutex> gf(g_feed_mu);
        const auto it = g_feed.find(h);
        if (it != g_feed.end())
            for (uint32_t& b : it->second)
                if (b < m) b = map[b] == RIO_GP_NONE ? RIO_GP_NODE_GONE : map[b];
    }
    std::vector<uint8_t> alive(m_new);
    for (uint32_t k = 0; k < m_new; ++k) alive[k] = h->alive[from[k]];
    h->alive.swap(alive);
    {
        std::lock_guard<std::mutex> gc(g_caps_mu);
        const auto it = g_caps.find(h);
        if (it != g_caps.end() && it->second.size() == m) {
            std::vector<uint64_t> cap(m_new);
            for (uint32_t k = 0; k < m_new; ++k) cap[k] = it->second[from[k]];
            it->second.swap(cap);
        }
    }
    if (evicted) *evicted = ev;
    return RIO_GP_OK;
}
