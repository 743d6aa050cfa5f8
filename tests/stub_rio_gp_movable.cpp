// stub_rio_gp_movable.cpp — TEST INFRASTRUCTURE ONLY: the host-memory stub of the dense C ABI with the order-aware rebalance
// (stub_rio_gp_rebalance_order.cpp and what it includes) plus a host double of what the string layer's immovable types use: a
// class column (rio_gp_set_classes, rio_gp_set_class_batch, rio_gp_get_classes) and the table of rule 13
// (rio_gp_set_class_movable, rio_gp_get_class_movable), honoured by rio_gp_rebalance — so that rio_op_set_type_movable_n and
// rio_op_rebalance[_ordered] run without a GPU (tests/test_movable_host.py).  Same contract as the library's
// (include/rio_gpu_placement.h, DESIGN.md section 2 rule 13), by the equivalence the rule states: the rebalance of the included
// stub over the table in which the affinity of every row of an immovable class reads RIO_GP_AFF_INACTIVE; the affinity column
// is as it was afterwards.  stub_mv_calls counts the dense calls of the family, for the tests of what a rebalance uploads.
#define rio_gp_rebalance stub_plain_rebalance
#define rio_gp_destroy stub_mv_base_destroy
#include "stub_rio_gp_rebalance_order.cpp"
#undef rio_gp_rebalance
#undef rio_gp_destroy

#include <atomic>

struct MvState {
    std::vector<uint8_t> K;
    uint8_t immovable[RIO_GP_MAX_CLASSES] = {};
};
static std::mutex g_mv_mu;
static std::map<const rio_gp*, MvState> g_mv;
static std::atomic<uint64_t> g_mv_calls[3];  // 0: rio_gp_set_classes, 1: rio_gp_set_class_batch, 2: rio_gp_set_class_movable

static MvState& mv_of(rio_gp* h) {  // (g_mv_mu held)
    MvState& s = g_mv[h];
    if (s.K.size() != h->assign.size()) s.K.assign(h->assign.size(), 0);
    return s;
}

extern "C" void rio_gp_destroy(rio_gp_t* h) {
    {
        std::lock_guard<std::mutex> g(g_mv_mu);
        g_mv.erase(h);  // (a later handle may live at this address)
    }
    stub_mv_base_destroy(h);
}

extern "C" uint64_t stub_mv_calls(int which) { return g_mv_calls[which].load(); }

extern "C" int rio_gp_set_classes(rio_gp_t* h, uint64_t first_row, uint64_t rows, const uint8_t* cls) {
    if (!h || (rows && !cls)) return RIO_GP_EINVAL;
    ++g_mv_calls[0];
    std::lock_guard<std::mutex> g(h->mu);
    if (first_row > h->n || rows > h->n - first_row) return h->fail("stub: the range exceeds the object table");
    std::lock_guard<std::mutex> gs(g_mv_mu);
    MvState& s = mv_of(h);
    for (uint64_t k = 0; k < rows; ++k) s.K[first_row + k] = cls[k];
    return RIO_GP_OK;
}

extern "C" int rio_gp_set_class_batch(rio_gp_t* h, uint64_t n, const uint32_t* idx, const uint8_t* cls) {
    if (!h || (n && (!idx || !cls))) return RIO_GP_EINVAL;
    ++g_mv_calls[1];
    std::lock_guard<std::mutex> g(h->mu);
    for (uint64_t k = 0; k < n; ++k)
        if (idx[k] >= h->n) return h->fail("stub: object index out of range");
    std::lock_guard<std::mutex> gs(g_mv_mu);
    MvState& s = mv_of(h);
    for (uint64_t k = 0; k < n; ++k) s.K[idx[k]] = cls[k];  // (in order: the last entry of a row wins)
    return RIO_GP_OK;
}

extern "C" int rio_gp_get_classes(rio_gp_t* h, uint64_t n, uint8_t* out) {
    if (!h || !out) return RIO_GP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (n != h->n) return h->fail("stub: n differs from the object table");
    std::lock_guard<std::mutex> gs(g_mv_mu);
    const MvState& s = mv_of(h);
    for (uint64_t r = 0; r < n; ++r) out[r] = s.K[r];
    return RIO_GP_OK;
}

extern "C" int rio_gp_set_class_movable(rio_gp_t* h, uint32_t n_classes, const uint8_t* movable) {
    if (!h) return RIO_GP_EINVAL;
    ++g_mv_calls[2];
    std::lock_guard<std::mutex> g(h->mu);
    if (n_classes > RIO_GP_MAX_CLASSES) return h->fail("stub: n_classes out of range");
    if (n_classes && !movable) return h->fail("stub: no array");
    std::lock_guard<std::mutex> gs(g_mv_mu);
    MvState& s = mv_of(h);
    for (uint32_t c = 0; c < RIO_GP_MAX_CLASSES; ++c) s.immovable[c] = c < n_classes && !movable[c];
    return RIO_GP_OK;
}

extern "C" int rio_gp_get_class_movable(rio_gp_t* h, uint8_t* out256) {
    if (!h || !out256) return RIO_GP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    std::lock_guard<std::mutex> gs(g_mv_mu);
    const MvState& s = mv_of(h);
    for (uint32_t c = 0; c < RIO_GP_MAX_CLASSES; ++c) out256[c] = !s.immovable[c];
    return RIO_GP_OK;
}

// (the string layer makes one dense call at a time per handle: nobody reads aff between the two swaps)
extern "C" int rio_gp_rebalance(rio_gp_t* h, const rio_gp_rebalance_cfg* cfg, rio_gp_rebalance_stats* st, uint32_t* out_rows,
                                uint32_t* out_from, uint32_t* out_to, uint64_t moves_cap, uint64_t* n_moves) {
    if (!h) return RIO_GP_EINVAL;
    std::vector<std::pair<uint64_t, uint32_t>> saved;  // (row, its affinity)
    {
        std::lock_guard<std::mutex> g(h->mu);
        std::lock_guard<std::mutex> gs(g_mv_mu);
        const MvState& s = mv_of(h);
        for (uint64_t r = 0; r < h->n; ++r)
            if (s.immovable[s.K[r]] && h->aff[r] != RIO_GP_AFF_INACTIVE) {
                saved.emplace_back(r, h->aff[r]);
                h->aff[r] = RIO_GP_AFF_INACTIVE;
            }
    }
    const int rc = stub_plain_rebalance(h, cfg, st, out_rows, out_from, out_to, moves_cap, n_moves);
    std::lock_guard<std::mutex> g(h->mu);
    for (const auto& p : saved) h->aff[p.first] = p.second;
    return rc;
}
