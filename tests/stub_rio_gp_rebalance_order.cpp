// stub_rio_gp_rebalance_order.cpp — TEST INFRASTRUCTURE ONLY: the host-memory stub of the dense C ABI (stub_rio_gp_index.cpp, included
// as it is) plus a host-memory rio_gp_rebalance that honours rio_gp_rebalance_cfg.order, so that the string layer's
// rio_op_rebalance_ordered runs without a GPU (tests/test_rebalance_order_host.py).  The stub keeps no capacities, so its
// rio_gp_set_nodes is wrapped here to record them (the targets of a rebalance without a target array).  Same contract as the
// library's (include/rio_gpu_placement.h): R0-R4 of DESIGN.md section 2 "rebalance" with R1 or R1', row by row.
#include <algorithm>
#include <cstddef>
#include <map>

#define rio_gp_set_nodes stub_base_set_nodes
#include "stub_rio_gp_index.cpp"  // (which includes stub_rio_gp.cpp): the reverse index as well
#undef rio_gp_set_nodes

static std::mutex g_caps_mu;
static std::map<const rio_gp*, std::vector<uint64_t>> g_caps;

extern "C" int rio_gp_set_nodes(rio_gp_t* h, uint32_t m, const uint64_t* cap, const uint8_t* alive) {
    {
        std::lock_guard<std::mutex> g(g_caps_mu);
        auto& c = g_caps[h];
        c.assign(m, RIO_GP_CAP_INF);
        if (cap && m) memcpy(c.data(), cap, (size_t)m * sizeof(uint64_t));
    }
    return stub_base_set_nodes(h, m, cap, alive);
}

static uint32_t wf_class(uint64_t f) {
    const uint32_t e = 63u - (uint32_t)__builtin_clzll(f);
    const uint32_t mant = e >= 2 ? (uint32_t)(f >> (e - 2)) & 3u : (uint32_t)(f << (2 - e)) & 3u;
    return e * 4u + mant;
}

extern "C" int rio_gp_rebalance(rio_gp_t* h, const rio_gp_rebalance_cfg* cfg, rio_gp_rebalance_stats* st, uint32_t* out_rows,
                                uint32_t* out_from, uint32_t* out_to, uint64_t moves_cap, uint64_t* n_moves) {
    if (!h || !cfg || cfg->rounds > 8) return RIO_GP_EINVAL;
    uint32_t order = RIO_GP_REBALANCE_ROW_ORDER;
    if (cfg->struct_size == sizeof(rio_gp_rebalance_cfg)) {
        if (cfg->order > RIO_GP_REBALANCE_BY_LOAD || cfg->reserved) return RIO_GP_EINVAL;
        order = cfg->order;
    } else if (cfg->struct_size != offsetof(rio_gp_rebalance_cfg, order)) {
        return RIO_GP_EINVAL;
    }
    if ((out_rows != nullptr) != (out_from != nullptr) || (out_rows != nullptr) != (out_to != nullptr) || (!out_rows && moves_cap))
        return RIO_GP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    const uint32_t m = (uint32_t)h->alive.size();
    std::vector<uint64_t> T(m, RIO_GP_CAP_INF);
    if (cfg->target) {
        memcpy(T.data(), cfg->target, (size_t)m * sizeof(uint64_t));
    } else {
        std::lock_guard<std::mutex> gc(g_caps_mu);
        const auto& c = g_caps[h];
        for (uint32_t j = 0; j < m && j < c.size(); ++j) T[j] = c[j];
    }
    const uint32_t rounds = cfg->rounds ? cfg->rounds : 2;
    const uint64_t B = out_rows ? std::min(cfg->max_moves, moves_cap) : cfg->max_moves;
    auto live = [&](uint32_t j) { return j < m && h->alive[j]; };
    rio_gp_rebalance_stats s{};
    std::vector<uint64_t> pin(m, 0), used(m, 0);
    std::vector<std::vector<uint64_t>> cands(m);
    for (uint64_t i = 0; i < h->n; ++i) {
        const uint32_t c = h->assign[i];
        if (c < m) used[c] += h->load[i];
        if (!live(c)) continue;
        if (h->aff[i] == RIO_GP_AFF_INACTIVE) pin[c] += h->load[i];
        else cands[c].push_back(i);
    }
    for (uint32_t j = 0; j < m; ++j) s.nodes_over_before += live(j) && used[j] > T[j];
    // R1 / R1': the candidates of a node in the order of the rule; the first whose inclusive prefix passes free and all later
    std::vector<uint64_t> surplus;
    for (uint32_t j = 0; j < m; ++j) {
        auto& cj = cands[j];
        if (order == RIO_GP_REBALANCE_BY_LOAD)
            std::stable_sort(cj.begin(), cj.end(), [&](uint64_t a, uint64_t b) { return h->load[a] < h->load[b]; });
        const uint64_t fr = T[j] > pin[j] ? T[j] - pin[j] : 0;
        uint64_t run = 0;
        bool over = false;
        for (uint64_t i : cj) {
            run += h->load[i];
            over = over || run > fr;
            if (over) surplus.push_back(i);
        }
    }
    std::sort(surplus.begin(), surplus.end());
    // R2: the first B in row order
    std::vector<uint64_t> sel;
    for (uint64_t i : surplus) {
        ++s.surplus_rows;
        s.surplus_load += h->load[i];
        if (sel.size() < B) { sel.push_back(i); s.selected_load += h->load[i]; used[h->assign[i]] -= h->load[i]; }
    }
    s.selected_rows = sel.size();
    // R3
    std::vector<uint32_t> nxt(sel.size(), RIO_GP_NONE);
    for (uint32_t r = 0; r < rounds; ++r) {
        std::vector<uint32_t> ord;
        std::vector<uint64_t> fr(m, 0);
        for (uint32_t j = 0; j < m; ++j)
            if (live(j) && T[j] > used[j]) { fr[j] = T[j] - used[j]; ord.push_back(j); }
        std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return wf_class(fr[a]) > wf_class(fr[b]); });
        std::vector<uint64_t> C(ord.size() + 1, 0);
        for (size_t k = 0; k < ord.size(); ++k) C[k + 1] = C[k] + fr[ord[k]] < C[k] ? RIO_GP_CAP_INF : C[k] + fr[ord[k]];
        uint64_t Q = 0;
        std::vector<std::pair<uint32_t, uint32_t>> placed;
        for (size_t k = 0; k < sel.size(); ++k) {
            if (nxt[k] != RIO_GP_NONE) continue;
            const uint32_t l = h->load[sel[k]];
            if (!ord.empty() && Q < C.back()) {
                const size_t at = (size_t)(std::upper_bound(C.begin(), C.begin() + ord.size(), Q) - C.begin()) - 1;
                if (Q + l <= C[at + 1]) { nxt[k] = ord[at]; placed.emplace_back(ord[at], l); }
            }
            Q += l;
        }
        for (auto& p : placed) used[p.first] += p.second;
    }
    // R4 + the column + the moves
    uint64_t nm = 0;
    for (size_t k = 0; k < sel.size(); ++k) {
        const uint32_t from = h->assign[sel[k]];
        if (nxt[k] == RIO_GP_NONE) { ++s.stayed_rows; used[from] += h->load[sel[k]]; continue; }
        if (nxt[k] == from) continue;
        h->assign[sel[k]] = nxt[k];
        ++s.moved_rows;
        s.moved_load += h->load[sel[k]];
        if (out_rows) { out_rows[nm] = (uint32_t)sel[k]; out_from[nm] = from; out_to[nm] = nxt[k]; }
        ++nm;
    }
    for (uint32_t j = 0; j < m; ++j) s.nodes_over_after += live(j) && used[j] > T[j];
    if (n_moves) *n_moves = nm;
    if (st) *st = s;
    return RIO_GP_OK;
}
