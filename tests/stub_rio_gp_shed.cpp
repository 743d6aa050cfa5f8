// stub_rio_gp_shed.cpp — TEST INFRASTRUCTURE ONLY: the host-memory stub of the dense C ABI with idle expiry and object classes
// (stub_rio_gp_classes.cpp and what it includes: the capacities of stub_rio_gp_rebalance.cpp, the last-seen column S, the class
// column K) plus a host double of rio_gp_set_class_movable and of rio_gp_shed_idle, so that the string layer's rio_op_shed_idle
// runs without a GPU (tests/test_shed_host.py).  Same contract as the library's (include/rio_gpu_placement.h, DESIGN.md section
// 2 rule 14), in its sequential form: per live node the candidates in (S descending, row ascending) order, kept while the
// inclusive prefix of their loads stays within T -sat pinned; the first B surplus rows in row order are un-placed (the stub
// always keeps the row lifecycle).  stub_shed_last() hands out the cfg of the last call, for the tests of what goes down.
#include "stub_rio_gp_classes.cpp"

static std::map<const rio_gp*, std::vector<uint8_t>> g_shed_imm;  // (g_seen_mu held) 1: the class is immovable
static rio_gp_shed_cfg g_shed_last_cfg;
static uint32_t g_shed_last_cutoffs[RIO_GP_MAX_CLASSES];

static std::vector<uint8_t>& imm_of(rio_gp* h) {  // (g_seen_mu held)
    if (!g_seen.count(h)) g_shed_imm.erase(h);  // (a handle freed earlier lived at this address)
    seen_of(h);
    std::vector<uint8_t>& t = g_shed_imm[h];
    if (t.size() != RIO_GP_MAX_CLASSES) t.assign(RIO_GP_MAX_CLASSES, 0);
    return t;
}

extern "C" int rio_gp_set_class_movable(rio_gp_t* h, uint32_t n_classes, const uint8_t* movable) {
    if (!h) return RIO_GP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (n_classes > RIO_GP_MAX_CLASSES) return h->fail("stub: n_classes out of range");
    if (n_classes && !movable) return h->fail("stub: no array");
    std::lock_guard<std::mutex> gs(g_seen_mu);
    std::vector<uint8_t>& t = imm_of(h);
    for (uint32_t c = 0; c < RIO_GP_MAX_CLASSES; ++c) t[c] = c < n_classes && !movable[c];
    return RIO_GP_OK;
}

// the last call's cfg: cutoff, max_rows, n_classes and (out256, may be NULL) the class cutoffs it carried
extern "C" void stub_shed_last(uint32_t* cutoff, uint64_t* max_rows, uint32_t* n_classes, uint32_t* out256) {
    *cutoff = g_shed_last_cfg.cutoff;
    *max_rows = g_shed_last_cfg.max_rows;
    *n_classes = g_shed_last_cfg.n_classes;
    if (out256) memcpy(out256, g_shed_last_cutoffs, sizeof g_shed_last_cutoffs);
}

extern "C" int rio_gp_shed_idle(rio_gp_t* h, const rio_gp_shed_cfg* cfg, rio_gp_shed_stats* st, uint32_t* out_rows, uint32_t* out_node,
                                uint64_t rows_cap, uint64_t* n_rows) {
    if (!h) return RIO_GP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (!cfg || cfg->struct_size != sizeof(rio_gp_shed_cfg) || cfg->reserved) return h->fail("stub: bad cfg");
    if (cfg->class_cutoffs ? (cfg->n_classes < 1 || cfg->n_classes > RIO_GP_MAX_CLASSES) : cfg->n_classes != 0)
        return h->fail("stub: n_classes does not fit class_cutoffs");
    if ((out_rows != nullptr) != (out_node != nullptr) || (!out_rows && rows_cap))
        return h->fail("stub: out_rows / out_node are given together or not at all");
    std::lock_guard<std::mutex> gs(g_seen_mu);
    g_shed_last_cfg = *cfg;
    memset(g_shed_last_cutoffs, 0, sizeof g_shed_last_cutoffs);
    if (cfg->class_cutoffs) memcpy(g_shed_last_cutoffs, cfg->class_cutoffs, cfg->n_classes * sizeof(uint32_t));
    const std::vector<uint32_t>& S = seen_of(h);
    const std::vector<uint8_t>& K = cls_of(h);
    const std::vector<uint8_t>& imm = imm_of(h);
    const uint32_t m = (uint32_t)h->alive.size();
    std::vector<uint64_t> T(m, RIO_GP_CAP_INF), used(m, 0), pinned(m, 0);
    if (cfg->target) {
        memcpy(T.data(), cfg->target, (size_t)m * sizeof(uint64_t));
    } else {
        std::lock_guard<std::mutex> gc(g_caps_mu);
        const auto& c = g_caps[h];
        for (uint32_t j = 0; j < m && j < c.size(); ++j) T[j] = c[j];
    }
    auto cutoff_of = [&](uint64_t r) -> uint32_t {
        if (imm[K[r]]) return 0;
        if (!cfg->class_cutoffs) return cfg->cutoff;
        return K[r] < cfg->n_classes ? cfg->class_cutoffs[K[r]] : 0u;
    };
    std::vector<std::vector<uint32_t>> cand(m);
    for (uint64_t r = 0; r < h->n; ++r) {
        const uint32_t j = h->assign[r];
        if (j >= m) continue;
        used[j] += h->load[r];
        if (!h->alive[j]) continue;
        if (h->aff[r] != RIO_GP_AFF_INACTIVE && h->load[r] >= 1 && S[r] < cutoff_of(r)) cand[j].push_back((uint32_t)r);
        else pinned[j] += h->load[r];
    }
    rio_gp_shed_stats s{};
    std::vector<uint32_t> surplus;
    for (uint32_t j = 0; j < m; ++j) {
        if (!h->alive[j]) continue;
        s.nodes_over_before += used[j] > T[j];
        const uint64_t fr = T[j] > pinned[j] ? T[j] - pinned[j] : 0;
        std::stable_sort(cand[j].begin(), cand[j].end(), [&](uint32_t a, uint32_t b) { return S[a] > S[b]; });
        uint64_t pre = 0;
        bool over = false;
        for (uint32_t r : cand[j]) {
            pre += h->load[r];
            over = over || pre > fr;
            if (over) surplus.push_back(r);
        }
    }
    std::sort(surplus.begin(), surplus.end());
    const uint64_t B = out_rows ? std::min(cfg->max_rows, rows_cap) : cfg->max_rows;
    for (uint32_t r : surplus) {
        s.surplus_rows += 1;
        s.surplus_load += h->load[r];
        if (s.shed_rows >= B) continue;
        if (out_rows) {
            out_rows[s.shed_rows] = r;
            out_node[s.shed_rows] = h->assign[r];
        }
        used[h->assign[r]] -= h->load[r];
        s.shed_rows += 1;
        s.shed_load += h->load[r];
        h->assign[r] = RIO_GP_NONE;
        h->aff[r] = RIO_GP_AFF_INACTIVE;
    }
    for (uint32_t j = 0; j < m; ++j) s.nodes_over_after += h->alive[j] && used[j] > T[j];
    if (n_rows) *n_rows = s.shed_rows;
    if (st) *st = s;
    return RIO_GP_OK;
}
