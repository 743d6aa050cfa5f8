// stub_rio_gp_classes.cpp — TEST INFRASTRUCTURE ONLY: the host-memory stub of the dense C ABI with idle expiry
// (stub_rio_gp_expire.cpp and what it includes) plus a host double of the object-class calls the string layer uses:
// rio_gp_set_classes, rio_gp_set_class_batch, rio_gp_get_classes, rio_gp_expire_classes and rio_gp_census, so that
// rio_op_set_type_idle_limit_n / rio_op_expire_by_type / rio_op_census run without a GPU (tests/test_classes_host.py, the
// ThreadSanitizer driver tests/host_layer_race_driver_classes.cpp).  Same contract as the library's (include/rio_gpu_placement.h,
// DESIGN.md section 2 rule 12): a class column K per handle, 0 to begin with; row r < n is idle iff assign[r] != RIO_GP_NONE and
// K[r] < n_classes and S[r] < cutoffs[K[r]].  Like S, K lives in a side map: a handle the expiry stub has no S entry for is a new
// one (its rio_gp_create erases the entry), so its K starts over too.
#include "stub_rio_gp_expire.cpp"

static std::map<const rio_gp*, std::vector<uint8_t>> g_cls;

static std::vector<uint8_t>& cls_of(rio_gp* h) {  // (g_seen_mu held)
    if (!g_seen.count(h)) g_cls.erase(h);  // (a handle freed earlier lived at this address)
    seen_of(h);
    std::vector<uint8_t>& k = g_cls[h];
    if (k.size() != h->assign.size()) k.assign(h->assign.size(), 0);
    return k;
}

extern "C" int rio_gp_set_classes(rio_gp_t* h, uint64_t first_row, uint64_t rows, const uint8_t* cls) {
    if (!h || (rows && !cls)) return RIO_GP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (first_row > h->n || rows > h->n - first_row) return h->fail("stub: the range exceeds the object table");
    std::lock_guard<std::mutex> gs(g_seen_mu);
    std::vector<uint8_t>& K = cls_of(h);
    for (uint64_t k = 0; k < rows; ++k) K[first_row + k] = cls[k];
    return RIO_GP_OK;
}

extern "C" int rio_gp_set_class_batch(rio_gp_t* h, uint64_t n, const uint32_t* idx, const uint8_t* cls) {
    if (!h || (n && (!idx || !cls))) return RIO_GP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    for (uint64_t k = 0; k < n; ++k)
        if (idx[k] >= h->n) return h->fail("stub: object index out of range");
    std::lock_guard<std::mutex> gs(g_seen_mu);
    std::vector<uint8_t>& K = cls_of(h);
    for (uint64_t k = 0; k < n; ++k) K[idx[k]] = cls[k];  // (in order: the last entry of a row wins)
    return RIO_GP_OK;
}

extern "C" int rio_gp_get_classes(rio_gp_t* h, uint64_t n, uint8_t* out) {
    if (!h || !out) return RIO_GP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (n != h->n) return h->fail("stub: n differs from the object table");
    std::lock_guard<std::mutex> gs(g_seen_mu);
    const std::vector<uint8_t>& K = cls_of(h);
    for (uint64_t r = 0; r < n; ++r) out[r] = K[r];
    return RIO_GP_OK;
}

extern "C" int rio_gp_expire_classes(rio_gp_t* h, uint32_t n_classes, const uint32_t* cutoffs, uint32_t* out_rows,
                                     uint32_t* out_node, uint64_t cap, uint64_t* n_idle, uint64_t* load_freed,
                                     uint64_t* idle_by_class) {
    if (!h) return RIO_GP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (n_classes < 1 || n_classes > RIO_GP_MAX_CLASSES || !cutoffs) return h->fail("stub: 1 .. RIO_GP_MAX_CLASSES cutoffs are needed");
    if (!n_idle) return h->fail("stub: n_idle is NULL");
    if ((out_rows != nullptr) != (out_node != nullptr) || (!out_rows && cap))
        return h->fail("stub: out_rows / out_node are given together or not at all");
    std::lock_guard<std::mutex> gs(g_seen_mu);
    const std::vector<uint8_t>& K = cls_of(h);
    const std::vector<uint32_t>& S = seen_of(h);
    uint64_t total = 0, freed = 0;
    if (idle_by_class)
        for (uint32_t c = 0; c < n_classes; ++c) idle_by_class[c] = 0;
    for (uint64_t r = 0; r < h->n; ++r) {
        if (h->assign[r] == RIO_GP_NONE || K[r] >= n_classes || S[r] >= cutoffs[K[r]]) continue;
        if (idle_by_class) ++idle_by_class[K[r]];
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

extern "C" int rio_gp_census(rio_gp_t* h, uint32_t flags, uint32_t n_classes, uint64_t* out_rows, uint64_t* out_load,
                             uint64_t* n_other) {
    if (!h) return RIO_GP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (flags & ~RIO_GP_CENSUS_BY_NODE) return h->fail("stub: unknown flags");
    if (n_classes < 1 || n_classes > RIO_GP_MAX_CLASSES) return h->fail("stub: n_classes out of range");
    if (!out_rows || !out_load || !n_other) return h->fail("stub: out_rows, out_load and n_other are needed");
    const bool by_node = flags & RIO_GP_CENSUS_BY_NODE;
    const uint64_t m = h->alive.size();
    if (by_node && m * n_classes > (1ull << 20)) return h->fail("stub: more than 2^20 cells");
    std::lock_guard<std::mutex> gs(g_seen_mu);
    const std::vector<uint8_t>& K = cls_of(h);
    const uint64_t cells = (by_node ? m : 1) * n_classes;
    for (uint64_t c = 0; c < cells; ++c) out_rows[c] = out_load[c] = 0;
    *n_other = 0;
    for (uint64_t r = 0; r < h->n; ++r) {
        const uint32_t a = h->assign[r];
        if (a == RIO_GP_NONE) continue;
        if (K[r] >= n_classes || (by_node && a >= m)) { ++*n_other; continue; }
        const uint64_t cell = (by_node ? (uint64_t)a * n_classes : 0) + K[r];
        out_rows[cell] += 1;
        out_load[cell] += h->load[r];
    }
    return RIO_GP_OK;
}
