// stub_rio_gp_index.cpp — TEST INFRASTRUCTURE ONLY: the host-memory stub of the dense C ABI (stub_rio_gp.cpp, included as it
// is) plus a host-memory rio_gp_rows_on_nodes, so that the string layer's rio_op_objects_on_server runs without a GPU
// (tests/test_node_index_host.py).  Same contract as the library's (include/rio_gpu_placement.h): the selected nodes' rows of
// the assignment column, ascending, in node order; RIO_GP_ERANGE when they do not fit, offsets and count filled.
#include "stub_rio_gp.cpp"

extern "C" int rio_gp_rows_on_nodes(rio_gp_t* h, const uint64_t* node_bitmap, uint64_t* out_offsets, uint32_t* out_rows,
                                    uint64_t rows_cap, uint64_t* n_rows) {
    if (!h || !out_offsets || !n_rows || (!out_rows && rows_cap)) return RIO_GP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    const uint32_t m = (uint32_t)h->alive.size();
    auto listed = [&](uint32_t a) { return a < m && (!node_bitmap || ((node_bitmap[a >> 6] >> (a & 63)) & 1ull)); };
    std::vector<uint64_t> off(m + 1, 0);
    for (uint64_t i = 0; i < h->n; ++i)
        if (listed(h->assign[i])) ++off[h->assign[i] + 1];
    for (uint32_t j = 0; j < m; ++j) off[j + 1] += off[j];
    memcpy(out_offsets, off.data(), (m + 1) * sizeof(uint64_t));
    *n_rows = off[m];
    if (!out_rows) return RIO_GP_OK;
    if (off[m] > rows_cap) { h->err = "stub: rows_cap too small"; return RIO_GP_ERANGE; }
    for (uint64_t i = 0; i < h->n; ++i)
        if (listed(h->assign[i])) out_rows[off[h->assign[i]]++] = (uint32_t)i;
    return RIO_GP_OK;
}
