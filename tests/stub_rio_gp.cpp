// stub_rio_gp.cpp — TEST INFRASTRUCTURE ONLY: a host-memory stand-in for the dense C ABI (include/rio_gpu_placement.h),
// just enough of it for the string layer (rio-rs_amd/csrc/gpu_object_placement.cpp) to run under ThreadSanitizer on a
// machine without a GPU (tests/test_host_layer_races.py).  It is linked into that one test binary and nowhere else; the
// product library has no CPU path.  Policy = the capacity-free reference policy (service.rs:193-254): sticky if the node
// is alive, else clean_server of the node it sat on and first touch on the requester (alive or, under
// RIO_GP_CFG_REF_SELF_ASSIGN, whatever membership says).  Like the real library it VALIDATES every index against the row count
// and the node table it was given (RIO_GP_EINVAL, nothing mutated) — which is what exposes an id that reaches the
// "device" ahead of the table entry it refers to — and it keeps the row-lifecycle column (RIO_GP_CFG_ROW_LIFECYCLE).
#ifndef STUB_RIO_GP_CPP  // (stub_rio_gp_all.cpp includes the stubs that each include this file: once is enough)
#define STUB_RIO_GP_CPP
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../include/rio_gpu_placement.h"

struct rio_gp {
    std::mutex mu;
    std::vector<uint32_t> assign, aff, load;
    std::vector<uint8_t> alive;
    uint64_t n = 0;
    bool sa = false;  // RIO_GP_CFG_REF_SELF_ASSIGN
    std::string err;
    int fail(const char* m) { err = m; return RIO_GP_EINVAL; }
};

// -DSTUB_LATENCY_US=n (measurement aid, tools/host_layer_scaling.sh): every batched call holds the "device" for n microseconds,
// the way a launch + wait does — the string layer's combiner is then measured against something shaped like a device
#ifdef STUB_LATENCY_US
#include <chrono>
static thread_local bool t_in_mixed = false;  // rio_gp_mixed_batch: ONE round trip for its four parts
static void device_latency() {
    if (t_in_mixed) return;
    const auto t0 = std::chrono::steady_clock::now();
    while (std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(STUB_LATENCY_US)) {}
}
#else
static thread_local bool t_in_mixed = false;
static void device_latency() {}
#endif

extern "C" {
uint32_t rio_gp_abi_version(void) { return RIO_GP_ABI_VERSION; }
const char* rio_gp_last_error(rio_gp_t* h) { return h ? h->err.c_str() : "stub"; }
const char* rio_gp_backend(rio_gp_t*) { return "stub:host (tests only)"; }
int rio_gp_create(const rio_gp_cfg* cfg, rio_gp_t** out) {
    if (!cfg || !out) return RIO_GP_EINVAL;
    rio_gp* h = new rio_gp();
    h->assign.assign(cfg->max_objects, RIO_GP_NONE);
    h->aff.assign(cfg->max_objects, RIO_GP_AFF_INACTIVE);
    h->load.assign(cfg->max_objects, 1);
    h->sa = (cfg->flags & RIO_GP_CFG_REF_SELF_ASSIGN) != 0;
    *out = h;
    return RIO_GP_OK;
}
void rio_gp_destroy(rio_gp_t* h) { delete h; }
int rio_gp_set_flags(rio_gp_t* h, uint32_t flags) {
    std::lock_guard<std::mutex> g(h->mu);
    h->sa = (flags & RIO_GP_CFG_REF_SELF_ASSIGN) != 0;
    return RIO_GP_OK;
}
int rio_gp_set_objects(rio_gp_t* h, uint64_t n, const uint32_t*, const uint32_t*) {
    std::lock_guard<std::mutex> g(h->mu);
    if (n > h->assign.size()) return h->fail("stub: n exceeds max_objects");
    h->n = n;
    return RIO_GP_OK;
}
int rio_gp_set_num_objects(rio_gp_t* h, uint64_t n) {
    std::lock_guard<std::mutex> g(h->mu);
    if (n > h->assign.size()) return h->fail("stub: n exceeds max_objects");
    h->n = n;
    return RIO_GP_OK;
}
int rio_gp_get_objects(rio_gp_t* h, uint64_t n, uint32_t* load, uint32_t* aff) {
    std::lock_guard<std::mutex> g(h->mu);
    if (n != h->n) return h->fail("stub: n differs");
    if (load) memcpy(load, h->load.data(), n * sizeof(uint32_t));
    if (aff) memcpy(aff, h->aff.data(), n * sizeof(uint32_t));
    return RIO_GP_OK;
}
int rio_gp_set_nodes(rio_gp_t* h, uint32_t m, const uint64_t*, const uint8_t* alive) {
    std::lock_guard<std::mutex> g(h->mu);
    h->alive.assign(m, 1);
    if (alive && m) memcpy(h->alive.data(), alive, m);
    return RIO_GP_OK;
}
int rio_gp_set_alive_all(rio_gp_t* h, uint32_t m, const uint8_t* alive) {
    std::lock_guard<std::mutex> g(h->mu);
    if (m != h->alive.size()) return h->fail("stub: m differs from the node table");
    memcpy(h->alive.data(), alive, m);
    return RIO_GP_OK;
}
int rio_gp_lookup_batch(rio_gp_t* h, uint64_t n, const uint32_t* idx, uint32_t* out) {
    std::lock_guard<std::mutex> g(h->mu);
    device_latency();
    for (uint64_t k = 0; k < n; ++k)
        if (idx[k] >= h->n) return h->fail("stub: object index out of range");
    for (uint64_t k = 0; k < n; ++k) out[k] = h->assign[idx[k]];
    return RIO_GP_OK;
}
int rio_gp_update_batch(rio_gp_t* h, uint64_t n, const uint32_t* idx, const uint32_t* node) {
    std::lock_guard<std::mutex> g(h->mu);
    device_latency();
    for (uint64_t k = 0; k < n; ++k)
        if (idx[k] >= h->n || (node[k] != RIO_GP_NONE && node[k] >= h->alive.size()))
            return h->fail("stub: index or node out of range");
    for (uint64_t k = 0; k < n; ++k) {
        h->assign[idx[k]] = node[k];
        h->aff[idx[k]] = node[k] == RIO_GP_NONE ? RIO_GP_AFF_INACTIVE : node[k];
    }
    return RIO_GP_OK;
}
int rio_gp_remove_batch(rio_gp_t* h, uint64_t n, const uint32_t* idx) {
    std::lock_guard<std::mutex> g(h->mu);
    device_latency();
    for (uint64_t k = 0; k < n; ++k)
        if (idx[k] >= h->n) return h->fail("stub: object index out of range");
    for (uint64_t k = 0; k < n; ++k) { h->assign[idx[k]] = RIO_GP_NONE; h->aff[idx[k]] = RIO_GP_AFF_INACTIVE; }
    return RIO_GP_OK;
}
int rio_gp_clean_server(rio_gp_t* h, uint32_t node, uint64_t* evicted) {
    std::lock_guard<std::mutex> g(h->mu);
    uint64_t ev = 0;
    for (uint64_t i = 0; i < h->n; ++i)
        if (h->assign[i] == node) { h->assign[i] = RIO_GP_NONE; h->aff[i] = RIO_GP_AFF_INACTIVE; ++ev; }
    if (evicted) *evicted = ev;
    return RIO_GP_OK;
}
int rio_gp_count_placed(rio_gp_t* h, uint64_t* out) {
    std::lock_guard<std::mutex> g(h->mu);
    uint64_t c = 0;
    for (uint64_t i = 0; i < h->n; ++i) c += h->assign[i] != RIO_GP_NONE;
    *out = c;
    return RIO_GP_OK;
}
int rio_gp_set_object_attrs(rio_gp_t* h, uint64_t n, const uint32_t* idx, const uint32_t* load, const uint32_t* aff) {
    std::lock_guard<std::mutex> g(h->mu);
    for (uint64_t k = 0; k < n; ++k)
        if (idx[k] >= h->n) return h->fail("stub: object index out of range");
    for (uint64_t k = 0; k < n; ++k) {
        if (load) h->load[idx[k]] = load[k];
        if (aff) h->aff[idx[k]] = aff[k];
    }
    return RIO_GP_OK;
}
int rio_gp_get_assign(rio_gp_t* h, uint64_t n, uint32_t* out) {
    std::lock_guard<std::mutex> g(h->mu);
    if (n != h->n) return h->fail("stub: n differs");
    memcpy(out, h->assign.data(), n * sizeof(uint32_t));
    return RIO_GP_OK;
}
int rio_gp_place_pending(rio_gp_t* h, uint64_t n, const uint32_t* idx, const uint32_t* req, uint32_t* out_node, uint32_t* out_flag) {
    std::lock_guard<std::mutex> g(h->mu);
    device_latency();
    for (uint64_t k = 0; k < n; ++k)
        if (idx[k] >= h->n || req[k] >= h->alive.size()) return h->fail("stub: object index or requester out of range");
    for (uint64_t k = 0; k < n; ++k) {
        uint32_t& a = h->assign[idx[k]];
        const bool up = a != RIO_GP_NONE && a < h->alive.size() && h->alive[a];
        uint32_t fl;
        if (up) fl = a == req[k] ? RIO_GP_FLAG_LOCAL : RIO_GP_FLAG_REDIRECT;
        else {
            uint32_t rep = 0;
            if (a != RIO_GP_NONE) {  // service.rs:227-237: the node it sits on is not alive — clean_server(that node), every object of it
                const uint32_t dead = a;
                rep = RIO_GP_FLAG_REPLACED;
                for (uint64_t i = 0; i < h->n; ++i)
                    if (h->assign[i] == dead) { h->assign[i] = RIO_GP_NONE; h->aff[i] = RIO_GP_AFF_INACTIVE; }
            }
            h->aff[idx[k]] = req[k];
            if (h->alive[req[k]] || h->sa) { a = req[k]; fl = RIO_GP_FLAG_PLACED | rep; }  // service.rs:244-252 asks nobody
            else { a = RIO_GP_NONE; fl = RIO_GP_FLAG_UNPLACED | rep; }
        }
        out_node[k] = a;
        if (out_flag) out_flag[k] = fl;
    }
    return RIO_GP_OK;
}
int rio_gp_mixed_batch(rio_gp_t* h, rio_gp_mixed* ops) {  // the four calls in order; a refused kind changes nothing, the others run
    if (!h || !ops || ops->struct_size < sizeof(rio_gp_mixed)) return RIO_GP_EINVAL;
    if (ops->n_update > 256 || ops->n_remove > 256 || ops->n_lookup > 256 || ops->n_place > 256) return RIO_GP_EINVAL;
    device_latency();
    t_in_mixed = true;
    ops->rc[0] = ops->n_update ? rio_gp_update_batch(h, ops->n_update, ops->update_idx, ops->update_node) : RIO_GP_OK;
    ops->rc[1] = ops->n_remove ? rio_gp_remove_batch(h, ops->n_remove, ops->remove_idx) : RIO_GP_OK;
    ops->rc[2] = ops->n_lookup ? rio_gp_lookup_batch(h, ops->n_lookup, ops->lookup_idx, ops->lookup_out) : RIO_GP_OK;
    ops->rc[3] = ops->n_place ? rio_gp_place_pending(h, ops->n_place, ops->place_idx, ops->place_requester, ops->place_node, ops->place_flag)
                              : RIO_GP_OK;
    t_in_mixed = false;
    return RIO_GP_OK;
}
int rio_gp_tick(rio_gp_t* h, rio_gp_stats* st) {
    std::lock_guard<std::mutex> g(h->mu);
    if (st) memset(st, 0, sizeof *st);
    for (uint64_t i = 0; i < h->n; ++i) {
        uint32_t& a = h->assign[i];
        if (a != RIO_GP_NONE && a < h->alive.size() && h->alive[a]) { if (st) ++st->kept; continue; }
        if (a != RIO_GP_NONE && st) ++st->evicted;
        a = RIO_GP_NONE;
        if (h->aff[i] == RIO_GP_AFF_INACTIVE) continue;                     // not an object
        for (uint32_t j = 0; j < h->alive.size(); ++j)
            if (h->alive[j]) { a = j; break; }
        if (st) { if (a != RIO_GP_NONE) ++st->spilled; else ++st->unplaced; }
    }
    if (st) st->n_objects = st->kept + st->spilled + st->unplaced;
    return RIO_GP_OK;
}
}  // extern "C"
#endif  // STUB_RIO_GP_CPP
