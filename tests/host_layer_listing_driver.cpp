// host_layer_listing_driver.cpp — TEST INFRASTRUCTURE ONLY: the string layer (gpu_object_placement.cpp) over the host-memory
// stub with every optional dense call (stub_rio_gp_listing.cpp), built with AddressSanitizer.  It pins the one rule the six
// key-listing calls share (include/rio_gpu_object_placement.h): the arrays a call hands out are the calling thread's until its
// next call of THAT function — whatever else the thread calls meanwhile, and whatever other threads call.
//   A  a listing of each of the six, copied; then the other five, every single-object call and a rio_op_remove_members (which
//      rebuilds the node id table) on the same thread: the listing still reads byte for byte what was copied
//   B  the same listing taken on a second thread meanwhile: the first thread's is unchanged, the second's arrays are others
//   C  rio_op_snapshot_key_lengths describes the calling thread's last snapshot; a thread without one gets RIO_GP_OK
//   D  a failing call leaves the n_out it set at 0, and a later call lists correctly
// With the argument "plain" the program is linked over the plain stub (stub_rio_gp.cpp, no optional call) and runs D's
// RIO_GP_EUPSTREAM case only.  A read of a string that was freed or moved is AddressSanitizer's finding and fails the run.
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../include/rio_gpu_object_placement.h"

static long g_wrong = 0;
#define CHECK(c) \
    do { \
        if (!(c)) { ++g_wrong; fprintf(stderr, "line %d: %s\n", __LINE__, #c); } \
    } while (0)

constexpr int kKeys = 40;  // max_objects is one more: a second new key finds the table full and makes the layer reclaim rows
enum Which { SNAPSHOT, ON_SERVER, REBALANCE, CHANGES, EXPIRE, HOTTEST, kCalls };

static std::string key_id(int k) {  // every fourth id holds a NUL byte
    std::string id = "id";
    if (k % 4 == 1) id.push_back('\0');
    return id + std::to_string(k);
}

// what a listing call handed out: the caller's view of the arrays (columns the call does not have stay NULL)
struct View {
    uint64_t n = 77;  // (a call that sets *n_out sets it whatever it finds here)
    const char* const* ty = nullptr;
    const char* const* id = nullptr;
    const char* const* a0 = nullptr;
    const char* const* a1 = nullptr;
    const size_t* tl = nullptr;
    const size_t* il = nullptr;
};
struct Entry {
    std::string ty, id, a0, a1;
    bool has0 = false, has1 = false;
};

static int take(rio_op_t* p, int which, View& v) {
    uint32_t loads[8];
    int full = 0;
    switch (which) {
        case SNAPSHOT: {
            const int rc = rio_op_snapshot(p, &v.n, &v.ty, &v.id, &v.a0);
            return rc ? rc : rio_op_snapshot_key_lengths(p, &v.tl, &v.il);
        }
        case ON_SERVER: return rio_op_objects_on_server(p, "s0:1", &v.n, &v.ty, &v.tl, &v.id, &v.il);
        case REBALANCE: return rio_op_rebalance(p, 6, &v.n, &v.ty, &v.tl, &v.id, &v.il, &v.a0, &v.a1);
        case CHANGES: return rio_op_changes(p, &v.n, &full, &v.ty, &v.tl, &v.id, &v.il, &v.a0, &v.a1);
        case EXPIRE: return rio_op_expire(p, 1000000u, 5, &v.n, nullptr, &v.ty, &v.tl, &v.id, &v.il, &v.a0);
        default: return rio_op_hottest_objects(p, nullptr, 0, 8, &v.n, nullptr, &v.ty, &v.tl, &v.id, &v.il, &v.a0, loads);
    }
}

static std::vector<Entry> copy_of(const View& v) {
    std::vector<Entry> out(v.n);
    for (uint64_t k = 0; k < v.n; ++k) {
        Entry& e = out[k];
        e.ty.assign(v.ty[k], v.tl[k]);
        e.id.assign(v.id[k], v.il[k]);
        if ((e.has0 = v.a0 && v.a0[k])) e.a0 = v.a0[k];
        if ((e.has1 = v.a1 && v.a1[k])) e.a1 = v.a1[k];
    }
    return out;
}

// the arrays read again, pointer by pointer and byte by byte, against the copy
static bool same(const View& v, const std::vector<Entry>& c) {
    if (v.n != c.size()) return false;
    for (uint64_t k = 0; k < v.n; ++k) {
        const Entry& e = c[k];
        if (v.tl[k] != e.ty.size() || memcmp(v.ty[k], e.ty.data(), e.ty.size()) || v.ty[k][v.tl[k]] != 0) return false;
        if (v.il[k] != e.id.size() || memcmp(v.id[k], e.id.data(), e.id.size()) || v.id[k][v.il[k]] != 0) return false;
        if (v.a0 && (e.has0 != (v.a0[k] != nullptr) || (e.has0 && e.a0 != v.a0[k]))) return false;
        if (v.a1 && (e.has1 != (v.a1[k] != nullptr) || (e.has1 && e.a1 != v.a1[k]))) return false;
    }
    return true;
}

// A table on which every one of the six calls has something to list.  Every key is placed and stamped with a clock below
// expire's cutoff.  All but the last six sit on s0:1, at least six units over its capacity: a rebalance moves some.  The last six
// swap between s1:1 and s2:1 from one round to the next: the feed has changes whatever was called since the last round.
static void prime(rio_op_t* p, int round) {
    CHECK(rio_op_set_clock(p, 10 + (uint32_t)round) == RIO_GP_OK);
    for (int k = 0; k < kKeys; ++k) {
        const std::string id = key_id(k);
        const char* home = k < kKeys - 6 ? "s0:1" : ((k + round) % 2 ? "s1:1" : "s2:1");
        CHECK(rio_op_update_n(p, "T", 1, id.data(), id.size(), home) == RIO_GP_OK);
    }
}

// everything a thread may call between a listing and its next call of the same function
static void everything_else(rio_op_t* p, int held, int round) {
    char buf[64];
    int found = 0;
    uint32_t flag = 0, load = 0;
    uint64_t n = 0, removed = 0, evicted = 0;
    for (int w = 0; w < kCalls; ++w) {
        if (w == held) continue;
        View v;
        CHECK(take(p, w, v) == RIO_GP_OK);
        CHECK(v.n > 0 && v.n != 77);
    }
    prime(p, round);  // (expire and rebalance changed the table: the single-object calls below find every key placed)
    // an address never seen holds nothing
    View none;
    if (held != ON_SERVER) CHECK(rio_op_objects_on_server(p, "never:1", &none.n, &none.ty, &none.tl, &none.id, &none.il) == RIO_GP_OK);
    if (held != ON_SERVER) CHECK(none.n == 0);
    if (held != HOTTEST)
        CHECK(rio_op_hottest_objects(p, "never:1", 0, 4, &none.n, nullptr, &none.ty, &none.tl, &none.id, &none.il, &none.a0, &load) == RIO_GP_OK);
    if (held != HOTTEST) CHECK(none.n == 0);
    // the single-object calls, keys with a NUL byte among them
    for (int k = 0; k < kKeys; k += 3) {
        const std::string id = key_id(k);
        CHECK(rio_op_lookup_n(p, "T", 1, id.data(), id.size(), buf, sizeof buf, &found) == RIO_GP_OK && found);
        const int rt = rio_op_try_lookup_n(p, "T", 1, id.data(), id.size(), buf, sizeof buf, &found);
        CHECK(rt == RIO_GP_OK || rt == RIO_GP_EAGAIN);
        CHECK(rio_op_get_or_create_placement_n(p, "T", 1, id.data(), id.size(), "s1:1", buf, sizeof buf, &flag) == RIO_GP_OK);
        const int rg = rio_op_try_get_or_create_placement_n(p, "T", 1, id.data(), id.size(), "s1:1", buf, sizeof buf, &flag);
        CHECK(rg == RIO_GP_OK || rg == RIO_GP_EAGAIN);
        CHECK(rio_op_set_object_load_n(p, "T", 1, id.data(), id.size(), 2 + (uint32_t)(k % 5)) == RIO_GP_OK);
        CHECK(rio_op_get_object_load(p, "T", 1, id.data(), id.size(), &load, &found) == RIO_GP_OK && found);
    }
    // two keys go and two new ones come: the table is full, so their rows are reclaimed and handed on (retired rows in the feed)
    for (int k = 0; k < 2; ++k) {
        const std::string old_id = key_id(2 + k), new_id = "fresh" + std::to_string(round) + "." + std::to_string(k);
        CHECK(rio_op_remove_n(p, "T", 1, old_id.data(), old_id.size()) == RIO_GP_OK);
        CHECK(rio_op_update(p, "U", new_id.c_str(), "s2:1") == RIO_GP_OK);
        CHECK(rio_op_remove(p, "U", new_id.c_str()) == RIO_GP_OK);
        CHECK(rio_op_update_n(p, "T", 1, old_id.data(), old_id.size(), "s0:1") == RIO_GP_OK);
    }
    CHECK(rio_op_len(p, &n) == RIO_GP_OK && n == (uint64_t)kKeys);
    CHECK(rio_op_invalidate_cache(p) == RIO_GP_OK);
    // a server none of the listings holds comes, is cleaned and is removed: the node id table is rebuilt
    const std::string guest = "guest" + std::to_string(round) + ":9";
    const char* guests[1] = {guest.c_str()};
    CHECK(rio_op_set_member(p, guest.c_str(), 1, RIO_GP_CAP_INF) == RIO_GP_OK);
    CHECK(rio_op_update(p, "T", "visitor", guest.c_str()) == RIO_GP_OK);
    CHECK(rio_op_clean_server(p, guest.c_str()) == RIO_GP_OK);
    CHECK(rio_op_remove_members(p, 1, guests, &removed, &evicted) == RIO_GP_OK && removed == 1);
    CHECK(rio_op_node_address(p, 0) != nullptr);
}

static void check_a_b(rio_op_t* p) {
    int round = 0;
    for (int w = 0; w < kCalls; ++w) {
        prime(p, ++round);
        View mine;
        CHECK(take(p, w, mine) == RIO_GP_OK);
        CHECK(mine.n > 0 && mine.n != 77);
        const std::vector<Entry> copy = copy_of(mine);
        // A: the thread's other calls
        everything_else(p, w, ++round);
        CHECK(same(mine, copy));
        everything_else(p, w, ++round);  // (twice: the other listings' own buffers are reused, grown and shrunk)
        CHECK(same(mine, copy));
        // B: the same call on another thread
        prime(p, ++round);
        View theirs;
        bool theirs_ok = false;
        std::thread other([&] {
            theirs_ok = take(p, w, theirs) == RIO_GP_OK && theirs.n > 0 && same(theirs, copy_of(theirs));
        });
        other.join();
        CHECK(theirs_ok);
        CHECK(theirs.ty != mine.ty && theirs.id != mine.id && theirs.tl != mine.tl && theirs.il != mine.il);  // (not read: gone)
        CHECK(same(mine, copy));
        if (g_wrong) fprintf(stderr, "... after listing call %d\n", w);
    }
}

static void check_c(rio_op_t* p) {
    prime(p, 100);
    View v;
    CHECK(take(p, SNAPSHOT, v) == RIO_GP_OK);
    CHECK(v.n == (uint64_t)kKeys);
    std::vector<int> seen(kKeys, 0);
    for (uint64_t k = 0; k < v.n && k < (uint64_t)kKeys; ++k) {
        const std::string id(v.id[k], v.il[k]);
        int which = -1;
        for (int q = 0; q < kKeys; ++q)
            if (id == key_id(q)) which = q;
        CHECK(which >= 0 && !seen[which < 0 ? 0 : which]++);
        CHECK(v.tl[k] == 1 && strlen(v.ty[k]) == 1 && v.ty[k][0] == 'T');
        // a key without a NUL byte has its strlen; one with a NUL byte is longer than that
        CHECK(which < 0 || (which % 4 == 1 ? strlen(v.id[k]) == 2 && v.il[k] > 3 : strlen(v.id[k]) == v.il[k]));
        CHECK(v.a0[k] && (!strcmp(v.a0[k], "s0:1") || !strcmp(v.a0[k], "s1:1") || !strcmp(v.a0[k], "s2:1")));
    }
    // the lengths are the calling thread's last snapshot's, also after the thread's other listing calls
    View other;
    CHECK(take(p, ON_SERVER, other) == RIO_GP_OK);
    const size_t* tl = nullptr;
    const size_t* il = nullptr;
    CHECK(rio_op_snapshot_key_lengths(p, &tl, &il) == RIO_GP_OK);
    for (uint64_t k = 0; k < v.n; ++k) CHECK(tl[k] == v.tl[k] && il[k] == v.il[k]);
    // a thread that never took a snapshot: RIO_GP_OK (it has no entries for the arrays to describe: they are not read)
    int rc = -1;
    std::thread fresh([&] {
        const size_t* a = nullptr;
        const size_t* b = nullptr;
        rc = rio_op_snapshot_key_lengths(p, &a, &b);
    });
    fresh.join();
    CHECK(rc == RIO_GP_OK);
}

// D over the full stub: a call refused for its arguments after it has set *n_out
static void check_d_einval(rio_op_t* p) {
    View v;
    uint64_t cand = 77;
    uint32_t loads[1];
    CHECK(rio_op_hottest_objects(p, nullptr, 0, (uint64_t)RIO_GP_TOP_MAX + 1, &v.n, &cand, &v.ty, &v.tl, &v.id, &v.il, &v.a0, loads) ==
          RIO_GP_EINVAL);
    CHECK(v.n == 0 && cand == 0);
    prime(p, 200);
    View ok;
    CHECK(take(p, HOTTEST, ok) == RIO_GP_OK);
    CHECK(ok.n == 8 && same(ok, copy_of(ok)));
}

// D over the plain stub: the dense layer has no rio_gp_expire
static void check_d_eupstream(rio_op_t* p) {
    prime(p, 1);
    View v;
    uint64_t idle = 77;
    CHECK(rio_op_expire(p, 1000000u, 5, &v.n, &idle, &v.ty, &v.tl, &v.id, &v.il, &v.a0) == RIO_GP_EUPSTREAM);
    CHECK(v.n == 0 && idle == 0);
    CHECK(strstr(rio_op_last_error(p), "idle expiry") != nullptr);
    View snap;
    CHECK(take(p, SNAPSHOT, snap) == RIO_GP_OK);
    CHECK(snap.n == (uint64_t)kKeys && same(snap, copy_of(snap)));
}

int main(int argc, char** argv) {
    rio_op_cfg cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = (uint32_t)sizeof cfg;
    cfg.max_objects = kKeys + 1;
    cfg.max_nodes = 8;
    rio_op_t* p = nullptr;
    if (rio_op_create(&cfg, &p) != RIO_GP_OK) return 2;
    // three servers; s0:1 may hold kKeys - 12 units, six fewer than prime() puts on it
    if (rio_op_set_member(p, "s0:1", 1, kKeys - 12) || rio_op_set_member(p, "s1:1", 1, RIO_GP_CAP_INF) ||
        rio_op_set_member(p, "s2:1", 1, RIO_GP_CAP_INF))
        return 3;
    if (argc > 1 && !strcmp(argv[1], "plain")) {
        check_d_eupstream(p);
    } else {
        check_a_b(p);
        check_c(p);
        check_d_einval(p);
    }
    rio_op_release(p);
    printf("wrong=%ld\n", g_wrong);
    return g_wrong ? 1 : 0;
}
