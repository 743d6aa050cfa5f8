// stub_rio_gp_all.cpp — TEST INFRASTRUCTURE ONLY: the host-memory stub of the dense C ABI with ALL of its optional calls — the
// reverse index (stub_rio_gp_index.cpp), the bounded rebalance (stub_rio_gp_rebalance.cpp) and the change feed
// (stub_rio_gp_changes.cpp) — in one translation unit, for the ThreadSanitizer run of the string layer
// (tests/test_host_layer_races.py).  The rebalance and the feed stubs each wrap one function of the base stub under another
// name; here the base is included once with both renamed, and their own includes of it fall away (its include guard).
#define rio_gp_destroy stub_base_destroy
#define rio_gp_set_nodes stub_base_set_nodes
#include "stub_rio_gp.cpp"
#undef rio_gp_destroy
#undef rio_gp_set_nodes
#include "stub_rio_gp_rebalance.cpp"
#include "stub_rio_gp_changes.cpp"
