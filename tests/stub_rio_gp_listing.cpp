// stub_rio_gp_listing.cpp — TEST INFRASTRUCTURE ONLY: the host-memory stub of the dense C ABI with the dense call of every one of
// the string layer's six key-listing functions in one translation unit, for tests/host_layer_listing_driver.cpp.  The expiry stub
// brings the reverse index, the rebalance, the change feed and node removal with it; the hot-object stub's own include of the base
// stub falls away (its include guard).
#include "stub_rio_gp_expire.cpp"
#include "stub_rio_gp_top.cpp"
