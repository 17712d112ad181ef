// Test-only: the product's sort.hip as it stands, compiled with the product's
// flags, plus host accessors for the main index's geometry (the constants sit
// in an anonymous namespace there; the product source stays untouched).
#include "sort.hip"

namespace rcg {
int isp_tile_keys() { return OS_TILE; }      // keys per tile of a global pass
int isp_local_cap() { return LS_CAP; }       // keys a range-local workgroup holds
int isp_list_len() { return LS_LIST; }       // oversized ranges the list holds
int isp_gbits_max() { return IX_GMAX; }      // most bits the global passes partition on
}  // namespace rcg
