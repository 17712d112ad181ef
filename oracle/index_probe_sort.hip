// Test-only: the product's sort.hip as it stands, compiled with the product's
// flags, plus host accessors for its geometry (the constants sit in an
// anonymous namespace there; the product sources themselves stay untouched,
// so profiles stamped with their hash stay valid).
#include "sort.hip"

namespace rcg {
int os_tile_keys() { return OS_TILE; }
int os_segments() { return OS_SEG; }
}  // namespace rcg
