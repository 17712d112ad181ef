// Test-only: the product's kernels.hip as it stands, compiled with the
// product's flags, plus a host accessor for the bucket fill's entries per
// thread (the product sources themselves stay untouched).
#include "kernels.hip"

namespace rcg {
int bucket_fill_per_thread() { return BF_PER; }
}  // namespace rcg
