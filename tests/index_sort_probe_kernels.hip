// Test-only: the product's kernels.hip as it stands, compiled with the
// product's flags (pack, fill and the whole-table bucket fill for the probe).
#include "kernels.hip"
