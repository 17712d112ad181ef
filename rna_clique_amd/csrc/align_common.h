// What extend.hip and rows.hip share: the block size of extend_kernel and the
// row kernels, and the grid both launch with.
#pragma once
#include "device.h"

namespace rcg {

constexpr int EBLOCK = 256;

// One resident wave per SIMD slot: a grid past the resident capacity leaves a
// partial second round of waves (static per-row work runs at low occupancy).
template <typename K>
static unsigned resident_blocks(K kernel, size_t lds)
{
    int dev = 0, cus = 256, per_cu = 1;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
        cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, EBLOCK, lds) != hipSuccess || per_cu < 1)
        per_cu = 1;
    return (unsigned)(cus * per_cu);
}

}  // namespace rcg
