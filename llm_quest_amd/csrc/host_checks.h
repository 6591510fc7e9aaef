// Host-side pieces that the side kernels' entry points share: the pointer alignment check and the two launch-grid clamps.
// norm_rope.hip keeps a copy of its own: its bytes are part of the step's source fingerprint (fingerprint.kernel_sources_sha).
#pragma once
#include <cstdint>
#include <initializer_list>

// the kernels move 16 bytes at a time: every operand pointer must be 16-byte aligned (NULL passes here and is refused by the null check)
inline bool aligned16(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if ((uintptr_t)p & 15) return false;
    return true;
}
// workgroups of four waves, one row per wave and trip
inline int row_grid(int64_t rows) {
    int64_t g = (rows + 3) / 4;
    return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}
// workgroups of 256 threads, one item per thread and trip
inline int flat_grid(int64_t items) {
    int64_t g = (items + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}
