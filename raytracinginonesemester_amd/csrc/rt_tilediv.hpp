// rt_tilediv.hpp — a tile index's column and row without a division: the render kernels split
// every work item's tile by tiles_x, a value the host knows when it fills RenderParams, and an
// integer division by a run-time value is some twenty instructions on gfx950.  One definition
// for the host (which makes the constant), the kernels and tests/native/tilediv_main.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rtd {

// floor(n / d) for 0 <= n < 2^31 and 1 <= d <= 2^31 as (mulhi(n, mul) + n) >> shift, where
// shift = ceil(log2 d) and 2^32 + mul = floor(2^(32 + shift) / d) + 1 (round-up method, Granlund
// & Montgomery 1994).  With M = 2^32 + mul, M * d = 2^(32 + shift) + e for some 0 < e <= d <=
// 2^shift, so n * M / 2^(32 + shift) = n / d + n * e / (d * 2^(32 + shift)), and the second term
// is below 1 / d for n < 2^32: the floor is n / d's.  n < 2^31 keeps mulhi(n, mul) + n, which is
// floor(n * M / 2^32), inside 32 bits.
struct TileDiv {
    uint32_t mul, shift;
};

__host__ __device__ __forceinline__ TileDiv tile_div_make(uint32_t d) {
    uint32_t l = 0;
    while (l < 31 && (1u << l) < d) ++l;
    const uint64_t M = (uint64_t(1) << (32 + l)) / d + 1;  // in [2^32 + 1, 2^33)
    return TileDiv{(uint32_t)(M - (uint64_t(1) << 32)), l};
}

__host__ __device__ __forceinline__ uint32_t tile_div(uint32_t n, TileDiv t) {
    return ((uint32_t)(((uint64_t)n * t.mul) >> 32) + n) >> t.shift;
}

}  // namespace rtd
