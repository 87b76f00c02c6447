// rt_raysort.hpp — the coherence key of a caller ray, one definition for the key
// kernel (rt_raysort.hip) and for rt_ray_keys_host / rt_ray_sort_host, which pin it on the CPU.
// Exact float32: every operation below is one IEEE operation in the order written (the build's
// -ffp-contract=off, correctly rounded / and sqrtf), so host and device keys agree bit for bit.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace rts {

constexpr int MODE_ORIGIN = 0, MODE_ORIGIN_DIR = 1;  // RT_SORT_ORIGIN, RT_SORT_ORIGIN_DIR
constexpr int MAX_BITS_ORIGIN = 10, MAX_BITS_ORIGIN_DIR = 5;

// Bits of the key: 3b (origin) or 6b (origin, then direction); 0 for a mode or b outside the table.
__host__ __device__ __forceinline__ int key_bits(int mode, int bits) {
    if (mode == MODE_ORIGIN) return bits >= 1 && bits <= MAX_BITS_ORIGIN ? 3 * bits : 0;
    if (mode == MODE_ORIGIN_DIR) return bits >= 1 && bits <= MAX_BITS_ORIGIN_DIR ? 6 * bits : 0;
    return 0;
}

// The cell of t = (position in [0, 1)) * 2^b on a 2^b grid: clamped to [0, 2^b - 1], NaN to 0.
// top = 2^b - 1 as a float.
__host__ __device__ __forceinline__ uint32_t clamp_cell(float t, float top) {
    float q = (t >= 0.0f) ? t : 0.0f;
    q = (q <= top) ? q : top;
    return (uint32_t)q;
}

// A coordinate's cell in [lo, hi]: a flat axis gives 0 / 0 -> cell 0 and x / 0 -> the last cell
// (the first for x < lo), defined, not an error.
__host__ __device__ __forceinline__ uint32_t coord_cell(float x, float lo, float hi, float scale, float top) {
    return clamp_cell(((x - lo) / (hi - lo)) * scale, top);
}

// A unit direction component's cell: u in [-1, 1] onto [0, 2^b].
__host__ __device__ __forceinline__ uint32_t dir_cell(float u, float scale, float top) {
    return clamp_cell((u + 1.0f) * 0.5f * scale, top);
}

// From the cells' most significant bit down, that bit of each cell in the order given (x leads,
// as in the LBVH's Morton code).
template <int N>
__host__ __device__ __forceinline__ uint32_t interleave(const uint32_t (&cell)[N], int bits) {
    uint32_t key = 0;
    for (int j = bits - 1; j >= 0; --j) {
#pragma unroll
        for (int c = 0; c < N; ++c) key = (key << 1) | ((cell[c] >> j) & 1u);
    }
    return key;
}

// The key of the ray r[0..5] (origin, direction) in the box b[0..5] (min corner, max corner);
// mode and bits are valid (key_bits(mode, bits) != 0).
__host__ __device__ __forceinline__ uint32_t ray_key(const float* r, const float* b, int mode, int bits) {
    const float scale = (float)(1u << bits), top = (float)((1u << bits) - 1u);
    if (mode == MODE_ORIGIN) {
        const uint32_t cell[3] = {coord_cell(r[0], b[0], b[3], scale, top), coord_cell(r[1], b[1], b[4], scale, top),
                                  coord_cell(r[2], b[2], b[5], scale, top)};
        return interleave(cell, bits);
    }
    const float len = sqrtf(r[3] * r[3] + r[4] * r[4] + r[5] * r[5]);
    const uint32_t cell[6] = {coord_cell(r[0], b[0], b[3], scale, top), coord_cell(r[1], b[1], b[4], scale, top),
                              coord_cell(r[2], b[2], b[5], scale, top), dir_cell(r[3] / len, scale, top),
                              dir_cell(r[4] / len, scale, top),        dir_cell(r[5] / len, scale, top)};
    return interleave(cell, bits);
}

// floor(u / w) for u < 4096 and 1 <= w <= 16 as (u * inv) >> 16, inv = ceil(2^16 / w): the error
// u * (inv - 2^16 / w) / 2^16 stays below 1/16 <= 1/w (and is 0 for w = 16).
__host__ __device__ __forceinline__ uint32_t div_inv(uint32_t w) { return (65536u + w - 1u) / w; }
__host__ __device__ __forceinline__ uint32_t div_small(uint32_t u, uint32_t inv) { return (u * inv) >> 16; }

}  // namespace rts
