// rt_film.hpp — the film's per-pixel arithmetic, shared by the film kernels
// (rt_frame.hip) and by rt_film_pixels_host, which pins it on the CPU.
// render()'s pixel (G/include/query.cu:130-166): col = col + sample in sample order in float, then
// col / float(spp), Vec3 / double: the double quotient rounded to float (vec3.h:334).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rtf {

// The running sum after samples at(0), at(1), ..., at(n - 1), added in that order.  Float adds
// only: the order is the result.
template <class At>
__host__ __device__ __forceinline__ float film_sum(float sum, int n, At at) {
    for (int s = 0; s < n; ++s) sum = sum + at(s);
    return sum;
}

// The pixel of a sum of `count` samples; fcount = float(count).
__host__ __device__ __forceinline__ float film_pixel(float sum, float fcount) {
    return (float)((double)sum / (double)fcount);
}

// The staged image of film_add_vec_kernel: one spare dword after every 32, so that lanes whose
// addresses differ by a pixel's 3n dwords spread over the 32 banks of dword reads and writes.
__host__ __device__ __forceinline__ uint32_t film_lds_index(uint32_t i) { return i + (i >> 5); }

}  // namespace rtf
