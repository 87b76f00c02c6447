// rt_afilm.hpp — the adaptive film's per-pixel arithmetic, shared by the
// kernels of rt_frame.hip and by their host builds (rt_afilm_host, rt_camera_rays_pixels_host),
// which pin it on the CPU.
// A pixel holds render()'s float sums (rt_film.hpp), its own sample count, and two float moments
// of the sample luminance from which the next pass's pixels are chosen.  jittered_samples(k, 42)
// is a prefix of jittered_samples(n, 42) and make_rng_seed does not read spp, so a pixel that got
// samples 0..c-1 in order and is resolved with its own count c is render()'s pixel at spp = c.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rt_film.hpp"
#include "rt_math.hpp"

namespace rtf {

constexpr uint32_t PIXEL_NONE = 0xFFFFFFFFu;  // RT_PIXEL_NONE: a list entry that names no pixel

// The luminance of a sample: float multiplies and adds in this order.
__host__ __device__ __forceinline__ float afilm_luma(float r, float g, float b) {
    return (0.2126f * r + 0.7152f * g) + 0.0722f * b;
}

// m1 = sum of y, m2 = sum of y * y over samples at(0..n-1) in that order (at(s, c): channel c).
template <class At>
__host__ __device__ __forceinline__ void afilm_moments(float& m1, float& m2, int n, At at) {
    for (int s = 0; s < n; ++s) {
        const float y = afilm_luma(at(s, 0), at(s, 1), at(s, 2));
        m1 = m1 + y;
        m2 = m2 + y * y;
    }
}

// The pixel of a sum with the pixel's own count; no samples: 0.
__host__ __device__ __forceinline__ float afilm_pixel(float sum, uint32_t count) {
    return count == 0u ? 0.0f : film_pixel(sum, (float)count);
}

struct SelectOpts {
    int32_t min_samples, max_samples, step;
    double tol, floor;
};

// Is the mean of n samples still uncertain?  In double from the float accumulators, with + - * /,
// max and comparisons only (no sqrt, no fma: the builds agree under -ffp-contract=off):
//   mean = m1 / n;  var = (max(0, m2 / n - mean * mean) * n) / (n - 1);
//   noisy iff var / n > (tol * max(mean, floor))^2.          n < 2: noisy.
__host__ __device__ __forceinline__ bool afilm_noisy(uint32_t count, float m1, float m2, double tol, double floor) {
    if (count < 2u) return true;
    const double n = (double)count;
    const double mean = (double)m1 / n;
    const double d = (double)m2 / n - mean * mean;
    const double var = ((d > 0.0 ? d : 0.0) * n) / (n - 1.0);
    const double lim = tol * (mean > floor ? mean : floor);
    return var / n > lim * lim;
}

// Does a pixel with `count` samples get `step` more?
__host__ __device__ __forceinline__ bool afilm_selected(uint32_t count, float m1, float m2, const SelectOpts& o) {
    if ((int64_t)count + (int64_t)o.step > (int64_t)o.max_samples) return false;
    return (int64_t)count < (int64_t)o.min_samples || afilm_noisy(count, m1, m2, o.tol, o.floor);
}

// Ray s of list entry `pix` (y * W + x) that already has `count` samples: sample count + s of that
// pixel, Camera::get_ray through camera_dir with that entry of the frame's jitter table (a sample
// past the table reads its last entry) and make_rng_seed(x, y, count + s).  pix >= npix: the null
// ray (origin = center, direction 0, seed 0).  R: 6 floats; seed may be null.
__host__ __device__ __forceinline__ void camera_pixel_ray(rtd::f3 center, rtd::f3 p00, rtd::f3 du, rtd::f3 dv, uint32_t W,
                                                          uint32_t npix, uint32_t pix, uint32_t count, uint32_t s,
                                                          const float* jitter, uint32_t table_spp, float* R, uint32_t* seed) {
    rtd::f3 d = rtd::mk(0.f, 0.f, 0.f);
    uint32_t sd = 0u;
    if (pix < npix) {
        const uint32_t si = count + s;
        const uint32_t j = si < table_spp ? si : table_spp - 1u;
        const uint32_t y = pix / W;
        const int x = (int)(pix - y * W);
        d = rtd::camera_dir(center, p00, du, dv, x, (int)y, jitter[2 * (size_t)j], jitter[2 * (size_t)j + 1]);
        sd = rtd::make_rng_seed(x, (int)y, (int)si);
    }
    R[0] = center.x;
    R[1] = center.y;
    R[2] = center.z;
    R[3] = d.x;
    R[4] = d.y;
    R[5] = d.z;
    if (seed != nullptr) *seed = sd;
}

}  // namespace rtf
