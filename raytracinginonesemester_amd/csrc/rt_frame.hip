// rt_frame.hip — the frame epilogue on gfx950: P6 quantisation of a
// device framebuffer and the band un-permute of gathered strips, so that neither the float
// frame nor the strips have to cross PCIe before the image exists.
//
// Quantisation is write_p6's per-sample conversion (HW1/ppm_p6_lib/src/ppm_p6.cpp:137-155,
// row loop :284-299): double(sample) -> [max(0,x) -> sqrt] -> [clamp to [0,1]] -> * maxval ->
// std::lround -> clamp to [0, maxval]; one byte per sample for maxval < 256, two (big endian,
// write_sample) otherwise.  HIP's double sqrt is correctly rounded, as glibc's is, so the
// samples are the reference's bit for bit (tests/test_gpu_frame.py sweeps every rounding
// boundary of maxval 255).
//
// Both kernels are streaming copies: 12 B in, 3 B out per pixel (quantise); row_bytes in and out
// per row (un-permute).  HBM-bound; c5's 99.5 MB frame quantises in ~25 us at ~5 TB/s.
//
// The film is the same step for caller-ray frames: film_add_*_kernel adds
// radiance samples to per-pixel float sums in render()'s order, film_resolve_*_kernel turns the
// sums into render()'s float pixels and P6 bytes.  Streaming as well: 12 n + 24 B per pixel (add),
// 12 B in and 12 + 3 B out (resolve).
//
// The adaptive film keeps a sample count and two luminance moments beside the sums
// of every pixel: afilm_add_*_kernel adds the samples of a pixel list, afilm_resolve_*_kernel divides
// each pixel by its own count, afilm_flag_kernel / afilm_scatter_kernel select the pixels to sample
// next (a stable compaction around rt_scan.hpp's scan), camera_rays_pixels_kernel makes their rays.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "rt_afilm.hpp"
#include "rt_common.hpp"
#include "rt_film.hpp"
#include "rt_hip_host.hpp"
#include "rt_ppm.hpp"

using rt::set_error;
using rt::hip_msg;

namespace {

constexpr int BLOCK = 256;
typedef float __attribute__((ext_vector_type(4))) vf4;
typedef uint32_t __attribute__((ext_vector_type(4))) vu4;

using rtp::float_to_sample;

struct QuantParams {
    const float* rgb;
    uint8_t* out;
    int64_t n;        // samples (rows * W * 3)
    int64_t row_len;  // samples per row (W * 3)
    int rows;
    int maxval;
    bool clamp, gamma2, flip;
};

// 16 consecutive samples per lane: four float4 loads, one 16-byte (maxval < 256) or two 16-byte
// stores.  Needs row order unchanged (no flip) and 16-byte aligned buffers; the host checks.
template <int BPS>
__global__ __launch_bounds__(BLOCK) void quantize_vec_kernel(QuantParams P) {
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t i0 = g * 16;
    if (i0 >= P.n) return;
    if (i0 + 16 > P.n) {  // ragged tail
        for (int64_t i = i0; i < P.n; ++i) {
            const uint32_t s = float_to_sample(P.rgb[i], P.maxval, P.clamp, P.gamma2);
            if (BPS == 1) P.out[i] = (uint8_t)s;
            else { P.out[2 * i] = (uint8_t)(s >> 8); P.out[2 * i + 1] = (uint8_t)(s & 0xFF); }
        }
        return;
    }
    const vf4* src = reinterpret_cast<const vf4*>(P.rgb + i0);
    float v[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const vf4 q = __builtin_nontemporal_load(src + k);
        v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
    }
    uint32_t w[BPS * 4];
#pragma unroll
    for (int k = 0; k < BPS * 4; ++k) w[k] = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t s = float_to_sample(v[k], P.maxval, P.clamp, P.gamma2);
        if (BPS == 1) {
            w[k >> 2] |= (s & 0xFFu) << (8 * (k & 3));
        } else {  // big endian pair per sample: bytes (hi, lo) at 2k, 2k+1
            const uint32_t be = ((s >> 8) & 0xFFu) | ((s & 0xFFu) << 8);
            w[k >> 1] |= be << (16 * (k & 1));
        }
    }
    vu4* dst = reinterpret_cast<vu4*>(P.out + i0 * BPS);
#pragma unroll
    for (int k = 0; k < BPS; ++k) dst[k] = (vu4){w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]};
}

// General case (flip_y, unaligned buffers): one sample per lane, output index order.
template <int BPS>
__global__ __launch_bounds__(BLOCK) void quantize_any_kernel(QuantParams P) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.n) return;
    int64_t src = i;
    if (P.flip) {
        const int64_t y = i / P.row_len;
        src = ((int64_t)P.rows - 1 - y) * P.row_len + (i - y * P.row_len);
    }
    const uint32_t s = float_to_sample(P.rgb[src], P.maxval, P.clamp, P.gamma2);
    if (BPS == 1) P.out[i] = (uint8_t)s;
    else { P.out[2 * i] = (uint8_t)(s >> 8); P.out[2 * i + 1] = (uint8_t)(s & 0xFF); }
}

// Frame row y (after the optional flip) comes from strip (band % count), row
// (band / count) * band_rows + y % band_rows of it — the strip layout rt_render_device writes
// for (band_rows, band_index, band_count).  One block per output row.
struct UnpermuteParams {
    const uint8_t* strips;
    uint8_t* frame;
    int64_t strip_stride;  // bytes between consecutive ranks' strips
    int64_t row_bytes;
    int height, band_rows, band_count;
    bool flip, vec;
};

__global__ __launch_bounds__(BLOCK) void unpermute_kernel(UnpermuteParams P) {
    const int y = (int)blockIdx.x;
    const int sy = P.flip ? P.height - 1 - y : y;
    const int band = sy / P.band_rows;
    const int rank = band % P.band_count;
    const int64_t k = (int64_t)(band / P.band_count) * P.band_rows + sy % P.band_rows;
    const uint8_t* src = P.strips + rank * P.strip_stride + k * P.row_bytes;
    uint8_t* dst = P.frame + (int64_t)y * P.row_bytes;
    if (P.vec) {
        const int64_t n16 = P.row_bytes >> 4;
        const vu4* s4 = reinterpret_cast<const vu4*>(src);
        vu4* d4 = reinterpret_cast<vu4*>(dst);
        for (int64_t j = threadIdx.x; j < n16; j += BLOCK) d4[j] = __builtin_nontemporal_load(s4 + j);
    } else {
        for (int64_t j = threadIdx.x; j < P.row_bytes; j += BLOCK) dst[j] = src[j];
    }
}

// ---- the film (rt_film.hpp) ----------------------------------------------------------------------
using rtf::film_lds_index;
using rtf::film_pixel;
using rtf::film_sum;

// Floats of radiance a block stages: 16.5 KB of LDS with the spare dwords, so the eight blocks
// that fill a CU's 32 wave slots take 132 of its 160 KB and LDS does not set the occupancy.
constexpr int FILM_TILE = 4096;

struct FilmAddParams {
    const float* rad;  // npix * n * 3: sample s of pixel p at (p * n + s) * 3
    float* sum;        // npix * 3, the band's running sums
    int64_t npix;      // rows * W
    int n;             // samples per pixel in rad
    int tile_pix;      // pixels per block (vec kernel): a multiple of 4, tile_pix * 3n <= FILM_TILE
};

// A block's tile_pix pixels are one contiguous span of rad that starts 16-byte aligned (rad is,
// and tile_pix * 3n floats is a multiple of 4): it is staged into LDS with 16-byte loads, then
// one (pixel, channel) per lane walks its n samples from LDS in order.  Consecutive lanes are
// consecutive floats of sum.  Only the last block's span can end off a 16-byte boundary.
__global__ __launch_bounds__(BLOCK) void film_add_vec_kernel(FilmAddParams P) {
    __shared__ float img[FILM_TILE + FILM_TILE / 32];
    const uint32_t tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * P.tile_pix;
    const int64_t left = P.npix - p0;
    if (left <= 0) return;
    const uint32_t np = left < (int64_t)P.tile_pix ? (uint32_t)left : (uint32_t)P.tile_pix;
    const uint32_t per = 3u * (uint32_t)P.n;
    const uint32_t span = np * per;  // <= FILM_TILE
    const float* src = P.rad + p0 * (int64_t)per;
    const vf4* src4 = reinterpret_cast<const vf4*>(src);
    const uint32_t nv = span >> 2;
    for (uint32_t j = tid; j < nv; j += BLOCK) {
        const vf4 q = __builtin_nontemporal_load(src4 + j);
        const uint32_t a = film_lds_index(4u * j);  // (4j .. 4j + 3 share their spare-dword count)
        img[a] = q.x;
        img[a + 1] = q.y;
        img[a + 2] = q.z;
        img[a + 3] = q.w;
    }
    for (uint32_t i = (nv << 2) + tid; i < span; i += BLOCK) img[film_lds_index(i)] = src[i];
    __syncthreads();
    float* dst = P.sum + p0 * 3;
    const uint32_t items = 3u * np;
    for (uint32_t it = tid; it < items; it += BLOCK) {
        const uint32_t p = it / 3u;
        const uint32_t base = p * per + (it - 3u * p);
        dst[it] = film_sum(dst[it], P.n, [&](int s) { return img[film_lds_index(base + 3u * (uint32_t)s)]; });
    }
}

// General case (unaligned rad, n too large for a tile): one (pixel, channel) per lane from global.
__global__ __launch_bounds__(BLOCK) void film_add_any_kernel(FilmAddParams P) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.npix * 3) return;
    const int64_t p = i / 3;
    const float* r = P.rad + p * 3 * (int64_t)P.n + (i - 3 * p);
    P.sum[i] = film_sum(P.sum[i], P.n, [&](int s) { return r[3 * (int64_t)s]; });
}

struct FilmResolveParams {
    const float* sum;
    float* rgb;     // n floats, or null
    uint8_t* p6;    // n bytes (write_p6 defaults), or null
    int64_t n;      // rows * W * 3
    float fcount;   // float(samples per pixel)
};

// Four consecutive samples per lane: one 16-byte load, one 16-byte float store and/or one dword of
// four bytes, so a wave's accesses are whole contiguous lines (1 KB in, 1 KB and 256 B out).
// Needs sum and rgb 16-byte and p6 4-byte aligned; the host checks.
__global__ __launch_bounds__(BLOCK) void film_resolve_vec_kernel(FilmResolveParams P) {
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t i0 = g * 4;
    if (i0 >= P.n) return;
    if (i0 + 4 > P.n) {  // ragged tail
        for (int64_t i = i0; i < P.n; ++i) {
            const float v = film_pixel(P.sum[i], P.fcount);
            if (P.rgb) P.rgb[i] = v;
            if (P.p6) P.p6[i] = rtp::p6_default_sample(v);
        }
        return;
    }
    // (the sums are read again by the next pass: no nontemporal hint)
    const vf4 q = *reinterpret_cast<const vf4*>(P.sum + i0);
    const vf4 v = (vf4){film_pixel(q.x, P.fcount), film_pixel(q.y, P.fcount), film_pixel(q.z, P.fcount),
                        film_pixel(q.w, P.fcount)};
    if (P.rgb) *reinterpret_cast<vf4*>(P.rgb + i0) = v;
    if (P.p6)
        *reinterpret_cast<uint32_t*>(P.p6 + i0) =
            (uint32_t)rtp::p6_default_sample(v.x) | ((uint32_t)rtp::p6_default_sample(v.y) << 8) |
            ((uint32_t)rtp::p6_default_sample(v.z) << 16) | ((uint32_t)rtp::p6_default_sample(v.w) << 24);
}

// General case (an unaligned buffer): one sample per lane.
__global__ __launch_bounds__(BLOCK) void film_resolve_any_kernel(FilmResolveParams P) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.n) return;
    const float v = film_pixel(P.sum[i], P.fcount);
    if (P.rgb) P.rgb[i] = v;
    if (P.p6) P.p6[i] = rtp::p6_default_sample(v);
}

// ---- the adaptive film (rt_afilm.hpp) ------------------------------------------
#include "rt_wave.hpp"
#include "rt_scan.hpp"

using rtf::afilm_moments;
using rtf::afilm_pixel;
using rtf::afilm_selected;

struct PixelRaysParams {
    rtd::f3 center, p00, du, dv;
    uint32_t W, npix;        // W * H < 2^31
    uint32_t ns, table_spp;  // samples per entry; entries of jitter
    uint32_t n;              // m * ns < 2^31
    const uint32_t* __restrict__ pixels;  // m, or null: entry k is pixel k
    const uint32_t* __restrict__ counts;  // npix, or null: 0
    const float* __restrict__ jitter;     // 2 * table_spp
    float* __restrict__ rays;             // n x rt_ray
    uint32_t* __restrict__ seeds;         // n, or null
};

// One sample per lane, ray k * ns + s: consecutive lanes write consecutive rays.  The only reads
// through a caller's value are counts[pix] with pix < npix and the table below table_spp.
__global__ __launch_bounds__(BLOCK) void camera_rays_pixels_kernel(PixelRaysParams P) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.n) return;
    const uint32_t k = i / P.ns, s = i - k * P.ns;
    const uint32_t pix = P.pixels != nullptr ? P.pixels[k] : k;
    const uint32_t c = pix < P.npix && P.counts != nullptr ? P.counts[pix] : 0u;
    rtf::camera_pixel_ray(P.center, P.p00, P.du, P.dv, P.W, P.npix, pix, c, s, P.jitter, P.table_spp,
                          P.rays + 6 * (size_t)i, P.seeds != nullptr ? P.seeds + i : nullptr);
}

struct AFilmAddParams {
    const float* rad;        // m * n * 3: sample s of entry k at (k * n + s) * 3
    const uint32_t* pixels;  // m, or null: entry k is pixel k
    float* sum;              // npix * 3
    uint32_t* count;         // npix
    float* mom;              // npix * 2: m1, m2
    int64_t m;               // entries
    uint32_t npix;           // W * H
    int n;                   // samples per entry in rad
    int tile_pix;            // entries per block (vec kernel): a multiple of 4, tile_pix * 3n <= FILM_TILE
};

// film_add_vec_kernel's staging as a gather: a block's tile_pix entries are one contiguous,
// 16-byte aligned span of rad whatever pixels they name; it is staged into LDS, then one (entry,
// channel) per lane adds its n samples to the named pixel's sum, and one entry per lane its
// moments and count.  An entry whose index is outside the image is skipped.  Indices are unique
// within a call, so every word has one writer.
__global__ __launch_bounds__(BLOCK) void afilm_add_vec_kernel(AFilmAddParams P) {
    __shared__ float img[FILM_TILE + FILM_TILE / 32];
    const uint32_t tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * P.tile_pix;
    const int64_t left = P.m - p0;
    if (left <= 0) return;
    const uint32_t np = left < (int64_t)P.tile_pix ? (uint32_t)left : (uint32_t)P.tile_pix;
    const uint32_t per = 3u * (uint32_t)P.n;
    const uint32_t span = np * per;  // <= FILM_TILE
    const float* src = P.rad + p0 * (int64_t)per;
    const vf4* src4 = reinterpret_cast<const vf4*>(src);
    const uint32_t nv = span >> 2;
    for (uint32_t j = tid; j < nv; j += BLOCK) {
        const vf4 q = __builtin_nontemporal_load(src4 + j);
        const uint32_t a = film_lds_index(4u * j);
        img[a] = q.x;
        img[a + 1] = q.y;
        img[a + 2] = q.z;
        img[a + 3] = q.w;
    }
    for (uint32_t i = (nv << 2) + tid; i < span; i += BLOCK) img[film_lds_index(i)] = src[i];
    __syncthreads();
    const uint32_t items = 3u * np;
    for (uint32_t it = tid; it < items; it += BLOCK) {
        const uint32_t p = it / 3u, c = it - 3u * p;
        const uint32_t pix = P.pixels != nullptr ? P.pixels[p0 + p] : (uint32_t)(p0 + p);
        if (pix >= P.npix) continue;
        const uint32_t base = p * per + c;
        float* d = P.sum + 3 * (size_t)pix + c;
        *d = film_sum(*d, P.n, [&](int s) { return img[film_lds_index(base + 3u * (uint32_t)s)]; });
    }
    for (uint32_t p = tid; p < np; p += BLOCK) {
        const uint32_t pix = P.pixels != nullptr ? P.pixels[p0 + p] : (uint32_t)(p0 + p);
        if (pix >= P.npix) continue;
        const uint32_t base = p * per;
        float m1 = P.mom[2 * (size_t)pix], m2 = P.mom[2 * (size_t)pix + 1];
        afilm_moments(m1, m2, P.n, [&](int s, int c) { return img[film_lds_index(base + 3u * (uint32_t)s + (uint32_t)c)]; });
        P.mom[2 * (size_t)pix] = m1;
        P.mom[2 * (size_t)pix + 1] = m2;
        P.count[pix] = P.count[pix] + (uint32_t)P.n;
    }
}

// General case (unaligned rad, n too large for a tile): four lanes per entry from global, three
// channel sums and the moments with the count.
__global__ __launch_bounds__(BLOCK) void afilm_add_any_kernel(AFilmAddParams P) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.m * 4) return;
    const int64_t k = i >> 2;
    const int c = (int)(i & 3);
    const uint32_t pix = P.pixels != nullptr ? P.pixels[k] : (uint32_t)k;
    if (pix >= P.npix) return;
    const float* r = P.rad + k * 3 * (int64_t)P.n;
    if (c < 3) {
        float* d = P.sum + 3 * (size_t)pix + c;
        *d = film_sum(*d, P.n, [&](int s) { return r[3 * (int64_t)s + c]; });
    } else {
        float m1 = P.mom[2 * (size_t)pix], m2 = P.mom[2 * (size_t)pix + 1];
        afilm_moments(m1, m2, P.n, [&](int s, int ch) { return r[3 * (int64_t)s + ch]; });
        P.mom[2 * (size_t)pix] = m1;
        P.mom[2 * (size_t)pix + 1] = m2;
        P.count[pix] = P.count[pix] + (uint32_t)P.n;
    }
}

struct AFilmResolveParams {
    const float* sum;       // the rows' sums
    const uint32_t* count;  // the rows' counts: sample i belongs to pixel i / 3
    float* rgb;             // n floats, or null
    uint8_t* p6;            // n bytes, or null
    int64_t n;              // rows * W * 3
};

// film_resolve_vec_kernel with each pixel's own count: four consecutive samples per lane.
__global__ __launch_bounds__(BLOCK) void afilm_resolve_vec_kernel(AFilmResolveParams P) {
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t i0 = g * 4;
    if (i0 >= P.n) return;
    if (i0 + 4 > P.n) {  // ragged tail
        for (int64_t i = i0; i < P.n; ++i) {
            const float v = afilm_pixel(P.sum[i], P.count[i / 3]);
            if (P.rgb) P.rgb[i] = v;
            if (P.p6) P.p6[i] = rtp::p6_default_sample(v);
        }
        return;
    }
    const vf4 q = *reinterpret_cast<const vf4*>(P.sum + i0);
    const int64_t pa = i0 / 3;  // samples r .. r + 3 of pixel pa's three: the last is always pixel pa + 1's, none pa + 2's
    const uint32_t r = (uint32_t)(i0 - 3 * pa);
    const uint32_t ca = P.count[pa], cb = P.count[pa + 1];
    const vf4 v = (vf4){afilm_pixel(q.x, ca), afilm_pixel(q.y, r + 1 < 3 ? ca : cb), afilm_pixel(q.z, r + 2 < 3 ? ca : cb),
                        afilm_pixel(q.w, cb)};
    if (P.rgb) *reinterpret_cast<vf4*>(P.rgb + i0) = v;
    if (P.p6)
        *reinterpret_cast<uint32_t*>(P.p6 + i0) =
            (uint32_t)rtp::p6_default_sample(v.x) | ((uint32_t)rtp::p6_default_sample(v.y) << 8) |
            ((uint32_t)rtp::p6_default_sample(v.z) << 16) | ((uint32_t)rtp::p6_default_sample(v.w) << 24);
}

// General case (an unaligned buffer): one sample per lane.
__global__ __launch_bounds__(BLOCK) void afilm_resolve_any_kernel(AFilmResolveParams P) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.n) return;
    const float v = afilm_pixel(P.sum[i], P.count[i / 3]);
    if (P.rgb) P.rgb[i] = v;
    if (P.p6) P.p6[i] = rtp::p6_default_sample(v);
}

// The selection is rt_path_compact_device's compaction (rt_path.hpp) with the flag computed from
// the accumulators: (1) each block decides its PATH_TILE pixels, keeps the flags as bytes and
// counts them; (2) path_scan turns the counts into offsets and the total; (3) each block writes
// the indices of its flagged pixels from its offset on, in increasing order.
struct AFilmSelectParams {
    const uint32_t* __restrict__ count;
    const float* __restrict__ mom;
    uint32_t npix;
    rtf::SelectOpts o;
    uint8_t* __restrict__ flags;    // npix
    uint32_t* __restrict__ counts;  // per tile
};

__global__ __launch_bounds__(BLOCK) void afilm_flag_kernel(AFilmSelectParams P) {
    __shared__ uint32_t part[PATH_WAVES];
    const uint64_t base = (uint64_t)blockIdx.x * PATH_TILE;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < PATH_ROUNDS; ++j) {
        const uint64_t k = base + (uint32_t)j * BLOCK + threadIdx.x;
        bool f = false;
        if (k < P.npix) {
            f = afilm_selected(P.count[k], P.mom[2 * k], P.mom[2 * k + 1], P.o);
            P.flags[k] = f ? 1 : 0;
        }
        c += (uint32_t)__popcll(ballot(f));  // wave-uniform
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < PATH_WAVES; ++w) s += part[w];
        P.counts[blockIdx.x] = s;
    }
}

// path_scatter_kernel's ranks, the payload the pixel's own index.
__global__ __launch_bounds__(BLOCK) void afilm_scatter_kernel(const uint8_t* __restrict__ flags, uint32_t npix,
                                                              const uint32_t* __restrict__ offsets,
                                                              uint32_t* __restrict__ pixels_out) {
    __shared__ uint32_t cnt[PATH_ROUNDS * PATH_WAVES];
    const uint64_t base = (uint64_t)blockIdx.x * PATH_TILE;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t below[PATH_ROUNDS];
    bool flag[PATH_ROUNDS];
#pragma unroll
    for (int j = 0; j < PATH_ROUNDS; ++j) {
        const uint64_t k = base + (uint32_t)j * BLOCK + threadIdx.x;
        flag[j] = k < npix && flags[k] != 0;
        const uint64_t mask = ballot(flag[j]);
        below[j] = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) cnt[j * PATH_WAVES + wave] = (uint32_t)__popcll(mask);
    }
    __syncthreads();
    const uint32_t off = offsets[blockIdx.x];
#pragma unroll
    for (int j = 0; j < PATH_ROUNDS; ++j) {
        if (!flag[j]) continue;
        uint32_t before = 0;
        for (int q = 0; q < j * PATH_WAVES + (int)wave; ++q) before += cnt[q];
        // off + before + below < the number of flagged pixels <= npix
        pixels_out[(size_t)off + before + below[j]] = (uint32_t)(base + (uint32_t)j * BLOCK + threadIdx.x);
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// rows [row0, row0 + rows) of a height-row image
bool rows_inside(int row0, int rows, int height) { return row0 >= 0 && rows >= 0 && row0 <= height && rows <= height - row0; }

}  // namespace

// Sums on the device, per-row sample counts on the host (updated as calls are enqueued).
struct rt_film {
    int device = 0, width = 0, height = 0;
    rt::DevBuf sum;
    std::vector<int64_t> count;
};

extern "C" int rt_film_create(int device, int width, int height, rt_film** out) {
    if (!out) return set_error(RT_ERR_ARG, "rt_film_create: null out");
    *out = nullptr;
    if (width < 1 || height < 1) return set_error(RT_ERR_ARG, "rt_film_create: an empty image");
    int rc = rt::check_device(device);
    if (rc != RT_OK) return rc;
    rt::DeviceGuard g(device);
    rt_film* f = new (std::nothrow) rt_film;
    if (!f) return set_error(RT_ERR_INTERNAL, "rt_film_create: out of memory");
    f->device = device;
    f->width = width;
    f->height = height;
    f->count.assign((size_t)height, 0);
    const size_t bytes = (size_t)width * (size_t)height * 3 * sizeof(float);
    hipError_t e = hipSuccess;
    if ((rc = f->sum.alloc(bytes)) == RT_OK && (e = hipMemset(f->sum.p, 0, bytes)) == hipSuccess)
        e = hipStreamSynchronize(nullptr);  // zeroed before any stream of the caller's can add
    if (rc == RT_OK && e != hipSuccess) rc = set_error(RT_ERR_HIP, hip_msg(e, "rt_film_create: hipMemset"));
    if (rc != RT_OK) {
        delete f;
        return rc;
    }
    *out = f;
    return RT_OK;
}

extern "C" void rt_film_destroy(rt_film* f) {
    if (!f) return;
    rt::DeviceGuard g(f->device);
    delete f;
}

extern "C" int rt_film_clear_device(rt_film* f, void* hip_stream) {
    if (!f) return set_error(RT_ERR_ARG, "rt_film_clear_device: null film");
    rt::DeviceGuard g(f->device);
    HIP_TRY(hipMemsetAsync(f->sum.p, 0, f->sum.n, static_cast<hipStream_t>(hip_stream)));
    f->count.assign(f->count.size(), 0);
    return RT_OK;
}

extern "C" int rt_film_add_device(rt_film* f, const float* radiance_dev, int row0, int rows, int nsamples,
                                  void* hip_stream) {
    if (!f || !radiance_dev) return set_error(RT_ERR_ARG, "rt_film_add_device: null film or radiance");
    if (nsamples < 1) return set_error(RT_ERR_ARG, "rt_film_add_device: nsamples < 1");
    if (!rows_inside(row0, rows, f->height)) return set_error(RT_ERR_ARG, "rt_film_add_device: rows outside the image");
    const int64_t npix = (int64_t)rows * f->width;
    if (npix > 0x7FFFFFFFll / nsamples)
        return set_error(RT_ERR_UNSUPPORTED, "rt_film_add_device: more than 2^31-1 samples in one call");
    if (rows == 0) return RT_OK;
    rt::DeviceGuard g(f->device);
    FilmAddParams P;
    P.rad = radiance_dev;
    P.sum = static_cast<float*>(f->sum.p) + (int64_t)row0 * f->width * 3;
    P.npix = npix;
    P.n = nsamples;
    P.tile_pix = (FILM_TILE / (3 * nsamples)) & ~3;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (P.tile_pix >= 4 && aligned16(radiance_dev)) {
        const dim3 grid((unsigned)((npix + P.tile_pix - 1) / P.tile_pix));
        hipLaunchKernelGGL(film_add_vec_kernel, grid, dim3(BLOCK), 0, st, P);
    } else {
        const dim3 grid((unsigned)((npix * 3 + BLOCK - 1) / BLOCK));
        hipLaunchKernelGGL(film_add_any_kernel, grid, dim3(BLOCK), 0, st, P);
    }
    HIP_TRY(hipGetLastError());
    for (int y = row0; y < row0 + rows; ++y) f->count[(size_t)y] += nsamples;
    return RT_OK;
}

extern "C" int rt_film_resolve_device(rt_film* f, int row0, int rows, float* rgb_dev, uint8_t* p6_dev,
                                      void* hip_stream) {
    if (!f) return set_error(RT_ERR_ARG, "rt_film_resolve_device: null film");
    if (!rgb_dev && !p6_dev) return set_error(RT_ERR_ARG, "rt_film_resolve_device: both outputs null");
    if (!rows_inside(row0, rows, f->height)) return set_error(RT_ERR_ARG, "rt_film_resolve_device: rows outside the image");
    if (rows == 0) return RT_OK;
    const int64_t count = f->count[(size_t)row0];
    if (count < 1) return set_error(RT_ERR_ARG, "rt_film_resolve_device: a row without samples");
    for (int y = row0; y < row0 + rows; ++y)
        if (f->count[(size_t)y] != count)
            return set_error(RT_ERR_ARG, "rt_film_resolve_device: rows with different sample counts");
    rt::DeviceGuard g(f->device);
    FilmResolveParams P;
    P.sum = static_cast<const float*>(f->sum.p) + (int64_t)row0 * f->width * 3;
    P.rgb = rgb_dev;
    P.p6 = p6_dev;
    P.n = (int64_t)rows * f->width * 3;
    P.fcount = (float)count;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (aligned16(P.sum) && aligned16(rgb_dev) && (reinterpret_cast<uintptr_t>(p6_dev) & 3u) == 0) {  // (null is aligned)
        const int64_t lanes = (P.n + 3) / 4;
        hipLaunchKernelGGL(film_resolve_vec_kernel, dim3((unsigned)((lanes + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, P);
    } else {
        hipLaunchKernelGGL(film_resolve_any_kernel, dim3((unsigned)((P.n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, P);
    }
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

extern "C" int rt_film_row_samples(const rt_film* f, int row, int64_t* count) {
    if (!f || !count) return set_error(RT_ERR_ARG, "rt_film_row_samples: null film or count");
    if (row < 0 || row >= f->height) return set_error(RT_ERR_ARG, "rt_film_row_samples: row outside the image");
    *count = f->count[(size_t)row];
    return RT_OK;
}

// The host build of the film: film_sum and film_pixel as the kernels run them.
extern "C" int rt_film_pixels_host(const float* radiance, int width, int rows, int nsamples, float* sum_inout,
                                   int64_t count_after, float* rgb_out) {
    if (!radiance || !sum_inout) return set_error(RT_ERR_ARG, "rt_film_pixels_host: null radiance or sums");
    if (nsamples < 1) return set_error(RT_ERR_ARG, "rt_film_pixels_host: nsamples < 1");
    if (width < 1 || rows < 0) return set_error(RT_ERR_ARG, "rt_film_pixels_host: bad shape");
    if (count_after < nsamples) return set_error(RT_ERR_ARG, "rt_film_pixels_host: count_after < nsamples");
    const int64_t npix = (int64_t)rows * width;
    if (npix > 0x7FFFFFFFll / nsamples)
        return set_error(RT_ERR_UNSUPPORTED, "rt_film_pixels_host: more than 2^31-1 samples in one call");
    const float fcount = (float)count_after;
    for (int64_t i = 0; i < npix * 3; ++i) {
        const int64_t p = i / 3;
        const float* r = radiance + p * 3 * (int64_t)nsamples + (i - 3 * p);
        sum_inout[i] = film_sum(sum_inout[i], nsamples, [&](int s) { return r[3 * (int64_t)s]; });
        if (rgb_out) rgb_out[i] = film_pixel(sum_inout[i], fcount);
    }
    return RT_OK;
}

// ---- adaptive sampling: pixel-list camera rays and the adaptive film -----------------------------
static_assert(rtf::PIXEL_NONE == RT_PIXEL_NONE, "RT_PIXEL_NONE");
static_assert(sizeof(rtf::SelectOpts) == sizeof(rt_afilm_select_opts), "rt_afilm_select_opts");

namespace {
// The checks of rt_camera_rays_pixels_host / _device: no HIP call before they pass.  *n_out: m * nsamples.
int pixel_rays_args(const rt_camera* cam, const uint32_t* pixels, size_t m, int nsamples, int table_spp, const void* rays,
                    size_t* n_out) {
    if (!cam || !rays) return set_error(RT_ERR_ARG, "rt_camera_rays_pixels: null camera or rays");
    if (nsamples < 1 || table_spp < 1) return set_error(RT_ERR_ARG, "rt_camera_rays_pixels: nsamples < 1 or table_spp < 1");
    const int W = cam->pixel_width, H = cam->pixel_height;
    if (W < 1 || H < 1) return set_error(RT_ERR_ARG, "rt_camera_rays_pixels: an empty image");
    if ((int64_t)W * H > 0x7FFFFFFFll) return set_error(RT_ERR_UNSUPPORTED, "rt_camera_rays_pixels: more than 2^31-1 pixels");
    if (m > 0x7FFFFFFFull / (unsigned)nsamples)
        return set_error(RT_ERR_UNSUPPORTED, "rt_camera_rays_pixels: more than 2^31-1 rays in one call");
    if (!pixels && m != 0 && m != (size_t)W * (size_t)H)
        return set_error(RT_ERR_ARG, "rt_camera_rays_pixels: a null pixel list with m != W * H");
    *n_out = m * (size_t)nsamples;
    return RT_OK;
}

void pixel_rays_camera(const rt_camera* cam, rtd::f3* center, rtd::f3* p00, rtd::f3* du, rtd::f3* dv) {
    *center = rtd::mk(cam->center.x, cam->center.y, cam->center.z);
    *p00 = rtd::mk(cam->pixel00_loc.x, cam->pixel00_loc.y, cam->pixel00_loc.z);
    *du = rtd::mk(cam->pixel_delta_u.x, cam->pixel_delta_u.y, cam->pixel_delta_u.z);
    *dv = rtd::mk(cam->pixel_delta_v.x, cam->pixel_delta_v.y, cam->pixel_delta_v.z);
}

int select_opts_args(const char* who, const rt_afilm_select_opts* o) {
    if (!o) return set_error(RT_ERR_ARG, std::string(who) + ": null opts");
    // (written so that a NaN fails)
    if (o->min_samples < 2 || o->step < 1 || !(o->tol >= 0.0) || !(o->floor > 0.0))
        return set_error(RT_ERR_ARG, std::string(who) + ": needs min_samples >= 2, step >= 1, tol >= 0 and floor > 0");
    return RT_OK;
}

rtf::SelectOpts select_opts(const rt_afilm_select_opts* o) {
    rtf::SelectOpts s;
    s.min_samples = o->min_samples;
    s.max_samples = o->max_samples;
    s.step = o->step;
    s.tol = o->tol;
    s.floor = o->floor;
    return s;
}
}  // namespace

extern "C" int rt_camera_rays_pixels_host(const rt_camera* cam, const uint32_t* pixels, size_t m, const uint32_t* counts,
                                          int nsamples, const float* jitter, int table_spp, rt_ray* rays, uint32_t* seeds) {
    size_t n = 0;
    int rc = pixel_rays_args(cam, pixels, m, nsamples, table_spp, rays, &n);
    if (rc != RT_OK || n == 0) return rc;
    std::vector<float> tab;
    if (!jitter) {
        tab.resize(size_t(2) * size_t(table_spp));
        if ((rc = rt_jittered_samples(table_spp, 42u, 1, tab.data())) != RT_OK) return rc;
        jitter = tab.data();
    }
    rtd::f3 center, p00, du, dv;
    pixel_rays_camera(cam, &center, &p00, &du, &dv);
    const uint32_t W = (uint32_t)cam->pixel_width, npix = W * (uint32_t)cam->pixel_height;
    for (size_t k = 0; k < m; ++k) {
        const uint32_t pix = pixels ? pixels[k] : (uint32_t)k;
        const uint32_t c = pix < npix && counts ? counts[pix] : 0u;
        for (int s = 0; s < nsamples; ++s) {
            const size_t i = k * (size_t)nsamples + (size_t)s;
            rtf::camera_pixel_ray(center, p00, du, dv, W, npix, pix, c, (uint32_t)s, jitter, (uint32_t)table_spp,
                                  reinterpret_cast<float*>(rays + i), seeds ? seeds + i : nullptr);
        }
    }
    return RT_OK;
}

extern "C" int rt_camera_rays_pixels_device(const rt_camera* cam, const uint32_t* pixels_dev, size_t m,
                                            const uint32_t* counts_dev, int nsamples, const float* jitter_dev, int table_spp,
                                            rt_ray* rays_dev, uint32_t* seeds_dev, int device, void* hip_stream) {
    size_t n = 0;
    int rc = pixel_rays_args(cam, pixels_dev, m, nsamples, table_spp, rays_dev, &n);
    if (rc != RT_OK) return rc;
    if (!jitter_dev) return set_error(RT_ERR_ARG, "rt_camera_rays_pixels_device: null jitter table");
    if (n == 0) return RT_OK;
    if ((rc = rt::check_device(device)) != RT_OK) return rc;
    rt::DeviceGuard g(device);
    PixelRaysParams P;
    std::memset(&P, 0, sizeof(P));
    pixel_rays_camera(cam, &P.center, &P.p00, &P.du, &P.dv);
    P.W = (uint32_t)cam->pixel_width;
    P.npix = P.W * (uint32_t)cam->pixel_height;
    P.ns = (uint32_t)nsamples;
    P.table_spp = (uint32_t)table_spp;
    P.n = (uint32_t)n;
    P.pixels = pixels_dev;
    P.counts = counts_dev;
    P.jitter = jitter_dev;
    P.rays = reinterpret_cast<float*>(rays_dev);
    P.seeds = seeds_dev;
    hipLaunchKernelGGL(camera_rays_pixels_kernel, dim3((P.n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0,
                       static_cast<hipStream_t>(hip_stream), P);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// Everything on the device: sums, counts and moments, 24 B per pixel.
struct rt_afilm {
    int device = 0, width = 0, height = 0;
    rt::DevBuf sum, count, mom;
    uint32_t npix() const { return (uint32_t)width * (uint32_t)height; }
};

extern "C" int rt_afilm_create(int device, int width, int height, rt_afilm** out) {
    if (!out) return set_error(RT_ERR_ARG, "rt_afilm_create: null out");
    *out = nullptr;
    if (width < 1 || height < 1) return set_error(RT_ERR_ARG, "rt_afilm_create: an empty image");
    if ((int64_t)width * height > 0x7FFFFFFFll) return set_error(RT_ERR_UNSUPPORTED, "rt_afilm_create: more than 2^31-1 pixels");
    int rc = rt::check_device(device);
    if (rc != RT_OK) return rc;
    rt::DeviceGuard g(device);
    rt_afilm* f = new (std::nothrow) rt_afilm;
    if (!f) return set_error(RT_ERR_INTERNAL, "rt_afilm_create: out of memory");
    f->device = device;
    f->width = width;
    f->height = height;
    const size_t np = (size_t)width * (size_t)height;
    hipError_t e = hipSuccess;
    if ((rc = f->sum.alloc(np * 3 * sizeof(float))) == RT_OK && (rc = f->count.alloc(np * sizeof(uint32_t))) == RT_OK &&
        (rc = f->mom.alloc(np * 2 * sizeof(float))) == RT_OK && (e = hipMemset(f->sum.p, 0, f->sum.n)) == hipSuccess &&
        (e = hipMemset(f->count.p, 0, f->count.n)) == hipSuccess && (e = hipMemset(f->mom.p, 0, f->mom.n)) == hipSuccess)
        e = hipStreamSynchronize(nullptr);  // zeroed before any stream of the caller's can add
    if (rc == RT_OK && e != hipSuccess) rc = set_error(RT_ERR_HIP, hip_msg(e, "rt_afilm_create: hipMemset"));
    if (rc != RT_OK) {
        delete f;
        return rc;
    }
    *out = f;
    return RT_OK;
}

extern "C" void rt_afilm_destroy(rt_afilm* f) {
    if (!f) return;
    rt::DeviceGuard g(f->device);
    delete f;
}

extern "C" int rt_afilm_clear_device(rt_afilm* f, void* hip_stream) {
    if (!f) return set_error(RT_ERR_ARG, "rt_afilm_clear_device: null film");
    rt::DeviceGuard g(f->device);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipMemsetAsync(f->sum.p, 0, f->sum.n, st));
    HIP_TRY(hipMemsetAsync(f->count.p, 0, f->count.n, st));
    HIP_TRY(hipMemsetAsync(f->mom.p, 0, f->mom.n, st));
    return RT_OK;
}

extern "C" const uint32_t* rt_afilm_counts_device(const rt_afilm* f) {
    return f ? static_cast<const uint32_t*>(f->count.p) : nullptr;
}

extern "C" int rt_afilm_add_device(rt_afilm* f, const uint32_t* pixels_dev, size_t m, const float* radiance_dev,
                                   int nsamples, void* hip_stream) {
    if (!f || !radiance_dev) return set_error(RT_ERR_ARG, "rt_afilm_add_device: null film or radiance");
    if (nsamples < 1) return set_error(RT_ERR_ARG, "rt_afilm_add_device: nsamples < 1");
    if (m > 0x7FFFFFFFull / (unsigned)nsamples)
        return set_error(RT_ERR_UNSUPPORTED, "rt_afilm_add_device: more than 2^31-1 samples in one call");
    if (!pixels_dev && m != 0 && m != f->npix()) return set_error(RT_ERR_ARG, "rt_afilm_add_device: a null pixel list with m != W * H");
    if (m == 0) return RT_OK;
    rt::DeviceGuard g(f->device);
    AFilmAddParams P;
    P.rad = radiance_dev;
    P.pixels = pixels_dev;
    P.sum = static_cast<float*>(f->sum.p);
    P.count = static_cast<uint32_t*>(f->count.p);
    P.mom = static_cast<float*>(f->mom.p);
    P.m = (int64_t)m;
    P.npix = f->npix();
    P.n = nsamples;
    P.tile_pix = (FILM_TILE / (3 * nsamples)) & ~3;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (P.tile_pix >= 4 && aligned16(radiance_dev)) {
        const dim3 grid((unsigned)((P.m + P.tile_pix - 1) / P.tile_pix));
        hipLaunchKernelGGL(afilm_add_vec_kernel, grid, dim3(BLOCK), 0, st, P);
    } else {
        const dim3 grid((unsigned)((P.m * 4 + BLOCK - 1) / BLOCK));
        hipLaunchKernelGGL(afilm_add_any_kernel, grid, dim3(BLOCK), 0, st, P);
    }
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

extern "C" int rt_afilm_resolve_device(rt_afilm* f, int row0, int rows, float* rgb_dev, uint8_t* p6_dev,
                                       uint32_t* counts_out_dev, void* hip_stream) {
    if (!f) return set_error(RT_ERR_ARG, "rt_afilm_resolve_device: null film");
    if (!rgb_dev && !p6_dev && !counts_out_dev) return set_error(RT_ERR_ARG, "rt_afilm_resolve_device: every output null");
    if (!rows_inside(row0, rows, f->height)) return set_error(RT_ERR_ARG, "rt_afilm_resolve_device: rows outside the image");
    if (rows == 0) return RT_OK;
    rt::DeviceGuard g(f->device);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const int64_t first = (int64_t)row0 * f->width, npix = (int64_t)rows * f->width;
    if (rgb_dev || p6_dev) {
        AFilmResolveParams P;
        P.sum = static_cast<const float*>(f->sum.p) + first * 3;
        P.count = static_cast<const uint32_t*>(f->count.p) + first;
        P.rgb = rgb_dev;
        P.p6 = p6_dev;
        P.n = npix * 3;
        if (aligned16(P.sum) && aligned16(rgb_dev) && (reinterpret_cast<uintptr_t>(p6_dev) & 3u) == 0) {  // (null is aligned)
            const int64_t lanes = (P.n + 3) / 4;
            hipLaunchKernelGGL(afilm_resolve_vec_kernel, dim3((unsigned)((lanes + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, P);
        } else {
            hipLaunchKernelGGL(afilm_resolve_any_kernel, dim3((unsigned)((P.n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, P);
        }
        HIP_TRY(hipGetLastError());
    }
    if (counts_out_dev)  // the sample-count map: a copy on the stream
        HIP_TRY(hipMemcpyAsync(counts_out_dev, static_cast<const uint32_t*>(f->count.p) + first, (size_t)npix * sizeof(uint32_t),
                               hipMemcpyDeviceToDevice, st));
    return RT_OK;
}

extern "C" size_t rt_afilm_select_scratch_bytes(const rt_afilm* f) {
    if (!f) return 0;
    const size_t nt = path_tiles(f->npix());
    return sizeof(uint32_t) * (nt + path_scan_words(nt)) + f->npix();
}

extern "C" int rt_afilm_select_device(rt_afilm* f, const rt_afilm_select_opts* opts, uint32_t* pixels_out_dev,
                                      uint32_t* count_dev, void* scratch_dev, void* hip_stream) {
    if (!f) return set_error(RT_ERR_ARG, "rt_afilm_select_device: null film");
    const int rc = select_opts_args("rt_afilm_select_device", opts);
    if (rc != RT_OK) return rc;
    if (!pixels_out_dev || !count_dev || !scratch_dev)
        return set_error(RT_ERR_ARG, "rt_afilm_select_device: null pixels_out, count or scratch");
    if (reinterpret_cast<uintptr_t>(scratch_dev) % 4 != 0)
        return set_error(RT_ERR_ARG, "rt_afilm_select_device: scratch_dev is not 4-byte aligned");
    rt::DeviceGuard g(f->device);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const uint32_t npix = f->npix();
    const size_t nt = path_tiles(npix);
    uint32_t* counts = static_cast<uint32_t*>(scratch_dev);
    AFilmSelectParams P;
    P.count = static_cast<const uint32_t*>(f->count.p);
    P.mom = static_cast<const float*>(f->mom.p);
    P.npix = npix;
    P.o = select_opts(opts);
    P.flags = reinterpret_cast<uint8_t*>(counts + nt + path_scan_words(nt));
    P.counts = counts;
    hipLaunchKernelGGL(afilm_flag_kernel, dim3(unsigned(nt)), dim3(BLOCK), 0, st, P);
    path_scan(counts, nt, counts + nt, count_dev, st);
    hipLaunchKernelGGL(afilm_scatter_kernel, dim3(unsigned(nt)), dim3(BLOCK), 0, st, P.flags, npix, counts, pixels_out_dev);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// The host build of the adaptive film: film_sum, afilm_moments, afilm_pixel and afilm_selected as
// the kernels run them, over host arrays.
extern "C" int rt_afilm_host(int width, int height, float* sum, uint32_t* count, float* moments, const uint32_t* pixels,
                             size_t m, const float* radiance, int nsamples, float* rgb_out, uint8_t* p6_out,
                             const rt_afilm_select_opts* opts, uint32_t* pixels_out, uint32_t* selected_out) {
    if (width < 1 || height < 1) return set_error(RT_ERR_ARG, "rt_afilm_host: an empty image");
    if ((int64_t)width * height > 0x7FFFFFFFll) return set_error(RT_ERR_UNSUPPORTED, "rt_afilm_host: more than 2^31-1 pixels");
    if (!sum || !count || !moments) return set_error(RT_ERR_ARG, "rt_afilm_host: null sums, counts or moments");
    const uint32_t npix = (uint32_t)width * (uint32_t)height;
    if (radiance) {
        if (nsamples < 1) return set_error(RT_ERR_ARG, "rt_afilm_host: nsamples < 1");
        if (m > 0x7FFFFFFFull / (unsigned)nsamples)
            return set_error(RT_ERR_UNSUPPORTED, "rt_afilm_host: more than 2^31-1 samples in one call");
        if (!pixels && m != 0 && m != npix) return set_error(RT_ERR_ARG, "rt_afilm_host: a null pixel list with m != W * H");
    }
    if (opts) {
        const int rc = select_opts_args("rt_afilm_host", opts);
        if (rc != RT_OK) return rc;
        if (!pixels_out || !selected_out) return set_error(RT_ERR_ARG, "rt_afilm_host: null pixels_out or selected_out");
    }
    if (radiance)
        for (size_t k = 0; k < m; ++k) {
            const uint32_t pix = pixels ? pixels[k] : (uint32_t)k;
            if (pix >= npix) continue;
            const float* r = radiance + k * 3 * (size_t)nsamples;
            for (int c = 0; c < 3; ++c) {
                float* d = sum + 3 * (size_t)pix + c;
                *d = film_sum(*d, nsamples, [&](int s) { return r[3 * (size_t)s + (size_t)c]; });
            }
            afilm_moments(moments[2 * (size_t)pix], moments[2 * (size_t)pix + 1], nsamples,
                          [&](int s, int c) { return r[3 * (size_t)s + (size_t)c]; });
            count[pix] = count[pix] + (uint32_t)nsamples;
        }
    if (rgb_out || p6_out)
        for (size_t i = 0; i < (size_t)npix * 3; ++i) {
            const float v = afilm_pixel(sum[i], count[i / 3]);
            if (rgb_out) rgb_out[i] = v;
            if (p6_out) p6_out[i] = rtp::p6_default_sample(v);
        }
    if (opts) {
        const rtf::SelectOpts o = select_opts(opts);
        uint32_t n = 0;
        for (uint32_t p = 0; p < npix; ++p)
            if (afilm_selected(count[p], moments[2 * (size_t)p], moments[2 * (size_t)p + 1], o)) pixels_out[n++] = p;
        *selected_out = n;
    }
    return RT_OK;
}

extern "C" int rt_ppm_header(int width, int height, int maxval, char* buf, size_t cap, size_t* written) {
    if (width <= 0 || height <= 0) return set_error(RT_ERR_ARG, "Image has non-positive dimensions.");
    if (maxval <= 0 || maxval > 65535) return set_error(RT_ERR_ARG, "Invalid maxval (must be 1..65535).");
    char h[64];
    const int n = std::snprintf(h, sizeof(h), "P6\n%d %d\n%d\n", width, height, maxval);
    if (written) *written = (size_t)n;
    if (!buf) return RT_OK;
    if (cap < (size_t)n) return set_error(RT_ERR_ARG, "rt_ppm_header: buffer too small");
    std::memcpy(buf, h, (size_t)n);
    return RT_OK;
}

extern "C" int rt_ppm_quantize_device(const float* rgb_dev, int width, int rows, const rt_ppm_options* opt,
                                      uint8_t* out_dev, void* hip_stream) {
    rt_ppm_options d;
    rt_ppm_options_default(&d);
    if (!opt) opt = &d;
    if (width <= 0 || rows <= 0) return set_error(RT_ERR_ARG, "Image has non-positive dimensions.");
    if (opt->maxval <= 0 || opt->maxval > 65535) return set_error(RT_ERR_ARG, "Invalid maxval (must be 1..65535).");
    if (!rgb_dev || !out_dev) return set_error(RT_ERR_ARG, "rt_ppm_quantize_device: null buffer");
    QuantParams P;
    P.rgb = rgb_dev;
    P.out = out_dev;
    P.row_len = (int64_t)width * 3;
    P.n = P.row_len * rows;
    P.rows = rows;
    P.maxval = opt->maxval;
    P.clamp = opt->clamp != 0;
    P.gamma2 = opt->gamma2 != 0;
    P.flip = opt->flip_y != 0 && rows > 1;
    const bool two = opt->maxval >= 256;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!P.flip && aligned16(rgb_dev) && aligned16(out_dev)) {
        const int64_t lanes = (P.n + 15) / 16;
        const dim3 grid((unsigned)((lanes + BLOCK - 1) / BLOCK));
        if (two) hipLaunchKernelGGL(quantize_vec_kernel<2>, grid, dim3(BLOCK), 0, st, P);
        else hipLaunchKernelGGL(quantize_vec_kernel<1>, grid, dim3(BLOCK), 0, st, P);
    } else {
        const dim3 grid((unsigned)((P.n + BLOCK - 1) / BLOCK));
        if (two) hipLaunchKernelGGL(quantize_any_kernel<2>, grid, dim3(BLOCK), 0, st, P);
        else hipLaunchKernelGGL(quantize_any_kernel<1>, grid, dim3(BLOCK), 0, st, P);
    }
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

extern "C" int rt_unpermute_strips_device(const void* strips_dev, int strip_rows, size_t row_bytes, int height,
                                          int band_rows, int band_count, int flip_y, void* frame_dev,
                                          void* hip_stream) {
    if (!strips_dev || !frame_dev) return set_error(RT_ERR_ARG, "rt_unpermute_strips_device: null buffer");
    if (height <= 0 || row_bytes == 0 || band_rows <= 0 || band_count <= 0)
        return set_error(RT_ERR_ARG, "rt_unpermute_strips_device: bad shape");
    for (int r = 0; r < band_count; ++r)
        if (rt_shard_rows(height, band_rows, r, band_count) > strip_rows)
            return set_error(RT_ERR_ARG, "rt_unpermute_strips_device: strip_rows smaller than a rank's rows");
    UnpermuteParams P;
    P.strips = static_cast<const uint8_t*>(strips_dev);
    P.frame = static_cast<uint8_t*>(frame_dev);
    P.row_bytes = (int64_t)row_bytes;
    P.strip_stride = (int64_t)strip_rows * P.row_bytes;
    P.height = height;
    P.band_rows = band_rows;
    P.band_count = band_count;
    P.flip = flip_y != 0;
    P.vec = (row_bytes % 16) == 0 && aligned16(strips_dev) && aligned16(frame_dev);
    hipLaunchKernelGGL(unpermute_kernel, dim3((unsigned)height), dim3(BLOCK), 0,
                       static_cast<hipStream_t>(hip_stream), P);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}
