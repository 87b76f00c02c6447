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
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

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
