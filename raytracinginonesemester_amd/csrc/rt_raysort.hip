// rt_raysort.hip — sorting caller rays for coherence on the device: the key of a
// ray (rt_raysort.hpp), a stable sort of the ray indices by key, and the gather / scatter that move
// per-ray arrays into and out of that order.  Nothing here reads a scene: the calls run on any
// stream beside frames and queries.
//
//  * ray_keys_kernel: one ray per lane; a lane reads its 24 bytes (three 8-byte words when the
//    array is 8-byte aligned, a wave's 1,536 bytes contiguous either way), writes its key and,
//    for the sort, its own index.
//  * the sort: rocprim::radix_sort_pairs over exactly the key's bits, stable, (key, index) pairs
//    with the indices in ascending order on entry, so equal keys keep increasing index and the
//    order is unique (as the LBVH build sorts its Morton codes, rt_lbvh.hip).
//  * permute_kernel: out[k] = in[order[k]] (gather) or out[order[k]] = in[k] (scatter) for
//    elements of 4..64 bytes.  An element is W units of 16, 8 or 4 bytes (the widest that its
//    size and both addresses allow); a block owns 256 consecutive k and its lanes walk the
//    256 * W units of that range in order, so the contiguous side is read or written as whole
//    consecutive units by consecutive lanes, and the W lanes of an element touch its W
//    consecutive units on the indexed side (one access of the element's bytes per index).
//    An index >= n is skipped, so no order can make the kernels leave their arrays.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>

#include "rt_common.hpp"
#include "rt_hip_host.hpp"
#include "rt_raysort.hpp"

using rt::set_error;
using rt::hip_msg;
using rt::DeviceGuard;

namespace {

constexpr int BLOCK = 256;
constexpr size_t MAX_N = 0x7FFFFFFFull;

struct Box6 {
    float v[6];
};

template <bool A8>
__global__ __launch_bounds__(BLOCK) void ray_keys_kernel(const float* __restrict__ rays, uint32_t n, Box6 box, int mode,
                                                         int bits, uint32_t* __restrict__ keys,
                                                         uint32_t* __restrict__ order) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    float r[6];
    if (A8) {
        const float2* p = reinterpret_cast<const float2*>(rays) + 3 * (size_t)i;
        const float2 a = p[0], b = p[1], c = p[2];
        r[0] = a.x, r[1] = a.y, r[2] = b.x, r[3] = b.y, r[4] = c.x, r[5] = c.y;
    } else {
        const float* p = rays + 6 * (size_t)i;
#pragma unroll
        for (int k = 0; k < 6; ++k) r[k] = p[k];
    }
    keys[i] = rts::ray_key(r, box.v, mode, bits);
    if (order) order[i] = i;
}

template <class T, bool SCATTER>
__global__ __launch_bounds__(BLOCK) void permute_kernel(const T* __restrict__ in, const uint32_t* __restrict__ order,
                                                        T* __restrict__ out, uint32_t n, uint32_t w, uint32_t inv) {
    const size_t e0 = (size_t)blockIdx.x * BLOCK;
    const uint32_t left = n - (uint32_t)e0;
    const uint32_t nu = (left < (uint32_t)BLOCK ? left : (uint32_t)BLOCK) * w;
    const size_t u0 = e0 * w;
#pragma unroll 4
    for (uint32_t u = threadIdx.x; u < nu; u += BLOCK) {
        const uint32_t e = rts::div_small(u, inv), r = u - e * w;
        const uint32_t o = order[e0 + e];
        if (o >= n) continue;
        const size_t far = (size_t)o * w + r;
        if (SCATTER) out[far] = in[u0 + u];
        else out[u0 + u] = in[far];
    }
}

unsigned grid_of(size_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && na && nb && x < y + nb && y < x + na;
}
bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// mode / bits / count rules shared by the key and sort calls (n == 0 is then RT_OK whatever the
// pointers); *kb receives the key's bits.
int key_args(const char* who, size_t n, int mode, int bits, int* kb) {
    *kb = rts::key_bits(mode, bits);
    if (*kb == 0)
        return set_error(RT_ERR_ARG, std::string(who) + ": mode must be RT_SORT_ORIGIN (bits 1..10) or RT_SORT_ORIGIN_DIR (bits 1..5)");
    if (n > MAX_N) return set_error(RT_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31-1 rays in one batch");
    return RT_OK;
}

Box6 box6(const rt_aabb* b) {
    return Box6{{b->min_corner.x, b->min_corner.y, b->min_corner.z, b->max_corner.x, b->max_corner.y, b->max_corner.z}};
}

void launch_keys(const rt_ray* rays, size_t n, int mode, int bits, const rt_aabb* box, uint32_t* keys, uint32_t* order,
                 hipStream_t st) {
    const float* r = reinterpret_cast<const float*>(rays);
    if (aligned(rays, 8))
        hipLaunchKernelGGL(ray_keys_kernel<true>, dim3(grid_of(n)), dim3(BLOCK), 0, st, r, (uint32_t)n, box6(box), mode, bits, keys, order);
    else
        hipLaunchKernelGGL(ray_keys_kernel<false>, dim3(grid_of(n)), dim3(BLOCK), 0, st, r, (uint32_t)n, box6(box), mode, bits, keys, order);
}

template <bool SCATTER>
void launch_permute(const void* in, size_t n, size_t elem_bytes, const uint32_t* order, void* out, hipStream_t st) {
    const dim3 grid(grid_of(n)), block(BLOCK);
    if (elem_bytes % 16 == 0 && aligned(in, 16) && aligned(out, 16)) {
        const uint32_t w = (uint32_t)(elem_bytes / 16);
        hipLaunchKernelGGL((permute_kernel<uint4, SCATTER>), grid, block, 0, st, static_cast<const uint4*>(in), order,
                           static_cast<uint4*>(out), (uint32_t)n, w, rts::div_inv(w));
    } else if (elem_bytes % 8 == 0 && aligned(in, 8) && aligned(out, 8)) {
        const uint32_t w = (uint32_t)(elem_bytes / 8);
        hipLaunchKernelGGL((permute_kernel<uint2, SCATTER>), grid, block, 0, st, static_cast<const uint2*>(in), order,
                           static_cast<uint2*>(out), (uint32_t)n, w, rts::div_inv(w));
    } else {
        const uint32_t w = (uint32_t)(elem_bytes / 4);
        hipLaunchKernelGGL((permute_kernel<uint32_t, SCATTER>), grid, block, 0, st, static_cast<const uint32_t*>(in), order,
                           static_cast<uint32_t*>(out), (uint32_t)n, w, rts::div_inv(w));
    }
}

template <bool SCATTER>
int permute_device(const char* who, int device, const void* in, size_t n, size_t elem_bytes, const uint32_t* order, void* out,
                   void* stream) {
    if (elem_bytes < 4 || elem_bytes > 64 || elem_bytes % 4 != 0)
        return set_error(RT_ERR_ARG, std::string(who) + ": elem_bytes must be a multiple of 4 in 4..64");
    if (n > MAX_N) return set_error(RT_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31-1 elements in one batch");
    if (n == 0) return RT_OK;
    if (!in || !order || !out) return set_error(RT_ERR_ARG, std::string(who) + ": null in, order or out");
    if (!aligned(in, 4) || !aligned(out, 4) || !aligned(order, 4))
        return set_error(RT_ERR_ARG, std::string(who) + ": a pointer is not 4-byte aligned");
    if (ranges_overlap(in, n * elem_bytes, out, n * elem_bytes)) return set_error(RT_ERR_ARG, std::string(who) + ": out overlaps in");
    int rc = rt::check_device(device);
    if (rc != RT_OK) return rc;
    DeviceGuard g(device);
    launch_permute<SCATTER>(in, n, elem_bytes, order, out, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// rt_ray_sort_device's scratch: three n-word arrays (keys, sorted keys, the ascending indices) and
// the sort's own storage, each from a 256-byte boundary.  The sort's need depends on the device's
// tuning of the library sort, so the reservation is a bound that does not: its two n-word
// temporaries, up to 2 bytes per item of per-block state (256 digits x 8 bytes per block of at
// least 1,024 items), and 64 KiB for digit tables and alignment.  rt_ray_sort_device asks the
// library for its actual need and refuses to run (RT_ERR_INTERNAL) should it ever be larger.
size_t align256(size_t b) { return (b + 255) & ~size_t(255); }
size_t sort_tmp_reserved(size_t n) { return align256(10 * n + 65536); }
size_t sort_scratch_bytes(size_t n) { return 256 + 3 * align256(4 * n) + sort_tmp_reserved(n); }

}  // namespace

extern "C" int rt_ray_key_bits(int mode, int bits) {
    const int kb = rts::key_bits(mode, bits);
    if (kb == 0) return set_error(RT_ERR_ARG, "rt_ray_key_bits: mode must be RT_SORT_ORIGIN (bits 1..10) or RT_SORT_ORIGIN_DIR (bits 1..5)");
    return kb;
}

extern "C" int rt_ray_keys_host(const rt_ray* rays, size_t n, int mode, int bits, const rt_aabb* box, uint32_t* keys) {
    int kb = 0;
    const int rc = key_args("rt_ray_keys_host", n, mode, bits, &kb);
    if (rc != RT_OK || n == 0) return rc;
    if (!rays || !box || !keys) return set_error(RT_ERR_ARG, "rt_ray_keys_host: null rays, box or keys");
    const Box6 b = box6(box);
    for (size_t i = 0; i < n; ++i) keys[i] = rts::ray_key(reinterpret_cast<const float*>(rays + i), b.v, mode, bits);
    return RT_OK;
}

extern "C" int rt_ray_sort_host(const rt_ray* rays, size_t n, int mode, int bits, const rt_aabb* box, uint32_t* order) {
    int kb = 0;
    const int rc = key_args("rt_ray_sort_host", n, mode, bits, &kb);
    if (rc != RT_OK || n == 0) return rc;
    if (!rays || !box || !order) return set_error(RT_ERR_ARG, "rt_ray_sort_host: null rays, box or order");
    std::vector<uint32_t> keys(n);
    const Box6 b = box6(box);
    for (size_t i = 0; i < n; ++i) keys[i] = rts::ray_key(reinterpret_cast<const float*>(rays + i), b.v, mode, bits);
    std::iota(order, order + n, 0u);
    std::stable_sort(order, order + n, [&](uint32_t x, uint32_t y) { return keys[x] < keys[y]; });
    return RT_OK;
}

extern "C" int rt_ray_keys_device(int device, const rt_ray* rays, size_t n, int mode, int bits, const rt_aabb* box,
                                  uint32_t* keys, void* stream) {
    int kb = 0;
    int rc = key_args("rt_ray_keys_device", n, mode, bits, &kb);
    if (rc != RT_OK || n == 0) return rc;
    if (!rays || !box || !keys) return set_error(RT_ERR_ARG, "rt_ray_keys_device: null rays, box or keys");
    if (!aligned(rays, 4) || !aligned(keys, 4)) return set_error(RT_ERR_ARG, "rt_ray_keys_device: a pointer is not 4-byte aligned");
    if ((rc = rt::check_device(device)) != RT_OK) return rc;
    DeviceGuard g(device);
    launch_keys(rays, n, mode, bits, box, keys, nullptr, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

extern "C" size_t rt_ray_sort_scratch_bytes(size_t n, int mode, int bits) {
    if (n == 0 || n > MAX_N || rts::key_bits(mode, bits) == 0) return 0;
    return sort_scratch_bytes(n);
}

extern "C" int rt_ray_sort_device(int device, const rt_ray* rays, size_t n, int mode, int bits, const rt_aabb* box,
                                  uint32_t* order, rt_ray* rays_out, void* scratch, void* stream) {
    int kb = 0;
    int rc = key_args("rt_ray_sort_device", n, mode, bits, &kb);
    if (rc != RT_OK || n == 0) return rc;
    if (!rays || !box || !order || !scratch) return set_error(RT_ERR_ARG, "rt_ray_sort_device: null rays, box, order or scratch");
    if (!aligned(rays, 4) || !aligned(order, 4) || !aligned(rays_out, 4))
        return set_error(RT_ERR_ARG, "rt_ray_sort_device: a pointer is not 4-byte aligned");
    if (ranges_overlap(rays, n * sizeof(rt_ray), rays_out, n * sizeof(rt_ray)))
        return set_error(RT_ERR_ARG, "rt_ray_sort_device: rays_out_dev overlaps rays_dev");
    if ((rc = rt::check_device(device)) != RT_OK) return rc;
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t cnt = (uint32_t)n;
    size_t need = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, need, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                      (uint32_t*)nullptr, cnt, 0u, (unsigned)kb, st));
    if (need > sort_tmp_reserved(n))
        return set_error(RT_ERR_INTERNAL, "rt_ray_sort_device: the library sort needs more storage than rt_ray_sort_scratch_bytes reserves");
    char* W = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(scratch) + 255) & ~uintptr_t(255));
    const size_t words = align256(4 * n);
    uint32_t* k0 = reinterpret_cast<uint32_t*>(W);
    uint32_t* k1 = reinterpret_cast<uint32_t*>(W + words);
    uint32_t* v0 = reinterpret_cast<uint32_t*>(W + 2 * words);
    launch_keys(rays, n, mode, bits, box, k0, v0, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::radix_sort_pairs(W + 3 * words, need, k0, k1, v0, order, cnt, 0u, (unsigned)kb, st));
    if (rays_out) {
        launch_permute<false>(rays, n, sizeof(rt_ray), order, rays_out, st);
        HIP_TRY(hipGetLastError());
    }
    return RT_OK;
}

extern "C" int rt_gather_device(int device, const void* in, size_t n, size_t elem_bytes, const uint32_t* order, void* out,
                                void* stream) {
    return permute_device<false>("rt_gather_device", device, in, n, elem_bytes, order, out, stream);
}

extern "C" int rt_scatter_device(int device, const void* in, size_t n, size_t elem_bytes, const uint32_t* order, void* out,
                                 void* stream) {
    return permute_device<true>("rt_scatter_device", device, in, n, elem_bytes, order, out, stream);
}
