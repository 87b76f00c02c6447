// rt_device.hip — the hot path on gfx950: camera ray -> BVH traversal -> Möller–Trumbore
// -> Lambert/Blinn-Phong with hard shadow rays (-> optional bounces), and the C-ABI
// entry points that own device memory.
//
// Reference path (G/ = HW2/HW2/GPUandCPU): render() CPU branch include/query.cu:130-166,
// TraceRayIterative query.h:156-220, SearchBVH query.h:224-311, ShadeDirect/IsInShadow
// shader.h:44-110, EvaluateBRDF brdf.h:12-40, Camera::get_ray camera.h:49-53.
//
// Device layout (built from the reference arrays by rt::pack_scene, rt_scene_pack.cpp):
//   inode[i]  64 B  children's AABBs + child refs of internal node i   (4 x float4)
//   ibox[i]   32 B  internal node i's own AABB (pop-time re-tests)      (2 x float4)
//   leaf[j]   64 B  v0, e1, e2, triangle index and the leaf's own AABB  (4 x float4)
//   tnorm[t]  48 B  n0, n1, n2 of triangle t (read once per hit)        (3 x float4)
// AABBs are stored as per-axis (min, max) pairs (BoxP), one packed FMA per axis.
// A child ref is an internal index, LEAF_BIT | leaf index, or NO_REF.
//
// Two traversal kernels, both bit-exact against the reference order:
//  * WAVE: one DFS per wavefront over a shared stack held in four VGPRs (entry k in lane
//    k, pushed with v_writelane, popped with v_readlane); each entry carries the 64-bit
//    mask of lanes that pushed it.  The reference's order (push left then right, pop
//    right first) is the same for every ray, so each lane sees exactly its own DFS as a
//    subsequence and makes every box/triangle decision with the same bestT the reference
//    would.  Node records are wave-uniform and come in through the scalar cache.
//  * LANE: one private stack per lane (the reference's structure, kept for A/B).
// Pop-time box re-tests are skipped when no lane's bestT changed since the push (the
// re-test would repeat the push-time computation with the same inputs).
//
// Source layout (round 6): this translation unit holds the render kernels and their host side
// (scenes, launches, frames).  Its device code is read in sections, each included at its place
// inside the anonymous namespace below (device functions are force-inlined into the render
// kernels, so they share one translation unit; the build has no device-side linking):
//   rt_wave.hpp        wavefront primitives, constant-space loads (also used by rt_hw1.hip)
//   rt_instrument.hpp  RT_STATS / RT_FRAME_SPAN / RT_WAVE_TIMES / RT_LANE_ITERS hooks (variant builds)
//   rt_traverse.hpp    the traversals (wave DFS, frustum, lane, LDS, deep)
//   rt_shade.hpp       hit resolution, materials, camera ray, shading, bounces, trace_sample
//   rt_prepass.hpp     tile bounds, root and tree-cut culling passes, work lists
//   rt_query.hpp       batched ray queries on a resident scene (rt_trace_rays*, rt_shade_rays*, rt_trace_hits*)
//   rt_multihit.hpp    multi-hit queries (rt_trace_multi_hits*)
//   rt_closest.hpp     closest-point queries (rt_closest_points*)
//   rt_path.hpp        path stages for caller hits (rt_path_*): step, begin, compaction, finish
//   rt_softshadow.hpp  spherical area lights for the staged path (rt_light_visibility_*, rt_path_step_vis_*)
//   rt_refit.hpp       refit of a resident scene for deforming geometry (rt_scene_refit*), mesh -> triangles
//   rt_rebuild.hpp     rebuild of a resident scene (rt_scene_rebuild*): the record weight on the device
//   rt_scan.hpp        the compaction's scan of tile counts (through rt_path.hpp; also used by rt_frame.hip)
// The host side of the caller queries is a section too, included after rt_scene and scene_view:
//   rt_query_host.hpp  rt_trace_rays*, rt_shade_rays*, rt_trace_hits*, rt_trace_multi_hits*, rt_closest_points*,
//                      rt_camera_rays*, rt_path_*, rt_light_*: checks, launches, staged forms, host builds
//                      
// Separate translation units: rt_scene_pack.cpp (the host half of rt_scene_create: checks, ids,
// stack bounds, every packed array), rt_records.cpp (host record builders), rt_hw1.hip (the HW1
// path), rt_frame.hip, rt_lbvh.hip, rt_renderer.hip.

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <functional>
#include <memory>
#include <new>
#include <string>
#include <array>
#include <vector>

#include "rt_common.hpp"
#include "rt_hip_host.hpp"
#include "rt_math.hpp"
#include "rt_ppm.hpp"
#include "rt_scene_pack.hpp"
#include "rt_tilediv.hpp"

using namespace rtd;

namespace {

// the constants the packed layout shares with its host builders (rt_records.hpp)
using rt::LEAF_BIT;
using rt::NO_REF;
using rt::FRUSTUM_STACK;
using rt::STACK_CAP;
using rt::LANE_LDS_CAP;
using rt::kBigSceneBytes;
constexpr uint32_t RT_FAULT_FRUSTUM_STACK = 1u;  // rt_scene_faults bit 0
constexpr uint32_t VER_FORCE = 0xFFFFFFFFu;   // pop must re-test (root)
constexpr int BLOCK = 256;
// Kernel instantiation flag on top of RT_KERNEL_WAVE: traverse the 4-ary records (SceneView::wide).
// A compile-time choice, so each kernel holds one traversal loop per ray kind.
constexpr int MODE_WIDE = 16;
constexpr int MODE_PK = 32;  // the wave traversal's box tests in packed FMAs (box_ends_pk): depth-1 kernels
// Trees whose DFS needs more than STACK_CAP entries: SearchBVH literally, per lane, with the
// reference's 512-entry stack, its overflow rule and brute-force completion (traverse_deep).
constexpr int MODE_DEEP = 64;
// The depth-1 kernels' one-light form: the scene has exactly one light, so shade_d1 has no light
// loop (whose loop-carried values spilled in the big-scene 8-wave build).
constexpr int MODE_1L = 128;
// The big-scene kernels' frustum traversal over the quantised records (qent/qhdr: 16 B per entry
// instead of 32; build_quant_records)
constexpr int MODE_QR = 256;
constexpr int REF_STACK = 512;                // query.h:245
constexpr uint32_t INV_LEAF = 0xFFFFFFFEu;    // deep stack entry: a leaf naming no triangle (query.h:263)
constexpr uint32_t BRUTE_BIT = 0x40000000u;   // HitState::slot of a brute-force hit: BRUTE_BIT | triangle
constexpr float RT_EPS = 1e-3f;               // shader.h:22

struct DevMaterial {  // rt_material, read through a 4-byte aligned pointer
    float albedo[3], kd, spec[3], ks, shininess, kr, emission[3];
};
struct DevLight {
    float pos[3], color[3];
    int32_t intensity;
};

struct SceneView {
    const float4* __restrict__ inode;
    const float4* __restrict__ wnode;  // 4-ary records (8 x float4) by internal index, if wide
    const float* __restrict__ fnode;   // 2^f_log2-ary records (8 x 2^f_log2 floats) of traverse_frustum, or null
    int32_t f_log2;                    // 3..5 with fnode; 2: traverse_frustum takes wnode
    const uint4* __restrict__ qent;    // fnode's records quantised (MODE_QR kernels): 2^f_log2 x 16 B each
    const float4* __restrict__ qhdr;   // their grids: (origin xyz, step x | step yz, -, -) per record
    const float4* __restrict__ ibox;
    const float4* __restrict__ rootb;  // the root's box, pairs (x | y, z), after ibox's entries
    const float4* __restrict__ leaf;
    const float4* __restrict__ tnorm;
    const int32_t* __restrict__ objids;
    const DevMaterial* __restrict__ mats;
    const DevLight* __restrict__ lights;
    int32_t num_tris, num_mats, num_lights;
    uint32_t root_ref;
    float root_box[6];
    float bmax[3];  // per axis max |coordinate| over every AABB of the scene (make_ray)
    int32_t wide;
    int32_t lane_stack;  // the binary DFS fits LANE_LDS_CAP entries: bounce rays take traverse_lane_lds
    int32_t lane_wide;   // ... and the 4-ary DFS fits them too: traverse_lane_lds_wide
    const float* __restrict__ cut;  // tile culling: boxes of a cut of the tree (6 floats each)
    int32_t ncut;
    const float* __restrict__ cut2;  // 2^cut_sub_log2 boxes of a cut of each cut box's subtree
    int32_t cut_sub_log2;            // 0: no second level
    const float4* __restrict__ tri;  // deep trees: v0 | e1, e2.x | e2.y, e2.z by triangle index (brute force)
    uint32_t* fault;  // RT_FAULT_* bits the kernels OR in (rt_scene_faults)
};

__device__ __forceinline__ f3 scene_bmax(const SceneView& sc) { return mk(sc.bmax[0], sc.bmax[1], sc.bmax[2]); }

struct RenderParams {
    SceneView sc;
    f3 cam_center, cam_p00, cam_du, cam_dv;
    int32_t W, H, spp, max_depth, diffuse_bounce;
    f3 miss;
    const float* __restrict__ jitter;  // 2*spp (device)
    int32_t band_rows, band_index, band_count, rows;  // rows = local rows rendered
    int32_t tile_w, tile_h, tiles_x, tiles_total;     // pixel tile per block
    int32_t lane_samples;                             // 1: one sample per lane; else pixel loop
    int32_t half_waves;                               // samples kernel: lanes >= 64 >> half_waves idle
    int32_t paired_only;                              // multi-bounce, half waves, one light: LS = 3 kernels
    int32_t tile_order;                               // RT_TILES_*
    int32_t spp_log2, tile_w_log2;                    // samples kernel: both powers of two
    int32_t cull;                                     // tile culling against the root box
    f3 miss_pixel;                                    // pixel value when all spp samples miss
    uint32_t* live_count;                             // [k * COUNTER_STRIDE], tile_cull_kernel
    int32_t* live_tiles;                              // nqueues lists of queue_cap entries
    int32_t* cut_tiles;   // tile_cut_kernel's survivors (not culled, not heavy), per list (sc.ncut > 0)
    uint32_t* next_count; // the counter set of the frame after next, zeroed by tile_cull_kernel
    int32_t cut_force;    // test every candidate in tile_cut_kernel (no pass-through)
    int32_t nqueues;
    int32_t queue_cap;
    uint32_t tiles_x_mul;  // tile / tiles_x without the division: TileDiv{tiles_x_mul, tiles_x_shift} (rt_tilediv.hpp)
    float* __restrict__ rgb;
    int32_t* __restrict__ hit_idx;
    float* __restrict__ hit_t;
    uint8_t* __restrict__ p6;  // optional: write_p6-default samples of the pixels (rows*W*3 bytes)
    uint8_t miss_p6[4];        // the culled pixels' samples
    uint32_t tiles_x_shift;
    // Heavy-first dispatch (speed only, an approximate longest-first schedule): render waves
    // record their duration per tile (tile_cost, 4 x u16 per tile, 10 ns ticks); the next frame's
    // cut pass moves tiles whose last cost is >= heavy_ticks[c] (descending) to list q's class-c
    // heavy list (heavy_tiles, heavy_cap entries per (class, list), lengths in counter slots
    // heavy_counter(c, q)).  Each work queue hands out its list's heavy entries first, heaviest
    // class first, so the longest tiles start first (render_tiles_kernel).  heavy_cap == 0: off.
    uint16_t* __restrict__ tile_cost;
    int32_t* heavy_tiles;
    int32_t heavy_cap;
    uint32_t heavy_ticks[8];  // NCLASS thresholds, descending
    // rt_count_rays only (LANE and DEEP kernels; null otherwise): [1] shadow rays cast, [2]
    // bounce rays traced, the classes of the oracle's orc_stats.rays ([0], camera rays, is
    // W*H*spp by definition and counted on the host), [3] camera rays of the tiles the culling
    // passes left to the render kernel (the camera rays that are actually traversed)
    unsigned long long* ray_count;
    // The pre-pass gate (RT_TUNE_PREPASS_GATE): the first waves to find their queue drained
    // store drain_tag into this host word, and the next frame's pre-passes wait for it on the
    // prep stream (hipStreamWaitValue32), so they take wave slots in this kernel's tail instead
    // of racing its grid for them at its start.  Null: no gate.
    uint32_t* drained;
    uint32_t drain_tag;
    int32_t gate_q8;  // the gate opens when a queue has handed out gate_q8/256 of its items (256: drained)
};
// tiles_x_mul and tiles_x_shift sit in two of the struct's alignment holes: every other field,
// and the kernel arguments after a RenderParams, keep the offsets the pre-pass kernels read
static_assert(sizeof(RenderParams) == 544, "RenderParams: a field moved");

#include "rt_wave.hpp"
#include "rt_instrument.hpp"
#include "rt_traverse.hpp"
#include "rt_shade.hpp"
#include "rt_prepass.hpp"
#include "rt_query.hpp"
#include "rt_multihit.hpp"
#include "rt_closest.hpp"
#include "rt_path.hpp"
#include "rt_softshadow.hpp"
#include "rt_refit.hpp"
#include "rt_rebuild.hpp"

// The render kernel's work: list q's entries, its heavy lists' first (classes in order,
// heaviest first; each capped at heavy_cap), then its survivors (the cut pass's list, or the
// cull pass's live list when there is no cut).  The lists are immutable while the render
// kernel runs, so their lengths and entries are read through the constant address space
// (scalar loads).
__device__ __forceinline__ int work_length(const RenderParams& P, int q, int& heavy) {
    heavy = 0;
    if (P.heavy_cap > 0)
        for (int k = 0; k < NCLASS; ++k) heavy += min((int)ldc_u32(P.live_count + heavy_counter(k, q)), P.heavy_cap);
    const int slot = P.sc.ncut > 0 ? CUT_SLOT0 + q : q;
    return heavy + (int)ldc_u32(&P.live_count[slot * COUNTER_STRIDE]);
}

// cls: the entry's heavy class (0 heaviest), NCLASS for a survivor.
__device__ __forceinline__ int work_tile(const RenderParams& P, int q, int e, int heavy, int& cls) {
    const uint32_t* list;
    cls = NCLASS;
    if (e < heavy) {
        int k = 0;
        for (; k < NCLASS - 1; ++k) {
            const int n = min((int)ldc_u32(P.live_count + heavy_counter(k, q)), P.heavy_cap);
            if (e < n) break;
            e -= n;
        }
        list = reinterpret_cast<const uint32_t*>(P.heavy_tiles) + ((size_t)k * 8 + q) * P.heavy_cap;
        cls = k;
    } else {
        e -= heavy;
        list = reinterpret_cast<const uint32_t*>(P.sc.ncut > 0 ? P.cut_tiles : P.live_tiles) + (size_t)q * P.queue_cap;
    }
    return (int)ldc_u32(list + e);
}

// The next work item of a queue: one returning device-scope atomic from lane 0 (a vector
// atomic), the value made wave-uniform.
__device__ __forceinline__ uint32_t dequeue(uint32_t* head, uint32_t lane) {
    uint32_t v = 0;
    if (lane == 0) v = __hip_atomic_fetch_add(head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return uni(v);
}

// One sample per lane: a block covers a tile_w x tile_h pixel tile x spp samples (spp a power
// of two <= 256, tile_w*tile_h*spp == BLOCK); per-pixel sums run in sample order from LDS.
template <int MODE, bool D1, int LS = 0>
// qw: the wave's quarter of the tile (its work item); LDS is indexed by the thread's own slot,
// t (the thread index, made afresh for each item).
__device__ __forceinline__ void samples_tile(const RenderParams& P, int tile, uint32_t qw, int t, float* col,
                                             int* kpix, float* park, const int* lds_zero) {
    const uint32_t wv = uni((uint32_t)t) >> 6;  // the wave's index in the block (an SGPR)
    // LS = 1, half waves (band shards of a multi-GPU frame, spp <= 32; the bounce kernels'
    // unpaired loop): each wave traces 32
    // samples in its low lanes, so a tile's longest wave, which bounds a short kernel, has half
    // the rays' path union; lt is the sample's index in the (half-size) tile.  A template
    // parameter: a run-time flag here cost the full-wave c3 kernel 0.8 % (register allocation).
    constexpr int wl = LS != 0 ? 32 : 64;  // lanes that trace
    const bool on = (t & 63) < wl;
    const int lt = ((int)qw * wl) | (t & (wl - 1));
    bool all_miss = false;  // wave-uniform, known after the shading
    {
        const int s = lt & (P.spp - 1);  // spp and tile_w are powers of two here
        const int pit = lt >> P.spp_log2;
        // The depth-1 kernels split the tile index by the host's multiplier and shift
        // (rt_tilediv.hpp); the bounce kernels stay instruction for instruction what they were.
        int tx, ty;
        if constexpr (D1) {
            ty = (int)tile_div((uint32_t)tile, TileDiv{P.tiles_x_mul, P.tiles_x_shift});
            tx = tile - ty * P.tiles_x;
        } else {
            tx = tile % P.tiles_x;
            ty = tile / P.tiles_x;
        }
#ifndef RT_ROW_PIXELS
        // Pixels in Z order inside a square tile (a wave's pixels form a square: 2x2 at 16 spp,
        // more coherent rays than a row of 4); row-major otherwise.  Any order gives the same
        // image: each sample is independent and each pixel's samples stay consecutive lanes.
        int px, py;
        if (P.tile_w == P.tile_h) {
            px = (pit & 1) | ((pit >> 1) & 2) | ((pit >> 2) & 4) | ((pit >> 3) & 8);
            py = ((pit >> 1) & 1) | ((pit >> 2) & 2) | ((pit >> 3) & 4) | ((pit >> 4) & 8);
        } else {
            px = pit & (P.tile_w - 1);
            py = pit >> P.tile_w_log2;
        }
#else
        const int px = pit & (P.tile_w - 1), py = pit >> P.tile_w_log2;
#endif
        const int x = tx * P.tile_w + px;
        const int r = ty * P.tile_h + py;
        const bool valid = on && x < P.W && r < P.rows;
        const int y = valid ? global_row(P, r) : 0;
        const int pix = valid ? r * P.W + x : -1;
        // The pixel's index goes through LDS (read back below), so the compiler does not keep
        // it, or addresses made from it, live (and spilled) across the shading.
        if (s == 0) kpix[t >> P.spp_log2] = pix;
        const int64_t aov = valid && P.hit_idx ? (int64_t)pix * P.spp + s : -1;
        if constexpr (D1) RT_PHASE_ITEM(park + (wv << 6), (uint32_t)tile * (BLOCK / 64) + qw);
        const f3 c = trace_sample<MODE, D1, LS == 3 ? 2 : 0>(P, valid, x, y, s, aov, park + t,
                                                                             park + (wv << 6));
        if constexpr (D1) RT_PHASE(park + (wv << 6), 1);
        // A depth-1 wave none of whose lanes hit (spp <= 64: its pixels are its own) has the pixel
        // the host knows, P.miss_pixel: the same ordered sum of clamp01(miss), then * 1/spp
        // (miss_pixel_value; the cull pass writes it to the tiles it culls).  Such a wave stores
        // no samples and sums none.
        if constexpr (D1) all_miss = P.spp <= 64 && !d1_wave_hit(park + (wv << 6));
        if (!all_miss) {
            // The thread index again, from the wave's index and a lane id the compiler cannot
            // merge with the first one (mbcnt of a zero read back from LDS): keeping t itself live
            // across the traversals cost a 4-byte scratch spill per lane (c3: ~8 MB of writes per
            // launch).
            const int te = (int)((wv << 6) | __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(
                                                      ~0u, (uint32_t)*(const volatile int*)lds_zero)));
            col[3 * te] = c.x;
            col[3 * te + 1] = c.y;
            col[3 * te + 2] = c.z;
        }
    }
    const int t2 = (int)((wv << 6) | __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(
                                             ~0u, (uint32_t)*(const volatile int*)lds_zero)));
    if (P.spp <= 64) {
        // A pixel's samples are consecutive lanes of one wave: only this wave's LDS writes are
        // read below, so the wave synchronises alone (its siblings in the block may still be
        // tracing; a block barrier here cost 13 % of the waves' time on c3).
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();  // a pixel's samples span the block's waves
    }
    // The depth-1 kernels' wave-level epilogue; the bounce kernels keep the sum below.
    if (D1 && P.spp <= 64) {
        // One lane per (channel, pixel of the wave): 12 lanes at 16 spp, each adding its
        // channel's samples in sample order (col = col + TraceRayIterative(...), then col /
        // float(spp)): the additions and their order are those of one lane per pixel.
        const int ppw_log2 = 6 - P.spp_log2;  // pixels per wave
        // 1 / spp, exact: spp is a power of two here.  x / 2^k and x * 2^-k are the same
        // correctly rounded value (the exact quotients are equal), so the divide is a multiply.
        const float rs = __int_as_float((127 - P.spp_log2) << 23);
        for (int i = t2 & 63; i < (3 << ppw_log2); i += 64) {
            const int ch = i >> ppw_log2, pw = i & ((1 << ppw_log2) - 1);
            const int pix = kpix[(int)(wv << ppw_log2) + pw];
            if (pix < 0) continue;
            const size_t k = (size_t)pix * 3 + ch;
            if (all_miss) {
                // the three values as scalars, the lane's chosen among them (a select between the
                // fields themselves became a per-lane load from the argument segment)
                const uint32_t m0 = uni((uint32_t)__float_as_int(P.miss_pixel.x)),
                               m1 = uni((uint32_t)__float_as_int(P.miss_pixel.y)),
                               m2 = uni((uint32_t)__float_as_int(P.miss_pixel.z));
                uint32_t b;  // the four bytes as one word (a scalar load; single bytes load per lane)
                __builtin_memcpy(&b, P.miss_p6, sizeof(b));
                b = uni(b);
                if (P.rgb) P.rgb[k] = __int_as_float((int)(ch == 0 ? m0 : ch == 1 ? m1 : m2));
                if (P.p6) P.p6[k] = (uint8_t)(b >> (8 * ch));
                continue;
            }
            const float* sp = col + 3 * (int)((wv << 6) + ((uint32_t)pw << P.spp_log2)) + ch;
            // the samples are read sixteen (four) at a time and then added in order: one LDS round
            // trip per group instead of one per sample
            float acc = 0.f;
            int j = 0;
            for (; j + 16 <= P.spp; j += 16) {
                float s[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) s[u] = sp[3 * (j + u)];
#pragma unroll
                for (int u = 0; u < 16; ++u) acc = acc + s[u];
            }
            for (; j + 4 <= P.spp; j += 4) {
                float s[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) s[u] = sp[3 * (j + u)];
#pragma unroll
                for (int u = 0; u < 4; ++u) acc = acc + s[u];
            }
            for (; j < P.spp; ++j) acc = acc + sp[3 * j];
            const float v = acc * rs;
            if (P.rgb) P.rgb[k] = v;
            if (P.p6) P.p6[k] = rtp::p6_default_sample(v);  // the frame epilogue fused in (write_p6 defaults)
        }
        if constexpr (D1) RT_PHASE(park + (wv << 6), 3);
        return;
    }
    if ((t2 & (P.spp - 1)) == 0) {
        const int pix = kpix[t2 >> P.spp_log2];
        if (pix >= 0) {
            // col = col + TraceRayIterative(...) in sample order, then col / float(spp)
            f3 acc = mk(0.f, 0.f, 0.f);
            for (int k = 0; k < P.spp; ++k)
                acc = add(acc, mk(col[3 * (t2 + k)], col[3 * (t2 + k) + 1], col[3 * (t2 + k) + 2]));
            // x / 2^k and x * 2^-k are the same correctly rounded value (the exact quotients
            // are equal), so the power-of-two divide is a multiply here.
            const float rs = 1.0f / (float)P.spp;
            const size_t k = (size_t)pix * 3;
            const f3 px = mk(acc.x * rs, acc.y * rs, acc.z * rs);
            if (P.rgb) {
                P.rgb[k] = px.x;
                P.rgb[k + 1] = px.y;
                P.rgb[k + 2] = px.z;
            }
            if (P.p6) {  // the frame epilogue fused in (write_p6 defaults)
                P.p6[k] = rtp::p6_default_sample(px.x);
                P.p6[k + 1] = rtp::p6_default_sample(px.y);
                P.p6[k + 2] = rtp::p6_default_sample(px.z);
            }
        }
    }
    if constexpr (D1) RT_PHASE(park + (wv << 6), 3);
}

// General spp: one pixel per lane looping over its samples in order (query.cu:146-163).
template <int MODE, bool D1>
__device__ __forceinline__ void pixels_tile(const RenderParams& P, int tile, uint32_t qw, int tid, float* park) {
    const int t = (int)((qw << 6) | (tid & 63));
    const int tx = tile % P.tiles_x, ty = tile / P.tiles_x;
    const int x = tx * P.tile_w + t % P.tile_w;
    const int r = ty * P.tile_h + t / P.tile_w;
    const bool valid = x < P.W && r < P.rows;
    const int y = valid ? global_row(P, r) : 0;
    f3 acc = mk(0.f, 0.f, 0.f);
    if constexpr (D1) RT_PHASE_ITEM(park + (uni((uint32_t)tid) & ~63u), (uint32_t)tile * (BLOCK / 64) + qw);
    for (int s = 0; s < P.spp; ++s) {
        const int64_t aov = valid && P.hit_idx ? ((int64_t)r * P.W + x) * P.spp + s : -1;
        acc = add(acc, trace_sample<MODE, D1>(P, valid, x, y, s, aov, park + tid, park + (uni((uint32_t)tid) & ~63u)));
    }
    if (valid) {
        const float fs = (float)P.spp;
        const size_t k = ((size_t)r * P.W + x) * 3;
        const f3 px = mk(acc.x / fs, acc.y / fs, acc.z / fs);
        if (P.rgb) {
            P.rgb[k] = px.x;
            P.rgb[k + 1] = px.y;
            P.rgb[k + 2] = px.z;
        }
        if (P.p6) {
            P.p6[k] = rtp::p6_default_sample(px.x);
            P.p6[k + 1] = rtp::p6_default_sample(px.y);
            P.p6[k + 2] = rtp::p6_default_sample(px.z);
        }
    }
}

// A persistent grid (the blocks one dispatch keeps resident) over per-XCD work queues: block b
// serves queue g = b % 8 (dispatch deals blocks round-robin over the XCDs, so queue g is served
// on XCD g and list g's tiles share an L2).  With 8 lists queue g is list g; with one list
// (RT_TILES_LINEAR) queue g takes the list's entries g, g+8, ....  Each wave dequeues its own
// item, a quarter of a tile (BLOCK / 64 waves per tile), so a wave that finishes early takes
// the next quarter at once; with spp > 64 a pixel's samples span the block's waves and the
// block takes whole tiles.  (One block per live-list slot of a frame-sized virtual grid, empty
// blocks leaving at once, cost c3 0.207 ms vs 0.183 for a grid sized exactly to the lists read
// back on the host: the ~10^5 empty blocks' dispatch is not free; the queues need neither.)
#ifndef RT_RENDER_WAVES
#define RT_RENDER_WAVES 7
#endif
// The multi-bounce kernels (D1 false): the bounce loop keeps more state live than the depth-1
// shading (RNG, throughput, the ray, two rays' RayPre, the 4-ary record in the lane traversal).
// c3b with the lane traversal over 4-ary records: 2.26 ms at 3 waves (167 VGPRs, no scratch)
// vs 2.81 at 4 (164 B scratch); binary records at 4 waves 3.20 (profiles/r03/exp/).
#ifndef RT_BOUNCE_WAVES
#define RT_BOUNCE_WAVES 3
#endif
// Scenes whose data (records, leaves, normals) exceed kBigSceneBytes do not stay in the L2s and
// MALL: their depth-1 wave kernels run 8 waves per SIMD (64 VGPRs, a few spills outside the
// traversal loops), more waves to hide the record loads' latency (c5, 345 MB: DESIGN.md §4.2).
// RT_TUNE_BIG_SCENE_BYTES (rt_tuning_set) overrides the threshold (A/B).
// The paired-only bounce kernels (one light, half waves: paired_bounces and nothing else).
#ifndef RT_PAIRED_WAVES
#define RT_PAIRED_WAVES 4
#endif
#ifndef RT_RENDER_WAVES_BIG
#define RT_RENDER_WAVES_BIG 8
#endif
// Two frames in one launch (RT_TUNE_PAIR_FRAMES, rt_renderer_submit_pair): frame A's parameters,
// then frame B's, one kernel argument.
struct PairParams {
    RenderParams f[2];
};

// Two frames in one render launch (render_pair_kernel) take their pre-passes in one launch
// each too: four dependent launches in the previous pair kernel's tail measured 51 us between
// pair kernels (profiles/r05/exp/pair_timeline_c3.log).  The frames' counter sets and lists are
// disjoint (a cull pass zeroes the set two frames ahead, rt_scene::kSets).
// tile_cull_kernel over both frames: frame A's blocks, then frame B's.
__global__ __launch_bounds__(BLOCK) void tile_cull_pair_kernel(PairParams PP) {
    __builtin_amdgcn_s_setprio(3);
    const int nba = (PP.f[0].tiles_total + BLOCK - 1) / BLOCK;
    const bool b = (int)blockIdx.x >= nba;
    const RenderParams& P = b ? PP.f[1] : PP.f[0];
    const int bx = b ? (int)blockIdx.x - nba : (int)blockIdx.x;
    if (bx == 0 && threadIdx.x < COUNTER_SLOTS) P.next_count[threadIdx.x * COUNTER_STRIDE] = 0u;
    cull_tiles(P, bx * BLOCK + (int)threadIdx.x);
}

// tile_cut_kernel over both frames: the even waves take frame A's (list, group) units, the odd
// waves frame B's, so a wave of this grid has about one unit (a wave that took its units of A
// and then of B made the chain two units long).
__global__ __launch_bounds__(BLOCK) void tile_cut_pair_kernel(PairParams PP) {
    __shared__ CutScratch scratch[BLOCK / 64];
    __builtin_amdgcn_s_setprio(3);
    const uint32_t lane = lane_id();
    const int wib = (int)uni(threadIdx.x / 64);  // (wave-uniform, and known to be)
    const int wave = (int)(blockIdx.x * (BLOCK / 64)) + wib;
    const int waves = (int)(gridDim.x * (BLOCK / 64)) / 2;
    const RenderParams& P = (wave & 1) ? PP.f[1] : PP.f[0];
    float box[6] = {0.f, 0.f, 0.f, -1.f, -1.f, -1.f};
    int max_len;
    const bool test = cut_setup(P, lane, box, max_len);
    for (int p = wave >> 1;; p += waves) {
        const int q = p % P.nqueues, g = p / P.nqueues;
        if (CUT_GROUP * g >= max_len) break;
        (void)cut_unit(P, lane, q, g, test, box, scratch[wib]);
    }
}

// The pair kernel's item e of queue q: the two frames' heavy lists class by class (A's class k,
// then B's, so the heaviest items of both start first), then A's survivors, then B's.  which:
// the frame; returns the tile, cls its class as work_tile's.
__device__ __forceinline__ int pair_tile(const RenderParams& A, const RenderParams& B, int q, int e, int& which,
                                         int& cls) {
    for (int k = 0; k < NCLASS; ++k) {
        const int na = A.heavy_cap > 0 ? min((int)ldc_u32(A.live_count + heavy_counter(k, q)), A.heavy_cap) : 0;
        if (e < na) {
            which = 0;
            cls = k;
            return (int)ldc_u32(reinterpret_cast<const uint32_t*>(A.heavy_tiles) + ((size_t)k * 8 + q) * A.heavy_cap + e);
        }
        e -= na;
        const int nb = B.heavy_cap > 0 ? min((int)ldc_u32(B.live_count + heavy_counter(k, q)), B.heavy_cap) : 0;
        if (e < nb) {
            which = 1;
            cls = k;
            return (int)ldc_u32(reinterpret_cast<const uint32_t*>(B.heavy_tiles) + ((size_t)k * 8 + q) * B.heavy_cap + e);
        }
        e -= nb;
    }
    cls = NCLASS;
    const int ra = (int)ldc_u32(&A.live_count[(A.sc.ncut > 0 ? CUT_SLOT0 + q : q) * COUNTER_STRIDE]);
    which = e < ra ? 0 : 1;
    const RenderParams& X = e < ra ? A : B;
    if (e >= ra) e -= ra;
    return (int)ldc_u32(reinterpret_cast<const uint32_t*>(X.sc.ncut > 0 ? X.cut_tiles : X.live_tiles) +
                        (size_t)q * X.queue_cap + e);
}

// Heavy-first dispatch: the queues hand out the heavy lists first; the waves record their
// items' costs.  PAIR: the kernel argument is a PairParams; the items of both frames come from
// frame A's queue heads (pair_tile), and frame B's parameters carry the pre-pass gate.
template <int MODE, bool SAMPLES, bool D1, int WAVES, int LS, bool PAIR>
__device__ __forceinline__ void render_tiles_body() {
    constexpr int WPT = BLOCK / 64;  // waves per tile
    __shared__ float col[SAMPLES ? BLOCK * 3 : 1];
    __shared__ int kpix[SAMPLES ? BLOCK : 1];
    // D1: shade_d1's state across shadow rays; else (WAVE kernels) traverse_lane_lds's stacks
    __shared__ float park[D1 ? PARK_SLOTS * BLOCK
                             : (MODE == RT_KERNEL_LANE || (MODE & MODE_DEEP) != 0 ? 1 : LANE_LDS_CAP * BLOCK)];
    // the wave's item start time goes through LDS (an SGPR pair live across the whole tile spilled)
    __shared__ uint32_t t_start[WPT], t_item[WPT];
    __shared__ int lds_zero;  // 0, written by every lane (samples_tile's fresh lane id)
    __shared__ uint32_t block_item;  // spp > 64: the block's item
    if constexpr (SAMPLES) lds_zero = 0;
    // the wave's index in the block as a uniform value (threadIdx.x itself, kept live to the
    // tile-cost write at the end, was spilled to scratch)
    const uint32_t wv = uni((uint32_t)threadIdx.x) >> 6;
    // The first item of each wave (block) is its place in the grid, the rest come from the
    // queue after those: 900 dequeues per head at once when the grid starts took ~10 us to serve.
    for (bool first = true;; first = false) {
        // Everything the item needs is derived inside the loop from a laundered block index and
        // parameter pointer (the kernel's argument segment): hoisted out of the loop, the
        // parameters' loads and the values made from them stay live across every item and spill.
        typedef const __attribute__((address_space(4))) RenderParams* KernargP;
        KernargP pp = (KernargP)__builtin_amdgcn_kernarg_segment_ptr();
        uint32_t bx = blockIdx.x;
        asm volatile("" : "+s"(pp), "+s"(bx));
        const RenderParams& R0 = *(const RenderParams*)pp;
        const RenderParams& RG = PAIR ? *(const RenderParams*)(pp + 1) : R0;  // the gate's frame
        const int g = (int)(bx & 7);
        const int q = R0.nqueues == 1 ? 0 : g;
        uint32_t* head = R0.live_count + (HEAD_SLOT0 + g) * COUNTER_STRIDE;
        const bool blockwise = SAMPLES && R0.spp > 64;
        const uint32_t lane = fresh_lane_id();
        RT_HOOK_FRAME_FIRST(first, lane, RG);
        const int tid = (int)((wv << 6) | lane);
        const uint32_t per_queue = (gridDim.x >> 3) * (blockwise ? 1u : (uint32_t)WPT);  // first items
        uint32_t j;
        if (first) {
            j = (bx >> 3) * (blockwise ? 1u : (uint32_t)WPT) + (blockwise ? 0u : wv);
        } else if (blockwise) {
            // one barrier per item: the previous item's LDS reads finished at samples_tile's
            // own barrier, before thread 0 overwrites block_item
            if (tid == 0) block_item = dequeue(head, lane);
            __syncthreads();
            j = per_queue + uni(block_item);
        } else {
            j = per_queue + dequeue(head, lane);
        }
        int heavy;
        int n = work_length(R0, q, heavy);
        if constexpr (PAIR) {
            int hb;
            n += work_length(RG, q, hb);
        }
        const int e = (R0.nqueues == 1 ? g : 0) + (R0.nqueues == 1 ? 8 : 1) * (int)(blockwise ? j : j / WPT);
        // the waves at the queue's gate item (its items are handed out in order, so every queue
        // has them; gate_q8 = 256: the first waves past its end) open the next frame's
        // pre-passes (a vector store to host memory)
        if (RG.drained && lane == 0) {
            const int ge = (int)(((int64_t)n * RG.gate_q8) >> 8);
            if (e >= ge && e < ge + (R0.nqueues == 1 ? 8 : 1))
                __hip_atomic_store(RG.drained, RG.drain_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        if (e >= n) {
            RT_HOOK_FRAME_LAST(lane, RG);
            break;
        }
        const uint32_t qw = blockwise ? wv : j % WPT;
        int cls;
        KernargP pr = pp;  // the item's frame
        int tile;
        if constexpr (PAIR) {
            int which;
            tile = pair_tile(R0, RG, q, e, which, cls);
            pr = pp + which;
        } else {
            tile = work_tile(R0, q, e, heavy, cls);
        }
        const RenderParams& R = *(const RenderParams*)pr;
        // Issue priority by cost class: every SIMD keeps all its wave slots busy until the queues
        // drain, so the heaviest items (the kernel's critical path, started first) would share
        // their SIMD with six other waves throughout; ahead of the rest they finish sooner
        // (c3 0.182 vs 0.210 ms without priorities, 0.199 with class 0 alone raised).
        if (cls == 0) __builtin_amdgcn_s_setprio(3);
        else if (cls == 1) __builtin_amdgcn_s_setprio(2);
        else if (cls == 2) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
        RT_HOOK_ITEM_START(wt0);
        if (R.tile_cost && lane == 0) {
            t_start[wv] = (uint32_t)wall_clock64();
            t_item[wv] = (uint32_t)tile * WPT + qw;
        }
        if constexpr (SAMPLES) samples_tile<MODE, D1, LS>(R, tile, qw, tid, col, kpix, park, &lds_zero);
        else pixels_tile<MODE, D1>(R, tile, qw, tid, park);
        if (R.tile_cost && fresh_lane_id() == 0) {  // this wave's duration, for the next frame's heavy lists
            asm volatile("" ::: "memory");
            const uint32_t d = (uint32_t)wall_clock64() - t_start[wv];
            R.tile_cost[t_item[wv]] = (uint16_t)(d < 0xffffu ? d : 0xffffu);
        }
        RT_HOOK_ITEM_END(wt0, tile, WPT, qw, bx, first, wv);
    }
}

template <int MODE, bool SAMPLES, bool D1, int WAVES = RT_RENDER_WAVES, int LS = 0>
__global__ __launch_bounds__(BLOCK, WAVES) void render_tiles_kernel(RenderParams P) {
    render_tiles_body<MODE, SAMPLES, D1, WAVES, LS, false>();
}

template <int MODE, bool SAMPLES, bool D1, int WAVES = RT_RENDER_WAVES, int LS = 0>
__global__ __launch_bounds__(BLOCK, WAVES) void render_pair_kernel(PairParams P) {
    render_tiles_body<MODE, SAMPLES, D1, WAVES, LS, true>();
}

__global__ __launch_bounds__(BLOCK) void powf_kernel(const float* __restrict__ x, const float* __restrict__ y, int n,
                                                     float* __restrict__ out) {
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i < n) out[i] = ref_powf(x[i], y[i]);
}

// rt_box_test_batch: the device build of the box tests, item i in lane i & 63 of its wave.  Every
// lane of a wave runs every form (the mask forms ballot); lanes past n repeat item n - 1 outside
// `act` and store nothing.
__global__ __launch_bounds__(BLOCK) void box_test_kernel(const float* __restrict__ rays, const float* __restrict__ boxes,
                                                         const float* __restrict__ tminmax,
                                                         const float* __restrict__ bmax,
                                                         const uint8_t* __restrict__ active, int n,
                                                         int32_t* __restrict__ out) {
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    const bool in = i < n;
    const size_t j = (size_t)(in ? i : n - 1);  // n > 0 (the host returns before the launch otherwise)
    const float* R = rays + 6 * j;
    const float* B = boxes + 6 * j;
    f3 bm;
    if (bmax != nullptr) {
        bm = mk(bmax[3 * j], bmax[3 * j + 1], bmax[3 * j + 2]);
    } else {  // as rt_box_test_host
        bm = mk(fmaxf(fabsf(B[0]), fabsf(B[3])), fmaxf(fabsf(B[1]), fabsf(B[4])), fmaxf(fabsf(B[2]), fabsf(B[5])));
        if (!(B[0] <= B[3] && B[1] <= B[4] && B[2] <= B[5])) bm = mk(INFINITY, INFINITY, INFINITY);
    }
    const BoxP b = {(v2f){B[0], B[3]}, (v2f){B[1], B[4]}, (v2f){B[2], B[5]}};
    const float tmin = tminmax[2 * j], tmax = tminmax[2 * j + 1];
    const RayPre r = make_ray(mk(R[0], R[1], R[2]), mk(R[3], R[4], R[5]), bm, tmin);
    const RayPre rw = make_ray(r.o, r.d, bm);  // the wave forms' tmin is the traversals'
    const uint64_t act = ballot(in && (active == nullptr || active[j] != 0));
    const int cls = box_classify(r, b, tmax);
    const bool h = box_hit(r, b, tmin, tmax);
    const uint64_t m0 = box_hit_mask<false, false>(rw, b, tmax, act);
    const uint64_t m1 = box_hit_mask<true, false>(rw, b, tmax, act);
    const uint64_t m2 = box_hit_mask<true, true>(rw, b, tmax, act);
    if (in) {
        int32_t* O = out + 5 * j;
        O[0] = h ? 1 : 0;
        O[1] = cls;
        O[2] = lane_in(m0) ? 1 : 0;
        O[3] = lane_in(m1) ? 1 : 0;
        O[4] = lane_in(m2) ? 1 : 0;
    }
}

// The camera words tile_dirs_f reads, from the ABI's camera.
__host__ __device__ __forceinline__ void tile_test_camera(RenderParams& P, const rt_camera& cam) {
    P.cam_center = f3{cam.center.x, cam.center.y, cam.center.z};
    P.cam_p00 = f3{cam.pixel00_loc.x, cam.pixel00_loc.y, cam.pixel00_loc.z};
    P.cam_du = f3{cam.pixel_delta_u.x, cam.pixel_delta_u.y, cam.pixel_delta_u.z};
    P.cam_dv = f3{cam.pixel_delta_v.x, cam.pixel_delta_v.y, cam.pixel_delta_v.z};
}

// rt_debug_tile_test_batch: the device build of the tile test, one lane per item.
__global__ __launch_bounds__(BLOCK) void tile_test_kernel(RenderParams P, const int32_t* __restrict__ tiles,
                                                          const float* __restrict__ boxes, int n,
                                                          int32_t* __restrict__ out) {
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i >= n) return;
    const int32_t* t = tiles + 4 * (size_t)i;
    float bx[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) bx[k] = boxes[6 * (size_t)i + k];
    out[i] = tile_misses_box_f(tile_dirs_f(P, t[0], t[1], t[2], t[3]), bx) ? 1 : 0;
}

// rt_debug_family_test_batch: one wave per item.  Lane l holds ray l of the wave (family_dirs
// over the lanes with a nonzero `active` byte, tmax_w as frustum_loop reduces it), then lane k
// (mod 32) tests entry k with the loop form the wave takes.  Every lane runs the reductions.
__global__ __launch_bounds__(BLOCK) void family_test_kernel(const float* __restrict__ rays,
                                                            const uint8_t* __restrict__ active,
                                                            const float* __restrict__ best_t,
                                                            const float* __restrict__ bmax,
                                                            const float* __restrict__ boxes, int n_waves,
                                                            int32_t* __restrict__ out, int32_t* __restrict__ out_loose) {
    const int w = (int)(blockIdx.x * (BLOCK / 64) + threadIdx.x / 64);
    if (w >= n_waves) return;  // (a whole wave)
    const uint32_t lane = lane_id();
    const size_t j = (size_t)w * 64 + lane;
    const float* R = rays + 6 * j;
    SceneView sc;
    sc.bmax[0] = bmax[3 * (size_t)w];
    sc.bmax[1] = bmax[3 * (size_t)w + 1];
    sc.bmax[2] = bmax[3 * (size_t)w + 2];
    const RayPre r = make_ray(mk(R[0], R[1], R[2]), mk(R[3], R[4], R[5]), mk(sc.bmax[0], sc.bmax[1], sc.bmax[2]));
    const bool live = active == nullptr || active[j] != 0;
    const float o[3] = {__int_as_float(uni(__float_as_int(r.o.x))), __int_as_float(uni(__float_as_int(r.o.y))),
                        __int_as_float(uni(__float_as_int(r.o.z)))};
    v2f U[3];
    const bool loose = family_dirs(sc, r, live, o, U);
    const float tmax_w = wave_reduce_f<true>(live ? best_t[j] : 0.0f);
    const float* B = boxes + 6 * ((size_t)w * 32 + (lane & 31u));
    const v2f bb[3] = {(v2f){B[0], B[3]}, (v2f){B[1], B[4]}, (v2f){B[2], B[5]}};
    bool pass;
    if (__builtin_amdgcn_readfirstlane((int)loose) != 0) pass = family_entry_passes<true>(bb, o, U, tmax_w);
    else pass = family_entry_passes<false>(bb, o, U, tmax_w);
    if (lane < 32u) out[(size_t)w * 32 + lane] = pass ? 1 : 0;
    if (lane == 0) out_loose[w] = loose ? 1 : 0;
}

// Batched ray-triangle queries (KAT path): one lane per ray.
__global__ __launch_bounds__(BLOCK) void intersect_kernel(f3 v0, f3 e1, f3 e2, f3 o, const float* __restrict__ dirs,
                                                          int n, int hw1, float tmin, float tmax,
                                                          int32_t* __restrict__ hit, float* __restrict__ tout) {
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i >= n) return;
    f3 d = mk(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
    float t = 0.f, u = 0.f, v = 0.f;
    bool h;
    if (hw1) {
        d = unit(d);
        h = mt_hw1(o, d, v0, e1, e2, t, u, v);
    } else {
        const RayPre r = make_ray_mt(o, d);
        h = mt_g(r, v0, e1, e2, tmin, tmax, t, u, v);
    }
    hit[i] = h ? 1 : 0;
    tout[i] = h ? t : -1.0f;
}

}  // namespace

// =========================================================================================
// Host side
// =========================================================================================
using rt::set_error;
using rt::hip_msg;
using rt::DevBuf;
using rt::check_device;
using rt::DeviceGuard;
using rt::KernelTimer;
using rt::Staging;

// The caller-query families (rt_query_host.hpp): each has a variant word of its own on the scene.
enum QueryKind { kTraceRays, kShadeRays, kTraceHits, kPathStep, kMultiHits, kClosestPoints, kLightVis, kQueryKinds };
static_assert(RT_RAYS_VARIANT_NONE == 0, "rt_scene::variant starts zeroed");

// The scene's two frame streams (rt_scene::rstream) at the pre-pass stream's high priority (0,
// the default) or at normal priority (1: the A/B build of DESIGN.md §4.9).
#ifndef RT_FRAME_STREAMS_NORMAL
#define RT_FRAME_STREAMS_NORMAL 0
#endif

struct rt_scene : rt::SceneMeta {  // the packed scene's facts (rt_scene_pack.hpp), then its device state
    int device = 0;
    const char* last_kernel = nullptr;  // the render kernel instantiation of the latest frame
    // RT_RAYS_VARIANT_* of the latest call of each query family (rt_*_variant): queries run beside
    // frames, from any thread, and these words are the one thing of the scene they write
    std::atomic<int> variant[kQueryKinds] = {};
    DevBuf inode, wnode, ibox, leaf, tnorm, objids, mats, lights, jitter;
    DevBuf fnode;    // 2^f_log2-ary records of the frustum traversal (empty: it takes wnode's 4-ary ones)
    DevBuf qent, qhdr;  // fnode quantised (build_quant_records): the big-scene kernels' records
    DevBuf fault;     // one word: RT_FAULT_* bits the kernels OR in (rt_scene_faults)
    DevBuf cut;  // tile culling: boxes of a cut of the tree (6 floats each)
    DevBuf cut2;  // 2^cut_sub_log2 boxes below each cut box (cut_unit's second level), 6 floats each
    DevBuf tri;         // deep: triangles by index (brute-force completion)
    // rt_scene_create_refittable: the refit plan on the device (rt::RefitPlan; rt_refit.hpp) — the
    // bottom-up schedule, its level offsets, fnode record -> node, the cut slots' nodes (cut's then
    // cut2's) — and the finite check's flag word
    bool refittable = false;
    DevBuf rf_order, rf_levels, rf_frec, rf_cut, rf_flag;
    uint32_t rf_n_int = 0, rf_n_leaf = 0, rf_nrec = 0, rf_ncut = 0, rf_ncut2 = 0;
    std::vector<uint32_t> rf_level_off;  // host copy: the launches per level
    int rebuild_path = RT_REBUILD_NONE;  // RT_REBUILD_* of the latest rt_scene_rebuild[_device] (rt_scene_rebuild_path)
    int64_t rebuild_launches = 0, rebuild_readbacks = 0;  // ... and its pack's kernel launches and host read-backs
    int binary_stack = 0, wide_stack = 0;  // DFS stack bounds of the records (rt_debug_scene_digest)
    DevBuf work;  // kSets counter sets, then kSets x (live lists | cut survivor lists | heavy lists)
    int64_t last_tiles_total = 0;
    int cus = 256;
    // heavy-first dispatch: per-tile wave durations of the last frames (4 x u16 per tile) for
    // the tile geometry cost_key, and the latest finished frame's render-kernel time
    DevBuf cost;
    uint64_t cost_key = 0;
    float kernel_ms_est = 0.f;
    int last_heavy_cap = 0;
    int jitter_spp = -1;
    std::vector<float> jitter_host;
    // Ring of HIP events per frame.  A frame's pre-passes (tile_cull_kernel, tile_cut_kernel)
    // run on the scene's own high-priority `prep` stream, its render kernel on the caller's:
    //   prep:   [wait ev1 of frame k-2 (k-1 too if the outputs overlap)] ev0 | cull | cut | pdone
    //   caller: [wait pdone] evm | render kernel | ev1
    // so frame k's pre-passes overlap frame k-1's render kernel (its tail leaves CUs idle).
    // Frame streams (RT_TUNE_FRAME_STREAMS, rt_renderer's single frames): the whole chain of frame
    // k sits on rstream[k & 1],
    //   rstream[k & 1]: [gate wait] cull | cut | render kernel | ev1
    // so cull -> cut -> render are same-queue successions with no event between them, "frame k
    // waits for frame k-2" is stream order, and the chain still overlaps frame k-1's render
    // kernel, which runs on the other stream.  ev0, pdone and evm ride only on the timed frames.
    static constexpr int kRing = 256;
    hipEvent_t ev0[kRing] = {}, evm[kRing] = {}, ev1[kRing] = {}, pdone[kRing] = {};
    // evm is recorded (the render kernel's start timestamp) only for timed frames: a start event
    // holds the kernel's dispatch until the previous kernel has completed and its timestamp is
    // written, ~5 us between back-to-back kernels (scripts/micro/kernel_gap.hip); the
    // renderer's frames time one in RT_TUNE_KERNEL_TIMING_EVERY
    bool timed[kRing] = {};
    // ev0 and pdone of the slot were recorded: every frame of the prep-stream schedule; of the
    // frame streams' the timed frames, and every frame while the caller reads the frame's start
    // (want_start)
    bool ptimed[kRing] = {};
    // frames of the slot's render launch: 2 for the frames of a pair (rt::render_pair; frame A's
    // events bracket the pair kernel, frame B's ev1 is recorded after it), else 1
    uint8_t span[kRing] = {};
    // evq: recorded on the caller's stream at the start of a frame; the prep stream waits for it
    // so the pre-passes (which write the culled tiles' pixels into the caller's buffers) come
    // after everything the caller queued on that stream before the call.  A caller that orders
    // its buffer reuse itself on the host (rt_renderer) sets caller_ordered and skips it.
    hipEvent_t evq[kRing] = {};
    bool caller_ordered = false;
    bool want_start = true;  // the caller reads every frame's ev0 (rt::scene_set_caller_ordered)
    hipStream_t prep = nullptr;
    // Caller-ordered frames only.  RT_TUNE_FRAME_STREAMS: frame k's gate wait, pre-passes and
    // render kernel on rstream[k & 1].  RT_TUNE_OVERLAP_FRAMES without it: the render kernels
    // alone alternate over the two, the pre-passes stay on prep.  Either way frame k+1's kernel
    // takes the wave slots frame k's tail leaves.  Both are created at prep's priority, one after
    // the other (create_sync): HIP spreads the streams of one priority over the hardware queues
    // in the order of their creation, so the two get a queue each.
    hipStream_t rstream[2] = {};
    // the previous frame took the frame streams: a frame in the other schedule than the one
    // before it first waits, on the host, for everything the scene has queued
    bool last_fs = false;
    // the previous frame queued a memset ahead of its cull: the next one waits for it (ev1)
    bool serialise_next = false;
    uint64_t launches = 0;
    // The pre-pass gate's host words (RenderParams::drained): kDrainStride apart, word 0 for the
    // frames of the prep-stream schedule and the even frames of the frame streams, word 1 for
    // their odd frames.  A word takes plain stores, so it has one writer kernel at a time: the
    // kernels of one stream.  drain_frame: the frame whose render kernel last armed a gate (~0:
    // none), drain_word: the word it stores into.
    static constexpr int kDrainStride = 16;
    uint32_t* drain = nullptr;
    uint64_t drain_frame = ~0ull;
    int drain_word = 0;
    uint64_t est_next = 0;  // the oldest frame not yet seen finished (heavy-threshold estimate)
    size_t bytes = 0;
    // Work buffers rotate over kSets per frame (frame k: set k % 6; its cull pass zeroes the
    // counters of set k+2, last used by frame k-4, so the two frames of a pair never touch each
    // other's sets and their pre-passes run side by side).  Six sets: the two frames of a
    // running pair kernel, the next pair's two, whose pre-passes run in its tail, and the two
    // sets those zero.  A frame launched on another stream than the previous one first waits for
    // that frame.  A frame whose launches failed part-way leaves the counter sets unknown: the
    // next frame zeroes them all.
    static constexpr int kSets = 6;
    hipStream_t last_stream = nullptr;
    bool counters_dirty = false;
    // the previous frame's output ranges (device byte ranges): overlapping outputs serialise
    struct Range { uintptr_t lo = 0, hi = 0; };
    Range prev_out[4];
    size_t set_bytes = 0;  // bytes of one set of lists for the current geometry
    ~rt_scene() {
        if (prep) (void)hipStreamSynchronize(prep);
        for (int i = 0; i < kRing; ++i) {
            if (ev0[i]) (void)hipEventDestroy(ev0[i]);
            if (evm[i]) (void)hipEventDestroy(evm[i]);
            if (ev1[i]) (void)hipEventDestroy(ev1[i]);
            if (pdone[i]) (void)hipEventDestroy(pdone[i]);
            if (evq[i]) (void)hipEventDestroy(evq[i]);
        }
        for (hipStream_t r : rstream)
            if (r) {
                (void)hipStreamSynchronize(r);
                (void)hipStreamDestroy(r);
            }
        if (prep) (void)hipStreamDestroy(prep);
        if (drain) (void)hipHostFree(drain);
    }
    int create_sync() {  // streams and events (rt_scene_create / rt_scene_clone)
        int lo = 0, hi = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIP_TRY(hipStreamCreateWithPriority(&prep, hipStreamNonBlocking, hi));
        for (hipStream_t& r : rstream)
            HIP_TRY(hipStreamCreateWithPriority(&r, hipStreamNonBlocking, RT_FRAME_STREAMS_NORMAL ? lo : hi));
        if (int rc = fault.alloc(sizeof(uint32_t)); rc != RT_OK) return rc;
        HIP_TRY(hipMemset(fault.p, 0, sizeof(uint32_t)));
        HIP_TRY(hipDeviceSynchronize());  // (the frames run on non-blocking streams)
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&drain), 2 * kDrainStride * sizeof(uint32_t), hipHostMallocCoherent));
        std::fill(drain, drain + 2 * kDrainStride, 0u);
        for (int i = 0; i < kRing; ++i) {
            HIP_TRY(hipEventCreate(&ev0[i]));
            HIP_TRY(hipEventCreate(&evm[i]));
            HIP_TRY(hipEventCreate(&ev1[i]));
            HIP_TRY(hipEventCreate(&pdone[i]));
            HIP_TRY(hipEventCreateWithFlags(&evq[i], hipEventDisableTiming));
        }
        return RT_OK;
    }
};

extern "C" int rt_device_count(int* n) {
    if (!n) return set_error(RT_ERR_ARG, "null");
    *n = 0;
    hipError_t e = hipGetDeviceCount(n);
    if (e != hipSuccess) { *n = 0; return set_error(RT_ERR_NODEVICE, hip_msg(e, "hipGetDeviceCount")); }
    return RT_OK;
}

// Scene creation is pack (rt::pack_scene, host code of its own: rt_scene_pack.cpp) -> upload.
// The scene's device arrays, once: rt::PackedScene::arrays() in its order, then the caller's
// tables.  rt_scene_create uploads them, rt_scene_clone copies them, `bytes` sums the counted.
namespace {
struct SceneBuf {
    DevBuf rt_scene::*buf;
    bool counted;  // part of rt_scene_device_bytes
};
constexpr SceneBuf kSceneBufs[] = {
    {&rt_scene::inode, true}, {&rt_scene::wnode, true}, {&rt_scene::fnode, true}, {&rt_scene::qent, false},
    {&rt_scene::qhdr, false}, {&rt_scene::ibox, true},  {&rt_scene::leaf, true},  {&rt_scene::tnorm, true},
    {&rt_scene::cut, false},  {&rt_scene::cut2, false}, {&rt_scene::tri, false},
    {&rt_scene::objids, true}, {&rt_scene::mats, true}, {&rt_scene::lights, true}};
static_assert(sizeof(kSceneBufs) / sizeof(kSceneBufs[0]) == rt::PackedScene::kArrays + 3, "packed arrays + objids, mats, lights");

// What the kernels read of a resident scene; the launches then set what depends on the frame
// or the query (wide, ncut, f_log2).
SceneView scene_view(const rt_scene* s) {
    SceneView v;
    std::memset(&v, 0, sizeof(v));
    v.inode = static_cast<const float4*>(s->inode.p);
    v.wnode = static_cast<const float4*>(s->wnode.p);
    v.fnode = static_cast<const float*>(s->fnode.p);
    v.f_log2 = s->fnode.p ? s->f_log2 : 2;
    v.qent = static_cast<const uint4*>(s->qent.p);
    v.qhdr = static_cast<const float4*>(s->qhdr.p);
    v.ibox = static_cast<const float4*>(s->ibox.p);
    v.rootb = static_cast<const float4*>(s->ibox.p) + s->ibox.n / sizeof(float4) - 2;
    v.leaf = static_cast<const float4*>(s->leaf.p);
    v.tnorm = static_cast<const float4*>(s->tnorm.p);
    v.objids = static_cast<const int32_t*>(s->objids.p);
    v.mats = static_cast<const DevMaterial*>(s->mats.p);
    v.lights = static_cast<const DevLight*>(s->lights.p);
    v.num_tris = int32_t(s->P);
    v.num_mats = s->nmat;
    v.num_lights = s->nlights;
    v.root_ref = s->root_ref;
    std::memcpy(v.root_box, s->root_box, sizeof(v.root_box));
    std::memcpy(v.bmax, s->bmax, sizeof(v.bmax));
    v.wide = s->wide ? 1 : 0;
    v.lane_stack = s->lane_stack ? 1 : 0;
    v.lane_wide = s->lane_wide ? 1 : 0;
    v.cut = static_cast<const float*>(s->cut.p);
    v.ncut = s->ncut;
    v.cut2 = static_cast<const float*>(s->cut2.p);
    v.cut_sub_log2 = s->cut2.p ? s->cut_sub_log2 : 0;
    v.tri = static_cast<const float4*>(s->tri.p);
    v.fault = static_cast<uint32_t*>(s->fault.p);
    return v;
}

// The refit plan's device buffers (rt_scene_create_refittable, and rt_scene_clone of such a scene).
constexpr DevBuf rt_scene::*kRefitBufs[] = {&rt_scene::rf_order, &rt_scene::rf_levels, &rt_scene::rf_frec,
                                            &rt_scene::rf_cut, &rt_scene::rf_flag};

int upload_words(DevBuf& b, const std::vector<uint32_t>& w) {  // (an empty list keeps one word: no null pointers)
    const uint32_t none = 0;
    return w.empty() ? b.upload(&none, sizeof(none)) : b.upload(w.data(), w.size() * sizeof(uint32_t));
}

int upload_plan(rt_scene* s, const rt::RefitPlan& plan) {
    s->refittable = true;
    s->rf_n_int = uint32_t(plan.n_int);
    s->rf_n_leaf = uint32_t(plan.n_leaf);
    s->rf_nrec = s->fnode.p ? uint32_t(plan.frec_node.size()) : 0u;
    s->rf_ncut = s->cut.p ? uint32_t(plan.cut_ref.size()) : 0u;
    s->rf_ncut2 = s->cut2.p ? uint32_t(plan.cut2_ref.size()) : 0u;
    s->rf_level_off = plan.level_off;
    std::vector<uint32_t> cuts(plan.cut_ref.begin(), plan.cut_ref.begin() + s->rf_ncut);
    cuts.insert(cuts.end(), plan.cut2_ref.begin(), plan.cut2_ref.begin() + s->rf_ncut2);
    int rc;
    if ((rc = upload_words(s->rf_order, plan.order)) != RT_OK) return rc;
    if ((rc = upload_words(s->rf_levels, plan.level_off)) != RT_OK) return rc;
    if ((rc = upload_words(s->rf_frec, plan.frec_node)) != RT_OK) return rc;
    if ((rc = upload_words(s->rf_cut, cuts)) != RT_OK) return rc;
    return upload_words(s->rf_flag, {});
}

// The packed facts and arrays into s (rt_scene_create; rt_scene_rebuild's fresh buffers).
int upload_pack(rt_scene* s, const rt::PackedScene& pk) {
    static_cast<rt::SceneMeta&>(*s) = pk.meta;
    s->binary_stack = pk.binary_stack;
    s->wide_stack = pk.wide_stack;
    size_t i = 0;
    for (const rt::PackedArray& a : pk.arrays()) {
        DevBuf& b = (*s).*kSceneBufs[i++].buf;
        if (int rc = a.bytes ? b.upload(a.data, a.bytes) : RT_OK; rc != RT_OK) return rc;
    }
    return RT_OK;
}

int scene_create(int device, size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs, const rt_triangle* tris,
                 const int32_t* objids, const rt_material* mats, int nmat, const rt_light* lights, int nlights,
                 bool refittable, rt_scene** out) {
    if (!out) return set_error(RT_ERR_ARG, "rt_scene_create: null out");
    *out = nullptr;
    int rc = rt::check_scene_arrays(P, nodes, aabbs, tris);
    if (rc != RT_OK) return rc;
    if (nmat < 0 || nlights < 0 || (nmat > 0 && !mats) || (nlights > 0 && !lights))
        return set_error(RT_ERR_ARG, "rt_scene_create: bad material/light arrays");
    rt::PackedScene pk;
    rt::RefitPlan plan;
    if ((rc = rt::pack_scene(P, nodes, aabbs, tris, pk, refittable ? &plan : nullptr)) != RT_OK) return rc;
    if ((rc = check_device(device)) != RT_OK) return rc;
    DeviceGuard g(device);
    std::unique_ptr<rt_scene> s(new (std::nothrow) rt_scene());
    if (!s) return set_error(RT_ERR_NOMEM, "out of memory");
    s->device = device;
    if ((rc = upload_pack(s.get(), pk)) != RT_OK) return rc;
    s->nmat = nmat;
    s->nlights = nlights;
    if (objids && (rc = s->objids.upload(objids, P * sizeof(int32_t))) != RT_OK) return rc;
    if (nmat > 0 && (rc = s->mats.upload(mats, size_t(nmat) * sizeof(rt_material))) != RT_OK) return rc;
    if (nlights > 0 && (rc = s->lights.upload(lights, size_t(nlights) * sizeof(rt_light))) != RT_OK) return rc;
    if (refittable && (rc = upload_plan(s.get(), plan)) != RT_OK) return rc;
    if ((rc = s->create_sync()) != RT_OK) return rc;
    for (const SceneBuf& b : kSceneBufs)
        if (b.counted) s->bytes += ((*s).*b.buf).n;
    if (refittable)
        for (DevBuf rt_scene::*b : kRefitBufs) s->bytes += ((*s).*b).n;
    *out = s.release();
    return RT_OK;
}
}  // namespace

extern "C" int rt_scene_create(int device, size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs,
                               const rt_triangle* tris, const int32_t* objids, const rt_material* mats,
                               int nmat, const rt_light* lights, int nlights, rt_scene** out) {
    return scene_create(device, P, nodes, aabbs, tris, objids, mats, nmat, lights, nlights, false, out);
}

extern "C" int rt_scene_create_refittable(int device, size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs,
                                          const rt_triangle* tris, const int32_t* objids, const rt_material* mats,
                                          int nmat, const rt_light* lights, int nlights, rt_scene** out) {
    return scene_create(device, P, nodes, aabbs, tris, objids, mats, nmat, lights, nlights, true, out);
}

extern "C" int rt_scene_clone(const rt_scene* src, int device, rt_scene** out) {
    if (!src || !out) return set_error(RT_ERR_ARG, "rt_scene_clone: null argument");
    *out = nullptr;
    int rc = check_device(device);
    if (rc != RT_OK) return rc;
    DeviceGuard g(device);
    std::unique_ptr<rt_scene> s(new (std::nothrow) rt_scene());
    if (!s) return set_error(RT_ERR_NOMEM, "out of memory");
    static_cast<rt::SceneMeta&>(*s) = *src;
    s->device = device;
    s->cus = src->cus;
    s->bytes = src->bytes;
    // device-to-device copies of the packed arrays (over xGMI when the devices differ)
    for (const SceneBuf& b : kSceneBufs) {
        DevBuf& d = (*s).*b.buf;
        const DevBuf& q = (*src).*b.buf;
        if ((rc = d.alloc(q.n)) != RT_OK) return rc;
        if (q.n) HIP_TRY(hipMemcpyPeer(d.p, device, q.p, src->device, q.n));
    }
    s->binary_stack = src->binary_stack;
    s->wide_stack = src->wide_stack;
    if (src->refittable) {  // the plan with it: a refittable scene's clone is refittable
        s->refittable = true;
        s->rf_n_int = src->rf_n_int, s->rf_n_leaf = src->rf_n_leaf, s->rf_nrec = src->rf_nrec;
        s->rf_ncut = src->rf_ncut, s->rf_ncut2 = src->rf_ncut2;
        s->rf_level_off = src->rf_level_off;
        for (DevBuf rt_scene::*b : kRefitBufs) {
            DevBuf& d = (*s).*b;
            const DevBuf& q = (*src).*b;
            if ((rc = d.alloc(q.n)) != RT_OK) return rc;
            if (q.n) HIP_TRY(hipMemcpyPeer(d.p, device, q.p, src->device, q.n));
        }
    }
    if ((rc = s->create_sync()) != RT_OK) return rc;
    *out = s.release();
    return RT_OK;
}

// ---- refit (rt_refit.hpp) ------------------------------------------------------------------------
namespace {
unsigned refit_grid(size_t n) { return unsigned((n + BLOCK - 1) / BLOCK); }

RefitView refit_view(const rt_scene* s) {
    RefitView v;
    std::memset(&v, 0, sizeof(v));
    v.inode = static_cast<float4*>(s->inode.p);
    v.wnode = static_cast<float4*>(s->wnode.p);
    v.fnode = static_cast<float*>(s->fnode.p);
    v.ibox = static_cast<float4*>(s->ibox.p);
    v.leaf = static_cast<float4*>(s->leaf.p);
    v.tnorm = static_cast<float4*>(s->tnorm.p);
    v.tri = static_cast<float4*>(s->tri.p);
    v.cut = static_cast<float*>(s->cut.p);
    v.cut2 = static_cast<float*>(s->cut2.p);
    v.order = static_cast<const uint32_t*>(s->rf_order.p);
    v.level_off = static_cast<const uint32_t*>(s->rf_levels.p);
    v.frec = static_cast<const uint32_t*>(s->rf_frec.p);
    v.cut_ref = static_cast<const uint32_t*>(s->rf_cut.p);
    v.n_int = s->rf_n_int;
    v.n_leaf = s->rf_n_leaf;
    v.P = uint32_t(s->P);
    v.root_ref = s->root_ref;
    v.f_log2 = uint32_t(s->f_log2);
    v.nrec = s->rf_nrec;
    v.ncut_slots = s->rf_ncut + s->rf_ncut2;
    return v;
}
}  // namespace

extern "C" int rt_scene_refit_device(rt_scene* s, const rt_triangle* tris_dev, void* hip_stream, float* ms) {
    if (!s || !tris_dev) return set_error(RT_ERR_ARG, "rt_scene_refit_device: null argument");
    if (!s->refittable) return set_error(RT_ERR_UNSUPPORTED, "rt_scene_refit_device: the scene was not created refittable");
    DeviceGuard g(s->device);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    // the scene's own streams (pre-passes, overlapped render kernels) and the caller's, before any write
    HIP_TRY(hipStreamSynchronize(s->prep));
    for (hipStream_t r : s->rstream) HIP_TRY(hipStreamSynchronize(r));
    HIP_TRY(hipStreamSynchronize(st));
    if (ms) *ms = 0.f;
    KernelTimer timer(ms != nullptr);
    if (const int rc = timer.start(st); rc != RT_OK) return rc;
    const RefitView v = refit_view(s);
    const float* tris = reinterpret_cast<const float*>(tris_dev);
    uint32_t* bad = static_cast<uint32_t*>(s->rf_flag.p);
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(refit_check_kernel, dim3(refit_grid(s->P)), dim3(BLOCK), 0, st, tris, v.P, bad);
    HIP_TRY(hipGetLastError());
    uint32_t hbad = 0;
    HIP_TRY(hipMemcpyAsync(&hbad, bad, sizeof(hbad), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (hbad) return set_error(RT_ERR_ARG, "rt_scene_refit_device: a vertex coordinate is not finite");
    hipLaunchKernelGGL(refit_leaves_kernel, dim3(refit_grid(v.n_leaf)), dim3(BLOCK), 0, st, v, tris);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(refit_triangles_kernel, dim3(refit_grid(v.P)), dim3(BLOCK), 0, st, v, tris);
    HIP_TRY(hipGetLastError());
    // levels wider than one workgroup launch by launch, the rest (they shrink) in one workgroup
    const std::vector<uint32_t>& off = s->rf_level_off;
    const uint32_t levels = uint32_t(off.size()) - 1;
    uint32_t h = 1;
    for (; h <= levels && off[h] - off[h - 1] > uint32_t(REFIT_TOP); ++h) {
        hipLaunchKernelGGL(refit_level_kernel, dim3(refit_grid(off[h] - off[h - 1])), dim3(BLOCK), 0, st, v, off[h - 1],
                           off[h] - off[h - 1]);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(refit_top_levels_kernel, dim3(1), dim3(REFIT_TOP), 0, st, v, h, levels);
    HIP_TRY(hipGetLastError());
    if (v.wnode && v.n_int > 0) {
        hipLaunchKernelGGL(refit_wnode_kernel, dim3(refit_grid(v.n_int)), dim3(BLOCK), 0, st, v);
        HIP_TRY(hipGetLastError());
    }
    if (v.fnode && v.nrec > 0) {
        hipLaunchKernelGGL(refit_fnode_kernel, dim3(refit_grid(size_t(v.nrec) << v.f_log2)), dim3(BLOCK), 0, st, v);
        HIP_TRY(hipGetLastError());
    }
    if (v.ncut_slots > 0) {
        hipLaunchKernelGGL(refit_cut_kernel, dim3(refit_grid(v.ncut_slots)), dim3(BLOCK), 0, st, v, s->rf_ncut);
        HIP_TRY(hipGetLastError());
    }
    if (const int rc = timer.stop(st); rc != RT_OK) return rc;
    // the root's box (its trailing ibox copy, pairs) back for the host-side root_box and bmax: the
    // boxes are nested and finite, so the root's |coordinates| bound every box's
    float rootb[8];
    const char* rootb_dev = static_cast<const char*>(s->ibox.p) + s->ibox.n - sizeof(rootb);
    HIP_TRY(hipMemcpyAsync(rootb, rootb_dev, sizeof(rootb), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (const int rc = timer.read(ms); rc != RT_OK) return rc;
    for (int a = 0; a < 3; ++a) {
        s->root_box[a] = rootb[2 * a];
        s->root_box[3 + a] = rootb[2 * a + 1];
        s->bmax[a] = std::max(std::fabs(rootb[2 * a]), std::fabs(rootb[2 * a + 1]));
    }
    s->cost_key = 0;  // the per-tile cost history is the old geometry's
    return RT_OK;
}

extern "C" int rt_scene_refit(rt_scene* s, const rt_triangle* tris, float* ms) {
    if (!s || !tris) return set_error(RT_ERR_ARG, "rt_scene_refit: null argument");
    if (!s->refittable) return set_error(RT_ERR_UNSUPPORTED, "rt_scene_refit: the scene was not created refittable");
    DeviceGuard g(s->device);
    DevBuf d;
    if (int rc = d.upload(tris, s->P * sizeof(rt_triangle)); rc != RT_OK) return rc;
    return rt_scene_refit_device(s, static_cast<const rt_triangle*>(d.p), nullptr, ms);
}

// ---- rebuild (rt_rebuild.hpp) -----------------------------------------------------
namespace {
void swap_bufs(DevBuf& a, DevBuf& b) {
    std::swap(a.p, b.p);
    std::swap(a.n, b.n);
}

int upload_words_of(DevBuf& b, const uint32_t* dev_words, size_t n, hipStream_t st) {  // (upload_words' rule: never empty)
    if (n == 0) return upload_words(b, {});
    if (int rc = b.alloc(n * sizeof(uint32_t)); rc != RT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(b.p, dev_words, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    return RT_OK;
}

// rt::pack_scene with a plan on the device (rt_rebuild.hpp), from the tree on the device into the
// scratch scene t: every array, fact and plan buffer of rt_scene_create_refittable.  *done = false
// (nothing of t is to be used) when the tree or the knobs are not what the device path handles: the
// caller then takes the host path.  P >= 2.
int path_scan_launches(size_t n) { return n <= PATH_TILE ? 1 : 2 + path_scan_launches(path_tiles(n)); }

int rebuild_pack_device(rt_scene* t, size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs, const rt_triangle* tris,
                        hipStream_t st, bool* done) {
    *done = false;
    const size_t n = P - 1;
    if (P < 2 || P >= (size_t(1) << 25)) return RT_OK;
    if (int(rt::tuning(RT_TUNE_RECORD_GREEDY, 2.0) + 0.5) != 2 || int(rt::tuning(RT_TUNE_WIDE4_GREEDY, 1.0) + 0.5) != 1 ||
        rt::tuning(RT_TUNE_QUANT_RECORDS, 0.0) != 0.0)
        return RT_OK;
    int rc;
    const unsigned nb = refit_grid(n);
    // scratch: 7 words per internal node + the 4-ary entries, the level counts and their scan, the
    // records' node, id, count and bound per internal node (a record expands one), the cuts
    const size_t cnt_words = size_t(REBUILD_LEVEL_BINS) * nb;
    DevBuf w_node, w_cnt, w_rec, w_cut, w_facts;
    if ((rc = w_node.alloc((6 + 4) * n * 4)) != RT_OK) return rc;
    if ((rc = w_cnt.alloc((cnt_words + path_scan_words(cnt_words) + 1) * 4)) != RT_OK) return rc;
    if ((rc = w_rec.alloc((4 * n + path_scan_words(n) + 2 + 33 * n) * 4)) != RT_OK) return rc;
    if ((rc = w_cut.alloc((6 * 64 + 6 * 64 * 64) * 4 + (64 + 64 * 64 + 1) * 4)) != RT_OK) return rc;
    if ((rc = w_facts.alloc(128 * 4)) != RT_OK) return rc;
    uint32_t* wn = static_cast<uint32_t*>(w_node.p);
    RebuildView v;
    v.nodes = nodes;
    v.aabbs = reinterpret_cast<const float*>(aabbs);
    v.tris = reinterpret_cast<const float*>(tris);
    v.P = uint32_t(P);
    v.ht = wn, v.nleaf = wn + n, v.S = wn + 2 * n, v.SW = wn + 3 * n, v.wk = wn + 4 * n, v.went = wn + 6 * n;
    uint32_t* facts = static_cast<uint32_t*>(w_facts.p);
    v.flag = facts + 100;
    HIP_TRY(hipMemsetAsync(facts, 0, 128 * 4, st));
    // per-node facts bottom-up: one launch per height
    hipLaunchKernelGGL(rebuild_wide_entries_kernel, dim3(nb), dim3(BLOCK), 0, st, v);
    HIP_TRY(hipGetLastError());
    ++t->rebuild_launches;
    const uint32_t hmax = uint32_t(std::min<size_t>(n, REBUILD_MAX_HEIGHT));
    for (uint32_t h = 1; h <= hmax; ++h) {
        hipLaunchKernelGGL(rebuild_level_kernel, dim3(nb), dim3(BLOCK), 0, st, v, h);
        HIP_TRY(hipGetLastError());
        ++t->rebuild_launches;
    }
    // the plan's order and level offsets
    uint32_t* cnt = static_cast<uint32_t*>(w_cnt.p);
    if ((rc = t->rf_order.alloc(n * 4)) != RT_OK) return rc;
    hipLaunchKernelGGL(rebuild_level_count_kernel, dim3(nb), dim3(BLOCK), 0, st, v, cnt, nb);
    HIP_TRY(hipGetLastError());
    ++t->rebuild_launches;
    t->rebuild_launches += path_scan_launches(cnt_words) - 1;
    path_scan(cnt, cnt_words, cnt + cnt_words, cnt + cnt_words + path_scan_words(cnt_words), st);
    HIP_TRY(hipGetLastError());
    ++t->rebuild_launches;
    hipLaunchKernelGGL(rebuild_order_kernel, dim3(nb), dim3(BLOCK), 0, st, v, cnt, nb, static_cast<uint32_t*>(t->rf_order.p),
                       facts);
    HIP_TRY(hipGetLastError());
    ++t->rebuild_launches;
    uint32_t hf[8 + REBUILD_MAX_HEIGHT + 1];
    HIP_TRY(hipMemcpyAsync(hf, facts, sizeof(hf), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    ++t->rebuild_readbacks;
    const uint32_t top = hf[0];
    const int sb = int(std::max(1u, hf[1])), sw = int(std::max(1u, hf[2]));
    // a root without a height (a tree higher than the bound), boxes that are not nested, a deep
    // tree or a 4-ary stack past the cap: the host path
    if (top == 0 || top > uint32_t(REBUILD_MAX_HEIGHT) || hf[8] != 0 || hf[3] != 0 || sb > rt::STACK_CAP || sw > rt::STACK_CAP)
        return RT_OK;
    std::vector<uint32_t> level_off(hf + 8, hf + 8 + top + 1);
    if (level_off[top] != n) return RT_OK;
    // the records by node
    rt::SceneMeta& m = *t;
    m = rt::SceneMeta();
    m.P = P;
    m.root_ref = 0;
    m.wide = true;
    m.lane_stack = sb <= rt::LANE_LDS_CAP;
    m.lane_wide = m.lane_stack && sw <= rt::LANE_LDS_CAP;
    m.deep = false;
    t->binary_stack = sb, t->wide_stack = sw;
    if ((rc = t->inode.alloc(16 * n * 4)) != RT_OK || (rc = t->ibox.alloc((8 * n + 8) * 4)) != RT_OK ||
        (rc = t->wnode.alloc(32 * n * 4)) != RT_OK || (rc = t->leaf.alloc(16 * P * 4)) != RT_OK ||
        (rc = t->tnorm.alloc(12 * P * 4)) != RT_OK)
        return rc;
    hipLaunchKernelGGL(rebuild_leaf_kernel, dim3(refit_grid(P)), dim3(BLOCK), 0, st, v, static_cast<float4*>(t->leaf.p));
    HIP_TRY(hipGetLastError());
    ++t->rebuild_launches;
    hipLaunchKernelGGL(rebuild_inode_kernel, dim3(nb), dim3(BLOCK), 0, st, v, static_cast<float*>(t->inode.p),
                       static_cast<float*>(t->ibox.p), static_cast<float*>(t->wnode.p));
    HIP_TRY(hipGetLastError());
    ++t->rebuild_launches;
    {
        RefitView rv;
        std::memset(&rv, 0, sizeof(rv));
        rv.tnorm = static_cast<float4*>(t->tnorm.p);
        rv.P = uint32_t(P);
        hipLaunchKernelGGL(refit_triangles_kernel, dim3(refit_grid(P)), dim3(BLOCK), 0, st, rv, v.tris);
        HIP_TRY(hipGetLastError());
        ++t->rebuild_launches;
    }
    // the frustum records: the largest arity whose DFS bound fits the cap
    uint32_t* recnode = static_cast<uint32_t*>(w_rec.p);
    uint32_t *fid = recnode + n, *rcnt = recnode + 2 * n, *SF = recnode + 3 * n, *rscan = recnode + 4 * n;
    uint32_t* rtotal = rscan + path_scan_words(n);
    uint32_t *rk = rtotal + 2, *ents = rk + n;  // a record's entries (32 words) and their number
    int fr_dmax = int(std::clamp(rt::tuning(RT_TUNE_FRUSTUM_ARITY, 5.0), 2.0, 5.0));
#ifdef RT_NO_F16
    fr_dmax = 2;
#endif
    const int cap = int(std::clamp(rt::tuning(RT_TUNE_FRUSTUM_STACK_CAP, double(rt::FRUSTUM_STACK)), 1.0, 1e6));
    size_t nrec = 0;
    for (int D = fr_dmax; D >= 3 && m.f_log2 == 2; --D) {
        const int A = 1 << D;
        HIP_TRY(hipMemsetAsync(recnode, 0, 4, st));  // record 0: the root
        std::vector<uint32_t> lv{0u, 1u};            // record levels: [lv[k], lv[k + 1])
        while (lv.back() > lv[lv.size() - 2]) {
            const uint32_t lo = lv[lv.size() - 2], hi = lv.back();
            if (lv.size() > size_t(REBUILD_MAX_HEIGHT) + 2) return RT_OK;  // (a level descends a tree level at least)
            const unsigned g = unsigned((hi - lo + 63) / 64);
            hipLaunchKernelGGL(rebuild_frec_count_kernel, dim3(g), dim3(64), 0, st, v, recnode, lo, hi, A, rcnt, ents, rk);
            HIP_TRY(hipGetLastError());
            ++t->rebuild_launches;
            t->rebuild_launches += path_scan_launches(hi - lo) - 1;
            path_scan(rcnt + lo, hi - lo, rscan, rtotal, st);
            HIP_TRY(hipGetLastError());
            ++t->rebuild_launches;
            hipLaunchKernelGGL(rebuild_frec_number_kernel, dim3(refit_grid(hi - lo)), dim3(BLOCK), 0, st, v, recnode, fid, lo, hi,
                               rcnt, uint32_t(n), ents, rk);
            HIP_TRY(hipGetLastError());
            ++t->rebuild_launches;
            uint32_t total = 0;
            HIP_TRY(hipMemcpyAsync(&total, rtotal, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            ++t->rebuild_readbacks;
            if (size_t(hi) + total > n) return RT_OK;  // (cannot be: a record expands one internal node)
            lv.push_back(hi + total);
        }
        nrec = lv.back();
        for (size_t k = lv.size() - 1; k-- > 0;) {
            if (lv[k + 1] == lv[k]) continue;
            hipLaunchKernelGGL(rebuild_frec_bound_kernel, dim3(refit_grid(lv[k + 1] - lv[k])), dim3(BLOCK), 0, st, v, fid, lv[k],
                               lv[k + 1], SF, ents, rk);
            HIP_TRY(hipGetLastError());
            ++t->rebuild_launches;
        }
        uint32_t sf0 = 0;
        HIP_TRY(hipMemcpyAsync(&sf0, SF, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        ++t->rebuild_readbacks;
        if (sf0 > uint32_t(cap)) continue;
        if ((rc = t->fnode.alloc(size_t(8 * A) * nrec * 4)) != RT_OK) return rc;
        HIP_TRY(hipMemsetAsync(t->fnode.p, 0, t->fnode.n, st));
        hipLaunchKernelGGL(rebuild_frec_write_kernel, dim3(refit_grid(nrec << D)), dim3(BLOCK), 0, st, v, fid, uint32_t(nrec), D,
                           static_cast<float*>(t->fnode.p), ents, rk);
        HIP_TRY(hipGetLastError());
        ++t->rebuild_launches;
        m.f_log2 = D;
        m.f_bound = int(sf0);
    }
    // the cuts
    const int kcut = int(std::clamp(rt::tuning(RT_TUNE_CULL_BOXES, 64.0), 0.0, 64.0));
    const int sub = int(std::clamp(rt::tuning(RT_TUNE_CUT_SUB, 16.0), 0.0, 64.0));
    int sl = 0;
    while ((2 << sl) <= sub) ++sl;
    const int S = sub < 2 ? 0 : 1 << sl;
    float* cutb = static_cast<float*>(w_cut.p);
    float* cut2b = cutb + 6 * 64;
    uint32_t* crefs = reinterpret_cast<uint32_t*>(cut2b + 6 * 64 * 64);
    uint32_t* ncut_dev = crefs + 64 + 64 * 64;
    uint32_t ncut = 0;
    if (kcut > 1) {
        hipLaunchKernelGGL(rebuild_cut_kernel, dim3(1), dim3(64), 0, st, v, kcut, S, cutb, cut2b, crefs, ncut_dev);
        HIP_TRY(hipGetLastError());
        ++t->rebuild_launches;
        HIP_TRY(hipMemcpyAsync(&ncut, ncut_dev, 4, hipMemcpyDeviceToHost, st));
    }
    float rootb[8];
    HIP_TRY(hipMemcpyAsync(rootb, static_cast<const char*>(t->ibox.p) + t->ibox.n - sizeof(rootb), sizeof(rootb),
                           hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    ++t->rebuild_readbacks;
    if (ncut > 64) return set_error(RT_ERR_INTERNAL, "rebuild: cut size");
    if (ncut > 0) {
        if ((rc = t->cut.alloc(size_t(6) * ncut * 4)) != RT_OK) return rc;
        HIP_TRY(hipMemcpyAsync(t->cut.p, cutb, t->cut.n, hipMemcpyDeviceToDevice, st));
        m.ncut = int(ncut);
        if (S >= 2) {
            if ((rc = t->cut2.alloc(size_t(6) * S * ncut * 4)) != RT_OK) return rc;
            HIP_TRY(hipMemcpyAsync(t->cut2.p, cut2b, t->cut2.n, hipMemcpyDeviceToDevice, st));
            m.cut_sub_log2 = sl;
        }
    }
    for (int a = 0; a < 3; ++a) {
        m.root_box[a] = rootb[2 * a];
        m.root_box[3 + a] = rootb[2 * a + 1];
        m.bmax[a] = std::max(0.f, std::max(std::fabs(rootb[2 * a]), std::fabs(rootb[2 * a + 1])));
        if (!(m.bmax[a] <= FLT_MAX)) m.bmax[a] = INFINITY;
    }
    // the plan (upload_plan's buffers and counts)
    t->refittable = true;
    t->rf_n_int = uint32_t(n), t->rf_n_leaf = uint32_t(P);
    t->rf_nrec = t->fnode.p ? uint32_t(nrec) : 0u;
    t->rf_ncut = t->cut.p ? ncut : 0u;
    t->rf_ncut2 = t->cut2.p ? ncut * uint32_t(S) : 0u;
    t->rf_level_off = level_off;
    if ((rc = upload_words(t->rf_levels, level_off)) != RT_OK) return rc;
    if ((rc = upload_words_of(t->rf_frec, recnode, t->rf_nrec, st)) != RT_OK) return rc;
    if ((rc = t->rf_cut.alloc(std::max<size_t>(1, t->rf_ncut + t->rf_ncut2) * 4)) != RT_OK) return rc;
    HIP_TRY(hipMemsetAsync(t->rf_cut.p, 0, t->rf_cut.n, st));
    if (t->rf_ncut) HIP_TRY(hipMemcpyAsync(t->rf_cut.p, crefs, size_t(t->rf_ncut) * 4, hipMemcpyDeviceToDevice, st));
    if (t->rf_ncut2)
        HIP_TRY(hipMemcpyAsync(static_cast<uint32_t*>(t->rf_cut.p) + t->rf_ncut, crefs + 64, size_t(t->rf_ncut2) * 4,
                               hipMemcpyDeviceToDevice, st));
    if ((rc = upload_words(t->rf_flag, {})) != RT_OK) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    *done = true;
    return RT_OK;
}
}  // namespace

extern "C" int rt_scene_rebuild_device(rt_scene* s, const rt_triangle* tris_dev, void* hip_stream,
                                       rt_bvh_node* nodes_out_dev, rt_aabb* aabbs_out_dev, float* ms) {
    if (!s || !tris_dev) return set_error(RT_ERR_ARG, "rt_scene_rebuild_device: null argument");
    if (!s->refittable) return set_error(RT_ERR_UNSUPPORTED, "rt_scene_rebuild_device: the scene was not created refittable");
    DeviceGuard g(s->device);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipStreamSynchronize(s->prep));
    for (hipStream_t r : s->rstream) HIP_TRY(hipStreamSynchronize(r));
    HIP_TRY(hipStreamSynchronize(st));
    if (ms) *ms = 0.f;
    KernelTimer timer(ms != nullptr);
    if (const int rc = timer.start(st); rc != RT_OK) return rc;
    const size_t P = s->P, NN = 2 * P - 1;
    // 1: every vertex coordinate finite (the refit's pass and flag word), before anything is built
    uint32_t* bad = static_cast<uint32_t*>(s->rf_flag.p);
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(refit_check_kernel, dim3(refit_grid(P)), dim3(BLOCK), 0, st, reinterpret_cast<const float*>(tris_dev),
                       uint32_t(P), bad);
    HIP_TRY(hipGetLastError());
    uint32_t hbad = 0;
    HIP_TRY(hipMemcpyAsync(&hbad, bad, sizeof(hbad), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (hbad) return set_error(RT_ERR_ARG, "rt_scene_rebuild_device: a vertex coordinate is not finite");
    // 2: the tree, on the device, into buffers of its own
    DevBuf tn, ta;
    int rc;
    if ((rc = tn.alloc(NN * sizeof(rt_bvh_node))) != RT_OK || (rc = ta.alloc(NN * sizeof(rt_aabb))) != RT_OK) return rc;
    if ((rc = rt::build_bvh_triangles_device(tris_dev, P, static_cast<rt_bvh_node*>(tn.p), static_cast<rt_aabb*>(ta.p), st)) != RT_OK)
        return rc;
    // 3: the records, into fresh buffers of a scratch scene; nothing of s has been written so far,
    // and an error from here to the swap leaves it so.  On the device where the tree and the knobs
    // allow (rebuild_pack_device), else the host path: the tree and the triangles come back,
    // rt::pack_scene packs them with a plan, and the arrays go up.
    std::unique_ptr<rt_scene> t(new (std::nothrow) rt_scene());
    if (!t) return set_error(RT_ERR_NOMEM, "out of memory");
    bool on_device = false;
    if ((rc = rebuild_pack_device(t.get(), P, static_cast<const rt_bvh_node*>(tn.p), static_cast<const rt_aabb*>(ta.p), tris_dev,
                                  st, &on_device)) != RT_OK)
        return rc;
    if (!on_device) {
        t.reset(new (std::nothrow) rt_scene());
        if (!t) return set_error(RT_ERR_NOMEM, "out of memory");
        std::vector<rt_bvh_node> nodes(NN);
        std::vector<rt_aabb> aabbs(NN);
        std::vector<rt_triangle> tris(P);
        HIP_TRY(hipMemcpyAsync(nodes.data(), tn.p, tn.n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(aabbs.data(), ta.p, ta.n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(tris.data(), tris_dev, P * sizeof(rt_triangle), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        rt::PackedScene pk;
        rt::RefitPlan plan;
        if ((rc = rt::rebuild_pack(P, nodes.data(), aabbs.data(), tris.data(), pk, plan)) != RT_OK) return rc;
        if ((rc = upload_pack(t.get(), pk)) != RT_OK || (rc = upload_plan(t.get(), plan)) != RT_OK) return rc;
    }
    if ((rc = timer.stop(st)) != RT_OK) return rc;
    if (nodes_out_dev) HIP_TRY(hipMemcpyAsync(nodes_out_dev, tn.p, tn.n, hipMemcpyDeviceToDevice, st));
    if (aabbs_out_dev) HIP_TRY(hipMemcpyAsync(aabbs_out_dev, ta.p, ta.n, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = timer.read(ms)) != RT_OK) return rc;
    // 4: the swap (no call that can fail from here on): the packed arrays and the plan; the
    // caller's tables (object ids, materials, lights) stay
    t->nmat = s->nmat;
    t->nlights = s->nlights;
    static_cast<rt::SceneMeta&>(*s) = *t;
    for (size_t i = 0; i < rt::PackedScene::kArrays; ++i) swap_bufs((*s).*kSceneBufs[i].buf, (*t).*kSceneBufs[i].buf);
    for (DevBuf rt_scene::*b : kRefitBufs) swap_bufs((*s).*b, (*t).*b);
    s->binary_stack = t->binary_stack, s->wide_stack = t->wide_stack;
    s->rf_n_int = t->rf_n_int, s->rf_n_leaf = t->rf_n_leaf, s->rf_nrec = t->rf_nrec;
    s->rf_ncut = t->rf_ncut, s->rf_ncut2 = t->rf_ncut2;
    s->rf_level_off = std::move(t->rf_level_off);
    s->bytes = 0;
    for (const SceneBuf& b : kSceneBufs)
        if (b.counted) s->bytes += ((*s).*b.buf).n;
    for (DevBuf rt_scene::*b : kRefitBufs) s->bytes += ((*s).*b).n;
    s->cost_key = 0;  // the per-tile cost history is the old geometry's
    s->rebuild_path = on_device ? RT_REBUILD_DEVICE : RT_REBUILD_HOST;
    s->rebuild_launches = on_device ? t->rebuild_launches : 0;
    s->rebuild_readbacks = on_device ? t->rebuild_readbacks : 3;  // (host path: the tree, the boxes, the triangles)
    return RT_OK;
}

extern "C" int rt_scene_rebuild(rt_scene* s, const rt_triangle* tris, rt_bvh_node* nodes_out, rt_aabb* aabbs_out, float* ms) {
    if (!s || !tris) return set_error(RT_ERR_ARG, "rt_scene_rebuild: null argument");
    if (!s->refittable) return set_error(RT_ERR_UNSUPPORTED, "rt_scene_rebuild: the scene was not created refittable");
    DeviceGuard g(s->device);
    const size_t NN = 2 * s->P - 1;
    DevBuf d, tn, ta;
    int rc;
    if ((rc = d.upload(tris, s->P * sizeof(rt_triangle))) != RT_OK) return rc;
    if (nodes_out && (rc = tn.alloc(NN * sizeof(rt_bvh_node))) != RT_OK) return rc;
    if (aabbs_out && (rc = ta.alloc(NN * sizeof(rt_aabb))) != RT_OK) return rc;
    rc = rt_scene_rebuild_device(s, static_cast<const rt_triangle*>(d.p), nullptr, static_cast<rt_bvh_node*>(tn.p),
                                 static_cast<rt_aabb*>(ta.p), ms);
    if (rc != RT_OK) return rc;
    if (nodes_out) HIP_TRY(hipMemcpy(nodes_out, tn.p, tn.n, hipMemcpyDeviceToHost));
    if (aabbs_out) HIP_TRY(hipMemcpy(aabbs_out, ta.p, ta.n, hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" int rt_scene_rebuild_path(const rt_scene* s) { return s ? s->rebuild_path : RT_REBUILD_NONE; }

extern "C" int rt_scene_rebuild_counts(const rt_scene* s, int64_t counts[2]) {
    if (!s || !counts) return set_error(RT_ERR_ARG, "rt_scene_rebuild_counts: null argument");
    counts[0] = s->rebuild_launches;
    counts[1] = s->rebuild_readbacks;
    return RT_OK;
}

extern "C" int rt_debug_box_weight_batch(int device, const float* boxes, const uint32_t* leaves, int rule, int n, double* out) {
    if (n < 0 || (n > 0 && (!boxes || !leaves || !out)) || (rule != 1 && rule != 2))
        return set_error(RT_ERR_ARG, "rt_debug_box_weight_batch: bad args (rules 1 and 2)");
    int rc = check_device(device);
    if (rc != RT_OK) return rc;
    if (n == 0) return RT_OK;
    DeviceGuard g(device);
    DevBuf db, dl, dout;
    if ((rc = db.upload(boxes, size_t(n) * 6 * sizeof(float))) != RT_OK) return rc;
    if ((rc = dl.upload(leaves, size_t(n) * sizeof(uint32_t))) != RT_OK) return rc;
    if ((rc = dout.alloc(size_t(n) * sizeof(double))) != RT_OK) return rc;
    hipLaunchKernelGGL(box_weight_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, nullptr,
                       static_cast<const float*>(db.p), static_cast<const uint32_t*>(dl.p), rule, n, static_cast<double*>(dout.p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout.p, size_t(n) * sizeof(double), hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" int rt_triangles_from_mesh_device(int device, const rt_vec3* positions_dev, size_t num_vertices,
                                             const rt_vec3* normals_dev, const uint32_t* indices_dev, size_t P,
                                             rt_triangle* tris_dev, void* hip_stream) {
    if (!positions_dev || !indices_dev || !tris_dev)
        return set_error(RT_ERR_ARG, "rt_triangles_from_mesh_device: null argument");
    if (P == 0) return set_error(RT_ERR_ARG, "no triangles");
    if (P > 0x7FFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, "more than 2^31-1 triangles");
    if (num_vertices > 0xFFFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, "more than 2^32-1 vertices");
    int rc = check_device(device);
    if (rc != RT_OK) return rc;
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    uint32_t* err = nullptr;
    HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&err), sizeof(uint32_t), st));
    struct Free {
        void* p; hipStream_t s;
        ~Free() { (void)hipFreeAsync(p, s); }
    } free_err{err, st};
    HIP_TRY(hipMemsetAsync(err, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(mesh_triangles_kernel, dim3(refit_grid(P)), dim3(BLOCK), 0, st,
                       reinterpret_cast<const float*>(positions_dev), reinterpret_cast<const float*>(normals_dev),
                       uint32_t(num_vertices), indices_dev, uint32_t(P), reinterpret_cast<float*>(tris_dev), err);
    HIP_TRY(hipGetLastError());
    uint32_t herr = 0;
    HIP_TRY(hipMemcpyAsync(&herr, err, sizeof(herr), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (herr) return set_error(RT_ERR_ARG, "triangle index out of range");
    return RT_OK;
}

// rt_debug_scene_pack's view of a resident scene: the packed arrays read back and hashed.
extern "C" int rt_debug_scene_digest(rt_scene* s, int64_t info[21], uint64_t digests[22]) {
    if (!s || !info || !digests) return set_error(RT_ERR_ARG, "rt_debug_scene_digest: null argument");
    DeviceGuard g(s->device);
    HIP_TRY(hipDeviceSynchronize());
    rt::scene_info_words(*s, s->binary_stack, s->wide_stack, info);
    std::vector<uint8_t> host;
    for (size_t i = 0; i < rt::PackedScene::kArrays; ++i) {
        const DevBuf& b = (*s).*kSceneBufs[i].buf;
        host.resize(b.n);
        if (b.n) HIP_TRY(hipMemcpy(host.data(), b.p, b.n, hipMemcpyDeviceToHost));
        digests[2 * i] = b.n;
        digests[2 * i + 1] = rt::fnv1a(host.data(), b.n);
    }
    return RT_OK;
}

extern "C" void rt_scene_destroy(rt_scene* s) {
    if (!s) return;
    DeviceGuard g(s->device);
    delete s;
}
extern "C" int rt_scene_device(const rt_scene* s) { return s ? s->device : -1; }

// The root box the scene holds now (a refit or rebuild replaces it): the box rt_ray_sort_* take.
extern "C" int rt_scene_bounds(const rt_scene* s, rt_aabb* out) {
    if (!s || !out) return set_error(RT_ERR_ARG, "rt_scene_bounds: null argument");
    std::memcpy(out, s->root_box, sizeof(rt_aabb));
    return RT_OK;
}

extern "C" int rt_scene_traversal_info(const rt_scene* s, int64_t info[4]) {
    if (!s || !info) return set_error(RT_ERR_ARG, "rt_scene_traversal_info: null argument");
    const bool frustum = s->wide && !s->deep;
    info[0] = frustum ? s->f_log2 : 0;
    info[1] = frustum && s->f_log2 > 2 ? s->f_bound : 0;
    info[2] = s->wide ? 1 : 0;
    info[3] = s->deep ? 1 : 0;
    return RT_OK;
}

extern "C" int rt_scene_faults(rt_scene* s, uint32_t* flags, int clear) {
    if (!s || !flags) return set_error(RT_ERR_ARG, "rt_scene_faults: null argument");
    DeviceGuard g(s->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(flags, s->fault.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (clear) {
        HIP_TRY(hipMemset(s->fault.p, 0, sizeof(uint32_t)));
        HIP_TRY(hipDeviceSynchronize());  // before any later frame on a non-blocking stream
    }
    return RT_OK;
}
extern "C" size_t rt_scene_device_bytes(const rt_scene* s) { return s ? s->bytes : 0; }

extern "C" void rt_render_opts_default(rt_render_opts* o) {
    o->max_depth = 1;
    o->spp = 1;
    o->diffuse_bounce = 1;
    o->miss_color = rt_vec3{0.f, 0.f, 0.f};
    o->jitter = nullptr;
    o->band_rows = 8;
    o->band_index = 0;
    o->band_count = 1;
    o->kernel = RT_KERNEL_AUTO;
    o->tile_order = RT_TILES_AUTO;
    o->flags = 0;
}

extern "C" int rt_shard_rows(int H, int band_rows, int band_index, int band_count) {
    if (H <= 0) return 0;
    if (band_count <= 1) return H;
    if (band_rows <= 0 || band_index < 0 || band_index >= band_count) return -1;
    const int nbands = (H + band_rows - 1) / band_rows;
    int rows = 0;
    for (int b = band_index; b < nbands; b += band_count) rows += std::min(band_rows, H - b * band_rows);
    return rows;
}

namespace {

int prepare_jitter(rt_scene* s, const rt_render_opts* o) {
    std::vector<float> tab(2 * size_t(o->spp));
    if (o->jitter) std::memcpy(tab.data(), o->jitter, tab.size() * sizeof(float));
    else {
        int rc = rt_jittered_samples(o->spp, 42u, 1, tab.data());
        if (rc != RT_OK) return rc;
    }
    if (s->jitter_spp == o->spp && s->jitter_host == tab) return RT_OK;
    int rc = s->jitter.upload(tab.data(), tab.size() * sizeof(float));
    if (rc != RT_OK) return rc;
    s->jitter_host = tab;
    s->jitter_spp = o->spp;
    return RT_OK;
}

// Every entry finite and within the tile tests' one-pixel pad (NaN fails the compare).
bool jitter_within_pad(const std::vector<float>& tab) {
    for (const float j : tab)
        if (!(fabsf(j) <= 1.0f)) return false;
    return true;
}
bool jitter_finite(const std::vector<float>& tab) {
    for (const float j : tab)
        if (!std::isfinite(j)) return false;
    return true;
}
// The largest |entry| of a finite table: how far a sample may sit from its pixel (camera_class).
double jitter_pad(const std::vector<float>& tab) {
    double m = 0.0;
    for (const float j : tab) m = std::max(m, double(fabsf(j)));
    return m;
}

// The render kernel's persistent grid: the blocks of it one dispatch keeps resident on every CU
// (the occupancy the kernel was compiled for, LDS permitting), a multiple of 8 (one share per
// XCD queue), at most one block per tile.  Blocks beyond residency would only find the queues
// empty.  The render kernel's start / end events (rt_kernel_times) go into its dispatch
// (hipExtLaunchKernel): no separate event packets on the stream between the frames' kernels.
struct Launch {
    hipStream_t st;
    hipEvent_t start, stop;
    int cus;
    bool big;  // scene data beyond kBigSceneBytes: the depth-1 wave kernels at RT_RENDER_WAVES_BIG
    bool qr;   // ... over the quantised frustum records (MODE_QR), which the scene has
    const char** name;  // out: the launched instantiation, as rocprofv3 names it (rt_scene_kernel_name)
};
template <int MODE, bool SAMPLES, bool D1, int WAVES = RT_RENDER_WAVES, int LS = 0>
void launch_render(const RenderParams& P, const Launch& L) {
    constexpr auto KERNEL = render_tiles_kernel<MODE, SAMPLES, D1, WAVES, LS>;
    static const int per_cu = [] {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, KERNEL, BLOCK, 0) != hipSuccess || n < 1) n = 1;
        return n;
    }();
    static const std::string name = "render_tiles_kernel<" + std::to_string(MODE) + (SAMPLES ? ", true" : ", false") +
                                    (D1 ? ", true, " : ", false, ") + std::to_string(WAVES) + ", " +
                                    std::to_string(LS) + ">";
    if (L.name) *L.name = name.c_str();
    const int tiles8 = (P.tiles_total + 7) / 8 * 8;
    const dim3 grid((unsigned)std::max(8, std::min(tiles8, L.cus * per_cu / 8 * 8)));
    hipExtLaunchKernelGGL(KERNEL, grid, dim3(BLOCK), 0, L.st, L.start, L.stop, 0, P);
}

// Two frames, one persistent grid (render_pair_kernel): the grid launch_render gives one frame,
// at most one block per tile of the two.
template <int MODE, bool SAMPLES, bool D1, int WAVES = RT_RENDER_WAVES, int LS = 0>
void launch_render_pair(const RenderParams& A, const RenderParams& B, const Launch& L, double reserve_default) {
    constexpr auto KERNEL = render_pair_kernel<MODE, SAMPLES, D1, WAVES, LS>;
    static const int per_cu = [] {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, KERNEL, BLOCK, 0) != hipSuccess || n < 1) n = 1;
        return n;
    }();
    static const std::string name = "render_pair_kernel<" + std::to_string(MODE) + (SAMPLES ? ", true" : ", false") +
                                    (D1 ? ", true, " : ", false, ") + std::to_string(WAVES) + ", " +
                                    std::to_string(LS) + ">";
    if (L.name) *L.name = name.c_str();
    const int tiles8 = (A.tiles_total + B.tiles_total + 7) / 8 * 8;
    // RT_TUNE_PAIR_RESERVE: block slots per CU left to the next pair's pre-passes, which then run
    // beside this kernel instead of after it (c3: 0.148 ms per delivered frame vs 0.151 with
    // none and 0.157 with two, profiles/r05/exp/pair_knobs_c3.log; fractions: that many slots
    // per CU on average).  The bounce kernels' pairs reserve none by default: a 1.2 ms kernel
    // hides its pre-passes anyway, and a slot is a quarter of their 4 waves per SIMD (c3b 1.53
    // ms per frame with one, 1.13 with none, profiles/r05/exp/pair_c3b.log).
    const double reserve = std::clamp(rt::tuning(RT_TUNE_PAIR_RESERVE, reserve_default), 0.0, double(per_cu - 1));
    const int blocks = L.cus * per_cu - int(std::lround(reserve * L.cus));
    const dim3 grid((unsigned)std::max(8, std::min(tiles8, blocks / 8 * 8)));
    PairParams PP;
    PP.f[0] = A;
    PP.f[1] = B;
    hipExtLaunchKernelGGL(KERNEL, grid, dim3(BLOCK), 0, L.st, L.start, L.stop, 0, PP);
}

// The frames a pair kernel is instantiated for: depth-1 sample kernels of the 4-ary-record wave
// traversal on a scene within kBigSceneBytes, full or half waves (c3 and its band shards).
// Anything else renders a pair as two launches.
// Multi-bounce frames take it too where launch_mode picks the paired-only bounce kernels (one
// light, half waves, LS = 3: c3b): their longest items bound a launch, and a pair overlaps two
// frames' longest items.
bool pair_kernel_fits(const RenderParams& P, bool samples, bool wave_wide, bool big) {
    const bool d1 = P.max_depth == 1;
    const bool bounce = P.max_depth > 1 && P.half_waves && P.paired_only;
    return samples && wave_wide && !big && (d1 || bounce) && P.nqueues == 8 && P.spp <= 64 && !P.ray_count &&
           P.lane_samples == 1;
}
void launch_pair(const RenderParams& A, const RenderParams& B, const Launch& L) {
    constexpr int M = RT_KERNEL_WAVE | MODE_WIDE | MODE_PK;  // launch_mode's D1_MODE for these
    if (A.max_depth > 1) launch_render_pair<RT_KERNEL_WAVE | MODE_WIDE, true, false, RT_PAIRED_WAVES, 3>(A, B, L, 0.0);
    else if (A.half_waves) launch_render_pair<M, true, true, RT_RENDER_WAVES, 1>(A, B, L, 1.0);
    else launch_render_pair<M, true, true>(A, B, L, 1.0);
}

template <int MODE, bool SAMPLES>
void launch_mode(const RenderParams& P, const Launch& L) {
    // depth-1 kernels of the wave traversal: packed box tests (box_ends_pk)
    constexpr int D1_MODE = (MODE & (MODE_DEEP | RT_KERNEL_LANE)) == 0 ? (MODE | MODE_PK) : MODE;
    if (P.max_depth == 1) {
        if constexpr (SAMPLES) {
            if (P.half_waves) {
                launch_render<D1_MODE, SAMPLES, true, RT_RENDER_WAVES, 1>(P, L);
                return;
            }
        }
        if constexpr ((MODE & (MODE_DEEP | RT_KERNEL_LANE)) == 0) {
            if (L.big) {
                if constexpr ((MODE & MODE_WIDE) != 0) {
                    if (L.qr) {
                        if (P.sc.num_lights == 1)
                            launch_render<D1_MODE | MODE_1L | MODE_QR, SAMPLES, true, RT_RENDER_WAVES_BIG>(P, L);
                        else launch_render<D1_MODE | MODE_QR, SAMPLES, true, RT_RENDER_WAVES_BIG>(P, L);
                        return;
                    }
                }
                if (P.sc.num_lights == 1) launch_render<D1_MODE | MODE_1L, SAMPLES, true, RT_RENDER_WAVES_BIG>(P, L);
                else launch_render<D1_MODE, SAMPLES, true, RT_RENDER_WAVES_BIG>(P, L);
                return;
            }
        }
        launch_render<D1_MODE, SAMPLES, true>(P, L);
    } else {
        if constexpr (SAMPLES && (MODE & (MODE_DEEP | RT_KERNEL_LANE)) == 0) {
            if (P.half_waves && P.paired_only) {
                launch_render<MODE, SAMPLES, false, RT_PAIRED_WAVES, 3>(P, L);
                return;
            }
        }
        if constexpr (SAMPLES) {
            if (P.half_waves) {
                // the unpaired loop alone (one-light scenes whose lanes can pair take LS = 3 above;
                // carrying paired_bounces here as well cost 84 B of scratch per lane: cornell 7.94
                // vs 7.06 ms, profiles/r04/exp/ls2_ab_cornell.log)
                launch_render<MODE, SAMPLES, false, RT_BOUNCE_WAVES, 1>(P, L);
                return;
            }
        }
        launch_render<MODE, SAMPLES, false, RT_BOUNCE_WAVES>(P, L);
    }
}

template <int MODE>
void launch(const RenderParams& P, bool samples, const Launch& L) {
    if (samples) launch_mode<MODE, true>(P, L);
    else launch_mode<MODE, false>(P, L);
}

// Host restatement of a pixel whose spp samples all miss the root: each sample is
// clamp(0 + (1,1,1) * missColor) (query.h:181-183), or 0 when max_depth <= 0 (query.h:172);
// col accumulates them in order and is divided by float(spp) (query.cu:146-163).
f3 miss_pixel_value(const rt_render_opts* o) {
    f3 c = mk(0.f, 0.f, 0.f);
    if (o->max_depth > 0)
        c = clamp01(add(mk(0.f, 0.f, 0.f), mul(mk(1.f, 1.f, 1.f), f3{o->miss_color.x, o->miss_color.y, o->miss_color.z})));
    f3 acc = mk(0.f, 0.f, 0.f);
    for (int k = 0; k < o->spp; ++k) acc = add(acc, c);
    const float fs = (float)o->spp;
    return f3{acc.x / fs, acc.y / fs, acc.z / fs};
}

}  // namespace

namespace {
// Fraction of the image covered by the bounding rectangle of the root box's projected corners
// (1 when a corner is not in front of the camera).  The tree-cut culling pass (tile_cut_kernel)
// is launched only when this is small: a scene that fills the view gains no culled tiles from
// it and pays for the pass (a speed choice; culling or not gives the same image).
double root_box_coverage(const float* rb, const rt_camera* cam) {
    const double c[3] = {cam->center.x, cam->center.y, cam->center.z};
    const double b0[3] = {cam->pixel00_loc.x - c[0], cam->pixel00_loc.y - c[1], cam->pixel00_loc.z - c[2]};
    const double du[3] = {cam->pixel_delta_u.x, cam->pixel_delta_u.y, cam->pixel_delta_u.z};
    const double dv[3] = {cam->pixel_delta_v.x, cam->pixel_delta_v.y, cam->pixel_delta_v.z};
    // solve s*b0 + a*du + b*dv = corner - c (Cramer); pixel = (a/s, b/s)
    auto det3 = [](const double* x, const double* y, const double* z) {
        return x[0] * (y[1] * z[2] - y[2] * z[1]) - y[0] * (x[1] * z[2] - x[2] * z[1]) + z[0] * (x[1] * y[2] - x[2] * y[1]);
    };
    const double D = det3(b0, du, dv);
    if (!(std::fabs(D) > 0.0) || !(rb[0] <= rb[3] && rb[1] <= rb[4] && rb[2] <= rb[5])) return 1.0;
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (int k = 0; k < 8; ++k) {
        const double p[3] = {double(rb[(k & 1) ? 3 : 0]) - c[0], double(rb[(k & 2) ? 4 : 1]) - c[1],
                             double(rb[(k & 4) ? 5 : 2]) - c[2]};
        const double sx = det3(p, du, dv) / D, a = det3(b0, p, dv) / D, b = det3(b0, du, p) / D;
        if (!(sx > 0.0)) return 1.0;
        x0 = std::min(x0, a / sx);
        x1 = std::max(x1, a / sx);
        y0 = std::min(y0, b / sx);
        y1 = std::max(y1, b / sx);
    }
    const double W = cam->pixel_width, H = cam->pixel_height;
    const double w = std::max(0.0, std::min(W, x1) - std::max(0.0, x0)), h = std::max(0.0, std::min(H, y1) - std::max(0.0, y0));
    return w * h / (W * H);
}

// What the frame path may assume of a camera.  Camera::get_ray's direction is
// cam_unit(D) with D(px, py) = (pixel00 + du*px) + dv*py - center in float: D / |D| only while
// 1e-12 <= |D| (below: the fallback (0,0,1), whatever D is) and |D|^2 stays finite (above ~1.8e19:
// a zero direction, or NaN once D itself is inf - inf).  The tile tests reason about D, the wave
// kernels' group-wide tests drop NaN lanes, so render_frame asks here first:
//   RT_CAMERA_PROVEN  every |D| over the padded frame lies in [2e-12, 9e18]: cull, cut, any kernel;
//   RT_CAMERA_NO_CULL finite rays, but some may take the fallback: any kernel, no cull and no cut;
//   RT_CAMERA_LANE    a non-finite word, or a |D| (or a term of it) that may overflow: the lane
//                     kernel without the cull, the reference's DFS ray by ray.
// The proof, in double: px in [-pad, W-1+pad], py in [-pad, H-1+pad] (pad: the jitter table's
// largest |entry|, at least the tile tests' one pixel).  Exact D is affine in (px, py), so |D|
// is largest at a corner; its smallest value is at least the smaller of the distance from the
// origin to the plane of the parallelogram and to its four edges, and at least the gap any axis
// keeps from zero over the four corners.  The float D is within E_a = 6 * 2^-24 * S_a of the exact
// one on axis a, S_a = |center_a| + |pixel00_a| + pxm |du_a| + pym |dv_a|: the six roundings
// (px, du*px, the sum, dv*py, the sum, the difference) add up to (3|p00| + 5|du px| + 4|dv py| +
// |c|) 2^-24.  Margin: a factor 2 on both ends (2e-12, 9e18), far above the 3 roundings of
// sqrtf(x*x + y*y + z*z) and of this function's own doubles (1e-16), and free: no camera that
// renders anything lives within a factor 2 of either end.
constexpr int RT_CAMERA_PROVEN = 0, RT_CAMERA_NO_CULL = 1, RT_CAMERA_LANE = 2;
int camera_class(const rt_camera* cam, double pad) {
    const double c[3] = {cam->center.x, cam->center.y, cam->center.z};
    const double p0[3] = {cam->pixel00_loc.x, cam->pixel00_loc.y, cam->pixel00_loc.z};
    const double du[3] = {cam->pixel_delta_u.x, cam->pixel_delta_u.y, cam->pixel_delta_u.z};
    const double dv[3] = {cam->pixel_delta_v.x, cam->pixel_delta_v.y, cam->pixel_delta_v.z};
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(c[a]) || !std::isfinite(p0[a]) || !std::isfinite(du[a]) || !std::isfinite(dv[a]))
            return RT_CAMERA_LANE;
    if (!(pad >= 1.0)) pad = 1.0;
    if (!(pad < 1e30)) return RT_CAMERA_LANE;
    const double xl = -pad, xh = double(cam->pixel_width) - 1.0 + pad, yl = -pad, yh = double(cam->pixel_height) - 1.0 + pad;
    const double pxm = std::max(std::fabs(xl), std::fabs(xh)), pym = std::max(std::fabs(yl), std::fabs(yh));
    constexpr double kU = 6.0 * 5.9604644775390625e-8;
    double E[3], E2 = 0.0, smax = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double S = std::fabs(c[a]) + std::fabs(p0[a]) + pxm * std::fabs(du[a]) + pym * std::fabs(dv[a]);
        smax = std::max(smax, S);
        E[a] = kU * S;
        E2 += E[a] * E[a];
    }
    E2 = std::sqrt(E2);
    if (!(smax < 1e38)) return RT_CAMERA_LANE;  // a term of the float sum may overflow
    // the corners: the largest |D|, and per axis the range of D
    double K[4][3], far = 0.0, lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < 4; ++k) {
        const double px = (k & 1) ? xh : xl, py = (k & 2) ? yh : yl;
        double n2 = 0.0;
        for (int a = 0; a < 3; ++a) {
            K[k][a] = (p0[a] - c[a]) + px * du[a] + py * dv[a];
            n2 += K[k][a] * K[k][a];
            lo[a] = std::min(lo[a], K[k][a]);
            hi[a] = std::max(hi[a], K[k][a]);
        }
        far = std::max(far, std::sqrt(n2));
    }
    if (!(far + E2 <= 9e18)) return RT_CAMERA_LANE;
    // the smallest |D|: an axis that keeps its sign ...
    double near_ = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double gap = lo[a] > 0.0 ? lo[a] : hi[a] < 0.0 ? -hi[a] : 0.0;
        near_ = std::max(near_, gap - E[a]);
    }
    // ... or the distance to the parallelogram: its plane (0 when the basis is collapsed) and its edges
    auto dot3 = [](const double* x, const double* y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; };
    const double eu[3] = {K[1][0] - K[0][0], K[1][1] - K[0][1], K[1][2] - K[0][2]};
    const double ev[3] = {K[2][0] - K[0][0], K[2][1] - K[0][1], K[2][2] - K[0][2]};
    const double nrm[3] = {eu[1] * ev[2] - eu[2] * ev[1], eu[2] * ev[0] - eu[0] * ev[2], eu[0] * ev[1] - eu[1] * ev[0]};
    const double nn = std::sqrt(dot3(nrm, nrm));
    // (a normal lost in the rounding of the cross product proves nothing)
    double dist = nn > 1e-9 * std::sqrt(dot3(eu, eu) * dot3(ev, ev)) ? std::fabs(dot3(K[0], nrm)) / nn : 0.0;
    static const int kEdge[4][2] = {{0, 1}, {2, 3}, {0, 2}, {1, 3}};
    for (const auto& e : kEdge) {
        const double* A = K[e[0]];
        const double* B = K[e[1]];
        const double ab[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
        const double l2 = dot3(ab, ab);
        const double t = l2 > 0.0 ? std::clamp(-dot3(A, ab) / l2, 0.0, 1.0) : 0.0;
        const double q[3] = {A[0] + t * ab[0], A[1] + t * ab[1], A[2] + t * ab[2]};
        dist = std::min(dist, std::sqrt(dot3(q, q)));
    }
    near_ = std::max(near_, dist - E2);
    return near_ >= 2e-12 ? RT_CAMERA_PROVEN : RT_CAMERA_NO_CULL;
}
}  // namespace

// Set by rt_count_rays around its one render (the calling thread's frame only).
thread_local unsigned long long* t_ray_count = nullptr;

extern "C" int rt_render_device(rt_scene* s, const rt_camera* cam, const rt_render_opts* o, float* rgb,
                                int32_t* hit_idx, float* hit_t, void* stream) {
    return rt_render_device_p6(s, cam, o, rgb, hit_idx, hit_t, nullptr, stream);
}

namespace {
// Two frames in one render launch (rt::render_pair).  Frame A's call runs its pre-passes and,
// when the pair kernel fits it (pair_kernel_fits, RT_TUNE_PAIR_FRAMES on), keeps its parameters
// here instead of launching; frame B's call runs its pre-passes and launches both.  A frame B
// that cannot join (another tile geometry or cut, a failed call) launches A on its own first.
struct PairStage {
    int phase = 0;          // 0: frame A's call, 1: frame B's
    bool deferred = false;  // frame A's render launch is held here
    RenderParams A;
    Launch LA{};
    uint64_t kA = 0;
    hipStream_t stream = nullptr;
};

// A frame's pre-passes on pp (the scene's prep stream, or the frame's own stream); ev0 / pdone:
// their start and end, recorded by the dispatches themselves when the frame's pre-passes are
// timed (events: an event in a dispatch holds it, and the one after it, for the timestamp).
int launch_prepasses(rt_scene* s, const RenderParams& P, int slot, hipStream_t pp, bool events = true) {
    const bool cut = P.cull && P.sc.ncut > 0;
    hipEvent_t ev0 = events ? s->ev0[slot] : nullptr, pdone = events ? s->pdone[slot] : nullptr;
    hipExtLaunchKernelGGL(tile_cull_kernel, dim3((P.tiles_total + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, pp, ev0,
                          cut ? nullptr : pdone, 0, P);
    HIP_TRY(hipGetLastError());
    if (cut) {
        // 16 waves per CU; each takes (list, group) pairs grid-stride (c3: about one each)
        const int cut_blocks = 4 * s->cus * (8 / CUT_GROUP);
        hipExtLaunchKernelGGL(tile_cut_kernel, dim3(cut_blocks), dim3(BLOCK), 0, pp, nullptr, pdone, 0, P);
        HIP_TRY(hipGetLastError());
    }
    return RT_OK;
}

int flush_pair_a(rt_scene* s, PairStage& ps) {
    if (!ps.deferred) return RT_OK;
    ps.deferred = false;
    const int slot = int(ps.kA % rt_scene::kRing);
    s->span[slot] = 1;
    if (int rc = launch_prepasses(s, ps.A, slot, s->prep); rc != RT_OK) return rc;
    HIP_TRY(hipStreamWaitEvent(ps.LA.st, s->pdone[slot], 0));
    launch<RT_KERNEL_WAVE | MODE_WIDE>(ps.A, true, ps.LA);
    HIP_TRY(hipGetLastError());
    if (ps.A.drained) s->drain_frame = ps.kA, s->drain_word = 0;
    return RT_OK;
}

int render_frame(rt_scene* s, const rt_camera* cam, const rt_render_opts* o, float* rgb, int32_t* hit_idx,
                 float* hit_t, uint8_t* p6, void* stream, PairStage* ps);
}  // namespace

extern "C" int rt_render_device_p6(rt_scene* s, const rt_camera* cam, const rt_render_opts* o, float* rgb,
                                   int32_t* hit_idx, float* hit_t, uint8_t* p6, void* stream) {
    return render_frame(s, cam, o, rgb, hit_idx, hit_t, p6, stream, nullptr);
}

extern "C" int rt_render_device_pair(rt_scene* s, const rt_camera* cam_a, const rt_camera* cam_b,
                                     const rt_render_opts* o, float* rgb_a, uint8_t* p6_a, float* rgb_b,
                                     uint8_t* p6_b, void* stream) {
    if (!s || !cam_a || !cam_b || !o || (!rgb_a && !p6_a) || (!rgb_b && !p6_b))
        return set_error(RT_ERR_ARG, "rt_render_device_pair: null argument");
    PairStage ps;
    int rc = render_frame(s, cam_a, o, rgb_a, nullptr, nullptr, p6_a, stream, &ps);
    if (rc != RT_OK) return rc;
    ps.phase = 1;
    rc = render_frame(s, cam_b, o, rgb_b, nullptr, nullptr, p6_b, stream, &ps);
    if (ps.deferred) {  // frame B failed before its launch: frame A still renders
        DeviceGuard g(s->device);
        const int rc2 = flush_pair_a(s, ps);
        if (rc == RT_OK) rc = rc2;
    }
    return rc;
}

namespace {
int render_frame(rt_scene* s, const rt_camera* cam, const rt_render_opts* o, float* rgb, int32_t* hit_idx,
                 float* hit_t, uint8_t* p6, void* stream, PairStage* ps) {
    if (!s || !cam || !o || (!rgb && !p6)) return set_error(RT_ERR_ARG, "rt_render_device: null argument");
    if (o->spp < 1) return set_error(RT_ERR_ARG, "spp must be >= 1");
    if ((hit_idx == nullptr) != (hit_t == nullptr)) return set_error(RT_ERR_ARG, "hit_idx and hit_t go together");
    const int W = cam->pixel_width, H = cam->pixel_height;
    if (W < 1 || H < 1) return set_error(RT_ERR_ARG, "camera has no pixels");
    const int rows = rt_shard_rows(H, o->band_rows, o->band_index, o->band_count);
    if (rows < 0) return set_error(RT_ERR_ARG, "bad band sharding parameters");
    DeviceGuard g(s->device);
    int rc = prepare_jitter(s, o);
    if (rc != RT_OK) return rc;
    if (rows == 0) return RT_OK;

    RenderParams P;
    std::memset(&P, 0, sizeof(P));
    P.sc = scene_view(s);
    if (o->flags & RT_FLAG_BINARY) P.sc.wide = 0;
    // RT_TUNE_CULL_COVERAGE: tests force the cut pass on (>= 1: always, untested candidates none)
    const double max_cov = rt::tuning(RT_TUNE_CULL_COVERAGE, 0.3);
    if (P.sc.ncut > 0 && !(root_box_coverage(s->root_box, cam) <= max_cov)) P.sc.ncut = 0;
    P.cut_force = max_cov >= 1.0 ? 1 : 0;
    P.cam_center = f3{cam->center.x, cam->center.y, cam->center.z};
    P.cam_p00 = f3{cam->pixel00_loc.x, cam->pixel00_loc.y, cam->pixel00_loc.z};
    P.cam_du = f3{cam->pixel_delta_u.x, cam->pixel_delta_u.y, cam->pixel_delta_u.z};
    P.cam_dv = f3{cam->pixel_delta_v.x, cam->pixel_delta_v.y, cam->pixel_delta_v.z};
    P.W = W;
    P.H = H;
    P.spp = o->spp;
    P.max_depth = o->max_depth;
    P.diffuse_bounce = o->diffuse_bounce ? 1 : 0;
    P.miss = f3{o->miss_color.x, o->miss_color.y, o->miss_color.z};
    P.jitter = static_cast<const float*>(s->jitter.p);
    P.band_rows = o->band_count <= 1 ? H : o->band_rows;
    P.band_index = o->band_count <= 1 ? 0 : o->band_index;
    P.band_count = o->band_count <= 1 ? 1 : o->band_count;
    P.rows = rows;
    P.rgb = rgb;
    P.hit_idx = hit_idx;
    P.hit_t = hit_t;
    P.p6 = p6;
    P.ray_count = t_ray_count;
    {
        const f3 mp = miss_pixel_value(o);
        P.miss_p6[0] = rtp::p6_default_sample(mp.x);
        P.miss_p6[1] = rtp::p6_default_sample(mp.y);
        P.miss_p6[2] = rtp::p6_default_sample(mp.z);
        P.miss_p6[3] = 0;
    }
    // A table with a non-finite entry gives that sample's rays a NaN direction.  In the reference
    // every compare of such a ray is false: every box test passes, every triangle "hits" with t =
    // NaN, and the ray ends on the last triangle of its own DFS.  The lane kernel is that DFS ray by
    // ray; the wave kernels' group-wide tests (the family's min / max drop a NaN lane) are not, so
    // such a frame takes the lane kernel.
    // A non-finite camera word gives exactly these rays for every sample, and so does a |D| that
    // overflows (a zero direction, or NaN once the pixel position is inf - inf): camera_class.
    const bool jfinite = jitter_finite(s->jitter_host);
    const int cam_class = jfinite ? camera_class(cam, jitter_pad(s->jitter_host)) : RT_CAMERA_LANE;
    const int kernel = cam_class != RT_CAMERA_LANE ? o->kernel : RT_KERNEL_LANE;
    const bool samples = kernel != RT_KERNEL_WAVE_PIXELS && o->spp <= BLOCK && (o->spp & (o->spp - 1)) == 0;
    // Half waves (32 samples per wave) for the shards of an 8-way split: a shard's kernel is then
    // bound by its longest waves, and halving their rays shortens them (c3 band shards on one
    // GPU, max over the 8: kernel 0.101 -> 0.095 ms, frame 0.122 -> 0.116; at 4 and fewer shards
    // the doubled wave count costs more: N = 4 0.106 -> 0.116, N = 1 0.211 -> 0.373;
    // scripts/half_waves_ab.py).  RT_TUNE_HALF_WAVES = 0/1 overrides.  (Quarter waves,
    // 16 samples, measured slower at N = 8 and were dropped.)
    // The multi-bounce kernels take half waves at any split: a wave's bounce paths end with its
    // longest lane's, and the longest waves bound the kernel (c3b 1.96 vs 2.37 ms per frame).
    // (With the frustum traversal, profiles/r04/exp/half_waves_ab_c3.log: N = 8 max kernel 0.0758
    // vs 0.0867 ms, N = 4 0.0831 vs 0.0857, N = 2 0.140 vs 0.097: half waves from 4 shards.)
    int half = o->band_count >= 4 || o->max_depth > 1 ? 1 : 0;
    if (const double h = rt::tuning(RT_TUNE_HALF_WAVES, -1.0); h >= 0.0) half = h >= 1.0 ? 1 : 0;
    if (!samples || o->spp > (64 >> half)) half = 0;
    P.half_waves = half;
    // One light and a tree whose DFS fits the per-lane LDS stacks: the bounce kernels that hold
    // only the paired loop (paired_bounces), fewer live registers than the kernels that also
    // carry the unpaired one.  RT_PAIRED_ONLY=0 turns them off (A/B: the unpaired loop on half waves).
    P.paired_only = half && o->max_depth > 1 && s->nlights == 1 && !s->deep && kernel != RT_KERNEL_LANE &&
                            (P.sc.wide ? s->lane_wide : s->lane_stack)
                        ? 1
                        : 0;
    P.paired_only = P.paired_only && rt::tuning(RT_TUNE_PAIRED_ONLY, 1.0) != 0.0;
    int ppb = samples ? (BLOCK >> half) / o->spp : BLOCK;  // pixels per block
    int tw = 1;
    while (tw * tw < ppb) tw <<= 1;                // square-ish power-of-two tile
    int th = ppb / tw;
    P.tile_w = tw;
    P.tile_h = th;
    P.tile_w_log2 = __builtin_ctz(unsigned(tw));
    P.spp_log2 = samples ? __builtin_ctz(unsigned(o->spp)) : 0;
    P.tiles_x = (W + tw - 1) / tw;
    {
        const TileDiv td = tile_div_make((uint32_t)P.tiles_x);
        P.tiles_x_mul = td.mul;
        P.tiles_x_shift = td.shift;
    }
    const int tiles_y = (rows + th - 1) / th;
    P.tiles_total = P.tiles_x * tiles_y;
    P.lane_samples = samples ? 1 : 0;
    P.tile_order = o->tile_order == RT_TILES_AUTO ? RT_TILES_ROWS : o->tile_order;
    P.cull = (o->flags & RT_FLAG_NO_CULL) ? 0 : 1;
    // The tile tests pad a tile by one pixel (tile_dirs_f): that covers a jitter table whose every
    // entry is finite with |entry| <= 1, the default table among them.  Any other caller table
    // (a wide reconstruction filter, a sub-frame shift) renders without the cull: as exact.
    if (P.cull && !jitter_within_pad(s->jitter_host)) P.cull = 0;
    // The tile tests take every ray direction for a positive multiple of D (tile_dirs_f): only a
    // camera whose |D| range is proven (camera_class) is culled or cut.
    if (cam_class != RT_CAMERA_PROVEN) P.cull = 0;
    if (!P.cull) P.sc.ncut = 0;  // the render kernel reads the cut pass's lists only when it ran
    P.miss_pixel = miss_pixel_value(o);
    P.nqueues = P.tile_order == RT_TILES_LINEAR ? 1 : 8;
    // a list holds at most tiles_x * ceil(tiles_y / 8) tiles (RT_TILES_ROWS) or ceil(tiles / 8)
    // (RT_TILES_XCD_CHUNK): tiles_x * ceil(tiles_y / 8) bounds both
    P.queue_cap = P.tile_order == RT_TILES_LINEAR ? P.tiles_total : P.tiles_x * ((tiles_y + 7) / 8);
    // Heavy-first dispatch needs the cut pass (it builds the heavy lists) and the 8 lists.
    // RT_TUNE_HEAVY_FRAC (speed experiments): a tile is in heavy class c when one of its waves took
    // at least 2^(2-c) times this fraction of the latest finished frame's render kernel
    // (0: off).
    // c3 (frustum traversal, profiles/r04/exp/heavy_frac_ab_c3*.log): 0.05 0.153, 0.06 0.149,
    // 0.08 0.148, 0.10 0.147, 0.12 0.150, 0.18 0.151, 0.25 0.158 ms, off 0.187
    const double heavy_frac = rt::tuning(RT_TUNE_HEAVY_FRAC, 0.10);
    const int mode = kernel == RT_KERNEL_LANE ? RT_KERNEL_LANE : RT_KERNEL_WAVE;
    const bool costs = P.cull && P.sc.ncut > 0 && P.nqueues == 8 && heavy_frac > 0.0;
    // RT_TUNE_HEAVY_CAP: entries per (class, list) (speed experiments)
    const int heavy_cap = int(std::clamp(rt::tuning(RT_TUNE_HEAVY_CAP, 512.0), 1.0, 1e9));
    P.heavy_cap = costs ? std::min(P.queue_cap, heavy_cap) : 0;
    // kSets counter sets (8 live lists, one spare, 8 heavy lists each) at fixed offsets, then
    // kSets x (live lists | cut survivor lists | heavy lists) sized for this geometry; rotating by frame
    constexpr size_t kCounterBytes = COUNTER_SET_U32 * sizeof(uint32_t);
    const size_t list_bytes = size_t(P.nqueues) * size_t(P.queue_cap) * sizeof(int32_t);
    const size_t cut_bytes = P.sc.ncut > 0 ? list_bytes : 0;
    const size_t heavy_bytes = size_t(8 * NCLASS) * size_t(P.heavy_cap) * sizeof(int32_t);
    const size_t set_bytes = list_bytes + cut_bytes + heavy_bytes;
    const size_t work_bytes = rt_scene::kSets * (kCounterBytes + set_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t k = s->launches;
    auto ev1_of = [&](uint64_t f) { return s->ev1[f % rt_scene::kRing]; };
    // The latest finished frame's render-kernel time sets the heavy threshold (non-blocking
    // queries; none finished yet: the previous estimate, or no heavy lists).  The frames are
    // scanned forward from the oldest one not yet seen finished (amortised one query per
    // frame), so a caller that submits many frames ahead of the GPU still gets an estimate once
    // its first frames finish (a look-back over the last three frames found none: all in flight).
    // frame B of a pair whose frame A waits in ps: its tiles and cut must be A's
    bool pair_b = ps && ps->phase == 1 && ps->deferred;
    if (pair_b) {
        const RenderParams& A = ps->A;
        const bool same = A.tiles_total == P.tiles_total && A.tiles_x == P.tiles_x && A.W == P.W && A.rows == P.rows &&
                          A.spp == P.spp && A.half_waves == P.half_waves && A.sc.ncut == P.sc.ncut && A.cull == P.cull &&
                          A.heavy_cap == P.heavy_cap && A.queue_cap == P.queue_cap && A.nqueues == P.nqueues &&
                          A.max_depth == P.max_depth && A.paired_only == P.paired_only && A.band_index == P.band_index &&
                          A.band_count == P.band_count && ps->stream == static_cast<hipStream_t>(stream) &&
                          mode == RT_KERNEL_WAVE;  // (a camera that takes frame B to the lane kernel: camera_class)
        if (!same) {
            pair_b = false;
            if ((rc = flush_pair_a(s, *ps)) != RT_OK) return rc;
        }
    }
    bool cost_reset = false;
    if (costs) {
        uint64_t f = std::max<uint64_t>(s->est_next, k >= uint64_t(rt_scene::kRing) ? k - (rt_scene::kRing - 1) : 0);
        int64_t last = -1;
        const uint64_t f_end = ps && ps->deferred ? k - 1 : k;  // frame A's events are not recorded yet
        for (; f < f_end; ++f) {
            if (hipEventQuery(s->ev1[f % rt_scene::kRing]) != hipSuccess) break;
            last = int64_t(f);
        }
        s->est_next = f;
        if (last >= 0) {
            const int fl = int(uint64_t(last) % rt_scene::kRing);
            // the render kernel's time, or the frame period when shorter (overlapping frames:
            // RT_FLAG_OVERLAP starts a kernel while the previous one still runs); a pair
            // kernel's time per frame
            float ms = 0.f, period = 0.f;
            if (s->timed[fl] && hipEventElapsedTime(&ms, s->evm[fl], s->ev1[fl]) == hipSuccess) {
                const int f0 = int(uint64_t(last - 1) % rt_scene::kRing);
                if (s->span[fl] > 1) ms /= float(s->span[fl]);
                else if (last >= 1 && s->span[f0] == 1 &&
                         hipEventElapsedTime(&period, s->ev1[f0], s->ev1[fl]) == hipSuccess && period > 0.f)
                    ms = std::min(ms, period);
                s->kernel_ms_est = ms;
            }
        }
        (void)hipGetLastError();  // a not-ready query is not an error of this call
        // 10 ns ticks (wall_clock64 runs at 100 MHz)
        for (int c = 0; c < NCLASS; ++c) {
            const double ticks = std::ldexp(heavy_frac, 2 - c) * double(s->kernel_ms_est) * 1e5;
            const bool used = c < (o->max_depth == 1 ? NCLASS_D1 : NCLASS);
            P.heavy_ticks[c] = s->kernel_ms_est > 0.f && used ? uint32_t(std::clamp(ticks, 1.0, 65535.0)) : 0xffffffffu;
        }
        // the costs are per tile of this geometry
        const uint64_t key = (uint64_t(uint32_t(P.tiles_total)) * 0x9E3779B97F4A7C15ull) ^
                             (uint64_t(uint32_t(P.tiles_x)) << 40) ^ (uint64_t(uint32_t(W)) << 20) ^
                             uint64_t(uint32_t(rows)) ^ (uint64_t(uint32_t(P.band_index)) << 52) ^
                             (uint64_t(uint32_t(P.band_count)) << 58) ^ (uint64_t(uint32_t(P.spp)) << 32);
        const size_t cost_bytes = size_t(P.tiles_total) * 4 * sizeof(uint16_t);
        if (s->cost.n < cost_bytes) {
            if (k > 0) {  // the old buffer may still be written
                HIP_TRY(hipStreamSynchronize(s->prep));
                for (hipStream_t r : s->rstream) HIP_TRY(hipStreamSynchronize(r));
                HIP_TRY(hipEventSynchronize(ev1_of(k - 1)));
            }
            if ((rc = s->cost.alloc(cost_bytes)) != RT_OK) return rc;
            s->cost_key = ~key;
        }
        cost_reset = s->cost_key != key;
        s->cost_key = key;
        P.tile_cost = static_cast<uint16_t*>(s->cost.p);
    }
    s->last_heavy_cap = P.heavy_cap;
    if (s->work.n < work_bytes) {
        if (k > 0) {  // the old buffers may still be read
            HIP_TRY(hipStreamSynchronize(s->prep));
            for (hipStream_t r : s->rstream) HIP_TRY(hipStreamSynchronize(r));
            HIP_TRY(hipEventSynchronize(ev1_of(k - 1)));
        }
        if ((rc = s->work.alloc(work_bytes)) != RT_OK) return rc;
        s->counters_dirty = true;
    }
    // This frame's outputs against the previous frame's: overlapping ranges (a caller reusing
    // one buffer) make the pre-passes, which write the culled tiles' pixels, wait for the
    // previous render kernel; distinct buffers (rt_renderer's frame slots) let them overlap it.
    const size_t npx = size_t(rows) * size_t(W);
    const rt_scene::Range out_now[4] = {
        {uintptr_t(rgb), uintptr_t(rgb) + (rgb ? npx * 3 * sizeof(float) : 0)},
        {uintptr_t(p6), uintptr_t(p6) + (p6 ? npx * 3 : 0)},
        {uintptr_t(hit_idx), uintptr_t(hit_idx) + (hit_idx ? npx * size_t(o->spp) * sizeof(int32_t) : 0)},
        {uintptr_t(hit_t), uintptr_t(hit_t) + (hit_t ? npx * size_t(o->spp) * sizeof(float) : 0)}};
    // a new list layout may place this frame's lists over the previous frame's: serialise too
    bool overlap = s->set_bytes != set_bytes || cost_reset;
    for (const auto& a : out_now)
        for (const auto& b : s->prev_out)
            overlap = overlap || (a.lo < a.hi && b.lo < b.hi && a.lo < b.hi && b.lo < a.hi);
    if (pair_b && overlap) {  // frame B writes over frame A: A renders first, on its own
        pair_b = false;
        if ((rc = flush_pair_a(s, *ps)) != RT_OK) return rc;
    }
    const size_t big_bytes = size_t(std::max(0.0, rt::tuning(RT_TUNE_BIG_SCENE_BYTES, double(kBigSceneBytes))));
    // RT_TUNE_FRAME_STREAMS: a caller-ordered single frame of an unsharded image takes the frame
    // streams (pairs and band shards keep the prep-stream schedule); RT_TUNE_OVERLAP_FRAMES then
    // adds nothing, the render kernels overlap already
    const bool fs = s->caller_ordered && !ps && P.band_count == 1 && rt::tuning(RT_TUNE_FRAME_STREAMS, 1.0) > 0.5;
    const bool ovl = !fs && s->caller_ordered && rt::tuning(RT_TUNE_OVERLAP_FRAMES, 0.0) > 0.5;
    // frame A of a pair: its launch waits for frame B's call (PairStage)
    const bool pair_a = ps && ps->phase == 0 && rt::tuning(RT_TUNE_PAIR_FRAMES, 1.0) > 0.5 && !ovl &&
                        pair_kernel_fits(P, samples, !s->deep && mode == RT_KERNEL_WAVE && P.sc.wide != 0,
                                         s->bytes > big_bytes);
    // the previous frame of this scene ran on another stream: wait for it.  (Letting two frames'
    // render kernels overlap on two streams, the next filling the CUs the last waves of the
    // previous one leave idle, measured slower for rt_renderer: 0.257 vs 0.246 ms per c3 frame.)
    if (k > 0 && st != s->last_stream) {
        HIP_TRY(hipStreamWaitEvent(st, ev1_of(k - 1), 0));
        // (overlapping frames, RT_TUNE_OVERLAP_FRAMES: the one before may finish last)
        if (k > 1) HIP_TRY(hipStreamWaitEvent(st, ev1_of(k - 2), 0));
    }
    s->last_stream = st;
    // The other schedule than the previous frame's (the knob flipped, or a direct call between a
    // renderer's frames): no order between the streams of the two holds across the change, and
    // it is rare, so the host waits for all of them.  So does a frame-stream frame that zeroes
    // every counter set (after a failed frame): the frame before it runs on the other stream.
    if (k > 0 && (s->last_fs != fs || (fs && s->counters_dirty))) {
        HIP_TRY(hipStreamSynchronize(s->prep));
        for (hipStream_t r : s->rstream) HIP_TRY(hipStreamSynchronize(r));
        HIP_TRY(hipEventSynchronize(ev1_of(k - 1)));
    }
    s->last_fs = fs;
    const int set = int(k % rt_scene::kSets), nset = int((k + 2) % rt_scene::kSets);
    char* base = static_cast<char*>(s->work.p);
    char* lists = base + rt_scene::kSets * kCounterBytes + set * set_bytes;
    P.live_count = reinterpret_cast<uint32_t*>(base + set * kCounterBytes);
    P.next_count = reinterpret_cast<uint32_t*>(base + nset * kCounterBytes);
    s->last_tiles_total = P.tiles_total;
    P.live_tiles = reinterpret_cast<int32_t*>(lists);
    P.cut_tiles = reinterpret_cast<int32_t*>(lists + list_bytes);
    P.heavy_tiles = reinterpret_cast<int32_t*>(lists + list_bytes + cut_bytes);
    const int slot = int(k % rt_scene::kRing);
    // From the cull launch on, a failure leaves the counter sets unknown (counters_dirty).
    auto frame = [&]() -> int {
        // frame streams: the whole chain on this frame's stream, else the pre-passes on prep
        hipStream_t pp = fs ? s->rstream[k & 1] : s->prep;
        P.drain_tag = uint32_t(k + 1);
        // set k was last read by frame k-6, set k+2 (zeroed by this cull pass) by frame k-4: a
        // frame waits for frame k-2 (the render kernel before the one its pre-passes overlap).
        // Frame A of a pair, k, waits for frame k-3 (the pair before the one running: frames
        // up to k-3 used the sets the pair reads and zeroes) and covers frame B: the pair's
        // pre-passes are launched together, after B's call has set B up.
        // On the frame streams frame k-2 is the work before this frame on its stream.  (The
        // pre-passes of frames k and k-1 are then ordered by the gate alone, and not at all
        // without it: they share no set.  A memset does touch other frames' sets, so the frame
        // after one waits for that frame.)
        if (fs) {
            if (k >= 1 && (overlap || s->serialise_next)) HIP_TRY(hipStreamWaitEvent(pp, ev1_of(k - 1), 0));
        } else {
            if (pair_a) {
                if (k >= 3) HIP_TRY(hipStreamWaitEvent(pp, ev1_of(k - 3), 0));
            } else if (!pair_b && k >= 2) {
                HIP_TRY(hipStreamWaitEvent(pp, ev1_of(k - 2), 0));
            }
            if (k >= 1 && overlap) HIP_TRY(hipStreamWaitEvent(pp, ev1_of(k - 1), 0));
        }
        s->serialise_next = fs && (s->counters_dirty || cost_reset);
        // the pre-pass gate: frame k-1's render kernel opens it when its first queue drains
        if (k >= 1 && s->drain_frame == k - 1)
            HIP_TRY(hipStreamWaitValue32(pp, s->drain + s->drain_word * rt_scene::kDrainStride, uint32_t(k),
                                         hipStreamWaitValueGte, 0xFFFFFFFFu));
        if (!s->caller_ordered) {  // stream order for the caller's buffers (see rt_scene::evq)
            HIP_TRY(hipEventRecord(s->evq[slot], st));
            HIP_TRY(hipStreamWaitEvent(pp, s->evq[slot], 0));
        }
        if (s->counters_dirty) {
            HIP_TRY(hipMemsetAsync(base, 0, rt_scene::kSets * kCounterBytes, pp));
            s->counters_dirty = false;
        }
        if (cost_reset) HIP_TRY(hipMemsetAsync(s->cost.p, 0, s->cost.n, pp));  // no heavy tiles yet
        // RT_TUNE_KERNEL_TIMING_EVERY: the caller-ordered (rt_renderer) frames record the render
        // kernel's start event in one frame of this many (direct calls: every frame); a pair
        // kernel's start is frame A's (frame B's slot is never timed).  On the frame streams the
        // pre-passes' events go with it, unless the caller reads every frame's start; there a
        // timed frame's three events cost ~30 us of its chain (8-17 us each when most frames
        // carry none), so the default is one frame in 16.
        const uint64_t every =
            uint64_t(std::clamp(rt::tuning(RT_TUNE_KERNEL_TIMING_EVERY, fs ? 16.0 : 4.0), 1.0, 256.0));
        s->timed[slot] = !pair_b && (!s->caller_ordered || k % every == 0 || (pair_a && (k + 1) % every == 0));
        s->ptimed[slot] = !fs || s->timed[slot] || s->want_start;
        // frame A of a pair: its pre-passes go out with frame B's (pair_b below, or flush_pair_a)
        if (pair_b) {
            // both frames' passes in one cull and one cut launch (the same cut: the pair's tile
            // geometry check); frame A's events bracket them, frame B's follow
            const int slot_a = int(ps->kA % rt_scene::kRing);
            PairParams PP;
            PP.f[0] = ps->A;
            PP.f[1] = P;
            // (frame B's pdone is the last launch's own end event: the render stream waits for it)
            const bool cut = P.cull && P.sc.ncut > 0;
            HIP_TRY(hipEventRecord(s->ev0[slot], pp));  // both frames' pre-pass times span the pair's
            hipExtLaunchKernelGGL(tile_cull_pair_kernel,
                                  dim3((ps->A.tiles_total + BLOCK - 1) / BLOCK + (P.tiles_total + BLOCK - 1) / BLOCK),
                                  dim3(BLOCK), 0, pp, s->ev0[slot_a], cut ? nullptr : s->pdone[slot], 0, PP);
            HIP_TRY(hipGetLastError());
            if (cut) {
                // 32 waves per CU (the cut kernel's occupancy): the pair's cut mostly runs after
                // the previous pair kernel has left the GPU, latency-bound per unit
                hipExtLaunchKernelGGL(tile_cut_pair_kernel, dim3(8 * s->cus * (8 / CUT_GROUP)), dim3(BLOCK), 0, pp, nullptr,
                                      s->pdone[slot], 0, PP);
                HIP_TRY(hipGetLastError());
            }
            HIP_TRY(hipEventRecord(s->pdone[slot_a], pp));
        } else if (!pair_a) {
            if ((rc = launch_prepasses(s, P, slot, pp, s->ptimed[slot])) != RT_OK) return rc;
        }
        // Frame streams: the render kernel follows the cut on the frame's stream.
        // RT_TUNE_OVERLAP_FRAMES: the render kernel on one of the scene's two render streams (the
        // caller orders its buffers itself; its stream then waits for the kernel), else on the
        // caller's stream
        const hipStream_t rs = fs ? pp : ovl ? s->rstream[k & 1] : st;
        // (frame A of a pair: frame B's pdone, later on the same prep stream, covers both)
        if (!pair_a && !fs) HIP_TRY(hipStreamWaitEvent(rs, s->pdone[slot], 0));
        const bool qr = P.sc.qent != nullptr && P.sc.f_log2 > 2;
        s->span[slot] = pair_a || pair_b ? 2 : 1;
        const Launch L{rs, s->timed[slot] ? s->evm[slot] : nullptr, s->ev1[slot], s->cus, s->bytes > big_bytes, qr,
                       &s->last_kernel};
        // RT_TUNE_PREPASS_GATE f in (0, 1]: this kernel opens the next frame's pre-passes when
        // its first queue has handed out the fraction f of its items (0.5 default; 1: drained);
        // 0 they start once the frame before this one has finished
        // (0.5: c3 0.1557-0.157 ms per delivered frame vs 0.1587-0.1593 at 1.0, the pre-passes
        // then finishing well before this kernel does; profiles/r05/exp/prepass_gate_frac_c3.log)
        // The gate word takes plain stores, so it needs one writer kernel at a time: with
        // overlapping frames (ovl: two render streams) a late store of frame k-2's kernel could
        // overwrite frame k-1's tag after frame k had started waiting for it, so ovl runs ungated.
        // The frame streams have a word each: its writers are the kernels of one stream, in turn.
        const double gate_f = ovl ? 0.0 : rt::tuning(RT_TUNE_PREPASS_GATE, 0.5);
        const bool gate = gate_f > 0.0;
        const int word = fs ? int(k & 1) : 0;
        P.drained = gate ? s->drain + word * rt_scene::kDrainStride : nullptr;
        P.drain_tag = uint32_t(k + 1);
        P.gate_q8 = int(std::clamp(gate_f, 0.0, 1.0) * 256.0 + 0.5);
        if (pair_a) {  // held for frame B's call
            ps->A = P;
            ps->LA = L;
            ps->kA = k;
            ps->stream = st;
            ps->deferred = true;
            return RT_OK;
        }
        if (pair_b) {
            // one grid over both frames: frame A's events bracket it (its start event when A is a
            // timed frame), frame B's end event follows; frame B's parameters carry the gate
            const int slot_a = int(ps->kA % rt_scene::kRing);
            RenderParams A = ps->A;
            A.drained = nullptr;
            const Launch LP{rs, s->timed[slot_a] ? s->evm[slot_a] : nullptr, s->ev1[slot_a], s->cus, false, false,
                            &s->last_kernel};
            ps->deferred = false;
            launch_pair(A, P, LP);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(s->ev1[slot], rs));
            if (gate) s->drain_frame = k, s->drain_word = word;
            return RT_OK;
        }
        if (s->deep) launch<MODE_DEEP>(P, samples, L);
        else if (mode == RT_KERNEL_LANE) launch<RT_KERNEL_LANE>(P, samples, L);
        else if (P.sc.wide) launch<RT_KERNEL_WAVE | MODE_WIDE>(P, samples, L);
        else launch<RT_KERNEL_WAVE>(P, samples, L);
        HIP_TRY(hipGetLastError());
        if (gate) s->drain_frame = k, s->drain_word = word;
        // the caller's stream follows the frame, as if the kernel had run on it
        if (ovl || fs) HIP_TRY(hipStreamWaitEvent(st, s->ev1[slot], 0));
        return RT_OK;
    };
    std::copy(std::begin(out_now), std::end(out_now), std::begin(s->prev_out));
    s->set_bytes = set_bytes;
    rc = frame();
    s->launches++;  // the events of this slot belong to this frame even when it failed
    if (rc != RT_OK) s->counters_dirty = true;
    return rc;
}
}  // namespace

#include "rt_query_host.hpp"

void rt::scene_set_caller_ordered(rt_scene* s, bool on, bool frame_start) {
    if (!s) return;
    s->caller_ordered = on;
    s->want_start = frame_start;
}

void rt::scene_frame_events(const rt_scene* s, hipEvent_t* first, hipEvent_t* last, int back) {
    hipEvent_t a = nullptr, b = nullptr;
    if (s && s->launches > uint64_t(back)) {
        const int slot = int((s->launches - 1 - uint64_t(back)) % rt_scene::kRing);
        a = s->ptimed[slot] ? s->ev0[slot] : nullptr;
        b = s->ev1[slot];
    }
    if (first) *first = a;
    if (last) *last = b;
}

namespace {
// what: 0 render kernel (evm -> ev1), 1 pre-passes (ev0 -> pdone), 2 both (the frame's device
// work: its pre-passes overlap the previous frame's render kernel, so the span ev0 -> ev1 would
// include the wait for it)
int event_times(const rt_scene* s, int what, float* ms_out, int max, int* n_out) {
    if (!s || max < 0 || (max > 0 && !ms_out)) return set_error(RT_ERR_ARG, "kernel times: bad args");
    DeviceGuard g(s->device);
    const uint64_t have = std::min<uint64_t>(s->launches, uint64_t(rt_scene::kRing));
    // the most recent frames with a kernel start event (all of them unless the renderer samples,
    // RT_TUNE_KERNEL_TIMING_EVERY), at most max, oldest first; the pre-passes' events ride on
    // every frame of the prep-stream schedule and on the timed frames of the frame streams
    std::vector<int> slots;
    for (uint64_t b = 1; b <= have && (int)slots.size() < max; ++b) {
        const int slot = int((s->launches - b) % rt_scene::kRing);
        if ((what == 0 || s->ptimed[slot]) && (what == 1 || s->timed[slot])) slots.push_back(slot);
    }
    const int n = (int)slots.size();
    for (int k = 0; k < n; ++k) {
        const int slot = slots[size_t(n - 1 - k)];
        HIP_TRY(hipEventSynchronize(s->ev1[slot]));
        float kern = 0.f, prep = 0.f;
        if (what != 1) HIP_TRY(hipEventElapsedTime(&kern, s->evm[slot], s->ev1[slot]));
        if (what != 0) HIP_TRY(hipEventElapsedTime(&prep, s->ev0[slot], s->pdone[slot]));
        ms_out[k] = kern + prep;
    }
    if (n_out) *n_out = n;
    return RT_OK;
}
}  // namespace

namespace {
int live_tiles(const rt_scene* s, int64_t* live, int64_t* heavy, int64_t* total) {
    if (!s || !live || !total) return set_error(RT_ERR_ARG, "rt_live_tiles: null argument");
    *live = 0;
    *total = s->last_tiles_total;
    if (!s->work.p || s->launches == 0) return RT_OK;
    DeviceGuard g(s->device);
    const int slot = int((s->launches - 1) % rt_scene::kRing);
    HIP_TRY(hipEventSynchronize(s->ev1[slot]));
    uint32_t c[COUNTER_SET_U32];
    // the last frame's counter set (the sets sit at the start of the work buffer)
    const size_t counter_bytes = COUNTER_SET_U32 * sizeof(uint32_t);
    HIP_TRY(hipMemcpy(c, static_cast<const char*>(s->work.p) + ((s->launches - 1) % rt_scene::kSets) * counter_bytes, sizeof(c),
                      hipMemcpyDeviceToHost));
    for (int k = 0; k < 8; ++k) *live += c[k * COUNTER_STRIDE];
    if (heavy) {
        *heavy = 0;
        if (s->last_heavy_cap > 0)
            for (int k = 0; k < 8 * NCLASS; ++k)
                *heavy += std::min<int64_t>(c[(HEAVY_SLOT0 + k) * COUNTER_STRIDE], s->last_heavy_cap);
    }
    return RT_OK;
}
}  // namespace

extern "C" int rt_live_tiles(const rt_scene* s, int64_t* live, int64_t* total) {
    return live_tiles(s, live, nullptr, total);
}

extern "C" const char* rt_scene_kernel_name(const rt_scene* s) {
    return (s && s->last_kernel) ? s->last_kernel : "";
}

extern "C" int rt_heavy_tiles(const rt_scene* s, int64_t* heavy) {
    if (!heavy) return set_error(RT_ERR_ARG, "rt_heavy_tiles: null argument");
    int64_t live = 0, total = 0;
    *heavy = 0;
    return live_tiles(s, &live, heavy, &total);
}

#ifdef RT_STATS
extern "C" int rt_debug_stats(unsigned long long* out, int reset) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rt_stats), sizeof(g_rt_stats)));
    if (reset) {
        unsigned long long z[24] = {};
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_rt_stats), z, sizeof(z)));
    }
    return RT_OK;
}
#endif

#ifdef RT_WAVE_TIMES
extern "C" int rt_debug_wave_meta_set(void* dev_ptr) {
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_wave_meta), &dev_ptr, sizeof(dev_ptr)));
    return RT_OK;
}
extern "C" int rt_debug_wave_phase_set(void* dev_ptr) {
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_wave_phase), &dev_ptr, sizeof(dev_ptr)));
    return RT_OK;
}
#ifdef RT_LANE_ITERS
extern "C" int rt_debug_lane_iters_set(void* iters_ptr, void* acc_ptr) {
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_lane_iters), &iters_ptr, sizeof(iters_ptr)));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_lane_acc), &acc_ptr, sizeof(acc_ptr)));
    return RT_OK;
}
#endif
extern "C" int rt_debug_wave_times_set(void* dev_ptr, void* cut_counts_ptr) {
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_wave_times), &dev_ptr, sizeof(dev_ptr)));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_cut_counts), &cut_counts_ptr, sizeof(cut_counts_ptr)));
    return RT_OK;
}
#endif
#ifdef RT_FRAME_SPAN
extern "C" int rt_debug_frame_span_set(void* dev_ptr) {
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_frame_span), &dev_ptr, sizeof(dev_ptr)));
    return RT_OK;
}
#endif

extern "C" int rt_kernel_times(const rt_scene* s, float* ms_out, int max, int* n_out) {
    return event_times(s, 0, ms_out, max, n_out);
}

extern "C" int rt_frame_times(const rt_scene* s, float* ms_out, int max, int* n_out) {
    return event_times(s, 2, ms_out, max, n_out);
}

extern "C" int rt_prepass_times(const rt_scene* s, float* ms_out, int max, int* n_out) {
    return event_times(s, 1, ms_out, max, n_out);
}

extern "C" int rt_render(rt_scene* s, const rt_camera* cam, const rt_render_opts* o, float* rgb_host,
                         int32_t* hit_idx_host, float* hit_t_host) {
    if (!s || !cam || !o || !rgb_host) return set_error(RT_ERR_ARG, "rt_render: null argument");
    if ((hit_idx_host == nullptr) != (hit_t_host == nullptr)) return set_error(RT_ERR_ARG, "hit_idx and hit_t go together");
    const int rows = rt_shard_rows(cam->pixel_height, o->band_rows, o->band_index, o->band_count);
    if (rows < 0) return set_error(RT_ERR_ARG, "bad band sharding parameters");
    if (o->spp < 1) return set_error(RT_ERR_ARG, "spp must be >= 1");
    DeviceGuard g(s->device);
    const size_t npx = size_t(rows) * size_t(std::max(cam->pixel_width, 0));
    DevBuf rgb, hi, ht;
    int rc;
    if ((rc = rgb.alloc(npx * 3 * sizeof(float))) != RT_OK) return rc;
    if (hit_idx_host) {
        if ((rc = hi.alloc(npx * size_t(o->spp) * sizeof(int32_t))) != RT_OK) return rc;
        if ((rc = ht.alloc(npx * size_t(o->spp) * sizeof(float))) != RT_OK) return rc;
    }
    // the fault word belongs to this frame: earlier frames finish first, then it is cleared
    // (rt_scene_faults still sees what this frame raised)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(s->fault.p, 0, sizeof(uint32_t)));
    HIP_TRY(hipDeviceSynchronize());  // (the frame runs on the scene's non-blocking streams)
    rc = rt_render_device(s, cam, o, static_cast<float*>(rgb.p), static_cast<int32_t*>(hi.p),
                          static_cast<float*>(ht.p), nullptr);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (npx) HIP_TRY(hipMemcpy(rgb_host, rgb.p, npx * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (hit_idx_host && npx) {
        HIP_TRY(hipMemcpy(hit_idx_host, hi.p, npx * size_t(o->spp) * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(hit_t_host, ht.p, npx * size_t(o->spp) * sizeof(float), hipMemcpyDeviceToHost));
    }
    // a device-side guard fired (the frame's answers are poisoned where it did): loud, not silent
    uint32_t fault = 0;
    HIP_TRY(hipMemcpy(&fault, s->fault.p, sizeof(fault), hipMemcpyDeviceToHost));
    if (fault & RT_FAULT_FRUSTUM_STACK) return set_error(RT_ERR_INTERNAL, "frustum traversal stack overflow");
    return RT_OK;
}

// Rays one frame traces, by the oracle's classes (orc_stats.rays: camera, shadow, bounce).
// Camera rays are W*rows*spp whenever max_depth > 0 (TraceRayIterative traces every sample);
// shadow and bounce rays are counted on the device by one LANE-kernel render of the frame
// (wave-aggregated atomics; the frame itself is discarded).  Synchronous.
extern "C" int rt_count_rays(rt_scene* s, const rt_camera* cam, const rt_render_opts* o, uint64_t* counts) {
    if (!counts) return set_error(RT_ERR_ARG, "rt_count_rays: null argument");
    uint64_t c4[4];
    const int rc = rt_count_rays_ex(s, cam, o, c4);
    if (rc == RT_OK) std::memcpy(counts, c4, 3 * sizeof(uint64_t));
    return rc;
}

extern "C" int rt_count_rays_ex(rt_scene* s, const rt_camera* cam, const rt_render_opts* o, uint64_t* counts) {
    if (!s || !cam || !o || !counts) return set_error(RT_ERR_ARG, "rt_count_rays: null argument");
    const int rows = rt_shard_rows(cam->pixel_height, o->band_rows, o->band_index, o->band_count);
    if (rows < 0) return set_error(RT_ERR_ARG, "bad band sharding parameters");
    if (o->spp < 1) return set_error(RT_ERR_ARG, "spp must be >= 1");
    if (cam->pixel_width < 1 || cam->pixel_height < 1) return set_error(RT_ERR_ARG, "camera has no pixels");
    DeviceGuard g(s->device);
    const size_t npx = size_t(rows) * size_t(cam->pixel_width);
    DevBuf rgb, cnt;
    int rc;
    if ((rc = rgb.alloc(std::max<size_t>(npx * 3 * sizeof(float), 4))) != RT_OK) return rc;
    if ((rc = cnt.alloc(4 * sizeof(unsigned long long))) != RT_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(cnt.p, 0, 4 * sizeof(unsigned long long)));
    HIP_TRY(hipDeviceSynchronize());
    rt_render_opts lo = *o;
    lo.kernel = RT_KERNEL_LANE;  // deep trees take the DEEP kernels, which count too
    t_ray_count = static_cast<unsigned long long*>(cnt.p);
    rc = rt_render_device(s, cam, &lo, static_cast<float*>(rgb.p), nullptr, nullptr, nullptr);
    t_ray_count = nullptr;
    if (rc != RT_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long h[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpy(h, cnt.p, sizeof(h), hipMemcpyDeviceToHost));
    counts[0] = o->max_depth > 0 ? uint64_t(npx) * uint64_t(o->spp) : 0;
    counts[1] = h[1];
    counts[2] = h[2];
    counts[3] = h[3];
    return RT_OK;
}

extern "C" int rt_render_reference(size_t P, int W, int H, const rt_camera* cam, rt_vec3 miss, int max_depth,
                                   int spp, const rt_bvh_node* nodes, const rt_aabb* aabbs,
                                   const rt_triangle* tris, const int32_t* objids, const rt_material* mats,
                                   int nmat, const rt_light* lights, int nlights, int diffuse_bounce,
                                   rt_vec3* output) {
    // query.cu:131-133: a null scene/output array is a silent no-op in the reference CPU
    // branch; here it is reported.
    if (!cam || !output) return set_error(RT_ERR_ARG, "rt_render_reference: null argument");
    if (W != cam->pixel_width || H != cam->pixel_height)
        return set_error(RT_ERR_ARG, "W/H must match the camera's pixel dimensions");
    rt_scene* s = nullptr;
    int rc = rt_scene_create(0, P, nodes, aabbs, tris, objids, mats, nmat, lights, nlights, &s);
    if (rc != RT_OK) return rc;
    rt_render_opts o;
    rt_render_opts_default(&o);
    o.max_depth = max_depth;
    o.spp = spp;
    o.diffuse_bounce = diffuse_bounce;
    o.miss_color = miss;
    rc = rt_render(s, cam, &o, reinterpret_cast<float*>(output), nullptr, nullptr);
    rt_scene_destroy(s);
    return rc;
}

// The HW1 path (rt_render_hw1*, rt_hw1_scene) is rt_hw1.hip.

extern "C" int rt_intersect_rays(int device, const rt_triangle* tri, const float origin[3], const float* dirs, int n,
                                 int hw1, float tmin, float tmax, int32_t* hit, float* t) {
    if (!tri || !origin || n < 0 || (n > 0 && (!dirs || !hit || !t))) return set_error(RT_ERR_ARG, "rt_intersect_rays: bad args");
    int rc = check_device(device);
    if (rc != RT_OK) return rc;
    if (n == 0) return RT_OK;
    DeviceGuard g(device);
    DevBuf dd, dh, dt;
    if ((rc = dd.upload(dirs, size_t(n) * 3 * sizeof(float))) != RT_OK) return rc;
    if ((rc = dh.alloc(size_t(n) * sizeof(int32_t))) != RT_OK) return rc;
    if ((rc = dt.alloc(size_t(n) * sizeof(float))) != RT_OK) return rc;
    const f3 v0{tri->v0.x, tri->v0.y, tri->v0.z};
    const f3 e1{tri->v1.x - tri->v0.x, tri->v1.y - tri->v0.y, tri->v1.z - tri->v0.z};
    const f3 e2{tri->v2.x - tri->v0.x, tri->v2.y - tri->v0.y, tri->v2.z - tri->v0.z};
    hipLaunchKernelGGL(intersect_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, nullptr, v0, e1, e2,
                       f3{origin[0], origin[1], origin[2]}, static_cast<const float*>(dd.p), n, hw1 ? 1 : 0, tmin,
                       tmax, static_cast<int32_t*>(dh.p), static_cast<float*>(dt.p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(hit, dh.p, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(t, dt.p, size_t(n) * sizeof(float), hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" float rt_powf_host(float x, float y) { return ref_powf(x, y); }

extern "C" int rt_powf_batch(int device, const float* x, const float* y, int n, float* out) {
    if (n < 0 || (n > 0 && (!x || !y || !out))) return set_error(RT_ERR_ARG, "rt_powf_batch: bad args");
    int rc = check_device(device);
    if (rc != RT_OK) return rc;
    if (n == 0) return RT_OK;
    DeviceGuard g(device);
    DevBuf dx, dy, dout;
    if ((rc = dx.upload(x, size_t(n) * sizeof(float))) != RT_OK) return rc;
    if ((rc = dy.upload(y, size_t(n) * sizeof(float))) != RT_OK) return rc;
    if ((rc = dout.alloc(size_t(n) * sizeof(float))) != RT_OK) return rc;
    hipLaunchKernelGGL(powf_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, nullptr,
                       static_cast<const float*>(dx.p), static_cast<const float*>(dy.p), n, static_cast<float*>(dout.p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout.p, size_t(n) * sizeof(float), hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" int rt_box_test_batch(int device, const float* rays, const float* boxes, const float* tminmax,
                                 const float* bmax, const uint8_t* active, int n, int32_t* out) {
    if (n < 0 || (n > 0 && (!rays || !boxes || !tminmax || !out)))
        return set_error(RT_ERR_ARG, "rt_box_test_batch: bad args");
    int rc = check_device(device);
    if (rc != RT_OK) return rc;
    if (n == 0) return RT_OK;
    DeviceGuard g(device);
    DevBuf dr, db, dt, dm, da, dout;
    if ((rc = dr.upload(rays, size_t(n) * 6 * sizeof(float))) != RT_OK) return rc;
    if ((rc = db.upload(boxes, size_t(n) * 6 * sizeof(float))) != RT_OK) return rc;
    if ((rc = dt.upload(tminmax, size_t(n) * 2 * sizeof(float))) != RT_OK) return rc;
    if (bmax && (rc = dm.upload(bmax, size_t(n) * 3 * sizeof(float))) != RT_OK) return rc;
    if (active && (rc = da.upload(active, size_t(n))) != RT_OK) return rc;
    if ((rc = dout.alloc(size_t(n) * 5 * sizeof(int32_t))) != RT_OK) return rc;
    hipLaunchKernelGGL(box_test_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, nullptr,
                       static_cast<const float*>(dr.p), static_cast<const float*>(db.p), static_cast<const float*>(dt.p),
                       bmax ? static_cast<const float*>(dm.p) : nullptr,
                       active ? static_cast<const uint8_t*>(da.p) : nullptr, n, static_cast<int32_t*>(dout.p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout.p, size_t(n) * 5 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" int rt_box_test_host(const float* rays, const float* boxes, const float* tminmax, int n,
                                int32_t* out_fast, int32_t* out_exact, int32_t* out_class) {
    if (n < 0 || (n > 0 && (!rays || !boxes || !tminmax || !out_fast || !out_exact || !out_class)))
        return set_error(RT_ERR_ARG, "rt_box_test_host: bad args");
    for (int i = 0; i < n; ++i) {
        const float* R = rays + 6 * i;
        const float* B = boxes + 6 * i;
        f3 bm = mk(fmaxf(fabsf(B[0]), fabsf(B[3])), fmaxf(fabsf(B[1]), fabsf(B[4])), fmaxf(fabsf(B[2]), fabsf(B[5])));
        if (!(B[0] <= B[3] && B[1] <= B[4] && B[2] <= B[5])) bm = mk(INFINITY, INFINITY, INFINITY);  // as rt_scene_create
        const RayPre r = make_ray(mk(R[0], R[1], R[2]), mk(R[3], R[4], R[5]), bm, tminmax[2 * i]);
        const BoxP b = {(v2f){B[0], B[3]}, (v2f){B[1], B[4]}, (v2f){B[2], B[5]}};
        out_class[i] = box_classify(r, b, tminmax[2 * i + 1]);
        out_fast[i] = box_hit(r, b, tminmax[2 * i], tminmax[2 * i + 1]) ? 1 : 0;
        out_exact[i] = box_hit_exact(r, b, (double)tminmax[2 * i], (double)tminmax[2 * i + 1]) ? 1 : 0;
    }
    return RT_OK;
}

extern "C" int rt_debug_tile_test_host(const rt_camera* cam, const int32_t* tiles, const float* boxes, int n,
                                       int32_t* out) {
    if (!cam || n < 0 || (n > 0 && (!tiles || !boxes || !out))) return set_error(RT_ERR_ARG, "rt_debug_tile_test_host: bad args");
    RenderParams P;
    std::memset(&P, 0, sizeof(P));
    tile_test_camera(P, *cam);
    // as in a frame: the tile test runs only for a camera whose |D| range is proven (camera_class)
    const bool proven = camera_class(cam, 1.0) == RT_CAMERA_PROVEN;
    for (int i = 0; i < n; ++i) {
        const int32_t* t = tiles + 4 * size_t(i);
        out[i] = proven && tile_misses_box_f(tile_dirs_f(P, t[0], t[1], t[2], t[3]), boxes + 6 * size_t(i)) ? 1 : 0;
    }
    return RT_OK;
}

extern "C" int rt_debug_camera_class(const rt_camera* cam, float pad, int32_t* out) {
    if (!cam || !out) return set_error(RT_ERR_ARG, "rt_debug_camera_class: null argument");
    *out = camera_class(cam, double(pad));
    return RT_OK;
}

extern "C" int rt_debug_tile_test_batch(int device, const rt_camera* cam, const int32_t* tiles, const float* boxes,
                                        int n, int32_t* out) {
    if (!cam || n < 0 || (n > 0 && (!tiles || !boxes || !out))) return set_error(RT_ERR_ARG, "rt_debug_tile_test_batch: bad args");
    int rc = check_device(device);
    if (rc != RT_OK) return rc;
    if (n == 0) return RT_OK;
    if (camera_class(cam, 1.0) != RT_CAMERA_PROVEN) {  // as in a frame: no tile test, nothing culled
        std::fill(out, out + n, 0);
        return RT_OK;
    }
    DeviceGuard g(device);
    DevBuf dt, db, dout;
    if ((rc = dt.upload(tiles, size_t(n) * 4 * sizeof(int32_t))) != RT_OK) return rc;
    if ((rc = db.upload(boxes, size_t(n) * 6 * sizeof(float))) != RT_OK) return rc;
    if ((rc = dout.alloc(size_t(n) * sizeof(int32_t))) != RT_OK) return rc;
    RenderParams P;
    std::memset(&P, 0, sizeof(P));
    tile_test_camera(P, *cam);
    hipLaunchKernelGGL(tile_test_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, nullptr, P,
                       static_cast<const int32_t*>(dt.p), static_cast<const float*>(db.p), n, static_cast<int32_t*>(dout.p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout.p, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" int rt_debug_family_test_host(const float* rays, const uint8_t* active, const float* best_t,
                                         const float* bmax, const float* boxes, int n_waves, int32_t* out,
                                         int32_t* out_loose) {
    if (n_waves < 0 || (n_waves > 0 && (!rays || !best_t || !bmax || !boxes || !out || !out_loose)))
        return set_error(RT_ERR_ARG, "rt_debug_family_test_host: bad args");
    for (int w = 0; w < n_waves; ++w) {
        const float* R = rays + 6 * 64 * size_t(w);
        const float o[3] = {R[0], R[1], R[2]};  // the shared origin: lane 0's
        // family_dirs and frustum_loop's tmax_w, the wave reductions as plain loops
        v2f U[3];
        bool loose = false;
        for (int a = 0; a < 3; ++a) {
            float dl = INFINITY, dh = -INFINITY;
            for (int l = 0; l < 64; ++l) {
                if (active && !active[64 * size_t(w) + l]) continue;
                dl = fminf(dl, R[6 * l + 3 + a]);
                dh = fmaxf(dh, R[6 * l + 3 + a]);
            }
            float u0, u1;
            const bool lz = family_axis(dl, dh, bmax[3 * size_t(w) + a] + fabsf(o[a]) < 1e30f, u0, u1);
            loose = loose || lz;
            U[a] = (v2f){u0, u1};
        }
        float tmax_w = 0.0f;
        for (int l = 0; l < 64; ++l)
            if (!active || active[64 * size_t(w) + l]) tmax_w = fmaxf(tmax_w, best_t[64 * size_t(w) + l]);
        out_loose[w] = loose ? 1 : 0;
        for (int k = 0; k < 32; ++k) {
            const float* B = boxes + 6 * (32 * size_t(w) + k);
            const v2f bb[3] = {(v2f){B[0], B[3]}, (v2f){B[1], B[4]}, (v2f){B[2], B[5]}};
            const bool pass = loose ? family_entry_passes<true>(bb, o, U, tmax_w) : family_entry_passes<false>(bb, o, U, tmax_w);
            out[32 * size_t(w) + k] = pass ? 1 : 0;
        }
    }
    return RT_OK;
}

extern "C" int rt_debug_family_test_batch(int device, const float* rays, const uint8_t* active, const float* best_t,
                                          const float* bmax, const float* boxes, int n_waves, int32_t* out,
                                          int32_t* out_loose) {
    if (n_waves < 0 || n_waves > (1 << 24) || (n_waves > 0 && (!rays || !best_t || !bmax || !boxes || !out || !out_loose)))
        return set_error(RT_ERR_ARG, "rt_debug_family_test_batch: bad args");
    int rc = check_device(device);
    if (rc != RT_OK) return rc;
    if (n_waves == 0) return RT_OK;
    DeviceGuard g(device);
    const size_t n = size_t(n_waves);
    DevBuf dr, da, dt, dm, db, dout, dl;
    if ((rc = dr.upload(rays, n * 64 * 6 * sizeof(float))) != RT_OK) return rc;
    if (active && (rc = da.upload(active, n * 64)) != RT_OK) return rc;
    if ((rc = dt.upload(best_t, n * 64 * sizeof(float))) != RT_OK) return rc;
    if ((rc = dm.upload(bmax, n * 3 * sizeof(float))) != RT_OK) return rc;
    if ((rc = db.upload(boxes, n * 32 * 6 * sizeof(float))) != RT_OK) return rc;
    if ((rc = dout.alloc(n * 32 * sizeof(int32_t))) != RT_OK) return rc;
    if ((rc = dl.alloc(n * sizeof(int32_t))) != RT_OK) return rc;
    constexpr int kWaves = BLOCK / 64;
    hipLaunchKernelGGL(family_test_kernel, dim3((n_waves + kWaves - 1) / kWaves), dim3(BLOCK), 0, nullptr,
                       static_cast<const float*>(dr.p), active ? static_cast<const uint8_t*>(da.p) : nullptr,
                       static_cast<const float*>(dt.p), static_cast<const float*>(dm.p), static_cast<const float*>(db.p),
                       n_waves, static_cast<int32_t*>(dout.p), static_cast<int32_t*>(dl.p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout.p, n * 32 * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_loose, dl.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}
