// rt_path.hpp — path stages for caller hits (rt_path_*, include/rt_mi355x.h): the body of
// TraceRayIterative's depth loop (G/include/query.h:178-217) as a stage of its own, over caller
// rays and hit records with an optional material per hit, and what runs a path in stages around
// it: the state's start (query.h:166-170), a stable compaction of the live rays, and the final
// clamp (shader.h:24-32).  trace_hits -> path_step -> compact -> trace_hits -> ... with nothing
// edited is shade_rays_kernel's path bit for bit.  DESIGN.md §4.21.
// Part of rt_device.hip's translation unit, included inside its anonymous namespace after rt_query.hpp.
#pragma once

constexpr uint32_t PATH_NONE = 0xFFFFFFFFu;  // RT_PATH_NONE: an entry that carries no path

// One entry of the step, for the kernel and for rt_path_step_host alike: everything it reads and
// writes is plain memory (R the ray's 6 floats, H the record's four 16-byte words, the path's
// state words), and the one thing the two builds do differently, IsInShadow's traversal
// (shader.h:44-62), is `occluded(light, origin, direction, dist)`.  The arithmetic and its order
// are shade_rays_kernel's, which is the reference's:
//   a miss (tri < 0)  radiance += throughput * miss                         (query.h:181-183)
//   ShadeDirect       N = unit(rec.normal), V = unit(ray.origin - rec.p), ambient + emission, then
//                     per light the NdotL > 0 test, the shadow ray from p + N eps bounded by the
//                     light's distance, EvaluateBRDF on the normal as stored  (shader.h:65-110)
//   the bounce        kd + kr <= 0 ends the path; xi = rng_next; the diffuse or the mirror ray and
//                     throughput; the 1e-4 cut-off                           (query.h:193-216)
// The material is mat_k (the caller's, 13 floats read through a 4-byte aligned pointer) or
// assignMaterialToHit's choice from the record's `material` word (query.h:134-153): the table's
// entry, or Material()'s defaults outside it.  It is re-read where it is used, as in
// shade_rays_kernel, so that none of it is live across a shadow traversal.
// last: no bounce and no draw.  next (6 floats, may be R itself), alive and direct (3 floats) may
// be null.  A dead entry's next ray is its input ray.
template <class OccFn>
__host__ __device__ __forceinline__ void path_step_one(const float* R, const uint4* H, const float* mat_k,
                                                       const DevMaterial* table, int num_table, const DevLight* lights,
                                                       int num_lights, f3 miss, bool diffuse_bounce, bool last,
                                                       float* radiance, float* throughput, uint32_t* rng_state, float* next,
                                                       uint8_t* alive, float* direct, OccFn occluded) {
    const f3 ro = mk(R[0], R[1], R[2]), rd = mk(R[3], R[4], R[5]);
    const uint4 w0 = H[0], w1 = H[1], w2 = H[2], w3 = H[3];
    f3 no = ro, nd = rd;
    f3 Lo = mk(0.f, 0.f, 0.f);
    bool live = false;
    if ((int32_t)w0.x < 0) {
        const f3 rad = mk(radiance[0], radiance[1], radiance[2]);
        const f3 thr = mk(throughput[0], throughput[1], throughput[2]);
        const f3 r = add(rad, mul(thr, miss));
        radiance[0] = r.x;
        radiance[1] = r.y;
        radiance[2] = r.z;
    } else {
        const f3 p = mk(pw::asf(w1.x), pw::asf(w1.y), pw::asf(w1.z));
        const f3 n = mk(pw::asf(w1.w), pw::asf(w2.x), pw::asf(w2.y));
        const int32_t mi = (int32_t)w3.w;
        const DevMaterial* M = reinterpret_cast<const DevMaterial*>(mat_k);
        if (M == nullptr && table != nullptr && mi >= 0 && mi < num_table) M = table + mi;
        auto material = [&]() {
            DevMaterial m = {{0.8f, 0.8f, 0.8f}, 1.0f, {0.04f, 0.04f, 0.04f}, 0.0f, 32.0f, 0.0f, {0.f, 0.f, 0.f}};
            if (M != nullptr) m = *M;
            return m;
        };
        // ShadeDirect (shader.h:65-110)
        const f3 N = unit(n);
        const f3 V = unit(sub(ro, p));
        {
            const DevMaterial m = material();
            Lo = add(Lo, scale(mk(m.albedo[0], m.albedo[1], m.albedo[2]), 0.05f));
            Lo = add(Lo, mk(m.emission[0], m.emission[1], m.emission[2]));
        }
        for (int li = 0; li < num_lights; ++li) {
            const DevLight& lt = lights[li];
            const f3 lpos = mk(lt.pos[0], lt.pos[1], lt.pos[2]);
            const f3 L = unit(sub(lpos, p));
            const float NdotL = fmaxf(dot(N, L), 0.0f);
            if (NdotL <= 0.0f) continue;
            // IsInShadow (shader.h:44-62)
            const f3 toL = sub(lpos, p);
            const float dist = sqrtf(dot(toL, toL));
            if (dist > 0.0f) {
                if (occluded(li, add(p, scale(N, RT_EPS)), divf(toL, dist), dist)) continue;
            }
            const DevMaterial m = material();
            const f3 f = eval_brdf(m, n, V, L);
            const f3 rad = scale(mk(lt.color[0], lt.color[1], lt.color[2]), (float)lt.intensity);
            Lo = add(Lo, scale(mul(rad, f), NdotL));
        }
        f3 thr = mk(throughput[0], throughput[1], throughput[2]);
        {
            const f3 rad = mk(radiance[0], radiance[1], radiance[2]);
            const f3 r = add(rad, mul(thr, Lo));
            radiance[0] = r.x;
            radiance[1] = r.y;
            radiance[2] = r.z;
        }
        if (!last) {
            // bounce (query.h:193-216)
            const DevMaterial m = material();
            const float kd = m.kd, kr = m.kr, total = kd + kr;
            if (total > 0.0f) {
                uint32_t rng = *rng_state;
                const float xi = rng_next(rng);
                if (diffuse_bounce && xi < kd / total) {
                    f3 dd = random_unit_vector(rng);
                    if (!(dot(dd, N) > 0.0f)) dd = mk(-dd.x, -dd.y, -dd.z);
                    const float nl = fmaxf(dot(N, dd), 0.0f);
                    nd = dd;
                    thr = mul(thr, scale(mk(m.albedo[0], m.albedo[1], m.albedo[2]), 2.0f * nl));
                } else {
                    const f3 I = unit(rd);
                    nd = sub(I, scale(N, 2.0f * dot(I, N)));
                    thr = mul(thr, scale(mk(m.spec[0], m.spec[1], m.spec[2]), kr));
                }
                no = add(p, scale(N, RT_EPS));
                *rng_state = rng;
                throughput[0] = thr.x;
                throughput[1] = thr.y;
                throughput[2] = thr.z;
                live = !(thr.x < 1e-4f && thr.y < 1e-4f && thr.z < 1e-4f);
                if (!live) {  // the reference leaves its loop: the new ray is never traced
                    no = ro;
                    nd = rd;
                }
            }
        }
    }
    if (next != nullptr) {
        next[0] = no.x;
        next[1] = no.y;
        next[2] = no.z;
        next[3] = nd.x;
        next[4] = nd.y;
        next[5] = nd.z;
    }
    if (alive != nullptr) *alive = live ? 1 : 0;
    if (direct != nullptr) {
        direct[0] = Lo.x;
        direct[1] = Lo.y;
        direct[2] = Lo.z;
    }
}

struct PathStepParams {
    SceneView sc;
    const float* rays;                  // m x rt_ray (next may be the same array: no __restrict__)
    const uint4* __restrict__ hits;     // m x rt_hit, 16-byte aligned
    const float* __restrict__ mats;     // m x rt_material, or null
    const uint32_t* __restrict__ ids;   // m path ids, or null: k
    uint32_t m;
    int32_t diffuse_bounce, last;
    f3 miss;
    float* __restrict__ radiance;       // the state, by path id
    float* __restrict__ throughput;
    uint32_t* __restrict__ rng;
    float* next;                        // m x rt_ray, or null (last)
    uint8_t* __restrict__ alive;        // m, or null (last)
    float* __restrict__ direct;         // 3m, or null
};

// One entry per lane.  Nothing is wave-wide, so a lane takes the reference's own control flow and
// leaves when its entry is done; its shadow rays are any-hit queries bounded by the light's
// distance, one after another on the lane's LDS stack (DEEP: the private stack), as in
// shade_rays_kernel.  Ids are unique, so each state word has one writer: plain stores.
template <int VARIANT>
__global__ __launch_bounds__(BLOCK) void path_step_kernel(PathStepParams P) {
    constexpr bool LDS = VARIANT != RT_RAYS_VARIANT_DEEP;
    __shared__ uint32_t stk_all[LDS ? LANE_LDS_CAP * BLOCK : 1];
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;  // m < 2^31
    if (k >= P.m) return;
    uint32_t* stk = stk_all + (LDS ? threadIdx.x : 0);
    const SceneView& sc = P.sc;
    const float* R = P.rays + 6 * (size_t)k;
    float* next = P.next != nullptr ? P.next + 6 * (size_t)k : nullptr;
    uint8_t* alive = P.alive != nullptr ? P.alive + k : nullptr;
    float* direct = P.direct != nullptr ? P.direct + 3 * (size_t)k : nullptr;
    const uint32_t id = P.ids != nullptr ? P.ids[k] : k;
    if (id == PATH_NONE) {  // no path: the ray passes through, no state word is touched
        const float r0 = R[0], r1 = R[1], r2 = R[2], r3 = R[3], r4 = R[4], r5 = R[5];
        if (next != nullptr) {
            next[0] = r0;
            next[1] = r1;
            next[2] = r2;
            next[3] = r3;
            next[4] = r4;
            next[5] = r5;
        }
        if (alive != nullptr) *alive = 0;
        if (direct != nullptr) direct[0] = direct[1] = direct[2] = 0.0f;
        return;
    }
    path_step_one(R, P.hits + 4 * (size_t)k, P.mats != nullptr ? P.mats + 13 * (size_t)k : nullptr, sc.mats, sc.num_mats,
                  sc.lights, sc.num_lights, P.miss, P.diffuse_bounce != 0, P.last != 0, P.radiance + 3 * (size_t)id,
                  P.throughput + 3 * (size_t)id, P.rng + id, next, alive, direct,
                  [&](int, f3 o, f3 d, float dist) {
                      const RayPre sray = make_ray(o, d, scene_bmax(sc));
                      HitState shs;
                      shade_traverse<VARIANT>(sc, sray, true, dist, shs, stk);
                      return shs.slot >= 0 && shs.bestT < dist;
                  });
}

// The state at the top of TraceRayIterative (query.h:166-170).
struct PathBeginParams {
    const uint32_t* __restrict__ seeds;  // n, or null: 42u
    uint32_t n;
    float* __restrict__ radiance;
    float* __restrict__ throughput;
    uint32_t* __restrict__ rng;
};
__global__ __launch_bounds__(BLOCK) void path_begin_kernel(PathBeginParams P) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.n) return;
    float* r = P.radiance + 3 * (size_t)i;
    float* t = P.throughput + 3 * (size_t)i;
    r[0] = r[1] = r[2] = 0.0f;
    t[0] = t[1] = t[2] = 1.0f;
    P.rng[i] = P.seeds != nullptr ? P.seeds[i] : 42u;
}

// The reference's clamp (shader.h:24-32) on every path's radiance: NaN and -0.0 stay as they are.
__global__ __launch_bounds__(BLOCK) void path_finish_kernel(float* __restrict__ radiance, uint32_t n) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    float* r = radiance + 3 * (size_t)i;
    const f3 c = clamp01(mk(r[0], r[1], r[2]));
    r[0] = c.x;
    r[1] = c.y;
    r[2] = c.z;
}

// ---- stable compaction of the live rays ----------------------------------------------------------
// Three kinds of launch in stream order, no block waits for another: (1) each block counts the
// flags of its PATH_TILE entries; (2) the counts become exclusive offsets by a scan that recurses
// through per-tile sums while more than one tile is left (one launch up to PATH_TILE^2 = 4 Mi
// entries); (3) each block scatters its live entries from its offset on.  Within a block entry
// base + j * BLOCK + t belongs to thread t in round j (coalesced), and its rank is the live
// entries of the rounds and waves before it plus the live lanes below it in its wave's ballot:
// increasing k, so the order is stable.
// (the tile constants and the scan of the counts: rt_scan.hpp, shared with the adaptive film)
#include "rt_scan.hpp"

__global__ __launch_bounds__(BLOCK) void path_count_kernel(const uint8_t* __restrict__ alive, uint32_t m,
                                                           uint32_t* __restrict__ counts) {
    __shared__ uint32_t part[PATH_WAVES];
    const uint64_t base = (uint64_t)blockIdx.x * PATH_TILE;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < PATH_ROUNDS; ++j) {
        const uint64_t k = base + (uint32_t)j * BLOCK + threadIdx.x;
        const bool f = k < m && alive[k] != 0;
        c += (uint32_t)__popcll(ballot(f));  // wave-uniform
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < PATH_WAVES; ++w) s += part[w];
        counts[blockIdx.x] = s;
    }
}

struct PathScatterParams {
    const uint8_t* __restrict__ alive;
    uint32_t m;
    const uint32_t* __restrict__ offsets;  // per tile: live entries before it
    const float* __restrict__ rays_in;
    const uint32_t* __restrict__ ids_in;   // or null: k
    float* __restrict__ rays_out;
    uint32_t* __restrict__ ids_out;
};
__global__ __launch_bounds__(BLOCK) void path_scatter_kernel(PathScatterParams P) {
    __shared__ uint32_t cnt[PATH_ROUNDS * PATH_WAVES];
    const uint64_t base = (uint64_t)blockIdx.x * PATH_TILE;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t below[PATH_ROUNDS];
    bool flag[PATH_ROUNDS];
#pragma unroll
    for (int j = 0; j < PATH_ROUNDS; ++j) {
        const uint64_t k = base + (uint32_t)j * BLOCK + threadIdx.x;
        flag[j] = k < P.m && P.alive[k] != 0;
        const uint64_t mask = ballot(flag[j]);
        below[j] = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) cnt[j * PATH_WAVES + wave] = (uint32_t)__popcll(mask);
    }
    __syncthreads();
    const uint32_t off = P.offsets[blockIdx.x];
#pragma unroll
    for (int j = 0; j < PATH_ROUNDS; ++j) {
        if (!flag[j]) continue;
        uint32_t before = 0;
        for (int q = 0; q < j * PATH_WAVES + (int)wave; ++q) before += cnt[q];
        const uint64_t k = base + (uint32_t)j * BLOCK + threadIdx.x;
        const size_t o = (size_t)off + before + below[j];  // < the number of live entries <= m
        const float* s = P.rays_in + 6 * (size_t)k;
        float* d = P.rays_out + 6 * o;
        d[0] = s[0];
        d[1] = s[1];
        d[2] = s[2];
        d[3] = s[3];
        d[4] = s[4];
        d[5] = s[5];
        P.ids_out[o] = P.ids_in != nullptr ? P.ids_in[k] : (uint32_t)k;
    }
}
