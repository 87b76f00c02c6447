// rt_query.hpp — batched ray queries on a resident scene (rt_trace_rays*, include/rt_mi355x.h):
// closest hit = SearchBVH (G/include/query.h:224-311) for caller rays, occlusion = the decision
// of IsInShadow (G/include/shader.h:59-61).  One ray per lane over the per-lane traversals of
// rt_traverse.hpp; DESIGN.md §4.17.  Below them the radiance queries (rt_shade_rays*):
// TraceRayIterative (G/include/query.h:156-220) for caller rays, one path per lane; §4.18.
// Then the hit records (rt_trace_hits*): the closest hit as the reference's whole HitRecord, and
// the camera rays that feed any of the three (rt_camera_rays*); §4.19.
// Part of rt_device.hip's translation unit, included inside its anonymous namespace after rt_shade.hpp.
#pragma once

struct QueryParams {
    SceneView sc;
    const float* __restrict__ rays;   // n x rt_ray: origin, direction (6 floats)
    const float* __restrict__ max_t;  // ANY: n distances
    uint32_t n;
    int32_t* __restrict__ hit_idx;
    float* __restrict__ hit_t;  // closest hit only; may be null
};

// Caller rays have no common origin and no common direction, so each lane runs the reference's
// DFS on its own (the wave's time is its longest lane's path, not the union of 64 paths):
//   WIDE    traverse_lane_lds_wide, the 4-ary records, stack in LDS (stride BLOCK)
//   BINARY  traverse_lane_lds, the binary records, stack in LDS
//   DEEP    traverse_deep, SearchBVH as written: 512-entry private stack, overflow rule and
//           brute-force completion; exact for any tree
// ANY: the lane may stop at the first accepted triangle with t < max_t (bestT only decreases
// afterwards, so `hit && t < max_t` is decided); the closest t is then unknown, so only the
// decision is written.  A lane past the batch leaves at once: the per-lane traversals use no
// wave-wide operation.
template <int VARIANT, bool ANY>
__global__ __launch_bounds__(BLOCK) void trace_rays_kernel(QueryParams Q) {
    constexpr bool LDS = VARIANT != RT_RAYS_VARIANT_DEEP;
    __shared__ uint32_t stk[LDS ? LANE_LDS_CAP * BLOCK : 1];
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;  // n < 2^31: the grid's last index fits
    if (i >= Q.n) return;
    const float* R = Q.rays + 6 * (size_t)i;
    const RayPre r = make_ray(mk(R[0], R[1], R[2]), mk(R[3], R[4], R[5]), scene_bmax(Q.sc));
    float dist = 0.0f;
    if constexpr (ANY) dist = Q.max_t[i];
    HitState hs;
    if constexpr (VARIANT == RT_RAYS_VARIANT_WIDE) traverse_lane_lds_wide(Q.sc, r, true, ANY, dist, hs, stk + threadIdx.x);
    else if constexpr (VARIANT == RT_RAYS_VARIANT_BINARY) traverse_lane_lds(Q.sc, r, true, ANY, dist, hs, stk + threadIdx.x);
    else traverse_deep(Q.sc, r, true, ANY, dist, hs);
    const bool hit = hs.slot >= 0;
    if constexpr (ANY) {
        Q.hit_idx[i] = hit && hs.bestT < dist ? 1 : 0;  // IsInShadow: hit && t < dist (a NaN dist: 0)
    } else {
        Q.hit_idx[i] = hit ? leaf_tri<!LDS>(Q.sc, hs.slot) : -1;
        if (Q.hit_t != nullptr) Q.hit_t[i] = hit ? hs.bestT : -1.0f;
    }
}

// ---- radiance queries (rt_shade_rays*): TraceRayIterative for caller rays, DESIGN.md §4.18 ----
struct ShadeParams {
    SceneView sc;
    const float* __restrict__ rays;     // n x rt_ray
    const uint32_t* __restrict__ seeds;  // n rng states, or null: 42u each (query.h:169)
    uint32_t n;
    int32_t max_depth, diffuse_bounce;
    f3 miss;
    float* __restrict__ radiance;  // 3n
    int32_t* __restrict__ hit_idx;  // the first segment's SearchBVH result; may be null
    float* __restrict__ hit_t;      // may be null
};

// The variant's per-lane traversal (the three of trace_rays_kernel).
template <int VARIANT>
__device__ __forceinline__ void shade_traverse(const SceneView& sc, const RayPre& r, bool any_hit, float any_hit_dist,
                                               HitState& hs, uint32_t* stk) {
    if constexpr (VARIANT == RT_RAYS_VARIANT_WIDE) traverse_lane_lds_wide(sc, r, true, any_hit, any_hit_dist, hs, stk);
    else if constexpr (VARIANT == RT_RAYS_VARIANT_BINARY) traverse_lane_lds(sc, r, true, any_hit, any_hit_dist, hs, stk);
    else traverse_deep(sc, r, true, any_hit, any_hit_dist, hs);
}

// One path per lane: TraceRayIterative (query.h:156-220) as written, with ShadeDirect
// (shader.h:65-110) and IsInShadow (shader.h:44-62) inside its depth loop.  The shading copies
// of rt_shade.hpp keep a wave together (every lane enters every traversal, masked); here nothing
// is wave-wide, so a lane takes the reference's own control flow: `continue` past a light that
// faces away, `break` on a miss, on kd + kr <= 0 and on a spent throughput, and it leaves when
// its path ends.  The lane's LDS stack serves its traversals one after another (each starts
// empty): the path segment of a depth, then one shadow ray per light.  A shadow ray is an
// any-hit query bounded by the light's distance (IsInShadow reads only `hit && t < dist`).
// The bounce of the last depth has no effect (its ray is never traced, its draws are never
// read) and is skipped, as in trace_sample.
template <int VARIANT>
__global__ __launch_bounds__(BLOCK) void shade_rays_kernel(ShadeParams S) {
    constexpr bool LDS = VARIANT != RT_RAYS_VARIANT_DEEP;
    __shared__ uint32_t stk_all[LDS ? LANE_LDS_CAP * BLOCK : 1];
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;  // n < 2^31
    if (i >= S.n) return;
    uint32_t* stk = stk_all + (LDS ? threadIdx.x : 0);
    const SceneView& sc = S.sc;
    const float* R = S.rays + 6 * (size_t)i;
    RayPre ray = make_ray(mk(R[0], R[1], R[2]), mk(R[3], R[4], R[5]), scene_bmax(sc));  // the direction as given
    uint32_t rng = S.seeds != nullptr ? S.seeds[i] : 42u;
    f3 radiance = mk(0.f, 0.f, 0.f);
    f3 thr = mk(1.f, 1.f, 1.f);
    const int max_depth = S.max_depth;
    if (max_depth <= 0) {  // query.h:172: no ray is traced
        if (S.hit_idx != nullptr) S.hit_idx[i] = -1;
        if (S.hit_t != nullptr) S.hit_t[i] = -1.0f;
    }
    for (int depth = 0; depth < max_depth; ++depth) {
        HitState hs;
        shade_traverse<VARIANT>(sc, ray, false, 0.0f, hs, stk);
        const bool hit = hs.slot >= 0;
        if (depth == 0) {  // written at once: nothing of it stays live across the shading
            if (S.hit_idx != nullptr) S.hit_idx[i] = hit ? leaf_tri<!LDS>(sc, hs.slot) : -1;
            if (S.hit_t != nullptr) S.hit_t[i] = hit ? hs.bestT : -1.0f;
        }
        if (!hit) {
            radiance = add(radiance, mul(thr, S.miss));
            break;
        }
        const SurfHit sh = resolve_hit<!LDS>(sc, ray, hs.slot);
        // ShadeDirect (shader.h:65-110)
        const f3 N = unit(sh.n);
        const f3 V = unit(sub(ray.o, sh.p));
        f3 Lo = mk(0.f, 0.f, 0.f);
        {
            const DevMaterial m = material_of(sc, sh.tri);
            Lo = add(Lo, scale(mk(m.albedo[0], m.albedo[1], m.albedo[2]), 0.05f));
            Lo = add(Lo, mk(m.emission[0], m.emission[1], m.emission[2]));
        }
        for (int li = 0; li < sc.num_lights; ++li) {
            const DevLight& lt = sc.lights[li];
            const f3 lpos = mk(lt.pos[0], lt.pos[1], lt.pos[2]);
            const f3 L = unit(sub(lpos, sh.p));
            const float NdotL = fmaxf(dot(N, L), 0.0f);
            if (NdotL <= 0.0f) continue;
            // IsInShadow (shader.h:44-62)
            const f3 toL = sub(lpos, sh.p);
            const float dist = sqrtf(dot(toL, toL));
            if (dist > 0.0f) {
                const RayPre sray = make_ray(add(sh.p, scale(N, RT_EPS)), divf(toL, dist), scene_bmax(sc));
                HitState shs;
                shade_traverse<VARIANT>(sc, sray, true, dist, shs, stk);
                if (shs.slot >= 0 && shs.bestT < dist) continue;
            }
            // the light's term, once its shadow ray is known to be clear
            const DevMaterial m = material_of(sc, sh.tri);
            const f3 f = eval_brdf(m, sh.n, V, L);
            const f3 rad = scale(mk(lt.color[0], lt.color[1], lt.color[2]), (float)lt.intensity);
            Lo = add(Lo, scale(mul(rad, f), NdotL));
        }
        radiance = add(radiance, mul(thr, Lo));
        if (depth + 1 >= max_depth) break;
        // bounce (query.h:193-216)
        const DevMaterial m = material_of(sc, sh.tri);
        const float kd = m.kd, kr = m.kr, total = kd + kr;
        if (total <= 0.0f) break;
        const float xi = rng_next(rng);
        if (S.diffuse_bounce && xi < kd / total) {
            f3 dd = random_unit_vector(rng);
            if (!(dot(dd, N) > 0.0f)) dd = mk(-dd.x, -dd.y, -dd.z);
            const float nl = fmaxf(dot(N, dd), 0.0f);
            ray = make_ray(add(sh.p, scale(N, RT_EPS)), dd, scene_bmax(sc));
            thr = mul(thr, scale(mk(m.albedo[0], m.albedo[1], m.albedo[2]), 2.0f * nl));
        } else {
            const f3 I = unit(ray.d);
            const f3 refl = sub(I, scale(N, 2.0f * dot(I, N)));
            ray = make_ray(add(sh.p, scale(N, RT_EPS)), refl, scene_bmax(sc));
            thr = mul(thr, scale(mk(m.spec[0], m.spec[1], m.spec[2]), kr));
        }
        if (thr.x < 1e-4f && thr.y < 1e-4f && thr.z < 1e-4f) break;
    }
    const f3 c = clamp01(radiance);
    S.radiance[3 * (size_t)i] = c.x;
    S.radiance[3 * (size_t)i + 1] = c.y;
    S.radiance[3 * (size_t)i + 2] = c.z;
}

// ---- hit records (rt_trace_hits*): SearchBVH's HitRecord for caller rays, DESIGN.md §4.19 ----
// rt_hit (include/rt_mi355x.h) as the four 16-byte words it is stored in.
struct HitWords {
    uint4 w[4];
};
// A miss: tri -1, t -1.0f, every other field zero.
__host__ __device__ __forceinline__ HitWords miss_record() {
    HitWords h;
    h.w[0] = make_uint4(0xFFFFFFFFu, pw::asu(-1.0f), 0u, 0u);
    h.w[1] = h.w[2] = h.w[3] = make_uint4(0u, 0u, 0u, 0u);
    return h;
}
// intersectTriangle's record (query.h:110-128) of a triangle the ray is known to hit at (t, u, v),
// with the ids assignMaterialToHit reads.
__host__ __device__ __forceinline__ HitWords hit_record(const RayPre& r, f3 e1, f3 e2, f3 n0, f3 n1, f3 n2, float t, float u,
                                                        float v, int32_t tri, int32_t object_id, int32_t material) {
    const HitFrame f = hit_frame_full(r, e1, e2, n0, n1, n2, t, u, v);
    HitWords h;
    h.w[0] = make_uint4((uint32_t)tri, pw::asu(t), pw::asu(u), pw::asu(v));
    h.w[1] = make_uint4(pw::asu(f.p.x), pw::asu(f.p.y), pw::asu(f.p.z), pw::asu(f.shadingN.x));
    h.w[2] = make_uint4(pw::asu(f.shadingN.y), pw::asu(f.shadingN.z), pw::asu(f.geomN.x), pw::asu(f.geomN.y));
    h.w[3] = make_uint4(pw::asu(f.geomN.z), f.front ? 1u : 0u, (uint32_t)object_id, (uint32_t)material);
    return h;
}

struct HitsParams {
    SceneView sc;
    const float* __restrict__ rays;  // n x rt_ray
    uint32_t n;
    uint4* __restrict__ hits;  // n x rt_hit, 16-byte aligned
};

// trace_rays_kernel's closest-hit traversal, then the winner's whole record in the same lane: the
// traversal leaves a slot of the packed leaf array (or, DEEP, BRUTE_BIT | triangle), and the
// record is rebuilt from that leaf and the ray as resolve_hit rebuilds it -- the accepting test's
// own t, u, v.  objids / mats: the range tests of material_of, which selects by them.  A lane
// stores its 64 bytes as four 16-byte words, so a wave writes 4 KiB contiguous.
template <int VARIANT>
__global__ __launch_bounds__(BLOCK) void trace_hits_kernel(HitsParams Q) {
    constexpr bool LDS = VARIANT != RT_RAYS_VARIANT_DEEP;
    constexpr bool DEEP = !LDS;
    __shared__ uint32_t stk[LDS ? LANE_LDS_CAP * BLOCK : 1];
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;  // n < 2^31
    if (i >= Q.n) return;
    const SceneView& sc = Q.sc;
    const float* R = Q.rays + 6 * (size_t)i;
    const RayPre r = make_ray(mk(R[0], R[1], R[2]), mk(R[3], R[4], R[5]), scene_bmax(sc));
    HitState hs;
    shade_traverse<VARIANT>(sc, r, false, 0.0f, hs, stk + (LDS ? threadIdx.x : 0));
    HitWords h = miss_record();
    if (hs.slot >= 0) {
        const int32_t slot = hs.slot;
        const float4* L = sc.leaf + 4 * (size_t)slot;
        bool brute = false;
        if constexpr (DEEP) {
            brute = ((uint32_t)slot & BRUTE_BIT) != 0;
            if (brute) L = sc.tri + 3 * (size_t)((uint32_t)slot & ~BRUTE_BIT);
        }
        const float4 a = L[0], b = L[1], c = L[2];
        const f3 v0 = mk(a.x, a.y, a.z), e1 = mk(b.x, b.y, b.z), e2 = mk(b.w, c.x, c.y);
        float t = 0.f, u = 0.f, v = 0.f;
        mt_g(r, v0, e1, e2, -FLT_MAX, FLT_MAX, t, u, v);  // same t/u/v as the accepting test
        const int32_t tri = brute ? (int32_t)((uint32_t)slot & ~BRUTE_BIT) : __float_as_int(a.w);
        const float4* Nn = sc.tnorm + 3 * (size_t)tri;
        const float4 n0 = Nn[0], n1 = Nn[1], n2 = Nn[2];
        int32_t oid = -1, mat = -1;
        if (sc.objids != nullptr && tri >= 0 && tri < sc.num_tris) {
            oid = sc.objids[tri];
            if (sc.mats != nullptr && oid >= 0 && oid < sc.num_mats) mat = oid;
        }
        h = hit_record(r, e1, e2, mk(n0.x, n0.y, n0.z), mk(n1.x, n1.y, n1.z), mk(n2.x, n2.y, n2.z), t, u, v, tri, oid, mat);
    }
    uint4* out = Q.hits + 4 * (size_t)i;
    out[0] = h.w[0];
    out[1] = h.w[1];
    out[2] = h.w[2];
    out[3] = h.w[3];
}

// ---- camera rays on the device (rt_camera_rays_device), DESIGN.md §4.19 -----------------------
struct CameraRaysParams {
    f3 center, p00, du, dv;
    int32_t W, spp, row0;
    int32_t sample0;  // the table's first sample is sample0 of the frame's (rt_camera_rays_pass_device)
    uint32_t n;  // W * rows * spp < 2^31
    const float* __restrict__ jitter;  // 2 * spp
    float* __restrict__ rays;          // n x rt_ray
    uint32_t* __restrict__ seeds;      // n, or null
};

// One sample per lane in the order of the reference's AOVs, ((y - row0) W + x) spp + s, so
// consecutive lanes write consecutive rays: the rays render() shoots (camera_dir, the arithmetic
// of the render kernels' camera_ray) and the rng states it seeds them with (query.cu:146-158).
__global__ __launch_bounds__(BLOCK) void camera_rays_kernel(CameraRaysParams P) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.n) return;
    const uint32_t pix = i / (uint32_t)P.spp;
    const int s = (int)(i - pix * (uint32_t)P.spp);
    const uint32_t yl = pix / (uint32_t)P.W;
    const int x = (int)(pix - yl * (uint32_t)P.W), y = P.row0 + (int)yl;
    const f3 d = camera_dir(P.center, P.p00, P.du, P.dv, x, y, P.jitter[2 * s], P.jitter[2 * s + 1]);
    float* R = P.rays + 6 * (size_t)i;
    R[0] = P.center.x;
    R[1] = P.center.y;
    R[2] = P.center.z;
    R[3] = d.x;
    R[4] = d.y;
    R[5] = d.z;
    if (P.seeds != nullptr) P.seeds[i] = make_rng_seed(x, y, P.sample0 + s);
}
