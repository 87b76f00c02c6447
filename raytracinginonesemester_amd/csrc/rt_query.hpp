// rt_query.hpp — batched ray queries on a resident scene (rt_trace_rays*, include/rt_mi355x.h):
// closest hit = SearchBVH (G/include/query.h:224-311) for caller rays, occlusion = the decision
// of IsInShadow (G/include/shader.h:59-61).  One ray per lane over the per-lane traversals of
// rt_traverse.hpp; DESIGN.md §4.17.
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
