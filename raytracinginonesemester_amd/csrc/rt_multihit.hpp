// rt_multihit.hpp — multi-hit queries on a resident scene (rt_trace_multi_hits*, include/rt_mi355x.h):
// every triangle a caller ray hits up to a fixed bound tmax, counted, and the k nearest of them in
// order.  The hit set is what SearchBVH (G/include/query.h:224-311) would collect if the bound it
// passes to intersectAABB and intersectTriangle stayed at tmax and every accepted triangle were
// kept.  One ray per lane, the three variants of rt_query.hpp; DESIGN.md §4.26.
// Part of rt_device.hip's translation unit, included inside its anonymous namespace after rt_query.hpp.
#pragma once

struct MultiHitParams {
    SceneView sc;
    const float* __restrict__ rays;   // n x rt_ray
    const float* __restrict__ max_t;  // n bounds, or null: FLT_MAX
    uint32_t n;
    int32_t k;                    // list length, 0 .. KC of the instantiation
    uint4* __restrict__ hits;     // n x k rt_multi_hit, 16-byte aligned; null with k == 0
    int32_t* __restrict__ count;  // n, or null
};

// The k classes the kernels are instantiated for (a lane's list takes 8 * KC bytes of LDS) and
// the block size of each: the k <= 32 class runs 128-thread blocks, so that its 48 KiB per block
// leave a CU three blocks rather than one of 96 KiB.
__host__ __device__ constexpr int mh_class(int k) { return k == 0 ? 0 : k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32; }
__host__ __device__ constexpr int mh_block(int kc) { return kc == 32 ? BLOCK / 2 : BLOCK; }

// A list entry names its triangle by where the lane found it: a slot of the packed leaf array, or
// BRUTE_BIT | triangle index after DEEP's brute-force completion (the tri array).
template <bool DEEP>
__device__ __forceinline__ const float4* mh_record(const SceneView& sc, uint32_t entry) {
    if constexpr (DEEP) {
        if (entry & BRUTE_BIT) return sc.tri + 3 * (size_t)(entry & ~BRUTE_BIT);
    }
    return sc.leaf + 4 * (size_t)entry;
}
template <bool DEEP>
__device__ __forceinline__ int32_t mh_tri(const SceneView& sc, uint32_t entry) {
    if constexpr (DEEP) {
        if (entry & BRUTE_BIT) return (int32_t)(entry & ~BRUTE_BIT);
    }
    return __float_as_int(sc.leaf[4 * (size_t)entry].w);
}

// A lane's hits so far: the full count, and its k best (t, triangle) pairs in ascending order in
// LDS (entry j at [j * NT]: t's bits in lt, the entry in le).  The order is by t's bit pattern,
// which for the t >= 1e-4 that intersectTriangle accepts is the order of the floats and stays a
// total order for a NaN t of unspecified inputs; equal t by ascending triangle index, read from
// the leaf record only on such a tie.  The bound never moves to the k-th entry: a candidate past
// it is counted and dropped, nothing is pruned.
template <int NT, bool DEEP>
struct MultiHitLane {
    uint32_t* lt;
    uint32_t* le;
    int k, m;  // capacity, entries held
    int32_t count;

    __device__ __forceinline__ void add(const SceneView& sc, uint32_t tb, uint32_t entry, int32_t tri) {
        ++count;
        if (k == 0) return;
        int j = m;
        if (m == k) {
            const uint32_t lb = lt[(k - 1) * NT];
            if (tb > lb || (tb == lb && tri >= mh_tri<DEEP>(sc, le[(k - 1) * NT]))) return;
            j = k - 1;
        } else {
            ++m;
        }
        while (j > 0) {
            const uint32_t pb = lt[(j - 1) * NT];
            if (pb < tb) break;
            const uint32_t pe = le[(j - 1) * NT];
            if (pb == tb && mh_tri<DEEP>(sc, pe) <= tri) break;
            lt[j * NT] = pb;
            le[j * NT] = pe;
            --j;
        }
        lt[j * NT] = tb;
        le[j * NT] = entry;
    }

    // intersectTriangle(ray, triangle, 1e-4, tmax) on a leaf or tri record's first three words.
    __device__ __forceinline__ void test(const SceneView& sc, const RayPre& r, float tmax, float4 a, float4 b, float4 c,
                                         uint32_t entry, int32_t tri) {
        float t, u, v;
        if (mt_g(r, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), mk(b.w, c.x, c.y), kRayTMin, tmax, t, u, v))
            add(sc, __float_as_uint(t), entry, tri);
    }
};

// traverse_lane_lds_wide with the bound fixed at tmax: with one bound a popped entry's re-test
// would repeat its push-time test, so there is no re-test, no stale watermark and no early exit.
// A record's entries are an internal node's grandchildren; a child's box contains theirs
// (rt_scene_create emits the records only then) and the slab test is monotone in the
// box, so an entry that passes implies its skipped parent passes: the leaves reached are those
// whose whole root-to-leaf path passes.
template <int NT, class Lane>
__device__ __forceinline__ void multi_hit_wide(const SceneView& sc, const RayPre& r, float tmax, Lane& ln, uint32_t* stk) {
    if (!box_hit(r, own_box(sc, sc.root_ref, true), kRayTMin, tmax)) return;
    uint32_t ref = sc.root_ref;
    int sp = 0;
    while (true) {
        const bool leaf = (ref & LEAF_BIT) != 0;
        const uint32_t idx = ref & ~LEAF_BIT;
        const float4* R = leaf ? sc.leaf + 4 * (size_t)idx : sc.wnode + 8 * (size_t)idx;
        const float4 w0 = R[0], w1 = R[1], w2 = R[2];
        float4 w3 = make_float4(0.f, 0.f, 0.f, 0.f), w4 = w3, w5 = w3, w6 = w3;
        if (!leaf) {
            w3 = R[3];
            w4 = R[4];
            w5 = R[5];
            w6 = R[6];
        }
        uint32_t next = NO_REF;  // the entry to hold
        if (leaf) {
            ln.test(sc, r, tmax, w0, w1, w2, idx, __float_as_int(w0.w));
        } else {
            const float4 wv[7] = {w0, w1, w2, w3, w4, w5, w6};
            const uint32_t refs[4] = {__float_as_uint(w6.x), __float_as_uint(w6.y), __float_as_uint(w6.z),
                                      __float_as_uint(w6.w)};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (refs[e] == NO_REF) continue;
                const float4 p = wv[(3 * e) / 2], q = wv[(3 * e) / 2 + 1];
                const BoxP bk = (e & 1) ? BoxP{hi2(p), lo2(q), hi2(q)} : BoxP{lo2(p), hi2(p), lo2(q)};
                if (box_hit(r, bk, kRayTMin, tmax)) {
                    if (next != NO_REF) {
                        stk[sp * NT] = next;
                        ++sp;
                    }
                    next = refs[e];
                }
            }
        }
        if (next != NO_REF) {
            ref = next;
            continue;
        }
        if (sp == 0) return;
        --sp;
        ref = stk[sp * NT];
    }
}

// traverse_lane_lds (the binary records) with the bound fixed.
template <int NT, class Lane>
__device__ __forceinline__ void multi_hit_binary(const SceneView& sc, const RayPre& r, float tmax, Lane& ln, uint32_t* stk) {
    if (!box_hit(r, own_box(sc, sc.root_ref, true), kRayTMin, tmax)) return;
    uint32_t ref = sc.root_ref;
    int sp = 0;
    while (true) {
        uint32_t next = NO_REF;
        if (ref & LEAF_BIT) {
            const uint32_t slot = ref & ~LEAF_BIT;
            const float4* L = sc.leaf + 4 * (size_t)slot;
            const float4 a = L[0], b = L[1], c = L[2];
            ln.test(sc, r, tmax, a, b, c, slot, __float_as_int(a.w));
        } else {
            const float4* N = sc.inode + 4 * (size_t)ref;
            const float4 q0 = N[0], q1 = N[1], q2 = N[2];
            const uint4 q3 = *reinterpret_cast<const uint4*>(N + 3);
            const bool hl = q3.x != NO_REF && box_hit(r, BoxP{lo2(q0), hi2(q0), lo2(q1)}, kRayTMin, tmax);
            const bool hr = q3.y != NO_REF && box_hit(r, BoxP{hi2(q1), lo2(q2), hi2(q2)}, kRayTMin, tmax);
            if (hl && hr) {
                stk[sp * NT] = q3.x;
                ++sp;
            }
            next = hr ? q3.y : (hl ? q3.x : NO_REF);
        }
        if (next != NO_REF) {
            ref = next;
            continue;
        }
        if (sp == 0) return;
        --sp;
        ref = stk[sp * NT];
    }
}

// traverse_deep with the bound fixed: SearchBVH's stack discipline as written (the root pushed
// unconditionally, every pop tests the node's own box, a leaf naming no triangle keeps its entry,
// a push onto a full stack sets the flag), so a lane overflows exactly when the reference's
// control flow would with this bound.  On overflow what the DFS collected is dropped and every
// triangle of the scene is tested in index order: the reference's brute-force completion, a
// superset of what the DFS saw.
template <class Lane>
__device__ void multi_hit_deep(const SceneView& sc, const RayPre& r, float tmax, Lane& ln) {
    uint32_t st[REF_STACK];
    int sp = 0;
    bool overflow = false;
    st[sp++] = sc.root_ref;
    while (sp > 0) {
        const uint32_t ref = st[--sp];
        if (ref == INV_LEAF) continue;
        if (!box_hit(r, own_box(sc, ref, false), kRayTMin, tmax)) continue;
        if (ref & LEAF_BIT) {
            const uint32_t slot = ref & ~LEAF_BIT;
            const float4* L = sc.leaf + 4 * (size_t)slot;
            const float4 a = ldc(L), b = ldc(L + 1), c = ldc(L + 2);
            ln.test(sc, r, tmax, a, b, c, slot, __float_as_int(a.w));
            continue;
        }
        const float4* N = sc.inode + 4 * (size_t)ref;
        const float4 q0 = ldc(N), q1 = ldc(N + 1), q2 = ldc(N + 2);
        const uint4 q3 = ldc_u(N + 3);  // left ref, right ref, invalid-leaf flags (bit 0 left, bit 1 right)
        if ((q3.x != NO_REF || (q3.z & 1u)) && box_hit(r, BoxP{lo2(q0), hi2(q0), lo2(q1)}, kRayTMin, tmax)) {
            if (sp < REF_STACK) st[sp++] = (q3.z & 1u) ? INV_LEAF : q3.x;
            else overflow = true;
        }
        if ((q3.y != NO_REF || (q3.z & 2u)) && box_hit(r, BoxP{hi2(q1), lo2(q2), hi2(q2)}, kRayTMin, tmax)) {
            if (sp < REF_STACK) st[sp++] = (q3.z & 2u) ? INV_LEAF : q3.y;
            else overflow = true;
        }
    }
    if (overflow) {
        ln.m = 0;
        ln.count = 0;
        for (int i = 0; i < sc.num_tris; ++i) {
            const float4* T = sc.tri + 3 * (size_t)i;
            ln.test(sc, r, tmax, ldc(T), ldc(T + 1), ldc(T + 2), BRUTE_BIT | (uint32_t)i, i);
        }
    }
}

// One ray per lane.  KC: the k class (0: counts only, no list).  The kept entries' u, v are not
// carried through the walk: each winner's triangle is tested once more at the end, by the same
// mt_g call that accepted it, which gives the same t, u, v.  A lane stores its k records as k
// 16-byte words; slots past its count get the miss record (-1, -1.0f, 0, 0).
template <int VARIANT, int KC>
__global__ __launch_bounds__(mh_block(KC)) void multi_hit_kernel(MultiHitParams Q) {
    constexpr int NT = mh_block(KC);
    constexpr bool LDS = VARIANT != RT_RAYS_VARIANT_DEEP;
    constexpr bool DEEP = !LDS;
    __shared__ uint32_t stk[LDS ? LANE_LDS_CAP * NT : 1];
    __shared__ uint32_t list_t[KC > 0 ? KC * NT : 1];
    __shared__ uint32_t list_e[KC > 0 ? KC * NT : 1];
    const uint32_t i = blockIdx.x * NT + threadIdx.x;  // n < 2^31
    if (i >= Q.n) return;
    const SceneView& sc = Q.sc;
    const float* R = Q.rays + 6 * (size_t)i;
    const RayPre r = make_ray(mk(R[0], R[1], R[2]), mk(R[3], R[4], R[5]), scene_bmax(sc));
    const float tmax = Q.max_t != nullptr ? Q.max_t[i] : FLT_MAX;
    MultiHitLane<NT, DEEP> ln;
    ln.lt = list_t + (KC > 0 ? threadIdx.x : 0);
    ln.le = list_e + (KC > 0 ? threadIdx.x : 0);
    ln.k = KC > 0 ? Q.k : 0;
    ln.m = 0;
    ln.count = 0;
    if constexpr (VARIANT == RT_RAYS_VARIANT_WIDE) multi_hit_wide<NT>(sc, r, tmax, ln, stk + threadIdx.x);
    else if constexpr (VARIANT == RT_RAYS_VARIANT_BINARY) multi_hit_binary<NT>(sc, r, tmax, ln, stk + threadIdx.x);
    else multi_hit_deep(sc, r, tmax, ln);
    if (Q.count != nullptr) Q.count[i] = ln.count;
    if constexpr (KC > 0) {
        uint4* out = Q.hits + (size_t)i * (size_t)ln.k;  // n * k < 2^31
        for (int j = 0; j < ln.k; ++j) {
            uint4 h = make_uint4(0xFFFFFFFFu, pw::asu(-1.0f), 0u, 0u);
            if (j < ln.m) {
                const uint32_t entry = ln.le[j * NT];
                const float4* T = mh_record<DEEP>(sc, entry);
                const float4 a = T[0], b = T[1], c = T[2];
                float t = 0.f, u = 0.f, v = 0.f;
                mt_g(r, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), mk(b.w, c.x, c.y), kRayTMin, tmax, t, u, v);
                const int32_t tri = DEEP && (entry & BRUTE_BIT) ? (int32_t)(entry & ~BRUTE_BIT) : __float_as_int(a.w);
                h = make_uint4((uint32_t)tri, ln.lt[j * NT], pw::asu(u), pw::asu(v));
            }
            out[j] = h;
        }
    }
}
