// rt_closest.hpp — closest-point queries on a resident scene (rt_closest_points*, include/rt_mi355x.h):
// per query point the nearest leaf triangle, its squared distance and the nearest point.  The answer
// is the minimum over every leaf of (D, triangle index), D in a fixed float32 arithmetic whose
// nearest point is confined to the leaf's box (cp_triangle); the float distance to a box (cp_box_lb)
// is then a lower bound of D for everything below the box, so a walk may skip a box whose bound
// exceeds the best D so far and still return the brute-force answer, in any visiting order.
// One point per lane, the three variants of rt_query.hpp; DESIGN.md §4.28.
// Part of rt_device.hip's translation unit, included inside its anonymous namespace after rt_multihit.hpp.
#pragma once

// ---- the definition: shared by the kernel and the host build (rt_closest_points_host) ----------
// One leaf's candidate, and the best so far: rt_point_hit's fields.
struct CpHit {
    int32_t tri;
    float D;
    f3 p;
    float v, w;
    int32_t region;
};

// x confined to [b.x, b.y]; a NaN stays NaN.
__host__ __device__ __forceinline__ float cp_confine(float x, v2f b) { return x < b.x ? b.x : (x > b.y ? b.y : x); }
__host__ __device__ __forceinline__ f3 cp_confine(f3 p, const BoxP& b) {
    return mk(cp_confine(p.x, b.x), cp_confine(p.y, b.y), cp_confine(p.z, b.z));
}

// lb(q, B): the squared distance from q to q confined to B, in D's operation order.
__host__ __device__ __forceinline__ float cp_box_lb(f3 q, const BoxP& b) {
    const f3 d = sub(q, cp_confine(q, b));
    return dot(d, d);
}

// The nearest point of triangle (a, a + e1, a + e2) to q by Voronoi region (first match in the order
// A, B, AB, C, AC, BC, face), confined to the leaf's box b, and its squared distance.  Every region's
// terms are computed and the region then selected: each value is a function of the inputs alone, so
// the order of evaluation does not show, and the lanes of a wave do not part by region.  The
// comparisons are written as the definition states them: a NaN fails each and falls to the face.
__host__ __device__ __forceinline__ CpHit cp_triangle(f3 q, f3 a, f3 e1, f3 e2, const BoxP& b, int32_t tri) {
    const f3 ap = sub(q, a);
    const float d1 = dot(e1, ap), d2 = dot(e2, ap);
    const f3 bp = sub(ap, e1);
    const float d3 = dot(e1, bp), d4 = dot(e2, bp);
    const f3 cp = sub(ap, e2);
    const float d5 = dot(e1, cp), d6 = dot(e2, cp);
    const float vc = d1 * d4 - d3 * d2;
    const float vb = d5 * d2 - d1 * d6;
    const float va = d3 * d6 - d5 * d4;
    const float d43 = d4 - d3, d56 = d5 - d6;
    // one division serves whichever region wins: num / den
    int32_t region = 6;
    float num = 1.0f, den = (va + vb) + vc;
    if (va <= 0.0f && d43 >= 0.0f && d56 >= 0.0f) region = 5, num = d43, den = d43 + d56;
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) region = 4, num = d2, den = d2 - d6;
    if (d6 >= 0.0f && d5 <= d6) region = 2;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) region = 3, num = d1, den = d1 - d3;
    if (d3 >= 0.0f && d4 <= d3) region = 1;
    if (d1 <= 0.0f && d2 <= 0.0f) region = 0;
    const float r = num / den;
    float v, w;
    switch (region) {
        case 0: v = 0.0f, w = 0.0f; break;
        case 1: v = 1.0f, w = 0.0f; break;
        case 2: v = 0.0f, w = 1.0f; break;
        case 3: v = r, w = 0.0f; break;
        case 4: v = 0.0f, w = r; break;
        case 5: w = r, v = 1.0f - w; break;
        default: v = vb * r, w = vc * r; break;
    }
    CpHit h;
    h.tri = tri;
    h.v = v;
    h.w = w;
    h.region = region;
    h.p = cp_confine(add(add(a, scale(e1, v)), scale(e2, w)), b);
    const f3 d = sub(q, h.p);
    h.D = dot(d, d);
    return h;
}

// The candidate wins: nearer, or as near with a lower triangle index.  A NaN D never wins.
__host__ __device__ __forceinline__ bool cp_wins(const CpHit& c, const CpHit& best) {
    return c.D < best.D || (c.D == best.D && c.tri < best.tri);
}

// The state before the first candidate: best.D is the bound (max_d2, or +inf), inclusive.
__host__ __device__ __forceinline__ CpHit cp_start(float bound) {
    CpHit h;
    h.tri = INT32_MAX;
    h.D = bound;
    h.p = mk(0.0f, 0.0f, 0.0f);
    h.v = h.w = 0.0f;
    h.region = -1;
    return h;
}

// ---- the kernel --------------------------------------------------------------------------------
struct ClosestParams {
    SceneView sc;
    const float* __restrict__ points;  // n x 3
    const float* __restrict__ max_d2;  // n bounds on D, or null: +inf
    uint32_t n;
    uint32_t n_leaf;              // records in sc.leaf (0: the scene has no triangle to find)
    uint4* __restrict__ hits;     // n x rt_point_hit, 16-byte aligned
    uint32_t* __restrict__ evals; // n, or null
};

// A lane's walk: the best candidate, the leaves evaluated, and whether a push met a full stack.
struct CpLane {
    f3 q;
    CpHit best;
    uint32_t evals;
    bool overflow;

    // A leaf's triangle and box from its one record: v0 | tri, e1, e2.x | e2.y e2.z, box x | box y, box z.
    __device__ __forceinline__ void leaf(float4 w0, float4 w1, float4 w2, float4 w3) {
        const CpHit c = cp_triangle(q, mk(w0.x, w0.y, w0.z), mk(w1.x, w1.y, w1.z), mk(w1.w, w2.x, w2.y),
                                    BoxP{hi2(w2), lo2(w3), hi2(w3)}, __float_as_int(w0.w));
        ++evals;
        if (cp_wins(c, best)) best = c;
    }
    // An entry's sort key: its bound's bits (a bound is a sum of squares: not negative, so the bits
    // order as the floats do), 0 for a NaN bound, which never prunes; NO_REF for an entry that is
    // absent or already further than the best.
    __device__ __forceinline__ uint32_t key(uint32_t ref, const BoxP& b) const {
        const float lb = cp_box_lb(q, b);
        if (ref == NO_REF || lb > best.D) return NO_REF;
        return lb == lb ? __float_as_uint(lb) : 0u;
    }
    __device__ __forceinline__ bool pruned(uint32_t key) const { return __uint_as_float(key) > best.D; }
};

// The stacks: entries of two words (ref, key).  In LDS a lane's words are NT apart, so the lanes of a
// wave at one depth touch consecutive banks; DEEP's is private, the reference's 512 entries.
template <int NT>
struct CpLdsStack {
    static constexpr int CAP = LANE_LDS_CAP;
    uint32_t* s;
    __device__ __forceinline__ void put(int sp, uint32_t ref, uint32_t key) {
        s[(2 * sp) * NT] = ref;
        s[(2 * sp + 1) * NT] = key;
    }
    __device__ __forceinline__ void get(int sp, uint32_t& ref, uint32_t& key) const {
        ref = s[(2 * sp) * NT];
        key = s[(2 * sp + 1) * NT];
    }
};
struct CpPrivateStack {
    static constexpr int CAP = REF_STACK;
    uint32_t r[REF_STACK], k[REF_STACK];
    __device__ __forceinline__ void put(int sp, uint32_t ref, uint32_t key) { r[sp] = ref, k[sp] = key; }
    __device__ __forceinline__ void get(int sp, uint32_t& ref, uint32_t& key) const { ref = r[sp], key = k[sp]; }
};

// Every push is guarded: one onto a full stack drops the entry and flags the lane, whose walk is
// then completed by a scan of every leaf (closest_complete).
template <class Stack>
__device__ __forceinline__ void cp_push(Stack& st, int& sp, bool& overflow, uint32_t ref, uint32_t key) {
    if (key == NO_REF) return;
    if (sp < Stack::CAP) {
        st.put(sp, ref, key);
        ++sp;
    } else {
        overflow = true;
    }
}
// The next entry off the stack that the current best does not prune (its box is not loaded again).
template <class Stack>
__device__ __forceinline__ bool cp_pop(const Stack& st, int& sp, const CpLane& ln, uint32_t& ref) {
    while (sp > 0) {
        uint32_t key;
        --sp;
        st.get(sp, ref, key);
        if (!ln.pruned(key)) return true;
    }
    return false;
}

__device__ __forceinline__ void cp_order(uint32_t& ka, uint32_t& ra, uint32_t& kb, uint32_t& rb) {
    const bool s = ka > kb;
    const uint32_t k0 = s ? kb : ka, r0 = s ? rb : ra, k1 = s ? ka : kb, r1 = s ? ra : rb;
    ka = k0, ra = r0, kb = k1, rb = r1;
}

// Near-first over the 4-ary records: the bounds of a record's up to four entries, the nearest
// surviving one next, the others pushed farthest first (a five-comparator sort of (key, ref) in
// registers).  An entry's box in the record is its node's own box, so a leaf reached here was bounded
// by the box its record holds.
template <class Stack>
__device__ __forceinline__ void closest_wide(const SceneView& sc, CpLane& ln, Stack& st) {
    uint32_t ref = sc.root_ref;
    int sp = 0;
    while (true) {
        const bool leaf = (ref & LEAF_BIT) != 0;
        const uint32_t idx = ref & ~LEAF_BIT;
        const float4* R = leaf ? sc.leaf + 4 * (size_t)idx : sc.wnode + 8 * (size_t)idx;
        const float4 w0 = R[0], w1 = R[1], w2 = R[2], w3 = R[3];
        float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f), w5 = w4, w6 = w4;
        if (!leaf) {
            w4 = R[4];
            w5 = R[5];
            w6 = R[6];
        }
        uint32_t next = NO_REF;
        if (leaf) {
            ln.leaf(w0, w1, w2, w3);
        } else {
            uint32_t r0 = __float_as_uint(w6.x), r1 = __float_as_uint(w6.y), r2 = __float_as_uint(w6.z),
                     r3 = __float_as_uint(w6.w);
            uint32_t k0 = ln.key(r0, BoxP{lo2(w0), hi2(w0), lo2(w1)}), k1 = ln.key(r1, BoxP{hi2(w1), lo2(w2), hi2(w2)}),
                     k2 = ln.key(r2, BoxP{lo2(w3), hi2(w3), lo2(w4)}), k3 = ln.key(r3, BoxP{hi2(w4), lo2(w5), hi2(w5)});
            cp_order(k0, r0, k1, r1);
            cp_order(k2, r2, k3, r3);
            cp_order(k0, r0, k2, r2);
            cp_order(k1, r1, k3, r3);
            cp_order(k1, r1, k2, r2);
            cp_push(st, sp, ln.overflow, r3, k3);
            cp_push(st, sp, ln.overflow, r2, k2);
            cp_push(st, sp, ln.overflow, r1, k1);
            if (k0 != NO_REF) next = r0;
        }
        if (next != NO_REF) {
            ref = next;
            continue;
        }
        if (!cp_pop(st, sp, ln, ref)) return;
    }
}

// Near-first over the binary records (inode): LDS stack for BINARY, the private one for DEEP.
template <class Stack>
__device__ __forceinline__ void closest_binary(const SceneView& sc, CpLane& ln, Stack& st) {
    uint32_t ref = sc.root_ref;
    int sp = 0;
    while (true) {
        uint32_t next = NO_REF;
        if (ref & LEAF_BIT) {
            const float4* L = sc.leaf + 4 * (size_t)(ref & ~LEAF_BIT);
            ln.leaf(L[0], L[1], L[2], L[3]);
        } else {
            const float4* N = sc.inode + 4 * (size_t)ref;
            const float4 q0 = N[0], q1 = N[1], q2 = N[2];
            const uint4 q3 = *reinterpret_cast<const uint4*>(N + 3);
            uint32_t r0 = q3.x, r1 = q3.y;
            uint32_t k0 = ln.key(r0, BoxP{lo2(q0), hi2(q0), lo2(q1)}), k1 = ln.key(r1, BoxP{hi2(q1), lo2(q2), hi2(q2)});
            cp_order(k0, r0, k1, r1);
            cp_push(st, sp, ln.overflow, r1, k1);
            if (k0 != NO_REF) next = r0;
        }
        if (next != NO_REF) {
            ref = next;
            continue;
        }
        if (!cp_pop(st, sp, ln, ref)) return;
    }
}

// A flagged lane's completion: the walk's state dropped, every leaf record in slot order.  The
// definition itself, so exact whatever the walk had dropped.
__device__ __forceinline__ void closest_complete(const SceneView& sc, uint32_t n_leaf, float bound, CpLane& ln) {
    ln.best = cp_start(bound);
    ln.evals = 0;
    for (uint32_t s = 0; s < n_leaf; ++s) {
        const float4* L = sc.leaf + 4 * (size_t)s;
        ln.leaf(L[0], L[1], L[2], L[3]);
    }
}

template <int VARIANT>
__device__ __forceinline__ void closest_walk(const SceneView& sc, CpLane& ln, uint32_t* stk) {
    if constexpr (VARIANT == RT_RAYS_VARIANT_DEEP) {
        CpPrivateStack st;
        closest_binary(sc, ln, st);
    } else {
        CpLdsStack<BLOCK> st{stk + threadIdx.x};
        if constexpr (VARIANT == RT_RAYS_VARIANT_WIDE) closest_wide(sc, ln, st);
        else closest_binary(sc, ln, st);
    }
}

// One point per lane.  The 32-byte record leaves as two 16-byte words; a point without a winner
// gets the miss record.
template <int VARIANT>
__global__ __launch_bounds__(BLOCK) void closest_points_kernel(ClosestParams Q) {
    constexpr bool LDS = VARIANT != RT_RAYS_VARIANT_DEEP;
    __shared__ uint32_t stk[LDS ? 2 * LANE_LDS_CAP * BLOCK : 1];
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;  // n < 2^31
    if (i >= Q.n) return;
    const SceneView& sc = Q.sc;
    const float* P = Q.points + 3 * (size_t)i;
    const float bound = Q.max_d2 != nullptr ? Q.max_d2[i] : INFINITY;
    CpLane ln;
    ln.q = mk(P[0], P[1], P[2]);
    ln.best = cp_start(bound);
    ln.evals = 0;
    ln.overflow = false;
    if (Q.n_leaf != 0 && !(cp_box_lb(ln.q, own_box(sc, sc.root_ref, true)) > bound)) {
        closest_walk<VARIANT>(sc, ln, stk);
        if (ln.overflow) closest_complete(sc, Q.n_leaf, bound, ln);
    }
    const CpHit& b = ln.best;
    const bool won = b.region >= 0;
    uint4* out = Q.hits + 2 * (size_t)i;
    out[0] = won ? make_uint4((uint32_t)b.tri, pw::asu(b.D), pw::asu(b.p.x), pw::asu(b.p.y))
                 : make_uint4(0xFFFFFFFFu, pw::asu(-1.0f), 0u, 0u);
    out[1] = won ? make_uint4(pw::asu(b.p.z), pw::asu(b.v), pw::asu(b.w), (uint32_t)b.region)
                 : make_uint4(0u, 0u, 0u, 0xFFFFFFFFu);
    if (Q.evals != nullptr) Q.evals[i] = ln.evals;
}
