// rt_math.hpp — device-side float/double math of the ray path, in the reference's exact
// evaluation order (G/include/vec3.h, bvh.h, query.h, shader.h, brdf.h, camera.h).
// The translation unit is compiled with -ffp-contract=off (no v_fma for a*b+c) and with
// HIP's default correctly-rounded f32 division and sqrt, so every helper below returns the
// bits the reference's x86-64 build returns; the one libm call on the path, powf, is a
// restatement of the reference libm's own algorithm (ref_powf below, DESIGN.md "Parity").
#pragma once

#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstdint>

namespace rtd {

struct f3 {
    float x, y, z;
};

__host__ __device__ __forceinline__ f3 mk(float x, float y, float z) { return f3{x, y, z}; }
__host__ __device__ __forceinline__ f3 add(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__host__ __device__ __forceinline__ f3 sub(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__host__ __device__ __forceinline__ f3 neg(f3 a) { return mk(-a.x, -a.y, -a.z); }
__host__ __device__ __forceinline__ f3 mul(f3 a, f3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
__host__ __device__ __forceinline__ f3 scale(f3 v, float t) { return mk(v.x * t, v.y * t, v.z * t); }
__host__ __device__ __forceinline__ float dot(f3 u, f3 v) { return u.x * v.x + u.y * v.y + u.z * v.z; }
__host__ __device__ __forceinline__ f3 cross(f3 u, f3 v) {
    return mk(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x);
}
// Vec3 / double(len) == correctly rounded f32 division (vec3.h:334).
__host__ __device__ __forceinline__ f3 divf(f3 v, float t) { return mk(v.x / t, v.y / t, v.z / t); }
// unit_vector (vec3.h:345-348) and normalize (vec3.h:343) round identically.
__host__ __device__ __forceinline__ f3 unit(f3 v) {
    const float len = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
    return divf(v, len);
}
// Camera::unit_vector with the 1e-12 fallback (camera.h:218-223).
__host__ __device__ __forceinline__ f3 cam_unit(f3 v) {
    const float len = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
    if ((double)len < 1e-12) return mk(0.0f, 0.0f, 1.0f);
    return divf(v, len);
}

// An axis-aligned box as the kernels hold it: per axis the (min, max) pair, adjacent so one
// packed instruction handles both slabs of an axis.
typedef float v2f __attribute__((ext_vector_type(2)));
struct BoxP {
    v2f x, y, z;
};

// Relative slack of the float pre-classification (see box_classify).
constexpr float kBoxRel = 1e-6f;
constexpr float kRayTMin = 1e-4f;  // query.h:233: the tmin of every traversal's box and triangle tests

// A ray as the slab test needs it.  `par` bit a: |dir[a]| < 1e-8f, where intersectAABB
// degenerates to an exact inside test on that axis (bvh.h:90-91).  iv is a float reciprocal
// of the direction (any <= 2 ulp approximation), +inf on parallel axes, split by sign into
// ivp = max(iv, 0) and ivn = min(iv, 0); c1 = -o*iv - E, c2 = -o*iv + E and e2 = 2E with a
// per-ray error bound E (box_classify).  A ray with a parallel axis, or whose slab parameters
// could come near the float range ((bmax + |o|) |iv| >= 1e37 on some axis, or not finite),
// gets c1 = c2 = NaN and tmin_pre = NaN: every test of it is ambiguous (exact path).  They
// serve the pre-classification only, never the decision of an ambiguous case.
struct RayPre {
    f3 o, d;
    v2f ivx, ivy, ivz;  // per axis (ivp, ivn)
    v2f cx, cy, cz;     // per axis (c1, c2)
    f3 e2;
    float m2;       // 2 max(e2): the one-margin HIT test's (box_sure_hit1); +inf if unsafe
    float tmin_pre;  // the box tests' tmin, or NaN for a ray the pre-classification does not handle
    uint32_t par;
};

__host__ __device__ __forceinline__ float rcp_approx(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);  // v_rcp_f32, 1 ulp
#else
    return 1.0f / x;
#endif
}

// bmax: per axis, an upper bound of |coordinate| over every box the ray will be tested
// against (the scene's; make_ray_mt for rays that meet no box).  tmin: the tmin of every box
// test the ray will take (the traversals' kRayTMin).
__host__ __device__ __forceinline__ RayPre make_ray(f3 o, f3 d, f3 bmax, float tmin = kRayTMin) {
    RayPre r;
    r.o = o;
    r.d = d;
    const float eps = 1e-8f;
    const bool px = fabsf(d.x) < eps, py = fabsf(d.y) < eps, pz = fabsf(d.z) < eps;
    r.par = (px ? 1u : 0u) | (py ? 2u : 0u) | (pz ? 4u : 0u);
    const float iv[3] = {px ? INFINITY : rcp_approx(d.x), py ? INFINITY : rcp_approx(d.y),
                         pz ? INFINITY : rcp_approx(d.z)};
    const float oc[3] = {o.x, o.y, o.z}, bm[3] = {bmax.x, bmax.y, bmax.z};
    float ivp[3], ivn[3], c1[3], c2[3], e2[3];
    bool safe = !(px || py || pz);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float oiv = oc[a] * iv[a];
        const float S = fabsf(oiv) + bm[a] * fabsf(iv[a]);  // >= |slab parameter| of any box
        safe = safe && S < 1e37f;
        const float E = kBoxRel * (2.0f * fabsf(oiv) + bm[a] * fabsf(iv[a])) + 1e-30f;
        ivp[a] = iv[a] >= 0.0f ? iv[a] : 0.0f;
        ivn[a] = iv[a] >= 0.0f ? 0.0f : iv[a];
        c1[a] = -oiv - E;
        c2[a] = -oiv + E;
        e2[a] = 2.0f * E;
    }
    if (!safe) c1[0] = c1[1] = c1[2] = c2[0] = c2[1] = c2[2] = NAN;
    r.ivx = (v2f){ivp[0], ivn[0]};
    r.ivy = (v2f){ivp[1], ivn[1]};
    r.ivz = (v2f){ivp[2], ivn[2]};
    r.cx = (v2f){c1[0], c2[0]};
    r.cy = (v2f){c1[1], c2[1]};
    r.cz = (v2f){c1[2], c2[2]};
    r.e2 = mk(e2[0], e2[1], e2[2]);
    r.m2 = safe ? 2.0f * fmaxf(fmaxf(e2[0], e2[1]), e2[2]) : INFINITY;
    r.tmin_pre = safe ? tmin : NAN;
    return r;
}

// A ray used only for triangle tests (origin and direction).
__host__ __device__ __forceinline__ RayPre make_ray_mt(f3 o, f3 d) { return make_ray(o, d, mk(0.f, 0.f, 0.f)); }

// intersectAABB(ray, box, tmin, tmax) exactly as the reference evaluates it (bvh.h:81-129):
// per axis inv = 1.0/double(dir), tNear/tFar = (double(bound) - double(orig)) * inv,
// reference compare/swap order.  The boolean equals the reference's early-return form
// because t0 only grows and t1 only shrinks.
template <bool LOCAL = false>
__host__ __device__ inline bool box_hit_exact(const RayPre& r, const BoxP& b, double tmin, double tmax) {
    double t0 = tmin, t1 = tmax;
    // No register-pinning asm here: an empty asm "+v" on o/d (to keep the compiler from hoisting
    // double(o) and 1/double(d) out of the traversal loops) measured no faster and, in the 6-wave
    // build, exposed a miscompile of the bounce and binary-record kernels (golden parity failures;
    // DESIGN.md §7).
    // LOCAL: hoisted out of a traversal loop, double(o) and 1/double(d) hold 12 VGPRs across
    // the whole loop for a test only ambiguous lanes reach (a few % of box tests).  An opaque
    // SGPR zero, made here (inside the wave-uniform branch that calls this), ORed into the float
    // bits ties them to this call, so they are recomputed per exact test instead (the c3 kernel
    // then has no scratch; c5's big-scene kernel, with 30x more exact tests, keeps the hoist).
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t oz = 0;
    if constexpr (LOCAL) asm volatile("" : "+s"(oz));
    const float o[3] = {__uint_as_float(__float_as_uint(r.o.x) | oz), __uint_as_float(__float_as_uint(r.o.y) | oz),
                        __uint_as_float(__float_as_uint(r.o.z) | oz)};
    const float d[3] = {__uint_as_float(__float_as_uint(r.d.x) | oz), __uint_as_float(__float_as_uint(r.d.y) | oz),
                        __uint_as_float(__float_as_uint(r.d.z) | oz)};
#else
    const float o[3] = {r.o.x, r.o.y, r.o.z}, d[3] = {r.d.x, r.d.y, r.d.z};
#endif
    const float mn[3] = {b.x.x, b.y.x, b.z.x}, mx[3] = {b.x.y, b.y.y, b.z.y};
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (r.par & (1u << a)) {
            ok = ok && !(o[a] < mn[a] || o[a] > mx[a]);
        } else {
            const double inv = 1.0 / (double)d[a];
            double tn = ((double)mn[a] - (double)o[a]) * inv;
            double tf = ((double)mx[a] - (double)o[a]) * inv;
            if (tn > tf) {
                const double tmp = tn;
                tn = tf;
                tf = tmp;
            }
            if (tn > t0) t0 = tn;
            if (tf < t1) t1 = tf;
            ok = ok && !(t0 > t1);
        }
    }
    return ok;
}

// Conservative float pre-classification of the same test: MISS / HIT are returned only when
// the reference's double computation is guaranteed to give that answer; AMBIG otherwise.
// Per axis, with the near bound (min if iv >= 0, else max) and the far one, the slab
// parameters' padded ends are FMAs against the per-ray constants:
//   lo' - E = fma(near, iv, c1),   hi' + E = fma(far, iv, c2),
// written sign-free as near*iv + c = fma(min, ivp, fma(max, ivn, c)) (one of ivp/ivn is 0, so
// the inner FMA returns c exactly) and far*iv + c = fma(max, ivp, fma(min, ivn, c)); then
// lo' + E = (lo' - E) + 2E and hi' - E = (hi' + E) - 2E, one more rounding each (in the
// slack below).
// Error budget (finite inputs): with iv = (1/d)(1+e1), |e1| <= 2^-23 (1-ulp reciprocal),
// oiv = o*iv rounded, c1/c2 rounded and the FMA's rounding (each <= 2^-24 relative), the
// distance between fma(b, iv, -oiv -+ E) and t -+ E, t = (b - o)/d exactly, is at most
// 1.8e-7 |t| + 2.4e-7 |oiv| + 1.2e-7 E (+ 6e-8 (|t| + 3E) for the +-2E steps); the reference's
// double tNear/tFar are within
// 3.4e-16 |t| of t.  E = kBoxRel (2 |oiv| + bmax |iv|) + 1e-30 >= kBoxRel (|t| + |oiv|)
// (|t| <= |b| |iv| + |oiv|) with kBoxRel = 1e-6 covers both with > 4x slack (the error is
// <= 2.4e-7 (|t| + |oiv|) + 3e-7 E <= 0.25 E; 4e-6 had 16x, but 4x more of the box tests fell
// to the double path: c3 -2 %, c5 -4 % at 1e-6); the 1e-30 term
// covers subnormal absolute error.  So lowLo <= exact lo <= lowHi and highLo <= exact hi <=
// highHi per axis, and with Lmax / Hmin the reference's max of lows / min of highs (tmin and
// tmax exact in both precisions):
//   MISS  if max(tmin, lowLo) > min(tmax, highHi)     (then Lmax > Hmin: reference rejects)
//   HIT   if max(tmin, lowHi) <= min(tmax, highLo)    (then Lmax <= Hmin: reference accepts)
// For a safe ray (make_ray) every estimate is finite and below 1e37 in magnitude, far from
// overflow.  An unsafe ray's estimates are NaN and so is the tmin folded into Lc and into the
// HIT tests (tmin_pre; max and min drop a NaN beside a number, but of two NaNs they return NaN):
// Lc is NaN, every compare with it is false, and neither MISS nor HIT is read.  Every test of an
// unsafe ray is decided in double.  (With a plain tmin there, MISS read tmin > tmax for an unsafe
// ray, which the reference does not reject for a ray parallel to all three axes: its answer is
// the inside test whatever tmin and tmax are.  No traversal makes that input, tmax being a bestT
// >= tmin; tests/box_cases.py's degenerate set does.)  The reference's parallel-axis inside test
// is only taken by unsafe rays, so it never needs a float counterpart.
enum : int { BOX_MISS = 0, BOX_HIT = 1, BOX_AMBIG = 2 };
// The per-axis padded ends lo' - E (lL) and hi' + E (hH).
struct AxisEnds {
    float lLx, lLy, lLz, hHx, hHy, hHz;
};
__host__ __device__ __forceinline__ AxisEnds box_ends(const RayPre& r, const BoxP& b) {
    AxisEnds e;
    e.lLx = __builtin_fmaf(b.x.x, r.ivx.x, __builtin_fmaf(b.x.y, r.ivx.y, r.cx.x));
    e.hHx = __builtin_fmaf(b.x.y, r.ivx.x, __builtin_fmaf(b.x.x, r.ivx.y, r.cx.y));
    e.lLy = __builtin_fmaf(b.y.x, r.ivy.x, __builtin_fmaf(b.y.y, r.ivy.y, r.cy.x));
    e.hHy = __builtin_fmaf(b.y.y, r.ivy.x, __builtin_fmaf(b.y.x, r.ivy.y, r.cy.y));
    e.lLz = __builtin_fmaf(b.z.x, r.ivz.x, __builtin_fmaf(b.z.y, r.ivz.y, r.cz.x));
    e.hHz = __builtin_fmaf(b.z.y, r.ivz.x, __builtin_fmaf(b.z.x, r.ivz.y, r.cz.y));
    return e;
}
#if defined(__HIP_DEVICE_COMPILE__)
// The same in packed FMAs (v_pk_fma_f32, two lanes of math per instruction; the min/max swap is
// an operand select): [lL, hH] = fma([min, max], [ivp, ivp], fma([max, min], [ivn, ivn], [c1, c2]))
// -- the same two roundings per end, so the same bits.  The depth-1 kernels' wave traversal uses
// it: c5 72.6 vs 76.1 ms, c3 0.1834 vs 0.1841 ms (`scripts/ab_libs.py`, one box, frames
// identical; profiles/r03/exp/packed_box_ends_ab_*.log).  The bounce kernels keep the scalar
// form (packed, their 3-wave build spilled 28 B per lane).
__device__ __forceinline__ v2f axis_ends(v2f b, v2f iv, v2f c) {
    const v2f sw = __builtin_shufflevector(b, b, 1, 0);
    const v2f ivn = __builtin_shufflevector(iv, iv, 1, 1), ivp = __builtin_shufflevector(iv, iv, 0, 0);
    return __builtin_elementwise_fma(b, ivp, __builtin_elementwise_fma(sw, ivn, c));
}
__device__ __forceinline__ AxisEnds box_ends_pk(const RayPre& r, const BoxP& b) {
    const v2f x = axis_ends(b.x, r.ivx, r.cx), y = axis_ends(b.y, r.ivy, r.cy), z = axis_ends(b.z, r.ivz, r.cz);
    AxisEnds e;
    e.lLx = x.x;
    e.hHx = x.y;
    e.lLy = y.x;
    e.hHy = y.y;
    e.lLz = z.x;
    e.hHz = z.y;
    return e;
}
#else
__device__ __forceinline__ AxisEnds box_ends_pk(const RayPre& r, const BoxP& b) { return box_ends(r, b); }  // host pass: parsed, never emitted
#endif
// Lc = max(tmin, lowLo) and Hc = min(tmax, highHi): MISS iff Lc > Hc.  tmin: the ray's tmin_pre.
struct BoxEnds {
    float Lc, Hc;
};
__host__ __device__ __forceinline__ BoxEnds box_lc_hc(const AxisEnds& e, float tmin, float tmax) {
    return BoxEnds{fmaxf(fmaxf(fmaxf(e.lLx, e.lLy), e.lLz), tmin), fminf(fminf(fminf(e.hHx, e.hHy), e.hHz), tmax)};
}
__host__ __device__ __forceinline__ bool box_miss(const BoxEnds& c) { return c.Lc > c.Hc; }
// HIT with one margin for all axes: lowHi <= lowLo + max(e2) and highLo >= highHi - max(e2), so
// Lc + 2 max(e2) <= Hc implies the per-axis HIT test (the rounding of the add is far inside
// the slack of E).  Cheap; ambiguous cases go on to box_sure_hit2.
__host__ __device__ __forceinline__ bool box_sure_hit1(const RayPre& r, const BoxEnds& c) { return c.Lc + r.m2 <= c.Hc; }
// HIT with the per-axis margins.
__host__ __device__ __forceinline__ bool box_sure_hit2(const RayPre& r, const AxisEnds& e, float tmax) {
    const float lowHi = fmaxf(fmaxf(e.lLx + r.e2.x, e.lLy + r.e2.y), e.lLz + r.e2.z);
    const float highLo = fminf(fminf(e.hHx - r.e2.x, e.hHy - r.e2.y), e.hHz - r.e2.z);
    return fmaxf(lowHi, r.tmin_pre) <= fminf(highLo, tmax);
}

// (tmin is the one the ray was made with, make_ray.)
__host__ __device__ __forceinline__ int box_classify(const RayPre& r, const BoxP& b, float tmax) {
    const AxisEnds e = box_ends(r, b);
    const BoxEnds c = box_lc_hc(e, r.tmin_pre, tmax);
    if (box_miss(c)) return BOX_MISS;
    if (box_sure_hit1(r, c) || box_sure_hit2(r, e, tmax)) return BOX_HIT;
    return BOX_AMBIG;
}

// intersectAABB with the float fast path; bit-identical answer to box_hit_exact.  tmin: the one
// the ray was made with (make_ray).
__host__ __device__ __forceinline__ bool box_hit(const RayPre& r, const BoxP& b, float tmin, float tmax) {
    const int c = box_classify(r, b, tmax);
    if (c != BOX_AMBIG) return c == BOX_HIT;
    return box_hit_exact(r, b, (double)tmin, (double)tmax);
}

// Möller–Trumbore of intersectTriangle (query.h:72-108) with e1 = v1-v0, e2 = v2-v0
// precomputed on the host (same float subtraction).  Returns hit and t/u/v.
__host__ __device__ __forceinline__ bool mt_g(const RayPre& r, f3 v0, f3 e1, f3 e2, float tmin, float tmax,
                                     float& t_out, float& u_out, float& v_out) {
    const f3 pvec = cross(r.d, e2);
    const float det = dot(e1, pvec);
    if (fabsf(det) < 1e-8f) return false;
    const float invDet = 1.0f / det;
    const f3 tvec = sub(r.o, v0);
    const float u = dot(tvec, pvec) * invDet;
    if (u < 0.0f || u > 1.0f) return false;
    const f3 qvec = cross(tvec, e1);
    const float v = dot(r.d, qvec) * invDet;
    if (v < 0.0f || (u + v) > 1.0f) return false;
    const float t = dot(e2, qvec) * invDet;
    if (t < tmin || t > tmax) return false;
    t_out = t;
    u_out = u;
    v_out = v;
    return true;
}

// HW1 ray_intersection (HW1/include/ray.h:67-104): eps = FLT_EPSILON, t >= 0, no tmax.
__host__ __device__ __forceinline__ bool mt_hw1(f3 o, f3 d, f3 v0, f3 e1, f3 e2, float& t_out, float& u_out,
                                       float& v_out) {
    const f3 pvec = cross(d, e2);
    const float det = dot(pvec, e1);
    if (fabsf(det) < FLT_EPSILON) return false;
    const float invDet = 1.0f / det;  // == (float)(1.0 / (double)det)
    const f3 tvec = sub(o, v0);
    const float u = dot(tvec, pvec) * invDet;
    if (u < 0.0f || u > 1.0f) return false;
    const f3 qvec = cross(tvec, e1);
    const float v = dot(d, qvec) * invDet;
    if (v < 0.0f || (u + v) > 1.0f) return false;
    const float t = dot(e2, qvec) * invDet;
    if (t < 0.0f) return false;
    t_out = t;
    u_out = u;
    v_out = v;
    return true;
}

// Hit-record completion of intersectTriangle (query.h:110-127) for the winning triangle.
__host__ __device__ __forceinline__ void hit_frame(const RayPre& r, f3 e1, f3 e2, f3 n0, f3 n1, f3 n2, float t,
                                          float u, float v, f3& p, f3& shadingN) {
    p = add(r.o, scale(r.d, t));
    f3 geomN = unit(cross(e1, e2));
    const bool front = dot(r.d, geomN) < 0.0f;
    if (!front) geomN = neg(geomN);
    const float w = 1.0f - u - v;
    f3 sN = add(add(scale(n0, w), scale(n1, u)), scale(n2, v));
    if (dot(sN, sN) < 1e-12f) {
        sN = geomN;
    } else {
        sN = unit(sN);
        if (dot(sN, geomN) < 0.0f) sN = neg(sN);
    }
    shadingN = sN;
}

// The same completion with everything intersectTriangle derives on the way kept (the hit records
// of rt_trace_hits): geomN after its flip towards the ray (query.h:115-117) and rec.front_face.
// A sibling, not a wrapper: hit_frame's callers keep their own code.
struct HitFrame {
    f3 p, shadingN, geomN;
    bool front;
};
__host__ __device__ __forceinline__ HitFrame hit_frame_full(const RayPre& r, f3 e1, f3 e2, f3 n0, f3 n1, f3 n2, float t,
                                                            float u, float v) {
    HitFrame h;
    h.p = add(r.o, scale(r.d, t));
    f3 geomN = unit(cross(e1, e2));
    h.front = dot(r.d, geomN) < 0.0f;
    if (!h.front) geomN = neg(geomN);
    const float w = 1.0f - u - v;
    f3 sN = add(add(scale(n0, w), scale(n1, u)), scale(n2, v));
    if (dot(sN, sN) < 1e-12f) {
        sN = geomN;
    } else {
        sN = unit(sN);
        if (dot(sN, geomN) < 0.0f) sN = neg(sN);
    }
    h.shadingN = sN;
    h.geomN = geomN;
    return h;
}

// Camera::get_ray(float, float) (camera.h:49-53): the direction of sample (x + jx, y + jy),
// unit_vector(pix - center) with pix = (p00 + du*px) + dv*py and Camera::unit_vector's double
// division and fallback (camera.h:218-223).  The expression of the render kernels' camera_ray
// (rt_shade.hpp), which keeps its own text: written through this helper, 27 render kernels came
// out with other instruction schedules (scripts/isa_diff.py), and those kernels are pinned.
__host__ __device__ __forceinline__ f3 camera_dir(f3 center, f3 p00, f3 du, f3 dv, int x, int y, float jx, float jy) {
    const float px = (float)x + jx, py = (float)y + jy;
    const f3 pix = add(add(p00, scale(du, px)), scale(dv, py));
    return cam_unit(sub(pix, center));
}

// G/include/query.h:32-48
__host__ __device__ __forceinline__ float rng_next(uint32_t& state) {
    state = state * 1664525u + 1013904223u;
    uint32_t h = state;
    h = (h ^ 61u) ^ (h >> 16u);
    h *= 9u;
    h ^= h >> 4u;
    h *= 0x27d4eb2du;
    h ^= h >> 15u;
    return (float)h / (float)0xFFFFFFFFu;
}
__host__ __device__ __forceinline__ uint32_t make_rng_seed(int x, int y, int s) {
    return (uint32_t)x * 73856093u ^ (uint32_t)y * 19349663u ^ (uint32_t)s * 83492791u;
}
__host__ __device__ __forceinline__ f3 random_unit_vector(uint32_t& st) {
    for (;;) {
        const float x = 2.0f * rng_next(st) - 1.0f;
        const float y = 2.0f * rng_next(st) - 1.0f;
        const float z = 2.0f * rng_next(st) - 1.0f;
        const float lensq = x * x + y * y + z * z;
        if (lensq > 1e-10f && lensq <= 1.0f) {
            const float inv = 1.0f / sqrtf(lensq);
            return mk(x * inv, y * inv, z * inv);
        }
    }
}

// ---- powf: the reference's libm, restated ---------------------------------------------
// The reference calls powf from glibc (Ubuntu GLIBC 2.35-0ubuntu3.11 in this image), whose
// single-precision pow is the ARM optimized-routines algorithm (glibc
// sysdeps/ieee754/flt-32/e_powf.c, e_powf_log2_data.c, e_exp2f_data.c): log2 through a
// 16-entry (invc, log2 c) table + degree-5 polynomial in double, times y, then exp2 through
// a 32-entry 2^(i/32) table + degree-3 polynomial, rounded once to float.  On x86-64 with
// FMA, glibc dispatches to the -mfma build of that file, where every a*b+c of the
// polynomial steps is one fused multiply-add; the fma() calls below are exactly those.
// Constants are the values of __powf_log2_data / __exp2f_data.  The restatement is pinned
// bit for bit against glibc powf by tests/test_powf.py (host build of this code and the
// device kernel); with it the whole shading chain is reproduced bit for bit.
namespace pw {
// (invc, log2 c) pairs of __powf_log2_data.tab and the 2^(i/32) bit patterns of
// __exp2f_data.tab.  Device copies live in constant memory (indexed per lane: an L1-cached
// vector load, no registers held across the kernel); the host copies serve rt_powf_host.
#define RT_POW_LOG_TAB                                                                        \
    {0x1.661ec79f8f3bep+0, -0x1.efec65b963019p-2, 0x1.571ed4aaf883dp+0, -0x1.b0b6832d4fca4p-2, \
     0x1.49539f0f010b0p+0, -0x1.7418b0a1fb77bp-2, 0x1.3c995b0b80385p+0, -0x1.39de91a6dcf7bp-2, \
     0x1.30d190c8864a5p+0, -0x1.01d9bf3f2b631p-2, 0x1.25e227b0b8ea0p+0, -0x1.97c1d1b3b7af0p-3, \
     0x1.1bb4a4a1a343fp+0, -0x1.2f9e393af3c9fp-3, 0x1.12358f08ae5bap+0, -0x1.960cbbf788d5cp-4, \
     0x1.0953f419900a7p+0, -0x1.a6f9db6475fcep-5, 0x1.0000000000000p+0, 0x0.0p+0,              \
     0x1.e608cfd9a47acp-1, 0x1.338ca9f24f53dp-4, 0x1.ca4b31f026aa0p-1, 0x1.476a9543891bap-3,   \
     0x1.b2036576afce6p-1, 0x1.e840b4ac4e4d2p-3, 0x1.9c2d163a1aa2dp-1, 0x1.40645f0c6651cp-2,   \
     0x1.886e6037841edp-1, 0x1.88e9c2c1b9ff8p-2, 0x1.767dcf5534862p-1, 0x1.ce0a44eb17bccp-2}
#define RT_EXP2_TAB                                                                           \
    {0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull, \
     0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull, \
     0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull, \
     0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull, \
     0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull, \
     0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull, \
     0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull, \
     0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull}
__constant__ const double kLogTabDev[32] = RT_POW_LOG_TAB;
__constant__ const uint64_t kExp2TabDev[32] = RT_EXP2_TAB;
static const double kLogTabHost[32] = RT_POW_LOG_TAB;
static const uint64_t kExp2TabHost[32] = RT_EXP2_TAB;

struct LogEntry {
    double invc, logc;
};
__host__ __device__ __forceinline__ LogEntry log_tab(int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return {kLogTabDev[2 * i], kLogTabDev[2 * i + 1]};
#else
    return {kLogTabHost[2 * i], kLogTabHost[2 * i + 1]};
#endif
}
__host__ __device__ __forceinline__ uint64_t exp2_tab(int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return kExp2TabDev[i];
#else
    return kExp2TabHost[i];
#endif
}
__host__ __device__ __forceinline__ uint32_t asu(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
__host__ __device__ __forceinline__ float asf(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
__host__ __device__ __forceinline__ uint64_t asu64(double f) { uint64_t u; __builtin_memcpy(&u, &f, 8); return u; }
__host__ __device__ __forceinline__ double asd(uint64_t u) { double f; __builtin_memcpy(&f, &u, 8); return f; }

// A double constant of the powf polynomials.  On the device it is made by two s_mov_b32 in
// volatile asm where it is used: otherwise the compiler hoists the constants out of the shading
// loop into VGPR pairs that stay live across the shadow traversal and spills them to scratch.
#if defined(__HIP_DEVICE_COMPILE__)
#define RT_KF64(name, val)                                                                     \
    double name;                                                                               \
    {                                                                                          \
        constexpr uint64_t b_ = __builtin_bit_cast(uint64_t, (double)(val));                   \
        uint32_t lo_, hi_;                                                                     \
        asm volatile("s_mov_b32 %0, %1" : "=s"(lo_) : "i"((int32_t)(uint32_t)b_));             \
        asm volatile("s_mov_b32 %0, %1" : "=s"(hi_) : "i"((int32_t)(uint32_t)(b_ >> 32)));     \
        name = __builtin_bit_cast(double, ((uint64_t)hi_ << 32) | lo_);                        \
    }
#else
#define RT_KF64(name, val) const double name = (val);
#endif

__host__ __device__ __forceinline__ double log2_inline(uint32_t ix) {
    const uint32_t tmp = ix - 0x3f330000u;
    const int i = int((tmp >> 19) % 16u);
    const uint32_t top = tmp & 0xff800000u;
    const uint32_t iz = ix - top;
    const int k = int32_t(top) >> 23;
    const LogEntry e = log_tab(i);
    const double z = double(asf(iz));
    RT_KF64(A0, 0x1.27616c9496e0bp-2)
    RT_KF64(A1, -0x1.71969a075c67ap-2)
    RT_KF64(A2, 0x1.ec70a6ca7baddp-2)
    RT_KF64(A3, -0x1.7154748bef6c8p-1)
    RT_KF64(A4, 0x1.71547652ab82bp+0)
    const double r = fma(z, e.invc, -1.0);
    const double y0 = e.logc + double(k);
    const double r2 = r * r;
    double y = fma(A0, r, A1);
    const double p = fma(A2, r, A3);
    const double r4 = r2 * r2;
    double q = fma(A4, r, y0);
    q = fma(p, r2, q);
    y = fma(y, r4, q);
    return y;
}

__host__ __device__ __forceinline__ float exp2_inline(double xd, uint32_t sign_bias) {
    const double SHIFT = 0x1.8p+47;  // 0x1.8p52 / 32
    RT_KF64(C0, 0x1.c6af84b912394p-5)
    RT_KF64(C1, 0x1.ebfce50fac4f3p-3)
    RT_KF64(C2, 0x1.62e42ff0c52d6p-1)
    double kd = xd + SHIFT;
    const uint64_t ki = asu64(kd);
    kd -= SHIFT;
    const double r = xd - kd;
    uint64_t t = exp2_tab(int(ki % 32u));
    const uint64_t ski = ki + sign_bias;
    // t += ski << (52 - 5), on the high word: the shifted value's low word is 0, so there is no
    // carry.  (A 64-bit value with a zero low word made the compiler keep a zero VGPR live
    // across the render kernel's item loop, spilled.)
    t = (uint64_t)((uint32_t)(t >> 32) + ((uint32_t)ski << 15)) << 32 | (uint32_t)t;
    const double s = asd(t);
    const double z = fma(C0, r, C1);
    const double r2 = r * r;
    double y = fma(C2, r, 1.0);
    y = fma(z, r2, y);
    y = y * s;
    return float(y);
}

__host__ __device__ __forceinline__ int checkint(uint32_t iy) {
    const int e = int(iy >> 23 & 0xff);
    if (e < 0x7f) return 0;
    if (e > 0x7f + 23) return 2;
    if (iy & ((1u << (0x7f + 23 - e)) - 1)) return 0;
    if (iy & (1u << (0x7f + 23 - e))) return 1;
    return 2;
}
__host__ __device__ __forceinline__ bool zeroinfnan(uint32_t ix) { return 2 * ix - 1 >= 2u * 0x7f800000u - 1; }
__host__ __device__ __forceinline__ bool issignaling(uint32_t ix) {
    return 2 * (ix ^ 0x00400000u) > 2u * 0x7fc00000u;
}
}  // namespace pw

__host__ __device__ inline float ref_powf(float x, float y) {
    using namespace pw;
    uint32_t sign_bias = 0;
    uint32_t ix = asu(x);
    const uint32_t iy = asu(y);
    if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u || zeroinfnan(iy)) {
        if (zeroinfnan(iy)) {
            if (2 * iy == 0) return issignaling(ix) ? x + y : 1.0f;
            if (ix == 0x3f800000u) return issignaling(iy) ? x + y : 1.0f;
            if (2 * ix > 2u * 0x7f800000u || 2 * iy > 2u * 0x7f800000u) return x + y;
            if (2 * ix == 2 * 0x3f800000u) return 1.0f;
            if ((2 * ix < 2 * 0x3f800000u) == !(iy & 0x80000000u)) return 0.0f;
            return y * y;
        }
        if (zeroinfnan(ix)) {
            float x2 = x * x;
            if ((ix & 0x80000000u) && checkint(iy) == 1) x2 = -x2;
            return (iy & 0x80000000u) ? 1.0f / x2 : x2;
        }
        if (ix & 0x80000000u) {
            const int yint = checkint(iy);
            if (yint == 0) return (x - x) / (x - x);
            if (yint == 1) sign_bias = 1u << (5 + 11);
            ix &= 0x7fffffffu;
        }
        if (ix < 0x00800000u) {
            ix = asu(x * 0x1p23f);
            ix &= 0x7fffffffu;
            ix -= 23u << 23;
        }
    }
    const double logx = log2_inline(ix);
    const double ylogx = double(y) * logx;
    // The library gates these two tests with (asuint64(ylogx) >> 47 & 0xffff) >= asuint64(126.0)
    // >> 47, i.e. |ylogx| >= 124 or NaN, a superset of both: they decide alone, so the gate is
    // dropped (its 64-bit mask kept a zero VGPR live across the render kernel's item loop).
    if (ylogx > 0x1.fffffffd1d571p+6) return sign_bias ? -INFINITY : INFINITY;
    if (ylogx <= -150.0) return sign_bias ? -0.0f : 0.0f;
    return exp2_inline(ylogx, sign_bias);
}

__host__ __device__ __forceinline__ f3 clamp01(f3 c) {  // shader.h:24-32
    if (c.x > 1.0f) c.x = 1.0f;
    if (c.y > 1.0f) c.y = 1.0f;
    if (c.z > 1.0f) c.z = 1.0f;
    if (c.x < 0.0f) c.x = 0.0f;
    if (c.y < 0.0f) c.y = 0.0f;
    if (c.z < 0.0f) c.z = 0.0f;
    return c;
}

}  // namespace rtd
