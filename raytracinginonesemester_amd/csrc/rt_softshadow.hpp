// rt_softshadow.hpp — spherical area lights for the staged path (rt_light_visibility_*,
// rt_path_step_vis_*, include/rt_mi355x.h): G/'s ShadeDirect with C/'s ShadowVisibility
// (C/include/raytracer.h:121-168) in place of IsInShadow.  A visibility stage between trace_hits
// and the step writes, per (entry, light), the unoccluded fraction of S shadow rays into a disk at
// the light that faces the shaded point; the step then scales the light's term by it.  The disk
// samples are drawn from the path's own rng_next stream (the lights' samples first, then the
// bounce's xi: C/'s order within a depth); the occlusion decision and RT_EPS are G/'s.  With every
// shape a point light the two stages are path_step_kernel bit for bit.  DESIGN.md §4.30.
// Part of rt_device.hip's translation unit, included inside its anonymous namespace after rt_path.hpp.
#pragma once

constexpr int SOFT_MAX_SAMPLES = 256;  // shadow_samples above it: RT_ERR_UNSUPPORTED

struct DevLightShape {  // rt_light_shape
    float radius;
    int32_t shadow_samples;
};

// What a (hit point, light) pair asks of the stage: steps 1 to 3 of the definition.
enum SoftClass {
    SOFT_DARK,   // NdotL <= 0: vis 0, nothing cast, nothing drawn
    SOFT_LIT,    // the light sits on the point: vis 1, nothing cast, nothing drawn
    SOFT_POINT,  // radius <= 0 or NaN: IsInShadow's one ray
    SOFT_DISK    // S samples of the disk
};

// toC, distC: the light's centre from p.  S: the rays of the pair (1 unless SOFT_DISK).
__host__ __device__ __forceinline__ SoftClass soft_class(f3 p, f3 N, f3 lpos, DevLightShape shape, f3& toC, float& distC,
                                                         int& S) {
    toC = sub(lpos, p);
    const f3 L = unit(toC);
    const float NdotL = fmaxf(dot(N, L), 0.0f);
    distC = 0.0f;
    S = 1;
    if (NdotL <= 0.0f) return SOFT_DARK;
    distC = sqrtf(dot(toC, toC));
    if (!(distC > 0.0f)) return SOFT_LIT;
    if (!(shape.radius > 0.0f)) return SOFT_POINT;
    S = shape.shadow_samples > 1 ? shape.shadow_samples : 1;
    return SOFT_DISK;
}

// The disk's basis (raytracer.h:136-140): W from the light to the point, T and B across it.
__host__ __device__ __forceinline__ void soft_basis(f3 p, f3 lpos, float distC, f3& T, f3& B) {
    const f3 W = divf(sub(p, lpos), distC);
    const f3 a = fabsf(W.x) > 0.9f ? mk(0.f, 1.f, 0.f) : mk(1.f, 0.f, 0.f);
    T = unit(cross(a, W));
    B = cross(W, T);
}

// One point of the unit disk by rejection (raytracer.h:143-150).  The LCG has full period and the
// accepted set is not empty, so the loop ends for any state.
__host__ __device__ __forceinline__ void soft_disk_draw(uint32_t& state, float& x, float& y) {
    for (;;) {
        x = 2.0f * rng_next(state) - 1.0f;
        y = 2.0f * rng_next(state) - 1.0f;
        const float r2 = x * x + y * y;
        if (r2 > 1e-10f && r2 <= 1.0f) return;
    }
}

// The sample's shadow ray from p: its direction and bound.  False: the sample sits on p, no ray,
// and it counts as unoccluded.
__host__ __device__ __forceinline__ bool soft_sample_ray(f3 p, f3 lpos, f3 T, f3 B, float radius, float x, float y, f3& dir,
                                                         float& d) {
    const f3 lp = add(add(lpos, scale(T, x * radius)), scale(B, y * radius));
    const f3 toL = sub(lp, p);
    d = sqrtf(dot(toL, toL));
    if (!(d > 0.0f)) return false;
    dir = divf(toL, d);
    return true;
}

struct LightVisParams {
    SceneView sc;
    const uint4* __restrict__ hits;            // m x rt_hit, 16-byte aligned
    const uint32_t* __restrict__ ids;          // m path ids, or null: k
    const DevLightShape* __restrict__ shapes;  // sc.num_lights
    uint32_t* __restrict__ rng;                // the state's rng, by path id
    float* __restrict__ vis;                   // m x sc.num_lights
    uint32_t m;
};

// G lanes per entry (a power of two; a wave serves 64 / G entries), lane j of a group tracing the
// samples j, j + G, ... of each light.  Every lane of a group holds the entry's p and N, the
// light's class and the rng state, so everything but the traversal is uniform within a group:
// the lanes of a group take every branch and every round of the sample loop together.  The
// rejection loop makes sample i's draws depend on all earlier ones, so each lane replays the
// light's whole sequence (a round's G draws, about a dozen integer operations each, against a
// traversal per lane) and keeps its own sample.  A round's unoccluded samples are counted by one
// ballot: the group's bits of the wave's mask, the same count in every lane of the group.  Lane 0
// of the group stores the vis word and, after the last light, the state.  The rays of a group
// share an origin and point into one small disk: they walk the same records.  Ids are unique, so
// each state word has one writer: plain stores.
template <int VARIANT, int G>
__global__ __launch_bounds__(BLOCK) void light_visibility_kernel(LightVisParams P) {
    static_assert(G >= 1 && G <= 64 && (G & (G - 1)) == 0, "a power of two within a wave");
    constexpr bool LDS = VARIANT != RT_RAYS_VARIANT_DEEP;
    __shared__ uint32_t stk_all[LDS ? LANE_LDS_CAP * BLOCK : 1];
    const uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint64_t k64 = t / G;
    if (k64 >= P.m) return;  // whole groups leave: BLOCK is a multiple of G
    const uint32_t k = (uint32_t)k64;
    const int j = (int)(threadIdx.x & (G - 1));
    const uint32_t gbase = (threadIdx.x & 63u) & ~(uint32_t)(G - 1);  // the group's first lane in its wave
    uint32_t* stk = stk_all + (LDS ? threadIdx.x : 0);
    const SceneView& sc = P.sc;
    const int nl = sc.num_lights;
    float* out = P.vis + (size_t)k * (size_t)nl;
    const uint32_t id = P.ids != nullptr ? P.ids[k] : k;
    const uint4* H = P.hits + 4 * (size_t)k;
    const uint4 w0 = H[0];
    if (id == PATH_NONE || (int32_t)w0.x < 0) {  // no path or a miss: a row of zeros, no state word touched
        for (int li = j; li < nl; li += G) out[li] = 0.0f;
        return;
    }
    const uint4 w1 = H[1], w2 = H[2];
    const f3 p = mk(pw::asf(w1.x), pw::asf(w1.y), pw::asf(w1.z));
    const f3 N = unit(mk(pw::asf(w1.w), pw::asf(w2.x), pw::asf(w2.y)));
    const f3 origin = add(p, scale(N, RT_EPS));
    uint32_t state = P.rng[id];
    auto clear = [&](f3 dir, float bound) {  // IsInShadow's decision (shader.h:44-62), negated
        const RayPre sray = make_ray(origin, dir, scene_bmax(sc));
        HitState shs;
        shade_traverse<VARIANT>(sc, sray, true, bound, shs, stk);
        return !(shs.slot >= 0 && shs.bestT < bound);
    };
    for (int li = 0; li < nl; ++li) {
        const DevLight& lt = sc.lights[li];
        const f3 lpos = mk(lt.pos[0], lt.pos[1], lt.pos[2]);
        const DevLightShape shape = P.shapes[li];
        f3 toC;
        float distC;
        int S;
        const SoftClass cls = soft_class(p, N, lpos, shape, toC, distC, S);
        float v;
        if (cls == SOFT_DARK) {
            v = 0.0f;
        } else if (cls == SOFT_LIT) {
            v = 1.0f;
        } else if (cls == SOFT_POINT) {
            bool c = false;
            if (j == 0) c = clear(divf(toC, distC), distC);
            v = c ? 1.0f : 0.0f;  // (lane 0's own answer: the lane that stores)
        } else {
            f3 T, B;
            soft_basis(p, lpos, distC, T, B);
            uint32_t count = 0;
            for (int i0 = 0; i0 < S; i0 += G) {
                const int round = S - i0 < G ? S - i0 : G;  // the samples of this round
                float mx = 0.0f, my = 0.0f;
                for (int q = 0; q < round; ++q) {
                    float x, y;
                    soft_disk_draw(state, x, y);
                    if (q == j) {
                        mx = x;
                        my = y;
                    }
                }
                bool c = false;
                if (j < round) {
                    f3 dir;
                    float d;
                    c = !soft_sample_ray(p, lpos, T, B, shape.radius, mx, my, dir, d) || clear(dir, d);
                }
                if constexpr (G == 1) count += c ? 1u : 0u;
                else if constexpr (G == 64) count += (uint32_t)__popcll(ballot(c));
                else count += (uint32_t)__popcll((ballot(c) >> gbase) & ((1ull << G) - 1ull));
            }
            v = (float)count / (float)S;
        }
        if (j == 0) out[li] = v;
    }
    if (j == 0) P.rng[id] = state;
}

// path_step_one (rt_path.hpp) with the lights' visibilities in place of the shadow traversal: a
// sibling, word for word but for the light loop, because path_step_kernel's instructions are
// pinned and came out differently when the two shared one template (scripts/isa_diff.py).  After
// the NdotL > 0 test v = vis[li]: a light with !(v > 0) is skipped, the others add
// (radiance * f) * (NdotL * v) (C/include/raytracer.h:195-207), which is path_step_one's term bit
// for bit when v == 1.  Everything else (the miss, the material, ambient and emission, the bounce
// and its draws, next / alive / direct) is that function's.
__host__ __device__ __forceinline__ void path_step_vis_one(const float* R, const uint4* H, const float* mat_k,
                                                           const DevMaterial* table, int num_table, const DevLight* lights,
                                                           int num_lights, const float* vis, f3 miss, bool diffuse_bounce,
                                                           bool last, float* radiance, float* throughput, uint32_t* rng_state,
                                                           float* next, uint8_t* alive, float* direct) {
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
        // ShadeDirect (shader.h:65-110) with the visibility's factor
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
            const float v = vis[li];
            if (!(v > 0.0f)) continue;
            const DevMaterial m = material();
            const f3 f = eval_brdf(m, n, V, L);
            const f3 rad = scale(mk(lt.color[0], lt.color[1], lt.color[2]), (float)lt.intensity);
            Lo = add(Lo, scale(mul(rad, f), NdotL * v));
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

struct PathStepVisParams {
    const float* rays;                  // as PathStepParams
    const uint4* __restrict__ hits;
    const float* __restrict__ mats;
    const uint32_t* __restrict__ ids;
    const float* __restrict__ vis;      // m x num_lights
    const DevMaterial* __restrict__ table;
    const DevLight* __restrict__ lights;
    int32_t num_table, num_lights;
    uint32_t m;
    int32_t diffuse_bounce, last;
    f3 miss;
    float* __restrict__ radiance;
    float* __restrict__ throughput;
    uint32_t* __restrict__ rng;
    float* next;
    uint8_t* __restrict__ alive;
    float* __restrict__ direct;
};

// path_step_kernel with the light's visibility read where that casts the shadow ray: one entry
// per lane, no traversal, no LDS, no variant.
__global__ __launch_bounds__(BLOCK) void path_step_vis_kernel(PathStepVisParams P) {
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;  // m < 2^31
    if (k >= P.m) return;
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
    path_step_vis_one(R, P.hits + 4 * (size_t)k, P.mats != nullptr ? P.mats + 13 * (size_t)k : nullptr, P.table, P.num_table,
                      P.lights, P.num_lights, P.vis + (size_t)k * (size_t)P.num_lights, P.miss, P.diffuse_bounce != 0,
                      P.last != 0, P.radiance + 3 * (size_t)id, P.throughput + 3 * (size_t)id, P.rng + id, next, alive, direct);
}
