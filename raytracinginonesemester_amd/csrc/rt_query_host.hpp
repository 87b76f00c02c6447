// rt_query_host.hpp — the host side of the caller queries on a resident scene, a section of
// rt_device.hip (included there once rt_scene and scene_view are defined; not a translation unit of
// its own: the traversals the query kernels share read the __device__ globals of rt_instrument.hpp).
// Per family: the argument checks (*_args), one launch (*_launch), the _device entry, the staged
// entry as a list of buffers (rt::Staging) and the variant getter; between them the host builds
// the tests compare against; then the camera rays and the path stages.  DESIGN.md §4.29.

namespace {
// What every caller query launches with: the scene's arrays, the records of its variant, no
// frustum records and no cut.
SceneView query_view(const rt_scene* s, int variant) {
    SceneView v = scene_view(s);
    v.wide = variant == RT_RAYS_VARIANT_WIDE ? 1 : 0;
    v.f_log2 = 2;
    v.ncut = 0;
    return v;
}

// DEEP's brute-force completion reads the triangle array, which only a deep scene keeps.
int deep_has_tris(const rt_scene* s, const char* who) {
    if (s->deep && !s->tri.p) return set_error(RT_ERR_INTERNAL, std::string(who) + ": a deep scene without its triangle array");
    return RT_OK;
}

// One query launch: launch(std::integral_constant<int, variant>) starts the family's kernel of
// that variant; after a launch that succeeded the family's variant word is written, the one scene
// field a query writes (nothing of the frame state: events, work sets, launches).
template <class Launch>
int launch_variant(rt_scene* s, QueryKind kind, int variant, Launch&& launch) {
    if (variant == RT_RAYS_VARIANT_WIDE) launch(std::integral_constant<int, RT_RAYS_VARIANT_WIDE>{});
    else if (variant == RT_RAYS_VARIANT_BINARY) launch(std::integral_constant<int, RT_RAYS_VARIANT_BINARY>{});
    else launch(std::integral_constant<int, RT_RAYS_VARIANT_DEEP>{});
    HIP_TRY(hipGetLastError());
    s->variant[kind].store(variant, std::memory_order_relaxed);
    return RT_OK;
}

int variant_of(const rt_scene* s, QueryKind kind) {
    return s ? s->variant[kind].load(std::memory_order_relaxed) : RT_RAYS_VARIANT_NONE;
}
}  // namespace

// ---- batched ray queries (rt_query.hpp) ----------------------------------------------------
namespace {
// The argument checks of rt_trace_rays[_device]: no HIP call and no read through s before they
// pass (a CPU-only host reaches every one of them).
int trace_rays_args(const rt_scene* s, int mode, const void* rays, const float* max_t, size_t n, int flags,
                    const int32_t* hit_idx, const float* hit_t) {
    if (!s) return set_error(RT_ERR_ARG, "rt_trace_rays: null scene");
    if (mode != RT_RAYS_CLOSEST && mode != RT_RAYS_OCCLUDED) return set_error(RT_ERR_ARG, "rt_trace_rays: unknown mode");
    if (mode == RT_RAYS_CLOSEST && max_t) return set_error(RT_ERR_ARG, "rt_trace_rays: closest-hit queries take no max_t");
    if (mode == RT_RAYS_OCCLUDED && !max_t) return set_error(RT_ERR_ARG, "rt_trace_rays: occlusion queries need max_t");
    if (mode == RT_RAYS_OCCLUDED && hit_t) return set_error(RT_ERR_ARG, "rt_trace_rays: occlusion queries write no hit_t");
    if (flags & ~RT_FLAG_BINARY) return set_error(RT_ERR_ARG, "rt_trace_rays: unknown flag");
    if (n > 0x7FFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, "rt_trace_rays: more than 2^31-1 rays in one batch");
    if (!rays || !hit_idx) return set_error(RT_ERR_ARG, "rt_trace_rays: null rays or hit_idx");
    return RT_OK;
}

// One launch on st.
int trace_rays_launch(rt_scene* s, int mode, const rt_ray* rays, const float* max_t, size_t n, int flags,
                      int32_t* hit_idx, float* hit_t, hipStream_t st) {
    if (const int rc = deep_has_tris(s, "rt_trace_rays"); rc != RT_OK) return rc;
    const int variant = s->query_variant(flags);
    QueryParams Q;
    std::memset(&Q, 0, sizeof(Q));
    Q.sc = query_view(s, variant);  // (the query kernels read none of the shading, frustum and cut arrays)
    Q.rays = reinterpret_cast<const float*>(rays);
    Q.max_t = max_t;
    Q.n = uint32_t(n);
    Q.hit_idx = hit_idx;
    Q.hit_t = hit_t;
    const bool any = mode == RT_RAYS_OCCLUDED;
    const dim3 grid((Q.n + BLOCK - 1) / BLOCK), block(BLOCK);
    return launch_variant(s, kTraceRays, variant, [&](auto V) {
        if (any) hipLaunchKernelGGL((trace_rays_kernel<V(), true>), grid, block, 0, st, Q);
        else hipLaunchKernelGGL((trace_rays_kernel<V(), false>), grid, block, 0, st, Q);
    });
}
}  // namespace

extern "C" int rt_trace_rays_device(rt_scene* s, int mode, const rt_ray* rays, const float* max_t, size_t n, int flags,
                                    int32_t* hit_idx, float* hit_t, void* stream) {
    const int rc = trace_rays_args(s, mode, rays, max_t, n, flags, hit_idx, hit_t);
    if (rc != RT_OK || n == 0) return rc;
    DeviceGuard g(s->device);
    return trace_rays_launch(s, mode, rays, max_t, n, flags, hit_idx, hit_t, static_cast<hipStream_t>(stream));
}

extern "C" int rt_trace_rays(rt_scene* s, int mode, const rt_ray* rays, const float* max_t, size_t n, int flags,
                             int32_t* hit_idx, float* hit_t, float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    const int rc = trace_rays_args(s, mode, rays, max_t, n, flags, hit_idx, hit_t);
    if (rc != RT_OK || n == 0) return rc;
    DeviceGuard g(s->device);
    Staging stage;
    const rt_ray* dr = stage.in(rays, n);
    const float* dm = stage.in(max_t, n);
    int32_t* di = stage.out(hit_idx, n);
    float* dt = stage.out(hit_t, n);
    return stage.run(kernel_ms, [&] { return trace_rays_launch(s, mode, dr, dm, n, flags, di, dt, nullptr); });
}

extern "C" int rt_trace_rays_variant(const rt_scene* s) {
    return variant_of(s, kTraceRays);
}

// ---- radiance queries (rt_query.hpp, shade_rays_kernel) ----------------------------------------
extern "C" void rt_shade_opts_default(rt_shade_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->max_depth = 1;
    o->diffuse_bounce = 1;
}

namespace {
// As trace_rays_args: no HIP call and no read through s before the checks pass.
int shade_rays_args(const rt_scene* s, const void* rays, size_t n, const rt_shade_opts* opt, const float* radiance) {
    if (!s) return set_error(RT_ERR_ARG, "rt_shade_rays: null scene");
    if (!opt) return set_error(RT_ERR_ARG, "rt_shade_rays: null opts");
    if (opt->flags & ~RT_FLAG_BINARY) return set_error(RT_ERR_ARG, "rt_shade_rays: unknown flag");
    if (n > 0x7FFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, "rt_shade_rays: more than 2^31-1 rays in one batch");
    if (!rays || !radiance) return set_error(RT_ERR_ARG, "rt_shade_rays: null rays or radiance");
    return RT_OK;
}

// One launch on st.
int shade_rays_launch(rt_scene* s, const rt_ray* rays, const uint32_t* seeds, size_t n, const rt_shade_opts& opt,
                      float* radiance, int32_t* hit_idx, float* hit_t, hipStream_t st) {
    if (const int rc = deep_has_tris(s, "rt_shade_rays"); rc != RT_OK) return rc;
    const int variant = s->query_variant(opt.flags);
    ShadeParams S;
    std::memset(&S, 0, sizeof(S));
    S.sc = query_view(s, variant);  // (the packed records and the shading tables; no frustum or cut array is read)
    S.rays = reinterpret_cast<const float*>(rays);
    S.seeds = seeds;
    S.n = uint32_t(n);
    S.max_depth = opt.max_depth;
    S.diffuse_bounce = opt.diffuse_bounce;
    S.miss = mk(opt.miss_color.x, opt.miss_color.y, opt.miss_color.z);
    S.radiance = radiance;
    S.hit_idx = hit_idx;
    S.hit_t = hit_t;
    const dim3 grid((S.n + BLOCK - 1) / BLOCK), block(BLOCK);
    return launch_variant(s, kShadeRays, variant,
                          [&](auto V) { hipLaunchKernelGGL((shade_rays_kernel<V()>), grid, block, 0, st, S); });
}
}  // namespace

extern "C" int rt_shade_rays_device(rt_scene* s, const rt_ray* rays, const uint32_t* seeds, size_t n,
                                    const rt_shade_opts* opt, float* radiance, int32_t* hit_idx, float* hit_t,
                                    void* stream) {
    const int rc = shade_rays_args(s, rays, n, opt, radiance);
    if (rc != RT_OK || n == 0) return rc;
    DeviceGuard g(s->device);
    return shade_rays_launch(s, rays, seeds, n, *opt, radiance, hit_idx, hit_t, static_cast<hipStream_t>(stream));
}

extern "C" int rt_shade_rays(rt_scene* s, const rt_ray* rays, const uint32_t* seeds, size_t n, const rt_shade_opts* opt,
                             float* radiance, int32_t* hit_idx, float* hit_t, float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    const int rc = shade_rays_args(s, rays, n, opt, radiance);
    if (rc != RT_OK || n == 0) return rc;
    DeviceGuard g(s->device);
    Staging stage;
    const rt_ray* dr = stage.in(rays, n);
    const uint32_t* ds = stage.in(seeds, n);
    float* dc = stage.out(radiance, 3 * n);
    int32_t* di = stage.out(hit_idx, n);
    float* dt = stage.out(hit_t, n);
    return stage.run(kernel_ms, [&] { return shade_rays_launch(s, dr, ds, n, *opt, dc, di, dt, nullptr); });
}

extern "C" int rt_shade_rays_variant(const rt_scene* s) {
    return variant_of(s, kShadeRays);
}

// ---- hit records (rt_query.hpp, trace_hits_kernel) ---------------------------------------------
static_assert(sizeof(rt_hit) == 64 && sizeof(HitWords) == sizeof(rt_hit), "rt_hit is four 16-byte words");

namespace {
// As trace_rays_args: no HIP call and no read through s before the checks pass.
int trace_hits_args(const rt_scene* s, const void* rays, size_t n, int flags, const rt_hit* hits) {
    if (!s) return set_error(RT_ERR_ARG, "rt_trace_hits: null scene");
    if (flags & ~RT_FLAG_BINARY) return set_error(RT_ERR_ARG, "rt_trace_hits: unknown flag");
    if (n > 0x7FFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, "rt_trace_hits: more than 2^31-1 rays in one batch");
    if (!rays || !hits) return set_error(RT_ERR_ARG, "rt_trace_hits: null rays or hits");
    return RT_OK;
}

// One launch on st.
int trace_hits_launch(rt_scene* s, const rt_ray* rays, size_t n, int flags, rt_hit* hits, hipStream_t st) {
    if (const int rc = deep_has_tris(s, "rt_trace_hits"); rc != RT_OK) return rc;
    const int variant = s->query_variant(flags);
    HitsParams Q;
    std::memset(&Q, 0, sizeof(Q));
    Q.sc = query_view(s, variant);  // (the packed records, tnorm, objids and the material table's bounds)
    Q.rays = reinterpret_cast<const float*>(rays);
    Q.n = uint32_t(n);
    Q.hits = reinterpret_cast<uint4*>(hits);
    const dim3 grid((Q.n + BLOCK - 1) / BLOCK), block(BLOCK);
    return launch_variant(s, kTraceHits, variant,
                          [&](auto V) { hipLaunchKernelGGL((trace_hits_kernel<V()>), grid, block, 0, st, Q); });
}
}  // namespace

extern "C" int rt_trace_hits_device(rt_scene* s, const rt_ray* rays, size_t n, int flags, rt_hit* hits, void* stream) {
    const int rc = trace_hits_args(s, rays, n, flags, hits);
    if (rc != RT_OK) return rc;
    // the kernel stores 16-byte words
    if (reinterpret_cast<uintptr_t>(hits) % 16 != 0) return set_error(RT_ERR_ARG, "rt_trace_hits_device: hits_dev is not 16-byte aligned");
    if (n == 0) return RT_OK;
    DeviceGuard g(s->device);
    return trace_hits_launch(s, rays, n, flags, hits, static_cast<hipStream_t>(stream));
}

extern "C" int rt_trace_hits(rt_scene* s, const rt_ray* rays, size_t n, int flags, rt_hit* hits, float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    const int rc = trace_hits_args(s, rays, n, flags, hits);
    if (rc != RT_OK || n == 0) return rc;
    DeviceGuard g(s->device);
    Staging stage;
    const rt_ray* dr = stage.in(rays, n);
    rt_hit* dh = stage.out(hits, n);
    return stage.run(kernel_ms, [&] { return trace_hits_launch(s, dr, n, flags, dh, nullptr); });
}

extern "C" int rt_trace_hits_variant(const rt_scene* s) {
    return variant_of(s, kTraceHits);
}

// The host build of the record: intersectTriangle(ray_i, tris[i], 1e-4f, FLT_MAX) through mt_g and
// hit_record, the functions trace_hits_kernel runs.
extern "C" int rt_hit_record_host(const rt_ray* rays, const rt_triangle* tris, int n, rt_hit* out) {
    if (n < 0 || (n > 0 && (!rays || !tris || !out))) return set_error(RT_ERR_ARG, "rt_hit_record_host: bad args");
    for (int i = 0; i < n; ++i) {
        const rt_ray& q = rays[i];
        const rt_triangle& T = tris[i];
        const RayPre r = make_ray_mt(mk(q.origin.x, q.origin.y, q.origin.z), mk(q.direction.x, q.direction.y, q.direction.z));
        const f3 v0 = mk(T.v0.x, T.v0.y, T.v0.z);
        const f3 e1 = sub(mk(T.v1.x, T.v1.y, T.v1.z), v0), e2 = sub(mk(T.v2.x, T.v2.y, T.v2.z), v0);
        float t = 0.f, u = 0.f, v = 0.f;
        HitWords h = miss_record();
        if (mt_g(r, v0, e1, e2, kRayTMin, FLT_MAX, t, u, v))
            h = hit_record(r, e1, e2, mk(T.n0.x, T.n0.y, T.n0.z), mk(T.n1.x, T.n1.y, T.n1.z), mk(T.n2.x, T.n2.y, T.n2.z), t, u,
                           v, i, -1, -1);
        std::memcpy(&out[i], &h, sizeof(rt_hit));
    }
    return RT_OK;
}

// ---- multi-hit queries (rt_multihit.hpp, multi_hit_kernel) --------------------------------------
static_assert(sizeof(rt_multi_hit) == 16, "rt_multi_hit is one 16-byte word");
static_assert(mh_class(RT_MULTI_HIT_MAX_K) == RT_MULTI_HIT_MAX_K, "the largest k class is RT_MULTI_HIT_MAX_K");

namespace {
// As trace_rays_args: no HIP call and no read through s before the checks pass.
int multi_hits_args(const rt_scene* s, const void* rays, size_t n, int k, int flags, const rt_multi_hit* hits,
                    const int32_t* count) {
    if (!s) return set_error(RT_ERR_ARG, "rt_trace_multi_hits: null scene");
    if (k < 0 || k > RT_MULTI_HIT_MAX_K) return set_error(RT_ERR_ARG, "rt_trace_multi_hits: k outside 0..RT_MULTI_HIT_MAX_K");
    if (flags & ~RT_FLAG_BINARY) return set_error(RT_ERR_ARG, "rt_trace_multi_hits: unknown flag");
    if (!rays) return set_error(RT_ERR_ARG, "rt_trace_multi_hits: null rays");
    if (k > 0 && !hits) return set_error(RT_ERR_ARG, "rt_trace_multi_hits: null hits with k > 0");
    if (k == 0 && !count) return set_error(RT_ERR_ARG, "rt_trace_multi_hits: k == 0 and a null count: no output");
    if (n > 0x7FFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, "rt_trace_multi_hits: more than 2^31-1 rays in one batch");
    if ((unsigned long long)n * (unsigned long long)k > 0x7FFFFFFFull)
        return set_error(RT_ERR_UNSUPPORTED, "rt_trace_multi_hits: more than 2^31-1 records (n * k) in one batch");
    return RT_OK;
}

// One launch on st.
int multi_hits_launch(rt_scene* s, const rt_ray* rays, const float* max_t, size_t n, int k, int flags, rt_multi_hit* hits,
                      int32_t* count, hipStream_t st) {
    if (const int rc = deep_has_tris(s, "rt_trace_multi_hits"); rc != RT_OK) return rc;
    const int variant = s->query_variant(flags);
    MultiHitParams Q;
    std::memset(&Q, 0, sizeof(Q));
    Q.sc = query_view(s, variant);  // (the packed records; DEEP's completion reads the triangle array)
    Q.rays = reinterpret_cast<const float*>(rays);
    Q.max_t = max_t;
    Q.n = uint32_t(n);
    Q.k = k;
    Q.hits = k > 0 ? reinterpret_cast<uint4*>(hits) : nullptr;
    Q.count = count;
    const int kc = mh_class(Q.k);
    const dim3 block(mh_block(kc)), grid((Q.n + block.x - 1) / block.x);
    return launch_variant(s, kMultiHits, variant, [&](auto V) {
        if (kc == 0) hipLaunchKernelGGL((multi_hit_kernel<V(), 0>), grid, block, 0, st, Q);
        else if (kc == 4) hipLaunchKernelGGL((multi_hit_kernel<V(), 4>), grid, block, 0, st, Q);
        else if (kc == 8) hipLaunchKernelGGL((multi_hit_kernel<V(), 8>), grid, block, 0, st, Q);
        else if (kc == 16) hipLaunchKernelGGL((multi_hit_kernel<V(), 16>), grid, block, 0, st, Q);
        else hipLaunchKernelGGL((multi_hit_kernel<V(), 32>), grid, block, 0, st, Q);
    });
}
}  // namespace

extern "C" int rt_trace_multi_hits_device(rt_scene* s, const rt_ray* rays, const float* max_t, size_t n, int k, int flags,
                                          rt_multi_hit* hits, int32_t* count, void* stream) {
    const int rc = multi_hits_args(s, rays, n, k, flags, hits, count);
    if (rc != RT_OK) return rc;
    // the kernel stores 16-byte words
    if (k > 0 && reinterpret_cast<uintptr_t>(hits) % 16 != 0)
        return set_error(RT_ERR_ARG, "rt_trace_multi_hits_device: hits_dev is not 16-byte aligned");
    if (n == 0) return RT_OK;
    DeviceGuard g(s->device);
    return multi_hits_launch(s, rays, max_t, n, k, flags, hits, count, static_cast<hipStream_t>(stream));
}

extern "C" int rt_trace_multi_hits(rt_scene* s, const rt_ray* rays, const float* max_t, size_t n, int k, int flags,
                                   rt_multi_hit* hits, int32_t* count, float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    const int rc = multi_hits_args(s, rays, n, k, flags, hits, count);
    if (rc != RT_OK || n == 0) return rc;
    DeviceGuard g(s->device);
    Staging stage;
    const rt_ray* dr = stage.in(rays, n);
    const float* dm = stage.in(max_t, n);
    rt_multi_hit* dh = stage.out(k > 0 ? hits : nullptr, n * size_t(k));  // (k == 0 keeps no list, whatever hits is)
    int32_t* dc = stage.out(count, n);
    return stage.run(kernel_ms, [&] { return multi_hits_launch(s, dr, dm, n, k, flags, dh, dc, nullptr); });
}

extern "C" int rt_trace_multi_hits_variant(const rt_scene* s) {
    return variant_of(s, kMultiHits);
}

// The host build of the query on arrays in the reference layout: SearchBVH's control flow with the
// bound fixed at tmax (512-entry stack, overflow flag, brute-force completion), through box_hit and
// mt_g, the functions the kernel runs; the list is a sort of everything collected.
extern "C" int rt_multi_hits_host(size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs, const rt_triangle* tris,
                                  const rt_ray* rays, const float* max_t, size_t n, int k, rt_multi_hit* hits,
                                  int32_t* count) {
    if (k < 0 || k > RT_MULTI_HIT_MAX_K) return set_error(RT_ERR_ARG, "rt_multi_hits_host: k outside 0..RT_MULTI_HIT_MAX_K");
    if (P == 0 || P > 0x7FFFFFFFull || !nodes || !aabbs || !tris) return set_error(RT_ERR_ARG, "rt_multi_hits_host: null or empty scene arrays");
    if (n > 0 && !rays) return set_error(RT_ERR_ARG, "rt_multi_hits_host: null rays");
    if (k > 0 && !hits) return set_error(RT_ERR_ARG, "rt_multi_hits_host: null hits with k > 0");
    if (k == 0 && !count) return set_error(RT_ERR_ARG, "rt_multi_hits_host: k == 0 and a null count: no output");
    if (n > 0x7FFFFFFFull || (unsigned long long)n * (unsigned long long)k > 0x7FFFFFFFull)
        return set_error(RT_ERR_UNSUPPORTED, "rt_multi_hits_host: more than 2^31-1 rays or records");
    const size_t nn = 2 * P - 1;
    // make_ray's bound of |coordinate| over every box (inf when a box is not finite: every test of
    // every ray is then decided in double)
    float bm[3] = {0.f, 0.f, 0.f};
    for (size_t i = 0; i < nn; ++i) {
        const float c[6] = {aabbs[i].min_corner.x, aabbs[i].min_corner.y, aabbs[i].min_corner.z,
                            aabbs[i].max_corner.x, aabbs[i].max_corner.y, aabbs[i].max_corner.z};
        for (int a = 0; a < 6; ++a) bm[a % 3] = std::isfinite(c[a]) ? fmaxf(bm[a % 3], fabsf(c[a])) : INFINITY;
    }
    for (size_t i = 0; i < nn; ++i) {
        if (nodes[i].object_idx != NO_REF) continue;
        if ((nodes[i].left_idx != NO_REF && nodes[i].left_idx >= nn) || (nodes[i].right_idx != NO_REF && nodes[i].right_idx >= nn))
            return set_error(RT_ERR_ARG, "rt_multi_hits_host: a child index outside the node array");
    }
    auto box_of = [&](uint32_t i) {
        const rt_aabb& b = aabbs[i];
        return BoxP{(v2f){b.min_corner.x, b.max_corner.x}, (v2f){b.min_corner.y, b.max_corner.y},
                    (v2f){b.min_corner.z, b.max_corner.z}};
    };
    struct Found {
        uint32_t tb;  // t's bits: the order of the floats for the t >= 1e-4 that are accepted
        int32_t tri;
        float u, v;
    };
    std::vector<Found> found;
    std::vector<uint32_t> stack(REF_STACK);
    for (size_t i = 0; i < n; ++i) {
        const rt_ray& q = rays[i];
        const RayPre r = make_ray(mk(q.origin.x, q.origin.y, q.origin.z), mk(q.direction.x, q.direction.y, q.direction.z),
                                  mk(bm[0], bm[1], bm[2]));
        const float tmax = max_t ? max_t[i] : FLT_MAX;
        auto test = [&](uint32_t tri) {
            const rt_triangle& T = tris[tri];
            const f3 v0 = mk(T.v0.x, T.v0.y, T.v0.z);
            const f3 e1 = sub(mk(T.v1.x, T.v1.y, T.v1.z), v0), e2 = sub(mk(T.v2.x, T.v2.y, T.v2.z), v0);
            float t, u, v;
            if (mt_g(r, v0, e1, e2, kRayTMin, tmax, t, u, v)) found.push_back(Found{pw::asu(t), (int32_t)tri, u, v});
        };
        found.clear();
        int sp = 0;
        bool overflow = false;
        size_t pops = 0;
        stack[sp++] = 0;
        while (sp > 0) {
            const uint32_t ni = stack[--sp];
            if (++pops > nn) return set_error(RT_ERR_ARG, "rt_multi_hits_host: the nodes are not a tree");
            if (!box_hit(r, box_of(ni), kRayTMin, tmax)) continue;
            const rt_bvh_node& nd = nodes[ni];
            if (nd.object_idx != NO_REF) {
                if (nd.object_idx < P) test(nd.object_idx);
                continue;
            }
            for (const uint32_t ch : {nd.left_idx, nd.right_idx}) {
                if (ch == NO_REF || !box_hit(r, box_of(ch), kRayTMin, tmax)) continue;
                if (sp < REF_STACK) stack[sp++] = ch;
                else overflow = true;
            }
        }
        if (overflow) {
            found.clear();
            for (size_t t = 0; t < P; ++t) test((uint32_t)t);
        }
        std::sort(found.begin(), found.end(),
                  [](const Found& a, const Found& b) { return a.tb != b.tb ? a.tb < b.tb : a.tri < b.tri; });
        if (count) count[i] = (int32_t)found.size();
        for (int j = 0; j < k; ++j) {
            rt_multi_hit h = {-1, -1.0f, 0.0f, 0.0f};
            if ((size_t)j < found.size()) h = {found[j].tri, pw::asf(found[j].tb), found[j].u, found[j].v};
            std::memcpy(&hits[i * size_t(k) + j], &h, sizeof(h));
        }
    }
    return RT_OK;
}

// ---- closest-point queries (rt_closest.hpp, closest_points_kernel) ------------------------------
static_assert(sizeof(rt_point_hit) == 32, "rt_point_hit is two 16-byte words");

namespace {
// As multi_hits_args: no HIP call and no read through s before the checks pass.
int closest_args(const rt_scene* s, const float* points, const float* max_d2, size_t n, int flags, const rt_point_hit* hits,
                 const uint32_t* evals) {
    if (!s) return set_error(RT_ERR_ARG, "rt_closest_points: null scene");
    if (flags & ~RT_FLAG_BINARY) return set_error(RT_ERR_ARG, "rt_closest_points: unknown flag");
    if (!points) return set_error(RT_ERR_ARG, "rt_closest_points: null points");
    if (!hits) return set_error(RT_ERR_ARG, "rt_closest_points: null hits");
    if (reinterpret_cast<uintptr_t>(points) % 4 != 0 || reinterpret_cast<uintptr_t>(max_d2) % 4 != 0 ||
        reinterpret_cast<uintptr_t>(evals) % 4 != 0)
        return set_error(RT_ERR_ARG, "rt_closest_points: points, max_d2 or evals is not 4-byte aligned");
    if (n > 0x7FFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, "rt_closest_points: more than 2^31-1 points in one batch");
    return RT_OK;
}

// One launch on st.
int closest_launch(rt_scene* s, const float* points, const float* max_d2, size_t n, int flags, rt_point_hit* hits,
                   uint32_t* evals, hipStream_t st) {
    // (no deep_has_tris: closest_complete, DEEP's completion here, reads the leaf records, not the triangle array)
    const int variant = s->query_variant(flags);
    ClosestParams Q;
    std::memset(&Q, 0, sizeof(Q));
    Q.sc = query_view(s, variant);
    Q.points = points;
    Q.max_d2 = max_d2;
    Q.n = uint32_t(n);
    // The leaf array keeps one zeroed record when no leaf names a triangle; the root is then a
    // leaf that names none, which pack_bounds marks with the empty root box.
    const bool no_leaf = (s->root_ref & LEAF_BIT) && s->root_box[0] > s->root_box[3];
    Q.n_leaf = no_leaf ? 0u : uint32_t(s->leaf.n / (4 * sizeof(float4)));
    Q.hits = reinterpret_cast<uint4*>(hits);
    Q.evals = evals;
    const dim3 block(BLOCK), grid((Q.n + BLOCK - 1) / BLOCK);
    return launch_variant(s, kClosestPoints, variant,
                          [&](auto V) { hipLaunchKernelGGL((closest_points_kernel<V()>), grid, block, 0, st, Q); });
}
}  // namespace

extern "C" int rt_closest_points_device(rt_scene* s, const float* points, const float* max_d2, size_t n, int flags,
                                        rt_point_hit* hits, uint32_t* evals, void* stream) {
    const int rc = closest_args(s, points, max_d2, n, flags, hits, evals);
    if (rc != RT_OK) return rc;
    // the kernel stores 16-byte words
    if (reinterpret_cast<uintptr_t>(hits) % 16 != 0)
        return set_error(RT_ERR_ARG, "rt_closest_points_device: hits_dev is not 16-byte aligned");
    if (n == 0) return RT_OK;
    DeviceGuard g(s->device);
    return closest_launch(s, points, max_d2, n, flags, hits, evals, static_cast<hipStream_t>(stream));
}

extern "C" int rt_closest_points(rt_scene* s, const float* points, const float* max_d2, size_t n, int flags,
                                 rt_point_hit* hits, uint32_t* evals, float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    const int rc = closest_args(s, points, max_d2, n, flags, hits, evals);
    if (rc != RT_OK || n == 0) return rc;
    DeviceGuard g(s->device);
    Staging stage;
    const float* dp = stage.in(points, 3 * n);
    const float* dm = stage.in(max_d2, n);
    rt_point_hit* dh = stage.out(hits, n);
    uint32_t* de = stage.out(evals, n);
    return stage.run(kernel_ms, [&] { return closest_launch(s, dp, dm, n, flags, dh, de, nullptr); });
}

extern "C" int rt_closest_points_variant(const rt_scene* s) {
    return variant_of(s, kClosestPoints);
}

// The host build of the query on arrays in the reference layout, and its definition: every leaf
// in index order through cp_triangle and cp_wins, the functions the kernel runs.  No tree walk.
extern "C" int rt_closest_points_host(size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs, const rt_triangle* tris,
                                      const float* points, const float* max_d2, size_t n, rt_point_hit* hits,
                                      uint32_t* evals) {
    if (P == 0 || P > 0x7FFFFFFFull || !nodes || !aabbs || !tris)
        return set_error(RT_ERR_ARG, "rt_closest_points_host: null or empty scene arrays");
    if (n > 0 && (!points || !hits)) return set_error(RT_ERR_ARG, "rt_closest_points_host: null points or hits");
    if (n > 0x7FFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, "rt_closest_points_host: more than 2^31-1 points");
    struct Leaf {
        f3 a, e1, e2;
        BoxP box;
        int32_t tri;
    };
    std::vector<Leaf> leaves;
    for (size_t j = P - 1; j < 2 * P - 1; ++j) {
        if (nodes[j].object_idx >= P) continue;  // names no triangle: contributes nothing
        const rt_triangle& T = tris[nodes[j].object_idx];
        const rt_aabb& b = aabbs[j];
        const f3 v0 = mk(T.v0.x, T.v0.y, T.v0.z);
        leaves.push_back(Leaf{v0, sub(mk(T.v1.x, T.v1.y, T.v1.z), v0), sub(mk(T.v2.x, T.v2.y, T.v2.z), v0),
                              BoxP{(v2f){b.min_corner.x, b.max_corner.x}, (v2f){b.min_corner.y, b.max_corner.y},
                                   (v2f){b.min_corner.z, b.max_corner.z}},
                              int32_t(nodes[j].object_idx)});
    }
    for (size_t i = 0; i < n; ++i) {
        const f3 q = mk(points[3 * i], points[3 * i + 1], points[3 * i + 2]);
        CpHit best = cp_start(max_d2 ? max_d2[i] : INFINITY);
        for (const Leaf& L : leaves) {
            const CpHit c = cp_triangle(q, L.a, L.e1, L.e2, L.box, L.tri);
            if (cp_wins(c, best)) best = c;
        }
        rt_point_hit h = {-1, -1.0f, {0.0f, 0.0f, 0.0f}, 0.0f, 0.0f, -1};
        if (best.region >= 0) h = {best.tri, best.D, {best.p.x, best.p.y, best.p.z}, best.v, best.w, best.region};
        std::memcpy(&hits[i], &h, sizeof(h));
        if (evals) evals[i] = uint32_t(leaves.size());
    }
    return RT_OK;
}

// ---- camera rays (rt_query.hpp, camera_rays_kernel) --------------------------------------------
namespace {
// The checks of rt_camera_rays[_pass]_host / _device: no HIP call before they pass.  spp: the
// samples of this call, [sample0, sample0 + spp) of the frame's.  *n_out: W * rows * spp.
int camera_rays_args(const rt_camera* cam, int sample0, int spp, int row0, int rows, const void* rays, size_t* n_out) {
    if (!cam || !rays) return set_error(RT_ERR_ARG, "rt_camera_rays: null camera or rays");
    if (spp < 1) return set_error(RT_ERR_ARG, "rt_camera_rays: spp < 1");
    if (sample0 < 0 || sample0 > INT32_MAX - spp) return set_error(RT_ERR_ARG, "rt_camera_rays: sample0 < 0 or past 2^31-1");
    const int W = cam->pixel_width, H = cam->pixel_height;
    if (W < 1 || H < 1) return set_error(RT_ERR_ARG, "rt_camera_rays: an empty image");
    if (row0 < 0 || rows < 0 || row0 > H || rows > H - row0) return set_error(RT_ERR_ARG, "rt_camera_rays: rows outside the image");
    const unsigned long long n = (unsigned long long)W * (unsigned long long)rows * (unsigned long long)spp;
    if (n > 0x7FFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, "rt_camera_rays: more than 2^31-1 rays in one call");
    *n_out = size_t(n);
    return RT_OK;
}
}  // namespace

extern "C" int rt_camera_rays_pass_host(const rt_camera* cam, int sample0, int spp, const float* jitter, int row0,
                                        int rows, rt_ray* rays, uint32_t* seeds) {
    size_t n = 0;
    int rc = camera_rays_args(cam, sample0, spp, row0, rows, rays, &n);
    if (rc != RT_OK) return rc;
    // (the default table is a whole frame's: a later slice of it is the caller's to cut)
    if (!jitter && sample0 != 0) return set_error(RT_ERR_ARG, "rt_camera_rays_pass_host: null jitter with sample0 > 0");
    if (n == 0) return RT_OK;
    std::vector<float> tab;
    if (!jitter) {
        tab.resize(size_t(2) * size_t(spp));
        if ((rc = rt_jittered_samples(spp, 42u, 1, tab.data())) != RT_OK) return rc;
        jitter = tab.data();
    }
    const f3 center = mk(cam->center.x, cam->center.y, cam->center.z);
    const f3 p00 = mk(cam->pixel00_loc.x, cam->pixel00_loc.y, cam->pixel00_loc.z);
    const f3 du = mk(cam->pixel_delta_u.x, cam->pixel_delta_u.y, cam->pixel_delta_u.z);
    const f3 dv = mk(cam->pixel_delta_v.x, cam->pixel_delta_v.y, cam->pixel_delta_v.z);
    const int W = cam->pixel_width;
    size_t i = 0;
    for (int y = row0; y < row0 + rows; ++y)
        for (int x = 0; x < W; ++x)
            for (int s = 0; s < spp; ++s, ++i) {
                const f3 d = camera_dir(center, p00, du, dv, x, y, jitter[2 * s], jitter[2 * s + 1]);
                rays[i].origin = cam->center;
                rays[i].direction = rt_vec3{d.x, d.y, d.z};
                if (seeds) seeds[i] = make_rng_seed(x, y, sample0 + s);
            }
    return RT_OK;
}

extern "C" int rt_camera_rays_host(const rt_camera* cam, int spp, const float* jitter, int row0, int rows, rt_ray* rays,
                                   uint32_t* seeds) {
    return rt_camera_rays_pass_host(cam, 0, spp, jitter, row0, rows, rays, seeds);
}

extern "C" int rt_camera_rays_pass_device(int device, const rt_camera* cam, int sample0, int spp, const float* jitter,
                                          int row0, int rows, rt_ray* rays, uint32_t* seeds, void* stream) {
    size_t n = 0;
    int rc = camera_rays_args(cam, sample0, spp, row0, rows, rays, &n);
    if (rc != RT_OK) return rc;
    if (!jitter) return set_error(RT_ERR_ARG, "rt_camera_rays_device: null jitter table");
    if (n == 0) return RT_OK;
    if ((rc = check_device(device)) != RT_OK) return rc;
    DeviceGuard g(device);
    CameraRaysParams P;
    std::memset(&P, 0, sizeof(P));
    P.center = mk(cam->center.x, cam->center.y, cam->center.z);
    P.p00 = mk(cam->pixel00_loc.x, cam->pixel00_loc.y, cam->pixel00_loc.z);
    P.du = mk(cam->pixel_delta_u.x, cam->pixel_delta_u.y, cam->pixel_delta_u.z);
    P.dv = mk(cam->pixel_delta_v.x, cam->pixel_delta_v.y, cam->pixel_delta_v.z);
    P.W = cam->pixel_width;
    P.spp = spp;
    P.row0 = row0;
    P.sample0 = sample0;
    P.n = uint32_t(n);
    P.jitter = jitter;
    P.rays = reinterpret_cast<float*>(rays);
    P.seeds = seeds;
    hipLaunchKernelGGL(camera_rays_kernel, dim3((P.n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), P);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

extern "C" int rt_camera_rays_device(int device, const rt_camera* cam, int spp, const float* jitter, int row0, int rows,
                                     rt_ray* rays, uint32_t* seeds, void* stream) {
    return rt_camera_rays_pass_device(device, cam, 0, spp, jitter, row0, rows, rays, seeds, stream);
}

// ---- path stages (rt_path.hpp) -------------------------------------------------------------------
static_assert(sizeof(DevMaterial) == sizeof(rt_material) && sizeof(DevLight) == sizeof(rt_light), "reference layouts");
static_assert(PATH_NONE == RT_PATH_NONE, "RT_PATH_NONE");

extern "C" void rt_path_opts_default(rt_path_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->diffuse_bounce = 1;
}

namespace {
// The checks the device and the host form of the step share: no HIP call and no read through any
// pointer but opt and st before they pass.
int path_step_args(const char* who, size_t m, const void* rays, const void* hits, const rt_path_opts* opt,
                   const rt_path_state* st, const void* next, const void* alive, int known_flags) {
    if (!opt) return set_error(RT_ERR_ARG, std::string(who) + ": null opts");
    if (opt->flags & ~known_flags) return set_error(RT_ERR_ARG, std::string(who) + ": unknown flag");
    if (m > 0x7FFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31-1 entries in one batch");
    if (!rays || !hits) return set_error(RT_ERR_ARG, std::string(who) + ": null rays or hits");
    if (!st || !st->radiance || !st->throughput || !st->rng) return set_error(RT_ERR_ARG, std::string(who) + ": null state");
    if (!(opt->flags & RT_PATH_LAST) && (!next || !alive))
        return set_error(RT_ERR_ARG, std::string(who) + ": next_rays and alive are required unless RT_PATH_LAST is set");
    return RT_OK;
}

int path_state_args(const char* who, size_t n, const rt_path_state* st) {
    if (!st || !st->radiance || !st->throughput || !st->rng) return set_error(RT_ERR_ARG, std::string(who) + ": null state");
    if (n > 0x7FFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31-1 paths");
    return RT_OK;
}

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && na && nb && x < y + nb && y < x + na;
}

}  // namespace

extern "C" int rt_path_begin_device(int device, size_t n, const uint32_t* seeds, const rt_path_state* state, void* stream) {
    int rc = path_state_args("rt_path_begin_device", n, state);
    if (rc != RT_OK || n == 0) return rc;
    if ((rc = check_device(device)) != RT_OK) return rc;
    DeviceGuard g(device);
    PathBeginParams P;
    std::memset(&P, 0, sizeof(P));
    P.seeds = seeds;
    P.n = uint32_t(n);
    P.radiance = state->radiance;
    P.throughput = state->throughput;
    P.rng = state->rng;
    hipLaunchKernelGGL(path_begin_kernel, dim3((P.n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), P);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

extern "C" int rt_path_finish_device(int device, size_t n, float* radiance, void* stream) {
    if (!radiance) return set_error(RT_ERR_ARG, "rt_path_finish_device: null radiance");
    if (n > 0x7FFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, "rt_path_finish_device: more than 2^31-1 paths");
    if (n == 0) return RT_OK;
    int rc = check_device(device);
    if (rc != RT_OK) return rc;
    DeviceGuard g(device);
    hipLaunchKernelGGL(path_finish_kernel, dim3((uint32_t(n) + BLOCK - 1) / BLOCK), dim3(BLOCK), 0,
                       static_cast<hipStream_t>(stream), radiance, uint32_t(n));
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

extern "C" int rt_path_step_device(rt_scene* s, size_t m, const rt_ray* rays, const rt_hit* hits, const rt_material* mats,
                                   const uint32_t* ids, const rt_path_opts* opt, const rt_path_state* state, rt_ray* next,
                                   uint8_t* alive, float* direct, void* stream) {
    if (!s) return set_error(RT_ERR_ARG, "rt_path_step_device: null scene");
    int rc = path_step_args("rt_path_step_device", m, rays, hits, opt, state, next, alive, RT_FLAG_BINARY | RT_PATH_LAST);
    if (rc != RT_OK) return rc;
    // the kernel loads 16-byte words
    if (reinterpret_cast<uintptr_t>(hits) % 16 != 0) return set_error(RT_ERR_ARG, "rt_path_step_device: hits_dev is not 16-byte aligned");
    if (m == 0) return RT_OK;
    DeviceGuard g(s->device);
    if ((rc = deep_has_tris(s, "rt_path_step_device")) != RT_OK) return rc;
    const int variant = s->query_variant(opt->flags);  // (RT_PATH_LAST is not a bit the rule reads)
    PathStepParams P;
    std::memset(&P, 0, sizeof(P));
    P.sc = query_view(s, variant);  // (the packed records of the shadow rays and the shading tables)
    P.rays = reinterpret_cast<const float*>(rays);
    P.hits = reinterpret_cast<const uint4*>(hits);
    P.mats = reinterpret_cast<const float*>(mats);
    P.ids = ids;
    P.m = uint32_t(m);
    P.diffuse_bounce = opt->diffuse_bounce;
    P.last = (opt->flags & RT_PATH_LAST) ? 1 : 0;
    P.miss = mk(opt->miss_color.x, opt->miss_color.y, opt->miss_color.z);
    P.radiance = state->radiance;
    P.throughput = state->throughput;
    P.rng = state->rng;
    P.next = P.last && !next ? nullptr : reinterpret_cast<float*>(next);
    P.alive = alive;
    P.direct = direct;
    const dim3 grid((P.m + BLOCK - 1) / BLOCK), block(BLOCK);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return launch_variant(s, kPathStep, variant,
                          [&](auto V) { hipLaunchKernelGGL((path_step_kernel<V()>), grid, block, 0, st, P); });
}

extern "C" int rt_path_step_variant(const rt_scene* s) {
    return variant_of(s, kPathStep);
}

// The host build of the step: path_step_one as path_step_kernel runs it, the shadow rays' answers
// read from `occluded`.
extern "C" int rt_path_step_host(size_t m, const rt_ray* rays, const rt_hit* hits, const rt_material* mats,
                                 const uint32_t* ids, const rt_material* table, int num_table, const rt_light* lights,
                                 int num_lights, const uint8_t* occluded, const rt_path_opts* opt, const rt_path_state* state,
                                 rt_ray* next, uint8_t* alive, float* direct) {
    const int rc = path_step_args("rt_path_step_host", m, rays, hits, opt, state, next, alive, RT_FLAG_BINARY | RT_PATH_LAST);
    if (rc != RT_OK) return rc;
    if (num_table < 0 || num_lights < 0 || (num_table > 0 && !table) || (num_lights > 0 && (!lights || !occluded)))
        return set_error(RT_ERR_ARG, "rt_path_step_host: a table, light set or occlusion array that does not match its count");
    const bool last = (opt->flags & RT_PATH_LAST) != 0;
    const f3 miss = mk(opt->miss_color.x, opt->miss_color.y, opt->miss_color.z);
    for (size_t k = 0; k < m; ++k) {
        const float* R = reinterpret_cast<const float*>(rays + k);
        float* nx = next ? reinterpret_cast<float*>(next + k) : nullptr;
        const uint32_t id = ids ? ids[k] : uint32_t(k);
        if (id == PATH_NONE) {
            if (nx) std::memmove(nx, R, sizeof(rt_ray));
            if (alive) alive[k] = 0;
            if (direct) direct[3 * k] = direct[3 * k + 1] = direct[3 * k + 2] = 0.0f;
            continue;
        }
        HitWords h;  // (the caller's records need no alignment)
        std::memcpy(&h, hits + k, sizeof(h));
        path_step_one(R, h.w, mats ? reinterpret_cast<const float*>(mats + k) : nullptr,
                      reinterpret_cast<const DevMaterial*>(table), num_table, reinterpret_cast<const DevLight*>(lights),
                      num_lights, miss, opt->diffuse_bounce != 0, last, state->radiance + 3 * size_t(id),
                      state->throughput + 3 * size_t(id), state->rng + id, nx, alive ? alive + k : nullptr,
                      direct ? direct + 3 * k : nullptr,
                      [&](int li, f3, f3, float) { return occluded[k * size_t(num_lights) + size_t(li)] != 0; });
    }
    return RT_OK;
}

extern "C" size_t rt_path_compact_scratch_bytes(size_t m) {
    if (m == 0 || m > 0x7FFFFFFFull) return 0;
    const size_t nt = path_tiles(m);
    return sizeof(uint32_t) * (nt + path_scan_words(nt));
}

extern "C" int rt_path_compact_device(int device, size_t m, const uint8_t* alive, const rt_ray* rays_in, const uint32_t* ids_in,
                                      rt_ray* rays_out, uint32_t* ids_out, uint32_t* count, void* scratch, void* stream) {
    if (m > 0x7FFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, "rt_path_compact_device: more than 2^31-1 entries in one batch");
    if (!count) return set_error(RT_ERR_ARG, "rt_path_compact_device: null count");
    if (m > 0) {
        if (!alive || !rays_in || !rays_out || !ids_out || !scratch)
            return set_error(RT_ERR_ARG, "rt_path_compact_device: null alive, rays, ids_out or scratch");
        if (reinterpret_cast<uintptr_t>(scratch) % 4 != 0) return set_error(RT_ERR_ARG, "rt_path_compact_device: scratch_dev is not 4-byte aligned");
        const size_t rb = m * sizeof(rt_ray), ib = m * sizeof(uint32_t), sb = rt_path_compact_scratch_bytes(m);
        const struct { const void* p; size_t n; } in[3] = {{alive, m}, {rays_in, rb}, {ids_in, ib}},
                                                  out[4] = {{rays_out, rb}, {ids_out, ib}, {count, sizeof(uint32_t)}, {scratch, sb}};
        for (const auto& o : out)
            for (const auto& i : in)
                if (ranges_overlap(o.p, o.n, i.p, i.n)) return set_error(RT_ERR_ARG, "rt_path_compact_device: an output overlaps an input");
        for (int a = 0; a < 4; ++a)
            for (int b = a + 1; b < 4; ++b)
                if (ranges_overlap(out[a].p, out[a].n, out[b].p, out[b].n))
                    return set_error(RT_ERR_ARG, "rt_path_compact_device: two outputs overlap");
    }
    int rc = check_device(device);
    if (rc != RT_OK) return rc;
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (m == 0) {
        HIP_TRY(hipMemsetAsync(count, 0, sizeof(uint32_t), st));
        return RT_OK;
    }
    const size_t nt = path_tiles(m);
    uint32_t* counts = static_cast<uint32_t*>(scratch);
    hipLaunchKernelGGL(path_count_kernel, dim3(unsigned(nt)), dim3(BLOCK), 0, st, alive, uint32_t(m), counts);
    path_scan(counts, nt, counts + nt, count, st);
    PathScatterParams P;
    std::memset(&P, 0, sizeof(P));
    P.alive = alive;
    P.m = uint32_t(m);
    P.offsets = counts;
    P.rays_in = reinterpret_cast<const float*>(rays_in);
    P.ids_in = ids_in;
    P.rays_out = reinterpret_cast<float*>(rays_out);
    P.ids_out = ids_out;
    hipLaunchKernelGGL(path_scatter_kernel, dim3(unsigned(nt)), dim3(BLOCK), 0, st, P);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// ---- spherical area lights for the staged path (rt_softshadow.hpp) ------------------------------
static_assert(sizeof(DevLightShape) == sizeof(rt_light_shape) && sizeof(rt_light_shape) == 8, "rt_light_shape");
static_assert(SOFT_MAX_SAMPLES == RT_LIGHT_MAX_SHADOW_SAMPLES, "RT_LIGHT_MAX_SHADOW_SAMPLES");

extern "C" int rt_scene_num_lights(const rt_scene* s) {
    return s ? s->nlights : 0;
}

namespace {
// The group sizes light_visibility_kernel is built at.
constexpr bool light_vis_built(int g) { return g == 1 || g == 8 || g == 32; }

// lanes_per_entry == 0: the group size for a launch whose largest light takes smax rays per
// entry: the largest built size that smax fills.  DESIGN.md §4.30's table
// (profiles/r14/soft_shadows.jsonl): at S = 1 a group of 8 or 32 costs 1.6x and 1.7x one lane per
// entry, at S = 8 one lane costs 2.2x a group of 8, at S = 32 and 128 a group of 8 costs 2.7x and
// 3.0x a group of 32.  The batch size is not part of the rule: one m was measured.
int light_vis_group(int smax) {
    if (smax >= 32) return 32;
    if (smax >= 8) return 8;
    return 1;
}

// No HIP call and no read through any pointer but s before the checks pass.
int light_vis_args(const rt_scene* s, size_t m, const void* hits, const void* ids, const void* shapes, const void* rng,
                   int lanes_per_entry, int flags, const void* vis) {
    if (!s) return set_error(RT_ERR_ARG, "rt_light_visibility_device: null scene");
    if (flags & ~RT_FLAG_BINARY) return set_error(RT_ERR_ARG, "rt_light_visibility_device: unknown flag");
    if (lanes_per_entry != 0 && !light_vis_built(lanes_per_entry))
        return set_error(RT_ERR_ARG, "rt_light_visibility_device: lanes_per_entry is not 0, 1, 8 or 32");
    if (m > 0x7FFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, "rt_light_visibility_device: more than 2^31-1 entries in one batch");
    if (m == 0 || s->nlights == 0) return RT_OK;
    if (!hits || !shapes || !rng || !vis) return set_error(RT_ERR_ARG, "rt_light_visibility_device: null hits, shapes, rng or vis");
    if (reinterpret_cast<uintptr_t>(hits) % 16 != 0) return set_error(RT_ERR_ARG, "rt_light_visibility_device: hits_dev is not 16-byte aligned");
    for (const void* p : {ids, shapes, rng, vis})
        if (reinterpret_cast<uintptr_t>(p) % 4 != 0) return set_error(RT_ERR_ARG, "rt_light_visibility_device: ids, shapes, rng or vis is not 4-byte aligned");
    return RT_OK;
}
}  // namespace

extern "C" int rt_light_visibility_device(rt_scene* s, size_t m, const rt_hit* hits, const uint32_t* ids,
                                          const rt_light_shape* shapes, uint32_t* rng, int lanes_per_entry, int flags,
                                          float* vis, void* stream) {
    int rc = light_vis_args(s, m, hits, ids, shapes, rng, lanes_per_entry, flags, vis);
    if (rc != RT_OK || m == 0 || s->nlights == 0) return rc;
    DeviceGuard g(s->device);
    if ((rc = deep_has_tris(s, "rt_light_visibility_device")) != RT_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // The shapes decide an error (too many samples) and the group size: one small copy back, in
    // stream order after whatever wrote them.
    std::vector<rt_light_shape> sh(size_t(s->nlights));
    HIP_TRY(hipMemcpyAsync(sh.data(), shapes, sh.size() * sizeof(rt_light_shape), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int smax = 1;
    for (const rt_light_shape& x : sh) {
        if (x.shadow_samples > SOFT_MAX_SAMPLES)
            return set_error(RT_ERR_UNSUPPORTED, "rt_light_visibility_device: shadow_samples above RT_LIGHT_MAX_SHADOW_SAMPLES");
        if (x.radius > 0.0f) smax = std::max(smax, x.shadow_samples);
    }
    const int G = lanes_per_entry != 0 ? lanes_per_entry : light_vis_group(smax);
    const int variant = s->query_variant(flags);
    LightVisParams P;
    std::memset(&P, 0, sizeof(P));
    P.sc = query_view(s, variant);  // (the packed records of the shadow rays and the lights)
    P.hits = reinterpret_cast<const uint4*>(hits);
    P.ids = ids;
    P.shapes = reinterpret_cast<const DevLightShape*>(shapes);
    P.rng = rng;
    P.vis = vis;
    P.m = uint32_t(m);
    const unsigned long long lanes = (unsigned long long)m * (unsigned long long)G;  // < 2^36
    const dim3 grid((unsigned)((lanes + BLOCK - 1) / BLOCK)), block(BLOCK);
    return launch_variant(s, kLightVis, variant, [&](auto V) {
        if (G == 1) hipLaunchKernelGGL((light_visibility_kernel<V(), 1>), grid, block, 0, st, P);
        else if (G == 8) hipLaunchKernelGGL((light_visibility_kernel<V(), 8>), grid, block, 0, st, P);
        else hipLaunchKernelGGL((light_visibility_kernel<V(), 32>), grid, block, 0, st, P);
    });
}

extern "C" int rt_light_visibility_variant(const rt_scene* s) {
    return variant_of(s, kLightVis);
}

extern "C" int rt_path_step_vis_device(rt_scene* s, size_t m, const rt_ray* rays, const rt_hit* hits, const rt_material* mats,
                                       const uint32_t* ids, const float* vis, const rt_path_opts* opt,
                                       const rt_path_state* state, rt_ray* next, uint8_t* alive, float* direct, void* stream) {
    if (!s) return set_error(RT_ERR_ARG, "rt_path_step_vis_device: null scene");
    int rc = path_step_args("rt_path_step_vis_device", m, rays, hits, opt, state, next, alive, RT_FLAG_BINARY | RT_PATH_LAST);
    if (rc != RT_OK) return rc;
    if (s->nlights > 0 && !vis) return set_error(RT_ERR_ARG, "rt_path_step_vis_device: null vis");
    // the kernel loads 16-byte words
    if (reinterpret_cast<uintptr_t>(hits) % 16 != 0) return set_error(RT_ERR_ARG, "rt_path_step_vis_device: hits_dev is not 16-byte aligned");
    if (m == 0) return RT_OK;
    DeviceGuard g(s->device);
    const SceneView v = scene_view(s);
    PathStepVisParams P;
    std::memset(&P, 0, sizeof(P));
    P.rays = reinterpret_cast<const float*>(rays);
    P.hits = reinterpret_cast<const uint4*>(hits);
    P.mats = reinterpret_cast<const float*>(mats);
    P.ids = ids;
    P.vis = vis;
    P.table = v.mats;
    P.lights = v.lights;
    P.num_table = v.num_mats;
    P.num_lights = v.num_lights;
    P.m = uint32_t(m);
    P.diffuse_bounce = opt->diffuse_bounce;
    P.last = (opt->flags & RT_PATH_LAST) ? 1 : 0;
    P.miss = mk(opt->miss_color.x, opt->miss_color.y, opt->miss_color.z);
    P.radiance = state->radiance;
    P.throughput = state->throughput;
    P.rng = state->rng;
    P.next = P.last && !next ? nullptr : reinterpret_cast<float*>(next);
    P.alive = alive;
    P.direct = direct;
    hipLaunchKernelGGL(path_step_vis_kernel, dim3((P.m + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), P);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// The host build of the visibility stage but for its traversals: per entry and light, in cast
// order, the shadow rays and their bounds through the functions the kernel runs.
extern "C" int rt_light_samples_host(size_t m, const rt_hit* hits, const uint32_t* ids, const rt_light* lights,
                                     const rt_light_shape* shapes, int num_lights, uint32_t* rng, size_t cap, rt_ray* rays,
                                     float* bounds, uint64_t* offsets) {
    if (m > 0x7FFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, "rt_light_samples_host: more than 2^31-1 entries in one batch");
    if (num_lights < 0 || !offsets || (m > 0 && (!hits || !rng)) || (num_lights > 0 && (!lights || !shapes)) || (rays && !bounds))
        return set_error(RT_ERR_ARG, "rt_light_samples_host: null hits, rng, lights, shapes, bounds or offsets");
    for (int l = 0; l < num_lights; ++l)
        if (shapes[l].shadow_samples > SOFT_MAX_SAMPLES)
            return set_error(RT_ERR_UNSUPPORTED, "rt_light_samples_host: shadow_samples above RT_LIGHT_MAX_SHADOW_SAMPLES");
    const DevLight* L = reinterpret_cast<const DevLight*>(lights);
    // write: store the rays and advance the rng; else count only, on copies of the state words
    auto pass = [&](bool write) {
        uint64_t n = 0;
        for (size_t k = 0; k < m; ++k) {
            const uint32_t id = ids ? ids[k] : uint32_t(k);
            HitWords h;  // (the caller's records need no alignment)
            std::memcpy(&h, hits + k, sizeof(h));
            const bool skip = id == PATH_NONE || (int32_t)h.w[0].x < 0;
            const f3 p = mk(pw::asf(h.w[1].x), pw::asf(h.w[1].y), pw::asf(h.w[1].z));
            const f3 N = skip ? p : unit(mk(pw::asf(h.w[1].w), pw::asf(h.w[2].x), pw::asf(h.w[2].y)));
            const f3 origin = add(p, scale(N, RT_EPS));
            uint32_t state = skip ? 0u : rng[id];
            auto emit = [&](f3 dir, float d) {
                if (write) {
                    rays[n].origin = rt_vec3{origin.x, origin.y, origin.z};
                    rays[n].direction = rt_vec3{dir.x, dir.y, dir.z};
                    bounds[n] = d;
                }
                ++n;
            };
            for (int l = 0; l < num_lights; ++l) {
                offsets[k * size_t(num_lights) + size_t(l)] = n;
                if (skip) continue;
                const f3 lpos = mk(L[l].pos[0], L[l].pos[1], L[l].pos[2]);
                const DevLightShape shape = {shapes[l].radius, shapes[l].shadow_samples};
                f3 toC;
                float distC;
                int S;
                const SoftClass cls = soft_class(p, N, lpos, shape, toC, distC, S);
                if (cls == SOFT_POINT) emit(divf(toC, distC), distC);
                if (cls != SOFT_DISK) continue;
                f3 T, B;
                soft_basis(p, lpos, distC, T, B);
                for (int i = 0; i < S; ++i) {
                    float x, y, d;
                    f3 dir;
                    soft_disk_draw(state, x, y);
                    if (soft_sample_ray(p, lpos, T, B, shape.radius, x, y, dir, d)) emit(dir, d);
                }
            }
            if (write && !skip) rng[id] = state;
        }
        offsets[m * size_t(num_lights)] = n;
        return n;
    };
    const uint64_t total = pass(false);
    if (!rays) return RT_OK;
    if (total > cap) return set_error(RT_ERR_ARG, "rt_light_samples_host: room for fewer rays than the batch casts");
    pass(true);
    return RT_OK;
}

// The host build of the step with visibilities: path_step_vis_one as path_step_vis_kernel runs it.
extern "C" int rt_path_step_vis_host(size_t m, const rt_ray* rays, const rt_hit* hits, const rt_material* mats,
                                     const uint32_t* ids, const rt_material* table, int num_table, const rt_light* lights,
                                     int num_lights, const float* vis, const rt_path_opts* opt, const rt_path_state* state,
                                     rt_ray* next, uint8_t* alive, float* direct) {
    const int rc = path_step_args("rt_path_step_vis_host", m, rays, hits, opt, state, next, alive, RT_FLAG_BINARY | RT_PATH_LAST);
    if (rc != RT_OK) return rc;
    if (num_table < 0 || num_lights < 0 || (num_table > 0 && !table) || (num_lights > 0 && (!lights || !vis)))
        return set_error(RT_ERR_ARG, "rt_path_step_vis_host: a table, light set or visibility array that does not match its count");
    const bool last = (opt->flags & RT_PATH_LAST) != 0;
    const f3 miss = mk(opt->miss_color.x, opt->miss_color.y, opt->miss_color.z);
    for (size_t k = 0; k < m; ++k) {
        const float* R = reinterpret_cast<const float*>(rays + k);
        float* nx = next ? reinterpret_cast<float*>(next + k) : nullptr;
        const uint32_t id = ids ? ids[k] : uint32_t(k);
        if (id == PATH_NONE) {
            if (nx) std::memmove(nx, R, sizeof(rt_ray));
            if (alive) alive[k] = 0;
            if (direct) direct[3 * k] = direct[3 * k + 1] = direct[3 * k + 2] = 0.0f;
            continue;
        }
        HitWords h;  // (the caller's records need no alignment)
        std::memcpy(&h, hits + k, sizeof(h));
        path_step_vis_one(R, h.w, mats ? reinterpret_cast<const float*>(mats + k) : nullptr,
                          reinterpret_cast<const DevMaterial*>(table), num_table, reinterpret_cast<const DevLight*>(lights),
                          num_lights, vis + k * size_t(num_lights), miss, opt->diffuse_bounce != 0, last,
                          state->radiance + 3 * size_t(id), state->throughput + 3 * size_t(id), state->rng + id, nx,
                          alive ? alive + k : nullptr, direct ? direct + 3 * k : nullptr);
    }
    return RT_OK;
}
