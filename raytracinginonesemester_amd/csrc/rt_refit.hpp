// rt_refit.hpp — refit of a resident scene for deforming geometry (rt_scene_refit_device; a
// section of rt_device.hip, included inside its anonymous namespace).
//
// The packed arrays hold the tree's topology in compact refs and one tree node's box in every box
// slot, so a refit keeps the topology and rewrites the boxes: a node's current box is its ibox
// entry (internal) or its leaf record's words 10-15, both per axis (min, max), and every other
// slot is a copy of one of those in the slot's own layout.  The host restatement is
// rt::refit_packed (rt_scene_pack.cpp); the two agree byte for byte.
//
// Order: finite check | leaves (box, v0 | e1 | e2), tnorm, tri | internal boxes bottom-up with the
// inode child boxes | the root's trailing ibox copy | wnode, fnode, cut, cut2.
//
// Bottom-up without a fence per node (the XCDs' L2s are not coherent: agent-scope ordering is an L2
// write-back and invalidate, rt_lbvh.hip): the plan lists the internal nodes by height, and a
// node's children sit in lower levels.  A level wider than one workgroup is one launch (the kernel
// boundary orders it after the levels below); the levels shrink towards the root, so from the
// first level of at most REFIT_TOP nodes on, one workgroup walks the rest with a workgroup
// barrier between levels (one CU, one L1).  No flags, no spin-waits.
//
// min / max are glibc's fminf / fmaxf on numbers (x < y ? x : y, the second argument winning the
// +-0 tie), as aabb_of_triangle and AABB::merge apply them on the host; the vertices are finite
// (checked first), so no NaN reaches them.

constexpr int REFIT_TOP = 1024;

struct RefitView {
    float4* inode;
    float4* wnode;  // or null
    float* fnode;   // or null
    float4* ibox;
    float4* leaf;
    float4* tnorm;
    float4* tri;  // or null
    float* cut;
    float* cut2;
    const uint32_t* order;      // internal nodes by height (RefitPlan::order)
    const uint32_t* level_off;  // level h: order[level_off[h - 1], level_off[h])
    const uint32_t* frec;       // fnode record -> internal node
    const uint32_t* cut_ref;    // the cut slots' nodes, then the cut2 slots'
    uint32_t n_int, n_leaf, P, root_ref;
    uint32_t f_log2, nrec, ncut_slots;  // ncut_slots: cut and cut2 slots together
};

struct RefitBox {  // per axis (min, max)
    float v[6];
};

__device__ __forceinline__ float refit_min(float x, float y) { return x < y ? x : y; }
__device__ __forceinline__ float refit_max(float x, float y) { return x > y ? x : y; }

__device__ __forceinline__ RefitBox refit_box(const RefitView& v, uint32_t ref) {
    RefitBox b;
    if (ref & LEAF_BIT) {
        const float2* q = reinterpret_cast<const float2*>(v.leaf + 4 * (size_t)(ref & ~LEAF_BIT)) + 5;
        const float2 x = q[0], y = q[1], z = q[2];
        b.v[0] = x.x, b.v[1] = x.y, b.v[2] = y.x, b.v[3] = y.y, b.v[4] = z.x, b.v[5] = z.y;
    } else {
        const float4 lo = v.ibox[2 * (size_t)ref], hi = v.ibox[2 * (size_t)ref + 1];
        b.v[0] = lo.x, b.v[1] = lo.y, b.v[2] = lo.z, b.v[3] = lo.w, b.v[4] = hi.x, b.v[5] = hi.y;
    }
    return b;
}

__device__ __forceinline__ void refit_store6(float* q, const RefitBox& b, bool corners) {  // q: 8-byte aligned
    float2* o = reinterpret_cast<float2*>(q);
    if (corners) {
        o[0] = make_float2(b.v[0], b.v[2]);
        o[1] = make_float2(b.v[4], b.v[1]);
        o[2] = make_float2(b.v[3], b.v[5]);
    } else {
        o[0] = make_float2(b.v[0], b.v[1]);
        o[1] = make_float2(b.v[2], b.v[3]);
        o[2] = make_float2(b.v[4], b.v[5]);
    }
}

__device__ __forceinline__ bool refit_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// The first pass: every vertex coordinate finite, or *bad is raised and nothing gets written.
__global__ __launch_bounds__(BLOCK) void refit_check_kernel(const float* __restrict__ tris, uint32_t P, uint32_t* bad) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P) return;
    const float* t = tris + 18 * (size_t)i;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) ok = ok && refit_finite(t[k]);
    if (!ok) atomicOr(bad, 1u);
}

// One leaf slot per lane: the record's triangle (word 3, kept), v0 | e1, e2.x | e2.y, e2.z and
// the box aabb_of_triangle gives (eps = 0: min - 0.0f is the identity, max + 0.0f turns -0 into +0).
__global__ __launch_bounds__(BLOCK) void refit_leaves_kernel(RefitView v, const float* __restrict__ tris) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= v.n_leaf) return;
    float4* q = v.leaf + 4 * (size_t)j;
    const float tif = q[0].w;
    const float* t = tris + 18 * (size_t)__float_as_uint(tif);
    float a[3], b[3], c[3], mn[3], mx[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = t[k], b[k] = t[3 + k], c[k] = t[6 + k];
        mn[k] = refit_min(a[k], refit_min(b[k], c[k])) - 0.0f;
        mx[k] = refit_max(a[k], refit_max(b[k], c[k])) + 0.0f;
    }
    q[0] = make_float4(a[0], a[1], a[2], tif);
    q[1] = make_float4(b[0] - a[0], b[1] - a[1], b[2] - a[2], c[0] - a[0]);
    q[2] = make_float4(c[1] - a[1], c[2] - a[2], mn[0], mx[0]);
    q[3] = make_float4(mn[1], mx[1], mn[2], mx[2]);
}

// One triangle per lane: tnorm, and the deep trees' v0 | e1 | e2 by triangle index.
__global__ __launch_bounds__(BLOCK) void refit_triangles_kernel(RefitView v, const float* __restrict__ tris) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= v.P) return;
    const float* t = tris + 18 * (size_t)i;
    float4* n = v.tnorm + 3 * (size_t)i;
    n[0] = make_float4(t[9], t[10], t[11], 0.f);
    n[1] = make_float4(t[12], t[13], t[14], 0.f);
    n[2] = make_float4(t[15], t[16], t[17], 0.f);
    if (v.tri) {
        float4* q = v.tri + 3 * (size_t)i;
        q[0] = make_float4(t[0], t[1], t[2], 0.f);
        q[1] = make_float4(t[3] - t[0], t[4] - t[1], t[5] - t[2], t[6] - t[0]);
        q[2] = make_float4(t[7] - t[1], t[8] - t[2], 0.f, 0.f);
    }
}

// Internal node i from its children's boxes: the inode child boxes (left x y | left z, right x |
// right y z; the refs in words 12-15 stay) and merge(left, right) into ibox.
__device__ __forceinline__ void refit_node(const RefitView& v, uint32_t i) {
    float4* q = v.inode + 4 * (size_t)i;
    const float4 refs = q[3];
    const RefitBox l = refit_box(v, __float_as_uint(refs.x)), r = refit_box(v, __float_as_uint(refs.y));
    q[0] = make_float4(l.v[0], l.v[1], l.v[2], l.v[3]);
    q[1] = make_float4(l.v[4], l.v[5], r.v[0], r.v[1]);
    q[2] = make_float4(r.v[2], r.v[3], r.v[4], r.v[5]);
    float m[6];
#pragma unroll
    for (int k = 0; k < 6; k += 2) {
        m[k] = refit_min(l.v[k], r.v[k]);
        m[k + 1] = refit_max(l.v[k + 1], r.v[k + 1]);
    }
    v.ibox[2 * (size_t)i] = make_float4(m[0], m[1], m[2], m[3]);
    v.ibox[2 * (size_t)i + 1] = make_float4(m[4], m[5], 0.f, 0.f);
}

// One level wider than a workgroup: order[first, first + count).
__global__ __launch_bounds__(BLOCK) void refit_level_kernel(RefitView v, uint32_t first, uint32_t count) {
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k < count) refit_node(v, v.order[first + k]);
}

// One workgroup: levels [level0, levels] in turn (level_off[h - 1] .. level_off[h]), a barrier
// between them, then the root's trailing ibox copy (SceneView::rootb).
__global__ __launch_bounds__(REFIT_TOP) void refit_top_levels_kernel(RefitView v, uint32_t level0, uint32_t levels) {
    for (uint32_t h = level0; h <= levels; ++h) {
        const uint32_t end = v.level_off[h];
        for (uint32_t k = v.level_off[h - 1] + threadIdx.x; k < end; k += REFIT_TOP) refit_node(v, v.order[k]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const RefitBox b = refit_box(v, v.root_ref);
        const size_t at = 2 * (size_t)(v.n_int > 0 ? v.n_int : 1);
        v.ibox[at] = make_float4(b.v[0], b.v[1], b.v[2], b.v[3]);
        v.ibox[at + 1] = make_float4(b.v[4], b.v[5], 0.f, 0.f);
    }
}

// 4-ary records, one per lane: 4 x (x pair, y pair, z pair) from the entries' refs (words 24-27,
// kept); an unused entry's box stays zero.
__global__ __launch_bounds__(BLOCK) void refit_wnode_kernel(RefitView v) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= v.n_int) return;
    float4* q = v.wnode + 8 * (size_t)i;
    const float4 refs = q[6];
    const uint32_t r[4] = {__float_as_uint(refs.x), __float_as_uint(refs.y), __float_as_uint(refs.z), __float_as_uint(refs.w)};
    float w[24];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        RefitBox b = {{0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
        if (r[e] != NO_REF) b = refit_box(v, r[e]);
#pragma unroll
        for (int k = 0; k < 6; ++k) w[6 * e + k] = b.v[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) q[k] = make_float4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

// Frustum records, one entry per lane: a leaf entry's box is the leaf's, an internal entry's ref
// is a record index, whose node the plan names.
__global__ __launch_bounds__(BLOCK) void refit_fnode_kernel(RefitView v) {
    const size_t e = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t A = 1u << v.f_log2;
    if (e >= (size_t)v.nrec * A) return;
    const size_t r = e >> v.f_log2;
    const uint32_t i = (uint32_t)(e & (A - 1));
    float* w = v.fnode + 8 * (size_t)A * r;
    const uint32_t ref = __float_as_uint(w[6 * A + i]);
    if (ref == NO_REF) return;
    refit_store6(w + 6 * i, refit_box(v, (ref & LEAF_BIT) ? ref : v.frec[ref]), false);
}

// The tile-culling cuts, one slot per lane (min corner, max corner): cut's slots, then cut2's,
// whose duplicates name their first sub-box's node in the plan.
__global__ __launch_bounds__(BLOCK) void refit_cut_kernel(RefitView v, uint32_t ncut) {
    const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
    if (s >= v.ncut_slots) return;
    float* q = s < ncut ? v.cut + 6 * (size_t)s : v.cut2 + 6 * (size_t)(s - ncut);
    refit_store6(q, refit_box(v, v.cut_ref[s]), true);
}

// Triangles from an indexed mesh (G/src/main.cu:388-404): positions and, when the mesh has them,
// normals by vertex index; zero normals otherwise.  An index past the vertices raises *err and
// writes nothing.
__global__ __launch_bounds__(BLOCK) void mesh_triangles_kernel(const float* __restrict__ pos, const float* __restrict__ nrm,
                                                               uint32_t nv, const uint32_t* __restrict__ idx, uint32_t P,
                                                               float* __restrict__ tris, uint32_t* err) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P) return;
    const uint32_t id[3] = {idx[3 * (size_t)i], idx[3 * (size_t)i + 1], idx[3 * (size_t)i + 2]};
    if (id[0] >= nv || id[1] >= nv || id[2] >= nv) {
        atomicOr(err, 1u);
        return;
    }
    float* t = tris + 18 * (size_t)i;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            t[3 * c + k] = pos[3 * (size_t)id[c] + k];
            t[9 + 3 * c + k] = nrm ? nrm[3 * (size_t)id[c] + k] : 0.0f;
        }
}
