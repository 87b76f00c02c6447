// rt_rebuild.hpp — rebuild of a resident scene: a new tree and new records under new triangles
// (rt_scene_rebuild_device; a section of rt_device.hip, included inside its anonymous namespace
// after rt_refit.hpp).
//
// The tree is built on the device (rt_lbvh.hip, from the triangle array) after the refit's finite
// check.  The records are then packed on the device too (the second part of this section,
// RT_REBUILD_DEVICE) or, for what that does not handle, by rt::pack_scene on the host from the
// downloaded tree (RT_REBUILD_HOST); both fill fresh buffers that rt_scene_rebuild_device swaps in.
// The first exactness question of a pack on the device is the greedy record rules' weight
// (rt::box_weight, rt_records.cpp) in the device's double arithmetic: rt_debug_box_weight_batch and
// its test hold it to the host's bit for bit (the device's f64 sqrt agreed on every value tried).

// rt::box_weight for rules 1 (half surface area) and 2 (x sqrt(leaves)): negative extents count 0
// (std::max(0.0, d): a NaN extent counts 0 too), dx*dy + dy*dz + dz*dx in that order without
// contraction (the unit is built with -ffp-contract=off), 1e300 when the result is not finite.
// b: min corner, max corner.
__device__ __forceinline__ double rebuild_box_weight(const float* b, int rule, uint32_t leaves) {
    const double ex = (double)b[3] - (double)b[0], ey = (double)b[4] - (double)b[1], ez = (double)b[5] - (double)b[2];
    const double dx = 0.0 < ex ? ex : 0.0, dy = 0.0 < ey ? ey : 0.0, dz = 0.0 < ez ? ez : 0.0;
    double a = dx * dy + dy * dz + dz * dx;
    if (rule == 2) a *= sqrt((double)leaves);
    const bool finite = (__double_as_longlong(a) & 0x7FF0000000000000ll) != 0x7FF0000000000000ll;
    return finite ? a : 1e300;
}

__global__ __launch_bounds__(BLOCK) void box_weight_kernel(const float* __restrict__ boxes,
                                                           const uint32_t* __restrict__ leaves, int rule, int n,
                                                           double* __restrict__ out) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) out[i] = rebuild_box_weight(boxes + 6 * (size_t)i, rule, leaves[i]);
}

// ---- rt::pack_scene on the device, for the tree rt_lbvh.hip builds over finite triangles ------------
// Internal nodes are [0, P-1) and leaves [P-1, 2P-1), every internal node has two children and the
// boxes are nested, so a node's compact ref is known in closed form (rebuild_ref) and every stored
// box is the tree's own.  Order is by kernel boundaries only: a bottom-up fact of a node is computed
// by the launch of its height (rebuild_level_kernel, one launch per height; a node reads children
// finished by EARLIER launches), the frustum records level by level from the root (one count, one
// scan, one numbering launch per record level).  No flags, no fences, no spin-waits.  The host's
// code this restates: rt_scene_pack.cpp (stack_bounds, pack_records, pack_cut, plan_schedule) and
// rt_records.cpp (expand_largest, build_frustum_records).

constexpr int REBUILD_MAX_HEIGHT = 64;  // 64-bit keys with distinct low words: a Karras tree is no higher
constexpr int REBUILD_LEVEL_BINS = REBUILD_MAX_HEIGHT + 2;

struct RebuildView {
    const rt_bvh_node* nodes;
    const float* aabbs;  // per node: min corner, max corner
    const float* tris;   // 18 floats per triangle
    uint32_t P;          // internal nodes: P - 1
    uint32_t* ht;        // per internal node: height (0: not yet known), leaves below, binary and
    uint32_t* nleaf;     // 4-ary DFS stack bounds, the 4-ary record's entries (nodes) and their count
    uint32_t* S;
    uint32_t* SW;
    uint32_t* went;
    uint32_t* wk;
    uint32_t* flag;  // bit 0: a child's box does not contain its children's (wide_ok is false)
};

__device__ __forceinline__ bool rebuild_is_leaf(const RebuildView& v, uint32_t node) { return node >= v.P - 1; }
__device__ __forceinline__ uint32_t rebuild_ref(const RebuildView& v, uint32_t node) {
    return rebuild_is_leaf(v, node) ? (LEAF_BIT | (node - (v.P - 1))) : node;
}

// pack_cut's area: not clamped, INFINITY when it is a NaN.
__device__ __forceinline__ double rebuild_cut_area(const float* b) {
    const double dx = (double)b[3] - (double)b[0], dy = (double)b[4] - (double)b[1], dz = (double)b[5] - (double)b[2];
    const double a = dx * dy + dy * dz + dz * dx;
    return a == a ? a : (double)INFINITY;
}

// kind 1: box_weight rule 1; 2: rule 2 with the leaves below; 3: the cut's area.
__device__ __forceinline__ double rebuild_weight(const RebuildView& v, uint32_t node, int kind) {
    const float* b = v.aabbs + 6 * (size_t)node;
    if (kind == 3) return rebuild_cut_area(b);
    return rebuild_box_weight(b, kind, kind == 2 ? v.nleaf[node] : 0u);
}

// rt::expand_largest over e[0..n) with the weights cached in w (a leaf's is never read): while
// n < cap, the FIRST internal entry of strictly largest weight (a > ba from -1) is replaced by its
// two children, at its own position (in_place) or at the end.  At most cap - n rounds.  Entry i is
// e[i * stride], w[i * stride]: 1 for a lane's own arrays, the workgroup's width for arrays in LDS
// that the lanes interleave.
__device__ int rebuild_expand(const RebuildView& v, uint32_t* e, double* w, int stride, int n, int cap, bool in_place, int kind) {
#define E(i) e[(i) * stride]
#define Wt(i) w[(i) * stride]
    for (int i = 0; i < n; ++i) Wt(i) = rebuild_is_leaf(v, E(i)) ? -2.0 : rebuild_weight(v, E(i), kind);
    while (n < cap) {
        int best = -1;
        double ba = -1.0;
        for (int i = 0; i < n; ++i) {
            const double a = Wt(i);  // (a leaf's -2 never exceeds ba)
            if (a > ba) {
                ba = a;
                best = i;
            }
        }
        if (best < 0) break;
        const rt_bvh_node nd = v.nodes[E(best)];
        if (in_place) {
            for (int i = n; i > best + 1; --i) E(i) = E(i - 1), Wt(i) = Wt(i - 1);
        } else {
            for (int i = best; i < n - 1; ++i) E(i) = E(i + 1), Wt(i) = Wt(i + 1);
        }
        const int at = in_place ? best : n - 1;
        E(at) = nd.left_idx, E(at + 1) = nd.right_idx;
        Wt(at) = rebuild_is_leaf(v, nd.left_idx) ? -2.0 : rebuild_weight(v, nd.left_idx, kind);
        Wt(at + 1) = rebuild_is_leaf(v, nd.right_idx) ? -2.0 : rebuild_weight(v, nd.right_idx, kind);
        ++n;
    }
    return n;
#undef E
#undef Wt
}

__device__ __forceinline__ bool rebuild_contains(const float* o, const float* i) {
    return o[0] <= i[0] && o[1] <= i[1] && o[2] <= i[2] && o[3] >= i[3] && o[4] >= i[4] && o[5] >= i[5];
}

__device__ __forceinline__ void rebuild_pairs(float* q, const float* b) {
    q[0] = b[0], q[1] = b[3], q[2] = b[1], q[3] = b[4], q[4] = b[2], q[5] = b[5];
}

// Per internal node: the 4-ary record's entries (WideRule::entries at rule 1), the containment
// check of stack_bounds, and ht = 0.
__global__ __launch_bounds__(BLOCK) void rebuild_wide_entries_kernel(RebuildView v) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i + 1 >= v.P) return;
    const rt_bvh_node nd = v.nodes[i];
    uint32_t e[4] = {nd.left_idx, nd.right_idx, 0u, 0u};
    double w[4];
    const int k = rebuild_expand(v, e, w, 1, 2, 4, true, 1);
    for (int j = 0; j < 4; ++j) v.went[4 * (size_t)i + j] = j < k ? e[j] : NO_REF;
    v.wk[i] = (uint32_t)k;
    v.ht[i] = 0u;
    for (int c = 0; c < 2; ++c) {
        const uint32_t ch = c ? nd.right_idx : nd.left_idx;
        if (rebuild_is_leaf(v, ch)) continue;
        const rt_bvh_node cn = v.nodes[ch];
        if (!rebuild_contains(v.aabbs + 6 * (size_t)ch, v.aabbs + 6 * (size_t)cn.left_idx) ||
            !rebuild_contains(v.aabbs + 6 * (size_t)ch, v.aabbs + 6 * (size_t)cn.right_idx))
            atomicOr(v.flag, 1u);
    }
}

// The launch of height h: every internal node without a height whose children got theirs in an
// EARLIER launch (a leaf: 0; an internal child: 0 < ht < h — a height written by this launch reads
// as 0 or h, not ready either way) takes height h, the leaves below, S and SW (stack_bounds).
__global__ __launch_bounds__(BLOCK) void rebuild_level_kernel(RebuildView v, uint32_t h) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i + 1 >= v.P || v.ht[i] != 0u) return;
    const rt_bvh_node nd = v.nodes[i];
    const bool ll = rebuild_is_leaf(v, nd.left_idx), rl = rebuild_is_leaf(v, nd.right_idx);
    const uint32_t hl = ll ? 0u : v.ht[nd.left_idx], hr = rl ? 0u : v.ht[nd.right_idx];
    if ((!ll && (hl == 0u || hl >= h)) || (!rl && (hr == 0u || hr >= h))) return;
    const uint32_t sl = ll ? 0u : v.S[nd.left_idx], sr = rl ? 0u : v.S[nd.right_idx];
    uint32_t s = 2u;
    s = max(s, 1u + sr);
    s = max(s, sl);
    const uint32_t k = v.wk[i];
    uint32_t sw = k;
    for (uint32_t j = 0; j < k; ++j) {
        const uint32_t en = v.went[4 * (size_t)i + j];
        if (!rebuild_is_leaf(v, en)) sw = max(sw, j + v.SW[en]);
    }
    v.nleaf[i] = (ll ? 1u : v.nleaf[nd.left_idx]) + (rl ? 1u : v.nleaf[nd.right_idx]);
    v.S[i] = s;
    v.SW[i] = sw;
    v.ht[i] = h;
}

// plan_schedule's counting sort by height, stable in the node index: per block of BLOCK nodes the
// count per height (cnt[h * nb + b]); after the exclusive scan of cnt, a node's place is its
// (height, block) offset plus its rank among the block's earlier nodes of that height.
__global__ __launch_bounds__(BLOCK) void rebuild_level_count_kernel(RebuildView v, uint32_t* cnt, uint32_t nb) {
    __shared__ uint32_t hist[REBUILD_LEVEL_BINS];
    if (threadIdx.x < REBUILD_LEVEL_BINS) hist[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i + 1 < v.P) atomicAdd(&hist[min(v.ht[i], (uint32_t)REBUILD_LEVEL_BINS - 1)], 1u);
    __syncthreads();
    if (threadIdx.x < REBUILD_LEVEL_BINS) cnt[(size_t)threadIdx.x * nb + blockIdx.x] = hist[threadIdx.x];
}

// facts: [0] ht, [1] S, [2] SW of the root, [3] the flag word, [8 + h] level_off[h] for h <= 64.
__global__ __launch_bounds__(BLOCK) void rebuild_order_kernel(RebuildView v, const uint32_t* __restrict__ cnt, uint32_t nb,
                                                              uint32_t* __restrict__ order, uint32_t* __restrict__ facts) {
    __shared__ uint32_t hs[BLOCK];
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const bool have = i + 1 < v.P;
    const uint32_t h = have ? min(v.ht[i], (uint32_t)REBUILD_LEVEL_BINS - 1) : 0xFFFFFFFFu;
    hs[threadIdx.x] = h;
    __syncthreads();
    if (have) {
        uint32_t rank = 0;
        for (uint32_t t = 0; t < threadIdx.x; ++t) rank += hs[t] == h ? 1u : 0u;
        order[cnt[(size_t)h * nb + blockIdx.x] + rank] = i;
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x <= REBUILD_MAX_HEIGHT) facts[8 + threadIdx.x] = cnt[(size_t)(threadIdx.x + 1) * nb];
        if (threadIdx.x == 0) facts[0] = v.ht[0], facts[1] = v.S[0], facts[2] = v.SW[0], facts[3] = *v.flag;
    }
}

// pack_records: a leaf slot per lane ...
__global__ __launch_bounds__(BLOCK) void rebuild_leaf_kernel(RebuildView v, float4* __restrict__ leaf) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= v.P) return;
    const uint32_t node = v.P - 1 + j;
    const uint32_t ti = v.nodes[node].object_idx;
    const float* t = v.tris + 18 * (size_t)ti;
    const float* b = v.aabbs + 6 * (size_t)node;
    float4* q = leaf + 4 * (size_t)j;
    q[0] = make_float4(t[0], t[1], t[2], __uint_as_float(ti));
    q[1] = make_float4(t[3] - t[0], t[4] - t[1], t[5] - t[2], t[6] - t[0]);
    q[2] = make_float4(t[7] - t[1], t[8] - t[2], b[0], b[3]);
    q[3] = make_float4(b[1], b[4], b[2], b[5]);
}

// ... and an internal node per lane: inode (child boxes, refs, inv = 0), ibox, wnode; node 0 also
// writes the root's trailing ibox copy.
__global__ __launch_bounds__(BLOCK) void rebuild_inode_kernel(RebuildView v, float* __restrict__ inode, float* __restrict__ ibox,
                                                              float* __restrict__ wnode) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i + 1 >= v.P) return;
    const rt_bvh_node nd = v.nodes[i];
    float* q = inode + 16 * (size_t)i;
    rebuild_pairs(q, v.aabbs + 6 * (size_t)nd.left_idx);
    rebuild_pairs(q + 6, v.aabbs + 6 * (size_t)nd.right_idx);
    q[12] = __uint_as_float(rebuild_ref(v, nd.left_idx));
    q[13] = __uint_as_float(rebuild_ref(v, nd.right_idx));
    q[14] = 0.f, q[15] = 0.f;
    float* ib = ibox + 8 * (size_t)i;
    rebuild_pairs(ib, v.aabbs + 6 * (size_t)i);
    ib[6] = 0.f, ib[7] = 0.f;
    if (i == 0) {
        float* rb = ibox + 8 * (size_t)(v.P - 1);
        rebuild_pairs(rb, v.aabbs);
        rb[6] = 0.f, rb[7] = 0.f;
    }
    float* wq = wnode + 32 * (size_t)i;
    for (int j = 0; j < 4; ++j) {
        const uint32_t en = v.went[4 * (size_t)i + j];
        if (en != NO_REF) {
            rebuild_pairs(wq + 6 * j, v.aabbs + 6 * (size_t)en);
        } else {
            for (int k = 0; k < 6; ++k) wq[6 * j + k] = 0.f;
        }
        wq[24 + j] = __uint_as_float(en == NO_REF ? NO_REF : rebuild_ref(v, en));
        wq[28 + j] = 0.f;
    }
}

// ---- frustum records (build_frustum_records at rule 2), record level by record level ---------------
// recnode: record -> node, breadth first.  A record's entries are expanded once, by the count pass
// of its level, into ents (32 words per record) and rk (their number); the later passes read them.
// cnt[r]: the internal entries of record r in [lo, hi).  One record per lane, its entry list and
// weights in LDS, interleaved over the 64 lanes.
__global__ __launch_bounds__(64) void rebuild_frec_count_kernel(RebuildView v, const uint32_t* __restrict__ recnode, uint32_t lo,
                                                                uint32_t hi, int A, uint32_t* __restrict__ cnt,
                                                                uint32_t* __restrict__ ents, uint32_t* __restrict__ rk) {
    __shared__ uint32_t se[32 * 64];
    __shared__ double sw[32 * 64];
    const uint32_t r = lo + blockIdx.x * 64 + threadIdx.x;
    if (r >= hi) return;
    uint32_t* e = se + threadIdx.x;
    const rt_bvh_node nd = v.nodes[recnode[r]];
    e[0] = nd.left_idx, e[64] = nd.right_idx;
    const int k = rebuild_expand(v, e, sw + threadIdx.x, 64, 2, A, true, 2);
    uint32_t c = 0;
    for (int i = 0; i < k; ++i) {
        const uint32_t en = e[64 * i];
        c += rebuild_is_leaf(v, en) ? 0u : 1u;
        ents[32 * (size_t)r + i] = en;
    }
    cnt[r] = c;
    rk[r] = (uint32_t)k;
}

// off[r]: the exclusive scan of cnt over [lo, hi).  Record r's internal entries, in entry order,
// become records hi + off[r], hi + off[r] + 1, ... (the host's breadth-first numbering).
__global__ __launch_bounds__(BLOCK) void rebuild_frec_number_kernel(RebuildView v, uint32_t* __restrict__ recnode,
                                                                    uint32_t* __restrict__ fid, uint32_t lo, uint32_t hi,
                                                                    const uint32_t* __restrict__ off, uint32_t cap,
                                                                    const uint32_t* __restrict__ ents,
                                                                    const uint32_t* __restrict__ rk) {
    const uint32_t r = lo + blockIdx.x * BLOCK + threadIdx.x;
    if (r >= hi) return;
    const uint32_t k = rk[r];
    uint32_t id = hi + off[r];
    for (uint32_t i = 0; i < k; ++i) {
        const uint32_t en = ents[32 * (size_t)r + i];
        if (!rebuild_is_leaf(v, en) && id < cap) {
            recnode[id] = en;
            fid[en] = id;
            ++id;
        }
    }
}

// SF of the records of one level, after the levels below it.
__global__ __launch_bounds__(BLOCK) void rebuild_frec_bound_kernel(RebuildView v, const uint32_t* __restrict__ fid, uint32_t lo,
                                                                   uint32_t hi, uint32_t* __restrict__ SF,
                                                                   const uint32_t* __restrict__ ents,
                                                                   const uint32_t* __restrict__ rk) {
    const uint32_t r = lo + blockIdx.x * BLOCK + threadIdx.x;
    if (r >= hi) return;
    const uint32_t k = rk[r];
    uint32_t sf = k;
    for (uint32_t i = 0; i < k; ++i) {
        const uint32_t en = ents[32 * (size_t)r + i];
        if (!rebuild_is_leaf(v, en)) sf = max(sf, i + SF[fid[en]]);
    }
    SF[r] = sf;
}

// fnode (zeroed before), one entry per lane: A x box pairs | A refs (NO_REF pads) | unused.
__global__ __launch_bounds__(BLOCK) void rebuild_frec_write_kernel(RebuildView v, const uint32_t* __restrict__ fid, uint32_t nrec,
                                                                   int f_log2, float* __restrict__ fnode,
                                                                   const uint32_t* __restrict__ ents,
                                                                   const uint32_t* __restrict__ rk) {
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t A = 1u << f_log2;
    if (t >= ((size_t)nrec << f_log2)) return;
    const size_t r = t >> f_log2;
    const uint32_t i = (uint32_t)(t & (A - 1));
    float* q = fnode + 8 * (size_t)A * r;
    uint32_t ref = NO_REF;
    if (i < rk[r]) {
        const uint32_t en = ents[32 * r + i];
        rebuild_pairs(q + 6 * i, v.aabbs + 6 * (size_t)en);
        ref = rebuild_is_leaf(v, en) ? rebuild_ref(v, en) : fid[en];
    }
    q[6 * A + i] = __uint_as_float(ref);
}

// ---- the cuts (pack_cut): one workgroup of 64 --------------------------------------------------------
// Lane 0 grows the cut from the root (at the end, not in place); then lane i grows the sub-boxes of
// cut node i.  cut / cut2: room for 64 and 64 x 64 boxes; refs: the cut slots' refs at [0, 64), the
// cut2 slots' at [64, 64 + 64 * 64); *ncut_out the cut's size.
__global__ __launch_bounds__(64) void rebuild_cut_kernel(RebuildView v, int kcut, int S, float* __restrict__ cut,
                                                         float* __restrict__ cut2, uint32_t* __restrict__ refs,
                                                         uint32_t* __restrict__ ncut_out) {
    __shared__ uint32_t cutn[64];
    __shared__ int ncut_s;
    __shared__ uint32_t se[64 * 64];  // entry lists and weights, interleaved over the lanes
    __shared__ double sw[64 * 64];
    if (threadIdx.x == 0) {
        se[0] = 0u;
        const int n = rebuild_expand(v, se, sw, 1, 1, kcut, false, 3);  // (the other lanes wait: the arrays are lane 0's)
        for (int i = 0; i < n; ++i) cutn[i] = se[i];
        ncut_s = n;
        *ncut_out = (uint32_t)n;
    }
    __syncthreads();
    const int ncut = ncut_s;
    const int i = threadIdx.x;
    if (i >= ncut) return;
    for (int k = 0; k < 6; ++k) cut[6 * i + k] = v.aabbs[6 * (size_t)cutn[i] + k];
    refs[i] = rebuild_ref(v, cutn[i]);
    if (S < 2) return;
    uint32_t* e = se + i;
    e[0] = cutn[i];
    const int ns = rebuild_expand(v, e, sw + i, 64, 1, S, false, 3);
    for (int j = 0; j < S; ++j) {
        const uint32_t n = e[64 * (j < ns ? j : 0)];
        for (int k = 0; k < 6; ++k) cut2[6 * ((size_t)i * S + j) + k] = v.aabbs[6 * (size_t)n + k];
        refs[64 + (size_t)i * S + j] = rebuild_ref(v, n);
    }
}
