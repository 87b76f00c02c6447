// rt_scene_pack.cpp — rt::pack_scene (rt_scene_pack.hpp): classify the nodes, bound the DFS
// stacks, pack the records, derive the bounds and build the tile-culling cut.  Host code only,
// compiled by the host compiler; rt_debug_scene_pack and rt_debug_frustum_records are the CPU
// tests' views of it.
#include "rt_scene_pack.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <utility>

#include "rt_common.hpp"

namespace rt {
namespace {

struct Tree {  // the caller's arrays and their ids
    size_t P, NN;
    const rt_bvh_node* nodes;
    const rt_aabb* aabbs;
    const uint32_t* cid;
    uint32_t ref(uint32_t n) const { return n == NO_REF ? NO_REF : cid[n]; }
};

void put4(float* q, float x, float y, float z, float w) { q[0] = x, q[1] = y, q[2] = z, q[3] = w; }
void put_pairs(float* q, const rt_aabb& b) {  // per axis (min, max)
    put4(q, b.min_corner.x, b.max_corner.x, b.min_corner.y, b.max_corner.y);
    q[4] = b.min_corner.z, q[5] = b.max_corner.z;
}
void put_corners(float* q, const rt_aabb& b) {  // min corner, max corner
    put4(q, b.min_corner.x, b.min_corner.y, b.min_corner.z, b.max_corner.x);
    q[4] = b.max_corner.y, q[5] = b.max_corner.z;
}

// Wide (4-ary) records: internal node n lists the children of its children in SearchBVH's
// push order (a leaf child stands for itself), so one visit tests and pushes what the
// reference reaches in two.  The result is the same provided every internal child's box
// contains its children's boxes (the pass the skipped test would give is then implied,
// slab tests being monotone in the box), checked by stack_bounds; the wave path falls back to
// the binary records otherwise, or when the 4-ary DFS stack would exceed 64 entries.
// RT_TUNE_WIDE4_GREEDY (default 1): the 4-ary records' entries grown from the node's children
// by expanding, in place, the internal entry of largest surface area (up to 4 entries; 2: area x
// sqrt(valid leaves below)); 0: the grandchildren.  Exact for the reasons the grandchildren are
// (every box contains its children's, checked for every parent-child pair; the DFS order is
// SearchBVH's; no leaf is tested between an expanded node's pop and its children's in the
// reference).  c3 0.1390 vs 0.1419 ms, c3b 1.2455 vs 1.2986, c5 40.35 vs 40.82
// (profiles/r05/exp/wide4_greedy_ab.log)
struct WideRule {
    int rule;
    std::vector<uint32_t> leaves;
    explicit WideRule(const Tree& t) : rule(int(tuning(RT_TUNE_WIDE4_GREEDY, 1.0) + 0.5)) {
        if (rule == 2) leaves = subtree_leaves(t.nodes, t.NN, t.cid);
    }
    int entries(const Tree& t, const rt_bvh_node& nd, uint32_t* e) const {
        int k = 0;
        if (rule > 0) {
            for (const uint32_t c : {nd.left_idx, nd.right_idx})
                if (t.ref(c) != NO_REF) e[k++] = c;
            return expand_largest(t.nodes, t.cid, e, k, 4, true, [&](uint32_t n) {
                return rule == 2 ? box_weight(t.aabbs[n], 2, leaves[n]) : box_weight(t.aabbs[n], 1, 0u);
            });
        }
        for (const uint32_t c : {nd.left_idx, nd.right_idx}) {
            if (t.ref(c) == NO_REF) continue;
            if (t.ref(c) & LEAF_BIT) {
                e[k++] = c;
                continue;
            }
            const rt_bvh_node& cn = t.nodes[c];
            if (t.ref(cn.left_idx) != NO_REF) e[k++] = cn.left_idx;
            if (t.ref(cn.right_idx) != NO_REF) e[k++] = cn.right_idx;
        }
        return k;
    }
};

struct StackBounds {
    int binary = 0, wide = 0;  // DFS stack entries the binary and the 4-ary records may need
    bool wide_ok = true;       // every internal child's box contains its children's
};

bool contains(const rt_aabb& o, const rt_aabb& i) {
    return o.min_corner.x <= i.min_corner.x && o.min_corner.y <= i.min_corner.y && o.min_corner.z <= i.min_corner.z &&
           o.max_corner.x >= i.max_corner.x && o.max_corner.y >= i.max_corner.y && o.max_corner.z >= i.max_corner.z;
}

// One post-order walk from the root: the reachable graph is a finite tree (RT_ERR_ARG for a
// cycle), and the stack bounds of SearchBVH's push/pop order over it.
int stack_bounds(const Tree& t, const WideRule& w, StackBounds& out) {
    std::vector<uint8_t> state(t.NN, 0);  // 0 new, 1 on path, 2 done
    std::vector<int> S(t.NN, 0), SW(t.NN, 0);
    std::vector<std::pair<uint32_t, bool>> st{{0u, false}};
    while (!st.empty()) {
        auto [v, post] = st.back();
        st.pop_back();
        const rt_bvh_node& nd = t.nodes[v];
        const bool internal = nd.object_idx == 0xFFFFFFFFu;
        if (!post) {
            if (state[v] == 1) return set_error(RT_ERR_ARG, "BVH contains a cycle");
            if (state[v] == 2) continue;
            state[v] = 1;
            st.push_back({v, true});
            if (internal) {
                if (nd.left_idx != NO_REF) st.push_back({nd.left_idx, false});
                if (nd.right_idx != NO_REF) st.push_back({nd.right_idx, false});
            }
        } else {
            state[v] = 2;
            if (!internal) continue;
            const int sl = nd.left_idx != NO_REF ? S[nd.left_idx] : 0;
            const int sr = nd.right_idx != NO_REF ? S[nd.right_idx] : 0;
            int s = (nd.left_idx != NO_REF) + (nd.right_idx != NO_REF);  // the pushes
            if (nd.right_idx != NO_REF) s = std::max(s, (nd.left_idx != NO_REF ? 1 : 0) + sr);
            if (nd.left_idx != NO_REF) s = std::max(s, sl);
            S[v] = s;
            for (const uint32_t c : {nd.left_idx, nd.right_idx}) {
                if (c == NO_REF || t.nodes[c].object_idx != 0xFFFFFFFFu) continue;
                for (const uint32_t g : {t.nodes[c].left_idx, t.nodes[c].right_idx})
                    if (g != NO_REF && !contains(t.aabbs[c], t.aabbs[g])) out.wide_ok = false;
            }
            uint32_t e[4];
            const int k = w.entries(t, nd, e);
            int sw = k;
            for (int i = 0; i < k; ++i)
                if (!(t.ref(e[i]) & LEAF_BIT)) sw = std::max(sw, i + SW[e[i]]);
            SW[v] = sw;
        }
    }
    out.binary = std::max(1, S[0]);
    out.wide = std::max(1, SW[0]);
    return RT_OK;
}

// inode, ibox (without the root's trailing box), wnode when `wide`, leaf, tnorm.
void pack_records(const Tree& t, const NodeIds& ids, const rt_triangle* tris, const WideRule& w, bool wide,
                  PackedScene& out) {
    out.inode.assign(16 * std::max<size_t>(ids.n_int, 1), 0.f);
    out.ibox.assign(8 * std::max<size_t>(ids.n_int, 1), 0.f);
    out.wnode.assign(wide ? 32 * std::max<size_t>(ids.n_int, 1) : 0, 0.f);
    out.leaf.assign(16 * std::max<size_t>(ids.n_leaf, 1), 0.f);
    out.tnorm.assign(12 * t.P, 0.f);
    for (size_t n = 0; n < t.NN; ++n) {
        const uint32_t c = t.cid[n];
        if (c == NO_REF) continue;
        const rt_bvh_node& nd = t.nodes[n];
        const rt_aabb& ob = t.aabbs[n];
        if (!(c & LEAF_BIT)) {
            const rt_aabb lb = nd.left_idx != NO_REF ? t.aabbs[nd.left_idx] : rt_aabb{};
            const rt_aabb rb = nd.right_idx != NO_REF ? t.aabbs[nd.right_idx] : rt_aabb{};
            float* q = &out.inode[16 * size_t(c)];  // per axis (min, max) pairs: left x y | left z, right x | right y z
            put_pairs(q, lb);
            put_pairs(q + 6, rb);
            // z: children that are leaves naming no triangle (pushed by SearchBVH all the same:
            // the deep kernels keep their stack entries)
            const uint32_t inv = (nd.left_idx != NO_REF && t.ref(nd.left_idx) == NO_REF ? 1u : 0u) |
                                 (nd.right_idx != NO_REF && t.ref(nd.right_idx) == NO_REF ? 2u : 0u);
            const uint32_t refs[4] = {t.ref(nd.left_idx), t.ref(nd.right_idx), inv, 0u};
            std::memcpy(q + 12, refs, 16);
            put_pairs(&out.ibox[8 * size_t(c)], ob);  // (x pair, y pair | z pair, 0, 0)
            if (wide) {  // 4 x (x pair, y pair, z pair) | 4 refs | unused
                float* wq = &out.wnode[32 * size_t(c)];
                uint32_t e[4], wr[4] = {NO_REF, NO_REF, NO_REF, NO_REF};
                const int k = w.entries(t, nd, e);
                for (int i = 0; i < k; ++i) {
                    put_pairs(wq + 6 * i, t.aabbs[e[i]]);
                    wr[i] = t.ref(e[i]);
                }
                std::memcpy(wq + 24, wr, sizeof(wr));
            }
        } else {
            const rt_triangle& tr = tris[nd.object_idx];
            float* q = &out.leaf[16 * size_t(c & ~LEAF_BIT)];
            const int32_t ti = int32_t(nd.object_idx);
            float tif;
            std::memcpy(&tif, &ti, 4);
            // e1 = v1 - v0, e2 = v2 - v0 exactly as intersectTriangle computes them
            // v0 | e1, e2.x | e2.y e2.z, box x pair | box y pair, box z pair
            put4(q, tr.v0.x, tr.v0.y, tr.v0.z, tif);
            put4(q + 4, tr.v1.x - tr.v0.x, tr.v1.y - tr.v0.y, tr.v1.z - tr.v0.z, tr.v2.x - tr.v0.x);
            q[8] = tr.v2.y - tr.v0.y, q[9] = tr.v2.z - tr.v0.z;
            put_pairs(q + 10, ob);
        }
    }
    for (size_t i = 0; i < t.P; ++i) {
        float* q = &out.tnorm[12 * i];
        put4(q, tris[i].n0.x, tris[i].n0.y, tris[i].n0.z, 0.f);
        put4(q + 4, tris[i].n1.x, tris[i].n1.y, tris[i].n1.z, 0.f);
        put4(q + 8, tris[i].n2.x, tris[i].n2.y, tris[i].n2.z, 0.f);
    }
}

// v0 | e1, e2.x | e2.y, e2.z by triangle index, e1/e2 as intersectTriangle computes them (deep
// trees: the brute-force completion).
void pack_triangles(size_t P, const rt_triangle* tris, std::vector<float>& tri) {
    tri.assign(12 * P, 0.f);
    for (size_t i = 0; i < P; ++i) {
        const rt_triangle& tr = tris[i];
        float* q = &tri[12 * i];
        put4(q, tr.v0.x, tr.v0.y, tr.v0.z, 0.f);
        put4(q + 4, tr.v1.x - tr.v0.x, tr.v1.y - tr.v0.y, tr.v1.z - tr.v0.z, tr.v2.x - tr.v0.x);
        q[8] = tr.v2.y - tr.v0.y, q[9] = tr.v2.z - tr.v0.z;
    }
}

// root_ref, bmax and root_box; the root's box again (pair layout) after ibox's entries, where
// the traversals' first test reads it with scalar loads like any other box (SceneView::rootb).
void pack_bounds(const Tree& t, PackedScene& out) {
    SceneMeta& m = out.meta;
    m.root_ref = t.cid[0];
    if (m.root_ref == NO_REF) m.root_ref = LEAF_BIT | 0u;  // degenerate: unreachable leaf
    // The pre-classification takes min <= max per axis (near/far bounds by the ray's sign); a
    // scene with an inverted, NaN or infinite box gets bmax = inf, which turns every float
    // classification ambiguous (make_ray: E = inf), so all its box tests take the exact path.
    bool sorted_boxes = true;
    for (size_t n = 0; n < t.NN; ++n) {
        const rt_aabb& bb = t.aabbs[n];
        m.bmax[0] = std::max({m.bmax[0], std::fabs(bb.min_corner.x), std::fabs(bb.max_corner.x)});
        m.bmax[1] = std::max({m.bmax[1], std::fabs(bb.min_corner.y), std::fabs(bb.max_corner.y)});
        m.bmax[2] = std::max({m.bmax[2], std::fabs(bb.min_corner.z), std::fabs(bb.max_corner.z)});
        sorted_boxes = sorted_boxes && bb.min_corner.x <= bb.max_corner.x && bb.min_corner.y <= bb.max_corner.y &&
                       bb.min_corner.z <= bb.max_corner.z;
    }
    for (float& v : m.bmax)
        if (!(v <= FLT_MAX) || !sorted_boxes) v = INFINITY;
    put_corners(m.root_box, t.aabbs[0]);
    if (t.cid[0] == NO_REF) {  // root names no triangle: nothing can be hit; empty box
        m.root_box[0] = m.root_box[1] = m.root_box[2] = INFINITY;
        m.root_box[3] = m.root_box[4] = m.root_box[5] = -INFINITY;
    }
    const float* r = m.root_box;
    const float rootb[8] = {r[0], r[3], r[1], r[4], r[2], r[5], 0.f, 0.f};
    out.ibox.insert(out.ibox.end(), rootb, rootb + 8);
}

// Tile-culling cut (tile_misses_scene): from the root, repeatedly replace the internal node
// with the largest box (half surface area) by its children, up to RT_TUNE_CULL_BOXES nodes: one
// box per lane of tile_cut_kernel (fewer, for tests).  Every leaf keeps exactly one
// ancestor-or-self in the set; a missing child (NO_REF) holds no leaf.
// Second level (RT_TUNE_CUT_SUB sub-boxes per cut box, a power of two <= 64): the same rule
// inside each cut node's subtree, so the tiles whose rays reach a cut box are tested against the
// boxes below it (cut_unit).  Unused slots repeat the node's first sub-box: a duplicate
// changes no "every box missed" decision.
void pack_cut(const Tree& t, PackedScene& out, RefitPlan* plan) {
    if (t.cid[0] == NO_REF || (t.cid[0] & LEAF_BIT)) return;
    const int kcut = int(std::clamp(tuning(RT_TUNE_CULL_BOXES, 64.0), 0.0, 64.0));
    auto area = [&](uint32_t n) {  // not clamped: a box with a negative area is never replaced
        const rt_aabb& bb = t.aabbs[n];
        const double dx = double(bb.max_corner.x) - bb.min_corner.x, dy = double(bb.max_corner.y) - bb.min_corner.y,
                     dz = double(bb.max_corner.z) - bb.min_corner.z;
        const double a = dx * dy + dy * dz + dz * dx;
        return a == a ? a : INFINITY;
    };
    uint32_t cutn[64] = {0u}, sn[64];
    const int ncut = expand_largest(t.nodes, t.cid, cutn, 1, kcut, false, area);
    if (kcut <= 1) return;
    out.cut.resize(size_t(6) * ncut);
    for (int i = 0; i < ncut; ++i) put_corners(&out.cut[6 * i], t.aabbs[cutn[i]]);
    if (plan)
        for (int i = 0; i < ncut; ++i) plan->cut_ref.push_back(t.cid[cutn[i]]);
    out.meta.ncut = ncut;
    const int sub = int(std::clamp(tuning(RT_TUNE_CUT_SUB, 16.0), 0.0, 64.0));
    if (sub < 2) return;
    int sl = 0;
    while ((2 << sl) <= sub) ++sl;
    const int S = 1 << sl;
    out.cut2.resize(size_t(6) * S * ncut);
    for (int i = 0; i < ncut; ++i) {
        sn[0] = cutn[i];
        int ns = expand_largest(t.nodes, t.cid, sn, 1, S, false, area);
        if (ns == 0) sn[ns++] = cutn[i];  // (an internal node without valid children)
        for (int j = 0; j < S; ++j) put_corners(&out.cut2[6 * (size_t(i) * S + j)], t.aabbs[sn[j < ns ? j : 0]]);
        if (plan)
            for (int j = 0; j < S; ++j) plan->cut2_ref.push_back(t.cid[sn[j < ns ? j : 0]]);
    }
    out.meta.cut_sub_log2 = sl;
}

// The camera rays' frustum records (build_frustum_records), for the traversal's 128-entry
// stack, and their quantised form.
void pack_frustum(const Tree& t, PackedScene& out, RefitPlan* plan) {
    // RT_TUNE_FRUSTUM_ARITY: the largest arity's log2 to try (tests; 2 = the 4-ary records)
    int fr_dmax = int(std::clamp(tuning(RT_TUNE_FRUSTUM_ARITY, 5.0), 2.0, 5.0));
#ifdef RT_NO_F16  // (variant builds for A/B runs: the frustum traversal over the 4-ary records)
    fr_dmax = 2;
#endif
    if (fr_dmax <= 2) return;
    // RT_TUNE_FRUSTUM_STACK_CAP (test hook only): records whose DFS may outgrow the stack,
    // to exercise traverse_frustum's overflow guard
    const int cap = int(std::clamp(tuning(RT_TUNE_FRUSTUM_STACK_CAP, double(FRUSTUM_STACK)), 1.0, 1e6));
    std::vector<uint32_t> rec_nodes;
    FrustumRecords fr = build_frustum_records(t.nodes, t.NN, t.cid, t.aabbs, fr_dmax, cap, plan ? &rec_nodes : nullptr);
    if (fr.log2 <= 2) return;
    if (plan)
        for (const uint32_t n : rec_nodes) plan->frec_node.push_back(t.cid[n]);
    out.meta.f_log2 = fr.log2;
    out.meta.f_bound = fr.bound;
    // RT_TUNE_QUANT_RECORDS: 1 quantised records for every scene with frustum records,
    // -1 for scenes whose float records alone exceed the big-scene threshold's eighth
    // (c5: 34 MB; frog: 0.6 MB), 0 (default) none: c5 45.5 vs 42.4 ms with them, the
    // dequantisation's VALU costing more than the halved record lines save
    // (profiles/r05/exp/quant_records_ab_c5.log)
    const double qk = tuning(RT_TUNE_QUANT_RECORDS, 0.0);
    const double big = tuning(RT_TUNE_BIG_SCENE_BYTES, double(kBigSceneBytes));
    const bool want_q = qk > 0.5 || (qk < -0.5 && double(fr.rec.size() * sizeof(float)) > big / 8.0);
    if (want_q && !build_quant_records(fr, out.qent, out.qhdr)) {
        out.qent.clear();
        out.qhdr.clear();
    }
    out.fnode = std::move(fr.rec);
}

}  // namespace

int check_scene_arrays(size_t P, const void* nodes, const void* aabbs, const void* tris) {
    if (P == 0 || !nodes || !aabbs || !tris) return set_error(RT_ERR_ARG, "rt_scene_create: empty scene");
    if (P > 0x3FFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, "more than 2^30 triangles");
    return RT_OK;
}

int classify_nodes(size_t P, const rt_bvh_node* nodes, NodeIds& ids) {
    const size_t NN = 2 * P - 1;
    ids.cid.assign(NN, NO_REF);
    ids.n_int = ids.n_leaf = 0;
    for (size_t n = 0; n < NN; ++n) {
        const rt_bvh_node& nd = nodes[n];
        if (nd.object_idx == 0xFFFFFFFFu) {
            if ((nd.left_idx != NO_REF && nd.left_idx >= NN) || (nd.right_idx != NO_REF && nd.right_idx >= NN))
                return set_error(RT_ERR_ARG, "BVH child index out of range");
            ids.cid[n] = uint32_t(ids.n_int++);
        } else if (nd.object_idx < P) {
            ids.cid[n] = LEAF_BIT | uint32_t(ids.n_leaf++);
        }  // leaves naming no valid triangle are skipped by SearchBVH (query.h:263): NO_REF
    }
    return RT_OK;
}

int check_proper_tree(size_t P, const rt_bvh_node* nodes, std::vector<uint32_t>* height) {
    const size_t NN = 2 * P - 1;
    std::vector<uint8_t> state(NN, 0);  // 0 new, 1 on path, 2 done
    std::vector<uint32_t> H(NN, 0u);
    std::vector<std::pair<uint32_t, bool>> st{{0u, false}};
    size_t reached = 0;
    while (!st.empty()) {
        auto [v, post] = st.back();
        st.pop_back();
        const rt_bvh_node& nd = nodes[v];
        const bool internal = nd.object_idx == 0xFFFFFFFFu;
        if (post) {
            state[v] = 2;
            H[v] = 1 + std::max(H[nd.left_idx], H[nd.right_idx]);
            continue;
        }
        if (state[v] == 1) return set_error(RT_ERR_ARG, "BVH contains a cycle");
        if (state[v] == 2) return set_error(RT_ERR_UNSUPPORTED, "refit: a node has two parents");
        ++reached;
        if (!internal) {
            if (nd.object_idx >= P) return set_error(RT_ERR_UNSUPPORTED, "refit: a leaf names no triangle");
            state[v] = 2;
            continue;
        }
        if (nd.left_idx == NO_REF || nd.right_idx == NO_REF)
            return set_error(RT_ERR_UNSUPPORTED, "refit: an internal node lacks a child");
        if (nd.left_idx >= NN || nd.right_idx >= NN) return set_error(RT_ERR_ARG, "BVH child index out of range");
        state[v] = 1;
        st.push_back({v, true});
        st.push_back({nd.left_idx, false});
        st.push_back({nd.right_idx, false});
    }
    if (reached != NN) return set_error(RT_ERR_UNSUPPORTED, "refit: a node is not reachable from the root");
    if (height) *height = std::move(H);
    return RT_OK;
}

namespace {

// The bottom-up schedule of a proper tree: its internal nodes' compact ids by height.
int plan_schedule(const Tree& t, const NodeIds& ids, RefitPlan& plan) {
    std::vector<uint32_t> height;
    if (int rc = check_proper_tree(t.P, t.nodes, &height); rc != RT_OK) return rc;
    plan.n_int = ids.n_int;
    plan.n_leaf = ids.n_leaf;
    const uint32_t top = height[0];
    std::vector<uint32_t> count(size_t(top) + 1, 0u);
    for (size_t n = 0; n < t.NN; ++n)
        if (height[n] > 0) ++count[height[n]];
    plan.level_off.assign(size_t(top) + 1, 0u);  // level_off[h]: the end of level h (level_off[0] = 0)
    for (uint32_t h = 1; h <= top; ++h) plan.level_off[h] = plan.level_off[h - 1] + count[h];
    plan.order.assign(ids.n_int, 0u);
    std::vector<uint32_t> at(plan.level_off.begin(), plan.level_off.end());
    for (size_t n = 0; n < t.NN; ++n)  // array order is compact-id order
        if (height[n] > 0) plan.order[at[height[n] - 1]++] = t.cid[n];
    return RT_OK;
}

}  // namespace

int pack_scene(size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs, const rt_triangle* tris, PackedScene& out,
               RefitPlan* plan) {
    int rc = check_scene_arrays(P, nodes, aabbs, tris);
    if (rc != RT_OK) return rc;
    out = PackedScene();
    NodeIds ids;
    if ((rc = classify_nodes(P, nodes, ids)) != RT_OK) return rc;
    const Tree t{P, 2 * P - 1, nodes, aabbs, ids.cid.data()};
    const WideRule w(t);
    StackBounds sb;
    if ((rc = stack_bounds(t, w, sb)) != RT_OK) return rc;
    if (plan) {
        *plan = RefitPlan();
        if ((rc = plan_schedule(t, ids, *plan)) != RT_OK) return rc;
    }
    // A tree whose DFS may need more than the 64-entry wave stack is rendered by the MODE_DEEP
    // kernels (the reference's 512-entry stack).  traverse_wave_split addresses records by 32-bit
    // byte offsets (ref << 7 into the 4-ary array, << 5 into ibox, slot << 6 into the leaves):
    // larger trees take those kernels too, which are exact for any tree.
    const bool deep = sb.binary > STACK_CAP || ids.n_int >= (size_t(1) << 25) || ids.n_leaf >= (size_t(1) << 26);
    const bool wide_ok = sb.wide_ok && !deep && sb.wide <= STACK_CAP;
    SceneMeta& m = out.meta;
    m.P = P;
    out.binary_stack = sb.binary;
    out.wide_stack = sb.wide;
    pack_records(t, ids, tris, w, wide_ok, out);
    pack_bounds(t, out);
    pack_cut(t, out, plan);
    m.wide = wide_ok && !(m.root_ref & LEAF_BIT);
    m.lane_stack = !deep && sb.binary <= LANE_LDS_CAP;
    m.lane_wide = m.wide && m.lane_stack && sb.wide <= LANE_LDS_CAP;
    m.deep = deep;
    if (m.wide) pack_frustum(t, out, plan);
    if (deep) pack_triangles(P, tris, out.tri);
    if (plan && !out.qent.empty())  // (their grids are per record: a refit would have to re-quantise)
        return set_error(RT_ERR_UNSUPPORTED, "refit: quantised records (RT_TUNE_QUANT_RECORDS) are not refitted");
    return RT_OK;
}

namespace {

uint32_t word(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// A node's current box in the packed arrays, per axis (min, max): an internal node's ibox entry, a
// leaf's record words 10-15.
const float* box_of(const PackedScene& pk, uint32_t ref) {
    return ref & LEAF_BIT ? &pk.leaf[16 * size_t(ref & ~LEAF_BIT) + 10] : &pk.ibox[8 * size_t(ref)];
}
void pairs_to_corners(float* q, const float* b) { put4(q, b[0], b[2], b[4], b[1]), q[4] = b[3], q[5] = b[5]; }

bool finite_vertices(size_t P, const rt_triangle* tris) {
    for (size_t i = 0; i < P; ++i)
        for (const rt_vec3& v : {tris[i].v0, tris[i].v1, tris[i].v2})
            if (!std::isfinite(v.x) || !std::isfinite(v.y) || !std::isfinite(v.z)) return false;
    return true;
}

}  // namespace

int refit_packed(PackedScene& pk, const RefitPlan& plan, const rt_triangle* tris) {
    const size_t P = pk.meta.P;
    if (!tris) return set_error(RT_ERR_ARG, "refit: null triangles");
    if (!finite_vertices(P, tris)) return set_error(RT_ERR_ARG, "refit: a vertex coordinate is not finite");
    // 1, 2: the leaves' boxes and v0 | e1 | e2 (pack_records), tnorm, tri (pack_triangles)
    for (size_t j = 0; j < plan.n_leaf; ++j) {
        float* q = &pk.leaf[16 * j];
        const rt_triangle& tr = tris[word(q[3])];
        const float tif = q[3];
        put4(q, tr.v0.x, tr.v0.y, tr.v0.z, tif);
        put4(q + 4, tr.v1.x - tr.v0.x, tr.v1.y - tr.v0.y, tr.v1.z - tr.v0.z, tr.v2.x - tr.v0.x);
        q[8] = tr.v2.y - tr.v0.y, q[9] = tr.v2.z - tr.v0.z;
        put_pairs(q + 10, aabb_of_triangle(tr.v0, tr.v1, tr.v2));
    }
    for (size_t i = 0; i < P; ++i) {
        float* q = &pk.tnorm[12 * i];
        put4(q, tris[i].n0.x, tris[i].n0.y, tris[i].n0.z, 0.f);
        put4(q + 4, tris[i].n1.x, tris[i].n1.y, tris[i].n1.z, 0.f);
        put4(q + 8, tris[i].n2.x, tris[i].n2.y, tris[i].n2.z, 0.f);
    }
    if (!pk.tri.empty()) pack_triangles(P, tris, pk.tri);
    // 3: internal boxes bottom-up, merge(left, right); with them the inode child boxes
    for (const uint32_t i : plan.order) {
        float* q = &pk.inode[16 * size_t(i)];
        const float* l = box_of(pk, word(q[12]));
        const float* r = box_of(pk, word(q[13]));
        float m[6];
        for (int k = 0; k < 6; k += 2) m[k] = fminf(l[k], r[k]), m[k + 1] = fmaxf(l[k + 1], r[k + 1]);
        std::copy(l, l + 6, q);
        std::copy(r, r + 6, q + 6);
        std::copy(m, m + 6, &pk.ibox[8 * size_t(i)]);
    }
    // 4: every other stored box from its node
    const float* root = box_of(pk, pk.meta.root_ref);
    std::copy(root, root + 6, &pk.ibox[8 * std::max<size_t>(plan.n_int, 1)]);
    for (size_t i = 0; i < (pk.wnode.empty() ? 0 : plan.n_int); ++i) {
        float* wq = &pk.wnode[32 * i];
        for (int e = 0; e < 4; ++e)
            if (word(wq[24 + e]) != NO_REF) std::copy_n(box_of(pk, word(wq[24 + e])), 6, wq + 6 * e);
    }
    const size_t A = size_t(1) << pk.meta.f_log2;
    for (size_t r = 0; r < (pk.fnode.empty() ? 0 : plan.frec_node.size()); ++r) {
        float* w = &pk.fnode[8 * A * r];
        for (size_t i = 0; i < A; ++i) {
            const uint32_t ref = word(w[6 * A + i]);
            if (ref == NO_REF) continue;
            std::copy_n(box_of(pk, ref & LEAF_BIT ? ref : plan.frec_node[ref]), 6, w + 6 * i);
        }
    }
    for (size_t s = 0; s < plan.cut_ref.size() && 6 * s < pk.cut.size(); ++s)
        pairs_to_corners(&pk.cut[6 * s], box_of(pk, plan.cut_ref[s]));
    for (size_t s = 0; s < plan.cut2_ref.size() && 6 * s < pk.cut2.size(); ++s)
        pairs_to_corners(&pk.cut2[6 * s], box_of(pk, plan.cut2_ref[s]));
    // root_box, and bmax: the boxes are nested and finite, so the root's |coordinates| bound them all
    SceneMeta& m = pk.meta;
    pairs_to_corners(m.root_box, root);
    for (int a = 0; a < 3; ++a) m.bmax[a] = std::max(std::fabs(root[2 * a]), std::fabs(root[2 * a + 1]));
    return RT_OK;
}

int rebuild_pack(size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs, const rt_triangle* tris, PackedScene& out,
                 RefitPlan& plan) {
    if (!tris) return set_error(RT_ERR_ARG, "rebuild: null triangles");
    if (!finite_vertices(P, tris)) return set_error(RT_ERR_ARG, "rebuild: a vertex coordinate is not finite");
    return pack_scene(P, nodes, aabbs, tris, out, &plan);
}

void scene_info_words(const SceneMeta& m, int binary_stack, int wide_stack, int64_t info[21]) {
    const int64_t facts[12] = {int64_t(m.P), m.root_ref,  m.ncut, m.cut_sub_log2, m.wide,       m.lane_stack,
                               m.lane_wide,  m.deep,      m.f_log2, m.f_bound,    binary_stack, wide_stack};
    std::copy(facts, facts + 12, info);
    uint32_t bits[9];
    std::memcpy(bits, m.root_box, sizeof(m.root_box));
    std::memcpy(bits + 6, m.bmax, sizeof(m.bmax));
    std::copy(bits, bits + 9, info + 12);
}

uint64_t fnv1a(const void* data, size_t bytes) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t b = 0; b < bytes; ++b) h = (h ^ static_cast<const uint8_t*>(data)[b]) * 0x100000001b3ull;
    return h;
}

}  // namespace rt

using rt::set_error;

// Host-only view of build_frustum_records for the CPU tests (no device), over the ids and the
// checks of pack_scene: as strict as rt_scene_create, so an out-of-range child of an internal
// node the root does not reach is refused too.  info: log2, bound, record count.  rec: copied
// when rec_cap (floats) suffices.
extern "C" int rt_debug_frustum_records(size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs, int max_log2,
                                        int stack_cap, int64_t* info, float* rec, size_t rec_cap) {
    if (P == 0 || !nodes || !aabbs || !info) return set_error(RT_ERR_ARG, "rt_debug_frustum_records: null argument");
    if (P > 0x3FFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, "more than 2^30 triangles");
    rt::NodeIds ids;
    int rc = rt::classify_nodes(P, nodes, ids);
    if (rc != RT_OK) return rc;
    const rt::Tree t{P, 2 * P - 1, nodes, aabbs, ids.cid.data()};
    rt::StackBounds sb;
    if ((rc = rt::stack_bounds(t, rt::WideRule(t), sb)) != RT_OK) return rc;  // (the cycle check)
    if (nodes[0].object_idx != 0xFFFFFFFFu) {  // a leaf root: no records (rt_scene_create makes none)
        info[0] = 2;
        info[1] = 0;
        info[2] = 0;
        return RT_OK;
    }
    const rt::FrustumRecords fr = rt::build_frustum_records(nodes, t.NN, t.cid, aabbs, std::clamp(max_log2, 2, 5), stack_cap);
    info[0] = fr.log2;
    info[1] = fr.bound;
    info[2] = (int64_t)fr.nrec;
    if (rec && rec_cap >= fr.rec.size() && !fr.rec.empty()) std::memcpy(rec, fr.rec.data(), fr.rec.size() * sizeof(float));
    return RT_OK;
}

// rt::box_weight (rt_records.hpp) for the tests, beside the device build's rt_debug_box_weight_batch:
// boxes n x (min corner, max corner), leaves n.
extern "C" int rt_debug_box_weight_host(const float* boxes, const uint32_t* leaves, int rule, int n, double* out) {
    if (n < 0 || (n > 0 && (!boxes || !leaves || !out))) return set_error(RT_ERR_ARG, "rt_debug_box_weight_host: bad args");
    for (int i = 0; i < n; ++i) {
        const float* b = boxes + 6 * size_t(i);
        out[i] = rt::box_weight(rt_aabb{{b[0], b[1], b[2]}, {b[3], b[4], b[5]}}, rule, leaves[i]);
    }
    return RT_OK;
}

// SceneMeta::query_variant for the tests: the caller queries' variant rule on the four facts it reads.
extern "C" int rt_debug_query_variant(int wide, int lane_stack, int lane_wide, int deep, int flags) {
    rt::SceneMeta m;
    m.wide = wide != 0, m.lane_stack = lane_stack != 0, m.lane_wide = lane_wide != 0, m.deep = deep != 0;
    return m.query_variant(flags);
}

static void digest_pack(const rt::PackedScene& pk, int64_t info[21], uint64_t digests[22]) {
    rt::scene_info_words(pk.meta, pk.binary_stack, pk.wide_stack, info);
    size_t i = 0;
    for (const rt::PackedArray& a : pk.arrays()) {
        digests[i++] = a.bytes;
        digests[i++] = rt::fnv1a(a.data, a.bytes);
    }
}

// pack_scene on the host for the CPU tests (no device).  info: P, root_ref, ncut, cut_sub_log2,
// wide, lane_stack, lane_wide, deep, f_log2, f_bound, binary stack bound, 4-ary stack bound, then
// the bit patterns of root_box[6] and bmax[3]; digests: per array of PackedScene::arrays(), its
// byte length and the 64-bit FNV-1a hash of its bytes.
extern "C" int rt_debug_scene_pack(size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs, const rt_triangle* tris,
                                   int64_t info[21], uint64_t digests[22]) {
    if (!info || !digests) return set_error(RT_ERR_ARG, "rt_debug_scene_pack: null argument");
    rt::PackedScene pk;
    const int rc = rt::pack_scene(P, nodes, aabbs, tris, pk);
    if (rc != RT_OK) return rc;
    digest_pack(pk, info, digests);
    return RT_OK;
}

// pack_scene on (nodes, aabbs, tris), then rt::refit_packed with new_tris: the host restatement of
// rt_scene_create_refittable + rt_scene_refit, in rt_debug_scene_pack's words.
extern "C" int rt_debug_scene_refit_pack(size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs, const rt_triangle* tris,
                                         const rt_triangle* new_tris, int64_t info[21], uint64_t digests[22]) {
    return rt_debug_scene_refit_chain(P, nodes, aabbs, tris, 1, &new_tris, info, digests);
}

// ... with n refits in turn (poses[0], then poses[1], ...).
extern "C" int rt_debug_scene_refit_chain(size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs, const rt_triangle* tris,
                                          int n, const rt_triangle* const* poses, int64_t info[21], uint64_t digests[22]) {
    if (!info || !digests || !poses || n < 0) return set_error(RT_ERR_ARG, "rt_debug_scene_refit_chain: bad argument");
    rt::PackedScene pk;
    rt::RefitPlan plan;
    int rc = rt::pack_scene(P, nodes, aabbs, tris, pk, &plan);
    if (rc != RT_OK) return rc;
    for (int i = 0; i < n; ++i)
        if ((rc = rt::refit_packed(pk, plan, poses[i])) != RT_OK) return rc;
    digest_pack(pk, info, digests);
    return RT_OK;
}

// The boxes a refit gives the caller's tree, by node: aabb_of_triangle per leaf, merge(left, right)
// bottom-up.  RT_ERR_UNSUPPORTED unless the tree is proper (rt_scene_create_refittable's rule).
extern "C" int rt_refit_aabbs_host(size_t P, const rt_bvh_node* nodes, const rt_triangle* tris, rt_aabb* aabbs_out) {
    int rc = rt::check_scene_arrays(P, nodes, aabbs_out, tris);
    if (rc != RT_OK) return rc;
    std::vector<uint32_t> height;
    if ((rc = rt::check_proper_tree(P, nodes, &height)) != RT_OK) return rc;
    const size_t NN = 2 * P - 1;
    std::vector<uint32_t> order;  // internal nodes by height: children before parents
    for (size_t n = 0; n < NN; ++n) {
        if (height[n] > 0) {
            order.push_back(uint32_t(n));
            continue;
        }
        const rt_triangle& tr = tris[nodes[n].object_idx];
        aabbs_out[n] = rt::aabb_of_triangle(tr.v0, tr.v1, tr.v2);
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return height[a] < height[b]; });
    for (const uint32_t n : order) aabbs_out[n] = rt::aabb_merge(aabbs_out[nodes[n].left_idx], aabbs_out[nodes[n].right_idx]);
    return RT_OK;
}
