// Stand-alone driver of the refit's host side for a sanitizer build (tests/test_refit_sanitize.py
// compiles it with the host units under -fsanitize=address,undefined and runs it): rt::pack_scene
// with a refit plan, rt::refit_packed and rt_refit_aabbs_host over a few hundred random proper
// trees (P <= 40, fixed seed) under a few knob settings, and over improper trees and poses that
// must be refused.  Per tree: a pose doubled exactly refits to the plain pack of the doubled
// scene, A -> B -> A returns A's arrays, the root box is rt_refit_aabbs_host's, a NaN pose changes
// nothing.  Exit status 0 when all of it holds; a sanitizer finding aborts the run.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <random>
#include <vector>

#include "rt_common.hpp"
#include "rt_scene_pack.hpp"

namespace {
constexpr uint32_t NONE = 0xFFFFFFFFu;

struct Scene {
    size_t P;
    std::vector<rt_bvh_node> nodes;
    std::vector<rt_aabb> aabbs;
    std::vector<rt_triangle> tris;
};

std::vector<rt_triangle> random_pose(std::mt19937& rng, size_t P, int kind) {
    std::uniform_real_distribution<float> U(-4.f, 4.f);
    std::vector<rt_triangle> t(P);
    for (rt_triangle& tr : t) {
        rt_vec3* v[3] = {&tr.v0, &tr.v1, &tr.v2};
        for (rt_vec3* p : v) *p = rt_vec3{U(rng), U(rng), kind == 1 ? 0.f : U(rng)};  // 1: flat
        if (kind == 2) tr.v1 = tr.v2 = tr.v0;                                           // 2: points
        tr.n0 = tr.n1 = tr.n2 = rt_vec3{U(rng), U(rng), U(rng)};
    }
    return t;
}

// A random proper binary tree over P leaves (2P-1 nodes, root 0, leaves naming a random
// permutation of the triangles), its boxes rt_refit_aabbs_host's.
Scene random_tree(std::mt19937& rng, size_t P) {
    const size_t NN = 2 * P - 1;
    Scene s{P, std::vector<rt_bvh_node>(NN, rt_bvh_node{NONE, NONE, NONE, 0}), std::vector<rt_aabb>(NN), random_pose(rng, P, 0)};
    std::vector<uint32_t> perm(P);
    for (size_t i = 0; i < P; ++i) perm[i] = uint32_t(i);
    std::shuffle(perm.begin(), perm.end(), rng);
    uint32_t next = 1, obj = 0;
    std::function<void(uint32_t, size_t)> grow = [&](uint32_t n, size_t k) {
        if (k == 1) {
            s.nodes[n].object_idx = perm[obj++];
            return;
        }
        const size_t a = 1 + rng() % (k - 1);
        const uint32_t l = next, r = next + 1;
        next += 2;
        s.nodes[n] = rt_bvh_node{s.nodes[n].parent_idx, l, r, NONE};
        s.nodes[l].parent_idx = s.nodes[r].parent_idx = n;
        grow(l, a);
        grow(r, k - a);
    };
    grow(0, P);
    if (rt_refit_aabbs_host(P, s.nodes.data(), s.tris.data(), s.aabbs.data()) != RT_OK) s.P = 0;
    return s;
}

int failures = 0;
void expect(bool ok, const char* what, size_t i) {
    if (ok) return;
    std::fprintf(stderr, "tree %zu: %s (%s)\n", i, what, rt_last_error());
    ++failures;
}

bool same_arrays(const rt::PackedScene& a, const rt::PackedScene& b) {
    const auto x = a.arrays(), y = b.arrays();
    for (size_t i = 0; i < x.size(); ++i)
        if (x[i].bytes != y[i].bytes || (x[i].bytes && std::memcmp(x[i].data, y[i].data, x[i].bytes) != 0)) return false;
    return std::memcmp(a.meta.root_box, b.meta.root_box, sizeof(a.meta.root_box)) == 0 &&
           std::memcmp(a.meta.bmax, b.meta.bmax, sizeof(a.meta.bmax)) == 0;
}

void refit_all(std::mt19937& rng, const std::vector<Scene>& scenes, bool quantised) {
    for (size_t i = 0; i < scenes.size(); ++i) {
        const Scene& s = scenes[i];
        rt::PackedScene pk, plain;
        rt::RefitPlan plan;
        const int rc = rt::pack_scene(s.P, s.nodes.data(), s.aabbs.data(), s.tris.data(), pk, &plan);
        if (quantised && rc == RT_ERR_UNSUPPORTED) continue;  // (trees with frustum records)
        expect(rc == RT_OK, "pack_scene with a plan refused a proper tree", i);
        if (rc != RT_OK) continue;
        expect(rt::pack_scene(s.P, s.nodes.data(), s.aabbs.data(), s.tris.data(), plain) == RT_OK && same_arrays(pk, plain),
               "the plan changed the arrays", i);
        expect(plan.n_int == s.P - 1 && plan.n_leaf == s.P && plan.order.size() == plan.n_int, "plan sizes", i);
        // identity, then an exact doubling: the plain pack of the doubled scene
        expect(rt::refit_packed(pk, plan, s.tris.data()) == RT_OK && same_arrays(pk, plain), "identity refit", i);
        std::vector<rt_triangle> twice = s.tris;
        std::vector<rt_aabb> boxes2(s.aabbs.size());
        for (rt_triangle& tr : twice)
            for (rt_vec3* p : {&tr.v0, &tr.v1, &tr.v2}) *p = rt_vec3{2 * p->x, 2 * p->y, 2 * p->z};
        expect(rt_refit_aabbs_host(s.P, s.nodes.data(), twice.data(), boxes2.data()) == RT_OK, "refit boxes", i);
        expect(rt::pack_scene(s.P, s.nodes.data(), boxes2.data(), twice.data(), plain) == RT_OK, "pack of the doubled scene", i);
        expect(rt::refit_packed(pk, plan, twice.data()) == RT_OK && same_arrays(pk, plain), "doubled refit", i);
        // A, B (flat or points), A
        const std::vector<rt_triangle> A = random_pose(rng, s.P, 0), B = random_pose(rng, s.P, 1 + int(i % 2));
        expect(rt::refit_packed(pk, plan, A.data()) == RT_OK, "refit A", i);
        const rt::PackedScene atA = pk;
        std::vector<rt_aabb> boxesA(s.aabbs.size());
        expect(rt_refit_aabbs_host(s.P, s.nodes.data(), A.data(), boxesA.data()) == RT_OK, "boxes of A", i);
        const float* r = pk.meta.root_box;
        const rt_aabb& b0 = boxesA[0];
        expect(r[0] == b0.min_corner.x && r[1] == b0.min_corner.y && r[2] == b0.min_corner.z && r[3] == b0.max_corner.x &&
                   r[4] == b0.max_corner.y && r[5] == b0.max_corner.z,
               "root box", i);
        expect(rt::refit_packed(pk, plan, B.data()) == RT_OK && !same_arrays(pk, atA), "refit B", i);
        expect(rt::refit_packed(pk, plan, A.data()) == RT_OK && same_arrays(pk, atA), "A again", i);
        // a pose with a NaN or an infinity is refused and changes nothing
        std::vector<rt_triangle> bad = B;
        (i % 2 ? bad[s.P - 1].v2.z : bad[0].v0.x) = i % 3 ? NAN : INFINITY;
        expect(rt::refit_packed(pk, plan, bad.data()) == RT_ERR_ARG && same_arrays(pk, atA), "a pose that is not finite", i);
    }
}
}  // namespace

int main() {
    std::mt19937 rng(20240923u);
    std::vector<Scene> scenes;
    for (int k = 0; k < 200; ++k) scenes.push_back(random_tree(rng, k < 3 ? size_t(k + 1) : 1 + rng() % 40));
    for (size_t i = 0; i < scenes.size(); ++i) expect(scenes[i].P > 0, "rt_refit_aabbs_host refused a proper tree", i);
    const struct { int id; double value; } settings[] = {
        {-1, 0}, {RT_TUNE_WIDE4_GREEDY, 0}, {RT_TUNE_CULL_BOXES, 3}, {RT_TUNE_CUT_SUB, 64}, {RT_TUNE_CUT_SUB, 0},
        {RT_TUNE_FRUSTUM_ARITY, 3}, {RT_TUNE_FRUSTUM_STACK_CAP, 4}, {RT_TUNE_RECORD_GREEDY, 0}, {RT_TUNE_QUANT_RECORDS, 1}};
    for (const auto& st : settings) {
        rt_tuning_reset();
        if (st.id >= 0 && rt_tuning_set(st.id, st.value) != RT_OK) return 2;
        refit_all(rng, scenes, st.id == RT_TUNE_QUANT_RECORDS);
    }
    rt_tuning_reset();
    // improper trees: a leaf naming no triangle, a missing child, an unreachable node (a shared child)
    size_t refused = 0;
    for (size_t i = 0; i < scenes.size(); ++i) {
        const Scene& s = scenes[i];
        if (s.P < 3) continue;
        rt::PackedScene pk;
        rt::RefitPlan plan;
        std::vector<rt_aabb> out(s.aabbs.size());
        for (int what = 0; what < 3; ++what) {
            Scene t = s;
            if (what == 0) t.nodes[2 * s.P - 2].object_idx = uint32_t(s.P + i % 4);  // (the last node is a leaf)
            if (what == 1) t.nodes[0].right_idx = NONE;
            if (what == 2) t.nodes[0].right_idx = t.nodes[0].left_idx;
            expect(rt::pack_scene(t.P, t.nodes.data(), t.aabbs.data(), t.tris.data(), pk, &plan) == RT_ERR_UNSUPPORTED,
                   "pack_scene planned an improper tree", i);
            expect(rt_refit_aabbs_host(t.P, t.nodes.data(), t.tris.data(), out.data()) == RT_ERR_UNSUPPORTED,
                   "rt_refit_aabbs_host took an improper tree", i);
            ++refused;
        }
    }
    std::printf("%zu trees x %zu settings refitted, %zu improper trees refused, %d failures\n", scenes.size(),
                sizeof(settings) / sizeof(settings[0]), refused, failures);
    return failures ? 1 : 0;
}
