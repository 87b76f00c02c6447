// Stand-alone driver of rt::pack_scene for a sanitizer build (tests/test_pack_sanitize.py
// compiles it with the host units under -fsanitize=address,undefined and runs it): the hand-made
// degenerate trees of tests/test_scene_pack.py, a few hundred random small trees (P <= 32, fixed
// seed) and malformed ones, each under a few knob settings.  Exit status 0 when every tree packs
// (or is refused) as expected; a sanitizer finding aborts the run.
#include <cmath>
#include <cstdio>
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

rt_bvh_node leaf(uint32_t parent, uint32_t obj) { return rt_bvh_node{parent, NONE, NONE, obj}; }
rt_aabb box(float x0, float y0, float z0, float x1, float y1, float z1) { return rt_aabb{{x0, y0, z0}, {x1, y1, z1}}; }

Scene scene(size_t P, std::vector<rt_bvh_node> nodes, std::vector<rt_aabb> aabbs) {
    Scene s{P, std::move(nodes), std::move(aabbs), std::vector<rt_triangle>(P)};
    for (size_t i = 0; i < P; ++i) {
        const float f = float(i);
        s.tris[i] = rt_triangle{{f, 0, 0}, {f + 1, 0, 0.25f * f}, {f, 1, 0}, {0, 0, 1}, {0, 0, 1}, {0, 0, 1}};
    }
    return s;
}

std::vector<Scene> hand_made() {
    const std::vector<rt_bvh_node> full = {{NONE, 1, 2, NONE}, {0, 3, 4, NONE}, {0, 5, 6, NONE}, leaf(1, 0),
                                           leaf(1, 1),         leaf(2, 2),      leaf(2, 3)};
    const std::vector<rt_bvh_node> two = {{NONE, 1, 2, NONE}, leaf(0, 0), leaf(0, 1)};
    return {
        scene(1, {leaf(NONE, 0)}, {box(0, 0, 0, 1, 1, 0)}),
        scene(1, {leaf(NONE, 5)}, {box(0, 0, 0, 1, 1, 0)}),
        scene(3, {{NONE, 1, 2, NONE}, {0, 3, NONE, NONE}, leaf(0, 0), leaf(1, 1), leaf(NONE, 2)},
              {box(0, 0, 0, 3, 1, 1), box(0, 0, 0, 2, 1, 1), box(2, 0, 0, 3, 1, 1), box(0, 0, 0, 2, 1, 0.5f), box(5, 5, 5, 6, 6, 6)}),
        scene(4, full,
              {box(0, 0, 0, 4, 1, 1), box(0, 0, 0, 2, 1, 1), box(2, 0, 0, 4, 1, 1), box(0, -0.5f, 0, 1, 1, 1), box(1, 0, 0, 2, 1, 1),
               box(2, 0, 0, 3, 1, 1), box(3, 0, 0, 4, 1, 1)}),
        scene(2, two, {box(0, 0, 0, 2, 1, 1), box(1, 0, 0, 0.5f, 1, 1), box(1, 0, 0, 2, 1, 1)}),
        scene(2, two, {box(0, 0, 0, 2, 1, 1), box(0, 0, 0, 1, 1, 1), box(1, 0, NAN, 2, 1, 1)}),
    };
}

// A random binary tree over P leaves (2P-1 nodes, root 0).  `loose`: random boxes instead of the
// children's unions; some leaves name no valid triangle, some internal nodes lose a child.
Scene random_tree(std::mt19937& rng, size_t P, bool loose) {
    const size_t NN = 2 * P - 1;
    std::vector<rt_bvh_node> nodes(NN, leaf(NONE, 0));
    std::vector<rt_aabb> aabbs(NN);
    std::uniform_real_distribution<float> U(-4.f, 4.f);
    uint32_t next = 1, obj = 0;
    std::function<void(uint32_t, size_t)> grow = [&](uint32_t n, size_t k) {
        if (k == 1) {
            nodes[n].object_idx = rng() % 8 == 0 ? uint32_t(P + rng() % 5) : obj;
            ++obj;
            const float x = U(rng), y = U(rng), z = U(rng);
            aabbs[n] = box(x, y, z, x + 0.5f, y + 0.5f, z + 0.5f);
            return;
        }
        const size_t a = 1 + rng() % (k - 1);
        const uint32_t l = next, r = next + 1;
        next += 2;
        nodes[n] = rt_bvh_node{nodes[n].parent_idx, l, r, NONE};
        nodes[l].parent_idx = nodes[r].parent_idx = n;
        grow(l, a);
        grow(r, k - a);
        const rt_aabb &A = aabbs[l], &B = aabbs[r];
        aabbs[n] = box(std::fmin(A.min_corner.x, B.min_corner.x), std::fmin(A.min_corner.y, B.min_corner.y),
                       std::fmin(A.min_corner.z, B.min_corner.z), std::fmax(A.max_corner.x, B.max_corner.x),
                       std::fmax(A.max_corner.y, B.max_corner.y), std::fmax(A.max_corner.z, B.max_corner.z));
        if (loose && rng() % 4 == 0) aabbs[n] = box(U(rng), U(rng), U(rng), U(rng), U(rng), U(rng));
        if (loose && rng() % 16 == 0) (rng() % 2 ? nodes[n].left_idx : nodes[n].right_idx) = NONE;
    };
    grow(0, P);
    return scene(P, std::move(nodes), std::move(aabbs));
}

int failures = 0;
void expect(bool ok, const char* what, size_t i) {
    if (ok) return;
    std::fprintf(stderr, "tree %zu: %s (%s)\n", i, what, rt_last_error());
    ++failures;
}

void pack_all(const std::vector<Scene>& scenes) {
    for (size_t i = 0; i < scenes.size(); ++i) {
        const Scene& s = scenes[i];
        rt::PackedScene pk;
        const int rc = rt::pack_scene(s.P, s.nodes.data(), s.aabbs.data(), s.tris.data(), pk);
        expect(rc == RT_OK, "pack_scene refused a valid tree", i);
        if (rc != RT_OK) continue;
        expect(pk.tnorm.size() == 12 * s.P && pk.ibox.size() == pk.inode.size() / 2 + 8, "array sizes", i);
        expect(pk.cut.size() == size_t(6) * pk.meta.ncut && pk.meta.ncut <= 64, "cut size", i);
        expect(pk.cut2.size() == (pk.meta.cut_sub_log2 ? (size_t(6) << pk.meta.cut_sub_log2) * pk.meta.ncut : 0), "cut2 size", i);
        expect(pk.tri.empty() == !pk.meta.deep && (!pk.meta.wide || !pk.wnode.empty()), "deep / wide arrays", i);
    }
}
}  // namespace

int main() {
    std::mt19937 rng(20240607u);
    std::vector<Scene> scenes = hand_made();
    for (int k = 0; k < 300; ++k) scenes.push_back(random_tree(rng, 1 + rng() % 32, k % 2 == 1));
    const struct { int id; double value; } settings[] = {
        {-1, 0},
        {RT_TUNE_WIDE4_GREEDY, 0}, {RT_TUNE_WIDE4_GREEDY, 2}, {RT_TUNE_CULL_BOXES, 1}, {RT_TUNE_CULL_BOXES, 3}, {RT_TUNE_CUT_SUB, 0},
        {RT_TUNE_CUT_SUB, 64}, {RT_TUNE_FRUSTUM_ARITY, 3}, {RT_TUNE_FRUSTUM_STACK_CAP, 4}, {RT_TUNE_QUANT_RECORDS, 1},
        {RT_TUNE_RECORD_GREEDY, 0}, {RT_TUNE_RECORD_GREEDY, 1}};
    for (const auto& st : settings) {
        rt_tuning_reset();
        if (st.id >= 0 && rt_tuning_set(st.id, st.value) != RT_OK) return 2;
        pack_all(scenes);
    }
    rt_tuning_reset();
    // malformed: a child past the arrays, a cycle through the root
    for (size_t i = 0; i < scenes.size(); ++i) {
        Scene s = scenes[i];
        if (s.P < 3 || s.nodes[0].object_idx != NONE) continue;
        rt::PackedScene pk;
        Scene past = s;
        past.nodes[0].left_idx = uint32_t(2 * s.P - 1 + i % 3);
        expect(rt::pack_scene(past.P, past.nodes.data(), past.aabbs.data(), past.tris.data(), pk) == RT_ERR_ARG, "child past the arrays", i);
        Scene loop = s;
        loop.nodes[0].right_idx = 0;
        expect(rt::pack_scene(loop.P, loop.nodes.data(), loop.aabbs.data(), loop.tris.data(), pk) == RT_ERR_ARG, "cycle", i);
    }
    rt::PackedScene pk;
    expect(rt::pack_scene(0, nullptr, nullptr, nullptr, pk) == RT_ERR_ARG, "empty scene", 0);
    std::printf("%zu trees x %zu settings packed, %d failures\n", scenes.size(), sizeof(settings) / sizeof(settings[0]), failures);
    return failures ? 1 : 0;
}
