// Stand-alone driver of the rebuild's host side for a sanitizer build (tests/test_rebuild_sanitize.py
// compiles it with the host units under -fsanitize=address,undefined and runs it):
// rt_build_bvh_triangles, the record weight (rt_debug_box_weight_host) and the host half of
// rt_scene_rebuild's host path (rt::rebuild_pack: the finite check, then rt::pack_scene with a plan
// of the built tree) over random triangle sets (fixed seed) that include P = 1, 2, 3, identical
// triangles and a vertex that is not finite, under a few knob settings.  Per set: the tree is
// rt_build_bvh's over the flattened vertices, internal nodes first; the pack equals the plain pack
// and its plan refits the scene to its own pose unchanged; a pose that is not finite is refused.
// Exit status 0 when all of it holds; a sanitizer finding aborts the run.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "rt_common.hpp"
#include "rt_scene_pack.hpp"

extern "C" int rt_debug_box_weight_host(const float* boxes, const uint32_t* leaves, int rule, int n, double* out);

namespace {
constexpr uint32_t NONE = 0xFFFFFFFFu;
int failures = 0;
void expect(bool ok, const char* what, size_t i) {
    if (ok) return;
    std::fprintf(stderr, "set %zu: %s (%s)\n", i, what, rt_last_error());
    ++failures;
}

std::vector<rt_triangle> random_tris(std::mt19937& rng, size_t P, int kind) {
    std::uniform_real_distribution<float> U(-4.f, 4.f);
    std::vector<rt_triangle> t(P);
    for (rt_triangle& tr : t) {
        for (rt_vec3* p : {&tr.v0, &tr.v1, &tr.v2}) *p = rt_vec3{U(rng), U(rng), kind == 1 ? 0.f : U(rng)};  // 1: flat
        tr.n0 = tr.n1 = tr.n2 = rt_vec3{U(rng), U(rng), U(rng)};
    }
    if (kind == 2)  // 2: identical triangles
        for (rt_triangle& tr : t) tr = t[0];
    return t;
}

bool same_arrays(const rt::PackedScene& a, const rt::PackedScene& b) {
    const auto x = a.arrays(), y = b.arrays();
    for (size_t i = 0; i < x.size(); ++i)
        if (x[i].bytes != y[i].bytes || (x[i].bytes && std::memcmp(x[i].data, y[i].data, x[i].bytes) != 0)) return false;
    return std::memcmp(a.meta.root_box, b.meta.root_box, sizeof(a.meta.root_box)) == 0 &&
           std::memcmp(a.meta.bmax, b.meta.bmax, sizeof(a.meta.bmax)) == 0;
}

void one_set(size_t i, const std::vector<rt_triangle>& tris, bool quantised) {
    const size_t P = tris.size(), NN = 2 * P - 1;
    std::vector<rt_bvh_node> nodes(NN), n2(NN);
    std::vector<rt_aabb> aabbs(NN), a2(NN);
    expect(rt_build_bvh_triangles(P, tris.data(), nodes.data(), aabbs.data()) == RT_OK, "rt_build_bvh_triangles", i);
    std::vector<rt_vec3> pos;
    std::vector<uint32_t> idx;
    for (const rt_triangle& tr : tris)
        for (const rt_vec3& p : {tr.v0, tr.v1, tr.v2}) idx.push_back(uint32_t(pos.size())), pos.push_back(p);
    expect(rt_build_bvh(pos.data(), pos.size(), idx.data(), P, n2.data(), a2.data()) == RT_OK, "rt_build_bvh", i);
    expect(std::memcmp(nodes.data(), n2.data(), NN * sizeof(rt_bvh_node)) == 0 &&
               std::memcmp(aabbs.data(), a2.data(), NN * sizeof(rt_aabb)) == 0,
           "the tree is not rt_build_bvh's over the flattened vertices", i);
    bool shape = true;
    for (size_t n = 0; n < NN; ++n) shape = shape && (nodes[n].object_idx == NONE) == (n + 1 < P);
    expect(shape, "internal nodes first, leaves last", i);
    // the weights of every box, rules 1 and 2
    std::vector<uint32_t> leaves(NN);
    std::vector<double> w(NN);
    for (size_t n = 0; n < NN; ++n) leaves[n] = uint32_t(1 + n % P);
    for (int rule = 1; rule <= 2; ++rule) {
        expect(rt_debug_box_weight_host(reinterpret_cast<const float*>(aabbs.data()), leaves.data(), rule, int(NN), w.data()) == RT_OK,
               "weights", i);
        bool ok = true;
        for (size_t n = 0; n < NN; ++n) ok = ok && w[n] >= 0.0 && std::isfinite(w[n]);
        expect(ok, "a weight is negative or not finite", i);
    }
    // the host half of the host path
    rt::PackedScene pk, plain;
    rt::RefitPlan plan;
    const int rc = rt::rebuild_pack(P, nodes.data(), aabbs.data(), tris.data(), pk, plan);
    if (quantised && rc == RT_ERR_UNSUPPORTED) return;
    expect(rc == RT_OK, "rebuild_pack", i);
    if (rc != RT_OK) return;
    expect(rt::pack_scene(P, nodes.data(), aabbs.data(), tris.data(), plain) == RT_OK && same_arrays(pk, plain),
           "the pack with a plan is not the plain pack", i);
    expect(plan.n_int == P - 1 && plan.n_leaf == P && plan.order.size() == P - 1, "plan sizes", i);
    expect(rt::refit_packed(pk, plan, tris.data()) == RT_OK && same_arrays(pk, plain), "identity refit by the new plan", i);
    // a vertex that is not finite: refused before anything is packed
    std::vector<rt_triangle> bad = tris;
    (i % 2 ? bad[P - 1].v2.z : bad[0].v0.x) = i % 3 ? NAN : -INFINITY;
    rt::PackedScene untouched = plain;
    rt::RefitPlan p2;
    expect(rt::rebuild_pack(P, nodes.data(), aabbs.data(), bad.data(), untouched, p2) == RT_ERR_ARG && same_arrays(untouched, plain),
           "a pose that is not finite", i);
}
}  // namespace

int main() {
    std::mt19937 rng(20241020u);
    std::vector<std::vector<rt_triangle>> sets;
    for (int k = 0; k < 150; ++k) {
        const size_t P = k < 6 ? size_t(k % 3 + 1) : 1 + rng() % 90;
        sets.push_back(random_tris(rng, P, k % 5 == 3 ? 2 : k % 7 == 5 ? 1 : 0));
    }
    sets.push_back(random_tris(rng, 700, 0));
    sets.push_back(random_tris(rng, 300, 2));
    const struct { int id; double value; } settings[] = {
        {-1, 0}, {RT_TUNE_WIDE4_GREEDY, 2}, {RT_TUNE_RECORD_GREEDY, 1}, {RT_TUNE_CULL_BOXES, 8}, {RT_TUNE_CUT_SUB, 4},
        {RT_TUNE_FRUSTUM_ARITY, 3}, {RT_TUNE_FRUSTUM_STACK_CAP, 6}, {RT_TUNE_QUANT_RECORDS, 1}};
    for (const auto& st : settings) {
        rt_tuning_reset();
        if (st.id >= 0 && rt_tuning_set(st.id, st.value) != RT_OK) return 2;
        for (size_t i = 0; i < sets.size(); ++i) one_set(i, sets[i], st.id == RT_TUNE_QUANT_RECORDS);
    }
    rt_tuning_reset();
    std::vector<rt_bvh_node> nodes(1);
    std::vector<rt_aabb> aabbs(1);
    expect(rt_build_bvh_triangles(0, sets[0].data(), nodes.data(), aabbs.data()) == RT_ERR_ARG, "P = 0", 0);
    expect(rt_build_bvh_triangles(1, nullptr, nodes.data(), aabbs.data()) == RT_ERR_ARG, "null triangles", 0);
    std::printf("%zu sets x %zu settings rebuilt, %d failures\n", sets.size(), sizeof(settings) / sizeof(settings[0]), failures);
    return failures ? 1 : 0;
}
