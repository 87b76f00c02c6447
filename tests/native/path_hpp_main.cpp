// The path stages' C++ wrappers of include/rt_mi355x.hpp on the host (tests/test_path_stages_host.py):
// rt::path_step_host over a fixed four-entry batch (a lit hit, a shadowed hit, a miss, an entry without a
// path), two depths, printed as hex words: per entry the next ray, alive and direct, then per path the
// state.  The device wrappers need a device: only their refusals of bad arguments are printed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_mi355x.hpp"

static uint32_t word(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

static rt_hit hit_at(int tri, rt_vec3 p, rt_vec3 n, int material) {
    rt_hit h;
    std::memset(&h, 0, sizeof(h));
    h.tri = tri;
    h.t = tri < 0 ? -1.0f : 1.0f;
    h.p = p;
    h.normal = n;
    h.geom_normal = n;
    h.front_face = 1;
    h.object_id = material;
    h.material = material;
    return h;
}

template <class F>
static void refusal(F f) {
    try {
        f();
        std::printf("0\n");
    } catch (const rt::Error& e) {
        std::printf("%d\n", e.code);
    }
}

int main() {
    const std::vector<rt_ray> rays = {{{0.0f, 0.0f, 3.0f}, {0.0f, 0.0f, -1.0f}},
                                      {{1.0f, 0.5f, 3.0f}, {0.0f, 0.0f, -1.0f}},
                                      {{2.0f, 0.0f, 3.0f}, {0.0f, 0.6f, 0.8f}},
                                      {{3.0f, 0.0f, 3.0f}, {1.0f, 0.0f, 0.0f}}};
    const std::vector<rt_hit> hits = {hit_at(5, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 2.0f}, 1),
                                      hit_at(9, {1.0f, 0.5f, 0.0f}, {0.0f, 0.6f, 0.8f}, 7),
                                      hit_at(-1, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 0),
                                      hit_at(2, {3.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 1.0f}, 0)};
    std::vector<rt_material> table(2);
    rt_material_default(&table[0]);
    rt_material_default(&table[1]);
    table[1].albedo = rt_vec3{0.25f, 0.5f, 0.75f};
    table[1].kd = 0.5f;
    table[1].ks = 0.5f;
    table[1].shininess = 7.3f;
    table[1].kr = 0.5f;
    table[1].emission = rt_vec3{0.0f, 0.125f, 0.0f};
    const std::vector<rt_light> lights = {{{1.0f, 2.0f, 4.0f}, {1.0f, 0.9f, 0.8f}, 2}, {{-2.0f, 1.0f, 3.0f}, {0.3f, 0.3f, 1.0f}, 1}};
    const std::vector<uint8_t> occluded = {0, 1, 1, 0, 0, 0, 0, 0};
    const std::vector<uint32_t> ids = {2, 0, 1, RT_PATH_NONE};
    std::vector<float> radiance(9, 0.0f), throughput(9, 1.0f);
    std::vector<uint32_t> rng = {42u, 7u, 99u};
    for (int depth = 0; depth < 2; ++depth) {
        const rt_path_opts opt = rt::path_opts(true, rt_vec3{0.25f, 0.5f, 0.125f}, depth == 1 ? RT_PATH_LAST : 0);
        const rt::PathStepHost out = rt::path_step_host(rays, hits, {}, ids, table, lights, occluded, opt, radiance, throughput, rng);
        for (size_t k = 0; k < rays.size(); ++k) {
            const rt_ray& r = out.next_rays[k];
            std::printf("%08x %08x %08x %08x %08x %08x %08x %08x %08x %08x\n", word(r.origin.x), word(r.origin.y), word(r.origin.z),
                        word(r.direction.x), word(r.direction.y), word(r.direction.z), unsigned(out.alive[k]),
                        word(out.direct[3 * k]), word(out.direct[3 * k + 1]), word(out.direct[3 * k + 2]));
        }
        for (size_t i = 0; i < rng.size(); ++i)
            std::printf("%08x %08x %08x %08x %08x %08x %08x\n", word(radiance[3 * i]), word(radiance[3 * i + 1]),
                        word(radiance[3 * i + 2]), word(throughput[3 * i]), word(throughput[3 * i + 1]),
                        word(throughput[3 * i + 2]), rng[i]);
        std::printf("--\n");
    }
    // refused before any device is looked for
    const rt_path_state none{nullptr, nullptr, nullptr};
    refusal([&] { rt::path_begin(0, 4, nullptr, none); });
    refusal([&] { rt::path_finish(0, 4, nullptr); });
    refusal([&] { rt::path_compact(0, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr); });
    refusal([&] { rt::path_step_host(rays, hits, {}, {7, 0, 1, 2}, table, lights, occluded, rt::path_opts(), radiance, throughput, rng); });
    return 0;
}
