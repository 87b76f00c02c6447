// The film's C++ wrappers of include/rt_mi355x.hpp on the host (tests/test_film_host.py): prints, as
// hex words, rt::film_pixels_host over two passes of a fixed sample table (one line per float of
// the image: sum, pixel) and then rt::camera_rays_pass of samples [3, 5) (one line per ray: six
// ray words and the seed).  rt::Film needs a device: only its refusal without one is printed.
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

int main() {
    const int W = 5, rows = 3, n = 7, first = 3;
    // sample s of float i of the image: a fixed pattern of values in [0, 1]
    auto value = [](int i, int s) { return float((i * 37 + s * 101) % 256) / 255.0f; };
    std::vector<float> a(size_t(W) * rows * first * 3), b(size_t(W) * rows * (n - first) * 3), sums;
    for (int p = 0; p < W * rows; ++p)
        for (int c = 0; c < 3; ++c) {
            for (int s = 0; s < first; ++s) a[(size_t(p) * first + s) * 3 + c] = value(p * 3 + c, s);
            for (int s = first; s < n; ++s) b[(size_t(p) * (n - first) + s - first) * 3 + c] = value(p * 3 + c, s);
        }
    rt::film_pixels_host(a, W, rows, first, sums, first);
    const std::vector<float> rgb = rt::film_pixels_host(b, W, rows, n - first, sums, n);
    for (size_t i = 0; i < rgb.size(); ++i) std::printf("%08x %08x\n", word(sums[i]), word(rgb[i]));
    std::printf("--\n");
    rt::Camera cam(rt_vec3{0.5f, 1.0f, 4.0f}, rt_vec3{0.0f, 0.5f, 0.0f}, rt_vec3{0.0f, 1.0f, 0.0f}, 35.0, 24.0, 9, 6);
    std::vector<uint32_t> seeds;
    const std::vector<rt_ray> rays = rt::camera_rays_pass(cam, 3, {0.25f, -0.125f, -0.375f, 0.5f}, 2, 3, &seeds);
    for (size_t i = 0; i < rays.size(); ++i)
        std::printf("%08x %08x %08x %08x %08x %08x %08x\n", word(rays[i].origin.x), word(rays[i].origin.y),
                    word(rays[i].origin.z), word(rays[i].direction.x), word(rays[i].direction.y),
                    word(rays[i].direction.z), seeds[i]);
    std::printf("--\n");
    try {
        rt::Film film(0, 4);  // refused before any device is looked for
        std::printf("made\n");
    } catch (const rt::Error& e) {
        std::printf("%d\n", e.code);
    }
    return 0;
}
