// tests/native/hit_records_hpp_main.cpp — the C++ wrappers of include/rt_mi355x.hpp over the hit-record
// and camera-ray entry points, the part that needs no device (tests/test_hit_records_host.py compiles
// and runs it): rt::camera_rays on the chain fixtures' camera, rows 5..11 at 4 spp, printed as hex
// words for the test to compare with rt_camera_rays_host.  (rt::trace_hits needs a device scene.)
#include <cstdio>
#include <cstring>

#include "rt_mi355x.hpp"

int main() {
    const float pos[3] = {0.0f, 0.0f, 5.0f}, look[3] = {0.0f, 0.0f, 0.0f}, up[3] = {0.0f, 1.0f, 0.0f};
    rt::Camera cam;
    if (rt_camera_init(&cam.c, pos, look, up, 30.0, 24.0, 48, 32, 0) != RT_OK) return 1;
    std::vector<uint32_t> seeds;
    const std::vector<rt_ray> rays = rt::camera_rays(cam, 4, 5, 7, &seeds);
    if (rays.size() != 48u * 7u * 4u || seeds.size() != rays.size()) return 2;
    if (rt::camera_rays(cam, 4, 5, 7).size() != rays.size() || !rt::camera_rays(cam, 1, 32, 0).empty()) return 3;
    try {
        rt::camera_rays(cam, 4, 30, 3);  // rows outside the image
        return 4;
    } catch (const rt::Error&) {
    }
    for (size_t i = 0; i < rays.size(); ++i) {
        uint32_t w[6];
        std::memcpy(w, &rays[i], sizeof(w));
        std::printf("%08x %08x %08x %08x %08x %08x %08x\n", w[0], w[1], w[2], w[3], w[4], w[5], seeds[i]);
    }
    return 0;
}
