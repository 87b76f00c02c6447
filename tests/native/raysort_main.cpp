// The ray key's host build (csrc/rt_raysort.hpp) as a stand-alone program for AddressSanitizer +
// UndefinedBehaviorSanitizer (tests/test_ray_sort_sanitize.py): every combination of a table of
// special floats as coordinate, box corner and direction component, and random bit patterns, through
// rts::ray_key in both modes at every bits value.  The float -> uint32 conversion at the end of
// clamp_cell is the operation a sanitizer can object to: it must only ever see a value in
// [0, 2^b - 1].  Prints the number of keys and of keys outside their bits.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rt_raysort.hpp"

static float from_bits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float special[] = {0.0f, -0.0f, 1.0f, -1.0f, 0.5f, 0.999999f, inf, -inf, nan, 1e30f, -1e30f,
                             3.4028235e38f, -3.4028235e38f, 1e-42f, -1e-42f, 1.17549435e-38f, 4294967296.0f, 1e-9f};
    const int ns = int(sizeof(special) / sizeof(special[0]));
    unsigned long long keys = 0, failures = 0;
    auto run = [&](const float* r, const float* b) {
        for (int mode = 0; mode < 2; ++mode)
            for (int bits = 1; bits <= (mode == rts::MODE_ORIGIN ? rts::MAX_BITS_ORIGIN : rts::MAX_BITS_ORIGIN_DIR); ++bits) {
                const int kb = rts::key_bits(mode, bits);
                const uint32_t k = rts::ray_key(r, b, mode, bits);
                ++keys;
                if (kb < 32 && (k >> kb) != 0) ++failures;
            }
    };
    // one axis at a time carries the specials (coordinate x lo x hi, and direction component), the
    // others stay ordinary
    for (int a = 0; a < ns; ++a)
        for (int l = 0; l < ns; ++l)
            for (int h = 0; h < ns; ++h)
                for (int axis = 0; axis < 3; ++axis) {
                    float r[6] = {0.25f, 0.5f, 0.75f, 0.6f, 0.0f, 0.8f}, b[6] = {0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1.0f};
                    r[axis] = special[a];
                    b[axis] = special[l];
                    b[3 + axis] = special[h];
                    r[3 + axis] = special[(a + l + h) % ns];
                    run(r, b);
                }
    for (int a = 0; a < ns; ++a)
        for (int c = 0; c < ns; ++c)
            for (int d = 0; d < ns; ++d) {
                const float r[6] = {0.5f, 0.5f, 0.5f, special[a], special[c], special[d]}, b[6] = {0, 0, 0, 1, 1, 1};
                run(r, b);
            }
    uint32_t s = 0x9E3779B9u;
    auto next = [&]() { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; };
    for (int i = 0; i < 20000; ++i) {
        float r[6], b[6];
        for (float& v : r) v = from_bits(next());
        for (float& v : b) v = from_bits(next());
        run(r, b);
    }
    // the small division of the gather / scatter kernels, over its whole domain
    for (uint32_t w = 1; w <= 16; ++w)
        for (uint32_t u = 0; u < 256 * w; ++u)
            if (rts::div_small(u, rts::div_inv(w)) != u / w) ++failures;
    if (rts::key_bits(0, 0) || rts::key_bits(0, 11) || rts::key_bits(1, 6) || rts::key_bits(2, 1) || rts::key_bits(-1, 1)) ++failures;
    std::printf("%llu keys, %llu failures\n", keys, failures);
    return failures ? 1 : 0;
}
