// The tile-coordinate helper's host build (csrc/rt_tilediv.hpp) as a stand-alone program
// (tests/test_tile_div.py; built with AddressSanitizer + UndefinedBehaviorSanitizer where the
// compiler has their host runtime): rtd::tile_div against / and % for every tiles_x in 1..1024
// with every tile index below 2^20, and at the ends of the helper's domain (n < 2^31, d <= 2^31).
// Prints the number of checks and of failures.
#include <cstdint>
#include <cstdio>

#include "rt_tilediv.hpp"

int main() {
    unsigned long long checks = 0, failures = 0;
    auto check = [&](uint32_t n, uint32_t d, rtd::TileDiv t) {
        const uint32_t q = rtd::tile_div(n, t);
        ++checks;
        if (q != n / d || n - q * d != n % d) ++failures;
    };
    for (uint32_t d = 1; d <= 1024; ++d) {
        const rtd::TileDiv t = rtd::tile_div_make(d);
        if (t.shift > 31) ++failures;
        for (uint32_t n = 0; n < (1u << 20); ++n) check(n, d, t);
    }
    // the 32-bit boundaries: divisors around every power of two up to 2^31 and a few odd ones, tile
    // indices around every multiple they have near 0, 2^16, 2^20, 2^30 and 2^31 - 1
    const uint32_t top = 0x7FFFFFFFu;
    uint32_t s = 0x9E3779B9u;
    auto next = [&]() { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; };
    auto around = [&](uint32_t d) {
        if (d < 1 || d > 0x80000000u) return;
        const rtd::TileDiv t = rtd::tile_div_make(d);
        const uint32_t bases[] = {0u, 1u << 16, 1u << 20, 1u << 30, top};
        for (uint32_t b : bases) {
            const uint32_t m = b / d * d;  // the multiple of d at or below b
            for (int k = -2; k <= 2; ++k) {
                const uint64_t n0 = (uint64_t)m + (uint64_t)(int64_t)k, n1 = n0 + d;
                if (n0 <= top) check((uint32_t)n0, d, t);
                if (n1 <= top) check((uint32_t)n1, d, t);
            }
            for (int k = 0; k <= 2; ++k) check(top - (uint32_t)k, d, t);
        }
        for (int i = 0; i < 64; ++i) check(next() & top, d, t);
    };
    for (int l = 0; l <= 31; ++l)
        for (int k = -3; k <= 3; ++k) around((uint32_t)((int64_t)(uint64_t(1) << l) + k));
    const uint32_t odd[] = {3, 5, 7, 641, 1025, 65535, 65537, 1000003, 0x7FFFFFFEu, 0x7FFFFFFFu, 0x55555555u, 0x33333333u};
    for (uint32_t d : odd) around(d);
    for (int i = 0; i < 4096; ++i) around((next() >> (next() & 31)) & 0x7FFFFFFFu);
    std::printf("%llu checks, %llu failures\n", checks, failures);
    return failures ? 1 : 0;
}
