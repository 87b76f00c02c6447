// rt_common.hpp — shared host-side helpers of the C ABI (error slot, small vector math).
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

#include "rt_mi355x.h"

namespace rt {

// Per-thread last-error message behind rt_last_error(); set_error returns the code so
// call sites can `return set_error(RT_ERR_ARG, "...")`.
int set_error(int code, const std::string& msg);
void clear_error();

// Knob id's value set through rt_tuning_set, else dflt (include/rt_mi355x.h, rt_tune_id).
double tuning(int id, double dflt);

// Float vector helpers with the reference's evaluation order (G/include/vec3.h:327-348).
inline rt_vec3 v3(float x, float y, float z) { return rt_vec3{x, y, z}; }
inline rt_vec3 operator+(rt_vec3 a, rt_vec3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline rt_vec3 operator-(rt_vec3 a, rt_vec3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline rt_vec3 operator*(rt_vec3 a, float t) { return v3(a.x * t, a.y * t, a.z * t); }
inline rt_vec3 operator*(rt_vec3 a, rt_vec3 b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
// Vec3 / double: the double quotient rounded to float (vec3.h:334).
inline rt_vec3 div_d(rt_vec3 a, double t) {
    return v3(float(double(a.x) / t), float(double(a.y) / t), float(double(a.z) / t));
}
// Vec3 / Vec3 elementwise float division (vec3.h:333).
inline rt_vec3 div_v(rt_vec3 a, rt_vec3 b) { return v3(a.x / b.x, a.y / b.y, a.z / b.z); }
inline float dot(rt_vec3 u, rt_vec3 v) { return u.x * v.x + u.y * v.y + u.z * v.z; }
inline rt_vec3 cross(rt_vec3 u, rt_vec3 v) {
    return v3(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x);
}

// AABB() / AABB::merge / aabb_of_triangle with eps = 0 (G/include/bvh.h:28-72) as the CPU LBVH
// build applies them (rt_host.cpp) and the refit restates them (rt_scene_pack.cpp): glibc's
// fminf / fmaxf, the second argument winning the +-0 tie.
inline rt_aabb aabb_empty() {
    return rt_aabb{v3(INFINITY, INFINITY, INFINITY), v3(-INFINITY, -INFINITY, -INFINITY)};
}
inline rt_aabb aabb_merge(const rt_aabb& a, const rt_aabb& b) {
    return rt_aabb{v3(fminf(a.min_corner.x, b.min_corner.x), fminf(a.min_corner.y, b.min_corner.y),
                      fminf(a.min_corner.z, b.min_corner.z)),
                   v3(fmaxf(a.max_corner.x, b.max_corner.x), fmaxf(a.max_corner.y, b.max_corner.y),
                      fmaxf(a.max_corner.z, b.max_corner.z))};
}
inline rt_aabb aabb_of_triangle(rt_vec3 a, rt_vec3 b, rt_vec3 c) {
    rt_aabb box;
    box.min_corner = v3(fminf(a.x, fminf(b.x, c.x)), fminf(a.y, fminf(b.y, c.y)), fminf(a.z, fminf(b.z, c.z)));
    box.max_corner = v3(fmaxf(a.x, fmaxf(b.x, c.x)), fmaxf(a.y, fmaxf(b.y, c.y)), fmaxf(a.z, fmaxf(b.z, c.z)));
    const float eps = 0.0f;
    box.min_corner = v3(box.min_corner.x - eps, box.min_corner.y - eps, box.min_corner.z - eps);
    box.max_corner = v3(box.max_corner.x + eps, box.max_corner.y + eps, box.max_corner.z + eps);
    return box;
}

}  // namespace rt
