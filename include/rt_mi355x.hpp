// include/rt_mi355x.hpp — C++ host API over the C ABI (header-only).
//
// The north-star drop-in shape `render(scene, camera) -> framebuffer`: the reference's app
// (G/src/main.cu:98-436) loads a scene, builds the LBVH, calls render() and writes an
// image; the same flow here is
//     rt::HostScene hs = rt::HostScene::load_json("frog.json");
//     rt::DeviceScene ds(hs);                       // arrays resident on the MI355X
//     rt::Camera cam = hs.camera();                 // Camera(pos, lookAt, up, mm, mm, W, H)
//     rt::Framebuffer fb = rt::render(ds, cam, hs.options());
//     rt::write_p6("out.ppm", fb);                  // ppm_p6 defaults
// Errors from the C ABI become rt::Error exceptions on this (C++) side only.
#pragma once

#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "rt_mi355x.h"

namespace rt {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

inline void check(int rc) {
    if (rc != RT_OK) throw Error(rc, rt_last_error());
}

struct Camera {
    rt_camera c{};
    Camera() = default;
    Camera(rt_vec3 pos, rt_vec3 look_at, rt_vec3 up, double focal_mm, double sensor_mm, int w, int h,
           bool hw1 = false) {
        const float p[3] = {pos.x, pos.y, pos.z}, l[3] = {look_at.x, look_at.y, look_at.z},
                    u[3] = {up.x, up.y, up.z};
        check(rt_camera_init(&c, p, l, u, focal_mm, sensor_mm, w, h, hw1 ? 1 : 0));
    }
    int width() const { return c.pixel_width; }
    int height() const { return c.pixel_height; }
};

struct Framebuffer {
    int width = 0, height = 0;
    std::vector<float> rgb;  // height*width*3, row 0 = top (G/include/query.cu:148)
};

class HostScene {
public:
    static HostScene load_json(const std::string& path, const char* project_dir = nullptr) {
        HostScene s;
        check(rt_host_scene_load_json(path.c_str(), project_dir, &s.h_));
        s.refresh();
        return s;
    }
    static HostScene load_objs(const std::vector<std::string>& paths) {
        std::vector<const char*> p;
        for (auto& s : paths) p.push_back(s.c_str());
        HostScene s;
        check(rt_host_scene_load_objs(p.data(), int(p.size()), &s.h_));
        s.refresh();
        return s;
    }
    HostScene() = default;
    HostScene(HostScene&& o) noexcept : h_(o.h_), info_(o.info_), arr_(o.arr_) { o.h_ = nullptr; }
    HostScene& operator=(HostScene&& o) noexcept {
        std::swap(h_, o.h_);
        info_ = o.info_;
        arr_ = o.arr_;
        return *this;
    }
    HostScene(const HostScene&) = delete;
    HostScene& operator=(const HostScene&) = delete;
    ~HostScene() { if (h_) rt_host_scene_free(h_); }

    const rt_scene_info& info() const { return info_; }
    const rt_scene_arrays& arrays() const { return arr_; }
    Camera camera(int w = 0, int h = 0) const {
        return Camera(info_.cam_position, info_.cam_look_at, info_.cam_up, info_.focal_length_mm,
                      info_.sensor_height_mm, w > 0 ? w : info_.pixel_width, h > 0 ? h : info_.pixel_height);
    }
    rt_render_opts options() const {
        rt_render_opts o;
        rt_render_opts_default(&o);
        o.max_depth = info_.max_depth;
        o.spp = info_.spp;
        o.diffuse_bounce = info_.diffuse_bounce;
        o.miss_color = info_.miss_color;
        return o;
    }

private:
    void refresh() {
        check(rt_host_scene_info(h_, &info_));
        check(rt_host_scene_arrays(h_, &arr_));
    }
    rt_host_scene* h_ = nullptr;
    rt_scene_info info_{};
    rt_scene_arrays arr_{};
};

class DeviceScene {
public:
    explicit DeviceScene(const HostScene& hs, int device = 0) {
        const auto& a = hs.arrays();
        const auto& i = hs.info();
        check(rt_scene_create(device, size_t(i.num_triangles), a.nodes, a.aabbs, a.triangles, a.tri_object_ids,
                              a.materials, i.num_materials, a.lights, i.num_lights, &s_));
    }
    DeviceScene(const DeviceScene&) = delete;
    DeviceScene& operator=(const DeviceScene&) = delete;
    ~DeviceScene() { if (s_) rt_scene_destroy(s_); }
    rt_scene* get() const { return s_; }

private:
    rt_scene* s_ = nullptr;
};

inline Framebuffer render(const DeviceScene& ds, const Camera& cam, const rt_render_opts& opt) {
    Framebuffer fb;
    fb.width = cam.width();
    fb.height = rt_shard_rows(cam.height(), opt.band_rows, opt.band_index, opt.band_count);
    if (fb.height < 0) throw Error(RT_ERR_ARG, "bad band parameters");
    fb.rgb.resize(size_t(fb.width) * size_t(fb.height) * 3);
    check(rt_render(ds.get(), &cam.c, &opt, fb.rgb.data(), nullptr, nullptr));
    return fb;
}

// Batched ray queries against a resident scene (rt_trace_rays): SearchBVH per ray
// (G/include/query.h:224-311), the direction used as given.
struct RayHits {
    std::vector<int32_t> tri;  // triangle index, -1 = miss
    std::vector<float> t;      // the reference's t, -1 = miss
};
inline RayHits trace_closest(const DeviceScene& ds, const std::vector<rt_ray>& rays, int flags = 0) {
    RayHits h;
    h.tri.resize(rays.size());
    h.t.resize(rays.size());
    if (!rays.empty())
        check(rt_trace_rays(ds.get(), RT_RAYS_CLOSEST, rays.data(), nullptr, rays.size(), flags, h.tri.data(),
                            h.t.data(), nullptr));
    return h;
}
// IsInShadow's decision (G/include/shader.h:59-61) per ray: 1 where a hit has t < max_t[i].
inline std::vector<int32_t> trace_occluded(const DeviceScene& ds, const std::vector<rt_ray>& rays,
                                           const std::vector<float>& max_t, int flags = 0) {
    if (max_t.size() != rays.size()) throw Error(RT_ERR_ARG, "trace_occluded: one max_t per ray");
    std::vector<int32_t> occ(rays.size());
    if (!rays.empty())
        check(rt_trace_rays(ds.get(), RT_RAYS_OCCLUDED, rays.data(), max_t.data(), rays.size(), flags, occ.data(),
                            nullptr, nullptr));
    return occ;
}

// The whole HitRecord of each ray's closest hit (rt_trace_hits): tri = -1, t = -1 on a miss.
inline std::vector<rt_hit> trace_hits(const DeviceScene& ds, const std::vector<rt_ray>& rays, int flags = 0) {
    std::vector<rt_hit> h(rays.size());
    if (!rays.empty()) check(rt_trace_hits(ds.get(), rays.data(), rays.size(), flags, h.data(), nullptr));
    return h;
}
// The camera rays of rows [row0, row0 + rows) as render() shoots them, sample s of pixel (x, y) at
// ((y - row0) * W + x) * spp + s (rt_camera_rays_host; jitter: jittered_samples(spp, 42)); seeds,
// if given, receives make_rng_seed(x, y, s) per ray.
inline std::vector<rt_ray> camera_rays(const Camera& cam, int spp, int row0, int rows,
                                       std::vector<uint32_t>* seeds = nullptr) {
    if (spp < 1 || rows < 0) throw Error(RT_ERR_ARG, "camera_rays: spp < 1 or rows < 0");
    const size_t n = size_t(cam.width()) * size_t(rows) * size_t(spp);
    std::vector<rt_ray> rays(n ? n : 1);
    if (seeds) seeds->assign(n ? n : 1, 0u);
    check(rt_camera_rays_host(&cam.c, spp, nullptr, row0, rows, rays.data(), seeds ? seeds->data() : nullptr));
    rays.resize(n);
    if (seeds) seeds->resize(n);
    return rays;
}

// One sample pass of a longer frame (rt_camera_rays_pass_host): samples [sample0, sample0 + jitter.size() / 2)
// with their slice of the frame's jitter table (jx, jy per sample); seeds make_rng_seed(x, y, sample0 + s).
inline std::vector<rt_ray> camera_rays_pass(const Camera& cam, int sample0, const std::vector<float>& jitter, int row0,
                                            int rows, std::vector<uint32_t>* seeds = nullptr) {
    const int ns = int(jitter.size() / 2);
    if (ns < 1 || jitter.size() % 2 != 0 || rows < 0) throw Error(RT_ERR_ARG, "camera_rays_pass: an empty or odd jitter table or rows < 0");
    const size_t n = size_t(cam.width()) * size_t(rows) * size_t(ns);
    std::vector<rt_ray> rays(n ? n : 1);
    if (seeds) seeds->assign(n ? n : 1, 0u);
    check(rt_camera_rays_pass_host(&cam.c, sample0, ns, jitter.data(), row0, rows, rays.data(), seeds ? seeds->data() : nullptr));
    rays.resize(n);
    if (seeds) seeds->resize(n);
    return rays;
}

// Per-pixel sums of radiance samples on a device (rt_film): add samples in render()'s order, resolve to
// render()'s float pixels and P6 bytes.  Device pointers; every call is one launch on hip_stream.
class Film {
public:
    Film(int width, int height, int device = 0) : w_(width), h_(height) { check(rt_film_create(device, width, height, &f_)); }
    Film(const Film&) = delete;
    Film& operator=(const Film&) = delete;
    ~Film() { if (f_) rt_film_destroy(f_); }
    rt_film* get() const { return f_; }
    int width() const { return w_; }
    int height() const { return h_; }
    // radiance_dev: rows*W*nsamples*3 floats, sample s of pixel (x, y) at ((y - row0) * W + x) * nsamples + s
    void add(const float* radiance_dev, int row0, int rows, int nsamples, void* hip_stream = nullptr) {
        check(rt_film_add_device(f_, radiance_dev, row0, rows, nsamples, hip_stream));
    }
    // rgb_dev: rows*W*3 floats, p6_dev: rows*W*3 bytes; one of them may be null.  Does not clear.
    void resolve(int row0, int rows, float* rgb_dev, uint8_t* p6_dev, void* hip_stream = nullptr) {
        check(rt_film_resolve_device(f_, row0, rows, rgb_dev, p6_dev, hip_stream));
    }
    void clear(void* hip_stream = nullptr) { check(rt_film_clear_device(f_, hip_stream)); }
    int64_t row_samples(int row) const {
        int64_t n = 0;
        check(rt_film_row_samples(f_, row, &n));
        return n;
    }

private:
    rt_film* f_ = nullptr;
    int w_ = 0, h_ = 0;
};

// The film's arithmetic on the host (rt_film_pixels_host): adds radiance (rows*width*nsamples*3) to sums
// (rows*width*3, resized and zeroed when empty) and returns the pixels of count_after samples per pixel.
inline std::vector<float> film_pixels_host(const std::vector<float>& radiance, int width, int rows, int nsamples,
                                           std::vector<float>& sums, int64_t count_after) {
    const size_t px = size_t(width > 0 ? width : 0) * size_t(rows > 0 ? rows : 0) * 3;
    if (sums.empty()) sums.assign(px, 0.0f);
    if (sums.size() != px || nsamples < 1 || radiance.size() != px * size_t(nsamples))
        throw Error(RT_ERR_ARG, "film_pixels_host: radiance and sums do not match the shape");
    std::vector<float> rgb(px);
    if (px) check(rt_film_pixels_host(radiance.data(), width, rows, nsamples, sums.data(), count_after, rgb.data()));
    return rgb;
}

// A film with a sample count and two luminance moments per pixel on a device (rt_afilm): add samples onto
// a pixel list, resolve every pixel with its own count, select the pixels to sample next; with
// rt_camera_rays_pixels_device (counts()) a pixel with c samples is render(spp = c)'s pixel.  Device pointers.
class AdaptiveFilm {
public:
    AdaptiveFilm(int width, int height, int device = 0) : w_(width), h_(height), dev_(device) {
        check(rt_afilm_create(device, width, height, &f_));
    }
    AdaptiveFilm(const AdaptiveFilm&) = delete;
    AdaptiveFilm& operator=(const AdaptiveFilm&) = delete;
    ~AdaptiveFilm() { if (f_) rt_afilm_destroy(f_); }
    rt_afilm* get() const { return f_; }
    int width() const { return w_; }
    int height() const { return h_; }
    int device() const { return dev_; }
    const uint32_t* counts() const { return rt_afilm_counts_device(f_); }
    // radiance_dev: m*nsamples*3 floats, sample s of entry k at k * nsamples + s; pixels_dev null: every pixel
    void add(const uint32_t* pixels_dev, size_t m, const float* radiance_dev, int nsamples, void* hip_stream = nullptr) {
        check(rt_afilm_add_device(f_, pixels_dev, m, radiance_dev, nsamples, hip_stream));
    }
    // rgb_dev: rows*W*3 floats, p6_dev: rows*W*3 bytes, counts_out_dev: rows*W words; two of them may be null
    void resolve(int row0, int rows, float* rgb_dev, uint8_t* p6_dev, uint32_t* counts_out_dev, void* hip_stream = nullptr) {
        check(rt_afilm_resolve_device(f_, row0, rows, rgb_dev, p6_dev, counts_out_dev, hip_stream));
    }
    size_t select_scratch_bytes() const { return rt_afilm_select_scratch_bytes(f_); }
    // pixels_out_dev: W*H words; *count_dev: their number, written in stream order (nothing is read back)
    void select(const rt_afilm_select_opts& opts, uint32_t* pixels_out_dev, uint32_t* count_dev, void* scratch_dev,
                void* hip_stream = nullptr) {
        check(rt_afilm_select_device(f_, &opts, pixels_out_dev, count_dev, scratch_dev, hip_stream));
    }
    void clear(void* hip_stream = nullptr) { check(rt_afilm_clear_device(f_, hip_stream)); }

private:
    rt_afilm* f_ = nullptr;
    int w_ = 0, h_ = 0, dev_ = 0;
};

// Path stages for caller hits (rt_path_*): TraceRayIterative's loop body on caller rays and hit records,
// with begin, compact and finish around it.  Device pointers; every call is asynchronous on hip_stream.
inline rt_path_opts path_opts(bool diffuse_bounce = true, rt_vec3 miss_color = rt_vec3{0.f, 0.f, 0.f}, int flags = 0) {
    rt_path_opts o;
    rt_path_opts_default(&o);
    o.diffuse_bounce = diffuse_bounce ? 1 : 0;
    o.miss_color = miss_color;
    o.flags = flags;
    return o;
}
inline void path_begin(int device, size_t n, const uint32_t* seeds_dev, const rt_path_state& st, void* hip_stream = nullptr) {
    check(rt_path_begin_device(device, n, seeds_dev, &st, hip_stream));
}
// mats_dev, ids_dev and direct_dev may be null; next_rays_dev and alive_dev too with RT_PATH_LAST in opt.flags.
inline void path_step(const DeviceScene& ds, size_t m, const rt_ray* rays_dev, const rt_hit* hits_dev,
                      const rt_material* mats_dev, const uint32_t* ids_dev, const rt_path_opts& opt, const rt_path_state& st,
                      rt_ray* next_rays_dev, uint8_t* alive_dev, float* direct_dev = nullptr, void* hip_stream = nullptr) {
    check(rt_path_step_device(ds.get(), m, rays_dev, hits_dev, mats_dev, ids_dev, &opt, &st, next_rays_dev, alive_dev,
                              direct_dev, hip_stream));
}
// scratch_dev: rt_path_compact_scratch_bytes(m) bytes.
inline void path_compact(int device, size_t m, const uint8_t* alive_dev, const rt_ray* rays_in_dev, const uint32_t* ids_in_dev,
                         rt_ray* rays_out_dev, uint32_t* ids_out_dev, uint32_t* count_dev, void* scratch_dev,
                         void* hip_stream = nullptr) {
    check(rt_path_compact_device(device, m, alive_dev, rays_in_dev, ids_in_dev, rays_out_dev, ids_out_dev, count_dev,
                                 scratch_dev, hip_stream));
}
inline void path_finish(int device, size_t n, float* radiance_dev, void* hip_stream = nullptr) {
    check(rt_path_finish_device(device, n, radiance_dev, hip_stream));
}

// Sorting caller rays for coherence (rt_ray_*, rt_gather_device, rt_scatter_device): keys in a box, the stable
// order by key, and the moves into and out of it.  A query on the sorted rays, scattered back, is the query.
inline rt_aabb scene_bounds(const DeviceScene& ds) {
    rt_aabb b;
    check(rt_scene_bounds(ds.get(), &b));
    return b;
}
inline int ray_key_bits(int mode, int bits) {
    const int kb = rt_ray_key_bits(mode, bits);
    if (kb < 0) check(kb);
    return kb;
}
inline std::vector<uint32_t> ray_keys_host(const std::vector<rt_ray>& rays, const rt_aabb& box, int mode, int bits) {
    std::vector<uint32_t> keys(rays.size());
    check(rt_ray_keys_host(rays.data(), rays.size(), mode, bits, &box, keys.data()));
    return keys;
}
inline std::vector<uint32_t> ray_sort_host(const std::vector<rt_ray>& rays, const rt_aabb& box, int mode, int bits) {
    std::vector<uint32_t> order(rays.size());
    check(rt_ray_sort_host(rays.data(), rays.size(), mode, bits, &box, order.data()));
    return order;
}
inline void ray_keys(int device, const rt_ray* rays_dev, size_t n, int mode, int bits, const rt_aabb& box, uint32_t* keys_dev,
                     void* hip_stream = nullptr) {
    check(rt_ray_keys_device(device, rays_dev, n, mode, bits, &box, keys_dev, hip_stream));
}
// scratch_dev: rt_ray_sort_scratch_bytes(n, mode, bits) bytes; rays_out_dev may be null.
inline size_t ray_sort_scratch_bytes(size_t n, int mode, int bits) { return rt_ray_sort_scratch_bytes(n, mode, bits); }
inline void ray_sort(int device, const rt_ray* rays_dev, size_t n, int mode, int bits, const rt_aabb& box, uint32_t* order_dev,
                     rt_ray* rays_out_dev, void* scratch_dev, void* hip_stream = nullptr) {
    check(rt_ray_sort_device(device, rays_dev, n, mode, bits, &box, order_dev, rays_out_dev, scratch_dev, hip_stream));
}
// out[k] = in[order[k]] / out[order[k]] = in[k] for n elements of sizeof(T) bytes (a multiple of 4 in 4..64).
template <class T>
inline void gather(int device, const T* in_dev, size_t n, const uint32_t* order_dev, T* out_dev, void* hip_stream = nullptr) {
    check(rt_gather_device(device, in_dev, n, sizeof(T), order_dev, out_dev, hip_stream));
}
template <class T>
inline void scatter(int device, const T* in_dev, size_t n, const uint32_t* order_dev, T* out_dev, void* hip_stream = nullptr) {
    check(rt_scatter_device(device, in_dev, n, sizeof(T), order_dev, out_dev, hip_stream));
}

// The step's arithmetic on the host (rt_path_step_host) over host vectors: the state of radiance.size() / 3
// paths is updated in place; occluded holds rays.size() * lights.size() bytes, entry k's answer for light l at
// k * lights.size() + l.  ids and mats may be empty (entry k is path k; the table's material of the record).
struct PathStepHost {
    std::vector<rt_ray> next_rays;
    std::vector<uint8_t> alive;
    std::vector<float> direct;
};
inline PathStepHost path_step_host(const std::vector<rt_ray>& rays, const std::vector<rt_hit>& hits,
                                   const std::vector<rt_material>& mats, const std::vector<uint32_t>& ids,
                                   const std::vector<rt_material>& table, const std::vector<rt_light>& lights,
                                   const std::vector<uint8_t>& occluded, const rt_path_opts& opt,
                                   std::vector<float>& radiance, std::vector<float>& throughput, std::vector<uint32_t>& rng) {
    const size_t m = rays.size();
    if (hits.size() != m || (!mats.empty() && mats.size() != m) || (!ids.empty() && ids.size() != m) ||
        occluded.size() != m * lights.size() || radiance.size() != throughput.size() || radiance.size() != 3 * rng.size())
        throw Error(RT_ERR_ARG, "path_step_host: the arrays do not match the batch");
    for (uint32_t id : ids)
        if (id != RT_PATH_NONE && id >= rng.size()) throw Error(RT_ERR_ARG, "path_step_host: a path id outside the state");
    if (ids.empty() && m > rng.size()) throw Error(RT_ERR_ARG, "path_step_host: more entries than paths");
    PathStepHost out;
    out.next_rays.resize(m);
    out.alive.resize(m);
    out.direct.resize(3 * m);
    if (m == 0) return out;
    const rt_path_state st{radiance.data(), throughput.data(), rng.data()};
    check(rt_path_step_host(m, rays.data(), hits.data(), mats.empty() ? nullptr : mats.data(), ids.empty() ? nullptr : ids.data(),
                            table.empty() ? nullptr : table.data(), int(table.size()), lights.empty() ? nullptr : lights.data(),
                            int(lights.size()), occluded.empty() ? nullptr : occluded.data(), &opt, &st, out.next_rays.data(),
                            out.alive.data(), out.direct.data()));
    return out;
}

inline void write_p6(const std::string& path, const Framebuffer& fb, const rt_ppm_options* opt = nullptr) {
    check(rt_ppm_write(path.c_str(), fb.rgb.data(), fb.width, fb.height, opt));
}

}  // namespace rt
