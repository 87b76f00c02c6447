// rt_hip_host.hpp — host-side HIP helpers shared by the device translation units
// (error mapping into the C ABI's RT_ERR_HIP, owned device buffers, the event pair of a timed
// span, the staged form of a query, gfx950 check).
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "rt_common.hpp"

namespace rt {

inline std::string hip_msg(hipError_t e, const char* what) {
    return std::string(what) + ": " + hipGetErrorString(e);
}
#define HIP_TRY(expr)                                                          \
    do {                                                                       \
        hipError_t e_ = (expr);                                                \
        if (e_ != hipSuccess) return set_error(RT_ERR_HIP, hip_msg(e_, #expr)); \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t n = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) {
        if (p) { (void)hipFree(p); p = nullptr; }
        n = bytes;
        if (bytes == 0) return RT_OK;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) { p = nullptr; return set_error(RT_ERR_HIP, hip_msg(e, "hipMalloc")); }
        return RT_OK;
    }
    int upload(const void* src, size_t bytes) {
        int rc = alloc(bytes);
        if (rc != RT_OK || bytes == 0) return rc;
        hipError_t e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return set_error(RT_ERR_HIP, hip_msg(e, "hipMemcpy H2D"));
        return RT_OK;
    }
};

// The HIP-event time of a span of one stream, for the entries that report one through an optional
// float*: every method does nothing when on is false (the caller passed no float*).
struct KernelTimer {
    bool on;
    hipEvent_t a = nullptr, b = nullptr;
    explicit KernelTimer(bool want) : on(want) {}
    KernelTimer(const KernelTimer&) = delete;
    KernelTimer& operator=(const KernelTimer&) = delete;
    ~KernelTimer() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    int start(hipStream_t st) {  // creates both events, records the first
        if (!on) return RT_OK;
        HIP_TRY(hipEventCreate(&a));
        HIP_TRY(hipEventCreate(&b));
        HIP_TRY(hipEventRecord(a, st));
        return RT_OK;
    }
    int stop(hipStream_t st) {
        if (on) HIP_TRY(hipEventRecord(b, st));
        return RT_OK;
    }
    int read(float* ms) {  // after the stream has been synchronised
        if (on) HIP_TRY(hipEventElapsedTime(ms, a, b));
        return RT_OK;
    }
};

// The staged (host-array) form of a query: inputs uploaded, then outputs allocated, then one launch
// on the null stream between the timer's two records, that stream synchronised, the time read and
// every output copied back.  An absent array (null host pointer) has a null device pointer.  The
// first error sticks: every later call does nothing and run returns it; the buffers are freed
// with the object.
struct Staging {
    static constexpr int kMax = 6;
    struct Slot {
        DevBuf d;
        void* back = nullptr;  // an output's host array
    } slot[kMax];
    int n = 0, rc = RT_OK;
    Slot* next(const void* host) {
        if (rc != RT_OK || !host) return nullptr;
        if (n == kMax) return rc = set_error(RT_ERR_INTERNAL, "Staging: more than kMax arrays"), nullptr;
        return &slot[n++];
    }
    template <class T>
    const T* in(const T* host, size_t count) {
        Slot* s = next(host);
        if (s) rc = s->d.upload(host, count * sizeof(T));
        return s ? static_cast<const T*>(s->d.p) : nullptr;
    }
    template <class T>
    T* out(T* host, size_t count) {
        Slot* s = next(host);
        if (s) s->back = host, rc = s->d.alloc(count * sizeof(T));
        return s ? static_cast<T*>(s->d.p) : nullptr;
    }
    // launch: int(), one *_launch on the null stream with the pointers in() and out() gave
    template <class Launch>
    int run(float* kernel_ms, Launch&& launch) {
        if (rc != RT_OK) return rc;
        KernelTimer t(kernel_ms != nullptr);
        if ((rc = t.start(nullptr)) != RT_OK || (rc = launch()) != RT_OK || (rc = t.stop(nullptr)) != RT_OK) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        if ((rc = t.read(kernel_ms)) != RT_OK) return rc;
        for (int i = 0; i < n; ++i)
            if (slot[i].back) HIP_TRY(hipMemcpy(slot[i].back, slot[i].d.p, slot[i].d.n, hipMemcpyDeviceToHost));
        return RT_OK;
    }
};

inline int check_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return set_error(RT_ERR_NODEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return set_error(RT_ERR_ARG, "device index out of range");
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return set_error(RT_ERR_HIP, hip_msg(e, "hipGetDeviceProperties"));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_error(RT_ERR_NODEVICE, std::string("kernels are built for gfx950, device is ") + prop.gcnArchName);
    return RT_OK;
}

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        (void)hipSetDevice(d);
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// The HIP events around the most recent frame of a scene (rt_render_device*, rt_device.hip):
// before its first launch and after its render kernel, both on the frame's stream and owned
// by the scene (valid for the scene's next 255 frames); nullptr before the first frame.
// rt_renderer synchronises on these instead of recording events of its own on that stream.
// first is nullptr for a frame whose start was not recorded (the frame streams' untimed frames of
// a caller that passed frame_start = false below).
// back: the frame that many frames before the most recent (1: frame A of a pair just rendered).
void scene_frame_events(const rt_scene* s, hipEvent_t* first, hipEvent_t* last, int back = 0);
// A caller that orders the reuse of its output buffers itself (rt_renderer: host waits per
// frame slot) lets a scene's frame pre-passes skip the wait for the work queued before the
// frame on its stream, so they overlap the previous frame's render kernel (rt_device.hip).
// frame_start = false: the caller reads no start event of its frames (scene_frame_events' first),
// so the frame streams record the pre-passes' events on the timed frames only.
void scene_set_caller_ordered(rt_scene* s, bool on, bool frame_start = true);
// rt_build_bvh_device's tree over a triangle array (rt_lbvh.hip): the build over the 3P vertices
// v0, v1, v2 of each triangle with indices 0..3P-1, on the current device; synchronises st.
int build_bvh_triangles_device(const rt_triangle* tris_dev, size_t P, rt_bvh_node* nodes_dev, rt_aabb* aabbs_dev,
                               hipStream_t st);

}  // namespace rt
