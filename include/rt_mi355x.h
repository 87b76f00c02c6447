/* include/rt_mi355x.h — C ABI of the MI355X (gfx950) per-pixel ray path.
 *
 * Drop-in boundary for the reference's render entry point
 *     void render(size_t numTriangles, int W, int H, const Camera cam, const Vec3 missColor,
 *                 int max_depth, int spp, const BVHNode* nodes, const AABB* aabbs,
 *                 const Triangle* triangles, const int32_t* triObjectIds,
 *                 const Material* objectMaterials, int numObjectMaterials,
 *                 const Light* lights, int numLights, bool diffuse_bounce, Vec3* output);
 * (HW2/HW2/GPUandCPU/include/query.h:13-29, defined at include/query.cu:79-167) and of the
 * host pieces around it that the reference keeps in C++ (scene JSON + OBJ loading,
 * camera setup, CPU LBVH build, ppm_p6 writer).  Plain C types, plain pointers and sizes;
 * every function returns RT_OK (0) or a negative RT_ERR_* code and never throws;
 * rt_last_error() returns the calling thread's last message.
 *
 * Structs marked "layout = reference" are byte-for-byte the reference's POD types, so a
 * caller holding the reference's arrays passes them unchanged.
 */
#ifndef RT_MI355X_H
#define RT_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 3  /* 2: rt_renderer_opts.host_frame_name, RT_GATHER_HOST_SHARED;
                              3: RT_ERR_INTERNAL, rt_scene_faults, rt_tuning_* (RT_TUNE_*) in place of
                                 environment variables, frame pairs, the resident HW1 scene;
                                 added since without a new version (new entry points only, nothing
                                 existing changed): rt_shade_opts, rt_shade_opts_default,
                                 rt_shade_rays, rt_shade_rays_device, rt_shade_rays_variant; rt_hit,
                                 rt_trace_hits, rt_trace_hits_device, rt_trace_hits_variant,
                                 rt_hit_record_host, rt_camera_rays_host, rt_camera_rays_device; rt_film,
                                 rt_film_create, rt_film_destroy, rt_film_clear_device,
                                 rt_film_add_device, rt_film_resolve_device, rt_film_row_samples,
                                 rt_film_pixels_host, rt_camera_rays_pass_host,
                                 rt_camera_rays_pass_device; rt_path_state, rt_path_opts, RT_PATH_LAST,
                                 RT_PATH_NONE, rt_path_opts_default, rt_path_begin_device,
                                 rt_path_step_device, rt_path_step_variant, rt_path_step_host,
                                 rt_path_compact_scratch_bytes, rt_path_compact_device,
                                 rt_path_finish_device; RT_PIXEL_NONE, rt_camera_rays_pixels_host,
                                 rt_camera_rays_pixels_device, rt_afilm, rt_afilm_select_opts,
                                 rt_afilm_create, rt_afilm_destroy, rt_afilm_clear_device,
                                 rt_afilm_counts_device, rt_afilm_add_device, rt_afilm_resolve_device,
                                 rt_afilm_select_scratch_bytes, rt_afilm_select_device, rt_afilm_host;
                                 rt_scene_create_refittable, rt_scene_refit_device, rt_scene_refit,
                                 rt_refit_aabbs_host, rt_triangles_from_mesh_device,
                                 rt_debug_scene_digest, rt_debug_scene_refit_pack,
                                 rt_debug_scene_refit_chain; rt_scene_rebuild_device, rt_scene_rebuild,
                                 rt_scene_rebuild_path (RT_REBUILD_*), rt_scene_rebuild_counts, rt_build_bvh_triangles,
                                 rt_debug_box_weight_host, rt_debug_box_weight_batch; RT_SORT_ORIGIN,
                                 RT_SORT_ORIGIN_DIR, rt_scene_bounds, rt_ray_key_bits, rt_ray_keys_host,
                                 rt_ray_keys_device, rt_ray_sort_host, rt_ray_sort_scratch_bytes,
                                 rt_ray_sort_device, rt_gather_device, rt_scatter_device; rt_multi_hit,
                                 RT_MULTI_HIT_MAX_K, rt_trace_multi_hits, rt_trace_multi_hits_device,
                                 rt_trace_multi_hits_variant, rt_multi_hits_host; rt_point_hit,
                                 rt_closest_points, rt_closest_points_device,
                                 rt_closest_points_variant, rt_closest_points_host;
                                 rt_debug_query_variant; rt_light_shape, RT_LIGHT_MAX_SHADOW_SAMPLES,
                                 rt_scene_num_lights, rt_light_visibility_device,
                                 rt_light_visibility_variant, rt_path_step_vis_device,
                                 rt_light_samples_host, rt_path_step_vis_host,
                                 rt_host_scene_light_shapes */

enum {
    RT_OK = 0,
    RT_ERR_ARG = -1,          /* bad argument / malformed arrays */
    RT_ERR_IO = -2,           /* file could not be opened / written */
    RT_ERR_PARSE = -3,        /* OBJ / JSON / PPM syntax */
    RT_ERR_HIP = -4,          /* HIP runtime error (message in rt_last_error) */
    RT_ERR_NOMEM = -5,
    RT_ERR_NODEVICE = -6,     /* no gfx950 device / code object not loadable */
    RT_ERR_UNSUPPORTED = -7,  /* input outside what the kernels handle (see rt_last_error) */
    RT_ERR_COMM = -8,         /* RCCL could not be loaded or a collective failed */
    RT_ERR_INTERNAL = -9      /* a device-side guard fired (rt_scene_faults); the frame is not valid */
};

/* ---- reference POD types ------------------------------------------------------------ */
typedef struct { float x, y, z; } rt_vec3;                       /* layout = reference: Vec3, G/include/vec3.h:299-304 */
typedef struct {                                                  /* layout = reference: BVHNode, G/include/bvh.h:7-13 */
    uint32_t parent_idx, left_idx, right_idx, object_idx;         /* object_idx == 0xFFFFFFFF: internal */
} rt_bvh_node;
typedef struct { rt_vec3 min_corner, max_corner; } rt_aabb;      /* layout = reference: AABB, G/include/bvh.h:28-52 */
typedef struct { rt_vec3 v0, v1, v2, n0, n1, n2; } rt_triangle;  /* layout = reference: Triangle, G/include/MeshOBJ.h:42-67 */
typedef struct {                                                  /* layout = reference: Material, G/include/material.h:6-21 */
    rt_vec3 albedo; float kd;
    rt_vec3 specular_color; float ks; float shininess;
    float kr;
    rt_vec3 emission;
} rt_material;
typedef struct { rt_vec3 position, color; int32_t intensity; } rt_light; /* layout = reference: Light, G/include/scene.h:21-25 */

/* Derived pinhole basis of the reference Camera (G/include/camera.h:208-216): the fields
 * render() reads.  Fill with rt_camera_init (same float/double arithmetic as
 * Camera::initialize, camera.h:72-94). */
typedef struct {
    rt_vec3 center, pixel00_loc, pixel_delta_u, pixel_delta_v;
    int32_t pixel_width, pixel_height;
} rt_camera;

/* Reference Material() defaults (material.h:8-19). */
void rt_material_default(rt_material* m);

/* Camera(pos, lookAt, up, focal_length_mm, sensor_height_mm, width, height)
 * (G/include/camera.h:13-28).  hw1 != 0 follows HW1/include/camera.h (error instead of
 * clamping width/height < 1). */
int rt_camera_init(rt_camera* cam, const float pos[3], const float look_at[3], const float up[3],
                   double focal_length_mm, double sensor_height_mm, int width, int height, int hw1);

/* jittered_samples(spp, seed) (G/include/antialias.h:12-27): std::mt19937 +
 * uniform_real_distribution<float>; centered != 0 subtracts 0.5 (G/), 0 keeps [0,1) (HW1).
 * out: 2*spp floats. */
int rt_jittered_samples(int spp, uint32_t seed, int centered, float* out);

/* ---- host scene: the reference's loaders + CPU LBVH (G/src/main.cu:104-317) -------- */
typedef struct rt_host_scene rt_host_scene;

typedef struct {
    /* settings (G/include/scene.h:15-19), miss colour, camera, counts */
    int32_t max_depth, spp, diffuse_bounce;
    rt_vec3 miss_color;
    rt_vec3 cam_position, cam_look_at, cam_up;
    double focal_length_mm, sensor_height_mm;
    int32_t pixel_width, pixel_height;
    uint64_t num_triangles, num_vertices;
    int32_t num_materials, num_lights, num_objects_loaded;
    int32_t bvh_max_stack;   /* DFS stack depth the traversal of this tree needs */
    int32_t bvh_height;
} rt_scene_info;

typedef struct {  /* views into rt_host_scene storage (valid until rt_host_scene_free) */
    const rt_bvh_node* nodes;        /* 2P-1 */
    const rt_aabb* aabbs;            /* 2P-1 */
    const rt_triangle* triangles;    /* P, packed as G/src/main.cu:388-404 */
    const int32_t* tri_object_ids;   /* P */
    const rt_material* materials;    /* num_materials */
    const rt_light* lights;          /* num_lights (fallback light added as main.cu:328-336) */
    const rt_vec3* positions;        /* num_vertices (transformed) */
    const rt_vec3* normals;          /* num_vertices or NULL */
    const uint32_t* indices;         /* 3P */
} rt_scene_arrays;

/* Scene JSON (G/include/scene.h:242-393) + every mesh object: LoadOBJ_ToMesh
 * (G/include/MeshOBJ.h:260-427), applyObjectTransform (G/src/main.cu:57-96), AppendMesh
 * (MeshOBJ.h:429-466); then calculateAABBs + CPU buildBVH (G/include/bvh.cu:60-89,209-317).
 * Relative mesh paths resolve like G/src/main.cu:119-147 with project_dir (NULL =
 * dirname(dirname(dirname(scene)))). */
int rt_host_scene_load_json(const char* scene_path, const char* project_dir, rt_host_scene** out);
/* OBJ path list without JSON (G/src/main.cu:151-157): default material/camera/settings. */
int rt_host_scene_load_objs(const char* const* obj_paths, int n, rt_host_scene** out);
int rt_host_scene_info(const rt_host_scene* s, rt_scene_info* out);
int rt_host_scene_arrays(const rt_host_scene* s, rt_scene_arrays* out);
void rt_host_scene_free(rt_host_scene* s);

/* CPU LBVH over caller arrays (leaf AABBs from indexed triangles), reference algorithm:
 * nodes/aabbs must hold 2P-1 entries. */
int rt_build_bvh(const rt_vec3* positions, size_t num_vertices, const uint32_t* indices,
                 size_t num_triangles, rt_bvh_node* nodes, rt_aabb* aabbs);
/* The same build on the GPU (the reference's CUDA build bvh.cu:34-206 and
 * its CPU build bvh.cu:209-317): positions_dev (num_vertices Vec3), indices_dev (3*P u32),
 * nodes_dev / aabbs_dev (2P-1 each) are device pointers on `device`.  The arrays are
 * byte-identical to rt_build_bvh's.  Runs on hip_stream and synchronises it before returning
 * (out-of-range vertex indices are reported as RT_ERR_ARG). */
int rt_build_bvh_device(int device, const rt_vec3* positions_dev, size_t num_vertices,
                        const uint32_t* indices_dev, size_t num_triangles, rt_bvh_node* nodes_dev,
                        rt_aabb* aabbs_dev, void* hip_stream);

/* HW1 mesh: LoadOBJ_ToMeshSOA (HW1/src/MeshOBJ.cpp:143-281). */
typedef struct rt_mesh rt_mesh;
typedef struct {
    const rt_vec3* positions; const rt_vec3* normals; const uint32_t* indices;
    uint64_t num_vertices, num_triangles; int32_t has_normals, has_uvs;
} rt_mesh_view;
int rt_mesh_load_obj_hw1(const char* path, rt_mesh** out);
int rt_mesh_view_get(const rt_mesh* m, rt_mesh_view* out);
void rt_mesh_free(rt_mesh* m);

/* ---- ppm_p6 (HW1/ppm_p6_lib/include/ppm_p6.hpp:46-85) ------------------------------- */
typedef struct { int32_t maxval, clamp, gamma2, flip_y; } rt_ppm_options;  /* defaults 255,1,1,0 */
void rt_ppm_options_default(rt_ppm_options* o);
/* rgb: W*H*3 floats, row 0 = top.  Writes "P6\n<W> <H>\n<maxval>\n" + samples. */
int rt_ppm_write(const char* path, const float* rgb, int width, int height, const rt_ppm_options* opt);
/* Same bytes into memory: needs 32 + W*H*3*(maxval<256 ? 1 : 2) bytes; *written = size. */
int rt_ppm_encode(const float* rgb, int width, int height, const rt_ppm_options* opt,
                  uint8_t* buf, size_t cap, size_t* written);
/* read_p6 (ppm_p6.cpp:303-372): rgb_out may be NULL to query W/H first. */
int rt_ppm_read(const char* path, float* rgb_out, size_t cap_floats, int* width, int* height, int* maxval);

/* ---- frame epilogue on the device --------------------------------- */
/* write_p6's header ("P6\n<W> <H>\n<maxval>\n", ppm_p6.cpp:275-277); buf may be NULL to
 * query the size. */
int rt_ppm_header(int width, int height, int maxval, char* buf, size_t cap, size_t* written);
/* write_p6's sample loop (ppm_p6.cpp:284-299 with float_to_sample :137-155) on the device:
 * rgb_dev = rows*W*3 floats (device), out_dev = rows*W*3*(maxval<256 ? 1 : 2) bytes (device),
 * the P6 body without its header; flip_y reverses the given rows.  Asynchronous on
 * hip_stream.  Byte-identical to rt_ppm_encode's body. */
int rt_ppm_quantize_device(const float* rgb_dev, int width, int rows, const rt_ppm_options* opt,
                           uint8_t* out_dev, void* hip_stream);
/* Band un-permute after a gather: strips_dev holds band_count strips back to back, strip r =
 * strip_rows rows of row_bytes bytes in the layout rt_render_device writes for
 * (band_rows, r, band_count) — float rows (W*12 B) or quantised P6 rows.  Writes the
 * height-row frame in image order (flip_y: bottom row first) to frame_dev.  Asynchronous. */
int rt_unpermute_strips_device(const void* strips_dev, int strip_rows, size_t row_bytes, int height,
                               int band_rows, int band_count, int flip_y, void* frame_dev, void* hip_stream);

/* ---- the hot path: device-resident scene + HIP render ---------------------------------- */
typedef struct rt_scene rt_scene;

/* Upload the reference arrays to `device`, validating them (indices in range, a proper
 * binary tree rooted at 0) and repacking them into the gfx950 traversal layout. */
int rt_scene_create(int device, size_t num_triangles, const rt_bvh_node* nodes, const rt_aabb* aabbs,
                    const rt_triangle* triangles, const int32_t* tri_object_ids,
                    const rt_material* materials, int num_materials, const rt_light* lights,
                    int num_lights, rt_scene** out);
void rt_scene_destroy(rt_scene* s);
/* The same scene on another device: device-to-device copies of the packed arrays (no host
 * repacking).  Frames of a scene run in launch order (see rt_render_device). */
int rt_scene_clone(const rt_scene* src, int device, rt_scene** out);
int rt_scene_device(const rt_scene* s);
size_t rt_scene_device_bytes(const rt_scene* s);

/* ---- refit: new vertex positions under a resident scene ---------------------- */
/* rt_scene_create's scene, its packed arrays byte for byte, plus what a refit needs on the device
 * (counted in rt_scene_device_bytes).  RT_ERR_UNSUPPORTED, creating nothing, unless the tree is
 * proper (every one of the 2P-1 nodes reached from node 0, once; two children per internal node;
 * every leaf naming a triangle), and when quantised records are in force (RT_TUNE_QUANT_RECORDS).
 * Trees that take the binary records and deep trees are supported.  rt_scene_clone of such a scene
 * is refittable too. */
int rt_scene_create_refittable(int device, size_t num_triangles, const rt_bvh_node* nodes, const rt_aabb* aabbs,
                               const rt_triangle* triangles, const int32_t* tri_object_ids,
                               const rt_material* materials, int num_materials, const rt_light* lights,
                               int num_lights, rt_scene** out);
/* Move the scene's triangles: tris_dev holds the P triangles on the scene's device, in the order
 * given at creation (normals included).  The tree and the record topology chosen at creation
 * stay; the leaf boxes are aabb_of_triangle's, the internal boxes merge(left, right) bottom-up
 * (rt_refit_aabbs_host), and every stored box, v0 | e1 | e2 and normal is rewritten from them, so
 * every query answers as the reference does on (nodes, those boxes, the new triangles).  A first
 * pass checks every vertex coordinate: RT_ERR_ARG, the scene untouched, if one is not finite.
 * The call waits for the scene's own streams and for hip_stream before it writes, runs on
 * hip_stream and synchronises it before returning; *ms (optional) is the HIP-event time of its
 * launches.  Frames and queries the caller has queued on OTHER streams are the caller's to order
 * against it.  The per-tile cost history is forgotten.  A long animation degrades the tree: the
 * topology is not rebuilt (rt_build_bvh_device and a new scene do that).  RT_ERR_UNSUPPORTED for
 * a scene not created refittable. */
int rt_scene_refit_device(rt_scene* s, const rt_triangle* tris_dev, void* hip_stream, float* ms);
/* The same from host memory. */
int rt_scene_refit(rt_scene* s, const rt_triangle* tris_host, float* ms);
/* The boxes a refit gives the tree (2P-1, by node), on the host.  RT_ERR_UNSUPPORTED unless the
 * tree is proper. */
int rt_refit_aabbs_host(size_t num_triangles, const rt_bvh_node* nodes, const rt_triangle* tris, rt_aabb* aabbs_out);
/* The triangle array of an indexed mesh on the device (G/src/main.cu:388-404; zero normals when
 * normals_dev is NULL), so deformed vertex buffers reach a refit without leaving the GPU.  Runs on
 * hip_stream and synchronises it; out-of-range indices are reported as RT_ERR_ARG. */
int rt_triangles_from_mesh_device(int device, const rt_vec3* positions_dev, size_t num_vertices,
                                  const rt_vec3* normals_dev, const uint32_t* indices_dev, size_t num_triangles,
                                  rt_triangle* tris_dev, void* hip_stream);

/* ---- rebuild: new triangles AND a new tree under a resident scene ------------ */
/* tris_dev: P triangles on the scene's device, in the order given at creation (object ids,
 * materials and lights stay).  The tree is the reference's LBVH over them: rt_build_bvh over the 3P
 * vertices v0, v1, v2 of each triangle with indices 0..3P-1 (rt_build_bvh_triangles), built on the
 * device.  Every packed array, every fact the launches choose kernels by and the refit plan are what
 * rt_scene_create_refittable makes from (that tree, tris), byte for byte, so every frame and query
 * answers as on a scene created from them, and the rebuilt scene (and its clone) can be refitted
 * and rebuilt again.  nodes_out_dev / aabbs_out_dev (optional, 2P-1 each): the tree.
 * Only scenes created refittable (RT_ERR_UNSUPPORTED otherwise, and when quantised records are in
 * force).  A first pass checks every vertex coordinate: RT_ERR_ARG if one is not finite.  The call
 * builds into fresh buffers and swaps them in after everything has succeeded: any error leaves
 * the scene, its digest and its answers as they were.  After the swap rt_scene_device_bytes
 * reflects the new sizes and the per-tile cost history is dropped.  Streams as the refit: the call
 * waits for the scene's own streams and for hip_stream before it works, runs on hip_stream and
 * synchronises it before returning.  *ms (optional): the HIP-event time from the finite check to the
 * last launch of the pack (the host path's host work included in the span).
 * Two paths inside the call, the same bytes from both (rt_scene_rebuild_path says which ran):
 * RT_REBUILD_DEVICE packs the records on the device too; it handles what the LBVH over finite
 * triangles gives at the default record rules (P >= 2, nested boxes, a tree that is not deep, a
 * 4-ary stack within the cap) and honours RT_TUNE_FRUSTUM_ARITY, RT_TUNE_FRUSTUM_STACK_CAP,
 * RT_TUNE_CULL_BOXES and RT_TUNE_CUT_SUB.  RT_REBUILD_HOST downloads the device-built tree, runs the
 * host pack with a plan and uploads the result: P == 1, RT_TUNE_RECORD_GREEDY != 2,
 * RT_TUNE_WIDE4_GREEDY != 1, a deep tree, and quantised records (which it refuses). */
int rt_scene_rebuild_device(rt_scene* s, const rt_triangle* tris_dev, void* hip_stream,
                            rt_bvh_node* nodes_out_dev, rt_aabb* aabbs_out_dev, float* ms);
/* The same from host memory (nodes_out / aabbs_out: host arrays). */
int rt_scene_rebuild(rt_scene* s, const rt_triangle* tris_host, rt_bvh_node* nodes_out, rt_aabb* aabbs_out, float* ms);
/* The tree a rebuild gives, on the host: rt_build_bvh over the flattened vertices.  Its internal
 * nodes are [0, P-1), its leaves [P-1, 2P-1). */
int rt_build_bvh_triangles(size_t num_triangles, const rt_triangle* tris, rt_bvh_node* nodes, rt_aabb* aabbs);
enum { RT_REBUILD_NONE = 0, RT_REBUILD_DEVICE = 1, RT_REBUILD_HOST = 2 };
int rt_scene_rebuild_path(const rt_scene* s);   /* which path the latest rebuild of s took */
/* counts[0]: kernel launches of the latest rebuild's pack on the device (the tree build's are not
 * counted), counts[1]: its host read-backs (the host path: 0 and 3).  For measurements. */
int rt_scene_rebuild_counts(const rt_scene* s, int64_t counts[2]);

enum {
    RT_KERNEL_AUTO = 0,      /* the fastest parity-equivalent kernel */
    RT_KERNEL_WAVE = 1,      /* wave-coherent masked DFS (shared per-wave stack) */
    RT_KERNEL_LANE = 2,      /* one private DFS stack per lane (baseline variant) */
    RT_KERNEL_WAVE_PIXELS = 3 /* WAVE traversal, one pixel per lane looping over its samples */
};

typedef struct {
    int32_t max_depth;        /* TraceRayIterative depth (query.h:156) */
    int32_t spp;
    int32_t diffuse_bounce;
    rt_vec3 miss_color;
    const float* jitter;      /* host, 2*spp floats; NULL = rt_jittered_samples(spp, 42, 1).  Any
                               * table renders exactly.  The tile culling covers tables whose
                               * every entry is finite with |entry| <= 1 (its one-pixel pad); a
                               * frame with any other table runs as with RT_FLAG_NO_CULL. */
    /* Image sharding: rows are cut into bands of band_rows; this call renders bands b with
     * b % band_count == band_index, written contiguously (band order) into the output
     * ("strip" layout).  band_count <= 1 renders the whole frame in row-major order. */
    int32_t band_rows, band_index, band_count;
    int32_t kernel;           /* RT_KERNEL_* */
    int32_t tile_order;       /* RT_TILES_*: block -> pixel-tile order (speed only) */
    int32_t flags;            /* RT_FLAG_* */
} rt_render_opts;

enum {
    RT_FLAG_NO_CULL = 1,      /* disable tile culling against the root box (A/B; same output) */
    RT_FLAG_BINARY = 4        /* wave traversal over the binary nodes, not the 4-ary records */
};

enum {
    RT_TILES_AUTO = 0,        /* RT_TILES_ROWS */
    RT_TILES_LINEAR = 1,      /* block b renders tile b (dispatch deals blocks round-robin to XCDs) */
    RT_TILES_XCD_CHUNK = 2,   /* each XCD's blocks take one contiguous 1/8 of the tiles */
    RT_TILES_ROWS = 3         /* each XCD's blocks take every 8th row of tiles */
};
void rt_render_opts_default(rt_render_opts* o);

/* Rows covered by (band_rows, band_index, band_count) for an H-row image. */
int rt_shard_rows(int height, int band_rows, int band_index, int band_count);

/* Render into device memory on `hip_stream` (hipStream_t; NULL = the null stream), no
 * host sync.  rgb_dev: rows*W*3 floats.  hit_idx_dev / hit_t_dev (optional, rows*W*spp):
 * primary-ray triangle index (-1 = miss) and t per (pixel, sample).
 * Stream-ordered: the frame's work starts after everything queued on hip_stream before the
 * call and is complete when hip_stream reaches the end of this call's work.  (A frame's tile
 * pre-passes, which write the culled tiles' pixels, run on the scene's own stream after an
 * event wait on hip_stream; rt_renderer, which orders its buffer reuse on the host, lets them
 * overlap the previous frame's render kernel instead.)  Frames of one scene are ordered: a
 * call on another stream than the scene's previous frame makes its stream wait for that frame. */
int rt_render_device(rt_scene* s, const rt_camera* cam, const rt_render_opts* opt,
                     float* rgb_dev, int32_t* hit_idx_dev, float* hit_t_dev, void* hip_stream);

/* rt_render_device that also writes the pixels' P6 samples (write_p6 defaults: maxval 255,
 * clamp, sqrt gamma; ppm_p6.cpp:137-155) to p6_dev (rows*W*3 bytes, same row order as
 * rgb_dev) from the render and cull kernels themselves: the frame epilogue fused into the
 * kernels that produce the pixels (p6_dev may be NULL).  rgb_dev may be NULL when p6_dev is
 * not: the frame is then produced as P6 samples only. */
int rt_render_device_p6(rt_scene* s, const rt_camera* cam, const rt_render_opts* opt,
                        float* rgb_dev, int32_t* hit_idx_dev, float* hit_t_dev, uint8_t* p6_dev,
                        void* hip_stream);

/* Two frames of one scene with the same options (two cameras of the same pixel size, e.g. the
 * next two frames of a sequence), as rt_render_device_p6 twice (frame a, then frame b; the same
 * images), rendered by one launch of the render kernel where it fits them
 * (RT_TUNE_PAIR_FRAMES): the second frame's work fills the first's tail and the launch gap
 * between two frames goes.  This batching is this library's own: the reference renders one
 * frame per render() call (G/src/main.cu:362-378 is a 1x1 warm-up launch, then one timed
 * render).  Outputs of a and b must not overlap. */
int rt_render_device_pair(rt_scene* s, const rt_camera* cam_a, const rt_camera* cam_b,
                          const rt_render_opts* opt, float* rgb_a_dev, uint8_t* p6_a_dev,
                          float* rgb_b_dev, uint8_t* p6_b_dev, void* hip_stream);

/* Synchronous convenience: render into host memory (rows*W*3 floats, + optional AOVs). */
int rt_render(rt_scene* s, const rt_camera* cam, const rt_render_opts* opt,
              float* rgb_host, int32_t* hit_idx_host, float* hit_t_host);

/* Rays one frame of rt_render traces, in the oracle's classes: counts[0] camera rays
 * (W*rows*spp when max_depth > 0), counts[1] shadow rays (IsInShadow calls that cast a ray,
 * shader.h:44-62 behind ShadeDirect's NdotL > 0, shader.h:87-93), counts[2] bounce rays
 * (TraceRayIterative depths > 0, query.h:156-220).  Renders the frame once more with counting
 * kernels (not the timed ones) and discards it; synchronous.  For total rays/s
 * (SURVEY.md §8(d)). */
int rt_count_rays(rt_scene* s, const rt_camera* cam, const rt_render_opts* opt, uint64_t counts[3]);
/* rt_count_rays + counts[3]: the camera rays that are traversed, i.e. those of the pixel tiles
 * the culling pre-passes leave to the render kernel (the others provably miss every box of the
 * tree, their samples are written as misses without a traversal). */
int rt_count_rays_ex(rt_scene* s, const rt_camera* cam, const rt_render_opts* opt, uint64_t counts[4]);

/* The reference signature verbatim (query.h:13-29) over host arrays: uploads to device 0,
 * renders on the GPU, writes W*H Vec3 to `output` (host).  Synchronous. */
int rt_render_reference(size_t num_triangles, int W, int H, const rt_camera* cam, rt_vec3 miss_color,
                        int max_depth, int spp, const rt_bvh_node* nodes, const rt_aabb* aabbs,
                        const rt_triangle* triangles, const int32_t* tri_object_ids,
                        const rt_material* materials, int num_materials, const rt_light* lights,
                        int num_lights, int diffuse_bounce, rt_vec3* output);

/* rt_render_reference over n_gpus devices (0..n_gpus-1) of this process: the image's 8-row
 * bands dealt round-robin over the GPUs, the float strips gathered to device 0 with RCCL and
 * copied into `output` (host).  The frame equals rt_render_reference's bit for bit.
 * (SURVEY.md §8(b) n_gpus / §8(e); G/include/query.h:13-29 has no multi-GPU form.) */
int rt_render_reference_gpus(size_t num_triangles, int W, int H, const rt_camera* cam, rt_vec3 miss_color,
                             int max_depth, int spp, const rt_bvh_node* nodes, const rt_aabb* aabbs,
                             const rt_triangle* triangles, const int32_t* tri_object_ids,
                             const rt_material* materials, int num_materials, const rt_light* lights,
                             int num_lights, int diffuse_bounce, int n_gpus, rt_vec3* output);

/* ---- frame renderer: render(scene, camera) -> frame in host memory on 1..N GPUs ----------
 * The loop around render() in G/src/main.cu:362-378 (render, then the frame copied to host
 * memory), pipelined and sharded.  Per frame, every rank renders the bands b with
 * b % world_size == rank (band_rows-row bands, rt_render_opts sharding) into a device strip on
 * its compute stream; the strips reach rank 0 over RCCL (one grouped ncclSend/ncclRecv per
 * rank on a comm stream, xGMI between GPUs); rank 0 copies them into a pinned host frame on a
 * copy stream, placing every band at its image rows (2-D copies: no un-permute pass).  Frames
 * are double/triple-buffered: frame k+1 renders while frame k is gathered and copied.
 *
 * Ranks: the process drives n_devices GPUs as global ranks rank0 .. rank0+n_devices-1 of
 * world_size.  world_size == n_devices (or 0): one process, the communicator made with
 * ncclCommInitAll.  world_size > n_devices: one rank group of a multi-process job (e.g. one
 * process per GPU under torchrun); every process passes the same 128-byte unique_id, made by
 * rt_comm_unique_id on the process holding rank 0 and shared by the caller.
 * A device id may repeat (several band shards on one GPU, for tests): then gather must be
 * RT_GATHER_DIRECT (one process) or RT_GATHER_HOST_SHARED (several), each rank copying its
 * bands straight into the host frame.
 *
 * RT_GATHER_HOST_SHARED (one process per GPU, e.g. under torchrun): the depth host frames are
 * one POSIX shared-memory segment (host_frame_name, the same on every process; rank 0's
 * process creates it, the others attach, each pins it with hipHostRegister).  Every rank
 * copies its own bands over its own PCIe link into their image rows, then publishes the frame
 * in the segment's per-rank completion word; rank 0's rt_renderer_wait returns once every rank
 * has published.  A rank copies frame t into a slot only after rank 0 has submitted frame t
 * (rank 0's caller then no longer holds frame t-depth).  RCCL is not used on this path. */
typedef struct rt_renderer rt_renderer;

enum {
    RT_DELIVER_P6 = 0,     /* the P6 body (write_p6 defaults), W*H*3 bytes, rows top to bottom */
    RT_DELIVER_F32 = 1,    /* the float framebuffer, W*H*3 floats (the reference's output) */
    RT_DELIVER_DEVICE = 2, /* P6 body assembled in rank 0's device memory; no host copy */
    RT_DELIVER_NONE = 3    /* render only (strips stay on each rank): measurement */
};
enum {
    RT_GATHER_AUTO = 0,    /* one process: DIRECT; several: HOST_SHARED with host_frame_name, else RCCL */
    RT_GATHER_RCCL = 1,    /* strips -> rank 0's GPU over RCCL, then one host copy stream */
    RT_GATHER_DIRECT = 2,  /* each local rank copies its own bands into the host frame (its own
                              PCIe link); single process only */
    RT_GATHER_HOST_SHARED = 3 /* each rank of a multi-process job copies its own bands into one
                                 host frame shared by the processes (host_frame_name); no RCCL */
};
enum { RT_RENDERER_SELF_SEND = 1 /* rank 0's own strip also goes through RCCL (tests at world 1) */ };

typedef struct {
    int32_t n_devices;        /* GPUs this process drives (1..64) */
    const int32_t* devices;   /* their device ids; NULL = 0 .. n_devices-1 */
    int32_t world_size;       /* ranks over all processes; 0 = n_devices */
    int32_t rank0;            /* global rank of devices[0]; the others follow */
    const void* unique_id;    /* 128 bytes (world_size > n_devices) */
    int32_t band_rows;        /* default 8 */
    int32_t deliver;          /* RT_DELIVER_* */
    int32_t gather;           /* RT_GATHER_* */
    int32_t depth;            /* frames in flight, 1..8 (default 3) */
    int32_t flags;            /* RT_RENDERER_* */
    const char* host_frame_name; /* RT_GATHER_HOST_SHARED: shared-memory name ("/..."), same on every
                                    process; RT_GATHER_AUTO picks HOST_SHARED for a multi-process
                                    renderer when it is set (RCCL otherwise) */
} rt_renderer_opts;
void rt_renderer_opts_default(rt_renderer_opts* o);

/* 1 when the renderer delivers its frames with SDMA copies queued through the HSA runtime (one
 * rank, RT_GATHER_DIRECT, a host frame; RT_TUNE_COPY_ENGINE), 0 when with the HIP runtime's
 * copies (blit kernels on the CUs). */
int rt_renderer_copy_engine(const rt_renderer* r);

/* 128-byte RCCL unique id for a multi-process renderer (call on rank 0's process). */
int rt_comm_unique_id(void* id128);

/* Scene upload (rt_scene_create's arguments) to every local device (one upload, then
 * device-to-device clones), stream/event/communicator setup. */
int rt_renderer_create(size_t num_triangles, const rt_bvh_node* nodes, const rt_aabb* aabbs,
                       const rt_triangle* triangles, const int32_t* tri_object_ids,
                       const rt_material* materials, int num_materials, const rt_light* lights,
                       int num_lights, const rt_renderer_opts* opts, rt_renderer** out);
void rt_renderer_destroy(rt_renderer* r);

/* Enqueue one frame (opts: its band fields are the renderer's).  Blocks only to reuse the
 * buffers of frame ticket-depth, which must then be complete.  *ticket numbers the frames. */
int rt_renderer_submit(rt_renderer* r, const rt_camera* cam, const rt_render_opts* opts, uint64_t* ticket);
/* Enqueue two frames (tickets *ticket_a, *ticket_a + 1) with the same options, rendered by one
 * launch per local rank (rt_render_device_pair); delivered as two rt_renderer_submit calls
 * would deliver them.  Needs depth >= 2; blocks to reuse both frames' buffers. */
int rt_renderer_submit_pair(rt_renderer* r, const rt_camera* cam_a, const rt_camera* cam_b,
                            const rt_render_opts* opts, uint64_t* ticket_a);
/* Wait for frame `ticket` (one of the last `depth` submitted, and not from before a change of
 * the frame size, which reallocates the buffers).  On the process holding rank 0,
 * *frame / *bytes give the delivered frame: pinned host memory (RT_DELIVER_P6/F32) or rank 0's
 * device memory (RT_DELIVER_DEVICE), valid until the submit of frame ticket+depth; elsewhere
 * NULL / 0.  Either pointer may be NULL. */
int rt_renderer_wait(rt_renderer* r, uint64_t ticket, const void** frame, size_t* bytes);
/* submit + wait + copy of the frame into out (cap bytes; rank 0 only). */
int rt_renderer_render(rt_renderer* r, const rt_camera* cam, const rt_render_opts* opts, void* out, size_t cap);
/* Local rank i's scene (for rt_frame_times / rt_kernel_times / rt_live_tiles). */
rt_scene* rt_renderer_scene(rt_renderer* r, int i);
int rt_renderer_local_ranks(const rt_renderer* r);
/* Durations (ms) of the gather (RT_TIME_GATHER: rank 0's receives, or its copy wait in DIRECT
 * mode) or of the host copy (RT_TIME_DELIVER) of the last min(max, frames) frames, oldest
 * first, from HIP events on those streams (rank 0's process; n_out = 0 elsewhere). */
enum { RT_TIME_GATHER = 0, RT_TIME_DELIVER = 1, RT_TIME_FRAME = 2 /* first render launch -> frame delivered */ };
int rt_renderer_times(rt_renderer* r, int kind, float* ms_out, int max, int* n_out);

/* HW1 brute-force path on the GPU (HW1/src/render.cpp:72-116 semantics: every triangle,
 * closest t >= 0 with the first index winning ties, HW1 shade).  Synchronous; host I/O. */
int rt_render_hw1(int device, const rt_vec3* positions, const rt_vec3* normals,
                  const uint32_t* indices, size_t num_triangles, const rt_camera* cam,
                  rt_vec3 light_position, rt_vec3 light_color, int spp, const float* jitter,
                  float* rgb_host, int32_t* hit_idx_host, float* hit_t_host);

/* rt_render_hw1 with a kernel selection and the device time of the kernels (HIP events;
 * kernel_ms may be NULL).  flags 0: binned — a conservative per-triangle pixel rectangle
 * (outside it ray_intersection provably rejects every camera ray), then per 16x16 block the
 * brute-force loop over the triangles whose rectangle meets the block, in index order, so
 * the output equals the brute-force loop's bit for bit; RT_HW1_BRUTE: every triangle for
 * every ray (HW1/src/render.cpp:72-116 literally). */
enum { RT_HW1_BRUTE = 1 };
int rt_render_hw1_ex(int device, const rt_vec3* positions, const rt_vec3* normals,
                     const uint32_t* indices, size_t num_triangles, const rt_camera* cam,
                     rt_vec3 light_position, rt_vec3 light_color, int spp, const float* jitter,
                     int flags, float* rgb_host, int32_t* hit_idx_host, float* hit_t_host,
                     float* kernel_ms);

/* Resident HW1 mesh for repeated frames (the C2 configuration on the device): the mesh packed
 * and uploaded once, the binning buffers kept.  rt_render_hw1_device renders one frame on
 * hip_stream (NULL = the default stream) without synchronising: rgb_dev (W*H*3 floats) and/or
 * p6_dev (W*H*3 bytes, write_p6 defaults) and the optional AOVs (W*H*spp each) are device
 * pointers; jitter NULL = jittered_samples(spp, 42) in [0,1); a caller's table with an entry
 * outside [0,1) takes the brute-force kernel (exact for every table).  rt_hw1_kernel_times: ms of the
 * frame's kernels (events around them) for the latest min(max, frames, 64) frames, oldest first;
 * rt_hw1_kernel_name: the render kernel the latest frame launched, as rocprofv3 names it. */
typedef struct rt_hw1_scene rt_hw1_scene;
int rt_hw1_scene_create(int device, const rt_vec3* positions, const rt_vec3* normals, const uint32_t* indices,
                        size_t num_triangles, rt_hw1_scene** out);
void rt_hw1_scene_destroy(rt_hw1_scene* s);
int rt_render_hw1_device(rt_hw1_scene* s, const rt_camera* cam, rt_vec3 light_position, rt_vec3 light_color,
                         int spp, const float* jitter, int flags, float* rgb_dev, uint8_t* p6_dev,
                         int32_t* hit_idx_dev, float* hit_t_dev, void* hip_stream);
/* One frame as rt_render_hw1_device renders it, into one of the scene's 8 device P6 bodies, then
 * that body copied to host_p6 (W*H*3 bytes, pinned) once the frame's kernels are done — by a DMA
 * (SDMA) engine, queued from a copier thread, or with RT_TUNE_COPY_ENGINE 0 by the HIP runtime
 * on the scene's copy stream — so the copy overlaps the next frames' kernels; *ticket numbers the
 * frame.  Frames alternate over the scene's lanes (binning buffers and a stream each,
 * RT_TUNE_HW1_LANES), after the work queued on hip_stream so far.  host_p6 must stay valid until
 * rt_hw1_wait(ticket) returns; a frame reuses the device body of the frame 8 before it (after
 * that frame's copy). */
int rt_render_hw1_deliver(rt_hw1_scene* s, const rt_camera* cam, rt_vec3 light_position, rt_vec3 light_color,
                          int spp, int flags, uint8_t* host_p6, void* hip_stream, uint64_t* ticket);
int rt_hw1_wait(rt_hw1_scene* s, uint64_t ticket);
int rt_hw1_kernel_times(const rt_hw1_scene* s, float* ms_out, int max, int* n_out);
const char* rt_hw1_kernel_name(const rt_hw1_scene* s);
/* info = {entries the bin list holds now, the latest frame's list total (waits for it)}: a
 * total above the capacity its frame ran with means that frame's overflowing tiles took the
 * brute-force loop; the next frame runs with a grown list. */
int rt_hw1_list_info(const rt_hw1_scene* s, int64_t info[2]);

/* The binned path's per-triangle bounds and their read-back, for tests.
 * The bounds assume the sample positions ix = (int)(x + jx) in {x, x + 1}, that is a jitter table
 * in [0,1).  rt_render_hw1_device and rt_render_hw1_ex therefore render a caller's table with any
 * entry outside [0,1) (NaN included) with the brute-force kernel, which is exact for every table;
 * rt_hw1_kernel_name says which kernel a frame took.
 * rt_hw1_rects_host: host build of the bounds (no device needed, like rt_powf_host), through the
 *   functions the count pass runs: per triangle k, rects[4k..] = (ix_lo, iy_lo, ix_hi, iy_hi), the
 *   integer pixel positions whose camera ray ray_intersection may accept (lo > hi: none), and
 *   tiles[4k..] = (tx0, tx1, ty0, ty1), the 16x4-pixel wave tiles listed for it, inclusive; an
 *   empty range is (0, -1, 0, -1).
 * rt_hw1_debug_bins: what the latest rt_render_hw1_device frame left in the scene's binning
 *   buffers (waits for that frame; RT_ERR_ARG when it took the brute-force kernel).  info =
 *   {triangles, tiles, list total, 1 if the total fits the capacity the frame ran with, else 0:
 *   tiles whose list ends past the capacity were not written}.  Each output may be NULL: rects
 *   4 * triangles ints, offsets tiles + 1 entries (offsets_cap: entries it holds), list
 *   min(total, capacity) triangle indices (list_cap: entries it holds), tile t's at
 *   [offsets[t], offsets[t + 1]) in the order the atomics gave.  Call with NULL outputs to size.
 * (Additive to ABI 3: rt_hw1_rects_host, rt_hw1_debug_bins.) */
int rt_hw1_rects_host(const rt_camera* cam, const rt_vec3* positions, const uint32_t* indices, size_t num_triangles,
                      int32_t* rects, int32_t* tiles);
int rt_hw1_debug_bins(rt_hw1_scene* s, int64_t info[4], int32_t* rects, uint32_t* offsets, size_t offsets_cap,
                      uint32_t* list, size_t list_cap);

/* Batched ray-triangle queries on the GPU (one triangle, n rays from `origin`), the device
 * Möller–Trumbore used by the kernels:  hw1 != 0 -> HW1 ray_intersection
 * (HW1/include/ray.h:67-117; the HW1 Ray constructor normalises each direction first, ray.h:25),
 * hw1 == 0 -> G/ intersectTriangle (G/include/query.h:72-108) over [tmin, tmax] with the
 * direction used as given.  Host arrays; hit[i] in {0,1}, t[i] = -1 on a miss. */
int rt_intersect_rays(int device, const rt_triangle* tri, const float origin[3], const float* dirs, int n,
                      int hw1, float tmin, float tmax, int32_t* hit, float* t);

/* ---- batched ray queries on a resident scene ---------------------------------------------
 * The reference's ray-level queries for caller rays against an rt_scene: one ray per GPU lane,
 * each lane running the reference's DFS on its own.
 *
 * RT_RAYS_CLOSEST: SearchBVH(numTriangles, Ray(origin, direction), ...) exactly
 *   (G/include/query.h:224-311): tmin = 1e-4 (:233), bestT = FLT_MAX, the direction used as given
 *   (never normalised), a later-visited triangle with t <= bestT wins (query.h:72-108 through
 *   :268-275), and on a tree that overflows the 512-entry stack (:245) the brute-force completion
 *   over every triangle in index order decides (:298-308).  hit_idx[i] = the triangle index, or -1
 *   on a miss; hit_t[i] = the reference's t bit for bit, or -1.0f on a miss (what
 *   rt_intersect_rays writes); hit_t may be NULL.  max_t must be NULL (the reference has no such
 *   bound): RT_ERR_ARG otherwise.
 * RT_RAYS_OCCLUDED: the decision of IsInShadow (G/include/shader.h:59-61): hit_idx[i] = 1 iff
 *   SearchBVH hits and t < max_t[i], else 0 (a NaN max_t[i] gives 0).  max_t is required and hit_t
 *   must be NULL (RT_ERR_ARG otherwise): a lane may stop at the first accepted triangle with
 *   t < max_t[i] (bestT only decreases after it, so the decision stands), and the closest t is
 *   then not known.
 * flags: RT_FLAG_BINARY traverses the binary records, not the 4-ary ones (same answers); any other
 *   bit is RT_ERR_ARG.  n == 0 is RT_OK with no launch; n > 2^31-1 is RT_ERR_UNSUPPORTED.  A null
 *   scene, rays or hit_idx is RT_ERR_ARG.  Every argument check runs before any HIP call.
 * A query reads only the scene's immutable packed arrays and takes no part in the frame ordering
 * of rt_render_device (none of its events, work buffers or frame counters): it may run on any
 * stream, and from any thread, beside frames of the same scene, of a clone (rt_scene_clone) or of
 * a scene owned by an rt_renderer (rt_renderer_scene).
 * For any float bit patterns in rays and max_t the call terminates and writes every output (the
 * DFS visits each node at most once whatever the comparisons say); the results are specified
 * for finite rays only. */
typedef struct { rt_vec3 origin, direction; } rt_ray;   /* layout = reference: Ray, G/include/ray.h:6-22 (24 B) */
enum { RT_RAYS_CLOSEST = 0, RT_RAYS_OCCLUDED = 1 };
enum { RT_RAYS_VARIANT_NONE = 0, RT_RAYS_VARIANT_WIDE = 1, RT_RAYS_VARIANT_BINARY = 2, RT_RAYS_VARIANT_DEEP = 3 };

/* Asynchronous on hip_stream (NULL = the null stream); all pointers are device pointers on the
 * scene's device: rays_dev n rt_ray, max_t_dev / hit_idx_dev / hit_t_dev n entries each. */
int rt_trace_rays_device(rt_scene* s, int mode, const rt_ray* rays_dev, const float* max_t_dev, size_t n,
                         int flags, int32_t* hit_idx_dev, float* hit_t_dev, void* hip_stream);
/* Host arrays; uploads, traces, downloads, synchronises.  kernel_ms (may be NULL): HIP-event time
 * of the kernel. */
int rt_trace_rays(rt_scene* s, int mode, const rt_ray* rays, const float* max_t, size_t n, int flags,
                  int32_t* hit_idx, float* hit_t, float* kernel_ms);
/* Which traversal the latest rt_trace_rays[_device] call on s launched (RT_RAYS_VARIANT_*; NONE
 * before the first): DEEP (SearchBVH as written, 512-entry private stack) for a scene that takes
 * the deep kernels (rt_scene_traversal_info) or whose per-lane stack does not fit LDS, else WIDE
 * (4-ary records, per-lane stack in LDS) or, with RT_FLAG_BINARY, BINARY. */
int rt_trace_rays_variant(const rt_scene* s);

/* ---- radiance queries on a resident scene -------------------------------------------------
 * The reference's ray-level entry point for caller rays: radiance[3i..3i+2] =
 *   TraceRayIterative(Ray(origin_i, direction_i), max_depth, miss_color, ..., rng_state = seeds[i],
 *                     diffuse_bounce)                                  (G/include/query.h:156-220)
 * bit for bit, the final clamp to [0, 1] included: one path per GPU lane with ShadeDirect's direct
 * lighting and hard shadow rays (G/include/shader.h:44-110), the diffuse / mirror bounce and the
 * throughput cut-off.  seeds == NULL: 42u for every ray, the reference's default argument.  The
 * direction is used as given, as the reference uses primaryRay, and normalised only where the
 * reference normalises it (unit_vector(ray.direction()) in the mirror branch).  Results are pinned
 * against the reference for unit-length directions only.
 * hit_idx / hit_t (each may be NULL): SearchBVH's result for the first segment, in rt_trace_rays'
 *   conventions (-1 / -1.0f on a miss).  max_depth <= 0: radiance 0, -1 / -1.0f, no ray is traced
 *   (query.h:172).
 * opt->flags: RT_FLAG_BINARY or 0, as for rt_trace_rays; any other bit is RT_ERR_ARG.  A null
 *   scene, rays, opt or radiance is RT_ERR_ARG; n > 2^31-1 is RT_ERR_UNSUPPORTED; n == 0 is RT_OK
 *   with no launch.  Every argument check runs before any HIP call.
 * Like a query, a shade call reads only the scene's immutable arrays, takes no part in the frame
 * ordering and may run on any stream, from any thread, beside frames of the same scene, of a clone
 * or of an rt_renderer's scene.  For any float bit patterns it terminates (at most max_depth
 * segments, each a DFS that visits a node at most once) and writes every output.
 * (Additive to ABI 3: rt_shade_opts, rt_shade_opts_default, rt_shade_rays, rt_shade_rays_device,
 * rt_shade_rays_variant.) */
typedef struct {
    int32_t max_depth;        /* TraceRayIterative's maxDepth */
    int32_t diffuse_bounce;
    rt_vec3 miss_color;
    int32_t flags;            /* RT_FLAG_BINARY or 0 */
} rt_shade_opts;
void rt_shade_opts_default(rt_shade_opts* o);   /* 1, 1, (0,0,0), 0 */

/* Asynchronous on hip_stream (NULL = the null stream); device pointers on the scene's device:
 * rays_dev n rt_ray, seeds_dev n (or NULL), radiance_dev 3n, hit_idx_dev / hit_t_dev n (or NULL). */
int rt_shade_rays_device(rt_scene* s, const rt_ray* rays_dev, const uint32_t* seeds_dev, size_t n,
                         const rt_shade_opts* opt, float* radiance_dev, int32_t* hit_idx_dev, float* hit_t_dev,
                         void* hip_stream);
/* Host arrays; uploads, shades, downloads, synchronises.  kernel_ms (may be NULL): HIP-event time
 * of the kernel. */
int rt_shade_rays(rt_scene* s, const rt_ray* rays, const uint32_t* seeds, size_t n, const rt_shade_opts* opt,
                  float* radiance, int32_t* hit_idx, float* hit_t, float* kernel_ms);
/* RT_RAYS_VARIANT_* of the latest rt_shade_rays[_device] call on s (NONE before the first), by
 * rt_trace_rays_variant's rule; a word of its own, which rt_trace_rays does not write. */
int rt_shade_rays_variant(const rt_scene* s);

/* ---- hit records on a resident scene -------------------------------------------------------
 * Between the two queries above: for caller rays, the whole HitRecord that
 * SearchBVH returns (G/include/query.h:224-311 with intersectTriangle's tail, :110-130) and the
 * ids assignMaterialToHit reads (:134-153), bit for bit, for callers that shade for themselves
 * (G-buffers, texture lookups, picking with a normal, baking, a BRDF of their own).
 * rt_trace_hits follows rt_trace_rays in RT_RAYS_CLOSEST mode in every convention: the direction is
 *   used as given, tmin = 1e-4, the same tie rule, deep-tree overflow rule and brute-force
 *   completion, so tri and t are rt_trace_rays' hit_idx and hit_t.  A miss writes tri = -1,
 *   t = -1.0f and zero in every other field; every byte of every record is written.
 * flags: RT_FLAG_BINARY or 0; any other bit is RT_ERR_ARG.  n == 0 is RT_OK with no launch;
 *   n > 2^31-1 is RT_ERR_UNSUPPORTED.  A null scene, rays or hits is RT_ERR_ARG, and so is a
 *   hits_dev that is not 16-byte aligned (the kernel stores 16-byte words; the host entry's
 *   `hits` needs no alignment).  Every argument check runs before any HIP call.
 * Like a query it reads only the scene's immutable arrays and takes no part in the frame ordering:
 * any stream, any thread, beside frames of the same scene, of a clone or of an rt_renderer's
 * scene.  For any float bit patterns in rays it terminates and writes every record; the results
 * are specified for finite rays only.
 * (Additive to ABI 3: rt_hit, rt_trace_hits, rt_trace_hits_device, rt_trace_hits_variant,
 * rt_hit_record_host, rt_camera_rays_host, rt_camera_rays_device.) */
typedef struct {            /* 64 bytes, this library's own layout */
    int32_t tri;            /* triangle index; -1: miss */
    float   t, u, v;        /* intersectTriangle's t, u, v (query.h:92-104) */
    rt_vec3 p;              /* rec.p = origin + direction * t */
    rt_vec3 normal;         /* rec.normal: the shading normal of query.h:119-128 */
    rt_vec3 geom_normal;    /* geomN of query.h:115-117, after the flip towards the ray */
    int32_t front_face;     /* rec.front_face, 0 / 1 */
    int32_t object_id;      /* triObjectIds[tri] as stored (-1 when the scene has none) */
    int32_t material;       /* the index assignMaterialToHit takes (query.h:149-152), -1: Material() defaults */
} rt_hit;

/* Asynchronous on hip_stream (NULL = the null stream); device pointers on the scene's device:
 * rays_dev n rt_ray, hits_dev n rt_hit (16-byte aligned). */
int rt_trace_hits_device(rt_scene* s, const rt_ray* rays_dev, size_t n, int flags, rt_hit* hits_dev, void* hip_stream);
/* Host arrays; uploads, traces, downloads, synchronises.  kernel_ms (may be NULL): HIP-event time
 * of the kernel. */
int rt_trace_hits(rt_scene* s, const rt_ray* rays, size_t n, int flags, rt_hit* hits, float* kernel_ms);
/* RT_RAYS_VARIANT_* of the latest rt_trace_hits[_device] call on s (NONE before the first), by
 * rt_trace_rays_variant's rule; a word of its own, which the other queries do not write. */
int rt_trace_hits_variant(const rt_scene* s);

/* Host build of the record's arithmetic (no device needed, like rt_powf_host): out[i] =
 * intersectTriangle(rays[i], tris[i], 1e-4f, FLT_MAX) as a full record, through the functions the
 * kernel runs.  tri = i on a hit, object_id = material = -1; a miss record otherwise. */
int rt_hit_record_host(const rt_ray* rays, const rt_triangle* tris, int n, rt_hit* out);

/* ---- multi-hit queries on a resident scene ---------------------------------------------------
 * Every surface along a caller ray, not only the first: the number of triangles
 * the ray hits up to a bound, and the k nearest of them in order — alpha cut-outs and transparent
 * shadow rays, thickness and X-ray images, inside/outside tests by crossing parity, depth-ordered
 * surface lists.
 *
 * For a ray (origin, direction) and a bound tmax (max_t[i]; FLT_MAX when max_t is NULL) the hit
 * set S is what SearchBVH (G/include/query.h:224-311) would collect if
 *   - the bound it passes to intersectAABB and intersectTriangle stayed at tmax and were never
 *     lowered to a hit,
 *   - every accepted triangle were kept, not only the last one,
 *   - the direction is used as given and tmin = 1e-4, as in every query here.
 * Without stack overflow S is the set of triangles for which every box on the root-to-leaf path,
 *   the root's own and the leaf's own included, passes intersectAABB(ray, box, 1e-4, tmax) and
 *   intersectTriangle(ray, tri, 1e-4, tmax) accepts (t <= tmax counts).  A leaf that names no
 *   triangle contributes nothing.  With one bound the push-time and pop-time tests of a box agree
 *   and the order of the visit does not matter.  (A triangle is counted once per leaf that names it.)
 * With stack overflow the rule follows the reference's 512-entry stack: SearchBVH pops a node,
 *   tests its own box, then pushes left and right when their boxes pass; if that control flow, run
 *   with the fixed bound, would set its overflow flag for this ray, S is instead every triangle of
 *   the scene that intersectTriangle(ray, tri, 1e-4, tmax) accepts: the reference's brute-force
 *   completion, a superset of what the DFS saw.  Whether a ray overflows is a deterministic
 *   property of the tree, the ray and tmax.
 * Outputs per ray: count[i] = |S|, the full number of hits, which may exceed k; hits[i*k + j] for
 *   j < min(|S|, k) are the first members of S by ascending t, then by ascending triangle index,
 *   each with intersectTriangle's t, u, v bit for bit (the t, u, v rt_hit has for that triangle);
 *   slots j >= |S| get tri = -1, t = -1.0f, u = v = 0.  Every byte of hits[i*k .. i*k + k-1] and of
 *   count[i] is written.
 * Nothing is pruned by the k-th distance: count would lose its meaning, and a float box test
 *   cannot prove a subtree empty of closer hits exactly.
 * Always true: the reference's closest hit is a member of S (its boxes passed with a smaller bound,
 *   and the slab test is monotone in tmax), count > 0 exactly when SearchBVH hits (with max_t NULL),
 *   and hits[0].t <= the closest-hit query's t.
 * Arguments: 0 <= k <= RT_MULTI_HIT_MAX_K.  With k == 0 only the counts are produced and hits may
 *   be NULL; with k > 0 count may be NULL.  RT_ERR_ARG: a null scene or rays, k out of range, no
 *   output (k == 0 with a null count, k > 0 with null hits), a hits_dev that is not 16-byte aligned
 *   (the kernel stores 16-byte words; the host entry's `hits` needs no alignment), a flag bit other
 *   than RT_FLAG_BINARY.  n == 0 is RT_OK with no launch; n > 2^31-1 or n*k > 2^31-1 is
 *   RT_ERR_UNSUPPORTED.  Every argument check runs before any HIP call.
 * For any float bit patterns in rays and max_t the call terminates and writes every output; the
 *   results are specified for finite rays and a max_t that is not NaN.
 * Like the other queries it reads only the scene's current packed arrays (after rt_scene_refit /
 * rt_scene_rebuild: the new ones) and takes no part in the frame ordering: any stream, any thread,
 * beside frames of the same scene, of a clone or of an rt_renderer's scene.
 * (Additive to ABI 3: rt_multi_hit, RT_MULTI_HIT_MAX_K, rt_trace_multi_hits,
 * rt_trace_multi_hits_device, rt_trace_multi_hits_variant, rt_multi_hits_host.) */
typedef struct {            /* 16 bytes */
    int32_t tri;            /* triangle index; -1: no such hit */
    float   t, u, v;        /* intersectTriangle's t, u, v (query.h:92-104) */
} rt_multi_hit;
#define RT_MULTI_HIT_MAX_K 32

/* Asynchronous on hip_stream (NULL = the null stream); device pointers on the scene's device:
 * rays_dev n rt_ray, max_t_dev n floats (or NULL), hits_dev n*k rt_multi_hit (16-byte aligned; may
 * be NULL with k == 0), count_dev n (may be NULL with k > 0). */
int rt_trace_multi_hits_device(rt_scene* s, const rt_ray* rays_dev, const float* max_t_dev, size_t n, int k, int flags,
                               rt_multi_hit* hits_dev, int32_t* count_dev, void* hip_stream);
/* Host arrays; uploads, traces, downloads, synchronises.  kernel_ms (may be NULL): HIP-event time
 * of the kernel. */
int rt_trace_multi_hits(rt_scene* s, const rt_ray* rays, const float* max_t, size_t n, int k, int flags,
                        rt_multi_hit* hits, int32_t* count, float* kernel_ms);
/* RT_RAYS_VARIANT_* of the latest rt_trace_multi_hits[_device] call on s (NONE before the first),
 * by rt_trace_rays_variant's rule; a word of its own, which the other queries do not write. */
int rt_trace_multi_hits_variant(const rt_scene* s);
/* The host build of the query (no device needed): the definition above, the overflow rule
 * included, on arrays in the reference layout (P triangles, 2P-1 nodes and boxes, the root node
 * 0), through the box and triangle tests the kernel runs.  max_t, hits and count as for
 * rt_trace_multi_hits.  A child index outside the node array, or nodes that are not a tree, are
 * RT_ERR_ARG. */
int rt_multi_hits_host(size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs, const rt_triangle* tris,
                       const rt_ray* rays, const float* max_t, size_t n, int k, rt_multi_hit* hits, int32_t* count);

/* ---- closest-point queries on a resident scene ------------------------------------------------
 * The query that starts from a point, not a ray: per point the nearest triangle
 * of the scene, the squared distance and the nearest point — distance fields, snapping and picking
 * without a direction, proximity tests, attribute transfer between meshes.
 *
 * Definition.  All arithmetic is float32 without contraction; dot(x, y) = (x0*y0 + x1*y1) + x2*y2,
 * len2(x) = dot(x, x).  The surfaces are the scene's leaves: node j in [P-1, 2P-1) with
 * object_idx = i < P, its triangle a = v0, e1 = v1 - v0, e2 = v2 - v0 (intersectTriangle's edges),
 * its box B_j = aabbs[j]; a leaf that names no triangle contributes nothing.  For a point q and a
 * leaf, with the regions tested in this order and the first match winning:
 *   ap = q - a;  d1 = dot(e1, ap);  d2 = dot(e2, ap)
 *   A  (region 0): d1 <= 0 && d2 <= 0                     -> v = 0, w = 0
 *   bp = ap - e1; d3 = dot(e1, bp);  d4 = dot(e2, bp)
 *   B  (1): d3 >= 0 && d4 <= d3                            -> v = 1, w = 0
 *   vc = d1*d4 - d3*d2
 *   AB (3): vc <= 0 && d1 >= 0 && d3 <= 0                  -> v = d1 / (d1 - d3), w = 0
 *   cp = ap - e2; d5 = dot(e1, cp);  d6 = dot(e2, cp)
 *   C  (2): d6 >= 0 && d5 <= d6                            -> v = 0, w = 1
 *   vb = d5*d2 - d1*d6
 *   AC (4): vb <= 0 && d2 >= 0 && d6 <= 0                  -> v = 0, w = d2 / (d2 - d6)
 *   va = d3*d6 - d5*d4
 *   BC (5): va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0    -> w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1 - w
 *   face (6): otherwise                                    -> den = 1 / ((va + vb) + vc); v = vb*den; w = vc*den
 *   p   = (a + e1*v) + e2*w                     per component, for every region
 *   p_c = p_c < lo_c ? lo_c : (p_c > hi_c ? hi_c : p_c)    confinement to B_j (a NaN stays NaN)
 *   D   = len2(q - p)
 * A candidate is accepted iff D < best_D || (D == best_D && i < best_tri), from best_D = max_d2[k]
 * (+inf when max_d2 is NULL) and best_tri = INT32_MAX: a surface at exactly max_d2 counts, the
 * lowest triangle index wins ties, a NaN D or a NaN bound never wins.  The answer is that of the
 * brute force over every leaf; the confinement is what makes the float distance to a box,
 * lb(q, B) = len2(q - c) with c = q confined to B, a lower bound of every D below it, so that the
 * kernel's pruned walk (a box is skipped iff lb > best_D) returns the same bytes in any order.
 * Output per point: the winner's rt_point_hit bit for bit, or {-1, -1.0f, 0, 0, 0, 0, 0, -1}; every
 * byte is written.  evals (may be NULL): per point the number of leaf triangles whose D was
 * computed (a lane whose stack filled up restarts with a scan of every leaf and reports their
 * number): a diagnostic of the pruning.
 * Specified for finite points and a tree whose boxes contain their children's boxes (rt_build_bvh*,
 * rt_refit_aabbs_host, refit and rebuild give such trees); for any bit patterns the call
 * terminates, visits a node at most once and writes every output.
 * Arguments: RT_ERR_ARG for a null scene, points or hits, a hits_dev that is not 16-byte aligned
 * (the kernel stores 16-byte words; the host entry's `hits` needs no alignment), a points, max_d2
 * or evals that is not 4-byte aligned, a flag bit other than RT_FLAG_BINARY; n == 0 is RT_OK with
 * no launch; n > 2^31-1 is RT_ERR_UNSUPPORTED.  Every argument check runs before any HIP call.
 * Like the other queries it reads only the scene's current packed arrays and takes no part in the
 * frame ordering: any stream, any thread, beside frames of the same scene or of a clone.
 * (Additive to ABI 3: rt_point_hit, rt_closest_points, rt_closest_points_device,
 * rt_closest_points_variant, rt_closest_points_host.) */
typedef struct {            /* 32 bytes */
    int32_t tri;            /* triangle index; -1: no surface within the bound */
    float   d2;             /* D, the squared distance */
    float   p[3];           /* the nearest point, confined to its leaf's box */
    float   v, w;           /* p = a + e1*v + e2*w before the confinement */
    int32_t region;         /* 0 A, 1 B, 2 C, 3 AB, 4 AC, 5 BC, 6 face; -1: none */
} rt_point_hit;

/* Asynchronous on hip_stream (NULL = the null stream); device pointers on the scene's device:
 * points_dev 3n floats, max_d2_dev n floats (or NULL), hits_dev n rt_point_hit (16-byte aligned),
 * evals_dev n (or NULL). */
int rt_closest_points_device(rt_scene* s, const float* points_dev, const float* max_d2_dev, size_t n, int flags,
                             rt_point_hit* hits_dev, uint32_t* evals_dev, void* hip_stream);
/* Host arrays; uploads, queries, downloads, synchronises.  kernel_ms (may be NULL): HIP-event time
 * of the kernel. */
int rt_closest_points(rt_scene* s, const float* points, const float* max_d2, size_t n, int flags,
                      rt_point_hit* hits, uint32_t* evals, float* kernel_ms);
/* RT_RAYS_VARIANT_* of the latest rt_closest_points[_device] call on s (NONE before the first), by
 * rt_trace_rays_variant's rule; a word of its own, which the other queries do not write. */
int rt_closest_points_variant(const rt_scene* s);
/* The host build of the query (no device needed) and its definition: the brute force over the
 * leaves in index order, on arrays in the reference layout (P triangles, 2P-1 nodes and boxes),
 * through the arithmetic the kernel runs.  evals (may be NULL) gets the number of leaves that name
 * a triangle. */
int rt_closest_points_host(size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs, const rt_triangle* tris,
                           const float* points, const float* max_d2, size_t n, rt_point_hit* hits, uint32_t* evals);

/* Camera rays of image rows [row0, row0 + rows): the rays render() shoots and the rng states it
 * gives them (G/include/query.cu:146-158), for rt_trace_rays / rt_trace_hits / rt_shade_rays.  The
 * ray of sample s of pixel (x, y) is at index ((y - row0) * W + x) * spp + s, the order of the
 * reference's AOVs: origin = cam->center, direction = unit_vector(pix - center) with
 * pix = (p00 + du * (float(x) + jx)) + dv * (float(y) + jy) as Camera::get_ray computes it, its
 * double division included (camera.h:49-53, 218-223); seeds[i] = make_rng_seed(x, y, s)
 * (query.h:44-48) with the absolute y.  jitter: 2*spp floats (jx, jy per sample); seeds may be NULL.
 * spp < 1, rows outside the image or a null camera or rays is RT_ERR_ARG; W * rows * spp > 2^31-1
 * is RT_ERR_UNSUPPORTED; rows == 0 is RT_OK and writes nothing.
 * rt_camera_rays_host needs no device; jitter == NULL means rt_jittered_samples(spp, 42, 1).
 * rt_camera_rays_device: one launch on hip_stream of `device` (asynchronous); jitter_dev, rays_dev
 * and seeds_dev are device pointers there, and a null jitter_dev is RT_ERR_ARG.  Every argument
 * check runs before any HIP call. */
int rt_camera_rays_host(const rt_camera* cam, int spp, const float* jitter, int row0, int rows, rt_ray* rays,
                        uint32_t* seeds);
int rt_camera_rays_device(int device, const rt_camera* cam, int spp, const float* jitter_dev, int row0, int rows,
                          rt_ray* rays_dev, uint32_t* seeds_dev, void* hip_stream);
/* The same for samples [sample0, sample0 + nsamples) of a longer table (a frame made in sample
 * passes): jitter holds the 2*nsamples floats of that slice, ray ((y - row0) * W + x) * nsamples + s
 * is sample sample0 + s of pixel (x, y) and its seed is make_rng_seed(x, y, sample0 + s).
 * sample0 == 0 is the call above; sample0 < 0 (or sample0 + nsamples past 2^31-1) is RT_ERR_ARG, and
 * so is a null jitter with sample0 > 0 on the host (the default table is a whole frame's). */
int rt_camera_rays_pass_host(const rt_camera* cam, int sample0, int nsamples, const float* jitter, int row0, int rows,
                             rt_ray* rays, uint32_t* seeds);
int rt_camera_rays_pass_device(int device, const rt_camera* cam, int sample0, int nsamples, const float* jitter_dev,
                               int row0, int rows, rt_ray* rays_dev, uint32_t* seeds_dev, void* hip_stream);

/* ---- film: radiance samples to a frame, on the device ---------------------------------------
 * The last step of a frame made from caller rays: per pixel and channel the
 * float sum of the radiance samples in the order they are added, col = col + sample as render()
 * adds them (G/include/query.cu:130-166), and from it render()'s pixel
 * float(double(col) / double(float(count))) and write_p6's byte.  camera rays -> rt_shade_rays ->
 * film is rt_render's frame bit for bit, and so is a film fed samples 0..k-1, then k..N-1, in row
 * bands or whole: the float sum is the same sequence of adds.
 * A film holds W*H*3 float sums on its device and a sample count per row on the host, updated when
 * a call is enqueued.  It takes no scene and touches no frame ordering, event or buffer of
 * rt_render_device.  Every call is one launch on the caller's hip_stream (NULL = the null stream),
 * asynchronous and ordered with the other film calls of that stream; calls on one film from
 * different streams or threads are the caller's to order.  Every argument check runs before any
 * HIP call.  Results are specified for finite radiance.
 * RT_ERR_ARG: a null film or radiance, nsamples < 1, rows outside the image, a resolve with both
 * outputs null or over rows whose counts differ or are 0.  rows * W * nsamples > 2^31-1 is
 * RT_ERR_UNSUPPORTED; rows == 0 is RT_OK with no launch.
 * (Additive to ABI 3: rt_film, rt_film_create, rt_film_destroy, rt_film_clear_device,
 * rt_film_add_device, rt_film_resolve_device, rt_film_row_samples, rt_film_pixels_host,
 * rt_camera_rays_pass_host, rt_camera_rays_pass_device.) */
typedef struct rt_film rt_film;
/* Sums of a width x height image on `device`, zeroed (synchronous). */
int rt_film_create(int device, int width, int height, rt_film** out);
void rt_film_destroy(rt_film* f);
/* The sums and every row's count to 0. */
int rt_film_clear_device(rt_film* f, void* hip_stream);
/* radiance_dev: rows*W*nsamples*3 floats, sample s of pixel (x, y) at ((y - row0) * W + x) * nsamples + s:
 * the order of rt_camera_rays_* and of rt_shade_rays' output for those rays.  Any alignment; a
 * 16-byte aligned pointer takes the faster kernel. */
int rt_film_add_device(rt_film* f, const float* radiance_dev, int row0, int rows, int nsamples, void* hip_stream);
/* rgb_dev (rows*W*3 floats) and/or p6_dev (rows*W*3 bytes, write_p6's defaults as
 * rt_render_device_p6 writes them); one of them may be NULL.  Does not clear: a film can be resolved
 * after every pass. */
int rt_film_resolve_device(rt_film* f, int row0, int rows, float* rgb_dev, uint8_t* p6_dev, void* hip_stream);
/* Samples added to that row since the film was made or cleared. */
int rt_film_row_samples(const rt_film* f, int row, int64_t* count);
/* Host build of the film's arithmetic (no device needed): adds radiance (rows*width*nsamples*3
 * floats, the layout above) to sum_inout (rows*width*3 running sums) and, unless rgb_out is NULL,
 * writes the pixels of count_after samples per pixel, the count after this add (>= nsamples). */
int rt_film_pixels_host(const float* radiance, int width, int rows, int nsamples, float* sum_inout,
                        int64_t count_after, float* rgb_out);

/* ---- path stages for caller hits -------------------------------------------------------------
 * The body of TraceRayIterative's depth loop (G/include/query.h:178-217) as a stage of its own
 * (DESIGN.md §4.21), for callers who change the surface between the trace and the shading: it
 * works on caller rays and hit records (rt_trace_hits' or the caller's own: only tri, p, normal
 * and material of a record are read) with an optional material per hit, and brings the library's
 * direct lighting, shadow rays and bounce to them.  A path runs as
 *   begin; repeat { rt_trace_hits_device -> [edit hits / pick materials] -> step -> compact }; finish
 * and with nothing edited its radiance is rt_shade_rays', and so the reference's, bit for bit.
 * All pointers are device pointers on the scene's (or `device`'s) device; every call is
 * asynchronous on hip_stream (NULL = the null stream) and ordered with the others of that stream.
 * There are no host-array forms: staged paths are a device-resident pipeline, rt_shade_rays is
 * the one-call form.
 *
 * The state of N paths, indexed by path id: radiance 3N floats, throughput 3N floats, rng N words.
 * rt_path_begin_device: radiance 0, throughput 1, rng[i] = seeds_dev ? seeds_dev[i] : 42u, the
 *   state at the top of TraceRayIterative (query.h:166-170).
 * rt_path_step_device: the loop body for entries k < m.  Entry k belongs to path
 *   id = ids_dev ? ids_dev[k] : k.  Ids are the caller's to keep unique within a call and below N:
 *   each state word then has one writer (plain stores, no atomics).  An id of RT_PATH_NONE marks an
 *   entry that carries no path (a path that ended, in a batch that is not compacted): no state
 *   word is read or written, alive[k] = 0, direct = 0, and its ray is copied to next_rays_dev[k].
 *   - hits[k].tri < 0 is a miss: radiance += throughput * miss_color, alive[k] = 0, direct = 0.
 *   - The material is mats_dev ? mats_dev[k] (13 floats, read through a 4-byte aligned pointer)
 *     : what assignMaterialToHit gives for the record (query.h:134-153): the scene's table entry
 *     hits[k].material, or the Material() defaults when that index is outside the table (-1).
 *   - ShadeDirect (G/include/shader.h:65-110) from the record: N = unit(hit.normal),
 *     V = unit(ray.origin - hit.p), ambient and emission of the material, then per scene light the
 *     NdotL > 0 test, IsInShadow's shadow ray (any-hit, bounded by the light's distance, skipped
 *     when that distance is <= 0) and EvaluateBRDF on the record's normal as stored.
 *     radiance += throughput * direct; direct_dev[3k..3k+2], when not NULL, receives ShadeDirect's
 *     value itself.
 *   - Unless opt->flags has RT_PATH_LAST, the bounce of query.h:193-216 with that material: the path
 *     ends on kd + kr <= 0; otherwise rng_next is drawn, then the diffuse (opt->diffuse_bounce and
 *     xi < kd / (kd + kr)) or the mirror ray and throughput, then the 1e-4 cut-off.  alive[k] = 1
 *     exactly when the reference's loop would go on to trace the new ray, which is then
 *     next_rays_dev[k]; a dead entry gets its input ray copied there, so every byte of
 *     next_rays_dev and alive_dev is written.  next_rays_dev may be rays_dev itself.
 *   - RT_PATH_LAST (a path's last depth): no bounce, no draw; next_rays_dev and alive_dev may be
 *     NULL (they are required otherwise), and alive_dev, when given, is written 0 throughout.
 *   Variant rule as for the queries (WIDE; BINARY with RT_FLAG_BINARY; DEEP), 16-byte alignment of
 *   hits_dev as for rt_trace_hits_device.  m == 0 is RT_OK with no launch; m > 2^31-1 is
 *   RT_ERR_UNSUPPORTED; a null scene, rays, hits, opt or state (or state member) is RT_ERR_ARG, and
 *   so is a flag bit other than RT_FLAG_BINARY | RT_PATH_LAST.  Every argument check runs before
 *   any HIP call.  Like a query the step reads only the scene's immutable arrays, takes no part in
 *   the frame ordering and may run on any stream beside frames of the same scene, of a clone or
 *   of an rt_renderer's scene.  It terminates for any bit patterns (per light one DFS that visits
 *   a node at most once; the bounce draws as rt_shade_rays does).
 * rt_path_compact_device: stable compaction.  For the k < m with alive_dev[k] != 0, in increasing
 *   k, rays_in_dev[k] and the id (ids_in_dev ? ids_in_dev[k] : k) go to the next slot of
 *   rays_out_dev / ids_out_dev (room for m entries each), and their number to *count_dev.
 *   scratch_dev: rt_path_compact_scratch_bytes(m) bytes, 4-byte aligned.  The outputs must not
 *   overlap the inputs (RT_ERR_ARG); any m up to 2^31-1 is accepted (above: RT_ERR_UNSUPPORTED);
 *   m == 0 writes count 0 and reads nothing else.  Launches in stream order (tile counts, a scan of
 *   the counts, scatter): no block waits for another.
 * rt_path_finish_device: the reference's clamp (shader.h:24-32) on all 3n radiance floats, once
 *   the paths are done: NaN and -0.0 stay as they are.
 * rt_path_step_host: host build of the step's arithmetic (no device, no traversal), through the
 *   function the kernel runs: host arrays, the scene's material table and lights passed as arrays
 *   (table may be NULL with num_table 0), and occluded[k * num_lights + l], consulted exactly where
 *   the kernel would cast entry k's shadow ray to light l (non-zero: in shadow).  hits needs no
 *   alignment.  Same argument rules; only RT_PATH_LAST of opt->flags has a meaning here.
 * (Additive to ABI 3: the names below.) */
typedef struct { float* radiance; float* throughput; uint32_t* rng; } rt_path_state;
typedef struct {
    int32_t diffuse_bounce;
    rt_vec3 miss_color;
    int32_t flags;            /* RT_FLAG_BINARY | RT_PATH_LAST */
} rt_path_opts;
enum { RT_PATH_LAST = 16 };   /* a bit no RT_FLAG_* uses */
#define RT_PATH_NONE 0xFFFFFFFFu
void rt_path_opts_default(rt_path_opts* o);   /* 1, (0,0,0), 0 */

int rt_path_begin_device(int device, size_t n, const uint32_t* seeds_dev, const rt_path_state* st, void* hip_stream);
int rt_path_step_device(rt_scene* s, size_t m, const rt_ray* rays_dev, const rt_hit* hits_dev,
                        const rt_material* mats_dev, const uint32_t* ids_dev, const rt_path_opts* opt,
                        const rt_path_state* st, rt_ray* next_rays_dev, uint8_t* alive_dev, float* direct_dev,
                        void* hip_stream);
/* RT_RAYS_VARIANT_* of the latest rt_path_step_device call on s (NONE before the first), by
 * rt_trace_rays_variant's rule; a word of its own. */
int rt_path_step_variant(const rt_scene* s);
int rt_path_step_host(size_t m, const rt_ray* rays, const rt_hit* hits, const rt_material* mats, const uint32_t* ids,
                      const rt_material* table, int num_table, const rt_light* lights, int num_lights,
                      const uint8_t* occluded, const rt_path_opts* opt, const rt_path_state* st, rt_ray* next_rays,
                      uint8_t* alive, float* direct);
size_t rt_path_compact_scratch_bytes(size_t m);
int rt_path_compact_device(int device, size_t m, const uint8_t* alive_dev, const rt_ray* rays_in_dev,
                           const uint32_t* ids_in_dev, rt_ray* rays_out_dev, uint32_t* ids_out_dev,
                           uint32_t* count_dev, void* scratch_dev, void* hip_stream);
int rt_path_finish_device(int device, size_t n, float* radiance_dev, void* hip_stream);

/* ---- soft shadows: spherical area lights for the staged path ------------------------------------
 * The reference's other HW2 fork, C/ (HW2/HW2/CPUOnly), gives a light a `radius` and a number of
 * `shadow_samples`: its ShadowVisibility (C/include/raytracer.h:121-168) samples a disk at the
 * light that faces the shaded point, and ShadeDirect multiplies the light's term by the unoccluded
 * fraction (:195-207).  Here that is two stages of the staged path,
 *   trace_hits -> rt_light_visibility_device -> rt_path_step_vis_device -> compact,
 * defined as G/'s ShadeDirect with C/'s ShadowVisibility in place of IsInShadow: random_float() is
 * rng_next(state) on the path's own state, the occlusion decision and RT_EPS (shader.h:22, 1e-3)
 * stay G/'s.  Float32, no contraction; dot, unit, divf (v / s per component) and cross are the
 * reference's operators, as in the step.
 *
 * rt_light_shape: one per scene light, in the lights' order.
 *
 * rt_light_visibility_device, for entry k < m with path id = ids_dev ? ids_dev[k] : k, when
 * id != RT_PATH_NONE and hits[k].tri >= 0: p and n come from the record, N = unit(n),
 * state = rng_dev[id], and each light l in index order is processed by steps 1 to 5:
 *   1. toC = lpos - p, L = unit(toC), NdotL = fmaxf(dot(N, L), 0) (the step's own expressions).
 *      NdotL <= 0: vis[k][l] = 0, nothing is drawn, next light.
 *   2. distC = sqrtf(dot(toC, toC)).  !(distC > 0): vis = 1, nothing is drawn, next light (the
 *      step casts no ray there and lights the point).
 *   3. soft = shapes[l].radius > 0 (NaN and negative radii are point lights);
 *      S = soft ? max(shadow_samples, 1) : 1.
 *   4. Not soft: IsInShadow's one ray, origin p + N * RT_EPS, direction toC / distC, occluded iff the
 *      any-hit traversal finds t < distC.  vis is 0 or 1; nothing is drawn.
 *   5. Soft: W = (p - lpos) / distC, a = fabsf(W.x) > 0.9f ? (0,1,0) : (1,0,0), T = unit(cross(a, W)),
 *      B = cross(W, T).  For i = 0 .. S-1: repeat x = 2 * rng_next(state) - 1, y = 2 * rng_next(state) - 1,
 *      r2 = x*x + y*y until r2 > 1e-10f && r2 <= 1; lp = (lpos + T * (x * radius)) + B * (y * radius),
 *      toL = lp - p, d = sqrtf(dot(toL, toL)); !(d > 0): the sample counts as unoccluded; otherwise
 *      the ray from p + N * RT_EPS along toL / d with bound d, decided as in step 4.  Every sample is
 *      cast (the count is the answer: no early out).  vis = float(unoccluded) / float(S).
 *   After the last light rng_dev[id] = state: within a depth the lights' disk samples are drawn
 *   first, then the bounce's xi (C/'s order).
 *   An entry with tri < 0 or id RT_PATH_NONE gets a row of zeros, and no state word of it is read
 *   or written.  vis_dev holds m * rt_scene_num_lights(s) floats, every one written.
 *   shapes_dev: rt_scene_num_lights(s) records; they are copied back once per call (the call waits
 *   for hip_stream up to that copy): a shadow_samples above RT_LIGHT_MAX_SHADOW_SAMPLES is
 *   RT_ERR_UNSUPPORTED with no launch, and the largest S picks the lane mapping when lanes_per_entry
 *   is 0.  lanes_per_entry: 0, or one of the built group sizes 1, 8, 32 (G lanes of a wave share an
 *   entry and split each light's samples; the results do not depend on it); anything else is
 *   RT_ERR_ARG.  flags: RT_FLAG_BINARY or 0; variant rule as for the queries, with a word of its
 *   own (rt_light_visibility_variant).  hits_dev 16-byte aligned.  m == 0 or a scene without lights
 *   is RT_OK with no launch; m > 2^31-1 is RT_ERR_UNSUPPORTED; every argument check runs before any
 *   HIP call.  Ids unique and inside the state, as for the step.  The walk terminates for any bit
 *   patterns (the LCG has full period, so the rejection loop ends; at most 256 * num_lights
 *   traversals, each visiting a node at most once).  Results are specified for finite inputs.
 *
 * rt_path_step_vis_device: rt_path_step_device with one difference per light.  After the
 *   NdotL > 0 test, v = vis_dev[k * num_lights + l]: !(v > 0) skips the light, otherwise
 *   Lo += (radiance * f) * (NdotL * v) (C/'s form), which is the step's Lo += (radiance * f) * NdotL
 *   bit for bit when v == 1.  With every shape a point light the two stages are therefore
 *   rt_path_step_device, rt_shade_rays and the reference, bit for bit.  RT_PATH_NONE, RT_PATH_LAST,
 *   mats_dev, direct_dev, the copy-through of dead entries and the argument rules are the step's; it
 *   casts no ray (no variant; RT_FLAG_BINARY is accepted and has no meaning).
 *
 * rt_light_samples_host: the host build of everything of the visibility stage but the traversals,
 *   through the functions the kernel runs.  For entry k and light l, rays[offsets[k * num_lights + l]
 *   .. offsets[k * num_lights + l + 1]) are the shadow rays in cast order (a sample with !(d > 0)
 *   casts none) and bounds[] their bounds; offsets holds m * num_lights + 1 words.  rays == NULL
 *   writes the offsets alone and leaves rng as it is; otherwise cap is the room in rays and bounds
 *   (too little: RT_ERR_ARG, nothing written but offsets) and rng is advanced as the stage does.
 * rt_path_step_vis_host: rt_path_step_host with vis (floats) where that takes occluded (bytes).
 * rt_host_scene_light_shapes: the shapes rt_host_scene_load_json read, one per light of
 *   rt_scene_arrays::lights (optional keys "radius" and "shadow_samples" of a light; 0 and 1 when
 *   absent; a key of another type than a number is RT_ERR_PARSE); cap: the room in out.
 * (Additive to ABI 3: the names below.) */
typedef struct { float radius; int32_t shadow_samples; } rt_light_shape;
#define RT_LIGHT_MAX_SHADOW_SAMPLES 256
int rt_scene_num_lights(const rt_scene* s);
int rt_light_visibility_device(rt_scene* s, size_t m, const rt_hit* hits_dev, const uint32_t* ids_dev,
                               const rt_light_shape* shapes_dev, uint32_t* rng_dev, int lanes_per_entry, int flags,
                               float* vis_dev, void* hip_stream);
int rt_light_visibility_variant(const rt_scene* s);
int rt_path_step_vis_device(rt_scene* s, size_t m, const rt_ray* rays_dev, const rt_hit* hits_dev,
                            const rt_material* mats_dev, const uint32_t* ids_dev, const float* vis_dev,
                            const rt_path_opts* opt, const rt_path_state* st, rt_ray* next_rays_dev, uint8_t* alive_dev,
                            float* direct_dev, void* hip_stream);
int rt_light_samples_host(size_t m, const rt_hit* hits, const uint32_t* ids, const rt_light* lights,
                          const rt_light_shape* shapes, int num_lights, uint32_t* rng, size_t cap, rt_ray* rays,
                          float* bounds, uint64_t* offsets);
int rt_path_step_vis_host(size_t m, const rt_ray* rays, const rt_hit* hits, const rt_material* mats, const uint32_t* ids,
                          const rt_material* table, int num_table, const rt_light* lights, int num_lights,
                          const float* vis, const rt_path_opts* opt, const rt_path_state* st, rt_ray* next_rays,
                          uint8_t* alive, float* direct);
int rt_host_scene_light_shapes(const rt_host_scene* s, rt_light_shape* out, int cap);

/* ---- adaptive sampling: per-pixel sample counts, pixel-list rays and film ----------------------
 * Spending samples unevenly, exactly.  jittered_samples(k, 42) is a prefix of
 * jittered_samples(n, 42) for k <= n (one mt19937 stream), make_rng_seed(x, y, s) does not read
 * spp, and render() sums in sample order and divides by float(spp): a pixel that has received
 * samples 0..c-1 in order and is resolved with its own count c is render()'s pixel at spp = c, bit
 * for bit.  A pass is  select -> rt_camera_rays_pixels_device -> rt_shade_rays_device (or the path
 * stages) -> rt_afilm_add_device,  all on the device; the only thing a host needs per pass is the
 * number of selected pixels.
 * Conventions as for rt_film_* and rt_path_*: device pointers on the object's device, one or a
 * few launches per call on the caller's hip_stream (NULL = the null stream), asynchronous, no host
 * synchronisation, every argument check before any HIP call, no block waits for another, one
 * writer per word (plain stores, no atomics).  Results are specified for finite radiance.
 *
 * rt_camera_rays_pixels_*: camera rays for a list of pixels.  pixels: m indices y * W + x in any
 *   order; NULL means entry k is pixel k, and m must then be W * H.  counts: W * H words, the
 *   samples each pixel already has (rt_afilm_counts_device); NULL means 0 for all.  Ray
 *   k * nsamples + s is sample counts[pixels[k]] + s of that pixel: Camera::get_ray with that
 *   entry of jitter (the whole frame's table, table_spp entries of (jx, jy); on the host NULL
 *   means rt_jittered_samples(table_spp, 42, 1)), the arithmetic of rt_camera_rays_pass_*; its seed
 *   is make_rng_seed(x, y, counts + s); seeds may be NULL.  Memory-safe for any input: an index
 *   >= W * H (RT_PIXEL_NONE is the marker) writes origin = center, direction 0 and seed 0; a sample
 *   index >= table_spp reads the table's last entry and its result is unspecified.
 *   m * nsamples > 2^31-1 (or W * H > 2^31-1) is RT_ERR_UNSUPPORTED; m == 0 is RT_OK with no launch;
 *   a null camera, rays or (on the device) jitter, nsamples < 1 or table_spp < 1 is RT_ERR_ARG.
 *
 * rt_afilm: per pixel three float sums (rt_film's), a uint32 sample count and two float moments of
 *   the sample luminance y = (0.2126f * r + 0.7152f * g) + 0.0722f * b (float multiplies and adds in
 *   that order): m1 = sum of y, m2 = sum of y * y, accumulated in sample order like the sums.
 *   24 bytes per pixel, all on the device: there are no host-side counts.
 * rt_afilm_add_device: radiance_dev holds m * nsamples * 3 floats in the ray generator's order; for
 *   entry k the samples go onto pixel pixels_dev[k]'s sums and moments in order and its count
 *   grows by nsamples.  pixels_dev NULL: the dense add, m == W * H.  Indices must be unique within
 *   a call (the caller's to keep); an index >= W * H is skipped.  Any alignment of radiance_dev; a
 *   16-byte aligned pointer takes the faster kernel.  m * nsamples > 2^31-1 is RT_ERR_UNSUPPORTED,
 *   m == 0 is RT_OK with no launch.
 * rt_afilm_resolve_device: for rows [row0, row0 + rows): rgb_dev (rows*W*3 floats), each pixel
 *   float(double(sum) / double(float(count))) with its own count; p6_dev (rows*W*3 bytes, write_p6's
 *   defaults as rt_film_resolve_device writes them); counts_out_dev (rows*W words), the sample-count
 *   map.  Any two of the three may be NULL.  A pixel with count 0 resolves to 0.0f, byte 0.  Does
 *   not clear.
 * rt_afilm_select_device: the indices of the pixels to sample next, in increasing order (a stable
 *   compaction: per-tile counts, a scan, a scatter, in stream order), to pixels_out_dev (room for
 *   W * H words) and their number to *count_dev.  scratch_dev: rt_afilm_select_scratch_bytes(f)
 *   bytes, 4-byte aligned.  opts: min_samples >= 2, step >= 1, tol >= 0, floor > 0, else RT_ERR_ARG.
 *   A pixel with count n is selected iff n + step <= max_samples and (n < min_samples or noisy(n)).
 *   noisy is computed in double from the float accumulators with + - * /, max and comparisons only:
 *     mean = m1 / n;  var = (max(0, m2 / n - mean * mean) * n) / (n - 1);
 *     noisy iff var / n > (tol * max(mean, floor))^2;  n < 2 counts as noisy.
 * rt_afilm_host: the host build of add, resolve and select over host arrays (no device needed),
 *   through the functions the kernels run.  sum (W*H*3), count (W*H) and moments (W*H*2) are the
 *   film's state, updated in place.  In this order: when radiance is not NULL, the add of m entries
 *   (pixels NULL: dense); when rgb_out or p6_out is not NULL, the resolve of the whole image; when
 *   opts is not NULL, the selection to pixels_out (W*H words) and *selected_out.  Same argument
 *   rules. */
#define RT_PIXEL_NONE 0xFFFFFFFFu
int rt_camera_rays_pixels_host(const rt_camera* cam, const uint32_t* pixels, size_t m, const uint32_t* counts,
                               int nsamples, const float* jitter, int table_spp, rt_ray* rays, uint32_t* seeds);
int rt_camera_rays_pixels_device(const rt_camera* cam, const uint32_t* pixels_dev, size_t m, const uint32_t* counts_dev,
                                 int nsamples, const float* jitter_dev, int table_spp, rt_ray* rays_dev,
                                 uint32_t* seeds_dev, int device, void* hip_stream);

typedef struct rt_afilm rt_afilm;
typedef struct {
    int32_t min_samples;      /* >= 2: below it a pixel is always selected */
    int32_t max_samples;      /* no pixel goes beyond it */
    int32_t step;             /* >= 1: the samples a selected pixel is about to get */
    double tol;               /* >= 0: relative standard error of the mean to reach */
    double floor;             /* > 0: the mean below which the error is absolute */
} rt_afilm_select_opts;
/* A width x height film on `device`, zeroed (synchronous). */
int rt_afilm_create(int device, int width, int height, rt_afilm** out);
void rt_afilm_destroy(rt_afilm* f);
/* Sums, counts and moments to 0. */
int rt_afilm_clear_device(rt_afilm* f, void* hip_stream);
/* The device pointer to the W * H counts (NULL for a null film), valid while the film lives. */
const uint32_t* rt_afilm_counts_device(const rt_afilm* f);
int rt_afilm_add_device(rt_afilm* f, const uint32_t* pixels_dev, size_t m, const float* radiance_dev, int nsamples,
                        void* hip_stream);
int rt_afilm_resolve_device(rt_afilm* f, int row0, int rows, float* rgb_dev, uint8_t* p6_dev, uint32_t* counts_out_dev,
                            void* hip_stream);
size_t rt_afilm_select_scratch_bytes(const rt_afilm* f);
int rt_afilm_select_device(rt_afilm* f, const rt_afilm_select_opts* opts, uint32_t* pixels_out_dev, uint32_t* count_dev,
                           void* scratch_dev, void* hip_stream);
int rt_afilm_host(int width, int height, float* sum, uint32_t* count, float* moments, const uint32_t* pixels, size_t m,
                  const float* radiance, int nsamples, float* rgb_out, uint8_t* p6_out, const rt_afilm_select_opts* opts,
                  uint32_t* pixels_out, uint32_t* selected_out);

/* ---- sorting caller rays for coherence: keys, order, gather / scatter ---------------------------
 * The caller-ray entry points run one ray per lane, and a wave costs what its longest lane costs;
 * these calls put a batch into an order in which neighbouring lanes start in neighbouring cells of
 * a box.  A ray's answer does not depend on its lane, so a query on the sorted
 * batch, scattered back, is the query on the batch, bit for bit.  No call reads a scene: all may
 * run on any stream beside frames and queries.  Device pointers are on `device`, device calls are
 * asynchronous on hip_stream (NULL = the null stream), every argument check runs before any HIP
 * call; n == 0 is RT_OK with no launch (whatever the pointers), n > 2^31-1 is RT_ERR_UNSUPPORTED,
 * a null argument or a bad mode / bits / elem_bytes is RT_ERR_ARG.
 *
 * The key of a ray in a box (lo, hi), with b = bits, all in float, one IEEE operation per
 * operator in the order written, no contraction:
 *   cell(x, lo, hi):  t = ((x - lo) / (hi - lo)) * 2^b;  q = t >= 0 ? t : 0  (NaN gives 0);
 *                     q = q <= 2^b - 1 ? q : 2^b - 1;  the cell is (uint32_t)q.
 *                     A flat axis gives 0 / 0 -> 0 and x / 0 -> the last cell (the first for x < lo).
 *   RT_SORT_ORIGIN, b in 1..10: the cells of origin.x, .y, .z; 3b bits.
 *   RT_SORT_ORIGIN_DIR, b in 1..5: those three, then for the direction d
 *                     len = sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z),  u = d / len per component,
 *                     t = ((u + 1.0f) * 0.5f) * 2^b, clamped as above (a zero or non-finite
 *                     direction is defined: cell 0); 6b bits.
 *   From the cells' most significant bit down, that bit of each cell in the order listed is
 *   appended to the key (x leads, as in the LBVH's Morton code).
 * rt_scene_bounds: the root box the scene holds now (after a refit or rebuild, the new one).
 * rt_ray_key_bits: 3b or 6b; RT_ERR_ARG for a mode or bits outside the table.
 * rt_ray_keys_host / rt_ray_keys_device: keys[i] of rays[i]; box is a host pointer in both.
 * rt_ray_sort_host / rt_ray_sort_device: order = the stable sort of 0..n-1 by key (equal keys keep
 *   increasing index, so the order is unique); on the device a stable radix sort over exactly
 *   rt_ray_key_bits bits.  rays_out_dev, when not NULL, receives rays_out[k] = rays[order[k]]; it
 *   must not overlap rays_dev.  scratch_dev: rt_ray_sort_scratch_bytes(n, mode, bits) bytes, any
 *   alignment (0 for n == 0, n > 2^31-1 or a bad mode / bits).
 * rt_gather_device: out[k] = in[order[k]];  rt_scatter_device: out[order[k]] = in[k], for n
 *   elements of elem_bytes each, a multiple of 4 in 4..64 (indices, t, seeds, max_t, ids: 4;
 *   radiance: 12; rt_ray: 24; rt_material: 52; rt_hit: 64).  Pointers 4-byte aligned; 16-byte (or
 *   8-byte) accesses are used when elem_bytes and both addresses allow.  in and out must not
 *   overlap.  order must be a permutation of 0..n-1, the caller's to keep (as path ids are); an
 *   entry >= n is skipped, so the calls stay inside their arrays for any order.
 * (Additive to ABI 3: the names below.) */
enum { RT_SORT_ORIGIN = 0, RT_SORT_ORIGIN_DIR = 1 };
int rt_scene_bounds(const rt_scene* s, rt_aabb* out);
int rt_ray_key_bits(int mode, int bits);
int rt_ray_keys_host(const rt_ray* rays, size_t n, int mode, int bits, const rt_aabb* box, uint32_t* keys);
int rt_ray_keys_device(int device, const rt_ray* rays_dev, size_t n, int mode, int bits, const rt_aabb* box,
                       uint32_t* keys_dev, void* hip_stream);
int rt_ray_sort_host(const rt_ray* rays, size_t n, int mode, int bits, const rt_aabb* box, uint32_t* order);
size_t rt_ray_sort_scratch_bytes(size_t n, int mode, int bits);
int rt_ray_sort_device(int device, const rt_ray* rays_dev, size_t n, int mode, int bits, const rt_aabb* box,
                       uint32_t* order_dev, rt_ray* rays_out_dev, void* scratch_dev, void* hip_stream);
int rt_gather_device(int device, const void* in_dev, size_t n, size_t elem_bytes, const uint32_t* order_dev,
                     void* out_dev, void* hip_stream);
int rt_scatter_device(int device, const void* in_dev, size_t n, size_t elem_bytes, const uint32_t* order_dev,
                      void* out_dev, void* hip_stream);

/* The Blinn-Phong powf of the kernels (restatement of the reference libm's powf, see
 * csrc/rt_math.hpp): rt_powf_host evaluates the host build, rt_powf_batch the device build
 * over n (x, y) pairs.  Exposed so both can be pinned against the C library's powf. */
float rt_powf_host(float x, float y);
int rt_powf_batch(int device, const float* x, const float* y, int n, float* out);

/* The greedy record rules' weight of a box (csrc/rt_records.hpp box_weight: half surface area in
 * double, rule 2 times sqrt(leaves), 1e300 when not finite) for n boxes (min corner, max corner)
 * and leaf counts: the host build, and the device build (rules 1 and 2), which a record builder on
 * the device would have to match bit for bit — the host's sqrt is correctly rounded. */
int rt_debug_box_weight_host(const float* boxes, const uint32_t* leaves, int rule, int n, double* out);
int rt_debug_box_weight_batch(int device, const float* boxes, const uint32_t* leaves, int rule, int n, double* out);

/* Host build of the kernels' AABB test for n (ray, box, [tmin,tmax]) triples: out_exact =
 * the reference's double slab test (bvh.h:81-129), out_fast = the float-pre-classified test
 * the kernels run (must equal out_exact), out_class = 0 miss / 1 hit / 2 ambiguous (decided
 * in double).  rays: n*6 floats (orig, dir), boxes: n*6 (min, max), tminmax: n*2. */
int rt_box_test_host(const float* rays, const float* boxes, const float* tminmax, int n,
                     int32_t* out_fast, int32_t* out_exact, int32_t* out_class);

/* The device build of the same tests (v_rcp_f32 reciprocals, packed FMAs, the wave forms with
 * their ballots), item i in lane i % 64 of a 256-thread block over 256 consecutive items, the
 * ray prepared by make_ray as the render kernels prepare it.  bmax: NULL for the per-item bounds
 * rt_box_test_host derives (inf for an inverted or NaN box), else n*3 floats, the caller's
 * per-axis bounds of |coordinate| (at least the box's own; larger ones model a scene's).
 * active: NULL for all items, else n bytes; the wave forms run for the lanes with a nonzero byte
 * and i < n (every lane of a wave calls them).  out: n*5 ints per item: [0] box_hit, [1]
 * box_classify (0 miss / 1 hit / 2 ambiguous), [2] [3] [4] the lane's bit of box_hit_mask<PK, XL>
 * for (PK, XL) = (0, 0), (1, 0), (1, 1), the forms the traversals instantiate, 0 for a lane
 * outside `active`.  [0] and [1] take tmin from tminmax; the wave forms' tmin is the traversals'
 * constant 1e-4f. */
int rt_box_test_batch(int device, const float* rays, const float* boxes, const float* tminmax,
                      const float* bmax, const uint8_t* active, int n, int32_t* out);

/* The group-wide box tests, item by item: the functions the kernels call (one definition each,
 * host and device builds of the same text), so a fuzz can hold them against the rays themselves.
 *
 * The tile test of the cull and cut pre-passes (csrc/rt_prepass.hpp tile_dirs_f,
 * tile_misses_box_f).  Item i: the pixel rectangle tiles[4i..] = (x0, x1, y0, y1), columns x0..x1
 * and rows y0..y1 inclusive, of cam's image, and the box boxes[6i..] = (min, max).  out[i] = 1
 * when the test says every camera ray of the rectangle, for any jitter with |entry| <= 1,
 * misses the box.  As in a frame, the test runs only for a camera whose range of |D| is proven
 * (rt_debug_camera_class 0); for any other camera every out[i] is 0.
 *
 * rt_debug_camera_class: what a frame does with this camera and a jitter table whose largest
 * |entry| is pad (at least 1).  *out = 0: every |pixel00 + px du + py dv - center| over the padded
 * frame is proven inside [2e-12, 9e18] (the cull and cut run, any kernel); 1: finite rays, some of
 * which may take Camera::get_ray's 1e-12 fallback (no cull, no cut); 2: a non-finite word, or a
 * length that may overflow (the lane kernel, no cull). */
int rt_debug_camera_class(const rt_camera* cam, float pad, int32_t* out);
int rt_debug_tile_test_host(const rt_camera* cam, const int32_t* tiles, const float* boxes, int n, int32_t* out);
int rt_debug_tile_test_batch(int device, const rt_camera* cam, const int32_t* tiles, const float* boxes, int n,
                             int32_t* out);

/* The wave-family entry test of the camera rays' frustum traversal (csrc/rt_traverse.hpp
 * family_axis, family_entry_passes: what family_dirs and frustum_loop call; float records, not
 * the quantised ones).  Wave w: 64 rays rays[384w..] (orig, dir; one origin, lane 0's, and
 * directions as the kernels hold them), active[64w..] bytes (NULL: all live; a wave needs a live
 * lane), best_t[64w..] the lanes' bestT, bmax[3w..] the scene's per-axis bound of |coordinate|,
 * and 32 boxes boxes[192w..] (min, max), entry k tested as lane k tests it.  out[32w + k] = 1
 * when entry k passes with tmax_w = the largest bestT over the live lanes; out_loose[w] = 1 when
 * the wave has a loose axis (the LOOSE loop form).  The batch form runs one wave per item. */
int rt_debug_family_test_host(const float* rays, const uint8_t* active, const float* best_t, const float* bmax,
                              const float* boxes, int n_waves, int32_t* out, int32_t* out_loose);
int rt_debug_family_test_batch(int device, const float* rays, const uint8_t* active, const float* best_t,
                               const float* bmax, const float* boxes, int n_waves, int32_t* out, int32_t* out_loose);

/* Host build of the camera rays' frustum records rt_scene_create makes (no device): for a BVH
 * of P triangles (the same arrays as rt_scene_create), the records of arity 2^info[0]
 * (8 x 2^info[0] floats each: per entry the (min, max) pairs of x, y, z, then the entries'
 * refs), info = {log2 arity (2: none fits), DFS stack bound, records}: the largest arity up to
 * 2^max_log2 whose DFS needs at most stack_cap entries (64; 128 for the big-scene kernels).
 * rec is written when rec_cap (floats) suffices; call with a null rec to size it.
 * DESIGN.md §4.12. */
int rt_debug_frustum_records(size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs, int max_log2, int stack_cap,
                             int64_t* info, float* rec, size_t rec_cap);

/* Host half of rt_scene_create (no device): the arrays it would upload for this BVH, digested.
 * info = {P, root ref, cut boxes, log2 sub-boxes per cut box, wide, lane_stack, lane_wide, deep,
 * frustum log2 arity, frustum stack bound, binary DFS stack bound, 4-ary DFS stack bound, then
 * the float bit patterns of the root box (min, max corner) and of bmax}; digests = per array
 * (inode, wnode, fnode, qent, qhdr, ibox, leaf, tnorm, cut, cut2, tri) its byte length and the
 * 64-bit FNV-1a hash of its bytes.  Errors as rt_scene_create reports them for these arrays. */
int rt_debug_scene_pack(size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs, const rt_triangle* tris,
                        int64_t info[21], uint64_t digests[22]);
/* The same words for a resident scene: its arrays read back from the device and hashed (waits for
 * the device). */
int rt_debug_scene_digest(rt_scene* s, int64_t info[21], uint64_t digests[22]);
/* rt_debug_scene_pack of (nodes, aabbs, tris), then the host restatement of rt_scene_refit with
 * new_tris (no device): what rt_debug_scene_digest answers after rt_scene_create_refittable and
 * that refit.  Errors as those two calls report them. */
int rt_debug_scene_refit_pack(size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs, const rt_triangle* tris,
                              const rt_triangle* new_tris, int64_t info[21], uint64_t digests[22]);
/* ... with n refits in turn: poses[0], then poses[1], ... (P triangles each). */
int rt_debug_scene_refit_chain(size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs, const rt_triangle* tris,
                               int n, const rt_triangle* const* poses, int64_t info[21], uint64_t digests[22]);
/* The variant rule of the caller queries (rt_trace_rays_variant and the other rt_*_variant), on
 * the facts of a scene it reads (rt_debug_scene_pack's info[4..7]) and a call's flags (no device):
 * RT_RAYS_VARIANT_DEEP when deep; else WIDE when wide and lane_wide without RT_FLAG_BINARY; else
 * BINARY when lane_stack; else DEEP. */
int rt_debug_query_variant(int wide, int lane_stack, int lane_wide, int deep, int flags);

/* Durations (ms) of the render kernel of the most recent min(max, launches, 256) timed
 * rt_render_device calls on this scene, oldest first, measured with HIP events recorded
 * on the launch stream around the kernel (direct calls are all timed; an rt_renderer's frames
 * one in RT_TUNE_KERNEL_TIMING_EVERY, *n_out then counts the timed ones).  Waits for those
 * launches to finish. */
int rt_kernel_times(const rt_scene* s, float* ms_out, int max, int* n_out);
/* The same for the whole device frame: the root-box cull pass and the tree-cut cull pass (when
 * it runs), timed on the scene's prep stream, plus the render kernel.  (A frame's pre-passes
 * overlap the previous frame's render kernel, so this is the frame's device work, not the
 * span from its first launch to its end.)  An rt_renderer's frames on the frame streams
 * (RT_TUNE_FRAME_STREAMS) carry the pre-passes' events on the frames whose render kernel is timed,
 * so this and rt_prepass_times report over those frames, as rt_kernel_times does. */
int rt_frame_times(const rt_scene* s, float* ms_out, int max, int* n_out);
/* The pre-passes alone (root-box cull + tree-cut cull). */
int rt_prepass_times(const rt_scene* s, float* ms_out, int max, int* n_out);
/* Pixel tiles of the most recent rt_render_device call that survived the root-box cull, and
 * all tiles (the tree-cut pass may still cull some of the survivors; those are flagged, not
 * removed from the lists).  Waits for that call to finish. */
int rt_live_tiles(const rt_scene* s, int64_t* live, int64_t* total);
/* Tiles of the most recent rt_render_device call that its render kernel took first (heavy-first
 * dispatch: tiles whose waves took >= 1/4 of the previous finished frame's render kernel in the
 * last frame that rendered them; their order only, never their pixels).  Waits for that call. */
int rt_heavy_tiles(const rt_scene* s, int64_t* heavy);
/* The render kernel instantiation the most recent rt_render_device call launched, as rocprofv3
 * names it ("render_tiles_kernel<49, true, true, 7, 0>"; "" before the first frame): bench.py
 * keys its measured per-launch HBM traffic by it. */
const char* rt_scene_kernel_name(const rt_scene* s);

/* Traversal setup rt_scene_create chose for s: info = {log2 of the camera rays' frustum-record
 * arity (3..5; 2 = the 4-ary records; 0 = no frustum traversal), their DFS stack bound
 * (<= 128 unless RT_TUNE_FRUSTUM_STACK_CAP raised it), 1 if the 4-ary records exist, 1 if the
 * scene takes the deep (512-entry stack) kernels}. */
int rt_scene_traversal_info(const rt_scene* s, int64_t info[4]);
/* Device-side fault flags of s, OR-ed by the kernels since the last clear (waits for the
 * scene's work): bit 0 = a camera-ray frustum traversal needed more than its 128 stack
 * entries (the host bound makes this impossible for records built with the default cap; the
 * wave's answers were poisoned: no hit).  clear != 0 resets the flags.  rt_render
 * returns RT_ERR_INTERNAL when its frame raised one (it clears the flags when the frame starts). */
int rt_scene_faults(rt_scene* s, uint32_t* flags, int clear);

/* ---- Tuning knobs (process-wide; read when a scene is created or a frame is set up) ----
 * The library reads no environment variables: every setting that selects among exact kernel
 * variants or schedules is set here, by tests and A/B scripts.  Frames are identical under
 * every value (order of work only), except RT_TUNE_FRUSTUM_STACK_CAP, a test hook. */
typedef enum {
    RT_TUNE_FRUSTUM_ARITY = 0,   /* log2 of the largest frustum-record arity to build, 2..5 (5) */
    RT_TUNE_HALF_WAVES = 1,      /* -1 auto (default: from 4 band shards, and multi-bounce), 0, 1 */
    RT_TUNE_PAIRED_ONLY = 2,     /* 1 (default): one-light bounce frames take the paired-only kernels */
    RT_TUNE_HEAVY_FRAC = 3,      /* heavy-first class threshold, fraction of a frame (0.10; 0 = off) */
    RT_TUNE_HEAVY_CAP = 4,       /* heavy-list entries per (class, list) (512) */
    RT_TUNE_CULL_COVERAGE = 5,   /* the cut pass runs when the root box covers <= this (0.3; >= 1: always) */
    RT_TUNE_CULL_BOXES = 6,      /* boxes of the tile-culling cut (64; at scene creation) */
    RT_TUNE_BIG_SCENE_BYTES = 7, /* scenes above this take the 8-wave depth-1 kernel (64 MiB) */
    RT_TUNE_FRUSTUM_STACK_CAP = 8, /* TEST HOOK: stack bound the frustum records may need (128) */
    RT_TUNE_PEER_TIMEOUT_S = 9,  /* rt_renderer: seconds to wait for a peer rank (120) */
    RT_TUNE_RENDERER_THREADS = 10, /* rt_renderer: -1 auto (default: a thread per further distinct
                                      GPU), 0 submit every rank from the caller, 1 threads always */
    RT_TUNE_COPY_ENGINE = 11,    /* rt_renderer's host delivery: -1 auto (SDMA where it applies: one rank,
                                    DIRECT, a host frame), 0 the HIP runtime's copies, 1 SDMA or fail */
    RT_TUNE_QUANT_RECORDS = 12,  /* quantised frustum records for the big-scene kernels, at scene creation:
                                    0 never (default; measured slower on c5), -1 scenes whose float
                                    records exceed 1/8 of RT_TUNE_BIG_SCENE_BYTES, 1 always */
    RT_TUNE_PREPASS_GATE = 13,   /* f in (0, 1]: a frame's render kernel opens the next frame's cull/cut
                                    pre-passes when its first work queue has handed out the fraction
                                    f of its items (0.5 default; 1: drained, they then fill its
                                    tail); 0: they start when the frame before it has finished.
                                    Off while RT_TUNE_OVERLAP_FRAMES is on without RT_TUNE_FRAME_STREAMS */
    RT_TUNE_OVERLAP_FRAMES = 14, /* rt_renderer frames: 1 lets a frame's render kernel start while the previous
                                    one's tail still runs (two render streams per scene); 0 (default).
                                    Frames on the frame streams (RT_TUNE_FRAME_STREAMS) overlap anyway */
    RT_TUNE_KERNEL_TIMING_EVERY = 15, /* rt_renderer frames: the render kernel's start event (kernel times) in one
                                    frame of this many (4; 16 on the frame streams, RT_TUNE_FRAME_STREAMS,
                                    where the pre-passes' events ride on the same frames); an event
                                    before every kernel held each dispatch ~5 us */
    RT_TUNE_RECORD_GREEDY = 16,  /* frustum records grown by expanding the entry of largest weight: 2
                                    (default) surface area x sqrt(leaves below), 1 surface area;
                                    0: every path to the same depth; at scene creation */
    RT_TUNE_WIDE4_GREEDY = 17,   /* the 4-ary records (shadow and bounce rays) grown by expanding the
                                    largest-area entry (1, default; 2: x sqrt(leaves below)) instead
                                    of the grandchildren (0); at scene creation */
    RT_TUNE_PAIR_FRAMES = 18,    /* rt_render_device_pair / rt_renderer_submit_pair: 1 (default) renders the
                                    two frames in one launch of the render kernel where it is
                                    instantiated for them (depth-1 sample kernels of the wave
                                    traversal and the paired-only bounce kernels, scene within
                                    RT_TUNE_BIG_SCENE_BYTES); 0 two launches */
    RT_TUNE_PAIR_RESERVE = 19,   /* pair kernels: block slots per CU left free for the next pair's pre-passes
                                    (default 1 for depth-1 frames, 0 for the bounce kernels'
                                    pairs; fractions: that many per CU on average) */
    RT_TUNE_CUT_SUB = 20,        /* sub-boxes per box of the tile-culling cut, tested for the tiles whose rays
                                    may reach that box (16; a power of two <= 64; < 2: one level);
                                    at scene creation */
    RT_TUNE_HW1_LANES = 21,      /* rt_render_hw1_deliver: frames alternate over this many lanes (binning
                                    buffers + a stream each, 1..8; default 2): a lane
                                    overlaps the others only on a hardware queue of its own (HIP:
                                    GPU_MAX_HW_QUEUES per process, 4 by default) */
    RT_TUNE_COPY_WAIT = 22,      /* the SDMA copier threads (rt_renderer's and rt_hw1_scene's deliveries): 1 waits
                                    for a frame with hipEventSynchronize, 0 polls hipEventQuery spinning,
                                    2..1000 polls every that many microseconds; default -1: the renderer
                                    spins, the HW1 scene waits; at the copier's creation */
    RT_TUNE_HW1_FUSE = 23,       /* the HW1 scene's frames: bit 0 the scan fused into the count pass (its last
                                    block, up to 5,120 tiles), bit 1 the resolve fused into the render pass
                                    (each tile's last item); default 2 */
    RT_TUNE_HW1_CHUNK = 24,      /* the HW1 scene's render work items: list entries per item, 16..256, a power of two
                                    (32) */
    RT_TUNE_FRAME_STREAMS = 25,  /* rt_renderer's single frames of an unsharded image: 1 (default) puts a frame's
                                    gate wait, cull, cut and render kernel on one of two streams of
                                    the scene, alternating by frame, so the three launches follow
                                    each other on one hardware queue with no event between them
                                    (the pre-passes' events then ride on the timed frames only, and
                                    the gate has a word per stream); 0 the pre-passes on the scene's
                                    prep stream and the render kernel on the caller's */
    RT_TUNE_COUNT = 26
} rt_tune_id;
/* Set knob id (NaN restores the default).  RT_ERR_ARG for an unknown id. */
int rt_tuning_set(int id, double value);
/* The value set for id, or NaN when it has its default. */
int rt_tuning_get(int id, double* value);
void rt_tuning_reset(void);

int rt_device_count(int* n);
const char* rt_last_error(void);
int rt_abi_version(void);
/* sha256 (hex) of the csrc/ and include/ sources and compile flags this library was built from
 * (raytracinginonesemester_amd/build.py: source_build_id), so a caller can prove which sources
 * the loaded binary came from. */
const char* rt_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_MI355X_H */
