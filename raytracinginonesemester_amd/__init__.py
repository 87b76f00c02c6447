"""MI355X-native per-pixel ray path of nirajbabar/raytracinginonesemester.

The compute lives in librt_mi355x.so (HIP kernels for gfx950 + the C ABI of
include/rt_mi355x.h); this package is the host-side mirror of the reference interface.
"""
from ._lib import (RTError, RT_DELIVER_DEVICE, RT_DELIVER_F32, RT_DELIVER_NONE, RT_DELIVER_P6,  # noqa: F401
                   RT_GATHER_AUTO, RT_GATHER_DIRECT, RT_GATHER_HOST_SHARED, RT_GATHER_RCCL, RT_KERNEL_AUTO, RT_KERNEL_LANE,
                   RT_KERNEL_WAVE, RT_FLAG_BINARY, RT_RAYS_CLOSEST, RT_RAYS_OCCLUDED, RT_RAYS_VARIANT_BINARY,
                   RT_RAYS_VARIANT_DEEP, RT_RAYS_VARIANT_NONE, RT_RAYS_VARIANT_WIDE, RT_RENDERER_SELF_SEND, RT_TILES_AUTO, RT_TILES_LINEAR, RT_TILES_ROWS,
                   RT_TILES_XCD_CHUNK, RT_TIME_DELIVER, RT_TIME_FRAME, RT_TIME_GATHER, ShadeOpts, RT_PATH_LAST, RT_PATH_NONE, PathOpts,
                   RT_REBUILD_DEVICE, RT_REBUILD_HOST, RT_REBUILD_NONE, RT_SORT_ORIGIN, RT_SORT_ORIGIN_DIR,
                   RT_MULTI_HIT_MAX_K, RT_LIGHT_MAX_SHADOW_SAMPLES, LIGHT_VIS_GROUPS)
from .api import (  # noqa: F401
    MULTI_HIT_DTYPE, multi_hits_host,
    POINT_HIT_DTYPE, closest_points_host,
    HIT_DTYPE, LIGHT_DTYPE, AdaptiveFilm, Camera, DeviceScene, Film, HostScene, HW1Scene, MeshHW1, Renderer, build_bvh, comm_unique_id, build_bvh_device, default_material, device_count,
    afilm_host, camera_rays, camera_rays_pixels, film_pixels_host, encode_p6, encode_p6_device, hit_fields, hit_record_host, intersect_rays, jittered_samples, p6_header, quantize_p6_device, read_p6,
    PathState, compact_paths, path_finish, path_step_host, refit_aabbs, triangles_from_mesh, build_bvh_triangles,
    gather, ray_key_bits, ray_keys, scatter, sort_rays,
    LIGHT_SHAPE_DTYPE, light_samples_host, path_step_vis_host,
    render, render_hw1, hw1_rects_host, unpermute_strips_device, write_p6, set_tuning, get_tuning, reset_tuning, tuning,
)
