"""Python mirror of the reference's host interface for the per-pixel ray path.

Names and argument meaning follow the reference (citations relative to the reference repo,
G/ = HW2/HW2/GPUandCPU):

* :class:`Camera`       — ``Camera(pos, lookAt, up, focal_length_mm, sensor_height_mm, w, h)``
                          (G/include/camera.h:13-28).
* :class:`HostScene`    — ``SceneIO::LoadSceneFromFile`` + the mesh/BVH pipeline of
                          G/src/main.cu:104-317 (loaders, transforms, CPU LBVH).
* :class:`DeviceScene`  — the scene arrays resident on one MI355X.
* :func:`render`        — ``render(numTriangles, W, H, cam, missColor, max_depth, spp, nodes,
                          aabbs, triangles, triObjectIds, objectMaterials, numObjectMaterials,
                          lights, numLights, diffuse_bounce, output)`` (G/include/query.h:13-29).
* :func:`render_hw1`    — the HW1 brute-force loop (HW1/src/render.cpp:72-116) on the GPU.
* :func:`write_p6` / :func:`read_p6` — ppm_p6 (HW1/ppm_p6_lib/include/ppm_p6.hpp:46-85).

All compute goes through librt_mi355x.so; there is no CPU render path here.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from . import _lib as L
from ._lib import check, lib, ptr

LIGHT_DTYPE = np.dtype([("position", "<f4", 3), ("color", "<f4", 3), ("intensity", "<i4")])
assert LIGHT_DTYPE.itemsize == C.sizeof(L.Light) == 28
# rt_light_shape: a light's radius (<= 0 or NaN: a point light) and shadow rays per shaded point
LIGHT_SHAPE_DTYPE = np.dtype([("radius", "<f4"), ("shadow_samples", "<i4")])
assert LIGHT_SHAPE_DTYPE.itemsize == 8
assert C.sizeof(L.Material) == 52 and C.sizeof(L.Triangle) == 72 and C.sizeof(L.AABB) == 24
# rt_hit (include/rt_mi355x.h): one record of DeviceScene.trace_hits
HIT_DTYPE = np.dtype([("tri", "<i4"), ("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("p", "<f4", 3), ("normal", "<f4", 3),
                      ("geom_normal", "<f4", 3), ("front_face", "<i4"), ("object_id", "<i4"), ("material", "<i4")])
assert HIT_DTYPE.itemsize == C.sizeof(L.Hit) == 64
# rt_multi_hit: one list entry of DeviceScene.trace_multi_hits
MULTI_HIT_DTYPE = np.dtype([("tri", "<i4"), ("t", "<f4"), ("u", "<f4"), ("v", "<f4")])
assert MULTI_HIT_DTYPE.itemsize == 16
# rt_point_hit: one answer of DeviceScene.closest_points
POINT_HIT_DTYPE = np.dtype([("tri", "<i4"), ("d2", "<f4"), ("p", "<f4", 3), ("v", "<f4"), ("w", "<f4"), ("region", "<i4")])
assert POINT_HIT_DTYPE.itemsize == 32


def _v3(v) -> L.Vec3:
    x, y, z = (float(c) for c in v)
    return L.Vec3(x, y, z)


def _f3(v) -> "C.Array":
    return (C.c_float * 3)(*[float(c) for c in v])


class Camera:
    """Pinhole camera; ``hw1=True`` follows HW1/include/camera.h (rejects w, h < 1)."""

    def __init__(self, pos=(0.0, 0.0, 0.0), look_at=(0.0, 1.0, 0.0), up=(0.0, 0.0, 1.0),
                 focal_length_mm: float = 50.0, sensor_height_mm: float = 24.0,
                 width: int = 100, height: int = 100, hw1: bool = False):
        self.pos, self.look_at, self.up = tuple(pos), tuple(look_at), tuple(up)
        self.focal_length_mm, self.sensor_height_mm = float(focal_length_mm), float(sensor_height_mm)
        self.c = L.CameraT()
        check(lib().rt_camera_init(C.byref(self.c), _f3(pos), _f3(look_at), _f3(up),
                                   self.focal_length_mm, self.sensor_height_mm, int(width), int(height),
                                   1 if hw1 else 0))

    @property
    def pixel_width(self) -> int:
        return self.c.pixel_width

    @property
    def pixel_height(self) -> int:
        return self.c.pixel_height

    def basis(self) -> dict:
        """center, pixel00_loc, pixel_delta_u, pixel_delta_v as float32 arrays."""
        return {k: np.array(tuple(getattr(self.c, k)), np.float32)
                for k in ("center", "pixel00_loc", "pixel_delta_u", "pixel_delta_v")}

    def resized(self, width: int, height: int) -> "Camera":
        return Camera(self.pos, self.look_at, self.up, self.focal_length_mm, self.sensor_height_mm,
                      width, height)

    @classmethod
    def from_basis(cls, center, pixel00_loc, pixel_delta_u, pixel_delta_v, width: int, height: int) -> "Camera":
        """A camera from its four basis vectors as given (any float32 words; no rt_camera_init):
        what rt_camera holds.  It has no constructor parameters, so no resized()."""
        self = cls.__new__(cls)
        self.pos = self.look_at = self.up = self.focal_length_mm = self.sensor_height_mm = None
        self.c = L.CameraT()
        self.c.center, self.c.pixel00_loc = _v3(center), _v3(pixel00_loc)
        self.c.pixel_delta_u, self.c.pixel_delta_v = _v3(pixel_delta_u), _v3(pixel_delta_v)
        self.c.pixel_width, self.c.pixel_height = int(width), int(height)
        return self

    def frame_class(self, pad: float = 1.0) -> int:
        """What a frame does with this camera (rt_debug_camera_class): 0 its |D| range is proven,
        the cull and cut run; 1 finite rays that may take get_ray's 1e-12 fallback, no cull; 2 a
        non-finite word or a length that may overflow, the lane kernel without the cull."""
        out = C.c_int32(-1)
        check(lib().rt_debug_camera_class(C.byref(self.c), float(pad), C.byref(out)))
        return int(out.value)


def jittered_samples(spp: int, seed: int = 42, centered: bool = True) -> np.ndarray:
    """(spp, 2) float32 sub-pixel offsets (G/include/antialias.h:12-27; HW1 when not centered)."""
    out = np.zeros((spp, 2), np.float32)
    check(lib().rt_jittered_samples(int(spp), int(seed), 1 if centered else 0, ptr(out)))
    return out


def default_material() -> np.ndarray:
    m = L.Material()
    lib().rt_material_default(C.byref(m))
    return np.frombuffer(bytes(m), np.float32).copy()


class HostScene:
    """A G/-dialect scene loaded and BVH-built on the host (arrays in the reference layouts)."""

    def __init__(self, handle: int):
        self._h = C.c_void_p(handle)
        info = L.SceneInfo()
        check(lib().rt_host_scene_info(self._h, C.byref(info)))
        self.info = info
        arr = L.SceneArrays()
        check(lib().rt_host_scene_arrays(self._h, C.byref(arr)))
        P = int(info.num_triangles)
        NN = 2 * P - 1
        nv = int(info.num_vertices)

        def view(addr, dtype, shape):
            if not addr:
                return None
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            buf = (C.c_char * n).from_address(addr)
            return np.frombuffer(buf, dtype).reshape(shape).copy()  # own the data

        self.num_triangles = P
        self.nodes = view(arr.nodes, np.uint32, (NN, 4))
        self.aabbs = view(arr.aabbs, np.float32, (NN, 6))
        self.triangles = view(arr.triangles, np.float32, (P, 18))
        self.tri_object_ids = view(arr.tri_object_ids, np.int32, (P,))
        self.materials = view(arr.materials, np.float32, (info.num_materials, 13))
        self.lights = view(arr.lights, LIGHT_DTYPE, (info.num_lights,))
        # the lights' shapes (the optional "radius" and "shadow_samples" of a light; point lights without)
        self.light_shapes = np.zeros(info.num_lights, LIGHT_SHAPE_DTYPE)
        check(lib().rt_host_scene_light_shapes(self._h, ptr(self.light_shapes), int(info.num_lights)))
        self.positions = view(arr.positions, np.float32, (nv, 3))
        self.normals = view(arr.normals, np.float32, (nv, 3))
        self.indices = view(arr.indices, np.uint32, (P, 3))

    @classmethod
    def load_json(cls, path, project_dir=None) -> "HostScene":
        h = C.c_void_p()
        check(lib().rt_host_scene_load_json(str(path).encode(),
                                            None if project_dir is None else str(project_dir).encode(),
                                            C.byref(h)))
        return cls(h.value)

    @classmethod
    def load_objs(cls, paths: Sequence) -> "HostScene":
        enc = [str(p).encode() for p in paths]
        arr = (C.c_char_p * len(enc))(*enc)
        h = C.c_void_p()
        check(lib().rt_host_scene_load_objs(C.cast(arr, C.c_void_p), len(enc), C.byref(h)))
        return cls(h.value)

    def camera(self, width: Optional[int] = None, height: Optional[int] = None) -> Camera:
        i = self.info
        return Camera(tuple(i.cam_position), tuple(i.cam_look_at), tuple(i.cam_up), i.focal_length_mm,
                      i.sensor_height_mm, width or i.pixel_width, height or i.pixel_height)

    @property
    def settings(self) -> dict:
        i = self.info
        return {"max_depth": i.max_depth, "spp": i.spp, "diffuse_bounce": bool(i.diffuse_bounce),
                "miss_color": tuple(i.miss_color)}

    def close(self) -> None:
        if self._h:
            lib().rt_host_scene_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MeshHW1:
    """LoadOBJ_ToMeshSOA (HW1/src/MeshOBJ.cpp:143-281)."""

    def __init__(self, path):
        h = C.c_void_p()
        check(lib().rt_mesh_load_obj_hw1(str(path).encode(), C.byref(h)))
        self._h = h
        v = L.MeshView()
        check(lib().rt_mesh_view_get(self._h, C.byref(v)))
        nv, nt = int(v.num_vertices), int(v.num_triangles)
        self.positions = np.frombuffer((C.c_char * (nv * 12)).from_address(v.positions), np.float32).reshape(nv, 3).copy()
        self.normals = (np.frombuffer((C.c_char * (nv * 12)).from_address(v.normals), np.float32).reshape(nv, 3).copy()
                        if v.normals else None)
        self.indices = np.frombuffer((C.c_char * (nt * 12)).from_address(v.indices), np.uint32).reshape(nt, 3).copy()
        self.num_triangles = nt

    def __del__(self):
        try:
            if self._h:
                lib().rt_mesh_free(self._h)
        except Exception:
            pass


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


class DeviceScene:
    """Reference arrays uploaded to one device (rt_scene_create; ``refittable=True``:
    rt_scene_create_refittable, the same scene plus what ``refit`` needs on the device)."""

    def __init__(self, num_triangles: int, nodes, aabbs, triangles, tri_object_ids=None,
                 materials=None, lights=None, device: int = 0, refittable: bool = False):
        P = int(num_triangles)
        self._keep = [_c(nodes, np.uint32), _c(aabbs, np.float32), _c(triangles, np.float32)]
        objs = None if tri_object_ids is None else _c(tri_object_ids, np.int32)
        mats = None if materials is None else _c(materials, np.float32).reshape(-1, 13)
        lts = None if lights is None else np.ascontiguousarray(lights, dtype=LIGHT_DTYPE)
        nmat = 0 if mats is None else mats.shape[0]
        nl = 0 if lts is None else lts.shape[0]
        h = C.c_void_p()
        create = lib().rt_scene_create_refittable if refittable else lib().rt_scene_create
        check(create(int(device), P, ptr(self._keep[0]), ptr(self._keep[1]), ptr(self._keep[2]),
                     ptr(objs), ptr(mats), nmat, ptr(lts), nl, C.byref(h)))
        self._h = h
        self._owned = True
        self.num_triangles = P
        self.device = device

    @classmethod
    def _borrow(cls, handle, num_triangles: int, owner) -> "DeviceScene":
        """A scene owned by a Renderer (its timing queries; destroyed with the renderer, which
        then invalidates this view: later calls raise instead of touching freed memory)."""
        self = cls.__new__(cls)
        self._h = C.c_void_p(handle)
        self._owned = False
        self._owner = owner
        self._keep = []
        self.num_triangles = num_triangles
        self.device = int(lib().rt_scene_device(self._h))
        return self

    def _handle(self) -> C.c_void_p:
        if not self._h:
            raise L.RTError(-1, "scene is closed (or its Renderer was closed)")
        return self._h

    @classmethod
    def from_host(cls, hs: HostScene, device: int = 0, refittable: bool = False) -> "DeviceScene":
        return cls(hs.num_triangles, hs.nodes, hs.aabbs, hs.triangles, hs.tri_object_ids, hs.materials,
                   hs.lights, device, refittable)

    def refit(self, triangles, stream: Optional[int] = None, timing: bool = False):
        """Move the scene's triangles (rt_scene_refit / rt_scene_refit_device): ``triangles`` holds
        the P triangles in the order given at creation, as a numpy (P, 18) float32 array (v0, v1,
        v2, n0, n1, n2) or a torch tensor of that shape on the scene's device, which takes the
        device path on ``stream`` (a HIP stream handle; default torch's current stream).  The tree
        and its records stay; every box, edge and normal is rewritten, so every query answers as
        the reference does on (nodes, refit_aabbs(nodes, triangles), triangles).  The call waits
        for the scene's own work and returns when the refit is done.  ``timing=True`` returns the
        HIP-event ms of its launches.  Only for scenes made with ``refittable=True``."""
        ms = C.c_float(0.0)
        P = self.num_triangles
        if _is_torch(triangles):
            import torch

            dev = torch.device("cuda", self.device)
            if triangles.device != dev or triangles.dtype != torch.float32 or triangles.numel() != 18 * P:
                raise ValueError(f"refit: expects a ({P}, 18) float32 tensor on {dev}")
            t = triangles.contiguous()
            check(lib().rt_scene_refit_device(self._handle(), t.data_ptr(), _stream_of(stream, dev),
                                              C.byref(ms) if timing else None))
        else:
            t = _c(triangles, np.float32)
            if t.size != 18 * P:
                raise ValueError(f"refit: expects a ({P}, 18) array of triangles")
            check(lib().rt_scene_refit(self._handle(), ptr(t), C.byref(ms) if timing else None))
        return ms.value if timing else None

    def rebuild(self, triangles, stream: Optional[int] = None, timing: bool = False, tree: bool = False):
        """New triangles and a new tree under the scene (rt_scene_rebuild / rt_scene_rebuild_device):
        ``triangles`` as ``refit`` takes them (a numpy (P, 18) array, or a tensor on the scene's
        device, which takes the device entry on ``stream``).  The tree is the reference's LBVH over
        them (build_bvh_triangles), built on the device; every packed array and the refit plan are
        what a refittable scene created from (that tree, triangles) holds, byte for byte, packed on
        the device too where the tree and the knobs allow (``rebuild_path``).  An error
        (a vertex that is not finite, quantised records) leaves the scene as it was.
        ``tree=True`` also returns (nodes (2P-1, 4) uint32, aabbs (2P-1, 6) float32), as numpy
        arrays or, for a tensor, device tensors (nodes as int32 bit patterns).  The return value is
        None, ms (``timing``), (nodes, aabbs) (``tree``) or (ms, nodes, aabbs) (both).  Only for
        scenes made with ``refittable=True``."""
        ms = C.c_float(0.0)
        P = self.num_triangles
        NN = 2 * P - 1
        nodes = aabbs = None
        if _is_torch(triangles):
            import torch

            dev = torch.device("cuda", self.device)
            if triangles.device != dev or triangles.dtype != torch.float32 or triangles.numel() != 18 * P:
                raise ValueError(f"rebuild: expects a ({P}, 18) float32 tensor on {dev}")
            t = triangles.contiguous()
            if tree:
                nodes = torch.empty((NN, 4), dtype=torch.int32, device=dev)
                aabbs = torch.empty((NN, 6), dtype=torch.float32, device=dev)
            check(lib().rt_scene_rebuild_device(self._handle(), t.data_ptr(), _stream_of(stream, dev),
                                                nodes.data_ptr() if tree else None, aabbs.data_ptr() if tree else None,
                                                C.byref(ms) if timing else None))
        else:
            t = _c(triangles, np.float32)
            if t.size != 18 * P:
                raise ValueError(f"rebuild: expects a ({P}, 18) array of triangles")
            if tree:
                nodes, aabbs = np.zeros((NN, 4), np.uint32), np.zeros((NN, 6), np.float32)
            check(lib().rt_scene_rebuild(self._handle(), ptr(t), ptr(nodes), ptr(aabbs), C.byref(ms) if timing else None))
        if tree:
            return (ms.value, nodes, aabbs) if timing else (nodes, aabbs)
        return ms.value if timing else None

    @property
    def rebuild_path(self) -> int:
        """RT_REBUILD_* of the latest ``rebuild`` (rt_scene_rebuild_path): RT_REBUILD_DEVICE when the
        records were packed on the device too, RT_REBUILD_HOST when the host packed them from the
        device-built tree, RT_REBUILD_NONE before any rebuild."""
        return int(lib().rt_scene_rebuild_path(self._handle()))

    @property
    def rebuild_counts(self) -> tuple:
        """(kernel launches of the latest rebuild's pack on the device, its host read-backs)."""
        c = np.zeros(2, np.int64)
        check(lib().rt_scene_rebuild_counts(self._handle(), ptr(c)))
        return int(c[0]), int(c[1])

    def digest(self) -> tuple:
        """(info (21,) int64, digests (22,) uint64) of the resident arrays, read back from the
        device and hashed (rt_debug_scene_digest): rt_debug_scene_pack's words."""
        info, dig = np.zeros(21, np.int64), np.zeros(22, np.uint64)
        check(lib().rt_debug_scene_digest(self._handle(), ptr(info), ptr(dig)))
        return info, dig

    def bounds(self) -> np.ndarray:
        """The root box the scene holds now, (6,) float32, min corner then max corner
        (rt_scene_bounds): after a ``refit`` or ``rebuild`` the new one.  The box ``sort=`` uses."""
        b = L.AABB()
        check(lib().rt_scene_bounds(self._handle(), C.byref(b)))
        return np.array([*b.min_corner, *b.max_corner], np.float32)

    def _sorted_rays(self, rays, sort, stream):
        """(rays in key order, order) for a query's ``sort=`` ("origin", "origin_dir" or True, the
        measured default) on the device path: the scene's box, the mode's default bits."""
        return sort_rays(rays, self.bounds(), SORT_DEFAULT if sort is True else sort, None, stream)

    def _sort_query(self, rays, sort, stream, *side):
        """A query's ``sort=`` prologue on the device path: (rays, order, *side), the rays sorted and
        the per-ray ``side`` tensors (None allowed) gathered; as given, with order None, without a sort."""
        if sort is None or sort is False or rays.shape[0] == 0:
            return (rays, None, *side)
        rays, order = self._sorted_rays(rays, sort, stream)
        return (rays, order, *(None if a is None else gather(a, order, stream=stream) for a in side))

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    @property
    def device_bytes(self) -> int:
        return int(lib().rt_scene_device_bytes(self._handle()))

    @staticmethod
    def make_opts(spp: int = 1, max_depth: int = 1, diffuse_bounce: bool = True, miss_color=(0, 0, 0),
                  jitter=None, band_rows: int = 8, band_index: int = 0, band_count: int = 1,
                  kernel: int = L.RT_KERNEL_AUTO, tile_order: int = L.RT_TILES_AUTO, flags: int = 0):
        o = L.RenderOpts()
        lib().rt_render_opts_default(C.byref(o))
        o.spp, o.max_depth, o.diffuse_bounce = int(spp), int(max_depth), 1 if diffuse_bounce else 0
        o.miss_color = _v3(miss_color)
        jit = None
        if jitter is not None:
            jit = _c(jitter, np.float32).reshape(-1)
            o.jitter = jit.ctypes.data
        o.band_rows, o.band_index, o.band_count, o.kernel = int(band_rows), int(band_index), int(band_count), int(kernel)
        o.tile_order = int(tile_order)
        o.flags = int(flags)
        return o, jit

    def render(self, camera: Camera, spp: int = 1, max_depth: int = 1, diffuse_bounce: bool = True,
               miss_color=(0, 0, 0), jitter=None, aov: bool = False, band_rows: int = 8,
               band_index: int = 0, band_count: int = 1, kernel: int = L.RT_KERNEL_AUTO,
               tile_order: int = L.RT_TILES_AUTO, flags: int = 0):
        """Synchronous render to host: (rows, W, 3) float32 [+ (rows, W, spp) hit idx / t]."""
        o, _jit = self.make_opts(spp, max_depth, diffuse_bounce, miss_color, jitter, band_rows, band_index,
                                 band_count, kernel, tile_order, flags)
        W = camera.pixel_width
        rows = lib().rt_shard_rows(camera.pixel_height, o.band_rows, o.band_index, o.band_count)
        if rows < 0:
            raise L.RTError(-1, "bad band parameters")
        rgb = np.zeros((rows, W, 3), np.float32)
        hi = ht = None
        if aov:
            hi = np.zeros((rows, W, spp), np.int32)
            ht = np.zeros((rows, W, spp), np.float32)
        check(lib().rt_render(self._handle(), C.byref(camera.c), C.byref(o), ptr(rgb), ptr(hi), ptr(ht)))
        return (rgb, hi, ht) if aov else rgb

    def count_rays(self, camera: Camera, spp: int = 1, max_depth: int = 1, diffuse_bounce: bool = True,
                   miss_color=(0, 0, 0), band_rows: int = 8, band_index: int = 0, band_count: int = 1) -> dict:
        """Rays one frame traces (rt_count_rays_ex): camera, shadow and bounce counts, the classes
        of the oracle's stats["rays"], and camera_traced, the camera rays of the tiles the culling
        passes leave to the render kernel (the rest provably miss and are not traversed)."""
        o, _jit = self.make_opts(spp, max_depth, diffuse_bounce, miss_color, None, band_rows, band_index,
                                 band_count)
        out = (C.c_uint64 * 4)()
        check(lib().rt_count_rays_ex(self._handle(), C.byref(camera.c), C.byref(o), out))
        return {"camera": int(out[0]), "shadow": int(out[1]), "bounce": int(out[2]), "camera_traced": int(out[3])}

    def render_device(self, camera: Camera, opts, rgb_dev_ptr: int, hit_idx_ptr=None, hit_t_ptr=None,
                      stream: Optional[int] = None, p6_dev_ptr=None) -> None:
        """Render into device memory (rt_render_device); with ``p6_dev_ptr`` the render and cull
        kernels also write the pixels' P6 samples (write_p6 defaults), rt_render_device_p6."""
        check(lib().rt_render_device_p6(self._handle(), C.byref(camera.c), C.byref(opts), rgb_dev_ptr, hit_idx_ptr,
                                        hit_t_ptr, p6_dev_ptr, stream))

    def render_device_pair(self, camera_a: Camera, camera_b: Camera, opts, rgb_a=None, p6_a=None, rgb_b=None,
                           p6_b=None, stream: Optional[int] = None) -> None:
        """Two frames with one launch of the render kernel where it fits them
        (rt_render_device_pair): the images of two render_device calls."""
        check(lib().rt_render_device_pair(self._handle(), C.byref(camera_a.c), C.byref(camera_b.c), C.byref(opts),
                                          rgb_a, p6_a, rgb_b, p6_b, stream))

    def kernel_times(self, max_launches: int = 256) -> np.ndarray:
        """ms of the render kernel for the most recent launches (HIP events on its stream)."""
        out = np.zeros(max_launches, np.float32)
        n = C.c_int()
        check(lib().rt_kernel_times(self._handle(), ptr(out), max_launches, C.byref(n)))
        return out[:n.value]

    def live_tiles(self) -> tuple:
        """(traced tiles, all tiles) of the most recent render."""
        live, total = C.c_int64(), C.c_int64()
        check(lib().rt_live_tiles(self._handle(), C.byref(live), C.byref(total)))
        return live.value, total.value

    def kernel_name(self) -> str:
        """The render kernel instantiation of the most recent frame, as rocprofv3 names it."""
        return lib().rt_scene_kernel_name(self._handle()).decode()

    def heavy_tiles(self) -> int:
        """Tiles the most recent render dispatched first (heavy-first order, speed only)."""
        n = C.c_int64()
        check(lib().rt_heavy_tiles(self._handle(), C.byref(n)))
        return n.value

    def frame_times(self, max_launches: int = 256) -> np.ndarray:
        """ms of the frame's device work (cull pre-passes + render kernel)."""
        out = np.zeros(max_launches, np.float32)
        n = C.c_int()
        check(lib().rt_frame_times(self._handle(), ptr(out), max_launches, C.byref(n)))
        return out[:n.value]

    def prepass_times(self, max_launches: int = 256) -> np.ndarray:
        """ms of the cull pre-passes (root-box cull + tree-cut cull) alone."""
        out = np.zeros(max_launches, np.float32)
        n = C.c_int()
        check(lib().rt_prepass_times(self._handle(), ptr(out), max_launches, C.byref(n)))
        return out[:n.value]

    def traversal_info(self) -> dict:
        """The traversal rt_scene_create chose (rt_scene_traversal_info)."""
        info = (C.c_int64 * 4)()
        check(lib().rt_scene_traversal_info(self._handle(), info))
        return {"frustum_log2": int(info[0]), "frustum_bound": int(info[1]), "wide": bool(info[2]),
                "deep": bool(info[3])}

    def trace_rays(self, rays, mode: str = "closest", max_t=None, flags: int = 0, stream: Optional[int] = None,
                   timing: bool = False, sort=None):
        """Batched ray queries against this scene (rt_trace_rays / rt_trace_rays_device): ``rays`` is
        (n, 6) float32, origin then direction, the direction used as given.

        * ``mode="closest"``: SearchBVH (G/include/query.h:224-311) per ray; returns ``(idx, t)``,
          int32 triangle indices (-1: miss) and the reference's float32 t (-1.0: miss).
        * ``mode="occluded"``: IsInShadow's decision (G/include/shader.h:59-61) against ``max_t``
          (n float32, required); returns a bool array, True where a hit has t < max_t.

        A numpy array takes the host path (upload, trace, download, synchronise; ``timing=True``
        appends the kernel's HIP-event ms).  Torch tensors on the scene's device take the device
        path: one launch on ``stream`` (a HIP stream handle; default torch's current stream), no
        host synchronisation, tensors returned.  ``flags``: RT_FLAG_BINARY or 0.

        ``sort`` (device path only): "origin", "origin_dir" or True (the measured default) runs the
        same query on the rays in coherence order (``sort_rays`` in the scene's ``bounds()``, ``max_t``
        gathered) and scatters the answers back to the caller's order: the same bits, a different
        assignment of rays to lanes."""
        modes = {"closest": L.RT_RAYS_CLOSEST, "occluded": L.RT_RAYS_OCCLUDED}
        if mode not in modes:
            raise ValueError(f"trace_rays: mode must be one of {sorted(modes)}, not {mode!r}")
        m = modes[mode]
        occluded = m == L.RT_RAYS_OCCLUDED
        if _is_torch(rays):
            import torch

            dev = self._torch_dev()
            rays = _query_tensor(rays, 6, dev, "trace_rays", timing)
            n = rays.shape[0]
            mt = _per_item(max_t, n, dev, "trace_rays", "max_t", "ray")
            stream = _stream_of(stream, dev)
            rays, order, mt = self._sort_query(rays, sort, stream, mt)
            idx = torch.empty(n, dtype=torch.int32, device=dev)
            t = None if occluded else torch.empty(n, dtype=torch.float32, device=dev)
            check(lib().rt_trace_rays_device(self._handle(), m, rays.data_ptr(), None if mt is None else mt.data_ptr(),
                                             n, int(flags), idx.data_ptr(), None if t is None else t.data_ptr(),
                                             stream))
            idx, t = _unsort(order, stream, dev, (rays, mt), idx, t)
            return idx != 0 if occluded else (idx, t)
        if sort is not None and sort is not False:
            raise ValueError("trace_rays: sort is for the device path (torch tensors) only")
        r = _query_array(rays, 6, "trace_rays", "origins and directions")
        n = r.shape[0]
        mt = _per_item(max_t, n, None, "trace_rays", "max_t", "ray")
        idx = np.zeros(n, np.int32)
        t = None if occluded else np.zeros(n, np.float32)
        ms = C.c_float(0.0)
        check(lib().rt_trace_rays(self._handle(), m, ptr(r), ptr(mt), n, int(flags), ptr(idx), ptr(t),
                                  C.byref(ms) if timing else None))
        out = idx != 0 if occluded else (idx, t)
        return (out, ms.value) if timing else out

    def trace_rays_variant(self) -> int:
        """The traversal the latest trace_rays call launched (RT_RAYS_VARIANT_*)."""
        return int(lib().rt_trace_rays_variant(self._handle()))

    def shade_rays(self, rays, seeds=None, max_depth: int = 1, diffuse_bounce: bool = True, miss_color=(0, 0, 0),
                   flags: int = 0, aov: bool = False, stream: Optional[int] = None, timing: bool = False, sort=None):
        """Radiance of caller rays (rt_shade_rays / rt_shade_rays_device): per ray the reference's
        TraceRayIterative (G/include/query.h:156-220) with ``rng_state = seeds[i]`` (uint32, n; None:
        42 for every ray), bit for bit, the final clamp included.  ``rays`` is (n, 6) float32, origin
        then direction, the direction used as given (results are pinned for unit directions).

        Returns ``radiance`` (n, 3) float32, or ``(radiance, idx, t)`` with ``aov=True``: the first
        segment's SearchBVH result as trace_rays gives it (-1 / -1.0 on a miss or max_depth <= 0).

        A numpy array takes the host path (upload, shade, download, synchronise; ``timing=True``
        appends the kernel's HIP-event ms).  Torch tensors on the scene's device take the device
        path: one launch on ``stream`` (a HIP stream handle; default torch's current stream), no
        host synchronisation, tensors returned.  ``flags``: RT_FLAG_BINARY or 0.  ``sort``: as for
        trace_rays (rays sorted, ``seeds`` gathered, every output scattered back)."""
        o = L.ShadeOpts()
        o.max_depth, o.diffuse_bounce = int(max_depth), 1 if diffuse_bounce else 0
        o.miss_color = _v3(miss_color)
        o.flags = int(flags)
        if _is_torch(rays):
            import torch

            dev = self._torch_dev()
            rays = _query_tensor(rays, 6, dev, "shade_rays", timing)
            n = rays.shape[0]
            sd = _seed_tensor(seeds, n, dev, "shade_rays", "ray")
            stream = _stream_of(stream, dev)
            # (uint32 tensors have few torch ops: int32 tensors carry the same 32 bits)
            rays, order, sd = self._sort_query(rays, sort, stream, None if sd is None else sd.view(torch.int32))
            rad = torch.empty((n, 3), dtype=torch.float32, device=dev)
            idx = torch.empty(n, dtype=torch.int32, device=dev) if aov else None
            t = torch.empty(n, dtype=torch.float32, device=dev) if aov else None
            check(lib().rt_shade_rays_device(self._handle(), rays.data_ptr(), None if sd is None else sd.data_ptr(), n,
                                             C.byref(o), rad.data_ptr(), None if idx is None else idx.data_ptr(),
                                             None if t is None else t.data_ptr(), stream))
            rad, idx, t = _unsort(order, stream, dev, (rays, sd), rad, idx, t)
            return (rad, idx, t) if aov else rad
        if sort is not None and sort is not False:
            raise ValueError("shade_rays: sort is for the device path (torch tensors) only")
        r = _query_array(rays, 6, "shade_rays", "origins and directions")
        n = r.shape[0]
        sd = None
        if seeds is not None:
            sd = _c(seeds, np.uint32)
            if sd.shape != (n,):
                raise ValueError("shade_rays: seeds must hold one uint32 per ray")
        rad = np.zeros((n, 3), np.float32)
        idx = np.zeros(n, np.int32) if aov else None
        t = np.zeros(n, np.float32) if aov else None
        ms = C.c_float(0.0)
        check(lib().rt_shade_rays(self._handle(), ptr(r), ptr(sd), n, C.byref(o), ptr(rad), ptr(idx), ptr(t),
                                  C.byref(ms) if timing else None))
        out = (rad, idx, t) if aov else rad
        return (out, ms.value) if timing else out

    def shade_rays_variant(self) -> int:
        """The traversal the latest shade_rays call launched (RT_RAYS_VARIANT_*)."""
        return int(lib().rt_shade_rays_variant(self._handle()))

    def render_rays(self, camera: Camera, spp: int, max_depth: int = 1, diffuse_bounce: bool = True,
                    miss_color=(0, 0, 0), jitter=None, pass_spp: Optional[int] = None,
                    band_rows: Optional[int] = None, ray_fn=None, p6: bool = False, film: Optional["Film"] = None,
                    material_fn=None, light_shapes=None):
        """A frame through the query path, on the device: for every sample pass (``pass_spp``
        samples; default all) and row band (``band_rows`` rows; default all) camera_rays ->
        ``ray_fn`` -> shade_rays -> Film.add, then one Film.resolve.  Memory is bounded by one
        band of one pass; with ``ray_fn=None`` the frame is render()'s bit for bit.

        ``ray_fn(rays, seeds, row0, rows, sample0, n) -> rays`` is the hook of a camera of one's
        own (thin lens, fisheye, resampling): it gets the pinhole rays ((rows*W*n, 6) float32 tensor)
        and seeds of the step and returns the rays to shade, same shape and order.
        ``jitter``: (spp, 2) float32, None for jittered_samples(spp).  ``film``: a Film of the
        camera's size to accumulate into (neither cleared before nor closed after: samples already
        there stay in the sums); default a new one, closed on return.
        ``material_fn``: when given, the step's radiance comes from trace_paths with that hook (a
        material per hit; see trace_paths) instead of shade_rays.
        ``light_shapes``: when given, the step's radiance comes from trace_paths with these shapes
        (soft shadows where a radius is positive; see trace_paths).
        Returns Film.resolve's result for the whole image, on torch's current stream."""
        W, H, spp = camera.pixel_width, camera.pixel_height, int(spp)
        if spp < 1:
            raise ValueError("render_rays: spp < 1")
        pass_spp = spp if pass_spp is None else int(pass_spp)
        band_rows = H if band_rows is None else int(band_rows)
        if pass_spp < 1 or band_rows < 1:
            raise ValueError("render_rays: pass_spp and band_rows must be positive")
        jit = (jittered_samples(spp) if jitter is None else _c(jitter, np.float32)).reshape(-1, 2)
        if jit.shape[0] != spp:
            raise ValueError("render_rays: jitter must hold (spp, 2) floats")
        own = film is None
        if own:
            film = Film(W, H, self.device)
        elif (film.width, film.height, film.device) != (W, H, self.device):
            raise ValueError("render_rays: the film is not of the camera's size on the scene's device")
        try:
            for s0 in range(0, spp, pass_spp):
                n = min(pass_spp, spp - s0)
                for r0 in range(0, H, band_rows):
                    rows = min(band_rows, H - r0)
                    rays, seeds = camera_rays(camera, n, jit[s0:s0 + n], r0, rows, device=self.device, sample0=s0)
                    if ray_fn is not None:
                        rays = ray_fn(rays, seeds, r0, rows, s0, n)
                    if material_fn is None and light_shapes is None:
                        rad = self.shade_rays(rays, seeds, max_depth, diffuse_bounce, miss_color)
                    else:
                        rad = self.trace_paths(rays, seeds, max_depth, diffuse_bounce, miss_color, material_fn=material_fn,
                                               light_shapes=light_shapes)
                    film.add(rad, r0, rows, n)
            return film.resolve(p6=p6)
        finally:
            if own:
                film.close()

    def render_adaptive(self, camera: Camera, min_spp: int, max_spp: int, step_spp: int, tol: float, max_depth: int = 1,
                        diffuse_bounce: bool = True, miss_color=(0, 0, 0), jitter=None, ray_fn=None, material_fn=None,
                        p6: bool = False, film: Optional["AdaptiveFilm"] = None):
        """A frame with per-pixel sample counts, on the device: one dense pass of ``min_spp``
        samples, then ``AdaptiveFilm.select -> camera_rays_pixels -> ray_fn -> shade_rays |
        trace_paths -> AdaptiveFilm.add`` with ``step_spp`` samples for the selected pixels until
        none is selected, then one resolve.  A pixel goes on while its count + step_spp <= max_spp
        and the standard error of its mean luminance exceeds ``tol`` times the mean (see
        AdaptiveFilm.select).  Every pixel gets its samples 0, 1, ... in order from the frame's
        jitter table, so a pixel that ends with c samples is render(spp=c)'s pixel bit for bit;
        ``tol=0`` with max_spp - min_spp a multiple of step_spp is render(spp=max_spp).

        ``jitter``: (max_spp, 2) float32, None for jittered_samples(max_spp).
        ``ray_fn(rays, seeds, pixels, counts, n) -> rays`` as in render_rays: the pass's pinhole rays
        ((m*n, 6), entry k's n samples together), their seeds, the pixel indices y*W+x ((m,) int32)
        and the film's count map ((W*H,) int32, the samples each pixel had before this pass).
        ``material_fn``: radiance from trace_paths with that hook instead of shade_rays.
        ``film``: an AdaptiveFilm of the camera's size to go on from (not cleared before, not
        closed after); default a new one, closed on return.
        One 4-byte read of the selected count per pass is the only host synchronisation.
        Returns ``(rgb, counts)`` [``, bytes`` with ``p6=True``]: (H, W, 3) float32, (H, W) int32
        samples per pixel, (H, W, 3) uint8 P6 samples."""
        import torch

        W, H = camera.pixel_width, camera.pixel_height
        min_spp, max_spp, step_spp = int(min_spp), int(max_spp), int(step_spp)
        if min_spp < 2 or max_spp < min_spp or step_spp < 1:
            raise ValueError("render_adaptive: needs 2 <= min_spp <= max_spp and step_spp >= 1")
        jit = (jittered_samples(max_spp) if jitter is None else _c(jitter, np.float32)).reshape(-1, 2)
        if jit.shape[0] < max_spp:
            raise ValueError("render_adaptive: jitter must hold (max_spp, 2) floats")
        dev = self._torch_dev()
        own = film is None
        if own:
            film = AdaptiveFilm(W, H, self.device)
        elif (film.width, film.height, film.device) != (W, H, self.device):
            raise ValueError("render_adaptive: the film is not of the camera's size on the scene's device")

        def shade(pixels, n):
            rays, seeds = camera_rays_pixels(camera, pixels, film, n, jd, device=self.device)
            if ray_fn is not None:
                shown = pixels if pixels is not None else torch.arange(W * H, dtype=torch.int32, device=dev)
                rays = ray_fn(rays, seeds, shown, film.counts, n)
            if material_fn is None:
                rad = self.shade_rays(rays, seeds, max_depth, diffuse_bounce, miss_color)
            else:
                rad = self.trace_paths(rays, seeds, max_depth, diffuse_bounce, miss_color, material_fn=material_fn)
            film.add(rad, pixels, n)

        try:
            jd = torch.from_numpy(np.ascontiguousarray(jit)).to(dev)
            shade(None, min_spp)
            while True:
                pixels, m = film.select(min_spp, max_spp, step_spp, tol)
                if m == 0:
                    break
                shade(pixels, step_spp)
            out = film.resolve(p6=p6, counts=True)
            return (out[0], out[1].view(H, W), out[2]) if p6 else (out[0], out[1].view(H, W))
        finally:
            if own:
                film.close()

    def trace_hits(self, rays, flags: int = 0, stream: Optional[int] = None, timing: bool = False, sort=None):
        """Hit records of caller rays (rt_trace_hits / rt_trace_hits_device): per ray the HitRecord
        SearchBVH returns (G/include/query.h:224-311, intersectTriangle's tail :110-130) with the ids
        assignMaterialToHit reads, bit for bit.  ``rays`` is (n, 6) float32, origin then direction,
        the direction used as given; ``tri`` and ``t`` are trace_rays' closest-hit answers.  A miss
        is tri -1, t -1.0 and zero elsewhere.

        A numpy array takes the host path and returns an (n,) array of HIT_DTYPE (``timing=True``
        appends the kernel's HIP-event ms).  A torch tensor on the scene's device takes the device
        path: one launch on ``stream`` (a HIP stream handle; default torch's current stream), no host
        synchronisation, and one (n, 16) int32 tensor is returned, the records' 32-bit words
        (hit_fields names them).  ``flags``: RT_FLAG_BINARY or 0.  ``sort``: as for trace_rays (rays
        sorted, the records scattered back)."""
        if _is_torch(rays):
            import torch

            dev = self._torch_dev()
            rays = _query_tensor(rays, 6, dev, "trace_hits", timing)
            n = rays.shape[0]
            stream = _stream_of(stream, dev)
            rays, order = self._sort_query(rays, sort, stream)
            hits = torch.empty((n, 16), dtype=torch.int32, device=dev)
            check(lib().rt_trace_hits_device(self._handle(), rays.data_ptr(), n, int(flags), hits.data_ptr(), stream))
            return _unsort(order, stream, dev, (rays,), hits)[0]
        if sort is not None and sort is not False:
            raise ValueError("trace_hits: sort is for the device path (torch tensors) only")
        r = _query_array(rays, 6, "trace_hits", "origins and directions")
        n = r.shape[0]
        hits = np.zeros(n, HIT_DTYPE)
        ms = C.c_float(0.0)
        check(lib().rt_trace_hits(self._handle(), ptr(r), n, int(flags), ptr(hits), C.byref(ms) if timing else None))
        return (hits, ms.value) if timing else hits

    def trace_hits_variant(self) -> int:
        """The traversal the latest trace_hits call launched (RT_RAYS_VARIANT_*)."""
        return int(lib().rt_trace_hits_variant(self._handle()))

    def trace_multi_hits(self, rays, k: int, max_t=None, flags: int = 0, stream: Optional[int] = None,
                         timing: bool = False):
        """Every hit along caller rays (rt_trace_multi_hits / rt_trace_multi_hits_device): per ray
        the number of triangles it hits in [1e-4, max_t] (``max_t`` n float32; None: FLT_MAX) and the
        ``k`` nearest of them (0 <= k <= RT_MULTI_HIT_MAX_K) by ascending t, then triangle index.
        Nothing stops at the first surface and nothing is pruned: the hit set is SearchBVH's
        (G/include/query.h:224-311) with the bound held at max_t, its overflow rule included.

        Returns ``(count, tri, t, u, v)``: ``count`` (n,) int32, the full number of hits (it may
        exceed k); ``tri`` (n, k) int32 and ``t``, ``u``, ``v`` (n, k) float32, intersectTriangle's
        values bit for bit, -1 / -1.0 / 0 / 0 in the slots past ``count``.

        A numpy array takes the host path (upload, trace, download, synchronise; ``timing=True``
        appends the kernel's HIP-event ms).  Torch tensors on the scene's device take the device
        path: one launch on ``stream`` (a HIP stream handle; default torch's current stream), no
        host synchronisation, tensors returned (views of one (n, k, 4) record tensor).  ``flags``:
        RT_FLAG_BINARY or 0."""
        k = int(k)
        if not 0 <= k <= L.RT_MULTI_HIT_MAX_K:
            raise ValueError(f"trace_multi_hits: k must be in 0..{L.RT_MULTI_HIT_MAX_K}")
        if _is_torch(rays):
            import torch

            dev = self._torch_dev()
            rays = _query_tensor(rays, 6, dev, "trace_multi_hits", timing)
            n = rays.shape[0]
            mt = _per_item(max_t, n, dev, "trace_multi_hits", "max_t", "ray")
            stream = _stream_of(stream, dev)
            count = torch.empty(n, dtype=torch.int32, device=dev)
            rec = torch.empty((n, k, 4), dtype=torch.int32, device=dev)
            if n > 0:  # (an empty tensor has no address to pass)
                check(lib().rt_trace_multi_hits_device(self._handle(), rays.data_ptr(), None if mt is None else mt.data_ptr(),
                                                       n, k, int(flags), rec.data_ptr() if k > 0 else None,
                                                       count.data_ptr(), stream))
            _used_on(stream, dev, rays, mt)
            f = rec.view(torch.float32)
            return count, rec[:, :, 0], f[:, :, 1], f[:, :, 2], f[:, :, 3]
        r = _query_array(rays, 6, "trace_multi_hits", "origins and directions")
        n = r.shape[0]
        mt = _per_item(max_t, n, None, "trace_multi_hits", "max_t", "ray")
        count = np.zeros(n, np.int32)
        rec = np.zeros((n, k), MULTI_HIT_DTYPE)
        ms = C.c_float(0.0)
        check(lib().rt_trace_multi_hits(self._handle(), ptr(r), ptr(mt), n, k, int(flags), ptr(rec) if k > 0 else None,
                                        ptr(count), C.byref(ms) if timing else None))
        out = (count, rec["tri"], rec["t"], rec["u"], rec["v"])
        return (*out, ms.value) if timing else out

    def count_hits(self, rays, max_t=None, flags: int = 0, stream: Optional[int] = None, timing: bool = False):
        """The number of triangles each ray hits in [1e-4, max_t]: trace_multi_hits with k = 0, which
        keeps no list.  Returns ``count`` (n,) int32 (``timing=True`` on the host path: ``(count, ms)``)."""
        out = self.trace_multi_hits(rays, 0, max_t=max_t, flags=flags, stream=stream, timing=timing)
        return (out[0], out[-1]) if timing else out[0]

    def multi_hits_variant(self) -> int:
        """The traversal the latest trace_multi_hits / count_hits call launched (RT_RAYS_VARIANT_*)."""
        return int(lib().rt_trace_multi_hits_variant(self._handle()))

    def closest_points(self, points, max_d2=None, flags: int = 0, stream: Optional[int] = None, timing: bool = False,
                       evals: bool = False):
        """The nearest triangle to each query point (rt_closest_points / rt_closest_points_device,
        DESIGN.md §4.28): the brute-force minimum of (squared distance, triangle index) over the
        scene's leaves in the float32 arithmetic of include/rt_mi355x.h, found by a walk that prunes
        by the distance to a box.  ``points`` (n, 3) float32; ``max_d2`` (n,) float32 bounds on the
        squared distance (a surface at exactly the bound counts; None: +inf).

        Returns ``(tri, d2, p, v, w, region)``: ``tri`` (n,) int32, ``d2`` (n,) float32, ``p`` (n, 3)
        float32 the nearest point, ``v``, ``w`` its coordinates along e1 and e2, ``region`` (n,) int32
        (0 A, 1 B, 2 C, 3 AB, 4 AC, 5 BC, 6 face); -1, -1.0, 0, 0, 0, -1 without a surface in bound.
        ``evals=True`` appends the number of leaf triangles evaluated per point (n,) uint32 (int32
        bits on the device path).

        A numpy array takes the host path (upload, query, download, synchronise; ``timing=True``
        appends the kernel's HIP-event ms).  Torch tensors on the scene's device take the device
        path: one launch on ``stream`` (a HIP stream handle; default torch's current stream), no
        host synchronisation, tensors returned (views of one (n, 8) record tensor).  ``flags``:
        RT_FLAG_BINARY or 0."""
        if _is_torch(points):
            import torch

            dev = self._torch_dev()
            points = _query_tensor(points, 3, dev, "closest_points", timing)
            n = points.shape[0]
            md = _per_item(max_d2, n, dev, "closest_points", "max_d2", "point")
            stream = _stream_of(stream, dev)
            rec = torch.empty((n, 8), dtype=torch.int32, device=dev)
            ev = torch.empty(n, dtype=torch.int32, device=dev) if evals else None
            if n > 0:  # (an empty tensor has no address to pass)
                check(lib().rt_closest_points_device(self._handle(), points.data_ptr(), None if md is None else md.data_ptr(),
                                                     n, int(flags), rec.data_ptr(), None if ev is None else ev.data_ptr(),
                                                     stream))
            _used_on(stream, dev, points, md)
            f = rec.view(torch.float32)
            out = (rec[:, 0], f[:, 1], f[:, 2:5], f[:, 5], f[:, 6], rec[:, 7])
            return (*out, ev) if evals else out
        q = _query_array(points, 3, "closest_points", "points")
        n = q.shape[0]
        md = _per_item(max_d2, n, None, "closest_points", "max_d2", "point")
        rec = np.zeros(n, POINT_HIT_DTYPE)
        ev = np.zeros(n, np.uint32) if evals else None
        ms = C.c_float(0.0)
        check(lib().rt_closest_points(self._handle(), ptr(q), ptr(md), n, int(flags), ptr(rec), ptr(ev),
                                      C.byref(ms) if timing else None))
        out = _point_hit_fields(rec)
        if evals:
            out = (*out, ev)
        return (*out, ms.value) if timing else out

    def closest_points_variant(self) -> int:
        """The traversal the latest closest_points call launched (RT_RAYS_VARIANT_*)."""
        return int(lib().rt_closest_points_variant(self._handle()))

    # ---- path stages for caller hits (rt_path_*) ------------------------------------------------
    def _torch_dev(self):
        import torch

        return torch.device("cuda", self.device)

    def path_begin(self, n: int, seeds=None, stream: Optional[int] = None) -> "PathState":
        """The state of ``n`` paths at the top of TraceRayIterative (rt_path_begin_device): radiance
        0, throughput 1, rng ``seeds`` (n uint32 as an int32 / uint32 tensor or an array; None: 42).
        One launch on ``stream`` (default torch's current stream)."""
        import torch

        dev, n = self._torch_dev(), int(n)
        sd = _seed_tensor(seeds, n, dev, "path_begin")
        st = PathState(torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev),
                       torch.empty(n, dtype=torch.int32, device=dev))
        if n > 0:
            check(lib().rt_path_begin_device(self.device, n, None if sd is None else sd.data_ptr(), C.byref(st.c),
                                             _stream_of(stream, dev)))
        return st

    def path_step(self, rays, hits, state: "PathState", ids=None, materials=None, diffuse_bounce: bool = True,
                  miss_color=(0, 0, 0), flags: int = 0, last: bool = False, direct: bool = False, next_rays=None,
                  stream: Optional[int] = None, vis=None):
        """One depth of TraceRayIterative's loop for ``m`` entries (rt_path_step_device): ``rays``
        (m, 6) float32 and ``hits`` (m, 16) int32, trace_hits' records or the caller's edits of
        them (tri, p, normal and material are read); entry k updates path ``ids[k]`` (int32 tensor,
        unique; None: k; -1: no path) of ``state``.  ``materials``: (m, 13) float32, a material per
        hit, or None for the scene's table entry of the record.  A miss adds throughput *
        ``miss_color``; a hit adds the direct lighting with shadow rays and, unless ``last``, makes
        the bounce.

        Returns ``(next_rays, alive)`` [``, direct`` with ``direct=True``: ShadeDirect's value per
        entry, (m, 3)]: alive (m,) uint8 is 1 where the path goes on with next_rays[k]; a dead entry
        keeps its input ray.  ``next_rays`` may name the output tensor, ``rays`` itself included.
        With ``last`` (a path's last depth) there is no bounce and no draw, and (None, None) is
        returned unless ``next_rays`` is given.  ``flags``: RT_FLAG_BINARY or 0.

        ``vis``: light_visibility's (m, num_lights) float32 tensor.  With it the step casts no
        shadow ray (rt_path_step_vis_device): a light with ``vis[k, l] <= 0`` is skipped and the
        others' terms are scaled by it; ``vis`` of 1 where the shadow ray is clear and 0 where it is
        not gives the plain step bit for bit."""
        import torch

        dev = self._torch_dev()
        if rays.device != dev or rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 6 or not rays.is_contiguous():
            raise ValueError(f"path_step: rays must be a contiguous (m, 6) float32 tensor on {dev}")
        m = rays.shape[0]
        if hits.device != dev or hits.dtype != torch.int32 or tuple(hits.shape) != (m, 16) or not hits.is_contiguous():
            raise ValueError("path_step: hits must be the contiguous (m, 16) int32 tensor of trace_hits")
        if ids is not None and (ids.device != dev or ids.dtype != torch.int32 or tuple(ids.shape) != (m,) or not ids.is_contiguous()):
            raise ValueError("path_step: ids must be a contiguous (m,) int32 tensor")
        if ids is None and m > state.n:
            raise ValueError("path_step: more entries than paths in the state")
        if materials is not None and (materials.device != dev or materials.dtype != torch.float32
                                      or tuple(materials.shape) != (m, 13) or not materials.is_contiguous()):
            raise ValueError("path_step: materials must be a contiguous (m, 13) float32 tensor")
        if next_rays is not None and (next_rays.device != dev or next_rays.dtype != torch.float32
                                      or tuple(next_rays.shape) != (m, 6) or not next_rays.is_contiguous()):
            raise ValueError("path_step: next_rays must be a contiguous (m, 6) float32 tensor")
        want_out = not last or next_rays is not None
        if want_out and next_rays is None:
            next_rays = torch.empty((m, 6), dtype=torch.float32, device=dev)
        alive = torch.empty(m, dtype=torch.uint8, device=dev) if want_out else None
        d = torch.empty((m, 3), dtype=torch.float32, device=dev) if direct else None
        if vis is not None:
            if vis.device != dev or vis.dtype != torch.float32 or tuple(vis.shape) != (m, self.num_lights) or not vis.is_contiguous():
                raise ValueError("path_step: vis must be the contiguous (m, num_lights) float32 tensor of light_visibility")
            if m > 0:
                o = L.PathOpts(1 if diffuse_bounce else 0, _v3(miss_color), int(flags) | (L.RT_PATH_LAST if last else 0))
                check(lib().rt_path_step_vis_device(self._handle(), m, rays.data_ptr(), hits.data_ptr(),
                                                    None if materials is None else materials.data_ptr(),
                                                    None if ids is None else ids.data_ptr(), vis.data_ptr(), C.byref(o),
                                                    C.byref(state.c), None if next_rays is None else next_rays.data_ptr(),
                                                    None if alive is None else alive.data_ptr(),
                                                    None if d is None else d.data_ptr(), _stream_of(stream, dev)))
        elif m > 0:
            o = L.PathOpts(1 if diffuse_bounce else 0, _v3(miss_color), int(flags) | (L.RT_PATH_LAST if last else 0))
            check(lib().rt_path_step_device(self._handle(), m, rays.data_ptr(), hits.data_ptr(),
                                            None if materials is None else materials.data_ptr(),
                                            None if ids is None else ids.data_ptr(), C.byref(o), C.byref(state.c),
                                            None if next_rays is None else next_rays.data_ptr(),
                                            None if alive is None else alive.data_ptr(), None if d is None else d.data_ptr(),
                                            _stream_of(stream, dev)))
        return (next_rays, alive, d) if direct else (next_rays, alive)

    def path_step_variant(self) -> int:
        """The traversal the latest path_step call launched for its shadow rays (RT_RAYS_VARIANT_*)."""
        return int(lib().rt_path_step_variant(self._handle()))

    # ---- soft shadows: spherical area lights for the staged path (rt_light_visibility_*) --------
    @property
    def num_lights(self) -> int:
        """The scene's light count (rt_scene_num_lights)."""
        return int(lib().rt_scene_num_lights(self._handle()))

    def _shape_tensor(self, light_shapes, who: str):
        """light_shapes as the (num_lights, 2) int32 tensor of rt_light_shape records on the scene's
        device: a LIGHT_SHAPE_DTYPE array (or anything np.asarray makes one of), such a tensor, or
        None for point lights."""
        import torch

        dev, nl = self._torch_dev(), self.num_lights
        if _is_torch(light_shapes):
            if light_shapes.device != dev or light_shapes.dtype != torch.int32 or tuple(light_shapes.shape) != (nl, 2) \
                    or not light_shapes.is_contiguous():
                raise ValueError(f"{who}: a light_shapes tensor must be contiguous (num_lights, 2) int32 on {dev}")
            return light_shapes
        a = np.zeros(nl, LIGHT_SHAPE_DTYPE)
        if light_shapes is None:
            a["shadow_samples"] = 1
        else:
            b = np.ascontiguousarray(light_shapes, LIGHT_SHAPE_DTYPE).reshape(-1)
            if b.shape != (nl,):
                raise ValueError(f"{who}: light_shapes must hold one record per scene light")
            a[:] = b
        return torch.from_numpy(a.view(np.int32).reshape(nl, 2).copy()).to(dev)

    def light_visibility(self, hits, state: "PathState", ids=None, light_shapes=None, lanes_per_entry: int = 0,
                         flags: int = 0, stream: Optional[int] = None):
        """The unoccluded fraction of every scene light at every hit (rt_light_visibility_device):
        ``hits`` (m, 16) int32, trace_hits' records; entry k belongs to path ``ids[k]`` (None: k;
        -1: no path) of ``state``, whose rng word the light's disk samples are drawn from and
        which is advanced.  ``light_shapes``: one LIGHT_SHAPE_DTYPE record per light (array, or a
        (num_lights, 2) int32 tensor of the same words); a radius <= 0 is a point light with one
        shadow ray, None means that for all.  ``lanes_per_entry``: 0 (the library chooses) or one
        of LIGHT_VIS_GROUPS; the result does not depend on it.  ``flags``: RT_FLAG_BINARY or 0.
        Returns the (m, num_lights) float32 tensor path_step takes as ``vis``; a miss or an entry
        without a path gets zeros.  The call reads the shapes back, which waits for the stream."""
        import torch

        dev = self._torch_dev()
        if hits.device != dev or hits.dtype != torch.int32 or hits.dim() != 2 or hits.shape[1] != 16 or not hits.is_contiguous():
            raise ValueError("light_visibility: hits must be the contiguous (m, 16) int32 tensor of trace_hits")
        m = hits.shape[0]
        if ids is not None and (ids.device != dev or ids.dtype != torch.int32 or tuple(ids.shape) != (m,) or not ids.is_contiguous()):
            raise ValueError("light_visibility: ids must be a contiguous (m,) int32 tensor")
        if ids is None and m > state.n:
            raise ValueError("light_visibility: more entries than paths in the state")
        sh = self._shape_tensor(light_shapes, "light_visibility")
        nl = self.num_lights
        vis = torch.empty((m, nl), dtype=torch.float32, device=dev)
        st = _stream_of(stream, dev)
        check(lib().rt_light_visibility_device(self._handle(), m, hits.data_ptr(), None if ids is None else ids.data_ptr(),
                                               sh.data_ptr(), state.rng.data_ptr(), int(lanes_per_entry), int(flags),
                                               vis.data_ptr(), st))
        _used_on(st, dev, sh)
        return vis

    def light_visibility_variant(self) -> int:
        """The traversal the latest light_visibility call launched (RT_RAYS_VARIANT_*)."""
        return int(lib().rt_light_visibility_variant(self._handle()))

    def trace_paths(self, rays, seeds=None, max_depth: int = 1, diffuse_bounce: bool = True, miss_color=(0, 0, 0),
                    material_fn=None, compact: bool = True, flags: int = 0, sort=None, light_shapes=None):
        """Radiance of caller rays by stages, on torch's current stream: path_begin, then per depth
        trace_hits -> ``material_fn`` -> path_step -> compact_paths, then path_finish.  With
        ``material_fn=None`` the result is shade_rays' bit for bit.

        ``material_fn(hits, rays, ids, depth)`` gets the depth's records ((m, 16) int32, hit_fields
        names them; it may edit them in place), rays and path ids ((m,) int32; -1: an ended path,
        only without ``compact``) and returns an (m, 13) float32 tensor, a material per hit, or None
        for the scene's table.  ``compact``: the live rays are packed after every depth (one read
        of their count, the one synchronisation per depth); without it every depth runs all n
        entries, the ended ones as no path.  The last depth's step is issued with RT_PATH_LAST;
        ``max_depth <= 0`` returns zeros without a launch.  Returns (n, 3) float32, clamped.

        ``sort`` ("origin", "origin_dir" or True, the measured default): before each depth's
        trace_hits, after the compaction, the current rays and their ids are put into coherence
        order (``sort_rays`` in the scene's ``bounds()``; the ids become the order at the first
        depth).  Nothing is scattered back, the state being indexed by id; ``material_fn`` sees the
        sorted entries with their ids.  The result is the same, bit for bit.

        ``light_shapes`` (one LIGHT_SHAPE_DTYPE record per light): when any radius is positive,
        every depth runs trace_hits -> light_visibility -> path_step(vis=...): soft shadows from
        spherical area lights, the disk samples drawn from each path's own rng before its bounce.
        None, or shapes that are all point lights, leave the stages as they are."""
        import torch

        dev = self._torch_dev()
        if rays.device != dev or rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 6:
            raise ValueError(f"trace_paths: expects an (n, 6) float32 tensor on {dev}")
        n = rays.shape[0]
        if int(max_depth) <= 0 or n == 0:
            return torch.zeros((n, 3), dtype=torch.float32, device=dev)
        state = self.path_begin(n, seeds)
        shapes = None
        if light_shapes is not None:
            sh_host = light_shapes.cpu().numpy().view(np.float32)[:, 0] if _is_torch(light_shapes) \
                else np.ascontiguousarray(light_shapes, LIGHT_SHAPE_DTYPE).reshape(-1)["radius"]
            if bool((sh_host > 0).any()):
                shapes = self._shape_tensor(light_shapes, "trace_paths")
        cur, ids = rays.contiguous(), None
        if sort is False:
            sort = None
        box = None if sort is None else self.bounds()
        for depth in range(int(max_depth)):
            last = depth + 1 == int(max_depth)
            if sort is not None:
                cur, order = sort_rays(cur, box, SORT_DEFAULT if sort is True else sort)
                ids = order if ids is None else gather(ids, order)
            hits = self.trace_hits(cur, flags)
            mats = None
            if material_fn is not None:
                shown = ids if ids is not None else torch.arange(n, dtype=torch.int32, device=dev)
                mats = material_fn(hits, cur, shown, depth)
                if mats is not None:
                    mats = mats.to(dtype=torch.float32).contiguous()
            vis = None if shapes is None else self.light_visibility(hits, state, ids, shapes, flags=flags)
            nxt, alive = self.path_step(cur, hits, state, ids, mats, diffuse_bounce, miss_color, flags, last=last, vis=vis)
            if last:
                break
            if compact:
                cur, ids, count = compact_paths(alive, nxt, ids)
                if count == 0:
                    break
            else:
                own = ids if ids is not None else torch.arange(n, dtype=torch.int32, device=dev)
                cur, ids = nxt, torch.where(alive != 0, own, torch.full_like(own, -1))
        return path_finish(state)

    def faults(self, clear: bool = True) -> int:
        """RT_FAULT_* bits the device guards raised since the last clear (rt_scene_faults)."""
        f = C.c_uint32()
        check(lib().rt_scene_faults(self._handle(), C.byref(f), 1 if clear else 0))
        return f.value

    def close(self) -> None:
        if self._h and self._owned:
            lib().rt_scene_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Renderer:
    """render(scene, camera) -> frame in host memory on 1..N GPUs (rt_renderer, include/rt_mi355x.h).

    Every rank renders its 8-row bands (band b -> rank b % world) into a device strip with the
    fused P6 epilogue; the strips reach the host frame band by band, pipelined `depth` frames
    deep: each GPU over its own PCIe link (RT_GATHER_DIRECT in one process; RT_GATHER_HOST_SHARED
    across processes, into the shared-memory frame ``host_frame_name``), or over RCCL to rank 0
    first (RT_GATHER_RCCL).  ``devices``: the GPUs this process drives;
    ``world_size``/``rank0``/``unique_id`` join a multi-process job (one process per GPU): rank
    0's process makes the RCCL id with :func:`comm_unique_id` and shares it.
    """

    def __init__(self, num_triangles: int, nodes, aabbs, triangles, tri_object_ids=None, materials=None,
                 lights=None, devices=(0,), world_size: int = 0, rank0: int = 0, unique_id: bytes = None,
                 band_rows: int = 8, deliver: int = L.RT_DELIVER_P6, gather: int = L.RT_GATHER_AUTO,
                 depth: int = 3, flags: int = 0, host_frame_name: Optional[str] = None):
        P = int(num_triangles)
        keep = [_c(nodes, np.uint32), _c(aabbs, np.float32), _c(triangles, np.float32)]
        objs = None if tri_object_ids is None else _c(tri_object_ids, np.int32)
        mats = None if materials is None else _c(materials, np.float32).reshape(-1, 13)
        lts = None if lights is None else np.ascontiguousarray(lights, dtype=LIGHT_DTYPE)
        devs = np.ascontiguousarray(list(devices), np.int32)
        o = L.RendererOpts()
        lib().rt_renderer_opts_default(C.byref(o))
        o.n_devices, o.devices = len(devs), devs.ctypes.data
        o.world_size, o.rank0 = int(world_size), int(rank0)
        uid = None
        if unique_id is not None:
            uid = C.create_string_buffer(bytes(unique_id), 128)
            o.unique_id = C.addressof(uid)
        o.band_rows, o.deliver, o.gather, o.depth, o.flags = int(band_rows), int(deliver), int(gather), int(depth), int(flags)
        name = None
        if host_frame_name:
            name = C.create_string_buffer(str(host_frame_name).encode())
            o.host_frame_name = C.addressof(name)
        h = C.c_void_p()
        check(lib().rt_renderer_create(P, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(objs), ptr(mats),
                                       0 if mats is None else mats.shape[0], ptr(lts),
                                       0 if lts is None else lts.shape[0], C.byref(o), C.byref(h)))
        self._h = h
        self._name = name
        self._borrowed = []  # DeviceScene views of this renderer's scenes (invalidated by close)
        self.num_triangles = P
        self.deliver = int(deliver)
        self.world = int(world_size) or len(devs)
        self.rank0 = int(rank0)

    @classmethod
    def from_host(cls, hs: HostScene, **kw) -> "Renderer":
        return cls(hs.num_triangles, hs.nodes, hs.aabbs, hs.triangles, hs.tri_object_ids, hs.materials,
                   hs.lights, **kw)

    @property
    def copy_engine(self) -> str:
        """"sdma" (copies queued through the HSA runtime on a DMA engine) or "runtime" (HIP's)."""
        return "sdma" if lib().rt_renderer_copy_engine(self._h) else "runtime"

    @property
    def local_ranks(self) -> int:
        return int(lib().rt_renderer_local_ranks(self._h))

    def scene(self, i: int = 0) -> DeviceScene:
        """Local rank i's device scene (frame/kernel timing queries)."""
        h = lib().rt_renderer_scene(self._h, int(i))
        if not h:
            raise L.RTError(-1, f"no local rank {i}")
        v = DeviceScene._borrow(h, self.num_triangles, self)
        self._borrowed.append(v)
        return v

    def submit(self, camera: Camera, opts) -> int:
        t = C.c_uint64()
        check(lib().rt_renderer_submit(self._h, C.byref(camera.c), C.byref(opts), C.byref(t)))
        return t.value

    def submit_pair(self, camera_a: Camera, camera_b: Camera, opts) -> tuple:
        """Two frames, one render launch per local rank (rt_renderer_submit_pair): their tickets."""
        t = C.c_uint64()
        check(lib().rt_renderer_submit_pair(self._h, C.byref(camera_a.c), C.byref(camera_b.c), C.byref(opts),
                                            C.byref(t)))
        return t.value, t.value + 1

    def wait(self, ticket: int):
        """(address, bytes) of the delivered frame on rank 0's process, else (None, 0)."""
        f, n = C.c_void_p(), C.c_size_t()
        check(lib().rt_renderer_wait(self._h, int(ticket), C.byref(f), C.byref(n)))
        return f.value, n.value

    def render(self, camera: Camera, spp: int = 1, max_depth: int = 1, diffuse_bounce: bool = True,
               miss_color=(0, 0, 0), jitter=None, kernel: int = L.RT_KERNEL_AUTO, flags: int = 0):
        """One synchronous frame: (H, W, 3) uint8 P6 samples or float32 (rank 0; None elsewhere)."""
        o, _jit = DeviceScene.make_opts(spp, max_depth, diffuse_bounce, miss_color, jitter, kernel=kernel, flags=flags)
        W, H = camera.pixel_width, camera.pixel_height
        f32 = self.deliver == L.RT_DELIVER_F32
        out = np.zeros((H, W, 3), np.float32 if f32 else np.uint8)
        check(lib().rt_renderer_render(self._h, C.byref(camera.c), C.byref(o), ptr(out), out.nbytes))
        return out if self.rank0 == 0 and self.deliver != L.RT_DELIVER_NONE else None

    def times(self, kind: int, max_frames: int = 256) -> np.ndarray:
        out = np.zeros(max_frames, np.float32)
        n = C.c_int()
        check(lib().rt_renderer_times(self._h, int(kind), ptr(out), int(max_frames), C.byref(n)))
        return out[:n.value]

    def close(self) -> None:
        for v in getattr(self, "_borrowed", []):
            v._h = C.c_void_p()
        self._borrowed = []
        if self._h:
            lib().rt_renderer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def comm_unique_id() -> bytes:
    """128-byte RCCL unique id for a multi-process Renderer (made on rank 0's process)."""
    b = C.create_string_buffer(128)
    check(lib().rt_comm_unique_id(b))
    return b.raw


def render(numTriangles, W, H, cam: Camera, missColor, max_depth, spp, nodes, aabbs, triangles,
           triObjectIds, objectMaterials, numObjectMaterials, lights, numLights, diffuse_bounce, output,
           n_gpus: int = 1):
    """The reference entry point (G/include/query.h:13-29) with host arrays; fills ``output``
    (H*W*3 float32, row-major, row 0 = top) like the CPU branch of query.cu:130-166.
    n_gpus > 1 shards the bands over GPUs 0..n_gpus-1 (rt_render_reference_gpus)."""
    out = np.asarray(output)
    if out.dtype != np.float32 or not out.flags.c_contiguous or out.size != W * H * 3:
        raise ValueError("output must be a contiguous float32 array of W*H*3")
    mats = _c(objectMaterials, np.float32).reshape(-1, 13)[:numObjectMaterials]
    lts = np.ascontiguousarray(lights, dtype=LIGHT_DTYPE)[:numLights]
    nd, ab, tr = _c(nodes, np.uint32), _c(aabbs, np.float32), _c(triangles, np.float32)
    ob = None if triObjectIds is None else _c(triObjectIds, np.int32)
    args = (int(numTriangles), int(W), int(H), C.byref(cam.c), _v3(missColor), int(max_depth), int(spp), ptr(nd),
            ptr(ab), ptr(tr), ptr(ob), ptr(mats), int(numObjectMaterials), ptr(lts), int(numLights),
            1 if diffuse_bounce else 0)
    if n_gpus == 1:
        check(lib().rt_render_reference(*args, ptr(out)))
    else:
        check(lib().rt_render_reference_gpus(*args, int(n_gpus), ptr(out)))
    return out


RT_HW1_BRUTE = 1


def render_hw1(positions, normals, indices, camera: Camera, light_position, light_color, spp: int = 1,
               jitter=None, aov: bool = False, device: int = 0, brute: bool = False, timing: bool = False):
    """HW1 path on the GPU (HW1/src/render.cpp:72-116 semantics): (H, W, 3) float32 [+ per-sample
    winning triangle / t] [+ device ms of the kernels when ``timing``].  ``brute`` runs every
    triangle for every ray; the default skips triangles outside their conservative pixel
    rectangle (same output bit for bit, see rt_render_hw1_ex)."""
    pos, nrm, idx = _c(positions, np.float32), _c(normals, np.float32), _c(indices, np.uint32)
    W, H = camera.pixel_width, camera.pixel_height
    rgb = np.zeros((H, W, 3), np.float32)
    hi = ht = None
    if aov:
        hi = np.zeros((H, W, spp), np.int32)
        ht = np.zeros((H, W, spp), np.float32)
    jit = None if jitter is None else _c(jitter, np.float32).reshape(-1)
    ms = C.c_float(0.0)
    check(lib().rt_render_hw1_ex(int(device), ptr(pos), ptr(nrm), ptr(idx), idx.size // 3, C.byref(camera.c),
                                 _v3(light_position), _v3(light_color), int(spp), ptr(jit),
                                 RT_HW1_BRUTE if brute else 0, ptr(rgb), ptr(hi), ptr(ht),
                                 C.byref(ms) if timing else None))
    out = (rgb, hi, ht) if aov else (rgb,)
    if timing:
        out = out + (ms.value,)
    return out if len(out) > 1 else out[0]


def hw1_rects_host(positions, indices, camera: Camera):
    """Host build of the binned HW1 path's per-triangle bounds (rt_hw1_rects_host; no device):
    rects (P, 4) int32 (ix_lo, iy_lo, ix_hi, iy_hi) and tiles (P, 4) int32 (tx0, tx1, ty0, ty1),
    the inclusive range of 16x4-pixel tiles the triangle is listed in; empty: tx1 < tx0."""
    pos, idx = _c(positions, np.float32), _c(indices, np.uint32)
    n = idx.size // 3
    rects, tiles = np.zeros((n, 4), np.int32), np.zeros((n, 4), np.int32)
    check(lib().rt_hw1_rects_host(C.byref(camera.c), ptr(pos), ptr(idx), n, ptr(rects), ptr(tiles)))
    return rects, tiles


class HW1Scene:
    """A HW1 mesh resident on one MI355X (rt_hw1_scene): repeated frames of the HW1 path
    (HW1/src/render.cpp:72-116) without re-uploading it."""

    def __init__(self, positions, normals, indices, device: int = 0):
        pos, nrm, idx = _c(positions, np.float32), _c(normals, np.float32), _c(indices, np.uint32)
        h = C.c_void_p()
        check(lib().rt_hw1_scene_create(int(device), ptr(pos), ptr(nrm), ptr(idx), idx.size // 3, C.byref(h)))
        self._h = h
        self.device = device

    def render_device(self, camera: Camera, light_position, light_color, spp: int = 1, rgb_ptr=None, p6_ptr=None,
                      hit_idx_ptr=None, hit_t_ptr=None, stream=None, jitter=None, brute: bool = False) -> None:
        """One frame into device buffers (raw pointers) on a HIP stream (handle), asynchronously."""
        jit = None if jitter is None else _c(jitter, np.float32).reshape(-1)
        check(lib().rt_render_hw1_device(self._h, C.byref(camera.c), _v3(light_position), _v3(light_color), int(spp),
                                         ptr(jit), RT_HW1_BRUTE if brute else 0, rgb_ptr, p6_ptr, hit_idx_ptr,
                                         hit_t_ptr, stream))

    def render_deliver(self, camera: Camera, light_position, light_color, spp: int, host_p6_ptr: int, stream=None,
                       brute: bool = False) -> int:
        """One frame's P6 body (write_p6 defaults) delivered to host memory at host_p6_ptr
        (W*H*3 bytes, pinned) by the scene's own copy stream, overlapping the next frames'
        kernels (rt_render_hw1_deliver); returns the frame's ticket for wait()."""
        t = C.c_uint64()
        check(lib().rt_render_hw1_deliver(self._h, C.byref(camera.c), _v3(light_position), _v3(light_color), int(spp),
                                          RT_HW1_BRUTE if brute else 0, host_p6_ptr, stream, C.byref(t)))
        return int(t.value)

    def wait(self, ticket: int) -> None:
        check(lib().rt_hw1_wait(self._h, int(ticket)))

    def kernel_times(self, max_frames: int = 64) -> np.ndarray:
        out = np.zeros(max_frames, np.float32)
        n = C.c_int()
        check(lib().rt_hw1_kernel_times(self._h, ptr(out), max_frames, C.byref(n)))
        return out[:n.value]

    def kernel_name(self) -> str:
        return lib().rt_hw1_kernel_name(self._h).decode()

    def list_info(self) -> tuple:
        """(bin-list capacity now, the latest frame's list total)."""
        info = (C.c_int64 * 2)()
        check(lib().rt_hw1_list_info(self._h, info))
        return int(info[0]), int(info[1])

    def bins(self) -> dict:
        """The binning state of the latest render_device frame (rt_hw1_debug_bins; waits for it):
        rects (P, 4) int32, offsets (tiles + 1) uint32, list (min(total, capacity)) uint32, total,
        complete (False: the total exceeded the capacity, so some tiles' lists were not written)."""
        info = (C.c_int64 * 4)()
        check(lib().rt_hw1_debug_bins(self._h, info, None, None, 0, None, 0))
        n, tiles, total = int(info[0]), int(info[1]), int(info[2])
        rects = np.zeros((n, 4), np.int32)
        offsets = np.zeros(tiles + 1, np.uint32)
        lst = np.zeros(total, np.uint32)  # (at least the entries written)
        check(lib().rt_hw1_debug_bins(self._h, info, ptr(rects), ptr(offsets), offsets.size, ptr(lst), lst.size))
        written = total if info[3] else min(total, self.list_info()[0])
        return {"rects": rects, "offsets": offsets, "list": lst[:written], "total": int(info[2]),
                "complete": bool(info[3])}

    def close(self) -> None:
        if self._h:
            lib().rt_hw1_scene_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def intersect_rays(triangle18, dirs, origin=(0.0, 0.0, 0.0), hw1: bool = True, tmin: float = 0.0,
                   tmax: float = 3.4028234663852886e38, device: int = 0):
    """Device Möller–Trumbore over a batch of rays against one triangle (v0,v1,v2,n0,n1,n2 as 18
    floats): HW1 ray_intersection semantics when hw1, else G/ intersectTriangle with [tmin, tmax]."""
    tri = L.Triangle.from_buffer_copy(_c(triangle18, np.float32).tobytes())
    d = _c(dirs, np.float32).reshape(-1, 3)
    n = d.shape[0]
    hit = np.zeros(n, np.int32)
    t = np.zeros(n, np.float32)
    check(lib().rt_intersect_rays(int(device), C.byref(tri), _f3(origin), ptr(d), n, 1 if hw1 else 0,
                                  float(tmin), float(tmax), ptr(hit), ptr(t)))
    return hit, t


def hit_record_host(rays, tris) -> np.ndarray:
    """Host build of the hit record's arithmetic (rt_hit_record_host, no device): record i is
    intersectTriangle(rays[i], tris[i], 1e-4, FLT_MAX) in full.  ``rays`` (n, 6), ``tris`` (n, 18)
    float32 (v0, v1, v2, n0, n1, n2); returns (n,) HIT_DTYPE with tri = i on a hit, object_id and
    material -1."""
    r, t = _c(rays, np.float32), _c(tris, np.float32)
    if r.ndim != 2 or r.shape[1] != 6 or t.shape != (r.shape[0], 18):
        raise ValueError("hit_record_host: expects (n, 6) rays and (n, 18) triangles")
    out = np.zeros(r.shape[0], HIT_DTYPE)
    check(lib().rt_hit_record_host(ptr(r), ptr(t), r.shape[0], ptr(out)))
    return out


def multi_hits_host(nodes, aabbs, triangles, rays, k: int, max_t=None):
    """Host build of DeviceScene.trace_multi_hits (rt_multi_hits_host, no device) on arrays in the
    reference layout: ``nodes`` (2P-1, 4) uint32, ``aabbs`` (2P-1, 6), ``triangles`` (P, 18), ``rays``
    (n, 6) float32, ``max_t`` (n,) float32 or None (FLT_MAX).  The reference's 512-entry stack and
    its overflow rule included.  Returns ``(count, tri, t, u, v)`` as the numpy path of
    trace_multi_hits does."""
    nd, bx, tr, r = _c(nodes, np.uint32), _c(aabbs, np.float32), _c(triangles, np.float32), _c(rays, np.float32)
    P = tr.size // 18
    k = int(k)
    if P == 0 or nd.size != 4 * (2 * P - 1) or bx.size != 6 * (2 * P - 1):
        raise ValueError("multi_hits_host: expects 2P-1 nodes and boxes for P >= 1 triangles")
    if r.ndim != 2 or r.shape[1] != 6:
        raise ValueError("multi_hits_host: expects an (n, 6) array of origins and directions")
    if not 0 <= k <= L.RT_MULTI_HIT_MAX_K:
        raise ValueError(f"multi_hits_host: k must be in 0..{L.RT_MULTI_HIT_MAX_K}")
    n = r.shape[0]
    mt = None
    if max_t is not None:
        mt = _c(max_t, np.float32)
        if mt.shape != (n,):
            raise ValueError("multi_hits_host: max_t must hold one float per ray")
    count = np.zeros(n, np.int32)
    rec = np.zeros((n, k), MULTI_HIT_DTYPE)
    check(lib().rt_multi_hits_host(P, ptr(nd), ptr(bx), ptr(tr), ptr(r), ptr(mt), n, k, ptr(rec) if k > 0 else None,
                                   ptr(count)))
    return count, rec["tri"], rec["t"], rec["u"], rec["v"]


def _point_hit_fields(rec: np.ndarray):
    """(tri, d2, p, v, w, region) of a POINT_HIT_DTYPE array, each contiguous."""
    return tuple(np.ascontiguousarray(rec[f]) for f in ("tri", "d2", "p", "v", "w", "region"))


def closest_points_host(nodes, aabbs, triangles, points, max_d2=None, evals: bool = False):
    """Host build of DeviceScene.closest_points (rt_closest_points_host, no device) and its
    definition: the brute force over the leaves in index order, on arrays in the reference layout:
    ``nodes`` (2P-1, 4) uint32, ``aabbs`` (2P-1, 6), ``triangles`` (P, 18), ``points`` (n, 3) float32,
    ``max_d2`` (n,) float32 or None (+inf).  Returns ``(tri, d2, p, v, w, region)`` as the numpy path
    of closest_points does; ``evals=True`` appends the number of leaves that name a triangle, per
    point."""
    nd, bx, tr, q = _c(nodes, np.uint32), _c(aabbs, np.float32), _c(triangles, np.float32), _c(points, np.float32)
    P = tr.size // 18
    if P == 0 or nd.size != 4 * (2 * P - 1) or bx.size != 6 * (2 * P - 1):
        raise ValueError("closest_points_host: expects 2P-1 nodes and boxes for P >= 1 triangles")
    if q.ndim != 2 or q.shape[1] != 3:
        raise ValueError("closest_points_host: expects an (n, 3) array of points")
    n = q.shape[0]
    md = None
    if max_d2 is not None:
        md = _c(max_d2, np.float32)
        if md.shape != (n,):
            raise ValueError("closest_points_host: max_d2 must hold one float per point")
    rec = np.zeros(n, POINT_HIT_DTYPE)
    ev = np.zeros(n, np.uint32) if evals else None
    check(lib().rt_closest_points_host(P, ptr(nd), ptr(bx), ptr(tr), ptr(q), ptr(md), n, ptr(rec), ptr(ev)))
    out = _point_hit_fields(rec)
    return (*out, ev) if evals else out


# rt_hit's 32-bit words by field: (first word, words, float)
_HIT_WORDS = {"tri": (0, 1, False), "t": (1, 1, True), "u": (2, 1, True), "v": (3, 1, True), "p": (4, 3, True),
              "normal": (7, 3, True), "geom_normal": (10, 3, True), "front_face": (13, 1, False),
              "object_id": (14, 1, False), "material": (15, 1, False)}


def hit_fields(hits) -> dict:
    """Named views (no copies) of the (n, 16) int32 tensor DeviceScene.trace_hits returns on the
    device path: int32 (n,) for tri, front_face, object_id and material, float32 (n,) for t, u and
    v, float32 (n, 3) for p, normal and geom_normal."""
    import torch

    if hits.dtype != torch.int32 or hits.dim() != 2 or hits.shape[1] != 16:
        raise ValueError("hit_fields: expects the (n, 16) int32 tensor of trace_hits")
    out = {}
    for name, (w, k, is_float) in _HIT_WORDS.items():
        v = hits[:, w] if k == 1 else hits[:, w:w + k]
        out[name] = v.view(torch.float32) if is_float else v
    return out


def camera_rays(camera: Camera, spp: int = 1, jitter=None, row0: int = 0, rows: Optional[int] = None,
                device: Optional[int] = None, stream: Optional[int] = None, sample0: int = 0):
    """The camera rays of image rows [row0, row0 + rows) (default: to the last row) and their rng
    seeds, as render() makes them (rt_camera_rays_host / rt_camera_rays_device): ray
    ((y - row0) * W + x) * spp + s is sample s of pixel (x, y), Camera::get_ray of
    (x + jitter[s, 0], y + jitter[s, 1]); its seed is make_rng_seed(x, y, s).  ``jitter``: (spp, 2)
    float32, None for jittered_samples(spp).

    ``device=None``: the host build, numpy ``(rays (n, 6) float32, seeds (n,) uint32)``.  An int
    device: one launch on ``stream`` of that device (a HIP stream handle; default torch's current
    stream), torch tensors ``(rays (n, 6) float32, seeds (n,) int32)``, the seeds' 32 bits as
    DeviceScene.shade_rays takes them; nothing passes through the host but the jitter table.

    ``sample0`` > 0: one sample pass of a longer frame (rt_camera_rays_pass_*): the ``spp`` samples
    are samples [sample0, sample0 + spp) of the frame's, ``jitter`` is that slice of the frame's
    table (required) and the seeds are make_rng_seed(x, y, sample0 + s)."""
    spp, sample0 = int(spp), int(sample0)
    if sample0 != 0 and jitter is None:
        raise ValueError("camera_rays: a pass with sample0 != 0 needs its slice of the jitter table")
    H = camera.pixel_height
    if rows is None:
        rows = H - int(row0)
    n = max(camera.pixel_width * int(rows) * spp, 0) if 0 <= int(rows) <= H and spp >= 1 else 0
    jit = None
    if jitter is not None:
        jit = _c(jitter, np.float32).reshape(-1)
        if jit.size != 2 * spp:
            raise ValueError("camera_rays: jitter must hold (spp, 2) floats")
    if device is None:
        rays = np.zeros((n, 6), np.float32)
        seeds = np.zeros(n, np.uint32)
        if sample0 != 0:
            check(lib().rt_camera_rays_pass_host(C.byref(camera.c), sample0, spp, ptr(jit), int(row0), int(rows), ptr(rays),
                                                 ptr(seeds)))
        else:
            check(lib().rt_camera_rays_host(C.byref(camera.c), spp, ptr(jit), int(row0), int(rows), ptr(rays), ptr(seeds)))
        return rays, seeds
    import torch

    dev = torch.device("cuda", int(device))
    if jit is None:
        jit = jittered_samples(spp).reshape(-1)
    cur = torch.cuda.current_stream(dev)
    jd = torch.from_numpy(jit).to(dev)  # on torch's current stream
    # (an empty tensor has no address: one spare element keeps the C checks' answers the same)
    rays = torch.empty((max(n, 1), 6), dtype=torch.float32, device=dev)[:n]
    seeds = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    foreign = stream is not None and stream != cur.cuda_stream
    if foreign:  # the table must be there before the launch is queued on the caller's stream
        cur.synchronize()
    st = stream if foreign else cur.cuda_stream
    if sample0 != 0:
        check(lib().rt_camera_rays_pass_device(int(device), C.byref(camera.c), sample0, spp, jd.data_ptr(), int(row0),
                                               int(rows), rays.data_ptr(), seeds.data_ptr(), st))
    else:
        check(lib().rt_camera_rays_device(int(device), C.byref(camera.c), spp, jd.data_ptr(), int(row0), int(rows),
                                          rays.data_ptr(), seeds.data_ptr(), st))
    if foreign:  # ... and stay until that launch has read it
        jd.record_stream(torch.cuda.ExternalStream(stream, device=dev))
    return rays, seeds


class Film:
    """Per-pixel float sums of radiance samples on one device (rt_film): the last step of a frame
    made from caller rays.  ``add`` adds samples in order as render() does (col = col + sample),
    ``resolve`` gives render()'s pixels float(double(col) / double(float(count))) and write_p6's
    bytes; camera_rays -> shade_rays -> add -> resolve is DeviceScene.render's frame bit for bit,
    in one pass or in sample passes and row bands.  Every call is one launch on ``stream`` (a HIP
    stream handle; default torch's current stream) with no host synchronisation."""

    def __init__(self, width: int, height: int, device: int = 0):
        h = C.c_void_p()
        check(lib().rt_film_create(int(device), int(width), int(height), C.byref(h)))
        self._h = h
        self.width, self.height, self.device = int(width), int(height), int(device)

    def _handle(self) -> C.c_void_p:
        if not self._h:
            raise L.RTError(-1, "film is closed")
        return self._h

    def _stream(self, stream):
        import torch

        return _stream_of(stream, torch.device("cuda", self.device))

    def add(self, radiance, row0: int = 0, rows: Optional[int] = None, nsamples: Optional[int] = None,
            stream: Optional[int] = None) -> None:
        """Add ``nsamples`` samples per pixel of rows [row0, row0 + rows) (default: to the last row):
        ``radiance`` is a float32 tensor on the film's device of rows*W*nsamples*3 elements, sample s
        of pixel (x, y) at ((y - row0) * W + x) * nsamples + s, the order of camera_rays and of
        shade_rays' output.  ``nsamples`` None: what the tensor's size gives."""
        import torch

        if rows is None:
            rows = self.height - int(row0)
        dev = torch.device("cuda", self.device)
        if radiance.device != dev or radiance.dtype != torch.float32:
            raise ValueError(f"Film.add: expects a float32 tensor on {dev}")
        radiance = radiance.contiguous()
        px = self.width * int(rows) * 3
        if nsamples is None:
            nsamples = radiance.numel() // px if px > 0 else 1
        if radiance.numel() != px * int(nsamples):
            raise ValueError("Film.add: radiance must hold rows * W * nsamples * 3 floats")
        # (an empty tensor has no address: the C checks still answer for rows == 0)
        p = radiance.data_ptr() if radiance.numel() else torch.empty(1, dtype=torch.float32, device=dev).data_ptr()
        check(lib().rt_film_add_device(self._handle(), p, int(row0), int(rows), int(nsamples), self._stream(stream)))

    def resolve(self, row0: int = 0, rows: Optional[int] = None, p6: bool = False, stream: Optional[int] = None):
        """The pixels of rows [row0, row0 + rows) from the sums so far: a (rows, W, 3) float32
        tensor, or with ``p6=True`` ``(rgb, bytes)``, bytes a (rows, W, 3) uint8 tensor of P6
        samples (write_p6 defaults).  The rows must hold the same, non-zero number of samples.
        Does not clear."""
        import torch

        if rows is None:
            rows = self.height - int(row0)
        dev = torch.device("cuda", self.device)
        shape = (max(int(rows), 0), self.width, 3)
        rgb = torch.empty(shape, dtype=torch.float32, device=dev)
        b = torch.empty(shape, dtype=torch.uint8, device=dev) if p6 else None
        spare = torch.empty(1, dtype=torch.float32, device=dev) if rgb.numel() == 0 else None
        check(lib().rt_film_resolve_device(self._handle(), int(row0), int(rows),
                                           rgb.data_ptr() if spare is None else spare.data_ptr(),
                                           None if b is None or spare is not None else b.data_ptr(), self._stream(stream)))
        return (rgb, b) if p6 else rgb

    def clear(self, stream: Optional[int] = None) -> None:
        """Sums and every row's sample count to 0."""
        check(lib().rt_film_clear_device(self._handle(), self._stream(stream)))

    def row_samples(self, row: int) -> int:
        """Samples added to that row since the film was made or cleared."""
        n = C.c_int64()
        check(lib().rt_film_row_samples(self._handle(), int(row), C.byref(n)))
        return int(n.value)

    def close(self) -> None:
        if self._h:
            lib().rt_film_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def camera_rays_pixels(camera: Camera, pixels, counts, nsamples: int, jitter, device: Optional[int] = None,
                       stream: Optional[int] = None):
    """Camera rays for a list of pixels (rt_camera_rays_pixels_host / _device): ``pixels`` holds m
    indices y * W + x in any order (None: every pixel in order), ``counts`` the W * H samples each
    pixel already has (None: 0), and ray k * nsamples + s is sample ``counts[pixels[k]] + s`` of
    that pixel, Camera::get_ray with that row of ``jitter`` and the seed make_rng_seed(x, y,
    counts + s).  ``jitter``: the whole frame's table, (table_spp, 2) float32, or an int table_spp
    for jittered_samples(table_spp).  An index >= W * H (RT_PIXEL_NONE) gives origin = center,
    direction 0, seed 0; a sample past the table reads its last row.

    ``device=None``: the host build over numpy arrays (uint32 ``pixels`` and ``counts``), numpy
    ``(rays (m*nsamples, 6) float32, seeds (m*nsamples,) uint32)``.  An int device: one launch on
    ``stream`` of that device (default torch's current stream); ``pixels`` and ``counts`` are int32
    tensors there (the words' 32 bits; ``counts`` may be an AdaptiveFilm, for its count map),
    ``jitter`` may be a float32 tensor there as well, and torch tensors ``(rays, seeds (int32))``
    are returned with no host synchronisation."""
    nsamples = int(nsamples)
    W, H = camera.pixel_width, camera.pixel_height
    if device is None:
        px = None if pixels is None else _c(pixels, np.uint32).reshape(-1)
        ct = None if counts is None else _c(counts, np.uint32).reshape(-1)
        if ct is not None and ct.size != W * H:
            raise ValueError("camera_rays_pixels: counts must hold W * H words")
        m = W * H if px is None else px.size
        if isinstance(jitter, (int, np.integer)):
            jit, table = None, int(jitter)
        else:
            jit = _c(jitter, np.float32).reshape(-1)
            if jit.size % 2 != 0:
                raise ValueError("camera_rays_pixels: jitter must hold (table_spp, 2) floats")
            table = jit.size // 2
        n = m * max(nsamples, 0)
        rays = np.zeros((max(n, 1), 6), np.float32)[:n]
        seeds = np.zeros(max(n, 1), np.uint32)[:n]
        check(lib().rt_camera_rays_pixels_host(C.byref(camera.c), ptr(px), m, ptr(ct), nsamples, ptr(jit), table, ptr(rays),
                                               ptr(seeds)))
        return rays, seeds
    import torch

    dev = torch.device("cuda", int(device))

    def words(a, who):
        if a is None:
            return None
        if not _is_torch(a):
            a = torch.from_numpy(_c(a, np.uint32).view(np.int32)).to(dev)
        if a.device != dev or a.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
            raise ValueError(f"camera_rays_pixels: {who} must be an int32 or uint32 tensor on {dev}")
        return a.contiguous().view(-1)

    cur = torch.cuda.current_stream(dev)
    foreign = stream is not None and stream != cur.cuda_stream
    px = words(pixels, "pixels")
    m = W * H if px is None else px.numel()
    if isinstance(counts, AdaptiveFilm):
        if (counts.width, counts.height, counts.device) != (W, H, int(device)):
            raise ValueError("camera_rays_pixels: the film is not of the camera's size on that device")
        ct, cp = None, counts._counts_ptr()
    else:
        ct = words(counts, "counts")
        if ct is not None and ct.numel() != W * H:
            raise ValueError("camera_rays_pixels: counts must hold W * H words")
        cp = None if ct is None else ct.data_ptr()
    if isinstance(jitter, (int, np.integer)):
        jitter = jittered_samples(int(jitter))
    if _is_torch(jitter):
        if jitter.device != dev or jitter.dtype != torch.float32 or jitter.numel() % 2 != 0:
            raise ValueError(f"camera_rays_pixels: jitter must be a (table_spp, 2) float32 tensor on {dev}")
        jd = jitter.contiguous()
    else:
        jit = _c(jitter, np.float32).reshape(-1)
        if jit.size % 2 != 0:
            raise ValueError("camera_rays_pixels: jitter must hold (table_spp, 2) floats")
        jd = torch.from_numpy(jit).to(dev)  # on torch's current stream
    table = jd.numel() // 2
    n = m * max(nsamples, 0)
    # (an empty tensor has no address: one spare element keeps the C checks' answers the same)
    rays = torch.empty((max(n, 1), 6), dtype=torch.float32, device=dev)[:n]
    seeds = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    spare = torch.empty(2, dtype=torch.float32, device=dev) if table == 0 else None
    if foreign:  # what was made on torch's stream must be there before the caller's stream reads it
        cur.synchronize()
    st = stream if foreign else cur.cuda_stream
    check(lib().rt_camera_rays_pixels_device(C.byref(camera.c), None if px is None or m == 0 else px.data_ptr(), m, cp,
                                             nsamples, jd.data_ptr() if spare is None else spare.data_ptr(), table,
                                             rays.data_ptr(), seeds.data_ptr(), int(device), st))
    if foreign:  # ... and stay until that launch has read it
        ext = torch.cuda.ExternalStream(stream, device=dev)
        for t in (jd, px, ct):
            if t is not None:
                t.record_stream(ext)
    return rays, seeds


class _DeviceWords:
    """W * H 32-bit words of device memory owned by a native object, for torch.as_tensor."""

    def __init__(self, address: int, n: int, owner):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (address, False), "version": 2,
                                         "strides": None}


class AdaptiveFilm:
    """A film with a sample count per pixel (rt_afilm): per pixel render()'s three float sums, a
    count, and two float moments of the sample luminance, 24 bytes, all on the device.  ``add``
    puts samples onto listed pixels in order, ``resolve`` divides every pixel by its own count,
    ``select`` names the pixels whose mean is still uncertain.  Fed each pixel's samples 0, 1, ...
    in order (camera_rays_pixels with this film's counts), a pixel with c samples is render(spp=c)'s
    pixel bit for bit.  Calls are launches on ``stream`` (a HIP stream handle; default torch's
    current stream) with no host synchronisation, select's returned count excepted."""

    def __init__(self, width: int, height: int, device: int = 0):
        h = C.c_void_p()
        check(lib().rt_afilm_create(int(device), int(width), int(height), C.byref(h)))
        self._h = h
        self.width, self.height, self.device = int(width), int(height), int(device)
        self._scratch = None
        self._count = None

    def _handle(self) -> C.c_void_p:
        if not self._h:
            raise L.RTError(-1, "film is closed")
        return self._h

    def _dev(self):
        import torch

        return torch.device("cuda", self.device)

    def _counts_ptr(self) -> int:
        return int(lib().rt_afilm_counts_device(self._handle()))

    @property
    def counts(self):
        """The (W*H,) int32 tensor view of the film's per-pixel sample counts: the device memory
        itself, valid until close() and changed by add and clear in stream order."""
        import torch

        return torch.as_tensor(_DeviceWords(self._counts_ptr(), self.width * self.height, self), device=self._dev())

    def add(self, radiance, pixels=None, nsamples: Optional[int] = None, stream: Optional[int] = None) -> None:
        """Add ``nsamples`` samples to each listed pixel: ``pixels`` an (m,) int32 tensor of indices
        y * W + x, unique within the call (None: every pixel in order; an index outside the image
        is skipped), ``radiance`` a float32 tensor of m*nsamples*3 elements, sample s of entry k at
        k * nsamples + s, the order of camera_rays_pixels and of shade_rays' output.  ``nsamples``
        None: what the tensor's size gives."""
        import torch

        dev = self._dev()
        if radiance.device != dev or radiance.dtype != torch.float32:
            raise ValueError(f"AdaptiveFilm.add: expects a float32 tensor on {dev}")
        if pixels is not None and (pixels.device != dev or pixels.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32))
                                   or pixels.dim() != 1 or not pixels.is_contiguous()):
            raise ValueError(f"AdaptiveFilm.add: pixels must be a contiguous (m,) int32 tensor on {dev}")
        radiance = radiance.contiguous()
        m = self.width * self.height if pixels is None else pixels.numel()
        if nsamples is None:
            nsamples = radiance.numel() // (3 * m) if m > 0 else 1
        if radiance.numel() != 3 * m * int(nsamples):
            raise ValueError("AdaptiveFilm.add: radiance must hold m * nsamples * 3 floats")
        if m == 0:
            return
        check(lib().rt_afilm_add_device(self._handle(), None if pixels is None else pixels.data_ptr(), m, radiance.data_ptr(),
                                        int(nsamples), _stream_of(stream, dev)))

    def resolve(self, p6: bool = False, counts: bool = False, row0: int = 0, rows: Optional[int] = None,
                stream: Optional[int] = None):
        """The pixels of rows [row0, row0 + rows) (default: to the last row), each from its own
        count (no samples: 0): a (rows, W, 3) float32 tensor ``rgb``, or ``(rgb[, counts][, bytes])``:
        with ``counts=True`` the rows' (rows, W) int32 sample-count map, with ``p6=True`` the
        (rows, W, 3) uint8 P6 samples (write_p6 defaults).  Does not clear."""
        import torch

        if rows is None:
            rows = self.height - int(row0)
        dev = self._dev()
        r = max(int(rows), 0)
        rgb = torch.empty((r, self.width, 3), dtype=torch.float32, device=dev)
        b = torch.empty((r, self.width, 3), dtype=torch.uint8, device=dev) if p6 else None
        c = torch.empty((r, self.width), dtype=torch.int32, device=dev) if counts else None
        spare = torch.empty(1, dtype=torch.float32, device=dev) if rgb.numel() == 0 else None
        check(lib().rt_afilm_resolve_device(self._handle(), int(row0), int(rows),
                                            rgb.data_ptr() if spare is None else spare.data_ptr(),
                                            None if b is None or spare is not None else b.data_ptr(),
                                            None if c is None or spare is not None else c.data_ptr(), _stream_of(stream, dev)))
        out = (rgb,) + ((c,) if counts else ()) + ((b,) if p6 else ())
        return out if len(out) > 1 else rgb

    def select(self, min_spp: int, max_spp: int, step: int, tol: float, floor: float = 1e-3, stream: Optional[int] = None):
        """The pixels to sample next (rt_afilm_select_device): a pixel with n samples is selected
        iff n + step <= max_spp and (n < min_spp or its mean is noisy): in double from the float
        moments, mean = m1 / n, var = (max(0, m2 / n - mean^2) * n) / (n - 1), noisy iff
        var / n > (tol * max(mean, floor))^2, the squared standard error of the mean luminance
        against the squared tolerance.  ``min_spp`` >= 2, ``step`` >= 1, ``tol`` >= 0, ``floor`` > 0.

        Returns ``(pixels, n)``: ``pixels`` an (n,) int32 device tensor of indices y * W + x in
        increasing order, ``n`` a Python int.  Reading ``n`` is one 4-byte host read per pass, which
        waits for the stream: the only synchronisation of an adaptive pass."""
        import torch

        dev = self._dev()
        o = L.AFilmSelectOpts(int(min_spp), int(max_spp), int(step), float(tol), float(floor))
        if self._scratch is None:
            nb = int(lib().rt_afilm_select_scratch_bytes(self._handle()))
            self._scratch = torch.empty((nb + 3) // 4, dtype=torch.int32, device=dev)
            self._count = torch.empty(1, dtype=torch.int32, device=dev)
        out = torch.empty(self.width * self.height, dtype=torch.int32, device=dev)
        cur = torch.cuda.current_stream(dev)
        st = _stream_of(stream, dev)
        check(lib().rt_afilm_select_device(self._handle(), C.byref(o), out.data_ptr(), self._count.data_ptr(),
                                           self._scratch.data_ptr(), st))
        if st != cur.cuda_stream:
            torch.cuda.ExternalStream(st, device=dev).synchronize()
        n = int(self._count.item())
        return out[:n], n

    def clear(self, stream: Optional[int] = None) -> None:
        """Sums, counts and moments to 0."""
        check(lib().rt_afilm_clear_device(self._handle(), _stream_of(stream, self._dev())))

    def close(self) -> None:
        if self._h:
            lib().rt_afilm_destroy(self._h)
            self._h = C.c_void_p()
            self._scratch = self._count = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def afilm_host(width: int, height: int, state=None, radiance=None, pixels=None, nsamples: Optional[int] = None,
               resolve: bool = False, select=None):
    """Host build of the adaptive film (rt_afilm_host, no device).  ``state``: ``(sums (H*W*3,)
    float32, counts (H*W,) uint32, moments (H*W*2,) float32)``, updated in place (None: zeros).
    In this order: ``radiance`` (m*nsamples*3 float32; None: no add) is added onto ``pixels`` ((m,)
    uint32; None: every pixel in order); with ``resolve`` the whole image's ``rgb`` (H, W, 3)
    float32 and P6 ``bytes`` (H, W, 3) uint8; with ``select = (min_spp, max_spp, step, tol[, floor])``
    the selected pixel indices.  Returns a dict: ``state``, and ``rgb``, ``bytes``, ``selected``
    where asked for."""
    width, height = int(width), int(height)
    np_ = max(width * height, 0)
    if state is None:
        state = (np.zeros(np_ * 3, np.float32), np.zeros(np_, np.uint32), np.zeros(np_ * 2, np.float32))
    sums, counts, mom = state
    for a, dt, k in ((sums, np.float32, 3), (counts, np.uint32, 1), (mom, np.float32, 2)):
        if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous and a.flags.writeable and a.size == np_ * k):
            raise ValueError("afilm_host: the state must be writeable contiguous arrays of W*H*3, W*H and W*H*2 elements")
    rad = px = None
    m = 0
    if radiance is not None:
        rad = _c(radiance, np.float32).reshape(-1)
        px = None if pixels is None else _c(pixels, np.uint32).reshape(-1)
        m = np_ if px is None else px.size
        if nsamples is None:
            nsamples = rad.size // (3 * m) if m > 0 else 1
        if rad.size != 3 * m * max(int(nsamples), 0):
            raise ValueError("afilm_host: radiance must hold m * nsamples * 3 floats")
        if rad.size == 0:
            rad = np.zeros(1, np.float32)  # (an empty array still has an address for the C checks)
    rgb = np.zeros((height, width, 3), np.float32) if resolve else None
    b = np.zeros((height, width, 3), np.uint8) if resolve else None
    o = None
    sel = n_sel = None
    if select is not None:
        mn, mx, stp, tol = select[:4]
        o = L.AFilmSelectOpts(int(mn), int(mx), int(stp), float(tol), float(select[4]) if len(select) > 4 else 1e-3)
        sel = np.zeros(max(np_, 1), np.uint32)
        n_sel = C.c_uint32(0)
    check(lib().rt_afilm_host(width, height, ptr(sums), ptr(counts), ptr(mom), ptr(px) if px is not None and px.size else None,
                              m, ptr(rad), int(nsamples) if nsamples is not None else 1, ptr(rgb), ptr(b),
                              C.byref(o) if o is not None else None, ptr(sel), C.byref(n_sel) if n_sel is not None else None))
    out = {"state": state}
    if resolve:
        out["rgb"], out["bytes"] = rgb, b
    if select is not None:
        out["selected"] = sel[:n_sel.value].copy()
    return out


def _stream_of(stream, dev):
    import torch

    return torch.cuda.current_stream(dev).cuda_stream if stream is None else stream


def _query_tensor(x, width: int, dev, who: str, timing: bool):
    """The device path's input check: x as a contiguous (n, width) float32 tensor on dev; no timing."""
    import torch

    if x.device != dev or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != width:
        raise ValueError(f"{who}: expects an (n, {width}) float32 tensor on {dev}")
    if timing:
        raise ValueError(f"{who}: timing is measured on the host path only")
    return x.contiguous()


def _query_array(x, width: int, who: str, noun: str) -> np.ndarray:
    """The host path's input check: x as a contiguous (n, width) float32 array of ``noun``."""
    a = _c(x, np.float32)
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError(f"{who}: expects an (n, {width}) array of {noun}")
    return a


def _per_item(x, n: int, dev, who: str, name: str, item: str):
    """None, or x as n float32 bounds (max_t, max_d2): a tensor on dev, or an array when dev is None."""
    if x is None:
        return None
    if dev is None:
        a = _c(x, np.float32)
    else:
        import torch

        a = torch.as_tensor(x, dtype=torch.float32, device=dev).contiguous()
    if tuple(a.shape) != (n,):
        raise ValueError(f"{who}: {name} must hold one float per {item}")
    return a


def _unsort(order, stream, dev, temps, *outs) -> tuple:
    """A query's ``sort=`` epilogue: ``outs`` (None allowed) scattered back to the caller's order;
    the sorted tensors, ``temps`` and ``order`` among them, are dropped on return (_used_on).
    ``outs`` as given when order is None."""
    if order is None:
        return outs
    back = tuple(None if a is None else scatter(a, order, stream=stream) for a in outs)
    _used_on(stream, dev, order, *temps, *outs)
    return back


def _used_on(stream, dev, *tensors) -> None:
    """Tell torch's allocator that ``tensors``, temporaries a call drops on return, are in use on
    ``stream`` (a HIP stream handle) when that is not torch's current stream, so that their memory
    is not handed out again before the launches on it have run."""
    import torch

    if stream is None or stream == torch.cuda.current_stream(dev).cuda_stream:
        return
    ext = torch.cuda.ExternalStream(stream, device=dev)
    for t in tensors:
        if t is not None:
            t.record_stream(ext)


def _seed_tensor(seeds, n: int, dev, who: str, item: str = "path"):
    """n uint32 seeds as an int32 tensor on dev (the same 32 bits), or None."""
    import torch

    if seeds is None:
        return None
    if _is_torch(seeds):
        if seeds.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or seeds.device != dev:
            raise ValueError(f"{who}: seeds must be an int32 or uint32 tensor on {dev}")
        sd = seeds.contiguous()
    else:
        sd = torch.from_numpy(_c(seeds, np.uint32).view(np.int32)).to(dev)
    if tuple(sd.shape) != (n,):
        raise ValueError(f"{who}: seeds must hold one uint32 per {item}")
    return sd


class PathState:
    """The state of n staged paths on a device (rt_path_state): ``radiance`` (n, 3) float32,
    ``throughput`` (n, 3) float32 and ``rng`` (n,) int32 (the rng's 32 bits), indexed by path id.
    DeviceScene.path_begin makes one; path_step updates it; path_finish clamps its radiance."""

    def __init__(self, radiance, throughput, rng):
        self.radiance, self.throughput, self.rng = radiance, throughput, rng
        self.n = int(rng.shape[0])
        self.c = L.PathStateT(radiance.data_ptr(), throughput.data_ptr(), rng.data_ptr())


def path_finish(state: PathState, stream: Optional[int] = None):
    """The reference's final clamp on every path's radiance, in place (rt_path_finish_device);
    returns ``state.radiance``."""
    dev = state.radiance.device
    if state.n > 0:
        check(lib().rt_path_finish_device(dev.index, state.n, state.radiance.data_ptr(), _stream_of(stream, dev)))
    return state.radiance


def compact_paths(alive, rays, ids=None, stream: Optional[int] = None):
    """Stable compaction of a step's live rays (rt_path_compact_device): for the k with
    ``alive[k] != 0``, in increasing k, ``rays[k]`` and its path id (``ids[k]``; None: k).
    ``alive`` (m,) uint8, ``rays`` (m, 6) float32, ``ids`` (m,) int32, on one device.  Returns
    ``(rays, ids, count)``, the first ``count`` rows of new tensors; count is read back, which
    waits for the stream."""
    import torch

    dev = rays.device
    m = rays.shape[0]
    if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 6 or not rays.is_contiguous():
        raise ValueError("compact_paths: rays must be a contiguous (m, 6) float32 tensor")
    if alive.device != dev or alive.dtype != torch.uint8 or tuple(alive.shape) != (m,) or not alive.is_contiguous():
        raise ValueError("compact_paths: alive must be a contiguous (m,) uint8 tensor on the rays' device")
    if ids is not None and (ids.device != dev or ids.dtype != torch.int32 or tuple(ids.shape) != (m,) or not ids.is_contiguous()):
        raise ValueError("compact_paths: ids must be a contiguous (m,) int32 tensor on the rays' device")
    out_r = torch.empty((m, 6), dtype=torch.float32, device=dev)
    out_i = torch.empty(m, dtype=torch.int32, device=dev)
    if m == 0:
        return out_r, out_i, 0
    count = torch.empty(1, dtype=torch.int32, device=dev)
    scratch = torch.empty(max(int(lib().rt_path_compact_scratch_bytes(m)) // 4, 1), dtype=torch.int32, device=dev)
    cur = torch.cuda.current_stream(dev)
    st = _stream_of(stream, dev)
    check(lib().rt_path_compact_device(dev.index, m, alive.data_ptr(), rays.data_ptr(), None if ids is None else ids.data_ptr(),
                                       out_r.data_ptr(), out_i.data_ptr(), count.data_ptr(), scratch.data_ptr(), st))
    if st != cur.cuda_stream:
        torch.cuda.ExternalStream(st, device=dev).synchronize()
    c = int(count.item())
    return out_r[:c], out_i[:c], c


# ---- sorting caller rays for coherence (rt_ray_*, rt_gather_device, rt_scatter_device) ---------------
SORT_MODES = {"origin": L.RT_SORT_ORIGIN, "origin_dir": L.RT_SORT_ORIGIN_DIR}
SORT_MAX_BITS = {"origin": 10, "origin_dir": 5}
# The bits a mode takes when none are given: per mode the sweep's lowest total of sort + query +
# scatter over the frog batches of classes B and C (profiles/r10/ray_sort.jsonl).
# ``sort=True`` is the lower of the two: origin at 8 bits.
SORT_DEFAULT_BITS = {"origin": 8, "origin_dir": 5}
SORT_DEFAULT = "origin"


def _sort_spec(mode, bits, who: str):
    """(RT_SORT_* id, bits) of a mode name (True: the default mode) and bits (None: the mode's default)."""
    if mode is True:
        mode = SORT_DEFAULT
    if mode not in SORT_MODES:
        raise ValueError(f"{who}: sort mode must be one of {sorted(SORT_MODES)} (or True), not {mode!r}")
    b = SORT_DEFAULT_BITS[mode] if bits is None else int(bits)
    if not 1 <= b <= SORT_MAX_BITS[mode]:
        raise ValueError(f"{who}: bits must be in 1..{SORT_MAX_BITS[mode]} for mode {mode!r}")
    return SORT_MODES[mode], b


def _aabb(box, who: str) -> L.AABB:
    b = np.asarray(box, np.float32).reshape(-1)
    if b.size != 6:
        raise ValueError(f"{who}: box must hold 6 floats (min corner, max corner)")
    return L.AABB(_v3(b[:3]), _v3(b[3:]))


def _is_torch(a) -> bool:
    return type(a).__module__.split(".")[0] == "torch"


def _ray_tensor(rays, who: str):
    import torch

    if rays.device.type != "cuda" or rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 6:
        raise ValueError(f"{who}: expects an (n, 6) float32 tensor on a device")
    return rays.contiguous()


def ray_key_bits(mode="origin", bits=None) -> int:
    """Bits of a mode's key (rt_ray_key_bits): 3 * bits (origin) or 6 * bits (origin_dir)."""
    m, b = _sort_spec(mode, bits, "ray_key_bits")
    return int(lib().rt_ray_key_bits(m, b))


def ray_keys(rays, box, mode="origin", bits=None, stream: Optional[int] = None):
    """Coherence keys of caller rays in ``box`` (6 floats, min then max corner; DeviceScene.bounds
    gives a scene's): per ray the interleaved cells of its origin on a 2^bits grid over the box
    (``mode="origin"``, bits 1..10) or of its origin and unit direction (``"origin_dir"``, bits
    1..5), in exact float32 (include/rt_mi355x.h states the arithmetic).  A numpy (n, 6) array takes
    the host build and returns uint32; a torch tensor takes the kernel on ``stream`` (default torch's
    current stream) and returns an int32 tensor with the same bits."""
    m, b = _sort_spec(mode, bits, "ray_keys")
    bx = _aabb(box, "ray_keys")
    if _is_torch(rays):
        import torch

        r = _ray_tensor(rays, "ray_keys")
        n = r.shape[0]
        keys = torch.empty(n, dtype=torch.int32, device=r.device)
        check(lib().rt_ray_keys_device(r.device.index, r.data_ptr(), n, m, b, C.byref(bx), keys.data_ptr(),
                                       _stream_of(stream, r.device)))
        return keys
    r = _c(rays, np.float32)
    if r.ndim != 2 or r.shape[1] != 6:
        raise ValueError("ray_keys: expects an (n, 6) array of origins and directions")
    keys = np.zeros(r.shape[0], np.uint32)
    check(lib().rt_ray_keys_host(ptr(r), r.shape[0], m, b, C.byref(bx), ptr(keys)))
    return keys


def sort_rays(rays, box, mode="origin", bits=None, stream: Optional[int] = None):
    """Rays in key order (rt_ray_sort_device / rt_ray_sort_host): returns ``(sorted_rays, order)``,
    ``order`` (n,) int32 the stable sort of the indices by ``ray_keys`` (equal keys keep increasing
    index), ``sorted_rays[k] = rays[order[k]]``.  A torch tensor is sorted on its device on ``stream``
    (default torch's current stream), with no host synchronisation; a numpy array on the host."""
    m, b = _sort_spec(mode, bits, "sort_rays")
    bx = _aabb(box, "sort_rays")
    if _is_torch(rays):
        import torch

        r = _ray_tensor(rays, "sort_rays")
        n = r.shape[0]
        out = torch.empty_like(r)
        order = torch.empty(n, dtype=torch.int32, device=r.device)
        if n > 0:
            scratch = torch.empty(int(lib().rt_ray_sort_scratch_bytes(n, m, b)), dtype=torch.uint8, device=r.device)
            check(lib().rt_ray_sort_device(r.device.index, r.data_ptr(), n, m, b, C.byref(bx), order.data_ptr(),
                                           out.data_ptr(), scratch.data_ptr(), _stream_of(stream, r.device)))
            _used_on(stream, r.device, scratch)
        return out, order
    r = _c(rays, np.float32)
    if r.ndim != 2 or r.shape[1] != 6:
        raise ValueError("sort_rays: expects an (n, 6) array of origins and directions")
    order = np.zeros(r.shape[0], np.uint32)
    check(lib().rt_ray_sort_host(ptr(r), r.shape[0], m, b, C.byref(bx), ptr(order)))
    return r[order], order.view(np.int32)


def _permute(fn, who: str, x, order, out, stream):
    import torch

    if not _is_torch(x) or x.device.type != "cuda" or x.dim() < 1 or not x.is_contiguous():
        raise ValueError(f"{who}: expects a contiguous device tensor with one row per entry")
    n = x.shape[0]
    eb = x.element_size()
    for d in x.shape[1:]:
        eb *= int(d)
    if eb % 4 != 0 or not 4 <= eb <= 64:
        raise ValueError(f"{who}: a row must hold a multiple of 4 bytes in 4..64, not {eb}")
    if order.device != x.device or order.dtype != torch.int32 or tuple(order.shape) != (n,) or not order.is_contiguous():
        raise ValueError(f"{who}: order must be a contiguous (n,) int32 tensor on the entries' device")
    if out is None:
        out = torch.empty_like(x)
    elif out.device != x.device or out.dtype != x.dtype or out.shape != x.shape or not out.is_contiguous():
        raise ValueError(f"{who}: out must be a contiguous tensor like the input")
    if n > 0:
        check(fn(x.device.index, x.data_ptr(), n, eb, order.data_ptr(), out.data_ptr(), _stream_of(stream, x.device)))
    return out


def gather(x, order, out=None, stream: Optional[int] = None):
    """``out[k] = x[order[k]]`` on the device (rt_gather_device): ``x`` a contiguous tensor whose rows
    hold 4..64 bytes (a multiple of 4), ``order`` (n,) int32, a permutation of 0..n-1.  One launch
    on ``stream`` (default torch's current stream); returns ``out`` (a new tensor unless given)."""
    return _permute(lib().rt_gather_device, "gather", x, order, out, stream)


def scatter(x, order, out=None, stream: Optional[int] = None):
    """``out[order[k]] = x[k]`` on the device (rt_scatter_device), the inverse of ``gather``."""
    return _permute(lib().rt_scatter_device, "scatter", x, order, out, stream)


def path_step_host(rays, hits, radiance, throughput, rng, occluded, lights, table=None, materials=None, ids=None,
                   diffuse_bounce: bool = True, miss_color=(0, 0, 0), last: bool = False):
    """Host build of the step's arithmetic (rt_path_step_host, no device): numpy arrays in
    path_step's shapes (``hits`` (m,) HIT_DTYPE, ``lights`` LIGHT_DTYPE, ``table`` (nm, 13) or None),
    the state arrays ``radiance``, ``throughput`` (N, 3) float32 and ``rng`` (N,) uint32 updated in
    place, and ``occluded`` (m, num_lights) uint8, read where the kernel would cast entry k's shadow
    ray to light l.  Returns ``(next_rays, alive, direct)``."""
    r = _c(rays, np.float32)
    m = r.shape[0]
    h = np.ascontiguousarray(hits, HIT_DTYPE)
    lt = np.ascontiguousarray(lights, LIGHT_DTYPE)
    occ = _c(occluded, np.uint8).reshape(m, lt.size)
    tb = None if table is None else _c(table, np.float32).reshape(-1, 13)
    mt = None if materials is None else _c(materials, np.float32)
    idv = None if ids is None else _c(ids, np.uint32)
    for a, dt in ((radiance, np.float32), (throughput, np.float32), (rng, np.uint32)):
        if not isinstance(a, np.ndarray) or a.dtype != dt or not a.flags.c_contiguous or not a.flags.writeable:
            raise ValueError("path_step_host: the state must be writeable contiguous float32 / uint32 arrays")
    N = rng.shape[0]
    if r.shape != (m, 6) or h.shape != (m,) or radiance.shape != (N, 3) or throughput.shape != (N, 3) \
            or (mt is not None and mt.shape != (m, 13)) or (idv is not None and idv.shape != (m,)):
        raise ValueError("path_step_host: the arrays do not match the batch")
    used = idv[idv != L.RT_PATH_NONE] if idv is not None else np.arange(m)
    if used.size and int(used.max()) >= N:
        raise ValueError("path_step_host: a path id outside the state")
    nxt = np.zeros((m, 6), np.float32)
    alive = np.zeros(m, np.uint8)
    direct = np.zeros((m, 3), np.float32)
    st = L.PathStateT(ptr(radiance), ptr(throughput), ptr(rng))
    o = L.PathOpts(1 if diffuse_bounce else 0, _v3(miss_color), L.RT_PATH_LAST if last else 0)
    if m > 0:
        check(lib().rt_path_step_host(m, ptr(r), ptr(h), ptr(mt), ptr(idv), ptr(tb) if tb is not None and tb.size else None,
                                      0 if tb is None else tb.shape[0], ptr(lt) if lt.size else None, lt.size,
                                      ptr(occ) if occ.size else None, C.byref(o), C.byref(st), ptr(nxt), ptr(alive), ptr(direct)))
    return nxt, alive, direct


def _host_state(who: str, *arrays):
    for a, dt in arrays:
        if not isinstance(a, np.ndarray) or a.dtype != dt or not a.flags.c_contiguous or not a.flags.writeable:
            raise ValueError(f"{who}: the state must be writeable contiguous float32 / uint32 arrays")


def light_samples_host(hits, lights, light_shapes, rng, ids=None):
    """Host build of the visibility stage but for its traversals (rt_light_samples_host, no
    device): ``hits`` (m,) HIT_DTYPE, ``lights`` LIGHT_DTYPE, ``light_shapes`` LIGHT_SHAPE_DTYPE,
    ``rng`` (N,) uint32 advanced in place as the stage advances it, ``ids`` (m,) uint32 or None.
    Returns ``(rays, bounds, offsets)``: the shadow rays (R, 6) float32 in cast order, their bounds
    (R,) float32, and offsets (m * num_lights + 1,) uint64 with entry k's rays to light l at
    ``offsets[k * num_lights + l] : offsets[k * num_lights + l + 1]``."""
    h = np.ascontiguousarray(hits, HIT_DTYPE)
    m = h.shape[0]
    lt = np.ascontiguousarray(lights, LIGHT_DTYPE).reshape(-1)
    sh = np.ascontiguousarray(light_shapes, LIGHT_SHAPE_DTYPE).reshape(-1)
    idv = None if ids is None else _c(ids, np.uint32)
    _host_state("light_samples_host", (rng, np.uint32))
    if h.shape != (m,) or sh.shape != lt.shape or (idv is not None and idv.shape != (m,)):
        raise ValueError("light_samples_host: the arrays do not match the batch")
    used = idv[idv != L.RT_PATH_NONE] if idv is not None else np.arange(m)
    if used.size and int(used.max()) >= rng.shape[0]:
        raise ValueError("light_samples_host: a path id outside the state")
    off = np.zeros(m * lt.size + 1, np.uint64)
    args = (m, ptr(h) if m else None, ptr(idv), ptr(lt) if lt.size else None, ptr(sh) if lt.size else None, lt.size,
            ptr(rng) if m else None)
    check(lib().rt_light_samples_host(*args, 0, None, None, ptr(off)))
    total = int(off[-1])
    rays, bounds = np.zeros((total, 6), np.float32), np.zeros(total, np.float32)
    if total:
        check(lib().rt_light_samples_host(*args, total, ptr(rays), ptr(bounds), ptr(off)))
    return rays, bounds, off


def path_step_vis_host(rays, hits, radiance, throughput, rng, vis, lights, table=None, materials=None, ids=None,
                       diffuse_bounce: bool = True, miss_color=(0, 0, 0), last: bool = False):
    """path_step_host with ``vis`` (m, num_lights) float32, light_visibility's values, where that
    takes ``occluded`` (rt_path_step_vis_host).  Returns ``(next_rays, alive, direct)``."""
    r = _c(rays, np.float32)
    m = r.shape[0]
    h = np.ascontiguousarray(hits, HIT_DTYPE)
    lt = np.ascontiguousarray(lights, LIGHT_DTYPE)
    vs = _c(vis, np.float32).reshape(m, lt.size)
    tb = None if table is None else _c(table, np.float32).reshape(-1, 13)
    mt = None if materials is None else _c(materials, np.float32)
    idv = None if ids is None else _c(ids, np.uint32)
    _host_state("path_step_vis_host", (radiance, np.float32), (throughput, np.float32), (rng, np.uint32))
    N = rng.shape[0]
    if r.shape != (m, 6) or h.shape != (m,) or radiance.shape != (N, 3) or throughput.shape != (N, 3) \
            or (mt is not None and mt.shape != (m, 13)) or (idv is not None and idv.shape != (m,)):
        raise ValueError("path_step_vis_host: the arrays do not match the batch")
    used = idv[idv != L.RT_PATH_NONE] if idv is not None else np.arange(m)
    if used.size and int(used.max()) >= N:
        raise ValueError("path_step_vis_host: a path id outside the state")
    nxt = np.zeros((m, 6), np.float32)
    alive = np.zeros(m, np.uint8)
    direct = np.zeros((m, 3), np.float32)
    st = L.PathStateT(ptr(radiance), ptr(throughput), ptr(rng))
    o = L.PathOpts(1 if diffuse_bounce else 0, _v3(miss_color), L.RT_PATH_LAST if last else 0)
    if m > 0:
        check(lib().rt_path_step_vis_host(m, ptr(r), ptr(h), ptr(mt), ptr(idv), ptr(tb) if tb is not None and tb.size else None,
                                          0 if tb is None else tb.shape[0], ptr(lt) if lt.size else None, lt.size,
                                          ptr(vs) if vs.size else None, C.byref(o), C.byref(st), ptr(nxt), ptr(alive), ptr(direct)))
    return nxt, alive, direct


def film_pixels_host(radiance, width: int, rows: int, nsamples: int, sums=None, count_after: Optional[int] = None):
    """Host build of the film's arithmetic (rt_film_pixels_host, no device): adds ``radiance``
    (rows*width*nsamples*3 float32, sample s of pixel p at p*nsamples + s) to the running ``sums``
    ((rows, width, 3) float32, updated in place; None: zeros) and returns ``(sums, rgb)``, rgb the
    pixels of ``count_after`` samples per pixel (default ``nsamples``: a film's first add)."""
    r = _c(radiance, np.float32).reshape(-1)
    width, rows, nsamples = int(width), int(rows), int(nsamples)
    if r.size != max(width * rows * nsamples * 3, 0):
        raise ValueError("film_pixels_host: radiance must hold rows * width * nsamples * 3 floats")
    if sums is None:
        sums = np.zeros((max(rows, 0), max(width, 0), 3), np.float32)
    if not (isinstance(sums, np.ndarray) and sums.dtype == np.float32 and sums.flags.c_contiguous
            and sums.size == max(rows * width * 3, 0)):
        raise ValueError("film_pixels_host: sums must be a contiguous (rows, width, 3) float32 array")
    rgb = np.zeros(sums.shape, np.float32)
    spare = np.zeros(1, np.float32)  # (an empty array still has an address for the C checks)
    check(lib().rt_film_pixels_host(ptr(r if r.size else spare), width, rows, nsamples, ptr(sums if sums.size else spare),
                                    int(nsamples if count_after is None else count_after), ptr(rgb if rgb.size else spare)))
    return sums, rgb


def build_bvh(positions, indices):
    """CPU LBVH (G/include/bvh.cu:209-317) over an indexed mesh: (nodes (2P-1,4), aabbs (2P-1,6))."""
    pos, idx = _c(positions, np.float32), _c(indices, np.uint32)
    P = idx.size // 3
    if P == 0:  # what rt_build_bvh answers for an empty mesh (no arrays to size)
        check(lib().rt_build_bvh(ptr(pos), pos.size // 3, None, 0, None, None))
    nodes = np.zeros((2 * P - 1, 4), np.uint32)
    aabbs = np.zeros((2 * P - 1, 6), np.float32)
    check(lib().rt_build_bvh(ptr(pos), pos.size // 3, ptr(idx), P, ptr(nodes), ptr(aabbs)))
    return nodes, aabbs


def build_bvh_triangles(triangles):
    """CPU LBVH over a (P, 18) triangle array (rt_build_bvh_triangles): build_bvh over the 3P
    vertices v0, v1, v2 with indices 0..3P-1, the tree DeviceScene.rebuild gives a scene.
    (nodes (2P-1,4), aabbs (2P-1,6)); internal nodes first, leaves from P-1 on."""
    tr = _c(triangles, np.float32)
    P = tr.size // 18
    if P == 0:
        check(lib().rt_build_bvh_triangles(0, ptr(np.zeros(18, np.float32)), None, None))
    nodes = np.zeros((2 * P - 1, 4), np.uint32)
    aabbs = np.zeros((2 * P - 1, 6), np.float32)
    check(lib().rt_build_bvh_triangles(P, ptr(tr), ptr(nodes), ptr(aabbs)))
    return nodes, aabbs


def refit_aabbs(nodes, triangles) -> np.ndarray:
    """The (2P-1, 6) boxes a refit gives the tree ``nodes`` over ``triangles`` (P, 18), on the host
    (rt_refit_aabbs_host): aabb_of_triangle per leaf, merge(left, right) bottom-up."""
    nd, tr = _c(nodes, np.uint32), _c(triangles, np.float32)
    P = tr.size // 18
    if nd.size != 4 * (2 * P - 1):
        raise ValueError("refit_aabbs: expects 2P-1 nodes for P triangles")
    out = np.zeros((2 * P - 1, 6), np.float32)
    check(lib().rt_refit_aabbs_host(P, ptr(nd), ptr(tr), ptr(out)))
    return out


def triangles_from_mesh(positions, indices, normals=None, device: int = 0, stream=None):
    """The (P, 18) triangle array of an indexed mesh as a device tensor
    (rt_triangles_from_mesh_device; G/src/main.cu:388-404: zero normals when the mesh has none).
    positions (nv, 3) float32, indices (P, 3) uint32 and normals (nv, 3) may be numpy arrays or
    device tensors; with tensors nothing leaves the GPU, so deformed vertices reach
    DeviceScene.refit directly."""
    import torch

    dev = torch.device("cuda", device)

    def on_dev(a, dt_np):
        if isinstance(a, torch.Tensor):
            return a.to(dev).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a, dt_np).view(np.int32 if dt_np == np.uint32 else dt_np)
                                .copy()).to(dev)

    pos = on_dev(positions, np.float32).reshape(-1, 3)
    idx = on_dev(indices, np.uint32).reshape(-1, 3)
    nrm = None if normals is None else on_dev(normals, np.float32).reshape(-1, 3)
    if nrm is not None and nrm.shape[0] != pos.shape[0]:
        raise ValueError("triangles_from_mesh: one normal per vertex")
    P = idx.shape[0]
    tris = torch.empty((P, 18), dtype=torch.float32, device=dev)
    check(lib().rt_triangles_from_mesh_device(device, pos.data_ptr(), pos.shape[0], None if nrm is None else nrm.data_ptr(),
                                              idx.data_ptr(), P, tris.data_ptr(), _stream_of(stream, dev)))
    return tris


def build_bvh_device(positions, indices, device: int = 0, stream=None, tensors: bool = False):
    """The LBVH build on the GPU (rt_build_bvh_device): the same (nodes (2P-1,4), aabbs (2P-1,6))
    as build_bvh.  positions (nv,3) float32 / indices (P,3) uint32 may be numpy arrays or device
    tensors; tensors=True returns device tensors (nodes as int32 bit patterns) instead of numpy."""
    import torch

    dev = torch.device("cuda", device)

    def on_dev(a, dt_np):
        if isinstance(a, torch.Tensor):
            return a.to(dev).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a, dt_np).view(np.int32 if dt_np == np.uint32 else dt_np)
                                .copy()).to(dev)

    pos = on_dev(positions, np.float32).reshape(-1, 3)
    idx = on_dev(indices, np.uint32).reshape(-1, 3)
    P = idx.shape[0]
    nodes = torch.empty((max(2 * P - 1, 1), 4), dtype=torch.int32, device=dev)
    aabbs = torch.empty((max(2 * P - 1, 1), 6), dtype=torch.float32, device=dev)
    check(lib().rt_build_bvh_device(device, pos.data_ptr(), pos.shape[0], idx.data_ptr(), P, nodes.data_ptr(),
                                    aabbs.data_ptr(), _stream_of(stream, dev)))
    if tensors:
        return nodes, aabbs
    return nodes.cpu().numpy().view(np.uint32), aabbs.cpu().numpy()


def _ppm_opts(maxval=255, clamp=True, gamma2=True, flip_y=False) -> L.PPMOptions:
    return L.PPMOptions(int(maxval), 1 if clamp else 0, 1 if gamma2 else 0, 1 if flip_y else 0)


def encode_p6(rgb, maxval=255, clamp=True, gamma2=True, flip_y=False) -> bytes:
    a = _c(rgb, np.float32)
    H, W = a.shape[0], a.shape[1]
    o = _ppm_opts(maxval, clamp, gamma2, flip_y)
    n = C.c_size_t()
    check(lib().rt_ppm_encode(ptr(a), W, H, C.byref(o), None, 0, C.byref(n)))
    buf = (C.c_uint8 * n.value)()
    check(lib().rt_ppm_encode(ptr(a), W, H, C.byref(o), C.cast(buf, C.c_void_p), n.value, C.byref(n)))
    return bytes(buf)


def write_p6(path, rgb, maxval=255, clamp=True, gamma2=True, flip_y=False) -> None:
    a = _c(rgb, np.float32)
    o = _ppm_opts(maxval, clamp, gamma2, flip_y)
    check(lib().rt_ppm_write(str(path).encode(), ptr(a), a.shape[1], a.shape[0], C.byref(o)))


def read_p6(path) -> np.ndarray:
    w, h, mv = C.c_int(), C.c_int(), C.c_int()
    check(lib().rt_ppm_read(str(path).encode(), None, 0, C.byref(w), C.byref(h), C.byref(mv)))
    out = np.zeros((h.value, w.value, 3), np.float32)
    check(lib().rt_ppm_read(str(path).encode(), ptr(out), out.size, C.byref(w), C.byref(h), C.byref(mv)))
    return out


def p6_header(width: int, height: int, maxval: int = 255) -> bytes:
    """write_p6's header bytes (ppm_p6.cpp:275-277)."""
    n = C.c_size_t()
    check(lib().rt_ppm_header(width, height, maxval, None, 0, C.byref(n)))
    buf = C.create_string_buffer(n.value)
    check(lib().rt_ppm_header(width, height, maxval, buf, n.value, C.byref(n)))
    return buf.raw[:n.value]


def quantize_p6_device(rgb_dev, width: int, rows: int, out_dev, maxval=255, clamp=True, gamma2=True,
                       flip_y=False, stream=None) -> None:
    """P6 body of a device framebuffer on the device (rt_ppm_quantize_device).  rgb_dev / out_dev
    are device addresses (ints, e.g. tensor.data_ptr()); asynchronous on `stream`."""
    o = _ppm_opts(maxval, clamp, gamma2, flip_y)
    check(lib().rt_ppm_quantize_device(rgb_dev, width, rows, C.byref(o), out_dev, stream))


def unpermute_strips_device(strips_dev, strip_rows: int, row_bytes: int, height: int, band_rows: int,
                            band_count: int, frame_dev, flip_y=False, stream=None) -> None:
    """Band un-permute of back-to-back gathered strips into an image-order frame on the device."""
    check(lib().rt_unpermute_strips_device(strips_dev, strip_rows, row_bytes, height, band_rows, band_count,
                                           1 if flip_y else 0, frame_dev, stream))


def encode_p6_device(rgb, maxval=255, clamp=True, gamma2=True, flip_y=False):
    """P6 file bytes of an (H, W, 3) float32 CUDA tensor, quantised on the device (only the
    quantised body crosses PCIe).  Same bytes as encode_p6 on the host copy."""
    import torch

    if not (isinstance(rgb, torch.Tensor) and rgb.is_cuda and rgb.dtype == torch.float32 and rgb.dim() == 3
            and rgb.shape[2] == 3):
        raise ValueError("encode_p6_device: expects an (H, W, 3) float32 device tensor")
    rgb = rgb.contiguous()
    H, W = rgb.shape[0], rgb.shape[1]
    bps = 1 if maxval < 256 else 2
    body = torch.empty(H * W * 3 * bps, dtype=torch.uint8, device=rgb.device)
    stream = _stream_of(None, rgb.device)
    quantize_p6_device(rgb.data_ptr(), W, H, body.data_ptr(), maxval, clamp, gamma2, flip_y, stream)
    return p6_header(W, H, maxval) + body.cpu().numpy().tobytes()


def set_tuning(name: str, value) -> None:
    """Process-wide tuning knob (rt_tuning_set; include/rt_mi355x.h rt_tune_id): None restores
    its default.  Read when a scene is created or a frame is set up."""
    check(lib().rt_tuning_set(L.TUNE[name], float("nan") if value is None else float(value)))


def get_tuning(name: str):
    """The value set for a knob, or None when it has its default."""
    v = C.c_double()
    check(lib().rt_tuning_get(L.TUNE[name], C.byref(v)))
    return None if v.value != v.value else v.value


def reset_tuning() -> None:
    lib().rt_tuning_reset()


class tuning:
    """Context manager: ``with rt.tuning(half_waves=1): ...`` sets knobs, restores them after."""

    def __init__(self, **knobs):
        self.knobs = knobs
        self.saved = {}

    def __enter__(self):
        for k, v in self.knobs.items():
            self.saved[k] = get_tuning(k)
            set_tuning(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            set_tuning(k, v)
        return False


def device_count() -> int:
    n = C.c_int()
    rc = lib().rt_device_count(C.byref(n))
    return n.value if rc == 0 else 0
