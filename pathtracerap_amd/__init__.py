"""MI355X-native PathTracerAP hot path.

Python mirror of the reference's host interface (Scene.h / Renderer.h of
purvakulkarni15/PathTracerAP) over the C ABI in ``include/pathtracer_amd.h``
(``libpathtracer_amd.so``: C++ host + gfx950 HIP kernels)::

    scene = Scene("scenes/reference_scene.txt")      # Scene::Scene(string config)
    renderer = Renderer(RenderConfig())              # Config.h constants at runtime
    renderer.allocateOnGPU(scene)                    # Renderer::allocateOnGPU
    renderer.renderLoop()                            # Renderer::renderLoop
    renderer.renderImage("Render.bmp")               # Renderer::renderImage
    renderer.free()                                  # Renderer::free

There is no CPU fallback: if the shared library is missing or no gfx950
device is present, the calls raise.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from dataclasses import dataclass, field

import numpy as np

__all__ = ["Scene", "Renderer", "RenderConfig", "Camera", "look_at", "Environment", "PathTracerError", "build", "lib", "hw_queues",
           "MATERIALS", "ACCEL_GRID", "ACCEL_BVH", "ACCEL_GRID_FAST"]

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("PT_LIB_PATH") or os.path.join(_HERE, "libpathtracer_amd.so")   # override: experiments

ACCEL_GRID = 0
ACCEL_BVH = 1
ACCEL_GRID_FAST = 2
NOISE_TILE = 16     # PT_NOISE_TILE: Renderer.noise()'s tile edge in pixels
DENOISE_MAX_PASSES = 6     # PT_DENOISE_MAX_PASSES
DENOISE_DEMODULATE = 1     # PT_DENOISE_DEMODULATE (pt_renderer_denoise_ex's flags)
DENOISE_TILE_COUNTS = 2    # PT_DENOISE_TILE_COUNTS
DENOISE_SAMPLED_GUIDES = 4  # PT_DENOISE_SAMPLED_GUIDES


def _denoise_flags(demodulate, tile_counts, flags, sampled_guides=False):
    if flags is not None:
        return int(flags)
    return ((DENOISE_DEMODULATE if demodulate else 0) | (DENOISE_TILE_COUNTS if tile_counts else 0) |
            (DENOISE_SAMPLED_GUIDES if sampled_guides else 0))


# renderer.h: segments[] slots after the per-bounce counters, as segments_per_bounce indices
_MAX_BOUNCE_COUNTERS = 64
_DEFERRED_SLOT = 50 + _MAX_BOUNCE_COUNTERS - 1     # kDeferredRayCounter
# Primitive.h:70-79
MATERIALS = {"DIFFUSE": 0, "SPECULAR": 1, "REFLECTIVE": 2, "REFRACTIVE": 3,
             "EMISSIVE": 4, "COAT": 5, "METAL": 6, "DIELECTRIC": 7}


class PathTracerError(RuntimeError):
    pass


def build(force: bool = False, jobs: int = 4) -> str:
    """Compile libpathtracer_amd.so for gfx950 in-tree (hipcc, no GPU needed)."""
    cmd = ["make", "-s", "-C", _HERE, f"-j{jobs}"]
    if force:
        subprocess.check_call(["make", "-s", "-C", _HERE, "clean"])
    subprocess.check_call(cmd)
    return _LIB_PATH


class _Cfg(ctypes.Structure):
    _fields_ = [
        ("width", ctypes.c_int), ("height", ctypes.c_int), ("iterations", ctypes.c_int),
        ("max_bounces", ctypes.c_int), ("accel", ctypes.c_int), ("grid", ctypes.c_int * 3),
        ("tail_drop", ctypes.c_int), ("cam", ctypes.c_double * 3), ("plane_z", ctypes.c_double),
        ("plane_x0", ctypes.c_double), ("plane_y0", ctypes.c_double),
        ("plane_w", ctypes.c_double), ("plane_h", ctypes.c_double), ("block", ctypes.c_int),
        ("pipelines", ctypes.c_int), ("ray_sort", ctypes.c_int),
    ]


class _DenoiseParams(ctypes.Structure):
    _fields_ = [("passes", ctypes.c_int), ("sigma_l", ctypes.c_float), ("sigma_z", ctypes.c_float)]


class _Camera(ctypes.Structure):
    _fields_ = [("origin", ctypes.c_float * 3), ("p0", ctypes.c_float * 3), ("du", ctypes.c_float * 3),
                ("dv", ctypes.c_float * 3), ("lens_u", ctypes.c_float * 3), ("lens_v", ctypes.c_float * 3),
                ("lens_radius", ctypes.c_float)]


_P_F = ctypes.POINTER(ctypes.c_float)


class _Environment(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int), ("texels_rgb", _P_F), ("scale", ctypes.c_float * 3),
                ("rotation", ctypes.c_float * 9)]


_P_I = ctypes.POINTER(ctypes.c_int)
_P_D = ctypes.POINTER(ctypes.c_double)
_lib = None
_HIP_BEFORE_LOAD = None     # set when the library loads (torch's HIP runtime already up?)

# (name, restype, argtypes) of every exported symbol of include/pathtracer_amd.h
EXPORTS = [
    ("pt_abi_version", ctypes.c_int, []),
    ("pt_last_error", ctypes.c_char_p, []),
    ("pt_hw_queue_info", ctypes.c_int, [_P_I, _P_I]),
    ("pt_default_config", None, [ctypes.POINTER(_Cfg)]),
    ("pt_scene_create", ctypes.c_void_p, []),
    ("pt_scene_destroy", None, [ctypes.c_void_p]),
    ("pt_scene_load_config", ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    ("pt_scene_apply_settings", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_Cfg)]),
    ("pt_scene_load_obj", ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    ("pt_scene_add_mesh", ctypes.c_int, [ctypes.c_void_p, _P_F, _P_F, ctypes.c_int, _P_I, ctypes.c_int]),
    ("pt_scene_add_model", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _P_F, _P_F, _P_F, ctypes.c_int, _P_F]),
    ("pt_scene_set_model_smooth", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    ("pt_scene_model_smooth", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    ("pt_scene_set_model_ior", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_float]),
    ("pt_scene_model_ior", ctypes.c_float, [ctypes.c_void_p, ctypes.c_int]),
    ("pt_scene_set_mesh_uv", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _P_F, ctypes.c_int]),
    ("pt_scene_export_uv", ctypes.c_int, [ctypes.c_void_p, _P_F]),
    ("pt_scene_mesh_has_uv", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    ("pt_scene_add_texture", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _P_F]),
    ("pt_scene_texture_count", ctypes.c_int, [ctypes.c_void_p]),
    ("pt_scene_texture", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _P_I, _P_I, _P_F]),
    ("pt_scene_set_model_texture", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    ("pt_scene_model_texture", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    ("pt_scene_build", ctypes.c_int, [ctypes.c_void_p, _P_I, ctypes.c_int]),
    ("pt_scene_counts", ctypes.c_int, [ctypes.c_void_p, _P_I]),
    ("pt_scene_export", ctypes.c_int, [ctypes.c_void_p, _P_F, _P_F, _P_I, _P_I, _P_F, _P_I, _P_F, _P_F,
                                       _P_F, _P_I, _P_F, _P_I, _P_I]),
    ("pt_scene_export_bvh", ctypes.c_int, [ctypes.c_void_p, _P_F, _P_I, _P_I]),
    ("pt_scene_export_bvh4", ctypes.c_int, [ctypes.c_void_p, _P_F, _P_I]),
    ("pt_scene_export_bvh4_leaf_base", ctypes.c_int, [ctypes.c_void_p, _P_I]),
    ("pt_renderer_create", ctypes.c_void_p, [ctypes.POINTER(_Cfg)]),
    ("pt_renderer_set_stream", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    ("pt_renderer_bind_image", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    ("pt_renderer_allocate_on_gpu", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    ("pt_renderer_clear_image", ctypes.c_int, [ctypes.c_void_p]),
    ("pt_renderer_render_loop", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    ("pt_renderer_synchronize", ctypes.c_int, [ctypes.c_void_p]),
    ("pt_renderer_read_image", ctypes.c_int, [ctypes.c_void_p, _P_F]),
    ("pt_renderer_render_image", ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]),
    ("pt_renderer_segments", ctypes.c_longlong, [ctypes.c_void_p]),
    ("pt_renderer_trace_faults", ctypes.c_longlong, [ctypes.c_void_p]),
    ("pt_renderer_segments_per_bounce", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]),
    ("pt_renderer_pipelines", ctypes.c_int, [ctypes.c_void_p]),
    ("pt_renderer_set_profiling", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    ("pt_renderer_kernel_stats", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]),
    ("pt_renderer_kernel_stats_ex", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int]),
    ("pt_renderer_primary_hits", ctypes.c_int, [ctypes.c_void_p, _P_F, _P_F, _P_I]),
    ("pt_renderer_intersect_rays", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _P_F, _P_F, _P_F, _P_F, _P_I]),
    ("pt_renderer_certify_check", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _P_F, _P_F, _P_I]),
    ("pt_renderer_trace_rays", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _P_F, _P_F, _P_I, ctypes.c_int,
                                              _P_F, _P_F, _P_I, _P_I]),
    ("pt_renderer_enable_moments", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    ("pt_renderer_read_moments", ctypes.c_int, [ctypes.c_void_p, _P_F]),
    ("pt_renderer_noise", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double), _P_F, _P_F]),
    ("pt_renderer_render_until", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_double, _P_I, ctypes.POINTER(ctypes.c_double)]),
    ("pt_default_denoise_params", None, [ctypes.POINTER(_DenoiseParams)]),
    ("pt_renderer_denoise", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(_DenoiseParams), ctypes.c_void_p,
                                           _P_F, _P_F]),
    ("pt_renderer_render_image_denoised", ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int,
                                                         ctypes.POINTER(_DenoiseParams)]),
    ("pt_renderer_denoise_times", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int]),
    ("pt_renderer_denoise_ex", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(_DenoiseParams), ctypes.c_int,
                                              ctypes.c_void_p, _P_F, _P_F]),
    ("pt_renderer_render_image_denoised_ex", ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int,
                                                            ctypes.POINTER(_DenoiseParams), ctypes.c_int]),
    ("pt_renderer_render_loop_masked", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                      ctypes.POINTER(ctypes.c_ubyte)]),
    ("pt_renderer_sample_counts", ctypes.c_int, [ctypes.c_void_p, _P_I]),
    ("pt_renderer_enable_guides", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    ("pt_renderer_read_guides", ctypes.c_int, [ctypes.c_void_p, _P_F]),
    ("pt_renderer_guide_counts", ctypes.c_int, [ctypes.c_void_p, _P_I]),
    ("pt_renderer_adaptive_noise", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), _P_F, _P_F]),
    ("pt_renderer_adaptive_mean", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, _P_F]),
    ("pt_renderer_render_image_adaptive", ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    ("pt_renderer_render_adaptive", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                   ctypes.c_double, _P_I, ctypes.POINTER(ctypes.c_longlong),
                                                   ctypes.POINTER(ctypes.c_double)]),
    ("pt_renderer_set_pixel_jitter", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_float]),
    ("pt_renderer_pixel_jitter", ctypes.c_int, [ctypes.c_void_p, _P_I, _P_F]),
    ("pt_renderer_set_camera", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_Camera)]),
    ("pt_renderer_camera", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_Camera)]),
    ("pt_camera_look_at", ctypes.c_int, [_P_D, _P_D, _P_D, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                         ctypes.c_int, ctypes.c_int, ctypes.POINTER(_Camera)]),
    ("pt_scene_camera", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_Camera)]),
    ("pt_renderer_set_environment", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_Environment)]),
    ("pt_renderer_environment", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_Environment), _P_F]),
    ("pt_renderer_env_lookup", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _P_F, _P_F]),
    ("pt_renderer_primary_albedo", ctypes.c_int, [ctypes.c_void_p, _P_F]),
    ("pt_renderer_hit_albedo", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _P_F, _P_F, _P_F, _P_I, _P_I, _P_F]),
    ("pt_environment_sky", ctypes.c_int, [_P_F, _P_F, _P_F, ctypes.c_int, _P_F]),
    ("pt_renderer_free", None, [ctypes.c_void_p]),
    ("pt_selftest_math", ctypes.c_int, [ctypes.c_int, _P_F, _P_F, _P_F]),
    ("pt_selftest_dielectric", ctypes.c_int, [ctypes.c_int, _P_F, _P_F, _P_F, _P_F, _P_F, _P_I]),
    ("pt_render", ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(_Cfg), ctypes.c_char_p]),
    ("pt_renderer_set_direct_light", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    ("pt_renderer_direct_light", ctypes.c_int, [ctypes.c_void_p, _P_I, _P_I, _P_F]),
    ("pt_scene_lights", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _P_F, _P_F]),
    ("pt_renderer_lights", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _P_F, _P_F]),
    ("pt_scene_direct_light", ctypes.c_int, [ctypes.c_void_p]),
    ("pt_renderer_occluded", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _P_F, _P_F, _P_I]),
    ("pt_renderer_direct_sample", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _P_F, _P_F, _P_F, _P_I, _P_I, _P_F, _P_I,
                                                 _P_F, _P_I]),
]
LIGHT_FLOATS = 20


def _light_table(call, what) -> dict:
    """The light table behind ``call(max_lights, recs, area)`` (pt_scene_lights / pt_renderer_lights)
    -> dict(p0, e1, e2, nl, emission (n, 3), area, cdf (n,) float32, model (n,) int32, area_total)."""
    area = ctypes.c_float()
    n = _err(call(0, None, ctypes.byref(area)), what)
    recs = np.zeros((n, LIGHT_FLOATS), np.float32)
    if n:
        _err(call(n, _fp(recs), ctypes.byref(area)), what)
    return dict(p0=recs[:, 0:3].copy(), area=recs[:, 3].copy(), e1=recs[:, 4:7].copy(),
                model=recs[:, 7].copy().view(np.int32), e2=recs[:, 8:11].copy(), cdf=recs[:, 11].copy(),
                nl=recs[:, 12:15].copy(), emission=recs[:, 16:19].copy(), area_total=np.float32(area.value))


def lib() -> ctypes.CDLL:
    """Load the in-tree HIP library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise PathTracerError(
                f"{_LIB_PATH} not found: run `make -C pathtracerap_amd` (or __graft_entry__.build())")
        global _HIP_BEFORE_LOAD
        import sys
        tc = sys.modules.get("torch.cuda")
        _HIP_BEFORE_LOAD = bool(tc is not None and tc.is_initialized())
        L = ctypes.CDLL(_LIB_PATH)
        for name, res, args in EXPORTS:
            if os.environ.get("PT_LIB_PATH") and not hasattr(L, name):
                continue            # an older build loaded for an A/B baseline: bind what it has
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def hw_queues() -> dict:
    """GPU_MAX_HW_QUEUES as the library found it at load (None: unset, then the
    library set 16), and whether HIP had already started in this process when the
    library loaded (then HIP runs with the value it read at its own start)."""
    a, s = ctypes.c_int(), ctypes.c_int()
    lib().pt_hw_queue_info(ctypes.byref(a), ctypes.byref(s))
    libc = ctypes.CDLL(None)            # the C environment (os.environ is a snapshot taken at start-up)
    libc.getenv.restype = ctypes.c_char_p
    env = libc.getenv(b"GPU_MAX_HW_QUEUES")
    env = env.decode() if env else None
    return {"at_library_load": None if a.value < 0 else a.value, "set_by_library": bool(s.value),
            "env_now": int(env) if env and env.isdigit() else None, "hip_started_before_load": _HIP_BEFORE_LOAD}


def _err(rc, what):
    if rc is None or (isinstance(rc, int) and rc < 0):
        msg = lib().pt_last_error()
        raise PathTracerError(f"{what}: {msg.decode() if msg else 'error'}")
    return rc


def _fp(a):
    return a.ctypes.data_as(_P_F)


def _ip(a):
    return a.ctypes.data_as(_P_I)


@dataclass
class RenderConfig:
    """Config.h (RESOLUTION_X/Y, ITER, GRID_X/Y/Z) and generateRaysKernel's
    constants (camera, image plane, bounce count), as runtime values."""
    width: int = 1000
    height: int = 800
    iterations: int = 500
    max_bounces: int = 5
    accel: int = ACCEL_GRID_FAST   # the reference grid's results, bit for bit (ACCEL_GRID: its list-walking DDA)
    grid: tuple = (25, 25, 25)
    tail_drop: int = 0
    cam: tuple = (0.0, 0.0, 920.0)
    plane_z: float = 900.0
    plane_x0: float = -10.0
    plane_y0: float = -4.0
    plane_w: float = 20.0
    plane_h: float = 16.0
    block: int = 64
    pipelines: int = 16   # iterations in flight (own HIP streams); results identical for any value
    ray_sort: int = -1    # ray sort key before each persistent trace (-1 auto, 0 off); results identical

    def c(self) -> _Cfg:
        c = _Cfg()
        c.width, c.height, c.iterations, c.max_bounces = self.width, self.height, self.iterations, self.max_bounces
        c.accel, c.tail_drop = self.accel, self.tail_drop
        for k in range(3):
            c.grid[k] = int(self.grid[k])
            c.cam[k] = float(self.cam[k])
        c.plane_z, c.plane_x0, c.plane_y0, c.plane_w, c.plane_h = (
            self.plane_z, self.plane_x0, self.plane_y0, self.plane_w, self.plane_h)
        c.block = self.block
        c.pipelines = self.pipelines
        c.ray_sort = self.ray_sort
        return c


_CAMERA_VECS = ("origin", "p0", "du", "dv", "lens_u", "lens_v")


@dataclass
class Camera:
    """pt_camera (include/pathtracer_amd.h): the free camera's lens centre, the world point
    of pixel coordinates (0, 0), the world steps per pixel, which span the plane in focus,
    and the lens's two spanning vectors and radius (0: a pinhole).  Values are float32."""
    origin: tuple = (0.0, 0.0, 0.0)
    p0: tuple = (0.0, 0.0, 0.0)
    du: tuple = (1.0, 0.0, 0.0)
    dv: tuple = (0.0, 1.0, 0.0)
    lens_u: tuple = (1.0, 0.0, 0.0)
    lens_v: tuple = (0.0, 1.0, 0.0)
    lens_radius: float = 0.0

    def c(self) -> _Camera:
        c = _Camera()
        for name in _CAMERA_VECS:
            for k in range(3):
                getattr(c, name)[k] = float(getattr(self, name)[k])
        c.lens_radius = float(self.lens_radius)
        return c

    @classmethod
    def from_c(cls, c: _Camera) -> "Camera":
        return cls(*(tuple(float(v) for v in getattr(c, name)) for name in _CAMERA_VECS), float(c.lens_radius))


def look_at(eye, target, up=(0.0, 1.0, 0.0), vfov_deg: float = 45.0, focus_dist: float | None = None,
            lens_radius: float = 0.0, width: int = 1000, height: int = 800) -> Camera:
    """A look-at view for a ``width`` x ``height`` frame (pt_camera_look_at, which does the
    arithmetic): the camera at ``eye`` looking at ``target``, a vertical field of view of
    ``vfov_deg`` degrees, the plane in focus ``focus_dist`` away (None: at the target) and a
    thin lens of ``lens_radius`` (0: a pinhole)."""
    e, t, u = ((ctypes.c_double * 3)(*(float(v) for v in a)) for a in (eye, target, up))
    if focus_dist is None:
        focus_dist = float(np.sqrt(sum((float(t[k]) - float(e[k])) ** 2 for k in range(3))))
    out = _Camera()
    _err(lib().pt_camera_look_at(e, t, u, float(vfov_deg), float(focus_dist), float(lens_radius), int(width),
                                 int(height), ctypes.byref(out)), "look_at")
    return Camera.from_c(out)


def _up_rotation(up) -> np.ndarray:
    """The rotation (3, 3), world -> environment frame, whose third row is ``up`` normalised:
    the environment's +z, the map's centre, points along world ``up``.  With a the axis two
    after up's largest component, x = normalize(a x z) and y = z x x: (0, 1, 0) gives
    e = (u.z, u.x, u.y) and (0, 0, 1) the identity.  Computed in double, rounded once."""
    z = np.asarray(up, np.float64)
    if z.shape != (3,) or not np.isfinite(z).all() or not z.any():
        raise ValueError("up must be three finite numbers, not all zero")
    z = z / np.linalg.norm(z)
    a = np.zeros(3)
    a[(int(np.argmax(np.abs(z))) + 2) % 3] = 1.0
    x = np.cross(a, z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z]).astype(np.float32)


def _octahedral_directions(n: int) -> np.ndarray:
    """(n, n, 3) float64: the unit direction, in the environment frame, of every texel centre of
    an n x n octahedral map, row y column x."""
    p = (np.arange(n) + 0.5) / n * 2.0 - 1.0
    px, py = np.meshgrid(p, p)                  # px varies along a row
    ez = 1.0 - np.abs(px) - np.abs(py)
    low = ez < 0
    ex = np.where(low, (1.0 - np.abs(py)) * np.where(px >= 0, 1.0, -1.0), px)
    ey = np.where(low, (1.0 - np.abs(px)) * np.where(py >= 0, 1.0, -1.0), py)
    d = np.stack([ex, ey, ez], axis=-1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


class Environment:
    """pt_environment (include/pathtracer_amd.h): what a ray that leaves the scene brings back.
    ``texels``: (n, n, 3) float32 in octahedral layout, 1 <= n <= 2048; ``scale``: per channel;
    ``rotation``: (3, 3) row-major, world -> environment frame, whose +z is the map's centre."""

    def __init__(self, texels, scale=(1.0, 1.0, 1.0), rotation=None):
        t = np.ascontiguousarray(texels, np.float32)
        if t.ndim != 3 or t.shape[0] != t.shape[1] or t.shape[2] != 3:
            raise ValueError("texels must have shape (n, n, 3)")
        self.texels = t
        self.scale = np.asarray(scale, np.float32).reshape(3).copy()
        self.rotation = (np.eye(3, dtype=np.float32) if rotation is None
                         else np.asarray(rotation, np.float32).reshape(3, 3).copy())

    @property
    def n(self) -> int:
        return self.texels.shape[0]

    def c(self) -> _Environment:
        """The C record; it points into ``self.texels``, so keep ``self`` alive while it is used."""
        c = _Environment()
        c.n = self.n
        c.texels_rgb = _fp(self.texels)
        for k in range(3):
            c.scale[k] = float(self.scale[k])
        for k in range(9):
            c.rotation[k] = float(self.rotation.reshape(-1)[k])
        return c

    @classmethod
    def constant(cls, rgb, scale=(1.0, 1.0, 1.0)) -> "Environment":
        """One texel: the same radiance from every direction (a number or three)."""
        return cls(np.broadcast_to(np.asarray(rgb, np.float32), (3,)).reshape(1, 1, 3), scale)

    @classmethod
    def sky(cls, zenith, horizon, ground=(0.0, 0.0, 0.0), n: int = 64, up=(0.0, 1.0, 0.0)) -> "Environment":
        """pt_environment_sky: ``horizon`` blended towards ``zenith`` with the height above the
        horizon, ``ground`` below it; ``up`` is the world direction of the zenith."""
        z, h, g = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32), (3,))) for v in (zenith, horizon, ground))
        t = np.empty((max(int(n), 0), max(int(n), 0), 3), np.float32)
        _err(lib().pt_environment_sky(_fp(z), _fp(h), _fp(g), int(n), _fp(t)), "environment_sky")
        return cls(t, rotation=_up_rotation(up))

    @classmethod
    def from_latlong(cls, image, n: int = 256, up=(0.0, 1.0, 0.0)) -> "Environment":
        """Resample a latitude-longitude image (rows from +up down to -up, columns once around
        it; (h, w, 3)) into an n x n octahedral map, on the host in double: every texel centre's
        direction reads the image bilinearly, wrapping around in longitude and clamped at the
        poles.  Column 0 starts at the environment frame's +x (see ``_up_rotation``)."""
        img = np.asarray(image, np.float64)
        if img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
            raise ValueError("image must have shape (h, w, 3)")
        if not 1 <= int(n) <= 2048:
            raise ValueError("n must be 1 .. 2048")
        h, w = img.shape[:2]
        d = _octahedral_directions(int(n))
        v = np.clip(np.arccos(np.clip(d[..., 2], -1.0, 1.0)) / np.pi * h - 0.5, 0.0, h - 1.0)
        u = (np.arctan2(d[..., 1], d[..., 0]) / (2.0 * np.pi) % 1.0) * w - 0.5
        v0 = np.floor(v).astype(np.int64)
        u0 = np.floor(u).astype(np.int64)
        tv, tu = (v - v0)[..., None], (u - u0)[..., None]
        v1 = np.minimum(v0 + 1, h - 1)
        u0, u1 = u0 % w, (u0 + 1) % w
        top = img[v0, u0] + (img[v0, u1] - img[v0, u0]) * tu
        bot = img[v1, u0] + (img[v1, u1] - img[v1, u0]) * tu
        return cls((top + (bot - top) * tv).astype(np.float32), rotation=_up_rotation(up))


class Scene:
    """Scene (Scene.h:21-40).  ``Scene(config_path)`` parses a Config.txt
    grammar file; ``Scene()`` starts empty for programmatic construction."""

    def __init__(self, config: str | None = None):
        self._h = lib().pt_scene_create()
        if not self._h:
            raise PathTracerError("pt_scene_create failed")
        if config is not None:
            _err(lib().pt_scene_load_config(self._h, os.fsencode(config)), f"load {config}")

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.pt_scene_destroy(h)
            self._h = None

    def apply_settings(self, cfg: RenderConfig) -> RenderConfig:
        c = cfg.c()
        _err(lib().pt_scene_apply_settings(self._h, ctypes.byref(c)), "apply_settings")
        cfg.width, cfg.height, cfg.iterations, cfg.max_bounces, cfg.accel = (
            c.width, c.height, c.iterations, c.max_bounces, c.accel)
        cfg.grid = tuple(c.grid)
        return cfg

    def camera(self, width: int, height: int) -> Camera | None:
        """The view the config's RENDER block set (camera_eye, camera_target, ...) for a
        ``width`` x ``height`` frame, or None when it set none (pt_scene_camera)."""
        out = _Camera()
        rc = _err(lib().pt_scene_camera(self._h, int(width), int(height), ctypes.byref(out)), "scene camera")
        return Camera.from_c(out) if rc > 0 else None

    def direct_light(self) -> bool:
        """Whether the config's RENDER block asked for direct lighting (direct_light: 1)."""
        return bool(_err(lib().pt_scene_direct_light(self._h), "scene direct_light"))

    def lights(self) -> dict:
        """The light table of direct lighting for the scene as it stands (pt_scene_lights): the
        world-space triangles of every EMISSIVE model; see ``Renderer.lights``."""
        return _light_table(lambda n, recs, area: lib().pt_scene_lights(self._h, n, recs, area), "scene lights")

    def loadAndProcessMeshFile(self, path: str) -> int:
        return _err(lib().pt_scene_load_obj(self._h, os.fsencode(path)), f"load {path}")

    def addMesh(self, pos, nrm, tris) -> int:
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(nrm, np.float32).reshape(-1, 3)
        tris = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
        return _err(lib().pt_scene_add_mesh(self._h, _fp(pos), _fp(nrm), len(pos), _ip(tris), len(tris)), "addMesh")

    def addModel(self, mesh: int, scale, rot_deg, translate, material, color, smooth: bool = False,
                 texture: int | None = None, ior: float | None = None) -> int:
        mt = MATERIALS[material] if isinstance(material, str) else int(material)
        s = np.array(scale, np.float32); r = np.array(rot_deg, np.float32)
        t = np.array(translate, np.float32); c = np.array(color, np.float32)
        m = _err(lib().pt_scene_add_model(self._h, int(mesh), _fp(s), _fp(r), _fp(t), mt, _fp(c)), "addModel")
        if smooth:
            self.set_smooth(m)
        if texture is not None:
            self.set_texture(m, texture)
        if ior is not None:
            self.set_ior(m, ior)
        return m

    def set_mesh_uv(self, mesh: int, uv) -> None:
        """Per-vertex (u, v) of ``mesh``, one row per vertex in ``addMesh``'s order
        (pt_scene_set_mesh_uv).  The grid and the BLAS are not touched."""
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        _err(lib().pt_scene_set_mesh_uv(self._h, int(mesh), _fp(uv), len(uv)), "set_mesh_uv")

    def mesh_has_uv(self, mesh: int) -> bool:
        return _err(lib().pt_scene_mesh_has_uv(self._h, int(mesh)), "mesh_has_uv") != 0

    def add_texture(self, rgb) -> int:
        """An (h, w, 3) array of linear RGB texels -> the texture's index (pt_scene_add_texture)."""
        t = np.ascontiguousarray(rgb, np.float32)
        if t.ndim != 3 or t.shape[2] != 3:
            raise PathTracerError("add_texture: texels must have shape (h, w, 3)")
        return _err(lib().pt_scene_add_texture(self._h, t.shape[1], t.shape[0], _fp(t)), "add_texture")

    def set_texture(self, model: int | None = None, texture: int | None = None) -> None:
        """Bind ``texture`` (None: no texture) as the albedo of ``model`` (None: every model added
        so far) (pt_scene_set_model_texture).  Before or after ``build``; a renderer reads the
        bindings in ``allocateOnGPU``."""
        _err(lib().pt_scene_set_model_texture(self._h, -1 if model is None else int(model),
                                              -1 if texture is None else int(texture)), "set_texture")

    def model_textures(self) -> np.ndarray:
        """The texture index of every model, -1 for none (pt_scene_model_texture)."""
        out = []
        for i in range(self.counts()["nmodel"]):
            t = lib().pt_scene_model_texture(self._h, i)
            if t < -1:
                _err(-1, "model_textures")
            out.append(t)
        return np.array(out, np.int32)

    def textures(self) -> list:
        """Every texture as an (h, w, 3) float32 array (pt_scene_texture)."""
        out = []
        for i in range(_err(lib().pt_scene_texture_count(self._h), "textures")):
            w = ctypes.c_int(); h = ctypes.c_int()
            _err(lib().pt_scene_texture(self._h, i, ctypes.byref(w), ctypes.byref(h), None), "textures")
            t = np.zeros((h.value, w.value, 3), np.float32)
            _err(lib().pt_scene_texture(self._h, i, None, None, _fp(t)), "textures")
            out.append(t)
        return out

    def set_smooth(self, model: int | None = None, on: bool = True) -> None:
        """Shade ``model`` (None: every model added so far) with the interpolated vertex normals
        instead of one normal per triangle (pt_scene_set_model_smooth).  Any time after the model
        exists, before or after ``build``; a renderer reads the flags in ``allocateOnGPU``."""
        _err(lib().pt_scene_set_model_smooth(self._h, -1 if model is None else int(model), 1 if on else 0),
             "set_smooth")

    def smooth(self) -> np.ndarray:
        """The smooth flag of every model, a bool array (pt_scene_model_smooth)."""
        n = self.counts()["nmodel"]
        return np.array([_err(lib().pt_scene_model_smooth(self._h, i), "smooth") != 0 for i in range(n)], bool)

    def set_ior(self, model: int | None = None, ior: float = 1.5) -> None:
        """The index of refraction of ``model`` (None: every model added so far), finite and in
        [1, 4] (pt_scene_set_model_ior).  Stored for every model, read only by a DIELECTRIC one.
        Before or after ``build``; a renderer reads the values in ``allocateOnGPU``."""
        _err(lib().pt_scene_set_model_ior(self._h, -1 if model is None else int(model), float(ior)), "set_ior")

    def ior(self, model: int) -> float:
        """The index of refraction of ``model``, 1.5 unless set (pt_scene_model_ior)."""
        v = lib().pt_scene_model_ior(self._h, int(model))
        if v < 0:
            _err(-1, "ior")
        return float(v)

    def build(self, grid=(25, 25, 25), bvh: bool = True) -> None:
        """addMeshesToGrid (grid) + the per-mesh BLAS that ACCEL_GRID_FAST / ACCEL_BVH
        traverse (``bvh=False``: grid only; allocateOnGPU then adds the BLAS on demand)."""
        g = (ctypes.c_int * 3)(*grid)
        _err(lib().pt_scene_build(self._h, g, 1 if bvh else 0), "build")

    def counts(self) -> dict:
        c = (ctypes.c_int * 9)()
        _err(lib().pt_scene_counts(self._h, c), "counts")
        keys = ["nv", "nt", "nmesh", "nmodel", "ngrid", "nvox", "npv", "nbvh_nodes", "nbvh_refs"]
        return dict(zip(keys, list(c)))

    def export(self) -> dict:
        """Flat copy of Scene.h's member vectors (same layout as oracle.FlatScene)."""
        n = self.counts()
        a = dict(
            vpos=np.zeros((n["nv"], 3), np.float32), vnrm=np.zeros((n["nv"], 3), np.float32),
            tris=np.zeros((n["nt"], 3), np.int32), mesh_ranges=np.zeros((n["nmesh"], 4), np.int32),
            mesh_bbox=np.zeros((n["nmesh"], 6), np.float32), model_ints=np.zeros((n["nmodel"], 3), np.int32),
            model_m2w=np.zeros((n["nmodel"], 16), np.float32), model_w2m=np.zeros((n["nmodel"], 16), np.float32),
            model_color=np.zeros((n["nmodel"], 3), np.float32), grid_ints=np.zeros((n["ngrid"], 4), np.int32),
            grid_vw=np.zeros((n["ngrid"], 3), np.float32), vox=np.zeros((n["nvox"], 3), np.int32),
            per_voxel=np.zeros(max(n["npv"], 1), np.int32))
        _err(lib().pt_scene_export(
            self._h, _fp(a["vpos"]), _fp(a["vnrm"]), _ip(a["tris"]), _ip(a["mesh_ranges"]), _fp(a["mesh_bbox"]),
            _ip(a["model_ints"]), _fp(a["model_m2w"]), _fp(a["model_w2m"]), _fp(a["model_color"]),
            _ip(a["grid_ints"]), _fp(a["grid_vw"]), _ip(a["vox"]), _ip(a["per_voxel"])), "export")
        a["per_voxel"] = a["per_voxel"][:n["npv"]]
        a["uv"] = np.zeros((n["nv"], 2), np.float32)
        _err(lib().pt_scene_export_uv(self._h, _fp(a["uv"])), "export uv")
        return a


def _scene_export_bvh(self) -> dict:
    n = self.counts()
    nodes = np.zeros((max(n["nbvh_nodes"], 1), 16), np.float32)
    refs = np.zeros(max(n["nbvh_refs"], 1), np.int32)
    roots = np.zeros(max(n["nmesh"], 1), np.int32)
    _err(lib().pt_scene_export_bvh(self._h, _fp(nodes), _ip(refs), _ip(roots)), "export_bvh")
    return dict(nodes=nodes[:n["nbvh_nodes"]], refs=refs[:n["nbvh_refs"]], roots=roots[:n["nmesh"]])


Scene.export_bvh = _scene_export_bvh


def _scene_export_bvh4(self) -> dict:
    """The 4-wide collapse of the BLAS (Bvh4Node: 32 words per node), each
    mesh's 4-wide root (-1: none; the 4-wide traces then refuse the scene) and
    each mesh's first leaf record (`leaf_base`: a leaf link's `first` is
    relative to it)."""
    n = self.counts()
    roots = np.zeros(max(n["nmesh"], 1), np.int32)
    cnt = _err(lib().pt_scene_export_bvh4(self._h, None, _ip(roots)), "export_bvh4")
    nodes = np.zeros((max(cnt, 1), 32), np.float32)
    _err(lib().pt_scene_export_bvh4(self._h, _fp(nodes), _ip(roots)), "export_bvh4")
    base = np.zeros(max(n["nmesh"], 1), np.int32)
    _err(lib().pt_scene_export_bvh4_leaf_base(self._h, _ip(base)), "export_bvh4_leaf_base")
    return dict(nodes=nodes[:cnt], roots=roots[:n["nmesh"]], leaf_base=base[:n["nmesh"]])


Scene.export_bvh4 = _scene_export_bvh4




def selftest_math(x, y) -> np.ndarray:
    """Device evaluation of the kernels' sin/cos/pow/sqrt/div (n x 5)."""
    x = np.ascontiguousarray(x, np.float32); y = np.ascontiguousarray(y, np.float32)
    out = np.zeros((len(x), 5), np.float32)
    _err(lib().pt_selftest_math(len(x), _fp(x), _fp(y), _fp(out)), "selftest_math")
    return out


def selftest_dielectric(dirs, normals, ior, u):
    """Device evaluation of the dielectric material's definition (pt_selftest_dielectric):
    ``dirs`` (n, 3) are normalised first, ``normals`` (n, 3) and ``ior`` (n) used as given, ``u``
    (n) takes the place of the draw.  Returns (directions (n, 3), events (n): 0 refraction
    entering, 1 refraction leaving, 2 Fresnel reflection, 3 total internal reflection)."""
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    nr = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    n = len(d)
    io = np.ascontiguousarray(np.broadcast_to(np.asarray(ior, np.float32), (n,)))
    uu = np.ascontiguousarray(np.broadcast_to(np.asarray(u, np.float32), (n,)))
    if len(nr) != n:
        raise PathTracerError("selftest_dielectric: dirs and normals differ in length")
    out = np.zeros((n, 3), np.float32)
    ev = np.zeros(n, np.int32)
    _err(lib().pt_selftest_dielectric(n, _fp(d), _fp(nr), _fp(io), _fp(uu), _fp(out), _ip(ev)), "selftest_dielectric")
    return out, ev


class Renderer:
    """Renderer (Renderer.h:46-55) on the gfx950 wavefront pipeline."""

    def __init__(self, cfg: RenderConfig | None = None):
        self.cfg = cfg or RenderConfig()
        self._c = self.cfg.c()
        self._h = lib().pt_renderer_create(ctypes.byref(self._c))
        if not self._h:
            _err(-1, "pt_renderer_create")
        self._image_ref = None
        self._m2_ref = None
        self._denoise_ref = None

    def set_stream(self, hip_stream: int) -> None:
        _err(lib().pt_renderer_set_stream(self._h, ctypes.c_void_p(int(hip_stream))), "set_stream")

    def bind_image(self, device_ptr: int, keepalive=None) -> None:
        self._image_ref = keepalive
        _err(lib().pt_renderer_bind_image(self._h, ctypes.c_void_p(int(device_ptr))), "bind_image")

    def allocateOnGPU(self, scene: Scene) -> None:
        self._scene = scene
        _err(lib().pt_renderer_allocate_on_gpu(self._h, scene._h), "allocateOnGPU")

    def clearImage(self) -> None:
        _err(lib().pt_renderer_clear_image(self._h), "clearImage")

    def renderLoop(self, first_iter: int = 0, n_iters: int | None = None, sync: bool = True) -> None:
        n = self.cfg.iterations if n_iters is None else n_iters
        _err(lib().pt_renderer_render_loop(self._h, int(first_iter), int(n)), "renderLoop")
        if sync:
            self.synchronize()

    def synchronize(self) -> None:
        _err(lib().pt_renderer_synchronize(self._h), "synchronize")

    def image(self) -> np.ndarray:
        out = np.zeros((self.cfg.width * self.cfg.height, 3), np.float32)
        _err(lib().pt_renderer_read_image(self._h, _fp(out)), "read_image")
        return out

    def renderImage(self, path: str = "Render.bmp", iterations_total: int | None = None) -> None:
        it = self.cfg.iterations if iterations_total is None else iterations_total
        _err(lib().pt_renderer_render_image(self._h, os.fsencode(path), int(it)), "renderImage")

    def segments(self) -> int:
        v = lib().pt_renderer_segments(self._h)
        return _err(v, "segments")

    def trace_faults(self) -> int:
        """Persistent-trace waves that gave up at the iteration cap (0 in a correct
        run; non-zero also makes synchronize() / image() raise)."""
        return _err(lib().pt_renderer_trace_faults(self._h), "trace_faults")

    def segments_per_bounce(self, n: int = 64) -> list:
        out = (ctypes.c_longlong * n)()
        _err(lib().pt_renderer_segments_per_bounce(self._h, out, n), "segments_per_bounce")
        return list(out)

    def pipelines(self) -> int:
        """Iterations in flight (own HIP streams) once allocated."""
        return _err(lib().pt_renderer_pipelines(self._h), "pipelines")

    def set_profiling(self, on) -> None:
        """HIP-event timing: False/0 off, True/1 every kernel group, 2 pipeline 0's trace phases only."""
        _err(lib().pt_renderer_set_profiling(self._h, int(on)), "set_profiling")

    def kernel_stats(self) -> dict:
        st = (ctypes.c_double * 11)()
        _err(lib().pt_renderer_kernel_stats_ex(self._h, st, 11), "kernel_stats")
        return dict(bounce_ms=st[0], scan_ms=st[1], primary_ms=st[2],
                    bounce_launches=int(st[3]), scan_launches=int(st[4]),
                    first_ms=st[5], first_launches=int(st[6]),
                    trace_ms=st[7], trace_launches=int(st[8]),
                    sort_ms=st[9], sort_launches=int(st[10]))

    def deferred_rays(self) -> int:
        """Rays k_trace_deferred traced since allocateOnGPU (grid_fast hit sets beyond
        the overflow pool, or undecided walks beyond the hand-on records' room)."""
        return self.segments_per_bounce(_DEFERRED_SLOT + 1)[_DEFERRED_SLOT]

    def primary_hits(self):
        n = self.cfg.width * self.cfg.height
        if self.cfg.tail_drop:
            n = (n // 32) * 32
        d = np.zeros(n, np.float32); nn = np.zeros((n, 3), np.float32); m = np.zeros(n, np.int32)
        _err(lib().pt_renderer_primary_hits(self._h, _fp(d), _fp(nn), _ip(m)), "primary_hits")
        return d, nn, m

    def primary_albedo(self) -> np.ndarray:
        """The albedo of each pixel's cached primary hit, (W*H, 3): the model colour times its
        texture's value at the hit; zero for a miss (pt_renderer_primary_albedo)."""
        out = np.zeros((self.cfg.width * self.cfg.height, 3), np.float32)
        _err(lib().pt_renderer_primary_albedo(self._h, _fp(out)), "primary_albedo")
        return out

    def hit_albedo(self, orig, dirs, dist, model, tri) -> np.ndarray:
        """Test hook: the albedo definition on the device for caller-given hits, the
        ``(dist, model, tri)`` of ``trace_rays`` (pt_renderer_hit_albedo) -> (n, 3)."""
        o = np.ascontiguousarray(orig, np.float32).reshape(-1, 3)
        dd = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(dist, np.float32).reshape(-1)
        m = np.ascontiguousarray(model, np.int32).reshape(-1)
        tr = np.ascontiguousarray(tri, np.int32).reshape(-1)
        if not (len(o) == len(dd) == len(t) == len(m) == len(tr)):
            raise PathTracerError("hit_albedo: arrays differ in length")
        out = np.zeros((len(o), 3), np.float32)
        _err(lib().pt_renderer_hit_albedo(self._h, len(o), _fp(o), _fp(dd), _fp(t), _ip(m), _ip(tr), _fp(out)), "hit_albedo")
        return out

    def intersect_rays(self, orig, dirs):
        o = np.ascontiguousarray(orig, np.float32).reshape(-1, 3)
        dd = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = len(o)
        t = np.zeros(n, np.float32); nn = np.zeros((n, 3), np.float32); m = np.zeros(n, np.int32)
        _err(lib().pt_renderer_intersect_rays(self._h, n, _fp(o), _fp(dd), _fp(t), _fp(nn), _ip(m)), "intersect_rays")
        return t, nn, m

    def certify_check(self, orig, dirs):
        """grid_fast test hook: per ray, (fast certificates tried, accepted,
        accepted but disagreeing with the exact walk, full certificates
        disagreeing) -- an (n, 4) int32 array; both disagreement columns must be 0."""
        o = np.ascontiguousarray(orig, np.float32).reshape(-1, 3)
        dd = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        out = np.zeros((len(o), 4), np.int32)
        _err(lib().pt_renderer_certify_check(self._h, len(o), _fp(o), _fp(dd), _ip(out)), "certify_check")
        return out

    def trace_rays(self, orig, dirs, block_counts=None):
        """Test hook (accel bvh / grid_fast): the rays through the persistent trace
        kernels as bounce 1 of an iteration runs them (k_scan, ray sort, main and tail
        launches, k_trace_deferred) -> (dist, normal, model, tri) per ray.
        ``block_counts``: the survivor layout, rays per source block of ``cfg.block``
        pool positions (None: dense)."""
        o = np.ascontiguousarray(orig, np.float32).reshape(-1, 3)
        dd = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = len(o)
        t = np.zeros(n, np.float32); nn = np.zeros((n, 3), np.float32)
        m = np.zeros(n, np.int32); tri = np.zeros(n, np.int32)
        bc = None if block_counts is None else np.ascontiguousarray(block_counts, np.int32).reshape(-1)
        _err(lib().pt_renderer_trace_rays(self._h, n, _fp(o), _fp(dd), None if bc is None else _ip(bc),
                                          0 if bc is None else len(bc), _fp(t), _fp(nn), _ip(m), _ip(tri)), "trace_rays")
        return t, nn, m, tri

    def enable_moments(self, device_ptr: int | None = None, keepalive=None) -> None:
        """Keep the per-pixel sum of squared contributions beside the image (before
        allocateOnGPU).  ``device_ptr``: a caller-owned W*H*3 float buffer (a torch
        tensor, kept alive by ``keepalive``); None: the renderer allocates it."""
        self._m2_ref = keepalive
        _err(lib().pt_renderer_enable_moments(self._h, ctypes.c_void_p(int(device_ptr)) if device_ptr else None),
             "enable_moments")

    def moments(self) -> np.ndarray:
        out = np.zeros((self.cfg.width * self.cfg.height, 3), np.float32)
        _err(lib().pt_renderer_read_moments(self._h, _fp(out)), "read_moments")
        return out

    def enable_guides(self, device_ptr: int | None = None, keepalive=None) -> None:
        """Accumulate the first hit's features (normal, depth, sqrt albedo, hit flag) of every
        jittered or lens sample beside the image and the moments (before allocateOnGPU; needs
        enable_moments; include/pathtracer_amd.h, pt_renderer_enable_guides).  ``device_ptr``: a
        caller-owned W*H*8 float buffer (a torch tensor, kept alive by ``keepalive``); None: the
        renderer allocates it."""
        self._guides_ref = keepalive
        _err(lib().pt_renderer_enable_guides(self._h, ctypes.c_void_p(int(device_ptr)) if device_ptr else None),
             "enable_guides")

    def guides(self) -> dict:
        """The sums G per pixel: ``normal`` (N, 3), ``depth`` (N,), ``sqrt_albedo`` (N, 3) and
        ``hits`` (N,), float32; divide by ``hits`` for the means."""
        g = np.zeros((self.cfg.width * self.cfg.height, 8), np.float32)
        _err(lib().pt_renderer_read_guides(self._h, _fp(g)), "read_guides")
        return dict(normal=g[:, 0:3].copy(), depth=g[:, 3].copy(), sqrt_albedo=g[:, 4:7].copy(), hits=g[:, 7].copy())

    def guide_counts(self) -> np.ndarray:
        """Samples per tile that accumulated guides since allocateOnGPU / clearImage,
        (ceil(H/16), ceil(W/16)) int32."""
        out = np.zeros(self._tiles(), np.int32)
        _err(lib().pt_renderer_guide_counts(self._h, _ip(out)), "guide_counts")
        return out

    def noise(self, samples: int | None = None) -> dict:
        """Relative noise estimate of the accumulated image (include/pathtracer_amd.h,
        pt_renderer_noise): ``mean`` over the frame, ``max_tile`` and the ``tiles``
        map, (ceil(H/16), ceil(W/16)) float32.  ``samples``: None = the iterations
        rendered since allocateOnGPU / clearImage."""
        ty, tx = (self.cfg.height + NOISE_TILE - 1) // NOISE_TILE, (self.cfg.width + NOISE_TILE - 1) // NOISE_TILE
        tiles = np.zeros((ty, tx), np.float32)
        mean, mx = ctypes.c_double(), ctypes.c_float()
        _err(lib().pt_renderer_noise(self._h, int(samples or 0), ctypes.byref(mean), ctypes.byref(mx), _fp(tiles)), "noise")
        return dict(mean=mean.value, max_tile=np.float32(mx.value), tiles=tiles)

    def render_until(self, target: float, max_iters: int, min_iters: int = 2, check_every: int = 32,
                     first_iter: int = 0):
        """Render in chunks of ``check_every`` iterations until the mean noise estimate
        is at most ``target`` or ``max_iters`` are done -> (converged, iters, mean)."""
        done, mean = ctypes.c_int(), ctypes.c_double()
        rc = _err(lib().pt_renderer_render_until(self._h, int(first_iter), int(min_iters), int(max_iters), int(check_every),
                                                 float(target), ctypes.byref(done), ctypes.byref(mean)), "render_until")
        return bool(rc), done.value, mean.value

    def denoise(self, samples: int | None = None, passes: int = 5, sigma_l: float = 4.0, sigma_z: float = 1.0,
                out_ptr: int | None = None, keepalive=None, variance: bool = False, demodulate: bool = False,
                tile_counts: bool = False, flags: int | None = None, sampled_guides: bool = False):
        """Variance-guided edge-avoiding filter of the accumulated mean image
        (include/pathtracer_amd.h, pt_renderer_denoise; needs enable_moments) -> the
        denoised (W*H, 3) float32 image, with ``variance=True`` (image, var (W*H,)).
        ``samples``: None = the iterations rendered since allocateOnGPU / clearImage (a
        caller who reduced shards into bound tensors passes the total).  ``out_ptr``: a
        caller-owned W*H*3 float device buffer (a torch tensor, kept alive by
        ``keepalive``) that receives the image too.  The image and the moments are not
        modified.  ``demodulate``: filter the image divided by the primary hit's albedo and
        multiply it back (DENOISE_DEMODULATE); ``tile_counts``: divide by each tile's own
        sample count, after masked or adaptive iterations (DENOISE_TILE_COUNTS);
        ``sampled_guides``: guide the filter by the means of the samples' own first hits
        (DENOISE_SAMPLED_GUIDES; needs enable_guides and jittered or lens iterations only); each
        goes through pt_renderer_denoise_ex, as does an explicit ``flags`` word."""
        self._denoise_ref = keepalive
        p = _DenoiseParams(int(passes), float(sigma_l), float(sigma_z))
        img = np.zeros((self.cfg.width * self.cfg.height, 3), np.float32)
        var = np.zeros(self.cfg.width * self.cfg.height, np.float32) if variance else None
        out = ctypes.c_void_p(int(out_ptr)) if out_ptr else None
        if flags is None and not demodulate and not tile_counts and not sampled_guides:
            _err(lib().pt_renderer_denoise(self._h, int(samples or 0), ctypes.byref(p), out, _fp(img),
                                           _fp(var) if variance else None), "denoise")
        else:
            _err(lib().pt_renderer_denoise_ex(self._h, int(samples or 0), ctypes.byref(p),
                                              _denoise_flags(demodulate, tile_counts, flags, sampled_guides), out,
                                              _fp(img),
                                              _fp(var) if variance else None), "denoise")
        return (img, var) if variance else img

    def renderImageDenoised(self, path: str = "Render.bmp", samples: int | None = None, passes: int = 5,
                            sigma_l: float = 4.0, sigma_z: float = 1.0, demodulate: bool = False,
                            tile_counts: bool = False, flags: int | None = None, sampled_guides: bool = False) -> None:
        """The BMP of the denoised mean (renderImage's conversion of D * 255); ``demodulate``,
        ``tile_counts``, ``sampled_guides`` and ``flags`` as for denoise()."""
        p = _DenoiseParams(int(passes), float(sigma_l), float(sigma_z))
        if flags is None and not demodulate and not tile_counts and not sampled_guides:
            _err(lib().pt_renderer_render_image_denoised(self._h, os.fsencode(path), int(samples or 0), ctypes.byref(p)),
                 "renderImageDenoised")
        else:
            _err(lib().pt_renderer_render_image_denoised_ex(self._h, os.fsencode(path), int(samples or 0), ctypes.byref(p),
                                                            _denoise_flags(demodulate, tile_counts, flags, sampled_guides)),
                 "renderImageDenoised")

    def denoise_times(self) -> dict:
        """HIP-event times (ms) of the last denoise() made with set_profiling on: ``prep``,
        ``passes`` (one per pass run), ``out`` (the copy into ``out_ptr``), ``total`` and
        ``remod`` (the remodulation of ``demodulate``; 0 when not run)."""
        ms = (ctypes.c_double * 10)()
        _err(lib().pt_renderer_denoise_times(self._h, ms, 10), "denoise_times")
        return dict(prep=ms[0], passes=[ms[1 + i] for i in range(DENOISE_MAX_PASSES)], out=ms[7], total=ms[8], remod=ms[9])

    def _tiles(self):
        return (self.cfg.height + NOISE_TILE - 1) // NOISE_TILE, (self.cfg.width + NOISE_TILE - 1) // NOISE_TILE

    def render_masked(self, mask=None, first_iter: int = 0, n_iters: int | None = None, sync: bool = True) -> None:
        """Iterations that sample only the 16 x 16 tiles whose ``mask`` entry is non-zero
        ((ceil(H/16), ceil(W/16)), any integer or bool dtype; None: every tile); needs
        enable_moments (include/pathtracer_amd.h, pt_renderer_render_loop_masked).  The
        mask is copied before the call returns."""
        n = self.cfg.iterations if n_iters is None else n_iters
        ptr = None
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
            if m.shape != self._tiles():
                raise PathTracerError(f"render_masked: mask shape {m.shape}, tiles {self._tiles()}")
            ptr = m.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte))
        _err(lib().pt_renderer_render_loop_masked(self._h, int(first_iter), int(n), ptr), "render_masked")
        if sync:
            self.synchronize()

    def sample_counts(self) -> np.ndarray:
        """Samples per tile since allocateOnGPU / clearImage, (ceil(H/16), ceil(W/16)) int32."""
        out = np.zeros(self._tiles(), np.int32)
        _err(lib().pt_renderer_sample_counts(self._h, _ip(out)), "sample_counts")
        return out

    def adaptive_noise(self) -> dict:
        """noise() with each tile's own sample count (pt_renderer_adaptive_noise): ``mean``,
        ``max_tile`` and the ``tiles`` map; a tile with fewer than 2 samples reads inf."""
        tiles = np.zeros(self._tiles(), np.float32)
        mean, mx = ctypes.c_double(), ctypes.c_float()
        _err(lib().pt_renderer_adaptive_noise(self._h, ctypes.byref(mean), ctypes.byref(mx), _fp(tiles)), "adaptive_noise")
        return dict(mean=mean.value, max_tile=np.float32(mx.value), tiles=tiles)

    def adaptive_mean(self, out_ptr: int | None = None, keepalive=None) -> np.ndarray:
        """The mean image S / count[tile] (0 where a tile has no sample), (W*H, 3) float32.
        ``out_ptr``: a caller-owned W*H*3 float device buffer that receives it too."""
        self._adaptive_ref = keepalive
        img = np.zeros((self.cfg.width * self.cfg.height, 3), np.float32)
        _err(lib().pt_renderer_adaptive_mean(self._h, ctypes.c_void_p(int(out_ptr)) if out_ptr else None, _fp(img)),
             "adaptive_mean")
        return img

    def renderImageAdaptive(self, path: str = "Render.bmp") -> None:
        """The BMP of adaptive_mean() (renderImage's conversion of M * 255)."""
        _err(lib().pt_renderer_render_image_adaptive(self._h, os.fsencode(path)), "renderImageAdaptive")

    def render_adaptive(self, tile_target: float, max_iters: int, min_iters: int = 2, check_every: int = 32,
                        first_iter: int = 0):
        """Render masked chunks of ``check_every`` iterations, switching off every tile whose
        estimate is at most ``tile_target``, until none is active or ``max_iters`` are done
        -> (converged, iters, pixel_samples, mean)."""
        done, taken, mean = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_double()
        rc = _err(lib().pt_renderer_render_adaptive(self._h, int(first_iter), int(min_iters), int(max_iters),
                                                    int(check_every), float(tile_target), ctypes.byref(done),
                                                    ctypes.byref(taken), ctypes.byref(mean)), "render_adaptive")
        return bool(rc), done.value, taken.value, mean.value

    def set_pixel_jitter(self, width: float = 1.0, on: bool = True) -> None:
        """Anti-aliasing (include/pathtracer_amd.h, pt_renderer_set_pixel_jitter): while on,
        every iteration enqueued sends each pixel's camera ray through a point drawn from a
        ``width``-pixel square about the pixel's own point, per (iteration, pixel).  Host
        state: before or after allocateOnGPU, between render calls, no synchronize needed.
        Width 0 reproduces the unjittered render bit for bit."""
        _err(lib().pt_renderer_set_pixel_jitter(self._h, 1 if on else 0, float(width)), "set_pixel_jitter")

    def pixel_jitter(self):
        """The current setting -> (on, width); (False, 1.0) until set."""
        on, width = ctypes.c_int(), ctypes.c_float()
        _err(lib().pt_renderer_pixel_jitter(self._h, ctypes.byref(on), ctypes.byref(width)), "pixel_jitter")
        return bool(on.value), float(width.value)

    def set_camera(self, cam: Camera | None) -> None:
        """A free view (include/pathtracer_amd.h, pt_renderer_set_camera) for the iterations
        enqueued from now on; None: back to the config's legacy camera.  Before or after
        allocateOnGPU; after it the call starts a new render (image, moments and sample counts
        read zero) and needs no synchronize.  A pinhole with the jitter off keeps the ordinary
        loop; a lens (``lens_radius`` > 0) or the jitter generates the rays per iteration."""
        _err(lib().pt_renderer_set_camera(self._h, ctypes.byref(cam.c()) if cam is not None else None), "set_camera")

    def camera(self):
        """-> (is_set, Camera): the camera in use; for the legacy camera (False) the general
        camera with the same rays."""
        out = _Camera()
        rc = _err(lib().pt_renderer_camera(self._h, ctypes.byref(out)), "camera")
        return bool(rc), Camera.from_c(out)

    def set_environment(self, env: Environment | None) -> None:
        """What a missing ray brings back (include/pathtracer_amd.h, pt_renderer_set_environment)
        for the iterations enqueued from now on; None: back to the constant 0.01.  Before or
        after allocateOnGPU; after it, a new environment starts a new render."""
        _err(lib().pt_renderer_set_environment(self._h, ctypes.byref(env.c()) if env is not None else None),
             "set_environment")

    def environment(self) -> Environment | None:
        """The environment in use (a copy), or None."""
        c = _Environment()
        if not _err(lib().pt_renderer_environment(self._h, ctypes.byref(c), None), "environment"):
            return None
        t = np.empty((c.n, c.n, 3), np.float32)
        _err(lib().pt_renderer_environment(self._h, None, _fp(t)), "environment")
        return Environment(t, tuple(c.scale), np.array(list(c.rotation), np.float32).reshape(3, 3))

    def environment_lookup(self, dirs) -> np.ndarray:
        """Test hook: the device's lookup (texel times scale) for each of the (n, 3) directions."""
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        out = np.empty_like(d)
        _err(lib().pt_renderer_env_lookup(self._h, len(d), _fp(d), _fp(out)), "env_lookup")
        return out

    def set_direct_light(self, on: bool = True) -> None:
        """Direct lighting (include/pathtracer_amd.h, "Direct lighting"): while on, every diffuse
        hit samples one point of one EMISSIVE triangle through a shadow ray.  Needs moments, the
        split trace (not ACCEL_GRID) and max_bounces <= 63.  Before or after allocateOnGPU; a
        change after it starts a new render."""
        _err(lib().pt_renderer_set_direct_light(self._h, 1 if on else 0), "set_direct_light")

    def direct_light(self):
        """-> (on, lights, area): the switch, and the allocation's light count and total area."""
        on, n, area = ctypes.c_int(), ctypes.c_int(), ctypes.c_float()
        _err(lib().pt_renderer_direct_light(self._h, ctypes.byref(on), ctypes.byref(n), ctypes.byref(area)), "direct_light")
        return bool(on.value), int(n.value), float(area.value)

    def lights(self) -> dict:
        """The allocation's light table (pt_renderer_lights): dict(p0, e1, e2, nl, emission (n, 3),
        area, cdf (n,), model (n,), area_total); empty before allocateOnGPU."""
        return _light_table(lambda n, recs, area: lib().pt_renderer_lights(self._h, n, recs, area), "lights")

    def occluded(self, orig, target) -> np.ndarray:
        """Test hook: the shadow-ray decision for the (n, 3) segments ``orig`` -> ``target``
        (pt_renderer_occluded) -> (n,) bool; a segment of zero length reads False."""
        o = np.ascontiguousarray(orig, np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(target, np.float32).reshape(-1, 3)
        if len(o) != len(t):
            raise PathTracerError("occluded: arrays differ in length")
        out = np.zeros(len(o), np.int32)
        _err(lib().pt_renderer_occluded(self._h, len(o), _fp(o), _fp(t), _ip(out)), "occluded")
        return out != 0

    def direct_sample(self, orig, dirs, dist, model, tri, color, it, slot, bounces) -> dict:
        """Test hook: the light sample of caller-given hits (pt_renderer_direct_sample) ->
        dict(light (n,) int32, -1 where the geometry test failed; y (n, 3); g (n,); dc (n, 3);
        visible (n,) bool)."""
        o = np.ascontiguousarray(orig, np.float32).reshape(-1, 3)
        n = len(o)
        dd = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(dist, np.float32).reshape(-1)
        m = np.ascontiguousarray(model, np.int32).reshape(-1)
        tr = np.ascontiguousarray(tri, np.int32).reshape(-1)
        c = np.ascontiguousarray(color, np.float32).reshape(-1, 3)
        ids = np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(a, np.int32), (n,)) for a in (it, slot, bounces)], 1))
        if not (len(dd) == len(t) == len(m) == len(tr) == len(c) == n):
            raise PathTracerError("direct_sample: arrays differ in length")
        of, oi = np.zeros((n, 8), np.float32), np.zeros((n, 2), np.int32)
        _err(lib().pt_renderer_direct_sample(self._h, n, _fp(o), _fp(dd), _fp(t), _ip(m), _ip(tr), _fp(c), _ip(ids), _fp(of),
                                             _ip(oi)), "direct_sample")
        return dict(light=oi[:, 0].copy(), y=of[:, 0:3].copy(), g=of[:, 3].copy(), dc=of[:, 4:7].copy(), visible=oi[:, 1] != 0)

    def free(self) -> None:
        if self._h:
            lib().pt_renderer_free(self._h)
            self._h = None

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            try:
                _lib.pt_renderer_free(self._h)
            except Exception:
                pass
            self._h = None


def render(scene_config: str, cfg: RenderConfig | None = None, bmp_out: str | None = "Render.bmp") -> None:
    """main.cpp:11-27 equivalent.  ``cfg=None``: the library's defaults
    (pt_default_config) overlaid with the scene file's RENDER block."""
    c = ctypes.byref(cfg.c()) if cfg is not None else None
    _err(lib().pt_render(os.fsencode(scene_config), c, os.fsencode(bmp_out) if bmp_out else None), "render")
