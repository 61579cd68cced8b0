"""ctypes binding of ``oracle/_ref/libptref.so``: the reference's own code,
compiled for the host by ``make -C oracle`` when the reference tree is present
(recipe and its list of differences from the CUDA build: ``oracle/ref/bridge.cpp``).

TEST INFRASTRUCTURE ONLY.  ``available()`` says whether the library was built;
nothing here reads the reference tree itself.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import FlatScene, _fp, _ip, lib as _oracle_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "libptref.so")

HEMISPHERE, METAL, COAT, REFLECT = 0, 1, 2, 3
POSITION, DIRECTION, NORMAL = 0, 1, 2
FLOAT_MAX = np.float32(9999999.0)

_lib = None


def available() -> bool:
    return os.path.exists(LIB_PATH)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _oracle_lib()       # libptref.so takes its three math functions from libptoracle.so
        L = ctypes.CDLL(LIB_PATH)
        L.ptref_u01_first.restype = ctypes.c_float
        L.ptref_u01_first.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.ptref_model_matrix.restype = None
        L.ptref_model_matrix.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p]
        _lib = L
    return _lib


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, np.float32)
    return a if shape is None else a.reshape(shape)


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def u01_first(iter_, index, depth) -> np.float32:
    return np.float32(lib().ptref_u01_first(int(iter_), int(index), int(depth)))


def scatter(kind, iters, slots, depths, normals, dirs):
    """One of the reference's scatter functions per ray, each with an engine
    seeded (iter, slot, depth).  Returns (n,3) f32."""
    normals = _f32(normals, (-1, 3)); dirs = _f32(dirs, (-1, 3))
    n = len(normals)
    iters, slots, depths = (_i32(np.broadcast_to(x, (n,))) for x in (iters, slots, depths))
    out = np.zeros((n, 3), np.float32)
    rc = lib().ptref_scatter(kind, n, _ip(iters), _ip(slots), _ip(depths), _fp(normals), _fp(dirs), _fp(out))
    if rc != 0:
        raise RuntimeError("ptref_scatter failed")
    return out


def transform(kind, m16, v):
    m16 = _f32(m16, (16,)); v = _f32(v, (-1, 3))
    out = np.zeros_like(v)
    rc = lib().ptref_transform(kind, len(v), _fp(m16), _fp(v), _fp(out))
    if rc != 0:
        raise RuntimeError("ptref_transform failed")
    return out


def model_matrix(scale, rot_y_deg, translate):
    s = _f32(scale, (3,)); t = _f32(translate, (3,))
    m2w = np.zeros(16, np.float32); w2m = np.zeros(16, np.float32)
    lib().ptref_model_matrix(s.ctypes.data, float(rot_y_deg), t.ctypes.data, m2w.ctypes.data, w2m.ctypes.data)
    return m2w, w2m


def intersect_rays(scene: FlatScene, orig, dirs, threads=0):
    """computeRaySceneIntersectionKernel per ray: (dist, normal, material type
    (-1 = miss), material colour)."""
    orig = _f32(orig, (-1, 3)); dirs = _f32(dirs, (-1, 3))
    n = len(orig)
    dist = np.zeros(n, np.float32); nrm = np.zeros((n, 3), np.float32)
    mtype = np.zeros(n, np.int32); mcol = np.zeros((n, 3), np.float32)
    cs = scene.c()
    rc = lib().ptref_intersect_rays(ctypes.byref(cs), n, _fp(orig), _fp(dirs), _fp(dist), _fp(nrm),
                                    _ip(mtype), _fp(mcol), int(threads))
    if rc != 0:
        raise RuntimeError("ptref_intersect_rays failed")
    return dist, nrm, mtype, mcol


def shade(iter_, slot, orig, dirs, color, bounces, hit_dist, hit_normal, hit_type, hit_color):
    """shadeRayKernel over a batch.  Returns new (orig, dir, color, bounces, hit_dist)."""
    orig = _f32(orig, (-1, 3)).copy(); dirs = _f32(dirs, (-1, 3)).copy(); color = _f32(color, (-1, 3)).copy()
    bounces = _i32(bounces).copy(); hit_dist = _f32(hit_dist).copy()
    slot = _i32(slot); hit_normal = _f32(hit_normal, (-1, 3)); hit_type = _i32(hit_type)
    hit_color = _f32(hit_color, (-1, 3))
    rc = lib().ptref_shade(len(orig), int(iter_), _ip(slot), _fp(orig), _fp(dirs), _fp(color), _ip(bounces),
                           _fp(hit_dist), _fp(hit_normal), _ip(hit_type), _fp(hit_color))
    if rc != 0:
        raise RuntimeError("ptref_shade failed")
    return orig, dirs, color, bounces, hit_dist


def render(scene: FlatScene, width, height, iterations, first_iter=0, tail_drop=0, threads=0, live_cap=8):
    """The reference's kernels in renderLoop's order.  Returns (accumulator
    (H*W,3) f32, live rays entering each bounce summed over iterations)."""
    image = np.zeros((width * height, 3), np.float32)
    live = np.zeros(live_cap, np.int64)
    cs = scene.c()
    rc = lib().ptref_render(ctypes.byref(cs), int(width), int(height), int(first_iter), int(iterations),
                            int(tail_drop), _fp(image), live.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
                            int(live_cap), int(threads))
    if rc != 0:
        raise RuntimeError("ptref_render failed")
    return image, live


def build_grids(scene: FlatScene):
    """Scene::addMeshesToGrid over the scene's meshes and models.  Returns
    (model grid indices, grid_ints, grid_vw, vox, per_voxel)."""
    cs = scene.c()
    G = int(np.prod(scene.gdim))
    nmesh = max(len(scene.mesh_ranges), 1)
    model_grid = np.zeros(max(len(scene.model_ints), 1), np.int32)
    grid_ints = np.zeros((nmesh, 4), np.int32); grid_vw = np.zeros((nmesh, 3), np.float32)
    vox = np.zeros((nmesh * G, 3), np.int32)
    cap = 1 << 20
    while True:
        pv = np.zeros(cap, np.int32)
        ng, nvx, npv = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        rc = lib().ptref_build_grids(ctypes.byref(cs), _ip(model_grid), ctypes.byref(ng), _ip(grid_ints),
                                     _fp(grid_vw), ctypes.byref(nvx), _ip(vox), cap, ctypes.byref(npv), _ip(pv))
        if rc == 0:
            break
        if rc == -1 or -rc <= cap:
            raise RuntimeError("ptref_build_grids failed")
        cap = -rc
    return (model_grid[:len(scene.model_ints)].copy(), grid_ints[:ng.value].copy(), grid_vw[:ng.value].copy(),
            vox[:nvx.value].copy(), pv[:npv.value].copy())
