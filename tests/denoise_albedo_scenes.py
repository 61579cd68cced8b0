"""Scenes of the albedo-demodulation tests (test infrastructure).

quality_spec: one DIFFUSE triangle facing the legacy camera and filling most of a 64 x 48 frame
(its top corners and a strip below it show the environment), under a seeded high-contrast 32 x 32
texture that repeats with texels about 3 pixels wide, lit by a seeded environment map alone: every
path is camera -> face -> sky, so a sample is sqrt(albedo * sky(direction)) and the noise is the
sky's.  A single triangle, so texture_ref identifies the hit triangle trivially.

torus_spec: texture_scenes' torus fixture with its 64 x 64 texture (the first torus's) given a
block of exact zeros, texels of 1e-8 inside it and a block without red."""
import copy

import numpy as np

import texture_scenes as TS

F = np.float32
TEXEL = 45.0                     # world units per texel; a pixel of the 64 x 48 frame is about 14.4 x 15.3
TEX_N = 32
FACE = np.float32([(-1.0, -0.17, 0.0), (1.0, -0.17, 0.0), (0.0, 1.1, 0.0)])     # x1000 when loaded
UP_Y = np.float32([[0, 0, 1], [1, 0, 0], [0, 1, 0]])


def quality_texture(seed=5):
    """Every texel dark (0.03 .. 0.08) or bright (0.7 .. 1.0), chosen per texel, tinted per channel."""
    rs = np.random.RandomState(seed)
    bright = rs.rand(TEX_N, TEX_N, 1) < 0.5
    return np.where(bright, rs.uniform(0.7, 1.0, (TEX_N, TEX_N, 3)), rs.uniform(0.03, 0.08, (TEX_N, TEX_N, 3))).astype(F)


def quality_spec():
    """texture_scenes.fixture_spec's layout: dict(meshes, models, smooth, binding, mesh_uv, textures)."""
    nrm = np.tile(np.float32([0, 0, 1]), (3, 1))
    uv = (FACE[:, :2].astype(np.float64) * 1000.0 / (TEX_N * TEXEL)).astype(F)
    return dict(meshes=[(FACE, nrm, np.int32([(0, 1, 2)]))],
                models=[dict(mesh=0, scale=(1, 1, 1), rot=(0, 0, 0), translate=(0, 0, 0), material="DIFFUSE",
                             color=(0.9, 0.85, 0.8))],
                smooth=np.array([False]), binding=np.array([0], np.int64), mesh_uv={0: uv}, textures=[quality_texture()])


def quality_env(P, seed=78):
    """A seeded 8 x 8 sky with a few texels far brighter than the rest: samples of high variance."""
    rs = np.random.RandomState(seed)
    return P.Environment((rs.uniform(0, 1, (8, 8, 3)) ** 4 * 6.0 + 0.05).astype(F), (1.0, 1.0, 1.0), UP_Y)


ZERO_BLOCK = (slice(8, 40), slice(8, 40))            # rows, columns of the 64 x 64 texture
TINY_TEXELS = (slice(12, 36, 4), slice(12, 36, 4))   # inside the zero block: their neighbourhoods interpolate to (0, 1e-8]
RED_FREE_BLOCK = (slice(40, 64), slice(0, 24))


def torus_spec():
    spec = copy.deepcopy(TS.fixture_spec())
    t = spec["textures"][5]
    assert t.shape == (64, 64, 3)
    t[ZERO_BLOCK] = 0.0
    t[TINY_TEXELS] = 1e-8
    t[RED_FREE_BLOCK + (0,)] = 0.0
    return spec
