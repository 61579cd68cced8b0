"""Environment lighting's host functions (include/pathtracer_amd.h: pt_renderer_set_environment
/ pt_renderer_environment before allocation, pt_environment_sky; Python's Environment and its
constructors): no compute calls, runs without a GPU."""
import ctypes
import inspect

import numpy as np
import pytest

import env_ref as ER
from helpers import assert_bitexact

F = np.float32
UP_Y = np.float32([[0, 0, 1], [1, 0, 0], [0, 1, 0]])        # e = (u.z, u.x, u.y): the environment's +z is world +y


def random_env(P, n=8, seed=1):
    return P.Environment(np.random.RandomState(seed).uniform(0, 2, (n, n, 3)), (1.5, 1.0, 0.5), UP_Y)


def test_round_trip_before_allocation(pt_mod):
    P = pt_mod
    r = P.Renderer(P.RenderConfig(width=64, height=48))
    assert r.environment() is None
    for env in (random_env(P), random_env(P, 5, 2), P.Environment.constant(0.25), random_env(P, 1, 3)):
        r.set_environment(env)
        got = r.environment()
        assert got.n == env.n
        assert_bitexact(got.texels, env.texels, "texels")
        assert_bitexact(got.scale, env.scale, "scale")
        assert_bitexact(got.rotation, env.rotation, "rotation")
    r.set_environment(None)
    assert r.environment() is None
    r.free()


def test_refusals(pt_mod):
    P = pt_mod
    r = P.Renderer(P.RenderConfig(width=64, height=48))
    kept = random_env(P)
    r.set_environment(kept)
    bad_texel, bad_scale, bad_rot = random_env(P), random_env(P), random_env(P)
    bad_texel.texels[7, 7, 2] = np.inf
    bad_scale.scale[1] = np.nan
    bad_rot.rotation[2, 0] = -np.inf
    cases = [(P.Environment(np.zeros((0, 0, 3), F)), r"n must be 1 \.\. 2048"),
             (P.Environment(np.zeros((2049, 2049, 3), F)), r"n must be 1 \.\. 2048"),
             (bad_texel, "every texel must be finite"),
             (bad_scale, "every scale entry must be finite"),
             (bad_rot, "every rotation entry must be finite")]
    for env, msg in cases:
        with pytest.raises(P.PathTracerError, match="set_environment: " + msg):
            r.set_environment(env)
    c = kept.c()
    c.texels_rgb = None
    assert P.lib().pt_renderer_set_environment(r._h, ctypes.byref(c)) < 0
    assert P.lib().pt_last_error() == b"set_environment: null texels"
    assert P.lib().pt_renderer_set_environment(None, ctypes.byref(kept.c())) < 0
    assert P.lib().pt_last_error() == b"null renderer"
    got = r.environment()                                    # a refusal changes nothing
    assert_bitexact(got.texels, kept.texels, "texels after the refusals")
    with pytest.raises(P.PathTracerError, match="env_lookup: not allocated"):
        r.environment_lookup(np.float32([[0, 0, 1]]))
    P.Environment(np.zeros((2048, 2048, 3), F))              # the largest map is accepted by the class ...
    r.free()
    for bad in (np.zeros((4, 5, 3)), np.zeros((4, 4)), np.zeros((4, 4, 4))):
        with pytest.raises(ValueError):
            P.Environment(bad)


@pytest.mark.parametrize("n", [1, 2, 5, 64, 301])
def test_sky_equals_its_restatement(pt_mod, n):
    P = pt_mod
    zenith, horizon, ground = (0.1, 0.3, 0.9), (0.8, 0.7, 0.6), (0.05, 0.04, 0.03)
    env = P.Environment.sky(zenith, horizon, ground, n=n)
    want = ER.sky_texels(zenith, horizon, ground, n)
    assert_bitexact(env.texels, want, f"sky n {n}")
    assert_bitexact(env.rotation, UP_Y, "up = +y")
    assert_bitexact(env.scale, np.ones(3, F), "scale")
    if n >= 5:
        lookup = lambda d: ER.lookup(env.texels, env.rotation, env.scale, np.float32([d]))[0]
        # straight up is within a texel of the zenith, straight down is the ground
        assert np.abs(lookup((0, 1, 0)) - np.float32(zenith)).max() < 1.5 / n
        assert_bitexact(lookup((0, -1, 0)), np.float32(ground), "nadir")
        # the sky darkens (here: reddens) towards the horizon
        assert lookup((1, 0.2, 0))[0] > lookup((1, 2, 0))[0]
    assert_bitexact(P.Environment.sky(zenith, horizon, n=n, up=(0, 0, 1)).rotation, np.eye(3, dtype=F), "up = +z")


def test_sky_refusals(pt_mod):
    P = pt_mod
    for n in (0, -1, 2049):
        with pytest.raises(P.PathTracerError, match=r"environment_sky: n must be 1 \.\. 2048"):
            P.Environment.sky((1, 1, 1), (1, 1, 1), n=n)
    z = (ctypes.c_float * 3)(1, 1, 1)
    assert P.lib().pt_environment_sky(z, z, z, 4, None) < 0
    assert P.lib().pt_last_error() == b"environment_sky: null argument"


def test_constant(pt_mod):
    P = pt_mod
    env = P.Environment.constant((0.2, 0.4, 0.6), scale=(2, 1, 1))
    assert env.n == 1 and env.texels.dtype == F
    d = np.random.RandomState(3).normal(size=(100, 3)).astype(F)
    got = ER.lookup(env.texels, env.rotation, env.scale, d)
    assert_bitexact(got, np.broadcast_to(np.float32([0.2, 0.4, 0.6]) * np.float32([2, 1, 1]), got.shape), "constant")
    assert_bitexact(P.Environment.constant(0.01).texels, np.full((1, 1, 3), 0.01, F), "a number is a grey")


@pytest.mark.parametrize("up", [(0, 1, 0), (0, 0, 1), (1, 0, 0), (0.3, -2.0, 0.5)])
def test_up_rotation_is_a_rotation(pt_mod, up):
    P = pt_mod
    rot = P.Environment.sky((1, 1, 1), (1, 1, 1), n=1, up=up).rotation.astype(np.float64)
    unit = np.array(up, np.float64) / np.linalg.norm(up)
    # rounded once from double: each entry within 2^-24, so R R^T within a few 2^-23 of the identity
    assert np.abs(rot @ rot.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(rot) - 1) < 1e-6
    assert np.abs(rot @ unit - [0, 0, 1]).max() < 1e-6         # world up -> the environment's +z


@pytest.mark.parametrize("up", [(0, 1, 0), (0.3, -2.0, 0.5)])
def test_from_latlong(pt_mod, up):
    P = pt_mod
    const = P.Environment.from_latlong(np.full((16, 32, 3), 0.375), n=32, up=up)
    assert const.texels.shape == (32, 32, 3) and const.texels.dtype == F
    assert_bitexact(const.texels, np.full((32, 32, 3), 0.375, F), "a constant image stays constant")
    img = np.zeros((32, 64, 3))
    img[:16] = 1.0                                           # rows run from +up down: 1 above the horizon, 0 below
    env = P.Environment.from_latlong(img, n=64, up=up)
    unit = (np.array(up, np.float64) / np.linalg.norm(up)).astype(F)
    lookup = lambda d: ER.lookup(env.texels, env.rotation, env.scale, np.float32([d]))[0]
    assert_bitexact(lookup(unit), np.ones(3, F), "+up")
    assert_bitexact(lookup(-unit), np.zeros(3, F), "-up")
    # well above and well below the horizon, all the way round
    side = np.cross(unit, [0.3, 0.5, 0.8])
    side /= np.linalg.norm(side)
    other = np.cross(unit, side)
    for a in np.linspace(0, 2 * np.pi, 16, endpoint=False):
        h = np.cos(a) * side + np.sin(a) * other
        assert_bitexact(lookup(h + 0.5 * unit), np.ones(3, F), "above")
        assert_bitexact(lookup(h - 0.5 * unit), np.zeros(3, F), "below")
    # longitude: column 0 starts at the environment's +x and runs towards its +y
    lon = np.zeros((8, 64, 3))
    lon[:, :16] = 1.0                                        # the first quarter turn
    e = P.Environment.from_latlong(lon, n=64, up=(0, 0, 1))  # identity rotation: the frame is the world
    look = lambda d: ER.lookup(e.texels, e.rotation, e.scale, np.float32([d]))[0, 0]
    assert look((1, 1, 0.3)) == 1 and look((-1, 1, 0.3)) == 0 and look((-1, -1, 0.3)) == 0 and look((1, -1, 0.3)) == 0
    for bad in (np.zeros((4, 4)), np.zeros((0, 4, 3))):
        with pytest.raises(ValueError):
            P.Environment.from_latlong(bad)
    with pytest.raises(ValueError):
        P.Environment.from_latlong(img, n=4096)


def test_signatures(pt_mod):
    """The public spellings the documents use."""
    P = pt_mod
    from pathtracerap_amd.dist import render_sharded
    assert inspect.signature(render_sharded).parameters["environment"].default is None
    assert list(inspect.signature(P.Environment.sky).parameters) == ["zenith", "horizon", "ground", "n", "up"]
    assert list(inspect.signature(P.Environment.from_latlong).parameters) == ["image", "n", "up"]
    assert "Environment" in P.__all__
    names = [e[0] for e in P.EXPORTS]
    for name in ("pt_renderer_set_environment", "pt_renderer_environment", "pt_renderer_env_lookup", "pt_environment_sky"):
        assert name in names and hasattr(P.lib(), name)
