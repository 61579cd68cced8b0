"""Environment lighting on the GPU (include/pathtracer_amd.h, pt_renderer_set_environment),
against the restatement in env_ref.py (which tests/test_env_ref.py holds to camera_ref's and
through it to the oracle) and, for the constant 0.01 map, against the renderer without an
environment.

S (image), Q (moments), the per-tile sample counts, the segment count and the per-bounce
segment counts are compared bit for bit; every render must leave trace_faults() at 0."""
import os
import subprocess

import numpy as np
import pytest

import adaptive_ref as AR
import camera_ref as CR
import denoise_ref as DR
import env_ref as ER
import path_scenes as PS
from conftest import REF_SCENE, ROOT
from helpers import assert_bitexact, flat_from_export, oracle_cfg

pytestmark = pytest.mark.gpu

F = np.float32
W, H, BOUNCES, ITERS, LENS = 64, 48, 5, 3, 25.0
VIEWS = {"A": dict(eye=(0, 800, 500), target=(0, 0, 0), vfov_deg=45, focus_dist=900),      # test_gpu_camera's
         "B": dict(eye=(650, 200, 650), target=(0, 0, 0), vfov_deg=45)}
UP_Y = np.float32([[0, 0, 1], [1, 0, 0], [0, 1, 0]])        # e = (u.z, u.x, u.y): the environment's +z is world +y
SCALE = (1.5, 1.0, 0.5)


def random_env(P, n=8, seed=77, rot=UP_Y):
    """A seeded n x n map with values in [0, 2)."""
    return P.Environment(np.random.RandomState(seed).uniform(0, 2, (n, n, 3)), SCALE, rot)


@pytest.fixture(scope="module")
def scene(pt_mod):
    s = pt_mod.Scene(REF_SCENE)
    s.build()
    return s


@pytest.fixture(scope="module")
def flat(scene):
    return flat_from_export(scene.export())


def miss_scene_spec():
    """test_gpu_denoise's: most camera rays miss.  A small emissive quad in front of the camera
    (the triangle test is one-sided, so a second one back to back with it lights what lies
    behind) and a diffuse quad behind it to the side, whose paths end on the emitter or leave
    the scene."""
    quad = PS._quads([0.0], 1.0)
    lamp = dict(mesh=0, scale=(0.1, 0.1, 0.1), translate=(-60, 120, 300), material="EMISSIVE", color=(0.99, 0.9, 0.8))
    return [quad], [dict(lamp, rot=(0, 0, 0)), dict(lamp, rot=(0, 180, 0), translate=(-60, 120, 299)),
                    dict(mesh=0, scale=(0.2, 0.2, 0.2), rot=(0, 20, 0), translate=(150, 100, 100), material="DIFFUSE",
                         color=(0.8, 0.7, 0.6))]


@pytest.fixture(scope="module")
def miss_scene(pt_mod):
    return PS.scene_from_spec(pt_mod, *miss_scene_spec())


@pytest.fixture(scope="module")
def miss_flat(miss_scene):
    return flat_from_export(miss_scene.export())


def accel_of(P, name):
    return {"grid_fast": P.ACCEL_GRID_FAST, "grid": P.ACCEL_GRID, "bvh": P.ACCEL_BVH}[name]


def make_cfg(P, accel="grid_fast", **kw):
    base = dict(width=W, height=H, max_bounces=BOUNCES, iterations=ITERS, accel=accel_of(P, accel))
    base.update(kw)
    return P.RenderConfig(**base)


def view(P, name, cfg, lens=0.0):
    return None if name is None else P.look_at(lens_radius=lens, width=cfg.width, height=cfg.height, **VIEWS[name])


def renderer(P, scene, cfg, env=None, cam=None, jitter=None, env_after=False):
    r = P.Renderer(cfg)
    r.enable_moments()
    if cam is not None:
        r.set_camera(cam)
    if jitter is not None:
        r.set_pixel_jitter(jitter)
    if env is not None and not env_after:
        r.set_environment(env)                           # before allocateOnGPU
    r.allocateOnGPU(scene)
    if env is not None and env_after:
        r.set_environment(env)
    return r


def one_tile(w, h, t):
    m = np.zeros(AR.tiles_shape(w, h), bool)
    m.reshape(-1)[t] = True
    return m


def half_mask(w, h, seed=20):
    ty, tx = AR.tiles_shape(w, h)
    m = (np.random.RandomState(seed).permutation(ty * tx) < (ty * tx) // 2).reshape(ty, tx)
    assert m.any() and not m.all()
    return m


def state(r):
    out = (r.image(), r.moments(), r.sample_counts(), r.segments(), r.segments_per_bounce(10))
    assert r.trace_faults() == 0
    return out


STATE = ("image", "moments", "counts", "segments", "segments per bounce")


def assert_same_state(got, want, what):
    for g, w, name in zip(got, want, STATE):
        if isinstance(w, np.ndarray):
            assert_bitexact(g, w, f"{what}: {name}")
        else:
            assert g == w, (what, name, g, w)


def check_state(r, ref, what):
    assert_bitexact(r.image(), ref.S, f"{what}: image")
    assert_bitexact(r.moments(), ref.Q, f"{what}: moments")
    assert_bitexact(r.sample_counts(), ref.counts, f"{what}: counts")
    assert r.segments() == ref.segments, (what, r.segments(), ref.segments)
    assert r.segments_per_bounce(10) == ref.per_bounce[:10].tolist(), what
    assert r.trace_faults() == 0, what


# ---- 1. the lookup ------------------------------------------------------------------------------

def lookup_directions():
    rs = np.random.RandomState(41)
    d = [rs.normal(size=(3000, 3)) * 10.0 ** rs.uniform(-3, 3, (3000, 1))]
    d.append([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0]])
    z = rs.normal(size=(300, 3))                          # zero and -0.0 components
    z[np.arange(300), rs.randint(0, 3, 300)] = np.where(rs.rand(300) < 0.5, 0.0, -0.0)
    z[:60, 0] = np.where(rs.rand(60) < 0.5, 0.0, -0.0)
    d.append(z)
    for k in (1, 2):                                      # e.z == 0 under the test rotation (k = 1) and the identity
        h = rs.normal(size=(150, 3))
        h[:, k] = 0.0
        d.append(h)
    for a, b in ((0, 1), (2, 0)):                         # |e.x| = |e.y|: identity (x, y), test rotation (z, x)
        g = rs.normal(size=(200, 3))
        g[:, b] = g[:, a] * np.where(rs.rand(200) < 0.5, 1.0, -1.0)
        d.append(g)
    p = (np.arange(8) + 0.5) / 8 * 2 - 1                  # an 8 x 8 map's texel centres and texel corners
    for q in (p, np.linspace(-1, 1, 9)):
        px, py = (v.reshape(-1) for v in np.meshgrid(q, q))
        ez = 1 - np.abs(px) - np.abs(py)
        low = ez < 0
        d.append(np.stack([np.where(low, (1 - np.abs(py)) * np.where(px >= 0, 1, -1), px),
                           np.where(low, (1 - np.abs(px)) * np.where(py >= 0, 1, -1), py), ez], axis=1))
    return np.ascontiguousarray(np.concatenate([np.asarray(v, np.float64) for v in d]), F)


@pytest.fixture(scope="module")
def small_renderer(pt_mod, scene):
    r = pt_mod.Renderer(make_cfg(pt_mod, width=16, height=16, pipelines=1))
    r.allocateOnGPU(scene)
    yield r
    r.free()


@pytest.mark.parametrize("n", [1, 2, 5, 8, 64])
def test_lookup_equals_the_restatement(gpu, pt_mod, small_renderer, n):
    P = pt_mod
    d = lookup_directions()
    assert 4000 <= len(d) <= 4500
    for rot, name in ((np.eye(3, dtype=F), "identity"), (UP_Y, "+z -> +y")):
        env = random_env(P, n, seed=100 + n, rot=rot)
        small_renderer.set_environment(env)
        got = small_renderer.environment_lookup(d)
        want = ER.lookup(env.texels, env.rotation, env.scale, d)
        assert np.isfinite(got).all()
        assert_bitexact(got, want, f"n {n} rotation {name}")
        if n > 1:
            assert len(np.unique(got[:, 0])) > 1000
    small_renderer.set_environment(None)
    with pytest.raises(P.PathTracerError, match="env_lookup: no environment is set"):
        small_renderer.environment_lookup(d[:4])


# ---- 2. the constant 0.01 is the legacy image ------------------------------------------------------

def sequence(P, scene, cfg, env, env_after=False):
    """Plain, a random half of the tiles, jitter 1.0 and view A through a lens: four renders."""
    r = renderer(P, scene, cfg, env, env_after=env_after)
    out = []
    for what in ("plain", "half mask", "jitter 1", "lens"):
        r.clearImage()
        if what == "jitter 1":
            r.set_pixel_jitter(1.0)
        if what == "lens":
            r.set_pixel_jitter(1.0, on=False)
            r.set_camera(view(P, "A", cfg, LENS))
        if what == "half mask":
            r.render_masked(half_mask(W, H), 0, ITERS)
        else:
            r.renderLoop(0, ITERS)
        out.append(state(r))
    assert (r.environment() is None) == (env is None)
    r.free()
    return out


LEGACY_CASES = [("grid", 3, {}), ("grid_fast", 1, {}), ("grid_fast", 3, {}), ("grid_fast", 16, {}), ("bvh", 1, {}),
                ("bvh", 3, {}), ("bvh", 16, {}),
                ("grid_fast", 3, {"PT_GF_SPLIT": "0"}), ("bvh", 3, {"PT_TRACE_SPLIT": "0"}),
                ("grid_fast", 16, {"PT_GRAPH": "1"}), ("bvh", 16, {"PT_GRAPH": "1"}),
                ("grid_fast", 3, {"PT_SLOT_MAP": "0"})]


@pytest.mark.parametrize("accel,pipes,envvars", LEGACY_CASES)
def test_constant_one_percent_is_the_legacy_image(gpu, pt_mod, scene, monkeypatch, accel, pipes, envvars):
    P = pt_mod
    for k, v in envvars.items():
        monkeypatch.setenv(k, v)                         # read by allocateOnGPU
    cfg = make_cfg(P, accel, pipelines=pipes)
    want = sequence(P, scene, cfg, None)
    assert want[0][0].any() and not np.array_equal(want[0][0], want[2][0]) and not np.array_equal(want[0][0], want[3][0])
    for after in (False, True):
        got = sequence(P, scene, cfg, P.Environment.constant(0.01), env_after=after)
        for k, label in enumerate(("plain", "half mask", "jitter 1", "lens")):
            assert_same_state(got[k], want[k], f"{accel} p{pipes} {envvars} set {'after' if after else 'before'}: {label}")


# ---- 3. a random map is the restatement -------------------------------------------------------------

_REFS = {}


def restated(P, flat, cfg, name, lens, jitter, tile, which="ref"):
    """The restated render of iterations [0, 3) under the random map (shared; never modified)."""
    o = oracle_cfg(cfg, threads=4)
    key = (which, o.width, o.height, o.accel, o.tail_drop, name, lens, jitter, tile)
    if key not in _REFS:
        e = random_env(P)
        cam = view(P, name, cfg, lens)
        ref = ER.Restatement(flat, o, width=jitter, camera=None if cam is None else CR.Cam.of(cam), env=ER.Env.of(e))
        ref.render(0, ITERS, None if tile is None else one_tile(o.width, o.height, tile))
        _REFS[key] = ref
    return _REFS[key]


FULL = (W, H, 0)
# view, lens, jitter, accel, (width, height, tail_drop), masked tile, pipelines
CASES = [(None, 0.0, None, "grid_fast", FULL, None, 1),
         (None, 0.0, None, "grid_fast", FULL, None, 16),
         (None, 0.0, None, "bvh", FULL, None, 16),
         ("A", 0.0, None, "grid_fast", FULL, None, 16),
         ("A", 0.0, None, "bvh", FULL, None, 1),
         ("B", 0.0, None, "grid_fast", FULL, None, 1),
         ("B", 0.0, None, "bvh", FULL, None, 16),
         (None, 0.0, 1.0, "grid_fast", FULL, None, 16),
         ("B", 0.0, 1.0, "bvh", FULL, None, 1),
         ("A", LENS, None, "grid_fast", FULL, None, 16),
         ("A", LENS, None, "bvh", FULL, None, 1),
         ("A", 0.0, None, "grid_fast", FULL, 5, 1),
         ("B", 0.0, None, "bvh", FULL, 3, 16),
         (None, 0.0, None, "grid_fast", (37, 23, 1), None, 16),
         ("B", 0.0, None, "bvh", (37, 23, 1), None, 1)]


def run_case(P, scene, cfg, env, name, lens, jitter, tile):
    r = renderer(P, scene, cfg, env, view(P, name, cfg, lens), jitter)
    if tile is None:
        r.renderLoop(0, ITERS)
    else:
        r.render_masked(one_tile(cfg.width, cfg.height, tile), 0, ITERS)
    return r


def differing_pixels(a, b):
    return (np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(axis=1)


@pytest.mark.parametrize("name,lens,jitter,accel,size,tile,pipes", CASES)
def test_random_map_equals_the_restatement(gpu, pt_mod, scene, flat, name, lens, jitter, accel, size, tile, pipes):
    P = pt_mod
    cfg = make_cfg(P, accel, width=size[0], height=size[1], tail_drop=size[2], pipelines=pipes)
    ref = restated(P, flat, cfg, name, lens, jitter, tile)
    r = run_case(P, scene, cfg, random_env(P), name, lens, jitter, tile)
    what = f"view {name} lens {lens} jitter {jitter} {accel} {size} tile {tile} p{pipes}"
    check_state(r, ref, what)
    r.free()
    # the comparison is about rays that missed: the restatement says they occurred
    if tile is None:
        sampled = np.zeros(cfg.width * cfg.height, bool)
        sampled[:ref.n_launch] = True
    else:
        sampled = one_tile(cfg.width, cfg.height, tile).reshape(-1)[ref.tile_of]
    share = sampled.sum() / (W * H)                      # of the 64 x 48 frame the counts below were measured on
    print(f"{what}: misses by depth {ref.misses[:BOUNCES].tolist()}")
    assert np.isfinite(ref.S).all()
    assert ref.misses[1:].sum() >= 100 * share           # secondary misses (3255 .. 6375 on the full frame)
    if name == "B" and tile is None:
        assert ref.misses[0] >= 1                        # view B looks past the room's edge
    if size[2]:
        assert ref.n_launch == 832 and not ref.S[832:].any()
    # ... and they colour most pixels: against the same render without an environment
    plain = run_case(P, scene, cfg, None, name, lens, jitter, tile)
    differ = differing_pixels(plain.image(), ref.S)
    assert plain.segments() == ref.segments
    plain.free()
    print(f"{what}: {differ.sum()} of {sampled.sum()} sampled pixels differ from the render without an environment")
    assert not differ[~sampled].any() and differ.sum() > sampled.sum() / 2


@pytest.mark.parametrize("accel,pipes,envvars", [("grid", 3, {}), ("grid_fast", 3, {"PT_GF_SPLIT": "0"}),
                                                 ("bvh", 3, {"PT_TRACE_SPLIT": "0"}), ("grid_fast", 3, {"PT_SLOT_MAP": "0"}),
                                                 ("grid_fast", 16, {"PT_GRAPH": "1"}), ("bvh", 16, {"PT_GRAPH": "1"})])
def test_random_map_on_the_other_shading_paths(gpu, pt_mod, scene, flat, monkeypatch, accel, pipes, envvars):
    """The list-walking grid, the fused bounce kernels, the blk_off search and graph replay
    colour a miss through the same shade_mat: the legacy view's restated render again."""
    P = pt_mod
    for k, v in envvars.items():
        monkeypatch.setenv(k, v)                         # read by allocateOnGPU
    cfg = make_cfg(P, accel, pipelines=pipes)
    r = run_case(P, scene, cfg, random_env(P), None, 0.0, None, None)
    check_state(r, restated(P, flat, cfg, None, 0.0, None, None), f"{accel} p{pipes} {envvars}")
    r.free()


@pytest.mark.parametrize("accel,pipes", [("grid_fast", 16), ("bvh", 1)])
def test_mostly_missing_scene_equals_the_restatement(gpu, pt_mod, miss_scene, miss_flat, accel, pipes):
    P = pt_mod
    cfg = make_cfg(P, accel, pipelines=pipes)
    ref = restated(P, miss_flat, cfg, None, 0.0, None, None, which="miss scene")
    r = run_case(P, miss_scene, cfg, random_env(P), None, 0.0, None, None)
    check_state(r, ref, f"miss scene {accel} p{pipes}")
    k = r.primary_hits()[2]
    r.free()
    assert (k < 0).mean() > 0.5 and ref.misses[0] == ITERS * (k < 0).sum()     # more than half the primary rays miss
    plain = run_case(P, miss_scene, cfg, None, None, 0.0, None, None)
    differ = differing_pixels(plain.image(), ref.S)
    plain.free()
    assert differ.sum() > W * H / 2


# ---- 4. switching -----------------------------------------------------------------------------------

@pytest.mark.parametrize("graph", [False, True], ids=["direct", "PT_GRAPH=1"])
def test_switching(gpu, pt_mod, scene, flat, monkeypatch, graph):
    """Captured launches hold the environment pointer by value: a switch between none and set
    must drop the graphs."""
    P = pt_mod
    if graph:
        monkeypatch.setenv("PT_GRAPH", "1")              # read by allocateOnGPU
    cfg = make_cfg(P, pipelines=16)
    env_a, env_b = random_env(P), random_env(P, 5, seed=78, rot=np.eye(3, dtype=F))
    ref_a = restated(P, flat, cfg, None, 0.0, None, None)
    fresh = {}
    for key, env in (("legacy", None), ("a", env_a), ("b", env_b)):
        q = renderer(P, scene, cfg, env)
        q.renderLoop(0, ITERS)
        fresh[key] = state(q)
        q.free()
    assert_bitexact(fresh["a"][0], ref_a.S, "set before allocation: image")
    assert not np.array_equal(fresh["a"][0], fresh["b"][0]) and not np.array_equal(fresh["a"][0], fresh["legacy"][0])
    r = renderer(P, scene, cfg)
    r.renderLoop(0, ITERS, sync=False)                   # the legacy render (and its graphs)
    hits = r.primary_hits()
    r.set_environment(env_a)                             # after allocateOnGPU
    for got, name in zip((r.image(), r.moments(), r.sample_counts()), STATE):
        assert not got.any(), f"after set_environment the {name} must read zero"
    r.renderLoop(0, ITERS, sync=False)
    for g, w, name in zip(state(r)[:3], fresh["a"][:3], STATE):
        assert_bitexact(g, w, f"set after allocation = set before: {name}")
    assert r.segments() == 2 * fresh["a"][3]             # the segment counters run on
    for g, w in zip(r.primary_hits(), hits):
        assert_bitexact(g, w, "the primary-hit cache stays")
    r.renderLoop(ITERS, 2, sync=False)
    r.set_environment(env_b)                             # between two renderLoop calls: only the second render stays
    r.renderLoop(0, ITERS, sync=False)
    for g, w, name in zip(state(r)[:3], fresh["b"][:3], STATE):
        assert_bitexact(g, w, f"a -> b: {name}")
    got = r.environment()
    assert_bitexact(got.texels, env_b.texels, "the getter after allocation")
    r.set_environment(None)
    assert r.environment() is None
    r.renderLoop(0, ITERS, sync=False)
    for g, w, name in zip(state(r)[:3], fresh["legacy"][:3], STATE):
        assert_bitexact(g, w, f"b -> none: {name}")
    r.set_environment(env_a)
    r.renderLoop(0, ITERS, sync=False)
    for g, w, name in zip(state(r)[:3], fresh["a"][:3], STATE):
        assert_bitexact(g, w, f"none -> a: {name}")
    r.free()


# ---- 5. the denoiser, 6. sharding, 7. the command line -------------------------------------------

def test_denoise_with_an_environment(gpu, pt_mod, miss_scene):
    P = pt_mod
    cfg = make_cfg(P, pipelines=3, iterations=6)
    r = renderer(P, miss_scene, cfg, random_env(P))
    r.renderLoop(0, 6)
    S, Q = r.image(), r.moments()
    d, n, k = r.primary_hits()
    img, var = r.denoise(variance=True)
    assert r.trace_faults() == 0
    r.free()
    want_img, want_var = DR.denoise(S, Q, W, H, 6, d, n, k)
    assert_bitexact(img, want_img, "denoise: image")
    assert_bitexact(var, want_var, "denoise: variance")
    miss = k < 0
    assert miss.mean() > 0.5 and np.isfinite(img).all()
    assert_bitexact(img[miss], (S / F(6))[miss], "miss pixels pass through")
    assert len(np.unique(img[miss], axis=0)) > 100       # ... and they show the map, not one grey


def test_render_sharded_without_a_process_group(gpu, pt_mod, scene, flat):
    P = pt_mod
    from pathtracerap_amd.dist import render_sharded
    cfg = make_cfg(P)
    image = render_sharded(scene, cfg, ITERS, environment=random_env(P))
    assert image.is_cuda
    assert_bitexact(image.cpu().numpy().reshape(-1, 3), restated(P, flat, cfg, None, 0.0, None, None).S, "sharded image")


def test_cli_sky(gpu, pt_mod, scene, tmp_path):
    P = pt_mod
    cfg = make_cfg(P, pipelines=3, iterations=6)
    bmp, want = str(tmp_path / "cli.bmp"), str(tmp_path / "python.bmp")
    p = subprocess.run([os.path.join(ROOT, "pathtracerap_amd", "pathtracer_amd"), REF_SCENE, bmp, "--res", str(W), str(H),
                        "--bounces", str(BOUNCES), "--grid-fast", "--pipelines", "3", "--iter", "6",
                        "--look-from", "650", "200", "650", "--look-at", "0", "0", "0",
                        "--sky", "0.1", "0.3", "0.9", "0.8", "0.7", "0.6", "--ground", "0.2", "0.15", "0.1"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    sky = P.Environment.sky((0.1, 0.3, 0.9), (0.8, 0.7, 0.6), (0.2, 0.15, 0.1))
    r = renderer(P, scene, cfg, sky, view(P, "B", cfg))
    r.renderLoop(0, 6)
    r.renderImage(want, 6)
    legacy = renderer(P, scene, cfg, None, view(P, "B", cfg))
    legacy.renderLoop(0, 6)
    assert differing_pixels(legacy.image(), r.image()).sum() > W * H / 2
    legacy.free()
    r.free()
    with open(bmp, "rb") as f, open(want, "rb") as g:
        assert f.read() == g.read()
