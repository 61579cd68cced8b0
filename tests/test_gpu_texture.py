"""Albedo textures on the GPU (include/pathtracer_amd.h, pt_scene_set_model_texture), against the
restatement in texture_ref.py (which tests/test_texture_ref.py holds to smooth_ref's and through it
to the oracle).

S (image), Q (moments), the per-tile sample counts, the segment count and the per-bounce segment
counts are compared bit for bit, as are the primary-hit cache, primary_albedo and the hit_albedo
hook; every render must leave trace_faults() at 0.  The fixture (texture_scenes.fixture_spec): a
displaced torus instanced as DIFFUSE, METAL (smooth as well), COAT, REFLECTIVE, EMISSIVE and
DIFFUSE again, each with one of six textures (1x1, 1x5, 5x1, 2x2, 5x3, 64x64), per-vertex uvs from
[-2, 3], in the untextured flat room under an untextured lamp.  The orientation tests do not use
the restatement: they read a 2x2 texture's four texels off a BOX face and an OBJ quad."""
import copy

import numpy as np
import pytest

import adaptive_ref as AR
import camera_ref as CR
import denoise_ref as DR
import env_ref as ER
import smooth_scenes as SS
import texture_ref as TR
import texture_scenes as TS
from helpers import assert_bitexact, flat_from_export, oracle_accel, oracle_cfg

pytestmark = pytest.mark.gpu

F = np.float32
W, H, BOUNCES, ITERS, LENS = 64, 48, 4, 3, 25.0
VIEW_A = dict(eye=(0, 800, 500), target=(0, 0, 0), vfov_deg=45, focus_dist=900)
UP_Y = np.float32([[0, 0, 1], [1, 0, 0], [0, 1, 0]])


def accel_of(P, name):
    return {"grid_fast": P.ACCEL_GRID_FAST, "grid": P.ACCEL_GRID, "bvh": P.ACCEL_BVH}[name]


def make_cfg(P, accel="grid_fast", **kw):
    base = dict(width=W, height=H, max_bounces=BOUNCES, iterations=ITERS, accel=accel_of(P, accel))
    base.update(kw)
    return P.RenderConfig(**base)


def white_spec(spec):
    """The spec with every textured model white and a uniform texture of its former colour."""
    out = copy.deepcopy(spec)
    textured = np.nonzero(spec["binding"] >= 0)[0]
    out["textures"] = [np.broadcast_to(F(spec["models"][i]["color"]), (2, 3, 3)).astype(F) for i in textured]
    for k, i in enumerate(textured):
        out["models"][i]["color"] = (1.0, 1.0, 1.0)
        out["binding"][i] = k
    return out


_SCENES = {}


def fixture(P, name="torus"):
    """(scene, FlatScene, spec) of a named fixture, built once."""
    if name not in _SCENES:
        spec = TS.fixture_spec(extra=TS.zero_area_extra() if name == "zero-area" else None)
        s = TS.gpu_scene(P, spec)
        assert s.model_textures().tolist() == spec["binding"].tolist() and s.smooth().tolist() == spec["smooth"].tolist()
        a = s.export()
        assert np.array_equal(a["uv"], TS.vertex_uv(spec))
        _SCENES[name] = (s, flat_from_export(a), spec)
    return _SCENES[name]


def random_env(P):
    return P.Environment(np.random.RandomState(77).uniform(0, 2, (8, 8, 3)), (1.5, 1.0, 0.5), UP_Y)


def half_mask(w, h, seed=20):
    ty, tx = AR.tiles_shape(w, h)
    m = (np.random.RandomState(seed).permutation(ty * tx) < (ty * tx) // 2).reshape(ty, tx)
    assert m.any() and not m.all()
    return m


def options(P, cfg, opt):
    cam = P.look_at(lens_radius=opt.get("lens", 0.0), width=cfg.width, height=cfg.height, **VIEW_A) if opt.get("view") else None
    mask = half_mask(cfg.width, cfg.height) if opt.get("mask") else None
    env = random_env(P) if opt.get("env") else None
    return cam, opt.get("jitter"), mask, env


def restatement(P, flat, spec, cfg, opt=None, textured=True):
    cam, jitter, _, env = options(P, cfg, opt or {})
    return TR.Restatement(flat, oracle_cfg(cfg, threads=4), width=jitter, camera=None if cam is None else CR.Cam.of(cam),
                          env=None if env is None else ER.Env.of(env), smooth=spec["smooth"], uv=TS.vertex_uv(spec),
                          textures=spec["textures"], binding=spec["binding"] if textured else None)


_REFS = {}


def restated(P, name, cfg, opt=None, textured=True):
    """The restated render of iterations [0, ITERS) (shared; never modified)."""
    opt = opt or {}
    _, flat, spec = fixture(P, name)
    o = oracle_cfg(cfg, threads=4)
    key = (name, textured, o.width, o.height, o.accel, o.tail_drop, tuple(sorted(opt.items())))
    if key not in _REFS:
        ref = restatement(P, flat, spec, cfg, opt, textured)
        ref.render(0, ITERS, options(P, cfg, opt)[2])
        assert ref.tex_ident.holds() and ref.ident.holds() and (ref.tex_hits > 100 or not textured)
        _REFS[key] = ref
    return _REFS[key]


def rendered(P, scene, cfg, opt=None):
    cam, jitter, mask, env = options(P, cfg, opt or {})
    r = P.Renderer(cfg)
    r.enable_moments()
    if cam is not None:
        r.set_camera(cam)
    if jitter is not None:
        r.set_pixel_jitter(jitter)
    if env is not None:
        r.set_environment(env)
    r.allocateOnGPU(scene)
    if mask is None:
        r.renderLoop(0, ITERS)
    else:
        r.render_masked(mask, 0, ITERS)
    return r


def check_state(r, ref, what):
    assert_bitexact(r.image(), ref.S, f"{what}: image")
    assert_bitexact(r.moments(), ref.Q, f"{what}: moments")
    assert_bitexact(r.sample_counts(), ref.counts, f"{what}: counts")
    assert r.segments() == ref.segments, (what, r.segments(), ref.segments)
    assert r.segments_per_bounce(10) == ref.per_bounce[:10].tolist(), what
    assert r.trace_faults() == 0, what


def differing_pixels(a, b):
    return (np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(axis=1)


def state(r):
    out = (r.image(), r.moments(), r.sample_counts(), r.segments(), r.segments_per_bounce(10))
    assert r.trace_faults() == 0
    return out


def assert_same_state(got, want, what):
    for g, w, name in zip(got, want, ("image", "moments", "counts", "segments", "segments per bounce")):
        if isinstance(w, np.ndarray):
            assert_bitexact(g, w, f"{what}: {name}")
        else:
            assert g == w, (what, name, g, w)


# ---- 1. the primary-hit cache and primary_albedo ------------------------------------------------

@pytest.mark.parametrize("accel", ["grid", "grid_fast", "bvh"])
@pytest.mark.parametrize("size", [(64, 48, 0), (37, 23, 1)])
@pytest.mark.parametrize("view", [False, True])
def test_primary_cache_and_albedo_equal_the_restatement(gpu, pt_mod, accel, size, view):
    P = pt_mod
    scene, flat, spec = fixture(P)
    cfg = make_cfg(P, accel, width=size[0], height=size[1], tail_drop=size[2], pipelines=1)
    opt = {"view": True} if view else {}
    ref = restatement(P, flat, spec, cfg, opt)
    want, want_albedo = ref.primary_hits(), ref.primary_albedo()
    assert ref.tex_ident.holds() and ref.tex_ident.hits > 50
    r = P.Renderer(cfg)
    if view:
        r.set_camera(options(P, cfg, opt)[0])
    r.allocateOnGPU(scene)
    got_albedo = r.primary_albedo()                      # builds the cache
    got = r.primary_hits()
    assert r.trace_faults() == 0
    n = len(got[0])
    for g, w, name in zip(got, want, ("distance", "normal", "model")):
        assert_bitexact(g, w[:n], f"{accel} {size}: primary {name}")
    assert_bitexact(got_albedo, want_albedo, f"{accel} {size} view {view}: primary albedo")
    assert got_albedo.shape == (size[0] * size[1], 3) and not got_albedo[n:].any()
    plain = np.where((want[2] >= 0)[:, None], flat.model_color[np.maximum(want[2], 0)], F(0)).astype(F)
    on_textured = (spec["binding"][np.maximum(want[2], 0)] >= 0) & (want[2] >= 0)
    on_textured[n:] = False
    plain[n:] = 0                                        # tail_drop: the pixels left out read zero
    moved = differing_pixels(want_albedo, plain)
    print(f"{accel} {size} view {view}: {on_textured.sum()} primary hits on textured models, {moved.sum()} albedos differ "
          f"from the model colour")
    assert not moved[~on_textured].any() and moved[on_textured].mean() > 0.9
    if view:                                             # set_camera rebuilds the albedo plane with the cache
        r.set_camera(None)
        back = restatement(P, flat, spec, cfg)
        assert_bitexact(r.primary_albedo(), back.primary_albedo(), "primary albedo after the camera is cleared")
    r.free()


def test_primary_albedo_without_textures_is_the_model_colour(gpu, pt_mod):
    P = pt_mod
    _, flat, spec = fixture(P)
    scene = TS.gpu_scene(P, spec, textured=False)
    cfg = make_cfg(P, "grid_fast", pipelines=1)
    r = P.Renderer(cfg)
    r.allocateOnGPU(scene)
    got = r.primary_albedo()
    model = r.primary_hits()[2]
    r.free()
    want = np.where((model >= 0)[:, None], flat.model_color[np.maximum(model, 0)], F(0)).astype(F)
    assert_bitexact(got, want, "untextured primary albedo")
    assert (model >= 0).sum() > 1000


# ---- 2. renders -----------------------------------------------------------------------------------

FULL = (W, H, 0)
# accel, (width, height, tail_drop), pipelines, environment variables, config fields, options
RENDER_CASES = [
    ("grid", FULL, 3, {}, {}, {}),
    ("grid_fast", FULL, 1, {}, {}, {}),
    ("grid_fast", FULL, 16, {}, {}, {}),
    ("bvh", FULL, 1, {}, {}, {}),
    ("bvh", FULL, 16, {}, {}, {}),
    ("grid_fast", FULL, 3, {"PT_GF_SPLIT": "0"}, {}, {}),          # the fused k_bounce
    ("bvh", FULL, 3, {"PT_TRACE_SPLIT": "0"}, {}, {}),
    ("grid_fast", FULL, 3, {}, {"ray_sort": 0}, {}),               # get_hit, no slot_src
    ("bvh", FULL, 3, {}, {"ray_sort": 0}, {}),
    ("grid_fast", FULL, 3, {"PT_SLOT_MAP": "0"}, {}, {}),          # sorted, get_hit
    ("bvh", FULL, 3, {"PT_SLOT_MAP": "0"}, {}, {}),
    ("grid_fast", FULL, 16, {"PT_GRAPH": "1"}, {}, {}),
    ("bvh", FULL, 16, {"PT_GRAPH": "1"}, {}, {}),
    ("grid_fast", FULL, 3, {}, {"block": 128}, {}),
    ("bvh", FULL, 3, {}, {"block": 128}, {}),
    ("grid_fast", FULL, 3, {}, {"block": 256}, {}),             # 64 is the default: every other case runs it
    ("bvh", FULL, 3, {}, {"block": 256}, {}),
    ("grid_fast", FULL, 3, {}, {"block": 256}, {"mask": True}),    # k_bounce_masked<256> through the albedo plane
    ("grid_fast", FULL, 3, {"PT_GF_SPLIT": "0"}, {"block": 256}, {}),      # the fused k_bounce at 256
    ("bvh", FULL, 3, {"PT_TRACE_SPLIT": "0"}, {"block": 256}, {}),
    ("grid", FULL, 3, {}, {"block": 256}, {}),
    ("grid_fast", FULL, 3, {"PT_GF_SPLIT": "0"}, {"block": 128}, {"mask": True}),
    ("grid_fast", FULL, 16, {}, {}, {"jitter": 1.0}),              # camera-ray hits through the hit buffer
    ("bvh", FULL, 1, {}, {}, {"view": True, "lens": LENS}),
    ("grid_fast", FULL, 3, {}, {}, {"view": True, "lens": LENS, "jitter": 1.0}),
    ("grid", FULL, 3, {}, {}, {"jitter": 1.0}),
    ("grid_fast", FULL, 3, {}, {}, {"view": True}),                # a pinhole: the albedo plane under a camera
    ("grid_fast", FULL, 3, {}, {}, {"mask": True}),                # k_bounce_masked through the albedo plane
    ("bvh", FULL, 16, {}, {}, {"mask": True}),
    ("grid_fast", (37, 23, 1), 16, {}, {}, {}),
    ("bvh", (37, 23, 0), 1, {}, {}, {}),
    ("grid", (37, 23, 1), 3, {}, {}, {}),
    ("grid_fast", (37, 23, 1), 3, {}, {}, {"jitter": 1.0, "mask": True}),
    ("grid_fast", FULL, 16, {}, {}, {"env": True}),
    ("bvh", FULL, 3, {}, {}, {"env": True}),
]


@pytest.mark.parametrize("accel,size,pipes,envvars,cfgkw,opt", RENDER_CASES)
def test_render_equals_the_restatement(gpu, pt_mod, monkeypatch, accel, size, pipes, envvars, cfgkw, opt):
    P = pt_mod
    for k, v in envvars.items():
        monkeypatch.setenv(k, v)                         # read by allocateOnGPU
    scene = fixture(P)[0]
    cfg = make_cfg(P, accel, width=size[0], height=size[1], tail_drop=size[2], pipelines=pipes, **cfgkw)
    ref = restated(P, "torus", cfg, opt)
    r = rendered(P, scene, cfg, opt)
    what = f"{accel} {size} p{pipes} {envvars} {cfgkw} {opt}"
    check_state(r, ref, what)
    # the frame-level records of this very renderer: the primary-hit cache and the albedo plane
    n = r.primary_hits()[0].shape[0]
    for g, w, name in zip(r.primary_hits(), ref.primary_hits(), ("distance", "normal", "model")):
        assert_bitexact(g, w[:n], f"{what}: primary {name}")
    assert_bitexact(r.primary_albedo(), ref.primary_albedo(), f"{what}: primary albedo")
    assert r.trace_faults() == 0
    r.free()
    assert np.isfinite(ref.S).all() and ref.S.any()
    plain = restated(P, "torus", cfg, opt, textured=False)
    differ = int(differing_pixels(ref.S, plain.S).sum())
    sampled = int((ref.S != 0).any(axis=1).sum())
    print(f"{what}: {ref.tex_hits} colours decided by a texture, {differ} of {size[0] * size[1]} pixels ({sampled} sampled) "
          f"differ from the untextured render")
    assert differ > size[0] * size[1] // 4               # a quarter of the frame, masked cases too


@pytest.mark.parametrize("accel,pipes", [("grid_fast", 16), ("bvh", 3), ("grid", 1)])
def test_white_and_uniform_textures_are_the_untextured_render(gpu, pt_mod, accel, pipes):
    """c * 1.0f is c: a 1x1 white texture on every model (the room and the lamp get uvs for it, so
    their hits, most of all hits, go through the textured pass too) changes no bit; and white tori
    with uniform textures of the fixture's colours are the fixture untextured."""
    P = pt_mod
    spec = fixture(P)[2]
    cfg = make_cfg(P, accel, pipelines=pipes)
    r = rendered(P, TS.gpu_scene(P, spec, textured=False), cfg)
    want, want_albedo = state(r), r.primary_albedo()
    r.free()
    assert_bitexact(want[0], restated(P, "torus", cfg, textured=False).S, "untextured: the restatement")
    white = TS.gpu_scene(P, spec, textured=False)
    one = white.add_texture(np.ones((1, 1, 3), F))
    ranges = white.export()["mesh_ranges"]
    for mesh in (0, 1):                                  # the room and the lamp: seeded uvs, like the torus
        nv = int(ranges[mesh, 1] - ranges[mesh, 0])
        white.set_mesh_uv(mesh, np.random.RandomState(60 + mesh).uniform(-2, 3, (nv, 2)))
    white.set_texture(None, one)
    assert (white.model_textures() == one).all()
    r = rendered(P, white, cfg)
    assert_same_state(state(r), want, f"{accel} p{pipes}: 1x1 white")
    assert_bitexact(r.primary_albedo(), want_albedo, "1x1 white: primary albedo")
    r.free()
    r = rendered(P, TS.gpu_scene(P, white_spec(spec)), cfg)
    assert_same_state(state(r), want, f"{accel} p{pipes}: uniform textures on white models")
    assert_bitexact(r.primary_albedo(), want_albedo, "uniform: primary albedo")
    r.free()


# ---- 3. the hit_albedo hook -----------------------------------------------------------------------

@pytest.mark.parametrize("accel", ["grid_fast", "bvh"])
def test_hit_albedo_over_traced_hits_equals_the_restatement(gpu, pt_mod, oracle_mod, accel):
    """trace_rays' hits (rays through vertices, edge midpoints, interior points and at grazing angles;
    dense and sparse survivor layouts) into hit_albedo, against the restatement over the oracle's
    hits of the same rays, which finds the triangles on its own."""
    P, O = pt_mod, oracle_mod
    scene, flat, spec = fixture(P, "zero-area")
    a = scene.export()
    o, d = zip(*(SS.torus_rays(a, m, seed=50 + m) for m in range(2, 8)))
    o, d = np.concatenate(o), np.concatenate(d)
    keep = np.random.RandomState(5).permutation(len(o))[:W * H]
    o, d = np.ascontiguousarray(o[keep]), np.ascontiguousarray(d[keep])
    cfg = make_cfg(P, accel, pipelines=1)
    ref = restatement(P, flat, spec, cfg)
    dist, nrm, model = O.intersect_rays(flat, o, d, accel=oracle_accel(cfg.accel), threads=4)
    want = ref.albedo(o, d, dist, nrm, model)
    assert ref.tex_ident.holds()
    textured = (model >= 2) & (model <= 7)
    plain = np.where((model >= 0)[:, None], flat.model_color[np.maximum(model, 0)], F(0)).astype(F)
    print(f"{accel}: {len(o)} rays, {textured.sum()} hit a textured torus, {(model == 0).sum()} the room, {(model < 0).sum()} "
          f"nothing; {differing_pixels(want, plain).sum()} albedos differ from the model colour")
    assert textured.sum() > len(o) // 2 and (model == 0).sum() > 20
    assert differing_pixels(want[textured], plain[textured]).mean() > 0.9
    assert_bitexact(want[~textured], plain[~textured], "an untextured model gives its colour, a miss zero")
    r = P.Renderer(cfg)
    r.allocateOnGPU(scene)
    td, _, tm, tt = r.trace_rays(o, d)
    assert_bitexact(td, dist, "trace_rays: distance")
    assert_bitexact(tm, model, "trace_rays: model")
    assert_bitexact(r.hit_albedo(o, d, td, tm, tt), want, f"{accel}: hit_albedo, dense layout")
    counts = np.random.RandomState(9).randint(0, cfg.block + 1, (W * H + cfg.block - 1) // cfg.block)
    m = min(int(counts.sum()), len(o))
    counts = np.minimum(counts, np.maximum(m - np.concatenate([[0], np.cumsum(counts)[:-1]]), 0))
    td, _, tm, tt = r.trace_rays(o[:m], d[:m], counts)
    assert_bitexact(r.hit_albedo(o[:m], d[:m], td, tm, tt), want[:m], f"{accel}: hit_albedo, sparse layout")
    # the zero-area triangle (two equal corners; no ray hits it: the hook takes it as given): den = 0,
    # both barycentrics clamp from NaN to 0 and the uv is the first corner's
    zmodel, ztri = len(spec["models"]) - 1, len(a["tris"]) - 1
    assert a["tris"][ztri, 0] == a["tris"][ztri, 1]
    k = 64
    zm, zt = np.full(k, zmodel, np.int32), np.full(k, ztri, np.int32)
    got = r.hit_albedo(o[:k], d[:k], np.abs(td[:k]) % F(1000), zm, zt)
    corner = a["uv"][a["tris"][ztri, 0]][None, :]
    want_z = (F(spec["models"][zmodel]["color"]) * TR.lookup(spec["textures"][spec["binding"][zmodel]], corner)).astype(F)
    assert_bitexact(got, np.repeat(want_z, k, axis=0), "zero-area triangle: the first corner's texel")
    assert_bitexact(got, TR.albedo_of_triangles(flat, ref.tables, ref.uvt, ref.textures, ref.binding, o[:k], d[:k],
                                                np.abs(td[:k]) % F(1000), zm, zt), "zero-area triangle: the restatement")
    # model < 0 gives zero whatever the rest says; indices out of range are refused before any launch
    assert not r.hit_albedo(o[:4], d[:4], td[:4], np.full(4, -1, np.int32), np.full(4, 10 ** 9, np.int32)).any()
    for bad_model, bad_tri, message in ((len(spec["models"]), 0, "model index out of range"),
                                        (2, len(a["tris"]), "triangle index out of range"), (2, -1, "triangle index out of range")):
        with pytest.raises(P.PathTracerError, match=message):
            r.hit_albedo(o[:1], d[:1], td[:1], [bad_model], [bad_tri])
    assert r.trace_faults() == 0
    r.free()


# ---- 4. orientation, without the restatement ------------------------------------------------------

QUADRANT_TEXELS = np.float32([[(0.9, 0.1, 0.1), (0.1, 0.9, 0.1)],          # row 0: columns 0, 1
                              [(0.1, 0.1, 0.9), (0.9, 0.9, 0.1)]])         # row 1
BOX_SCENE = """
DIFFUSE
white
[1, 1, 1]

TEXTURE
quadrants
PPM
q.ppm

BOX
slab
[0.2, 0.2, 0]
[-0.2, -0.2, -0.01]
material:white
texture:quadrants
"""
QUAD_SCENE = BOX_SCENE[:BOX_SCENE.index("BOX")] + "MESH\nquad\nquad.obj\nmaterial:white\ntexture:quadrants\n"
QUAD_OBJ = ("v -0.2 -0.2 0\nv 0.2 -0.2 0\nv 0.2 0.2 0\nv -0.2 0.2 0\nvn 0 0 1\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\n"
            "f 1/1/1 2/2/1 3/3/1 4/4/1\n")


def quadrant_albedo(P, tmp_path, text, accel):
    """primary_albedo of an 8x8 frame of the legacy camera at (0, 0, 1000) whose pixel (x, y) looks
    through (-50 + 100 x, -50 + 100 y, 500): pixels (0,0), (1,0), (0,1), (1,1) hit the plane z = 0 at
    (-100,-100), (100,-100), (-100,100), (100,100), the quadrant centres of a face spanning +-200."""
    bytes_ = np.round(QUADRANT_TEXELS * 10).astype(np.uint8)        # maxval 10: 0.9 -> 9
    (tmp_path / "q.ppm").write_bytes(b"P6\n2 2\n10\n" + bytes_.tobytes())
    (tmp_path / "quad.obj").write_text(QUAD_OBJ)
    (tmp_path / "scene.txt").write_text(text)
    s = P.Scene(str(tmp_path / "scene.txt"))
    s.build()
    cfg = P.RenderConfig(width=8, height=8, max_bounces=2, iterations=1, accel=accel_of(P, accel), pipelines=1,
                         cam=(0.0, 0.0, 1000.0), plane_z=500.0, plane_x0=-50.0, plane_y0=-50.0, plane_w=800.0, plane_h=800.0)
    r = P.Renderer(cfg)
    r.allocateOnGPU(s)
    albedo = r.primary_albedo().reshape(8, 8, 3)          # [y][x]
    model = r.primary_hits()[2].reshape(8, 8)
    assert r.trace_faults() == 0
    r.free()
    assert (model[:2, :2] == 0).all() and (model[2:, :] < 0).all() and (model[:, 2:] < 0).all()
    return albedo[:2, :2]


@pytest.mark.parametrize("accel", ["grid", "grid_fast", "bvh"])
def test_a_box_face_shows_the_texture_the_right_way_round(gpu, pt_mod, tmp_path, accel):
    """gen_box's +z face: its corners' uv[q] = (0,0), (1,0), (1,1), (0,1) sit at (lo,lo), (hi,lo), (hi,hi),
    (lo,hi) of (x, y), so u grows with x and v with y: world (-100,-100) is uv (0.25, 0.25), the
    centre of texel (row 0, column 0), where the bilinear weights are exactly 0.  The rounding of the
    uv (about 1e-6) times 2 texels times unit contrast is far below the 1e-3 bound; a swapped axis or
    a flip is wrong by order 1."""
    got = quadrant_albedo(pt_mod, tmp_path, BOX_SCENE, accel)
    want = np.round(QUADRANT_TEXELS * 10) / 10           # [row v][column u] = [y][x]
    print(f"{accel}: largest difference from the quadrants' texels {np.abs(got - want).max():.3g}")
    assert np.abs(got - want).max() <= 1e-3


def test_an_obj_quad_shows_the_texture_flipped_in_v(gpu, pt_mod, tmp_path):
    """The OBJ's vt (0,0) is at (-0.2,-0.2): stored as (u, 1 - v), so y = -100 reads row 1."""
    got = quadrant_albedo(pt_mod, tmp_path, QUAD_SCENE, "bvh")
    want = (np.round(QUADRANT_TEXELS * 10) / 10)[::-1]
    print(f"largest difference from the quadrants' texels {np.abs(got - want).max():.3g}")
    assert np.abs(got - want).max() <= 1e-3


# ---- 5. lifecycle -----------------------------------------------------------------------------------

@pytest.mark.parametrize("accel,pipes", [("grid_fast", 16), ("bvh", 3)])
def test_bindings_are_snapshot_at_allocation(gpu, pt_mod, accel, pipes):
    P = pt_mod
    spec = fixture(P)[2]
    cfg = make_cfg(P, accel, pipelines=pipes)
    r = rendered(P, TS.gpu_scene(P, spec, textured=False), cfg)
    want = state(r)
    r.free()
    cleared = TS.gpu_scene(P, spec)
    for i in np.nonzero(spec["binding"] >= 0)[0]:
        cleared.set_texture(int(i), None)                # bound, then cleared before allocation
    r = rendered(P, cleared, cfg)
    assert_same_state(state(r), want, f"{accel} p{pipes}: bound and cleared")
    for i, t in enumerate(spec["binding"]):              # a binding made after allocateOnGPU applies to the next allocation
        if t >= 0:
            cleared.set_texture(i, int(t))
    r.clearImage()
    r.renderLoop(0, ITERS)
    assert_same_state(state(r)[:3], want[:3], "bound after allocation: still the snapshot")
    r.allocateOnGPU(cleared)
    r.renderLoop(0, ITERS)
    assert_bitexact(r.image(), restated(P, "torus", cfg).S, "the next allocation: textured")
    assert r.trace_faults() == 0
    r.free()


# ---- 6. the denoiser --------------------------------------------------------------------------------

@pytest.mark.parametrize("accel,size", [("grid_fast", (64, 48)), ("bvh", (37, 23))])
def test_denoise_of_a_textured_render_equals_its_reference(gpu, pt_mod, accel, size):
    P = pt_mod
    scene, flat, spec = fixture(P)
    cfg = make_cfg(P, accel, width=size[0], height=size[1], pipelines=3, iterations=6)
    r = P.Renderer(cfg)
    r.enable_moments()
    r.allocateOnGPU(scene)
    r.renderLoop(0, 6)
    S, Q = r.image(), r.moments()
    d, n, k = r.primary_hits()
    img, var = r.denoise(variance=True)
    assert r.trace_faults() == 0
    r.free()
    ref = restatement(P, flat, spec, cfg)
    ref.render(0, 6)
    assert_bitexact(S, ref.S, "the textured render")
    want_img, want_var = DR.denoise(S, Q, size[0], size[1], 6, d, n, k)
    assert_bitexact(img, want_img, "denoise: image")
    assert_bitexact(var, want_var, "denoise: variance")
