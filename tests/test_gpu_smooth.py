"""Smooth shading on the GPU (include/pathtracer_amd.h, pt_scene_set_model_smooth), against the
restatement in smooth_ref.py (which tests/test_smooth_ref.py holds to env_ref's and through it to
the oracle).

S (image), Q (moments), the per-tile sample counts, the segment count and the per-bounce segment
counts are compared bit for bit, as are the primary-hit cache and the hooks' normals; every
render must leave trace_faults() at 0.  The fixture (smooth_scenes.fixture_spec): a displaced
torus instanced smooth as DIFFUSE, METAL, COAT and REFLECTIVE and once flat, in the flat room
under an emissive lamp.

Two of the fallback fixtures differ from a first reading of the feature's definition, which this
file follows to the letter.  The flat normal g is itself built from the vertex normals, so a mesh
with every vertex normal negated has g negated too and dot(s, g) > 0 still holds: smooth does not
fall back there, it equals the restatement.  And a mesh whose vertex normals are all zero has a NaN
flat normal, which sends non-finite rays into the traces, outside the renderer's contract.  The
"mixed" fixture reaches both branches with finite flat normals: next to a negated vertex normal
dot(s, g) <= 0, and a hit clamped onto a zeroed one interpolates to exactly zero."""
import numpy as np
import pytest

import adaptive_ref as AR
import camera_ref as CR
import denoise_ref as DR
import env_ref as ER
import smooth_ref as SR
import smooth_scenes as SS
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


_SCENES = {}


def fixture(P, name="torus-320"):
    """(scene, FlatScene, smooth flags) of a named fixture, built once."""
    if name not in _SCENES:
        kw = {"torus-320": dict(ntri=320), "torus-1000": dict(ntri=1000), "negated": dict(normals="negated"),
              "mixed": dict(normals="mixed"), "zero-area": dict(extra=SS.zero_area_extra())}[name]
        spec = SS.fixture_spec(**kw)
        s = SS.gpu_scene(P, spec)
        assert s.smooth().tolist() == spec[2].tolist()
        _SCENES[name] = (s, flat_from_export(s.export()), spec[2])
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


_REFS = {}


def restated(P, name, cfg, opt=None, smooth=True):
    """The restated render of iterations [0, ITERS) (shared; never modified)."""
    opt = opt or {}
    _, flat, flags = fixture(P, name)
    o = oracle_cfg(cfg, threads=4)
    key = (name, smooth, o.width, o.height, o.accel, o.tail_drop, tuple(sorted(opt.items())))
    if key not in _REFS:
        cam, jitter, mask, env = options(P, cfg, opt)
        ref = SR.Restatement(flat, o, width=jitter, camera=None if cam is None else CR.Cam.of(cam),
                             env=None if env is None else ER.Env.of(env), smooth=flags if smooth else None)
        ref.render(0, ITERS, mask)
        assert ref.ident.holds() and (ref.ident.hits > 100 or not smooth)
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


# ---- 1. the primary-hit cache -------------------------------------------------------------------

@pytest.mark.parametrize("accel", ["grid", "grid_fast", "bvh"])
@pytest.mark.parametrize("size", [(64, 48), (37, 23)])
def test_primary_cache_equals_the_restatement(gpu, pt_mod, accel, size):
    P = pt_mod
    scene, flat, flags = fixture(P)
    cfg = make_cfg(P, accel, width=size[0], height=size[1], pipelines=1)
    ref = SR.Restatement(flat, oracle_cfg(cfg, threads=4), smooth=flags)
    want = ref.primary_hits()
    assert ref.ident.holds() and ref.ident.hits > 100
    r = P.Renderer(cfg)
    r.allocateOnGPU(scene)
    r.renderLoop(0, 1)                                   # builds the cache
    got = r.primary_hits()
    assert r.trace_faults() == 0
    r.free()
    for g, w, name in zip(got, want, ("distance", "normal", "model")):
        assert_bitexact(g, w, f"{accel} {size}: primary {name}")
    on_smooth = flags[np.maximum(want[2], 0)] & (want[2] >= 0)
    moved = differing_pixels(want[1], ref.hit_nrm)
    print(f"{accel} {size}: {on_smooth.sum()} primary hits on smooth models, {moved.sum()} normals differ from flat")
    assert not moved[~on_smooth].any() and moved[on_smooth].mean() > 0.9
    hit6 = want[2] == 6                                  # the flat instance of the same mesh keeps its flat normals
    assert size != (64, 48) or hit6.sum() > 20


# ---- 2. renders -----------------------------------------------------------------------------------

FULL = (W, H, 0)
# fixture, accel, (width, height, tail_drop), pipelines, environment variables, config fields, options
RENDER_CASES = [
    ("torus-320", "grid", FULL, 3, {}, {}, {}),
    ("torus-320", "grid_fast", FULL, 1, {}, {}, {}),
    ("torus-320", "grid_fast", FULL, 16, {}, {}, {}),
    ("torus-320", "bvh", FULL, 1, {}, {}, {}),
    ("torus-320", "bvh", FULL, 16, {}, {}, {}),
    ("torus-1000", "grid_fast", FULL, 16, {}, {}, {}),
    ("torus-1000", "bvh", FULL, 3, {}, {}, {}),
    ("torus-320", "grid_fast", FULL, 3, {"PT_GF_SPLIT": "0"}, {}, {}),          # the fused k_bounce
    ("torus-320", "bvh", FULL, 3, {"PT_TRACE_SPLIT": "0"}, {}, {}),
    ("torus-320", "grid_fast", FULL, 3, {}, {"ray_sort": 0}, {}),               # get_hit, no slot_src
    ("torus-320", "bvh", FULL, 3, {}, {"ray_sort": 0}, {}),
    ("torus-320", "grid_fast", FULL, 3, {"PT_SLOT_MAP": "0"}, {}, {}),          # sorted, get_hit
    ("torus-320", "grid_fast", FULL, 16, {"PT_GRAPH": "1"}, {}, {}),
    ("torus-320", "bvh", FULL, 16, {"PT_GRAPH": "1"}, {}, {}),
    ("torus-320", "grid_fast", FULL, 16, {}, {}, {"jitter": 1.0}),              # camera-ray hits through the hit buffer
    ("torus-320", "bvh", FULL, 1, {}, {}, {"view": True, "lens": LENS}),
    ("torus-320", "grid_fast", FULL, 3, {}, {}, {"view": True, "lens": LENS, "jitter": 1.0}),
    ("torus-320", "grid", FULL, 3, {}, {}, {"jitter": 1.0}),
    ("torus-320", "grid_fast", FULL, 3, {}, {}, {"view": True}),                # a pinhole: the cache under a camera
    ("torus-320", "grid_fast", FULL, 3, {}, {}, {"mask": True}),                # k_bounce_masked through the cache
    ("torus-320", "bvh", FULL, 16, {}, {}, {"mask": True}),
    ("torus-320", "grid_fast", (37, 23, 1), 16, {}, {}, {}),
    ("torus-320", "bvh", (37, 23, 0), 1, {}, {}, {}),
    ("torus-320", "grid", (37, 23, 1), 3, {}, {}, {}),
    ("torus-320", "grid_fast", (37, 23, 1), 3, {}, {}, {"jitter": 1.0, "mask": True}),
    ("torus-320", "grid_fast", FULL, 16, {}, {}, {"env": True}),
    ("torus-320", "bvh", FULL, 3, {}, {}, {"env": True}),
    ("zero-area", "grid", FULL, 3, {}, {}, {}),
    ("zero-area", "grid_fast", FULL, 16, {}, {}, {}),
    ("zero-area", "bvh", FULL, 3, {}, {}, {}),
    ("negated", "grid_fast", FULL, 16, {}, {}, {}),
    ("negated", "bvh", FULL, 3, {}, {}, {}),
    ("mixed", "grid", FULL, 3, {}, {}, {}),
    ("mixed", "grid_fast", FULL, 16, {}, {}, {}),
    ("mixed", "bvh", FULL, 3, {}, {}, {}),
]


@pytest.mark.parametrize("name,accel,size,pipes,envvars,cfgkw,opt", RENDER_CASES)
def test_render_equals_the_restatement(gpu, pt_mod, monkeypatch, name, accel, size, pipes, envvars, cfgkw, opt):
    P = pt_mod
    for k, v in envvars.items():
        monkeypatch.setenv(k, v)                         # read by allocateOnGPU
    scene = fixture(P, name)[0]
    cfg = make_cfg(P, accel, width=size[0], height=size[1], tail_drop=size[2], pipelines=pipes, **cfgkw)
    ref = restated(P, name, cfg, opt)
    r = rendered(P, scene, cfg, opt)
    what = f"{name} {accel} {size} p{pipes} {envvars} {cfgkw} {opt}"
    check_state(r, ref, what)
    r.free()
    assert np.isfinite(ref.S).all() and ref.S.any()
    # smooth shading changed the image: against the restated render of the same scene, all flat
    flat_ref = restated(P, name, cfg, opt, smooth=False)
    differ = differing_pixels(ref.S, flat_ref.S).sum()
    print(f"{what}: {ref.ident.hits} hits on smooth models ({ref.ident.not_finite} + {ref.ident.opposed} kept the flat "
          f"normal), {differ} of {size[0] * size[1]} pixels differ from the flat render")
    # (with every normal negated the paths that touch a torus run on inside it until their bounces are
    # spent, whichever normal scattered them: that image cannot tell; the hooks test below can)
    assert name == "negated" or differ > (20 if opt.get("mask") or size != FULL else 100)
    if name == "mixed":
        assert ref.ident.opposed >= 20
    if name == "zero-area":
        assert (ref.hit_model == 7).sum() > 10           # the camera sees the model with the zero-area triangle


# ---- 3. the hooks ---------------------------------------------------------------------------------

def hook_rays(flat_export, models, limit=None):
    o, d = zip(*(SS.torus_rays(flat_export, m, seed=30 + m) for m in models))
    o, d = np.concatenate(o), np.concatenate(d)
    if limit is not None and len(o) > limit:
        keep = np.random.RandomState(5).permutation(len(o))[:limit]
        o, d = np.ascontiguousarray(o[keep]), np.ascontiguousarray(d[keep])
    return o, d


def vertex_rays(a, model, vertices, per=12, seed=3):
    """`per` rays at each of the mesh vertices `vertices` of a model (world space), from seeded
    directions within 50 degrees of the vertex normal's side: hits land on and beside the vertex."""
    m2w = a["model_m2w"][model].astype(np.float64).reshape(4, 4).T
    p = np.repeat(a["vpos"][vertices].astype(np.float64) @ m2w[:3, :3].T + m2w[:3, 3], per, axis=0)
    rs = np.random.RandomState(seed)
    centre = m2w[:3, 3]
    out = p - centre                                     # roughly outward for a torus tube seen from far away
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    u = rs.normal(size=out.shape)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = p + (out + u) * 120.0
    return np.ascontiguousarray(o, F), np.ascontiguousarray(p - o, F)


def hook_reference(O, flat, flags, o, d, accel):
    dist, nrm, model = O.intersect_rays(flat, o, d, accel=oracle_accel(accel), threads=4)
    ident = SR.Identification()
    want, tri, why = SR.shading_normals(flat, SR.Tables(flat), flags, o, d, dist, nrm, model, ident)
    assert ident.holds()
    return dist, want, model, nrm, tri, why


@pytest.mark.parametrize("accel", ["grid", "grid_fast", "bvh"])
@pytest.mark.parametrize("name", ["torus-320", "torus-1000", "mixed", "negated"])
def test_hook_normals_equal_the_restatement(gpu, pt_mod, oracle_mod, accel, name):
    """intersect_rays for the three accels and trace_rays for the two with persistent traces: rays
    through vertices and edge midpoints (the clamp), interior points and grazing rays."""
    P, O = pt_mod, oracle_mod
    scene, flat, flags = fixture(P, name)
    a = scene.export()
    o, d = hook_rays(a, (2, 3, 4, 5, 6))
    if name == "mixed":
        mesh_first = int(a["mesh_ranges"][2, 0])
        zeroed = mesh_first + np.nonzero(~a["vnrm"][mesh_first:int(a["mesh_ranges"][2, 1])].any(axis=1))[0]
        assert len(zeroed) >= 5
        vo, vd = vertex_rays(a, 3, zeroed)
        o, d = np.concatenate([o, vo]), np.concatenate([d, vd])
    cfg = make_cfg(P, accel, pipelines=1)
    dist, want, model, flat_nrm, tri, why = hook_reference(O, flat, flags, o, d, cfg.accel)
    hit_smooth = (model >= 2) & (model <= 5)
    print(f"{name} {accel}: {len(o)} rays, {hit_smooth.sum()} hit a smooth torus, {(model == 6).sum()} the flat one; "
          f"kept the flat normal: {(why == 1).sum()} not finite, {(why == 2).sum()} opposed")
    assert hit_smooth.sum() > len(o) // 2 and (model == 6).sum() > 100
    if name == "mixed":
        assert (why == 1).sum() >= 3 and (why == 2).sum() >= 20
        assert_bitexact(want[why > 0], flat_nrm[why > 0], "a fallback is the flat normal")
    else:
        assert differing_pixels(want[hit_smooth], flat_nrm[hit_smooth]).mean() > 0.9
    r = P.Renderer(cfg)
    r.allocateOnGPU(scene)
    got = r.intersect_rays(o, d)
    for g, w, what in zip(got, (dist, want, model), ("distance", "normal", "model")):
        assert_bitexact(g, w, f"{name} {accel} intersect_rays: {what}")
    if accel != "grid":
        n = min(len(o), W * H)
        td, tn, tm, tt = r.trace_rays(o[:n], d[:n])
        for g, w, what in zip((td, tn, tm), (dist[:n], want[:n], model[:n]), ("distance", "normal", "model")):
            assert_bitexact(g, w, f"{name} {accel} trace_rays: {what}")
        looked = tri[:n] >= 0
        assert np.array_equal(tt[looked], tri[:n][looked])           # the identified triangle is the traced one
        # a sparse survivor layout: the slot's ray is found through k_scan's offsets
        counts = np.random.RandomState(9).randint(0, cfg.block + 1, (W * H + cfg.block - 1) // cfg.block)
        m = min(int(counts.sum()), n)
        counts = np.minimum(counts, np.maximum(m - np.concatenate([[0], np.cumsum(counts)[:-1]]), 0))
        td, tn, tm, _ = r.trace_rays(o[:m], d[:m], counts)
        assert_bitexact(tn, want[:m], f"{name} {accel} trace_rays, sparse layout: normal")
        assert_bitexact(tm, model[:m], f"{name} {accel} trace_rays, sparse layout: model")
    assert r.trace_faults() == 0
    r.free()


# ---- 4. off means off -----------------------------------------------------------------------------

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


@pytest.mark.parametrize("accel,pipes", [("grid_fast", 16), ("bvh", 3), ("grid", 1)])
def test_off_means_off_and_flags_are_snapshot_at_allocation(gpu, pt_mod, accel, pipes):
    P = pt_mod
    spec = SS.fixture_spec(320)
    never = SS.gpu_scene(P, (spec[0], spec[1], np.zeros(len(spec[1]), bool)))
    cfg = make_cfg(P, accel, pipelines=pipes)
    r = rendered(P, never, cfg)
    want, want_hits = state(r), r.primary_hits()
    r.free()
    flat_ref = restated(P, "torus-320", cfg, smooth=False)
    assert_bitexact(want[0], flat_ref.S, "never set: the flat restatement")
    cleared = SS.gpu_scene(P, spec)
    cleared.set_smooth(None, False)                      # set, then cleared before allocation
    r = rendered(P, cleared, cfg)
    assert_same_state(state(r), want, f"{accel} p{pipes}: set and cleared")
    for g, w in zip(r.primary_hits(), want_hits):
        assert_bitexact(g, w, "set and cleared: primary hits")
    # a flag changed after allocateOnGPU applies to the next allocation
    for i in np.nonzero(spec[2])[0]:
        cleared.set_smooth(int(i))
    r.clearImage()
    r.renderLoop(0, ITERS)
    assert_same_state(state(r)[:3], want[:3], "flags set after allocation: still the snapshot")
    r.allocateOnGPU(cleared)
    r.renderLoop(0, ITERS)
    smooth_ref = restated(P, "torus-320", cfg)
    assert_bitexact(r.image(), smooth_ref.S, "the next allocation: smooth")
    assert r.trace_faults() == 0
    r.free()


# ---- 5. it is actually smooth ---------------------------------------------------------------------

SPHERE_SCENE = """
METAL
chrome
[0.9, 0.9, 0.95]

SPHERE
ball
0.1
[0.02, 0.05, -0.03]
translate:[40,120,60]
rotate:[25,40,10]
scale:[1.5,1.5,1.5]
material:chrome
shading:smooth
"""
SPHERE_CENTRE, SPHERE_RADIUS = (0.02, 0.05, -0.03), 0.1


@pytest.mark.parametrize("accel", ["grid", "grid_fast", "bvh"])
def test_a_smooth_sphere_has_radial_normals(gpu, pt_mod, tmp_path, accel):
    """In exact arithmetic the interpolated normal of a sphere with radial vertex normals is the
    radial direction of the hit point on the facet.  What remains: float32 rounding (about 1e-5)
    and the clamp at edge points the triangle test accepts a tolerance outside the facet, at most
    0.01 of a barycentric coordinate times the 0.13 rad facet angle = 1.3e-3.  Bound: 5e-3 per
    component.  The flat normal on the same rays is off by up to half a facet (0.065 rad)."""
    P = pt_mod
    path = tmp_path / "sphere.txt"
    path.write_text(SPHERE_SCENE)
    s = P.Scene(str(path))
    assert s.smooth().tolist() == [True] and s.counts()["nt"] == 2208
    s.build()
    a = s.export()
    m2w = a["model_m2w"][0].astype(np.float64).reshape(4, 4).T
    centre = m2w[:3, :3] @ (np.array(SPHERE_CENTRE) * 1000.0) + m2w[:3, 3]
    radius = SPHERE_RADIUS * 1000.0 * 1.5
    rs = np.random.RandomState(17)
    u = rs.normal(size=(3000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = rs.normal(size=(3000, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    o = centre + u * radius * 4.0
    target = centre + v * radius * rs.uniform(0, 0.999, (3000, 1))       # through the ball: head-on to grazing
    o, d = np.ascontiguousarray(o, F), np.ascontiguousarray((target - o) * rs.uniform(0.1, 2.0, (3000, 1)), F)
    cfg = make_cfg(P, accel, pipelines=1)
    worst = {}
    for smooth in (True, False):
        s.set_smooth(0, smooth)
        r = P.Renderer(cfg)
        r.allocateOnGPU(s)
        dist, n, model = r.intersect_rays(o, d)
        assert r.trace_faults() == 0
        r.free()
        hit = model == 0
        assert hit.sum() > 2500
        o64, d64 = o.astype(np.float64)[hit], d.astype(np.float64)[hit]
        ip = o64 + d64 / np.linalg.norm(d64, axis=1, keepdims=True) * dist[hit].astype(np.float64)[:, None]
        radial = (ip - centre) / np.linalg.norm(ip - centre, axis=1, keepdims=True)
        worst[smooth] = float(np.abs(n[hit].astype(np.float64) - radial).max())
    print(f"{accel}: largest component difference from the radial direction: smooth {worst[True]:.3g}, flat {worst[False]:.3g}")
    assert worst[True] <= 5e-3
    assert worst[False] > 2e-2


# ---- 6. the denoiser ------------------------------------------------------------------------------

@pytest.mark.parametrize("accel,size", [("grid_fast", (64, 48)), ("bvh", (37, 23))])
def test_denoise_reads_the_smooth_guides(gpu, pt_mod, accel, size):
    P = pt_mod
    scene, flat, flags = fixture(P)
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
    ref = SR.Restatement(flat, oracle_cfg(cfg, threads=4), smooth=flags)
    for g, w, name in zip((d, n, k), ref.primary_hits(), ("distance", "normal", "model")):
        assert_bitexact(g, w, f"guides: {name}")
    want_img, want_var = DR.denoise(S, Q, size[0], size[1], 6, d, n, k)
    assert_bitexact(img, want_img, "denoise: image")
    assert_bitexact(var, want_var, "denoise: variance")
    flat_img, _ = DR.denoise(S, Q, size[0], size[1], 6, d, ref.hit_nrm, k)
    assert differing_pixels(img, flat_img).sum() > 20       # the guides matter: flat ones filter differently
