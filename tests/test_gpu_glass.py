"""The dielectric material on the GPU (include/pathtracer_amd.h, "Dielectric material"), against
the restatement in glass_ref.py (which tests/test_glass_ref.py holds to texture_ref's, to a float64
evaluation and to Snell's law).

S (image), Q (moments), the per-tile sample counts, the segment count and the per-bounce segment
counts are compared bit for bit; every render must leave trace_faults() at 0 and a finite image.
The fixture (glass_scenes.fixture_spec): a glass box and the displaced torus as glass flat, smooth
and textured, and once diffuse, in the flat room under its lamp; iors 1.33, 1.5 and 2.4."""
import numpy as np
import pytest

import adaptive_ref as AR
import camera_ref as CR
import denoise_albedo_ref as DAR
import env_ref as ER
import glass_ref as GR
import glass_scenes as GS
from helpers import assert_bitexact, flat_from_export, oracle_cfg

pytestmark = pytest.mark.gpu

F = np.float32
W, H, BOUNCES, ITERS, LENS = 64, 48, 6, 3, 25.0
VIEW_A = dict(eye=(0, 800, 500), target=(0, 0, 0), vfov_deg=45, focus_dist=900)
UP_Y = np.float32([[0, 0, 1], [1, 0, 0], [0, 1, 0]])


def accel_of(P, name):
    return {"grid_fast": P.ACCEL_GRID_FAST, "grid": P.ACCEL_GRID, "bvh": P.ACCEL_BVH}[name]


def make_cfg(P, accel="grid_fast", **kw):
    base = dict(width=W, height=H, max_bounces=BOUNCES, iterations=ITERS, accel=accel_of(P, accel))
    base.update(kw)
    return P.RenderConfig(**base)


_SCENES = {}


def fixture(P):
    """(scene, FlatScene, spec), built once."""
    if not _SCENES:
        spec = GS.fixture_spec()
        s = GS.gpu_scene(P, spec)
        assert [np.float32(s.ior(i)) for i in range(len(spec["ior"]))] == spec["ior"].tolist()
        _SCENES["f"] = (s, flat_from_export(s.export()), spec)
    return _SCENES["f"]


def half_mask(w, h, seed=20):
    ty, tx = AR.tiles_shape(w, h)
    m = (np.random.RandomState(seed).permutation(ty * tx) < (ty * tx) // 2).reshape(ty, tx)
    assert m.any() and not m.all()
    return m


def options(P, cfg, opt):
    cam = P.look_at(lens_radius=opt.get("lens", 0.0), width=cfg.width, height=cfg.height, **VIEW_A) if opt.get("view") else None
    mask = half_mask(cfg.width, cfg.height) if opt.get("mask") else None
    env = P.Environment(np.random.RandomState(77).uniform(0, 2, (8, 8, 3)), (1.5, 1.0, 0.5), UP_Y) if opt.get("env") else None
    return cam, opt.get("jitter"), mask, env


def restatement(P, flat, spec, cfg, opt=None, textured=True, smooth=True):
    cam, jitter, _, env = options(P, cfg, opt or {})
    return GR.Restatement(flat, oracle_cfg(cfg, threads=4), width=jitter, camera=None if cam is None else CR.Cam.of(cam),
                          env=None if env is None else ER.Env.of(env), smooth=spec["smooth"] if smooth else None,
                          uv=GS.vertex_uv(spec), textures=spec["textures"], binding=spec["binding"] if textured else None,
                          ior=spec["ior"])


_REFS = {}


def restated(P, cfg, opt=None, textured=True, smooth=True):
    """The restated render of iterations [0, ITERS) (shared; never modified)."""
    opt = {k: v for k, v in (opt or {}).items() if k != "loops"}
    _, flat, spec = fixture(P)
    o = oracle_cfg(cfg, threads=4)
    key = (textured, smooth, o.width, o.height, o.accel, o.tail_drop, tuple(sorted(opt.items())))
    if key not in _REFS:
        ref = restatement(P, flat, spec, cfg, opt, textured, smooth)
        ref.render(0, ITERS, options(P, cfg, opt)[2])
        assert ref.tex_ident.holds() and ref.ident.holds()
        assert np.isfinite(ref.S).all() and ref.S.any()
        _REFS[key] = ref
    return _REFS[key]


def rendered(P, scene, cfg, opt=None):
    opt = opt or {}
    cam, jitter, mask, env = options(P, cfg, opt)
    r = P.Renderer(cfg)
    r.enable_moments()
    if cam is not None:
        r.set_camera(cam)
    if jitter is not None:
        r.set_pixel_jitter(jitter)
    if env is not None:
        r.set_environment(env)
    r.allocateOnGPU(scene)
    for first, n in opt.get("loops", [(0, ITERS)]):
        if mask is None:
            r.renderLoop(first, n)
        else:
            r.render_masked(mask, first, n)
    return r


def check_state(r, ref, what):
    assert_bitexact(r.image(), ref.S, f"{what}: image")
    assert_bitexact(r.moments(), ref.Q, f"{what}: moments")
    assert_bitexact(r.sample_counts(), ref.counts, f"{what}: counts")
    assert r.segments() == ref.segments, (what, r.segments(), ref.segments)
    assert r.segments_per_bounce(10) == ref.per_bounce[:10].tolist(), what
    assert r.trace_faults() == 0, what
    assert np.isfinite(r.image()).all(), what


def state(r):
    out = (r.image(), r.moments(), r.sample_counts(), r.segments(), r.segments_per_bounce(10))
    assert r.trace_faults() == 0 and np.isfinite(out[0]).all()
    return out


def assert_same_state(got, want, what):
    for g, w, name in zip(got, want, ("image", "moments", "counts", "segments", "segments per bounce")):
        if isinstance(w, np.ndarray):
            assert_bitexact(g, w, f"{what}: {name}")
        else:
            assert g == w, (what, name, g, w)


def differing_pixels(a, b):
    return (np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(axis=1)


# ---- 1. the hook ------------------------------------------------------------------------------------

def test_the_hook_equals_the_definition(gpu, pt_mod):
    """4096 random inputs and the edge cases of glass_scenes.hook_inputs: normal incidence from both
    sides, |ci| below 1e-6, c stepped ulp by ulp across the critical angle for ior 1.33, 1.5 and 4,
    ior exactly 1, u equal to Fr, one ulp below it and 0, and unnormalised directions."""
    P = pt_mod
    (d, n, ior, u), where = GS.hook_inputs()
    want_dir, want_event = GR.hook(d, n, ior, u)
    got_dir, got_event = P.selftest_dielectric(d, n, ior, u)
    for name, sl in where.items():
        assert np.array_equal(got_event[sl], want_event[sl]), f"{name}: event"
        assert_bitexact(got_dir[sl], want_dir[sl], f"{name}: direction")
    assert np.isfinite(got_dir).all() and len(got_dir) == len(d) > 4096 + 500
    assert all(c > 100 for c in np.bincount(got_event, minlength=4))
    empty = P.selftest_dielectric(np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros(0, F), np.zeros(0, F))
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,)


# ---- 2, 3, 5. renders ---------------------------------------------------------------------------------

FULL = (W, H, 0)
ODD = (37, 23, 1)
# accel, (width, height, tail_drop), pipelines, environment variables, config fields, options
RENDER_CASES = [
    ("grid", FULL, 1, {}, {}, {}),
    ("grid", ODD, 16, {}, {}, {}),
    ("grid_fast", FULL, 1, {}, {}, {}),
    ("grid_fast", FULL, 16, {}, {}, {}),
    ("grid_fast", ODD, 16, {}, {}, {}),
    ("grid_fast", (37, 23, 0), 1, {}, {}, {}),
    ("bvh", FULL, 1, {}, {}, {}),
    ("bvh", FULL, 16, {}, {}, {}),
    ("bvh", ODD, 1, {}, {}, {}),
    ("grid_fast", FULL, 16, {}, {"block": 128}, {}),            # 64 is the default: every other case runs it
    ("bvh", FULL, 1, {}, {"block": 128}, {}),
    ("grid_fast", FULL, 1, {}, {"block": 256}, {}),
    ("bvh", FULL, 16, {}, {"block": 256}, {}),
    ("grid", FULL, 16, {}, {"block": 256}, {}),
    ("grid_fast", FULL, 16, {"PT_GF_SPLIT": "0"}, {}, {}),         # the fused k_bounce
    ("bvh", FULL, 1, {"PT_TRACE_SPLIT": "0"}, {}, {}),
    ("grid_fast", ODD, 1, {"PT_GF_SPLIT": "0"}, {"block": 256}, {}),
    ("grid_fast", FULL, 16, {}, {"ray_sort": 0}, {}),              # get_hit, no slot_src
    ("bvh", FULL, 16, {}, {"ray_sort": 0}, {}),
    ("grid_fast", FULL, 16, {}, {"ray_sort": 7}, {}),
    ("grid_fast", FULL, 16, {"PT_SLOT_MAP": "0"}, {}, {}),         # sorted, get_hit
    ("bvh", FULL, 1, {"PT_SLOT_MAP": "0"}, {}, {}),
    ("grid_fast", FULL, 16, {}, {}, {"jitter": 1.0}),              # camera-ray hits through the hit buffer
    ("bvh", FULL, 1, {}, {}, {"view": True, "lens": LENS}),
    ("grid_fast", FULL, 16, {}, {}, {"view": True}),
    ("grid_fast", FULL, 16, {}, {}, {"mask": True}),               # k_bounce_masked
    ("bvh", FULL, 1, {}, {"block": 256}, {"mask": True}),
    ("grid_fast", ODD, 16, {}, {}, {"jitter": 1.0, "mask": True}),
    ("grid_fast", FULL, 16, {}, {}, {"env": True}),
    ("bvh", FULL, 1, {}, {}, {"env": True}),
    ("grid_fast", FULL, 16, {"PT_GRAPH": "1"}, {}, {"loops": ((0, 1), (1, 2))}),
    ("bvh", FULL, 16, {"PT_GRAPH": "1"}, {}, {"loops": ((0, 2), (2, 1))}),
]


@pytest.mark.parametrize("accel,size,pipes,envvars,cfgkw,opt", RENDER_CASES)
def test_render_equals_the_restatement(gpu, pt_mod, monkeypatch, accel, size, pipes, envvars, cfgkw, opt):
    P = pt_mod
    for k, v in envvars.items():
        monkeypatch.setenv(k, v)                         # read by allocateOnGPU
    scene = fixture(P)[0]
    cfg = make_cfg(P, accel, width=size[0], height=size[1], tail_drop=size[2], pipelines=pipes, **cfgkw)
    ref = restated(P, cfg, opt)
    r = rendered(P, scene, cfg, opt)
    what = f"{accel} {size} p{pipes} {envvars} {cfgkw} {opt}"
    try:
        check_state(r, ref, what)
    finally:
        r.free()
    print(f"{what}: events {dict(zip(GR.EVENT_NAMES, ref.events.tolist()))}, {ref.smooth_exits} exits on the smooth instance")
    if not opt.get("mask") and size == FULL:
        assert (ref.events >= 50).all() and ref.smooth_exits >= 20


# ---- 4. smooth glass and textured glass ---------------------------------------------------------------

@pytest.mark.parametrize("accel,pipes", [("grid_fast", 16), ("bvh", 1)])
def test_smooth_and_textured_glass(gpu, pt_mod, accel, pipes):
    """The smooth instance refracts by its interpolated normal and the textured one tints by its
    texture's albedo on entry: the render equals the restatement with both, and differs from the
    restatements without the smooth flag and without the binding."""
    P = pt_mod
    scene, flat, spec = fixture(P)
    cfg = make_cfg(P, accel, pipelines=pipes)
    ref = restated(P, cfg)
    r = rendered(P, scene, cfg)
    try:
        check_state(r, ref, f"{accel} p{pipes}")
        albedo, model = r.primary_albedo(), r.primary_hits()[2]
    finally:
        r.free()
    assert_bitexact(albedo, ref.primary_albedo(), "primary albedo")
    flat_ref, plain_ref = restated(P, cfg, smooth=False), restated(P, cfg, textured=False)
    unsmoothed, untextured = differing_pixels(ref.S, flat_ref.S).sum(), differing_pixels(ref.S, plain_ref.S).sum()
    print(f"{accel}: {unsmoothed} pixels differ from the render without the smooth flag, {untextured} from the one without "
          f"the texture; {(model == GS.SMOOTH).sum()} / {(model == GS.TEXTURED).sum()} primary hits on the two instances")
    assert unsmoothed > 20 and untextured > 20
    assert (model == GS.SMOOTH).sum() > 20 and (model == GS.TEXTURED).sum() > 20
    # primary_albedo on a glass pixel: the model's colour; on the textured instance: times the texture
    box = model == GS.BOX
    assert box.sum() > 20
    assert_bitexact(albedo[box], np.repeat(F(spec["models"][GS.BOX]["color"])[None, :], box.sum(), axis=0), "glass box albedo")
    tex = model == GS.TEXTURED
    assert differing_pixels(albedo[tex], np.repeat(F(spec["models"][GS.TEXTURED]["color"])[None, :], tex.sum(), axis=0)).mean() > 0.9


# ---- 6. off by default ----------------------------------------------------------------------------------

@pytest.mark.parametrize("accel,pipes", [("grid_fast", 16), ("bvh", 1), ("grid", 1)])
def test_an_ior_on_diffuse_models_changes_nothing(gpu, pt_mod, accel, pipes):
    P = pt_mod
    spec = GS.as_diffuse(fixture(P)[2])
    cfg = make_cfg(P, accel, pipelines=pipes)
    r = rendered(P, GS.gpu_scene(P, spec, ior=False), cfg)
    want = state(r)
    r.free()
    with_ior = GS.gpu_scene(P, spec, ior=True)
    assert np.float32(with_ior.ior(GS.TEXTURED)) == np.float32(2.4)
    r = rendered(P, with_ior, cfg)
    got = state(r)
    r.free()
    assert_same_state(got, want, f"{accel} p{pipes}: an ior on diffuse models")
    assert differing_pixels(want[0], restated(P, cfg).S).sum() > W * H // 8        # and glass is another image


# ---- 7. the denoiser ------------------------------------------------------------------------------------

@pytest.mark.parametrize("accel,size", [("grid_fast", (64, 48)), ("bvh", (37, 23))])
def test_demodulated_denoise_of_a_glass_render_equals_its_reference(gpu, pt_mod, accel, size):
    P = pt_mod
    scene, flat, spec = fixture(P)
    cfg = make_cfg(P, accel, width=size[0], height=size[1], pipelines=3)
    r = rendered(P, scene, cfg)
    try:
        S, Q = r.image(), r.moments()
        d, n, k = r.primary_hits()
        albedo = r.primary_albedo()
        for flags in (DAR.DEMODULATE, DAR.DEMODULATE | DAR.TILE_COUNTS):
            by_tile = bool(flags & DAR.TILE_COUNTS)
            img, var = r.denoise(variance=True, flags=flags)
            want_img, want_var = DAR.denoise(S, Q, size[0], size[1], None if by_tile else ITERS, d, n, k, albedo=albedo,
                                             counts=r.sample_counts() if by_tile else None)
            assert_bitexact(img, want_img, f"{accel} {size} flags={flags}: image")
            assert_bitexact(var, want_var, f"{accel} {size} flags={flags}: variance")
            assert np.isfinite(img).all()
        assert r.trace_faults() == 0
    finally:
        r.free()
    assert_bitexact(S, restated(P, cfg).S, "the glass render")
    glass = np.isin(k, GS.glass_models(spec))
    assert glass.sum() > 50
    colour = np.asarray(flat.model_color, F)[np.maximum(k, 0)]
    untextured = glass & (k != GS.TEXTURED)
    assert_bitexact(albedo[untextured], colour[untextured], "primary_albedo on a glass pixel: the model's colour")
