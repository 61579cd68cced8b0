"""Direct lighting on the GPU (include/pathtracer_amd.h, "Direct lighting"), against the
restatement in direct_ref.py (which tests/test_direct_ref.py holds to glass_ref's and to the plain
estimator's expectation).

The any-hit query (pt_renderer_occluded) is compared with the oracle's exact closest hit on about
4k segments per scene; the estimator (pt_renderer_direct_sample) and whole renders are compared bit
for bit.  A shadow ray whose closest occluder lies within direct_ref.NEAR_TIE * tmax of tmax is a
near tie, where the any-hit walk may round one distance the other way: such segments, and the
pixels that traced one, are left out, and their share is asserted from the oracle alone."""
import numpy as np
import pytest

import adaptive_ref as AR
import camera_ref as CR
import denoise_albedo_ref as DAR
import direct_ref as DR
import direct_scenes as DS
import env_ref as ER
import glass_scenes as GS
import path_scenes as PS
from helpers import assert_bitexact, flat_from_export, oracle_cfg

pytestmark = pytest.mark.gpu

F = np.float32
W, H, BOUNCES, ITERS, LENS = 64, 48, 4, 2, 25.0
VIEW_A = dict(eye=(0, 800, 500), target=(0, 0, 0), vfov_deg=45, focus_dist=900)
UP_Y = np.float32([[0, 0, 1], [1, 0, 0], [0, 1, 0]])
SEGMENT_TIES, PIXEL_TIES = 0.01, 0.005


def accel_of(P, name):
    return {"grid_fast": P.ACCEL_GRID_FAST, "grid": P.ACCEL_GRID, "bvh": P.ACCEL_BVH}[name]


def make_cfg(P, accel="grid_fast", **kw):
    base = dict(width=W, height=H, max_bounces=BOUNCES, iterations=ITERS, accel=accel_of(P, accel))
    base.update(kw)
    return P.RenderConfig(**base)


_SCENES = {}


def fixture(P, lights=True):
    """(scene, FlatScene, spec), built once."""
    if lights not in _SCENES:
        spec = DS.direct_spec() if lights else DS.without_lights(DS.direct_spec())
        s = GS.gpu_scene(P, spec)
        _SCENES[lights] = (s, flat_from_export(s.export()), spec)
    return _SCENES[lights]


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


def restatement(P, flat, spec, cfg, opt=None, **kw):
    cam, jitter, _, env = options(P, cfg, opt or {})
    return DR.Restatement(flat, oracle_cfg(cfg, threads=4), width=jitter, camera=None if cam is None else CR.Cam.of(cam),
                          env=None if env is None else ER.Env.of(env), smooth=spec["smooth"], uv=GS.vertex_uv(spec),
                          textures=spec["textures"], binding=spec["binding"], ior=spec["ior"], **kw)


_REFS = {}


def restated(P, cfg, opt=None):
    """The restated direct-light render of iterations [0, ITERS) (shared; never modified)."""
    opt = {k: v for k, v in (opt or {}).items() if k != "loops"}
    _, flat, spec = fixture(P)
    o = oracle_cfg(cfg, threads=4)
    key = (o.width, o.height, o.accel, o.tail_drop, tuple(sorted(opt.items())))
    if key not in _REFS:
        ref = restatement(P, flat, spec, cfg, opt)
        ref.render(0, ITERS, options(P, cfg, opt)[2])
        assert ref.tex_ident.holds() and ref.ident.holds()
        assert np.isfinite(ref.S).all() and ref.S.any()
        _REFS[key] = ref
    return _REFS[key]


def rendered(P, scene, cfg, opt=None, direct=True):
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
    if direct:
        r.set_direct_light()
    r.allocateOnGPU(scene)
    for first, n in opt.get("loops", [(0, ITERS)]):
        if mask is None:
            r.renderLoop(first, n)
        else:
            r.render_masked(mask, first, n)
    return r


def check_state(r, ref, what):
    keep = ~ref.near_tie_pixels
    assert ref.near_tie_pixels.sum() <= PIXEL_TIES * len(keep), (what, int(ref.near_tie_pixels.sum()))
    assert_bitexact(r.image()[keep], ref.S[keep], f"{what}: image")
    assert_bitexact(r.moments()[keep], ref.Q[keep], f"{what}: moments")
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


# ---- 1. the any-hit query ---------------------------------------------------------------------------

def segments_of(P, name):
    if name == "room":
        s, flat, _ = fixture(P)
        o, t, where = DS.room_segments(flat, DR.light_table(flat))
        return s, flat, o, t, where
    s, o, d = PS.degenerate_case(P, name)
    flat = flat_from_export(s.export())
    o, t = DS.ray_segments(flat, o, d)
    return s, flat, o, t, {"all": slice(0, len(o))}


@pytest.mark.parametrize("name", DS.SCENES)
@pytest.mark.parametrize("accel", ["bvh", "grid_fast"])
def test_occluded_equals_the_oracle(gpu, pt_mod, oracle_mod, name, accel):
    P = pt_mod
    s, flat, o, t, where = segments_of(P, name)
    want, near = DS.decided(flat, o, t)
    zero = (o == t).all(axis=1)
    assert len(o) >= 3500 and near.mean() <= SEGMENT_TIES and zero.sum() >= 100
    assert want[~near].sum() > 300 and (~want[~near & ~zero]).sum() > 300          # both answers, often
    r = P.Renderer(P.RenderConfig(width=8, height=8, iterations=1, accel=accel_of(P, accel), pipelines=1))
    r.allocateOnGPU(s)
    try:
        got = r.occluded(o, t)
        assert r.trace_faults() == 0
        assert r.occluded(np.zeros((0, 3), F), np.zeros((0, 3), F)).shape == (0,)
    finally:
        r.free()
    assert not got[zero].any(), "a segment of zero length reads unoccluded"
    for part, sl in where.items():
        k = ~near[sl]
        bad = np.nonzero(got[sl][k] != want[sl][k])[0]
        assert len(bad) == 0, f"{name} {accel} {part}: {len(bad)} of {k.sum()} segments differ, first {bad[:5]}"
    print(f"{name} {accel}: {len(o)} segments, {int(want.sum())} occluded, {int(near.sum())} near ties left out, "
          f"{int((got[near] != want[near]).sum())} of them differ")


# ---- 2. the estimator -------------------------------------------------------------------------------

def test_direct_sample_equals_the_restatement(gpu, pt_mod, oracle_mod):
    """The recorded diffuse hits of two iterations of the fixture room (flat room, flat, smooth and
    textured torus as receivers; a rotated, non-uniformly scaled lamp and a second rotated one):
    the chosen light, y, g and Dc bit for bit, the visibility flag on every hit that is no near tie."""
    P = pt_mod
    scene, flat, spec = fixture(P)
    cfg = make_cfg(P, "bvh", pipelines=1)
    ref = restatement(P, flat, spec, cfg, record=True)
    ref.render(0, 2)
    rec = {k: np.concatenate([b[k] for b in ref.records]) for k in ref.records[0]}
    n = len(rec["slot"])
    per_model = np.bincount(rec["model"], minlength=len(spec["models"]))
    assert n > 5000 and per_model[0] > 1000 and min(per_model[GS.SMOOTH], per_model[GS.TEXTURED], per_model[GS.DIFFUSE]) > 20
    assert rec["near"].mean() <= PIXEL_TIES
    r = rendered(P, scene, cfg, {"loops": []})
    try:
        assert DR.same_table(r.lights(), ref.lights), "lights() is the table the restatement was given"
        on, count, area = r.direct_light()
        assert on and count == len(ref.lights["cdf"]) == 24 and F(area) == ref.lights["area_total"]
        # the scene triangle of every recorded hit, from the trace (at most a frame of rays per call)
        parts = [r.trace_rays(rec["o"][a:a + W * H], rec["d"][a:a + W * H]) for a in range(0, n, W * H)]
        dist, _, model, tri = (np.concatenate([p[q] for p in parts]) for q in range(4))
        assert_bitexact(dist, rec["dist"], "the recorded hits' distances")
        assert np.array_equal(model, rec["model"]) and (tri >= 0).all()
        got = r.direct_sample(rec["o"], rec["d"], rec["dist"], rec["model"], tri, rec["color"], rec["it"], rec["slot"],
                              rec["bounces"])
        assert r.trace_faults() == 0
        with pytest.raises(P.PathTracerError, match="model index out of range"):
            r.direct_sample(rec["o"][:1], rec["d"][:1], rec["dist"][:1], [99], tri[:1], rec["color"][:1], 0, 0, 1)
        with pytest.raises(P.PathTracerError, match="triangle index out of range"):
            r.direct_sample(rec["o"][:1], rec["d"][:1], rec["dist"][:1], rec["model"][:1], [-1], rec["color"][:1], 0, 0, 1)
        with pytest.raises(P.PathTracerError, match="bounces in 0 .. 63"):
            r.direct_sample(rec["o"][:1], rec["d"][:1], rec["dist"][:1], rec["model"][:1], tri[:1], rec["color"][:1], 0, 0, 64)
    finally:
        r.free()
    assert np.array_equal(got["light"], rec["light"])
    for key in ("y", "g", "dc"):
        assert_bitexact(got[key], rec[key], f"direct_sample: {key}")
    k = ~rec["near"]
    assert np.array_equal(got["visible"][k], rec["visible"][k])
    chosen = np.bincount(rec["light"][rec["light"] >= 0], minlength=24)
    print(f"{n} hits, {int((rec['light'] < 0).sum())} failed the geometry test, {int(rec['visible'].sum())} unoccluded, "
          f"{int(rec['near'].sum())} near ties; lights chosen {chosen.tolist()}")
    assert (rec["light"] < 0).sum() > 50 and rec["visible"].sum() > 500 and (chosen[12:] > 0).sum() >= 2


# ---- 3. renders -------------------------------------------------------------------------------------

FULL = (W, H, 0)
ODD = (37, 23, 1)
# accel, (width, height, tail_drop), pipelines, environment variables, config fields, options
RENDER_CASES = [
    ("bvh", FULL, 1, {}, {}, {}),
    ("bvh", FULL, 3, {}, {}, {}),
    ("bvh", FULL, 16, {}, {}, {}),
    ("grid_fast", FULL, 1, {}, {}, {}),
    ("grid_fast", FULL, 3, {}, {}, {}),
    ("grid_fast", FULL, 16, {}, {}, {}),
    ("bvh", ODD, 3, {}, {}, {}),
    ("grid_fast", ODD, 16, {}, {}, {}),
    ("grid_fast", (37, 23, 0), 1, {}, {}, {}),
    ("bvh", (37, 23, 0), 16, {}, {}, {}),
    ("bvh", (1, 1, 0), 1, {}, {}, {}),
    ("grid_fast", (1, 1, 0), 3, {}, {}, {}),
    ("grid_fast", FULL, 16, {}, {"block": 256}, {}),              # 64 is the default: every other case runs it
    ("bvh", FULL, 1, {}, {"block": 256}, {}),
    ("bvh", ODD, 3, {}, {"block": 256}, {}),
    ("grid_fast", FULL, 16, {}, {"ray_sort": 0}, {}),              # no sort: the blk_off search
    ("bvh", FULL, 3, {}, {"ray_sort": 0}, {}),
    ("grid_fast", FULL, 16, {"PT_SLOT_MAP": "0"}, {}, {}),         # sorted, without the slot map
    ("bvh", FULL, 1, {"PT_SLOT_MAP": "0"}, {}, {}),
    ("grid_fast", FULL, 16, {}, {}, {"jitter": 1.0}),              # generated rays: every hit through the hit buffer
    ("bvh", FULL, 3, {}, {}, {"view": True, "lens": LENS}),
    ("grid_fast", FULL, 3, {}, {}, {"view": True}),
    ("grid_fast", FULL, 16, {}, {}, {"mask": True}),               # k_direct<FIRST> under the tile mask
    ("bvh", FULL, 1, {}, {"block": 256}, {"mask": True}),
    ("grid_fast", ODD, 16, {}, {}, {"jitter": 1.0, "mask": True}),
    ("grid_fast", FULL, 16, {}, {}, {"env": True}),
    ("bvh", FULL, 1, {}, {}, {"env": True}),
    ("grid_fast", FULL, 3, {"PT_GRAPH": "1"}, {}, {"loops": ((0, 1), (1, 1))}),     # the second call replays pipeline 0's graph
    ("bvh", FULL, 1, {"PT_GRAPH": "1"}, {}, {}),                                    # captured at iteration 0, replayed at 1
    ("bvh", FULL, 16, {}, {}, {"loops": ((0, 1), (1, 1))}),
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
    print(f"{what}: {ref.sampled} light samples, {ref.shadow_rays} shadow rays, {ref.shadow_occluded} occluded, "
          f"{ref.suppressed_hits} suppressed emissive hits, {int(ref.near_tie_pixels.sum())} near-tie pixels left out")
    if size == FULL and not opt.get("mask"):
        assert ref.sampled > 5000 and ref.shadow_occluded > 500 and ref.suppressed_hits > 50


# ---- 4. off means off -------------------------------------------------------------------------------

@pytest.mark.parametrize("accel,pipes", [("grid_fast", 16), ("bvh", 1)])
def test_no_light_in_the_scene_is_the_plain_render(gpu, pt_mod, accel, pipes):
    P = pt_mod
    scene = fixture(P, lights=False)[0]
    cfg = make_cfg(P, accel, pipelines=pipes)
    r = rendered(P, scene, cfg, direct=False)
    want = state(r)
    r.free()
    r = rendered(P, scene, cfg)
    assert r.direct_light() == (True, 0, 0.0) and len(r.lights()["cdf"]) == 0
    got = state(r)
    with pytest.raises(P.PathTracerError, match="the scene has no light"):
        r.direct_sample(np.zeros((1, 3), F), np.ones((1, 3), F), [1.0], [0], [0], np.ones((1, 3), F), 0, 0, 1)
    r.free()
    assert_same_state(got, want, f"{accel} p{pipes}: direct light without a light")


@pytest.mark.parametrize("accel,pipes,graph", [("grid_fast", 16, "0"), ("bvh", 3, "1")])
def test_switching_after_allocation(gpu, pt_mod, monkeypatch, accel, pipes, graph):
    """Off after on equals the plain render; on after off equals the restatement; each change
    clears the accumulators and drops the captured graphs."""
    P = pt_mod
    monkeypatch.setenv("PT_GRAPH", graph)
    scene = fixture(P)[0]
    cfg = make_cfg(P, accel, pipelines=pipes)
    r = rendered(P, scene, cfg, direct=False)
    plain = state(r)
    r.set_direct_light()                                  # allocated: the table and the state come now
    assert not r.image().any() and not r.moments().any() and not r.sample_counts().any()
    assert r.direct_light()[:2] == (True, 24)
    r.renderLoop(0, ITERS)
    check_state_but_segments(r, restated(P, cfg), f"{accel} p{pipes}: on after off")
    r.set_direct_light(False)
    assert not r.image().any()
    r.renderLoop(0, ITERS)
    got = state(r)
    r.free()
    for g, w, name in zip(got[:3], plain[:3], ("image", "moments", "counts")):
        assert_bitexact(g, w, f"{accel} p{pipes}: off after on: {name}")
    differ = (got[0].view(np.uint32) != restated(P, cfg).S.view(np.uint32)).any(axis=1).sum()
    assert differ > W * H // 2                           # and direct light is another image
    # a renderer without moments refuses the switch after allocation, and renders on unchanged
    r = P.Renderer(cfg)
    r.allocateOnGPU(scene)
    with pytest.raises(P.PathTracerError, match="direct light needs moments"):
        r.set_direct_light()
    assert r.direct_light()[0] is False
    r.renderLoop(0, ITERS)
    assert_bitexact(r.image(), plain[0], "after the refusal")
    r.free()


def check_state_but_segments(r, ref, what):
    """check_state for a renderer whose segment counters hold an earlier render too."""
    keep = ~ref.near_tie_pixels
    assert_bitexact(r.image()[keep], ref.S[keep], f"{what}: image")
    assert_bitexact(r.moments()[keep], ref.Q[keep], f"{what}: moments")
    assert_bitexact(r.sample_counts(), ref.counts, f"{what}: counts")
    assert r.trace_faults() == 0, what


# ---- 5. the denoiser and the adaptive render ---------------------------------------------------------

@pytest.mark.parametrize("accel,size", [("grid_fast", (64, 48)), ("bvh", (37, 23))])
def test_denoise_of_a_direct_light_render(gpu, pt_mod, accel, size):
    P = pt_mod
    scene = fixture(P)[0]
    cfg = make_cfg(P, accel, width=size[0], height=size[1], pipelines=3)
    r = rendered(P, scene, cfg)
    try:
        S, Q = r.image(), r.moments()
        d, n, k = r.primary_hits()
        albedo = r.primary_albedo()
        for flags in (0, DAR.DEMODULATE, DAR.DEMODULATE | DAR.TILE_COUNTS):
            by_tile = bool(flags & DAR.TILE_COUNTS)
            img, var = r.denoise(variance=True, flags=flags)
            want_img, want_var = DAR.denoise(S, Q, size[0], size[1], None if by_tile else ITERS, d, n, k,
                                             albedo=albedo if flags & DAR.DEMODULATE else None,
                                             counts=r.sample_counts() if by_tile else None)
            assert_bitexact(img, want_img, f"{accel} {size} flags={flags}: image")
            assert_bitexact(var, want_var, f"{accel} {size} flags={flags}: variance")
            assert np.isfinite(img).all()
        assert r.trace_faults() == 0
    finally:
        r.free()
    ref = restated(P, cfg)
    assert_bitexact(S[~ref.near_tie_pixels], ref.S[~ref.near_tie_pixels], "the direct-light render")


def test_render_adaptive_of_a_direct_light_render(gpu, pt_mod):
    P = pt_mod
    scene, flat, spec = fixture(P)
    cfg = make_cfg(P, "grid_fast", pipelines=3, max_bounces=2)      # fewer shadow rays per pixel: fewer near ties
    kw = dict(max_iters=6, min_iters=2, check_every=2)
    first = restatement(P, flat, spec, cfg).render_adaptive(-1.0, 2, min_iters=2, check_every=2)
    e = np.sort(first["checks"][0][1].reshape(-1).astype(np.float64))
    g = int(np.argmax(np.diff(e)))
    target = 0.5 * (e[g] + e[g + 1])
    ref = restatement(P, flat, spec, cfg)
    want = ref.render_adaptive(target, **kw)
    margin = min(np.abs(t.astype(np.float64) - target).min() / target for _, t, _ in want["checks"])
    assert margin > 1e-4 and ref.near_tie_pixels.sum() <= PIXEL_TIES * W * H
    r = P.Renderer(cfg)
    r.enable_moments()
    r.set_direct_light()
    r.allocateOnGPU(scene)
    try:
        converged, iters, samples, mean = r.render_adaptive(target, **kw)
        assert (converged, iters, samples) == (want["converged"], want["iters"], want["pixel_samples"])
        assert samples < iters * W * H                    # a tile went off
        keep = ~ref.near_tie_pixels
        assert_bitexact(r.image()[keep], ref.S[keep], "render_adaptive: image")
        assert_bitexact(r.moments()[keep], ref.Q[keep], "render_adaptive: moments")
        assert_bitexact(r.sample_counts(), ref.counts, "render_adaptive: counts")
        if not ref.near_tie_pixels.any():
            assert abs(mean - want["mean"]) <= 1e-12 * want["mean"]
        assert r.trace_faults() == 0
    finally:
        r.free()
