"""The kernels against the reference's own code (GPU).

What test_reference_code.py asserts of the CPU oracle is asserted here of the HIP
kernels directly, against oracle/_ref/libptref.so (the reference's text compiled
for the host, see oracle/ref/bridge.cpp) or its recordings under
tests/golden/reference_code/ -- never against the oracle's restatement:
pt_renderer_intersect_rays under PT_ACCEL_GRID and PT_ACCEL_GRID_FAST, the
persistent trace kernels through pt_renderer_trace_rays, and whole renders.
Every ray and every pixel is compared; nothing is left out (the intersection
difference the reference's default build shows is that build's, see
test_reference_code.py)."""
import numpy as np
import pytest

import path_scenes as S
import reference_code_cases as C
from helpers import assert_bitexact
from oracle import reference_code as R

pytestmark = pytest.mark.gpu

needs_library = pytest.mark.skipif(not R.available(), reason=f"{R.LIB_PATH} is not built (no reference tree at build time) "
                                                              "and this check has no recording")
GRID_ACCELS = [0, 2]                # PT_ACCEL_GRID, PT_ACCEL_GRID_FAST


def _scene(P, name):
    if name == "ref":
        return S._ref_scene(P)
    return S.scene_once(("reference_code", name), lambda: S.scene_from_spec(P, *C.spec_of(name)))


def _renderer(P, scene, accel, width=256, height=160, **kw):
    r = P.Renderer(P.RenderConfig(width=width, height=height, iterations=2, accel=accel, **kw))
    r.allocateOnGPU(scene)
    return r


def _types(scene, model):
    """Material type per hit model (-1 for a miss): what the reference's hit record carries."""
    mi = scene.export()["model_ints"]
    return np.where(model >= 0, mi[np.maximum(model, 0), 2], -1).astype(np.int32)


def _check_hits(scene, got, ref, what):
    t, n, m = got
    rd, rn, rt = ref
    assert_bitexact(_types(scene, m), rt, f"material {what}")
    assert_bitexact(t, rd, f"distance {what}")
    hit = m >= 0
    assert_bitexact(n[hit], rn[hit], f"normal {what}")


def _big_batch():
    """25,000 camera and 25,000 secondary rays of the reference scene and the reference's hits."""
    def make():
        os_, ds, ref = [], [], []
        for name, seed in (("camera", 51), ("secondary", 52)):
            _, o, d = C.batch(name, full=True)
            idx = C.subset(len(o), seed, 25000)
            full = C.reference_hits_full(name)
            os_.append(o[idx]); ds.append(d[idx]); ref.append(tuple(v[idx] for v in full))
        return (np.ascontiguousarray(np.concatenate(os_)), np.ascontiguousarray(np.concatenate(ds)),
                tuple(np.concatenate([r[k] for r in ref]) for k in range(3)))
    return C.once("gpu_big_batch", make)


@pytest.mark.parametrize("accel", GRID_ACCELS)
@pytest.mark.parametrize("name", list(C.BATCHES) + C.DEGENERATE)
def test_intersect_rays_recorded_batches(gpu, pt_mod, name, accel):
    """pt_renderer_intersect_rays == computeRaySceneIntersectionKernel on the recorded batches."""
    P = pt_mod
    sc, o, d = C.batch(name, full=False)
    rd, rn, rt, src = C.reference_hits(name)
    s = _scene(P, sc)
    r = _renderer(P, s, accel)
    try:
        _check_hits(s, r.intersect_rays(o, d), (rd, rn, rt), f"{name} accel={accel} ({src})")
    finally:
        r.free()


@needs_library
@pytest.mark.parametrize("accel", GRID_ACCELS)
def test_intersect_rays_50000(gpu, pt_mod, accel):
    P = pt_mod
    o, d, ref = _big_batch()
    s = _scene(P, "ref")
    r = _renderer(P, s, accel, width=320, height=200)
    try:
        _check_hits(s, r.intersect_rays(o, d), ref, f"50,000 rays accel={accel}")
    finally:
        r.free()


def _check_trace(P, scene, o, d, ref, width, height, what):
    """trace_rays under PT_ACCEL_GRID_FAST, dense and in a random sparse block layout."""
    r = _renderer(P, scene, 2, width=width, height=height)
    try:
        lay = S.layouts(width * height, r.cfg.block, len(o), 7)
        for layout in ("dense", "random"):
            t, n, m, tri = r.trace_rays(o, d, None if layout == "dense" else lay[layout])
            assert r.trace_faults() == 0, (what, layout)
            _check_hits(scene, (t, n, m), ref, f"{what} {layout}")
            a = scene.export()
            hit = m >= 0
            rng = a["mesh_ranges"][a["model_ints"][m[hit], 0]]
            assert ((tri[hit] >= rng[:, 2]) & (tri[hit] < rng[:, 3])).all(), f"triangle outside the hit model's mesh {what}"
    finally:
        r.free()


@pytest.mark.parametrize("name", list(C.BATCHES) + C.DEGENERATE)
def test_trace_rays_recorded_batches(gpu, pt_mod, name):
    """The persistent trace kernels == the reference's code, not a restatement of it."""
    P = pt_mod
    sc, o, d = C.batch(name, full=False)
    rd, rn, rt, src = C.reference_hits(name)
    _check_trace(P, _scene(P, sc), o, d, (rd, rn, rt), 256, 160, f"{name} ({src})")


@needs_library
def test_trace_rays_50000(gpu, pt_mod):
    P = pt_mod
    o, d, ref = _big_batch()
    _check_trace(P, _scene(P, "ref"), o, d, ref, 320, 200, "50,000 rays")


@pytest.mark.parametrize("block", [64, 256])
@pytest.mark.parametrize("pipes", [1, 16])
@pytest.mark.parametrize("accel", GRID_ACCELS)
@pytest.mark.parametrize("case", C.RENDERS, ids=C.render_id)
def test_render(gpu, pt_mod, case, accel, pipes, block):
    """Image, rays per bounce and trace_faults() == 0 against the reference's kernels run
    in renderLoop's order."""
    P = pt_mod
    sc, w, h, td = case
    img, live, src = C.reference_render(case)
    s = _scene(P, sc)
    cfg = P.RenderConfig(width=w, height=h, iterations=C.RENDER_ITERS, max_bounces=C.MAX_BOUNCES, accel=accel,
                         tail_drop=td, pipelines=pipes, block=block)
    r = P.Renderer(cfg)
    try:
        r.allocateOnGPU(s)
        r.renderLoop()
        assert r.trace_faults() == 0
        got = r.image()
        per_bounce = r.segments_per_bounce(len(live))
        seg = r.segments()
    finally:
        r.free()
    what = f"{C.render_id(case)} accel={accel} pipes={pipes} block={block} ({src})"
    assert list(per_bounce) == live.tolist(), (what, per_bounce, live)
    assert seg == int(live.sum()), what
    assert_bitexact(got, img, f"image {what}")
