"""The slot-to-source map (k_sort_scatter writes KParams::slot_src, the shading pass of
the same bounce reads its ray's pool index from it) and the sort keys stored by the
kernels that write the rays.  Every case renders with PT_SLOT_MAP=1 and PT_SLOT_MAP=0
(read at allocateOnGPU): both images bit-equal to the CPU yardstick (the oracle, or its
restatements for masked and jittered iterations) and byte-equal to each other, equal
segments per bounce, trace_faults() == 0.  Frames are the smallest that reach each path."""
import numpy as np
import pytest

import adaptive_ref as AR
import jitter_ref as JR
import path_scenes as S
from conftest import REF_SCENE
from helpers import assert_bitexact, flat_from_export, oracle_cfg
from slot_map_cases import SPARSE_FRAME, SPARSE_KEY, sparse_condition, sparse_scene

pytestmark = pytest.mark.gpu

ACCELS = [2, 1]
ACCEL_IDS = ["grid_fast", "bvh"]
SWITCH = ("1", "0")


def _ref_scene(P):
    def make():
        s = P.Scene(REF_SCENE)
        s.build(bvh=True)
        return s
    return S.scene_once("ref", make)          # path_scenes' own reference scene: the same build


def _render(P, scene, cfg, loops=None, setup=None, run=None):
    """(image, segments, segments per bounce) of one renderer; `setup(r)` before
    allocateOnGPU, `run(r)` instead of the renderLoop calls."""
    r = P.Renderer(cfg)
    try:
        if setup:
            setup(r)
        r.allocateOnGPU(scene)
        if run:
            run(r)
        else:
            for first, n in (loops or [(0, cfg.iterations)]):
                r.renderLoop(first, n)
        assert r.trace_faults() == 0
        return r.image(), r.segments(), r.segments_per_bounce(16)
    finally:
        r.free()


def _both(monkeypatch, render, want_img, want_seg, what):
    """render() under PT_SLOT_MAP=1 and =0: each the yardstick's image and segments,
    the two byte-equal with equal segments per bounce; returns the per-bounce counts."""
    got = {}
    for sw in SWITCH:
        monkeypatch.setenv("PT_SLOT_MAP", sw)
        img, seg, per = render()
        assert seg == want_seg, (what, sw, seg, want_seg)
        assert_bitexact(img, want_img, f"{what} PT_SLOT_MAP={sw}: image")
        got[sw] = (img, per)
    assert got["1"][0].tobytes() == got["0"][0].tobytes(), what
    assert got["1"][1] == got["0"][1], (what, got["1"][1], got["0"][1])
    return got["1"][1]


def _oracle_both(P, O, monkeypatch, key, scene, cfg, what, loops=None):
    oimg, oseg = S.oracle_render(O, key, scene, cfg)
    per = _both(monkeypatch, lambda: _render(P, scene, cfg, loops), oimg, oseg, what)
    assert sum(per) == oseg, (what, per, oseg)
    return per


# ---- two sort workgroups, the second partial; one partial chunk ------------------------------

@pytest.mark.parametrize("pipes", [1, 3])
@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
def test_two_sort_workgroups(gpu, pt_mod, oracle_mod, monkeypatch, accel, pipes):
    """96 x 64 = 6144 pixels, 96 chunks: a sort workgroup covers 4096 source indices, so
    bounce 1's sort runs a full and a partial workgroup; bounce 2 reads the map again."""
    P = pt_mod
    cfg = P.RenderConfig(width=96, height=64, iterations=2, accel=accel, pipelines=pipes)
    per = _oracle_both(P, oracle_mod, monkeypatch, "ref", _ref_scene(P), cfg, f"96x64 accel={accel} p{pipes}")
    assert per[1] > 0 and per[2] > 0


@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
def test_one_partial_chunk(gpu, pt_mod, oracle_mod, monkeypatch, accel):
    P = pt_mod
    cfg = P.RenderConfig(width=7, height=5, iterations=2, accel=accel, pipelines=1)
    _oracle_both(P, oracle_mod, monkeypatch, "ref", _ref_scene(P), cfg, f"7x5 accel={accel}")


# ---- many empty and partly filled chunks -------------------------------------------------------

@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
def test_sparse_compaction(gpu, pt_mod, oracle_mod, monkeypatch, accel):
    """Most camera rays miss (test_slot_map_scene.py: the oracle alone says so), so bounce
    1's survivors are spread thinly over the chunks and bounce 2 reads the map after a
    sparse compaction."""
    P = pt_mod
    cfg = P.RenderConfig(accel=accel, pipelines=3, **SPARSE_FRAME)
    per = _oracle_both(P, oracle_mod, monkeypatch, SPARSE_KEY, sparse_scene(P), cfg, f"sparse accel={accel}")
    sparse_condition(per, cfg)


# ---- jittered iterations: bounce 1 is traced unsorted by default ----------------------------------

_JITTER_REF = {}


def _jitter_ref(P, scene, cfg):
    o = oracle_cfg(cfg, threads=4)
    if o.accel not in _JITTER_REF:
        ref = JR.Restatement(flat_from_export(scene.export()), o, width=1.0)
        ref.render(0, 3)
        _JITTER_REF[o.accel] = ref
    return _JITTER_REF[o.accel]


@pytest.mark.parametrize("pipes", [1, 3])
@pytest.mark.parametrize("jitter_sort", [None, "1"], ids=["unsorted-b1", "sorted-b1"])
@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
def test_jittered_iterations(gpu, pt_mod, monkeypatch, accel, jitter_sort, pipes):
    """Three iterations: with one pipeline each starts with the map the previous one's
    last bounce left, which bounce 1 must not read when its trace ran unsorted."""
    P = pt_mod
    if jitter_sort:
        monkeypatch.setenv("PT_JITTER_SORT", jitter_sort)
    cfg = P.RenderConfig(width=64, height=48, iterations=3, accel=accel, pipelines=pipes)
    scene = _ref_scene(P)
    ref = _jitter_ref(P, scene, cfg)
    per = _both(monkeypatch, lambda: _render(P, scene, cfg, setup=lambda r: r.set_pixel_jitter(1.0)),
                ref.S, ref.segments, f"jitter accel={accel} sort={jitter_sort} p{pipes}")
    assert per[:10] == ref.per_bounce[:10].tolist()


# ---- masked iterations ----------------------------------------------------------------------------

def test_masked_checkerboard(gpu, pt_mod, monkeypatch):
    P = pt_mod
    W, H = 64, 48
    cfg = P.RenderConfig(width=W, height=H, iterations=3, accel=P.ACCEL_GRID_FAST, pipelines=3)
    ty, tx = AR.tiles_shape(W, H)
    mask = (np.add.outer(np.arange(ty), np.arange(tx)) % 2 == 0)
    assert mask.any() and not mask.all()
    scene = _ref_scene(P)
    ref = AR.Restatement(flat_from_export(scene.export()), oracle_cfg(cfg, threads=4))
    ref.render(0, 3, mask)
    _both(monkeypatch, lambda: _render(P, scene, cfg, setup=lambda r: r.enable_moments(),
                                       run=lambda r: r.render_masked(mask, 0, 3)),
          ref.S, ref.segments, "checkerboard")


# ---- graph replay ---------------------------------------------------------------------------------

def test_graph_replay(gpu, pt_mod, oracle_mod, monkeypatch):
    P = pt_mod
    monkeypatch.setenv("PT_GRAPH", "1")
    cfg = P.RenderConfig(width=64, height=48, iterations=8, accel=P.ACCEL_GRID_FAST, pipelines=3)
    _oracle_both(P, oracle_mod, monkeypatch, "ref", _ref_scene(P), cfg, "graph", loops=[(0, 4), (4, 4)])


# ---- no sort, one bounce: the fallback search -----------------------------------------------------

@pytest.mark.parametrize("bounces", [1, 2])
@pytest.mark.parametrize("sort", ["0", None], ids=["nosort", "sort"])
@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
def test_no_sort_and_one_bounce(gpu, pt_mod, oracle_mod, monkeypatch, accel, sort, bounces):
    P = pt_mod
    if sort:
        monkeypatch.setenv("PT_SORT", sort)
    cfg = P.RenderConfig(width=64, height=48, iterations=2, max_bounces=bounces, accel=accel, pipelines=1)
    _oracle_both(P, oracle_mod, monkeypatch, "ref", _ref_scene(P), cfg, f"accel={accel} PT_SORT={sort} b{bounces}")


# ---- sort keys stored by the kernels that write the rays -------------------------------------------

@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
def test_trace_rays_after_a_render(gpu, pt_mod, oracle_mod, accel):
    """trace_rays uploads its rays: the keys the render's kernels left belong to other
    rays, so its sort computes them; and the render after it is the render before it."""
    P, O = pt_mod, oracle_mod
    s, grid, o, d, _ = S.ray_set(P, "ref")
    r = P.Renderer(P.RenderConfig(width=256, height=160, iterations=2, accel=accel, pipelines=4))
    try:
        r.allocateOnGPU(s)
        r.renderLoop(0, 2)
        first = r.image()
        S.check_rays(r, s, o, d, S.ray_set_oracle(P, O, "ref", accel), what=f"after a render, accel={accel}")
        r.clearImage()
        r.renderLoop(0, 2)
        assert r.trace_faults() == 0
        assert first.any()
        assert_bitexact(r.image(), first, "the render after trace_rays")
    finally:
        r.free()
