"""Trace and compaction paths the scheduling tests never reach, each against
the CPU oracle bit for bit (image and segments, trace faults 0): the traversal
stack's global spill alone and across drain / walk hand-ons, grid_fast hit sets
beyond LDS, beyond one pool block and beyond the pool, block = 128 / 256 and the
fallback to 256, grids other than 25^3, the model-count variants as
allocateOnGPU picks them, pipelines 17..32, meshes without triangles, an
all-miss frame, an off-default camera and cfg.ray_sort.  Scenes and their CPU
preconditions: path_scenes.py / test_path_scenes.py."""
import numpy as np
import pytest

import path_scenes as S
from conftest import REF_SCENE
from helpers import assert_bitexact, flat_from_export

pytestmark = pytest.mark.gpu

_SCENES = {}


def _scene(key, make):
    """One build per scene and module run (the BLAS and grid builds are the slow part)."""
    if key not in _SCENES:
        _SCENES[key] = make()
    return _SCENES[key]


def _ref_scene(P, grid=(25, 25, 25)):
    def make():
        s = P.Scene(REF_SCENE)
        s.build(grid=grid, bvh=True)
        return s
    return _scene(("ref", tuple(grid)), make)


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _check_intersections(P, O, scene, o, d, accels, grid=(25, 25, 25), oracle_accel=0, min_hit=0.2):
    """intersect_rays for each accel == the oracle's (model, distance, normal of the hits)."""
    a = scene.export()
    ot, on, om = O.intersect_rays(flat_from_export(a, grid), o, d, accel=oracle_accel, threads=16)
    assert (om >= 0).mean() > min_hit, (om >= 0).mean()
    for accel in accels:
        r = P.Renderer(P.RenderConfig(width=8, height=8, accel=accel, grid=tuple(grid)))
        r.allocateOnGPU(scene)
        t, n, m = r.intersect_rays(o, d)
        r.free()
        assert_bitexact(m, om, f"model accel={accel}")
        assert_bitexact(t, ot, f"dist accel={accel}")
        assert_bitexact(n[om >= 0], on[om >= 0], f"normal accel={accel}")
    return om


# --- A. stack spill, alone and across hand-ons --------------------------------

@pytest.mark.parametrize("accel,pipes,env", [
    (1, 1, {}), (2, 1, {}),
    (1, 4, {}), (2, 4, {}),
    (1, 4, {"PT_DRAIN_DUMP": "64", "PT_DRAIN_LEVELS": "2", "PT_DRAIN_DUMP_TAIL": "64"}),
    (2, 4, {"PT_DRAIN_DUMP": "64", "PT_DRAIN_LEVELS": "2", "PT_DRAIN_DUMP_TAIL": "64"}),
    (2, 4, {"PT_WALK_WCAP": "7"}),
], ids=["bvh-p1", "gf-p1", "bvh-p4", "gf-p4", "bvh-drain2", "gf-drain2", "gf-wcap7"])
@pytest.mark.parametrize("variant", [0.0, S.STACK_TAPER, "dense"], ids=["equal", "tapered", "dense"])
def test_stack_spill_bit_identical(gpu, pt_mod, oracle_mod, monkeypatch, variant, accel, pipes, env):
    """The geometric stack (test_path_scenes: half the bounce rays emulate to 28
    stack entries or more, all to 16 or more): k_trace_bvh's 24 and k_trace_gf's 12
    LDS entries overflow into the global spill area, with one pipeline, with four,
    with every ray in flight at exhaustion handed on twice with its stack spilled
    (the tail lanes pop and push in the donors' areas), and with walk hand-ons and
    k_trace_deferred while spilled.  With equal quads at scale 0.01 no result
    depends on a spilled entry (they are farther siblings: a library whose spilled
    entries pop as a fixed leaf renders that scene unchanged).  The same library
    fails k_trace_gf's renders of the tapered stack and k_trace_bvh's renders of
    the dense one on MI355X, where rays find their hits among the popped entries."""
    P, O = pt_mod, oracle_mod
    _setenv(monkeypatch, env)
    s = _scene(("stack", variant), lambda: S.dense_stack_scene(P) if variant == "dense" else S.stack_scene(P, variant))
    cfg = P.RenderConfig(accel=accel, pipelines=pipes, **S.STACK_FRAME)
    S.check_render(P, O, ("stack", variant), s, cfg, what=f"{variant} accel={accel} pipes={pipes} {env}")


# --- B. hit sets beyond LDS, one pool block, the pool ---------------------------

def test_one_lane_hitset_beyond_a_pool_block(gpu, pt_mod, oracle_mod):
    """intersect_rays (the one-lane bvh4_traverse path): rays along a 100-plane
    comb's axis cross 100 triangles or more, beyond the 4 LDS + 64 pool members."""
    P, O = pt_mod, oracle_mod
    s = _scene("comb_pair", lambda: S.comb_pair_scene(P))
    o, d = S.comb_axis_rays(s.export(), 20000, 9)
    o2, d2 = S.random_rays(20000, 4)
    _check_intersections(P, O, s, np.concatenate([o, o2]), np.concatenate([d, d2]), (0, 2))


@pytest.mark.parametrize("pipes", [1, 4])
@pytest.mark.parametrize("pool", [None, "1"], ids=["pool-default", "pool-1"])
def test_persistent_hitset_overflow_exits(gpu, pt_mod, oracle_mod, monkeypatch, pool, pipes):
    """k_trace_gf on a camera looking along a DIFFUSE comb's axis: hit sets leave
    LDS for a 64-member pool block; with PT_HS_POOL_BLOCKS=1 the pool is exhausted
    and the rays go to k_trace_deferred (deferred_rays() > 0 is the precondition
    that the exit was taken: 194 on MI355X at pipelines 1 and 4).  With the default
    pool (65536 blocks, never exhausted by 3072 rays) deferred_rays() reports the
    "pool block full too" exit: 1 on MI355X with 100 planes at pipelines 1 and 4,
    so that exit is reached too, and asserted."""
    P, O = pt_mod, oracle_mod
    if pool:
        monkeypatch.setenv("PT_HS_POOL_BLOCKS", pool)
    s = _scene("comb_view", lambda: S.comb_view_scene(P))
    cfg = P.RenderConfig(width=64, height=48, iterations=2, max_bounces=5, accel=P.ACCEL_GRID_FAST, pipelines=pipes)
    deferred, _ = S.check_render(P, O, "comb_view", s, cfg, what=f"pool={pool} pipes={pipes}")
    print(f"comb 100 planes pool={pool or 'default'} pipelines={pipes}: deferred_rays={deferred}")
    assert deferred > 0


# --- C. block 128 / 256 ---------------------------------------------------------

@pytest.mark.parametrize("w,h", [(37, 23), (130, 2), (1, 1)])
@pytest.mark.parametrize("accel", [0, 1, 2])
@pytest.mark.parametrize("block", [128, 256])
def test_block_sizes_bit_identical(gpu, pt_mod, oracle_mod, block, accel, w, h):
    """k_bounce's cross-wave compaction, k_scan's chunks, slot_source and the sort
    kernels' chunk arithmetic at 128 and 256 lanes (130 x 2 = 260 pixels: two
    chunks of 256 with 4 live in the last, or three of 128)."""
    P, O = pt_mod, oracle_mod
    cfg = P.RenderConfig(width=w, height=h, iterations=2, accel=accel, block=block)
    S.check_render(P, O, "ref", _ref_scene(P), cfg, what=f"block={block} accel={accel} {w}x{h}")


@pytest.mark.parametrize("block", [128, 256])
@pytest.mark.parametrize("accel,kw,env", [
    (2, dict(width=300, height=3, tail_drop=1), {}),
    (1, dict(width=300, height=3, tail_drop=1), {}),
    (2, dict(width=80, height=64), {"PT_GF_SPLIT": "0"}),
    (1, dict(width=80, height=64), {"PT_TRACE_SPLIT": "0"}),
    (2, dict(width=80, height=64, iterations=4, pipelines=3), {}),
    (2, dict(width=80, height=64), {"PT_GRAPH": "1"}),
], ids=["gf-taildrop", "bvh-taildrop", "gf-fused", "bvh-fused", "gf-p3-it4", "gf-graph"])
def test_block_sizes_with_other_paths(gpu, pt_mod, oracle_mod, monkeypatch, block, accel, kw, env):
    P, O = pt_mod, oracle_mod
    _setenv(monkeypatch, env)
    cfg = P.RenderConfig(**{**dict(iterations=2, accel=accel, block=block), **kw})
    S.check_render(P, O, "ref", _ref_scene(P), cfg, what=f"block={block} {kw} {env}")


@pytest.mark.parametrize("accel", [0, 1, 2])
@pytest.mark.parametrize("block", [0, 96])
def test_other_block_values_fall_back_to_256(gpu, pt_mod, oracle_mod, block, accel):
    """pt_render_config.block: any value but 64, 128 and 256 renders as 256."""
    P, O = pt_mod, oracle_mod
    s = _ref_scene(P)
    imgs = []
    for b in (256, block):
        cfg = P.RenderConfig(width=130, height=7, iterations=2, accel=accel, block=b)
        img, seg, _, _ = S.render_gpu(P, s, cfg)
        oimg, oseg = S.oracle_render(O, "ref", s, cfg)
        assert seg == oseg
        assert_bitexact(img, oimg, f"block={b}")
        imgs.append(img)
    assert_bitexact(imgs[1], imgs[0], f"block={block} vs 256")


# --- D. grids other than 25^3 ---------------------------------------------------

@pytest.mark.parametrize("transformed", [False, True], ids=["identity", "transformed"])
@pytest.mark.parametrize("grid", S.GRIDS, ids=str)
def test_grids_boundary_and_interior_rays(gpu, pt_mod, oracle_mod, grid, transformed):
    """grid and grid_fast == the reference grid at that gdim on rays that start,
    pass and end on voxel boundaries 0..grid[k] of the torus' and the room's grids
    (identity transforms, and rotation + anisotropic scale + translation) and on
    bounce-like interior rays."""
    P, O = pt_mod, oracle_mod
    s = _scene(("boundary", grid, transformed), lambda: S.boundary_scene(P, grid, transformed))
    a = s.export()
    o, d = S.boundary_rays(a, 20000, 5, grid)
    o2, d2 = S.interior_rays(a, 20000, 6)
    _check_intersections(P, O, s, np.concatenate([o, o2]), np.concatenate([d, d2]), (0, 2), grid=grid, min_hit=0.3)


@pytest.mark.parametrize("transformed", [False, True], ids=["identity", "transformed"])
@pytest.mark.parametrize("grid", S.GRIDS, ids=str)
def test_grids_walk_certificates(gpu, pt_mod, grid, transformed):
    """Both walk certificates agree with the exact walk wherever they accept, at
    every voxel width (cslack, wdelta, reach, the 10-bit voxel boxes).  No
    acceptance floor: a 1^3 grid has nothing to skip."""
    P = pt_mod
    s = _scene(("boundary", grid, transformed), lambda: S.boundary_scene(P, grid, transformed))
    a = s.export()
    r = P.Renderer(P.RenderConfig(width=8, height=8, accel=P.ACCEL_GRID_FAST, grid=grid))
    r.allocateOnGPU(s)
    try:
        for name, (o, d) in (("boundary", S.boundary_rays(a, 20000, 11, grid)), ("interior", S.interior_rays(a, 20000, 12))):
            tried, ok, fast_bad, full_bad = (int(v) for v in r.certify_check(o, d).sum(0))
            print(f"certify grid={grid} transformed={transformed} {name}: tried={tried} accepted={ok}")
            assert fast_bad == 0 and full_bad == 0 and tried > 0, \
                f"{name}: tried {tried} accepted {ok} fast_bad {fast_bad} full_bad {full_bad}"
    finally:
        r.free()


@pytest.mark.parametrize("accel", [0, 2])
@pytest.mark.parametrize("grid", S.GRIDS, ids=str)
def test_grids_render_reference_scene(gpu, pt_mod, oracle_mod, grid, accel):
    P, O = pt_mod, oracle_mod
    cfg = P.RenderConfig(width=64, height=48, iterations=2, max_bounces=5, accel=accel, grid=grid, pipelines=4)
    S.check_render(P, O, "ref", _ref_scene(P, grid), cfg, grid=grid, what=f"grid={grid} accel={accel}")


# --- E. model-count boundaries ----------------------------------------------------

@pytest.mark.parametrize("pipes", [1, 4])
@pytest.mark.parametrize("accel", [1, 2])
@pytest.mark.parametrize("k", S.MODEL_COUNTS)
def test_model_count_variants(gpu, pt_mod, oracle_mod, k, accel, pipes):
    """8 models (records in LDS), 9 and 12 (the wide LDS table), 13 and 33 (global
    memory): the variant allocateOnGPU picks by itself, no env override."""
    P, O = pt_mod, oracle_mod
    s = _scene(("models", k), lambda: S.scene_from_spec(P, *S.model_count_spec(k)))
    assert s.counts()["nmodel"] == k
    cfg = P.RenderConfig(width=64, height=48, iterations=2, max_bounces=6, accel=accel, pipelines=pipes)
    S.check_render(P, O, ("models", k), s, cfg, what=f"k={k} accel={accel} pipes={pipes}")


# --- F. pipelines beyond 16 ---------------------------------------------------------

@pytest.fixture(scope="module")
def pipes_scene(pt_mod, tmp_path_factory):
    from pathtracerap_amd import synthetic
    s = pt_mod.Scene(synthetic.diffuse_scene(str(tmp_path_factory.mktemp("paths")), ntri=3000, seed=5))
    s.build(bvh=True)
    return s


@pytest.mark.parametrize("accel", [1, 2])
@pytest.mark.parametrize("pipes,loops", [(17, [(0, 20), (20, 17)]), (32, [(0, 20), (20, 17)]), (32, [(0, 3)])],
                         ids=["p17-it37", "p32-it37", "p32-it3"])
def test_pipelines_beyond_16(gpu, pt_mod, oracle_mod, pipes_scene, accel, pipes, loops):
    """17 and 32 iterations in flight over 37 iterations in two calls (the
    pipelines wrap, some stay unused in the second call, the join crosses the
    calls), and 32 pipelines for 3 iterations."""
    P, O = pt_mod, oracle_mod
    its = sum(n for _, n in loops)
    cfg = P.RenderConfig(width=72, height=56, iterations=its, max_bounces=6, accel=accel, pipelines=pipes)
    _, got = S.check_render(P, O, "pipes", pipes_scene, cfg, loops=loops, what=f"pipelines={pipes} accel={accel}")
    assert got == pipes


# --- G. empty and minimal meshes, all-miss frame, camera, cfg.ray_sort -------------------

@pytest.mark.parametrize("accel", [0, 1, 2])
@pytest.mark.parametrize("where,vertices", [("first", True), ("middle", True), ("last", True), ("middle", False)],
                         ids=["first", "middle", "last", "middle-novertex"])
def test_empty_mesh_model(gpu, pt_mod, oracle_mod, where, vertices, accel):
    """A model whose mesh has no triangles (skipped at select: 4-wide root -1)
    first, in the middle and last in model order, beside a 1-triangle instance
    and a mesh with a zero-area triangle."""
    P, O = pt_mod, oracle_mod
    key = ("empty", where, vertices)
    s = _scene(key, lambda: S.scene_from_spec(P, *S.empty_mesh_spec(where, vertices)[:2]))
    for pipes in (1, 4):
        cfg = P.RenderConfig(width=64, height=48, iterations=2, accel=accel, pipelines=pipes)
        S.check_render(P, O, key, s, cfg, what=f"{where} accel={accel} pipes={pipes}")


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_intersect_rays_never_reports_the_empty_model(gpu, pt_mod, oracle_mod, where):
    P, O = pt_mod, oracle_mod
    at = S.empty_mesh_spec(where)[2]
    s = _scene(("empty", where, True), lambda: S.scene_from_spec(P, *S.empty_mesh_spec(where)[:2]))
    o, d = S.random_rays(20000, 8, center=(0.0, 200.0, 0.0), spread=450.0)
    o[:2000] = np.float32([50, 100, 600])                      # towards the empty model's place
    d[:2000] = np.float32([50, 100, 100]) - o[:2000] + np.random.RandomState(2).normal(size=(2000, 3)).astype(np.float32) * 40
    for oracle_accel, accels in ((0, (0, 2)), (1, (1,))):
        om = _check_intersections(P, O, s, o, d, accels, oracle_accel=oracle_accel)
        assert not (om == at).any()


@pytest.mark.parametrize("accel", [0, 1, 2])
@pytest.mark.parametrize("pipes", [1, 4])
def test_all_rays_miss(gpu, pt_mod, oracle_mod, pipes, accel):
    """The camera looks away from the scene: no live ray after bounce 0, so the
    persistent traces are launched over nothing."""
    P, O = pt_mod, oracle_mod
    s = _scene(("empty", "middle", True), lambda: S.scene_from_spec(P, *S.empty_mesh_spec("middle")[:2]))
    cfg = P.RenderConfig(width=64, height=48, iterations=2, accel=accel, pipelines=pipes,
                         cam=(0.0, 0.0, 2000.0), plane_z=2020.0)
    S.check_render(P, O, ("empty", "middle", True), s, cfg, what=f"all miss accel={accel}")
    _, oseg = S.oracle_render(O, ("empty", "middle", True), s, cfg)
    assert oseg == 64 * 48 * 2                                   # the precondition: one segment per primary ray


@pytest.mark.parametrize("accel", [2, 1])
def test_off_default_camera(gpu, pt_mod, oracle_mod, accel):
    P, O = pt_mod, oracle_mod
    cfg = P.RenderConfig(width=64, height=48, iterations=2, accel=accel, cam=(300.0, 250.0, 700.0), plane_z=690.0,
                         plane_x0=290.0, plane_y0=244.0, plane_w=20.0, plane_h=15.0)
    S.check_render(P, O, "ref", _ref_scene(P), cfg, what=f"camera accel={accel}")
    oimg, _ = S.oracle_render(O, "ref", _ref_scene(P), cfg)
    assert oimg.any()


@pytest.mark.parametrize("accel", [1, 2])
@pytest.mark.parametrize("sort", [0, 3])
def test_config_ray_sort(gpu, pt_mod, oracle_mod, sort, accel):
    """cfg.ray_sort set in the config (not through PT_SORT): off, and key layout 3."""
    P, O = pt_mod, oracle_mod
    cfg = P.RenderConfig(width=64, height=48, iterations=2, accel=accel, ray_sort=sort)
    S.check_render(P, O, "ref", _ref_scene(P), cfg, what=f"ray_sort={sort} accel={accel}")
