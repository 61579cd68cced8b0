"""CPU preconditions of test_gpu_paths.py and test_gpu_trace_rays.py: the scenes
of path_scenes.py reach the paths they are built for (emulated traversal
depths, the oracle's segment floor), scenes with empty meshes build exactly as
the oracle builds them, and the ray sets, scaled directions and survivor
layouts of the trace_rays tests are what those tests take them for."""
import numpy as np
import pytest

import path_scenes as S
from helpers import assert_bitexact, flat_from_export, oracle_cfg

KEYS = ["vpos", "vnrm", "tris", "mesh_ranges", "mesh_bbox", "model_ints", "model_m2w", "model_w2m",
        "model_color", "grid_ints", "grid_vw", "vox", "per_voxel"]


def _compare(a, o):
    for k in KEYS:
        assert_bitexact(a[k], getattr(o, k), k)


def _one_quad_pair_b4(P):
    """Two far-apart quads: a root with two leaf slots."""
    s = P.Scene()
    m = s.addMesh(*S._quads(np.array([0.0, 5.0]), 1.0))
    s.addModel(m, (1, 1, 1), (0, 0, 0), (0, 0, 0), "DIFFUSE", (0.5, 0.5, 0.5))
    s.build(bvh=True)
    return s.export_bvh4()


def test_emulator_counts_pushed_siblings(pt_mod):
    """A ray through both leaves of a two-leaf root pushes one sibling; a ray
    through one leaf, or through none, pushes nothing."""
    b4 = _one_quad_pair_b4(pt_mod)
    ints = b4["nodes"].view(np.int32)
    assert (ints[b4["roots"][0], 28:32] > 0).sum() == 2          # the shape this check assumes
    assert S.emulate_stack_depth(b4, 0, (100.0, 200.0, -500.0), (0.0, 0.0, 1.0)) == 1
    assert S.emulate_stack_depth(b4, 0, (100.0, 200.0, 2500.0), (0.0, 0.0, 1.0)) == 0
    assert S.emulate_stack_depth(b4, 0, (5000.0, 200.0, -500.0), (0.0, 0.0, 1.0)) == 0


@pytest.mark.parametrize("taper", [0.0, S.STACK_TAPER], ids=["equal", "tapered"])
def test_geometric_stack_spills_both_traces(pt_mod, taper):
    """256 seeded cosine-weighted rays from a point on the first plane: at least
    half emulate to kStack + 4 = 28 entries (k_trace_bvh spills), all to
    kGfStack + 4 = 16 (k_trace_gf spills).  Conditions on the scene, not
    tolerances: if a builder change breaks them, change the scene."""
    d = S.stack_depths(pt_mod, taper=taper)
    assert len(d) == 256
    assert (d >= 28).mean() >= 0.5, (np.median(d), (d >= 28).mean())
    assert d.min() >= 16, d.min()
    # and the spill area holds them: kStack / kGfStack + kSpillEntries (64)
    assert d.max() <= 12 + 64


@pytest.mark.parametrize("accel", [1, 2])
def test_stack_scene_bounces_through_the_stack(pt_mod, oracle_mod, accel):
    """The oracle's render of the GPU test's configuration counts at least
    3 W H iterations segments at max_bounces = 4: most paths bounce on through
    the stack (the normals point away from the camera), and some leave it (the
    image is not uniform, so it tells paths apart)."""
    P, O = pt_mod, oracle_mod
    s = S.stack_scene(P)
    cfg = P.RenderConfig(accel=accel, **S.STACK_FRAME)
    img, seg = S.oracle_render(O, ("stack", 0.0), s, cfg)
    assert seg >= 3 * cfg.width * cfg.height * cfg.iterations, seg
    assert len(np.unique(img, axis=0)) >= 8


@pytest.mark.parametrize("variant", [S.STACK_TAPER, "dense"], ids=["tapered", "dense"])
@pytest.mark.parametrize("accel", [1, 2])
def test_stack_variants_bounce(pt_mod, oracle_mod, accel, variant):
    """The tapered variant shows its small near quads to fewer pixels, and the
    dense one ends half its paths at each bounce (the interleaved emissive
    planes): the floor here is 2 W H iterations segments (on average every path
    traces a bounce ray), and the image is not uniform."""
    P, O = pt_mod, oracle_mod
    s = S.dense_stack_scene(P) if variant == "dense" else S.stack_scene(P, variant)
    cfg = P.RenderConfig(accel=accel, **S.STACK_FRAME)
    img, seg = S.oracle_render(O, ("stack", variant), s, cfg)
    assert seg >= 2 * cfg.width * cfg.height * cfg.iterations, seg
    assert len(np.unique(img, axis=0)) >= 8


@pytest.mark.parametrize("vertices", [True, False])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_empty_mesh_scene_builds_as_the_oracle(pt_mod, oracle_mod, where, vertices):
    """A mesh without triangles (with or without vertices) instanced once: every
    exported vector equals oracle.build_scene's, the mesh's 4-wide root is -1
    (the traces skip the model at select) while every other mesh has one, and
    the oracle renders the scene."""
    P, O = pt_mod, oracle_mod
    meshes, models, at = S.empty_mesh_spec(where, vertices)
    s = S.scene_from_spec(P, meshes, models)
    a = s.export()
    _compare(a, S.oracle_scene_from_spec(O, meshes, models))
    assert a["model_ints"][at, 0] == 2
    roots = s.export_bvh4()["roots"]
    assert roots[2] == -1 and (np.delete(roots, 2) >= 0).all(), roots
    cfg = P.RenderConfig(width=16, height=12, iterations=1, accel=1)
    for accel in (0, 1):
        cfg.accel = accel
        img, seg = O.render(flat_from_export(a), oracle_cfg(cfg))
        assert seg >= 16 * 12 and np.isfinite(img).all()


@pytest.mark.parametrize("k", S.MODEL_COUNTS)
def test_model_count_scene_builds_as_the_oracle(pt_mod, oracle_mod, k):
    meshes, models = S.model_count_spec(k)
    s = S.scene_from_spec(pt_mod, meshes, models)
    assert s.counts()["nmodel"] == k
    assert {m["material"] for m in models} >= {"DIFFUSE", "EMISSIVE"}
    _compare(s.export(), S.oracle_scene_from_spec(oracle_mod, meshes, models))


# --- ray batches and survivor layouts of test_gpu_trace_rays.py -------------------

@pytest.mark.parametrize("accel", [0, 1], ids=["grid", "bvh"])
@pytest.mark.parametrize("name", S.RAY_SET_NAMES)
def test_ray_sets_hit_share(pt_mod, oracle_mod, name, accel):
    """Each ray set of the trace_rays tests hits on more than the share the
    one-lane tests ask of the same generators (0.3 reference and boundary scenes,
    0.2 elsewhere), on the reference grid and on the exact closest hit; the
    oracle's result is the one the GPU tests compare with."""
    _, _, o, d, floor = S.ray_set(pt_mod, name)
    assert 20000 <= len(o) <= 40000
    t, n, m = S.ray_set_oracle(pt_mod, oracle_mod, name, accel)
    share = (m >= 0).mean()
    print(f"ray set {name} oracle accel={accel}: {len(o)} rays, hit share {share:.4f}")
    assert share > floor, share


@pytest.mark.parametrize("variant", ["tapered", "dense"])
def test_stack_rays_spill(pt_mod, variant):
    """stack_rays: origins on the first planes inside the quads' footprint; of
    the first 256, at least half emulate to kStack + 4 = 28 entries
    (k_trace_bvh spills; k_trace_gf's 12 overflow before that), none beyond the
    spill area, and most origins lie outside the tapered stack's near quads."""
    P = pt_mod
    s, _, o, d, _ = S.ray_set(P, f"stack-{variant}")
    om, dm = S._stack_rays_mesh(len(o), 21)
    assert_bitexact(S.to_world(s.export(), 0, om).astype(np.float32), o, "origins")
    assert (np.abs(om[:, :2]) <= 20000.0).all() and (np.abs(om[:, :2]).max(1) > 2000.0).mean() > 0.5
    assert (om[:, 2] >= 1.0).all() and (om[:, 2] <= S.STACK_R ** 8).all()
    b4 = s.export_bvh4()
    depth = np.array([S.emulate_stack_depth(b4, 0, om[i], dm[i]) for i in range(256)])
    print(f"stack_rays {variant}: depth median {np.median(depth)}, min {depth.min()}, max {depth.max()}")
    assert (depth >= 28).mean() >= 0.5, (np.median(depth), (depth >= 28).mean())
    assert depth.max() <= 12 + 64


@pytest.mark.parametrize("accel", [0, 1], ids=["grid", "bvh"])
def test_scaled_directions_keep_the_oracle_result(pt_mod, oracle_mod, accel):
    """20 000 rays from inside the reference room with their directions scaled
    (scaled(): powers of two, reflect_ref's |1 - 2c|, 1e-6..1e-3, 1e-6..1e6): more
    than half hit at every scaling, and a power-of-two factor leaves the oracle's
    distance bit-identical and the model identical for every ray (both normalise
    the direction first; a power of two scales it exactly).  The other kinds
    round differently: the share of rays whose model changes and the largest
    relative distance change are printed, not asserted."""
    P, O = pt_mod, oracle_mod
    s = S._ref_scene(P)
    o, d = S.room_interior_rays(s.export(), 20000, 31)
    t0, _, m0 = S.oracle_hits(O, "scaled-none", s, o, d, accel)
    assert (m0 >= 0).mean() > 0.5
    for i, kind in enumerate(S.SCALINGS):
        dk = S.scaled(d, kind, 40 + i)
        assert not np.array_equal(dk, d)
        t, _, m = S.oracle_hits(O, f"scaled-{kind}", s, o, dk, accel)
        share = (m >= 0).mean()
        both = (m >= 0) & (m0 >= 0)
        rel = np.abs(t[both].astype(np.float64) - t0[both]) / t0[both]
        print(f"scaled {kind} oracle accel={accel}: hit share {share:.4f}, model differs on {(m != m0).sum()} rays, "
              f"max relative distance change {rel.max():.3g}")
        assert share > 0.5, share
        if kind == "pow2":
            assert_bitexact(t, t0, "pow2 distance")
            assert_bitexact(m, m0, "pow2 model")


@pytest.mark.parametrize("n_slots,chunk,n", [(640 * 512, 64, 20000), (128 * 96, 128, 4000), (128 * 96, 256, 4000),
                                             (64 * 48, 64, 3072), (130, 64, 1)])
def test_layouts_are_valid_block_counts(n_slots, chunk, n):
    """Every count in [0, chunk], the counts sum to the rays the layout carries
    (n; islands: one per island), over exactly the frame's blocks; at 5120 blocks
    tile_gap and islands reach past one k_scan tile of 4096 counts, tile_gap
    with a run of at least 4096 empty blocks across the tile boundary."""
    nb = (n_slots + chunk - 1) // chunk
    L = S.layouts(n_slots, chunk, n, 3)
    assert {"dense", "random", "last"} <= set(L)
    for name, c in L.items():
        assert c.dtype == np.int32 and len(c) == nb, name
        assert c.min() >= 0 and c.max() <= chunk, name
        assert c.sum() == (n if name != "islands" else min(n, (c > 0).sum())), (name, c.sum())
    if 2 * chunk < n <= n_slots // 2:
        assert len({c.tobytes() for c in L.values()}) == len(L)       # all different
        assert "ragged" in L and set(L["ragged"][:4].tolist()) == {1, chunk - 1}
        assert L["last"][-1] == chunk and L["last"][0] == 0 and L["dense"][0] == chunk and L["dense"][-1] == 0
        r = L["random"]
        assert len(np.unique(r[r > 0])) > min(chunk, (r > 0).sum()) // 4       # many different counts
    if nb > S.SCAN_TILE + 400:
        g = L["tile_gap"]
        assert g[0] == chunk and not g[1:1 + S.SCAN_TILE].any() and g[1 + S.SCAN_TILE] == chunk
        assert np.nonzero(g)[0].max() > S.SCAN_TILE               # full blocks in the second tile
        i = np.nonzero(L["islands"])[0]
        assert i[0] > 0 and i[-1] < nb - 1 and (np.diff(i) == 97).all() and i[-1] - i[0] > S.SCAN_TILE
    else:
        assert "tile_gap" not in L


@pytest.mark.parametrize("transformed", [False, True])
@pytest.mark.parametrize("grid", S.GRIDS)
def test_boundary_rays_sit_on_voxel_boundaries(pt_mod, grid, transformed):
    """Mapped back to model space, most ray origins have a coordinate within 0.6
    of a voxel boundary 0..grid[k] of their model's grid (every index occurs for
    small grids), also under the non-identity transform."""
    s = S.boundary_scene(pt_mod, grid, transformed)
    a = s.export()
    o, d = S.boundary_rays(a, 4000, 3, grid)
    assert np.isfinite(o).all() and np.isfinite(d).all() and (np.abs(d).max(1) > 0).all()
    near = np.zeros(len(o), bool)
    seen = [set(), set(), set()]
    for i in range(2):
        W = a["model_w2m"][i].reshape(4, 4).T.astype(np.float64)
        pm = o.astype(np.float64) @ W[:3, :3].T + W[:3, 3]
        bb = a["mesh_bbox"][a["model_ints"][i, 0]].astype(np.float64)
        vw = a["grid_vw"][a["model_ints"][i, 1]].astype(np.float64)
        for k in range(3):
            q = (pm[:, k] - bb[k]) / vw[k]
            on = (np.abs(q - np.rint(q)) * vw[k] < 0.6) & (np.rint(q) >= 0) & (np.rint(q) <= grid[k])
            near |= on
            seen[k] |= set(np.rint(q[on]).astype(int).tolist())
    assert near.mean() > 0.8, near.mean()
    for k in range(3):
        if grid[k] <= 31:
            assert seen[k] >= set(range(grid[k] + 1)), (k, sorted(seen[k]))
