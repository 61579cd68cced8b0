"""The oracle against the reference's own code (CPU).

oracle/ptoracle.c is a restatement of the reference written for this project;
oracle/_ref/libptref.so is the reference's text itself, compiled for the host
(oracle/ref/bridge.cpp lists the differences from its CUDA build).  These tests
hold the first to the second, bit for bit: with the library when it is built,
with the recordings under tests/golden/reference_code/ otherwise (and with both,
the recordings must equal the library).

Intersection.  A default optimising build of the reference's code differs from
the oracle's grid walk on 284 of the 200,000 camera rays, 1,074 of the 200,000
secondary rays and 44 of the 20,000 random rays of reference_code_cases, always towards the
exhaustive closest hit.  The cause is not the oracle and not a float->int
conversion: computeRayGridIntersection has no return statement where the ray
misses the mesh's bounding box, the optimiser treats that path as unreachable
and drops the rejection, and the walk then runs for rays that pass just outside
a face, where the triangle test's EPSILON slack accepts them.  Built with
-fno-strict-return (the recipe's build) the path stays, the function reports no
hit there, and all 420,000 rays equal the oracle bit for bit.  No ray is left
out of any comparison here.
"""
import numpy as np
import pytest

import oracle as O
from oracle import reference_code as R

from helpers import assert_bitexact
import reference_code_cases as C

needs_library = pytest.mark.skipif(not R.available(), reason=f"{R.LIB_PATH} is not built (no reference tree at build time) "
                                                              "and this check has no recording")


# ---------------------------------------------------------------------------
# RNG and scatter
# ---------------------------------------------------------------------------

def test_first_uniform_equals_the_engine():
    it, slot, dp = C.seed_triples()
    want, src = C.reference_u01()
    L = O.lib()
    mine = np.array([L.ptor_u01_first(int(a), int(b), int(c)) for a, b, c in zip(it, slot, dp)], np.float32)
    assert set(it.tolist()) == set(C.ITERS) and set(dp.tolist()) == set(C.DEPTHS + C.SEED_DEPTHS)
    assert slot.max() == C.MAX_SLOT and slot.min() == 0
    assert_bitexact(mine, want, f"ptor_u01_first vs the reference's engine ({src})")


@pytest.mark.parametrize("it", C.ITERS)
def test_shade_kernel(it):
    """shadeRayKernel == ptor_shade for every material type, hit or miss, any bounce count."""
    slot, orig, dirs, color, bounces, hit_dist, nrm, hit_type, hit_color = C.shade_inputs()
    r_orig, r_dir, r_color, r_bounces, r_hit, src = C.reference_shade(it)
    assert set(hit_type.tolist()) == set(range(7))
    assert set(C.DEPTHS) <= set(bounces.tolist()) and (bounces <= 0).any()
    assert (hit_dist == C.FLOAT_MAX).any()
    o_orig, o_dir, o_color, o_bounces = O.shade(it, slot, orig, dirs, color, bounces, hit_dist, nrm, hit_type, hit_color)
    assert_bitexact(o_bounces, r_bounces, f"bounces ({src})")
    assert_bitexact(o_color, r_color, f"colour ({src})")
    assert_bitexact(o_orig, r_orig, f"origin ({src})")
    assert_bitexact(o_dir, r_dir, f"direction ({src})")
    assert (r_hit == C.FLOAT_MAX).all()                       # every path leaves impact_distance reset


def test_shade_kernel_leaves_specular_and_refractive_rays_in_place():
    """The reference has no branch for SPECULAR and REFRACTIVE: a live ray that hits
    one keeps origin, direction and colour and loses one bounce."""
    slot, orig, dirs, color, bounces, hit_dist, nrm, hit_type, hit_color = C.shade_inputs()
    r_orig, r_dir, r_color, r_bounces, _, src = C.reference_shade(C.ITERS[1])
    sel = np.isin(hit_type, [O.MATERIALS["SPECULAR"], O.MATERIALS["REFRACTIVE"]]) & (bounces > 0) & (hit_dist < C.FLOAT_MAX)
    assert sel.sum() > 300                                    # 2 of 7 types of 2048 rays, less the dead and the misses
    assert_bitexact(r_orig[sel], orig[sel], f"origin ({src})")
    assert_bitexact(r_dir[sel], dirs[sel], f"direction ({src})")
    assert_bitexact(r_color[sel], color[sel], f"colour ({src})")
    assert np.array_equal(r_bounces[sel], bounces[sel] - 1)
    o = O.shade(C.ITERS[1], slot, orig, dirs, color, bounces, hit_dist, nrm, hit_type, hit_color)
    assert_bitexact(o[0][sel], orig[sel], "oracle origin")
    assert_bitexact(o[1][sel], dirs[sel], "oracle direction")
    assert np.array_equal(o[3][sel], bounces[sel] - 1)


@pytest.mark.parametrize("kind", list(C.SCATTER_KINDS))
def test_scatter_functions(kind):
    """calculateRandomDirectionInHemisphere / MetalScattering / CoatScattering / reflectRay,
    called directly with glm::normalize of the incoming direction, as shadeRayKernel calls
    them, == the direction ptor_shade leaves for the matching material, seeds and raw direction."""
    it, slot, dp, nrm, dirs = C.scatter_inputs()
    want, src = C.reference_scatter(kind)
    n = len(nrm)
    mat = O.MATERIALS[C.SCATTER_KINDS[kind][1]]
    got = np.zeros((n, 3), np.float32)
    for i in sorted(set(it.tolist())):                         # ptor_shade takes one iteration per call
        s = it == i
        k = int(s.sum())
        # remaining_bounces is the seed's depth
        out = O.shade(i, slot[s], np.zeros((k, 3), np.float32), dirs[s], np.ones((k, 3), np.float32), dp[s],
                      np.full(k, 1.0, np.float32), nrm[s], np.full(k, mat, np.int32), np.ones((k, 3), np.float32))
        got[s] = out[1]
    assert_bitexact(got, want, f"{kind} ({src})")


def test_transcendentals_equal_float64_rounded():
    """What pt_math.h and bridge.cpp say of ptor_sinf / ptor_cosf / ptor_powf: on 100,000
    arguments each they equal the float64 value rounded to float."""
    L = O.lib()
    rs = np.random.RandomState(1)
    x = rs.uniform(0, 2 * np.pi, 100000).astype(np.float32)
    s = np.array([L.ptor_sinf(float(v)) for v in x], np.float32)
    c = np.array([L.ptor_cosf(float(v)) for v in x], np.float32)
    assert_bitexact(s, np.sin(x.astype(np.float64)).astype(np.float32), "sin")
    assert_bitexact(c, np.cos(x.astype(np.float64)).astype(np.float32), "cos")
    u = rs.uniform(0, 1, 100000).astype(np.float32)
    y = np.float32(1.0) / np.float32(31.0)                    # calculateMetalScattering's exponent
    p = np.array([L.ptor_powf(float(v), float(y)) for v in u], np.float32)
    assert_bitexact(p, np.power(u.astype(np.float64), np.float64(y)).astype(np.float32), "pow")


# ---------------------------------------------------------------------------
# transforms and the model matrix
# ---------------------------------------------------------------------------

def test_model_matrices_and_transforms():
    """glm's translate * rotate * scale and inverse, and transformPosition / Direction /
    Normal under each, for the reference scene's eleven models."""
    pts = C.transform_points()
    models = O.REFERENCE_MODELS
    assert len(models) == 11
    got, src = C.reference_transforms()
    fs = C.ref_scene()
    for i, m in enumerate(models):
        m2w, w2m = O.model_matrix(m["scale"], m["rot"], m["translate"])
        assert_bitexact(m2w, got[f"m{i}_m2w"], f"model {i} model_to_world ({src})")
        assert_bitexact(w2m, got[f"m{i}_w2m"], f"model {i} world_to_model ({src})")
        assert_bitexact(fs.model_m2w[i], got[f"m{i}_m2w"], f"scene model {i} model_to_world")
        assert_bitexact(fs.model_w2m[i], got[f"m{i}_w2m"], f"scene model {i} world_to_model")
        for mat, tag in ((m2w, "f"), (w2m, "i")):
            for k, name in ((0, "p"), (1, "d"), (2, "n")):
                assert_bitexact(O.transform(k, mat, pts), got[f"m{i}_{name}{tag}"], f"model {i} transform {name}{tag} ({src})")


# ---------------------------------------------------------------------------
# intersection
# ---------------------------------------------------------------------------

def _check_hits(fs, o, d, ref, what):
    rd, rn, rt = ref
    od, on, om = O.intersect_rays(fs, o, d, accel=0)
    assert_bitexact(C.oracle_types(fs, om), rt, f"material {what}")
    assert_bitexact(od, rd, f"distance {what}")
    hit = om >= 0
    assert_bitexact(on[hit], rn[hit], f"normal {what}")
    return od, on, om


@pytest.mark.parametrize("name", list(C.BATCHES) + C.DEGENERATE)
def test_intersection_recorded_batches(name):
    """computeRaySceneIntersectionKernel == the oracle's grid walk on every ray of the
    recorded subset: distance, normal and material."""
    sc, o, d = C.batch(name, full=False)
    rd, rn, rt, src = C.reference_hits(name)
    assert len(o) <= C.RECORD_RAYS
    od, on, om = _check_hits(C.flat_scene(sc), o, d, (rd, rn, rt), f"{name} ({src})")
    assert (om >= 0).mean() > 0.2, "the batch hardly hits anything"


@needs_library
@pytest.mark.parametrize("name", list(C.BATCHES))
def test_intersection_whole_batches(name):
    """The same on all 200,000 camera, 200,000 secondary and 20,000 random rays."""
    sc, o, d = C.batch(name, full=True)
    assert len(o) == {"camera": 200000, "secondary": 200000, "random": 20000}[name]
    _check_hits(C.flat_scene(sc), o, d, C.reference_hits_full(name), name)


def test_bounding_box_rejection_is_what_separates_walk_and_closest_hit():
    """The rays on which a build that drops the bounding-box rejection differs are there
    and are tested: rays that miss a model's box (so the walk reports nothing for it) while
    a triangle of it, tested with its EPSILON slack, is the closest hit.  On them the
    reference's code sides with the oracle's walk, not with the exhaustive closest hit."""
    fs = C.ref_scene()
    for name, floor in (("camera", 1), ("secondary", 10)):
        _, o, d = C.batch(name, full=False)
        rd, rn, rt, src = C.reference_hits(name)
        gd, gn, gm = O.intersect_rays(fs, o, d, accel=0)
        bd, bn, bm = O.intersect_rays(fs, o, d, accel=1)
        differ = gd.view(np.uint32) != bd.view(np.uint32)
        assert differ.sum() >= floor, (name, int(differ.sum()))
        assert (bd[differ] < gd[differ]).all()
        assert_bitexact(rd[differ], gd[differ], f"{name}: reference vs walk where walk != closest hit ({src})")


# ---------------------------------------------------------------------------
# whole renders
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", C.RENDERS, ids=C.render_id)
def test_render(case):
    """The reference's kernels in renderLoop's order == oracle.render: the accumulator
    bit for bit, and the rays alive at each bounce."""
    sc, w, h, td = case
    img, live, src = C.reference_render(case)
    cfg = O.RenderConfig(width=w, height=h, iterations=C.RENDER_ITERS, max_bounces=C.MAX_BOUNCES, accel=0, tail_drop=td)
    oimg, oseg, olive = O.render_bounces(C.flat_scene(sc), cfg, live_cap=len(live))
    assert np.array_equal(olive, live), (olive, live, src)
    assert oseg == int(live.sum())
    launched = (w * h // 32) * 32 if td else w * h
    assert live[0] == C.RENDER_ITERS * launched and live[C.MAX_BOUNCES:].sum() == 0
    assert_bitexact(oimg, img, f"accumulator {C.render_id(case)} ({src})")
    if td:
        assert (img[launched:] == 0).all() and (img[:launched] > 0).any()


def test_seven_material_render_reaches_every_material():
    """Precondition of the seven-material case: primary or bounce rays hit every type."""
    fs = C.flat_scene(C.SEVEN)
    o, d = C.camera_rays(64, 48)
    t, n, m = O.intersect_rays(fs, o, d, accel=0)
    assert set(C.oracle_types(fs, m[m >= 0]).tolist()) == set(range(7))


# ---------------------------------------------------------------------------
# the grid builder
# ---------------------------------------------------------------------------

def test_grid_build():
    """Scene::addMeshesToGrid == ptor_build_grids for the reference scene: every vector."""
    fs = C.ref_scene()
    got, src = C.reference_grid()
    assert_bitexact(fs.model_ints[:, 1], got["model_grid"], f"grid index per model ({src})")
    assert_bitexact(fs.grid_ints, got["grid_ints"], f"grids ({src})")
    assert_bitexact(fs.grid_vw, got["grid_vw"], f"voxel widths ({src})")
    assert_bitexact(fs.vox, got["vox"], f"voxels ({src})")
    assert_bitexact(fs.per_voxel, got["per_voxel"], f"per-voxel triangle lists ({src})")
