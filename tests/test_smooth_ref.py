"""The yardstick of the smooth-shading tests, held to the oracle (CPU only): with no smooth
model the restatement in smooth_ref.py is env_ref's and the oracle's render bit for bit; the
triangle identification it rests on holds on every fixture, for every hit; and its float32
normals agree with a float64 evaluation of the same formulas."""
import numpy as np
import pytest

import env_ref as ER
import path_scenes as PS
import smooth_ref as SR
import smooth_scenes as SS
from helpers import assert_bitexact

F = np.float32
W, H, BOUNCES, ITERS = 64, 48, 4, 2


def fixture(O, ntri=320, normals="own", extra=None):
    meshes, models, smooth = SS.fixture_spec(ntri, normals, extra)
    return PS.oracle_scene_from_spec(O, meshes, models), smooth


def cfg_of(O, accel):
    return O.RenderConfig(width=W, height=H, max_bounces=BOUNCES, accel=accel, threads=4)


@pytest.mark.parametrize("accel", [0, 1])
def test_no_smooth_model_is_the_parent_and_the_oracle(oracle_mod, accel):
    O = oracle_mod
    flat, _ = fixture(O)
    cfg = cfg_of(O, accel)
    want = ER.Restatement(flat, cfg)
    want.render(0, ITERS)
    got = SR.Restatement(flat, cfg, smooth=None)
    got.render(0, ITERS)
    assert want.S.any()
    assert_bitexact(got.S, want.S, "image")
    assert_bitexact(got.Q, want.Q, "moments")
    assert got.segments == want.segments and got.live == want.live
    assert got.per_bounce.tolist() == want.per_bounce.tolist()
    assert got.ident.hits == 0
    image, seg = O.render(flat, O.RenderConfig(width=W, height=H, iterations=ITERS, max_bounces=BOUNCES, accel=accel,
                                               threads=4))
    assert_bitexact(got.S, image, "the oracle's image")
    for a, b, name in zip(got.primary_hits(), (want.hit_dist, want.hit_nrm, want.hit_model), ("dist", "normal", "model")):
        assert_bitexact(a, b, f"primary {name}")


@pytest.mark.parametrize("mesh,least", [(("torus", 320), 1.6e-3), (("torus", 1000), 2.4e-3), (("torus", 3000), 1.1e-3)])
def test_flat_normals_of_a_fixture_mesh_are_distinct(mesh, least):
    from pathtracerap_amd.synthetic import torus_mesh
    got = SS.min_flat_normal_distance(*torus_mesh(mesh[1], seed=SS.TORUS_SEED))
    print(f"{mesh}: minimum distance between two flat normals {got:.3g}")
    assert got >= 0.9 * least and got >= 10 * SR.FAR


FIXTURES = [("torus-320", dict(ntri=320)), ("torus-1000", dict(ntri=1000)),
            ("negated", dict(normals="negated")), ("mixed", dict(normals="mixed")),
            ("zero-area", dict(extra="zero_area"))]


@pytest.mark.parametrize("name,kw", FIXTURES)
@pytest.mark.parametrize("accel", [0, 1])
def test_identification_holds_for_every_hit(oracle_mod, name, kw, accel):
    """A render of each fixture: shading_normals asserts the condition hit by hit (none is left
    out), and the record over all of them is asserted again here."""
    O = oracle_mod
    kw = dict(kw)
    if kw.get("extra") == "zero_area":
        kw["extra"] = SS.zero_area_extra()
    flat, smooth = fixture(O, **kw)
    ref = SR.Restatement(flat, cfg_of(O, accel), smooth=smooth)
    ref.primary_hits()
    ref.render(0, ITERS)
    i = ref.ident
    print(f"{name} accel {accel}: {i.hits} hits on smooth models, nearest candidate at most {i.worst_near:.3g} away, "
          f"second nearest at least {i.least_second:.3g}; {i.fell_back} kept the flat normal")
    assert i.hits > 1000 and i.holds()
    assert i.worst_near <= SR.NEAR and i.least_second >= SR.FAR
    assert np.isfinite(ref.S).all()
    if name == "mixed":
        assert i.opposed >= 20                   # next to a negated vertex normal: dot(s, g) <= 0
    else:
        assert i.fell_back < i.hits // 20


def smooth_normal_f64(flat, model, tri, o, d, dist, g):
    """The header's formulas in float64 from the float32 inputs (matrices included)."""
    w2m = np.asarray(flat.model_w2m, np.float64)[model].reshape(4, 4).T
    nm = np.linalg.inv(np.asarray(flat.model_m2w, np.float64)[model].reshape(4, 4).T[:3, :3])
    P, N, t = np.asarray(flat.vpos, np.float64), np.asarray(flat.vnrm, np.float64), np.asarray(flat.tris)[tri]
    v0, e1, e2 = P[t[:, 0]], P[t[:, 1]] - P[t[:, 0]], P[t[:, 2]] - P[t[:, 0]]
    o, d, dist = o.astype(np.float64), d.astype(np.float64), dist.astype(np.float64)
    ip = o + d / np.linalg.norm(d, axis=1, keepdims=True) * dist[:, None]
    q = ip @ w2m[:3, :3].T + w2m[:3, 3] - v0
    dot = lambda a, b: (a * b).sum(axis=1)                                              # noqa: E731
    d11, d12, d22, q1, q2 = dot(e1, e1), dot(e1, e2), dot(e2, e2), dot(q, e1), dot(q, e2)
    den = d11 * d22 - d12 * d12
    b1 = np.clip((d22 * q1 - d12 * q2) / den, 0.0, 1.0)
    b2 = np.minimum(np.maximum((d11 * q2 - d12 * q1) / den, 0.0), 1.0 - b1)
    b0 = 1.0 - b1 - b2
    m = N[t[:, 0]] * b0[:, None] + N[t[:, 1]] * b1[:, None] + N[t[:, 2]] * b2[:, None]
    s = m @ nm                                           # the inverse transpose times m
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    return np.where((dot(s, g.astype(np.float64)) > 0)[:, None], s, g.astype(np.float64)), (b0, b1, b2)


@pytest.mark.parametrize("ntri", [320, 1000])
def test_float32_normals_agree_with_float64(oracle_mod, ntri):
    """On the fixtures' hits (camera rays and rays aimed at vertices, edge midpoints and at
    grazing angles) the float32 normal is within 1e-4 per component of the float64 one."""
    O = oracle_mod
    flat, smooth = fixture(O, ntri=ntri)
    a = dict(model_ints=flat.model_ints, mesh_ranges=flat.mesh_ranges, tris=flat.tris, vpos=flat.vpos, vnrm=flat.vnrm,
             model_m2w=flat.model_m2w)
    tables = SR.Tables(flat)
    worst, total, clamped = 0.0, 0, 0
    for model in (2, 3, 4, 5):
        o, d = SS.torus_rays(a, model, seed=10 + model)
        dist, nrm, hit = O.intersect_rays(flat, o, d, accel=1, threads=4)
        sel = hit == model
        assert sel.sum() > len(o) // 2
        got, tri, _ = SR.shading_normals(flat, tables, smooth, o[sel], d[sel], dist[sel], nrm[sel], hit[sel])
        want, (b0, b1, b2) = smooth_normal_f64(flat, model, tri, o[sel], d[sel], dist[sel], nrm[sel])
        worst = max(worst, float(np.abs(got.astype(np.float64) - want).max()))
        total += int(sel.sum())
        clamped += int(((b0 == 0) | (b1 == 0) | (b2 == 0)).sum())
    print(f"{ntri} triangles: {total} hits, {clamped} with a clamped barycentric, largest float32 - float64 "
          f"component difference {worst:.3g}")
    assert clamped >= 20
    assert worst <= 1e-4
