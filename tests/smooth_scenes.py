"""Fixture scenes of the smooth-shading tests (test infrastructure), as (meshes, models, smooth
flags) specs for path_scenes.scene_from_spec / oracle_scene_from_spec.

The smooth models are displaced tori (pathtracerap_amd.synthetic.torus_mesh, seed 2): their flat
normals are averages of distinct vertex normals, so no two triangles of the mesh share one (the
minimum distance between two is 1.6e-3 at 320 triangles, 2.4e-3 at 1000) and smooth_ref can tell
the hit triangle from the oracle's normal.  Meshes with repeated flat normals (the room, the
lamp's box) appear as flat models only."""
import numpy as np

import path_scenes as PS
from pathtracerap_amd.synthetic import light_mesh, room_mesh, torus_mesh

TORUS_SEED = 2
# (material, colour, scale, rotation, translation, smooth): four smooth instances and a flat one of
# the same mesh, non-uniform scales and rotations about every axis
_TORI = [("DIFFUSE", (0.75, 0.62, 0.40), (0.030, 0.040, 0.025), (35, 20, 10), (-300, 60, 60), True),
         ("METAL", (0.90, 0.90, 0.95), (0.035, 0.025, 0.030), (70, -30, 15), (-90, 90, 150), True),
         ("COAT", (0.15, 0.30, 0.90), (0.025, 0.035, 0.040), (20, 60, -40), (120, 70, 80), True),
         ("REFLECTIVE", (0.99, 0.99, 0.75), (0.030, 0.030, 0.045), (100, 10, 30), (320, 110, 0), True),
         ("METAL", (0.95, 0.60, 0.20), (0.040, 0.030, 0.030), (50, 45, 0), (10, 330, -60), False)]


def torus_models(mesh):
    return [dict(mesh=mesh, scale=s, rot=r, translate=t, material=m, color=c) for m, c, s, r, t, _ in _TORI]


def fixture_spec(ntri=320, normals="own", extra=None):
    """The flat room (model 0), an emissive lamp (model 1), then the tori (models 2..6; 6 is the
    flat instance).  normals: the torus mesh's "own" vertex normals, all of them "negated", or
    "mixed" (every 9th vertex of the grid -- no two in one triangle -- alternately negated and
    zeroed: next to a negated one the interpolated normal opposes the flat one, and a hit clamped
    onto a zeroed one interpolates to exactly zero, while every flat normal stays finite).
    extra: a (mesh, model dict, smooth) added last."""
    pos, nrm, tris = torus_mesh(ntri, seed=TORUS_SEED)
    if normals == "negated":
        nrm = -nrm
    elif normals == "mixed":
        nv = max(3, int(round(np.sqrt(ntri / 4.0))))            # torus_mesh's grid: vertex iu * nv + iv
        iu, iv = np.divmod(np.arange(len(nrm)), nv)
        nu = len(nrm) // nv
        pick = (iu % 3 == 0) & (iv % 3 == 0) & (iu < nu - nu % 3) & (iv < nv - nv % 3)     # not across the seam
        which = np.cumsum(pick) % 2 == 0
        nrm = nrm.copy()
        nrm[pick & which] *= -1
        nrm[pick & ~which] = 0
        assert (pick[tris].sum(axis=1) <= 1).all()
    else:
        assert normals == "own"
    meshes = [room_mesh(), light_mesh(), (pos, nrm, tris)]
    models = [dict(mesh=0, scale=(0.1, 0.1, 0.1), rot=(0, 0, 0), translate=(0, -120, 0), material="DIFFUSE",
                   color=(0.85, 0.85, 0.85)),
              dict(mesh=1, scale=(0.2, 0.02, 0.2), rot=(0, 0, 0), translate=(0, 870, -50), material="EMISSIVE",
                   color=(0.99, 0.99, 0.99))] + torus_models(2)
    smooth = [False, False] + [t[5] for t in _TORI]
    if extra is not None:
        mesh, model, sm = extra
        meshes.append(mesh)
        models.append(dict(model, mesh=len(meshes) - 1))
        smooth.append(sm)
    return meshes, models, np.array(smooth, bool)


def zero_area_extra():
    """path_scenes.zero_area_mesh as a smooth diffuse model in front of the tori."""
    return (PS.zero_area_mesh(), dict(scale=(0.08, 0.08, 0.08), rot=(60, 0, 0), translate=(-150, 260, 250),
                                      material="DIFFUSE", color=(0.3, 0.8, 0.4)), True)


def gpu_scene(P, spec):
    meshes, models, smooth = spec
    s = PS.scene_from_spec(P, meshes, models)
    for i in np.nonzero(smooth)[0]:
        s.set_smooth(int(i))
    return s


def min_flat_normal_distance(pos, nrm, tris):
    """The least distance between the flat normals of two triangles of a mesh (float64)."""
    n = nrm.astype(np.float64)[tris].sum(axis=1)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    best = np.inf
    for a in range(0, len(n), 1024):
        dd = np.sqrt(((n[a:a + 1024, None, :] - n[None, :, :]) ** 2).sum(axis=2))
        dd[np.arange(len(dd)), np.arange(a, a + len(dd))] = np.inf
        best = min(best, float(dd.min()))
    return best


def torus_targets(a, model, seed, n_random=600):
    """World points on a torus instance (export a, model index): every 7th vertex, the edge
    midpoints of every 5th triangle (so the clamp of the barycentrics is exercised) and seeded
    interior points.  -> (points (m, 3) float64, outward world directions (m, 3) float64)."""
    mesh = int(a["model_ints"][model, 0])
    ts, te = int(a["mesh_ranges"][mesh, 2]), int(a["mesh_ranges"][mesh, 3])
    t = a["tris"][ts:te]
    P, N = a["vpos"].astype(np.float64), a["vnrm"].astype(np.float64)
    # the outward side from the geometry, not from the vertex normals (a fixture may zero or negate
    # some): the triangles' geometric normals, signed like most of the vertex-normal sums
    geo = np.cross(P[t[:, 1]] - P[t[:, 0]], P[t[:, 2]] - P[t[:, 0]])
    if ((geo * N[t].sum(axis=1)).sum(axis=1) < 0).mean() > 0.5:
        geo = -geo
    pts, nrm = [P[t[::7, 0]]], [geo[::7]]
    for i, j in ((0, 1), (1, 2), (2, 0)):
        pts.append(0.5 * (P[t[::5, i]] + P[t[::5, j]]))
        nrm.append(geo[::5])
    rs = np.random.RandomState(seed)
    k = rs.randint(0, len(t), n_random)
    b = rs.dirichlet((1, 1, 1), n_random)
    pts.append((P[t[k]] * b[:, :, None]).sum(axis=1))
    nrm.append(geo[k])
    pts, nrm = np.concatenate(pts), np.concatenate(nrm)
    m2w = a["model_m2w"][model].astype(np.float64).reshape(4, 4).T
    w = pts @ m2w[:3, :3].T + m2w[:3, 3]
    nw = nrm @ np.linalg.inv(m2w[:3, :3])               # normals transform with the inverse transpose
    return w, nw / np.linalg.norm(nw, axis=1, keepdims=True)


def torus_rays(a, model, seed):
    """Rays aimed at torus_targets from outside: along the normal with a seeded tilt, and a
    quarter of them grazing (80 to 89 degrees off the normal)."""
    w, nw = torus_targets(a, model, seed)
    rs = np.random.RandomState(seed + 1)
    tang = np.cross(nw, rs.normal(size=nw.shape))
    tang /= np.linalg.norm(tang, axis=1, keepdims=True)
    ang = np.radians(rs.uniform(0, 60, len(w)))
    graze = np.arange(len(w)) % 4 == 3
    ang[graze] = np.radians(rs.uniform(80, 89, graze.sum()))
    out = nw * np.cos(ang)[:, None] + tang * np.sin(ang)[:, None]
    o = w + out * 150.0
    d = (w - o) * rs.uniform(0.01, 3.0, (len(w), 1))     # not normalised
    assert np.isfinite(o).all() and np.isfinite(d).all() and (np.abs(d).max(axis=1) > 0).all()
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
