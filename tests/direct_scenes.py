"""Segments for the any-hit tests of direct lighting (test infrastructure): about 4k per scene,
built from a scene's own rays and the oracle's closest hits along them, so that the mix holds
random pairs, surface point to light point, axis-parallel and zero-component directions, origins
inside boxes, occluders just before and just beyond the target, and segments of zero length.

"Just before / beyond": the target is placed so that the nearest occluder lies at tmax * (1 -/+
EDGE) with EDGE ten times direct_ref.NEAR_TIE, so these are decided cases, not near ties."""
import numpy as np

import direct_ref as DR
import oracle as O

F = np.float32
EDGE = 1e-3
SCENES = ["room", "flat-y-h0-id", "flat-x-h2^-7-xf", "flat-z-h4-xf", "pair-2-middle-ab", "pair-14-last-ba"]


def direct_spec():
    """glass_scenes.fixture_spec for the direct-lighting renders: the lamp rotated (it stays
    non-uniformly scaled), a second small lamp rotated about all three axes, and the smooth and
    the textured torus DIFFUSE, so that light is sampled at flat, smooth and textured diffuse
    receivers; the box and the flat torus stay glass."""
    import glass_scenes as GS
    spec = GS.fixture_spec()
    spec["models"][1]["rot"] = (8, 30, -6)
    for i in (GS.SMOOTH, GS.TEXTURED):
        spec["models"][i]["material"] = "DIFFUSE"
    spec["models"].append(dict(mesh=1, scale=(0.05, 0.05, 0.02), rot=(40, 10, 70), translate=(250, 400, -200),
                               material="EMISSIVE", color=(0.9, 0.6, 0.3)))
    spec["smooth"] = np.append(spec["smooth"], False)
    spec["binding"] = np.append(spec["binding"], -1)
    spec["ior"] = np.append(spec["ior"], F(1.5))
    return spec


def without_lights(spec):
    """The spec with every EMISSIVE instance switched to DIFFUSE."""
    import copy
    out = copy.deepcopy(spec)
    for m in out["models"]:
        if m["material"] == "EMISSIVE":
            m["material"] = "DIFFUSE"
    return out


def _unit(d):
    d = np.asarray(d, np.float64)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def along_rays(flat, o, d, seed):
    """Targets along the rays (o, d): a third at random lengths, the hits' rays split between
    far short of, just before and just beyond their closest hit."""
    rs = np.random.RandomState(seed)
    o = np.ascontiguousarray(o, F)
    dn = _unit(d)
    t, _, model = O.intersect_rays(flat, o, np.ascontiguousarray(dn, F), accel=1, threads=4)
    t, hit = t.astype(np.float64), model >= 0
    kind = rs.randint(0, 4, len(o))
    r = rs.uniform(1.0, 1500.0, len(o))
    near = np.where(hit, t, r)
    r = np.where(kind == 1, near * 0.5, r)
    r = np.where(kind == 2, near / 0.999 * (1 - EDGE), r)        # tmax just short of the occluder
    r = np.where(kind == 3, near / 0.999 * (1 + EDGE), r)        # ... just beyond it
    return o, (o.astype(np.float64) + dn * r[:, None]).astype(F)


def room_segments(flat, lights, n=4096, seed=5, lo=(-450.0, -100.0, -450.0), hi=(450.0, 850.0, 450.0)):
    """The fixture room's mix -> (orig, target, {name: slice})."""
    rs = np.random.RandomState(seed)
    lo, hi = np.array(lo), np.array(hi)
    k = n // 8
    parts, where = [], {}

    def add(name, o, t):
        start = sum(len(p[0]) for p in parts)
        parts.append((np.asarray(o, F).reshape(-1, 3), np.asarray(t, F).reshape(-1, 3)))
        where[name] = slice(start, start + len(parts[-1][0]))

    add("random pairs", rs.uniform(lo, hi, (2 * k, 3)), rs.uniform(lo, hi, (2 * k, 3)))
    # surface point to light point: the closest hits of random rays, lifted off the surface
    o = rs.uniform(lo * 0.8, hi * 0.8, (2 * k, 3)).astype(F)
    dn = _unit(rs.normal(size=(2 * k, 3)))
    t, nrm, model = O.intersect_rays(flat, o, np.ascontiguousarray(dn, F), accel=1, threads=4)
    ok = model >= 0
    surf = (o.astype(np.float64) + dn * t.astype(np.float64)[:, None] + nrm.astype(np.float64) * 0.1)[ok]
    li = rs.randint(0, len(lights["cdf"]), len(surf))
    a, b = rs.uniform(0, 1, len(surf)), rs.uniform(0, 1, len(surf))
    s = np.sqrt(a)
    y = lights["p0"][li].astype(np.float64) + lights["e1"][li] * (s * (1 - b))[:, None] + lights["e2"][li] * (s * b)[:, None]
    add("surface to light", surf, y)
    # axis-parallel and zero-component directions
    o = rs.uniform(lo, hi, (k, 3))
    d = rs.normal(size=(k, 3))
    d[: k // 2, rs.randint(0, 3)] = 0.0
    ax = rs.randint(0, 3, k - k // 2)
    d[k // 2:] = np.eye(3)[ax] * rs.choice([-1.0, 1.0], k - k // 2)[:, None]
    add("axis-parallel", o, o + _unit(d) * rs.uniform(10.0, 1200.0, (k, 1)))
    # origins inside the instances' boxes (the world boxes of their vertices)
    vpos = np.asarray(flat.vpos, np.float64)
    inside = []
    for m in range(2, len(flat.model_ints)):
        mesh = int(flat.model_ints[m, 0])
        v = vpos[int(flat.mesh_ranges[mesh, 0]):int(flat.mesh_ranges[mesh, 1])]
        M = np.asarray(flat.model_m2w, np.float64)[m].reshape(4, 4).T
        w = (np.c_[v, np.ones(len(v))] @ M.T)[:, :3]
        c, h = (w.max(0) + w.min(0)) / 2, (w.max(0) - w.min(0)) / 2
        inside.append(c + rs.uniform(-0.5, 0.5, (k // 5, 3)) * h)
    inside = np.concatenate(inside)
    add("inside boxes", inside, rs.uniform(lo, hi, inside.shape))
    # occluders just before and just beyond the target, and short segments
    o, tgt = along_rays(flat, rs.uniform(lo * 0.9, hi * 0.9, (2 * k, 3)), rs.normal(size=(2 * k, 3)), seed + 1)
    add("along rays", o, tgt)
    z = rs.uniform(lo, hi, (k // 4, 3))
    add("zero length", z, z)
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), where


def ray_segments(flat, o, d, n=4096, seed=9):
    """A degenerate scene's mix from its own rays: along_rays, and a 32nd of zero length."""
    o, t = along_rays(flat, np.asarray(o)[:n], np.asarray(d)[:n], seed)
    t = np.array(t, copy=True)
    t[::32] = o[::32]
    return o, t


def decided(flat, orig, target):
    """-> (occluded, near tie) from the oracle alone."""
    return DR.segments_occluded(flat, orig, target)
