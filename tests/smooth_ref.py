"""numpy restatement of smooth shading (test infrastructure; include/pathtracer_amd.h,
pt_scene_set_model_smooth): the hit normal of a smooth model, operation by operation in
float32, and env_ref.Restatement with one change before the oracle's ptor_shade: a hit on a
smooth model is shaded with that normal instead of the oracle's flat one.  The primary-hit
cache gets the same treatment.  Nothing else changes, so with no smooth model this is the
parent restatement (tests/test_smooth_ref.py holds it to that and to the oracle).

The oracle returns no triangle index.  The restatement takes the triangle of the hit model
whose flat world normal is nearest to the oracle's normal, and asserts for every hit that the
nearest candidate is within NEAR and the second nearest at least FAR away: a condition on the
fixtures, not a tolerance.  No hit is left out.  A triangle with a zero edge (two equal
corners) is no candidate: the reference triangle test computes det = dot(e1, cross(dir, e2)),
which is exactly 0 when e1 or e2 is, and rejects it, so such a triangle is never hit."""
import numpy as np

import env_ref as ER

F = np.float32
NEAR, FAR = 1e-5, 1e-4
_dot = ER._dot


def _normalize(a):
    """pt_math.h normalize: a * (1.0f / sqrtf(dot(a, a)))."""
    with np.errstate(all="ignore"):
        s = (F(1) / np.sqrt(_dot(a, a)).astype(F)).astype(F)
        return (a * s[..., None]).astype(F)


def normal_matrix(m2w):
    """scene.cpp m3_inverse_of_m4 of a column-major mat4 (16 float32): nm[9], float32 scalar by scalar."""
    m = [F(v) for v in np.asarray(m2w, F).reshape(16)]
    M = lambda c, r: m[c * 4 + r]                                                      # noqa: E731
    with np.errstate(all="ignore"):
        od = F(1) / (+M(0, 0) * (M(1, 1) * M(2, 2) - M(2, 1) * M(1, 2))
                     - M(1, 0) * (M(0, 1) * M(2, 2) - M(2, 1) * M(0, 2))
                     + M(2, 0) * (M(0, 1) * M(1, 2) - M(1, 1) * M(0, 2)))
        out = [None] * 9
        out[0 * 3 + 0] = +(M(1, 1) * M(2, 2) - M(2, 1) * M(1, 2)) * od
        out[1 * 3 + 0] = -(M(1, 0) * M(2, 2) - M(2, 0) * M(1, 2)) * od
        out[2 * 3 + 0] = +(M(1, 0) * M(2, 1) - M(2, 0) * M(1, 1)) * od
        out[0 * 3 + 1] = -(M(0, 1) * M(2, 2) - M(2, 1) * M(0, 2)) * od
        out[1 * 3 + 1] = +(M(0, 0) * M(2, 2) - M(2, 0) * M(0, 2)) * od
        out[2 * 3 + 1] = -(M(0, 0) * M(2, 1) - M(2, 0) * M(0, 1)) * od
        out[0 * 3 + 2] = +(M(0, 1) * M(1, 2) - M(1, 1) * M(0, 2)) * od
        out[1 * 3 + 2] = -(M(0, 0) * M(1, 2) - M(1, 0) * M(0, 2)) * od
        out[2 * 3 + 2] = +(M(0, 0) * M(1, 1) - M(1, 0) * M(0, 1)) * od
    assert all(type(v) is F for v in out)
    return np.array(out, F)


def xform_point(m16, p):
    """pt_math.h xform12 with w = 1: (m0*x + m1*y) + (m2*z + m3*1.0f) per row; m16 column-major."""
    m = np.asarray(m16, F).reshape(4, 4)                  # m[c][r]
    cols = []
    for k in range(3):
        a0, a1, a2 = ((m[c, k] * p[..., c]).astype(F) for c in range(3))
        a3 = F(m[3, k] * F(1))
        cols.append(((a0 + a1).astype(F) + (a2 + a3).astype(F)).astype(F))
    return np.stack(cols, axis=-1)


def xform_normal(nm, n):
    """pt_math.h xform_normal9: (nm[r][0]*x + nm[r][1]*y) + nm[r][2]*z."""
    nm = np.asarray(nm, F).reshape(3, 3)
    with np.errstate(all="ignore"):
        return np.stack([(((nm[r, 0] * n[..., 0]).astype(F) + (nm[r, 1] * n[..., 1]).astype(F)).astype(F)
                          + (nm[r, 2] * n[..., 2]).astype(F)).astype(F) for r in range(3)], axis=-1)


def smooth_normal(w2m, nm, v0, e1, e2, n0, n1, n2, o, d, dist, g):
    """The header's definition for m hits: every argument after nm is (m, 3) float32 (dist (m,)).
    Returns n (m, 3) float32 and why a hit kept the flat normal g (m,): 0 it did not, 1 s was not
    finite, 2 dot(s, g) <= 0."""
    o, d, g = (np.ascontiguousarray(a, F) for a in (o, d, g))
    dist = np.ascontiguousarray(dist, F)
    with np.errstate(all="ignore"):
        dr = _normalize(d)
        ip = (o + (dr * dist[:, None]).astype(F)).astype(F)
        pm = xform_point(w2m, ip)
        q = (pm - v0).astype(F)
        d11, d12, d22, q1, q2 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(q, e1), _dot(q, e2)
        den = ((d11 * d22).astype(F) - (d12 * d12).astype(F)).astype(F)
        b1 = (((d22 * q1).astype(F) - (d12 * q2).astype(F)).astype(F) / den).astype(F)
        b2 = (((d11 * q2).astype(F) - (d12 * q1).astype(F)).astype(F) / den).astype(F)
        b1 = np.fmin(np.fmax(b1, F(0)), F(1)).astype(F)                  # fmaxf / fminf: a NaN gives way
        b2 = np.fmin(np.fmax(b2, F(0)), (F(1) - b1).astype(F)).astype(F)
        b0 = ((F(1) - b1).astype(F) - b2).astype(F)
        m = (((n0 * b0[:, None]).astype(F) + (n1 * b1[:, None]).astype(F)).astype(F)
             + (n2 * b2[:, None]).astype(F)).astype(F)
        s = _normalize(xform_normal(nm, m))
        finite = np.isfinite(s).all(axis=1)
        ok = finite & (_dot(s, g) > 0)
    out = np.where(ok[:, None], s, g).astype(F)
    assert out.dtype == F
    return out, np.where(ok, 0, np.where(finite, 2, 1))


class Tables:
    """Per model of a FlatScene: its triangles' v0, e1, e2, n0, n1, n2, flat world normals and the
    candidate mask; per model nm."""

    def __init__(self, flat):
        self.flat = flat
        self.nm = [normal_matrix(m) for m in np.asarray(flat.model_m2w, F)]
        self.tri = {}

    def of(self, model):
        if model not in self.tri:
            f = self.flat
            mesh = int(f.model_ints[model, 0])
            ts, te = int(f.mesh_ranges[mesh, 2]), int(f.mesh_ranges[mesh, 3])
            t = np.asarray(f.tris, np.int32)[ts:te]
            P, N = np.asarray(f.vpos, F), np.asarray(f.vnrm, F)
            v0 = P[t[:, 0]]
            e1, e2 = (P[t[:, 1]] - v0).astype(F), (P[t[:, 2]] - v0).astype(F)
            n0, n1, n2 = N[t[:, 0]], N[t[:, 1]], N[t[:, 2]]
            # scene.cpp buildDeviceTables: normalize(((n0 + n1) + n2) * (1 / 3.0f)), then make_hit's transform
            tn = _normalize((((n0 + n1).astype(F) + n2).astype(F) * (F(1) / F(3))).astype(F))
            g = _normalize(xform_normal(self.nm[model], tn))
            cand = e1.any(axis=1) & e2.any(axis=1)              # a zero edge: det == 0, never hit
            self.tri[model] = dict(v0=v0, e1=e1, e2=e2, n0=n0, n1=n1, n2=n2, g=g, cand=cand, first=ts)
        return self.tri[model]


class Identification:
    """What the triangle identification saw, over every hit it was asked about."""

    def __init__(self):
        self.hits, self.worst_near, self.least_second = 0, 0.0, np.inf
        self.not_finite, self.opposed = 0, 0            # hits that kept the flat normal, by reason

    @property
    def fell_back(self):
        return self.not_finite + self.opposed

    def holds(self):
        return self.worst_near <= NEAR and self.least_second >= FAR


def shading_normals(flat, tables, smooth, o, d, dist, nrm, model, ident=None, check=True):
    """The normals the shading pass uses for the oracle's hits (dist, nrm, model) of the rays
    (o, d): nrm, with the hits on smooth models replaced.  -> (normals, scene triangle per hit, -1
    where none was looked up, smooth_normal's reason per hit)."""
    model = np.asarray(model)
    out = np.array(nrm, F, copy=True)
    tri = np.full(len(model), -1, np.int64)
    why = np.zeros(len(model), np.int64)
    for k in np.unique(model[model >= 0]):
        if not smooth[k]:
            continue
        sel = np.nonzero(model == k)[0]
        T = tables.of(int(k))
        ci = np.nonzero(T["cand"])[0]
        g = np.asarray(nrm, F)[sel]
        t = np.empty(len(sel), np.int64)
        for a in range(0, len(sel), 4096):                  # (hits, candidates) distances, in blocks
            gg = g[a:a + 4096].astype(np.float64)
            dd = np.sqrt(((gg[:, None, :] - T["g"][ci].astype(np.float64)[None, :, :]) ** 2).sum(axis=2))
            best = np.argmin(dd, axis=1)
            near = dd[np.arange(len(gg)), best]
            dd[np.arange(len(gg)), best] = np.inf
            second = dd.min(axis=1) if len(ci) > 1 else np.full(len(gg), np.inf)
            if ident is not None:
                ident.hits += len(gg)
                ident.worst_near = max(ident.worst_near, float(near.max()))
                ident.least_second = min(ident.least_second, float(second.min()))
            if check:
                assert near.max() <= NEAR, f"model {k}: nearest flat normal {near.max()} away"
                assert second.min() >= FAR, f"model {k}: second nearest flat normal only {second.min()} away"
            t[a:a + 4096] = ci[best]
        n, fell = smooth_normal(np.asarray(flat.model_w2m, F)[k], tables.nm[k],
                                *(T[name][t] for name in ("v0", "e1", "e2", "n0", "n1", "n2")),
                                np.asarray(o, F)[sel], np.asarray(d, F)[sel], np.asarray(dist, F)[sel], g)
        if ident is not None:
            ident.not_finite += int((fell == 1).sum())
            ident.opposed += int((fell == 2).sum())
        out[sel] = n
        tri[sel] = t + T["first"]
        why[sel] = fell
    return out, tri, why


class Restatement(ER.Restatement):
    """env_ref.Restatement with per-model smooth flags (a bool per model, or None: none)."""

    def __init__(self, flat, cfg, width=None, camera=None, env=None, smooth=None):
        nmodel = len(flat.model_ints)
        self.smooth = np.zeros(nmodel, bool) if smooth is None else np.asarray(smooth, bool).reshape(nmodel)
        self.tables = Tables(flat)
        self.ident = Identification()
        super().__init__(flat, cfg, width, camera, env)

    def primary_hits(self):
        """pt_renderer_primary_hits: the cached hits of the current view with the shading normal.
        hit_nrm itself stays the oracle's flat normal: the normal is a function of the ray, the
        distance, the model and the triangle alone, so _shade_batch derives it from a cached hit
        as it does from any other and gets the cache's bits."""
        nrm = self.hit_nrm
        if self.smooth.any():
            o = np.repeat(np.asarray(self.cam, F)[None, :], self.npix, axis=0)
            nrm = shading_normals(self.flat, self.tables, self.smooth, o, self.dirs, self.hit_dist, self.hit_nrm,
                                  self.hit_model, self.ident)[0]
        return self.hit_dist, nrm, self.hit_model

    def _shade_batch(self, it, slot, o, d, color, bounces, dist, nrm, model):
        if self.smooth.any():
            nrm = shading_normals(self.flat, self.tables, self.smooth, o, d, dist, nrm, model, self.ident)[0]
        super()._shade_batch(it, slot, o, d, color, bounces, dist, nrm, model)
