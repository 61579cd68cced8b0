"""numpy restatement of direct lighting (test infrastructure; include/pathtracer_amd.h, "Direct
lighting"): the light table in float64, the estimator operation by operation in float32 with
every intermediate cast, and glass_ref.Restatement with light sampling around it.

The restatement follows the pixels of every batch itself (_shade_batch receives none): a batch's
rays are the survivors, in order, of the batch before, and the first batch's are the iteration's
active pixels in ascending order.  Each iteration is rendered into zeroed S and Q, which then hold
t, the value the path's end wrote; the sample of the header's section goes into the sums instead.
Visibility is the oracle's exact closest hit (ptor_intersect_rays with accel 1) along the shadow
ray: occluded when its distance is below tmax.  A shadow ray whose closest distance lies within
NEAR_TIE * tmax of tmax is recorded as a near tie: there the any-hit decision of the device, which
meets the triangles in another order, may differ by the rounding of one distance.

With no EMISSIVE model, or with the switch off, this is the parent restatement
(tests/test_direct_ref.py holds it to that)."""
import numpy as np

import glass_ref as GR
import oracle as O
import smooth_ref as SR

F = np.float32
_dot = SR._dot
DIFFUSE, EMISSIVE = 0, 4
NEAR_TIE = 1e-4
PI = F(3.14159265358979323846)


def light_table(flat):
    """Scene::lightTable in float64 numpy: the triangles of every EMISSIVE model, models in index
    order and triangles in mesh order -> the dict Renderer.lights() returns."""
    vpos = np.asarray(flat.vpos, F).astype(np.float64)
    tris = np.asarray(flat.tris, np.int64)
    P0, E1, E2, NL, A, M, E = [], [], [], [], [], [], []
    for k in range(len(flat.model_ints)):
        if int(flat.model_ints[k, 2]) != EMISSIVE:
            continue
        mesh = int(flat.model_ints[k, 0])
        ts, te = int(flat.mesh_ranges[mesh, 2]), int(flat.mesh_ranges[mesh, 3])
        m = np.asarray(flat.model_m2w, F)[k].astype(np.float64).reshape(4, 4)        # m[c][r]
        v = vpos[tris[ts:te]]                                                       # (t, 3 corners, 3)
        pw = ((m[0][None, None, :3] * v[..., 0:1] + m[1][None, None, :3] * v[..., 1:2])
              + m[2][None, None, :3] * v[..., 2:3]) + m[3][None, None, :3]
        e1, e2 = pw[:, 1] - pw[:, 0], pw[:, 2] - pw[:, 0]
        cr = np.stack([e1[:, 1] * e2[:, 2] - e2[:, 1] * e1[:, 2], e1[:, 2] * e2[:, 0] - e2[:, 2] * e1[:, 0],
                       e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1]], axis=1)
        ln = np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])
        with np.errstate(all="ignore"):
            nl = np.where(ln[:, None] > 0, cr / ln[:, None], 0.0)
        P0.append(pw[:, 0]); E1.append(e1); E2.append(e2); NL.append(nl); A.append(0.5 * ln)
        M.append(np.full(te - ts, k, np.int32))
        E.append(np.repeat(np.asarray(flat.model_color, F)[k][None, :], te - ts, axis=0))
    if not A:
        z3 = np.zeros((0, 3), F)
        return dict(p0=z3, e1=z3, e2=z3, nl=z3, emission=z3, area=np.zeros(0, F), cdf=np.zeros(0, F),
                    model=np.zeros(0, np.int32), area_total=F(0))
    area = np.concatenate(A)
    total = 0.0
    acc = np.empty(len(area))
    for i, a in enumerate(area):                 # the running sum, in order
        total += a
        acc[i] = total
    cdf = (acc / total).astype(F) if total > 0 else np.zeros(len(area), F)
    cdf[-1] = F(1)
    return dict(p0=np.concatenate(P0).astype(F), e1=np.concatenate(E1).astype(F), e2=np.concatenate(E2).astype(F),
                nl=np.concatenate(NL).astype(F), emission=np.concatenate(E).astype(F), area=area.astype(F), cdf=cdf,
                model=np.concatenate(M), area_total=F(total))


def same_table(got, want):
    """Both tables bit for bit."""
    for key in ("p0", "e1", "e2", "nl", "emission", "area", "cdf"):
        a, b = np.ascontiguousarray(got[key], F), np.ascontiguousarray(want[key], F)
        if a.shape != b.shape or (a.view(np.uint32) != b.view(np.uint32)).any():
            return False
    return (np.asarray(got["model"]) == np.asarray(want["model"])).all() and \
        F(got["area_total"]).view(np.uint32) == F(want["area_total"]).view(np.uint32)


def uniforms(it, slot, bounces):
    """u0, u1, u2 of the hits (GR.u01_first under the three depth codes)."""
    b = np.asarray(bounces, np.int64)
    return tuple(GR.u01_first(it, slot, c + b) for c in (256, 320, 384))


def sample(lights, o, d, dist, n, mc, c, u0, u1, u2):
    """The estimator up to the shadow ray for m hits -> dict(light (m,) int32, -1 where the
    geometry test fails; y, g, dc; xo, wn, tmax: the shadow ray).  Every array float32."""
    o, d, n, mc, c = (np.ascontiguousarray(a, F).reshape(-1, 3) for a in (o, d, n, mc, c))
    dist = np.ascontiguousarray(dist, F).reshape(-1)
    u0, u1, u2 = (np.ascontiguousarray(a, F).reshape(-1) for a in (u0, u1, u2))
    cdf = np.asarray(lights["cdf"], F)
    with np.errstate(all="ignore"):
        i = np.minimum(np.searchsorted(cdf, u0, side="right"), len(cdf) - 1)      # the smallest i with u0 < cdf[i]
        s = np.sqrt(u1).astype(F)
        a1 = (s * (F(1) - u2).astype(F)).astype(F)
        a2 = (s * u2).astype(F)
        y = ((lights["p0"][i] + (lights["e1"][i] * a1[:, None]).astype(F)).astype(F)
             + (lights["e2"][i] * a2[:, None]).astype(F)).astype(F)
        dirn = SR._normalize(d)
        ip = (o + (dirn * dist[:, None]).astype(F)).astype(F)
        xo = (ip + (n * F(0.1)).astype(F)).astype(F)
        w = (y - xo).astype(F)
        r2 = _dot(w, w)
        r = np.sqrt(r2).astype(F)
        wn = SR._normalize(w)
        cx = _dot(n, wn)
        cy = np.abs(_dot(lights["nl"][i], wn)).astype(F)
        ok = (cx > 0) & (cy > 0) & (r2 > 0)
        g = (((cx * cy).astype(F) / (PI * r2).astype(F)).astype(F) * F(lights["area_total"])).astype(F)
        dc = ((((c * mc).astype(F) * lights["emission"][i]).astype(F)) * g[:, None]).astype(F)
        tmax = (r * F(0.999)).astype(F)
    z = ~ok
    light = np.where(ok, i, -1).astype(np.int32)
    y, g, dc = np.where(z[:, None], F(0), y).astype(F), np.where(z, F(0), g).astype(F), np.where(z[:, None], F(0), dc).astype(F)
    assert y.dtype == F and g.dtype == F and dc.dtype == F and tmax.dtype == F and wn.dtype == F
    return dict(light=light, y=y, g=g, dc=dc, xo=xo, wn=wn, tmax=tmax)


def shadow(flat, xo, wn, tmax):
    """The shadow rays' decision from the oracle -> (occluded (m,), near tie (m,))."""
    if not len(xo):
        return np.zeros(0, bool), np.zeros(0, bool)
    dist, _, model = O.intersect_rays(flat, xo, wn, accel=1, threads=4)
    tmax = np.asarray(tmax, F)
    hit = model >= 0                             # a miss reports a large finite distance, not a hit at it
    with np.errstate(all="ignore"):
        near = hit & (np.abs(dist.astype(np.float64) - tmax.astype(np.float64)) <= NEAR_TIE * tmax.astype(np.float64))
    return hit & (dist < tmax), near


def segment_rays(orig, target):
    """pt_renderer_occluded's shadow ray of each segment -> (wn, tmax, has length)."""
    o, t = (np.ascontiguousarray(a, F).reshape(-1, 3) for a in (orig, target))
    with np.errstate(all="ignore"):
        w = (t - o).astype(F)
        r2 = _dot(w, w)
        wn = SR._normalize(w)
        tmax = (np.sqrt(r2).astype(F) * F(0.999)).astype(F)
    return wn, tmax, r2 > 0


def segments_occluded(flat, orig, target):
    """pt_renderer_occluded from the oracle -> (occluded, near tie); zero length reads unoccluded."""
    wn, tmax, has = segment_rays(orig, target)
    occ, near = np.zeros(len(has), bool), np.zeros(len(has), bool)
    sel = np.nonzero(has)[0]
    occ[sel], near[sel] = shadow(flat, np.ascontiguousarray(orig, F).reshape(-1, 3)[sel], wn[sel], tmax[sel])
    return occ, near


def combine(t, D, suppressed):
    """The sample per pixel and channel: t' = 0 where suppressed; (D == 0) ? t' : sqrt(t'*t' + D)."""
    tp = np.where(np.asarray(suppressed)[:, None], F(0), t).astype(F)
    with np.errstate(all="ignore"):
        lit = np.sqrt(((tp * tp).astype(F) + D).astype(F)).astype(F)
    return np.where(D == 0, tp, lit).astype(F)


class Restatement(GR.Restatement):
    """glass_ref.Restatement with pt_renderer_set_direct_light.  lights: the table (None:
    light_table(flat)); record: keep every sampled hit's inputs and results in self.records."""

    def __init__(self, *a, direct=True, lights=None, record=False, **kw):
        self.direct_on = bool(direct)
        self.record = record
        self.records = []
        self.near_tie_pixels = None
        self.shadow_rays = self.shadow_near = self.shadow_occluded = self.sampled = self.suppressed_hits = 0
        self._pix = None
        super().__init__(*a, **kw)
        self.lights = light_table(self.flat) if lights is None else lights
        self.near_tie_pixels = np.zeros(self.npix, bool)

    def set_direct_light(self, on=True):
        if bool(on) != self.direct_on:
            self.direct_on = bool(on)
            self.S = np.zeros((self.npix, 3), F)
            self.Q = np.zeros((self.npix, 3), F)
            self.counts[...] = 0

    def active(self):
        return self.direct_on and len(self.lights["cdf"]) > 0 and float(self.lights["area_total"]) > 0

    def iteration(self, it, mask=None):
        if not self.active():
            return super().iteration(it, mask)
        on = np.ones(self.counts.shape, bool) if mask is None else (np.asarray(mask) != 0)
        if not on.any():
            return super().iteration(it, mask)
        S0, Q0 = self.S, self.Q
        self.S, self.Q = np.zeros((self.npix, 3), F), np.zeros((self.npix, 3), F)
        self._pix = np.nonzero(on.reshape(-1)[self.tile_of[:self.n_launch]])[0].astype(np.int64)      # ascending
        self._prev = np.zeros(len(self._pix), bool)
        self._D = np.zeros((self.npix, 3), F)
        self._sup = np.zeros(self.npix, bool)
        try:
            super().iteration(it, mask)
        finally:
            self._pix = None
        c = combine(self.S, self._D, self._sup)
        self.S = S0 + c
        self.Q = Q0 + c * c

    def _shade_batch(self, it, slot, o, d, color, bounces, dist, nrm, model):
        if self._pix is None:
            return super()._shade_batch(it, slot, o, d, color, bounces, dist, nrm, model)
        pix = self._pix
        assert len(pix) == len(slot), "the batch is not the survivors of the batch before"
        model = np.asarray(model)
        hit = (model >= 0) & (np.asarray(bounces) > 0)
        mt = np.where(hit, self.mat_type[np.where(hit, model, 0)], -1)
        sup = hit & (mt == EMISSIVE) & self._prev
        self._sup[pix[sup]] = True
        self.suppressed_hits += int(sup.sum())
        diffuse = hit & (mt == DIFFUSE)
        sel = np.nonzero(diffuse)[0]
        if len(sel):
            so, sd, sdist, snrm, smodel = (np.ascontiguousarray(np.asarray(a)[sel]) for a in (o, d, dist, nrm, model))
            n = SR.shading_normals(self.flat, self.tables, self.smooth, so, sd, sdist, snrm, smodel, self.ident)[0]
            mc = self.albedo(so, sd, sdist, snrm, smodel)
            sslot, sb = np.asarray(slot)[sel], np.asarray(bounces)[sel]
            sc = np.array(color[sel], F, copy=True)
            s = sample(self.lights, so, sd, sdist, n, mc, sc, *uniforms(it, sslot, sb))
            ok = np.nonzero(s["light"] >= 0)[0]
            occ, near = shadow(self.flat, s["xo"][ok], s["wn"][ok], s["tmax"][ok])
            vis = np.zeros(len(sel), bool)
            vis[ok] = ~occ
            tie = np.zeros(len(sel), bool)
            tie[ok] = near
            self.sampled += len(sel)
            self.shadow_rays += len(ok)
            self.shadow_near += int(near.sum())
            self.shadow_occluded += int(occ.sum())
            self.near_tie_pixels[pix[sel][tie]] = True
            p = pix[sel][vis]                                  # a pixel owns one ray: no index repeats
            self._D[p] = (self._D[p] + s["dc"][vis]).astype(F)
            if self.record:
                self.records.append(dict(it=np.full(len(sel), it, np.int32), slot=sslot.astype(np.int32), bounces=sb.astype(np.int32),
                                         o=so, d=sd, dist=sdist, nrm=snrm, model=smodel.astype(np.int32), color=sc, n=n, mc=mc,
                                         light=s["light"], y=s["y"], g=s["g"], dc=s["dc"], visible=vis, near=tie,
                                         pixel=pix[sel].astype(np.int32)))
        super()._shade_batch(it, slot, o, d, color, bounces, dist, nrm, model)
        keep = np.asarray(bounces) > 0
        self._pix = pix[keep]
        self._prev = diffuse[keep]
