"""numpy restatement of albedo textures (test infrastructure; include/pathtracer_amd.h,
pt_scene_set_model_texture): the albedo mc of a hit on a textured model, operation by operation
in float32, and smooth_ref.Restatement with one change after the oracle's ptor_shade: a hit with
bounces left on a textured model whose material multiplies by the model colour (DIFFUSE, METAL,
COAT, EMISSIVE, REFLECTIVE) has colour = colour before the shade * mc.  That is exact: the
shade's only use of the model colour is that one multiply per channel.  Nothing else changes, so
with no textured model this is the parent restatement (tests/test_texture_ref.py holds it to
that and to the oracle).

The triangle of a hit comes from smooth_ref's identification (nearest flat normal, NEAR / FAR
asserted on every hit), run over the textured models; a model that is only textured keeps its
flat normal."""
import numpy as np

import smooth_ref as SR

F = np.float32
_dot = SR._dot
MULTIPLYING = (0, 2, 4, 5, 6)          # DIFFUSE, REFLECTIVE, EMISSIVE, COAT, METAL (Primitive.h:70-79)


def barycentrics(w2m, v0, e1, e2, o, d, dist):
    """b0, b1, b2 of pt_scene_set_model_smooth's definition (smooth_ref.smooth_normal's lines)."""
    o, d = (np.ascontiguousarray(a, F) for a in (o, d))
    dist = np.ascontiguousarray(dist, F)
    with np.errstate(all="ignore"):
        dr = SR._normalize(d)
        ip = (o + (dr * dist[:, None]).astype(F)).astype(F)
        pm = SR.xform_point(w2m, ip)
        q = (pm - v0).astype(F)
        d11, d12, d22, q1, q2 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(q, e1), _dot(q, e2)
        den = ((d11 * d22).astype(F) - (d12 * d12).astype(F)).astype(F)
        b1 = (((d22 * q1).astype(F) - (d12 * q2).astype(F)).astype(F) / den).astype(F)
        b2 = (((d11 * q2).astype(F) - (d12 * q1).astype(F)).astype(F) / den).astype(F)
        b1 = np.fmin(np.fmax(b1, F(0)), F(1)).astype(F)
        b2 = np.fmin(np.fmax(b2, F(0)), (F(1) - b1).astype(F)).astype(F)
        b0 = ((F(1) - b1).astype(F) - b2).astype(F)
    return b0, b1, b2


def interpolate_uv(uv0, uv1, uv2, b0, b1, b2):
    """uv_k = (uv0_k*b0 + uv1_k*b1) + uv2_k*b2: (m, 2) float32."""
    with np.errstate(all="ignore"):
        return (((uv0 * b0[:, None]).astype(F) + (uv1 * b1[:, None]).astype(F)).astype(F)
                + (uv2 * b2[:, None]).astype(F)).astype(F)


def axis(a, n):
    """One axis of the lookup: coordinate a (m,) float32 on n texels -> (i0, i1, t)."""
    a = np.ascontiguousarray(a, F)
    with np.errstate(all="ignore"):
        fr = (a - np.floor(a).astype(F)).astype(F)
        f = ((fr * F(n)).astype(F) - F(0.5)).astype(F)
        f = np.fmin(np.fmax(f, F(-0.5)), F(F(n) - F(0.5))).astype(F)      # fmaxf / fminf: a NaN gives way
        fl = np.floor(f).astype(F)
        t = (f - fl).astype(F)
    i0 = fl.astype(np.int64)
    i0 = np.where(i0 < 0, i0 + n, i0)
    i1 = i0 + 1
    i1 = np.where(i1 >= n, i1 - n, i1)
    return i0, i1, t


def lookup(tex, uv):
    """The bilinear value v of texture tex (h, w, 3) float32 at uv (m, 2) float32: (m, 3) float32."""
    tex = np.asarray(tex, F)
    h, w = tex.shape[:2]
    x0, x1, tx = axis(uv[:, 0], w)
    y0, y1, ty = axis(uv[:, 1], h)
    tx, ty = tx[:, None], ty[:, None]
    c00, c01, c10, c11 = tex[y0, x0], tex[y0, x1], tex[y1, x0], tex[y1, x1]
    top = (c00 + ((c01 - c00).astype(F) * tx).astype(F)).astype(F)
    bot = (c10 + ((c11 - c10).astype(F) * tx).astype(F)).astype(F)
    out = (top + ((bot - top).astype(F) * ty).astype(F)).astype(F)
    assert out.dtype == F
    return out


def lookup64(tex, uv):
    """The same formula in float64 from the same float32 inputs (what the float32 one is measured against)."""
    tex = np.asarray(tex, F).astype(np.float64)
    uv = np.asarray(uv, F).astype(np.float64)
    h, w = tex.shape[:2]
    out = []
    for a, n in ((uv[:, 0], w), (uv[:, 1], h)):
        fr = a - np.floor(a)
        f = np.clip(fr * n - 0.5, -0.5, n - 0.5)
        fl = np.floor(f)
        i0 = fl.astype(np.int64)
        i0 = np.where(i0 < 0, i0 + n, i0)
        i1 = np.where(i0 + 1 >= n, i0 + 1 - n, i0 + 1)
        out.append((i0, i1, (f - fl)[:, None]))
    (x0, x1, tx), (y0, y1, ty) = out
    top = tex[y0, x0] + (tex[y0, x1] - tex[y0, x0]) * tx
    bot = tex[y1, x0] + (tex[y1, x1] - tex[y1, x0]) * tx
    return top + (bot - top) * ty


class UvTables:
    """Per model of a FlatScene with per-vertex uv (nv, 2): its triangles' three vertex uvs."""

    def __init__(self, flat, uv):
        self.flat, self.uv, self.tri = flat, np.asarray(uv, F), {}

    def of(self, model):
        if model not in self.tri:
            f = self.flat
            mesh = int(f.model_ints[model, 0])
            ts, te = int(f.mesh_ranges[mesh, 2]), int(f.mesh_ranges[mesh, 3])
            t = np.asarray(f.tris, np.int32)[ts:te]
            self.tri[model] = (self.uv[t[:, 0]], self.uv[t[:, 1]], self.uv[t[:, 2]])
        return self.tri[model]


def albedo_of_triangles(flat, tables, uvt, textures, binding, o, d, dist, model, tri):
    """mc for hits whose scene triangle is known (tri; -1 where model < 0): the model colour, times
    the texture's value on a textured model; (0, 0, 0) for model < 0."""
    model, tri = np.asarray(model), np.asarray(tri)
    out = np.zeros((len(model), 3), F)
    color = np.asarray(flat.model_color, F)
    for k in np.unique(model[model >= 0]):
        sel = np.nonzero(model == k)[0]
        out[sel] = color[k]
        if binding[k] < 0:
            continue
        T = tables.of(int(k))
        t = tri[sel] - T["first"]
        b0, b1, b2 = barycentrics(np.asarray(flat.model_w2m, F)[k], T["v0"][t], T["e1"][t], T["e2"][t],
                                  np.asarray(o, F)[sel], np.asarray(d, F)[sel], np.asarray(dist, F)[sel])
        u0, u1, u2 = uvt.of(int(k))
        v = lookup(textures[binding[k]], interpolate_uv(u0[t], u1[t], u2[t], b0, b1, b2))
        out[sel] = (color[k][None, :] * v).astype(F)
    return out


class Restatement(SR.Restatement):
    """smooth_ref.Restatement with albedo textures.  uv: (nv, 2) per-vertex uv (Scene.export()["uv"]);
    textures: a list of (h, w, 3) arrays; binding: a texture index per model, -1 for none (None: none)."""

    def __init__(self, flat, cfg, width=None, camera=None, env=None, smooth=None, uv=None, textures=(), binding=None):
        nmodel = len(flat.model_ints)
        self.binding = np.full(nmodel, -1, np.int64) if binding is None else np.asarray(binding, np.int64).reshape(nmodel)
        self.textures = [np.asarray(t, F) for t in textures]
        self.textured = self.binding >= 0
        assert (self.binding < len(self.textures)).all()
        self.uvt = UvTables(flat, np.zeros((len(flat.vpos), 2), F) if uv is None else uv)
        self.tex_ident = SR.Identification()
        self.tex_hits = 0                                  # hits whose colour a texture decided
        super().__init__(flat, cfg, width, camera, env, smooth)

    def albedo(self, o, d, dist, nrm, model):
        """mc for the oracle's hits (dist, nrm, model) of the rays (o, d)."""
        tri = SR.shading_normals(self.flat, self.tables, self.textured, o, d, dist, nrm, model, self.tex_ident)[1]
        return albedo_of_triangles(self.flat, self.tables, self.uvt, self.textures, self.binding, o, d, dist, model, tri)

    def primary_albedo(self):
        """pt_renderer_primary_albedo of the current view: (npix, 3), zero for a miss and past n_launch."""
        o = np.repeat(np.asarray(self.cam, F)[None, :], self.npix, axis=0)
        out = self.albedo(o, self.dirs, self.hit_dist, self.hit_nrm, self.hit_model)
        out[self.n_launch:] = 0
        return out

    def _shade_batch(self, it, slot, o, d, color, bounces, dist, nrm, model):
        if not self.textured.any():
            return super()._shade_batch(it, slot, o, d, color, bounces, dist, nrm, model)
        model = np.asarray(model)
        hit = model >= 0
        safe = np.where(hit, model, 0)
        takes = hit & (bounces > 0) & self.textured[safe] & np.isin(self.mat_type[safe], MULTIPLYING)
        saved = color.copy()
        mc = self.albedo(o, d, dist, nrm, np.where(takes, model, -1))       # before the shade moves o and d
        super()._shade_batch(it, slot, o, d, color, bounces, dist, nrm, model)
        color[takes] = (saved[takes] * mc[takes]).astype(F)
        self.tex_hits += int(takes.sum())
