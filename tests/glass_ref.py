"""numpy restatement of the dielectric material (test infrastructure; include/pathtracer_amd.h,
"Dielectric material"): the definition operation by operation in float32, every intermediate
cast, and texture_ref.Restatement with one change around the oracle's ptor_shade: a hit with
bounces left on a DIELECTRIC model is shaded as SPECULAR (the oracle's shade then leaves its
origin, direction and colour alone and takes one bounce, which tests/test_reference_code.py
holds) and its origin, direction and colour are then written from the definition.  The shading
normal and the albedo of those hits are taken before the shade moves the rays, as texture_ref
takes its albedo.  With no dielectric model this is the parent restatement
(tests/test_glass_ref.py holds it to that)."""
import numpy as np

import oracle as O
import smooth_ref as SR
import texture_ref as TR

F = np.float32
_dot = SR._dot
DIELECTRIC, SPECULAR = 7, 1
REFRACT_IN, REFRACT_OUT, REFLECT, TIR = 0, 1, 2, 3
EVENT_NAMES = ("refract_in", "refract_out", "reflect", "tir")


def scatter(dirn, n, ior, u):
    """The definition for m hits: dirn (m, 3) normalised directions, n (m, 3) shading normals,
    ior (m,), u (m,) the draw.  -> dict(d (m, 3), nn (m, 3), event (m,), fr (m,), k (m,)); fr
    is NaN under total internal reflection."""
    dirn, n = np.ascontiguousarray(dirn, F).reshape(-1, 3), np.ascontiguousarray(n, F).reshape(-1, 3)
    m = len(dirn)
    ior = np.ascontiguousarray(np.broadcast_to(np.asarray(ior, F), (m,)))
    u = np.ascontiguousarray(np.broadcast_to(np.asarray(u, F), (m,)))
    with np.errstate(all="ignore"):
        ci = _dot(dirn, n)
        ent = ci < F(0)
        nn = np.where(ent[:, None], n, -n).astype(F)
        c = np.where(ent, -ci, ci).astype(F)
        c = np.fmin(c, F(1)).astype(F)
        eta = np.where(ent, (F(1) / ior).astype(F), ior).astype(F)
        k = (F(1) - ((eta * eta).astype(F) * (F(1) - (c * c).astype(F)).astype(F)).astype(F)).astype(F)
        a = ((F(1) - ior).astype(F) / (F(1) + ior).astype(F)).astype(F)
        r0 = (a * a).astype(F)
        tir = k < F(0)
        sk = np.sqrt(np.where(tir, F(0), k)).astype(F)
        x = (F(1) - np.where(ent, c, sk)).astype(F)
        x2 = (x * x).astype(F)
        x5 = ((x2 * x2).astype(F) * x).astype(F)
        fr = (r0 + ((F(1) - r0).astype(F) * x5).astype(F)).astype(F)
        reflect = tir | (u < fr)
        event = np.where(tir, TIR, np.where(reflect, REFLECT, np.where(ent, REFRACT_IN, REFRACT_OUT))).astype(np.int32)
        d_refl = (dirn + (nn * (F(2) * c).astype(F)[:, None]).astype(F)).astype(F)
        d_refr = ((dirn * eta[:, None]).astype(F)
                  + (nn * ((eta * c).astype(F) - sk).astype(F)[:, None]).astype(F)).astype(F)
    d = np.where(reflect[:, None], d_refl, d_refr).astype(F)
    assert d.dtype == F and nn.dtype == F and k.dtype == F and fr.dtype == F
    return dict(d=d, nn=nn, event=event, fr=np.where(tir, F(np.nan), fr).astype(F), k=k)


def scatter64(dirn, n, ior):
    """The same formulas in float64 from the same float32 inputs, both branches:
    dict(k, tir, fr, d_reflect, d_refract) (fr and d_refract NaN under total internal reflection)."""
    dirn, n = np.asarray(dirn, F).astype(np.float64), np.asarray(n, F).astype(np.float64)
    ior = np.broadcast_to(np.asarray(ior, F), (len(dirn),)).astype(np.float64)
    with np.errstate(all="ignore"):
        ci = (dirn * n).sum(axis=1)
        ent = ci < 0
        nn = np.where(ent[:, None], n, -n)
        c = np.minimum(np.abs(ci), 1.0)
        eta = np.where(ent, 1.0 / ior, ior)
        k = 1.0 - eta * eta * (1.0 - c * c)
        r0 = ((1.0 - ior) / (1.0 + ior)) ** 2
        sk = np.sqrt(k)
        x = 1.0 - np.where(ent, c, sk)
        fr = r0 + (1.0 - r0) * x ** 5
        d_refl = dirn + nn * (2.0 * c)[:, None]
        d_refr = dirn * eta[:, None] + nn * (eta * c - sk)[:, None]
    return dict(k=k, tir=k < 0, fr=fr, d_reflect=d_refl, d_refract=d_refr, ent=ent, nn=nn, eta=eta)


def hook(dirs, normals, ior, u):
    """What pt_selftest_dielectric computes: dirs normalised first, as the shading does."""
    with np.errstate(all="ignore"):
        dn = SR._normalize(np.ascontiguousarray(dirs, F).reshape(-1, 3))
    r = scatter(dn, normals, ior, u)
    return r["d"], r["event"]


def u01_first(it, slot, bounces):
    """The first uniform of the engine seeded (it, slot, bounces) per ray (ptor_u01_first)."""
    fn = O.lib().ptor_u01_first
    return np.array([fn(int(it), int(s), int(b)) for s, b in zip(slot, bounces)], F)


class Restatement(TR.Restatement):
    """texture_ref.Restatement with the dielectric material.  ior: one value per model (None:
    1.5 each), read only for the models whose exported material is DIELECTRIC."""

    def __init__(self, flat, cfg, width=None, camera=None, env=None, smooth=None, uv=None, textures=(), binding=None,
                 ior=None):
        nmodel = len(flat.model_ints)
        self.ior = np.full(nmodel, 1.5, F) if ior is None else np.asarray(ior, F).reshape(nmodel)
        self.events = np.zeros(4, np.int64)        # by event code
        self.smooth_exits = 0                      # refractions leaving a smooth model
        super().__init__(flat, cfg, width, camera, env, smooth, uv, textures, binding)
        self.glass = self.mat_type == DIELECTRIC
        # what the oracle's shade is given for those models: it then only takes a bounce
        self.mat_type = np.where(self.glass, SPECULAR, self.mat_type).astype(np.int32)

    def _shade_batch(self, it, slot, o, d, color, bounces, dist, nrm, model):
        if not self.glass.any():
            return super()._shade_batch(it, slot, o, d, color, bounces, dist, nrm, model)
        model = np.asarray(model)
        hit = model >= 0
        safe = np.where(hit, model, 0)
        takes = hit & (bounces > 0) & self.glass[safe]
        sel = np.nonzero(takes)[0]
        if len(sel):
            so, sd, sdist, snrm, smodel = (np.ascontiguousarray(np.asarray(a)[sel]) for a in (o, d, dist, nrm, model))
            n = SR.shading_normals(self.flat, self.tables, self.smooth, so, sd, sdist, snrm, smodel, self.ident)[0]
            mc = self.albedo(so, sd, sdist, snrm, smodel)
            with np.errstate(all="ignore"):
                dirn = SR._normalize(sd.astype(F))
                ip = (so + (dirn * sdist.astype(F)[:, None]).astype(F)).astype(F)
            r = scatter(dirn, n, self.ior[smodel], u01_first(it, np.asarray(slot)[sel], bounces[sel]))
            off = (r["nn"] * F(0.1)).astype(F)
            refl = r["event"] >= REFLECT
            new_o = np.where(refl[:, None], (ip + off).astype(F), (ip - off).astype(F)).astype(F)
            tint = r["event"] == REFRACT_IN
            new_c = np.where(tint[:, None], (color[sel] * mc).astype(F), color[sel]).astype(F)
            self.events += np.bincount(r["event"], minlength=4)
            self.smooth_exits += int(((r["event"] == REFRACT_OUT) & self.smooth[smodel]).sum())
        super()._shade_batch(it, slot, o, d, color, bounces, dist, nrm, model)
        if len(sel):
            o[sel], d[sel], color[sel] = new_o, r["d"], new_c
