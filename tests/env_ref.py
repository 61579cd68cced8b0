"""numpy restatement of environment lighting (test infrastructure; include/pathtracer_amd.h,
pt_renderer_set_environment): the octahedral lookup, operation by operation in float32, and
camera_ref.Restatement with one override after the oracle's ptor_shade: a ray that missed
ends with colour = (its colour before the shade) * lookup(its direction) instead of * 0.01.
Nothing else changes: the same rays survive with the same slots, so the counts and the
segments are the parent's (tests/test_env_ref.py holds this file to the oracle)."""
import numpy as np

import camera_ref as CR

F = np.float32


class Env:
    """pt_environment in float32: tex (n, n, 3), scale (3,), rot (3, 3) row-major."""

    def __init__(self, tex, scale=(1, 1, 1), rot=None):
        self.tex = np.ascontiguousarray(tex, F)
        assert self.tex.ndim == 3 and self.tex.shape[0] == self.tex.shape[1] and self.tex.shape[2] == 3
        self.scale = np.asarray(scale, np.float64).astype(F).reshape(3)
        self.rot = np.eye(3, dtype=F) if rot is None else np.asarray(rot, np.float64).astype(F).reshape(3, 3)

    @classmethod
    def of(cls, e):
        """From anything with texels / scale / rotation (pathtracerap_amd.Environment)."""
        return cls(e.texels, e.scale, e.rotation)


def _dot(a, b):
    """pt_math.h dot: (x*x' + y*y') + z*z', every product and sum rounded to float32."""
    t = [(a[..., k] * b[..., k]).astype(F) for k in range(3)]
    return ((t[0] + t[1]).astype(F) + t[2]).astype(F)


def _axis(p, n):
    f = (((p * F(0.5)).astype(F) + F(0.5)).astype(F) * F(n)).astype(F) - F(0.5)
    f = np.fmin(np.fmax(f.astype(F), F(0)), F(n - 1)).astype(F)       # fmaxf / fminf: a NaN gives way
    i0 = f.astype(np.int32)
    i1 = np.minimum(i0 + 1, n - 1)
    return i0, i1, (f - i0.astype(F)).astype(F)


def lookup(tex, rot, scale, d):
    """The radiance from directions d (m, 3) float32 (any length): texel times scale, (m, 3)."""
    tex, rot, scale = np.asarray(tex, F), np.asarray(rot, F).reshape(3, 3), np.asarray(scale, F).reshape(3)
    d = np.ascontiguousarray(d, F).reshape(-1, 3)
    n = tex.shape[0]
    with np.errstate(all="ignore"):
        s = (F(1) / np.sqrt(_dot(d, d)).astype(F)).astype(F)
        u = (d * s[:, None]).astype(F)
        e = np.stack([_dot(np.broadcast_to(rot[k], u.shape), u) for k in range(3)], axis=1)
        a = np.abs(e)
        l = ((a[:, 0] + a[:, 1]).astype(F) + a[:, 2]).astype(F)
        px, py = (e[:, 0] / l).astype(F), (e[:, 1] / l).astype(F)
        qx = ((F(1) - np.abs(py)).astype(F) * np.where(px >= 0, F(1), F(-1))).astype(F)
        qy = ((F(1) - np.abs(px)).astype(F) * np.where(py >= 0, F(1), F(-1))).astype(F)
        low = e[:, 2] < 0
        px, py = np.where(low, qx, px).astype(F), np.where(low, qy, py).astype(F)
        x0, x1, tx = _axis(px, n)
        y0, y1, ty = _axis(py, n)
    tx, ty = tx[:, None], ty[:, None]
    top = (tex[y0, x0] + ((tex[y0, x1] - tex[y0, x0]).astype(F) * tx).astype(F)).astype(F)
    bot = (tex[y1, x0] + ((tex[y1, x1] - tex[y1, x0]).astype(F) * tx).astype(F)).astype(F)
    v = (top + ((bot - top).astype(F) * ty).astype(F)).astype(F)
    out = (v * scale[None, :]).astype(F)
    assert out.dtype == F
    return out


def sky_texels(zenith, horizon, ground, n):
    """pt_environment_sky restated: (n, n, 3) float32."""
    z, h, g = (np.asarray(v, np.float64).astype(F).reshape(3) for v in (zenith, horizon, ground))
    p = ((((np.arange(n).astype(F) + F(0.5)).astype(F) / F(n)).astype(F) * F(2)).astype(F) - F(1)).astype(F)
    px, py = np.meshgrid(p, p)
    ez = ((F(1) - np.abs(px)).astype(F) - np.abs(py)).astype(F)
    low = ez < 0
    ex = np.where(low, ((F(1) - np.abs(py)).astype(F) * np.where(px >= 0, F(1), F(-1))).astype(F), px).astype(F)
    ey = np.where(low, ((F(1) - np.abs(px)).astype(F) * np.where(py >= 0, F(1), F(-1))).astype(F), py).astype(F)
    vec = np.stack([ex, ey, ez], axis=-1)
    uz = (ez * (F(1) / np.sqrt(_dot(vec, vec)).astype(F)).astype(F)).astype(F)
    up = (h + ((z - h).astype(F) * uz[..., None]).astype(F)).astype(F)
    return np.where(low[..., None], g, up).astype(F)


class Restatement(CR.Restatement):
    """camera_ref.Restatement with pt_renderer_set_environment; env: an Env or None."""

    def __init__(self, flat, cfg, width=None, camera=None, env=None):
        super().__init__(flat, cfg, width, camera)
        self.env = env
        self.misses = np.zeros(64, np.int64)      # rays that missed, by depth (0: the primary ray)

    def set_environment(self, env):
        """A new environment is a new render: S, Q and the counts read zero; the segment counters run on."""
        self.env = env
        self.S = np.zeros((self.npix, 3), F)
        self.Q = np.zeros((self.npix, 3), F)
        self.counts[...] = 0

    def _shade_batch(self, it, slot, o, d, color, bounces, dist, nrm, model):
        saved_c, saved_d = color.copy(), d.copy()
        depth = self.cfg.max_bounces - bounces                 # before the shade: 0 for a camera ray
        super()._shade_batch(it, slot, o, d, color, bounces, dist, nrm, model)
        miss = np.asarray(model) < 0
        np.add.at(self.misses, depth[miss], 1)
        if self.env is not None and miss.any():
            color[miss] = (saved_c[miss] * lookup(self.env.tex, self.env.rot, self.env.scale, saved_d[miss])).astype(F)
