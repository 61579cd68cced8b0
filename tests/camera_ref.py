"""numpy / ctypes restatement of the free camera with a thin lens (test infrastructure;
include/pathtracer_amd.h, pt_renderer_set_camera), a subclass of jitter_ref.Restatement
built on the same oracle primitives: ptor_u01_first, ptor_sinf, ptor_cosf for the rays,
ptor_intersect_rays and ptor_shade for what follows.

With a camera set the cached primary hits are ptor_intersect_rays of the pinhole rays
through every pixel's own point.  A pinhole with the jitter off renders adaptive_ref's
cached iteration over those rays and hits; with the jitter on or a lens an iteration is
jitter_ref's generation iteration over the camera's rays.  Without a camera everything
is jitter_ref's.  set_camera starts a new render (S, Q and the tile counts read zero)
and, like the device, leaves the segment counters running."""
from dataclasses import dataclass

import numpy as np

import jitter_ref as JR
import oracle as O

F = np.float32
VECS = ("origin", "p0", "du", "dv", "lens_u", "lens_v")


@dataclass
class Cam:
    """pt_camera in float32.  Cam.of(x) copies any object with pt_camera's fields."""
    origin: np.ndarray
    p0: np.ndarray
    du: np.ndarray
    dv: np.ndarray
    lens_u: np.ndarray
    lens_v: np.ndarray
    lens_radius: np.float32

    @classmethod
    def of(cls, c):
        return cls(*(np.array([float(v) for v in getattr(c, n)], np.float64).astype(F) for n in VECS),
                   F(c.lens_radius))


def legacy_camera(cfg):
    """The general camera whose rays are the legacy camera's (cfg: anything with
    RenderConfig's fields): origin = cam, p0 = (plane_x0, plane_y0, plane_z),
    du = ((float)(plane_w / W), 0, 0), dv = (0, (float)(plane_h / H), 0)."""
    z = F(0)
    return Cam(origin=np.array(cfg.cam, np.float64).astype(F),
               p0=np.array([cfg.plane_x0, cfg.plane_y0, cfg.plane_z], np.float64).astype(F),
               du=np.array([F(cfg.plane_w / cfg.width), z, z], F), dv=np.array([z, F(cfg.plane_h / cfg.height), z], F),
               lens_u=np.array([1, 0, 0], F), lens_v=np.array([0, 1, 0], F), lens_radius=F(0))


def plane_points(cam, fx, fy):
    """t_k = (p0_k + fx*du_k) + fy*dv_k in float32, products rounded before the adds; (n, 3)."""
    fx, fy = np.asarray(fx, F), np.asarray(fy, F)
    cols = []
    for k in range(3):
        a = (fx * cam.du[k]).astype(F)
        b = (fy * cam.dv[k]).astype(F)
        cols.append(((cam.p0[k] + a).astype(F) + b).astype(F))
    return np.stack(cols, axis=1)


def lens_uniforms(it, pix, max_bounces):
    """(u1, u2) float32: the first uniforms of the engines seeded (it, p, max_bounces + 3 / + 4)."""
    u01 = O.lib().ptor_u01_first
    u1 = np.array([u01(int(it), int(p), max_bounces + 3) for p in pix], F)
    u2 = np.array([u01(int(it), int(p), max_bounces + 4) for p in pix], F)
    return u1, u2


def lens_origins(cam, u1, u2):
    """o_k = (origin_k + a*lens_u_k) + b*lens_v_k with rr = R * sqrtf(u1), phi = 6.2831855f * u2,
    a = rr * cosf(phi), b = rr * sinf(phi); (n, 3) float32."""
    L = O.lib()
    u1, u2 = np.asarray(u1, F), np.asarray(u2, F)
    rr = (cam.lens_radius * np.sqrt(u1).astype(F)).astype(F)
    phi = (F(6.2831855) * u2).astype(F)
    c = np.array([L.ptor_cosf(float(v)) for v in phi], F)
    s = np.array([L.ptor_sinf(float(v)) for v in phi], F)
    a, b = (rr * c).astype(F), (rr * s).astype(F)
    cols = []
    for k in range(3):
        au = (a * cam.lens_u[k]).astype(F)
        bv = (b * cam.lens_v[k]).astype(F)
        cols.append(((cam.origin[k] + au).astype(F) + bv).astype(F))
    return np.stack(cols, axis=1)


def camera_rays(cam, cfg, it, pix, width=None):
    """(o, d) float32 of the camera rays of pixels `pix` in iteration `it`: through the
    pixel's own point (width None) or the jittered one, from the lens when it has one."""
    pix = np.asarray(pix)
    if width is None:
        y, x = np.divmod(pix, cfg.width)
        fx, fy = x.astype(F), y.astype(F)
    else:
        fx, fy = JR.jitter_points(cfg, it, pix, width)
    t = plane_points(cam, fx, fy)
    if cam.lens_radius > 0:
        o = lens_origins(cam, *lens_uniforms(it, pix, cfg.max_bounces))
    else:
        o = np.repeat(cam.origin[None, :], len(pix), axis=0).astype(F)
    return np.ascontiguousarray(o, F), np.ascontiguousarray((t - o).astype(F), F)


def pinhole(cam):
    return Cam(cam.origin, cam.p0, cam.du, cam.dv, cam.lens_u, cam.lens_v, F(0))


def centre_hits(flat, cfg, cam):
    """The primary-hit cache under `cam`: ptor_intersect_rays of the pinhole rays through
    every pixel's own point -> (origin (3,), dirs (npix, 3), dist, normal, model)."""
    o, d = camera_rays(pinhole(cam), cfg, 0, np.arange(cfg.width * cfg.height))
    dist, nrm, model = O.intersect_rays(flat, o, d, accel=cfg.accel, threads=4)
    return cam.origin.copy(), d, dist, nrm, model


class Restatement(JR.Restatement):
    """jitter_ref.Restatement with pt_renderer_set_camera; camera: a Cam, or None for the
    legacy camera."""

    def __init__(self, flat, cfg, width=None, camera=None):
        super().__init__(flat, cfg, width)
        self._legacy = (self.cam, self.dirs, self.hit_dist, self.hit_nrm, self.hit_model)
        self.camera = None
        if camera is not None:
            self.set_camera(camera)

    def set_camera(self, camera):
        self.camera = camera
        if camera is None:
            self.cam, self.dirs, self.hit_dist, self.hit_nrm, self.hit_model = self._legacy
        else:
            self.cam, self.dirs, self.hit_dist, self.hit_nrm, self.hit_model = centre_hits(self.flat, self.cfg, camera)
        # pt_renderer_clear_image: the accumulators and the sample counts, not the segment counters
        self.S = np.zeros((self.npix, 3), F)
        self.Q = np.zeros((self.npix, 3), F)
        self.counts[...] = 0

    def generated(self):
        """Does the next iteration generate its rays (the jittered iteration's path)?"""
        return self.jitter_on or (self.camera is not None and self.camera.lens_radius > 0)

    def iteration(self, it, mask=None):
        if self.camera is None:
            return super().iteration(it, mask)
        if not self.generated():
            # adaptive_ref's cached iteration over self.cam / dirs / hit_*, which are the camera's
            on, self.jitter_on = self.jitter_on, False
            try:
                return super().iteration(it, mask)
            finally:
                self.jitter_on = on
        on = np.ones(self.counts.shape, bool) if mask is None else (np.asarray(mask) != 0)
        assert on.shape == self.counts.shape
        if not on.any():
            return
        pix = np.nonzero(on.reshape(-1)[self.tile_of[:self.n_launch]])[0].astype(np.int32)    # ascending
        n = len(pix)
        o, d = camera_rays(self.camera, self.cfg, it, pix, self.jitter_width if self.jitter_on else None)
        color = np.ones((n, 3), F)
        bounces = np.full(n, self.cfg.max_bounces, np.int32)
        c = np.zeros((self.npix, 3), F)
        live = []
        while len(pix):
            live.append(len(pix))
            slot = np.arange(len(pix), dtype=np.int32)
            dist, nrm, model = O.intersect_rays(self.flat, o, d, accel=self.cfg.accel, threads=4)
            self._shade_batch(it, slot, o, d, color, bounces, dist, nrm, model)
            dead = bounces <= 0
            c[pix[dead]] = np.sqrt(color[dead])
            keep = ~dead
            pix, o, d, color, bounces = (np.ascontiguousarray(a[keep]) for a in (pix, o, d, color, bounces))
        self.S = self.S + c
        self.Q = self.Q + c * c
        self.counts[on] += 1
        self.segments += self.n_launch + sum(live)
        self.live.append(live)
        self._count([self.n_launch] + live)
