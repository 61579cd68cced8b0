"""numpy / ctypes restatement of pixel-jittered iterations (test infrastructure;
include/pathtracer_amd.h, pt_renderer_set_pixel_jitter), a subclass of
adaptive_ref.Restatement built on the same oracle primitives plus ptor_u01_first.

One jittered iteration: every launched pixel of an active tile, in ascending order, gets
a camera ray through (x + w*(ux - 0.5), y + w*(uy - 0.5)) with ux, uy the first uniforms
of the engines seeded (iteration, pixel, max_bounces + 1) and (.., max_bounces + 2).  The
rays are intersected with ptor_intersect_rays (nothing is cached), shaded with RNG slot =
rank, and from there on the loop is adaptive_ref's.  Segments: launched pixels + emitted
rays + later live rays.  With the jitter off an iteration is adaptive_ref's, so one
object restates any sequence of jittered and unjittered, plain and masked iterations."""
import numpy as np

import adaptive_ref as AR
import oracle as O

F = np.float32


def jitter_offsets(it, pix, max_bounces):
    """(ux, uy) float32 of the pixels `pix` in iteration `it`."""
    u01 = O.lib().ptor_u01_first
    ux = np.array([u01(int(it), int(p), max_bounces + 1) for p in pix], F)
    uy = np.array([u01(int(it), int(p), max_bounces + 2) for p in pix], F)
    return ux, uy


def jitter_points(cfg, it, pix, width):
    """(fx, fy) float32: the point of each pixel, in pixel units, its ray goes through."""
    y, x = np.divmod(np.asarray(pix), cfg.width)
    ux, uy = jitter_offsets(it, pix, cfg.max_bounces)
    w = F(width)
    fx = (x.astype(F) + (w * (ux - F(0.5))).astype(F)).astype(F)
    fy = (y.astype(F) + (w * (uy - F(0.5))).astype(F)).astype(F)
    return fx, fy


def jitter_dirs(cfg, it, pix, width):
    """Unnormalised float32 directions of the jittered camera rays of `pix`."""
    fx, fy = jitter_points(cfg, it, pix, width)
    cam = np.array(cfg.cam, np.float64).astype(F)
    step_x, step_y = F(cfg.plane_w / cfg.width), F(cfg.plane_h / cfg.height)
    wx = (cfg.plane_x0 + (fx * step_x).astype(F).astype(np.float64)).astype(F)
    wy = (cfg.plane_y0 + (fy * step_y).astype(F).astype(np.float64)).astype(F)
    wz = np.full(len(fx), F(cfg.plane_z), F)
    return (np.stack([wx, wy, wz], axis=1) - cam[None, :]).astype(F)


class Restatement(AR.Restatement):
    """adaptive_ref.Restatement with pt_renderer_set_pixel_jitter.  `live` of a jittered
    iteration starts with the emitted rays (the rays entering bounce 1)."""

    def __init__(self, flat, cfg, width=None):
        super().__init__(flat, cfg)
        self.jitter_on, self.jitter_width = width is not None, 1.0 if width is None else float(width)

    def clear(self):
        super().clear()
        self.per_bounce = np.zeros(64, np.int64)      # pt_renderer_segments_per_bounce

    def set_pixel_jitter(self, width=1.0, on=True):
        self.jitter_on, self.jitter_width = bool(on), float(width)

    def iteration(self, it, mask=None):
        if not self.jitter_on:
            before = len(self.live)
            super().iteration(it, mask)
            if len(self.live) > before:
                self._count([self.n_launch] + self.live[-1])
            return
        on = np.ones(self.counts.shape, bool) if mask is None else (np.asarray(mask) != 0)
        assert on.shape == self.counts.shape
        if not on.any():
            return
        pix = np.nonzero(on.reshape(-1)[self.tile_of[:self.n_launch]])[0].astype(np.int32)    # ascending
        n = len(pix)
        o = np.ascontiguousarray(np.repeat(self.cam[None, :], n, axis=0), F)
        d = np.ascontiguousarray(jitter_dirs(self.cfg, it, pix, self.jitter_width), F)
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

    def _count(self, per_bounce):
        for b, v in enumerate(per_bounce):
            self.per_bounce[b] += v
