"""numpy / ctypes restatement of tile-masked sampling and the adaptive render (test
infrastructure; include/pathtracer_amd.h, pt_renderer_render_loop_masked and the calls
after it), built from the oracle's exported primitives: ptor_intersect_primary for the
cached primary hits, ptor_shade for one bounce's shading and ptor_intersect_rays for the
secondary rays.

One masked iteration: the active pixels in ascending order are shaded against their
cached hit with RNG slot = pixel index; the survivors, in order, get slots 0, 1, 2, ...
and are intersected, shaded and compacted until the pool is empty.  Every ray that
terminates adds sqrt(color) to its pixel's S and the float32 square of that to Q; a
pixel of an inactive tile adds nothing.  With every tile active this is the oracle's
render loop, one iteration at a time (tests/test_adaptive_ref.py holds it to that)."""
import ctypes

import numpy as np

import noise_ref as NR
import oracle as O

TILE = NR.TILE
F = np.float32

_P_F = ctypes.POINTER(ctypes.c_float)
_P_I = ctypes.POINTER(ctypes.c_int)


def _shade():
    """ptor_shade (oracle/ptoracle.h), which oracle/__init__.py does not wrap."""
    fn = O.lib().ptor_shade
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_int, _P_I, _P_F, _P_F, _P_F, _P_I, _P_F, _P_F, _P_I, _P_F]
    return fn


def tiles_shape(width, height):
    return (height + TILE - 1) // TILE, (width + TILE - 1) // TILE


def pixel_tiles(width, height):
    """Row-major tile index of every pixel, (H*W,)."""
    tx = tiles_shape(width, height)[1]
    y, x = np.divmod(np.arange(width * height), width)
    return (y // TILE) * tx + (x // TILE)


def tile_pixels(width, height):
    """Pixels per tile (edge tiles partial), (ty, tx) int64."""
    ty, tx = tiles_shape(width, height)
    return np.bincount(pixel_tiles(width, height), minlength=ty * tx).reshape(ty, tx).astype(np.int64)


def camera_dirs(cfg):
    """generateRaysKernel (Renderer.cpp:521-555) as the oracle's gen_ray states it:
    float32 camera origin and unnormalised float32 directions of every pixel."""
    W, H = cfg.width, cfg.height
    cam = np.array(cfg.cam, np.float64).astype(F)
    y, x = np.divmod(np.arange(W * H), W)
    step_x, step_y = F(cfg.plane_w / W), F(cfg.plane_h / H)
    wx = (cfg.plane_x0 + (x.astype(F) * step_x).astype(np.float64)).astype(F)
    wy = (cfg.plane_y0 + (y.astype(F) * step_y).astype(np.float64)).astype(F)
    wz = np.full(W * H, F(cfg.plane_z), F)
    return cam, (np.stack([wx, wy, wz], axis=1) - cam[None, :]).astype(F)


class Restatement:
    """S, Q, per-tile sample counts and the segment count of a renderer with moments on,
    for any sequence of plain and masked iterations.  cfg: an oracle.RenderConfig."""

    def __init__(self, flat, cfg):
        self.flat, self.cfg = flat, cfg
        W, H = cfg.width, cfg.height
        self.npix = W * H
        self.n_launch = (self.npix // 32) * 32 if cfg.tail_drop else self.npix
        self.cam, self.dirs = camera_dirs(cfg)
        self.hit_dist, self.hit_nrm, self.hit_model = O.intersect_primary(flat, cfg)
        self.mat_type = np.ascontiguousarray(flat.model_ints[:, 2], np.int32)
        self.mat_color = np.ascontiguousarray(flat.model_color, F)
        self.tile_of = pixel_tiles(W, H)
        self.shade = _shade()
        self.clear()

    def clear(self):
        self.S = np.zeros((self.npix, 3), F)
        self.Q = np.zeros((self.npix, 3), F)
        self.counts = np.zeros(tiles_shape(self.cfg.width, self.cfg.height), np.int32)
        self.segments = 0
        self.live = []                 # per iteration: live rays entering bounce 1, 2, ...

    def _shade_batch(self, it, slot, o, d, color, bounces, dist, nrm, model):
        hit = model >= 0
        mtype = np.where(hit, self.mat_type[np.where(hit, model, 0)], 0).astype(np.int32)
        mcolor = np.where(hit[:, None], self.mat_color[np.where(hit, model, 0)], F(0)).astype(F)
        slot = np.ascontiguousarray(slot, np.int32)
        dist = np.ascontiguousarray(dist, F)
        nrm = np.ascontiguousarray(nrm, F)
        rc = self.shade(len(slot), int(it), slot.ctypes.data_as(_P_I), o.ctypes.data_as(_P_F), d.ctypes.data_as(_P_F),
                        color.ctypes.data_as(_P_F), bounces.ctypes.data_as(_P_I), dist.ctypes.data_as(_P_F),
                        nrm.ctypes.data_as(_P_F), mtype.ctypes.data_as(_P_I), mcolor.ctypes.data_as(_P_F))
        assert rc == 0

    def iteration(self, it, mask=None):
        """Iteration id `it` under `mask` ((ty, tx), non-zero = sample; None = every tile)."""
        on = np.ones(self.counts.shape, bool) if mask is None else (np.asarray(mask) != 0)
        assert on.shape == self.counts.shape
        if not on.any():
            return
        pix = np.nonzero(on.reshape(-1)[self.tile_of[:self.n_launch]])[0].astype(np.int32)    # ascending
        n = len(pix)
        o = np.ascontiguousarray(np.repeat(self.cam[None, :], n, axis=0), F)
        d = np.ascontiguousarray(self.dirs[pix], F)
        color = np.ones((n, 3), F)
        bounces = np.full(n, self.cfg.max_bounces, np.int32)
        slot = pix.copy()
        dist, nrm, model = self.hit_dist[pix], self.hit_nrm[pix], self.hit_model[pix]
        c = np.zeros((self.npix, 3), F)
        live = []
        while True:
            self._shade_batch(it, slot, o, d, color, bounces, dist, nrm, model)
            dead = bounces <= 0
            c[pix[dead]] = np.sqrt(color[dead])
            keep = ~dead
            if not keep.any():
                break
            pix, o, d, color, bounces = (np.ascontiguousarray(a[keep]) for a in (pix, o, d, color, bounces))
            slot = np.arange(len(pix), dtype=np.int32)
            live.append(len(pix))
            dist, nrm, model = O.intersect_rays(self.flat, o, d, accel=self.cfg.accel, threads=4)
        self.S = self.S + c
        self.Q = self.Q + c * c
        self.counts[on] += 1
        self.segments += self.n_launch + sum(live)
        self.live.append(live)

    def render(self, first_iter, n_iters, mask=None):
        for it in range(first_iter, first_iter + n_iters):
            self.iteration(it, mask)

    def noise(self):
        return tile_noise(self.S, self.Q, self.cfg.width, self.cfg.height, self.counts)

    def mean(self):
        return tile_mean(self.S, self.cfg.width, self.cfg.height, self.counts)

    def render_adaptive(self, tile_target, max_iters, min_iters=2, check_every=32, first_iter=0):
        """pt_renderer_render_adaptive -> dict(converged, iters, pixel_samples, mean,
        checks: [(iterations done, tile errors, mask after the check)])."""
        if check_every <= 0:
            check_every = 32
        min_check = max(min_iters, 2)
        tp = tile_pixels(self.cfg.width, self.cfg.height)
        mask = np.ones(self.counts.shape, bool)
        done, taken, mean, checks, fresh = 0, 0, -1.0, [], False
        while done < max_iters and mask.any():
            n = min(check_every, max_iters - done)
            self.render(first_iter + done, n, mask)
            taken += int(tp[mask].sum()) * n
            done += n
            fresh = False
            if done >= min_check:
                est = self.noise()
                mean, fresh = est["mean"], True
                mask = mask & ~(est["tiles"].astype(np.float64) <= tile_target)
                checks.append((done, est["tiles"], mask.copy()))
        if not fresh:
            mean = self.noise()["mean"]
        return dict(converged=not mask.any(), iters=done, pixel_samples=taken, mean=mean, checks=checks)


def tile_noise(S, Q, width, height, counts):
    """pt_renderer_adaptive_noise: noise_ref's per-pixel error with nf = (float)count of
    the pixel's tile; a tile with fewer than 2 samples reads inf and is left out of the
    mean's sum (which is still divided by W*H).  -> dict(err, tiles, mean, max_tile)."""
    counts = np.asarray(counts)
    per_pixel = counts.reshape(-1)[pixel_tiles(width, height)]
    err = np.zeros(width * height, F)
    for c in np.unique(counts):
        if c >= 2:
            sel = per_pixel == c
            err[sel] = NR.pixel_err(S, Q, int(c))[sel]
    err = err.reshape(height, width)
    ty, tx = counts.shape
    sums = np.zeros((ty, tx), np.float64)
    tiles = np.zeros((ty, tx), F)
    for j in range(ty):
        for i in range(tx):
            t = err[j * TILE:(j + 1) * TILE, i * TILE:(i + 1) * TILE]
            if counts[j, i] >= 2:
                sums[j, i] = t.astype(np.float64).sum()
                tiles[j, i] = F(sums[j, i] / t.size)
            else:
                tiles[j, i] = np.inf
    return dict(err=err, tiles=tiles, mean=float(sums.sum() / (width * height)), max_tile=tiles.max())


def tile_mean(S, width, height, counts):
    """pt_renderer_adaptive_mean: float32 S / (float)count[tile], 0 where the count is 0."""
    per_pixel = np.asarray(counts).reshape(-1)[pixel_tiles(width, height)]
    S = np.ascontiguousarray(S, F).reshape(-1, 3)
    out = np.zeros_like(S)
    has = per_pixel > 0
    out[has] = S[has] / per_pixel[has].astype(F)[:, None]
    assert out.dtype == F
    return out
