"""numpy restatement of the sampled first-hit guides (test infrastructure;
include/pathtracer_amd.h, pt_renderer_enable_guides and PT_DENOISE_SAMPLED_GUIDES).

Restatement: texture_ref.Restatement that also keeps G, the (npix, 8) float32 sums
(Nx, Ny, Nz, Z, Ar, Ag, Ab, Hc), and the per-tile guide counts.  A generated iteration (the jitter
on, or a camera with a lens) shades its emitted rays first: that first _shade_batch holds the
rays (o, d) and the oracle's first hits (dist, flat normal, model) before the shade moves them.
The record of a hit is the normal the shade uses (smooth_ref.shading_normals), the distance,
sqrtf(pos(mc)) of texture_ref's albedo and 1; a miss is eight zeros.  G gets one float32 add per
float per iteration, at the emitted rays' pixels, in iteration order.

guided_prep / denoise: the denoiser's prep from G, float32 operation by operation in the header's
order, feeding denoise_ref's unchanged passes; with demodulation it is denoise_albedo_ref's prep
with the sampled e."""
import numpy as np

import denoise_albedo_ref as AR
import denoise_ref as DR
import smooth_ref as SR
import texture_ref as TR

F = np.float32
FLT_MAX = DR.FLT_MAX
DEMODULATE, TILE_COUNTS, SAMPLED_GUIDES = 1, 2, 4
FLOOR = AR.FLOOR


def records(ref, o, d, dist, nrm, model):
    """The (m, 8) float32 records of first hits (dist, nrm, model) of the rays (o, d)."""
    model = np.asarray(model)
    hit = model >= 0
    n = SR.shading_normals(ref.flat, ref.tables, ref.smooth, o, d, dist, nrm, model, ref.ident)[0]
    mc = ref.albedo(o, d, dist, nrm, model)
    with np.errstate(invalid="ignore"):
        sa = np.sqrt(np.where(mc > 0, mc, F(0)).astype(F)).astype(F)
    g = np.zeros((len(model), 8), F)
    g[:, 0:3] = n
    g[:, 3] = np.asarray(dist, F)
    g[:, 4:7] = sa
    g[:, 7] = F(1)
    g[~hit] = F(0)
    return g


class Restatement(TR.Restatement):
    """texture_ref.Restatement with pt_renderer_enable_guides."""

    def __init__(self, *a, **kw):
        self._want = None
        super().__init__(*a, **kw)
        self._clear_guides()

    def _clear_guides(self):
        self.G = np.zeros((self.npix, 8), F)
        self.guide_counts = np.zeros(AR_tiles(self.cfg.width, self.cfg.height), np.int32)

    def clear(self):
        super().clear()
        self._clear_guides()

    def set_camera(self, camera):
        super().set_camera(camera)
        self._clear_guides()

    def set_environment(self, env):
        super().set_environment(env)
        if hasattr(self, "G"):
            self._clear_guides()

    def iteration(self, it, mask=None):
        on = np.ones(self.counts.shape, bool) if mask is None else (np.asarray(mask) != 0)
        if not self.generated() or not on.any():
            self._want = None
            return super().iteration(it, mask)
        # the emitted rays' pixels: the launched pixels of active tiles, ascending
        self._want = np.nonzero(on.reshape(-1)[self.tile_of[:self.n_launch]])[0]
        super().iteration(it, mask)
        assert self._want is None, "the iteration shaded nothing"
        self.guide_counts[on] += 1

    def _shade_batch(self, it, slot, o, d, color, bounces, dist, nrm, model):
        if self._want is not None:
            pix, self._want = self._want, None
            assert len(pix) == len(model)
            g = np.zeros((self.npix, 8), F)
            g[pix] = records(self, o.copy(), d.copy(), np.array(dist, F), np.array(nrm, F), np.array(model))
            self.G = (self.G + g).astype(F)
        return super()._shade_batch(it, slot, o, d, color, bounces, dist, nrm, model)


def AR_tiles(width, height):
    return (height + AR.TILE - 1) // AR.TILE, (width + AR.TILE - 1) // AR.TILE


def guided_prep(S, Q, G, width, height, nf, demodulate):
    """-> (c (npix, 3), V (npix,), d (H, W), n (H, W, 3), k (H, W), slope (H, W), sa or None).
    nf: a float32 scalar or per pixel (npix,)."""
    G = np.ascontiguousarray(G, F).reshape(-1, 8)
    h = G[:, 7]
    hit = h > 0
    nfp = np.broadcast_to(np.asarray(nf, F).reshape(-1), (len(G),)) if np.ndim(nf) else np.full(len(G), F(nf), F)
    with np.errstate(all="ignore"):
        d = np.where(hit, G[:, 3] / h, FLT_MAX).astype(F)
        n = np.where(hit[:, None], G[:, 0:3] / h[:, None], F(0)).astype(F)
        k = np.where(hit, 0, -1).astype(np.int32)
        sa = e = None
        if demodulate:
            sa = ((G[:, 4:7] + (nfp - h).astype(F)[:, None]).astype(F) / nfp[:, None]).astype(F)
            e = np.where(sa > FLOOR, sa, FLOOR).astype(F)
        c, V = AR.prep(S, Q, nf, e)
    d = d.reshape(height, width)
    return c, V, d, n.reshape(height, width, 3), k.reshape(height, width), DR.slope(d), sa


def denoise(S, Q, G, width, height, samples=None, counts=None, flags=SAMPLED_GUIDES, passes=5, sigma_l=4.0, sigma_z=1.0):
    """pt_renderer_denoise_ex with PT_DENOISE_SAMPLED_GUIDES set in flags -> (D (npix, 3), V (npix,)).
    samples: the explicit count; counts: (tiles_y, tiles_x), with PT_DENOISE_TILE_COUNTS."""
    assert flags & SAMPLED_GUIDES and 1 <= passes <= DR.MAX_PASSES
    by_tile = bool(flags & TILE_COUNTS)
    assert by_tile == (counts is not None) and (by_tile or samples >= 2)
    nf = AR.pixel_counts(counts, width, height) if by_tile else F(samples)
    c, V, d, n, k, g, sa = guided_prep(S, Q, G, width, height, nf, bool(flags & DEMODULATE))
    c, V = c.reshape(height, width, 3), V.reshape(height, width)
    for s in range(passes):
        c, V = DR.one_pass(c, V, d, n, k, g, 1 << s, sigma_l, sigma_z)
    c = c.reshape(-1, 3)
    if sa is not None:
        c = c * sa
    assert c.dtype == F and V.dtype == F
    return np.ascontiguousarray(c), np.ascontiguousarray(V.reshape(-1))


def refusal(guides_enabled, samples, sample_counts, guide_counts):
    """The message pt_renderer_denoise_ex refuses PT_DENOISE_SAMPLED_GUIDES with, or None: the
    conditions restated (the other flags' refusals are denoise_ex's own)."""
    if not guides_enabled:
        return "guides not enabled"
    if (samples is None or samples <= 0) and not np.array_equal(np.asarray(sample_counts), np.asarray(guide_counts)):
        return "guide count differs from its sample count"
    return None


def allocation_refusal(guides_enabled, moments_enabled, split_trace):
    """allocate_on_gpu's refusals for guides, or None."""
    if guides_enabled and not moments_enabled:
        return "guides need moments"
    if guides_enabled and not split_trace:
        return "guides need the split trace"
    return None
