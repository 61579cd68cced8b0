"""numpy float32 restatement of pt_renderer_denoise_ex's two options (test infrastructure;
include/pathtracer_amd.h): albedo demodulation and per-tile sample counts.

It adds only the new prep and the remodulation; the guides, the slope and the passes are
denoise_ref's.  Every operation is a float32 numpy operation in the order the header states, so
the values match the device bit for bit."""
import numpy as np

import denoise_ref as DR

F = np.float32
TILE = 16
DEMODULATE, TILE_COUNTS = 1, 2           # PT_DENOISE_DEMODULATE, PT_DENOISE_TILE_COUNTS
FLOOR = F(1e-3)


def sqrt_albedo(albedo, k):
    """-> (sa, e), (npix, 3) each: sa = sqrtf(A > 0 ? A : 0), e = max(sa, 1e-3f); 1 where k < 0.
    albedo: pt_renderer_primary_albedo's (npix, 3); k: the guide model per pixel (npix,)."""
    A = np.ascontiguousarray(albedo, F).reshape(-1, 3)
    k = np.asarray(k).reshape(-1)
    assert len(A) == len(k)
    with np.errstate(invalid="ignore"):
        t = np.where(A > 0, A, F(0)).astype(F)           # a NaN compares false
    sa = np.sqrt(t)
    e = np.where(sa > FLOOR, sa, FLOOR).astype(F)
    hit = (k >= 0)[:, None]
    sa = np.where(hit, sa, F(1.0)).astype(F)
    e = np.where(hit, e, F(1.0)).astype(F)
    assert sa.dtype == F and e.dtype == F
    return sa, e


def pixel_counts(counts, width, height):
    """The (tiles_y, tiles_x) sample counts as nf per pixel, (npix,) float32."""
    c = np.asarray(counts)
    ty, tx = (height + TILE - 1) // TILE, (width + TILE - 1) // TILE
    assert c.shape == (ty, tx) and (c >= 2).all()
    ys, xs = np.mgrid[0:height, 0:width]
    return c[ys // TILE, xs // TILE].reshape(-1).astype(F)


def prep(S, Q, nf, e=None):
    """denoise_ref.prep with nf a scalar or per pixel (npix,), then the division by e (npix, 3)."""
    S = np.ascontiguousarray(S, F).reshape(-1, 3)
    Q = np.ascontiguousarray(Q, F).reshape(-1, 3)
    nf = np.asarray(nf, F)
    if nf.ndim:
        nf = nf.reshape(-1, 1)
    m = S / nf
    q = Q / nf
    v = q - m * m
    v = np.where(v > 0, v, F(0))
    v = v / (nf - F(1.0))
    if e is not None:
        m = m / e
        v = v / (e * e)
    assert m.dtype == F and v.dtype == F
    return m, (v[:, 0] + v[:, 1]) + v[:, 2]


def denoise(S, Q, width, height, samples, dist, normal, model, passes=5, sigma_l=4.0, sigma_z=1.0, albedo=None,
            counts=None):
    """-> (D (npix, 3), V (npix,)).  albedo: (npix, 3) of pt_renderer_primary_albedo, None: no
    demodulation; counts: (tiles_y, tiles_x) of pt_renderer_sample_counts in place of `samples`."""
    assert 1 <= passes <= DR.MAX_PASSES
    assert (counts is None) != (samples is None) and (counts is not None or samples >= 2)
    d, n, k = DR.guides(dist, normal, model, width, height)
    sa = e = None
    if albedo is not None:
        sa, e = sqrt_albedo(albedo, k)
    nf = F(samples) if counts is None else pixel_counts(counts, width, height)
    c, V = prep(S, Q, nf, e)
    g = DR.slope(d)
    c, V = c.reshape(height, width, 3), V.reshape(height, width)
    for s in range(passes):
        c, V = DR.one_pass(c, V, d, n, k, g, 1 << s, sigma_l, sigma_z)
    c = c.reshape(-1, 3)
    if sa is not None:
        c = c * sa
    assert c.dtype == F and V.dtype == F
    return np.ascontiguousarray(c), np.ascontiguousarray(V.reshape(-1))
