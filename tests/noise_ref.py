"""numpy float32 restatement of the renderer's second-moment sum and noise
estimate (test infrastructure; include/pathtracer_amd.h, pt_renderer_noise).

Every operation is a float32 numpy operation on float32 arrays, in the order
the header states, so the per-pixel values match the device bit for bit (IEEE
add, multiply, divide and square root).  The tile and frame sums are float64."""
import numpy as np

TILE = 16
F = np.float32


def moment_sums(contribs):
    """Sequential float32 sums over iterations of c and of c*c (c*c rounded before
    the add): contribs is an iterable of (npix, 3) float32 arrays -> (S, Q)."""
    S = Q = None
    for c in contribs:
        c = np.ascontiguousarray(c, F)
        if S is None:
            S, Q = np.zeros_like(c), np.zeros_like(c)
        S = S + c
        Q = Q + c * c
    return S, Q


def pixel_err(S, Q, samples):
    """Per-pixel relative error, float32 (npix,)."""
    S = np.ascontiguousarray(S, F).reshape(-1, 3)
    Q = np.ascontiguousarray(Q, F).reshape(-1, 3)
    nf = F(samples)
    m = S / nf
    q = Q / nf
    v = q - m * m
    v = np.where(v > 0, v, F(0))
    e = np.sqrt(v / (nf - F(1.0)))
    assert m.dtype == F and e.dtype == F
    return ((e[:, 0] + e[:, 1]) + e[:, 2]) / (((m[:, 0] + m[:, 1]) + m[:, 2]) + F(0.01))


def noise(S, Q, width, height, samples):
    """-> dict(err (H, W) float32, tiles (ty, tx) float32, counts (ty, tx) pixels per
    tile, mean float64, max_tile float32)."""
    err = pixel_err(S, Q, samples).reshape(height, width)
    ty, tx = (height + TILE - 1) // TILE, (width + TILE - 1) // TILE
    sums = np.zeros((ty, tx), np.float64)
    counts = np.zeros((ty, tx), np.int64)
    for j in range(ty):
        for i in range(tx):
            t = err[j * TILE:(j + 1) * TILE, i * TILE:(i + 1) * TILE]
            sums[j, i] = t.astype(np.float64).sum()
            counts[j, i] = t.size
    tiles = (sums / counts).astype(F)
    return dict(err=err, tiles=tiles, counts=counts, mean=float(sums.sum() / (width * height)),
                max_tile=tiles.max())


def ulp_diff(a, b):
    """Largest distance in float32 units in the last place (non-negative finite values)."""
    a = np.ascontiguousarray(a, F).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, F).view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max()) if a.size else 0
