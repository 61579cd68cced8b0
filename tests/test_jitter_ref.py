"""The yardstick of the pixel-jitter tests, held to the oracle (CPU only): the restatement
in jitter_ref.py at width 0 is adaptive_ref's (which test_adaptive_ref.py holds to the
oracle's render loop), its offsets stay inside the stated square, and at width 1 it
anti-aliases: against a 4 x 4 supersampled render of the oracle the error of edge pixels
falls well below the unjittered render's while the other pixels' does not rise."""
import numpy as np
import pytest

import adaptive_ref as AR
import jitter_ref as JR
from conftest import INPUT_DATA
from helpers import assert_bitexact


@pytest.fixture(scope="module")
def flat(oracle_mod):
    return oracle_mod.reference_scene(INPUT_DATA)


@pytest.mark.parametrize("w,h,accel,tail_drop", [(64, 48, 0, 0), (64, 48, 1, 0), (37, 23, 0, 1)])
def test_width_zero_is_the_unjittered_restatement(oracle_mod, flat, w, h, accel, tail_drop):
    O = oracle_mod
    cfg = O.RenderConfig(width=w, height=h, max_bounces=5, accel=accel, tail_drop=tail_drop, threads=4)
    plain = AR.Restatement(flat, cfg)
    plain.render(0, 3)
    jit = JR.Restatement(flat, cfg, width=0.0)
    jit.render(0, 3)
    assert plain.S.any()
    assert_bitexact(jit.S, plain.S, "width 0: image")
    assert_bitexact(jit.Q, plain.Q, "width 0: moments")
    assert jit.segments - 3 * jit.n_launch == plain.segments
    assert (jit.counts == 3).all()
    # the emitted rays are the launched pixels, and what follows is the plain loop's
    assert [l[0] for l in jit.live] == [jit.n_launch] * 3
    assert [l[1:] for l in jit.live] == plain.live
    assert jit.per_bounce[0] == jit.per_bounce[1] == 3 * jit.n_launch
    if tail_drop:
        assert jit.n_launch == (w * h // 32) * 32 and not jit.S[jit.n_launch:].any()


@pytest.mark.parametrize("width", [0.5, 1.0, 2.0])
def test_offsets_stay_inside_the_square(oracle_mod, width):
    O = oracle_mod
    cfg = O.RenderConfig(width=64, height=48, max_bounces=5)
    pix = np.arange(64 * 48)
    y, x = np.divmod(pix, 64)
    lo, hi = np.float32(1.0), np.float32(0.0)
    for it in (0, 1, 255, 256, 100000):
        ux, uy = JR.jitter_offsets(it, pix, cfg.max_bounces)
        assert ux.dtype == np.float32 and (ux >= 0).all() and (ux < 1).all() and (uy >= 0).all() and (uy < 1).all()
        assert not np.array_equal(ux, uy)                   # two depths, two streams
        lo, hi = min(lo, ux.min(), uy.min()), max(hi, ux.max(), uy.max())
        fx, fy = JR.jitter_points(cfg, it, pix, width)
        half = width / 2
        assert (fx >= x - half).all() and (fx <= x + half).all()
        assert (fy >= y - half).all() and (fy <= y + half).all()
    assert lo < 0.01 and hi > 0.99                          # the offsets fill the square
    # the seeding depths are the two above every depth the shading uses (1 .. max_bounces)
    u01 = O.lib().ptor_u01_first
    ux, uy = JR.jitter_offsets(7, [11], cfg.max_bounces)
    assert ux[0] == np.float32(u01(7, 11, cfg.max_bounces + 1)) and uy[0] == np.float32(u01(7, 11, cfg.max_bounces + 2))


def test_it_anti_aliases(oracle_mod, flat):
    O = oracle_mod
    W, H, N, SS = 64, 48, 32, 4
    cfg = O.RenderConfig(width=W, height=H, max_bounces=5, accel=0, threads=4)
    # ground truth: 4 x 4 sub-pixels about every pixel's own point, other iteration ids
    hi_cfg = O.RenderConfig(width=SS * W, height=SS * H, max_bounces=5, accel=0, threads=4, first_iter=1000, iterations=16)
    hi, _ = O.render(flat, hi_cfg)
    hi = (hi / np.float32(16)).reshape(SS * H, SS * W, 3).astype(np.float64)
    ys, xs = np.arange(1, H - 1), np.arange(1, W - 1)           # the pixels whose 16 sub-pixels are in the frame
    sub = np.stack([hi[SS * ys[:, None] + j, SS * xs[None, :] + i] for j in range(-2, 2) for i in range(-2, 2)])
    truth = sub.mean(axis=0)                                     # (46, 62, 3)
    spread = (sub.max(axis=0) - sub.min(axis=0)).sum(axis=-1).reshape(-1)
    n_edge = round(0.15 * spread.size)
    assert (spread.size, n_edge) == (2852, 428)
    edge = np.zeros(spread.size, bool)
    edge[np.argsort(-spread, kind="stable")[:n_edge]] = True
    mse = {}
    for width in (0.0, 1.0):
        r = AR.Restatement(flat, cfg) if width == 0.0 else JR.Restatement(flat, cfg, width=width)
        r.render(0, N)
        mean = (r.S / np.float32(N)).reshape(H, W, 3)[1:H - 1, 1:W - 1].astype(np.float64)
        err = ((mean - truth) ** 2).mean(axis=-1).reshape(-1)
        mse[width] = err[edge].mean(), err[~edge].mean()
    edge_ratio, other_ratio = mse[1.0][0] / mse[0.0][0], mse[1.0][1] / mse[0.0][1]
    print(f"edge pixels: width 0 {mse[0.0][0]:.5f}, width 1 {mse[1.0][0]:.5f}, ratio {edge_ratio:.3f}; "
          f"other pixels: width 0 {mse[0.0][1]:.5f}, width 1 {mse[1.0][1]:.5f}, ratio {other_ratio:.3f}")
    assert edge_ratio <= 0.6
    assert other_ratio <= 1.05
