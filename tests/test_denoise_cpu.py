"""The denoiser without a GPU: denoise_ref (the numpy float32 restatement the device
reproduces bit for bit) on the oracle's renders and on hand-made data, and the C
ABI's refusals on a renderer that was never allocated."""
import ctypes

import numpy as np
import pytest

import denoise_ref as DR
import noise_ref as NR
from conftest import INPUT_DATA

F = np.float32
BOUNCES = 5
TRUTH_ITERS, TRUTH_FIRST = 512, 1000


def oracle_sums(O, scene, w, h, n):
    """(S, Q) of iterations 0..n-1, one oracle render each into a zero image."""
    cs = []
    for it in range(n):
        cfg = O.RenderConfig(width=w, height=h, iterations=1, first_iter=it, max_bounces=BOUNCES, threads=4)
        cs.append(O.render(scene, cfg)[0])
    return NR.moment_sums(cs)


def mse(a, b):
    return float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean())


def test_reference_filter_reduces_the_error(oracle_mod):
    """8 samples at 64x48 against the mean of 512 other iterations: the filtered image's
    error is under half the raw mean's (a cap; the filter alone measured 0.121)."""
    O = oracle_mod
    w, h, n = 64, 48, 8
    scene = O.reference_scene(INPUT_DATA)
    S, Q = oracle_sums(O, scene, w, h, n)
    cfg = O.RenderConfig(width=w, height=h, max_bounces=BOUNCES, threads=4)
    dist, nrm, model = O.intersect_primary(scene, cfg)
    truth, _ = O.render(scene, O.RenderConfig(width=w, height=h, iterations=TRUTH_ITERS, first_iter=TRUTH_FIRST,
                                              max_bounces=BOUNCES, threads=4))
    truth = truth / F(TRUTH_ITERS)
    D, V = DR.denoise(S, Q, w, h, n, dist, nrm, model)
    raw = S / F(n)
    ratio = mse(D, truth) / mse(raw, truth)
    print(f"64x48, 8 samples: MSE(denoised) / MSE(raw) = {ratio:.4f}")
    assert np.isfinite(D).all() and np.isfinite(V).all()
    assert ratio < 0.5


def synthetic_guides(w, h, seed=3):
    """Three slanted model regions, a block of misses and noisy normals."""
    rs = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    k = ((xs * 3) // max(w, 1) % 3).astype(np.int32)
    k[(ys > h // 2) & (xs > w // 2)] = 5
    d = (20.0 + 0.5 * xs + 0.25 * ys + 3.0 * k).astype(F)
    n = rs.normal(size=(h, w, 3)) * 0.05 + np.array([0.0, 0.0, 1.0])
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F)
    miss = (ys < h // 4) & (xs > w // 3) & (xs < 2 * w // 3)
    k[miss] = -1
    d[miss] = DR.FLT_MAX
    n[miss] = 0
    return d.reshape(-1), n.reshape(-1, 3), k.reshape(-1)


def test_per_model_constants_are_kept():
    w, h, n = 37, 23, 6
    d, nn, k = synthetic_guides(w, h)
    S, Q, _ = DR.per_model_constant_sums(k, n)
    c0, V0 = DR.prep(S, Q, n)
    np.testing.assert_allclose(V0, 3 * 50.0, rtol=1e-3)                  # v_k = 50 in every channel
    D, V = DR.denoise(S, Q, w, h, n, d, nn, k)
    DR.check_per_model_constants(D, V, S, Q, k, n)
    hit = k >= 0
    assert V[hit].max() < 0.5 * V0[hit].max()             # and it falls where there is something to average


@pytest.mark.parametrize("passes", [1, 6])
def test_misses_and_dropped_tail_pass_through(passes):
    w, h, n = 37, 23, 4
    d, nn, k = synthetic_guides(w, h)
    live = (w * h // 32) * 32                              # tail_drop: the last 19 pixels have no guides
    rs = np.random.RandomState(11)
    cs = [rs.uniform(0, 1, (w * h, 3)).astype(F) for _ in range(n)]
    for c in cs:
        c[live:] = 0
    S, Q = NR.moment_sums(cs)
    D, V = DR.denoise(S, Q, w, h, n, d[:live], nn[:live], k[:live], passes=passes)
    c0, V0 = DR.prep(S, Q, n)
    kk = k.copy()
    kk[live:] = -1
    assert (kk < 0).sum() > 19 and (kk >= 0).sum() > 0
    assert np.array_equal(D[kk < 0], c0[kk < 0]) and np.array_equal(V[kk < 0], V0[kk < 0])
    assert not D[live:].any() and not V[live:].any()
    assert np.isfinite(D).all() and np.isfinite(V).all()  # a miss (d = FLT_MAX) beside a hit
    assert not np.array_equal(D[kk >= 0], c0[kk >= 0])
    # a hit pixel is a convex combination of same-model inputs
    for m in np.unique(kk[kk >= 0]):
        sel = kk == m
        assert D[sel].min() >= c0[sel].min() * (1 - 1e-5) and D[sel].max() <= c0[sel].max() * (1 + 1e-5)


def test_single_pixel_frame():
    S = np.array([[2.0, 1.0, 0.5]], F)
    Q = np.array([[3.0, 1.0, 0.25]], F)
    for model in (0, -1):
        for passes in (1, 5, 6):
            D, V = DR.denoise(S, Q, 1, 1, 2, [7.0], [[0.0, 0.0, 1.0]], [model], passes=passes)
            c0, V0 = DR.prep(S, Q, 2)
            # the centre tap alone: c * w / w and V * w*w / (w*w) with w = 9/64, exact here
            assert np.array_equal(D, c0) and np.array_equal(V, V0)


# ---- the C ABI without a device ----

def test_default_denoise_params(pt_mod):
    p = pt_mod._DenoiseParams()
    pt_mod.lib().pt_default_denoise_params(ctypes.byref(p))
    assert (p.passes, p.sigma_l, p.sigma_z) == (5, 4.0, 1.0)
    assert pt_mod.DENOISE_MAX_PASSES == DR.MAX_PASSES == 6


def test_null_and_unallocated_renderers_are_refused(pt_mod, tmp_path):
    P = pt_mod
    L = P.lib()
    buf = (ctypes.c_float * 3)()
    assert L.pt_renderer_denoise(None, 2, None, None, buf, None) == -1
    assert b"null renderer" in L.pt_last_error()
    assert L.pt_renderer_render_image_denoised(None, b"x.bmp", 2, None) == -1
    assert b"null renderer" in L.pt_last_error()
    r = P.Renderer(P.RenderConfig(width=8, height=8))
    try:
        r.enable_moments()
        with pytest.raises(P.PathTracerError, match="not allocated"):
            r.denoise()
        with pytest.raises(P.PathTracerError, match="not allocated"):
            r.renderImageDenoised(str(tmp_path / "never.bmp"), samples=4)
        assert not (tmp_path / "never.bmp").exists()
    finally:
        r.free()
