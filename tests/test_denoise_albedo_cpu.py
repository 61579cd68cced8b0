"""pt_renderer_denoise_ex's options without a GPU: denoise_albedo_ref (the numpy float32
restatement the device reproduces bit for bit) against denoise_ref where the two must agree, on
hand-made data, and on texture_ref's render of the quality scene; and the C ABI's refusals on a
renderer that was never allocated."""
import ctypes

import numpy as np
import pytest

import denoise_albedo_ref as AR
import denoise_albedo_scenes as AS
import denoise_ref as DR
import env_ref as ER
import noise_ref as NR
import texture_ref as TR
import texture_scenes as TS
from helpers import assert_bitexact, flat_from_export, oracle_cfg
from test_denoise_cpu import synthetic_guides

F = np.float32
W, H = 37, 23


def random_sums(w, h, n, seed):
    rs = np.random.RandomState(seed)
    return NR.moment_sums([rs.uniform(0, 1, (w * h, 3)).astype(F) for _ in range(n)])


@pytest.mark.parametrize("passes", [1, 5])
def test_an_albedo_of_ones_and_uniform_counts_are_the_plain_filter(passes):
    """x / 1.0f and x * 1.0f are x: the restatement with sa = e = 1 is denoise_ref bit for bit; and
    counts that are the same in every tile are the scalar sample count."""
    n = 6
    d, nn, k = synthetic_guides(W, H)
    S, Q = random_sums(W, H, n, 21)
    want = DR.denoise(S, Q, W, H, n, d, nn, k, passes=passes)
    ones = np.ones((W * H, 3), F)
    counts = np.full(((H + 15) // 16, (W + 15) // 16), n, np.int32)
    for what, got in (("albedo of ones", AR.denoise(S, Q, W, H, n, d, nn, k, passes=passes, albedo=ones)),
                      ("uniform counts", AR.denoise(S, Q, W, H, None, d, nn, k, passes=passes, counts=counts)),
                      ("both", AR.denoise(S, Q, W, H, None, d, nn, k, passes=passes, albedo=ones, counts=counts)),
                      ("neither", AR.denoise(S, Q, W, H, n, d, nn, k, passes=passes))):
        assert_bitexact(got[0], want[0], f"{what}: image")
        assert_bitexact(got[1], want[1], f"{what}: variance")


def test_mixed_counts_divide_each_tile_by_its_own():
    """Sums of 4 samples in some tiles and 7 in the others: with the counts the prep equals each
    tile's own scalar prep; a scalar count does not."""
    d, nn, k = synthetic_guides(W, H)
    ty, tx = (H + 15) // 16, (W + 15) // 16
    counts = np.where(np.random.RandomState(3).rand(ty, tx) < 0.5, 4, 7).astype(np.int32)
    assert len(np.unique(counts)) == 2
    nf = AR.pixel_counts(counts, W, H)
    S4, Q4 = random_sums(W, H, 4, 5)
    S3, Q3 = random_sums(W, H, 3, 6)
    more = (nf == 7)[:, None]
    S, Q = np.where(more, S4 + S3, S4).astype(F), np.where(more, Q4 + Q3, Q4).astype(F)
    c, V = AR.prep(S, Q, nf)
    for cnt in (4, 7):
        c1, V1 = DR.prep(S, Q, cnt)
        sel = nf == cnt
        assert_bitexact(c[sel], c1[sel], f"tiles of {cnt}: mean")
        assert_bitexact(V[sel], V1[sel], f"tiles of {cnt}: variance")
    D, V = AR.denoise(S, Q, W, H, None, d, nn, k, counts=counts)
    assert np.isfinite(D).all() and np.isfinite(V).all()
    assert not np.array_equal(D, DR.denoise(S, Q, W, H, 4, d, nn, k)[0])


def test_a_constant_demodulated_image_per_model_stays_constant():
    """denoise_ref.per_model_constant_sums times a seeded albedo pattern: the plain filter averages
    across the pattern, the demodulated one returns pattern * constant within
    check_per_model_constants' bound (2e-5: the passes' roundings) plus the three roundings of the
    construction, the division and the multiplication (under 4e-7)."""
    n = 8
    d, nn, k = synthetic_guides(W, H)
    rs = np.random.RandomState(9)
    A = rs.uniform(0.05, 1.0, (W * H, 3)).astype(F)
    S0, Q0, col = DR.per_model_constant_sums(k, n)
    sa, e = AR.sqrt_albedo(A, k)
    assert np.array_equal(sa, e)
    S, Q = (S0 * sa).astype(F), (Q0 * (sa * sa)).astype(F)
    D, V = AR.denoise(S, Q, W, H, n, d, nn, k, albedo=A)
    hit = k >= 0
    want = col * sa.astype(np.float64)
    rel = np.abs(D[hit].astype(np.float64) - want[hit]) / want[hit]
    plain = DR.denoise(S, Q, W, H, n, d, nn, k)[0]
    rel_plain = np.abs(plain[hit].astype(np.float64) - want[hit]) / want[hit]
    print(f"constant per model under an albedo pattern: max relative deviation demodulated {rel.max():.3g}, plain {rel_plain.max():.3g}")
    assert rel.max() <= 2.1e-5
    assert rel_plain.max() > 0.1                         # the pattern is there to be blurred
    c0, V0 = AR.prep(S, Q, n, e)
    assert np.all(V[hit] <= V0[hit])
    assert_bitexact(D[~hit], (S / F(n))[~hit], "misses copy through")


def test_black_tiny_and_nan_albedos_give_finite_c_and_zero_D():
    """A = 0, 1e-8 and NaN in one channel each over a block of pixels: e is the floor there, c and
    D are finite, and D is exactly 0 where sa is 0 (A = 0, NaN); with A = 1e-8, sa = 1e-4 is under
    the floor, so c = m / 1e-3 and D = c * 1e-4, a tenth of the mean, not a blow-up."""
    n = 6
    d, nn, k = synthetic_guides(W, H)
    S, Q = random_sums(W, H, n, 33)
    A = np.random.RandomState(4).uniform(0.2, 1.0, (W * H, 3)).astype(F)
    px = np.arange(W * H)
    zero, tiny, nan = (px % 7 == 0), (px % 7 == 1), (px % 7 == 2)
    A[zero, 0] = 0.0
    A[tiny, 1] = 1e-8
    A[nan, 2] = np.nan
    A[px % 7 == 3, 0] = -0.5                             # negative: 0 as well
    sa, e = AR.sqrt_albedo(A, k)
    hit = k >= 0
    assert (e[hit] >= F(1e-3)).all() and np.isfinite(e).all() and np.isfinite(sa).all()
    assert (sa[hit & zero, 0] == 0).all() and (sa[hit & nan, 2] == 0).all() and (sa[hit & (px % 7 == 3), 0] == 0).all()
    assert_bitexact(sa[hit & tiny, 1], np.full((hit & tiny).sum(), np.sqrt(F(1e-8)), F), "sqrt(1e-8)")
    c, V0 = AR.prep(S, Q, n, e)
    assert np.isfinite(c).all() and np.isfinite(V0).all()
    for passes in (1, 5):
        D, V = AR.denoise(S, Q, W, H, n, d, nn, k, passes=passes, albedo=A)
        assert np.isfinite(D).all() and np.isfinite(V).all()
        assert (D[hit & zero, 0] == 0).all() and (D[hit & nan, 2] == 0).all() and (D[hit & (px % 7 == 3), 0] == 0).all()
        assert (D[hit & tiny, 1] > 0).all() and (D[hit & tiny, 1] <= (S / F(n)).max() * F(0.11)).all()
        # a miss keeps its mean whatever its albedo entry says
        assert_bitexact(D[~hit], (S / F(n))[~hit], "misses copy through")
        assert_bitexact(V[~hit], DR.prep(S, Q, n)[1][~hit], "misses keep their variance")


def test_dropped_tail_and_single_pixel():
    """Guides shorter than the frame (tail_drop): the pixels past them are misses, sa = 1."""
    n = 4
    d, nn, k = synthetic_guides(W, H)
    live = (W * H // 32) * 32
    S, Q = random_sums(W, H, n, 8)
    A = np.random.RandomState(2).uniform(0.1, 1.0, (W * H, 3)).astype(F)
    A[live:] = 0                                         # what primary_albedo reports there
    D, V = AR.denoise(S, Q, W, H, n, d[:live], nn[:live], k[:live], albedo=A)
    assert_bitexact(D[live:], (S / F(n))[live:], "dropped pixels copy through")
    assert np.isfinite(D).all() and np.isfinite(V).all()
    S1, Q1 = np.array([[2.0, 1.0, 0.5]], F), np.array([[3.0, 1.0, 0.25]], F)
    D, V = AR.denoise(S1, Q1, 1, 1, None, [7.0], [[0.0, 0.0, 1.0]], [0], albedo=[[0.25, 1.0, 0.0]],
                      counts=np.array([[2]], np.int32))
    assert_bitexact(D, np.array([[1.0, 0.5, 0.0]], F), "1x1: (m / sa) * sa with sa = 0.5, 1 and 0")


_QUALITY = {}


def quality_render(P):
    """texture_ref's render of the quality scene: 8 samples, and the truth of 512 others."""
    if not _QUALITY:
        spec = AS.quality_spec()
        flat = flat_from_export(TS.gpu_scene(P, spec).export())
        cfg = P.RenderConfig(width=64, height=48, max_bounces=4, iterations=8, accel=P.ACCEL_GRID_FAST)

        def restatement():
            return TR.Restatement(flat, oracle_cfg(cfg, threads=4), env=ER.Env.of(AS.quality_env(P)), smooth=spec["smooth"],
                                  uv=TS.vertex_uv(spec), textures=spec["textures"], binding=spec["binding"])
        r = restatement()
        r.render(0, 8)
        t = restatement()
        t.render(1000, 512)
        _QUALITY.update(S=r.S, Q=r.Q, hits=r.primary_hits(), albedo=r.primary_albedo(), truth=t.S / F(512))
    return _QUALITY


def test_demodulation_beats_the_plain_filter_on_a_textured_face(pt_mod, oracle_mod):
    """The feature's purpose, on the restatement's render (a few seconds): at 8 samples the
    demodulated filter's error against 512 other iterations is below the plain filter's on the
    same sums, and below the raw mean's, over every pixel whose primary hit is the textured face.
    Measured: raw 0.010813, plain 0.004026, demodulated 0.000171 (demodulated / plain 0.0426)."""
    q = quality_render(pt_mod)
    d, n, k = q["hits"]
    on_face = k == 0
    assert on_face.mean() > 0.9
    tex_px = 64 * AS.TEXEL / 920.0
    assert 2.0 <= tex_px <= 4.0
    mse = lambda a: float(((a.astype(np.float64) - q["truth"].astype(np.float64))[on_face] ** 2).mean())
    raw = q["S"] / F(8)
    plain = DR.denoise(q["S"], q["Q"], 64, 48, 8, d, n, k)[0]
    demod = AR.denoise(q["S"], q["Q"], 64, 48, 8, d, n, k, albedo=q["albedo"])[0]
    print(f"64x48, 8 samples, textured face: MSE raw {mse(raw):.6f}, plain denoise {mse(plain):.6f}, demodulated "
          f"{mse(demod):.6f}; demodulated / plain {mse(demod) / mse(plain):.4f}")
    assert mse(demod) < mse(plain)
    assert mse(demod) < mse(raw)


# ---- the C ABI without a device ----

def test_null_and_unallocated_renderers_are_refused(pt_mod, tmp_path):
    P = pt_mod
    L = P.lib()
    buf = (ctypes.c_float * 3)()
    assert L.pt_renderer_denoise_ex(None, 2, None, 1, None, buf, None) == -1
    assert b"null renderer" in L.pt_last_error()
    assert L.pt_renderer_render_image_denoised_ex(None, b"x.bmp", 2, None, 1) == -1
    assert b"null renderer" in L.pt_last_error()
    assert (P.DENOISE_DEMODULATE, P.DENOISE_TILE_COUNTS) == (AR.DEMODULATE, AR.TILE_COUNTS) == (1, 2)
    r = P.Renderer(P.RenderConfig(width=8, height=8))
    try:
        r.enable_moments()
        for kw in (dict(demodulate=True), dict(tile_counts=True), dict(flags=0), dict(flags=4)):
            with pytest.raises(P.PathTracerError, match="not allocated"):
                r.denoise(**kw)
        with pytest.raises(P.PathTracerError, match="not allocated"):
            r.renderImageDenoised(str(tmp_path / "never.bmp"), samples=4, demodulate=True)
        assert not (tmp_path / "never.bmp").exists()
        assert L.pt_renderer_render_image_denoised_ex(r._h, None, 2, None, 1) == -1
        assert b"bad arguments" in L.pt_last_error()
    finally:
        r.free()
