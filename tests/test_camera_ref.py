"""The yardstick of the free-camera tests, held to the oracle (CPU only): with the
legacy-equivalent camera the restatement in camera_ref.py is adaptive_ref's (jitter off)
and jitter_ref's (jitter on) bit for bit, which test_adaptive_ref.py and test_jitter_ref.py
hold to the oracle's render loop; and its lens samples stay on the lens and aim at the
pinhole's point of the plane in focus."""
import numpy as np
import pytest

import adaptive_ref as AR
import camera_ref as CR
import jitter_ref as JR
from conftest import INPUT_DATA
from helpers import assert_bitexact

F = np.float32
EPS = 2.0 ** -23          # ulp(v) <= EPS * |v| for a normal float32 v; one rounding errs by at most half of it


@pytest.fixture(scope="module")
def flat(oracle_mod):
    return oracle_mod.reference_scene(INPUT_DATA)


def cam_from(eye, target, fov, focus, lens, W, H, up=(0.0, 1.0, 0.0)):
    """pt_camera_look_at restated in float64, rounded once (tests/test_camera_api.py holds the
    library's to the same properties)."""
    eye, target, up = (np.array(v, np.float64) for v in (eye, target, up))
    f = (target - eye) / np.linalg.norm(target - eye)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    hh = focus * np.tan(np.radians(fov) / 2)
    hw = hh * W / H
    return CR.Cam(origin=eye.astype(F), p0=(eye + f * focus - r * hw - u * hh).astype(F), du=(r * (2 * hw / W)).astype(F),
                  dv=(u * (2 * hh / H)).astype(F), lens_u=r.astype(F), lens_v=u.astype(F), lens_radius=F(lens))


@pytest.mark.parametrize("accel", [0, 1])
@pytest.mark.parametrize("w,h,tail_drop", [(64, 48, 0), (37, 23, 1)])
def test_the_legacy_equivalent_camera_is_the_legacy_camera(oracle_mod, flat, w, h, tail_drop, accel):
    O = oracle_mod
    cfg = O.RenderConfig(width=w, height=h, max_bounces=5, accel=accel, tail_drop=tail_drop, threads=4)
    cam = CR.legacy_camera(cfg)
    pix = np.arange(w * h)
    # the rays themselves, plain and jittered
    _, legacy_dirs = AR.camera_dirs(cfg)
    o, d = CR.camera_rays(cam, cfg, 0, pix)
    assert_bitexact(d, legacy_dirs, "plain directions")
    assert_bitexact(o, np.repeat(np.array(cfg.cam, np.float64).astype(F)[None, :], w * h, axis=0), "origins")
    for width in (None, 0.5, 1.0, 2.0):
        want = AR.Restatement(flat, cfg) if width is None else JR.Restatement(flat, cfg, width=width)
        want.render(0, 3)
        got = CR.Restatement(flat, cfg, width=width, camera=cam)
        if width is None:
            assert_bitexact(got.hit_dist, want.hit_dist, "cache: distance")
            assert_bitexact(got.hit_nrm, want.hit_nrm, "cache: normal")
            assert_bitexact(got.hit_model, want.hit_model, "cache: model")
        else:
            assert_bitexact(CR.camera_rays(cam, cfg, 7, pix, width)[1], JR.jitter_dirs(cfg, 7, pix, width),
                            f"width {width}: directions")
        got.render(0, 3)
        what = f"{w}x{h} accel {accel} width {width}"
        assert want.S.any()
        assert_bitexact(got.S, want.S, f"{what}: image")
        assert_bitexact(got.Q, want.Q, f"{what}: moments")
        assert got.segments == want.segments, what
        assert got.live == want.live, what
        assert (got.counts == 3).all()


VIEW_A = dict(eye=(0, 800, 500), target=(0, 0, 0), fov=45, focus=900)
VIEW_B = dict(eye=(650, 200, 650), target=(0, 0, 0), fov=45, focus=float(np.sqrt(650 ** 2 + 200 ** 2 + 650 ** 2)))


@pytest.mark.parametrize("view", [VIEW_A, VIEW_B], ids=["A", "B"])
def test_lens_samples(oracle_mod, view):
    O = oracle_mod
    W, H, R = 64, 48, 25.0
    cfg = O.RenderConfig(width=W, height=H, max_bounces=5)
    cam = cam_from(lens=R, W=W, H=H, **view)
    pin = CR.pinhole(cam)
    pix = np.arange(W * H)
    origin = cam.origin.astype(np.float64)
    far, u_max = 0.0, 0.0
    for it in (0, 1, 255, 256, 100000):
        u1, u2 = CR.lens_uniforms(it, pix, cfg.max_bounces)
        assert u1.dtype == F and (u1 >= 0).all() and (u1 < 1).all() and (u2 >= 0).all() and (u2 < 1).all()
        ux, uy = JR.jitter_offsets(it, pix, cfg.max_bounces)
        for a in (ux, uy, u2):
            assert not np.array_equal(u1, a)                    # four depths, four streams
        assert not np.array_equal(u2, ux) and not np.array_equal(u2, uy)
        for width in (None, 1.0):
            o, d = CR.camera_rays(cam, cfg, it, pix, width)
            op, dp = CR.camera_rays(pin, cfg, it, pix, width)
            assert o.dtype == F and d.dtype == F
            # On the lens.  lens_u and lens_v are orthonormal to float32 rounding, so in exact
            # arithmetic |o - origin|^2 = rr^2 (cos^2 + sin^2) <= R^2 u1 < R^2.  Float32: rr, cos,
            # sin, a, b and the two products per coordinate carry one rounding each (relative
            # EPS/2; lens_u / lens_v another EPS/2 each from look_at's rounding): under 4 EPS R in
            # all; each coordinate's two adds round at magnitude <= |origin_k| + R, EPS/2 of it each.
            dist = np.linalg.norm(o.astype(np.float64) - origin, axis=1)
            tol = 4 * EPS * R + np.sqrt(3.0) * EPS * (np.abs(origin).max() + R)
            assert (dist <= R * np.sqrt(u1.astype(np.float64)) + tol).all()
            assert dist.max() <= R + tol
            far, u_max = max(far, dist.max()), max(u_max, float(u1.max()))
            # Aimed at the pinhole's point: t is the same float32 point for both, d = fl(t - o), so
            # o + d and origin + d_pinhole (summed exactly, in double) each miss t by the rounding
            # of their one subtraction, at most half an ulp of the difference: EPS/2 * |d_k|.
            lens_t = o.astype(np.float64) + d.astype(np.float64)
            pin_t = op.astype(np.float64) + dp.astype(np.float64)
            bound = 0.5 * EPS * (np.abs(d).astype(np.float64) + np.abs(dp).astype(np.float64))
            assert (np.abs(lens_t - pin_t) <= bound).all(), np.abs(lens_t - pin_t).max()
            assert not np.array_equal(o, op)
    assert u_max > 0.999 and far > 0.999 * R                    # samples reach the rim (u1 -> 1) and stay on the lens


def test_a_lens_changes_what_some_centre_rays_hit(oracle_mod, flat):
    """View A at 64 x 32 with a lens of 25: a few centre rays' models change, so a lens that
    did nothing would not pass the GPU tests against this restatement."""
    O = oracle_mod
    W, H = 64, 32
    cfg = O.RenderConfig(width=W, height=H, max_bounces=5, accel=0)
    cam = cam_from(lens=25.0, W=W, H=H, **VIEW_A)
    pix = np.arange(W * H)
    _, _, _, _, model = CR.centre_hits(flat, cfg, cam)
    assert (model >= 0).all() and len(np.unique(model)) == 9      # every centre ray hits, across 9 models
    o, d = CR.camera_rays(cam, cfg, 0, pix)
    _, _, lens_model = O.intersect_rays(flat, o, d, accel=0, threads=4)
    changed = int((lens_model != model).sum())
    print(f"lens 25 changes the model of {changed} of {W * H} centre rays")
    assert 0 < changed < W * H // 20
