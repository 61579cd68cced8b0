"""The variance-guided edge-avoiding denoiser on the GPU.

denoise_ref restates the filter in numpy float32; its inputs are what the same
renderer reports through paths the other tests hold bit-exact (image(),
moments(), primary_hits()), and the device's image and variance must equal its
output bit for bit: for every frame shape, pass count, pipeline count and
PT_DENOISE_LDS value."""
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as DR
import path_scenes as PS
from conftest import REF_SCENE, ROOT
from helpers import assert_bitexact

pytestmark = pytest.mark.gpu

F = np.float32
W, H, BOUNCES, ITERS = 64, 48, 5, 6


@pytest.fixture(scope="module")
def scene(pt_mod):
    s = pt_mod.Scene(REF_SCENE)
    s.build()
    return s


def make_cfg(P, accel=None, **kw):
    base = dict(width=W, height=H, max_bounces=BOUNCES, iterations=ITERS,
                accel=P.ACCEL_GRID_FAST if accel is None else accel)
    base.update(kw)
    return P.RenderConfig(**base)


def rendered(P, scene, cfg, iters=ITERS, first=0):
    r = P.Renderer(cfg)
    r.enable_moments()
    r.allocateOnGPU(scene)
    r.renderLoop(first, iters)
    return r


def reference(r, samples=ITERS, **params):
    """denoise_ref on the renderer's own sums and guides."""
    d, n, k = r.primary_hits()
    return DR.denoise(r.image(), r.moments(), r.cfg.width, r.cfg.height, samples, d, n, k, **params)


def check(r, what, samples=None, **params):
    """denoise(**params) == denoise_ref, image and variance, bit for bit."""
    img, var = r.denoise(samples=samples, variance=True, **params)
    want_img, want_var = reference(r, samples or ITERS, **params)
    assert img.shape == (r.cfg.width * r.cfg.height, 3) and img.dtype == F and var.shape == (len(img),)
    assert_bitexact(img, want_img, f"{what}: image")
    assert_bitexact(var, want_var, f"{what}: variance")
    return img, var


@pytest.mark.parametrize("w,h,tail_drop", [(64, 48, 0), (37, 23, 0), (37, 23, 1), (1, 1, 0)])
def test_bitexact_against_the_reference_filter(gpu, pt_mod, scene, w, h, tail_drop):
    """Aligned tiles; partial tiles, where steps 8 and 16 reach past the frame from
    every pixel; the 19 pixels tail_drop leaves out pass through as 0; one pixel."""
    P = pt_mod
    r = rendered(P, scene, make_cfg(P, width=w, height=h, tail_drop=tail_drop))
    try:
        raw = r.image() / F(ITERS)
        for passes in (1, 3, 5, 6):
            img, var = check(r, f"{w}x{h} tail_drop={tail_drop} passes={passes}", passes=passes)
            assert np.isfinite(img).all() and np.isfinite(var).all()
            if w > 1:
                assert not np.array_equal(img, raw)           # it filters
        if tail_drop:
            live = (w * h // 32) * 32
            assert w * h - live == 19 and not img[live:].any() and not var[live:].any()
    finally:
        r.free()


@pytest.mark.parametrize("variant", ["pipelines1", "bvh", "sigmas"])
def test_bitexact_variants(gpu, pt_mod, scene, variant):
    P = pt_mod
    kw, params = {}, {}
    if variant == "pipelines1":
        kw = dict(pipelines=1)
    elif variant == "bvh":
        kw = dict(accel=P.ACCEL_BVH)
    else:
        params = dict(sigma_l=1.5, sigma_z=0.25, passes=4)
    r = rendered(P, scene, make_cfg(P, width=37, height=23, **kw))
    try:
        check(r, variant, **params)
    finally:
        r.free()


@pytest.mark.parametrize("w,h", [(64, 48), (37, 23)])
def test_identical_for_every_lds_setting(gpu, pt_mod, scene, monkeypatch, w, h):
    """PT_DENOISE_LDS (read at every call) picks the passes that stage their tile in
    LDS: the result does not depend on it, and a second call repeats bit for bit."""
    P = pt_mod
    r = rendered(P, scene, make_cfg(P, width=w, height=h))
    try:
        want_img, want_var = reference(r, passes=6)
        for v in ("0", "1", "2", "4", "8", None):
            if v is None:
                monkeypatch.delenv("PT_DENOISE_LDS")
            else:
                monkeypatch.setenv("PT_DENOISE_LDS", v)
            img, var = r.denoise(passes=6, variance=True)
            assert_bitexact(img, want_img, f"{w}x{h} PT_DENOISE_LDS={v}: image")
            assert_bitexact(var, want_var, f"{w}x{h} PT_DENOISE_LDS={v}: variance")
            again = r.denoise(passes=6, variance=True)
            assert_bitexact(again[0], img, "second call: image")
            assert_bitexact(again[1], var, "second call: variance")
        monkeypatch.setenv("PT_DENOISE_LDS", "3")
        with pytest.raises(P.PathTracerError, match="PT_DENOISE_LDS must be 0, 1, 2, 4 or 8"):
            r.denoise()
    finally:
        r.free()


def miss_scene_spec():
    """Most camera rays miss: a small emissive quad in front of the camera (the triangle
    test is one-sided, so a second one back to back with it lights what lies behind) and
    a diffuse quad behind it to the side, whose paths end on the emitter or leave the scene."""
    quad = PS._quads([0.0], 1.0)
    lamp = dict(mesh=0, scale=(0.1, 0.1, 0.1), translate=(-60, 120, 300), material="EMISSIVE", color=(0.99, 0.9, 0.8))
    return [quad], [dict(lamp, rot=(0, 0, 0)), dict(lamp, rot=(0, 180, 0), translate=(-60, 120, 299)),
                    dict(mesh=0, scale=(0.2, 0.2, 0.2), rot=(0, 20, 0), translate=(150, 100, 100), material="DIFFUSE",
                         color=(0.8, 0.7, 0.6))]


def test_scene_with_misses(gpu, pt_mod):
    P = pt_mod
    s = PS.scene_from_spec(P, *miss_scene_spec())
    r = rendered(P, s, make_cfg(P))
    try:
        d, n, k = r.primary_hits()
        miss = k < 0
        assert miss.mean() > 0.5 and set(np.unique(k)) == {-1, 0, 2}     # the camera sees the lamp's front and the quad
        S, Q = r.image(), r.moments()
        _, V0 = DR.prep(S, Q, ITERS)
        assert (V0[k == 2] > 0).mean() > 0.1                            # noise to filter
        img, var = check(r, "misses")
        assert np.isfinite(img).all() and np.isfinite(var).all()
        assert_bitexact(img[miss], (S / F(ITERS))[miss], "miss pixels pass through")
        assert var[k == 2].max() < V0[k == 2].max()
    finally:
        r.free()


def bound_renderer(P, scene, cfg):
    """A renderer whose image and moment sums are torch tensors."""
    import torch
    n = cfg.width * cfg.height * 3
    S = torch.zeros(n, dtype=torch.float32, device="cuda")
    Q = torch.zeros(n, dtype=torch.float32, device="cuda")
    r = P.Renderer(cfg)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    r.bind_image(S.data_ptr(), keepalive=S)
    r.enable_moments(Q.data_ptr(), keepalive=Q)
    r.allocateOnGPU(scene)
    return r, S, Q


def test_synthetic_sums_in_bound_tensors(gpu, pt_mod, scene):
    """The caller's sums (as after a reduction over shards) with an explicit sample
    count, on the reference scene's real guides."""
    import torch
    P = pt_mod
    cfg = make_cfg(P)
    r, S, Q = bound_renderer(P, scene, cfg)
    try:
        with pytest.raises(P.PathTracerError, match="need at least 2 samples"):
            r.denoise()                                      # nothing rendered, no count given
        d, n, k = r.primary_hits()
        assert len(np.unique(k[k >= 0])) > 3
        # a constant per model, channel variance 50: stays within 2e-5 of the constant
        s_np, q_np, _ = DR.per_model_constant_sums(k, 8)
        S.copy_(torch.from_numpy(s_np.reshape(-1)))
        Q.copy_(torch.from_numpy(q_np.reshape(-1)))
        img, var = check(r, "per-model constants", samples=8)
        DR.check_per_model_constants(img, var, s_np, q_np, k, 8)
        # random sums with large second moments
        rs = np.random.RandomState(17)
        s_np = (rs.uniform(0, 1, (W * H, 3)) * 5).astype(F)
        q_np = (s_np * s_np / F(5) + rs.uniform(0, 250, (W * H, 3))).astype(F)
        S.copy_(torch.from_numpy(s_np.reshape(-1)))
        Q.copy_(torch.from_numpy(q_np.reshape(-1)))
        img, var = check(r, "random sums", samples=5, passes=6)
        assert var.max() > 1.0
    finally:
        r.free()


def test_unaligned_bound_sums_take_the_scalar_prep(gpu, pt_mod, scene):
    """Sums with 4-byte alignment only (k_denoise_prep<false>)."""
    import torch
    P = pt_mod
    cfg = make_cfg(P, width=37, height=23)
    n = 37 * 23 * 3
    base_s = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
    base_q = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
    S, Q = base_s[1:], base_q[1:]
    assert S.data_ptr() % 16 == 4
    r = P.Renderer(cfg)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    r.bind_image(S.data_ptr(), keepalive=base_s)
    r.enable_moments(Q.data_ptr(), keepalive=base_q)
    r.allocateOnGPU(scene)
    try:
        r.renderLoop(0, ITERS)
        check(r, "unaligned sums")
    finally:
        r.free()


def test_error_reduction(gpu, pt_mod, scene):
    """8 samples against the mean of 512 other iterations: the filtered image's error
    is under half the raw mean's (the cap of the CPU test; the filter measured 0.121)."""
    P = pt_mod
    cfg = make_cfg(P)
    r = rendered(P, scene, cfg, iters=512, first=1000)
    truth = r.image() / F(512)
    r.clearImage()
    r.renderLoop(0, 8)
    raw = r.image() / F(8)
    D = r.denoise()
    r.free()
    mse = lambda a: float(((a.astype(np.float64) - truth.astype(np.float64)) ** 2).mean())
    ratio = mse(D) / mse(raw)
    print(f"64x48, 8 samples: MSE(denoised) / MSE(raw) = {ratio:.4f}")
    assert ratio < 0.5


def test_caller_owned_output_and_untouched_sums(gpu, pt_mod, scene):
    import torch
    P = pt_mod
    r = rendered(P, scene, make_cfg(P, width=37, height=23))
    try:
        S, Q = r.image(), r.moments()
        out = torch.full((37 * 23 * 3 + 8,), -7.0, dtype=torch.float32, device=gpu)
        img = r.denoise(out_ptr=out.data_ptr(), keepalive=out)
        got = out.cpu().numpy()
        assert_bitexact(got[:37 * 23 * 3].reshape(-1, 3), img, "caller-owned output")
        assert np.all(got[37 * 23 * 3:] == F(-7.0))             # nothing past W*H*3
        assert_bitexact(r.image(), S, "image after denoise")
        assert_bitexact(r.moments(), Q, "moments after denoise")
        assert_bitexact(r.denoise(), img, "without out_ptr")
    finally:
        r.free()


def test_refusals(gpu, pt_mod, scene):
    P = pt_mod
    r = P.Renderer(make_cfg(P))
    r.allocateOnGPU(scene)
    r.renderLoop(0, 2)
    with pytest.raises(P.PathTracerError, match="moments not enabled"):
        r.denoise()
    r.free()
    r = P.Renderer(make_cfg(P))
    r.enable_moments()
    r.allocateOnGPU(scene)
    try:
        r.renderLoop(0, 1)
        for call in (r.denoise, lambda: r.denoise(samples=1)):
            with pytest.raises(P.PathTracerError, match="need at least 2 samples"):
                call()
        r.renderLoop(1, 1)
        for bad in (dict(passes=0), dict(passes=7), dict(sigma_l=0.0), dict(sigma_z=0.0), dict(sigma_l=float("nan")),
                    dict(sigma_z=float("nan")), dict(sigma_l=float("inf")), dict(sigma_z=-1.0)):
            with pytest.raises(P.PathTracerError, match="bad denoise parameters"):
                r.denoise(**bad)
        with pytest.raises(P.PathTracerError, match="no timed denoise call"):
            r.denoise_times()
        assert np.isfinite(r.denoise()).all()                  # two samples are enough
    finally:
        r.free()


def test_denoise_times_under_profiling(gpu, pt_mod, scene):
    P = pt_mod
    r = rendered(P, scene, make_cfg(P))
    try:
        r.set_profiling(1)
        r.denoise(passes=3)
        t = r.denoise_times()
        assert t["prep"] > 0 and all(v > 0 for v in t["passes"][:3]) and not any(t["passes"][3:])
        assert t["total"] >= 0.99 * (t["prep"] + sum(t["passes"]))      # float milliseconds
    finally:
        r.free()


def test_bmp_and_command_line(gpu, pt_mod, scene, tmp_path):
    """renderImageDenoised writes the reference image through the writer's conversion,
    and pathtracer_amd --denoise the same file for the same settings."""
    P = pt_mod
    r = rendered(P, scene, make_cfg(P, pipelines=3))
    try:
        files = {}
        for passes in (5, 3):
            D, _ = reference(r, passes=passes)
            path = str(tmp_path / f"lib{passes}.bmp")
            r.renderImageDenoised(path, passes=passes)
            with open(path, "rb") as f:
                files[passes] = f.read()
            assert files[passes] == DR.bmp_bytes(D, W, H)
        assert files[5] != files[3]
    finally:
        r.free()
    exe = os.path.join(ROOT, "pathtracerap_amd", "pathtracer_amd")
    base = [exe, REF_SCENE, None, "--res", str(W), str(H), "--bounces", str(BOUNCES), "--grid-fast", "--pipelines", "3",
            "--iter", str(ITERS), "--denoise"]
    for passes, extra in ((5, []), (3, ["--denoise-passes", "3"])):
        bmp = str(tmp_path / f"cli{passes}.bmp")
        cmd = list(base) + extra
        cmd[2] = bmp
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        with open(bmp, "rb") as f:
            assert f.read() == files[passes], f"--denoise passes={passes}"
