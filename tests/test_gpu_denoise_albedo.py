"""pt_renderer_denoise_ex on the GPU: albedo demodulation and per-tile sample counts.

denoise_albedo_ref restates the two options in numpy float32 on top of denoise_ref's passes; its
inputs are what the same renderer reports through paths the other tests hold bit-exact (image(),
moments(), primary_hits(), primary_albedo(), sample_counts()), and the device's image and
variance must equal its output bit for bit.  The textured fixture is texture_scenes' torus scene
with a block of exact zeros, texels of 1e-8 inside it and a block without red in its 64 x 64 texture
(denoise_albedo_scenes.torus_spec): 6 iterations, 4 bounces."""
import os
import subprocess

import numpy as np
import pytest

import adaptive_ref as ADR
import denoise_albedo_ref as AR
import denoise_albedo_scenes as AS
import denoise_ref as DR
import texture_scenes as TS
from conftest import REF_SCENE, ROOT
from helpers import assert_bitexact

pytestmark = pytest.mark.gpu

F = np.float32
W, H, BOUNCES, ITERS = 64, 48, 4, 6
_SCENES = {}


def scene_of(P, name):
    """A named scene, built once: the textured torus fixture, the same untextured with every
    model white, the reference scene, the quality scene and a small textured face among misses."""
    if name not in _SCENES:
        if name == "torus":
            s = TS.gpu_scene(P, AS.torus_spec())
        elif name == "white":
            spec = AS.torus_spec()
            for m in spec["models"]:
                m["color"] = (1.0, 1.0, 1.0)
            s = TS.gpu_scene(P, spec, textured=False)
        elif name == "ref":
            s = P.Scene(REF_SCENE)
            s.build()
        elif name == "quality":
            s = TS.gpu_scene(P, AS.quality_spec())
        elif name == "misses":
            spec = AS.quality_spec()
            spec["models"][0].update(scale=(0.3, 0.3, 1.0), translate=(100, 150, 0))
            s = TS.gpu_scene(P, spec)
        else:
            raise ValueError(name)
        _SCENES[name] = s
    return _SCENES[name]


def half_mask(w, h, seed=20):
    """Half the tiles on, picked at random with a fixed seed."""
    ty, tx = ADR.tiles_shape(w, h)
    m = (np.random.RandomState(seed).permutation(ty * tx) < (ty * tx) // 2).reshape(ty, tx)
    assert m.any() and not m.all()
    return m


def make_cfg(P, accel=None, **kw):
    base = dict(width=W, height=H, max_bounces=BOUNCES, iterations=ITERS,
                accel=P.ACCEL_GRID_FAST if accel is None else accel)
    base.update(kw)
    return P.RenderConfig(**base)


def rendered(P, scene, cfg, iters=ITERS, first=0, env=None):
    r = P.Renderer(cfg)
    r.enable_moments()
    if env is not None:
        r.set_environment(env)
    r.allocateOnGPU(scene)
    if iters:
        r.renderLoop(first, iters)
    return r


def reference(r, flags, samples=None, **params):
    """denoise_albedo_ref on the renderer's own sums, guides, albedo and counts."""
    d, n, k = r.primary_hits()
    by_tile = bool(flags & AR.TILE_COUNTS)
    return AR.denoise(r.image(), r.moments(), r.cfg.width, r.cfg.height, None if by_tile else (samples or ITERS), d, n, k,
                      albedo=r.primary_albedo() if flags & AR.DEMODULATE else None,
                      counts=r.sample_counts() if by_tile else None, **params)


def check(r, what, flags, samples=None, **params):
    """denoise(flags=flags) == the restatement, image and variance, bit for bit."""
    img, var = r.denoise(samples=samples, variance=True, flags=flags, **params)
    want_img, want_var = reference(r, flags, samples, **params)
    assert img.shape == (r.cfg.width * r.cfg.height, 3) and img.dtype == F and var.shape == (len(img),)
    assert_bitexact(img, want_img, f"{what} flags={flags}: image")
    assert_bitexact(var, want_var, f"{what} flags={flags}: variance")
    assert np.isfinite(img).all() and np.isfinite(var).all()
    return img, var


# ---- 1. bit for bit against the restatement -------------------------------------------------------

@pytest.mark.parametrize("w,h,tail_drop", [(64, 48, 0), (37, 23, 0), (37, 23, 1), (1, 1, 0)])
def test_textured_scene_equals_the_restatement(gpu, pt_mod, w, h, tail_drop):
    """4 x 3 full tiles; partial tiles, 851 pixels (a 3-pixel remainder of the 4-per-lane prep) and
    steps 8 and 16 past the frame; the 19 pixels tail_drop leaves out; one pixel."""
    P = pt_mod
    r = rendered(P, scene_of(P, "torus"), make_cfg(P, width=w, height=h, tail_drop=tail_drop))
    try:
        plain = r.denoise(passes=6)
        for flags in (1, 2, 3):
            for passes in (1, 6):
                img, var = check(r, f"{w}x{h} tail_drop={tail_drop} passes={passes}", flags, passes=passes)
            if w > 1 and flags & 1:
                assert not np.array_equal(img, plain)         # the albedo changes what is filtered
            if tail_drop:
                live = (w * h // 32) * 32
                assert w * h - live == 19 and not img[live:].any() and not var[live:].any()
        assert r.trace_faults() == 0
    finally:
        r.free()


@pytest.mark.parametrize("variant", ["pipelines1", "pipelines16", "bvh"])
def test_textured_variants(gpu, pt_mod, variant):
    P = pt_mod
    kw = {"pipelines1": dict(pipelines=1), "pipelines16": dict(pipelines=16), "bvh": dict(accel=P.ACCEL_BVH)}[variant]
    r = rendered(P, scene_of(P, "torus"), make_cfg(P, width=37, height=23, **kw))
    try:
        for flags in (1, 2, 3):
            check(r, variant, flags)
    finally:
        r.free()


@pytest.mark.parametrize("w,h", [(64, 48), (37, 23)])
def test_identical_for_every_lds_setting(gpu, pt_mod, monkeypatch, w, h):
    """PT_DENOISE_LDS keeps its meaning: 0 and 8 give the default's bits, and a call repeats."""
    P = pt_mod
    r = rendered(P, scene_of(P, "torus"), make_cfg(P, width=w, height=h))
    try:
        want = reference(r, 3, passes=6)
        for v in ("0", "8", None):
            if v is None:
                monkeypatch.delenv("PT_DENOISE_LDS")
            else:
                monkeypatch.setenv("PT_DENOISE_LDS", v)
            for _ in range(2):
                img, var = r.denoise(passes=6, variance=True, flags=3)
                assert_bitexact(img, want[0], f"{w}x{h} PT_DENOISE_LDS={v}: image")
                assert_bitexact(var, want[1], f"{w}x{h} PT_DENOISE_LDS={v}: variance")
        monkeypatch.setenv("PT_DENOISE_LDS", "3")
        with pytest.raises(P.PathTracerError, match="PT_DENOISE_LDS must be 0, 1, 2, 4 or 8"):
            r.denoise(flags=1)
    finally:
        r.free()


def test_textured_face_among_misses_under_an_environment(gpu, pt_mod):
    """Most camera rays miss and show the environment: those pixels are not demodulated."""
    P = pt_mod
    r = rendered(P, scene_of(P, "misses"), make_cfg(P), env=AS.quality_env(P))
    try:
        k = r.primary_hits()[2]
        miss = k < 0
        assert 0.5 < miss.mean() < 0.95
        S = r.image()
        for flags in (1, 2, 3):
            img, var = check(r, "misses", flags)
            assert_bitexact(img[miss], (S / F(ITERS))[miss], "miss pixels pass through")
        assert S[miss].any()                                 # the environment is there
    finally:
        r.free()


@pytest.mark.parametrize("w,h,tail_drop", [(64, 48, 0), (37, 23, 1)])
def test_untextured_scene_takes_the_model_colours(gpu, pt_mod, w, h, tail_drop):
    """No texture in the allocation: A is ModelShade::color of the cached model."""
    P = pt_mod
    r = rendered(P, scene_of(P, "ref"), make_cfg(P, width=w, height=h, tail_drop=tail_drop))
    try:
        A, k = r.primary_albedo(), r.primary_hits()[2]
        assert len(np.unique(k[k >= 0])) > 3 and len(np.unique(A[:len(k)][k >= 0], axis=0)) > 3
        for flags in (1, 3):
            img, _ = check(r, f"untextured {w}x{h}", flags)
        assert not np.array_equal(img, r.denoise())
    finally:
        r.free()


def bound_renderer(P, scene, cfg, offset):
    """A renderer whose sums are torch tensors `offset` floats into their allocations."""
    import torch
    n = cfg.width * cfg.height * 3
    base_s = torch.zeros(n + offset, dtype=torch.float32, device="cuda")
    base_q = torch.zeros(n + offset, dtype=torch.float32, device="cuda")
    S, Q = base_s[offset:], base_q[offset:]
    assert S.data_ptr() % 16 == 4 * offset and Q.data_ptr() % 16 == 4 * offset
    r = P.Renderer(cfg)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    r.bind_image(S.data_ptr(), keepalive=base_s)
    r.enable_moments(Q.data_ptr(), keepalive=base_q)
    r.allocateOnGPU(scene)
    return r, S, Q


@pytest.mark.parametrize("offset", [0, 1])
def test_synthetic_sums_in_bound_tensors(gpu, pt_mod, offset):
    """The caller's sums with an explicit sample count, 16-byte aligned (the 4-per-lane prep) and
    4 bytes off (the scalar prep), on the textured fixture's guides and albedo; the result in a
    caller-owned buffer too.  Then a render into the same tensors, with the tiles' counts."""
    import torch
    P = pt_mod
    w, h = 37, 23
    r, S, Q = bound_renderer(P, scene_of(P, "torus"), make_cfg(P, width=w, height=h), offset)
    try:
        with pytest.raises(P.PathTracerError, match="need at least 2 samples"):
            r.denoise(flags=1)                                # nothing rendered, no count given
        k = r.primary_hits()[2]
        sa, _ = AR.sqrt_albedo(r.primary_albedo(), k)
        s0, q0, _ = DR.per_model_constant_sums(k, 8)
        s_np, q_np = (s0 * sa).astype(F), (q0 * (sa * sa)).astype(F)
        S.copy_(torch.from_numpy(s_np.reshape(-1)))
        Q.copy_(torch.from_numpy(q_np.reshape(-1)))
        check(r, f"offset {offset}: constants under the albedo", 1, samples=8)
        rs = np.random.RandomState(17)
        s_np = (rs.uniform(0, 1, (w * h, 3)) * 5).astype(F)
        q_np = (s_np * s_np / F(5) + rs.uniform(0, 250, (w * h, 3))).astype(F)
        S.copy_(torch.from_numpy(s_np.reshape(-1)))
        Q.copy_(torch.from_numpy(q_np.reshape(-1)))
        out = torch.full((w * h * 3 + 8,), -7.0, dtype=torch.float32, device=gpu)
        img = r.denoise(samples=5, passes=6, flags=1, out_ptr=out.data_ptr(), keepalive=out)
        assert_bitexact(img, reference(r, 1, samples=5, passes=6)[0], f"offset {offset}: random sums")
        got = out.cpu().numpy()
        assert_bitexact(got[:w * h * 3].reshape(-1, 3), img, "caller-owned output is the remodulated image")
        assert np.all(got[w * h * 3:] == F(-7.0))
        r.clearImage()
        r.renderLoop(0, ITERS)
        for flags in (1, 2, 3):
            check(r, f"offset {offset}: rendered", flags)
    finally:
        r.free()


@pytest.mark.parametrize("w,h", [(64, 48), (37, 23)])
def test_mixed_sample_counts(gpu, pt_mod, w, h):
    """4 iterations everywhere, then 3 under a seeded half mask: the tiles hold 4 or 7 samples."""
    P = pt_mod
    r = rendered(P, scene_of(P, "torus"), make_cfg(P, width=w, height=h), iters=0)
    try:
        r.render_masked(None, 0, 4)
        r.render_masked(half_mask(w, h), 4, 3)
        assert sorted(np.unique(r.sample_counts())) == [4, 7]
        for flags in (2, 3):
            for passes in (1, 6):
                check(r, f"mixed counts {w}x{h} passes={passes}", flags, passes=passes)
        for call in (r.denoise, lambda: r.denoise(flags=0), lambda: r.denoise(flags=1)):
            with pytest.raises(P.PathTracerError, match="tiles have different sample counts"):
                call()
        with pytest.raises(P.PathTracerError, match="PT_DENOISE_TILE_COUNTS takes every tile's own sample count"):
            r.denoise(samples=4, flags=2)
        check(r, "mixed counts, explicit samples", 1, samples=4)     # allowed, as for denoise()
        r.clearImage()
        r.render_masked(half_mask(w, h), 0, 1)
        r.render_masked(None, 1, 1)
        assert sorted(np.unique(r.sample_counts())) == [1, 2]
        for flags in (2, 3):
            with pytest.raises(P.PathTracerError, match="needs at least 2 samples in every tile"):
                r.denoise(flags=flags)
    finally:
        r.free()


# ---- 2. identities, with no tolerance -------------------------------------------------------------

def test_identities(gpu, pt_mod):
    P = pt_mod
    r = rendered(P, scene_of(P, "torus"), make_cfg(P, width=37, height=23))
    try:
        S, Q = r.image(), r.moments()
        plain = r.denoise(variance=True)
        for what, got in (("flags 0 through _ex", r.denoise(variance=True, flags=0)),
                          ("uniform counts", r.denoise(variance=True, tile_counts=True))):
            assert_bitexact(got[0], plain[0], f"{what}: image")
            assert_bitexact(got[1], plain[1], f"{what}: variance")
        A, k = r.primary_albedo(), r.primary_hits()[2]
        kk = np.full(len(A), -1, np.int32)
        kk[:len(k)] = k
        black = (A == 0) & (kk >= 0)[:, None]
        tiny = (A > 0) & (A < 1e-6)
        print(f"37x23: {black.sum()} channel values with albedo exactly 0 on a hit, {tiny.sum()} in (0, 1e-6)")
        assert black[:, 0].sum() > black[:, 1].sum() > 0        # the zero block, and the block without red
        assert tiny.sum() > 0                                   # under the floor: e = 1e-3 there
        for flags in (1, 3):
            D = r.denoise(demodulate=True, tile_counts=bool(flags & 2))
            assert (D[black] == 0).all() and np.isfinite(D).all()
        assert not (S / F(ITERS))[black].any() and plain[0][black].any()     # the plain filter bleeds light into them
        assert_bitexact(r.image(), S, "image after denoise")
        assert_bitexact(r.moments(), Q, "moments after denoise")
    finally:
        r.free()
    r = rendered(P, scene_of(P, "white"), make_cfg(P, width=37, height=23))
    try:
        A, k = r.primary_albedo(), r.primary_hits()[2]
        assert (A[k >= 0] == 1).all()
        plain, got = r.denoise(variance=True), r.denoise(variance=True, demodulate=True)
        assert_bitexact(got[0], plain[0], "all-white scene, sa = 1: image")
        assert_bitexact(got[1], plain[1], "all-white scene, sa = 1: variance")
    finally:
        r.free()


# ---- 3. refusals, times, files --------------------------------------------------------------------

def test_refusals(gpu, pt_mod):
    P = pt_mod
    scene = scene_of(P, "torus")
    r = P.Renderer(make_cfg(P))
    r.allocateOnGPU(scene)
    r.renderLoop(0, 2)
    with pytest.raises(P.PathTracerError, match="moments not enabled"):
        r.denoise(flags=3)
    r.free()
    r = rendered(P, scene, make_cfg(P), iters=1)
    try:
        for flags in (0, 1):
            for call in (lambda: r.denoise(flags=flags), lambda: r.denoise(samples=1, flags=flags)):
                with pytest.raises(P.PathTracerError, match="need at least 2 samples"):
                    call()
        with pytest.raises(P.PathTracerError, match="needs at least 2 samples in every tile"):
            r.denoise(flags=2)
        r.renderLoop(1, 1)
        for flags in (4, 5, 8 | 2, -1, 1 << 30):
            with pytest.raises(P.PathTracerError, match="denoise_ex: unknown flag bits"):
                r.denoise(flags=flags)
        with pytest.raises(P.PathTracerError, match="samples must be <= 0"):
            r.denoise(samples=2, flags=3)
        for bad in (dict(passes=0), dict(passes=7), dict(sigma_l=0.0), dict(sigma_z=float("nan")), dict(sigma_l=float("inf"))):
            with pytest.raises(P.PathTracerError, match="bad denoise parameters"):
                r.denoise(flags=3, **bad)
        with pytest.raises(P.PathTracerError, match="no timed denoise call"):
            r.denoise_times()
        assert np.isfinite(r.denoise(flags=3)).all()              # two samples are enough
    finally:
        r.free()
    r = rendered(P, scene, make_cfg(P, max_bounces=0), iters=0)   # refused before any launch: nothing is rendered
    try:
        with pytest.raises(P.PathTracerError, match="PT_DENOISE_DEMODULATE needs max_bounces >= 1"):
            r.denoise(samples=4, flags=1)
    finally:
        r.free()


def test_denoise_times_report_the_remodulation(gpu, pt_mod):
    P = pt_mod
    r = rendered(P, scene_of(P, "torus"), make_cfg(P))
    try:
        r.set_profiling(1)
        r.denoise(passes=3, demodulate=True)
        t = r.denoise_times()
        assert t["remod"] > 0 and t["prep"] > 0 and all(v > 0 for v in t["passes"][:3]) and not any(t["passes"][3:])
        assert t["total"] >= 0.99 * (t["prep"] + sum(t["passes"]) + t["remod"])
        for kw in (dict(), dict(tile_counts=True), dict(flags=0)):
            r.denoise(passes=3, **kw)
            t = r.denoise_times()
            assert t["remod"] == 0 and t["prep"] > 0 and t["total"] > 0
    finally:
        r.free()


CLI_SCENE = """
DIFFUSE
white
[0.9, 0.9, 0.9]

EMISSIVE
light
[0.99, 0.99, 0.99]

TEXTURE
check
CHECKER
[0.95, 0.9, 0.1]
[0.05, 0.1, 0.6]
8

BOX
slab
[0.4, 0.5, 0]
[-0.4, -0.15, -0.01]
material:white
texture:check

BOX
lamp
[0.3, 0.9, 0.5]
[-0.3, 0.85, 0.1]
material:light
"""


def test_bmp_and_command_line(gpu, pt_mod, tmp_path):
    """renderImageDenoised(demodulate=True) writes the restatement's D through the writer's
    conversion, and pathtracer_amd --denoise-albedo the same file for the same settings."""
    P = pt_mod
    (tmp_path / "scene.txt").write_text(CLI_SCENE)
    s = P.Scene(str(tmp_path / "scene.txt"))
    s.build()
    r = rendered(P, s, make_cfg(P, pipelines=3))
    try:
        k = r.primary_hits()[2]
        assert (k == 0).mean() > 0.3 and s.model_textures().tolist() == [0, -1]
        files = {}
        for passes in (5, 3):
            D, _ = reference(r, 1, passes=passes)
            path = str(tmp_path / f"lib{passes}.bmp")
            r.renderImageDenoised(path, passes=passes, demodulate=True)
            with open(path, "rb") as f:
                files[passes] = f.read()
            assert files[passes] == DR.bmp_bytes(D, W, H)
        assert files[5] != files[3]
        path = str(tmp_path / "plain.bmp")
        r.renderImageDenoised(path)
        with open(path, "rb") as f:
            assert f.read() != files[5]
        path = str(tmp_path / "both.bmp")
        r.renderImageDenoised(path, demodulate=True, tile_counts=True)
        with open(path, "rb") as f:
            assert f.read() == files[5]                          # uniform counts
    finally:
        r.free()
    exe = os.path.join(ROOT, "pathtracerap_amd", "pathtracer_amd")
    base = [exe, str(tmp_path / "scene.txt"), None, "--res", str(W), str(H), "--bounces", str(BOUNCES), "--grid-fast",
            "--pipelines", "3", "--iter", str(ITERS), "--denoise-albedo"]
    for passes, extra in ((5, []), (3, ["--denoise-passes", "3"])):
        bmp = str(tmp_path / f"cli{passes}.bmp")
        cmd = list(base) + extra
        cmd[2] = bmp
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        with open(bmp, "rb") as f:
            assert f.read() == files[passes], f"--denoise-albedo passes={passes}"


# ---- 4. what it is for ----------------------------------------------------------------------------

def test_demodulation_beats_the_plain_filter_on_a_textured_face(gpu, pt_mod):
    """A diffuse face filling most of the frame under a high-contrast texture with texels about 3
    pixels wide (denoise_albedo_scenes.quality_spec), 8 samples, against the mean of 512 other
    iterations, over every pixel whose primary hit is the textured face: the demodulated filter's
    error is below the plain filter's on the same sums (denoise_ref.denoise, the yardstick) and
    below the raw mean's.  The restatement's render of the same scene measured raw 0.010813,
    plain 0.004026, demodulated 0.000171 (tests/test_denoise_albedo_cpu.py)."""
    P = pt_mod
    r = rendered(P, scene_of(P, "quality"), make_cfg(P), iters=512, first=1000, env=AS.quality_env(P))
    try:
        truth = r.image() / F(512)
        r.clearImage()
        r.renderLoop(0, 8)
        S, Q = r.image(), r.moments()
        d, n, k = r.primary_hits()
        on_face = k == 0
        assert on_face.mean() > 0.9
        demod = r.denoise(demodulate=True)
        plain = r.denoise()
        assert_bitexact(plain, DR.denoise(S, Q, W, H, 8, d, n, k)[0], "the yardstick is the parent's filter")
    finally:
        r.free()
    mse = lambda a: float(((a.astype(np.float64) - truth.astype(np.float64))[on_face] ** 2).mean())
    raw = S / F(8)
    print(f"64x48, 8 samples, textured face: MSE raw {mse(raw):.6f}, plain denoise {mse(plain):.6f}, demodulated "
          f"{mse(demod):.6f}; demodulated / plain {mse(demod) / mse(plain):.4f}")
    assert mse(demod) < mse(plain)
    assert mse(demod) < mse(raw)
