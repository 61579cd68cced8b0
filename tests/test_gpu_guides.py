"""Sampled first-hit guides on the GPU (pt_renderer_enable_guides, PT_DENOISE_SAMPLED_GUIDES).

Every case renders a few generated (jittered or lens) iterations and holds, bit for bit against
guides_ref's restatement of the same iterations: the sums G (guides()), the guide counts, S and Q,
and then denoise(sampled_guides=True) image and variance, with and without demodulate and
tile_counts, against guides_ref.denoise on the restatement's sums."""
import os
import subprocess

import numpy as np
import pytest

import camera_ref as CR
import denoise_albedo_scenes as AS
import denoise_ref as DR
import env_ref as ER
import guides_ref as GR
import texture_scenes as TS
from conftest import REF_SCENE, ROOT
from helpers import assert_bitexact, flat_from_export, oracle_cfg
from test_gpu_dist import _run_ranks

pytestmark = pytest.mark.gpu

F = np.float32
W, H, BOUNCES, ITERS = 64, 48, 3, 6
VIEW = dict(eye=(0, 800, 500), target=(0, 0, 0), vfov_deg=45, focus_dist=900)
_SCENES = {}


def fixture(P, name):
    """(scene, FlatScene, spec) of a named scene, built once: the reference scene, the smooth and
    textured torus fixture, and the quality scene (a textured face against a sky)."""
    if name not in _SCENES:
        if name == "ref":
            s = P.Scene(REF_SCENE)
            s.build()
            spec = dict(smooth=None, binding=None, textures=[], uv=None)
        else:
            spec = dict(TS.fixture_spec() if name == "torus" else AS.quality_spec())
            s = TS.gpu_scene(P, spec)
            spec["uv"] = TS.vertex_uv(spec)
        _SCENES[name] = (s, flat_from_export(s.export()), spec)
    return _SCENES[name]


def make_cfg(P, **kw):
    base = dict(width=W, height=H, max_bounces=BOUNCES, iterations=ITERS, accel=P.ACCEL_GRID_FAST)
    base.update(kw)
    return P.RenderConfig(**base)


def camera_of(P, cfg, opt):
    if not opt.get("view"):
        return None
    return P.look_at(lens_radius=opt.get("lens", 0.0), width=cfg.width, height=cfg.height, **VIEW)


def env_of(P, opt):
    return AS.quality_env(P) if opt.get("env") else None


def renderer(P, name, cfg, opt, guides=True, bind=None):
    """An allocated renderer with moments and (guides) guides on; opt: jitter (a width), view, lens, env."""
    r = P.Renderer(cfg)
    r.enable_moments()
    if bind is not None:
        r.enable_guides(bind.data_ptr(), keepalive=bind)
    elif guides:
        r.enable_guides()
    cam = camera_of(P, cfg, opt)
    if cam is not None:
        r.set_camera(cam)
    if opt.get("jitter") is not None:
        r.set_pixel_jitter(opt["jitter"])
    if opt.get("env"):
        r.set_environment(env_of(P, opt))
    r.allocateOnGPU(fixture(P, name)[0])
    return r


def restatement(P, name, cfg, opt):
    _, flat, spec = fixture(P, name)
    cam, env = camera_of(P, cfg, opt), env_of(P, opt)
    return GR.Restatement(flat, oracle_cfg(cfg, threads=4), width=opt.get("jitter"),
                          camera=None if cam is None else CR.Cam.of(cam), env=None if env is None else ER.Env.of(env),
                          smooth=spec["smooth"], uv=spec["uv"], textures=spec["textures"], binding=spec["binding"])


_REFS = {}


def restated(P, name, cfg, opt, iters=ITERS):
    """The restated render of iterations [0, iters) (shared; never modified)."""
    o = oracle_cfg(cfg, threads=4)
    key = (name, o.width, o.height, o.accel, o.tail_drop, o.max_bounces, iters, tuple(sorted(opt.items())))
    if key not in _REFS:
        ref = restatement(P, name, cfg, opt)
        ref.render(0, iters)
        assert ref.tex_ident.holds() and ref.ident.holds()
        _REFS[key] = ref
    return _REFS[key]


def check_sums(r, ref, what):
    g = r.guides()
    assert g["normal"].shape == (ref.npix, 3) and g["depth"].shape == (ref.npix,) and g["hits"].dtype == F
    got = np.concatenate([g["normal"], g["depth"][:, None], g["sqrt_albedo"], g["hits"][:, None]], axis=1)
    assert_bitexact(got, ref.G, f"{what}: G")
    assert_bitexact(r.guide_counts(), ref.guide_counts, f"{what}: guide counts")
    assert_bitexact(r.sample_counts(), ref.counts, f"{what}: sample counts")
    assert_bitexact(r.image(), ref.S, f"{what}: image")
    assert_bitexact(r.moments(), ref.Q, f"{what}: moments")
    assert r.trace_faults() == 0, what


def check_denoise(r, ref, what, flag_sets=(4, 5, 6, 7), samples=None, passes=(5,)):
    """denoise with the sampled guides == the restatement on the restatement's own sums."""
    w, h = r.cfg.width, r.cfg.height
    out = {}
    for flags in flag_sets:
        for np_ in passes:
            by_tile = bool(flags & GR.TILE_COUNTS)
            n = None if by_tile else (samples or int(ref.counts.max()))
            want = GR.denoise(ref.S, ref.Q, ref.G, w, h, samples=n, counts=ref.counts if by_tile else None, flags=flags,
                              passes=np_)
            img, var = r.denoise(samples=None if by_tile else samples, passes=np_, variance=True,
                                 demodulate=bool(flags & 1), tile_counts=by_tile, sampled_guides=True)
            assert_bitexact(img, want[0], f"{what} flags={flags} passes={np_}: image")
            assert_bitexact(var, want[1], f"{what} flags={flags} passes={np_}: variance")
            out[flags] = img
    return out


def check(P, name, cfg, opt, what, iters=ITERS, **kw):
    ref = restated(P, name, cfg, opt, iters)
    r = renderer(P, name, cfg, opt)
    try:
        r.renderLoop(0, iters)
        check_sums(r, ref, what)
        out = check_denoise(r, ref, what, **kw)
    finally:
        r.free()
    return ref, out


# ---- 1. bit for bit against the restatement -------------------------------------------------------

@pytest.mark.parametrize("pipes", [1, 3, 16])
@pytest.mark.parametrize("accel", ["grid_fast", "bvh"])
def test_reference_scene_under_jitter(gpu, pt_mod, accel, pipes):
    P = pt_mod
    cfg = make_cfg(P, accel=P.ACCEL_BVH if accel == "bvh" else P.ACCEL_GRID_FAST, pipelines=pipes)
    ref, out = check(P, "ref", cfg, dict(jitter=1.0), f"ref {accel} pipelines={pipes}")
    h = ref.G[:, 7]
    assert (h == ITERS).all()                                    # a closed room: every sample hits
    short = np.sqrt((ref.G[:, 0:3].astype(np.float64) ** 2).sum(axis=1)) / h
    assert (short < 0.99).any() and (short > 0.999).any()        # anti-aliased edges mix orientations: a short mean normal
    assert not np.array_equal(out[4], out[5])


def test_partial_tiles_with_pipelines_reused(gpu, pt_mod):
    """37 x 23 = 851 pixels (no multiple of 64 or 4), 19 iterations on 16 pipelines: three
    pipelines merge twice, in iteration order."""
    P = pt_mod
    check(P, "torus", make_cfg(P, width=37, height=23, pipelines=16), dict(jitter=1.0), "37x23 x19", iters=19,
          passes=(1, 6))


def test_tail_drop_leaves_the_last_pixels_without_records(gpu, pt_mod):
    P = pt_mod
    ref, out = check(P, "torus", make_cfg(P, width=37, height=23, tail_drop=1), dict(jitter=1.0), "37x23 tail_drop")
    assert ref.n_launch == 832 and not ref.G[832:].any()
    assert_bitexact(out[5][832:], (ref.S / F(ITERS))[832:], "dropped pixels copy through")


def test_one_pixel(gpu, pt_mod):
    P = pt_mod
    check(P, "torus", make_cfg(P, width=1, height=1), dict(jitter=1.0), "1x1")


def test_sorted_first_pass_takes_the_slot_map(gpu, pt_mod, monkeypatch):
    """PT_JITTER_SORT=1: pass 1 is sorted, so k_guide_first finds its ray through slot_src."""
    P = pt_mod
    monkeypatch.setenv("PT_JITTER_SORT", "1")
    check(P, "torus", make_cfg(P), dict(jitter=1.0), "PT_JITTER_SORT=1", flag_sets=(7,))


def test_graph_mode_enqueues_generated_iterations_directly(gpu, pt_mod, monkeypatch):
    P = pt_mod
    monkeypatch.setenv("PT_GRAPH", "1")
    check(P, "torus", make_cfg(P), dict(jitter=1.0), "PT_GRAPH=1", flag_sets=(5,))


@pytest.mark.parametrize("opt", [dict(view=1, lens=25.0), dict(view=1, lens=25.0, jitter=1.0), dict(view=1, jitter=1.0)],
                         ids=["lens", "lens+jitter", "look_at+jitter"])
def test_cameras(gpu, pt_mod, opt):
    P = pt_mod
    check(P, "torus", make_cfg(P), opt, str(opt), flag_sets=(5, 7))


def test_quality_scene_under_its_environment(gpu, pt_mod):
    """Most top-corner rays miss: pixels with h = 0 copy through, pixels with 0 < h < n are
    demodulated by a mix of the face's albedo and 1."""
    P = pt_mod
    ref, out = check(P, "quality", make_cfg(P, max_bounces=4), dict(jitter=1.0, env=1), "quality")
    h = ref.G[:, 7]
    assert (h == 0).any() and ((h > 0) & (h < ITERS)).any()
    assert_bitexact(out[5][h == 0], (ref.S / F(ITERS))[h == 0], "no sample hit: the mean")


def test_masks_and_tile_counts(gpu, pt_mod):
    """A checkerboard of tiles, its complement, the checkerboard again: the per-pipeline buffers
    hold the other mask's records for the inactive pixels, which must not be added."""
    P = pt_mod
    cfg = make_cfg(P, pipelines=3)
    opt = dict(jitter=1.0)
    ref = restatement(P, "torus", cfg, opt)
    ty, tx = ref.counts.shape
    a = (np.add.outer(np.arange(ty), np.arange(tx)) % 2) == 0
    r = renderer(P, "torus", cfg, opt)
    try:
        for first, n, m in ((0, 2, a), (2, 2, ~a), (4, 1, a)):
            r.render_masked(m, first, n)
            ref.render(first, n, m)
        check_sums(r, ref, "masks")
        assert set(ref.guide_counts.reshape(-1).tolist()) == {2, 3}
        check_denoise(r, ref, "masks", flag_sets=(6, 7))
        with pytest.raises(P.PathTracerError, match="different sample counts"):
            r.denoise(sampled_guides=True)
    finally:
        r.free()


@pytest.mark.parametrize("offset", [0, 1])
def test_caller_owned_guides(gpu, pt_mod, offset):
    """G in a torch tensor, 16-byte aligned and 4 bytes off (the scalar merge and prep)."""
    import torch
    P = pt_mod
    cfg = make_cfg(P, width=37, height=23)
    opt = dict(jitter=1.0)
    ref = restated(P, "torus", cfg, opt)
    base = torch.zeros(37 * 23 * 8 + offset, dtype=torch.float32, device="cuda")
    G = base[offset:]
    assert G.data_ptr() % 16 == 4 * offset
    r = renderer(P, "torus", cfg, opt, bind=G)
    try:
        r.renderLoop(0, ITERS)
        check_sums(r, ref, f"offset {offset}")
        assert_bitexact(G.cpu().numpy().reshape(-1, 8), ref.G, "the caller's tensor")
        check_denoise(r, ref, f"offset {offset}", flag_sets=(5, 7))
    finally:
        r.free()


def test_clear_and_set_camera_zero_the_sums_and_two_loops_equal_one(gpu, pt_mod):
    P = pt_mod
    cfg = make_cfg(P, width=37, height=23)
    opt = dict(jitter=1.0)
    ref = restated(P, "torus", cfg, opt)
    r = renderer(P, "torus", cfg, opt)
    try:
        r.renderLoop(0, 2)
        r.renderLoop(2, ITERS - 2)
        check_sums(r, ref, "two loops")
        r.clearImage()
        assert not any(v.any() for v in r.guides().values()) and not r.guide_counts().any()
        r.renderLoop(0, ITERS)
        check_sums(r, ref, "after clearImage")
        r.set_camera(P.look_at(width=37, height=23, **VIEW))
        assert not any(v.any() for v in r.guides().values()) and not r.guide_counts().any()
        r.set_camera(None)
        r.renderLoop(0, ITERS)
        check_sums(r, ref, "after set_camera")
        r.set_environment(AS.quality_env(P))
        assert not any(v.any() for v in r.guides().values()) and not r.guide_counts().any()
    finally:
        r.free()


def test_guides_on_never_changes_the_existing_outputs(gpu, pt_mod):
    P = pt_mod
    cfg = make_cfg(P, width=37, height=23)
    opt = dict(jitter=1.0)
    got = []
    for guides in (False, True):
        r = renderer(P, "torus", cfg, opt, guides=guides)
        try:
            r.renderLoop(0, ITERS)
            got.append([r.image(), r.moments()] + [np.concatenate(r.denoise(variance=True, flags=f), axis=None)
                                                   for f in (0, 1, 2, 3)])
        finally:
            r.free()
    for a, b, what in zip(got[0], got[1], ("S", "Q", "flags 0", "flags 1", "flags 2", "flags 3")):
        assert_bitexact(b, a, f"guides on: {what}")


# ---- 2. refusals ------------------------------------------------------------------------------------

def test_refusals(gpu, pt_mod, monkeypatch):
    P = pt_mod
    scene = fixture(P, "torus")[0]
    r = P.Renderer(make_cfg(P))
    r.enable_guides()
    with pytest.raises(P.PathTracerError, match="guides need moments"):
        r.allocateOnGPU(scene)
    r.free()
    for accel, var in ((P.ACCEL_GRID, None), (P.ACCEL_GRID_FAST, "PT_GF_SPLIT"), (P.ACCEL_BVH, "PT_TRACE_SPLIT")):
        if var:
            monkeypatch.setenv(var, "0")
        r = P.Renderer(make_cfg(P, accel=accel))
        r.enable_moments()
        r.enable_guides()
        with pytest.raises(P.PathTracerError, match="guides need the split trace"):
            r.allocateOnGPU(scene)
        r.free()
        if var:
            monkeypatch.delenv(var)
    r = renderer(P, "torus", make_cfg(P), dict(jitter=1.0), guides=False)
    try:
        r.renderLoop(0, 2)
        with pytest.raises(P.PathTracerError, match="guides not enabled"):
            r.denoise(sampled_guides=True)
        with pytest.raises(P.PathTracerError, match="guides not enabled"):
            r.guides()
        with pytest.raises(P.PathTracerError, match="guides not enabled"):
            r.guide_counts()
        with pytest.raises(P.PathTracerError, match="enable_guides must precede allocateOnGPU"):
            r.enable_guides()
    finally:
        r.free()
    r = renderer(P, "torus", make_cfg(P), dict(jitter=1.0))
    try:
        r.renderLoop(0, 2)
        r.set_pixel_jitter(on=False)
        r.renderLoop(2, 1)                                       # an ordinary iteration: a sample without a record
        assert (r.sample_counts() == 3).all() and (r.guide_counts() == 2).all()
        with pytest.raises(P.PathTracerError, match="every sample since the last clear must be a generated"):
            r.denoise(sampled_guides=True)
        with pytest.raises(P.PathTracerError, match="every sample since the last clear must be a generated"):
            r.denoise(sampled_guides=True, tile_counts=True)
        assert np.isfinite(r.denoise(samples=3, sampled_guides=True)).all()       # the caller vouches
        with pytest.raises(P.PathTracerError, match="unknown flag bits"):
            r.denoise(flags=8 | 4)
    finally:
        r.free()


def test_denoise_times_count_the_guided_prep(gpu, pt_mod):
    P = pt_mod
    r = renderer(P, "torus", make_cfg(P), dict(jitter=1.0))
    try:
        r.renderLoop(0, 2)
        r.set_profiling(1)
        r.denoise(passes=3, demodulate=True, sampled_guides=True)
        t = r.denoise_times()
        assert t["prep"] > 0 and t["remod"] > 0 and all(v > 0 for v in t["passes"][:3]) and not any(t["passes"][3:])
    finally:
        r.free()


# ---- 3. sharded sums and the command line -----------------------------------------------------------

WORKER = r"""
import os, sys
sys.path.insert(0, {root!r})
import numpy as np
import torch
import torch.distributed as dist
import pathtracerap_amd as P
from pathtracerap_amd.dist import render_sharded
rank = int(os.environ["RANK"])
dist.init_process_group("gloo")
torch.cuda.set_device(0)
s = P.Scene({scene!r})
s.build()
cfg = P.RenderConfig(width=64, height=48, iterations=5, max_bounces=3)
img, m2, g, noise = render_sharded(s, cfg, 5, moments=True, jitter=1.0, guides=True)
assert g.is_cuda and g.numel() == 64 * 48 * 8
if rank == 0:
    np.save({out!r}, g.cpu().numpy())
dist.barrier()
dist.destroy_process_group()
"""


def test_render_sharded_two_ranks(gpu, pt_mod, tmp_path):
    """Two gloo ranks sharing the card render 3 + 2 jittered iterations; the all-reduced G equals the
    single-rank sums up to float32 summation order (rtol 1e-6, as for the image in test_gpu_dist)."""
    P = pt_mod
    out = str(tmp_path / "g.npy")
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, scene=REF_SCENE, out=out))
    _run_ranks(script, timeout=120)
    got = np.load(out).reshape(-1, 8)
    r = renderer(P, "ref", make_cfg(P, iterations=5), dict(jitter=1.0))
    try:
        r.renderLoop(0, 5)
        g = r.guides()
    finally:
        r.free()
    want = np.concatenate([g["normal"], g["depth"][:, None], g["sqrt_albedo"], g["hits"][:, None]], axis=1)
    assert np.abs(got).sum() > 0
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6)


def test_command_line(gpu, pt_mod, tmp_path):
    """pathtracer_amd --denoise-guides writes renderImageDenoised(sampled_guides=True)'s bytes, and
    is refused without --jitter or a lens."""
    from test_gpu_denoise_albedo import CLI_SCENE
    P = pt_mod
    (tmp_path / "scene.txt").write_text(CLI_SCENE)
    s = P.Scene(str(tmp_path / "scene.txt"))
    s.build()
    r = P.Renderer(make_cfg(P, pipelines=3))
    r.enable_moments()
    r.enable_guides()
    r.set_pixel_jitter(1.0)
    r.allocateOnGPU(s)
    try:
        r.renderLoop(0, ITERS)
        files = {}
        for demod in (False, True):
            path = str(tmp_path / f"lib{demod}.bmp")
            r.renderImageDenoised(path, demodulate=demod, sampled_guides=True)
            files[demod] = open(path, "rb").read()
            D = r.denoise(demodulate=demod, sampled_guides=True)
            assert files[demod] == DR.bmp_bytes(D, W, H)
        assert files[False] != files[True]
    finally:
        r.free()
    exe = os.path.join(ROOT, "pathtracerap_amd", "pathtracer_amd")
    base = [exe, str(tmp_path / "scene.txt"), None, "--res", str(W), str(H), "--bounces", str(BOUNCES), "--grid-fast",
            "--pipelines", "3", "--iter", str(ITERS), "--denoise-guides"]
    for demod, extra in ((False, ["--jitter", "1"]), (True, ["--jitter", "1", "--denoise-albedo"])):
        bmp = str(tmp_path / f"cli{demod}.bmp")
        cmd = list(base) + extra
        cmd[2] = bmp
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        assert open(bmp, "rb").read() == files[demod], f"--denoise-guides {extra}"
    cmd = list(base)
    cmd[2] = str(tmp_path / "never.bmp")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--denoise-guides needs --jitter or a lens" in p.stderr
    assert not (tmp_path / "never.bmp").exists()


# ---- 4. what it is for ------------------------------------------------------------------------------

def test_quality_on_the_textured_face_against_a_sky(gpu, pt_mod):
    """denoise_albedo_scenes.quality_spec at 64 x 48, jitter 1.0, 8 samples, against the mean of 512
    other jittered iterations: (a) PT_DENOISE_DEMODULATE with the centre ray's guides, (b) the same
    with PT_DENOISE_SAMPLED_GUIDES, over the whole frame and over the pixels whose sampled record
    differs from the centre ray's (0 < Hc < n, or the centre ray misses while Hc > 0).  The figures
    are the restatement's (the images are bit-equal); (b) is below (a) on the differing pixels, and
    over the frame no worse than (a) by more than what two disjoint 512-iteration means differ by
    for (a): the yardstick's own noise.  Measured figures: DESIGN.md, "Sampled first-hit guides"."""
    import denoise_albedo_ref as AR
    P = pt_mod
    cfg = make_cfg(P, max_bounces=4)
    opt = dict(jitter=1.0, env=1)
    n = 8
    r = renderer(P, "quality", cfg, opt)
    try:
        truths = []
        for first in (1000, 2000):
            r.renderLoop(first, 512)
            truths.append((r.image() / F(512)).astype(np.float64))
            r.clearImage()
        r.renderLoop(0, n)
        S, Q, g = r.image(), r.moments(), r.guides()
        G = np.concatenate([g["normal"], g["depth"][:, None], g["sqrt_albedo"], g["hits"][:, None]], axis=1)
        d, nn, k = r.primary_hits()
        a = r.denoise(demodulate=True)
        b = r.denoise(demodulate=True, sampled_guides=True)
        assert_bitexact(a, AR.denoise(S, Q, W, H, n, d, nn, k, albedo=r.primary_albedo())[0], "(a) is the restatement's")
        assert_bitexact(b, GR.denoise(S, Q, G, W, H, samples=n, flags=5)[0], "(b) is the restatement's")
    finally:
        r.free()
    ref = restated(P, "quality", cfg, opt, iters=n)
    assert_bitexact(S, ref.S, "S")
    assert_bitexact(G, ref.G, "G")
    h = G[:, 7]
    differ = ((h > 0) & (h < n)) | ((k < 0) & (h > 0))
    assert differ.sum() > 50
    mse = lambda img, t, sel: float(((img.astype(np.float64) - t)[sel] ** 2).mean())
    every = np.ones(len(h), bool)
    fig = {(nm, reg): mse(img, truths[0], sel) for nm, img in (("a", a), ("b", b))
           for reg, sel in (("frame", every), ("differ", differ))}
    yard = abs(mse(a, truths[0], every) - mse(a, truths[1], every))
    print(f"quality 64x48 jitter 1.0, {n} samples, {differ.sum()} differing pixels: MSE frame (a) {fig['a', 'frame']:.6g} "
          f"(b) {fig['b', 'frame']:.6g}; differing (a) {fig['a', 'differ']:.6g} (b) {fig['b', 'differ']:.6g}; "
          f"yardstick noise {yard:.3g}")
    assert fig["b", "differ"] < fig["a", "differ"]
    assert fig["b", "frame"] <= fig["a", "frame"] + yard
