"""Pixel-jittered camera rays on the GPU (include/pathtracer_amd.h,
pt_renderer_set_pixel_jitter), against the restatement in jitter_ref.py (which
tests/test_jitter_ref.py holds to adaptive_ref's and through it to the oracle).

S (image), Q (moments), the per-tile sample counts, the segment count and the per-bounce
segment counts are compared bit for bit.  Estimates read back from the device are held to
the bounds of tests/test_gpu_adaptive.py and tests/test_gpu_noise.py for the same
reasons: the per-pixel float32 values are exact, the order of the double sums may differ."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import adaptive_ref as AR
import denoise_ref as DR
import jitter_ref as JR
import noise_ref as NR
from conftest import REF_SCENE, ROOT
from helpers import assert_bitexact, flat_from_export, oracle_cfg

pytestmark = pytest.mark.gpu

W, H, BOUNCES = 64, 48, 5


@pytest.fixture(scope="module")
def scene(pt_mod):
    s = pt_mod.Scene(REF_SCENE)
    s.build()
    return s


@pytest.fixture(scope="module")
def flat(scene):
    return flat_from_export(scene.export())


def make_cfg(P, accel=None, **kw):
    base = dict(width=W, height=H, max_bounces=BOUNCES, iterations=6,
                accel=P.ACCEL_GRID_FAST if accel is None else accel)
    base.update(kw)
    return P.RenderConfig(**base)


def renderer(P, scene, cfg, width=None, moments=True):
    r = P.Renderer(cfg)
    if moments:
        r.enable_moments()
    if width is not None:
        r.set_pixel_jitter(width)                    # before allocateOnGPU
    r.allocateOnGPU(scene)
    return r


def restatement(flat, cfg, width=None):
    return JR.Restatement(flat, oracle_cfg(cfg, threads=4), width=width)


_REFS = {}


def plain_ref(flat, cfg, width, first=0, n=3):
    """The restated jittered render of iterations [first, first + n) (shared; never modified).
    GRID and GRID_FAST share the oracle's accel 0."""
    o = oracle_cfg(cfg, threads=4)
    key = (o.width, o.height, o.accel, o.tail_drop, o.max_bounces, float(width), first, n)
    if key not in _REFS:
        ref = restatement(flat, cfg, width)
        ref.render(first, n)
        _REFS[key] = ref
    return _REFS[key]


def check_state(r, ref, what):
    assert_bitexact(r.image(), ref.S, f"{what}: image")
    assert_bitexact(r.moments(), ref.Q, f"{what}: moments")
    assert_bitexact(r.sample_counts(), ref.counts, f"{what}: counts")
    assert r.segments() == ref.segments, (what, r.segments(), ref.segments)
    assert r.segments_per_bounce(10) == ref.per_bounce[:10].tolist(), what


def half_mask(w, h, seed=20):
    ty, tx = AR.tiles_shape(w, h)
    m = (np.random.RandomState(seed).permutation(ty * tx) < (ty * tx) // 2).reshape(ty, tx)
    assert m.any() and not m.all()
    return m


def one_tile(w, h, t):
    m = np.zeros(AR.tiles_shape(w, h), bool)
    m.reshape(-1)[t] = True
    return m


# ---- 4. on with width 0 is renderLoop ------------------------------------------------------

WIDTH0 = [("grid_fast", 1, 64, True), ("grid_fast", 3, 64, True), ("grid_fast", 16, 64, True),
          ("grid", 3, 64, True), ("bvh", 3, 64, True),
          ("grid_fast", 1, 64, False), ("grid_fast", 16, 64, False),       # direct add / k_merge
          ("grid_fast", 3, 128, True), ("grid_fast", 3, 256, True)]


@pytest.mark.parametrize("accel,pipes,block,moments", WIDTH0)
def test_width_zero_equals_render_loop(gpu, pt_mod, scene, accel, pipes, block, moments):
    P = pt_mod
    cfg = make_cfg(P, accel={"grid_fast": P.ACCEL_GRID_FAST, "grid": P.ACCEL_GRID, "bvh": P.ACCEL_BVH}[accel],
                   pipelines=pipes, block=block)
    out = []
    for width in (None, 0.0):
        r = renderer(P, scene, cfg, width, moments)
        assert r.pixel_jitter() == (width is not None, 1.0 if width is None else 0.0)
        r.renderLoop(0, 4)
        out.append((r.image(), r.moments() if moments else None, r.segments(), r.segments_per_bounce(8)))
        r.free()
    (img, m2, seg, per), (jimg, jm2, jseg, jper) = out
    what = f"{accel} p{pipes} block {block} moments {moments}"
    assert img.any()
    assert_bitexact(jimg, img, f"{what}: image")
    if moments:
        assert m2.any()
        assert_bitexact(jm2, m2, f"{what}: moments")
    assert jseg == seg + 4 * W * H
    assert jper == [4 * W * H] + per[:7]                 # the traced camera rays are bounce 1


# ---- 5. width > 0 is the restatement --------------------------------------------------------

@pytest.mark.parametrize("accel", ["grid_fast", "grid", "bvh"])
def test_width_one_equals_the_restatement(gpu, pt_mod, scene, flat, accel):
    P = pt_mod
    cfg = make_cfg(P, accel={"grid_fast": P.ACCEL_GRID_FAST, "grid": P.ACCEL_GRID, "bvh": P.ACCEL_BVH}[accel], pipelines=3)
    ref = plain_ref(flat, cfg, 1.0)
    r = renderer(P, scene, cfg, 1.0)
    r.renderLoop(0, 3)
    check_state(r, ref, f"{accel} width 1")
    r.free()
    unjittered = plain_ref(flat, cfg, 0.0)
    assert not np.array_equal(ref.S, unjittered.S)       # it moves the rays


@pytest.mark.parametrize("tail_drop", [0, 1])
def test_partial_blocks_and_tail_drop(gpu, pt_mod, scene, flat, tail_drop):
    P = pt_mod
    cfg = make_cfg(P, width=37, height=23, tail_drop=tail_drop, pipelines=3)
    ref = plain_ref(flat, cfg, 1.0)
    r = renderer(P, scene, cfg, 1.0)
    r.renderLoop(0, 3)
    check_state(r, ref, f"37x23 tail_drop={tail_drop}")
    r.free()
    assert ref.n_launch == (832 if tail_drop else 851)   # 13 blocks exactly / a partial last block
    if tail_drop:
        assert not ref.S[832:].any()


@pytest.mark.parametrize("width", [0.5, 2.0])
def test_other_widths(gpu, pt_mod, scene, flat, width):
    P = pt_mod
    cfg = make_cfg(P, pipelines=3)
    r = renderer(P, scene, cfg)
    r.set_pixel_jitter(width)                            # after allocateOnGPU
    assert r.pixel_jitter() == (True, width)
    r.renderLoop(0, 3)
    check_state(r, plain_ref(flat, cfg, width), f"width {width}")
    r.free()


def test_iteration_ids_from_254(gpu, pt_mod, scene, flat):
    P = pt_mod
    cfg = make_cfg(P, pipelines=3)
    r = renderer(P, scene, cfg, 1.0)
    r.renderLoop(254, 3)                                 # 254, 255, 256
    check_state(r, plain_ref(flat, cfg, 1.0, first=254), "iterations 254..256")
    r.free()


def test_sorting_the_camera_rays_changes_nothing(gpu, pt_mod, scene, flat, monkeypatch):
    """By default the generated rays, in pixel order already, are traced unsorted at
    bounce 1; PT_JITTER_SORT=1 sorts them like every later bounce's."""
    P = pt_mod
    monkeypatch.setenv("PT_JITTER_SORT", "1")            # read by allocateOnGPU
    cfg = make_cfg(P, pipelines=3)
    r = renderer(P, scene, cfg, 1.0)
    r.renderLoop(0, 3)
    check_state(r, plain_ref(flat, cfg, 1.0), "PT_JITTER_SORT=1")
    r.free()


# ---- 6. masks with jitter --------------------------------------------------------------------

@pytest.fixture(scope="module")
def masked_sequence(pt_mod, flat):
    """2 jittered iterations, 3 under half_mask, 1 more (shared; never modified)."""
    mask = half_mask(W, H)
    ref = restatement(flat, make_cfg(pt_mod), 1.0)
    ref.render(0, 2)
    ref.render(2, 3, mask)
    ref.render(5, 1)
    return mask, ref


@pytest.mark.parametrize("pipes", [1, 16])
def test_random_mask_between_plain_iterations(gpu, pt_mod, scene, masked_sequence, pipes):
    P = pt_mod
    mask, ref = masked_sequence
    r = renderer(P, scene, make_cfg(P, pipelines=pipes), 1.0)
    r.renderLoop(0, 2)
    before = r.image(), r.moments()
    r.render_masked(mask, 2, 3)
    after = r.image(), r.moments()
    r.renderLoop(5, 1)
    off = ~mask.reshape(-1)[AR.pixel_tiles(W, H)]
    assert off.any() and not off.all()
    assert_bitexact(after[0][off], before[0][off], f"p{pipes}: inactive tiles' image across the masked call")
    assert_bitexact(after[1][off], before[1][off], f"p{pipes}: inactive tiles' moments across the masked call")
    assert not np.array_equal(after[0][~off], before[0][~off])
    check_state(r, ref, f"masked sequence p{pipes}")
    r.free()


def test_one_tile_of_twelve(gpu, pt_mod, scene, flat):
    P = pt_mod
    cfg = make_cfg(P, pipelines=3)
    mask = one_tile(W, H, 5)
    ref = restatement(flat, cfg, 1.0)
    ref.render(0, 3, mask)
    print(f"live rays per bounce {ref.live}")
    assert all(live[0] == 256 for live in ref.live)      # a full tile emits its 256 rays: 16 of 48 blocks hold 16 each
    r = renderer(P, scene, cfg, 1.0)
    r.render_masked(mask, 0, 3)
    check_state(r, ref, "one tile of twelve")
    r.free()


def test_one_partial_edge_tile(gpu, pt_mod, scene, flat):
    P = pt_mod
    cfg = make_cfg(P, width=37, height=23, pipelines=3)
    mask = one_tile(37, 23, 5)                           # 5 x 7 pixels
    ref = restatement(flat, cfg, 1.0)
    ref.render(0, 3, mask)
    assert all(live[0] == 35 for live in ref.live)       # less than one block from the start
    r = renderer(P, scene, cfg, 1.0)
    r.render_masked(mask, 0, 3)
    check_state(r, ref, "one partial edge tile")
    r.free()


def test_empty_mask_changes_nothing(gpu, pt_mod, scene):
    P = pt_mod
    r = renderer(P, scene, make_cfg(P, pipelines=3), 1.0)
    r.renderLoop(0, 2)
    before = r.image(), r.moments(), r.sample_counts(), r.segments()
    r.render_masked(np.zeros(AR.tiles_shape(W, H), np.uint8), 2, 3)
    assert_bitexact(r.image(), before[0], "empty mask: image")
    assert_bitexact(r.moments(), before[1], "empty mask: moments")
    assert_bitexact(r.sample_counts(), before[2], "empty mask: counts")
    assert r.segments() == before[3]
    r.free()


def test_two_masks_without_synchronize(gpu, pt_mod, scene, flat):
    P = pt_mod
    cfg = make_cfg(P, pipelines=16)
    a, b = half_mask(W, H, seed=1), half_mask(W, H, seed=2)
    assert (a != b).any()
    ref = restatement(flat, cfg, 1.0)
    ref.render(0, 3, a)
    ref.render(3, 3, b)
    r = renderer(P, scene, cfg, 1.0)
    r.render_masked(a, 0, 3, sync=False)
    r.render_masked(b, 3, 3)
    check_state(r, ref, "two masks")
    r.free()


# ---- 7. switching ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def switching_ref(pt_mod, flat):
    ref = restatement(flat, make_cfg(pt_mod))
    ref.render(0, 2)
    ref.set_pixel_jitter(1.0)
    ref.render(2, 2)
    ref.set_pixel_jitter(1.0, on=False)
    ref.render(4, 2)
    return ref


def run_switching(P, scene):
    r = renderer(P, scene, make_cfg(P, pipelines=16))
    r.renderLoop(0, 2, sync=False)
    r.set_pixel_jitter(1.0)
    r.renderLoop(2, 2, sync=False)
    r.set_pixel_jitter(1.0, on=False)
    assert r.pixel_jitter() == (False, 1.0)
    r.renderLoop(4, 2)
    return r


def test_switching_without_synchronize(gpu, pt_mod, scene, switching_ref):
    r = run_switching(pt_mod, scene)
    check_state(r, switching_ref, "off, on, off")
    r.free()


def test_switching_around_graph_replay(gpu, pt_mod, scene, switching_ref, monkeypatch):
    """Jittered iterations are enqueued directly; the graphs captured by the first two
    unjittered iterations are replayed by the last two."""
    monkeypatch.setenv("PT_GRAPH", "1")                  # read by allocateOnGPU
    r = run_switching(pt_mod, scene)
    check_state(r, switching_ref, "PT_GRAPH=1: off, on, off")
    r.free()


# ---- 8. render_until and render_adaptive ----------------------------------------------------

UNTIL_MAX = 12


def test_render_until(gpu, pt_mod, scene, flat):
    P = pt_mod
    cfg = make_cfg(P, pipelines=3)
    ref = restatement(flat, cfg, 1.0)
    seq, sums = {}, {}
    for k in range(2, UNTIL_MAX + 1, 2):
        ref.render(k - 2, 2)
        sums[k] = ref.S.copy(), ref.Q.copy()
        seq[k] = NR.noise(ref.S, ref.Q, W, H, k)["mean"]
    target = 0.5 * (seq[6] + seq[8])
    margin = min(abs(v - target) / target for v in seq.values())
    stop = next(k for k in sorted(seq) if seq[k] <= target)
    print(f"render_until: target {target!r}, margin {margin:.3g}, sequence {seq}, stop {stop}")
    assert margin > 0.01                                 # the device mean may differ by 1e-12 relative
    assert 2 < stop < UNTIL_MAX
    r = renderer(P, scene, cfg, 1.0)
    converged, iters, mean = r.render_until(target, UNTIL_MAX, check_every=2)
    assert converged is True and iters == stop
    assert abs(mean - seq[stop]) <= 1e-12 * seq[stop]
    assert_bitexact(r.image(), sums[stop][0], "render_until: image")
    assert_bitexact(r.moments(), sums[stop][1], "render_until: moments")
    r.free()


ADAPT = dict(max_iters=12, min_iters=4, check_every=2)


def adaptive_margin(res, target):
    return min(np.abs(t.astype(np.float64) - target).min() / target for _, t, _ in res["checks"])


def test_render_adaptive(gpu, pt_mod, scene, flat):
    """The target: the middle of a gap of the first check's sorted tile errors (the first
    check does not depend on the target), the widest gap for which no tile error of any
    check of the restated loop lies within 1 % of it (the device's may differ by 1 ulp)."""
    P = pt_mod
    cfg = make_cfg(P, pipelines=3)
    first = restatement(flat, cfg, 1.0).render_adaptive(-1.0, 4, min_iters=4, check_every=2)
    e = np.sort(first["checks"][0][1].reshape(-1).astype(np.float64))
    for k in np.argsort(-np.diff(e), kind="stable"):
        target = 0.5 * (e[k] + e[k + 1])
        ref = restatement(flat, cfg, 1.0)
        want = ref.render_adaptive(target, **ADAPT)
        if adaptive_margin(want, target) > 0.01:
            break
    margin = adaptive_margin(want, target)
    active = [int(m.sum()) for _, _, m in want["checks"]]
    print(f"target {target!r}, margin {margin:.3g}, active tiles after each check {active}")
    assert margin > 0.01
    assert 0 < active[0] < 12                            # a tile went off at the first check, one stayed on
    r = renderer(P, scene, cfg, 1.0)
    converged, iters, samples, mean = r.render_adaptive(target, **ADAPT)
    assert (converged, iters, samples) == (want["converged"], want["iters"], want["pixel_samples"])
    assert abs(mean - want["mean"]) <= 1e-12 * want["mean"]
    assert samples < iters * W * H
    check_state(r, ref, "render_adaptive")
    r.free()


# ---- 9. the denoiser after jittered iterations ------------------------------------------------

def test_denoise_reads_the_pixel_corner_guides(gpu, pt_mod, scene, flat):
    P = pt_mod
    cfg = make_cfg(P, pipelines=3)
    r = renderer(P, scene, cfg, 1.0)                     # never renders an unjittered iteration
    r.renderLoop(0, 6)
    ref = plain_ref(flat, cfg, 1.0, n=6)
    S, Q = r.image(), r.moments()
    assert_bitexact(S, ref.S, "image")
    assert_bitexact(Q, ref.Q, "moments")
    d, n, k = r.primary_hits()
    assert_bitexact(d, ref.hit_dist, "guides: the unjittered primary hit's distance")
    assert_bitexact(n, ref.hit_nrm, "guides: its normal")
    assert_bitexact(k, ref.hit_model, "guides: its model")
    img, var = r.denoise(variance=True)
    r.free()
    want_img, want_var = DR.denoise(S, Q, W, H, 6, d, n, k)
    assert_bitexact(img, want_img, "denoise: image")
    assert_bitexact(var, want_var, "denoise: variance")


# ---- 10. Python, the command line and sharding --------------------------------------------------

def test_cli_jitter(gpu, pt_mod, oracle_mod, flat, tmp_path):
    P = pt_mod
    ref = plain_ref(flat, make_cfg(P), 1.0, n=6)
    bmp = str(tmp_path / "jitter.bmp")
    p = subprocess.run([os.path.join(ROOT, "pathtracerap_amd", "pathtracer_amd"), REF_SCENE, bmp, "--res", str(W), str(H),
                        "--bounces", str(BOUNCES), "--grid-fast", "--pipelines", "3", "--iter", "6", "--jitter", "1"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    with open(bmp, "rb") as f:
        assert f.read() == oracle_mod.to_bmp_bytes(ref.S, W, H, 6)


SHARD_WORKER = r"""
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
cfg = P.RenderConfig(width={w}, height={h}, iterations=5, max_bounces={bounces})
image = render_sharded(s, cfg, 5, jitter=1.0)                        # 3 + 2 iterations
assert image.is_cuda
if rank == 0:
    np.save({out!r}, image.cpu().numpy())
dist.barrier()
dist.destroy_process_group()
"""


def test_render_sharded_two_ranks(gpu, pt_mod, scene, flat, tmp_path):
    P = pt_mod
    out = str(tmp_path / "sharded.npy")
    script = tmp_path / "worker_jitter.py"
    script.write_text(SHARD_WORKER.format(root=ROOT, scene=REF_SCENE, w=W, h=H, bounces=BOUNCES, out=out))
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=240)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    got = np.load(out).reshape(-1, 3)
    cfg = make_cfg(P, iterations=5)
    r = renderer(P, scene, cfg, 1.0, moments=False)
    r.renderLoop(0, 5)
    single = r.image()
    r.free()
    assert_bitexact(single, plain_ref(flat, cfg, 1.0, n=5).S, "single rank: image")
    np.testing.assert_allclose(got, single, rtol=1e-6, atol=0)
