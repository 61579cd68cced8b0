"""Second-moment buffer, noise estimate and render-until-converged on the GPU.

The oracle renders one iteration at a time into a zero image, which gives
every iteration's per-pixel contributions c; noise_ref restates the sums of c
and c*c and the estimate in numpy float32.  The image and the moments must
match bit for bit for every pipeline count (contributions merge in iteration
order), the estimate's per-pixel float32 values exactly (the frame mean to
1e-12, which a float32 slip in one pixel exceeds by orders of magnitude) and
the tile map to one float32 ulp (the double sums' order may differ)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import noise_ref as NR
from conftest import REF_SCENE, ROOT
from helpers import assert_bitexact, flat_from_export, oracle_cfg

pytestmark = pytest.mark.gpu

W, H, BOUNCES, ITERS = 64, 48, 5, 6
UNTIL_MAX = 12                      # render_until's max_iters: contributions of iterations 0..11


@pytest.fixture(scope="module")
def scene(pt_mod):
    s = pt_mod.Scene(REF_SCENE)
    s.build()
    return s


@pytest.fixture(scope="module")
def flat(scene):
    return flat_from_export(scene.export())


def contributions(O, flat, cfg, iters):
    """Iterations 0..iters-1, one oracle render each into a zero image."""
    out = []
    for it in range(iters):
        c = oracle_cfg(cfg, threads=4)
        c.first_iter, c.iterations = it, 1
        out.append(O.render(flat, c)[0])
    return out


def make_cfg(P, accel=None, **kw):
    base = dict(width=W, height=H, max_bounces=BOUNCES, iterations=ITERS,
                accel=P.ACCEL_GRID_FAST if accel is None else accel)
    base.update(kw)
    return P.RenderConfig(**base)


@pytest.fixture(scope="module")
def contribs(pt_mod, oracle_mod, flat):
    """64x48 grid contributions of iterations 0..11 (shared; never modified)."""
    cs = contributions(oracle_mod, flat, make_cfg(pt_mod), UNTIL_MAX)
    for c in cs:
        c.setflags(write=False)
    return cs


def moments_renderer(P, scene, cfg):
    r = P.Renderer(cfg)
    r.enable_moments()
    r.allocateOnGPU(scene)
    return r


def check_noise(got, S, Q, cfg, samples, what):
    want = NR.noise(S, Q, cfg.width, cfg.height, samples)
    assert got["tiles"].shape == want["tiles"].shape and got["tiles"].dtype == np.float32, what
    ulps = NR.ulp_diff(got["tiles"], want["tiles"])
    mean64 = float(want["err"].astype(np.float64).sum() / (cfg.width * cfg.height))
    rel = abs(got["mean"] - mean64) / mean64 if mean64 else abs(got["mean"])
    print(f"{what}: tile map {ulps} ulp, mean {got['mean']!r} vs {mean64!r} (rel {rel:.3g}), "
          f"max_tile {got['max_tile']!r}")
    assert ulps <= 1, what
    assert rel <= 1e-12, what
    assert got["max_tile"] == got["tiles"].max(), what
    return want


def check_render(P, scene, cfg, cs, what):
    """Render len(cs) iterations with moments on: image, moments and estimate."""
    S, Q = NR.moment_sums(cs)
    r = moments_renderer(P, scene, cfg)
    r.renderLoop(0, len(cs))
    img, m2, got = r.image(), r.moments(), r.noise()
    same = r.noise(len(cs))
    r.free()
    assert_bitexact(img, S, f"{what}: image")
    assert_bitexact(m2, Q, f"{what}: moments")
    want = check_noise(got, S, Q, cfg, len(cs), what)
    assert same["mean"] == got["mean"] and np.array_equal(same["tiles"], got["tiles"]), what   # repeats bit for bit
    return want


@pytest.mark.parametrize("pipes", [1, 3, 16])
def test_image_moments_and_noise_match_the_oracle(gpu, pt_mod, scene, contribs, pipes):
    want = check_render(pt_mod, scene, make_cfg(pt_mod, pipelines=pipes), contribs[:ITERS], f"grid_fast p{pipes}")
    assert want["mean"] > 0 and want["max_tile"] > want["tiles"].min()       # a real, uneven noise map


def test_bvh_three_pipelines(gpu, pt_mod, oracle_mod, scene, flat):
    P = pt_mod
    cfg = make_cfg(P, accel=P.ACCEL_BVH, pipelines=3)
    check_render(P, scene, cfg, contributions(oracle_mod, flat, cfg, ITERS), "bvh p3")


@pytest.mark.parametrize("w,h,tail_drop,pipes", [(37, 23, 0, 3), (37, 23, 1, 3), (37, 23, 1, 1), (1, 1, 0, 3), (1, 1, 0, 1)])
def test_frame_shapes(gpu, pt_mod, oracle_mod, scene, flat, w, h, tail_drop, pipes):
    """Partial tiles; pixels the reference's launch truncation drops keep moment 0
    and error 0; a single pixel (3 floats: the merge's remainder path alone)."""
    P = pt_mod
    cfg = make_cfg(P, width=w, height=h, tail_drop=tail_drop, pipelines=pipes)
    cs = contributions(oracle_mod, flat, cfg, ITERS)
    want = check_render(P, scene, cfg, cs, f"{w}x{h} tail_drop={tail_drop} p{pipes}")
    if (w, h) == (37, 23):
        assert want["counts"].tolist() == [[256, 256, 80], [112, 112, 35]]
        if tail_drop:
            dropped = want["err"].reshape(-1)[(w * h // 32) * 32:]
            assert len(dropped) == 19 and not dropped.any()


def test_split_calls_clear_and_sample_count(gpu, pt_mod, scene, contribs):
    P = pt_mod
    cfg = make_cfg(P, pipelines=3)
    S, Q = NR.moment_sums(contribs[:ITERS])
    r = moments_renderer(P, scene, cfg)
    with pytest.raises(P.PathTracerError, match="need at least 2 samples"):
        r.noise()
    r.renderLoop(0, 2)
    r.renderLoop(2, 4)
    assert_bitexact(r.moments(), Q, "split calls: moments")
    assert_bitexact(r.image(), S, "split calls: image")
    check_noise(r.noise(), S, Q, cfg, ITERS, "split calls")            # the count spans both calls
    r.clearImage()
    assert not r.moments().any() and not r.image().any()
    with pytest.raises(P.PathTracerError, match="need at least 2 samples"):
        r.noise()
    r.renderLoop(0, 1)
    with pytest.raises(P.PathTracerError, match="need at least 2 samples"):
        r.noise()                                                      # the count restarted at the clear
    with pytest.raises(P.PathTracerError, match="need at least 2 samples"):
        r.noise(1)
    r.renderLoop(1, ITERS - 1)
    assert_bitexact(r.moments(), Q, "after clear: moments")
    check_noise(r.noise(), S, Q, cfg, ITERS, "after clear")
    r.free()


def test_enable_moments_after_allocate_is_refused(gpu, pt_mod, scene):
    P = pt_mod
    r = P.Renderer(make_cfg(P))
    r.allocateOnGPU(scene)
    with pytest.raises(P.PathTracerError, match="enable_moments must precede allocateOnGPU"):
        r.enable_moments()
    for call in (r.moments, lambda: r.noise(4), lambda: r.render_until(0.1, 4)):
        with pytest.raises(P.PathTracerError, match="moments not enabled"):
            call()
    r.renderLoop(0, 2)
    assert r.image().any()                       # still renders, moments off
    r.free()


@pytest.mark.parametrize("offset,pipes", [(0, 3), (1, 3), (0, 1)])
def test_caller_owned_moments_on_the_torch_stream(gpu, pt_mod, scene, contribs, offset, pipes):
    """A torch tensor as the moment buffer, read by a torch op on the same stream
    with no host synchronisation in between.  offset 1: a buffer with only 4-byte
    alignment (the scalar merge)."""
    import torch
    P = pt_mod
    cfg = make_cfg(P, pipelines=pipes)
    S, Q = NR.moment_sums(contribs[:ITERS])
    n = W * H * 3
    base = torch.zeros(n + offset, dtype=torch.float32, device=gpu)
    m2 = base[offset:]
    assert m2.data_ptr() % 16 == (4 * offset) % 16
    r = P.Renderer(cfg)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    r.enable_moments(m2.data_ptr(), keepalive=base)
    r.allocateOnGPU(scene)
    r.renderLoop(sync=False)
    got = (m2 * 1.0).cpu().numpy().reshape(-1, 3)        # torch op on the same stream: ordered after the render
    own = r.moments()
    img = r.image()
    r.free()
    assert_bitexact(got, Q, "caller-owned moments")
    assert_bitexact(own, Q, "moments() of the caller's buffer")
    assert_bitexact(img, S, "image beside caller-owned moments")


def test_render_until(gpu, pt_mod, scene, contribs):
    P = pt_mod
    cfg = make_cfg(P, pipelines=3)
    # the estimate after 2, 4, ... 12 iterations, from the oracle's contributions
    seq, sums = {}, {}
    for k in range(2, UNTIL_MAX + 1, 2):
        sums[k] = NR.moment_sums(contribs[:k])
        seq[k] = NR.noise(*sums[k], W, H, k)["mean"]
    # target: midway between two consecutive distinct values, far from every value
    # of the sequence against the 1e-12 the device mean may differ by
    a, b = seq[6], seq[8]
    assert a != b
    target = 0.5 * (a + b)
    assert min(abs(v - target) / target for v in seq.values()) > 1e-6
    stop = next(k for k in sorted(seq) if seq[k] <= target)
    assert 2 < stop < UNTIL_MAX, seq
    r = moments_renderer(P, scene, cfg)
    converged, iters, mean = r.render_until(target, UNTIL_MAX, check_every=2)
    img, m2 = r.image(), r.moments()
    print(f"render_until: target {target!r} sequence {seq} -> {converged} {iters} {mean!r}")
    assert converged is True and iters == stop
    assert abs(mean - seq[stop]) <= 1e-12 * seq[stop]
    assert_bitexact(img, sums[stop][0], "render_until: image")
    assert_bitexact(m2, sums[stop][1], "render_until: moments")
    # target 0: every chunk checks, none converges
    r.clearImage()
    converged, iters, mean = r.render_until(0.0, UNTIL_MAX, check_every=2)
    assert converged is False and iters == UNTIL_MAX
    assert abs(mean - seq[UNTIL_MAX]) <= 1e-12 * seq[UNTIL_MAX]
    assert_bitexact(r.image(), sums[UNTIL_MAX][0], "render_until to max_iters: image")
    # min_iters holds the first check back; the last chunk is cut at max_iters
    r.clearImage()
    converged, iters, mean = r.render_until(1e9, 5, min_iters=4, check_every=3)
    assert converged is True and iters == 5
    S5, Q5 = NR.moment_sums(contribs[:5])
    assert_bitexact(r.moments(), Q5, "render_until 3 + 2: moments")
    assert abs(mean - NR.noise(S5, Q5, W, H, 5)["mean"]) <= 1e-12 * mean
    r.free()


@pytest.mark.parametrize("pipes", [1, 3])
def test_graph_replay_with_moments(gpu, pt_mod, scene, contribs, monkeypatch, pipes):
    """PT_GRAPH=1: the merge runs outside the captured bounce loop, so replay needs
    no new capture; split calls replay the graphs the first call captured."""
    P = pt_mod
    monkeypatch.setenv("PT_GRAPH", "1")                  # read by allocateOnGPU
    cfg = make_cfg(P, pipelines=pipes)
    S, Q = NR.moment_sums(contribs[:ITERS])
    r = moments_renderer(P, scene, cfg)
    r.renderLoop(0, 4)
    r.renderLoop(4, 2)
    img, m2, got = r.image(), r.moments(), r.noise()
    r.free()
    assert_bitexact(img, S, f"graph p{pipes}: image")
    assert_bitexact(m2, Q, f"graph p{pipes}: moments")
    check_noise(got, S, Q, cfg, ITERS, f"graph p{pipes}")


def test_cli_noise_target(gpu, pt_mod, oracle_mod, contribs, tmp_path):
    """pathtracer_amd --noise-target: --iter is the most iterations, the iterations
    used and the estimate are printed, and the BMP is divided by the iterations
    actually rendered."""
    import re
    O = oracle_mod
    seq = {k: NR.noise(*NR.moment_sums(contribs[:k]), W, H, k)["mean"] for k in range(2, UNTIL_MAX + 1, 2)}
    target = 0.5 * (seq[6] + seq[8])
    stop = next(k for k in sorted(seq) if seq[k] <= target)
    bmp = str(tmp_path / "until.bmp")
    p = subprocess.run([os.path.join(ROOT, "pathtracerap_amd", "pathtracer_amd"), REF_SCENE, bmp, "--res", str(W), str(H),
                        "--bounces", str(BOUNCES), "--grid-fast", "--pipelines", "3", "--iter", str(UNTIL_MAX),
                        "--noise-target", repr(target), "--check-every", "2"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"Converged after (\d+) of at most (\d+) iterations: noise estimate (\S+)", p.stdout)
    assert m, p.stdout
    assert (int(m.group(1)), int(m.group(2))) == (stop, UNTIL_MAX)
    assert abs(float(m.group(3)) - seq[stop]) <= 1e-5 * seq[stop]           # printed with 6 digits
    S, _ = NR.moment_sums(contribs[:stop])
    with open(bmp, "rb") as f:
        assert f.read() == O.to_bmp_bytes(S, W, H, stop)


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
image, m2, noise = render_sharded(s, cfg, 5, moments=True)          # 3 + 2 iterations
assert image.is_cuda and m2.is_cuda
plain = render_sharded(s, cfg, 5)                                    # moments off: the image alone, as before
assert isinstance(plain, torch.Tensor) and torch.equal(plain, image)
if rank == 0:
    np.savez({out!r}, image=image.cpu().numpy(), m2=m2.cpu().numpy(), mean=noise["mean"],
             max_tile=noise["max_tile"], tiles=noise["tiles"])
dist.barrier()
dist.destroy_process_group()
"""


def test_render_sharded_moments_two_ranks(gpu, pt_mod, scene, contribs, tmp_path):
    import socket
    P = pt_mod
    out = str(tmp_path / "sharded.npz")
    script = tmp_path / "worker_moments.py"
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
    got = np.load(out)
    # the single-rank run
    r = moments_renderer(P, scene, make_cfg(P, iterations=5))
    r.renderLoop(0, 5)
    img, m2 = r.image(), r.moments()
    r.free()
    S, Q = NR.moment_sums(contribs[:5])
    assert_bitexact(img, S, "single rank: image")
    assert_bitexact(m2, Q, "single rank: moments")
    np.testing.assert_allclose(got["image"].reshape(-1, 3), img, rtol=1e-6, atol=0)
    np.testing.assert_allclose(got["m2"].reshape(-1, 3), m2, rtol=1e-6, atol=0)
    want = NR.noise(got["image"], got["m2"], W, H, 5)          # noise_ref on the reduced buffers
    print(f"sharded: mean {float(got['mean'])!r} vs noise_ref {want['mean']!r}")
    assert abs(float(got["mean"]) - want["mean"]) <= 1e-5 * want["mean"]
    assert got["tiles"].shape == want["tiles"].shape and got["max_tile"] == got["tiles"].max()
