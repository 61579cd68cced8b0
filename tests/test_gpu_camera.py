"""The free camera with a thin lens on the GPU (include/pathtracer_amd.h,
pt_renderer_set_camera), against the restatement in camera_ref.py (which
tests/test_camera_ref.py holds to jitter_ref's and adaptive_ref's and through them to the
oracle) and, for the legacy-equivalent camera, against the renderer without a camera.

S (image), Q (moments), the per-tile sample counts, the segment count and the per-bounce
segment counts are compared bit for bit."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import adaptive_ref as AR
import camera_ref as CR
import denoise_ref as DR
from conftest import REF_SCENE, ROOT
from helpers import assert_bitexact, flat_from_export, oracle_cfg

pytestmark = pytest.mark.gpu

W, H, BOUNCES, LENS = 64, 48, 5, 25.0
VIEW_A = dict(eye=(0, 800, 500), target=(0, 0, 0), vfov_deg=45, focus_dist=900)
VIEW_B = dict(eye=(650, 200, 650), target=(0, 0, 0), vfov_deg=45)
VIEWS = {"A": VIEW_A, "B": VIEW_B}


@pytest.fixture(scope="module")
def scene(pt_mod):
    s = pt_mod.Scene(REF_SCENE)
    s.build()
    return s


@pytest.fixture(scope="module")
def flat(scene):
    return flat_from_export(scene.export())


def accel_of(P, name):
    return {"grid_fast": P.ACCEL_GRID_FAST, "grid": P.ACCEL_GRID, "bvh": P.ACCEL_BVH}[name]


def make_cfg(P, accel="grid_fast", **kw):
    base = dict(width=W, height=H, max_bounces=BOUNCES, iterations=3, accel=accel_of(P, accel))
    base.update(kw)
    return P.RenderConfig(**base)


def view(P, name, cfg, lens=0.0):
    return P.look_at(lens_radius=lens, width=cfg.width, height=cfg.height, **VIEWS[name])


def renderer(P, scene, cfg, cam=None, jitter=None, moments=True):
    r = P.Renderer(cfg)
    if moments:
        r.enable_moments()
    if cam is not None:
        r.set_camera(cam)                                # before allocateOnGPU
    if jitter is not None:
        r.set_pixel_jitter(jitter)
    r.allocateOnGPU(scene)
    return r


def one_tile(w, h, t):
    m = np.zeros(AR.tiles_shape(w, h), bool)
    m.reshape(-1)[t] = True
    return m


def half_mask(w, h, seed=20):
    ty, tx = AR.tiles_shape(w, h)
    m = (np.random.RandomState(seed).permutation(ty * tx) < (ty * tx) // 2).reshape(ty, tx)
    assert m.any() and not m.all()
    return m


_REFS = {}


def restated(P, flat, cfg, name, lens, jitter, first=0, n=3, mask_tile=None):
    """The restated render of iterations [first, first + n) through view `name` (shared; never
    modified).  GRID and GRID_FAST share the oracle's accel 0."""
    o = oracle_cfg(cfg, threads=4)
    key = (o.width, o.height, o.accel, o.tail_drop, name, lens, jitter, first, n, mask_tile)
    if key not in _REFS:
        ref = CR.Restatement(flat, o, width=jitter, camera=CR.Cam.of(view(P, name, cfg, lens)))
        ref.render(first, n, None if mask_tile is None else one_tile(o.width, o.height, mask_tile))
        _REFS[key] = ref
    return _REFS[key]


def check_state(r, ref, what):
    assert_bitexact(r.image(), ref.S, f"{what}: image")
    assert_bitexact(r.moments(), ref.Q, f"{what}: moments")
    assert_bitexact(r.sample_counts(), ref.counts, f"{what}: counts")
    assert r.segments() == ref.segments, (what, r.segments(), ref.segments)
    assert r.segments_per_bounce(10) == ref.per_bounce[:10].tolist(), what


def state(r):
    return (r.image(), r.moments(), r.sample_counts(), r.segments(), r.segments_per_bounce(10)) + r.primary_hits()


STATE = ("image", "moments", "counts", "segments", "segments per bounce", "primary hit distance",
         "primary hit normal", "primary hit model")


def assert_same_state(got, want, what):
    for g, w, name in zip(got, want, STATE):
        if isinstance(w, np.ndarray):
            assert_bitexact(g, w, f"{what}: {name}")
        else:
            assert g == w, (what, name, g, w)


# ---- 1. the legacy-equivalent camera is the legacy camera ------------------------------------

def legacy_sequence(P, scene, cfg, with_camera):
    """Jitter off and width 1, every tile and a random half: four renders of 3 iterations."""
    r = renderer(P, scene, cfg)
    if with_camera:
        on, cam = r.camera()
        assert on is False
        r.set_camera(cam)                                # after allocateOnGPU
        assert r.camera() == (True, cam)
    out = []
    for jitter in (None, 1.0):
        for mask in (None, half_mask(W, H)):
            r.clearImage()
            r.set_pixel_jitter(1.0 if jitter is None else jitter, on=jitter is not None)
            if mask is None:
                r.renderLoop(0, 3)
            else:
                r.render_masked(mask, 0, 3)
            out.append(state(r))
    r.free()
    return out


@pytest.mark.parametrize("accel,pipes", [("grid_fast", 1), ("grid_fast", 3), ("grid_fast", 16), ("grid", 3), ("bvh", 3)])
def test_legacy_equivalent_camera(gpu, pt_mod, scene, accel, pipes):
    P = pt_mod
    cfg = make_cfg(P, accel, pipelines=pipes)
    want = legacy_sequence(P, scene, cfg, False)
    got = legacy_sequence(P, scene, cfg, True)
    assert want[0][0].any() and not np.array_equal(want[0][0], want[2][0])
    for k, label in enumerate(("plain", "half mask", "jitter 1", "jitter 1, half mask")):
        assert_same_state(got[k], want[k], f"{accel} p{pipes} {label}")


GRAPH_WORKER = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import pathtracerap_amd as P
import test_gpu_camera as T
s = P.Scene({scene!r})
s.build()
out = T.legacy_sequence(P, s, T.make_cfg(P, pipelines=16), True)
np.savez({out!r}, **{{f"{{k}}_{{i}}": np.asarray(v) for k, st in enumerate(out) for i, v in enumerate(st)}})
"""


def test_legacy_equivalent_camera_under_graph_replay(gpu, pt_mod, scene, tmp_path):
    """The camera's renders in a process of their own that has PT_GRAPH=1 from its start."""
    P = pt_mod
    want = legacy_sequence(P, scene, make_cfg(P, pipelines=16), False)
    out = str(tmp_path / "graph.npz")
    script = tmp_path / "worker_graph.py"
    script.write_text(GRAPH_WORKER.format(root=ROOT, tests=os.path.join(ROOT, "tests"), scene=REF_SCENE, out=out))
    p = subprocess.run([sys.executable, str(script)], env=dict(os.environ, PT_GRAPH="1"), capture_output=True, text=True,
                       timeout=240)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.load(out)
    for k, label in enumerate(("plain", "half mask", "jitter 1", "jitter 1, half mask")):
        for i, (w, name) in enumerate(zip(want[k], STATE)):
            assert_bitexact(got[f"{k}_{i}"], np.asarray(w), f"PT_GRAPH=1 {label}: {name}")


# ---- 2. free views are the restatement ---------------------------------------------------------

# view, lens, jitter, accel, (width, height, tail_drop), first iteration, masked tile, pipelines
FULL = (W, H, 0)
CASES = [("A", 0.0, None, "grid_fast", FULL, 0, None, 3),
         ("A", 0.0, 1.0, "grid_fast", FULL, 0, None, 1),
         ("A", LENS, None, "grid_fast", FULL, 0, None, 16),
         ("A", LENS, 1.0, "grid_fast", FULL, 0, None, 3),
         ("B", 0.0, None, "grid_fast", FULL, 0, None, 16),
         ("B", 0.0, 1.0, "grid_fast", FULL, 0, None, 3),
         ("B", LENS, None, "grid_fast", FULL, 0, None, 1),
         ("B", LENS, 1.0, "grid_fast", FULL, 0, None, 3),
         ("A", LENS, None, "grid", FULL, 0, None, 3),
         ("B", 0.0, None, "grid", FULL, 0, None, 3),
         ("A", 0.0, None, "bvh", FULL, 0, None, 3),
         ("B", LENS, 1.0, "bvh", FULL, 0, None, 3),
         ("A", LENS, 1.0, "grid_fast", (37, 23, 0), 0, None, 3),
         ("B", LENS, None, "grid_fast", (37, 23, 1), 0, None, 3),
         ("A", 0.0, None, "grid_fast", (37, 23, 1), 0, None, 3),
         ("B", 0.0, 1.0, "grid_fast", (37, 23, 0), 0, None, 3),
         ("A", 0.0, None, "grid_fast", FULL, 254, None, 3),
         ("B", LENS, 1.0, "grid_fast", FULL, 254, None, 3),
         ("A", LENS, None, "grid_fast", FULL, 0, 5, 3),
         ("B", 0.0, None, "grid_fast", FULL, 0, 5, 16),
         ("B", LENS, 1.0, "grid_fast", FULL, 0, 5, 1)]


@pytest.mark.parametrize("name,lens,jitter,accel,size,first,tile,pipes", CASES)
def test_free_view_equals_the_restatement(gpu, pt_mod, scene, flat, name, lens, jitter, accel, size, first, tile, pipes):
    P = pt_mod
    cfg = make_cfg(P, accel, width=size[0], height=size[1], tail_drop=size[2], pipelines=pipes)
    ref = restated(P, flat, cfg, name, lens, jitter, first=first, mask_tile=tile)
    r = renderer(P, scene, cfg, view(P, name, cfg, lens), jitter)
    if tile is None:
        r.renderLoop(first, 3)
    else:
        r.render_masked(one_tile(cfg.width, cfg.height, tile), first, 3)
    check_state(r, ref, f"view {name} lens {lens} jitter {jitter} {accel} {size} from {first} tile {tile} p{pipes}")
    r.free()
    assert ref.S.any()
    if size[2]:
        assert ref.n_launch == 832 and not ref.S[832:].any()
    if lens or jitter:
        assert ref.per_bounce[0] == 3 * ref.n_launch     # the generated rays are bounce 0, the traced ones bounce 1
        if tile is None:
            assert ref.per_bounce[1] == 3 * ref.n_launch
    if name == "B" and tile is None and not lens and not jitter:
        assert (ref.hit_model < 0).any()                 # view B looks past the room's edge: some centre rays miss


def test_the_lens_and_the_views_differ(gpu, pt_mod, flat):
    """What the cases above compare against is not one image: the restated renders of the two
    views, and of a view with and without the lens, differ."""
    P = pt_mod
    cfg = make_cfg(P)
    a, al = restated(P, flat, cfg, "A", 0.0, None), restated(P, flat, cfg, "A", LENS, None)
    b = restated(P, flat, cfg, "B", 0.0, None)
    assert not np.array_equal(a.S, al.S) and not np.array_equal(a.S, b.S)
    assert (a.hit_model >= 0).all() and len(np.unique(a.hit_model)) == 9
    assert len(np.unique(b.hit_model[b.hit_model >= 0])) == 6


def test_empty_mask_changes_nothing(gpu, pt_mod, scene):
    P = pt_mod
    cfg = make_cfg(P, pipelines=3)
    r = renderer(P, scene, cfg, view(P, "A", cfg, LENS))
    r.renderLoop(0, 2)
    before = r.image(), r.moments(), r.sample_counts(), r.segments()
    r.render_masked(np.zeros(AR.tiles_shape(W, H), np.uint8), 2, 3)
    assert_bitexact(r.image(), before[0], "empty mask: image")
    assert_bitexact(r.moments(), before[1], "empty mask: moments")
    assert_bitexact(r.sample_counts(), before[2], "empty mask: counts")
    assert r.segments() == before[3]
    r.free()


# ---- 3. the cache and the denoiser's guides are the pinhole's ------------------------------------

def test_primary_hits_and_denoise_after_set_camera(gpu, pt_mod, scene, flat):
    P = pt_mod
    cfg = make_cfg(P, pipelines=3)
    cam = view(P, "A", cfg, LENS)
    r = renderer(P, scene, cfg)
    r.renderLoop(0, 2)                                   # the legacy cache is built, then invalidated
    r.set_camera(cam)
    d, n, k = r.primary_hits()                           # rebuilt by the first call that needs it
    o, dirs = CR.camera_rays(CR.pinhole(CR.Cam.of(cam)), oracle_cfg(cfg), 0, np.arange(W * H))
    for got, want, what in zip((d, n, k), r.intersect_rays(o, dirs), ("distance", "normal", "model")):
        assert_bitexact(got, want, f"cache = intersect_rays of the pinhole centre rays: {what}")
    ref = restated(P, flat, cfg, "A", LENS, None, n=6)
    assert_bitexact(d, ref.hit_dist, "guides: the pinhole hit's distance")
    assert_bitexact(n, ref.hit_nrm, "guides: its normal")
    assert_bitexact(k, ref.hit_model, "guides: its model")
    r.renderLoop(0, 6)                                   # only iterations through the lens
    S, Q = r.image(), r.moments()
    assert_bitexact(S, ref.S, "image")
    assert_bitexact(Q, ref.Q, "moments")
    img, var = r.denoise(variance=True)
    r.free()
    want_img, want_var = DR.denoise(S, Q, W, H, 6, d, n, k)
    assert_bitexact(img, want_img, "denoise: image")
    assert_bitexact(var, want_var, "denoise: variance")


# ---- 4. switching -----------------------------------------------------------------------------------

def fresh(P, scene, cfg, cam):
    r = renderer(P, scene, cfg, cam)
    r.renderLoop(0, 3)
    out = r.image(), r.moments(), r.sample_counts()
    r.free()
    return out


def assert_render(r, want, what):
    for got, w, name in zip((r.image(), r.moments(), r.sample_counts()), want, STATE):
        assert_bitexact(got, w, f"{what}: {name}")


def test_switching_without_synchronize(gpu, pt_mod, scene):
    P = pt_mod
    cfg = make_cfg(P, pipelines=16)
    a, b = view(P, "A", cfg), view(P, "B", cfg, LENS)    # a pinhole (the cached path) and a lens (the generated one)
    want = {k: fresh(P, scene, cfg, c) for k, c in (("legacy", None), ("A", a), ("B", b))}
    assert not np.array_equal(want["A"][0], want["legacy"][0]) and not np.array_equal(want["A"][0], want["B"][0])
    r = renderer(P, scene, cfg)
    r.renderLoop(0, 3, sync=False)
    r.set_camera(a)
    r.renderLoop(0, 3, sync=False)
    assert_render(r, want["A"], "legacy -> A")
    r.renderLoop(3, 2, sync=False)
    r.set_camera(b)
    for got, name in zip((r.image(), r.moments(), r.sample_counts()), STATE):
        assert not got.any(), f"after set_camera the {name} must read zero"
    r.renderLoop(0, 3, sync=False)
    r.set_camera(a)
    r.renderLoop(0, 3, sync=False)
    r.set_camera(b)
    r.renderLoop(0, 3, sync=False)
    assert_render(r, want["B"], "A -> B -> A -> B")
    r.set_camera(None)
    assert r.camera()[0] is False
    r.renderLoop(0, 3, sync=False)
    assert_render(r, want["legacy"], "B -> NULL")
    r.free()


def test_switching_pinhole_views_under_graph_replay(gpu, pt_mod, scene, flat, monkeypatch):
    """Captured launches hold the camera pointer by value: a switch must drop the graphs."""
    P = pt_mod
    cfg = make_cfg(P, pipelines=16)
    monkeypatch.setenv("PT_GRAPH", "1")                  # read by allocateOnGPU
    r = renderer(P, scene, cfg)
    r.renderLoop(0, 3, sync=False)                       # the legacy camera's graphs
    r.set_camera(view(P, "A", cfg))
    r.renderLoop(0, 3, sync=False)
    ref = restated(P, flat, cfg, "A", 0.0, None)
    assert_render(r, (ref.S, ref.Q, ref.counts), "PT_GRAPH=1 legacy -> A")
    r.set_camera(view(P, "B", cfg))
    r.renderLoop(0, 3, sync=False)
    ref = restated(P, flat, cfg, "B", 0.0, None)
    assert_render(r, (ref.S, ref.Q, ref.counts), "PT_GRAPH=1 A -> B")
    r.free()


# ---- 5. sharding, 6. the command line --------------------------------------------------------------

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
cam = P.look_at(lens_radius={lens}, width={w}, height={h}, **{view!r})
image = render_sharded(s, cfg, 5, jitter=1.0, camera=cam)            # 3 + 2 iterations
assert image.is_cuda
if rank == 0:
    np.save({out!r}, image.cpu().numpy())
dist.barrier()
dist.destroy_process_group()
"""


def test_render_sharded_two_ranks(gpu, pt_mod, scene, flat, tmp_path):
    P = pt_mod
    out = str(tmp_path / "sharded.npy")
    script = tmp_path / "worker_camera.py"
    script.write_text(SHARD_WORKER.format(root=ROOT, scene=REF_SCENE, w=W, h=H, bounces=BOUNCES, out=out, lens=LENS,
                                          view=VIEW_A))
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
    r = renderer(P, scene, cfg, view(P, "A", cfg, LENS), 1.0, moments=False)
    r.renderLoop(0, 5)
    single = r.image()
    r.free()
    assert_bitexact(single, restated(P, flat, cfg, "A", LENS, 1.0, n=5).S, "single rank: image")
    np.testing.assert_allclose(got, single, rtol=1e-6, atol=0)


def test_cli_camera(gpu, pt_mod, scene, tmp_path):
    P = pt_mod
    cfg = make_cfg(P, pipelines=3, iterations=6)
    bmp, want = str(tmp_path / "cli.bmp"), str(tmp_path / "python.bmp")
    p = subprocess.run([os.path.join(ROOT, "pathtracerap_amd", "pathtracer_amd"), REF_SCENE, bmp, "--res", str(W), str(H),
                        "--bounces", str(BOUNCES), "--grid-fast", "--pipelines", "3", "--iter", "6",
                        "--look-from", "0", "800", "500", "--look-at", "0", "0", "0", "--focus", "900", "--lens", str(LENS)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    r = renderer(P, scene, cfg, view(P, "A", cfg, LENS), moments=False)
    r.renderLoop(0, 6)
    r.renderImage(want, 6)
    legacy = renderer(P, scene, cfg, moments=False)
    legacy.renderLoop(0, 6)
    assert not np.array_equal(legacy.image(), r.image())
    legacy.free()
    r.free()
    with open(bmp, "rb") as f, open(want, "rb") as g:
        assert f.read() == g.read()
