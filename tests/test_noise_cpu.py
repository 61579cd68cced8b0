"""The noise estimate without a GPU: noise_ref on hand-made data, the C ABI's
refusals on a renderer that was never allocated, and the sharded moment sums
on two gloo CPU ranks with the oracle as the renderer."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import noise_ref as NR
from conftest import INPUT_DATA

F = np.float32


# ---- noise_ref on hand-made data ----

def test_constant_image_has_no_noise():
    c = np.full((37 * 23, 3), 0.5, F)          # 0.5 and 0.25 sum exactly
    S, Q = NR.moment_sums([c] * 8)
    assert np.all(S == F(4.0)) and np.all(Q == F(2.0))
    n = NR.noise(S, Q, 37, 23, 8)
    assert not n["err"].any() and not n["tiles"].any()
    assert n["mean"] == 0.0 and n["max_tile"] == 0.0


def test_two_samples_closed_form():
    """Samples a and b in every channel: mean (a+b)/2, variance of the raw-moment
    form ((a-b)/2)^2, standard error |a-b| / 2 (n - 1 = 1), and the relative error
    3 * |a-b|/2 over 3 * (a+b)/2 + 0.01.  a = 0.25, b = 0.75: every step is exact."""
    a, b = F(0.25), F(0.75)
    S, Q = NR.moment_sums([np.full((4, 3), a, F), np.full((4, 3), b, F)])
    assert np.all(S == F(1.0)) and np.all(Q == F(0.625))
    err = NR.pixel_err(S, Q, 2)
    want = F(0.75) / (F(1.5) + F(0.01))
    assert err.dtype == F and np.all(err == want)
    n = NR.noise(S, Q, 2, 2, 2)
    assert n["tiles"].shape == (1, 1) and n["tiles"][0, 0] == want
    assert n["mean"] == float(want) and n["max_tile"] == want


def test_negative_variance_clamps_to_zero():
    """Cancellation can leave q - m*m below zero: the estimate clamps it."""
    S = np.full((1, 3), 3.0, F)
    Q = np.full((1, 3), np.nextafter(F(3.0), F(0.0)), F)      # three samples of 1, Q one ulp short
    assert NR.pixel_err(S, Q, 3)[0] == 0.0


def test_partial_tiles_37x23():
    rs = np.random.RandomState(5)
    cs = [rs.uniform(0, 1, (37 * 23, 3)).astype(F) for _ in range(4)]
    S, Q = NR.moment_sums(cs)
    n = NR.noise(S, Q, 37, 23, 4)
    assert n["tiles"].shape == (2, 3)
    assert n["counts"].tolist() == [[256, 256, 80], [112, 112, 35]]
    assert n["counts"].sum() == 37 * 23
    err = n["err"]
    assert err.shape == (23, 37)
    # the corner tile: rows 16..22, columns 32..36
    want = F(err[16:, 32:].astype(np.float64).sum() / 35)
    assert n["tiles"][1, 2] == want
    np.testing.assert_allclose(n["mean"], err.astype(np.float64).mean(), rtol=1e-13)
    assert n["max_tile"] == n["tiles"].max() and n["max_tile"] > 0
    # sequential float32 sums, c*c rounded before the add
    q = np.zeros_like(cs[0])
    for c in cs:
        q = (q + (c * c).astype(F)).astype(F)
    assert np.array_equal(q, Q)


def test_ulp_diff():
    a = np.array([1.0, 0.0], F)
    assert NR.ulp_diff(a, a) == 0
    assert NR.ulp_diff(a, np.array([np.nextafter(F(1.0), F(2.0)), 0.0], F)) == 1


# ---- refusals through the C ABI (no device is touched) ----

def test_null_handles_are_refused(pt_mod):
    L = pt_mod.lib()
    buf = (ctypes.c_float * 4)()
    mean, mx, it = ctypes.c_double(), ctypes.c_float(), ctypes.c_int()
    assert L.pt_renderer_enable_moments(None, None) == -1
    assert b"null renderer" in L.pt_last_error()
    assert L.pt_renderer_read_moments(None, buf) == -1
    assert b"null renderer" in L.pt_last_error()
    assert L.pt_renderer_noise(None, 2, ctypes.byref(mean), ctypes.byref(mx), None) == -1
    assert b"null renderer" in L.pt_last_error()
    assert L.pt_renderer_render_until(None, 0, 2, 4, 2, 0.1, ctypes.byref(it), ctypes.byref(mean)) == -1
    assert b"null renderer" in L.pt_last_error()


@pytest.mark.parametrize("enabled", [False, True])
def test_unallocated_renderer_refuses_noise_calls(pt_mod, enabled):
    P = pt_mod
    r = P.Renderer(P.RenderConfig(width=8, height=8))
    try:
        if enabled:
            r.enable_moments()                   # before allocateOnGPU: accepted, allocates nothing yet
        for call in (r.moments, r.noise, lambda: r.noise(4), lambda: r.render_until(0.1, 4)):
            with pytest.raises(P.PathTracerError, match="not allocated|moments not enabled"):
                call()
        L = P.lib()
        assert L.pt_renderer_read_moments(r._h, None) == -1
        assert b"null buffer" in L.pt_last_error()
    finally:
        r.free()


# ---- render_sharded(moments=True) on two gloo CPU ranks, the oracle as render_fn ----

W, H, ITERS = 32, 24, 5


def _contribution(O, scene, it):
    """Iteration `it`'s per-pixel contributions: a one-iteration render into a zero image."""
    c, _ = O.render(scene, O.RenderConfig(width=W, height=H, iterations=1, first_iter=it, threads=1))
    return c


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_path):
    import torch
    import torch.distributed as dist
    import oracle as O
    from pathtracerap_amd.dist import render_sharded, shard_iterations
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    scene = O.reference_scene(INPUT_DATA)
    cfg = O.RenderConfig(width=W, height=H, iterations=ITERS, threads=1)
    assert shard_iterations(ITERS, rank, world) == ((0, 3), (3, 2))[rank]

    def render_fn(first, n, image, m2):
        S, Q = NR.moment_sums(_contribution(O, scene, it) for it in range(first, first + n))
        image.copy_(torch.from_numpy(S.reshape(-1)))
        m2.copy_(torch.from_numpy(Q.reshape(-1)))

    out = render_sharded(None, cfg, ITERS, render_fn=render_fn, moments=True)
    assert isinstance(out, tuple) and len(out) == 3 and out[2] is None
    if rank == 0:
        np.savez(out_path, image=out[0].numpy(), m2=out[1].numpy())
    dist.destroy_process_group()


def test_gloo_world2_moments_match_single_process(tmp_path, oracle_mod):
    O = oracle_mod
    out = str(tmp_path / "sums.npz")
    mp.start_processes(_worker, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    got = np.load(out)
    scene = O.reference_scene(INPUT_DATA)
    S, Q = NR.moment_sums(_contribution(O, scene, it) for it in range(ITERS))
    whole, _ = O.render(scene, O.RenderConfig(width=W, height=H, iterations=ITERS, threads=1))
    assert np.array_equal(S, whole)               # the per-iteration contributions are the render's
    assert np.abs(Q).sum() > 0
    np.testing.assert_allclose(got["image"].reshape(-1, 3), S, rtol=1e-6, atol=0)
    np.testing.assert_allclose(got["m2"].reshape(-1, 3), Q, rtol=1e-6, atol=0)
