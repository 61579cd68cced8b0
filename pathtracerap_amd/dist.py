"""Sample-sharded multi-GPU rendering (one process per GPU, RCCL over xGMI).

A ray's RNG seed depends on its slot in the globally compacted ray pool of
its iteration, so pixels cannot be split without changing the samples; whole
iterations can.  Each rank renders a contiguous iteration range into its
own float3 accumulator and one all-reduce (sum) combines them.  The
all-reduce runs whenever a process group exists, at world size 1 too, so a
one-rank RCCL group exercises the same ordering (the collective on the torch
stream after the renderer's launches) as the 8-GPU run.

Sums of squared contributions add over iteration shards like the image, so
``moments=True`` all-reduces a second buffer and evaluates the noise estimate
on the reduced pair.
"""
from __future__ import annotations

from typing import Callable, Optional


def shard_iterations(total: int, rank: int, world: int) -> tuple[int, int]:
    """Contiguous, balanced split of iterations [0, total): (first, count)."""
    if world <= 0 or not (0 <= rank < world) or total < 0:
        raise ValueError("bad shard arguments")
    base, extra = divmod(total, world)
    first = rank * base + min(rank, extra)
    return first, base + (1 if rank < extra else 0)


def render_sharded(scene, cfg, total_iters: int, device=None,
                   render_fn: Optional[Callable] = None, moments: bool = False,
                   jitter: Optional[float] = None, camera=None, environment=None, guides: bool = False):
    """Render ``total_iters`` samples per pixel across the process group and
    return the summed accumulator (a (W*H*3,) float32 tensor on every rank).

    ``render_fn(first, n, image_tensor)`` may replace the GPU renderer (used
    by the CPU tests with the oracle); by default the gfx950 Renderer renders
    straight into ``image_tensor`` on the current stream.

    ``moments=True`` also accumulates the per-pixel sums of squared
    contributions (Renderer.enable_moments) in a second tensor, all-reduces it
    beside the image and returns ``(image, m2, noise)``: ``noise`` is
    ``Renderer.noise(total_iters)`` on the reduced buffers.  ``render_fn`` is
    then called as ``render_fn(first, n, image_tensor, m2_tensor)`` and
    ``noise`` is None.

    ``guides=True`` (needs ``moments=True`` and generated iterations: ``jitter`` or a lens)
    also accumulates the sampled first-hit guides (Renderer.enable_guides) in a third tensor of
    W*H*8 floats; the sums are additive over iteration shards like the other two, so it is
    all-reduced beside them and returned after ``m2``: ``(image, m2, guides, noise)``.
    ``render_fn`` is then called as ``render_fn(first, n, image_tensor, m2_tensor, guides_tensor)``.

    ``jitter``: a width turns on pixel-jittered camera rays (Renderer.set_pixel_jitter)
    on every rank; the offset depends on (iteration, pixel) only, so the shards add up
    to the one-rank render.  None: unjittered.  Ignored with ``render_fn``.

    ``camera``: a ``Camera`` (Renderer.set_camera) every rank renders through; its lens
    draws depend on (iteration, pixel) only, like the jitter's, so sharding stays exact.
    None: the config's legacy camera.  Ignored with ``render_fn``.

    ``environment``: an ``Environment`` (Renderer.set_environment) every rank lights its
    missing rays with; the lookup depends on the ray only, so the shards add up.  None: the
    constant 0.01.  Ignored with ``render_fn``.
    """
    import torch
    import torch.distributed as dist

    grouped = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size() if grouped else 1
    rank = dist.get_rank() if grouped else 0
    first, n = shard_iterations(total_iters, rank, world)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if render_fn is None else torch.device("cpu")
    image = torch.zeros(cfg.width * cfg.height * 3, dtype=torch.float32, device=device)
    m2 = torch.zeros_like(image) if moments else None
    if guides and not moments:
        raise ValueError("render_sharded: guides=True needs moments=True")
    g = torch.zeros(cfg.width * cfg.height * 8, dtype=torch.float32, device=device) if guides else None
    if render_fn is not None:
        if guides:
            render_fn(first, n, image, m2, g)
        elif moments:
            render_fn(first, n, image, m2)
        else:
            render_fn(first, n, image)
    else:
        from . import Renderer
        r = Renderer(cfg)
        r.set_stream(torch.cuda.current_stream(device).cuda_stream)
        r.bind_image(image.data_ptr(), keepalive=image)
        if moments:
            r.enable_moments(m2.data_ptr(), keepalive=m2)
        if guides:
            r.enable_guides(g.data_ptr(), keepalive=g)
        if jitter is not None:
            r.set_pixel_jitter(jitter)
        if camera is not None:
            r.set_camera(camera)
        if environment is not None:
            r.set_environment(environment)
        r.allocateOnGPU(scene)
        r.renderLoop(first_iter=first, n_iters=n, sync=False)
    if grouped:
        dist.all_reduce(image, op=dist.ReduceOp.SUM)      # RCCL (nccl backend) over xGMI, or gloo
        if moments:
            dist.all_reduce(m2, op=dist.ReduceOp.SUM)
        if guides:
            dist.all_reduce(g, op=dist.ReduceOp.SUM)
    noise = None
    if render_fn is None:
        torch.cuda.synchronize(device)
        if moments:
            noise = r.noise(total_iters)      # on the reduced image and moments, before they are unbound
        r.free()
    if guides:
        return image, m2, g, noise
    return (image, m2, noise) if moments else image
