#!/usr/bin/env python3
"""What tile-masked sampling costs and saves: one renderer with moments on, the
variants timed in interleaved rounds in one process (scripts/noise_cost.py's method).

  * renderLoop against render_masked(None): the masked path's fixed cost;
  * ms per iteration at 100 / 50 / 25 / 12.5 / 6.25 % active tiles, random tiles and a
    contiguous block of tiles of the same share;
  * on the reference scene: render_adaptive to a tile target against a plain
    renderLoop of as many iterations as the adaptive run's most-sampled tile received
    (what uniform sampling needs to bring the worst tile to the same target).

    python scripts/adaptive_cost.py --rounds 5 --steps 20 --warmup 5

Each timing is a host clock around a call that ends in a device synchronise.  Prints
one JSON object.
"""
import argparse
import json
import math
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHARES = [1.0, 0.5, 0.25, 0.125, 0.0625]


def spread(ms):
    med = statistics.median(ms)
    return {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
            "spread_pct": round(100.0 * (max(ms) - min(ms)) / med, 2), "rounds": [round(x, 4) for x in ms]}


def random_mask(ty, tx, share, seed=7):
    n = ty * tx
    return (np.random.RandomState(seed).permutation(n) < round(n * share)).reshape(ty, tx)


def block_mask(ty, tx, share):
    """A centred rectangle of tiles with the frame's aspect and about `share` of the tiles."""
    cols = max(1, round(tx * math.sqrt(share)))
    rows = max(1, min(ty, round(ty * tx * share / cols)))
    m = np.zeros((ty, tx), bool)
    y0, x0 = (ty - rows) // 2, (tx - cols) // 2
    m[y0:y0 + rows, x0:x0 + cols] = True
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ntri", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--pipelines", type=int, default=16)
    ap.add_argument("--adaptive-max", type=int, default=512, help="max_iters of the end-to-end run")
    ap.add_argument("--adaptive-min", type=int, default=32, help="its min_iters and check_every")
    ap.add_argument("--skip-end-to-end", action="store_true")
    a = ap.parse_args()
    import torch
    import pathtracerap_amd as P
    from pathtracerap_amd import synthetic
    assert torch.cuda.is_available(), "needs a GPU"
    out = {"config": {"ntri": a.ntri, "width": a.width, "height": a.height, "bounces": a.bounces,
                      "pipelines": a.pipelines, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds}}

    # ---- the cost curve on the bench workload -------------------------------------------
    s = P.Scene(synthetic.diffuse_scene(tempfile.mkdtemp(), ntri=a.ntri))
    s.build()
    cfg = P.RenderConfig(width=a.width, height=a.height, max_bounces=a.bounces, pipelines=a.pipelines)
    r = P.Renderer(cfg)
    r.enable_moments()
    r.allocateOnGPU(s)
    ty, tx = r.sample_counts().shape
    variants = {"render_loop": "loop", "masked_none": None}
    shares = {}
    for sh in SHARES:
        for kind, m in (("random", random_mask(ty, tx, sh)), ("block", block_mask(ty, tx, sh))):
            name = f"{kind}_{100 * sh:g}"
            variants[name] = m
            shares[name] = round(float(m.mean()), 4)
    r.renderLoop(1000, a.warmup)              # warm + primary cache
    r.render_masked(None, 1000, a.warmup)
    times = {v: [] for v in variants}
    for rnd in range(a.rounds):
        for v, m in variants.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            if isinstance(m, str):
                r.renderLoop(rnd * a.steps, a.steps)
            else:
                r.render_masked(m, rnd * a.steps, a.steps)
            times[v].append((time.perf_counter() - t) / a.steps * 1e3)
    out["ms_per_iteration"] = {v: {**spread(times[v]), **({"active_share": shares[v]} if v in shares else {})}
                               for v in variants}
    loop, none = out["ms_per_iteration"]["render_loop"]["median"], out["ms_per_iteration"]["masked_none"]["median"]
    out["masked_none_over_loop_pct"] = round(100.0 * (none - loop) / loop, 2)
    r.free()

    # ---- end to end on the reference scene ---------------------------------------------
    if not a.skip_end_to_end:
        s = P.Scene(os.path.join(ROOT, "scenes", "reference_scene.txt"))
        s.build()
        cfg = P.RenderConfig(width=a.width, height=a.height, pipelines=a.pipelines)
        r = P.Renderer(cfg)
        r.enable_moments()
        r.allocateOnGPU(s)
        # the target: the median tile error after the first check's samples, so about half the
        # tiles stop there and the noisiest need (error / target)^2 times as many
        r.renderLoop(0, a.adaptive_min)
        tiles = r.adaptive_noise()["tiles"]
        target = float(np.median(tiles))
        e2e = {"adaptive_ms": [], "uniform_ms": []}
        for rnd in range(a.rounds):
            r.clearImage()
            torch.cuda.synchronize()
            t = time.perf_counter()
            conv, iters, samples, mean = r.render_adaptive(target, a.adaptive_max, min_iters=a.adaptive_min,
                                                           check_every=a.adaptive_min)
            e2e["adaptive_ms"].append((time.perf_counter() - t) * 1e3)
            counts = r.sample_counts()
            most = int(counts.max())
            r.clearImage()
            torch.cuda.synchronize()
            t = time.perf_counter()
            r.renderLoop(0, most)
            e2e["uniform_ms"].append((time.perf_counter() - t) * 1e3)
        ad, un = statistics.median(e2e["adaptive_ms"]), statistics.median(e2e["uniform_ms"])
        uniform_samples = most * a.width * a.height
        out["end_to_end"] = {
            "tile_target": target, "first_check_tile_error": {"min": float(tiles.min()), "max": float(tiles.max())},
            "converged": conv, "iters": iters, "mean_err": mean,
            "adaptive_ms": spread(e2e["adaptive_ms"]), "uniform_ms": spread(e2e["uniform_ms"]),
            "uniform_iters": most, "adaptive_pixel_samples": samples, "uniform_pixel_samples": uniform_samples,
            "pixel_sample_ratio": round(samples / uniform_samples, 4), "time_ratio": round(ad / un, 4),
            "tile_counts": {"min": int(counts.min()), "median": float(np.median(counts)), "max": most}}
        r.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
