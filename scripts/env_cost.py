#!/usr/bin/env python3
"""What environment lighting costs on the bench workload (configs[1], the legacy view): the
variants timed in interleaved rounds in one process (scripts/camera_cost.py's method).

  * off: no environment (KParams::env null, the constant 0.01);
  * const8: a constant 8 x 8 map (1 KiB of texels: the lookup's arithmetic and four loads
    that always hit);
  * rand256: a random 256 x 256 map (1 MiB of float4 texels, inside one XCD's 4 MiB L2);
  * rand2048: a random 2048 x 2048 map (64 MiB, sixteen times an XCD's L2).

The rays are the same in every variant bit for bit (an environment changes only the colour
of a ray that has already missed), so the segments per iteration must agree.  The share of
segments that miss is counted with a black map: a path that ends in a miss then contributes
exactly 0, any other path more, so the zero pixels of one iteration are the misses.

    python scripts/env_cost.py --rounds 5 --steps 20 --warmup 5

Each timing is a host clock around renderLoop, which ends in a device synchronise.
Prints one JSON object.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(ms):
    med = statistics.median(ms)
    return {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
            "spread_pct": round(100.0 * (max(ms) - min(ms)) / med, 2), "rounds": [round(x, 4) for x in ms]}


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
    ap.add_argument("--scene-dir", default="", help="where the synthetic scene is written (default: a temporary folder)")
    a = ap.parse_args()
    a.scene_dir = a.scene_dir or tempfile.mkdtemp()
    import numpy as np
    import torch
    import pathtracerap_amd as P
    from pathtracerap_amd import synthetic
    assert torch.cuda.is_available(), "needs a GPU"
    s = P.Scene(synthetic.diffuse_scene(a.scene_dir, ntri=a.ntri))
    s.build()
    out = {"config": {"ntri": a.ntri, "width": a.width, "height": a.height, "bounces": a.bounces,
                      "pipelines": a.pipelines, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds}}
    up_y = np.float32([[0, 0, 1], [1, 0, 0], [0, 1, 0]])

    def random_map(n):
        return P.Environment(np.random.RandomState(n).uniform(0, 2, (n, n, 3)).astype(np.float32), rotation=up_y)

    envs = {"off": None, "const8": P.Environment(np.full((8, 8, 3), 0.5, np.float32), rotation=up_y),
            "rand256": random_map(256), "rand2048": random_map(2048)}

    def renderer(env, pipelines=a.pipelines):
        r = P.Renderer(P.RenderConfig(width=a.width, height=a.height, max_bounces=a.bounces, pipelines=pipelines))
        if env is not None:
            r.set_environment(env)
        r.allocateOnGPU(s)
        return r

    rs = {v: renderer(e) for v, e in envs.items()}
    for r in rs.values():
        r.renderLoop(1000, a.warmup)              # warm + primary cache
    times = {v: [] for v in rs}
    segs = {}
    for rnd in range(a.rounds):
        for v, r in rs.items():
            s0 = r.segments()
            torch.cuda.synchronize()
            t = time.perf_counter()
            r.renderLoop(rnd * a.steps, a.steps)
            times[v].append((time.perf_counter() - t) / a.steps * 1e3)
            segs[v] = (r.segments() - s0) / a.steps
    faults = {v: r.trace_faults() for v, r in rs.items()}
    for r in rs.values():
        r.free()
    m = out["ms_per_iteration"] = {v: spread(times[v]) for v in rs}
    out["segments_per_iteration"] = segs
    out["trace_faults"] = faults
    for v in ("const8", "rand256", "rand2048"):
        out[f"{v}_over_off_pct"] = round(100.0 * (m[v]["median"] - m["off"]["median"]) / m["off"]["median"], 2)
    out["map_MiB"] = {v: round(e.n * e.n * 16 / 2 ** 20, 3) for v, e in envs.items() if e is not None}
    # the misses: one iteration at a time under a black map
    r = renderer(P.Environment.constant(0.0), pipelines=1)
    misses, per_iter = [], []
    for it in range(4):
        r.clearImage()
        s0 = r.segments()
        r.renderLoop(it, 1)
        misses.append(int((~r.image().any(axis=1)).sum()))
        per_iter.append(r.segments() - s0)
    primary_miss = int((r.primary_hits()[2] < 0).sum())
    r.free()
    out["misses_per_iteration"] = misses
    out["primary_misses"] = primary_miss
    out["missing_share_of_segments"] = round(sum(misses) / sum(per_iter), 4)
    out["missing_share_of_paths"] = round(sum(misses) / (4.0 * a.width * a.height), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
