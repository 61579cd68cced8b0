#!/usr/bin/env python3
"""What one denoise() call costs on the bench workload (1280 x 1024, 32 samples
rendered once), and which passes should stage their tile in LDS.

    python scripts/denoise_cost.py --rounds 9 --warmup 3

PT_DENOISE_LDS in {0, 1, 2, 4, 8} (the largest a-trous step whose pass goes through
LDS; read at every call) is timed interleaved in one process on one renderer: every
round runs each value once.  Times are HIP events around the call's kernels
(Renderer.denoise_times: prep, every pass, first kernel to last), medians over the
rounds.  Each pass is also reported against its algorithmic traffic, 36 bytes read
and 16 written per pixel.  One render iteration of the same renderer is timed with a
host clock around renderLoop for comparison.  Prints one JSON object.
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

LDS_VALUES = [0, 1, 2, 4, 8]
PASS_BYTES_PER_PIXEL = 36 + 16


def med(v):
    return round(statistics.median(v), 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--ntri", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--pipelines", type=int, default=16)
    ap.add_argument("--render-steps", type=int, default=20, help="iterations of the render timing")
    a = ap.parse_args()
    import numpy as np
    import torch
    import pathtracerap_amd as P
    from pathtracerap_amd import synthetic
    assert torch.cuda.is_available(), "needs a GPU"
    s = P.Scene(synthetic.diffuse_scene(tempfile.mkdtemp(), ntri=a.ntri))
    s.build()
    cfg = P.RenderConfig(width=a.width, height=a.height, max_bounces=a.bounces, pipelines=a.pipelines)
    r = P.Renderer(cfg)
    r.enable_moments()
    r.allocateOnGPU(s)
    r.renderLoop(1000, 5)                       # warm + primary cache
    render_ms = []
    for rnd in range(3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r.renderLoop(2000 + rnd * a.render_steps, a.render_steps)
        render_ms.append((time.perf_counter() - t) / a.render_steps * 1e3)
    r.clearImage()
    r.renderLoop(0, a.samples)
    r.set_profiling(1)
    npix = a.width * a.height
    times = {v: {"total": [], "prep": [], "passes": [[] for _ in range(a.passes)]} for v in LDS_VALUES}
    images = {}
    for rnd in range(a.warmup + a.rounds):
        for v in LDS_VALUES:
            os.environ["PT_DENOISE_LDS"] = str(v)
            img = r.denoise(passes=a.passes)
            t = r.denoise_times()
            if rnd == 0:
                images[v] = img
            if rnd >= a.warmup:
                times[v]["total"].append(t["total"])
                times[v]["prep"].append(t["prep"])
                for i in range(a.passes):
                    times[v]["passes"][i].append(t["passes"][i])
    os.environ.pop("PT_DENOISE_LDS")
    same = all(np.array_equal(images[0].view(np.uint32), images[v].view(np.uint32)) for v in LDS_VALUES)
    out = {"config": {"ntri": a.ntri, "width": a.width, "height": a.height, "bounces": a.bounces,
                      "pipelines": a.pipelines, "samples": a.samples, "passes": a.passes, "rounds": a.rounds,
                      "warmup": a.warmup},
           "render_ms_per_iteration": med(render_ms), "identical_for_every_value": same, "lds": {}}
    for v in LDS_VALUES:
        tv = times[v]
        pm = [med(p) for p in tv["passes"]]
        out["lds"][str(v)] = {
            "total_ms": med(tv["total"]), "total_min": round(min(tv["total"]), 5), "total_max": round(max(tv["total"]), 5),
            "prep_ms": med(tv["prep"]), "pass_ms": pm,
            "pass_staged": [(1 << i) <= v for i in range(a.passes)],
            "pass_gb_per_s": [round(npix * PASS_BYTES_PER_PIXEL / (p * 1e-3) / 1e9, 1) for p in pm],
            "total_over_render_iteration": round(med(tv["total"]) / med(render_ms), 3)}
    base = out["lds"]["0"]["total_ms"]
    for v in LDS_VALUES:
        out["lds"][str(v)]["total_over_lds0"] = round(out["lds"][str(v)]["total_ms"] / base, 3)
    r.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
