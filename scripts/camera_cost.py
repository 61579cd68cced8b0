#!/usr/bin/env python3
"""What a set camera costs on the bench workload (configs[1]): the variants timed in
interleaved rounds in one process (scripts/jitter_cost.py's method).

  * legacy against the legacy-equivalent set_camera, jitter off: the camera_ray branch alone
    (the rays, and so every later kernel's work, are the same bit for bit);
  * jitter 1 on the legacy camera (k_gen_jitter) against jitter 1 on the camera (k_gen_camera);
  * the camera with a lens (the legacy-equivalent view, lens radius --lens) against jitter 1
    on the camera: ms per iteration, medians of the rounds, spread;
  * per launch, from HIP events on one pipeline with max_bounces 1: the generating kernel of
    each variant against 48 B per pixel at the measured copy rate.

    python scripts/camera_cost.py --rounds 5 --steps 20 --warmup 5

Each timing is a host clock around renderLoop, which ends in a device synchronise.
Prints one JSON object.
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS = 6.29          # measured device copy rate, TB/s


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
    ap.add_argument("--lens", type=float, default=0.05, help="lens radius of the lens variants, world units")
    ap.add_argument("--scene-dir", default="", help="where the synthetic scene is written (default: a temporary folder)")
    a = ap.parse_args()
    a.scene_dir = a.scene_dir or tempfile.mkdtemp()
    import torch
    import pathtracerap_amd as P
    from pathtracerap_amd import synthetic
    assert torch.cuda.is_available(), "needs a GPU"
    s = P.Scene(synthetic.diffuse_scene(a.scene_dir, ntri=a.ntri))
    s.build()
    out = {"config": {"ntri": a.ntri, "width": a.width, "height": a.height, "bounces": a.bounces,
                      "pipelines": a.pipelines, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "lens": a.lens}}

    def renderer(camera, jitter, lens, bounces=a.bounces, pipelines=a.pipelines):
        r = P.Renderer(P.RenderConfig(width=a.width, height=a.height, max_bounces=bounces, pipelines=pipelines))
        if camera:
            cam = r.camera()[1]                          # the legacy-equivalent view
            r.set_camera(dataclasses.replace(cam, lens_radius=a.lens) if lens else cam)
        if jitter:
            r.set_pixel_jitter(1.0)
        r.allocateOnGPU(s)
        return r

    variants = {"legacy": (False, False, False), "camera": (True, False, False),
                "legacy_jitter": (False, True, False), "camera_jitter": (True, True, False),
                "camera_lens": (True, False, True), "camera_lens_jitter": (True, True, True)}
    rs = {v: renderer(*cjl) for v, cjl in variants.items()}
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
    m = out["ms_per_iteration"] = {v: spread(times[v]) for v in rs}
    out["segments_per_iteration"] = segs
    for r in rs.values():
        r.free()
    for v, base in (("camera", "legacy"), ("camera_jitter", "legacy_jitter"), ("camera_lens", "camera_jitter"),
                    ("camera_lens_jitter", "camera_jitter")):
        out[f"{v}_over_{base}_pct"] = round(100.0 * (m[v]["median"] - m[base]["median"]) / m[base]["median"], 2)
    # per launch: one pipeline, max_bounces 1, so an iteration is the generating kernel, k_scan, the
    # trace of the W*H camera rays, their shading pass, k_scan
    npix = a.width * a.height
    per = {}
    for v in ("legacy_jitter", "camera_jitter", "camera_lens", "camera_lens_jitter"):
        r = renderer(*variants[v], bounces=1, pipelines=1)
        r.renderLoop(1000, a.warmup)
        r.set_profiling(1)
        r.renderLoop(0, a.steps)
        k = r.kernel_stats()
        r.free()
        gen = k["first_ms"] / max(k["first_launches"], 1)
        per[v] = {"kernel": "k_gen_jitter" if v == "legacy_jitter" else "k_gen_camera", "gen_ms": round(gen, 5),
                  "gen_GBs": round(48.0 * npix / (gen * 1e-3) / 1e9, 1),
                  "gen_share_of_copy_rate": round(48.0 * npix / (gen * 1e-3) / (COPY_TBS * 1e12), 3),
                  "bounce1_trace_ms": round(k["trace_ms"] / max(k["trace_launches"], 1), 5),
                  "bounce1_shade_ms": round(k["bounce_ms"] / max(k["bounce_launches"], 1), 5),
                  "launches": k["first_launches"]}
    out["per_launch_one_pipeline"] = per
    out["floor_ms_48B_per_pixel_at_copy_rate"] = round(48.0 * npix / (COPY_TBS * 1e12) * 1e3, 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
