#!/usr/bin/env python3
"""What pt_renderer_denoise_ex's options cost on the bench workload (configs[1]: 1280 x 1024,
32 samples rendered once), by scripts/denoise_cost.py's method.

    python scripts/denoise_albedo_cost.py --rounds 9 --warmup 3

Two renderers in one process, the torus textured (scripts/texture_cost.py's seeded 1024 x 1024
texture and uvs) and untextured.  Every round runs each variant once, interleaved:

    plain            denoise()                                 on the untextured renderer
    plain_textured   denoise()                                 on the textured one
    demod_textured   flags = PT_DENOISE_DEMODULATE             albedo from the plane
    demod_plain      flags = PT_DENOISE_DEMODULATE             albedo from the models' colours
    tile_counts      flags = PT_DENOISE_TILE_COUNTS            on the untextured renderer

Times are HIP events around the call's kernels (Renderer.denoise_times), medians over the rounds
with the in-process minimum and maximum.  Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = [("plain", "plain", 0), ("plain_textured", "textured", 0), ("demod_textured", "textured", 1),
            ("demod_plain", "plain", 1), ("tile_counts", "plain", 2)]


def spread(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}


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
    ap.add_argument("--texture", type=int, default=1024, help="the texture's width and height")
    a = ap.parse_args()
    import numpy as np
    import torch
    import pathtracerap_amd as P
    from pathtracerap_amd import synthetic
    assert torch.cuda.is_available(), "needs a GPU"
    path = synthetic.diffuse_scene(tempfile.mkdtemp(), ntri=a.ntri)
    rs = {}
    for v in ("plain", "textured"):
        s = P.Scene(path)
        s.build()
        if v == "textured":                           # scripts/texture_cost.py's texture and uvs
            e = s.export()
            mesh = int(e["model_ints"][1, 0])
            nv = int(e["mesh_ranges"][mesh, 1] - e["mesh_ranges"][mesh, 0])
            rnd = np.random.RandomState(1)
            s.set_mesh_uv(mesh, rnd.uniform(0, 4, (nv, 2)))
            s.set_texture(1, s.add_texture(rnd.uniform(0.2, 1.0, (a.texture, a.texture, 3))))
        r = P.Renderer(P.RenderConfig(width=a.width, height=a.height, max_bounces=a.bounces, pipelines=a.pipelines))
        r.enable_moments()
        r.allocateOnGPU(s)
        r.renderLoop(0, a.samples)
        r.set_profiling(1)
        rs[v] = r
    keys = ("total", "prep", "remod")
    times = {name: {k: [] for k in keys} for name, _, _ in VARIANTS}
    passes = {name: [[] for _ in range(a.passes)] for name, _, _ in VARIANTS}
    images = {}
    for rnd in range(a.warmup + a.rounds):
        for name, which, flags in VARIANTS:
            img = rs[which].denoise(passes=a.passes, flags=flags) if flags else rs[which].denoise(passes=a.passes)
            t = rs[which].denoise_times()
            if rnd == 0:
                images[name] = img
            if rnd >= a.warmup:
                for k in keys:
                    times[name][k].append(t[k])
                for i in range(a.passes):
                    passes[name][i].append(t["passes"][i])
    npix = a.width * a.height
    out = {"config": {"ntri": a.ntri, "width": a.width, "height": a.height, "bounces": a.bounces, "pipelines": a.pipelines,
                      "samples": a.samples, "passes": a.passes, "rounds": a.rounds, "warmup": a.warmup,
                      "texture": [a.texture, a.texture]},
           "uniform_counts_equal_plain": bool(np.array_equal(images["plain"].view(np.uint32),
                                                             images["tile_counts"].view(np.uint32))),
           "primary_hits_on_the_textured_torus": int((rs["textured"].primary_hits()[2] == 1).sum()),
           "ms": {}}
    for name, _, _ in VARIANTS:
        out["ms"][name] = {k: spread(times[name][k]) for k in keys}
        out["ms"][name]["passes_median"] = [round(statistics.median(p), 5) for p in passes[name]]
    m = out["ms"]
    out["demod_textured_minus_plain_textured_ms"] = round(m["demod_textured"]["total"]["median"] - m["plain_textured"]["total"]["median"], 5)
    out["demod_plain_minus_plain_ms"] = round(m["demod_plain"]["total"]["median"] - m["plain"]["total"]["median"], 5)
    out["tile_counts_minus_plain_ms"] = round(m["tile_counts"]["total"]["median"] - m["plain"]["total"]["median"], 5)
    out["remod_gb_per_s"] = round(npix * 48 / (m["demod_textured"]["remod"]["median"] * 1e-3) / 1e9, 1)
    for r in rs.values():
        r.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
