#!/usr/bin/env python3
"""What the second-moment buffer costs on the bench workload: two renderers in
one process, moments off and on, timed in interleaved rounds on one device
(scripts/ab.py's method), plus the time of one noise() evaluation and of
render_until's checks.

    python scripts/noise_cost.py --rounds 5 --steps 20 --warmup 5
    PT_LIB_PATH=build_variants/lib_parent.so python scripts/noise_cost.py --off-only   (an older build: off alone)

Each timing is a host clock around renderLoop, which ends in a device
synchronise.  Prints one JSON object.
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
    return {"ms_per_spp_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
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
    ap.add_argument("--off-only", action="store_true", help="time the moments-off renderer alone (older builds)")
    ap.add_argument("--until-iters", type=int, default=128, help="iterations of the render_until comparison")
    a = ap.parse_args()
    import torch
    import pathtracerap_amd as P
    from pathtracerap_amd import synthetic
    assert torch.cuda.is_available(), "needs a GPU"
    s = P.Scene(synthetic.diffuse_scene(tempfile.mkdtemp(), ntri=a.ntri))
    s.build()
    cfg = P.RenderConfig(width=a.width, height=a.height, max_bounces=a.bounces, pipelines=a.pipelines)
    rs = {}
    for name in (["off"] if a.off_only else ["off", "on"]):
        r = P.Renderer(cfg)
        if name == "on":
            r.enable_moments()
        r.allocateOnGPU(s)
        r.renderLoop(1000, a.warmup)          # warm + primary cache
        rs[name] = r
    times = {v: [] for v in rs}
    for rnd in range(a.rounds):
        for v, r in rs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            r.renderLoop(rnd * a.steps, a.steps)
            times[v].append((time.perf_counter() - t) / a.steps * 1e3)
    out = {"config": {"ntri": a.ntri, "width": a.width, "height": a.height, "bounces": a.bounces,
                      "pipelines": a.pipelines, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
                      "lib": os.environ.get("PT_LIB_PATH", "in-tree")}}
    for v in rs:
        out[v] = spread(times[v])
    if "on" in rs:
        off, on = out["off"]["ms_per_spp_median"], out["on"]["ms_per_spp_median"]
        out["on_over_off_pct"] = round(100.0 * (on - off) / off, 2)
        r = rs["on"]
        nt = []
        for _ in range(7):
            t = time.perf_counter()
            n = r.noise()
            nt.append((time.perf_counter() - t) * 1e3)
        out["noise_call_ms"] = {"median": round(statistics.median(nt), 4), "min": round(min(nt), 4)}
        out["noise_mean"] = n["mean"]
        # render_until against one renderLoop of the same length, interleaved; target 0 never converges
        un = {"render_loop": [], "check_every_32": [], "check_every_8": []}
        for rnd in range(max(3, a.rounds)):
            for name, ce in (("render_loop", 0), ("check_every_32", 32), ("check_every_8", 8)):
                r.clearImage()
                torch.cuda.synchronize()
                t = time.perf_counter()
                if ce:
                    r.render_until(0.0, a.until_iters, check_every=ce)
                else:
                    r.renderLoop(0, a.until_iters)
                un[name].append((time.perf_counter() - t) / a.until_iters * 1e3)
        out["render_until"] = {"iters": a.until_iters, **{k: spread(v) for k, v in un.items()}}
    for r in rs.values():
        r.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
