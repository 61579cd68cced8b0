#!/usr/bin/env python3
"""What pixel-jittered camera rays cost on the bench workload (configs[1]): the variants
timed in interleaved rounds in one process (scripts/noise_cost.py's method).

  * jitter off, on (width 1) and on with the ray sort before the bounce-1 trace too
    (PT_JITTER_SORT=1): ms per iteration, medians of the rounds, spread;
  * per launch, from HIP events on one pipeline with max_bounces 1 (so the only trace is
    the one of the generated camera rays): k_gen_jitter against 48 B per pixel at the
    measured copy rate, the sort, the bounce-1 trace and its shading pass;
  * --against LIB: jitter off of this build against an older build of the library,
    alternating fresh child processes (one library per process), --off-only in each.

    python scripts/jitter_cost.py --rounds 5 --steps 20 --warmup 5
    python scripts/jitter_cost.py --against build_variants/lib_parent.so --rounds 5

Each timing is a host clock around renderLoop, which ends in a device synchronise.
Prints one JSON object.
"""
import argparse
import json
import os
import statistics
import subprocess
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


def against(a):
    """Alternate child processes: the older library, then this build, a.rounds times."""
    runs = {"other": [], "tree": []}
    for _ in range(a.rounds):
        for name in ("other", "tree"):
            env = dict(os.environ)
            env.pop("PT_LIB_PATH", None)
            if name == "other":
                env["PT_LIB_PATH"] = os.path.abspath(a.against)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--off-only", "--rounds", "3", "--steps", str(a.steps),
                                "--warmup", str(a.warmup), "--ntri", str(a.ntri), "--width", str(a.width),
                                "--height", str(a.height), "--bounces", str(a.bounces), "--pipelines", str(a.pipelines),
                                "--scene-dir", a.scene_dir], env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit(f"child ({name}) failed with {p.returncode}:\n{p.stdout}\n{p.stderr}")
            runs[name].append(json.loads(p.stdout.strip().splitlines()[-1])["ms_per_iteration"]["off"]["median"])
    out = {"against": a.against, "ms_per_iteration": {k: spread(v) for k, v in runs.items()}}
    o, t = out["ms_per_iteration"]["other"], out["ms_per_iteration"]["tree"]
    out["tree_over_other_pct"] = round(100.0 * (t["median"] - o["median"]) / o["median"], 2)
    print(json.dumps(out))


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
    ap.add_argument("--off-only", action="store_true", help="time the unjittered renderer alone (older builds)")
    ap.add_argument("--against", default="", metavar="LIB", help="an older libpathtracer_amd.so to alternate with")
    ap.add_argument("--scene-dir", default="", help="where the synthetic scene is written (default: a temporary folder)")
    a = ap.parse_args()
    a.scene_dir = a.scene_dir or tempfile.mkdtemp()
    if a.against:
        return against(a)
    import torch
    import pathtracerap_amd as P
    from pathtracerap_amd import synthetic
    assert torch.cuda.is_available(), "needs a GPU"
    s = P.Scene(synthetic.diffuse_scene(a.scene_dir, ntri=a.ntri))
    s.build()
    out = {"config": {"ntri": a.ntri, "width": a.width, "height": a.height, "bounces": a.bounces,
                      "pipelines": a.pipelines, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
                      "lib": os.environ.get("PT_LIB_PATH", "in-tree")}}

    def renderer(jitter, sort1, bounces=a.bounces, pipelines=a.pipelines):
        if sort1:
            os.environ["PT_JITTER_SORT"] = "1"           # read by allocateOnGPU
        r = P.Renderer(P.RenderConfig(width=a.width, height=a.height, max_bounces=bounces, pipelines=pipelines))
        if jitter:
            r.set_pixel_jitter(1.0)
        r.allocateOnGPU(s)
        os.environ.pop("PT_JITTER_SORT", None)
        return r

    variants = {"off": (False, False)}
    if not a.off_only:
        variants.update({"on": (True, False), "on_sorted_bounce1": (True, True)})
    rs = {v: renderer(*jv) for v, jv in variants.items()}
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
    out["ms_per_iteration"] = {v: spread(times[v]) for v in rs}
    out["segments_per_iteration"] = segs
    for r in rs.values():
        r.free()
    if not a.off_only:
        m = out["ms_per_iteration"]
        for v in ("on", "on_sorted_bounce1"):
            out[f"{v}_over_off_pct"] = round(100.0 * (m[v]["median"] - m["off"]["median"]) / m["off"]["median"], 2)
        # per launch: one pipeline, max_bounces 1, so an iteration is k_gen_jitter, k_scan, [sort,] the
        # trace of the W*H camera rays, their shading pass, k_scan
        npix = a.width * a.height
        per = {}
        for v, sort1 in (("unsorted", False), ("sorted", True)):
            r = renderer(True, sort1, bounces=1, pipelines=1)
            r.renderLoop(1000, a.warmup)
            r.set_profiling(1)
            r.renderLoop(0, a.steps)
            k = r.kernel_stats()
            r.free()
            gen = k["first_ms"] / max(k["first_launches"], 1)
            per[v] = {"k_gen_jitter_ms": round(gen, 5),
                      "k_gen_jitter_GBs": round(48.0 * npix / (gen * 1e-3) / 1e9, 1),
                      "k_gen_jitter_share_of_copy_rate": round(48.0 * npix / (gen * 1e-3) / (COPY_TBS * 1e12), 3),
                      "sort_ms": round(k["sort_ms"] / max(k["sort_launches"], 1), 5), "sort_launches": k["sort_launches"],
                      "bounce1_trace_ms": round(k["trace_ms"] / max(k["trace_launches"], 1), 5),
                      "bounce1_shade_ms": round(k["bounce_ms"] / max(k["bounce_launches"], 1), 5),
                      "scan_ms": round(k["scan_ms"] / max(k["scan_launches"], 1), 5), "launches": k["first_launches"]}
        out["per_launch_one_pipeline"] = per
        out["floor_ms_48B_per_pixel_at_copy_rate"] = round(48.0 * npix / (COPY_TBS * 1e12) * 1e3, 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
