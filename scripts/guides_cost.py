#!/usr/bin/env python3
"""What the sampled first-hit guides cost on the bench workload (configs[1]) under pixel jitter
1.0 with 16 pipelines: three variants timed as alternating fresh child processes (one library per
process), scripts/jitter_cost.py's --against method:

  * parent: the parent commit's library (--parent LIB, loaded through PT_LIB_PATH), jitter on;
  * off:    this build, guides never enabled (its launches are the parent's);
  * on:     this build with enable_guides (k_guide_first and k_merge_guides per iteration).

ms per iteration, medians over the rounds, with the spread.  "off" must sit within the parent's own
run-to-run spread; "on" is reported, not gated.  The "on" child also reports denoise_times() for
PT_DENOISE_DEMODULATE with and without PT_DENOISE_SAMPLED_GUIDES on its own sums.

    python scripts/guides_cost.py --parent build_variants/lib_parent.so --rounds 5 > profiles/guides_cost.json

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


def spread(ms):
    med = statistics.median(ms)
    return {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
            "spread_pct": round(100.0 * (max(ms) - min(ms)) / med, 2), "rounds": [round(x, 4) for x in ms]}


def child(a):
    """One variant in this process: a.rounds timings of a.steps iterations each."""
    import torch
    import pathtracerap_amd as P
    from pathtracerap_amd import synthetic
    assert torch.cuda.is_available(), "needs a GPU"
    s = P.Scene(synthetic.diffuse_scene(a.scene_dir, ntri=a.ntri))
    s.build()
    r = P.Renderer(P.RenderConfig(width=a.width, height=a.height, max_bounces=a.bounces, pipelines=a.pipelines))
    r.enable_moments()
    if a.child == "on":
        r.enable_guides()
    r.set_pixel_jitter(1.0)
    r.allocateOnGPU(s)
    r.renderLoop(1000, a.warmup)
    ms = []
    for rnd in range(a.rounds):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r.renderLoop(rnd * a.steps, a.steps)
        ms.append((time.perf_counter() - t) / a.steps * 1e3)
    out = {"ms": ms}
    if a.child == "on":
        r.set_profiling(1)
        dn = {}
        for name, kw in (("demodulate", dict(demodulate=True)), ("demodulate_sampled_guides", dict(demodulate=True, sampled_guides=True))):
            runs = []
            for _ in range(5):
                r.denoise(**kw)
                runs.append(r.denoise_times())
            dn[name] = {k: round(statistics.median(t[k] for t in runs), 5) for k in ("prep", "remod", "total")}
        out["denoise_times_ms"] = dn
    r.free()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="", metavar="LIB", help="the parent commit's libpathtracer_amd.so")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the variants")
    ap.add_argument("--child-rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ntri", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--pipelines", type=int, default=16)
    ap.add_argument("--scene-dir", default="")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.scene_dir = a.scene_dir or tempfile.mkdtemp()
    if a.child:
        a.rounds = a.child_rounds
        return child(a)
    variants = (["parent"] if a.parent else []) + ["off", "on"]
    runs = {v: [] for v in variants}
    denoise = None
    for _ in range(a.rounds):
        for v in variants:
            env = dict(os.environ)
            env.pop("PT_LIB_PATH", None)
            if v == "parent":
                env["PT_LIB_PATH"] = os.path.abspath(a.parent)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "off" if v == "parent" else v,
                                "--child-rounds", str(a.child_rounds), "--steps", str(a.steps), "--warmup", str(a.warmup),
                                "--ntri", str(a.ntri), "--width", str(a.width), "--height", str(a.height),
                                "--bounces", str(a.bounces), "--pipelines", str(a.pipelines), "--scene-dir", a.scene_dir],
                               env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit(f"child ({v}) failed with {p.returncode}:\n{p.stdout}\n{p.stderr}")
            res = json.loads(p.stdout.strip().splitlines()[-1])
            runs[v].append(statistics.median(res["ms"]))
            denoise = res.get("denoise_times_ms", denoise)
    out = {"config": {"ntri": a.ntri, "width": a.width, "height": a.height, "bounces": a.bounces, "pipelines": a.pipelines,
                      "jitter": 1.0, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "child_rounds": a.child_rounds,
                      "parent": a.parent},
           "ms_per_iteration": {v: spread(ms) for v, ms in runs.items()}, "denoise_times_ms": denoise}
    m = out["ms_per_iteration"]
    base = m["parent"] if a.parent else m["off"]
    if a.parent:
        out["off_over_parent_pct"] = round(100.0 * (m["off"]["median"] - base["median"]) / base["median"], 2)
        out["off_within_parent_spread"] = m["parent"]["min"] <= m["off"]["median"] <= m["parent"]["max"]
    out["on_over_off_pct"] = round(100.0 * (m["on"]["median"] - m["off"]["median"]) / m["off"]["median"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
