#!/usr/bin/env python3
"""What direct lighting costs and buys (DESIGN.md "Direct lighting"), three measurements, one JSON
object each:

  on     configs[1] (100k-triangle torus in the room, 1280 x 1024, 8 bounces, 16 pipelines) and
         scenes/small_light.txt (640 x 480, 5 bounces): two renderers of one scene, both with
         moments, one with direct light, timed in interleaved rounds in one process
         (scripts/smooth_cost.py's method): ms per iteration.  Then the noise estimate reached
         after equal time: each renderer is cleared and renders the iterations that fit the time
         the plain one needs for --noise-iters, by its own measured median, and pt_renderer_noise
         is read from each.
  off    the feature off: scripts/smooth_cost.py's `off` (bench.py in fresh processes, a parent
         build's library and this build alternating).  The new median must lie inside the
         parent's own min-max spread.
  kres   scripts/kres.sh of this tree against a saved output of the parent's.

    python scripts/direct_cost.py on --rounds 5 --steps 20 --warmup 5
    python scripts/direct_cost.py off --parent-lib /path/to/parent/libpathtracer_amd.so --pairs 4
    python scripts/direct_cost.py kres --before kres_parent.txt

Each timing of `on` is a host clock around renderLoop, which ends in a device synchronise."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import smooth_cost as SC  # noqa: E402


def one_scene(P, torch, a, scene, cfg):
    rs = {}
    for v in ("plain", "direct"):
        r = P.Renderer(cfg)
        r.enable_moments()
        if v == "direct":
            r.set_direct_light()
        r.allocateOnGPU(scene)
        r.renderLoop(1000, a.warmup)          # warm + primary cache
        rs[v] = r
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
    ms = {v: SC.spread(times[v]) for v in rs}
    # equal time: the iterations each renderer fits into the time the plain one needs for noise_iters
    budget_ms = a.noise_iters * ms["plain"]["median"]
    iters = {v: max(2, int(budget_ms / ms[v]["median"])) for v in rs}
    noise, took = {}, {}
    for v, r in rs.items():
        r.clearImage()
        torch.cuda.synchronize()
        t = time.perf_counter()
        r.renderLoop(0, iters[v])
        took[v] = round((time.perf_counter() - t) * 1e3, 2)
        noise[v] = r.noise()["mean"]
    on, n, area = rs["direct"].direct_light()
    out = {"ms_per_iteration": ms, "segments_per_iteration": segs,
           "direct_over_plain_pct": round(100.0 * (ms["direct"]["median"] - ms["plain"]["median"]) / ms["plain"]["median"], 2),
           "lights": n, "light_area": area,
           "equal_time": {"budget_ms": round(budget_ms, 2), "iterations": iters, "ms_taken": took, "noise_estimate": noise,
                          "direct_over_plain": round(noise["direct"] / noise["plain"], 4)},
           "trace_faults": {v: r.trace_faults() for v, r in rs.items()}}
    for r in rs.values():
        r.free()
    return out


def cost_on(a):
    import torch
    import pathtracerap_amd as P
    from pathtracerap_amd import synthetic
    assert torch.cuda.is_available(), "needs a GPU"
    out = {"config": {"steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "noise_iters": a.noise_iters,
                      "pipelines": a.pipelines}}
    s = P.Scene(synthetic.diffuse_scene(a.scene_dir or tempfile.mkdtemp(), ntri=a.ntri))
    s.build()
    out["configs1"] = one_scene(P, torch, a, s, P.RenderConfig(width=1280, height=1024, max_bounces=8, pipelines=a.pipelines))
    s = P.Scene(os.path.join(ROOT, "scenes", "small_light.txt"))
    cfg = s.apply_settings(P.RenderConfig(pipelines=a.pipelines))
    s.build()
    out["small_light"] = one_scene(P, torch, a, s, cfg)
    return out


def cost_kres(a):
    before = SC.parse_kres(open(a.before).read())
    after = SC.parse_kres(subprocess.run(["bash", os.path.join(ROOT, "scripts", "kres.sh")], capture_output=True, text=True,
                                         check=True).stdout)
    added = {k: after[k] for k in after if k not in before}
    assert before and set(before) <= set(after), sorted(set(before) - set(after))
    changed = {k: {"before": before[k], "after": after[k]} for k in before if before[k] != after[k]}
    return {"kernels_listed": len(before), "identical_before_and_after": len(before) - len(changed), "changed": changed,
            "added": added,
            "note": "scripts/kres.sh (-Rpass-analysis=kernel-resource-usage of renderer.hip for gfx950): the k_primary, "
                    "k_trace_* and k_bounce* instantiations, parent commit against this build; added: the new kernels"}


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    on = sub.add_parser("on")
    on.add_argument("--rounds", type=int, default=5)
    on.add_argument("--steps", type=int, default=20)
    on.add_argument("--warmup", type=int, default=5)
    on.add_argument("--ntri", type=int, default=100_000)
    on.add_argument("--pipelines", type=int, default=16)
    on.add_argument("--noise-iters", type=int, default=64, help="the plain renderer's iterations that set the equal-time budget")
    on.add_argument("--scene-dir", default="", help="where the synthetic scene is written (default: a temporary folder)")
    off = sub.add_parser("off")
    off.add_argument("--parent-lib", required=True, help="libpathtracer_amd.so built from the parent commit")
    off.add_argument("--pairs", type=int, default=6)
    off.add_argument("--budget", type=float, default=0.0, help="seconds after which no further pair is started (0: none)")
    off.add_argument("--run-timeout", type=float, default=600.0, help="seconds one bench.py run may take")
    kres = sub.add_parser("kres")
    kres.add_argument("--before", required=True, help="saved scripts/kres.sh output of the parent commit")
    a = ap.parse_args()
    print(json.dumps({a.what: {"on": cost_on, "off": SC.cost_off, "kres": cost_kres}[a.what](a)}))


if __name__ == "__main__":
    main()
