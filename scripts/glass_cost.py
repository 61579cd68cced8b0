#!/usr/bin/env python3
"""What the dielectric material costs (DESIGN.md "Dielectric material"), three measurements, one
JSON object each:

  on     configs[1] (100k-triangle torus in the room, 1280 x 1024, 8 bounces, 16 pipelines) with
         the torus DIELECTRIC (ior 1.5, flat) against DIFFUSE: two renderers timed in interleaved
         rounds in one process (scripts/smooth_cost.py's method), ms per iteration and segments
         per iteration.  The paths differ (glass passes on what a diffuse surface scatters), so
         the figures are reported without a threshold.
  off    no dielectric model: scripts/smooth_cost.py's `off` (bench.py in fresh processes, a
         parent build's library and this build alternating).  The new median must lie inside the
         parent's own min-max spread.
  kres   scripts/kres.sh of this tree against a saved output of the parent's.

    python scripts/glass_cost.py on --rounds 5 --steps 20 --warmup 5
    python scripts/glass_cost.py off --parent-lib /path/to/parent/libpathtracer_amd.so --pairs 6
    python scripts/glass_cost.py kres --before kres_parent.txt

Each timing of `on` is a host clock around renderLoop, which ends in a device synchronise."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import smooth_cost as SC  # noqa: E402


def cost_on(a):
    import torch
    import pathtracerap_amd as P
    from pathtracerap_amd import synthetic
    assert torch.cuda.is_available(), "needs a GPU"
    path = synthetic.diffuse_scene(a.scene_dir or tempfile.mkdtemp(), ntri=a.ntri)
    text = open(path).read()
    assert text.count("DIFFUSE\ntorus_mat\n") == 1
    glass_path = path[:-4] + "_glass.txt"
    with open(glass_path, "w") as f:              # the torus's material block, nothing else
        f.write(text.replace("DIFFUSE\ntorus_mat\n", "DIELECTRIC\ntorus_mat\n"))
    scenes = {}
    for v, p in (("diffuse", path), ("glass", glass_path)):
        s = P.Scene(p)
        s.set_ior(1, a.ior)                       # the torus (synthetic._MODELS order); read by the glass one alone
        s.build()
        scenes[v] = s
    mats = {v: int(s.export()["model_ints"][1, 2]) for v, s in scenes.items()}
    assert mats == {"diffuse": 0, "glass": 7}, mats
    rs = {}
    for v, s in scenes.items():
        r = P.Renderer(P.RenderConfig(width=a.width, height=a.height, max_bounces=a.bounces, pipelines=a.pipelines))
        r.allocateOnGPU(s)
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
    out = {"config": {"ntri": a.ntri, "width": a.width, "height": a.height, "bounces": a.bounces, "pipelines": a.pipelines,
                      "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "ior": a.ior},
           "ms_per_iteration": {v: SC.spread(times[v]) for v in rs}, "segments_per_iteration": segs,
           "trace_faults": {v: r.trace_faults() for v, r in rs.items()},
           "primary_hits_on_the_torus": int((rs["glass"].primary_hits()[2] == 1).sum())}
    m = out["ms_per_iteration"]
    out["glass_over_diffuse_pct"] = round(100.0 * (m["glass"]["median"] - m["diffuse"]["median"]) / m["diffuse"]["median"], 2)
    out["ns_per_segment"] = {v: round(m[v]["median"] * 1e6 / segs[v], 4) for v in rs}
    for r in rs.values():
        r.free()
    return out


def cost_kres(a):
    before = SC.parse_kres(open(a.before).read())
    after = SC.parse_kres(subprocess.run(["bash", os.path.join(ROOT, "scripts", "kres.sh")], capture_output=True, text=True,
                                         check=True).stdout)
    # k_bounce gained a last template argument, GLASS: <..., false> is the parent's kernel of that name
    after = {re.sub(r"(k_bounceILb[01]ELi\dELi\d+ELb[01]ELb[01])ELb0E", r"\1E", k): v for k, v in after.items()}
    added = {k: after[k] for k in after if k not in before}
    assert before and set(before) <= set(after), sorted(set(before) - set(after))
    changed = {k: {"before": before[k], "after": after[k]} for k in before if before[k] != after[k]}
    return {"kernels_listed": len(before), "identical_before_and_after": len(before) - len(changed), "changed": changed,
            "added": added, "figures": {"before": before, "after": after},
            "note": "scripts/kres.sh (-Rpass-analysis=kernel-resource-usage of renderer.hip for gfx950): the k_primary, "
                    "k_trace_* and k_bounce* instantiations, parent commit against this build"}


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    on = sub.add_parser("on")
    on.add_argument("--rounds", type=int, default=5)
    on.add_argument("--steps", type=int, default=20)
    on.add_argument("--warmup", type=int, default=5)
    on.add_argument("--ntri", type=int, default=100_000)
    on.add_argument("--width", type=int, default=1280)
    on.add_argument("--height", type=int, default=1024)
    on.add_argument("--bounces", type=int, default=8)
    on.add_argument("--pipelines", type=int, default=16)
    on.add_argument("--ior", type=float, default=1.5)
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
