#!/usr/bin/env python3
"""What smooth shading costs (DESIGN.md "Smooth shading"), three measurements, one JSON object each:

  on     configs[1] (100k-triangle torus in the room, 1280 x 1024, 8 bounces, 16 pipelines) with
         the torus smooth against flat: two renderers timed in interleaved rounds in one process
         (scripts/env_cost.py's method), ms per iteration and segments per iteration.  The paths
         differ (another normal scatters another way), so the segment counts differ too.
  off    no smooth model: bench.py --gpus 1 --steps 20 --warmup 5 in fresh processes, a parent
         build's library (PT_LIB_PATH) and this build alternating, parent first, --pairs times.
         The new median must lie inside the parent's own min-max spread.
  kres   scripts/kres.sh of this tree against a saved output of the parent's: the kernels whose
         figures changed, and how many are identical.

    python scripts/smooth_cost.py on --rounds 5 --steps 20 --warmup 5
    python scripts/smooth_cost.py off --parent-lib /path/to/parent/libpathtracer_amd.so --pairs 6
    python scripts/smooth_cost.py kres --before kres_parent.txt

Each timing of `on` is a host clock around renderLoop, which ends in a device synchronise."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v, digits=4):
    med = statistics.median(v)
    return {"median": round(med, digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "spread_pct": round(100.0 * (max(v) - min(v)) / med, 2), "rounds": [round(x, digits) for x in v]}


def cost_on(a):
    import torch
    import pathtracerap_amd as P
    from pathtracerap_amd import synthetic
    assert torch.cuda.is_available(), "needs a GPU"
    path = synthetic.diffuse_scene(a.scene_dir or tempfile.mkdtemp(), ntri=a.ntri)
    scenes = {}
    for v in ("flat", "smooth"):
        s = P.Scene(path)
        if v == "smooth":
            s.set_smooth(1)                   # the torus (synthetic._MODELS order)
        s.build()
        scenes[v] = s
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
                      "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds},
           "ms_per_iteration": {v: spread(times[v]) for v in rs}, "segments_per_iteration": segs,
           "trace_faults": {v: r.trace_faults() for v, r in rs.items()},
           "primary_hits_on_the_torus": int((rs["smooth"].primary_hits()[2] == 1).sum()),
           "shading_table_MiB": round(scenes["smooth"].counts()["nt"] * 96 / 2 ** 20, 2)}
    m = out["ms_per_iteration"]
    out["smooth_over_flat_pct"] = round(100.0 * (m["smooth"]["median"] - m["flat"]["median"]) / m["flat"]["median"], 2)
    out["ns_per_segment"] = {v: round(m[v]["median"] * 1e6 / segs[v], 4) for v in rs}
    for r in rs.values():
        r.free()
    return out


def cost_off(a):
    runs = {"parent": [], "new": []}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"]
    t0, longest, pairs = time.perf_counter(), 0.0, 0
    for _ in range(a.pairs):
        if a.budget > 0 and time.perf_counter() - t0 + 2.2 * longest > a.budget:
            break                             # no room for another pair: report the pairs there are
        pairs += 1
        for who in ("parent", "new"):
            t1 = time.perf_counter()
            env = dict(os.environ)
            if who == "parent":
                env["PT_LIB_PATH"] = os.path.abspath(a.parent_lib)
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.run_timeout)
            if p.returncode != 0:             # stop: start nothing more on the GPU after a failed run
                raise SystemExit(f"bench.py ({who}) failed with {p.returncode}:\n{p.stderr[-2000:]}")
            res = json.loads(p.stdout.strip().splitlines()[-1])
            assert res["config"]["trace_faults"] == 0 and res["config"]["image_finite"]
            runs[who].append(res["value"])
            longest = max(longest, time.perf_counter() - t1)
            print(f"{who}: {res['value']} Mrays/s in {time.perf_counter() - t1:.0f} s", file=sys.stderr, flush=True)
    out = {who: dict(spread(v, 3), mrays_per_s=v) for who, v in runs.items()}
    for who in out:
        del out[who]["rounds"]
    out["new_over_parent_pct"] = round(100.0 * (out["new"]["median"] - out["parent"]["median"]) / out["parent"]["median"], 2)
    out["new_median_inside_parent_spread"] = bool(out["parent"]["min"] <= out["new"]["median"] <= out["parent"]["max"])
    out["method"] = ("bench.py --gpus 1 --steps 20 --warmup 5, the parent commit's library and this build alternating in "
                     f"fresh processes, {pairs} pairs, parent first")
    return out


def parse_kres(text):
    out = {}
    for line in text.splitlines():
        f = line.split()
        if len(f) >= 2 and "=" in f[1]:
            out[f[0]] = dict(kv.split("=") for kv in f[1:])
    return out


def cost_kres(a):
    before = parse_kres(open(a.before).read())
    after = parse_kres(subprocess.run(["bash", os.path.join(ROOT, "scripts", "kres.sh")], capture_output=True, text=True,
                                      check=True).stdout)
    # k_bounce gained a last template argument, SMOOTH: <..., false> is the parent's kernel of that name
    after = {re.sub(r"(k_bounceILb[01]ELi\dELi\d+)ELb0E", r"\1E", k): v for k, v in after.items()}
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
    on.add_argument("--scene-dir", default="", help="where the synthetic scene is written (default: a temporary folder)")
    off = sub.add_parser("off")
    off.add_argument("--parent-lib", required=True, help="libpathtracer_amd.so built from the parent commit")
    off.add_argument("--pairs", type=int, default=6)
    off.add_argument("--budget", type=float, default=0.0, help="seconds after which no further pair is started (0: none)")
    off.add_argument("--run-timeout", type=float, default=600.0, help="seconds one bench.py run may take")
    kres = sub.add_parser("kres")
    kres.add_argument("--before", required=True, help="saved scripts/kres.sh output of the parent commit")
    a = ap.parse_args()
    print(json.dumps({a.what: {"on": cost_on, "off": cost_off, "kres": cost_kres}[a.what](a)}))


if __name__ == "__main__":
    main()
