"""Flat meshes, exact ties and coincident instances through every trace
(path_scenes.py section I; CPU preconditions: test_degenerate_cpu.py).  Every
scene: intersect_rays (the one-lane path) in all three modes and trace_rays (the
persistent traces, walking in place and with hand-ons) in bvh and grid_fast mode
bit-equal to the CPU oracle in distance, model and normal, and to each other;
trace_faults() == 0.  A mesh with no extent on a model axis has a voxel width of
exactly 0 there, which puts inf and NaN into the walks and their certificates:
grid_fast must still equal the grid on every ray, which sees such a mesh from one
side only.  The persistent traces run under a lowered iteration cap, so a wave
that cannot finish is a reported trace fault at once."""
import numpy as np
import pytest

import path_scenes as S
from helpers import assert_bitexact, flat_from_export, oracle_cfg

pytestmark = pytest.mark.gpu

# 1/64 of the default cap: a safety net, not a tolerance (test_iteration_cap_has_room)
ITER_CAP = 1048576
G25 = (25, 25, 25)


@pytest.fixture(autouse=True)
def _iteration_cap(monkeypatch):
    monkeypatch.setenv("PT_TRACE_ITER_CAP", str(ITER_CAP))


def _renderer(P, scene, accel, pipes, width=256, height=160):
    r = P.Renderer(P.RenderConfig(width=width, height=height, iterations=2, accel=accel, grid=G25, pipelines=pipes))
    r.allocateOnGPU(scene)
    return r


def _one_lane(P, scene, accel, o, d, want, what):
    """intersect_rays at `accel` == the oracle's (dist, normal, model); returns the GPU's."""
    r = _renderer(P, scene, accel, 1)
    try:
        t, n, m = r.intersect_rays(o, d)
        assert r.trace_faults() == 0, what
    finally:
        r.free()
    assert_bitexact(m, want[2], f"model {what}")
    assert_bitexact(t, want[0], f"dist {what}")
    hit = want[2] >= 0
    assert_bitexact(n[hit], want[1][hit], f"normal {what}")
    return t, n, m


def _all_traces(P, O, name):
    """Every comparison of the module docstring for one named scene; returns
    {accel: intersect_rays' (dist, normal, model)}."""
    s, o, d = S.degenerate_case(P, name)
    got = {}
    for accel in (0, 1, 2):
        got[accel] = _one_lane(P, s, accel, o, d, S.degenerate_oracle(P, O, name, accel), f"{name} intersect_rays accel={accel}")
    for accel in (1, 2):
        for pipes in (1, 4):
            r = _renderer(P, s, accel, pipes)
            try:
                S.check_rays(r, s, o, d, S.degenerate_oracle(P, O, name, accel), what=f"{name} accel={accel} pipes={pipes}")
                if accel == 2:
                    print(f"{name} pipes={pipes}: deferred_rays={r.deferred_rays()}")
            finally:
                r.free()
    return got


def test_iteration_cap_has_room(gpu, pt_mod, oracle_mod):
    """The reference-scene ray set at this file's batch size traces without a fault
    under the lowered cap, in both traces, in place and with hand-ons."""
    P, O = pt_mod, oracle_mod
    s, grid, o, d, _ = S.ray_set(P, "ref")
    for accel in (1, 2):
        want = tuple(v[:4096] for v in S.ray_set_oracle(P, O, "ref", accel))
        for pipes in (1, 4):
            r = _renderer(P, s, accel, pipes)
            try:
                S.check_rays(r, s, o[:4096], d[:4096], want, what=f"ref accel={accel} pipes={pipes} cap={ITER_CAP}")
            finally:
                r.free()


@pytest.mark.parametrize("name", S.FLAT_NAMES)
def test_flat_and_thin_meshes(gpu, pt_mod, oracle_mod, name):
    """h = 0 in addition: grid_fast equals the grid on every ray, and no ray with a
    positive model-space direction on the flat axis hits in either."""
    P, O = pt_mod, oracle_mod
    got = _all_traces(P, O, name)
    if "-h0-" in name:
        s, o, d = S.degenerate_case(P, name)
        pos = S.flat_rays(s.export())[2]
        for k, what in enumerate(("dist", "normal", "model")):
            assert_bitexact(got[2][k], got[0][k], f"{name}: grid_fast vs grid, {what}")
        assert pos.sum() >= 1500
        assert (got[0][2][pos] == -1).all() and (got[2][2][pos] == -1).all()
        assert (got[1][2][pos] == 0).mean() >= 0.99          # the exact mode sees that side


@pytest.mark.parametrize("name", S.FLAT_NAMES)
def test_certificates_agree_with_the_exact_walk(gpu, pt_mod, name):
    """k_certify_check on the same rays: wherever walk_certify_fast or walk_certify
    accepts, it equals the stepped walk on the same hit set (for h = 0: no certificate
    may accept a hit the walk, starting at the last voxel of the flat axis, never reaches)."""
    P = pt_mod
    s, o, d = S.degenerate_case(P, name)
    r = _renderer(P, s, 2, 1, width=8, height=8)
    try:
        tried, ok, fast_bad, full_bad = (int(v) for v in r.certify_check(o, d).sum(0))
    finally:
        r.free()
    print(f"certify {name}: tried={tried} fast accepted={ok}")
    assert fast_bad == 0 and full_bad == 0 and tried > 0, f"tried {tried} accepted {ok} fast_bad {fast_bad} full_bad {full_bad}"
    if "-h0-" in name:
        assert ok == 0          # a box of width 0 cannot shrink: the fast certificate never applies


@pytest.mark.parametrize("name", S.NEEDLE_NAMES)
def test_needle(gpu, pt_mod, oracle_mod, name):
    got = _all_traces(pt_mod, oracle_mod, name)
    for accel in (0, 1, 2):
        assert (got[accel][2] == -1).all()


@pytest.mark.parametrize("name", S.RIDGE_NAMES)
def test_ridge(gpu, pt_mod, oracle_mod, name):
    """On-ridge rays and off-ridge controls in one batch.  Exact mode in addition:
    the winning side is the one the triangle order puts first, as the oracle has it."""
    got = _all_traces(pt_mod, oracle_mod, name)
    n = S.RIDGE_RAYS
    assert (got[1][2] == 0).all()
    assert_bitexact(np.sign(got[1][1][:n, 2]), S.ridge_tie_sides(name[len("ridge-"):]).astype(np.float32),
                    f"{name}: winning side of the ties, accel=1")


@pytest.mark.parametrize("name", S.COINCIDENT_NAMES)
def test_coincident_pair(gpu, pt_mod, oracle_mod, name):
    P, O = pt_mod, oracle_mod
    got = _all_traces(P, O, name)
    _, k, where, _ = name.split("-")
    at = S.coincident_spec(int(k), where)[2]
    for accel in (0, 1, 2):
        m = got[accel][2]
        assert ((m == at) | (m == at + 1)).sum() >= 1000 and not (m == at + 1).any()


ENV_VARIANTS = [{"PT_GF_SPLIT": "0"}, {"PT_WALK_HANDON": "0"}, {"PT_WALK_HANDON": "1"}, {"PT_GF_FLAGS": "8"},
                {"PT_HS_POOL_BLOCKS": "1"}]


@pytest.mark.parametrize("env", ENV_VARIANTS, ids=lambda v: "-".join(f"{k[3:].lower()}{x}" for k, x in v.items()))
@pytest.mark.parametrize("name", ["flat-x-h0-xf", "flat-y-h0-id", "flat-z-h0-xf", "ridge-interleaved", "ridge-permuted"])
def test_grid_fast_env_variants(gpu, pt_mod, oracle_mod, monkeypatch, name, env):
    """grid_fast with the fused bounce's one-lane trace (no split: trace_rays refuses,
    intersect_rays runs), walks in place and handed on at one and four pipelines,
    model records from global memory, and one hit-set pool block."""
    P, O = pt_mod, oracle_mod
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s, o, d = S.degenerate_case(P, name)
    want = S.degenerate_oracle(P, O, name, 2)
    if env.get("PT_GF_SPLIT") == "0":
        _one_lane(P, s, 2, o, d, want, f"{name} {env}")
        return
    for pipes in (1, 4):
        r = _renderer(P, s, 2, pipes)
        try:
            S.check_rays(r, s, o, d, want, what=f"{name} {env} pipes={pipes}")
            print(f"{name} {env} pipes={pipes}: deferred_rays={r.deferred_rays()}")
        finally:
            r.free()


@pytest.mark.parametrize("accel,pipes,env", [(a, p, {}) for a in (0, 1, 2) for p in (1, 4)] +
                         [(2, p, {"PT_GF_SPLIT": "0"}) for p in (1, 4)],
                         ids=lambda v: ("gf_split0" if v else "default") if isinstance(v, dict) else str(v))
def test_room_with_flat_quads_and_a_ridge_renders_as_the_oracle(gpu, pt_mod, oracle_mod, monkeypatch, accel, pipes, env):
    """A flat floor quad, a flat lamp facing down and a ridge in the synthetic room,
    64 x 48, 2 iterations, 4 bounces: image and segments bit-equal to the oracle's,
    primary_hits to intersect_primary.  Bounce rays start 0.1 off the flat quads.
    grid_fast also through the fused bounce's one-lane trace (PT_GF_SPLIT=0)."""
    P, O = pt_mod, oracle_mod
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = S.scene_once("degenerate-room", lambda: S.scene_from_spec(P, *S.degenerate_room_spec()))
    cfg = P.RenderConfig(accel=accel, pipelines=pipes, **S.DEGENERATE_FRAME)
    S.check_render(P, O, "degenerate-room", s, cfg, what=f"degenerate room accel={accel} pipes={pipes} {env}")
    r = P.Renderer(cfg)
    try:
        r.allocateOnGPU(s)
        got = r.primary_hits()
    finally:
        r.free()
    want = O.intersect_primary(flat_from_export(s.export()), oracle_cfg(cfg))
    assert_bitexact(got[2], want[2], "primary model")
    assert_bitexact(got[0], want[0], "primary dist")
    hit = want[2] >= 0
    assert_bitexact(got[1][hit], want[1][hit], "primary normal")
