"""Adversarial ray batches through the persistent trace kernels (k_trace_gf /
k_trace_bvh with their tail launches and k_trace_deferred) and the compaction
plumbing they read through (k_scan's blk_off / dst_start, slot_source, the sort
kernels), via Renderer.trace_rays: the caller's rays become bounce 0's
survivors in a chosen block layout and bounce 1's real launch sequence runs
over them.  Every case: distance, model and normal (on hits) bit-equal to the
CPU oracle and to intersect_rays (the one-lane path) of the same renderer, the
triangle inside the hit model's mesh, trace_faults() == 0.  Ray sets, layouts
and their CPU preconditions: path_scenes.py / test_path_scenes.py.  Zero-length
and non-finite directions are out of scope on purpose."""
import ctypes

import numpy as np
import pytest

import path_scenes as S
from helpers import assert_bitexact

pytestmark = pytest.mark.gpu

G25 = (25, 25, 25)
DRAIN2 = {"PT_DRAIN_DUMP": "64", "PT_DRAIN_LEVELS": "2", "PT_DRAIN_DUMP_TAIL": "64"}


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _renderer(P, scene, accel, pipes, grid=G25, width=256, height=160, **kw):
    r = P.Renderer(P.RenderConfig(width=width, height=height, iterations=2, accel=accel, grid=tuple(grid),
                                  pipelines=pipes, **kw))
    r.allocateOnGPU(scene)
    return r


_check = S.check_rays


def _first(want, k):
    return tuple(v[:k] for v in want)


# --- A. every ray set, both traces, walking in place and with hand-ons -----------------

@pytest.mark.parametrize("pipes", [1, 4])
@pytest.mark.parametrize("accel", [1, 2])
@pytest.mark.parametrize("name", S.RAY_SET_NAMES)
def test_ray_sets(gpu, pt_mod, oracle_mod, name, accel, pipes):
    """One pipeline: k_trace_gf<64,25> walks in place, no drain; four: <64,9> hands
    walks on to its tail and both traces drain.  The model-count scenes pick the
    LDS, wide and global-record variants by themselves."""
    P, O = pt_mod, oracle_mod
    s, grid, o, d, _ = S.ray_set(P, name)
    r = _renderer(P, s, accel, pipes, grid)
    try:
        _check(r, s, o, d, S.ray_set_oracle(P, O, name, accel), what=f"{name} accel={accel} pipes={pipes}")
    finally:
        r.free()


# --- B. environment variants -----------------------------------------------------------

@pytest.mark.parametrize("name,accel,env,deferred", [
    ("ref", 2, {"PT_WALK_WCAP": "7"}, True), ("comb", 2, {"PT_WALK_WCAP": "7"}, True),
    ("comb", 2, {"PT_HS_POOL_BLOCKS": "1"}, True),
    ("ref", 1, DRAIN2, False), ("ref", 2, DRAIN2, False), ("comb", 1, DRAIN2, False), ("comb", 2, DRAIN2, False),
    ("stack-tapered", 1, DRAIN2, False), ("stack-tapered", 2, DRAIN2, False),
    ("stack-dense", 1, DRAIN2, False), ("stack-dense", 2, DRAIN2, False),
    ("ref", 1, {"PT_SORT": "0"}, False), ("ref", 2, {"PT_SORT": "0"}, False),
    ("comb", 1, {"PT_SORT": "0"}, False), ("comb", 2, {"PT_SORT": "0"}, False),
    ("ref", 1, {"PT_SORT": "4"}, False), ("ref", 2, {"PT_SORT": "4"}, False),
    ("comb", 1, {"PT_SORT": "4"}, False), ("comb", 2, {"PT_SORT": "4"}, False),
    ("ref", 1, {"PT_TAIL_BLOCKS": "1"}, False), ("ref", 2, {"PT_TAIL_BLOCKS": "1"}, False),
    ("comb", 1, {"PT_TAIL_BLOCKS": "1"}, False), ("comb", 2, {"PT_TAIL_BLOCKS": "1"}, False),
    ("ref", 1, {"PT_TRACE_RPL": "1000000"}, False), ("ref", 2, {"PT_TRACE_RPL": "1000000"}, False),
    ("comb", 1, {"PT_TRACE_RPL": "1000000"}, False), ("comb", 2, {"PT_TRACE_RPL": "1000000"}, False),
], ids=lambda v: "-".join(f"{k[3:].lower()}{x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_env_variants(gpu, pt_mod, oracle_mod, monkeypatch, name, accel, env, deferred):
    """Four pipelines.  Seven walk hand-on records (the other walks go whole to
    k_trace_deferred), one hit-set pool block on the comb (hit sets beyond it are
    deferred), every ray in flight at exhaustion handed on twice (the stack sets:
    with its stack spilled), no sort and the direction-only key, tail launches on
    one workgroup, and a main launch cut to trace_min_blocks waves."""
    P, O = pt_mod, oracle_mod
    _setenv(monkeypatch, env)
    s, grid, o, d, _ = S.ray_set(P, name)
    r = _renderer(P, s, accel, 4, grid)
    try:
        _check(r, s, o, d, S.ray_set_oracle(P, O, name, accel), what=f"{name} accel={accel} {env}")
        got = r.deferred_rays()
        print(f"trace_rays {name} accel={accel} {env}: deferred_rays={got}")
        if deferred:
            assert got > 0
    finally:
        r.free()


# --- C. batch shapes ---------------------------------------------------------------------

def _miss_rays(n, seed):
    """Origins far outside every world box, pointing away from the scene."""
    rs = np.random.RandomState(seed)
    u = rs.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return (u * rs.uniform(20000, 30000, (n, 1))).astype(np.float32), (u + rs.normal(size=(n, 3)) * 0.2).astype(np.float32)


@pytest.mark.parametrize("pipes", [1, 4])
@pytest.mark.parametrize("accel", [1, 2])
def test_batch_sizes(gpu, pt_mod, oracle_mod, accel, pipes):
    """1, 63, 64, 65 and 3072 rays (one lane, a wave less one, a wave, a wave and
    one, the whole 64 x 48 frame) of the reference-scene set on one renderer."""
    P, O = pt_mod, oracle_mod
    s, grid, o, d, _ = S.ray_set(P, "ref")
    want = S.ray_set_oracle(P, O, "ref", accel)
    r = _renderer(P, s, accel, pipes, width=64, height=48)
    try:
        for n in (1, 63, 64, 65, 3072, 1):
            _check(r, s, o[:n], d[:n], _first(want, n), what=f"n={n} accel={accel} pipes={pipes}")
    finally:
        r.free()


@pytest.mark.parametrize("pipes", [1, 4])
@pytest.mark.parametrize("accel", [1, 2])
def test_all_miss_and_one_hit_among_misses(gpu, pt_mod, oracle_mod, accel, pipes):
    """3072 rays that miss every world box (every lane is done at its first
    select), then one comb-axis ray (a hit set beyond the LDS entries) first and,
    the batch reversed, last among 3071 of them."""
    P, O = pt_mod, oracle_mod
    s, grid, o, d, _ = S.ray_set(P, "comb")
    mo, md = _miss_rays(3072, 17)
    r = _renderer(P, s, accel, pipes, width=64, height=48)
    try:
        want = S.oracle_hits(O, "comb-miss", s, mo, md, accel)
        assert (want[2] == -1).all()
        _check(r, s, mo, md, want, what="all miss")
        o1 = np.concatenate([o[:1], mo[1:]]); d1 = np.concatenate([d[:1], md[1:]])
        want = S.oracle_hits(O, "comb-one", s, o1, d1, accel)
        assert want[2][0] >= 0 and (want[2][1:] == -1).all()
        _check(r, s, o1, d1, want, what="one hit first")
        _check(r, s, o1[::-1].copy(), d1[::-1].copy(), tuple(v[::-1].copy() for v in want), what="one hit last")
    finally:
        r.free()


@pytest.mark.parametrize("pipes", [1, 4])
@pytest.mark.parametrize("accel", [1, 2])
def test_results_follow_the_rays(gpu, pt_mod, oracle_mod, accel, pipes):
    """3072 rays sorted by the oracle's model id (misses first: whole waves whose
    lanes finish together) and the same rays shuffled."""
    P, O = pt_mod, oracle_mod
    s, grid, o, d, _ = S.ray_set(P, "ref")
    want = _first(S.ray_set_oracle(P, O, "ref", accel), 3072)
    r = _renderer(P, s, accel, pipes, width=64, height=48)
    try:
        for what, order in (("by model", np.argsort(want[2], kind="stable")),
                            ("shuffled", np.random.RandomState(23).permutation(3072))):
            _check(r, s, o[:3072][order], d[:3072][order], tuple(v[order] for v in want), what=what)
    finally:
        r.free()


# --- D. survivor layouts -------------------------------------------------------------------

@pytest.mark.parametrize("sort", [-1, 0], ids=["sort", "nosort"])
@pytest.mark.parametrize("accel", [1, 2])
def test_layouts_across_scan_tiles(gpu, pt_mod, oracle_mod, accel, sort):
    """640 x 512 at chunk 64: 5120 source blocks, two k_scan tiles.  20 000 rays of
    the reference-scene set dense, at random counts, as islands of one ray 97
    blocks apart, behind 4096 empty blocks, in the last blocks and in blocks of
    alternately 1 and 63."""
    P, O = pt_mod, oracle_mod
    s, grid, o, d, _ = S.ray_set(P, "ref")
    want = S.ray_set_oracle(P, O, "ref", accel)
    L = S.layouts(640 * 512, 64, 20000, 3)
    assert set(L) == {"dense", "random", "islands", "tile_gap", "last", "ragged"}
    r = _renderer(P, s, accel, 4, width=640, height=512, ray_sort=sort)
    try:
        for name, c in L.items():
            k = int(c.sum())
            _check(r, s, o[:k], d[:k], _first(want, k), counts=c, what=f"layout {name} accel={accel} sort={sort}")
    finally:
        r.free()


@pytest.mark.parametrize("sort", [-1, 0], ids=["sort", "nosort"])
@pytest.mark.parametrize("accel", [1, 2])
@pytest.mark.parametrize("block", [128, 256])
def test_layouts_at_larger_chunks(gpu, pt_mod, oracle_mod, block, accel, sort):
    """128 x 96 at chunk 128 and 256 (k_scan's chunk, slot_source and the sort
    kernels' index arithmetic; the hook runs no k_bounce): 4000 rays at random
    counts, at alternately 1 and chunk - 1, and as islands."""
    P, O = pt_mod, oracle_mod
    s, grid, o, d, _ = S.ray_set(P, "ref")
    want = S.ray_set_oracle(P, O, "ref", accel)
    L = S.layouts(128 * 96, block, 4000, 5)
    r = _renderer(P, s, accel, 4, width=128, height=96, ray_sort=sort, block=block)
    try:
        for name in ("random", "ragged", "islands"):
            k = int(L[name].sum())
            _check(r, s, o[:k], d[:k], _first(want, k), counts=L[name], what=f"layout {name} block={block} accel={accel}")
    finally:
        r.free()


# --- E. scaled directions ----------------------------------------------------------------------

@pytest.mark.parametrize("accel", [1, 2])
@pytest.mark.parametrize("kind", S.SCALINGS)
def test_scaled_directions(gpu, pt_mod, oracle_mod, kind, accel):
    """Directions of length 2^-20..2^20, |1 - 2c|, 1e-6..1e-3 and 1e-6..1e6 (a
    bounce direction is not a unit vector): the oracle's result for the scaled
    rays, and for powers of two the GPU's own distances of the unscaled rays."""
    P, O = pt_mod, oracle_mod
    s = S._ref_scene(P)
    o, d = S.room_interior_rays(s.export(), 20000, 31)
    dk = S.scaled(d, kind, 40 + S.SCALINGS.index(kind))
    r = _renderer(P, s, accel, 4)
    try:
        t, _, m, _ = _check(r, s, o, dk, S.oracle_hits(O, f"scaled-{kind}", s, o, dk, accel), what=f"{kind} accel={accel}")
        if kind == "pow2":
            t0, _, m0, _ = r.trace_rays(o, d)
            assert_bitexact(t, t0, "pow2 vs unscaled dist")
            assert_bitexact(m, m0, "pow2 vs unscaled model")
    finally:
        r.free()


# --- F. renderer state ---------------------------------------------------------------------------

@pytest.mark.parametrize("pipes", [1, 4])
@pytest.mark.parametrize("accel", [1, 2])
def test_renderer_state_is_a_finished_bounce(gpu, pt_mod, oracle_mod, accel, pipes):
    """trace_rays twice gives the same records; a render after it, and a render
    around it (iterations 0-1, trace_rays, iterations 2-3), equal the oracle's
    image and segment count, and the per-bounce counters equal those of a
    renderer that never ran the hook."""
    P, O = pt_mod, oracle_mod
    s, grid, o, d, _ = S.ray_set(P, "ref")
    want = _first(S.ray_set_oracle(P, O, "ref", accel), 3000)
    o, d = o[:3000], d[:3000]
    counts = S.layouts(64 * 48, 64, 3000, 9)["random"]
    for iters, loops in ((2, [(0, 2)]), (4, [(0, 2), (2, 2)])):
        cfg = P.RenderConfig(width=64, height=48, iterations=iters, accel=accel, pipelines=pipes)
        oimg, oseg = S.oracle_render(O, "ref", s, cfg)
        plain = P.Renderer(cfg)
        r = P.Renderer(cfg)
        try:
            plain.allocateOnGPU(s)
            for first, n in loops:
                plain.renderLoop(first, n)
            r.allocateOnGPU(s)
            if len(loops) == 2:
                r.renderLoop(*loops[0])
            a = _check(r, s, o, d, want, counts=counts, what=f"first call, {iters} iterations")
            b = _check(r, s, o, d, want, counts=counts, what=f"second call, {iters} iterations")
            for x, y in zip(a, b):
                assert_bitexact(x, y, "trace_rays twice")
            r.renderLoop(*loops[-1])
            assert r.trace_faults() == 0
            assert r.segments() == oseg == plain.segments()
            assert_bitexact(r.image(), oimg, f"image after trace_rays, {iters} iterations")
            assert r.segments_per_bounce(8) == plain.segments_per_bounce(8)
        finally:
            r.free()
            plain.free()


# --- G. refusals ---------------------------------------------------------------------------------

def test_refusals_start_nothing(gpu, pt_mod, oracle_mod, monkeypatch):
    """Every unusable input is refused with a message before any launch: the
    counters do not move, and the renderer then traces and renders correctly."""
    P, O = pt_mod, oracle_mod
    s, grid, o, d, _ = S.ray_set(P, "ref")
    o, d = o[:100], d[:100]
    r = P.Renderer(P.RenderConfig(width=64, height=48, iterations=2, accel=2))
    with pytest.raises(P.PathTracerError, match="not allocated"):
        r.trace_rays(o, d)
    r.free()
    r = _renderer(P, s, 0, 4, width=64, height=48)
    with pytest.raises(P.PathTracerError, match="accel"):
        r.trace_rays(o, d)
    r.free()
    for accel, var in ((2, "PT_GF_SPLIT"), (1, "PT_TRACE_SPLIT")):
        monkeypatch.setenv(var, "0")
        r = _renderer(P, s, accel, 4, width=64, height=48)
        monkeypatch.delenv(var)
        with pytest.raises(P.PathTracerError, match="split"):
            r.trace_rays(o, d)
        r.free()
    for accel in (1, 2):
        cfg = P.RenderConfig(width=64, height=48, iterations=2, accel=accel, pipelines=4)
        r = P.Renderer(cfg)
        r.allocateOnGPU(s)
        try:
            r.renderLoop(0, 1)
            before = (r.segments(), r.segments_per_bounce(128))
            big = np.zeros((64 * 48 + 1, 3), np.float32) + 1
            full = np.full(48, 64, np.int32)
            for what, args in (("n must be", (big, big)),
                               ("outside", (o, d, [101, -1])), ("outside", (o, d, [35, 65])),
                               ("do not sum", (o, d, [64, 35])), ("do not sum", (o, d, [64, 37])),
                               ("more blocks", (o, d, [0] * 47 + [50, 50]))):
                with pytest.raises(P.PathTracerError, match=what):
                    r.trace_rays(*args)
            t = np.zeros(4, np.float32); m = np.zeros(4, np.int32)
            fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
            rc = P.lib().pt_renderer_trace_rays(r._h, -1, o.ctypes.data_as(fp), d.ctypes.data_as(fp), None, 0,
                                               t.ctypes.data_as(fp), t.ctypes.data_as(fp), m.ctypes.data_as(ip),
                                               m.ctypes.data_as(ip))
            assert rc < 0 and b"n must be" in P.lib().pt_last_error()
            assert (r.segments(), r.segments_per_bounce(128)) == before
            _check(r, s, o, d, _first(S.ray_set_oracle(P, O, "ref", accel), 100), counts=[64, 36])
            _check(r, s, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32),
                   _first(S.ray_set_oracle(P, O, "ref", accel), 0), counts=full * 0)
            r.renderLoop(1, 1)
            oimg, oseg = S.oracle_render(O, "ref", s, cfg)
            assert r.segments() == oseg
            assert_bitexact(r.image(), oimg, "image after the refusals")
        finally:
            r.free()
