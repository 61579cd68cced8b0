"""The yardstick of the environment tests, held to the oracle (CPU only): with a constant
0.01 map the restatement in env_ref.py is camera_ref's bit for bit (0.01 + 0*t is exact, so
the lookup returns the reference's constant for every direction, rotation and map size), and
the assumption its override rests on -- ptor_shade gives a missing ray (its colour) * 0.01f
and bounces 0 -- is checked directly."""
import numpy as np
import pytest

import camera_ref as CR
import env_ref as ER
from conftest import INPUT_DATA
from helpers import assert_bitexact

F = np.float32
W, H, BOUNCES = 64, 48, 5


@pytest.fixture(scope="module")
def flat(oracle_mod):
    return oracle_mod.reference_scene(INPUT_DATA)


def random_rotation(seed):
    q, r = np.linalg.qr(np.random.RandomState(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[2] = -q[2]
    return q.astype(F)


def directions(seed, m=2000):
    rs = np.random.RandomState(seed)
    d = (rs.normal(size=(m, 3)) * 10.0 ** rs.uniform(-3, 3, (m, 1))).astype(F)
    d[:6] = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    d[np.arange(6, 40), rs.randint(0, 3, 34)] = 0.0
    return d


_WANT = {}


def parent_render(flat, cfg, accel):
    if accel not in _WANT:
        ref = CR.Restatement(flat, cfg)
        ref.render(0, 3)
        _WANT[accel] = ref
    return _WANT[accel]


@pytest.mark.parametrize("accel", [0, 1])
@pytest.mark.parametrize("n,rot_seed", [(1, None), (1, 3), (2, 4), (5, 5)])
def test_constant_one_percent_is_the_parent(oracle_mod, flat, accel, n, rot_seed):
    O = oracle_mod
    cfg = O.RenderConfig(width=W, height=H, max_bounces=BOUNCES, accel=accel, threads=4)
    want = parent_render(flat, cfg, accel)
    env = ER.Env(np.full((n, n, 3), 0.01, F), rot=None if rot_seed is None else random_rotation(rot_seed))
    got = ER.Restatement(flat, cfg, env=env)
    got.render(0, 3)
    what = f"accel {accel} n {n} rotation {rot_seed}"
    assert want.S.any() and got.misses[1:].sum() >= 100, got.misses[:6]
    assert_bitexact(got.S, want.S, f"{what}: image")
    assert_bitexact(got.Q, want.Q, f"{what}: moments")
    assert_bitexact(got.counts, want.counts, f"{what}: counts")
    assert got.segments == want.segments and got.live == want.live, what
    assert got.per_bounce.tolist() == want.per_bounce.tolist(), what


def test_an_environment_changes_colours_only(oracle_mod, flat):
    """A random map: other colours, the same rays."""
    O = oracle_mod
    cfg = O.RenderConfig(width=W, height=H, max_bounces=BOUNCES, accel=0, threads=4)
    want = parent_render(flat, cfg, 0)
    env = ER.Env(np.random.RandomState(8).uniform(0, 2, (8, 8, 3)), (1.5, 1, 0.5), random_rotation(9))
    got = ER.Restatement(flat, cfg, env=env)
    got.render(0, 3)
    assert np.isfinite(got.S).all()
    differ = (got.S.view(np.uint32) != want.S.view(np.uint32)).any(axis=1).sum()
    print(f"{differ} of {W * H} pixels differ; misses by depth {got.misses[:BOUNCES].tolist()}")
    assert differ > W * H // 2
    assert got.segments == want.segments and got.live == want.live
    assert_bitexact(got.counts, want.counts, "counts")


@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_constant_map_returns_the_constant_times_the_scale(n):
    c, scale = np.float32([0.3, 1.7, 0.01]), np.float32([1.5, 1.0, 0.5])
    d = directions(n)
    d[40] = 0.0                                                   # a zero direction: NaN coordinates read texel (0, 0)
    for rot in (None, random_rotation(n)):
        got = ER.lookup(np.broadcast_to(c, (n, n, 3)), np.eye(3, dtype=F) if rot is None else rot, scale, d)
        assert_bitexact(got, np.broadcast_to((c * scale).astype(F), got.shape), f"n {n}")


def test_lookup_reads_the_texel_under_the_direction():
    """On a map whose texels hold their own column and row, the direction of every texel's
    centre reads that texel's coordinates: the mapping and its fold are the layout's inverse."""
    n = 8
    tex = np.zeros((n, n, 3), F)
    tex[..., 0] = np.arange(n)[None, :]
    tex[..., 1] = np.arange(n)[:, None]
    p = (np.arange(n) + 0.5) / n * 2 - 1
    px, py = np.meshgrid(p, p)
    ez = 1 - np.abs(px) - np.abs(py)
    low = ez < 0
    ex = np.where(low, (1 - np.abs(py)) * np.where(px >= 0, 1, -1), px)
    ey = np.where(low, (1 - np.abs(px)) * np.where(py >= 0, 1, -1), py)
    d = np.stack([ex, ey, ez], axis=-1).reshape(-1, 3).astype(F)
    got = ER.lookup(tex, np.eye(3, dtype=F), (1, 1, 1), d).reshape(n, n, 3)
    # the coordinate is recovered to float32 rounding (a few ulp of 1 times n/2 texels): the
    # bilinear value of an index ramp is the coordinate itself
    assert np.abs(got[..., 0] - tex[..., 0]).max() < 1e-5 and np.abs(got[..., 1] - tex[..., 1]).max() < 1e-5
    # the poles: +z is the map's centre, -z its corners
    mid = ER.lookup(tex, np.eye(3, dtype=F), (1, 1, 1), np.float32([[0, 0, 2]]))[0]
    assert mid[0] == F(3.5) and mid[1] == F(3.5)
    low = ER.lookup(tex, np.eye(3, dtype=F), (1, 1, 1), np.float32([[0, 0, -2]]))[0]
    assert low[0] == F(7) and low[1] == F(7)


def test_the_parent_gives_a_missing_ray_one_percent_and_no_bounces(oracle_mod, flat):
    """What the override replaces: for rays that miss, ptor_shade leaves colour = saved * 0.01f
    and bounces = 0, whatever their depth."""
    O = oracle_mod
    cfg = O.RenderConfig(width=W, height=H, max_bounces=BOUNCES, accel=0, threads=4)
    ref = CR.Restatement(flat, cfg)
    rs = np.random.RandomState(12)
    m = 512
    o = np.ascontiguousarray(rs.uniform(-300, 300, (m, 3)) + [0, 100, 0], F)
    d = np.ascontiguousarray(rs.normal(size=(m, 3)), F)
    dist, nrm, model = O.intersect_rays(flat, o, d, accel=0, threads=4)
    miss = model < 0
    assert 20 < miss.sum() < m - 20
    for depth_left in (BOUNCES, 3, 1):
        color = np.ascontiguousarray(rs.uniform(0, 1, (m, 3)), F)
        bounces = np.full(m, depth_left, np.int32)
        saved, oo, dd = color.copy(), o.copy(), d.copy()
        ref._shade_batch(0, np.arange(m, dtype=np.int32), oo, dd, color, bounces, dist, nrm, model)
        assert_bitexact(color[miss], (saved[miss] * F(0.01)).astype(F), f"bounces {depth_left}: a miss's colour")
        assert (bounces[miss] == 0).all()
