"""The yardstick of the dielectric-material tests (CPU only): with no dielectric model the
restatement in glass_ref.py is texture_ref's bit for bit; the float32 definition agrees with a
float64 evaluation of the same formulas; its outputs are finite for every input of the GPU hook
test; refracted directions obey Snell's law; and the fixture reaches every event often enough.

Float32 against float64, measured on the 10^6 pairs below: the share of inputs within 1e-5 of the
critical angle (|k64| <= 1e-5, left out, where the event itself may differ) is about 3e-6, the
largest difference of a direction component 4.9e-5 and of Fr 2.6e-4.  The bounds are about four
times those: 2e-4 and 1e-3."""
import numpy as np
import pytest

import glass_ref as GR
import glass_scenes as GS
import path_scenes as PS
import texture_ref as TR
from helpers import assert_bitexact, flat_from_export, oracle_cfg

F = np.float32
W, H, BOUNCES, ITERS = 64, 48, 6, 3
K_LEFT_OUT, SHARE_BOUND, DIR_BOUND, FR_BOUND = 1e-5, 0.01, 2e-4, 1e-3
EVENTS_AT_LEAST, SMOOTH_EXITS_AT_LEAST = 50, 20


def same_render(got, want, what):
    assert_bitexact(got.S, want.S, f"{what}: image")
    assert_bitexact(got.Q, want.Q, f"{what}: moments")
    assert got.segments == want.segments and got.live == want.live, what
    assert got.per_bounce.tolist() == want.per_bounce.tolist(), what


@pytest.mark.parametrize("accel", [0, 1])
def test_no_dielectric_model_is_the_parent(oracle_mod, accel):
    O = oracle_mod
    flat = PS.oracle_scene_from_spec(O, *PS.seven_material_spec())
    cfg = O.RenderConfig(width=W, height=H, max_bounces=BOUNCES, accel=accel, threads=4)
    want = TR.Restatement(flat, cfg)
    want.render(0, ITERS)
    got = GR.Restatement(flat, cfg, ior=np.full(len(flat.model_ints), 2.0, F))       # an ior alone changes nothing
    got.render(0, ITERS)
    assert want.S.any() and not got.glass.any() and not got.events.any()
    same_render(got, want, "no dielectric model")


def random_pairs(n, seed):
    rs = np.random.RandomState(seed)
    d = GS.unit(rs.normal(size=(n, 3))).astype(F)
    nrm = GS.unit(rs.normal(size=(n, 3))).astype(F)
    return GR.SR._normalize(d), nrm, rs.uniform(1.0, 4.0, n).astype(F), rs.uniform(0, 1, n).astype(F)


def test_float32_definition_agrees_with_float64():
    d, n, ior, u = random_pairs(1_000_000, 5)
    got, want = GR.scatter(d, n, ior, u), GR.scatter64(d, n, ior)
    keep = np.abs(want["k"]) > K_LEFT_OUT
    share = 1.0 - keep.mean()
    tir32 = got["event"] == GR.TIR
    refl = got["event"] >= GR.REFLECT
    d64 = np.where(refl[:, None], want["d_reflect"], want["d_refract"])
    ok = keep & (tir32 == want["tir"])
    dir_diff = float(np.abs(got["d"].astype(np.float64) - d64)[ok].max())
    pair = ok & ~tir32
    fr_diff = float(np.abs(got["fr"].astype(np.float64) - want["fr"])[pair].max())
    print(f"{share:.3g} of the inputs within {K_LEFT_OUT} of the critical angle; {tir32.sum()} total internal reflections; "
          f"largest float32 - float64 difference {dir_diff:.3g} in a direction component, {fr_diff:.3g} in Fr")
    assert share < SHARE_BOUND
    assert (tir32 == want["tir"])[keep].all()
    assert tir32.sum() > 10_000 and (got["event"] == GR.REFRACT_OUT).sum() > 10_000
    assert dir_diff <= DIR_BOUND and fr_diff <= FR_BOUND
    # the sides: a reflected direction on nn's side, a refracted one on the other, none short
    side = GR._dot(got["d"], got["nn"])
    assert (side[refl] >= 0).all() and (side[~refl] <= 0).all()
    length = np.sqrt((got["d"].astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(length - 1.0).max() <= 2e-6 * 4                     # ior up to 4 scales the rounding of dir * eta


def test_outputs_are_finite_for_the_hook_inputs():
    (d, n, ior, u), where = GS.hook_inputs()
    out, event = GR.hook(d, n, ior, u)
    assert np.isfinite(out).all() and out.dtype == F and set(np.unique(event)) <= {0, 1, 2, 3}
    counts = {name: np.bincount(event[sl], minlength=4).tolist() for name, sl in where.items()}
    print(counts)
    assert all(c > 100 for c in counts["random"])                    # every event among the random inputs
    assert counts["normal incidence, entering"] == [6, 0, 0, 0] and counts["normal incidence, leaving"] == [0, 6, 0, 0]
    for ior_c in (1.33, 1.5, 4.0):                                   # the ulp steps cross the critical angle: both events
        c = counts[f"critical angle, ior {ior_c}"]
        assert c[GR.TIR] > 10 and c[GR.REFRACT_OUT] + c[GR.REFLECT] > 10 and c[GR.REFRACT_IN] == 0
    sl = where["u at Fr"]
    fr = GR.scatter(GR.SR._normalize(d[sl]), n[sl], ior[sl], u[sl])["fr"]
    has = np.isfinite(fr)
    kind = np.arange(96) % 3
    refracts = event[sl] <= GR.REFRACT_OUT
    assert refracts[has & (kind == 0)].all()                         # u == Fr: not u < Fr
    assert not refracts[has & (kind == 1)].any() and not refracts[has & (kind == 2)].any()
    # ior 1: k = 1 - (1 - c*c) is c*c up to 2^-23, so there is no total internal reflection and a
    # refracted ray goes straight on up to |c - sk| <= sqrt(2 * 2^-23) = 4.9e-4
    one = where["ior one"]
    through = event[one] <= GR.REFRACT_OUT
    assert (event[one] != GR.TIR).all() and through.sum() > 32
    assert np.abs(out[one] - GR.SR._normalize(d[one]))[through].max() <= 4.9e-4


def test_refracted_directions_obey_snells_law():
    d, n, ior, u = random_pairs(200_000, 9)
    got = GR.scatter(d, n, ior, u)
    refr = got["event"] <= GR.REFRACT_OUT
    assert refr.sum() > 50_000
    d64, n64, o64 = d.astype(np.float64)[refr], n.astype(np.float64)[refr], got["d"].astype(np.float64)[refr]
    ent = got["event"][refr] == GR.REFRACT_IN
    n1 = np.where(ent, 1.0, ior.astype(np.float64)[refr])
    n2 = np.where(ent, ior.astype(np.float64)[refr], 1.0)
    sin_i = np.linalg.norm(np.cross(d64, n64), axis=1)
    sin_t = np.linalg.norm(np.cross(o64, n64), axis=1)
    worst = float(np.abs(n1 * sin_i - n2 * sin_t).max())
    # the tangential parts are parallel: the refracted ray stays in the plane of incidence
    ti = d64 - (d64 * n64).sum(axis=1, keepdims=True) * n64
    tt = o64 - (o64 * n64).sum(axis=1, keepdims=True) * n64
    out_of_plane = float(np.linalg.norm(np.cross(ti, tt), axis=1).max())
    print(f"{refr.sum()} refractions: largest |n1 sin(i) - n2 sin(t)| {worst:.3g}, out of plane {out_of_plane:.3g}")
    # float32 directions (unit to 2e-6, components to 5e-5 under ior up to 4): 4 * 2e-4
    assert worst <= 8e-4 and out_of_plane <= 8e-4


_FIX = {}


def fixture(P):
    if not _FIX:
        spec = GS.fixture_spec()
        scene = GS.gpu_scene(P, spec)
        _FIX["f"] = (flat_from_export(scene.export()), spec)
    return _FIX["f"]


@pytest.mark.parametrize("accel", ["grid_fast", "bvh"])
def test_the_fixture_reaches_every_event(pt_mod, oracle_mod, accel):
    P = pt_mod
    flat, spec = fixture(P)
    assert flat.model_ints[:, 2].tolist() == [0, 4, 7, 7, 7, 7, 0]
    cfg = P.RenderConfig(width=W, height=H, max_bounces=BOUNCES, iterations=ITERS,
                         accel={"grid_fast": P.ACCEL_GRID_FAST, "bvh": P.ACCEL_BVH}[accel])
    ref = GR.Restatement(flat, oracle_cfg(cfg, threads=4), smooth=spec["smooth"], uv=GS.vertex_uv(spec),
                         textures=spec["textures"], binding=spec["binding"], ior=spec["ior"])
    ref.render(0, ITERS)
    print(f"{accel}: events {dict(zip(GR.EVENT_NAMES, ref.events.tolist()))}, {ref.smooth_exits} exits on the smooth instance, "
          f"{ref.tex_hits} colours decided by a texture")
    assert (ref.events >= EVENTS_AT_LEAST).all()
    assert ref.smooth_exits >= SMOOTH_EXITS_AT_LEAST
    assert ref.ident.holds() and ref.tex_ident.holds() and ref.ident.hits > 100 and ref.tex_ident.hits > 100
    assert np.isfinite(ref.S).all() and ref.S.any()
    # glass is not diffuse: the same fixture with the dielectric instances DIFFUSE renders another image
    plain = GR.Restatement(flat_as_diffuse(flat), oracle_cfg(cfg, threads=4), smooth=spec["smooth"], uv=GS.vertex_uv(spec),
                           textures=spec["textures"], binding=spec["binding"], ior=spec["ior"])
    plain.render(0, ITERS)
    assert not plain.events.any()
    differ = (ref.S.view(np.uint32) != plain.S.view(np.uint32)).any(axis=1).sum()
    assert differ > W * H // 8


def flat_as_diffuse(flat):
    import copy
    out = copy.copy(flat)
    ints = np.array(flat.model_ints, copy=True)
    ints[ints[:, 2] == GR.DIELECTRIC, 2] = 0
    out.model_ints = ints
    return out
