"""The yardstick of the texture tests, held to the oracle (CPU only): with no textured model the
restatement in texture_ref.py is smooth_ref's and the oracle's render bit for bit, as it is with a
1x1 white texture on every model; a uniform texture of colour k on a white model is that model
coloured k; the triangle identification holds on the fixtures for every hit; the texel indices stay
inside the texture for every float input; and the float32 lookup agrees with a float64 evaluation
of the same formula.

Float32 against float64, measured over the fixtures' hits and the synthetic uvs below: the largest
difference of a looked-up value is 1.9e-6 for textures of up to 64 texels a side (the rounding of
fr * n, about 6e-8 * n of a texel, times the contrast between neighbouring texels) and 1.2e-4 at
4096 texels a side.  The bounds are about 30 times that: 6e-5 and 4e-3."""
import numpy as np
import pytest

import path_scenes as PS
import smooth_ref as SR
import texture_ref as TR
import texture_scenes as TS
from helpers import assert_bitexact

F = np.float32
W, H, BOUNCES, ITERS = 64, 48, 4, 2
BOUND_SMALL, BOUND_4096 = 6e-5, 4e-3


def cfg_of(O, accel):
    return O.RenderConfig(width=W, height=H, max_bounces=BOUNCES, accel=accel, threads=4)


_FIX = {}


def fixture(O, extra=False):
    if extra not in _FIX:
        spec = TS.fixture_spec(extra=TS.zero_area_extra() if extra else None)
        _FIX[extra] = (PS.oracle_scene_from_spec(O, spec["meshes"], spec["models"]), spec)
    return _FIX[extra]


def restate(flat, cfg, spec, binding="own", textures=None, smooth=True):
    ref = TR.Restatement(flat, cfg, smooth=spec["smooth"] if smooth else None, uv=TS.vertex_uv(spec),
                         textures=spec["textures"] if textures is None else textures,
                         binding=spec["binding"] if isinstance(binding, str) else binding)
    ref.render(0, ITERS)
    return ref


def same_render(got, want, what):
    assert_bitexact(got.S, want.S, f"{what}: image")
    assert_bitexact(got.Q, want.Q, f"{what}: moments")
    assert got.segments == want.segments and got.live == want.live, what
    assert got.per_bounce.tolist() == want.per_bounce.tolist(), what


@pytest.mark.parametrize("accel", [0, 1])
def test_no_textured_model_is_the_parent_and_the_oracle(oracle_mod, accel):
    O = oracle_mod
    flat, spec = fixture(O)
    cfg = cfg_of(O, accel)
    want = SR.Restatement(flat, cfg, smooth=spec["smooth"])
    want.render(0, ITERS)
    got = restate(flat, cfg, spec, binding=None)
    assert want.S.any() and got.tex_hits == 0 and got.tex_ident.hits == 0
    same_render(got, want, "no textured model")
    unsmooth = restate(flat, cfg, spec, binding=None, smooth=False)
    image, _ = O.render(flat, O.RenderConfig(width=W, height=H, iterations=ITERS, max_bounces=BOUNCES, accel=accel, threads=4))
    assert_bitexact(unsmooth.S, image, "the oracle's image")
    # without textures the primary albedo is the hit model's colour
    want_albedo = np.where((want.hit_model >= 0)[:, None], flat.model_color[np.maximum(want.hit_model, 0)], F(0))
    assert_bitexact(got.primary_albedo(), want_albedo.astype(F), "primary albedo, untextured")


def test_a_white_texel_on_every_model_changes_nothing(oracle_mod):
    """c * 1.0f is c.  The torus models only: the identification needs distinct flat normals."""
    O = oracle_mod
    flat, spec = fixture(O)
    cfg = cfg_of(O, 1)
    want = restate(flat, cfg, spec, binding=None)
    binding = np.where(spec["binding"] >= 0, 0, -1)
    got = restate(flat, cfg, spec, binding=binding, textures=[np.ones((1, 1, 3), F)])
    assert got.tex_hits > 1000
    same_render(got, want, "1x1 white")


def test_a_uniform_texture_on_a_white_model_is_that_colour(oracle_mod):
    O = oracle_mod
    flat, spec = fixture(O)
    cfg = cfg_of(O, 0)
    colours = np.asarray(flat.model_color, F).copy()
    textured = spec["binding"] >= 0
    uniform = [np.broadcast_to(colours[i], (3, 2, 3)).astype(F) for i in np.nonzero(textured)[0]]
    binding = np.full(len(textured), -1)
    binding[textured] = np.arange(textured.sum())
    want = restate(flat, cfg, spec, binding=None)
    import copy
    white = copy.copy(flat)
    white.model_color = np.where(textured[:, None], F(1), colours).astype(F)
    got = restate(white, cfg, spec, binding=binding, textures=uniform)
    assert got.tex_hits > 1000
    same_render(got, want, "uniform texture on white")


@pytest.mark.parametrize("accel", [0, 1])
def test_identification_holds_for_every_textured_hit(oracle_mod, accel):
    O = oracle_mod
    flat, spec = fixture(O, extra=True)
    ref = restate(flat, cfg_of(O, accel), spec)
    albedo = ref.primary_albedo()
    i = ref.tex_ident
    print(f"accel {accel}: {i.hits} identified hits on textured models, nearest candidate at most {i.worst_near:.3g} "
          f"away, second nearest at least {i.least_second:.3g}; {ref.tex_hits} colours decided by a texture")
    assert i.hits > 1000 and i.holds() and ref.tex_hits > 1000
    assert np.isfinite(ref.S).all() and np.isfinite(albedo).all()
    plain = restate(flat, cfg_of(O, accel), spec, binding=None)
    differ = (ref.S.view(np.uint32) != plain.S.view(np.uint32)).any(axis=1).sum()
    print(f"{differ} of {W * H} pixels differ from the untextured render")
    assert differ > W * H // 4


def synthetic_uv(n):
    """Negative values, values above 1, exact integers, k/n texel borders, texel centres, and
    -1e-9 (where fr rounds to 1.0); with seeded fill."""
    rs = np.random.RandomState(7)
    k = np.arange(-2 * n, 3 * n + 1, max(1, n // 64))
    special = np.concatenate([np.arange(-4, 5).astype(np.float64), k / n, (k + 0.5) / n, [-1e-9, 1e-9, 1 - 1e-9, -0.5 / n],
                              np.nextafter(F(1), F(0), dtype=F).astype(np.float64)[None]])
    u = np.concatenate([special, rs.uniform(-2, 3, 2000)]).astype(F)
    v = np.concatenate([rs.permutation(special), rs.uniform(-2, 3, 2000)]).astype(F)
    return np.stack([u, v], axis=1)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 4096])
def test_texel_indices_stay_inside_the_texture(n):
    bad = F([np.nan, np.inf, -np.inf, 3.4e38, -3.4e38, 1e-45, -1e-45, 0.0, -0.0, 16777216.0, -16777217.0])
    a = np.concatenate([synthetic_uv(n).reshape(-1), bad])
    i0, i1, t = TR.axis(a, n)
    assert i0.min() >= 0 and i0.max() <= n - 1 and i1.min() >= 0 and i1.max() <= n - 1
    assert np.isfinite(t).all() and t.min() >= 0 and t.max() < 1
    assert (i1 == (i0 + 1) % n).all()
    near_one = TR.axis(F([-1e-9]), n)                    # fr rounds to 1.0: f = n - 0.5, between the last texel and the first
    assert (int(near_one[0][0]), int(near_one[1][0]), float(near_one[2][0])) == (n - 1, 0, 0.5)


def test_float32_lookup_agrees_with_float64(oracle_mod):
    O = oracle_mod
    flat, spec = fixture(O)
    # the fixtures' hits: the uvs the restatement interpolates at the primary hits of the textured models
    ref = TR.Restatement(flat, cfg_of(O, 1), smooth=spec["smooth"], uv=TS.vertex_uv(spec), textures=spec["textures"],
                         binding=spec["binding"])
    o = np.repeat(np.asarray(ref.cam, F)[None, :], ref.npix, axis=0)
    tri = SR.shading_normals(flat, ref.tables, ref.textured, o, ref.dirs, ref.hit_dist, ref.hit_nrm, ref.hit_model)[1]
    worst_small, hits = 0.0, 0
    for k in np.nonzero(ref.textured)[0]:
        sel = np.nonzero(ref.hit_model == k)[0]
        T = ref.tables.of(int(k))
        t = tri[sel] - T["first"]
        b = TR.barycentrics(np.asarray(flat.model_w2m, F)[k], T["v0"][t], T["e1"][t], T["e2"][t], o[sel], ref.dirs[sel],
                            ref.hit_dist[sel])
        uv = TR.interpolate_uv(*(u[t] for u in ref.uvt.of(int(k))), *b)
        tex = ref.textures[ref.binding[k]]
        worst_small = max(worst_small, float(np.abs(TR.lookup(tex, uv).astype(np.float64) - TR.lookup64(tex, uv)).max()))
        hits += len(sel)
    assert hits > 300
    rs = np.random.RandomState(3)
    worst_4096 = 0.0
    for w, h in TS.TEXTURE_SIZES + [(3, 2), (4096, 1), (1, 4096), (4096, 3)]:
        tex = rs.uniform(0, 1, (h, w, 3)).astype(F)
        for n in (w, h):
            uv = synthetic_uv(n)
            diff = float(np.abs(TR.lookup(tex, uv).astype(np.float64) - TR.lookup64(tex, uv)).max())
            if max(w, h) > 64:
                worst_4096 = max(worst_4096, diff)
            else:
                worst_small = max(worst_small, diff)
    print(f"{hits} fixture hits and the synthetic uvs: largest float32 - float64 difference {worst_small:.3g} up to 64 "
          f"texels a side, {worst_4096:.3g} at 4096")
    assert worst_small <= BOUND_SMALL and worst_4096 <= BOUND_4096
