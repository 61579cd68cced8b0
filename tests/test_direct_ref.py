"""The yardstick of the direct-lighting tests (CPU only): with no EMISSIVE model, or with the
switch off, the restatement in direct_ref.py is glass_ref's bit for bit; the estimator with and
without light sampling has the same expectation; and light sampling lowers the noise estimate.

Same expectation, measured with the iteration ids below (16 x 12 frame of the fixture room,
ACCEL_BVH, max_bounces 4, 8 batches of 32 iterations each way): per image quadrant the two
estimators' batch means differ by -2.5, -1.5, -2.0 and -2.4 standard errors of the difference
(light sampling the brighter one: a path's last diffuse vertex samples the lights too, where the
plain estimator's scattered ray is never traced).  The frame-mean noise estimate at 32 samples is
0.0970 with light sampling against 0.1034 without, a ratio of 0.94."""
import copy

import numpy as np
import pytest

import direct_ref as DR
import glass_ref as GR
import glass_scenes as GS
import noise_ref as NR
import path_scenes as PS
from helpers import assert_bitexact, flat_from_export, oracle_cfg

F = np.float32
W, H, BOUNCES = 16, 12, 4
BATCHES, PER_BATCH = 8, 32
_FIX = {}


def fixture(P):
    if not _FIX:
        spec = GS.fixture_spec()
        scene = GS.gpu_scene(P, spec)
        scene.build()
        _FIX["f"] = (flat_from_export(scene.export()), spec)
    return _FIX["f"]


def ref_kw(spec):
    return dict(smooth=spec["smooth"], uv=GS.vertex_uv(spec), textures=spec["textures"], binding=spec["binding"], ior=spec["ior"])


def same_render(got, want, what):
    assert_bitexact(got.S, want.S, f"{what}: image")
    assert_bitexact(got.Q, want.Q, f"{what}: moments")
    assert got.segments == want.segments and got.live == want.live, what
    assert (got.counts == want.counts).all(), what


def without_lights(flat):
    out = copy.copy(flat)
    ints = np.array(flat.model_ints, copy=True)
    ints[ints[:, 2] == DR.EMISSIVE, 2] = DR.DIFFUSE
    out.model_ints = ints
    return out


@pytest.mark.parametrize("case", ["switch off", "no EMISSIVE model"])
def test_is_the_parent_restatement(pt_mod, oracle_mod, case):
    P = pt_mod
    flat, spec = fixture(P)
    if case == "no EMISSIVE model":
        flat = without_lights(flat)
    cfg = P.RenderConfig(width=37, height=23, max_bounces=BOUNCES, accel=P.ACCEL_BVH)
    want = GR.Restatement(flat, oracle_cfg(cfg, threads=4), **ref_kw(spec))
    got = DR.Restatement(flat, oracle_cfg(cfg, threads=4), direct=case != "switch off", **ref_kw(spec))
    mask = np.zeros(want.counts.shape, bool)
    mask[0, :2] = True
    for r in (want, got):
        r.render(0, 2)
        r.render(2, 1, mask)
    assert want.S.any() and got.sampled == 0 and got.active() is False
    assert (len(got.lights["cdf"]) == 0) == (case == "no EMISSIVE model")
    same_render(got, want, case)


def test_a_pixel_without_direct_light_keeps_its_bits():
    t = np.array([[0.5, 0.25, 0.0], [0.3, 0.3, 0.3], [0.7, 0.1, 0.2]], F)
    D = np.array([[0.0, 0.0, 0.0], [0.0, 0.5, 0.0], [0.25, 0.0, 0.0]], F)
    out = DR.combine(t, D, np.array([False, False, True]))
    assert_bitexact(out[0], t[0], "no direct light")
    assert out[1].tolist() == [t[1, 0], np.sqrt(F(t[1, 1] * t[1, 1]) + F(0.5), dtype=F), t[1, 2]]
    assert out[2].tolist() == [0.5, 0.0, 0.0]                   # suppressed: only the direct light counts


def test_same_expectation_and_lower_noise(pt_mod, oracle_mod):
    P = pt_mod
    flat, spec = fixture(P)
    cfg = P.RenderConfig(width=W, height=H, max_bounces=BOUNCES, accel=P.ACCEL_BVH)
    means, noise, refs = {}, {}, {}
    for direct in (False, True):
        r = DR.Restatement(flat, oracle_cfg(cfg, threads=4), direct=direct, **ref_kw(spec))
        per_batch = []
        for b in range(BATCHES):
            r.clear()
            r.render(1000 * b, PER_BATCH)                       # disjoint ids
            per_batch.append((r.Q.astype(np.float64) / PER_BATCH).reshape(H, W, 3))     # the linear mean
        means[direct] = np.array(per_batch)
        est = NR.noise(r.S, r.Q, W, H, PER_BATCH)
        noise[direct] = float(est["mean"])
        refs[direct] = r
    lit = refs[True]
    assert lit.sampled > 50_000 and lit.shadow_occluded > 10_000 and lit.shadow_rays - lit.shadow_occluded > 10_000
    assert lit.suppressed_hits > 1000 and refs[False].sampled == 0
    worst = 0.0
    for qy in (0, 1):
        for qx in (0, 1):
            sl = (slice(None), slice(qy * H // 2, (qy + 1) * H // 2), slice(qx * W // 2, (qx + 1) * W // 2))
            a, b = means[False][sl].sum(axis=(1, 2, 3)), means[True][sl].sum(axis=(1, 2, 3))
            se = np.sqrt(a.var(ddof=1) / BATCHES + b.var(ddof=1) / BATCHES)
            z = (a.mean() - b.mean()) / se
            print(f"quadrant ({qy}, {qx}): plain {a.mean():.4f}, direct {b.mean():.4f}, {z:+.2f} standard errors")
            worst = max(worst, abs(z))
            assert abs(z) <= 4.0
    print(f"frame-mean noise estimate at {PER_BATCH} samples: direct {noise[True]:.6g}, plain {noise[False]:.6g}, "
          f"ratio {noise[True] / noise[False]:.3f}")
    assert noise[True] < noise[False]
