"""The yardstick of the tile-masked tests, held to the oracle (CPU only): the
restatement in adaptive_ref.py with every tile active is the oracle's render loop,
and its per-tile estimate with uniform counts is noise_ref's."""
import numpy as np
import pytest

import adaptive_ref as AR
import noise_ref as NR
from conftest import INPUT_DATA
from helpers import assert_bitexact


@pytest.fixture(scope="module")
def flat(oracle_mod):
    return oracle_mod.reference_scene(INPUT_DATA)


def oracle_iterations(O, flat, cfg, iters):
    out, seg = [], 0
    for it in range(iters):
        c = O.RenderConfig(**{**cfg.__dict__, "first_iter": it, "iterations": 1})
        img, s = O.render(flat, c)
        out.append(img)
        seg += s
    return out, seg


@pytest.mark.parametrize("w,h,accel,tail_drop", [(64, 48, 0, 0), (64, 48, 1, 0), (37, 23, 0, 1)])
def test_all_ones_mask_is_the_oracle_render(oracle_mod, flat, w, h, accel, tail_drop):
    O = oracle_mod
    cfg = O.RenderConfig(width=w, height=h, max_bounces=5, accel=accel, tail_drop=tail_drop, threads=4)
    cs, seg = oracle_iterations(O, flat, cfg, 3)
    S, Q = NR.moment_sums(cs)
    r = AR.Restatement(flat, cfg)
    r.render(0, 2, np.ones(AR.tiles_shape(w, h), np.uint8))
    r.render(2, 1)                                           # None: every tile
    assert_bitexact(r.S, S, "restatement: image")
    assert_bitexact(r.Q, Q, "restatement: moments")
    assert r.segments == seg
    assert (r.counts == 3).all()
    whole, _ = O.render(flat, O.RenderConfig(**{**cfg.__dict__, "iterations": 3}))
    assert_bitexact(r.S, whole, "restatement: the oracle's three iterations in one call")
    if tail_drop:
        assert not r.S[(w * h // 32) * 32:].any()


def test_uniform_counts_give_noise_ref(oracle_mod, flat):
    O = oracle_mod
    w, h = 37, 23
    cfg = O.RenderConfig(width=w, height=h, max_bounces=5, threads=4)
    cs, _ = oracle_iterations(O, flat, cfg, 4)
    S, Q = NR.moment_sums(cs)
    counts = np.full(AR.tiles_shape(w, h), 4, np.int32)
    got, want = AR.tile_noise(S, Q, w, h, counts), NR.noise(S, Q, w, h, 4)
    assert_bitexact(got["err"], want["err"], "per-pixel error")
    assert_bitexact(got["tiles"], want["tiles"], "tile map")
    assert got["mean"] == want["mean"] and got["max_tile"] == want["max_tile"]
    assert_bitexact(AR.tile_mean(S, w, h, counts), S / np.float32(4), "mean")
    assert (AR.tile_pixels(w, h) == want["counts"]).all()
    # a tile below 2 samples: inf in the map, nothing in the mean's sum
    counts[0, 1] = 1
    low = AR.tile_noise(S, Q, w, h, counts)
    assert np.isinf(low["tiles"][0, 1]) and np.isfinite(np.delete(low["tiles"].reshape(-1), 1)).all()
    assert low["mean"] < want["mean"]
