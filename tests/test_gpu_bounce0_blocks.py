"""The bounce-0 kernels at every block size (RenderConfig.block 64, 128, 256).

The kernels that start an iteration -- k_bounce<true>, k_bounce_masked, k_gen_jitter and
k_gen_camera -- share one block-stable compaction, one ray store and one tile test.  At
block 64 a block is one wave; at 128 and 256 the waves of a block exchange their counts
through LDS, a path the masked kernels take at no other place in the suite.  The block size
must not change a bit of the result: for block 128 and 256 the image, the moments, the
sample counts, the segment count and the segments per bounce equal those of the same
sequence at block 64, which tests/test_gpu_adaptive.py, test_gpu_jitter.py and
test_gpu_camera.py tie to the CPU restatements.

The frame is 72 x 40: 2,880 pixels are 45 blocks of 64, 22.5 of 128 and 11.25 of 256 (a
partial last block at both larger sizes); a row is 4.5 tiles (a partial tile column); blocks
of 128 and 256 span rows, so one block holds pixels of active and of inactive tiles."""
import numpy as np
import pytest

import adaptive_ref as AR
from conftest import REF_SCENE
from helpers import assert_bitexact
from test_gpu_camera import LENS, view
from test_gpu_jitter import half_mask, one_tile

pytestmark = pytest.mark.gpu

W, H, BOUNCES, PIPES, ITERS = 72, 40, 5, 3, 3
MASKS = {"half": lambda: half_mask(W, H, seed=26), "one_tile": lambda: one_tile(W, H, 7)}
MODES = ("cached", "jitter", "camera")


@pytest.fixture(scope="module")
def scene(pt_mod):
    s = pt_mod.Scene(REF_SCENE)
    s.build()
    return s


def block_census(mask, block):
    """Per block of `block` consecutive pixel indices: (pixels inside the frame, of which active)."""
    on = np.asarray(mask, bool).reshape(-1)[AR.pixel_tiles(W, H)]
    assert on.shape == (W * H,)
    return [(len(on[j0:j0 + block]), int(on[j0:j0 + block].sum())) for j0 in range(0, W * H, block)]


@pytest.mark.parametrize("mask_name", sorted(MASKS))
def test_the_masks_meet_every_block_kind(mask_name):
    """From the mask alone, before anything renders: at block 256 some block mixes active and
    inactive pixels, some block is wholly inactive, and the last block is partial."""
    mask = MASKS[mask_name]()
    assert mask.shape == AR.tiles_shape(W, H) == (3, 5)
    census = block_census(mask, 256)
    assert len(census) == 12
    assert any(0 < on < size for size, on in census), census
    assert any(on == 0 for size, on in census), census
    assert census[-1][0] == W * H - 11 * 256 == 64
    assert all(size == 256 for size, _ in census[:-1])
    assert block_census(mask, 128)[-1][0] == 64             # partial at 128 too


def run_sequence(P, scene, mode, mask, block):
    """One plain call and one masked call of 3 iterations each; the state after both."""
    cfg = P.RenderConfig(width=W, height=H, max_bounces=BOUNCES, iterations=2 * ITERS, accel=P.ACCEL_GRID_FAST,
                         pipelines=PIPES, block=block)
    r = P.Renderer(cfg)
    r.enable_moments()
    if mode == "camera":
        r.set_camera(view(P, "A", cfg, LENS))                # a lens: k_gen_camera
    if mode != "cached":
        r.set_pixel_jitter(1.0)                              # legacy camera: k_gen_jitter
    r.allocateOnGPU(scene)
    r.renderLoop(0, ITERS)                                   # unmasked: <BS, false> / k_bounce<true>
    plain = r.image()
    r.render_masked(mask, ITERS, ITERS)                      # masked: <BS, true> / k_bounce_masked
    out = (r.image(), r.moments(), r.sample_counts(), r.segments(), r.segments_per_bounce(10), plain)
    r.free()
    return out


STATE = ("image", "moments", "sample counts", "segments", "segments per bounce", "image after the plain call")
_BLOCK64 = {}


def block64(P, scene, mode, mask_name):
    """The sequence at block 64 (shared; never modified)."""
    key = (mode, mask_name)
    if key not in _BLOCK64:
        _BLOCK64[key] = run_sequence(P, scene, mode, MASKS[mask_name](), 64)
    return _BLOCK64[key]


@pytest.mark.parametrize("mask_name", sorted(MASKS))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("block", [128, 256])
def test_block_size_changes_no_bit(gpu, pt_mod, scene, block, mode, mask_name):
    P = pt_mod
    mask = MASKS[mask_name]()
    want = block64(P, scene, mode, mask_name)
    got = run_sequence(P, scene, mode, mask, block)
    what = f"block {block} {mode} {mask_name}"
    assert want[0].any() and want[3] > 0
    off = ~np.asarray(mask, bool).reshape(-1)[AR.pixel_tiles(W, H)]
    assert_bitexact(want[0][off], want[5][off], f"{what}: block 64, inactive tiles across the masked call")
    assert not np.array_equal(want[0][~off], want[5][~off])  # the masked call sampled the active tiles
    for g, w, name in zip(got, want, STATE):
        if isinstance(w, np.ndarray):
            assert_bitexact(g, w, f"{what}: {name}")
        else:
            assert g == w, (what, name, g, w)
