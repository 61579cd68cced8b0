"""pt_renderer_set_pixel_jitter / pt_renderer_pixel_jitter as host state: the setting
reads back, and the refusals are reported before anything is launched (no compute calls:
runs without a GPU)."""
import inspect

import pytest


def test_setting_and_refusals(pt_mod):
    P = pt_mod
    cfg = dict(width=64, height=48)
    r = P.Renderer(P.RenderConfig(**cfg))
    assert r.pixel_jitter() == (False, 1.0)              # off by default
    r.set_pixel_jitter()
    assert r.pixel_jitter() == (True, 1.0)
    r.set_pixel_jitter(0.25, on=False)
    assert r.pixel_jitter() == (False, 0.25)
    r.set_pixel_jitter(0.0)
    assert r.pixel_jitter() == (True, 0.0)
    for bad in (float("nan"), float("inf"), -1.0):
        with pytest.raises(P.PathTracerError, match="width must be finite"):
            r.set_pixel_jitter(bad)
    assert r.pixel_jitter() == (True, 0.0)               # a refused call changes nothing
    r.free()
    L = P.lib()
    assert L.pt_renderer_set_pixel_jitter(None, 1, 1.0) == -1 and b"null renderer" in L.pt_last_error()
    assert L.pt_renderer_pixel_jitter(None, None, None) == -1 and b"null renderer" in L.pt_last_error()
    r = P.Renderer(P.RenderConfig(max_bounces=510, **cfg))      # depths 511 and 512: one past the field
    with pytest.raises(P.PathTracerError, match="511"):
        r.set_pixel_jitter(1.0)
    assert r.pixel_jitter() == (False, 1.0)
    r.set_pixel_jitter(1.0, on=False)                    # off needs no depth
    r.free()
    r = P.Renderer(P.RenderConfig(max_bounces=509, **cfg))      # depths 510 and 511
    r.set_pixel_jitter(1.0)
    assert r.pixel_jitter() == (True, 1.0)
    r.free()


def test_render_sharded_takes_a_jitter_width_and_defaults_to_none():
    from pathtracerap_amd.dist import render_sharded
    p = inspect.signature(render_sharded).parameters
    assert p["jitter"].default is None
    assert list(p)[:6] == ["scene", "cfg", "total_iters", "device", "render_fn", "moments"]    # today's calls as they are
