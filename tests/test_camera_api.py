"""The free camera's host functions (include/pathtracer_amd.h: pt_camera_look_at,
pt_renderer_set_camera / pt_renderer_camera before allocation, pt_scene_camera and the RENDER
block's camera_* keys): no compute calls, runs without a GPU."""
import inspect

import numpy as np
import pytest

import camera_ref as CR
from conftest import REF_SCENE
from helpers import assert_bitexact

EPS = 2.0 ** -23          # ulp(v) <= EPS * |v| for a normal float32 v; one rounding errs by at most half of it

VIEWS = [dict(eye=(0, 800, 500), target=(0, 0, 0), vfov_deg=45, focus_dist=900, width=64, height=48),
         dict(eye=(650, 200, 650), target=(0, 0, 0), vfov_deg=45, focus_dist=None, width=37, height=23),
         dict(eye=(-3, 2, 920), target=(10, -40, 0), up=(0.2, 1, 0.1), vfov_deg=100, focus_dist=55, lens_radius=2.5,
              width=1280, height=1024)]


def vec(c, name):
    return np.array(getattr(c, name), np.float64)


@pytest.mark.parametrize("view", VIEWS, ids=["A", "B", "tilted"])
def test_look_at(pt_mod, view):
    """Every field is a double value rounded once: it errs by at most EPS/2 of its own magnitude,
    which is at most M = the largest coordinate of the frame's corners, the eye or 1.  The bounds
    below count those roundings (and a few more, to stay clear of counting errors)."""
    P = pt_mod
    c = P.look_at(**view)
    W, H = view["width"], view["height"]
    eye, target = np.array(view["eye"], np.float64), np.array(view["target"], np.float64)
    focus = view["focus_dist"] if view["focus_dist"] is not None else np.linalg.norm(target - eye)
    f = (target - eye) / np.linalg.norm(target - eye)
    origin, p0, du, dv, lu, lv = (vec(c, n) for n in CR.VECS)
    corners = [p0, p0 + W * du, p0 + H * dv, p0 + W * du + H * dv]
    M = max(1.0, np.abs(eye).max(), max(np.abs(k).max() for k in corners))
    assert_bitexact(np.array(c.origin, np.float32), eye.astype(np.float32), "origin = eye, rounded")
    assert c.lens_radius == np.float32(view.get("lens_radius", 0.0))
    # the centre of the frame lies on the eye -> target line at focus_dist: p0 (EPS/2 M per
    # coordinate) + W/2 du + H/2 dv (each EPS/2 of a length <= 2M)
    centre = p0 + 0.5 * W * du + 0.5 * H * dv
    assert np.abs(centre - (eye + f * focus)).max() <= 4 * EPS * M
    # du, dv and the view are mutually perpendicular: the dot of two vectors, each with a
    # per-coordinate error of EPS/2 of its length, errs by at most sqrt(3) EPS |a| |b|
    for a, b in ((du, dv), (du, f), (dv, f), (lu, lv), (lu, f), (lv, f)):
        assert abs(a @ b) <= 2 * EPS * np.linalg.norm(a) * np.linalg.norm(b)
    # square pixels: |du| W / (|dv| H) = W / H, each length within sqrt(3)/2 EPS relative
    nu, nv = np.linalg.norm(du), np.linalg.norm(dv)
    assert abs(nu / nv - 1.0) <= 2 * EPS
    # the vertical extent is the field of view at focus_dist
    assert abs(nv * H - 2 * focus * np.tan(np.radians(view["vfov_deg"]) / 2)) <= 2 * EPS * nv * H
    # the lens spans the image plane's axes with unit vectors; y grows along +up
    assert abs(np.linalg.norm(lu) - 1) <= 2 * EPS and abs(np.linalg.norm(lv) - 1) <= 2 * EPS
    assert np.abs(du / nu - lu).max() <= 2 * EPS and np.abs(dv / nv - lv).max() <= 2 * EPS
    assert dv @ np.array(view.get("up", (0, 1, 0)), np.float64) > 0
    # right-handed: du x dv points back at the viewer, as the legacy camera's +x, +y and -z view
    assert np.cross(du, dv) @ f < 0


def test_look_at_refusals(pt_mod):
    P = pt_mod
    ok = dict(eye=(0, 0, 10), target=(0, 0, 0), width=64, height=48)
    P.look_at(**ok)
    cases = [(dict(ok, target=(0, 0, 10)), "eye and target coincide"),
             (dict(ok, up=(0, 0, -3)), "up is parallel to the view"),
             (dict(ok, up=(0, 0, 0)), "up is parallel to the view"),
             (dict(ok, vfov_deg=0), r"vfov_deg must lie in \(0, 180\)"),
             (dict(ok, vfov_deg=180), r"vfov_deg must lie in \(0, 180\)"),
             (dict(ok, vfov_deg=-20), r"vfov_deg must lie in \(0, 180\)"),
             (dict(ok, focus_dist=0), "focus_dist must be > 0"),
             (dict(ok, focus_dist=-1), "focus_dist must be > 0"),
             (dict(ok, lens_radius=-0.5), "lens_radius must be >= 0"),
             (dict(ok, eye=(0, float("nan"), 10)), "must be finite"),
             (dict(ok, vfov_deg=float("inf")), "must be finite"),
             (dict(ok, width=0), "bad resolution")]
    for kw, msg in cases:
        with pytest.raises(P.PathTracerError, match=msg):
            P.look_at(**kw)
    L = P.lib()
    assert L.pt_camera_look_at(None, None, None, 45.0, 1.0, 0.0, 64, 48, None) == -1 and b"null argument" in L.pt_last_error()


def test_set_camera_round_trip_and_refusals(pt_mod):
    P = pt_mod
    cfg = P.RenderConfig(width=64, height=48)
    r = P.Renderer(cfg)
    on, legacy = r.camera()                                  # before allocation: host state
    assert on is False
    want = CR.legacy_camera(cfg)
    for n in CR.VECS:
        assert_bitexact(np.array(getattr(legacy, n), np.float32), getattr(want, n), f"legacy-equivalent {n}")
    assert legacy.lens_radius == 0.0
    cam = P.look_at((0, 800, 500), (0, 0, 0), focus_dist=900, lens_radius=25, width=64, height=48)
    r.set_camera(cam)
    assert r.camera() == (True, cam)
    bad = [(dict(origin=(0, float("nan"), 0)), "every field must be finite"),
           (dict(p0=(float("inf"), 0, 0)), "every field must be finite"),
           (dict(lens_v=(0, 0, float("-inf"))), "every field must be finite"),
           (dict(lens_radius=float("nan")), "every field must be finite"),
           (dict(du=(0, 0, 0)), "du and dv must not be zero"),
           (dict(dv=(0.0, -0.0, 0.0)), "du and dv must not be zero"),
           (dict(lens_radius=-1.0), "lens_radius must be >= 0")]
    for kw, msg in bad:
        with pytest.raises(P.PathTracerError, match=msg):
            r.set_camera(P.Camera(**kw))
        assert r.camera() == (True, cam)                     # a refused call changes nothing
    r.set_camera(None)
    assert r.camera() == (False, legacy)
    r.set_camera(legacy)                                     # the legacy-equivalent camera is a camera
    assert r.camera() == (True, legacy)
    r.free()
    L = P.lib()
    assert L.pt_renderer_set_camera(None, None) == -1 and b"null renderer" in L.pt_last_error()
    assert L.pt_renderer_camera(None, None) == -1 and b"null renderer" in L.pt_last_error()
    # the lens draws seed with depths max_bounces + 3 and + 4 of a 9-bit field
    r = P.Renderer(P.RenderConfig(width=64, height=48, max_bounces=508))      # depths 511 and 512: one past the field
    with pytest.raises(P.PathTracerError, match="511"):
        r.set_camera(cam)
    assert r.camera()[0] is False
    r.set_camera(P.Camera(**dict(cam.__dict__, lens_radius=0.0)))            # a pinhole needs no depth
    r.free()
    r = P.Renderer(P.RenderConfig(width=64, height=48, max_bounces=507))      # depths 510 and 511
    r.set_camera(cam)
    assert r.camera() == (True, cam)
    r.free()


SCENE_TAIL = """
DIFFUSE
m1
[0.98, 0.98, 0]

BOX
box1
[1,1,1]
[-1,-1,-1]
material:m1
"""


def test_render_block_camera_keys(pt_mod, tmp_path):
    P = pt_mod
    p = tmp_path / "cam.txt"
    p.write_text("RENDER\nresolution:[64,48]\ncamera_eye:[0,800,500]\ncamera_target:[0,0,0]\ncamera_up:[0,1,0]\n"
                 "camera_fov:45\ncamera_focus:900\ncamera_lens:25\n" + SCENE_TAIL)
    s = P.Scene(str(p))
    assert s.camera(64, 48) == P.look_at((0, 800, 500), (0, 0, 0), (0, 1, 0), 45, 900, 25, 64, 48)
    assert s.apply_settings(P.RenderConfig()).width == 64    # the other keys still parse
    p.write_text("RENDER\ncamera_target:[0,0,0]\ncamera_eye:[650,200,650]\n" + SCENE_TAIL)      # the defaults
    s = P.Scene(str(p))
    assert s.camera(37, 23) == P.look_at((650, 200, 650), (0, 0, 0), width=37, height=23)
    assert s.camera(37, 23).lens_radius == 0.0
    for block, msg in (("camera_eye:[0,0,1]\n", "camera_eye and camera_target"),
                       ("camera_fov:30\n", "camera_eye and camera_target"),
                       ("camera_eye:[0,0]\ncamera_target:[0,0,0]\n", "bad RENDER line"),
                       ("camera_eye:[0,0,1]\ncamera_target:[0,0,0]\ncamera_fov:wide\n", "bad RENDER line"),
                       ("camera_eye:[0,0,1]\ncamera_target:[0,0,0]\ncamera_focus:-2\n", "bad RENDER line"),
                       ("camera_eye:[0,0,1]\ncamera_target:[0,0,0]\ncamera_zoom:2\n", "bad RENDER line")):
        p.write_text("RENDER\n" + block + SCENE_TAIL)
        with pytest.raises(P.PathTracerError, match=msg):
            P.Scene(str(p))
    p.write_text("RENDER\ncamera_eye:[1,1,1]\ncamera_target:[1,1,1]\n" + SCENE_TAIL)             # parses; no view
    with pytest.raises(P.PathTracerError, match="eye and target coincide"):
        P.Scene(str(p)).camera(64, 48)
    # scene files without the keys report no camera
    assert P.Scene(REF_SCENE).camera(64, 48) is None
    p.write_text("RENDER\nresolution:[64,48]\n" + SCENE_TAIL)
    assert P.Scene(str(p)).camera(64, 48) is None
    assert P.Scene().camera(64, 48) is None
    L = P.lib()
    assert L.pt_scene_camera(None, 64, 48, None) == -1 and b"null argument" in L.pt_last_error()


def test_render_sharded_takes_a_camera_and_defaults_to_none():
    from pathtracerap_amd.dist import render_sharded
    p = inspect.signature(render_sharded).parameters
    assert p["camera"].default is None
    assert list(p)[:7] == ["scene", "cfg", "total_iters", "device", "render_fn", "moments", "jitter"]    # today's calls as they are

