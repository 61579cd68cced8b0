"""The smooth-shading flag's host functions (include/pathtracer_amd.h: pt_scene_set_model_smooth,
pt_scene_model_smooth, the scene grammar's shading: attribute and the Python mirror): no compute
calls, runs without a GPU."""
import ctypes

import numpy as np
import pytest

import smooth_scenes as SS


def small_scene(P, build=False):
    meshes, models, _ = SS.fixture_spec(320)
    s = P.Scene()
    ids = [s.addMesh(*m) for m in meshes]
    for m in models:
        s.addModel(ids[m["mesh"]], m["scale"], m["rot"], m["translate"], m["material"], m["color"])
    if build:
        s.build()
    return s, len(models)


def test_c_getters_and_setters(pt_mod):
    P = pt_mod
    L = P.lib()
    s, n = small_scene(P)
    assert [L.pt_scene_model_smooth(s._h, i) for i in range(n)] == [0] * n          # off by default
    assert L.pt_scene_set_model_smooth(s._h, 3, 1) == 0
    assert [L.pt_scene_model_smooth(s._h, i) for i in range(n)] == [0, 0, 0, 1] + [0] * (n - 4)
    assert L.pt_scene_set_model_smooth(s._h, 3, 7) == 0                               # any non-zero value is on
    assert L.pt_scene_model_smooth(s._h, 3) == 1
    assert L.pt_scene_set_model_smooth(s._h, -1, 1) == 0                              # every model added so far
    assert [L.pt_scene_model_smooth(s._h, i) for i in range(n)] == [1] * n
    late = s.addModel(0, (1, 1, 1), (0, 0, 0), (0, 0, 0), "DIFFUSE", (1, 1, 1))
    assert L.pt_scene_model_smooth(s._h, late) == 0                                   # added afterwards: off
    assert L.pt_scene_set_model_smooth(s._h, 2, 0) == 0
    assert L.pt_scene_set_model_smooth(s._h, -1, 0) == 0
    assert [L.pt_scene_model_smooth(s._h, i) for i in range(n + 1)] == [0] * (n + 1)


def test_bad_indices_are_refused_with_a_message(pt_mod):
    P = pt_mod
    L = P.lib()
    s, n = small_scene(P)
    for bad in (n, n + 5, -2, -100):
        assert L.pt_scene_set_model_smooth(s._h, bad, 1) < 0
        assert b"setModelSmooth: bad model index" in L.pt_last_error()
    for bad in (n, -1, -2):
        assert L.pt_scene_model_smooth(s._h, bad) < 0
        assert b"pt_scene_model_smooth: bad model index" in L.pt_last_error()
    assert L.pt_scene_set_model_smooth(None, 0, 1) < 0 and b"null scene" in L.pt_last_error()
    assert L.pt_scene_model_smooth(None, 0) < 0 and b"null scene" in L.pt_last_error()
    assert not s.smooth().any()                                                       # a refused call changes nothing
    empty = P.Scene()
    assert L.pt_scene_set_model_smooth(empty._h, -1, 1) == 0                          # all of no models
    assert L.pt_scene_set_model_smooth(empty._h, 0, 1) < 0


def test_abi_is_unchanged(pt_mod):
    assert pt_mod.lib().pt_abi_version() == 9
    assert ctypes.sizeof(pt_mod._Cfg) == 120


def test_python_mirror(pt_mod):
    P = pt_mod
    s, n = small_scene(P)
    assert s.smooth().dtype == bool and s.smooth().tolist() == [False] * n
    s.set_smooth(2)
    s.set_smooth(4, True)
    assert s.smooth().tolist() == [i in (2, 4) for i in range(n)]
    s.set_smooth(2, on=False)
    assert s.smooth().tolist() == [i == 4 for i in range(n)]
    s.set_smooth()                                                                    # None: every model
    assert s.smooth().all()
    s.set_smooth(None, False)
    assert not s.smooth().any()
    a = s.addModel(2, (0.03, 0.03, 0.03), (0, 0, 0), (0, 500, 0), "METAL", (0.9, 0.9, 0.9), smooth=True)
    b = s.addModel(2, (0.03, 0.03, 0.03), (0, 0, 0), (0, 600, 0), "METAL", (0.9, 0.9, 0.9))
    assert s.smooth()[a] and not s.smooth()[b]
    with pytest.raises(P.PathTracerError, match="bad model index"):
        s.set_smooth(n + 2)


def test_flags_survive_build_and_leave_the_build_alone(pt_mod):
    """The flag is not part of the grid or the BLAS: building with it set, or setting it after the
    build, gives the export and the BVH of a scene that never had it."""
    P = pt_mod
    plain, n = small_scene(P, build=True)
    before, _ = small_scene(P)
    before.set_smooth(3)
    before.set_smooth(5)
    before.build()
    assert before.smooth().tolist() == [i in (3, 5) for i in range(n)]
    after, _ = small_scene(P, build=True)
    after.set_smooth(3)
    after.set_smooth(5)
    assert after.smooth().tolist() == before.smooth().tolist()
    after.build()                                                                     # a rebuild keeps them too
    assert after.smooth().tolist() == before.smooth().tolist()
    want, want_bvh = plain.export(), plain.export_bvh4()
    for s in (before, after):
        assert s.counts() == plain.counts()
        got, got_bvh = s.export(), s.export_bvh4()
        for k in want:
            assert np.array_equal(got[k].view(np.uint32) if got[k].dtype == np.float32 else got[k],
                                  want[k].view(np.uint32) if want[k].dtype == np.float32 else want[k]), k
        for k in want_bvh:
            assert np.array_equal(got_bvh[k].view(np.uint32), want_bvh[k].view(np.uint32)), k


SCENE_TEXT = """
DIFFUSE
grey
[0.8, 0.8, 0.8]

METAL
chrome
[0.9, 0.9, 0.95]

SPHERE
ball
0.05
[0, 0, 0]
translate:[0,100,0]
shading:smooth
material:chrome

SPHERE
facets
0.05
[0, 0, 0]
translate:[150,100,0]
material:chrome
shading:flat

BOX
crate
[0.1, 0.1, 0.1]
[-0.1, -0.1, -0.1]
shading:smooth
translate:[-150,100,0]
material:grey

BOX
floor
[1, 0, 1]
[-1, -0.1, -1]
material:grey
%s
"""

MESH_BLOCK = """
MESH
tri
%s
shading:%s
scale:[0.1,0.1,0.1]
material:grey
"""


def write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_grammar(pt_mod, tmp_path):
    P = pt_mod
    obj = write(tmp_path, "tri.obj", "v -1 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//1 3//1\n")
    s = P.Scene(write(tmp_path, "scene.txt", SCENE_TEXT % (MESH_BLOCK % (obj, "smooth") + MESH_BLOCK % (obj, "flat"))))
    # SPHERE smooth, SPHERE flat, BOX smooth, BOX with the default, MESH smooth, MESH flat
    assert s.smooth().tolist() == [True, False, True, False, True, False]
    default = P.Scene(write(tmp_path, "default.txt", SCENE_TEXT % ""))
    assert default.smooth().tolist() == [True, False, True, False]
    for bad in ("phong", "", "Smooth", "[1,2,3]"):
        with pytest.raises(P.PathTracerError, match="bad attribute shading:" + bad.replace("[", r"\[").replace("]", r"\]")):
            P.Scene(write(tmp_path, "bad.txt", SCENE_TEXT % (MESH_BLOCK % (obj, bad))))
    s.build()
    assert s.smooth().tolist() == [True, False, True, False, True, False]
