"""The dielectric material's host functions (include/pathtracer_amd.h, "Dielectric material":
material 7, pt_scene_set_model_ior, pt_scene_model_ior, the grammar's DIELECTRIC block and ior:
attribute, the Python mirror and the demo scene): no compute calls, runs without a GPU."""
import ctypes
import os

import numpy as np
import pytest

import glass_scenes as GS
from conftest import ROOT

F = np.float32


def small_scene(P, build=False):
    spec = GS.as_diffuse(GS.fixture_spec())
    s = P.Scene()
    ids = [s.addMesh(*m) for m in spec["meshes"]]
    for m in spec["models"]:
        s.addModel(ids[m["mesh"]], m["scale"], m["rot"], m["translate"], m["material"], m["color"])
    if build:
        s.build()
    return s, len(spec["models"])


def test_material_seven_is_accepted_and_nine_still_refused(pt_mod):
    P = pt_mod
    L = P.lib()
    assert P.MATERIALS["DIELECTRIC"] == 7
    s, n = small_scene(P)
    one = (ctypes.c_float * 3)(1, 1, 1)
    zero = (ctypes.c_float * 3)(0, 0, 0)
    assert L.pt_scene_add_model(s._h, 2, one, zero, zero, 7, one) == n
    assert s.addModel(2, (1, 1, 1), (0, 0, 0), (0, 0, 0), "DIELECTRIC", (1, 1, 1)) == n + 1
    assert s.addModel(2, (1, 1, 1), (0, 0, 0), (0, 0, 0), 7, (1, 1, 1)) == n + 2
    for bad in (8, 9, -1):
        assert L.pt_scene_add_model(s._h, 2, one, zero, zero, bad, one) < 0
        assert b"addModel: bad material" in L.pt_last_error()
    s.build()
    assert s.export()["model_ints"][n:, 2].tolist() == [7, 7, 7]
    assert s.export()["model_ints"][:n, 2].max() < 7


def test_ior_default_set_get_and_refusals(pt_mod):
    P = pt_mod
    L = P.lib()
    s, n = small_scene(P)
    assert [L.pt_scene_model_ior(s._h, i) for i in range(n)] == [1.5] * n                 # the default
    assert L.pt_scene_set_model_ior(s._h, 3, 1.33) == 0                                   # a diffuse model: stored
    assert F(L.pt_scene_model_ior(s._h, 3)) == F(1.33)
    assert [L.pt_scene_model_ior(s._h, i) for i in range(n) if i != 3] == [1.5] * (n - 1)
    assert L.pt_scene_set_model_ior(s._h, -1, 2.4) == 0                                   # every model added so far
    assert [F(L.pt_scene_model_ior(s._h, i)) for i in range(n)] == [F(2.4)] * n
    late = s.addModel(2, (1, 1, 1), (0, 0, 0), (0, 0, 0), "DIELECTRIC", (1, 1, 1))
    assert L.pt_scene_model_ior(s._h, late) == 1.5                                        # added afterwards: the default
    for edge in (1.0, 4.0):
        assert L.pt_scene_set_model_ior(s._h, 0, edge) == 0 and L.pt_scene_model_ior(s._h, 0) == edge
    for bad in (n + 1, n + 7, -2, -100):
        assert L.pt_scene_set_model_ior(s._h, bad, 1.5) < 0
        assert b"setModelIor: bad model index" in L.pt_last_error()
    for bad in (0.999, 4.001, 0.0, -1.5, float("nan"), float("inf"), -float("inf")):
        for model in (1, -1):
            assert L.pt_scene_set_model_ior(s._h, model, bad) < 0
            assert b"setModelIor: ior must be finite and in [1, 4]" in L.pt_last_error()
    assert F(L.pt_scene_model_ior(s._h, 1)) == F(2.4)                                     # a refused call changes nothing
    for bad in (n + 1, -1, -2):
        assert L.pt_scene_model_ior(s._h, bad) < 0
        assert b"pt_scene_model_ior: bad model index" in L.pt_last_error()
    assert L.pt_scene_set_model_ior(None, 0, 1.5) < 0 and b"null scene" in L.pt_last_error()
    assert L.pt_scene_model_ior(None, 0) < 0 and b"null scene" in L.pt_last_error()
    empty = P.Scene()
    assert L.pt_scene_set_model_ior(empty._h, -1, 2.0) == 0                               # all of no models
    assert L.pt_scene_set_model_ior(empty._h, 0, 2.0) < 0


def test_abi_is_unchanged(pt_mod):
    assert pt_mod.lib().pt_abi_version() == 9
    assert ctypes.sizeof(pt_mod._Cfg) == 120


def test_python_mirror(pt_mod):
    P = pt_mod
    s, n = small_scene(P)
    assert s.ior(0) == 1.5
    s.set_ior(2, 1.33)
    assert F(s.ior(2)) == F(1.33) and s.ior(3) == 1.5
    s.set_ior(None, 2.0)
    assert [s.ior(i) for i in range(n)] == [2.0] * n
    s.set_ior()                                                                          # None, 1.5
    assert [s.ior(i) for i in range(n)] == [1.5] * n
    a = s.addModel(2, (0.03, 0.03, 0.03), (0, 0, 0), (0, 500, 0), "DIELECTRIC", (0.9, 0.9, 0.9), ior=2.4)
    b = s.addModel(2, (0.03, 0.03, 0.03), (0, 0, 0), (0, 600, 0), "DIELECTRIC", (0.9, 0.9, 0.9))
    assert F(s.ior(a)) == F(2.4) and s.ior(b) == 1.5
    with pytest.raises(P.PathTracerError, match="bad model index"):
        s.set_ior(n + 5, 1.5)
    with pytest.raises(P.PathTracerError, match="bad model index"):
        s.ior(n + 5)
    with pytest.raises(P.PathTracerError, match=r"ior must be finite and in \[1, 4\]"):
        s.set_ior(0, 0.5)


def test_ior_survives_build_and_leaves_the_build_alone(pt_mod):
    P = pt_mod
    plain, n = small_scene(P, build=True)
    before, _ = small_scene(P)
    before.set_ior(3, 1.33)
    before.build()
    after, _ = small_scene(P, build=True)
    after.set_ior(3, 1.33)
    after.build()
    want, want_bvh = plain.export(), plain.export_bvh4()
    for s in (before, after):
        assert F(s.ior(3)) == F(1.33) and s.ior(2) == 1.5
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

DIELECTRIC
glass
[0.9, 0.95, 0.9]

SPHERE
ball
0.05
[0, 0, 0]
translate:[0,100,0]
shading:smooth
material:glass
ior:1.33

BOX
block
[0.1, 0.1, 0.1]
[-0.1, -0.1, -0.1]
translate:[-150,100,0]
material:glass

BOX
floor
[1, 0, 1]
[-1, -0.1, -1]
ior:2.5
material:grey
%s
"""

MESH_BLOCK = """
MESH
tri
%s
ior:%s
scale:[0.1,0.1,0.1]
material:glass
"""


def write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_grammar(pt_mod, tmp_path):
    P = pt_mod
    obj = write(tmp_path, "tri.obj", "v -1 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//1 3//1\n")
    s = P.Scene(write(tmp_path, "scene.txt", SCENE_TEXT % (MESH_BLOCK % (obj, "4") + MESH_BLOCK % (obj, "1.0"))))
    assert [F(s.ior(i)) for i in range(5)] == [F(1.33), F(1.5), F(2.5), F(4), F(1)]
    s.build()
    assert s.export()["model_ints"][:, 2].tolist() == [7, 7, 0, 7, 7]
    assert [F(s.ior(i)) for i in range(5)] == [F(1.33), F(1.5), F(2.5), F(4), F(1)]
    for bad in ("0.99", "4.5", "", "glass", "[1,2,3]", "1.5x", "nan", "inf", "-2"):
        with pytest.raises(P.PathTracerError, match="bad attribute ior:" + bad.replace("[", r"\[").replace("]", r"\]")):
            P.Scene(write(tmp_path, "bad.txt", SCENE_TEXT % (MESH_BLOCK % (obj, bad))))


def test_the_demo_scene_loads(pt_mod):
    P = pt_mod
    s = P.Scene(os.path.join(ROOT, "scenes", "glass_room.txt"))
    s.build()
    mats = s.export()["model_ints"][:, 2]
    glass = np.nonzero(mats == 7)[0]
    assert len(glass) == 2                                                # the block and the ball
    assert sorted(F(s.ior(int(i))) for i in glass) == [F(1.33), F(1.5)]
    assert s.smooth()[glass].tolist().count(True) == 1                    # the ball
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "scenes/glass_room.txt" in text
