"""The host side of albedo textures (include/pathtracer_amd.h: pt_scene_set_mesh_uv,
pt_scene_add_texture, pt_scene_set_model_texture and their getters, the OBJ loader's vt, the
generated primitives' uvs, the scene grammar's TEXTURE block and texture: attribute, and the
Python mirror): no compute calls, runs without a GPU."""
import ctypes

import numpy as np
import pytest

import texture_scenes as TS

F = np.float32


def small_scene(P, build=False):
    spec = TS.fixture_spec(320)
    s = P.Scene()
    ids = [s.addMesh(*m) for m in spec["meshes"]]
    for m in spec["models"]:
        s.addModel(ids[m["mesh"]], m["scale"], m["rot"], m["translate"], m["material"], m["color"])
    if build:
        s.build()
    return s, spec


def fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def err(P):
    return P.lib().pt_last_error().decode()


# ---- uv -------------------------------------------------------------------------------------------

def test_mesh_uv_setter_export_and_refusals(pt_mod):
    P = pt_mod
    L = P.lib()
    s, spec = small_scene(P, build=True)
    before = s.export()
    assert [L.pt_scene_mesh_has_uv(s._h, m) for m in range(3)] == [0, 0, 0]
    assert not before["uv"].any() and before["uv"].shape == (s.counts()["nv"], 2)
    uv = spec["mesh_uv"][TS.TORUS_MESH]
    assert L.pt_scene_set_mesh_uv(s._h, TS.TORUS_MESH, fp(uv), len(uv)) == 0
    assert [L.pt_scene_mesh_has_uv(s._h, m) for m in range(3)] == [0, 0, 1]
    after = s.export()
    first = int(after["mesh_ranges"][TS.TORUS_MESH, 0])
    assert np.array_equal(after["uv"][first:first + len(uv)], uv) and not after["uv"][:first].any()
    assert np.array_equal(after["uv"], TS.vertex_uv(spec))
    for k in before:                                     # built, the grid and the BLAS are left alone
        if k != "uv":
            assert np.array_equal(before[k], after[k]), k
    assert L.pt_scene_export_uv(s._h, None) == s.counts()["nv"]
    for mesh in (-1, 3, 99):
        assert L.pt_scene_set_mesh_uv(s._h, mesh, fp(uv), len(uv)) < 0 and "setMeshUv: bad mesh index" in err(P)
        assert L.pt_scene_mesh_has_uv(s._h, mesh) < 0 and "pt_scene_mesh_has_uv: bad mesh index" in err(P)
    for nv in (len(uv) - 1, len(uv) + 1, 0):
        assert L.pt_scene_set_mesh_uv(s._h, TS.TORUS_MESH, fp(uv), nv) < 0
        assert "setMeshUv: nv is not the mesh's vertex count" in err(P)
    for bad in (np.nan, np.inf, -np.inf):
        w = uv.copy()
        w[5, 1] = bad
        assert L.pt_scene_set_mesh_uv(s._h, TS.TORUS_MESH, fp(w), len(w)) < 0 and "setMeshUv: non-finite uv" in err(P)
    assert L.pt_scene_set_mesh_uv(s._h, TS.TORUS_MESH, None, len(uv)) < 0
    assert np.array_equal(s.export()["uv"], after["uv"])                  # a refused call changes nothing


# ---- textures and bindings ------------------------------------------------------------------------

def test_textures_bindings_and_refusals(pt_mod):
    P = pt_mod
    L = P.lib()
    s, spec = small_scene(P)
    n = len(spec["models"])
    assert s.textures() == [] and s.model_textures().tolist() == [-1] * n
    for t in spec["textures"]:
        s.add_texture(t)
    back = s.textures()
    assert len(back) == 6 and all(np.array_equal(a, b) and a.dtype == F for a, b in zip(back, spec["textures"]))
    assert [(t.shape[1], t.shape[0]) for t in back] == TS.TEXTURE_SIZES
    w, h = ctypes.c_int(), ctypes.c_int()
    assert L.pt_scene_texture(s._h, 4, ctypes.byref(w), ctypes.byref(h), None) == 0 and (w.value, h.value) == (5, 3)
    assert L.pt_scene_texture(s._h, 6, None, None, None) < 0 and "pt_scene_texture: bad texture index" in err(P)
    one = np.ones(3, F)
    for bw, bh in ((0, 1), (1, 0), (4097, 1), (1, 4097), (-1, 1)):
        assert L.pt_scene_add_texture(s._h, bw, bh, fp(one)) < 0
        assert "addTexture: width and height must be in [1,4096]" in err(P)
    for bad in (np.nan, np.inf):
        t = np.ones((2, 2, 3), F)
        t[1, 0, 2] = bad
        assert L.pt_scene_add_texture(s._h, 2, 2, fp(t)) < 0 and "addTexture: non-finite texel" in err(P)
    assert L.pt_scene_add_texture(s._h, 1, 1, None) < 0
    assert L.pt_scene_texture_count(s._h) == 6
    # a mesh without uv takes no texture
    assert L.pt_scene_set_model_texture(s._h, 2, 0) < 0 and "setModelTexture: mesh has no uv" in err(P)
    s.set_mesh_uv(TS.TORUS_MESH, spec["mesh_uv"][TS.TORUS_MESH])
    assert L.pt_scene_set_model_texture(s._h, 2, 5) == 0
    assert L.pt_scene_model_texture(s._h, 2) == 5 and s.model_textures().tolist() == [-1, -1, 5] + [-1] * (n - 3)
    assert L.pt_scene_set_model_texture(s._h, 0, 0) < 0 and "setModelTexture: mesh has no uv" in err(P)     # the room
    assert L.pt_scene_set_model_texture(s._h, -1, 0) < 0 and "setModelTexture: mesh has no uv" in err(P)    # all: the room too
    assert s.model_textures().tolist() == [-1, -1, 5] + [-1] * (n - 3)                                        # nothing changed
    assert L.pt_scene_set_model_texture(s._h, -1, -1) == 0 and s.model_textures().tolist() == [-1] * n        # -1 clears all
    for bad in (n, -2, 100):
        assert L.pt_scene_set_model_texture(s._h, bad, 0) < 0 and "setModelTexture: bad model index" in err(P)
        assert L.pt_scene_model_texture(s._h, bad if bad != -2 else -1) < -1
        assert "pt_scene_model_texture: bad model index" in err(P)
    for bad in (6, -2, 100):
        assert L.pt_scene_set_model_texture(s._h, 2, bad) < 0 and "setModelTexture: bad texture index" in err(P)
    assert L.pt_scene_set_model_texture(None, 0, 0) < 0 and "null scene" in err(P)
    assert L.pt_abi_version() == 9


def test_bindings_survive_build_and_may_follow_it(pt_mod):
    P = pt_mod
    spec = TS.fixture_spec(320)
    s = TS.gpu_scene(P, spec)                            # binds after build
    want = spec["binding"].tolist()
    assert s.model_textures().tolist() == want
    s.build()
    assert s.model_textures().tolist() == want and np.array_equal(s.export()["uv"], TS.vertex_uv(spec))
    s2, _ = small_scene(P)                               # binds before build
    s2.set_mesh_uv(TS.TORUS_MESH, spec["mesh_uv"][TS.TORUS_MESH])
    t = s2.add_texture(spec["textures"][3])
    s2.set_texture(None, None)
    s2.set_texture(4, t)
    late = s2.addModel(TS.TORUS_MESH, (1, 1, 1), (0, 0, 0), (0, 0, 0), "DIFFUSE", (1, 1, 1), texture=t)
    s2.build()
    assert s2.model_textures().tolist() == [-1, -1, -1, -1, 0, -1, -1, -1, 0] and late == 8
    with pytest.raises(P.PathTracerError, match="mesh has no uv"):
        s2.addModel(0, (1, 1, 1), (0, 0, 0), (0, 0, 0), "DIFFUSE", (1, 1, 1), texture=t)
    with pytest.raises(P.PathTracerError, match="shape"):
        s2.add_texture(np.ones((2, 2), F))


# ---- OBJ ------------------------------------------------------------------------------------------

OBJ_VT = """v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 0 0 1
vn 0 0 1
vn 0 1 0
vt 0.25 0.75
vt 1.5 -0.5
vt 0.1 0.2 0.9
f 1/1/1 2/2/1 3/3/1
f 1/-3 3/-1 4
f 1//2 2//2 5//2
f 1/2/2 2/1/2 5/3/2 4/1/2
"""


def strip_vt(text):
    out = []
    for line in text.splitlines():
        if line.startswith("vt "):
            continue
        if line.startswith("f "):
            toks = []
            for tok in line.split()[1:]:
                p = tok.split("/")
                toks.append(p[0] if len(p) < 3 or not p[2] else f"{p[0]}//{p[2]}")
            line = "f " + " ".join(toks)
        out.append(line)
    return "\n".join(out) + "\n"


def test_obj_vt_parsing_flip_and_geometry(pt_mod, tmp_path):
    P = pt_mod
    (tmp_path / "a.obj").write_text(OBJ_VT)
    (tmp_path / "b.obj").write_text(strip_vt(OBJ_VT))
    assert "vt" not in strip_vt(OBJ_VT) and "1//1" in strip_vt(OBJ_VT)
    sa, sb = P.Scene(), P.Scene()
    ma = sa.loadAndProcessMeshFile(str(tmp_path / "a.obj"))
    mb = sb.loadAndProcessMeshFile(str(tmp_path / "b.obj"))
    assert sa.mesh_has_uv(ma) and not sb.mesh_has_uv(mb)
    for s in (sa, sb):
        s.addModel(0, (1, 1, 1), (0, 0, 0), (0, 0, 0), "DIFFUSE", (1, 1, 1))
    a, b = sa.export(), sb.export()
    for k in ("vpos", "vnrm", "tris", "mesh_ranges", "mesh_bbox"):          # byte-identical geometry
        assert a[k].tobytes() == b[k].tobytes(), k
    assert not b["uv"].any()
    vt = [(F(0.25), F(1) - F(0.75)), (F(1.5), F(1) - F(-0.5)), (F(0.1), F(1) - F(0.2))]      # (u, 1 - v), float32
    z = (F(0), F(0))
    want = [vt[0], vt[1], vt[2],          # v/vt/vn
            vt[0], vt[2], z,              # v/vt with negative indices; a corner without vt
            z, z, z,                      # v//vn
            vt[1], vt[0], vt[2], vt[0]]   # a quad: one vertex per corner, fan-triangulated
    assert a["uv"].tolist() == [[float(u), float(v)] for u, v in want]
    assert a["tris"].tolist()[-2:] == [[9, 10, 11], [9, 11, 12]]
    for bad in ("f 1/4/1 2/1/1 3/1/1", "f 1/-4 2/1 3/1", "f 1/0/1 2/1/1 3/1/1"):
        (tmp_path / "bad.obj").write_text(OBJ_VT + bad + "\n")
        with pytest.raises(P.PathTracerError, match="bad face index"):
            P.Scene().loadAndProcessMeshFile(str(tmp_path / "bad.obj"))


def test_existing_obj_files_keep_their_geometry(pt_mod):
    """The repository's own OBJ files through the loader: counts as ever, uv flag from their vt lines."""
    import os
    P = pt_mod
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes", "input_data")
    for name in sorted(os.listdir(here)):
        if not name.endswith(".obj"):
            continue
        text = open(os.path.join(here, name)).read()
        s = P.Scene()
        m = s.loadAndProcessMeshFile(os.path.join(here, name))
        corners = sum(len(line.split()) - 1 for line in text.splitlines() if line.startswith("f "))
        assert s.counts()["nv"] == corners, name
        has_vt = any("/" in tok and tok.split("/")[1] for line in text.splitlines() if line.startswith("f ")
                     for tok in line.split()[1:])
        assert s.mesh_has_uv(m) == has_vt, name


# ---- generated primitives and the grammar -----------------------------------------------------------

GRAMMAR = """
DIFFUSE
paint
[0.8, 0.7, 0.6]

TEXTURE
check
CHECKER
[1, 0.5, 0.25]
[0.1,0.2,0.3]
3

TEXTURE
photo
PPM
tex/p.ppm

BOX
floor
[1, 0.1, 1]
[-1, 0, -1]
material:paint
texture:check

SPHERE
ball
0.1
[0, 0.3, 0]
texture:photo
shading:smooth

OBJ
quadmesh
quad.obj

MESH
q
quadmesh
texture:check

MESH
q2
quadmesh
"""

QUAD_OBJ = "v -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nvn 0 0 1\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nf 1/1/1 2/2/1 3/3/1 4/4/1\n"


def write_ppm(path, w, h, maxval, data, comment=True):
    head = b"P6\n" + (b"# a comment\n" if comment else b"") + f"{w} {h}\n{maxval}\n".encode()
    path.write_bytes(head + bytes(data))


def grammar_dir(tmp_path, text=GRAMMAR):
    (tmp_path / "tex").mkdir(exist_ok=True)
    rs = np.random.RandomState(1)
    data = rs.randint(0, 201, 4 * 3 * 3).astype(np.uint8)
    write_ppm(tmp_path / "tex" / "p.ppm", 4, 3, 200, data)
    (tmp_path / "quad.obj").write_text(QUAD_OBJ)
    (tmp_path / "scene.txt").write_text(text)
    return str(tmp_path / "scene.txt"), data


def test_grammar_checker_ppm_and_the_texture_attribute(pt_mod, tmp_path):
    P = pt_mod
    path, data = grammar_dir(tmp_path)
    s = P.Scene(path)
    check, photo = s.textures()
    c0, c1 = F([1, 0.5, 0.25]), F([0.1, 0.2, 0.3])
    assert check.shape == (3, 3, 3)
    for y in range(3):
        for x in range(3):
            assert np.array_equal(check[y, x], c0 if (x + y) % 2 == 0 else c1)
    assert photo.shape == (3, 4, 3)
    assert np.array_equal(photo, (data.astype(F) / F(200)).reshape(3, 4, 3))       # (float)byte / (float)maxval
    assert s.model_textures().tolist() == [0, 1, 0, -1]
    assert s.smooth().tolist() == [False, True, False, False]
    assert [s.mesh_has_uv(m) for m in range(3)] == [True, True, True]
    a = s.export()
    # BOX: each face's four corners carry (0,0), (1,0), (1,1), (0,1)
    assert a["uv"][:24].tolist() == [[0, 0], [1, 0], [1, 1], [0, 1]] * 6
    # SPHERE: vertex (j, i) of the 25 x 49 grid has ((float)((double)i / 48), (float)((double)j / 24))
    first = int(a["mesh_ranges"][1, 0])
    j, i = np.divmod(np.arange(25 * 49), 49)
    want = np.stack([(i.astype(np.float64) / 48).astype(F), (j.astype(np.float64) / 24).astype(F)], axis=1)
    assert np.array_equal(a["uv"][first:first + 25 * 49], want)
    # OBJ quad: (u, 1 - v)
    q = int(a["mesh_ranges"][2, 0])
    assert a["uv"][q:q + 4].tolist() == [[0, 1], [1, 1], [1, 0], [0, 0]]


@pytest.mark.parametrize("change,message", [
    (("texture:check", "texture:nope"), "unknown texture nope"),
    (("CHECKER\n[1, 0.5, 0.25]\n[0.1,0.2,0.3]\n3", "CHECKER\n[1, 0.5, 0.25]\n[0.1,0.2,0.3]\n0"), "size must be in [1,4096]"),
    (("CHECKER\n[1, 0.5, 0.25]\n[0.1,0.2,0.3]\n3", "CHECKER\n[1, 0.5, 0.25]\n[0.1,0.2,0.3]\n4097"), "size must be in [1,4096]"),
    (("CHECKER\n[1, 0.5, 0.25]\n[0.1,0.2,0.3]\n3", "CHECKER\n[1, 0.5]\n[0.1,0.2,0.3]\n3"), "TEXTURE CHECKER needs"),
    (("CHECKER\n[1, 0.5, 0.25]\n[0.1,0.2,0.3]\n3", "CHECKER\n[1, 0.5, 0.25]"), "TEXTURE CHECKER needs"),
    (("CHECKER\n[1, 0.5, 0.25]\n[0.1,0.2,0.3]\n3", "STRIPES\n[1, 0.5, 0.25]"), "unknown TEXTURE kind STRIPES"),
    (("TEXTURE\nphoto\nPPM\ntex/p.ppm", "TEXTURE\nphoto"), "TEXTURE block needs"),
    (("tex/p.ppm", "tex/missing.ppm"), "tex/missing.ppm"),
])
def test_grammar_refusals(pt_mod, tmp_path, change, message):
    P = pt_mod
    assert change[0] in GRAMMAR
    path, _ = grammar_dir(tmp_path, GRAMMAR.replace(change[0], change[1], 1))
    with pytest.raises(P.PathTracerError) as e:
        P.Scene(path)
    assert message in str(e.value)


def test_texture_on_a_mesh_without_uv_is_refused_by_the_grammar(pt_mod, tmp_path):
    P = pt_mod
    path, _ = grammar_dir(tmp_path)
    (tmp_path / "quad.obj").write_text(strip_vt(QUAD_OBJ))
    with pytest.raises(P.PathTracerError, match="mesh has no uv"):
        P.Scene(path)


@pytest.mark.parametrize("what", ["magic", "maxval", "zero maxval", "short", "size", "header", "byte"])
def test_malformed_ppm_is_refused_with_its_path(pt_mod, tmp_path, what):
    P = pt_mod
    path, data = grammar_dir(tmp_path)
    p = tmp_path / "tex" / "p.ppm"
    if what == "magic":
        p.write_bytes(b"P3\n4 3\n200\n" + bytes(data))
    elif what == "maxval":
        write_ppm(p, 4, 3, 256, data)
    elif what == "zero maxval":
        write_ppm(p, 4, 3, 0, data)
    elif what == "short":
        write_ppm(p, 4, 3, 200, data[:-1])
    elif what == "size":
        write_ppm(p, 0, 3, 200, data)
    elif what == "header":
        p.write_bytes(b"P6\n4 x\n200\n" + bytes(data))
    else:
        bad = data.copy()
        bad[7] = 201
        write_ppm(p, 4, 3, 200, bad)
    with pytest.raises(P.PathTracerError) as e:
        P.Scene(path)
    assert "tex/p.ppm" in str(e.value) and "Error loading texture" in str(e.value)
