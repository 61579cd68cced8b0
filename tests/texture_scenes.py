"""Fixture scenes of the texture tests (test infrastructure).

The textured models are instances of smooth_scenes' displaced torus (no two of its triangles share
a flat normal, so texture_ref can tell the hit triangle from the oracle's normal): one per material
that multiplies by the model colour, and a second DIFFUSE one for the sixth texture.  The room and
the lamp (meshes with repeated flat normals, and without uv) stay untextured.  Per-vertex uvs are
seeded draws from [-2, 3]: wrap, negative values and large gradients across a triangle occur.
Textures are seeded random texels at the smallest shapes where wrap and index arithmetic can go
wrong (w x h): 1x1, 1x5, 5x1, 2x2, 5x3, and 64x64."""
import numpy as np

import path_scenes as PS
import smooth_scenes as SS
from pathtracerap_amd.synthetic import light_mesh, room_mesh, torus_mesh

F = np.float32
TEXTURE_SIZES = [(1, 1), (1, 5), (5, 1), (2, 2), (5, 3), (64, 64)]          # (w, h)
# (material, colour, scale, rotation, translation, smooth, texture)
_TORI = [("DIFFUSE", (0.75, 0.62, 0.40), (0.030, 0.040, 0.025), (35, 20, 10), (-300, 60, 60), False, 5),
         ("METAL", (0.90, 0.90, 0.95), (0.035, 0.025, 0.030), (70, -30, 15), (-90, 90, 150), True, 4),
         ("COAT", (0.15, 0.30, 0.90), (0.025, 0.035, 0.040), (20, 60, -40), (120, 70, 80), False, 3),
         ("REFLECTIVE", (0.99, 0.99, 0.75), (0.030, 0.030, 0.045), (100, 10, 30), (320, 110, 0), False, 2),
         ("EMISSIVE", (0.95, 0.60, 0.20), (0.040, 0.030, 0.030), (50, 45, 0), (10, 330, -60), False, 1),
         ("DIFFUSE", (0.60, 0.90, 0.55), (0.030, 0.030, 0.030), (10, 80, 50), (230, 330, 120), False, 0)]
TORUS_MESH = 2
FIRST_TORUS = 2                                      # models 0, 1: the room and the lamp


def textures(seed=41):
    rs = np.random.RandomState(seed)
    return [rs.uniform(0.05, 1.0, (h, w, 3)).astype(F) for w, h in TEXTURE_SIZES]


def fixture_spec(ntri=320, uv_seed=43, extra=None):
    """-> dict(meshes, models, smooth, binding, mesh_uv {mesh: (nv, 2)}, textures).
    extra: a (mesh, model dict, uv, texture) added last."""
    pos, nrm, tris = torus_mesh(ntri, seed=SS.TORUS_SEED)
    meshes = [room_mesh(), light_mesh(), (pos, nrm, tris)]
    models = [dict(mesh=0, scale=(0.1, 0.1, 0.1), rot=(0, 0, 0), translate=(0, -120, 0), material="DIFFUSE",
                   color=(0.85, 0.85, 0.85)),
              dict(mesh=1, scale=(0.2, 0.02, 0.2), rot=(0, 0, 0), translate=(0, 870, -50), material="EMISSIVE",
                   color=(0.99, 0.99, 0.99))]
    models += [dict(mesh=TORUS_MESH, scale=s, rot=r, translate=t, material=m, color=c) for m, c, s, r, t, _, _ in _TORI]
    smooth = [False, False] + [t[5] for t in _TORI]
    binding = [-1, -1] + [t[6] for t in _TORI]
    mesh_uv = {TORUS_MESH: np.random.RandomState(uv_seed).uniform(-2, 3, (len(pos), 2)).astype(F)}
    if extra is not None:
        mesh, model, uv, tex = extra
        meshes.append(mesh)
        models.append(dict(model, mesh=len(meshes) - 1))
        smooth.append(False)
        binding.append(tex)
        mesh_uv[len(meshes) - 1] = np.asarray(uv, F)
    return dict(meshes=meshes, models=models, smooth=np.array(smooth, bool), binding=np.array(binding, np.int64),
                mesh_uv=mesh_uv, textures=textures())


def zero_area_extra():
    """path_scenes.zero_area_mesh as a textured diffuse model in front of the tori."""
    return (PS.zero_area_mesh(), dict(scale=(0.08, 0.08, 0.08), rot=(60, 0, 0), translate=(-150, 260, 250),
                                      material="DIFFUSE", color=(0.3, 0.8, 0.4)),
            [(0.1, 0.2), (1.3, -0.4), (0.6, 2.2), (-1.7, 0.45)], 4)


def gpu_scene(P, spec, textured=True, smooth=True):
    """The scene of a spec; textured / smooth False: without the bindings / the flags (the uvs and
    the textures are there all the same)."""
    s = PS.scene_from_spec(P, spec["meshes"], spec["models"])
    for mesh, uv in spec["mesh_uv"].items():
        s.set_mesh_uv(mesh, uv)
    for t in spec["textures"]:
        s.add_texture(t)
    if smooth:
        for i in np.nonzero(spec["smooth"])[0]:
            s.set_smooth(int(i))
    if textured:
        for i, t in enumerate(spec["binding"]):
            if t >= 0:
                s.set_texture(i, int(t))
    return s


def vertex_uv(spec):
    """The (nv_total, 2) per-vertex uv of a spec's scene, (0, 0) for a mesh without uv (Scene.export()["uv"])."""
    return np.concatenate([spec["mesh_uv"].get(i, np.zeros((len(np.asarray(m[0]).reshape(-1, 3)), 2), F))
                           for i, m in enumerate(spec["meshes"])]).astype(F)
