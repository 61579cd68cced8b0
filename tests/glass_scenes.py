"""Fixture scene of the dielectric-material tests (test infrastructure).

smooth_scenes' room under its lamp with a glass BOX (synthetic.light_mesh's cube: repeated flat
normals, so it stays flat and untextured, which needs no triangle identification) and four
instances of the displaced torus (no two of its triangles share a flat normal): glass flat, glass
smooth, glass with a texture, and one DIFFUSE.  A sphere alone never reaches total internal
reflection (its inner angle of incidence equals its refraction angle); the box and the torus do.
The iors cover water, crown glass and diamond."""
import copy

import numpy as np

import glass_ref as GR
import path_scenes as PS
import smooth_scenes as SS
from pathtracerap_amd.synthetic import light_mesh, room_mesh, torus_mesh

F = np.float32
BOX, FLAT, SMOOTH, TEXTURED, DIFFUSE = 2, 3, 4, 5, 6          # model indices (0, 1: the room and the lamp)
TORUS_MESH = 2
# (mesh, material, colour, scale, rotation, translation, smooth, texture, ior)
_MODELS = [(1, "DIELECTRIC", (0.95, 0.99, 0.95), (0.07, 0.07, 0.07), (20, 30, 10), (10, 330, -60), False, -1, 1.5),
           (2, "DIELECTRIC", (0.75, 0.92, 0.99), (0.030, 0.040, 0.025), (35, 20, 10), (-300, 60, 60), False, -1, 1.33),
           (2, "DIELECTRIC", (0.99, 0.90, 0.95), (0.035, 0.025, 0.030), (70, -30, 15), (-90, 90, 150), True, -1, 1.5),
           (2, "DIELECTRIC", (0.90, 0.95, 0.70), (0.025, 0.035, 0.040), (20, 60, -40), (120, 70, 80), False, 0, 2.4),
           (2, "DIFFUSE", (0.99, 0.99, 0.75), (0.030, 0.030, 0.045), (100, 10, 30), (320, 110, 0), False, -1, 1.5)]


def fixture_spec(ntri=320, uv_seed=43, tex_seed=47):
    """-> dict(meshes, models, smooth, binding, ior, mesh_uv {mesh: (nv, 2)}, textures)."""
    pos, nrm, tris = torus_mesh(ntri, seed=SS.TORUS_SEED)
    meshes = [room_mesh(), light_mesh(), (pos, nrm, tris)]
    models = [dict(mesh=0, scale=(0.1, 0.1, 0.1), rot=(0, 0, 0), translate=(0, -120, 0), material="DIFFUSE",
                   color=(0.85, 0.85, 0.85)),
              dict(mesh=1, scale=(0.2, 0.02, 0.2), rot=(0, 0, 0), translate=(0, 870, -50), material="EMISSIVE",
                   color=(0.99, 0.99, 0.99))]
    models += [dict(mesh=me, scale=s, rot=r, translate=t, material=m, color=c) for me, m, c, s, r, t, _, _, _ in _MODELS]
    return dict(meshes=meshes, models=models, smooth=np.array([False, False] + [m[6] for m in _MODELS], bool),
                binding=np.array([-1, -1] + [m[7] for m in _MODELS], np.int64),
                ior=np.array([1.5, 1.5] + [m[8] for m in _MODELS], F),
                mesh_uv={TORUS_MESH: np.random.RandomState(uv_seed).uniform(-2, 3, (len(pos), 2)).astype(F)},
                textures=[np.random.RandomState(tex_seed).uniform(0.3, 1.0, (3, 5, 3)).astype(F)])


def glass_models(spec):
    return [i for i, m in enumerate(spec["models"]) if m["material"] == "DIELECTRIC"]


def as_diffuse(spec):
    """The spec with every dielectric instance switched to DIFFUSE."""
    out = copy.deepcopy(spec)
    for i in glass_models(spec):
        out["models"][i]["material"] = "DIFFUSE"
    return out


def gpu_scene(P, spec, ior=True):
    """The scene of a spec; ior False: without the iors set (every model keeps the default)."""
    s = PS.scene_from_spec(P, spec["meshes"], spec["models"])
    for mesh, uv in spec["mesh_uv"].items():
        s.set_mesh_uv(mesh, uv)
    for t in spec["textures"]:
        s.add_texture(t)
    for i in np.nonzero(spec["smooth"])[0]:
        s.set_smooth(int(i))
    for i, t in enumerate(spec["binding"]):
        if t >= 0:
            s.set_texture(i, int(t))
    if ior:
        for i, v in enumerate(spec["ior"]):
            s.set_ior(i, float(v))
    return s


def vertex_uv(spec):
    return np.concatenate([spec["mesh_uv"].get(i, np.zeros((len(np.asarray(m[0]).reshape(-1, 3)), 2), F))
                           for i, m in enumerate(spec["meshes"])]).astype(F)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def next_up(x, steps):
    """float32 x moved `steps` ulps (either sign)."""
    return (np.asarray(x, F).view(np.int32) + np.asarray(steps, np.int32)).view(F)


def hook_inputs(seed=3, n_random=4096):
    """The inputs of the hook test: (dirs, normals, ior, u) float32, and the slices of the edge
    cases by name.  Normals are unit length up to float32 rounding; dirs are unit length except
    the unnormalised block."""
    rs = np.random.RandomState(seed)
    D, N, I, U, where = [], [], [], [], {}

    def add(name, d, n, ior, u):
        d, n = np.asarray(d, F).reshape(-1, 3), np.asarray(n, F).reshape(-1, 3)
        m = len(d)
        start = sum(len(x) for x in D)
        D.append(d); N.append(n)
        I.append(np.broadcast_to(np.asarray(ior, F), (m,)).copy()); U.append(np.broadcast_to(np.asarray(u, F), (m,)).copy())
        where[name] = slice(start, start + m)

    add("random", unit(rs.normal(size=(n_random, 3))), unit(rs.normal(size=(n_random, 3))),
        rs.choice(np.array([1.0, 1.0001, 1.33, 1.5, 2.4, 4.0], F), n_random), rs.uniform(0, 1, n_random))
    # exact normal incidence from both sides, every axis
    ax = np.concatenate([np.eye(3), -np.eye(3)])
    add("normal incidence, entering", -ax, ax, 1.5, 0.5)
    add("normal incidence, leaving", ax, ax, 1.5, 0.5)
    # |ci| below 1e-6, both signs, and exactly 0
    n = unit(rs.normal(size=(64, 3)))
    t = unit(np.cross(n, rs.normal(size=(64, 3))))
    eps = rs.uniform(-1e-6, 1e-6, (64, 1))
    eps[:4] = 0.0
    add("grazing", t + eps * n, n, rs.choice(np.array([1.0, 1.33, 1.5, 4.0], F), 64), rs.uniform(0, 1, 64))
    # c stepped ulp by ulp across the critical angle, leaving: dir = (s, 0, c), n = (0, 0, 1)
    for ior in (1.33, 1.5, 4.0):
        cc = np.sqrt(1.0 - 1.0 / (np.float64(F(ior)) ** 2))
        c = next_up(np.full(129, cc, F), np.arange(-64, 65))
        s = np.sqrt(np.maximum(0.0, 1.0 - c.astype(np.float64) ** 2))
        add(f"critical angle, ior {ior}", np.stack([s, np.zeros_like(s), c.astype(np.float64)], 1), [[0, 0, 1]] * 129, ior, 0.999)
    # ior exactly 1: r0 = 0, eta = 1
    add("ior one", unit(rs.normal(size=(64, 3))), unit(rs.normal(size=(64, 3))), 1.0, rs.uniform(0, 1, 64))
    # unnormalised directions
    add("unnormalised", unit(rs.normal(size=(64, 3))) * rs.uniform(1e-3, 1e3, (64, 1)), unit(rs.normal(size=(64, 3))),
        rs.choice(np.array([1.33, 1.5, 2.4], F), 64), rs.uniform(0, 1, 64))
    # u equal to Fr (refraction), just below it (reflection) and 0 (filled in below)
    d, n = unit(rs.normal(size=(96, 3))), unit(rs.normal(size=(96, 3)))
    add("u at Fr", d, n, 1.5, 0.0)
    D, N, I, U = (np.concatenate(x) for x in (D, N, I, U))
    sl = where["u at Fr"]
    fr = GR.scatter(GR.SR._normalize(D[sl]), N[sl], I[sl], U[sl])["fr"]      # of the direction the hook normalises
    has = np.isfinite(fr)                                   # not under total internal reflection
    assert has.sum() > 48
    kind = np.arange(96) % 3                                # 0: u = Fr, 1: one ulp below, 2: u = 0
    U[sl] = np.where(has & (kind == 0), fr, np.where(has & (kind == 1), next_up(np.where(has, fr, F(1)), -1), F(0)))
    return (D, N, I, U), where
