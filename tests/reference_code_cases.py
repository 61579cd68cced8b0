"""Fixed inputs for the tests that hold the oracle and the kernels to the
reference's own code (oracle/_ref/libptref.so, see oracle/ref/bridge.cpp), and
the recordings of what that code returned for them.

Every input is generated from seeds here; a recording (tests/golden/
reference_code/*.npz, written by tests/golden/make_reference_code.py from the
built library) holds the library's outputs plus a digest of the inputs, so a
checkout without the reference tree still compares against the reference's
answers and notices if a generator drifts.  Test infrastructure: used by
test_reference_code.py (CPU) and test_gpu_reference_code.py."""
import hashlib
import os

import numpy as np

import oracle as O
from oracle import reference_code as R

from conftest import GOLDEN, INPUT_DATA
import path_scenes as S

RECORDINGS = os.path.join(GOLDEN, "reference_code")
RECORD_RAYS = 4096
FLOAT_MAX = np.float32(9999999.0)

ITERS = [0, 255, 1023, 4095, (1 << 22) - 1]
MAX_SLOT = 2800 * 2240 - 1
MAX_BOUNCES = 5
DEPTHS = list(range(1, 17))                       # remaining_bounces as shading seeds with
SEED_DEPTHS = [MAX_BOUNCES + k for k in (1, 2, 3, 4)]   # what jitter and the lens seed with
SQRT_OF_ONE_THIRD = np.float32(0.5773502691896257645091487805019574556476)

RECORD = False          # set by tests/golden/make_reference_code.py: write the recordings instead of reading them

_CACHE = {}


def once(key, make):
    if key not in _CACHE:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------
# the library or its recordings
# ---------------------------------------------------------------------------

def recording_path(name):
    return os.path.join(RECORDINGS, name.replace("^", "") + ".npz")


def reference_result(name, inputs, compute, fields):
    """What the reference's code gives for `inputs` (a tuple of arrays): from the
    built library when present, otherwise from the recording `name`.  With both,
    the recording must equal the library.  Returns (dict of arrays, source)."""
    import pytest
    path = recording_path(name)
    rec = None
    if RECORD:
        values = compute()
        write_recording(name, inputs, fields, values)
        return dict(zip(fields, values)), "library"
    if os.path.exists(path):
        with np.load(path) as z:
            rec = {k: z[k] for k in z.files}
        assert str(rec["inputs_sha256"]) == digest(*inputs), (
            f"{path} was recorded for other inputs: regenerate it with tests/golden/make_reference_code.py")
    if R.available():
        got = dict(zip(fields, compute()))
        if rec is not None:
            for k in fields:
                assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(rec[k]).view(np.uint8)), (
                    f"{path}: field {k} differs from what the built library returns")
        return got, "library"
    if rec is not None:
        return {k: rec[k] for k in fields}, "recording"
    pytest.skip(f"neither {R.LIB_PATH} (built from the reference tree) nor the recording {path} exists")


def write_recording(name, inputs, fields, values):
    os.makedirs(RECORDINGS, exist_ok=True)
    np.savez_compressed(recording_path(name), inputs_sha256=np.array(digest(*inputs)),
                        **{k: np.ascontiguousarray(v) for k, v in zip(fields, values)})


def subset(n, seed, k=RECORD_RAYS):
    """Sorted indices of the recorded subset of a batch of n."""
    if n <= k:
        return np.arange(n)
    return np.sort(np.random.RandomState(seed).choice(n, k, replace=False))


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------

def ref_scene():
    return once("ref_scene", lambda: O.reference_scene(INPUT_DATA))


def export_of(fs):
    """A FlatScene as the dict Scene.export() gives (what path_scenes' ray generators read)."""
    return {k: getattr(fs, k) for k in ("vpos", "vnrm", "tris", "mesh_ranges", "mesh_bbox", "model_ints", "model_m2w",
                                        "model_w2m", "model_color", "grid_ints", "grid_vw", "vox", "per_voxel")}


# Section I scenes of path_scenes that the host build of the reference can stand
# for: every flat axis and each non-zero thickness, the exact ties, the coincident
# pairs.  The exactly flat quads and the needle (a voxel width of 0) are left out:
# there every ray reaches computeRayGridIntersection's float->int conversion of
# +inf or NaN, which the host converts to INT_MIN and the GPU saturates
# (oracle/ref/bridge.cpp, difference 5); those scenes stay with test_degenerate_cpu
# and test_gpu_degenerate.
DEGENERATE = ["flat-x-h2^-7-xf", "flat-y-h2^-2-id", "flat-z-h4-xf", "flat-y-h2^-7-id",
              "ridge-side-major", "ridge-interleaved", "ridge-permuted",
              "pair-2-first-ab", "pair-10-middle-ba", "pair-14-last-ab"]
DEGENERATE_RAYS = 1024
SEVEN = "seven-materials"


def spec_of(name):
    if name == SEVEN:
        return S.seven_material_spec()
    return S.degenerate_spec(name)


def flat_scene(name):
    """The oracle builder's FlatScene of a named scene ('ref', SEVEN or one of DEGENERATE)."""
    if name == "ref":
        return ref_scene()
    return once(("scene", name), lambda: S.oracle_scene_from_spec(O, *spec_of(name)))


def degenerate_rays(name):
    def make():
        a = export_of(flat_scene(name))
        kind = name.split("-")[0]
        if kind == "flat":
            o, d, _ = S.flat_rays(a)
        elif kind == "ridge":
            on, off, d = S.ridge_rays()
            o, d = np.concatenate([on, off]), np.concatenate([d, d])
        else:
            o, d = S.coincident_rays()
        idx = subset(len(o), 17, DEGENERATE_RAYS)
        return np.ascontiguousarray(o[idx], np.float32), np.ascontiguousarray(d[idx], np.float32)
    return once(("rays", name), make)


# ---------------------------------------------------------------------------
# ray batches in the reference scene
# ---------------------------------------------------------------------------

CAM_W, CAM_H = 500, 400


def camera_rays(w=CAM_W, h=CAM_H):
    """generateRaysKernel's rays of a w x h frame (Renderer.cpp:521-555), in float32 as it computes them."""
    def make():
        i = np.arange(w * h)
        x = (i % w).astype(np.float32); y = (i // w).astype(np.float32)
        sx = np.float32(20.0 / w); sy = np.float32(16.0 / h)
        wx = (-10.0 + (x * sx).astype(np.float64)).astype(np.float32)
        wy = (-4.0 + (y * sy).astype(np.float64)).astype(np.float32)
        cam = np.float32([0, 0, 920])
        d = np.stack([wx, wy, np.full_like(wx, 900.0)], 1) - cam
        return np.tile(cam, (w * h, 1)), np.ascontiguousarray(d, np.float32)
    return once(("camera", w, h), make)


def secondary_rays():
    """Rays leaving the camera rays' hits (the oracle's exhaustive closest hit, so
    that the batch does not depend on the walk under test) from ip + 0.1 n into the
    hemisphere about n: seeded normal directions, turned to n's side, not normalised."""
    def make():
        o, d = camera_rays()
        t, n, m = O.intersect_rays(ref_scene(), o, d, accel=1)
        assert (m >= 0).all()
        u = d / np.linalg.norm(d.astype(np.float64), axis=1)[:, None]
        ip = o + u * t[:, None]
        o2 = (ip + 0.1 * n.astype(np.float64)).astype(np.float32)
        rs = np.random.RandomState(23)
        d2 = rs.normal(size=d.shape) * (10.0 ** rs.uniform(-1, 1, (len(d), 1)))
        flip = (d2 * n).sum(1) < 0
        d2[flip] = -d2[flip]
        return o2, np.ascontiguousarray(d2, np.float32)
    return once("secondary", make)


def random_rays(n=20000):
    """Origins uniform in +-150, normal directions; the first quarter axis-aligned."""
    def make():
        rs = np.random.RandomState(31)
        o = rs.uniform(-150, 150, (n, 3)).astype(np.float32)
        d = rs.normal(size=(n, 3)).astype(np.float32)
        k = n // 4
        d[:k] = 0.0
        d[np.arange(k), rs.randint(0, 3, k)] = rs.choice([-1.0, 1.0], k)
        return o, d
    return once(("random", n), make)


BATCHES = {"camera": camera_rays, "secondary": secondary_rays, "random": random_rays}
BATCH_SEED = {"camera": 41, "secondary": 42, "random": 43}


def batch(name, full):
    """(scene name, origins, directions) of a named batch: the whole batch, or its recorded subset."""
    if name in BATCHES:
        o, d = BATCHES[name]()
        if not full:
            idx = subset(len(o), BATCH_SEED[name])
            o, d = np.ascontiguousarray(o[idx]), np.ascontiguousarray(d[idx])
        return "ref", o, d
    o, d = degenerate_rays(name)
    return name, o, d


HIT_FIELDS = ("dist", "normal", "mtype")


def reference_hits(name):
    """The reference's (dist, normal, material type) for the recorded subset of a batch."""
    def make():
        sc, o, d = batch(name, full=False)
        got, src = reference_result("hits_" + name, (o, d), lambda: R.intersect_rays(flat_scene(sc), o, d)[:3], HIT_FIELDS)
        return got["dist"], got["normal"], got["mtype"], src
    return once(("ref_hits", name), make)


def reference_hits_full(name):
    """The same for the whole batch; needs the library."""
    def make():
        sc, o, d = batch(name, full=True)
        return R.intersect_rays(flat_scene(sc), o, d)[:3]
    return once(("ref_hits_full", name), make)


def oracle_types(fs, model):
    """Material type per hit model index (-1 for a miss)."""
    model = np.asarray(model)
    return np.where(model >= 0, fs.model_ints[np.maximum(model, 0), 2], -1).astype(np.int32)


# ---------------------------------------------------------------------------
# shading and scatter inputs
# ---------------------------------------------------------------------------

def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=1)[:, None]


def edge_normals():
    """Unit-ish normals whose |x|, and |x| and |y|, sit on and one ulp either side of
    SQRT_OF_ONE_THIRD: calculateRandomDirectionInHemisphere's two branch boundaries."""
    s = SQRT_OF_ONE_THIRD
    vals = [np.nextafter(s, np.float32(0)), s, np.nextafter(s, np.float32(1))]
    out = []
    for sx in (1, -1):
        for a in vals:
            r = np.sqrt(max(0.0, 1.0 - float(a) ** 2))
            out.append((sx * a, 0.6 * r, 0.8 * r))                  # |y| below the threshold
            for sy in (1, -1):
                for b in vals:
                    z = np.sqrt(max(0.0, 1.0 - float(a) ** 2 - float(b) ** 2))
                    out.append((sx * a, sy * b, z))                  # |x| >= and |y| around it
    return np.array(out, np.float32)


def metal_edge_pairs():
    """(normal, incoming direction) pairs whose mirrored direction w has |w.x| on and
    a few ulp either side of 0.1: calculateMetalScattering's basis branch."""
    n, d = [], []
    c = np.float32(0.1)
    xs = [c]
    for _ in range(3):
        xs = [np.nextafter(xs[0], np.float32(0))] + xs + [np.nextafter(xs[-1], np.float32(1))]
    for sx in (1, -1):
        for x in xs:
            r = np.sqrt(1.0 - float(x) ** 2)
            for ang in (0.3, 1.9, 4.0):
                # the normal is orthogonal to d, so the mirrored direction is d itself
                dd = np.array([sx * float(x), r * np.cos(ang), r * np.sin(ang)])
                nn = np.array([0.0, -np.sin(ang), np.cos(ang)])
                n.append(nn); d.append(dd)
    return np.array(n, np.float32), np.array(d, np.float32)


def shade_inputs(n=2048, seed=5):
    """One shadeRayKernel batch: every material type (SPECULAR and REFRACTIVE too),
    hits and misses, remaining bounces 1..16 and a few <= 0, slots up to MAX_SLOT,
    incoming directions of any length, normals on the branch boundaries."""
    def make():
        rs = np.random.RandomState(seed)
        slot = rs.randint(0, MAX_SLOT + 1, n).astype(np.int32)
        slot[:4] = [0, 1, MAX_SLOT, MAX_SLOT - 1]
        orig = rs.uniform(-500, 500, (n, 3)).astype(np.float32)
        dirs = (unit(rs.normal(size=(n, 3))) * 10.0 ** rs.uniform(-3, 3, (n, 1))).astype(np.float32)
        color = rs.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
        bounces = np.asarray(DEPTHS, np.int32)[np.arange(n) % len(DEPTHS)].copy()
        bounces[rs.rand(n) < 0.03] = 0
        bounces[rs.rand(n) < 0.02] = -1
        hit_type = (np.arange(n) // len(DEPTHS) % 7).astype(np.int32)
        hit_dist = rs.uniform(0.0, 2000.0, n).astype(np.float32)
        hit_dist[rs.rand(n) < 0.1] = FLOAT_MAX
        nrm = unit(rs.normal(size=(n, 3))).astype(np.float32)
        en = edge_normals()
        mn, md = metal_edge_pairs()
        k0 = 64
        nrm[k0:k0 + len(en)] = en
        k1 = k0 + len(en)
        nrm[k1:k1 + len(mn)] = mn
        dirs[k1:k1 + len(md)] = md * rs.choice([0.25, 1.0, 8.0], (len(md), 1)).astype(np.float32)
        hit_type[k1:k1 + len(mn)] = O.MATERIALS["METAL"]
        hit_dist[k0:k1 + len(mn)] = 100.0
        bounces[k0:k1 + len(mn)] = np.maximum(bounces[k0:k1 + len(mn)], 1)
        # the hemisphere's boundaries matter to DIFFUSE and (half the time) COAT
        hit_type[k0:k1] = np.where(np.arange(len(en)) % 2 == 0, O.MATERIALS["DIFFUSE"], O.MATERIALS["COAT"])
        hit_color = rs.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
        return slot, orig, dirs, color, bounces, hit_dist, nrm, hit_type, hit_color
    return once(("shade", n, seed), make)


SHADE_FIELDS = ("orig", "dir", "color", "bounces", "hit_dist")


def reference_shade(it):
    def make():
        inp = shade_inputs()
        slot, orig, dirs, color, bounces, hit_dist, nrm, hit_type, hit_color = inp
        got, src = reference_result(f"shade_iter{it}", inp + (np.int64(it),),
                                    lambda: R.shade(it, slot, orig, dirs, color, bounces, hit_dist, nrm, hit_type, hit_color),
                                    SHADE_FIELDS)
        return tuple(got[k] for k in SHADE_FIELDS) + (src,)
    return once(("ref_shade", it), make)


def seed_triples(n=RECORD_RAYS, seed=9):
    """(iter, slot, depth) triples: every iteration of ITERS with depths 1..16 and
    max_bounces + 1..4, slots up to MAX_SLOT with both ends."""
    def make():
        rs = np.random.RandomState(seed)
        depths = np.asarray(DEPTHS + SEED_DEPTHS, np.int32)
        it = np.asarray(ITERS, np.int32)[np.arange(n) % len(ITERS)]
        dp = depths[(np.arange(n) // len(ITERS)) % len(depths)]
        slot = rs.randint(0, MAX_SLOT + 1, n).astype(np.int32)
        slot[:len(ITERS)] = 0
        slot[len(ITERS):2 * len(ITERS)] = MAX_SLOT
        return it.copy(), slot, dp.copy()
    return once(("triples", n, seed), make)


def normalize_f32(d):
    """glm::normalize in float32: d * (1 / sqrt((x x + y y) + z z))."""
    d = np.asarray(d, np.float32)
    t = d * d
    s = (t[:, 0] + t[:, 1]) + t[:, 2]
    inv = np.float32(1.0) / np.sqrt(s, dtype=np.float32)
    return (d * inv[:, None]).astype(np.float32)


SCATTER_KINDS = {"hemisphere": (R.HEMISPHERE, "DIFFUSE"), "metal": (R.METAL, "METAL"), "coat": (R.COAT, "COAT"),
                 "reflect": (R.REFLECT, "REFLECTIVE")}


def scatter_inputs(n=2048, seed=13):
    def make():
        rs = np.random.RandomState(seed)
        it, slot, dp = seed_triples(n, seed + 1)
        nrm = unit(rs.normal(size=(n, 3))).astype(np.float32)
        dirs = (unit(rs.normal(size=(n, 3))) * 10.0 ** rs.uniform(-3, 3, (n, 1))).astype(np.float32)
        en = edge_normals()
        mn, md = metal_edge_pairs()
        nrm[32:32 + len(en)] = en
        k = 32 + len(en)
        nrm[k:k + len(mn)] = mn
        dirs[k:k + len(md)] = md * rs.choice([0.25, 1.0, 8.0], (len(md), 1)).astype(np.float32)
        return it, slot, dp, nrm, dirs
    return once(("scatter", n, seed), make)


def reference_scatter(kind):
    """The reference's scatter function `kind` on scatter_inputs(), the incoming
    directions passed through normalize_f32 first, as shadeRayKernel passes them."""
    def make():
        inp = scatter_inputs()
        it, slot, dp, nrm, dirs = inp
        got, src = reference_result("scatter_" + kind, inp, lambda: (R.scatter(SCATTER_KINDS[kind][0], it, slot, dp, nrm, normalize_f32(dirs)),),
                                    ("out",))
        return got["out"], src
    return once(("ref_scatter", kind), make)


def reference_u01():
    def make():
        it, slot, dp = seed_triples()
        got, src = reference_result(
            "u01_first", (it, slot, dp),
            lambda: (np.array([R.u01_first(a, b, c) for a, b, c in zip(it, slot, dp)], np.float32),), ("u",))
        return got["u"], src
    return once("ref_u01", make)


# ---------------------------------------------------------------------------
# transforms, the grid builder
# ---------------------------------------------------------------------------

def transform_points():
    rs = np.random.RandomState(3)
    return np.concatenate([rs.uniform(-1000, 1000, (64, 3)), unit(rs.normal(size=(64, 3))),
                           np.eye(3), np.zeros((1, 3))]).astype(np.float32)


TRANSFORM_FIELDS = [f"m{i}_{k}" for i in range(11) for k in ("m2w", "w2m", "pf", "df", "nf", "pi", "di", "ni")]


def reference_transforms():
    """Per reference model i: m{i}_m2w, m{i}_w2m (glm's translate * rotate * scale and its
    inverse) and transformPosition / Direction / Normal of transform_points() under the
    forward (p/d/n + f) and the inverse (+ i) matrix."""
    def make():
        pts = transform_points()
        models = O.REFERENCE_MODELS

        def compute():
            out = []
            for m in models:
                assert m["rot"][0] == 0 and m["rot"][2] == 0        # Scene.cpp rotates about y only
                m2w, w2m = R.model_matrix(m["scale"], m["rot"][1], m["translate"])
                out += [m2w, w2m]
                for mat in (m2w, w2m):
                    out += [R.transform(k, mat, pts) for k in (R.POSITION, R.DIRECTION, R.NORMAL)]
            return out
        inputs = (pts, np.array([m["scale"] + m["rot"] + m["translate"] for m in models], np.float64))
        return reference_result("transforms", inputs, compute, TRANSFORM_FIELDS)
    return once("ref_transforms", make)


GRID_FIELDS = ("model_grid", "grid_ints", "grid_vw", "vox", "per_voxel")


def reference_grid():
    def make():
        fs = ref_scene()
        inputs = (fs.vpos, fs.tris, fs.mesh_ranges, fs.mesh_bbox, fs.model_ints[:, 0])
        return reference_result("grid_build", inputs, lambda: R.build_grids(fs), GRID_FIELDS)
    return once("ref_grid", make)


# ---------------------------------------------------------------------------
# renders
# ---------------------------------------------------------------------------

RENDER_ITERS = 3
RENDERS = [("ref", 64, 48, 0), ("ref", 37, 23, 0), ("ref", 37, 23, 1), ("ref", 64, 48, 1), (SEVEN, 64, 48, 0)]
RENDER_FIELDS = ("image", "live")


def render_id(case):
    sc, w, h, td = case
    return f"{sc}-{w}x{h}-td{td}"


def reference_render(case):
    """The reference's (accumulator, live rays per bounce, source) for a render case."""
    def make():
        sc, w, h, td = case
        fs = flat_scene(sc)
        inputs = (fs.vpos, fs.tris, fs.model_m2w, fs.per_voxel, np.int64([w, h, td, RENDER_ITERS]))
        got, src = reference_result("render_" + render_id(case), inputs,
                                    lambda: R.render(fs, w, h, RENDER_ITERS, tail_drop=td), RENDER_FIELDS)
        return got["image"], got["live"], src
    return once(("ref_render", case), make)
