"""CPU preconditions of test_gpu_degenerate.py (path_scenes.py section I; no GPU:
the oracle and the product's host build).  The product builds every flat, thin
and needle mesh exactly as the oracle's builder does; the reference grid sees a
mesh with no extent on a model axis only from rays with a negative model-space
direction on that axis, the exact closest hit from both sides; a ray down onto the
ridge is an exact tie that the triangle order decides; of two coincident
instances the lower model index answers.  The shares asserted here are
conditions the GPU tests rely on, not measurements."""
import itertools

import numpy as np
import pytest

import path_scenes as S
from helpers import assert_bitexact, flat_from_export
from test_bvh_build import _walk, _walk4

FLAT_CASES = [(ax, h, xf) for ax in range(3) for h in S.FLAT_THICKNESS for xf in (False, True)]
_flat_id = lambda c: f"{'xyz'[c[0]]}-{S._h_id(c[1])}-{'xf' if c[2] else 'id'}"


def _compare(a, o):
    for k in ("vpos", "vnrm", "tris", "mesh_ranges", "mesh_bbox", "model_ints", "model_m2w", "model_w2m", "model_color",
              "grid_ints", "grid_vw", "vox", "per_voxel"):
        assert_bitexact(a[k], getattr(o, k), k)


def _check_build(P, O, meshes, models, zero_axes):
    """Product export == oracle.build_scene bit for bit (the per-voxel lists among
    it); grid_vw is exactly 0 on `zero_axes` and positive elsewhere; every triangle
    is in exactly one leaf of the binary and of the 4-wide BLAS, whose boxes are finite."""
    s = S.scene_from_spec(P, meshes, models)
    a = s.export()
    _compare(a, S.oracle_scene_from_spec(O, meshes, models))
    vw = a["grid_vw"][0]
    for k in range(3):
        assert (vw[k] == 0.0) if k in zero_axes else (vw[k] > 0.0), (k, vw)
    nt = len(a["tris"])
    # a flat axis' triangles sit in voxel 0 of it, whatever the other indices
    lists = [a["per_voxel"][v[0]:v[1]] for v in a["vox"]]
    held = np.zeros(nt, int)
    for i, l in enumerate(lists):
        idx = (i % 25, (i // 25) % 25, i // 625)
        if len(l):
            assert all(idx[k] == 0 for k in zero_axes), idx
            held[l] += 1
    assert (held > 0).all()
    b, b4 = s.export_bvh(), s.export_bvh4()
    leaves, depth = _walk(b["nodes"], b["roots"][0])
    seen = np.zeros(nt, int)
    for first, cnt, (lo, hi) in leaves:
        assert np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()
        refs = b["refs"][first:first + cnt]
        seen[refs[refs >= 0]] += 1
    assert (seen == 1).all() and depth <= 23
    leaves4, _, _ = _walk4(b4["nodes"], b4["roots"][0], b4["leaf_base"][0])
    seen4 = np.zeros(nt, int)
    for first, cnt, (lo, hi) in leaves4:
        assert np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()
        refs = b["refs"][first:first + cnt]
        seen4[refs[refs >= 0]] += 1
    assert (seen4 == 1).all()
    return a


@pytest.mark.parametrize("case", FLAT_CASES, ids=_flat_id)
def test_flat_and_thin_meshes_build_as_the_oracle_builds_them(pt_mod, oracle_mod, case):
    ax, h, xf = case
    a = _check_build(pt_mod, oracle_mod, *S.flat_spec(ax, h, xf), zero_axes=[ax] if h == 0.0 else [])
    bb = a["mesh_bbox"][0]
    assert bb[3 + ax] - bb[ax] == np.float32(h)                 # the loaded coordinates are the dyadic values themselves
    assert bb[(ax + 1) % 3] == -S.FLAT_HALF and bb[3 + (ax + 2) % 3] == S.FLAT_HALF
    if h > 0:
        assert a["grid_vw"][0][ax] == np.float32(h) / np.float32(25)


@pytest.mark.parametrize("xf", [False, True], ids=["id", "xf"])
def test_needle_builds_as_the_oracle_builds_it(pt_mod, oracle_mod, xf):
    _check_build(pt_mod, oracle_mod, *S.flat_spec(0, 0.0, xf, mesh=S.needle_mesh()), zero_axes=[1, 2])


@pytest.mark.parametrize("order", S.RIDGE_ORDERS)
def test_ridge_builds_as_the_oracle_builds_it(pt_mod, oracle_mod, order):
    a = _check_build(pt_mod, oracle_mod, *S.ridge_spec(order), zero_axes=[])
    assert len(a["tris"]) == 4 * S.RIDGE_SEGMENTS
    assert_bitexact(a["mesh_bbox"][0], np.float32([-1024, 0, -1024, 1024, 1024, 1024]), "ridge box")


@pytest.mark.parametrize("case", FLAT_CASES, ids=_flat_id)
def test_oracle_sees_a_flat_mesh_from_one_side_in_grid_mode(pt_mod, oracle_mod, case):
    """h = 0: the grid reports no hit at all for a positive model-space direction on
    the flat axis and nearly all for a negative one, the exact mode nearly all from
    both sides; a mesh of any thickness > 0 is seen from both sides in both modes."""
    P, O = pt_mod, oracle_mod
    ax, h, xf = case
    s, o, d = S.degenerate_case(P, f"flat-{_flat_id(case)}")
    a = s.export()
    assert len(o) == 4096 and S.flat_axis(a) == ax
    pos = S.flat_rays(a)[2]
    dm = S.model_dir(a, d)[:, ax]
    neg = dm < 0
    assert_bitexact(pos, dm > 0, "positive mask")
    assert pos.sum() >= 1500 and neg.sum() >= 1500 and (~pos & ~neg).sum() == (0 if xf else 512)
    for accel in (0, 1):
        hit = S.degenerate_oracle(P, O, f"flat-{_flat_id(case)}", accel)[2] >= 0
        print(f"flat {_flat_id(case)} oracle accel={accel}: hit share positive {hit[pos].mean():.4f} "
              f"negative {hit[neg].mean():.4f}")
        if h == 0.0 and accel == 0:
            assert not hit[pos].any()
            assert hit[neg].mean() >= 0.99
        elif h == 0.0:
            assert hit[pos].mean() >= 0.99 and hit[neg].mean() >= 0.99
        else:
            assert hit[pos].mean() >= 0.9 and hit[neg].mean() >= 0.9


@pytest.mark.parametrize("xf", [False, True], ids=["id", "xf"])
def test_oracle_never_hits_the_needle(pt_mod, oracle_mod, xf):
    name = f"needle-{'xf' if xf else 'id'}"
    for accel in (0, 1):
        assert (S.degenerate_oracle(pt_mod, oracle_mod, name, accel)[2] == -1).all()


def _ridge_results(P, O, accel):
    n = S.RIDGE_RAYS
    out = {}
    for order in S.RIDGE_ORDERS:
        t, nrm, m = S.degenerate_oracle(P, O, f"ridge-{order}", accel)
        out[order] = (t[:n], nrm[:n], m[:n]), (t[n:], nrm[n:], m[n:])
    return out


@pytest.mark.parametrize("accel", [0, 1], ids=["grid", "exact"])
def test_ridge_rays_are_exact_ties_the_triangle_order_decides(pt_mod, oracle_mod, accel):
    """Every pair of triangle orders: on at least half of the on-ridge rays the
    oracle's t is bit-equal and the normal's z sign differs (a tie is shown); the
    winner is the side holding the lowest index among the triangles at the ridge
    point; off the ridge no ray changes with the order."""
    R = _ridge_results(pt_mod, oracle_mod, accel)
    for order in S.RIDGE_ORDERS:
        (t, nrm, m), (t2, nrm2, m2) = R[order]
        assert (m == 0).all() and (m2 == 0).all()
        assert_bitexact(np.sign(nrm[:, 2]), S.ridge_tie_sides(order).astype(np.float32), f"winning side, {order}")
    for a, b in itertools.combinations(S.RIDGE_ORDERS, 2):
        (ta, na, _), (ta2, na2, _) = R[a]
        (tb, nb, _), (tb2, nb2, _) = R[b]
        assert_bitexact(ta, tb, f"on-ridge t {a} vs {b}")
        share = (np.sign(na[:, 2]) != np.sign(nb[:, 2])).mean()
        print(f"ridge accel={accel} {a} vs {b}: tie share {share:.4f}")
        assert share >= 0.5
        assert_bitexact(ta2, tb2, f"off-ridge t {a} vs {b}")
        assert_bitexact(na2, nb2, f"off-ridge normal {a} vs {b}")


def test_ridge_rays_cover_boundaries_and_strips():
    on, off, d = S.ridge_rays()
    n = S.RIDGE_RAYS
    x = on[:, 0].astype(np.float64) / S.FLAT_SCALE
    w = 2 * S.FLAT_HALF / S.RIDGE_SEGMENTS
    s = (x + S.FLAT_HALF) / w
    assert (s[: n // 2] == np.round(s[: n // 2])).all() and len(np.unique(s[: n // 2])) == S.RIDGE_SEGMENTS // 2
    assert (s[n // 2:] != np.round(s[n // 2:])).all() and len(np.unique(np.floor(s[n // 2:]))) == S.RIDGE_SEGMENTS
    assert (on[:, 2] == 0).all() and (np.abs(off[:, 2]) == 2.0 ** -6).all() and (d == np.float32([0, -1, 0])).all()
    assert_bitexact(on[:, :2], off[:, :2], "control origins")


@pytest.mark.parametrize("where", S.COINCIDENT_AT)
@pytest.mark.parametrize("k", S.COINCIDENT_K)
def test_oracle_reports_the_lower_index_of_a_coincident_pair(pt_mod, oracle_mod, k, where):
    P, O = pt_mod, oracle_mod
    _, models, at = S.coincident_spec(k, where)
    assert len(models) == k + 2 and models[at]["material"] == "DIFFUSE" and models[at + 1]["material"] == "METAL"
    assert S.coincident_spec(k, where, swapped=True)[1][at]["material"] == "METAL"
    for accel in (0, 1):
        m_ab = S.degenerate_oracle(P, O, f"pair-{k}-{where}-ab", accel)[2]
        m_ba = S.degenerate_oracle(P, O, f"pair-{k}-{where}-ba", accel)[2]
        a_ab = S.degenerate_case(P, f"pair-{k}-{where}-ab")[0].export()
        a_ba = S.degenerate_case(P, f"pair-{k}-{where}-ba")[0].export()
        onp = (m_ab == at) | (m_ab == at + 1)
        assert onp.sum() >= 1000
        assert (m_ab[onp] == at).mean() >= 0.9
        # the same rays answer from the same place in model order: the other instance of the pair
        assert_bitexact(m_ba, m_ab, "model index, pair swapped")
        assert (a_ab["model_ints"][m_ab[onp], 2] != a_ba["model_ints"][m_ba[onp], 2]).all()
