"""The numpy restatement of the per-point normals (tests/fusion_normals_ref.py) pinned to geometry:
exact planes, orientation, depth staircases, the discontinuity gate, degenerate windows.  CPU only."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "aa-rmvsnet_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fusion_dedup_ref as dr  # noqa: E402
import fusion_normals_ref as nr  # noqa: E402

H, W = 48, 64
ULP = 2.0 ** -23            # one float32 ulp below 1
FRONTO, SLANT_A, SLANT_B = (0.0, 0.0, -1.0), (0.3, -0.2, -1.0), (-0.45, 0.35, -1.0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("n_cam", [FRONTO, SLANT_A, SLANT_B])
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_exact_planes_give_the_exact_normal(n_cam, radius):
    K, E = nr.camera(seed=3)
    depth = nr.plane_depth(K, H, W, n_cam, 600.0)
    normal, has = nr.estimate_normals(depth, np.ones((H, W), bool), (K, E), radius=radius)
    assert has.all()
    err = np.abs(normal.astype(np.float64) - nr.world_normal(E, n_cam)).max()
    assert err <= ULP, err


@pytest.mark.parametrize("n_cam", [FRONTO, SLANT_A, SLANT_B])
def test_exact_planes_at_the_far_corner_of_a_large_frame(n_cam):
    """A 48x64 window whose pixel coordinates run to (1599, 1183) of a 1600x1184 frame (principal point
    (800, 592), f = 1920): cabs = (c - a x0) - b y0 cancels most there."""
    K, E = nr.camera(f=1920.0, cx=800.0, cy=592.0, seed=4)
    origin = (1600 - W, 1184 - H)
    assert origin == (1536, 1136)
    depth = nr.plane_depth(K, H, W, n_cam, 600.0, origin)
    normal, has = nr.estimate_normals(depth, np.ones((H, W), bool), (K, E), origin=origin)
    assert has.all()
    err = np.abs(normal.astype(np.float64) - nr.world_normal(E, n_cam)).max()
    assert err <= ULP, err


def _centre(E):
    return np.linalg.inv(np.asarray(E, np.float64))[:3, 3]


def _faces_camera(xyz, nrm, E):
    return ((_centre(E) - xyz.astype(np.float64)) * nrm.astype(np.float64)).sum(-1)


def test_normals_face_the_camera_on_a_plane_and_on_a_sphere():
    K, E = nr.camera(seed=5)
    everything = np.ones((H, W), bool)
    depth = nr.plane_depth(K, H, W, SLANT_B, 600.0)
    normal, has = nr.estimate_normals(depth, everything, (K, E))
    xyz, _ = dr.fuse_points(depth, has, (K, E))
    assert has.all() and (_faces_camera(xyz, normal[has], E) > 0).all()
    depth, truth = nr.sphere_depth(K, H, W, (0.0, 0.0, 620.0), 80.0)
    on = np.isfinite(depth)
    assert 0.5 * H * W < on.sum() < H * W
    normal, has = nr.estimate_normals(depth, on, (K, E))
    xyz, _ = dr.fuse_points(np.where(on, depth, 0.0), has, (K, E))
    assert (_faces_camera(xyz, normal[has], E) > 0).all() and not has[~on].any()
    # only silhouette pixels (an off-sphere pixel among the 8 neighbours: grazing rays, the gate
    # leaves them alone) go without a normal
    pad = np.pad(on, 1, constant_values=True)
    inside = np.all([pad[1 + v:1 + v + H, 1 + u:1 + u + W] for v in (-1, 0, 1) for u in (-1, 0, 1)], axis=0)
    assert has[inside].all() and has.sum() > 0.99 * on.sum()
    # and they are the sphere's normals (prototype: median 0.03 degrees)
    Rw = np.linalg.inv(np.asarray(E, np.float32))[:3, :3].astype(np.float64)
    ang = nr.angle_deg(normal[has], truth[has] @ Rw.T)
    assert np.median(ang) < 0.1, np.median(ang)


def test_normals_face_the_camera_on_a_synthetic_scan():
    sc = dr.scene(40, 52, 2, 2)
    with np.errstate(all="ignore"):
        out = nr.fuse_views_normals(*sc, dedup=False)
    pairs, _, _, cams, _ = sc
    assert out["normals"].shape == out["xyz"].shape and out["xyz"].shape[0] > 0
    at = 0
    for ref, _ in pairs:
        final, has = out["masks"][ref]["final"], out["has_normal"][ref]
        n = out["counts"][ref]
        assert n == final.sum()
        xyz, nrm = out["xyz"][at:at + n], out["normals"][at:at + n]
        at += n
        got = nrm.any(axis=1)
        np.testing.assert_array_equal(got, has[final])
        assert got.mean() > 0.99                               # prototype: 99.9-100 % of the final pixels
        assert (_faces_camera(xyz[got], nrm[got], cams[ref][1]) > 0).all()
        np.testing.assert_allclose(np.linalg.norm(nrm[got].astype(np.float64), axis=1), 1.0, atol=2e-7)
        assert not has[~final].any()
    assert at == out["xyz"].shape[0]


def _staircase():
    K, E = nr.camera(seed=6)
    exact = nr.plane_depth(K, H, W, SLANT_A, 640.0)
    planes = 425.0 + 2.5 * np.arange(192)                      # 192 hypotheses, DTU's interval
    assert planes[0] < exact.min() and exact.max() < planes[-1]
    snapped = planes[np.abs(exact[..., None] - planes).argmin(-1)]
    return K, E, exact, snapped


def test_depth_staircases_fit_against_cross_product():
    """A slanted plane snapped to 192 depth hypotheses (2.5 apart at depth 640: steps a few pixels
    wide).  Median angular error over the interior pixels, measured here on the CPU: the
    inverse-depth fit 6.91 degrees at r = 1, 1.83 at r = 2, 0.58 at r = 3; the central-difference
    cross product 19.65 (the first prototype, on another plane: 1.07 at r = 2, 0.46 at r = 3, 8.8).
    The assertion is the comparison, not a threshold."""
    K, E, exact, snapped = _staircase()
    assert 10 < np.unique(snapped).size < 40
    truth_cam = np.asarray(SLANT_A) / np.linalg.norm(SLANT_A)
    inner = (slice(3, -3), slice(3, -3))
    cross = nr.angle_deg(nr.cross_product_normals(snapped, K)[inner], truth_cam)
    med_cross = float(np.median(cross))
    meds = {}
    for r in (1, 2, 3):
        normal, has = nr.estimate_normals(snapped, np.ones((H, W), bool), (K, E), radius=r)
        assert has.all()
        meds[r] = float(np.median(nr.angle_deg(normal[inner], nr.world_normal(E, SLANT_A))))
    print(f"staircase: median angular error fit r=1/2/3 {meds[1]:.2f}/{meds[2]:.2f}/{meds[3]:.2f} deg, "
          f"cross product {med_cross:.2f} deg")
    assert meds[2] < med_cross and meds[3] < med_cross and meds[1] < med_cross


def test_the_gate_keeps_windows_from_straddling_a_depth_step():
    K, E = nr.camera(seed=7)
    near, far = nr.plane_depth(K, H, W, SLANT_B, 600.0), nr.plane_depth(K, H, W, SLANT_B, 630.0)
    depth = near.copy()
    depth[:, W // 2:] = far[:, W // 2:]                        # a 5 % step, the same normal on both sides
    everything = np.ones((H, W), bool)
    for r in (1, 2, 3):
        normal, has = nr.estimate_normals(depth, everything, (K, E), radius=r, max_rel_jump=0.01)
        assert has.all()
        assert np.abs(normal.astype(np.float64) - nr.world_normal(E, SLANT_B)).max() <= ULP
    # without the gate the windows at the step mix the two planes
    normal, has = nr.estimate_normals(depth, everything, (K, E), max_rel_jump=0.1)
    ang = nr.angle_deg(normal, nr.world_normal(E, SLANT_B))
    assert ang[:, W // 2 - 2:W // 2 + 2].min() > 1.0 and ang[:, :W // 2 - 2].max() < 0.05


def test_degenerate_windows():
    K, E = nr.camera(seed=8)
    depth = nr.plane_depth(K, H, W, SLANT_A, 600.0)
    # one valid row: N >= 3 but the pixels are collinear (det == 0)
    row = np.zeros((H, W), bool)
    row[20] = True
    normal, has = nr.estimate_normals(depth, row, (K, E), radius=3)
    assert not has.any() and not normal.any()
    col = np.zeros((H, W), bool)
    col[:, 31] = True
    assert not nr.estimate_normals(depth, col, (K, E), radius=2)[1].any()
    diag = np.eye(H, W, dtype=bool)
    assert not nr.estimate_normals(depth, diag, (K, E), radius=2)[1].any()
    # two valid pixels
    two = np.zeros((H, W), bool)
    two[10, 10] = two[11, 11] = True
    assert not nr.estimate_normals(depth, two, (K, E))[1].any()
    # three that are not collinear: every one of them has the plane's normal
    three = two.copy()
    three[10, 11] = True
    normal, has = nr.estimate_normals(depth, three, (K, E))
    np.testing.assert_array_equal(has, three)
    assert np.abs(normal[three].astype(np.float64) - nr.world_normal(E, SLANT_A)).max() <= ULP


@pytest.mark.parametrize("bad", [np.nan, np.inf, 0.0, -600.0])
def test_an_unusable_depth_has_no_normal_and_feeds_no_fit(bad):
    K, E = nr.camera(seed=9)
    rng = np.random.default_rng(1)
    depth = nr.plane_depth(K, H, W, SLANT_A, 600.0) * (1.0 + 0.002 * rng.standard_normal((H, W)))
    spots = [(0, 0), (H - 1, W - 1), (0, 17), (23, 0), (20, 30)]        # corners, edges, interior
    planted = depth.copy()
    for y, x in spots:
        planted[y, x] = bad
    masked = np.ones((H, W), bool)
    for y, x in spots:
        masked[y, x] = False
    got_n, got_h = nr.estimate_normals(planted, np.ones((H, W), bool), (K, E))
    want_n, want_h = nr.estimate_normals(depth, masked, (K, E))
    for y, x in spots:
        assert not got_h[y, x] and not got_n[y, x].any()
    np.testing.assert_array_equal(got_h, want_h)
    np.testing.assert_array_equal(_bits(got_n), _bits(want_n))
    assert got_h.sum() == H * W - len(spots)


def test_raising_min_count_only_removes_normals():
    K, E = nr.camera(seed=10)
    rng = np.random.default_rng(2)
    depth = nr.plane_depth(K, H, W, SLANT_B, 600.0) * (1.0 + 0.002 * rng.standard_normal((H, W)))
    valid = rng.random((H, W)) > 0.6                           # 60 % holes: sparse windows
    base_n, base_h = nr.estimate_normals(depth, valid, (K, E), min_count=3)
    counts = [int(base_h.sum())]
    for mc in (6, 12, 25):
        n, h = nr.estimate_normals(depth, valid, (K, E), min_count=mc)
        assert not (h & ~base_h).any()
        np.testing.assert_array_equal(_bits(n[h]), _bits(base_n[h]))
        assert not n[~h].any()
        counts.append(int(h.sum()))
    assert counts[0] > counts[1] > counts[2] > counts[3] == 0
