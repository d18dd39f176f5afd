"""The cases of tests/fusion_edge_cases.py say what tests/test_gpu_fusion_edge.py believes they say
(CPU only: the numpy oracle and the host-side packing, no kernel):

* ``edge_views`` with the plain cameras is ``synthetic.fusion_views`` bit for bit, the other kinds have
  the cameras they are named for (every intrinsic entry differs per view; inv(E) of the ``pose`` /
  ``both`` views has no identity row or column and t_z != 0);
* non-vacuity: the views of ``intrinsics``, ``pose`` and ``both`` still see one surface (geo >= 0.5),
  ``behind``'s turned view has the scene behind it for a share of the reference pixels in [0.1, 0.9] and
  sends at least one float32 coordinate into remap_linear's branch for non-finite / |32 v| >= 2^31
  values, ``bad_maps`` holds each of its ten values in every map, the four leading photo values are
  F, F, T, T and depth_avg carries NaN and infinities;
* discrimination: on the per-view intrinsics, taking the reference's K for the sources' (or a source's
  for the reference's) changes geo and depth_avg; on ``synthetic.fusion_views`` neither changes a
  single value, which is why these cases exist;
* ``pack_cameras`` and ``pack_point_cameras`` on the ``both`` cameras: every block of every view is the
  numpy expression it restates;
* the Tanks and Temples restatement of the filter core runs on ``both`` with 10 source views and
  agrees with the oracle's; ``save_pfm`` / ``read_pfm`` keep NaN and -0.0.

The measured shares: profiles/fusion_edge_cases.txt (``python tests/fusion_edge_cases.py``).
"""
import numpy as np
import pytest

import fusion_edge_cases as ec
import fusion_tnt_ref as tr
from aarmvs import fusion, synthetic as syn

REGULAR = [c for c in ec.CASES if not c.name.startswith("thin")]
BEHIND = [c for c in ec.CASES if c.kind == "behind"]
BAD = [c for c in ec.CASES if c.bad]


# ---------------------------------------------------------------------------------
# the generator and the case table
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,nsrc,seed", [(40, 52, 4, 1), (36, 52, 10, 30), (1, 7, 2, 0), (5, 1, 1, 3)])
def test_plain_kind_is_fusion_views(H, W, nsrc, seed):
    a, b = ec.edge_views(H, W, nsrc, "plain", seed), syn.fusion_views(H, W, nsrc, seed=seed)
    for x, y in zip(a[0], b[0]):
        assert x.dtype == y.dtype == np.float32 and x.tobytes() == y.tobytes()
    for (K, E), (K2, E2) in zip(a[1], b[1]):
        assert K.dtype == E.dtype == np.float32 and K.tobytes() == K2.tobytes() and E.tobytes() == E2.tobytes()
    assert a[2].tobytes() == b[2].tobytes()


def test_case_table_is_the_agreed_one():
    t = {c.name: (c.H, c.W, c.nsrc, c.kind, c.bad) for c in ec.CASES}
    for k in ("intrinsics", "pose", "both", "behind"):
        assert t[k] == (40, 52, 4, k, False)
    assert t["both_n10"] == (40, 52, 10, "both", False) and t["behind_n10"] == (40, 52, 10, "behind", False)
    assert t["both_75x101"] == (75, 101, 4, "both", False) and (75 * 101) % 256 != 0
    for k in ("intrinsics", "both", "behind"):
        assert t["bad_" + k] == (40, 52, 4, k, True)
    thin = {(c.H, c.W, c.nsrc) for c in ec.CASES if c.name.startswith("thin")}
    assert thin == {(h, w, n) for h, w in ((1, 1), (1, 7), (5, 1), (2, 3)) for n in (1, 2)}
    assert all(c.kind == "intrinsics" and not c.bad for c in ec.CASES if c.name.startswith("thin"))
    assert all(c.seed == 1 for c in ec.CASES) and len(ec.CASES) == len(ec.BY_NAME) == 18
    # every frame but the one that is no multiple of 256 is 40 x 52 or smaller
    assert all(c.H * c.W <= 40 * 52 for c in ec.CASES if c.name != "both_75x101")
    assert set(ec.FILTER_CASES) == set(ec.BY_NAME)
    assert ec.PHOTO_THRESHOLD == 0.35 and ec.BAD_REPEAT == 10 and len(ec.BAD_VALUES) == 10
    v = np.array(ec.BAD_VALUES, np.float32)
    assert np.isnan(v[0]) and v[1] == np.inf and v[2] == -np.inf and not np.signbit(v[3]) and np.signbit(v[4])
    assert v[3] == 0 and v[4] == 0 and v[5] == -600 and np.isfinite(v[8]) and v[8] > 3e38
    assert 0 < v[9] < np.finfo(np.float32).tiny and 0 < v[7] and v[6] == np.float32(1e30)   # 1e-42: a denormal


def test_cameras_are_what_the_kinds_are_named_for():
    H, W, nsrc = 40, 52, 4
    for kind in ("intrinsics", "both"):
        cams = ec.cameras(H, W, nsrc, kind)
        for v, (K, _) in enumerate(cams):
            u = v - nsrc / 2
            fx = 1.2 * W * (1 + 0.07 * u)
            np.testing.assert_array_equal(K, np.array([[fx, 0, W / 2 + 3 * v], [0, 1.03 * fx, H / 2 - 2 * v],
                                                       [0, 0, 1]], np.float32))
        for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)):     # every intrinsic entry differs from view to view
            assert len({float(K[i, j]) for K, _ in cams}) == nsrc + 1
        assert all(K[0, 0] != K[1, 1] for K, _ in cams)
    for kind in ("plain", "pose", "behind"):
        cams = ec.cameras(H, W, nsrc, kind)
        assert all(np.array_equal(K, cams[0][0]) for K, _ in cams)
    for kind in ("pose", "both"):
        for v, (_, E) in enumerate(ec.cameras(H, W, nsrc, kind)):
            u = v - nsrc / 2
            np.testing.assert_array_equal(E[:3, 3], np.array([-30 * u, 12 * u, 25 * u], np.float32))
            R = E[:3, :3].astype(np.float64)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and np.linalg.det(R) > 0.999
            if u != 0:
                # a rotation about all three axes: inv(E) has no row or column of the identity
                assert np.abs(np.linalg.inv(E)[:3, :3] - np.eye(3)).min() > 1e-4 and E[2, 3] != 0
    # the old poses: y row and column of the identity, t_z = 0
    for _, E in ec.cameras(H, W, nsrc, "intrinsics"):
        assert E[1, 1] == 1 and E[0, 1] == E[1, 0] == E[1, 2] == E[2, 1] == 0 and E[2, 3] == 0
    _, E = ec.cameras(H, W, nsrc, "behind")[nsrc]
    np.testing.assert_array_equal(E[:3, 3], np.zeros(3, np.float32))
    assert E[0, 2] == np.float32(np.sin(1.45)) and E[0, 0] == np.float32(np.cos(1.45))


# ---------------------------------------------------------------------------------
# non-vacuity
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in REGULAR if c.kind in ("intrinsics", "pose", "both")])
def test_the_views_still_see_one_surface(name):
    case = ec.BY_NAME[name]
    photo, geo, final, avg = ec.reference(case)
    print(f"\n{name}: geo {geo.mean():.4f} final {final.mean():.4f}")
    assert geo.mean() >= 0.5
    np.testing.assert_array_equal(final, photo & geo)
    assert avg.dtype == np.float64 and geo.dtype == photo.dtype == np.bool_


@pytest.mark.parametrize("name", [c.name for c in BEHIND])
def test_behind_has_the_scene_behind_the_turned_view(name):
    case = ec.BY_NAME[name]
    kz, xs, ys = ec.source_coordinates(case, case.nsrc)
    with np.errstate(invalid="ignore"):
        share = float((kz <= 0).mean())
    neg = float((ec.inputs(case)[0][case.nsrc] < 0).mean())
    print(f"\n{name}: kz <= 0 on {share:.4f}, turned view's depth negative on {neg:.4f}")
    assert 0.1 <= share <= 0.9 and 0.1 <= neg <= 0.9
    # the other source views have the whole scene in front of them
    for v in range(1, case.nsrc):
        kz_v = ec.source_coordinates(case, v)[0]
        ok = np.isfinite(kz_v) & (ec.inputs(case)[0][0].reshape(-1) > 0)
        assert (kz_v[ok] > 0).all()


@pytest.mark.parametrize("name", ["behind", "bad_behind", "bad_both"])
def test_coordinates_reach_the_fixed_point_overflow_branch(name):
    """At least one float32 source coordinate is +-inf, NaN or has |32 v| >= 2^31: the branch of
    remap_linear's to_fixed that the oracle takes by an int64 cast."""
    case = ec.BY_NAME[name]
    n = nonfinite = 0
    for v in range(1, case.nsrc + 1):
        for c in ec.source_coordinates(case, v)[1:]:
            assert c.dtype == np.float32
            n += int(ec.outside_fixed_point(c).sum())
            nonfinite += int((~np.isfinite(c)).sum())
    print(f"\n{name}: {n} coordinates outside the fixed-point range, {nonfinite} of them not finite")
    assert n >= 1
    if case.bad:                    # NaN, +-inf and 0 depths: 0 / 0 and x / 0
        assert nonfinite >= 1
    if case.kind == "behind":       # kz next to 0: finite, and too large for the 1/32-pixel grid
        assert n > nonfinite


@pytest.mark.parametrize("name", [c.name for c in BAD])
def test_bad_maps_hold_every_value_and_reach_the_outputs(name):
    case = ec.BY_NAME[name]
    depths, _, conf = ec.inputs(case)
    assert len(depths) == case.nsrc + 1
    for d in depths:
        for value in ec.BAD_VALUES:
            n = ec.holds(d, value)
            assert n >= ec.BAD_REPEAT if value == 0.0 and not np.signbit(value) else n == ec.BAD_REPEAT, value
    thr = np.float32(ec.PHOTO_THRESHOLD)
    head = conf.reshape(-1)[:4]
    assert np.isnan(head[0]) and head[1] == thr and head[2] > thr and head[3] == np.inf
    assert np.nextafter(head[2], np.float32(0)) == thr
    photo, geo, final, avg = ec.reference(case)
    assert photo.reshape(-1)[:4].tolist() == [False, False, True, True]
    assert np.isnan(avg).sum() >= 1 and np.isinf(avg).sum() >= 1
    s = ec.shares(case)
    print(f"\n{name}: {s}")
    if name == "bad_intrinsics":     # the record of the measurement the cases were agreed on
        assert 0.55 <= s["geo"] <= 0.65 and (s["avg_nan"], s["avg_inf"], s["final_bad_avg"]) == (10, 20, 0)


@pytest.mark.parametrize("name", [c.name for c in ec.CASES if c.name.startswith("thin")])
def test_the_oracle_runs_on_the_thin_frames(name):
    case = ec.BY_NAME[name]
    photo, geo, final, avg = ec.reference(case)
    assert photo.shape == geo.shape == final.shape == avg.shape == (case.H, case.W)
    # the shifted principal points put every source coordinate's bilinear taps at least partly
    # outside these frames: nothing is consistent, the average is the reference depth itself
    assert not geo.any()
    np.testing.assert_array_equal(avg, ec.inputs(case)[0][0].astype(np.float64))


# ---------------------------------------------------------------------------------
# discrimination
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in REGULAR if c.kind in ("intrinsics", "both")])
def test_a_K_taken_from_the_wrong_view_is_seen(name):
    case = ec.BY_NAME[name]
    depths, cams, conf = ec.inputs(case)
    _, geo, _, avg = ec.reference(case)
    for what, swap in (("source K <- reference K", ec.swap_source_K), ("reference K <- source K", ec.swap_reference_K)):
        _, geo2, _, avg2 = ec.oracle_filter(depths, swap(cams), conf)
        dg, da = ec.changed(geo2, geo), ec.changed(avg2, avg)
        print(f"\n{name}: {what} changes {dg} of {geo.size} geo pixels and {da} averages")
        assert dg >= geo.size // 10 and da >= geo.size // 10


def test_the_old_scene_cannot_see_a_K_from_the_wrong_view():
    H, W, nsrc, seed = ec.OLD_SCENE
    depths, cams, conf = syn.fusion_views(H, W, nsrc, seed=seed)
    ref = ec.oracle_filter(depths, cams, conf)
    for swap in (ec.swap_source_K, ec.swap_reference_K):
        got = ec.oracle_filter(depths, swap(cams), conf)
        for g, r in zip(got, ref):
            assert ec.changed(g, r) == 0
    # the same holds for the shared-K kinds of the new generator: they are there for the poses
    for name in ("pose", "behind"):
        d, c, cf = ec.inputs(ec.BY_NAME[name])
        assert ec.changed(ec.oracle_filter(d, ec.swap_source_K(c), cf)[3], ec.reference(ec.BY_NAME[name])[3]) == 0


# ---------------------------------------------------------------------------------
# the packing
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["both", "both_n10"])
def test_pack_cameras_block_by_block(name):
    case = ec.BY_NAME[name]
    _, cams, _ = ec.inputs(case)
    (K_ref, E_ref), srcs = cams[0], cams[1:]
    p = fusion.pack_cameras(cams[0], srcs)
    assert p.dtype == np.float32 and p.flags["C_CONTIGUOUS"] and p.size == 18 + 42 * case.nsrc
    np.testing.assert_array_equal(p[0:9], np.linalg.inv(K_ref).ravel())
    np.testing.assert_array_equal(p[9:18], K_ref.ravel())
    blocks = [p[0:9].tobytes(), p[9:18].tobytes()]
    for v, (K, E) in enumerate(srcs):
        c = p[18 + 42 * v:18 + 42 * (v + 1)]
        assert K.dtype == E.dtype == np.float32
        np.testing.assert_array_equal(c[0:9], K.ravel())
        np.testing.assert_array_equal(c[9:18], np.linalg.inv(K).ravel())
        np.testing.assert_array_equal(c[18:30], np.matmul(E, np.linalg.inv(E_ref))[:3].ravel())
        np.testing.assert_array_equal(c[30:42], np.matmul(E_ref, np.linalg.inv(E))[:3].ravel())
        blocks += [c[0:9].tobytes(), c[9:18].tobytes(), c[18:30].tobytes(), c[30:42].tobytes()]
    # no two blocks are the same bytes: a block read from another block's place is another matrix
    assert len(set(blocks)) == len(blocks) == 2 + 4 * case.nsrc
    for K, E in cams:
        q = fusion.pack_point_cameras((K, E))
        assert q.dtype == np.float32 and q.size == 25 and q.flags["C_CONTIGUOUS"]
        np.testing.assert_array_equal(q[:9], np.linalg.inv(K).ravel())
        np.testing.assert_array_equal(q[9:], np.linalg.inv(E).ravel())


# ---------------------------------------------------------------------------------
# the other restatements and the files
# ---------------------------------------------------------------------------------
def test_tnt_restatement_on_both_cameras_with_ten_views():
    case = ec.BY_NAME["both_n10"]
    want = ec.reference(case)
    got = ec.oracle_filter(*ec.inputs(case), core=tr.filter_depth_core)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    assert got[3].dtype == np.float64 and want[1].mean() >= 0.5


def test_scan_for_the_drivers():
    pairs, depths, confs, cams, images = ec.scan()
    H, W, nsrc, _ = ec.SCAN
    assert sorted(depths) == sorted(confs) == sorted(cams) == sorted(images) == list(range(nsrc + 1))
    assert [r for r, _ in pairs] == list(range(nsrc + 1)) and all(len(s) == nsrc and r not in s for r, s in pairs)
    for v in depths:
        assert depths[v].shape == confs[v].shape == (H, W) and images[v].shape == (H, W, 3)
        for value in ec.BAD_VALUES:
            assert ec.holds(depths[v], value) >= ec.BAD_REPEAT
        assert np.isnan(confs[v][0, 0]) and confs[v][0, 3] == np.inf
    for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)):
        assert len({float(cams[v][0][i, j]) for v in cams}) == nsrc + 1
    with np.errstate(all="ignore"):
        import fusion_dedup_ref as dr
        want = dr.fuse_views(pairs, depths, confs, cams, images, ec.PHOTO_THRESHOLD, dedup=True)
    finals = sum(int(m["final"].sum()) for m in want["masks"].values())
    print(f"\nscan: {finals} final pixels, {want['xyz'].shape[0]} emitted with the de-duplication")
    assert 100 <= want["xyz"].shape[0] < finals


def test_pfm_keeps_nan_and_negative_zero(tmp_path):
    m = np.array(ec.BAD_VALUES + (1.5, -2.5), np.float32).reshape(3, 4)
    fusion.save_pfm(str(tmp_path / "m.pfm"), m)
    back, scale = fusion.read_pfm(str(tmp_path / "m.pfm"))
    assert scale == 1.0 and back.dtype == np.float32 and back.shape == m.shape
    # bit patterns: NaN stays NaN, -0.0 keeps its sign, the denormal is not flushed
    np.testing.assert_array_equal(np.ascontiguousarray(back).view(np.uint32), m.view(np.uint32))
    assert np.isnan(back[0, 0]) and np.signbit(back[1, 0]) and back[1, 0] == 0 and back[2, 1] == np.float32(1e-42)
