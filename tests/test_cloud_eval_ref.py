"""The point-cloud evaluation's numpy restatement (tests/cloud_eval_ref.py) against
scipy.spatial.cKDTree: the yardstick of the GPU tests is checked here, on the CPU, first."""
import math

import numpy as np
import pytest
from scipy.spatial import cKDTree

import cloud_eval_ref as ref


def _clouds(seed, nq, m, scale=10.0):
    rng = np.random.default_rng(seed)
    return (rng.random((nq, 3)) * scale).astype(np.float32), (rng.random((m, 3)) * scale).astype(np.float32)


@pytest.mark.parametrize("max_dist", [0.25, 0.6, 3.0])
def test_brute_force_neighbour_equals_ckdtree(max_dist):
    q, t = _clouds(1, 1500, 2500)
    origin, cell = ref.grid_for([q, t], max_dist)
    dist, index = ref.nn(q, t, origin, cell, max_dist)
    d_kd, i_kd = cKDTree(t.astype(np.float64)).query(q.astype(np.float64), k=1, distance_upper_bound=max_dist)
    found = np.isfinite(d_kd)
    # cKDTree's bound is exclusive and ours inclusive: no random distance sits exactly on it
    assert 0 < found.sum() and (max_dist > 1 or found.sum() < q.shape[0])
    np.testing.assert_array_equal(np.isfinite(dist), found)
    np.testing.assert_array_equal(dist[found], d_kd[found].astype(np.float32))
    np.testing.assert_array_equal(index[found], i_kd[found])   # random data: the minimum is unique
    assert np.isinf(dist[~found]).all() and (dist[~found] > 0).all() and (index[~found] == -1).all()


def test_ties_go_to_the_lowest_id_and_ids_are_honoured():
    t = np.array([[1, 0, 0], [-1, 0, 0], [1, 0, 0], [0, 5, 0]], np.float32)
    q = np.array([[0, 0, 0], [1, 0, 0], [0, 4, 0]], np.float32)
    origin, cell = np.array([-1.0, 0, 0]), 1.0
    d, i = ref.nn(q, t, origin, cell, 2.0)
    np.testing.assert_array_equal(d, np.float32([1, 0, 1]))
    np.testing.assert_array_equal(i, [0, 0, 3])
    d, i = ref.nn(q, t, origin, cell, 2.0, target_ids=[7, 3, 5, 9])
    np.testing.assert_array_equal(i, [3, 5, 9])
    # inclusive at max_dist, +inf / -1 beyond it, NaN for a non-finite query, +inf outside the grid
    q2 = np.array([[0, 7, 0], [0, 7.5, 0], [np.nan, 0, 0], [np.inf, 0, 0], [-5, 0, 0]], np.float32)
    d, i = ref.nn(q2, t, origin, cell, 2.0)
    assert d[0] == 2.0 and i[0] == 3 and np.isposinf(d[1]) and np.isnan(d[2]) and np.isnan(d[3]) and np.isposinf(d[4])
    np.testing.assert_array_equal(i[1:], -1)
    # targets outside the grid are no neighbours
    d, i = ref.nn(np.float32([[-1, 0, 0]]), np.float32([[-1.5, 0, 0], [np.nan, 0, 0], [0, 0, 0]]), origin, cell, 2.0)
    assert d[0] == 1.0 and i[0] == 2


def test_keys_and_the_row_contiguity_property():
    """x in the low bits: after sorting by key, the points of the cells (i_x - r .. i_x + r, i_y, i_z)
    are one contiguous span, for every row and every r."""
    rng = np.random.default_rng(2)
    p = (rng.random((4000, 3)) * 6).astype(np.float32)
    origin, cell = np.zeros(3), 0.75
    i, ok = ref.cells(p, origin, cell)
    k = ref.keys(p, origin, cell)
    assert ok.all()
    np.testing.assert_array_equal(k, (i[:, 2] << 42) | (i[:, 1] << 21) | i[:, 0])
    order = np.argsort(k, kind="stable")
    si = i[order]
    for (cx, cy, cz, r) in [(3, 2, 5, 1), (0, 0, 0, 2), (7, 7, 7, 3), (4, 6, 1, 8)]:
        hit = np.nonzero((si[:, 1] == cy) & (si[:, 2] == cz) & (np.abs(si[:, 0] - cx) <= r))[0]
        assert hit.size and (np.diff(hit) == 1).all()
        base = (cz << 42) | (cy << 21)
        lo = np.searchsorted(k[order], base | max(cx - r, 0), "left")
        hi = np.searchsorted(k[order], base | (cx + r), "right")
        assert (lo, hi) == (hit[0], hit[-1] + 1)
    # outside the grid, non-finite, and the two ends of an axis
    edge = np.float32([[-0.1, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, 0], [1e30, 0, 0]])
    np.testing.assert_array_equal(ref.keys(edge, origin, cell), [ref.NO_KEY, ref.NO_KEY, ref.NO_KEY, 0, ref.NO_KEY])
    far = np.float32([[(1 << 21) - 1, 0, 0], [1 << 21, 0, 0], [0, (1 << 21) - 1, 5]])
    np.testing.assert_array_equal(ref.keys(far, origin, 1.0),
                                  [(1 << 21) - 1, ref.NO_KEY, (5 << 42) | (((1 << 21) - 1) << 21)])


def test_stats_and_the_fixed_order_sum():
    rng = np.random.default_rng(3)
    d = rng.random(10000).astype(np.float32) * 3
    d[::7] = np.inf
    d[::11] = np.nan
    st = ref.stats(d, (1.0, 2.5))
    fin = np.isfinite(d)
    assert st[0] == fin.sum() and st[2] == np.isnan(d).sum()
    assert st[3] == (d[fin] < 1.0).sum() and st[4] == (d[fin] < 2.5).sum()
    assert st[1] == math.fsum(float(v) for v in d[fin])
    assert abs(ref.fixed_order_sum(d) - st[1]) <= 1e-12 * st[1]
    assert ref.fixed_order_sum(np.float32([])) == 0.0 and ref.fixed_order_sum(np.float32([np.nan, 2.5])) == 2.5


def test_voxel_centroids_restated():
    p = np.float32([[0.1, 0.1, 0.1], [2.5, 0, 0], [0.3, 0.2, 0.9], [np.nan, 0, 0], [0.2, 0.9, 0.5], [1.0, 0, 0]])
    out = ref.voxel_centroids(p, np.zeros(3), 1.0)
    want0 = ((p[0].astype(np.float64) + p[2]) + p[4]) / 3.0
    np.testing.assert_array_equal(out, np.stack([want0.astype(np.float32), p[5], p[1]]))


def test_ground_truth_cloud_is_the_noise_free_scan():
    """fusion_ground_truth's points project back to their pixels at fusion_views' noise-free depth;
    fusion_views itself is untouched (its digest is pinned by the fusion tests)."""
    from aarmvs import synthetic as syn
    H, W, nsrc = 24, 36, 2
    depths, cams, _ = syn.fusion_views(H, W, nsrc, seed=0)
    gt = syn.fusion_ground_truth(H, W, nsrc)
    assert gt.dtype == np.float32 and gt.shape == ((nsrc + 1) * H * W, 3)
    ys, xs = np.mgrid[0:H, 0:W]
    for v, (K, E) in enumerate(cams):
        pw = gt[v * H * W:(v + 1) * H * W].astype(np.float64)
        pc = E[:3, :3].astype(np.float64) @ pw.T + E[:3, 3:4].astype(np.float64)
        uv = K.astype(np.float64) @ pc
        np.testing.assert_allclose(uv[0] / uv[2], xs.ravel(), atol=2e-3)
        np.testing.assert_allclose(uv[1] / uv[2], ys.ravel(), atol=2e-3)
        d = depths[v].ravel()
        seen = d > 0
        # the scan's depth is this one plus N(0, 0.3) noise: within 6 sigma, and unbiased
        assert np.abs(d[seen] - pc[2][seen]).max() < 2.0 and abs((d[seen] - pc[2][seen]).mean()) < 0.05
    # on the surface z = 600 + 0.05 x, up to the bumps (4 units of depth along the ray)
    assert np.abs(gt[:, 2] - (600.0 + 0.05 * gt[:, 0])).max() < 4.5


def test_evaluate_restated_on_a_case_worked_out_by_hand():
    recon, gt, max_dist, taus, want = ref.hand_case()
    got = ref.evaluate(recon, gt, max_dist, taus)
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-15, abs=0), k
    # no point within reach: every share is 0 and F is 0, not 0 / 0
    far = ref.evaluate(np.float32([[0, 0, 0]]), np.float32([[50, 0, 0]]), 2.0, (1.0,))
    assert far["precision@1"] == far["recall@1"] == far["fscore@1"] == 0.0
    assert np.isnan(far["accuracy_mean"]) and far["recon_beyond_max_dist"] == far["gt_beyond_max_dist"] == 1
