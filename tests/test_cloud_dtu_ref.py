"""The DTU protocol's numpy restatement (tests/cloud_dtu_ref.py) checked on the CPU: the round rule
against the literal sequential walk, the walk against a cKDTree walk where d2 is exact, the region
tests on hand-worked points, the readers of the dataset's files, and mutants of the round rule that
the cases of tests/test_gpu_cloud_dtu.py tell apart."""
import numpy as np
import pytest

import cloud_dtu_ref as dtu

R = dtu.R


def _cases():
    line = dtu.line()
    rng = np.random.default_rng(5)
    mixed = dtu.lattice_cloud(4, 600, seed=3)
    mixed[::37, 1], mixed[5, 0], mixed[9, 2] = np.nan, np.inf, -np.inf
    return {
        "sparse_random": (dtu.lattice_cloud(12), "random"),
        "sparse_input": (dtu.lattice_cloud(12), "input"),
        "dense_random": (dtu.lattice_cloud(6), "random"),
        "dense_input": (dtu.lattice_cloud(6), "input"),
        "raster_input": (dtu.raster_plane(), "input"),
        "raster_random": (dtu.raster_plane(), "random"),
        "line_input": (line, "input"),
        "line_random": (line, "random"),
        "copies": (np.tile(np.float32([[1.25, -2, 3]]), (1000, 1)), "random"),
        "negative": ((rng.integers(-9, 10, (3000, 3)) * 0.25).astype(np.float32), "random"),
        "non_finite": (mixed, "random"),
    }


CASES = _cases()


@pytest.fixture(scope="module")
def solved():
    """Per case: (xyz, rank, kept by the walk, kept by the rounds, rounds), computed once."""
    out = {}
    for name, (xyz, order) in CASES.items():
        rank = dtu.ranks_of(order, 0, xyz.shape[0])
        out[name] = (xyz, rank, dtu.thin_sequential(xyz, R, rank)) + dtu.thin_rounds(xyz, R, rank)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_the_rounds_give_the_sequential_walk(solved, name):
    xyz, rank, seq, par, rounds = solved[name]
    np.testing.assert_array_equal(par, seq)
    assert 1 <= rounds <= xyz.shape[0] and 0 < seq.sum() <= xyz.shape[0]


@pytest.mark.parametrize("name", list(CASES))
def test_the_kept_set_is_independent_and_maximal(solved, name):
    xyz, rank, kept, _, _ = solved[name]
    a, b = dtu.neighbour_pairs(xyz, R)
    assert not (kept[a] & kept[b]).any()                       # no two kept points within r
    covered = np.zeros(xyz.shape[0], bool)
    ok = kept[b] & (rank[b] < rank[a])
    covered[a[ok]] = True                                      # a kept lower-ranked neighbour
    dropped = ~kept & np.isfinite(xyz).all(1)
    assert dropped.any() and covered[dropped].all()
    assert not kept[~np.isfinite(xyz).all(1)].any()


@pytest.mark.parametrize("name", ["sparse_random", "dense_input", "raster_input", "line_input", "copies", "negative"])
def test_the_walk_equals_a_ckdtree_walk_where_d2_is_exact(solved, name):
    """On the quarter lattice with r = 0.75 every d2 is exact in float64, so the tree's 'within r'
    (inclusive) is the definition's."""
    from scipy.spatial import cKDTree
    xyz, rank, kept, _, _ = solved[name]
    p = xyz.astype(np.float64)
    tree = cKDTree(p)
    gone, want = np.zeros(p.shape[0], bool), np.zeros(p.shape[0], bool)
    for i in np.argsort(rank):
        if not gone[i]:
            want[i] = True
            gone[tree.query_ball_point(p[i], R)] = True
    np.testing.assert_array_equal(kept, want)


def test_round_counts(solved):
    """The line in input order decides one point per round: exactly n rounds, the hard upper bound.
    The same line in a random order, and random clouds, stay far below."""
    assert solved["line_input"][4] == 256
    assert solved["line_random"][4] <= 32
    assert solved["raster_input"][4] > 100 and solved["raster_random"][4] <= 32
    for name in ("sparse_random", "sparse_input", "dense_random", "dense_input"):
        assert solved[name][4] <= 40, name
    assert solved["copies"][4] == 2 and solved["copies"][2].sum() == 1
    assert solved["copies"][2][np.argmin(solved["copies"][1])]          # the lowest rank survives


def test_a_pair_exactly_at_r_and_one_just_beyond():
    r = np.float32(0.75)
    beyond = np.nextafter(r, np.float32(2))
    for gap, n_kept in ((r, 1), (beyond, 2)):
        xyz = np.float32([[1, 0, 3], [1, gap, 3]])      # the difference is the gap itself, exactly
        kept = dtu.thin_sequential(xyz, r, [0, 1])
        assert kept.sum() == n_kept and kept[0]
        np.testing.assert_array_equal(dtu.thin_rounds(xyz, r, [0, 1])[0], kept)


@pytest.mark.parametrize("rule", ["ignore_rank", "undecided_as_removed"])
@pytest.mark.parametrize("name", ["line_input", "raster_input"])
def test_mutants_of_the_round_rule_give_another_set(solved, name, rule):
    """A rule that ignores rank, or takes an undecided lower neighbour for a removed one, is told
    apart by the line and the raster: the GPU test on these cases is not vacuous."""
    xyz, rank, kept, _, _ = solved[name]
    mutant, _ = dtu.thin_rounds(xyz, R, rank, rule=rule, max_rounds=300)
    assert (mutant != kept).any()


# --------------------------------------------------------------------------------- regions
def test_regions_on_points_worked_out_by_hand():
    pts, mask, bb, res, patch, plane, want = dtu.hand_regions()
    got = dtu.regions(pts, mask, bb, res, patch, plane)
    np.testing.assert_array_equal(got, want)
    # the forms without a mask, a box or a plane
    np.testing.assert_array_equal(dtu.regions(pts, None, bb, None, patch, plane), got & 5)
    np.testing.assert_array_equal(dtu.regions(pts, mask, bb, res, patch), got & 3)
    np.testing.assert_array_equal(dtu.regions(pts, plane=plane), got & 4)


# --------------------------------------------------------------------------------- the dataset's files
def _mask_file_contents():
    rng = np.random.default_rng(8)
    mask = rng.random((5, 4, 3)) < 0.5
    return mask, np.float64([[-1.5, 2, 3], [8.5, 10, 9]]), 2.5, np.float64([0.1, -0.2, 0.97, -3.5])


@pytest.mark.parametrize("kind", ["mat", "npz"])
def test_the_readers_round_trip_a_tiny_file(tmp_path, kind):
    from aarmvs import cloud_eval as ce
    mask, bb, res, plane = _mask_file_contents()
    m, p = str(tmp_path / f"ObsMask1_10.{kind}"), str(tmp_path / f"Plane1.{kind}")
    if kind == "mat":
        from scipy.io import savemat
        # as MATLAB stores them: a Fortran-ordered logical volume, Res a 1x1 matrix, P a column
        savemat(m, {"ObsMask": np.asfortranarray(mask), "BB": bb, "Res": np.float64([[res]])})
        savemat(p, {"P": plane.reshape(4, 1)})
    else:
        np.savez(m, ObsMask=np.asfortranarray(mask), BB=bb, Res=res)
        np.savez(p, P=plane)
    got = ce.read_dtu_mask(m)
    assert sorted(got) == ["bb", "obs_mask", "res"]
    assert got["obs_mask"].dtype == np.uint8 and got["obs_mask"].flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(got["obs_mask"], mask.astype(np.uint8))
    assert got["bb"].dtype == np.float64 and got["bb"].shape == (2, 3) and (got["bb"] == bb).all()
    assert got["res"] == res and isinstance(got["res"], float)
    gp = ce.read_dtu_plane(p)
    assert gp.dtype == np.float64 and gp.shape == (4,) and (gp == plane).all()


def test_a_mat_file_without_scipy_is_a_clear_error(tmp_path, monkeypatch):
    import sys
    from aarmvs import cloud_eval as ce
    monkeypatch.setitem(sys.modules, "scipy.io", None)
    with pytest.raises(ImportError, match="scipy"):
        ce.read_dtu_plane(str(tmp_path / "Plane1.mat"))


# --------------------------------------------------------------------------------- the protocol
def test_evaluate_dtu_on_a_case_worked_out_by_hand():
    """Two coincident recon points thin to one; the mask drops one point from the accuracy side but
    not from the completeness side's targets; the plane drops one ground-truth point; a distance
    equal to max_dist does not count."""
    recon = np.float32([[0, 0, 0], [0, 0, 0], [4, 0, 0], [8, 0, 0], [np.nan, 0, 0]])
    gt = np.float32([[0, 0, 1], [4, 0, 0.5], [8, 0, 2], [6, 0, -1]])
    mask = np.ones((9, 1, 1), np.uint8)
    mask[8] = 0                                       # the voxel of x = 8
    bb = np.float64([[0, 0, 0], [8, 0, 0]])
    plane = np.float64([0, 0, 1, 0])                  # above: z > 0
    got = dtu.evaluate_dtu(recon, gt, mask, bb, 1.0, plane, thin=0.5, patch=3.0, max_dist=2.0, seed=0)
    want = dict(n_recon=5, n_thinned=3, n_in_box=3, n_in_obs=2, n_gt=4, n_gt_above=3, thin_rounds=2,
                accuracy_mean=0.75, accuracy_median=0.5,             # {1, 0.5}
                completeness_mean=0.75, completeness_median=0.5,     # {1, 0.5}; 2 == max_dist is beyond
                overall=0.75, recon_beyond_max_dist=0, gt_beyond_max_dist=1, recon_nonfinite=1, gt_nonfinite=0,
                thin=0.5, patch=3.0, max_dist=2.0, seed=0, order="random")
    assert got == want
