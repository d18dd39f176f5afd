"""The visibility de-duplication's contract on its numpy restatement (tests/fusion_dedup_ref.py):
known point counts on the synthetic fusion scenes, the properties every scan must have, and
that the cloud still covers the surface.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "aa-rmvsnet_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fusion_dedup_ref as dr  # noqa: E402
from oracle import fusion_oracle as fo  # noqa: E402

# (H, W, nsrc, seed) -> (final points, emitted points)
KNOWN = {(40, 52, 2, 2): (3114, 1678), (48, 64, 3, 5): (7109, 2984), (75, 101, 4, 1): (23143, 7970),
         (96, 128, 10, 0): (84348, 15227)}
SMALL = [(40, 52, 2, 2), (48, 64, 3, 5)]

_RUNS = {}


def _run(case):
    """(scene, de-duplicated scan, plain scan) of a case; computed once and not modified."""
    if case not in _RUNS:
        sc = dr.scene(*case)
        with np.errstate(all="ignore"):
            _RUNS[case] = (sc, dr.fuse_views(*sc, dedup=True), dr.fuse_views(*sc, dedup=False))
    return _RUNS[case]


@pytest.mark.parametrize("case", list(KNOWN))
def test_known_point_counts(case):
    _, on, off = _run(case)
    n_final, n_emit = off["xyz"].shape[0], on["xyz"].shape[0]
    print(case, n_final, n_emit, round(n_emit / n_final, 3))
    assert (n_final, n_emit) == KNOWN[case]
    assert n_emit / n_final <= 0.6
    assert sum(on["counts"].values()) == n_emit and on["rgb"].shape == (n_emit, 3)


@pytest.mark.parametrize("case", list(KNOWN))
def test_scan_properties(case):
    (pairs, depths, confs, cams, _), on, off = _run(case)
    first = pairs[0][0]
    for v, m in on["masks"].items():
        assert not (m["emit"] & ~m["final"]).any()                         # emit is a subset of final
        for k in ("photo", "geo", "final"):                                 # the filter is unchanged
            np.testing.assert_array_equal(m[k], off["masks"][v][k])
        np.testing.assert_array_equal(on["avg"][v], off["avg"][v])
        assert on["counts"][v] == int(m["emit"].sum())
    np.testing.assert_array_equal(on["masks"][first]["emit"], on["masks"][first]["final"])
    assert sorted(on["used"]) == sorted(depths)
    for u in on["used"].values():
        assert u.dtype == np.uint8 and set(np.unique(u)) <= {0, 1}
    # a later view emits nothing where an earlier one marked it
    last = pairs[-1][0]
    assert on["counts"][last] < on["counts"][first]


def test_the_order_of_the_views_matters_and_is_pinned():
    sc = dr.scene(75, 101, 4, 1, reverse=True)
    assert [r for r, _ in sc[0]] == [4, 3, 2, 1, 0]
    with np.errstate(all="ignore"):
        on = dr.fuse_views(*sc, dedup=True)
    assert on["xyz"].shape[0] == 8026
    np.testing.assert_array_equal(on["masks"][4]["emit"], on["masks"][4]["final"])


def test_marks_come_from_final_pixels_not_only_from_emitted_ones():
    """Marking from emit only is the other reading of the contract: it gives another count."""
    sc = dr.scene(75, 101, 4, 1)
    with np.errstate(all="ignore"):
        other = dr.fuse_views(*sc, dedup=True, mark_from_emit=True)
    assert other["xyz"].shape[0] == 9467 != KNOWN[(75, 101, 4, 1)][1]


@pytest.mark.parametrize("case", SMALL)
def test_every_full_cloud_point_has_an_emitted_point_nearby(case):
    _, on, off = _run(case)
    gap = dr.largest_gap(off["xyz"], on["xyz"]) / dr.footprint(case[1])
    print(case, "largest gap", round(gap, 2), "footprints")
    assert gap <= 2.0


def test_one_view_against_hand_made_used_maps():
    """used_ref removes exactly its pixels; None entries are not marked; marks are the rounded
    source coordinates of final, consistent pixels inside the image."""
    H, W = 40, 52
    pairs, depths, confs, cams, _ = dr.scene(H, W, 2, 2)
    args = (depths[0], confs[0], cams[0], [depths[1], depths[2]], [cams[1], cams[2]], 0.35)
    with np.errstate(all="ignore"):
        photo, geo, final, avg = fo.filter_depth_core(*args)
        used_ref = (np.random.default_rng(0).random((H, W)) < 0.5).astype(np.uint8)
        u1 = np.zeros((H, W), np.uint8)
        out = dr.filter_depth_dedup(*args, used_ref, [u1, None])
        np.testing.assert_array_equal(out[3], final & (used_ref == 0))
        np.testing.assert_array_equal(out[2], final)
        np.testing.assert_array_equal(out[4], avg)
        none = dr.filter_depth_dedup(*args, None, [None, None])
        np.testing.assert_array_equal(none[3], final)
        # the marks, pixel by pixel
        _, m, _, xs, ys, _ = fo.check_geometric_consistency(depths[0], *cams[0], depths[1], *cams[1])
    want = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            if final[y, x] and m[y, x]:
                X, Y = float(np.rint(xs[y, x])), float(np.rint(ys[y, x]))
                if 0 <= X < W and 0 <= Y < H:
                    want[int(Y), int(X)] = 1
    assert want.sum() > 100
    np.testing.assert_array_equal(u1, want)


def test_rint_rounds_ties_to_even_and_ignores_non_finite_values():
    H, W = 4, 6
    used = np.zeros((H, W), np.uint8)
    xs = np.array([0.5, 1.5, 2.5, -0.5, 5.5, np.nan, np.inf, 4.49], np.float32)
    X = np.rint(xs)
    np.testing.assert_array_equal(X[:5], np.array([0, 2, 2, -0.0, 6], np.float32))
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(X) & (X >= 0) & (X < W)
    used[0, X[ok].astype(np.int64)] = 1
    np.testing.assert_array_equal(used[0], np.array([1, 0, 1, 0, 1, 0], np.uint8))
