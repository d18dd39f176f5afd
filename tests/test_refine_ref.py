"""CPU checks of the numpy restatement of the sub-plane refinement (tests/refine_ref.py): the
sequential float32 form against the float64 definition from the volume, and the properties the
definition promises (include/aarmvs.h, aarmvs_sweep_r)."""
import numpy as np
import pytest

import refine_ref as rr


def volume(seed, B=2, D=9, HW=257, scale=3.0, inverse=False):
    g = np.random.default_rng(seed)
    cost = (g.standard_normal((B, D, HW)) * scale).astype(np.float32)
    if inverse:   # inverse-depth spacing: uniform in 1/d
        dv = (1.0 / np.linspace(1.0 / 425.0, 1.0 / 935.0, D)).astype(np.float32)
    else:
        dv = np.linspace(425.0, 935.0, D).astype(np.float32)
    return cost, np.stack([dv, dv * np.float32(1.1)][:B])


@pytest.mark.parametrize("seed,D,inverse", [(0, 9, False), (1, 17, True), (2, 3, False), (3, 5, True)])
def test_sequential_form_agrees_with_the_float64_definition(seed, D, inverse):
    cost, dv = volume(seed, D=D, inverse=inverse)
    a, b = rr.sequential(cost, dv), rr.from_volume64(cost, dv)
    keep = ~b["near_tie"]
    assert keep.mean() > 0.99
    assert np.array_equal(a["index"][keep], b["index"][keep])
    assert np.array_equal(a["refined"][keep], b["refined"][keep])
    assert a["refined"].any() and (~a["refined"]).any()
    err = np.abs(a["depth_refined"].astype(np.float64) - b["depth_refined"])
    assert (err[keep] <= rr.depth_bound(b)[keep]).all()
    assert np.allclose(a["conf_window"][keep], b["conf_window"][keep], rtol=1e-5, atol=0)


@pytest.mark.parametrize("inverse", [False, True])
def test_refined_depth_lies_between_the_neighbours(inverse):
    cost, dv = volume(5, D=12, inverse=inverse)
    a = rr.sequential(cost, dv)
    w = a["index"]
    r = a["refined"]
    B, D = dv.shape
    take = lambda k: np.take_along_axis(dv, np.clip(k, 0, D - 1), 1)
    lo = np.minimum(take(w - 1), take(w + 1)).astype(np.float64)
    hi = np.maximum(take(w - 1), take(w + 1)).astype(np.float64)
    d = a["depth_refined"].astype(np.float64)
    slack = 2.0 ** -22 * np.abs(hi)          # the final add's rounding, and one more ulp
    assert r.any()
    assert (d[r] >= lo[r] - slack[r]).all() and (d[r] <= hi[r] + slack[r]).all()
    # the offset is a convex combination: strictly inside unless a neighbour holds all the mass
    assert (np.abs(d[r] - take(w)[r]) <= np.maximum(hi - take(w), take(w) - lo)[r] + slack[r]).all()


def test_unrefined_pixels_equal_wta_and_the_window_confidence_dominates():
    cost, dv = volume(7, D=6)
    cost[0, 0, :40] = 9.0      # winners on the first plane
    cost[0, 5, 40:80] = 9.0    # winners on the last plane
    cost[1, :, :16] = -200.0   # p == 0 everywhere: no winner
    a = rr.sequential(cost, dv)
    u = ~a["refined"]
    assert np.array_equal(a["depth_refined"][u], a["depth"][u])
    assert (a["index"][0, :40] == 0).all() and u[0, :40].all()
    assert (a["index"][0, 40:80] == 5).all() and u[0, 40:80].all()
    assert (a["index"][1, :16] == -1).all() and (a["depth_refined"][1, :16] == 0).all()
    ok = np.isfinite(a["conf"])
    assert (a["conf_window"][ok] >= a["conf"][ok]).all()
    assert np.array_equal(np.isnan(a["conf_window"]), np.isnan(a["conf"]))
    # one-sided sums at the borders are larger than the single plane's mass where p > 0
    assert (a["conf_window"][0, :80] > a["conf"][0, :80]).all()


def test_a_prefix_of_the_planes_is_a_sweep_of_its_own():
    """n planes of the sequential form are the whole form on the first n planes (what a d_range
    piece reports), and a winner on the last plane seen is unrefined until the next is seen."""
    cost, dv = volume(11, D=5)
    cost[0, 2, :32] = 8.0
    part, whole = rr.sequential(cost, dv, n=3), rr.sequential(cost[:, :3], dv[:, :3])
    for k in ("depth_refined", "conf_window", "index"):
        assert np.array_equal(part[k], whole[k], equal_nan=True)
    assert (part["index"][0, :32] == 2).all() and not part["refined"][0, :32].any()
    assert rr.sequential(cost, dv)["refined"][0, :32].all()


def test_overflow_and_nan_fall_back_to_wta():
    dv = np.linspace(1.0, 2.0, 4, dtype=np.float32)[None]
    cost = np.zeros((1, 4, 8), np.float32)
    cost[0, 1, :] = 1.0
    cost[0, 1, 0] = 100.0            # exp overflows in float32
    cost[0, 2, 1] = np.nan           # a NaN plane beside the winner
    a = rr.sequential(cost, dv)
    assert a["depth_refined"][0, 0] == dv[0, 1] and np.isnan(a["conf_window"][0, 0]) and np.isnan(a["conf"][0, 0])
    assert a["depth_refined"][0, 1] == dv[0, 1] and not a["refined"][0, 1]
    assert a["refined"][0, 2:].all()
