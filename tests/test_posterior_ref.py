"""The depth-posterior statistics' float32 op sequence against their float64 definition, on the
CPU: tests/posterior_ref.py's bounds hold on every pixel, they are tight enough to reject the
naive variance update, and the invariants of the definition (include/aarmvs.h,
aarmvs_posterior_args)."""
import numpy as np
import pytest

import posterior_ref as pr

F = np.float32
HW = 96


def _depths(D, spacing):
    if spacing == "linear":
        d = np.linspace(425.0, 935.0, D)
    else:   # inverse depth, uniformly spaced
        d = 1.0 / np.linspace(1.0 / 425.0, 1.0 / 935.0, D)
    return np.stack([d, d[::-1]]).astype(F)   # the second batch element sweeps far to near


def _randn_case(D, scale, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((2, D, HW)) * scale).astype(F)


CASES = [(D, s, sp) for D in (5, 17, 512, 898) for s in (1, 3, 6) for sp in ("linear", "inverse")]


@pytest.mark.parametrize("D,scale,spacing", CASES)
def test_sequential32_is_within_the_bounds_of_the_float64_definition(D, scale, spacing):
    cost, dv = _randn_case(D, scale, 1000 * D + scale), _depths(D, spacing)
    got, ref = pr.sequential32(cost, dv), pr.from_volume64(cost, dv)
    for k in pr.KEYS:
        assert np.isfinite(got[k]).all(), k
    ratio = pr.error_over_bound(got, ref)
    print(f"D={D} scale={scale} {spacing}: worst error / bound {ratio}")
    assert all(r <= 1.0 for r in ratio.values()), ratio


@pytest.mark.parametrize("spacing", ["linear", "inverse"])
def test_late_dominant_plane(spacing):
    """One plane holds all but ~1e-8 of the mass.  The S0 / S1 form stays within the bounds; the
    naive (1 - k) form loses the standard deviation and must violate its bound."""
    rng = np.random.default_rng(42)
    cost, dv = pr.late_dominant(rng, 2, 512, HW), _depths(512, spacing)
    ref = pr.from_volume64(cost, dv)
    good = pr.error_over_bound(pr.sequential32(cost, dv), ref)
    naive = pr.error_over_bound(pr.sequential32(cost, dv, naive=True), ref)
    print(f"late-dominant {spacing}: error / bound, S0/S1 form {good}; naive form {naive}; "
          f"true std {ref['depth_std'].min():.3g} .. {ref['depth_std'].max():.3g}")
    assert all(r <= 1.0 for r in good.values()), good
    assert naive["depth_std"] > 1.0, "the std bound is too loose to tell the naive update apart"


@pytest.mark.parametrize("naive", [False, True])
def test_the_variance_is_never_negative(naive):
    rng = np.random.default_rng(3)
    for cost in (_randn_case(17, 6, 5), pr.late_dominant(rng, 2, 512, HW)):
        D = cost.shape[1]
        got = pr.sequential32(cost, _depths(D, "inverse"), naive=naive)
        assert (got["var_min"] >= 0).all() and (got["var"] >= 0).all()


@pytest.mark.parametrize("D,scale", [(5, 1), (17, 6), (512, 3), (898, 6)])
def test_the_mean_stays_inside_the_depth_range(D, scale):
    cost, dv = _randn_case(D, scale, 7), _depths(D, "inverse")
    mu = pr.sequential32(cost, dv)["depth_mean"]
    lo, hi = dv.min(), dv.max()
    ulp = np.spacing(hi)
    assert (mu >= lo - ulp).all() and (mu <= hi + ulp).all(), (mu.min(), mu.max())


def test_partial_sweep_and_single_plane():
    cost, dv = _randn_case(5, 3, 11), _depths(5, "linear")
    got, ref = pr.sequential32(cost, dv, n=3), pr.from_volume64(cost, dv, n=3)
    assert all(r <= 1.0 for r in pr.error_over_bound(got, ref).values())
    one = pr.sequential32(cost, dv, n=1)
    assert (one["depth_mean"] == dv[:, :1]).all()
    for k in ("depth_std", "runner_up"):
        assert (one[k] == 0).all(), k
    # logf(expf(c)) - c is zero only up to the two functions' rounding
    ref1 = pr.from_volume64(cost, dv, n=1)
    assert (one["entropy"] <= pr.bounds(ref1)["entropy"]).all() and (ref1["entropy"] == 0).all()


def test_nan_exactly_where_the_confidence_is_nan():
    dv = np.array([[1, 2, 3, 4]], F)
    cost = np.zeros((1, 4, 4), F)
    cost[0, 1, 1] = 100.0        # exp overflows: inf / inf
    cost[0, :, 2] = -200.0       # every exp underflows: 0 / 0
    cost[0, 2, 3] = np.nan
    got = pr.sequential32(cost, dv)
    for k in pr.KEYS:
        assert (np.isnan(got[k][0]) == np.array([False, True, True, True])).all(), k
    assert (np.isnan(got["conf"][0]) == np.array([False, True, True, True])).all()
    # the uniform pixel: mean 2.5, std sqrt(1.25), entropy ln 4, and the tie rule
    assert abs(got["depth_mean"][0, 0] - 2.5) < 1e-6 and abs(got["depth_std"][0, 0] - 1.25 ** 0.5) < 1e-6
    assert abs(got["entropy"][0, 0] - np.log(4.0)) < 1e-6
    assert got["runner_up"][0, 0] == got["conf"][0, 0] == F(0.25)


def test_ause():
    rng = np.random.default_rng(0)
    err = np.abs(rng.standard_normal((12, 15)))
    mask = (rng.random((12, 15)) > 0.3).astype(F)
    assert pr.ause(err, err, mask) == 0.0
    assert pr.ause(err, 3.0 * err + 1.0, mask) == 0.0          # any increasing map of the error
    assert pr.ause(err, -err, mask) > 0.0                      # the reversed ranking
    noisy = pr.ause(err, err + 0.5 * rng.standard_normal(err.shape), mask)
    assert 0.0 < noisy < pr.ause(err, -err, mask)
    # pixels outside the mask do not count
    wild = np.where(mask > 0.5, err, 1e9)
    assert pr.ause(wild, wild, mask) == 0.0 and pr.ause(wild, -wild, mask) == pr.ause(err, -err, mask)
