"""The cases of tests/fwd_range_cases.py say what tests/test_gpu_fwd_range.py believes they say
(CPU only: the oracle in float64 and float32 and the float64 model of the documented staging, no
library):

* every case's float32 reference is finite and agrees with the float64 one at the parity
  tolerance (cost atol = rtol = 1e-4): a case that does not is out of the reference's own range
  and has no place in the table;
* scale-56 and scale-60 have 0 < 8 max|f|^2 < 2^-100 in fp32 (below the exponent's clamp), flush
  has it equal to 0, zero_all has every feature 0;
* the documented staging of x and sq (float64 model) costs at most a quarter of the tolerance,
  max |stage64 - ref64| <= 2.5e-5 on cost, for every scale and zero case and every outlier case
  but outlier_src3000, where it costs more than 1e-4: the cliff of the global bound lies between
  R = 300 and R = 3000.  (The measure is the one of the design study: the maximum absolute
  difference against the tolerance's absolute part.  At R = 3000 the model's 4.1e-4 falls where
  |cost| ~ 40, so it is still inside atol + rtol |cost| there: 0.11 of it.);
* every outlier is what its name says: the rest of the frame is the base frame bit for bit, N(0,1)
  to 5%, and max|f| is the stated R (one element) or the stated factor times the view's own
  maximum (a whole view).
"""
import pytest
import torch

import fwd_range_cases as fc

QUARTER = 0.25 * fc.TOL


@pytest.fixture(scope="module", autouse=True)
def _threads():
    prev = torch.get_num_threads()
    yield
    torch.set_num_threads(prev)


def test_case_table_is_the_agreed_one():
    assert fc.SHAPE == (1, 3, 32, 48, 3) and fc.SEED == 5 and fc.TOL == 1e-4
    assert fc.NAMES == (
        "scale-60", "scale-56", "scale-40", "scale-20", "scale-8", "scale+8", "scale+20",
        "zero_all", "zero_src", "zero_ref", "flush",
        "outlier_src30", "outlier_src300", "outlier_src3000", "outlier_ref300", "view_x10",
        "gn_tiny", "gn_zero", "weights-8", "weights+2")
    assert [c.name for c in fc.CASES if c.beyond] == ["outlier_src3000"]
    feats, proj, dv, P = fc.inputs(fc.BASE)
    assert tuple(feats.shape) == (3, 1, 32, 32, 48) and tuple(dv.shape) == (1, 3)
    assert set(fc.CELL_W + fc.DECONV_W + fc.DECONV_GN) <= set(P)


def test_staging_model_is_the_documented_one():
    """bound 2^-e in [2^14, 2^15) (omega: [2^13, 2^15), e even), the clamps, and the split."""
    for b in (1.0, 181.0, 7.2e5, 2.0 ** -99.5, 2.0 ** 120, 3.0):
        e, eo = fc.guard_exp(b), fc.omega_exp(b)
        assert 2.0 ** 14 <= b * 2.0 ** -e < 2.0 ** 15, (b, e)
        assert 2.0 ** 13 <= b * 2.0 ** -eo < 2.0 ** 15 and eo % 2 == 0 and eo - e in (0, 1), (b, eo)
    assert fc.guard_exp(0.0) == 0 and fc.omega_exp(0.0) == 0 and fc.guard_exp(-1.0) == 0
    assert fc.guard_exp(2.0 ** -101) == -114 and fc.guard_exp(2.0 ** -140) == -114
    assert fc.guard_exp(2.0 ** -100) == -114 and fc.guard_exp(2.0 ** -99) == -113
    assert fc.guard_exp(2.0 ** 133) == 119 and fc.guard_exp(2.0 ** 134) == 120
    v = torch.tensor([1.0, 1.0 + 2.0 ** -20, 3.0e-5, -0.7, 0.0], dtype=torch.float64)
    t = v * 2.0 ** 7
    s = fc.split_fp16(t, 7 - 14)   # staged at t 2^7: 1.0 -> 2^14
    # two fp16 parts: 22 bits for values near the bound; for small ones the lo part is a
    # subnormal, quantum 2^-24 in staged units
    err = (s - t).abs() * 2.0 ** 7
    assert bool((err <= torch.clamp(t.abs() * 2.0 ** 7 * 2.0 ** -22, min=2.0 ** -25)).all()), err
    assert float(err.max()) > 0.0 and float(s[4]) == 0.0 and float(s[0]) == 2.0 ** 7


@pytest.mark.parametrize("name", fc.NAMES + (fc.BASE.name,))
def test_case_keeps_the_gpu_test_honest(name):
    case = fc.BY_NAME[name]
    feats, proj, dv, P = fc.inputs(case)
    base = fc.inputs(fc.BASE)[0]
    r = fc.references(case)
    B, N, H, W, D = fc.SHAPE
    for ref in (r.ref64, r.ref32, r.stage64):
        assert tuple(ref["cost"].shape) == (B, D, H, W) and tuple(ref["depth"].shape) == (B, H, W)
        assert all(bool(torch.isfinite(ref[k]).all()) for k in ("cost", "depth", "conf")), name
    assert r.ref64["cost"].dtype == torch.float64 and r.ref32["cost"].dtype == torch.float32
    e32 = fc.max_abs(r.ref32["cost"], r.ref64["cost"])
    est = fc.max_abs(r.stage64["cost"], r.ref64["cost"])
    bound = fc.feature_bound(feats)
    print(f"\n{name:16s} 8 max|f|^2 = {bound:.3e} (e = {fc.guard_exp(bound)}, omega {fc.omega_exp(bound)}); "
          f"cost max|err| vs float64: float32 {e32:.3e}, staging model {est:.3e}; max|cost| "
          f"{float(r.ref64['cost'].abs().max()):.3e}")
    assert fc.within(r.ref32["cost"], r.ref64["cost"]), e32
    # the case reaches what it is meant for
    if case.kind == "scale" or name == "flush":
        assert torch.equal(feats, base * 2.0 ** case.k)
    if name in ("scale-56", "scale-60"):
        assert 0.0 < bound < 2.0 ** -100 and fc.guard_exp(bound) == -114
    if name == "scale+20":
        assert fc.guard_exp(bound) == fc.guard_exp(fc.feature_bound(base)) + 40
    if name == "flush":
        assert bound == 0.0 and float(feats.abs().max()) > 0.0
    if name == "zero_all":
        assert bound == 0.0 and float(feats.abs().max()) == 0.0
    if name == "zero_src":
        assert float(feats[1].abs().max()) == 0.0 and torch.equal(feats[0], base[0]) and torch.equal(feats[2], base[2])
    if name == "zero_ref":
        assert float(feats[0].abs().max()) == 0.0 and torch.equal(feats[1:], base[1:])
    if case.kind in ("scale", "zero") or (case.kind == "outlier" and not case.beyond):
        assert est <= QUARTER, est
    if case.beyond:
        assert est > fc.TOL, est
    if case.kind == "outlier":
        assert 0.95 <= float(base.std()) <= 1.05 and abs(float(base.mean())) <= 0.05
        changed = feats != base
        if name.startswith("view_"):
            assert bool(changed[2].any()) and not bool(changed[:2].any())
            assert float(feats.abs().max()) == float(base[2].abs().max() * case.factor)   # (fp32 product)
            ratio = float(feats.abs().max()) / float(base[:2].abs().max())
            assert case.factor / 1.5 <= ratio <= case.factor * 1.5, ratio
        else:
            view = 0 if "ref" in name else 1
            assert int(changed.sum()) == 1 and bool(changed[(view,) + fc.OUTLIER])
            assert float(feats.abs().max()) == case.factor == float(feats[(view,) + fc.OUTLIER])
            others = float(feats.masked_fill(changed, 0.0).abs().max())
            assert others == float(base.abs().max()) < 5.0   # max|f| / max|other| = R / 4.76
    if case.kind in ("gn", "weight"):
        assert torch.equal(feats, base)
        P0 = fc.inputs(fc.BASE)[3]
        moved = {k for k in P if not torch.equal(P[k], P0[k])}
        assert moved == set(fc.DECONV_GN if case.kind == "gn" else fc.CELL_W + fc.DECONV_W), moved
    if name == "gn_zero":
        assert all(float(P[k].abs().max()) == 0.0 for k in fc.DECONV_GN)


@pytest.mark.parametrize("name", ["outlier_src300", "outlier_ref300"])
def test_sharp_bound_rejects_a_staging_eight_bits_short(name):
    """What the GPU test's bound on the maximum absolute error (2 x float32's own + 3 x the staging
    model's loss) is worth: the same model with x and sq staged 2^8 lower than documented, as a
    wrong exponent in the kernels would stage them, exceeds it on the R = 300 outliers.  (On the
    plain frame the staging has bits to spare: 8 fewer lose 5.6e-7, against 4.7e-7.)"""
    from oracle import sweep_oracle as orc
    case = fc.BY_NAME[name]
    feats, proj, dv, P = fc.inputs(case)
    r = fc.references(case)
    b = fc.feature_bound(feats)
    short = {"x": lambda x: fc.split_fp16(x, fc.guard_exp(b) + 8),
             "sq": lambda sq: fc.split_fp16(sq, fc.omega_exp(b) + 8)}
    out = orc.sweep(*fc.views(feats, proj), dv, P, fast=True, dtype=torch.float64, stage=short)
    loss = fc.max_abs(out["cost"], r.ref64["cost"])
    sharp = 2.0 * fc.max_abs(r.ref32["cost"], r.ref64["cost"]) + 3.0 * fc.max_abs(r.stage64["cost"], r.ref64["cost"])
    print(f"\n{name}: 8 bits short loses {loss:.3e} on cost, the bound is {sharp:.3e}; "
          f"inside the parity tolerance: {fc.within(out['cost'], r.ref64['cost'])}")
    assert loss > sharp, (loss, sharp)


def test_standalone_references():
    """The standalone entries' references: the outlier reaches the omega conv's scale, and the
    models' losses are finite figures of the expected order."""
    for name in ("outlier_src300", "outlier_src3000"):
        s = fc.slice_reference(fc.BY_NAME[name], 0)
        assert bool(torch.isfinite(s.x).all()) and bool(torch.isfinite(s.omega).all())
        assert 0.0 <= float(s.omega.min()) and float(s.omega.max()) <= 1.0
        print(f"\n{name}: sq staging model, max loss on omega {s.omega_loss:.3e}, on the slice {s.x_loss:.3e} "
              f"(max|x| {float(s.x.abs().max()):.3e})")
    lo, hi = (fc.slice_reference(fc.BY_NAME[n], 0) for n in ("outlier_src300", "outlier_src3000"))
    assert lo.omega_loss < hi.omega_loss and lo.x_loss < hi.x_loss
    x1, c1, _ = fc.step_reference(1e3)
    base = fc.references(fc.BASE).x0
    assert torch.equal(x1[0, :, 5, 7], base.float()[0, :, 5, 7] * 1e3)
    keep = torch.ones_like(x1, dtype=torch.bool)
    keep[fc.PIXEL] = False
    assert torch.equal(x1[keep], base.float()[keep])
    for f in fc.PIXEL_FACTORS:
        x, c, loss = fc.step_reference(f)
        print(f"step, one pixel x {f:.0e}: max|x| {float(x.abs().max()):.3e}, x staging model loses {loss:.3e} on cost")
        assert bool(torch.isfinite(c).all()) and loss < 1e-3
