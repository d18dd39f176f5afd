"""GPU test of the forward sweep over the cases of tests/fwd_range_cases.py: features x 2^-60 ..
2^+20, x 2^-80 and exact zeros, one element or one view far above the rest of the frame,
GroupNorm affines x 2^-40 and 0, conv weights x 2^-8 and x 2^+2.

Every case: cost, depth and confidence are finite wherever the float32 oracle's are.  Every case
but outlier_src3000: cost within atol = rtol = 1e-4 of the float64 oracle, depth within 1e-3
relative L1, confidence within 1e-4 (test_gpu_parity.py's tolerances).  outlier_src3000 lies past
the point where the float64 model of the documented staging (stage64) loses 1e-4; its bound would be
1e-4 (1 + |ref64|) + 3 max|stage64 - ref64| (3: the recurrent h and the deconvs are staged the same
way and the model leaves them out), but the kernels keep the plain tolerance there (measured:
profiles/fwd_range_errors.txt: 0.12 of it, the 4.3e-4 falling where |cost| ~ 40), so the plain
tolerance is what is asserted.  That tolerance is wide where |cost| is large, so every case also
keeps its maximum absolute error within 2 x the float32 oracle's own + 3 x the staging model's,
and the scale cases hold the cost slice itself (the debug output) to the float64 oracle at their
own scale: below 2^-8 the regulariser sees x ~ 0 and the cost cannot tell a wrong slice.

The standalone entries localise a failure: aarmvs_cost_slice on the two large outliers (the omega
conv's sq staging alone), aarmvs_unet_step on a slice with one pixel x 1e3 .. 1e7 (cell 0's x
staging alone, the bound being max|x| itself).  The recorded training forward repeats the
inference one to 2e-5 of its scale and its backward is finite on outlier_src300, zero_src and
scale-56; on outlier_src300 dL/dref and dL/dsrc match float64 autograd within max(2e-5, 2 x
float32 autograd's own error).

tests/test_fwd_range_cases.py checks on the CPU what the references are trusted for.
"""
import functools
import os

import numpy as np
import pytest
import torch

import fwd_range_cases as fc
from test_gpu_bptt import _record_forward, bound, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def rel_l1(a, b):
    return float(np.abs(a - b).sum() / max(np.abs(b).sum(), 1e-30))


def _sweep_of(case):
    from aarmvs import ops
    feats, proj, dv, P = fc.inputs(case)
    sw = ops.DepthSweep({k: v.to(DEV) for k, v in P.items()}, DEV)
    return sw, fc.views(feats.to(DEV), proj) + (dv,)


@functools.lru_cache(maxsize=None)
def _run(case):
    """The case through the inference sweep (default precision and streams) -> host tensors."""
    sw, args = _sweep_of(case)
    out = sw(*args, want_cost=True)
    torch.cuda.synchronize()
    return {k: out[k].cpu() for k in ("cost", "depth", "conf")}


@functools.lru_cache(maxsize=None)
def _debug_slice(case):
    sw, args = _sweep_of(case)
    out = sw(*args, want_cost=True, debug=True)
    torch.cuda.synchronize()
    return out["slice"].cpu()


@pytest.mark.parametrize("name", fc.NAMES)
def test_sweep_matches_float64_over_feature_range(name):
    case = fc.BY_NAME[name]
    r = fc.references(case)
    got = _run(case)
    for k in ("cost", "depth", "conf"):
        fin = torch.isfinite(r.ref32[k])
        assert bool(torch.isfinite(got[k][fin]).all()), (name, k)
    c64 = r.ref64["cost"]
    figs = {who: (fc.max_abs(t, c64), fc.rel_l2(t, c64))
            for who, t in (("gpu", got["cost"]), ("ref32", r.ref32["cost"]), ("stage64", r.stage64["cost"]))}
    drl1 = rel_l1(got["depth"].numpy().astype(np.float64), r.ref64["depth"].numpy())
    cerr = fc.max_abs(got["conf"], r.ref64["conf"])
    print(f"\nFIG {name:16s} cost vs float64, max abs / relative L2: "
          + ", ".join(f"{who} {a:.3e} / {l:.3e}" for who, (a, l) in figs.items())
          + f"; gpu depth rel L1 {drl1:.3e}, conf max abs {cerr:.3e} "
          f"(float32 {fc.max_abs(r.ref32['conf'], r.ref64['conf']):.3e})")
    if case.beyond:
        allowed = fc.TOL * (1.0 + c64.abs()) + 3.0 * figs["stage64"][0]
        worst = float(((got["cost"].double() - c64).abs() / allowed).max())
        plain = float(((got["cost"].double() - c64).abs() / (fc.TOL * (1.0 + c64.abs()))).max())
        print(f"  beyond the model's cliff: worst error / (1e-4 (1 + |ref64|) + 3 x model loss) = {worst:.3f}, "
              f"/ the plain tolerance = {plain:.3f}")
    # the kernels keep the plain tolerance at R = 3000 as well (see the module docstring)
    np.testing.assert_allclose(got["cost"].numpy(), c64.numpy(), atol=fc.TOL, rtol=fc.TOL)
    assert drl1 <= 1e-3
    np.testing.assert_allclose(got["conf"].numpy(), r.ref64["conf"].numpy(), atol=1e-4)
    # The parity tolerance is 4e-3 where |cost| ~ 40 and would pass a staging that is several bits
    # short.  The sharper bound, in maximum absolute error: twice the float32 oracle's own (the
    # backward tests' rule) plus three times the staging model's loss (the factor as above).
    # tests/test_fwd_range_cases.py shows on the model that 8 lost bits break it.
    sharp = 2.0 * figs["ref32"][0] + 3.0 * figs["stage64"][0]
    print(f"  max abs error / (2 x float32's + 3 x the model's) = {figs['gpu'][0] / sharp:.3f}")
    assert figs["gpu"][0] <= sharp, (figs["gpu"][0], sharp)
    if case.kind == "scale":
        # printed, not asserted: omega's GroupNorm eps is not scale-free (below 2^-8 the omega
        # conv's output is far under sqrt(eps) and every weight goes to the biases' sigmoid)
        s0 = _debug_slice(fc.BASE)
        sk = _debug_slice(case).double() * 2.0 ** (-2 * case.k)
        print(f"  last plane's slice x 2^{-2 * case.k} vs the unscaled run's: max abs {fc.max_abs(sk, s0):.3e} "
              f"(max|x| {float(s0.abs().max()):.3e}), relative L2 {fc.rel_l2(sk, s0):.3e}, "
              f"bit-identical {bool((sk == s0.double()).all())}")
        # The regulariser sees x ~ 0 at the small scales (their costs are zero_all's), so the cost
        # says nothing about x there: the slice itself against the float64 oracle at the case's
        # own scale, in relative L2.  Bound: 4 x 2^-22 ~ 1e-6 (the omega conv's split-fp16
        # products are 2^-22 each and reach x through 1 + w; the rest is a dozen fp32 roundings),
        # or four times the float32 oracle's own error where that is larger.
        s = fc.slice_reference(case, fc.SHAPE[4] - 1)
        e = fc.rel_l2(_debug_slice(case), s.x)
        print(f"  last plane's slice vs float64 at this scale: relative L2 {e:.3e} (float32 oracle {s.x32_rl2:.3e})")
        assert e <= max(1e-6, 4.0 * s.x32_rl2), (e, s.x32_rl2)


@pytest.mark.parametrize("name", ["outlier_src300", "outlier_src3000"])
def test_standalone_cost_slice_with_an_outlier(name):
    """aarmvs_cost_slice on plane 0 against float64 orc.cost_slice / omega_weight: omega within
    1e-5, the slice within atol 1e-4, rtol 1e-5 (test_gpu_configs.py's), plus three times the sq
    staging model's loss where that is not under a quarter of those."""
    case = fc.BY_NAME[name]
    s = fc.slice_reference(case, 0)
    sw, args = _sweep_of(case)
    x, om = sw.cost_slice(*args[:4], args[4][:, 0].contiguous(), want_omega=True)
    torch.cuda.synchronize()
    x, om = x.cpu(), om.cpu()
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(om).all())
    x_tol = 1e-4 + 1e-5 * s.x.abs()
    x_extra = 0.0 if s.x_loss < 0.25 * 1e-4 else 3.0 * s.x_loss
    om_extra = 0.0 if s.omega_loss < 0.25 * 1e-5 else 3.0 * s.omega_loss
    x_worst = float(((x.double() - s.x).abs() / (x_tol + x_extra)).max())
    om_worst = fc.max_abs(om, s.omega) / (1e-5 + om_extra)
    print(f"\nFIG slice:{name:16s} omega max abs {fc.max_abs(om, s.omega):.3e} (model {s.omega_loss:.3e}, bound "
          f"{1e-5 + om_extra:.3e}); slice max abs {fc.max_abs(x, s.x):.3e}, relative L2 {fc.rel_l2(x, s.x):.3e} "
          f"(model {s.x_loss:.3e}, max|x| {float(s.x.abs().max()):.3e}), worst error / bound {x_worst:.3f}")
    assert om_worst <= 1.0, om_worst
    assert x_worst <= 1.0, x_worst


@pytest.mark.parametrize("factor", fc.PIXEL_FACTORS)
def test_standalone_unet_step_with_one_large_pixel(factor):
    """aarmvs_unet_step (which takes max|x| itself) on the base frame's plane-0 slice with one
    pixel x factor, against float64 orc.unet_step: atol = rtol = 1e-4, plus three times the x
    staging model's loss where that is not under a quarter of 1e-4."""
    x, c64, loss = fc.step_reference(factor)
    sw, _ = _sweep_of(fc.BASE)
    got = sw.unet_step(x.to(DEV), 0).cpu()
    extra = 0.0 if loss < 0.25 * fc.TOL else 3.0 * loss
    worst = float(((got.double() - c64).abs() / (fc.TOL * (1.0 + c64.abs()) + extra)).max())
    print(f"\nFIG step:x{factor:.0e}        cost max abs {fc.max_abs(got, c64):.3e}, relative L2 {fc.rel_l2(got, c64):.3e} "
          f"(model {loss:.3e}, max|x| {float(x.abs().max()):.3e}), worst error / bound {worst:.3f}")
    assert bool(torch.isfinite(got).all())
    assert worst <= 1.0, worst


@pytest.mark.parametrize("name", ["outlier_src300", "zero_src", "scale-56"])
def test_recorded_forward_and_backward_over_feature_range(name):
    case = fc.BY_NAME[name]
    B, N, H, W, D = fc.SHAPE
    sw, args = _sweep_of(case)
    cost, rec, rel = _record_forward(sw, args, B, H, W, D)
    g_ref, g_src, gp, _ = sw.backward(args[0], args[1], rel, args[4], rec, torch.ones_like(cost))
    torch.cuda.synchronize()
    ev = _run(case)["cost"]
    scale = float(ev.abs().max())
    print(f"\nFIG rec:{name:16s} recorded vs inference cost max abs {fc.max_abs(cost.cpu(), ev):.3e} "
          f"(2e-5 of the scale: {2e-5 * scale:.3e})")
    torch.testing.assert_close(cost.cpu(), ev, rtol=0, atol=2e-5 * scale)
    grads = {"ref": g_ref, **{f"src{v}": g for v, g in enumerate(g_src)}, **gp}
    nonfinite = [k for k, g in grads.items() if not bool(torch.isfinite(g).all())]
    assert not nonfinite, nonfinite
    if name != "outlier_src300":
        return
    ref = fc.grad_reference(case)
    _, gf64, _, _ = ref.g64
    gfeat = torch.stack([g_ref] + g_src).cpu().numpy()
    errs = {"features": (rel_l2(gfeat, gf64.numpy()), ref.e32["features"])}
    for v in range(N):
        k = f"features[{v},0]"
        errs[k] = (rel_l2(gfeat[v, 0], gf64[v, 0].numpy()), ref.e32[k])
    print("  dL/dfeatures, relative L2 vs float64 (gpu, cpu float32, bound):")
    for k, (e, c) in errs.items():
        print(f"FIG grad:{k:16s} {e:.3e} {c:.3e} {bound(k, c):.3e}")
    bad = {k: e for k, e in errs.items() if not e[0] <= bound(k, e[1])}
    assert not bad, bad
