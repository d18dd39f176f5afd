"""GPU test of the three small training-side kernel families over the cases of tests/
aux_kernel_cases.py: ops.group_norm (span boundaries, C/G == 1, a strided stats loop, affine
variants, 5-D and non-contiguous inputs, far means, extreme scales, constant groups, zero and
cancelling cotangents), ops.lstm_gates (the saturation grid, index shapes with a distribution per
gate block, non-finite inputs) and ops.deform_sample's backward (samples on the kink, on and
just outside the clamp range, inside the padding ring, far outside, single-lane and single-tap
cotangents, and 891 same-signed atomic terms into one pixel), each forward plus backward.

Every output is compared element by element with the float64 CPU reference of the case:

    m = max |got - ref64| / (|ref64| + s_t)  <=  max(16 * 2^-24 * kappa, 3 * m_f32)

with s_t, kappa and m_f32 (float32 CPU torch's own m) as aux_kernel_cases defines them; a tensor
whose uncancelled magnitude is zero must be exactly 0, for the deform outputs element by element.
The collision case's gx is held to N 2^-24 sum |terms|.  tests/test_aux_kernel_cases.py checks on
the CPU that the cases contain what they are named for and that float32 torch stays below the
floor, so that the 3 * m_f32 arm carries only the cases listed there.  Each case prints one line
(the worst tensor's m / m_f32 / bound); profiles/aux_kernel_errors.txt records them.
"""
import pytest
import torch

import aux_kernel_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def _check(label, got, ref, f32, bounds=None):
    """Every tensor of a case against its reference; prints the case's record line."""
    rows, bad = [], []
    for k, r in ref.out.items():
        if r is None:
            assert got[k] is None, f"{label} {k}: a gradient without an input"
            continue
        g = got[k].detach().cpu()
        assert tuple(g.shape) == tuple(r.shape), f"{label} {k}: shape {tuple(g.shape)} vs {tuple(r.shape)}"
        if k in ref.zero and not bool((g == 0).all()):
            bad.append(f"{k}: zero magnitude, but max |got| = {float(g.abs().max()):.3g}")
        m = ac.measure(g, r, ref.scales[k])
        b = ac.bound(f32[k], ref.kappa) if bounds is None or k not in bounds else bounds[k]
        rows.append((m / b, k, m, f32[k], b))
        if not m <= b:
            bad.append(f"{k}: m = {m:.3e} > bound {b:.3e} (float32 CPU torch {f32[k]:.3e})")
    _, k, m, m32, b = max(rows)
    print(f"\nAUX {label:48s} worst {k:8s} m {m:.3e} m_f32 {m32:.3e} bound {b:.3e} "
          + " ".join(f"{kk}={mm:.2e}" for _, kk, mm, _, _ in sorted(rows, key=lambda t: t[1])))
    assert not bad, f"{label}: " + "; ".join(bad)


# ---------------------------------------------------------------------------------------------
# group norm
# ---------------------------------------------------------------------------------------------
def _gn_run(case):
    from aarmvs import ops
    x, w, b, gy = ac.gn_inputs(case)
    xd, gyd = x.to(DEV), gy.to(DEV)
    assert xd.is_contiguous() == x.is_contiguous() and gyd.is_contiguous() == gy.is_contiguous()
    leaves = [t.clone().requires_grad_(True) if t is not None else None
              for t in (xd, None if w is None else w.to(DEV), None if b is None else b.to(DEV))]
    if case.layout == "x":   # clone() of a permuted view keeps its strides
        assert not leaves[0].is_contiguous()
    y = ops.group_norm(leaves[0], case.G, leaves[1], leaves[2], ac.EPS)
    y.backward(gyd)
    torch.cuda.synchronize()
    return {"y": y.detach(), "dx": leaves[0].grad,
            "dgamma": leaves[1].grad if leaves[1] is not None else None,
            "dbeta": leaves[2].grad if leaves[2] is not None else None}


@pytest.mark.parametrize("name", [c.name for c in ac.GN_CASES])
def test_group_norm_matches_float64(name):
    case = ac.GN_BY_NAME[name]
    got = _gn_run(case)
    _check("gn " + name, got, ac.gn_reference(case), ac.gn_f32(case))
    if case.repeat:   # fixed-order reductions: a second run repeats the first bit for bit
        again = _gn_run(case)
        for k, g in got.items():
            assert torch.equal(again[k], g), f"gn {name} {k}: a second run differs"


# ---------------------------------------------------------------------------------------------
# LSTM gates
# ---------------------------------------------------------------------------------------------
def _gate_run(case, cot):
    from aarmvs import ops
    z, c, _, _ = ac.gate_inputs(case)
    zd, cd = z.to(DEV).requires_grad_(True), c.to(DEV).requires_grad_(True)
    h, cn = ops.lstm_gates(zd, cd)
    dh, dc = ac.gate_cotangents(case, cot)
    outs, cots = {"both": ([h, cn], [dh, dc]), "dh": ([h], [dh]), "dc": ([cn], [dc])}[cot]
    torch.autograd.backward(outs, [t.to(DEV) for t in cots])
    torch.cuda.synchronize()
    return {"h": h.detach(), "c": cn.detach(), "dz": zd.grad, "dc_prev": cd.grad}


@pytest.mark.parametrize("cot", ac.GATE_COTS)
@pytest.mark.parametrize("name", [c.name for c in ac.GATE_CASES])
def test_lstm_gates_match_float64(name, cot):
    case = ac.GATE_BY_NAME[name]
    got = _gate_run(case, cot)
    ref = ac.gate_reference(case, cot)
    if case.kind == "nonfinite":
        for k in ac.GATE_TENSORS:
            pg, pr = ac.nonfinite_pattern(got[k]), ac.nonfinite_pattern(ref.out[k])
            assert torch.equal(pg, pr), (f"gates {name} {cot} {k}: inf / NaN pattern differs from float64's at "
                                         f"{(pg != pr).nonzero()[:8].tolist()}")
    else:
        assert all(bool(torch.isfinite(t).all()) for t in got.values())
    _check(f"gates {name} {cot}", got, ref, ac.gate_f32(case, cot))
    if case.repeat:
        again = _gate_run(case, cot)
        for k, g in got.items():
            assert torch.equal(again[k], g), f"gates {name} {cot} {k}: a second run differs"


# ---------------------------------------------------------------------------------------------
# deformable sampling
# ---------------------------------------------------------------------------------------------
def _df_run(case):
    """val, gx, goff, gm of ops.deform_sample in planar_val's layouts, and the kernel count."""
    from aarmvs import ops
    x, offset, mask, gval = ac.df_inputs(case)
    B, H, W, stride = case.shape
    h, w = ac.df_out_hw(case)
    xn = x.permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
    od = offset.to(DEV).requires_grad_(True)
    md = mask.to(DEV).requires_grad_(True) if mask is not None else None
    gk = gval.permute(0, 2, 3, 4, 1).reshape(B, h * w, ac.DF_TAPS * ac.DF_C).contiguous().to(DEV)
    ops.profile_enable(True)
    ops.profile_reset()
    try:
        val = ops.deform_sample(xn, od, md, stride, 1)
        val.backward(gk)
        torch.cuda.synchronize()
        launches = ops.profile_read()["deform_sample"][0]
    finally:
        ops.profile_enable(False)
    got = {"val": val.detach().view(B, h, w, ac.DF_TAPS, ac.DF_C).permute(0, 4, 1, 2, 3),
           "gx": xn.grad.permute(0, 3, 1, 2), "goff": od.grad, "gm": md.grad if md is not None else None}
    return got, launches


@pytest.mark.parametrize("name", [c.name for c in ac.DF_CASES])
def test_deform_sample_backward_matches_float64(name):
    case = ac.DF_BY_NAME[name]
    got, launches = _df_run(case)
    assert launches == 2, f"deform {name}: {launches} deform_sample launches (forward + backward = 2)"
    ref = ac.df_reference(case)
    mag = ac.df_magnitude(case)
    for k, r in ref.out.items():   # no term, or only zero terms: exactly 0 (far outside, the zero ring, ...)
        if r is not None:
            g = got[k].detach().cpu()
            stray = (mag[k] == 0) & (g != 0)
            assert not bool(stray.any()), f"deform {name} {k}: nonzero without a term at {stray.nonzero()[:8].tolist()}"
    bounds = None
    if case.pattern == "collision":
        # gx: the worst case of a float32 sum of N = 9 h w same-signed terms in any order
        lim = ac.collision_gx_bound()
        err = (got["gx"].detach().double().cpu() - ref.out["gx"]).abs()
        over = err > lim
        print(f"\nAUX deform collision gx: max |err| / (N 2^-24 sum|terms|) = "
              f"{float((err / lim.clamp_min(1e-300)).max()):.3e}, N = {ac.collision_terms()}")
        assert not bool(over.any()), (f"deform {name} gx: |err| up to {float(err.max()):.3e} over N 2^-24 sum|terms| "
                                      f"at {over.nonzero()[:8].tolist()}")
        bounds = {"gx": float("inf")}   # held above
    _check("deform " + name, got, ref, ac.df_f32(case), bounds)
