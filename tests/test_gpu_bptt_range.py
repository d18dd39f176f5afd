"""GPU test of the training backward (aarmvs_sweep_backward) over the cases of tests/
bptt_range_cases.py: the argument limits (nsrc 1 and 16, the 4x4 frame, a strip, a ragged frame,
B = 3), plane counts 1 and 17, cotangents that vanish on whole plane groups, sit on one plane or
on two pixels or are zero, and cotangents scaled by 2^-96 .. 2^+96.

The steps and the bound are those of test_gpu_bptt.test_backward_matches_float64_autograd: the
recorded forward, one backward with want_grad_x, every tensor (dL/dx, dL/dfeatures whole and per
(view, batch element) slice, every parameter gradient) in relative L2 against float64 autograd of
the oracle, within max(2e-5, 2 x float32 CPU autograd's own error for the case's cotangent);
omega.reweight_network.2.bias within that or |error| <= 0.5 u sum|terms|.  Under the linear loss
(dL/dcost = R') cost_regularization.conv_0.bias is sum(R') and held to the common bound; under the
softmax loss its true value is 0 and it keeps <= 1e-5 sum|dL/dcost|.  Every output is finite, the
recorded forward's cost volume matches float64 at atol = rtol = 1e-4, and a second backward
repeats the first bit for bit.  tests/test_bptt_range_cases.py checks on the CPU that float32's
error (hence the bound) stays below 1e-3 and that the vanishing groups are below 2^-113.
"""
import functools
import os

import numpy as np
import pytest
import torch

import bptt_range_cases as rc
from test_gpu_bptt import F32_THREADS, _record_forward, bound, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
KB = "omega.reweight_network.2.bias"
HB = "cost_regularization.conv_0.bias"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def _gpu_run(case):
    """Recorded forward and two backward calls -> (cost, dL/dcost, first, second)."""
    from aarmvs import ops
    B, N, H, W, D = case.shape
    feats, proj, dv, P, Rp = rc.inputs(case)
    sw = ops.DepthSweep({k: v.to(DEV) for k, v in P.items()}, DEV)
    fd = feats.to(DEV)
    args = (fd[0], [fd[v] for v in range(1, N)], proj[:, 0], [proj[:, v] for v in range(1, N)], dv)
    cost, rec, rel = _record_forward(sw, args, B, H, W, D)
    Rd = Rp.to(DEV)
    if case.loss == "linear":
        gcost = Rd
    else:   # dL/dcost of sum(R' * softmax(cost))
        prob = torch.softmax(cost, dim=1)
        gcost = prob * (Rd - (Rd * prob).sum(dim=1, keepdim=True))
    first = sw.backward(args[0], args[1], rel, dv, rec, gcost, want_grad_x=True)
    second = sw.backward(args[0], args[1], rel, dv, rec, gcost, want_grad_x=True)
    torch.cuda.synchronize()
    return cost, gcost, first, second


def _tensors(out):
    """{name: tensor} of a backward's outputs, on the host."""
    g_ref, g_src, gp, gx = out
    t = {"features": torch.stack([g_ref] + g_src).cpu(), "x": gx.cpu()}
    t.update({"all:" + k: g.cpu() for k, g in gp.items()})
    return t


@functools.lru_cache(maxsize=None)
def _scale_base_tensors():
    """The k = 0 run of the scale cases on the GPU (for the bit-identity count only)."""
    return _tensors(_gpu_run(rc.SCALE_BASE)[2])


def test_standalone_warp_backward_over_cotangent_scale():
    """aarmvs_homo_warp_backward sums dL/dsrc in the same 64-bit fixed point as the sweep's
    backward, with its own exponent (warp.hip warp_bwd_exp): grad_out * 2^k for k = -96 ..
    +96 on the scale cases' scene, against float64 autograd through the oracle's warp within
    max(2e-5, 2 x float32 grid_sample's own error) relative L2; for k = -48, +48, +96 also
    bit-identical to the k = 0 result after rescaling (a power-of-two scale only moves the
    exponent; at -96 the smallest weight x gradient products are subnormal and round)."""
    from aarmvs import ops
    from oracle import sweep_oracle as orc
    feats, proj, dv, _, _ = rc.inputs(rc.SCALE_BASE)
    N, B, C, H, W = feats.shape
    gout = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(7))
    rel = ops.relative_projection(proj[:, 1], proj[:, 0])
    dep = dv[:, 1].contiguous()
    s64 = feats[1].double().requires_grad_(True)
    orc.homo_warp(s64, rel, dep, fast=True).backward(gout.double())
    s32 = feats[1].clone().requires_grad_(True)
    orc.homo_warp(s32, rel, dep, fast=True).backward(gout)
    e32 = rel_l2(s32.grad.numpy(), s64.grad.numpy())
    base = ops.homo_warp_backward(gout.to(DEV), rel, dep, (B, C, H, W)).cpu()
    print(f"\nstandalone warp backward, relative L2 vs float64: k = 0 {rel_l2(base.numpy(), s64.grad.numpy()):.3e}, "
          f"cpu float32 {e32:.3e}")
    for k in (0,) + rc.SCALE_KS:
        gb = ops.homo_warp_backward((gout * 2.0 ** k).to(DEV), rel, dep, (B, C, H, W)).cpu()
        assert bool(torch.isfinite(gb).all()), k
        e = rel_l2((gb.double() * 2.0 ** -k).numpy(), s64.grad.numpy())
        print(f"  k = {k:+3d}: {e:.3e}, bit-identical to k = 0: {torch.equal(gb * 2.0 ** -k, base)}")
        assert e <= max(2e-5, 2.0 * e32), (k, e, e32)
        if k != -96:
            assert torch.equal(gb * 2.0 ** -k, base), k


@pytest.mark.parametrize("name", rc.NAMES)
def test_backward_matches_float64_autograd_over_range_and_limits(name):
    case = rc.BY_NAME[name]
    B, N, H, W, D = case.shape
    ref = rc.reference(case)
    prob64, gf64, gp64, gx64 = ref.g64
    cost, gcost, first, second = _gpu_run(case)
    got = _tensors(first)
    print(f"\n== {name}: B, N, H, W, D = {case.shape}, {case.loss} loss")
    # forward
    cerr = float((cost.cpu().double() - ref.cost).abs().max())
    print(f"forward: cost max|err| {cerr:.3e} (max|cost| {float(ref.cost.abs().max()):.3e})")
    np.testing.assert_allclose(cost.cpu().numpy(), ref.cost.numpy(), atol=1e-4, rtol=1e-4)
    if case.loss == "softmax":
        np.testing.assert_allclose(torch.softmax(cost, dim=1).cpu().numpy(), prob64.numpy(), atol=1e-5)
    # every output finite, the second call bit for bit
    nonfinite = [k for k, t in got.items() if not bool(torch.isfinite(t).all())]
    assert not nonfinite, nonfinite
    for k, t in _tensors(second).items():
        assert torch.equal(got[k], t), k
    if name == "zero":
        nonzero = [k for k, t in got.items() if float(t.abs().max()) != 0.0]
        assert not nonzero, nonzero
        return
    # backward vs float64, float32 autograd's spread for this cotangent
    e32 = rc.f32_spread(case)
    gfeat = got["features"].numpy()
    gx = got["x"].permute(0, 1, 4, 2, 3).numpy()   # [D,B,32,H,W]
    errs = {"x": (rel_l2(gx, np.stack([g.numpy() for g in gx64])), e32["x"]),
            "features": (rel_l2(gfeat, gf64.numpy()), e32["features"])}
    for v in range(N):
        for b in range(B):
            k = f"features[{v},{b}]"
            errs[k] = (rel_l2(gfeat[v, b], gf64[v, b].numpy()), e32[k])
    for k in gp64:
        if k != HB or case.loss == "linear":   # softmax: true gradient 0
            errs["all:" + k] = (rel_l2(got["all:" + k].numpy(), gp64[k].numpy()), e32[k])
    print(f"relative L2 vs float64 (gpu, cpu float32 max over threads {F32_THREADS}):")
    for k, (e, c) in errs.items():
        print(f"  {k:52s} {e:.3e} {c:.3e}")
    ulp_sum = abs(float(got["all:" + KB]) - float(gp64[KB])) / (2.0 ** -24 * ref.tsum)
    print(f"  all:{KB} |error| / (u sum|terms|) = {ulp_sum:.3f}")
    worst = max(errs, key=lambda k: errs[k][0] / bound(k, errs[k][1]))
    print(f"  worst error / bound: {errs[worst][0] / bound(worst, errs[worst][1]):.3f} ({worst})")
    if case.k != 0:
        base = _scale_base_tensors()
        same = [k for k, t in got.items() if torch.equal(t * 2.0 ** -case.k, base[k])]
        print(f"  bit-identical to the k = 0 run after rescaling: {len(same)} of {len(got)} tensors")
    bad = {k: e for k, e in errs.items()
           if not (e[0] <= bound(k, e[1]) or (k == "all:" + KB and ulp_sum <= 0.5))}
    assert not bad, bad
    if case.loss == "softmax":
        assert abs(float(got["all:" + HB])) <= 1e-5 * float(gcost.abs().sum())
