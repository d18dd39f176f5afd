"""GPU test of the kernels that turn a cost volume into what the user sees, over the cases of
tests/epilogue_cases.py:

* ops.softmax_depth on the unroll / tail plane counts, the hand-made finite columns (ascending,
  descending, ties, underflowing and subnormal terms, an overflowing difference) and the
  non-finite ones: NaN exactly where float32 torch.softmax has it, elsewhere rtol 1e-5 / atol 1e-7
  of float64 torch.softmax;
* ops.wta_update plane by plane on hand-made columns (ties, exp = 0, exp = inf once and twice,
  NaN planes, both depth orders, D = 1) against the float32 restatement of drmvsnet.py:324-334:
  depth bit for bit, max_prob within 4 * 2^-24, exp_sum within (4 + D) * 2^-24, equal NaN / inf
  patterns;
* ops.evidential_epilogue, forward and backward, per case and per tensor against float64
  autograd:  m = max |got - ref64| / (|ref64| + s_t) <= max(73 * 2^-24, 3 * m_f32), a tensor
  whose uncancelled magnitude is zero exactly 0, and the kernel's NaN pattern equal to float32 CPU
  torch's where that is not finite (evidence logits of -120).  Each case prints its worst
  tensor; profiles/epilogue_errors.txt records every tensor (tools/epilogue_profile.py);
* the 1028 x 1024 frame, one stride past 4096 x 256 pixels: softmax_depth, wta_update, the
  refinement and the posterior statistics (each from the volume and as the per-plane pair) against
  their tiled references and, bit for bit, against their own result on the 4099-pixel base;
  homo_warp and its backward against the oracle and float64 autograd.
"""
import os

import numpy as np
import pytest
import torch

import epilogue_cases as ec
import geometry_cases as gc
import posterior_ref as pr
import refine_ref as rr
from test_gpu_bptt import F32_THREADS, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    torch.set_num_threads(min(16, os.cpu_count() or 1))


# ---------------------------------------------------------------------------------------------
# softmax_depth
# ---------------------------------------------------------------------------------------------
def _softmax(cost):
    from aarmvs import ops
    out = ops.softmax_depth(cost.to(DEV))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("D", ec.SM_UNROLL_D)
def test_softmax_depth_unroll_and_tail(D):
    cost = ec.sm_random(D)
    ec.sm_check(_softmax(cost), cost, f"softmax D={D}")


@pytest.mark.parametrize("name", list(ec.SM_FINITE))
def test_softmax_depth_finite_columns(name):
    cost = ec.sm_volume(ec.SM_FINITE[name])
    got = _softmax(cost)
    assert bool(torch.isfinite(got).all())
    ec.sm_check(got, cost, f"softmax {name}")
    assert bool((got == got[:1, :, :, :1]).all()), "the same column at every pixel of both batch elements"


@pytest.mark.parametrize("name", list(ec.SM_NONFINITE))
def test_softmax_depth_non_finite_columns(name):
    cost = ec.sm_volume(ec.SM_NONFINITE[name])
    ec.sm_check(_softmax(cost), cost, f"softmax {name}")


# ---------------------------------------------------------------------------------------------
# standalone WTA
# ---------------------------------------------------------------------------------------------
def _wta_run(cost, dv):
    """ops.wta_update plane by plane over cost [B,D,H,W] (on the device), dv [B,D]."""
    from aarmvs import ops
    mp, dm, es = (torch.zeros_like(cost[:, 0]).contiguous() for _ in range(3))
    for d in range(cost.shape[1]):
        ops.wta_update(cost[:, d].contiguous(), dv[:, d], mp, dm, es)
    torch.cuda.synchronize()
    return {"depth": dm, "max_prob": mp, "exp_sum": es}


@pytest.mark.parametrize("name", [c.name for c in ec.WTA_CASES])
def test_wta_update_columns(name):
    case = ec.WTA_BY_NAME[name]
    cost, dv = ec.wta_volume(case), ec.wta_depths(case)[None]
    got = _wta_run(cost.to(DEV), torch.from_numpy(dv))
    ref = ec.wta_restatement(cost.view(1, len(case.costs), -1).numpy(), dv)
    ec.wta_check({k: v.cpu().numpy() for k, v in got.items()}, ref, len(case.costs), f"wta {name}")


# ---------------------------------------------------------------------------------------------
# evidential epilogue
# ---------------------------------------------------------------------------------------------
def _ev_run(case):
    from aarmvs import ops
    heads, g_ev, g_pc = ec.ev_inputs(case)
    hs = [h.to(DEV).requires_grad_(True) for h in heads]
    ev, pc = ops.evidential_epilogue(*hs, ec.ev_depths().to(DEV))
    outs = [(o, g.to(DEV)) for o, g in ((ev, g_ev), (pc, g_pc)) if g is not None]
    torch.autograd.backward([o for o, _ in outs], [g for _, g in outs])
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in ec.ev_named(ev, pc, [h.grad for h in hs]).items()}


def ev_rows(case, got):
    """(tensor, m, m_f32, bound) per tensor, and the failures."""
    ref, f32, f32o = ec.ev_reference(case), ec.ev_f32(case), ec.ev_f32_out(case)
    rows, bad = [], []
    for k in ec.EV_TENSORS:
        g, r = got[k], ref.out[k]
        assert tuple(g.shape) == tuple(r.shape), f"{case.name} {k}: shape {tuple(g.shape)} vs {tuple(r.shape)}"
        if k in ref.zero and not bool((g == 0).all()):
            bad.append(f"{k}: zero magnitude, but max |got| = {float(g.abs().max()):.3g}")
        if k in ec.EV_NONFINITE_F32.get(case.name, ()):
            if not torch.equal(torch.isnan(g), torch.isnan(f32o[k])):
                bad.append(f"{k}: NaN pattern differs from float32 CPU torch's "
                           f"({int(torch.isnan(g).sum())} vs {int(torch.isnan(f32o[k]).sum())} of {g.numel()})")
        m = ec.measure(g, ec.ev_masked(case, k), ref.scales[k])
        b = ec.ev_bound(f32[k])
        rows.append((k, m, f32[k], b))
        if not m <= b:
            bad.append(f"{k}: m = {m:.3e} > bound {b:.3e} (float32 CPU torch {f32[k]:.3e})")
    return rows, bad


@pytest.mark.parametrize("name", [c.name for c in ec.EV_CASES])
def test_evidential_epilogue_matches_float64(name):
    case = ec.EV_BY_NAME[name]
    got = _ev_run(case)
    rows, bad = ev_rows(case, got)
    k, m, m32, b = max(rows, key=lambda t: t[1] / t[3])
    print(f"\nEPI {name:28s} worst {k:9s} m {m:.3e} m_f32 {m32:.3e} bound {b:.3e}")
    assert not bad, f"evidential {name}: " + "; ".join(bad)


# ---------------------------------------------------------------------------------------------
# one stride past 4096 x 256 pixels
# ---------------------------------------------------------------------------------------------
def same(a, b):
    """Bit-for-bit equality that also holds where both are NaN."""
    if a.dtype.is_floating_point:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def _frames(D):
    """The base [2, D, 1, 4099] and the large frame [2, D, 1028, 1024] on the device, and the
    tiling of a [2, ..., 4099] result to the large frame."""
    base = ec.big_base(D)
    big = ec.big_tile(base).view(ec.BIG_B, D, ec.BIG_H, ec.BIG_W).to(DEV)
    return base.view(ec.BIG_B, D, 1, ec.BIG_BASE).to(DEV), big


def _tiled(t):
    t = torch.as_tensor(t)
    return ec.big_tile(t.reshape(ec.BIG_B, -1, ec.BIG_BASE)).view(ec.BIG_B, -1, ec.BIG_H, ec.BIG_W)


def _same_as_small(big, small, what):
    """out[b][p] == small[b][p % 4099], bit for bit."""
    for k in small:
        assert same(big[k].cpu().reshape(ec.BIG_B, -1), _tiled(small[k].cpu()).reshape(ec.BIG_B, -1)), f"{what} {k}"


def test_large_frame_softmax_depth():
    from aarmvs import ops
    small, big = _frames(5)
    got, got_small = ops.softmax_depth(big), ops.softmax_depth(small)
    torch.cuda.synchronize()
    ref = _tiled(ec.sm_reference(ec.big_base(5)))
    np.testing.assert_allclose(got.cpu().double().numpy(), ref.numpy(), rtol=ec.SM_RTOL, atol=ec.SM_ATOL)
    _same_as_small({"prob": got}, {"prob": got_small}, "softmax_depth")


def test_large_frame_wta_update():
    D = 2
    small, big = _frames(D)
    dv = ec.big_depths(D)
    got, got_small = _wta_run(big, dv), _wta_run(small, dv)
    ref = ec.wta_restatement(ec.big_base(D).numpy(), dv.numpy())
    ec.wta_check({k: v.cpu().numpy().reshape(ec.BIG_B, -1) for k, v in got.items()},
                 {k: _tiled(v).reshape(ec.BIG_B, -1).numpy() for k, v in ref.items()}, D, "wta 1028x1024")
    _same_as_small(got, got_small, "wta_update")


RKEYS = ("depth_refined", "conf_window", "index")


def _refine_pair(cost, dv):
    from aarmvs import ops
    B, D = cost.shape[:2]
    mp, dm, es = (torch.zeros_like(cost[:, 0]).contiguous() for _ in range(3))
    st = ops.refine_state(B, cost[0, 0].numel(), cost.device)
    for d in range(D):
        ops.wta_refine_update(cost[:, d].contiguous(), d, dv[:, d], mp, dm, es, st)
    return ops.wta_refine_finalize(mp, dm, es, st, dv, D)


def test_large_frame_refinement():
    """refine_from_cost and the wta_refine_update / _finalize pair at D = 3, at
    test_gpu_refine.test_against_the_float64_definition's tolerances."""
    from aarmvs import ops
    D = 3
    small, big = _frames(D)
    dv = ec.big_depths(D).to(DEV)
    vol, pair = ops.refine_from_cost(big, dv), _refine_pair(big, dv)
    vol_small, pair_small = ops.refine_from_cost(small, dv), _refine_pair(small, dv)
    torch.cuda.synchronize()
    ref = rr.from_volume64(ec.big_base(D).numpy(), dv.cpu().numpy())
    keep = _tiled(~ref["near_tie"]).numpy().reshape(-1)
    assert 1.0 - float(keep.mean()) <= 0.01 and ref["refined"].any()
    bound = _tiled(rr.depth_bound(ref)).numpy().reshape(-1)
    tile = lambda k: _tiled(ref[k]).numpy().reshape(-1)   # noqa: E731
    for what, out in (("refine_from_cost", vol), ("the per-plane pair", pair)):
        idx = out["index"].cpu().numpy().reshape(-1)
        assert np.array_equal(idx[keep], tile("index")[keep]), what
        err = np.abs(out["depth_refined"].cpu().numpy().astype(np.float64).reshape(-1) - tile("depth_refined"))
        assert (err[keep] <= bound[keep]).all(), what
        cw = out["conf_window"].cpu().numpy().astype(np.float64).reshape(-1)
        assert np.allclose(cw[keep], tile("conf_window")[keep], rtol=1e-5, atol=0), what
    for k in RKEYS:
        assert same(vol[k], pair[k]), k
    _same_as_small({k: vol[k] for k in RKEYS}, {k: vol_small[k] for k in RKEYS}, "refine_from_cost")
    _same_as_small({k: pair[k] for k in RKEYS}, {k: pair_small[k] for k in RKEYS}, "wta_refine pair")


def _posterior_pair(cost, dv):
    from aarmvs import ops
    B, D = cost.shape[:2]
    mp, dm, es = (torch.zeros_like(cost[:, 0]).contiguous() for _ in range(3))
    st = ops.posterior_state(B, cost[0, 0].numel(), cost.device)
    for d in range(D):
        ops.wta_posterior_update(cost[:, d].contiguous(), d, dv[:, d], mp, dm, es, st)
    return ops.wta_posterior_finalize(es, st)


def test_large_frame_posterior():
    """posterior_from_cost and the wta_posterior_update / _finalize pair at D = 3, within
    posterior_ref.bounds of the float64 definition as in test_gpu_posterior.check_bounds."""
    from aarmvs import ops
    D = 3
    small, big = _frames(D)
    dv = ec.big_depths(D).to(DEV)
    vol, pair = ops.posterior_from_cost(big, dv), _posterior_pair(big, dv)
    vol_small, pair_small = ops.posterior_from_cost(small, dv), _posterior_pair(small, dv)
    torch.cuda.synchronize()
    ref = pr.from_volume64(ec.big_base(D).numpy(), dv.cpu().numpy())
    bnd = pr.bounds(ref)
    big_ref = {k: (_tiled(v).numpy().reshape(ec.BIG_B, -1) if isinstance(v, np.ndarray) else v) for k, v in ref.items()}
    big_bnd = {k: _tiled(v).numpy().reshape(ec.BIG_B, -1) for k, v in bnd.items()}
    for what, out in (("posterior_from_cost", vol), ("the per-plane pair", pair)):
        got = {k: out[k].cpu().numpy().reshape(ec.BIG_B, -1) for k in pr.KEYS}
        assert all(np.isfinite(got[k]).all() for k in pr.KEYS), what
        ratio = pr.error_over_bound(got, big_ref, big_bnd)
        print(f"\n{what} 1028x1024: worst error / bound " + ", ".join(f"{k} {v:.4f}" for k, v in ratio.items()))
        assert all(r <= 1.0 for r in ratio.values()), (what, ratio)
    for k in pr.KEYS:
        assert same(vol[k], pair[k]), k
    _same_as_small({k: vol[k] for k in pr.KEYS}, {k: vol_small[k] for k in pr.KEYS}, "posterior_from_cost")
    _same_as_small({k: pair[k] for k in pr.KEYS}, {k: pair_small[k] for k in pr.KEYS}, "wta_posterior pair")


def big_warp_inputs():
    """(src [2,2,1028,1024], rel [2,3,4], depth [2], grad_out): element 0 under the plain rig,
    element 1 under geometry_cases' 'shift', which sends most of the frame out of bounds."""
    from aarmvs import synthetic as syn
    from oracle import sweep_oracle as orc
    H, W = ec.BIG_H, ec.BIG_W
    proj = torch.from_numpy(syn.camera_projections(2, H, W)).unsqueeze(0).repeat(2, 1, 1, 1)
    proj = gc.apply(proj, [(1, 1, "shift")], H, W)
    rel = orc.relative_projection(proj[:, 1], proj[:, 0])
    g = ec._gen("big:warp")
    src = torch.randn(ec.BIG_B, 2, H, W, generator=g)
    gout = torch.randn(ec.BIG_B, 2, H, W, generator=g)
    return src, rel, torch.tensor([600.0, 750.0]), gout


def test_large_frame_homo_warp_and_backward():
    """The forward at test_gpu_geometry's atol 1e-5 against the oracle; the backward per batch
    element within max(2e-5, 2 x float32 grid_sample's own error) relative L2 of float64 autograd,
    the bound of test_standalone_warp_matches_oracle_per_batch_element."""
    from aarmvs import ops
    from oracle import sweep_oracle as orc
    src, rel, dep, gout = big_warp_inputs()
    B, C, H, W = src.shape
    want = orc.homo_warp(src, rel, dep)
    inside = [float((want[b] != 0).float().mean()) for b in range(B)]
    assert inside[0] > 0.9 and 0.02 < inside[1] < 0.6, inside   # element 1 is partly out of bounds
    got = ops.homo_warp(src.to(DEV), rel, dep).cpu().numpy()
    np.testing.assert_allclose(got, want.numpy(), atol=1e-5, rtol=0)
    s64 = src.double().requires_grad_(True)
    orc.homo_warp(s64, rel, dep, fast=True).backward(gout.double())
    e32 = np.zeros(B)
    prev = torch.get_num_threads()
    try:
        for n in F32_THREADS:
            torch.set_num_threads(n)
            s32 = src.clone().requires_grad_(True)
            orc.homo_warp(s32, rel, dep, fast=True).backward(gout)
            e32 = np.maximum(e32, [rel_l2(s32.grad[b].numpy(), s64.grad[b].numpy()) for b in range(B)])
    finally:
        torch.set_num_threads(prev)
    gb = ops.homo_warp_backward(gout.to(DEV), rel, dep, (B, C, H, W)).cpu().numpy()
    for b in range(B):
        e = rel_l2(gb[b], s64.grad[b].numpy())
        print(f"\nwarp backward 1028x1024 b {b}: {e:.3e} (cpu float32 {e32[b]:.3e})")
        assert e <= max(2e-5, 2.0 * e32[b]), (b, e, e32[b])
