"""GPU tests of the sweep and its training backward under adversarial camera geometry
(tests/geometry_cases.py), against the CPU oracle and its float64 autograd.

Every other GPU test draws its cameras from aarmvs.synthetic.scene: one fronto-parallel rig and
one depth list broadcast over the batch.  There the cost-slice backward (cost_bwd.hip
cbw_feat_kernel) only ever takes its in-box gather, and no index of the form
``Rel + 12 * (v * B + b)`` or ``dvals[b * D + d]`` can be told from its b = 0 value.  Here:

* one case per kind (zoom out, zoom in, in-plane rotation, points behind the source camera, a
  mostly non-overlapping view) on source view 1, at ragged 36x52 / 44x60 frames: the fallbacks of
  the source-box gather (overflowing cells, oversized, empty and behind-camera boxes, taps outside
  the box) carry the feature gradient.  tests/test_geometry_cases.py asserts on the CPU that each
  case reaches its regime at these shapes;
* a B = 2 batch whose two elements have different cameras for every source view and different
  (ascending / descending) depth lists, over a 16-plane group and a ragged 2-plane one;
* the standalone entry points (homo_warp, homo_warp_backward, cost_slice, wta_update) on the
  batch's cameras and per-element depths.

Tolerances are the project's: cost volume atol = rtol = 1e-4, depth rel-L1 <= 1e-3, confidence
atol 1e-4; every gradient within max(2e-5, 2 x float32 CPU autograd's own error) relative L2 of
float64 autograd (test_gpu_bptt.bound), the feature gradient also per (view, batch element)
slice, each slice against its own float32 spread: an error confined to one view's fallback path
is small in the whole tensor's norm.  Two backward calls agree bit for bit (the fixed-point
atomics carry most of the sum here).
"""
import functools
import os

import numpy as np
import pytest
import torch

from aarmvs import synthetic as syn

import geometry_cases as gc
from test_gpu_bptt import F32_THREADS, _f32_spread, _oracle_grads, bound, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
KB = "omega.reweight_network.2.bias"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def rel_l1(a, b):
    return float(np.abs(a - b).sum() / max(np.abs(b).sum(), 1e-30))


def _views(feats, proj):
    N = feats.shape[0]
    return feats[0], [feats[v] for v in range(1, N)], proj[:, 0], [proj[:, v] for v in range(1, N)]


def _weights(wseed):
    return {k: torch.from_numpy(v) for k, v in syn.sweep_weights(wseed).items()}


def _gpu_run(feats, proj, dv, P, gcost_of):
    """Eval sweep, recorded forward and two backward calls on the GPU.  gcost_of(cost) -> dL/dcost."""
    from aarmvs import ops
    N, B, C, H, W = feats.shape
    D = dv.shape[1]
    sw = ops.DepthSweep({k: v.to(DEV) for k, v in P.items()}, DEV)
    ref, srcs, ref_proj, src_projs = _views(feats.to(DEV), proj)
    ev = sw(ref, srcs, ref_proj, src_projs, dv)
    rec = sw.record_buffers(B, H, W, D, DEV, nsrc=N - 1)
    rel = sw.relative(ref_proj, src_projs, B)
    cost = torch.empty(B, D, H, W, device=DEV)
    sw(ref, srcs, ref_proj, src_projs, dv, want_depth=False, cost_out=cost, rel=rel, record=rec)
    gcost = gcost_of(cost)
    first = sw.backward(ref, srcs, rel, dv, rec, gcost, want_grad_x=True)
    second = sw.backward(ref, srcs, rel, dv, rec, gcost, want_grad_x=True)
    torch.cuda.synchronize()
    return ev, cost, gcost, first, second


def _check(label, feats, proj, dv, wseed):
    """The forward against the oracle's sweep and the backward against float64 autograd, the
    feature gradient per (view, batch element) slice.  Returns the GPU results."""
    from oracle import sweep_oracle as orc
    N, B, C, H, W = feats.shape
    D = dv.shape[1]
    P = _weights(wseed)
    want = orc.sweep(*_views(feats, proj), dv, P)
    R = torch.randn(B, D, H, W, generator=torch.Generator().manual_seed(5))
    Rd = R.to(DEV)

    def gcost_of(cost):   # dL/dcost of sum(R * softmax(cost))
        prob = torch.softmax(cost, dim=1)
        return prob * (Rd - (Rd * prob).sum(dim=1, keepdim=True))

    ev, cost, gcost, first, second = _gpu_run(feats, proj, dv, P, gcost_of)
    # forward
    np.testing.assert_allclose(cost.cpu().numpy(), want["cost"].numpy(), atol=1e-4, rtol=1e-4)
    l1 = rel_l1(ev["depth"].cpu().numpy(), want["depth"].numpy())
    cerr = float((ev["conf"].cpu() - want["conf"]).abs().max())
    print(f"\n== {label}: B, N, H, W, D = {(B, N, H, W, D)}")
    print(f"forward: cost max|err| {float((cost.cpu() - want['cost']).abs().max()):.3e}, "
          f"depth rel-L1 {l1:.3e}, conf max|err| {cerr:.3e}")
    assert l1 <= 1e-3
    np.testing.assert_allclose(ev["conf"].cpu().numpy(), want["conf"].numpy(), atol=1e-4)
    # backward: float64 autograd, float32 autograd's spread
    tsum = [0.0]   # sum of |dL/d omega logit|: the terms of the logits' bias gradient
    orc.LOGIT_HOOK = lambda z: z.register_hook(lambda g: tsum.__setitem__(0, tsum[0] + float(g.abs().sum())))
    try:
        g64 = _oracle_grads(feats, proj, dv, P, R, torch.float64)
    finally:
        orc.LOGIT_HOOK = None
    prob64, gf64, gp64, gx64 = g64
    e32 = _f32_spread(feats, proj, dv, P, R, g64)
    np.testing.assert_allclose(torch.softmax(cost, dim=1).cpu().numpy(), prob64.numpy(), atol=1e-5)
    g_ref, g_src, gp, gx = first
    gfeat = torch.stack([g_ref] + g_src).cpu().numpy()
    assert np.isfinite(gfeat).all() and np.isfinite(gf64.numpy()).all()
    gx = gx.permute(0, 1, 4, 2, 3).cpu().numpy()   # [D,B,32,H,W]
    errs = {"x": (rel_l2(gx, np.stack([g.numpy() for g in gx64])), e32["x"]),
            "features": (rel_l2(gfeat, gf64.numpy()), e32["features"])}
    for v in range(N):
        for b in range(B):
            k = f"features[{v},{b}]"
            errs[k] = (rel_l2(gfeat[v, b], gf64[v, b].numpy()), e32[k])
    for k, g in gp.items():
        if k != "cost_regularization.conv_0.bias":   # true gradient 0 (softmax over D)
            errs["all:" + k] = (rel_l2(g.cpu().numpy(), gp64[k].numpy()), e32[k])
    print(f"relative L2 vs float64 (gpu, cpu float32 max over threads {F32_THREADS}):")
    for k, (e, c) in errs.items():
        print(f"  {k:52s} {e:.3e} {c:.3e}")
    ulp_sum = abs(float(gp[KB]) - float(gp64[KB])) / (2.0 ** -24 * tsum[0])
    print(f"  all:{KB} |error| / (u sum|terms|) = {ulp_sum:.3f}")
    worst = max(errs, key=lambda k: errs[k][0] / bound(k, errs[k][1]))
    print(f"  worst error / bound: {errs[worst][0] / bound(worst, errs[worst][1]):.3f} ({worst})")
    loose = [k for k, (_, c) in errs.items() if bound(k, c) > 1e-3]
    if loose:   # float32 autograd itself too far from float64 to say anything about the GPU
        print(f"  bound above 1e-3: {loose}")
    bad = {k: e for k, e in errs.items()
           if not (e[0] <= bound(k, e[1]) or (k == "all:" + KB and ulp_sum <= 0.5))}
    assert not bad, bad
    assert abs(float(gp["cost_regularization.conv_0.bias"])) <= 1e-5 * float(gcost.abs().sum())
    # the second backward, bit for bit
    assert torch.equal(first[0], second[0])
    for v, (x, y) in enumerate(zip(first[1], second[1])):
        assert torch.equal(x, y), v
    for k in first[2]:
        assert torch.equal(first[2][k], second[2][k]), k
    return ev, cost, first


@pytest.mark.parametrize("kind", gc.KINDS)
def test_single_geometry_matches_oracle_and_float64_autograd(kind):
    """B = 1, N = 3, D = 5: source view 1 under the case, view 2 plain.  36x52 (44x60 for
    magnify, whose oversized boxes need whole tiles inside the zoomed frame): H and W are no
    multiples of the 16-px tile."""
    B, N, D = 1, 3, 5
    H, W = (44, 60) if kind == "magnify" else (36, 52)
    sc = syn.scene(B, N, H, W, D, seed=31)
    proj = gc.apply(torch.from_numpy(sc["proj_matrices"]), [(0, 1, kind)], H, W)
    _check(kind, torch.from_numpy(sc["features"]), proj, torch.from_numpy(sc["depth_values"]), 6)


MIXED = (2, 4, 24, 40, 18)
MIXED_VIEWS = ((0, 1, "minify"), (0, 2, "rotate"), (0, 3, None),
               (1, 1, "behind"), (1, 2, "magnify"), (1, 3, "shift"))


# The feature seed of the mixed batch is chosen by the reference's own error alone.  The case
# has 1.2 M ReLU inputs in the omega network; float32 autograd samples ~2e-6 px off float64's
# position, and a ReLU input that close to zero takes the other branch in float64.  One such
# pixel is 1e-4 of a feature slice and, the omega parameters' gradients being sums of terms of
# either sign, 1e-3 of those: at 7 of the 16 seeds 37..52 float32 autograd's own error is
# above 3e-4 for some tensor (3.2e-3 at seed 37), and twice that bounds nothing.  46 is the seed of
# that range with the smallest worst float32 error (4.7e-6, every tensor; profiles/
# geometry_backward_errors.txt), so every bound of the case is the 2e-5 floor.
MIXED_SEED = 46


@functools.lru_cache(maxsize=None)
def _mixed(seed=MIXED_SEED):
    """(features [N,B,32,H,W], proj [B,N,4,4], depth_values [B,D]) of the mixed batch: element 0
    sees (minify, rotate, plain) on the scene's depths, element 1 (behind, magnify, shift) on
    linspace(1200, 600, D).  Shared, never modified."""
    B, N, H, W, D = MIXED
    sc = syn.scene(B, N, H, W, D, seed=seed)
    proj = gc.apply(torch.from_numpy(sc["proj_matrices"]), MIXED_VIEWS, H, W)
    dv = torch.from_numpy(sc["depth_values"]).clone()
    dv[1] = torch.linspace(1200.0, 600.0, D)
    return torch.from_numpy(sc["features"]), proj, dv


def test_mixed_batch_matches_oracle_and_float64_autograd():
    """Cameras and depths that differ across the batch: fails if any rel or depth index of the
    sweep or its backward drops b.  The same run with element 1's cameras and depths copied
    from element 0 gives another result, so the inputs matter."""
    feats, proj, dv = _mixed()
    ev, cost, (g_ref, g_src, gp, _) = _check("mixed batch", feats, proj, dv, 6)
    proj0, dv0 = proj.clone(), dv.clone()
    proj0[1], dv0[1] = proj[0], dv[0]
    ev0, cost0, _, (g_ref0, g_src0, _, _), _ = _gpu_run(feats, proj0, dv0, _weights(6),
                                                      lambda c: torch.ones_like(c))
    assert not torch.equal(cost[1], cost0[1]) and not torch.equal(ev["depth"][1], ev0["depth"][1])
    # element 0's cost differs from the copy run's by rounding at the most (shared scales)
    torch.testing.assert_close(cost[0], cost0[0], atol=1e-4, rtol=1e-4)
    assert float((cost[1] - cost0[1]).abs().max()) > 1e-2


def test_standalone_warp_matches_oracle_per_batch_element():
    """aarmvs_homo_warp and aarmvs_homo_warp_backward on the mixed batch's rel [B,3,4] and
    per-element depths, one call per source view: the warp at the fixture test's atol 1e-5, its
    backward per batch element within max(2e-5, 2 x float32 grid_sample's own error) relative
    L2 of float64 autograd through the oracle's warp."""
    from aarmvs import ops
    from oracle import sweep_oracle as orc
    feats, proj, dv = _mixed()
    N, B, C, H, W = feats.shape
    gout = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(7))
    print("\n== standalone warp backward, relative L2 vs float64 per (view, b) (gpu, cpu float32):")
    prev = torch.get_num_threads()
    for v in range(1, N):
        rel = ops.relative_projection(proj[:, v], proj[:, 0])
        assert torch.equal(rel, orc.relative_projection(proj[:, v], proj[:, 0]))
        for d in (0, 7, 16, 17):
            dep = dv[:, d].contiguous()
            got = ops.homo_warp(feats[v].to(DEV), rel, dep).cpu().numpy()
            np.testing.assert_allclose(got, orc.homo_warp(feats[v], rel, dep).numpy(), atol=1e-5, rtol=0)
            s64 = feats[v].double().requires_grad_(True)
            orc.homo_warp(s64, rel, dep, fast=True).backward(gout.double())
            e32 = np.zeros(B)
            try:
                for n in F32_THREADS:
                    torch.set_num_threads(n)
                    s32 = feats[v].clone().requires_grad_(True)
                    orc.homo_warp(s32, rel, dep, fast=True).backward(gout)
                    e32 = np.maximum(e32, [rel_l2(s32.grad[b].numpy(), s64.grad[b].numpy()) for b in range(B)])
            finally:
                torch.set_num_threads(prev)
            gb = ops.homo_warp_backward(gout.to(DEV), rel, dep, (B, C, H, W)).cpu().numpy()
            for b in range(B):
                e = rel_l2(gb[b], s64.grad[b].numpy())
                print(f"  view {v} plane {d:2d} b {b}: {e:.3e} {e32[b]:.3e}")
                assert e <= max(2e-5, 2.0 * e32[b]), (v, d, b, e, e32[b])


def test_standalone_cost_slice_and_wta_match_per_batch_element():
    """aarmvs_cost_slice on the mixed batch at depth [B] with unequal entries against the
    oracle's slice (atol 1e-4), and aarmvs_wta_update over the sweep's cost volume with
    per-element depths against the sweep's fused WTA, bit for bit."""
    from aarmvs import ops
    from oracle import sweep_oracle as orc
    feats, proj, dv = _mixed()
    N, B, C, H, W = feats.shape
    D = dv.shape[1]
    P = _weights(6)
    sw = ops.DepthSweep({k: v.to(DEV) for k, v in P.items()}, DEV)
    ref, srcs, ref_proj, src_projs = _views(feats.to(DEV), proj)
    rels = [orc.relative_projection(sp, ref_proj) for sp in src_projs]
    for d in (0, 9, 17):
        dep = dv[:, d].contiguous()
        x, _ = sw.cost_slice(ref, srcs, ref_proj, src_projs, dep)
        want = orc.cost_slice(feats[0], [feats[v] for v in range(1, N)], rels, dep, P)
        np.testing.assert_allclose(x.cpu().numpy(), want.numpy(), atol=1e-4, rtol=0)
    out = sw(ref, srcs, ref_proj, src_projs, dv, want_cost=True)
    mp, dm, es = (torch.zeros(B, H, W, device=DEV) for _ in range(3))
    for d in range(D):
        ops.wta_update(out["cost"][:, d].contiguous(), dv[:, d], mp, dm, es)
    assert torch.equal(dm, out["depth"])
    assert torch.equal(mp / es, out["conf"])
    # both depth lists are in use: element 1's depths come from its own, descending list
    assert set(np.unique(out["depth"][1].cpu().numpy())) <= set(dv[1].numpy()) | {0.0}
    assert not set(np.unique(out["depth"][1].cpu().numpy())) <= set(dv[0].numpy()) | {0.0}
