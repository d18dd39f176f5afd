"""cost_x with several planes per thread (AARMVS_COST_X_PLANES = 2, 4) against one plane per
thread (= 1): the sweep's outputs must be equal bit for bit.

A thread of the multi-plane kernel keeps a (pixel, view)'s four taps in registers from one
plane to the next and reloads them only where the tap floor moved, so the cases are chosen by how
many lanes reload: some (consecutive planes of a 512-plane sweep), all (planes far apart), none
(planes a hair apart), plus ragged plane blocks, a sweep split into calls, and positions behind
a source camera (NaN / infinite positions, z = 0).  The three reload regimes are asserted from
tools/tap_coincidence.py on the very cameras and depths the case runs, so that a change to the
synthetic cameras cannot quietly empty a case.

The synthetic cameras' baseline (20 mm per view at focal length W) gives sub-pixel disparities
at these small widths: a 512-plane step moves a tap by about 0.01 px, and a whole-range step of
D = 6 by less than one.  The cases therefore scale the baseline by 1600 / W, which gives the
small frames the headline frame's disparities in pixels (0.04 .. 1 px per plane of 512).
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from aarmvs import synthetic as syn

pytestmark = pytest.mark.gpu

DEV = "cuda"
ENV = "AARMVS_COST_X_PLANES"
KEYS = ("cost", "slice", "omega", "depth", "conf")
SHAPES = [(2, 3, 64, 96),     # whole 4 x 32 tiles, two batch elements (blockIdx.y)
          (1, 4, 68, 100)]    # ragged on the right and at the bottom


def _tool():
    spec = importlib.util.spec_from_file_location(
        "tap_coincidence", os.path.join(ROOT, "tools", "tap_coincidence.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


tc = _tool()


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from aarmvs import ops  # noqa: F401  (loads libaarmvs.so, raises if missing)


def make_scene(B, N, H, W, depths, seed):
    rng = np.random.default_rng(seed)
    feats = torch.from_numpy(rng.standard_normal((N, B, 32, H, W), dtype=np.float32))
    proj = syn.camera_projections(N, H, W, baseline=20.0 * 1600.0 / W)
    proj = torch.from_numpy(np.broadcast_to(proj, (B, N, 4, 4)).copy())
    dv = torch.from_numpy(np.broadcast_to(np.asarray(depths, np.float32), (B, len(depths))).copy())
    return feats, proj, dv


def lane_shares(proj, dv, H, W):
    """Follower-lane reload share over all views for 2 and 4 planes per thread, on the relative
    projections the sweep itself uses."""
    from aarmvs import ops
    N = proj.shape[1]
    rel = np.stack([ops.relative_projection(proj[:1, v], proj[:1, 0])[0].numpy()
                    for v in range(1, N)])
    return [tc.reload_shares(rel, dv[0].numpy(), H, W, pp)["all"]["lane"] for pp in (2, 4)]


def sweep_outputs(pp, feats, proj, dv, wseed, pieces=None):
    """The sweep's outputs under AARMVS_COST_X_PLANES=pp; ``pieces``: the d_range calls."""
    from aarmvs import ops
    N = feats.shape[0]
    old = os.environ.get(ENV)
    os.environ[ENV] = str(pp)
    try:
        P = {k: torch.from_numpy(v).to(DEV) for k, v in syn.sweep_weights(wseed).items()}
        sw = ops.DepthSweep(P, DEV)
        fd = feats.to(DEV)
        args = (fd[0], [fd[v] for v in range(1, N)], proj[:, 0], [proj[:, v] for v in range(1, N)], dv)
        if pieces is None:
            out = sw(*args, want_cost=True, debug=True)
        else:
            B, _, H, W = fd[0].shape
            cost = torch.empty(B, dv.shape[1], H, W, device=DEV)
            for d0, d1 in pieces:
                out = sw(*args, d_range=(d0, d1), cost_out=cost, debug=True)
        torch.cuda.synchronize()
        return {k: out[k].cpu() for k in KEYS}
    finally:
        if old is None:
            del os.environ[ENV]
        else:
            os.environ[ENV] = old


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_planes(feats, proj, dv, wseed, pieces=None):
    ref = sweep_outputs(1, feats, proj, dv, wseed)
    for pp in (2, 4):
        got = sweep_outputs(pp, feats, proj, dv, wseed, pieces)
        for k in KEYS:
            assert same_bits(got[k], ref[k]), (pp, k)
    return ref


@pytest.mark.parametrize("B,N,H,W", SHAPES)
def test_mixed_masks(B, N, H, W):
    """Six consecutive planes of the 512-plane sweep: some lanes of most waves reload."""
    feats, proj, dv = make_scene(B, N, H, W, syn.depth_hypotheses(512)[:6], seed=31)
    for s in lane_shares(proj, dv, H, W):
        assert 0.1 <= s <= 0.6, s
    check_planes(feats, proj, dv, wseed=3)


@pytest.mark.parametrize("B,N,H,W", SHAPES)
def test_all_reload(B, N, H, W):
    """D = 6 over the whole depth range: shifts of many pixels, every lane reloads."""
    feats, proj, dv = make_scene(B, N, H, W, syn.depth_hypotheses(6), seed=32)
    for s in lane_shares(proj, dv, H, W):
        assert s >= 0.95, s
    check_planes(feats, proj, dv, wseed=4)


@pytest.mark.parametrize("B,N,H,W", SHAPES)
def test_none_reload(B, N, H, W):
    """Six planes within a 1e-4 relative span around mid-range: whole waves skip the reload."""
    mid = 0.5 * (425.0 + 935.0)
    feats, proj, dv = make_scene(B, N, H, W, mid * (1.0 + np.linspace(-0.5e-4, 0.5e-4, 6)), seed=33)
    for s in lane_shares(proj, dv, H, W):
        assert s <= 0.02, s
    check_planes(feats, proj, dv, wseed=5)


@pytest.mark.parametrize("D", [5, 1])
@pytest.mark.parametrize("B,N,H,W", SHAPES)
def test_tails(B, N, H, W, D):
    """A ragged last plane block (5 = 2 + 2 + 1 = 4 + 1) and a single plane."""
    feats, proj, dv = make_scene(B, N, H, W, syn.depth_hypotheses(512)[200:200 + D], seed=34)
    check_planes(feats, proj, dv, wseed=6)


@pytest.mark.parametrize("B,N,H,W", SHAPES)
def test_split_sweep(B, N, H, W):
    """D = 6 run as d_range pieces (0, 3) + (3, 6) equals one call (of one plane per thread)."""
    feats, proj, dv = make_scene(B, N, H, W, syn.depth_hypotheses(512)[300:306], seed=35)
    check_planes(feats, proj, dv, wseed=7, pieces=[(0, 3), (3, 6)])


def test_behind_the_camera():
    """The geometry of test_gpu_parity's behind-the-camera sweep: a source projection whose z row
    is mixed with its x row, so that z' changes sign across the image (NaN and infinite
    positions, z = 0, positions far outside the image)."""
    from aarmvs import ops
    B, N, H, W, D = 1, 3, 64, 160, 4
    sc = syn.scene(B, N, H, W, D, seed=23)
    proj = torch.from_numpy(sc["proj_matrices"]).clone()
    M = torch.eye(4)
    M[2, 0] = -1.0 / (W / 2)
    proj[:, 2] = M @ proj[:, 2]
    rel = ops.relative_projection(proj[:, 2], proj[:, 0])[0].numpy()
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    zs = [(rel[2, 0] * xs + rel[2, 1] * ys + rel[2, 2]) * d + rel[2, 3] for d in sc["depth_values"][0]]
    neg = float(np.mean(np.stack(zs) <= 0))
    assert 0.1 < neg < 0.9, neg
    check_planes(torch.from_numpy(sc["features"]), proj, torch.from_numpy(sc["depth_values"]), wseed=6)
