"""omega_conv with two planes per item (AARMVS_OMEGA_PLANES = 2) against one plane per item
(= 1): the sweep's outputs must be equal bit for bit.

A plane-pair item runs planes kp, kp + 1 of one (tile, view) on the union of their source boxes:
one box reduce, one set of box and reference DMAs and chunk barriers, each plane's arithmetic
unchanged.  A pair forms only inside a block's ``AARMVS_OMEGA_IPB`` consecutive items and inside
one launch's planes; a pair whose union exceeds the LDS capacity runs as two single items, each
in LDS or on the global-gather path by its own box.  The cases therefore cross whole and odd
plane counts, launches of 16, 16 and 5 planes, sweeps cut into d_range pieces inside a pair,
items per block 1 (no pair), 2, 3 (pairs and singles alternate) and 8, and box capacities at
which all three paths occur.  Which paths occur is asserted from tools/omega_pair_paths.py on
the very cameras and depths the case runs, so that a change to the synthetic cameras cannot
quietly empty a case.

As in test_gpu_cost_x_planes.py the synthetic baseline is scaled by 1600 / W, which gives the
small frames the headline frame's disparities in pixels.
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
ENV, ENV_IPB, ENV_CAP = "AARMVS_OMEGA_PLANES", "AARMVS_OMEGA_IPB", "AARMVS_PIPE_BOX_CAP"
KEYS = ("cost", "slice", "omega", "depth", "conf")
SHAPES = [(2, 3, 64, 96),     # blockIdx.z > 0; 64 and 96 are no multiples of the 14-pixel tile
          (1, 4, 68, 100)]    # views 2 and 3 wholly out of frame at the scaled baseline
IPBS = [1, 2, 3, 8]
# box capacities: the kernel's own, and one below the largest single boxes of every shape here
# (15 x 18 = 270 px at 64 x 96, 18 x 18 elsewhere), at which pairs in LDS, pairs split into
# singles and singles on the global path all occur
CAPS = [None, 240]


def _tool():
    spec = importlib.util.spec_from_file_location(
        "omega_pair_paths", os.path.join(ROOT, "tools", "omega_pair_paths.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


opp = _tool()


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


def paths(proj, dv, H, W, cap, ipb, pieces=None):
    """The tool's path counts on the relative projections the sweep itself uses."""
    from aarmvs import ops
    N = proj.shape[1]
    rel = np.stack([ops.relative_projection(proj[:1, v], proj[:1, 0])[0].numpy()
                    for v in range(1, N)])
    D = dv.shape[1]
    groups = [g for d0, d1 in (pieces or [(0, D)]) for g in opp.plane_groups(d0, d1)]
    return opp.omega_paths(rel, dv[0].numpy(), H, W, cap, ipb, groups)


class _Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def sweep_outputs(pp, feats, proj, dv, wseed, ipb=8, cap=None, pieces=None, overlap=True):
    """The sweep's outputs under AARMVS_OMEGA_PLANES=pp; ``pieces``: the d_range calls.  (Items
    per block are always forced: the library's default falls to 1, where no pair can form, on
    frames as small as these.)"""
    from aarmvs import ops
    N = feats.shape[0]
    with _Env(**{ENV: pp, ENV_IPB: ipb, ENV_CAP: cap}):
        P = {k: torch.from_numpy(v).to(DEV) for k, v in syn.sweep_weights(wseed).items()}
        sw = ops.DepthSweep(P, DEV, overlap=overlap)
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


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def assert_same(got, ref, what):
    for k in KEYS:
        assert same_bits(got[k], ref[k]), (what, k)


_REF = {}


def small_scene(shape, D):
    """A small scene of D consecutive planes of the 512-plane sweep and its outputs at one plane
    per item, computed once per (shape, D) and left unchanged."""
    key = (shape, D)
    if key not in _REF:
        B, N, H, W = shape
        sc = make_scene(B, N, H, W, syn.depth_hypotheses(512)[:D], seed=41 + D)
        _REF[key] = (sc, sweep_outputs(1, *sc, wseed=3))
    return _REF[key]


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("ipb", IPBS)
@pytest.mark.parametrize("D", [6, 5])
@pytest.mark.parametrize("shape", SHAPES)
def test_pairs_tails_blocks_and_capacities(shape, D, ipb, cap):
    """Whole pairs (D = 6) and an odd last plane per (tile, view) (D = 5), by items per block and
    box capacity."""
    (feats, proj, dv), ref = small_scene(shape, D)
    H, W = shape[2:]
    p = paths(proj, dv, H, W, cap, ipb)
    if ipb == 1:
        assert p["pair_lds"] == 0 and p["pair_split"] == 0, p
    else:
        assert p["pair_lds"] > 0, p
        if D == 5 or ipb == 3:
            assert p["single_lds"] > 0, p   # planes no pair can take
        if cap is not None:   # all three paths
            assert p["pair_split"] > 0 and p["single_global"] > 0, p
        else:
            assert p["pair_split"] == 0 and p["single_global"] == 0, p
    assert_same(sweep_outputs(2, feats, proj, dv, wseed=3, ipb=ipb, cap=cap), ref, (shape, D, ipb, cap))


@pytest.mark.parametrize("shape", SHAPES)
def test_planes_far_apart_split_at_the_kernels_capacity(shape):
    """D = 6 over the whole depth range: every box moves by many pixels from plane to plane, and
    some unions exceed the kernel's own 512-pixel capacity while their planes' boxes fit."""
    B, N, H, W = shape
    feats, proj, dv = make_scene(B, N, H, W, syn.depth_hypotheses(6), seed=43)
    p = paths(proj, dv, H, W, None, 8)
    assert p["pair_lds"] > 0 and p["pair_split"] > 0 and p["single_global"] == 0, p
    ref = sweep_outputs(1, feats, proj, dv, wseed=4)
    assert_same(sweep_outputs(2, feats, proj, dv, wseed=4), ref, shape)


D37 = (1, 3, 128, 160)
# d_range cuts inside a pair (odd offsets) and at a launch's end (16 planes)
PIECES = [None, [(0, 3), (3, 16), (16, 37)], [(0, 21), (21, 37)]]


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("ipb", IPBS)
@pytest.mark.parametrize("pieces", PIECES, ids=["whole", "3+13+21", "21+16"])
def test_launches_of_16_16_5_and_split_sweeps(pieces, ipb, cap):
    """160 x 128, D = 37: launches of 16, 16 and 5 planes; the same sweep cut into d_range calls
    equals the whole sweep at one plane per item, by items per block and box capacity."""
    (feats, proj, dv), ref = small_scene(D37, 37)
    if pieces is None:
        assert [n for _, n in opp.plane_groups(0, 37)] == [16, 16, 5]
    p = paths(proj, dv, 128, 160, cap, ipb, pieces)
    if ipb == 1:
        assert p["pair_lds"] == 0 and p["pair_split"] == 0, p
    else:
        assert p["pair_lds"] > 0 and p["single_lds"] > 0, p
        if cap is not None:
            assert p["pair_split"] > 0 and p["single_global"] > 0, p
    assert_same(sweep_outputs(2, feats, proj, dv, wseed=3, ipb=ipb, cap=cap, pieces=pieces), ref,
                (pieces, ipb, cap))


@pytest.mark.parametrize("ipb", [3, 8])
def test_behind_the_camera_and_out_of_frame(ipb):
    """The geometry of test_gpu_parity's behind-the-camera sweep (a source projection whose z row
    is mixed with its x row: NaN and infinite positions, z = 0, positions far outside the image)
    on view 2, and view 3 shifted wholly out of frame (empty boxes: no DMA, all taps zero)."""
    from aarmvs import ops
    B, N, H, W, D = 1, 4, 64, 160, 5
    sc = syn.scene(B, N, H, W, D, seed=23)
    proj = torch.from_numpy(sc["proj_matrices"]).clone()
    M = torch.eye(4)
    M[2, 0] = -1.0 / (W / 2)
    proj[:, 2] = M @ proj[:, 2]
    S = torch.eye(4)
    S[0, 2] = 4.0 * W   # x' += 4 W z: four image widths to the right
    proj[:, 3] = S @ proj[:, 3]
    dv = torch.from_numpy(sc["depth_values"])
    rel = ops.relative_projection(proj[:, 2], proj[:, 0])[0].numpy()
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    zs = [(rel[2, 0] * xs + rel[2, 1] * ys + rel[2, 2]) * d + rel[2, 3] for d in sc["depth_values"][0]]
    neg = float(np.mean(np.stack(zs) <= 0))
    assert 0.1 < neg < 0.9, neg
    rel3 = ops.relative_projection(proj[:, 3], proj[:, 0])[0].numpy()
    for d in sc["depth_values"][0]:
        assert (opp.box_px(opp.tile_boxes(rel3, d, H, W)) == 0).all()
    # pairs form on the plain view and on the behind-the-camera view (its unions fit the LDS)
    for v in (1, 2):
        rv = ops.relative_projection(proj[:1, v], proj[:1, 0])[0].numpy()[None]
        p = opp.omega_paths(rv, dv[0].numpy(), H, W, None, ipb)
        assert p["pair_lds"] > 0, (v, p)
    feats = torch.from_numpy(sc["features"])
    ref = sweep_outputs(1, feats, proj, dv, wseed=6)
    assert_same(sweep_outputs(2, feats, proj, dv, wseed=6, ipb=ipb), ref, ipb)


def test_one_stream_and_default_schedule_give_the_same_bits():
    """Two planes per item on the multi-stream default schedule and on one stream."""
    (feats, proj, dv), ref = small_scene(D37, 37)
    assert_same(sweep_outputs(2, feats, proj, dv, wseed=3, overlap=False), ref, "one stream")
    assert_same(sweep_outputs(2, feats, proj, dv, wseed=3, overlap=True), ref, "default schedule")
