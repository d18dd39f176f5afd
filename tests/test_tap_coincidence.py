"""tools/tap_coincidence.py (CPU): the reload shares on hand-made geometry, and its sampling
positions against the oracle's grid."""
import importlib.util
import os

import numpy as np
import torch

from conftest import ROOT
from aarmvs import synthetic as syn


def load_tool():
    spec = importlib.util.spec_from_file_location(
        "tap_coincidence", os.path.join(ROOT, "tools", "tap_coincidence.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


tc = load_tool()

# W - 1 and H - 1 are powers of two, so the grid normalisation is exact
H, W = 17, 33


def translation_rel(k):
    """One view whose sampling position is ix = x + 0.25 + k (2 / d), iy = y + 0.25: with depths
    1 and 2 the second plane is the first one shifted by exactly k pixels.  z = d, so
    px = a x + c + t / d, and ix = px W / (W - 1) - 0.5; the quarter-pixel phase keeps every
    floor away from a rounding."""
    sx, sy = (W - 1) / W, (H - 1) / H
    m = np.zeros((1, 3, 4), np.float32)
    m[0, 0] = [sx, 0, 0.75 * sx, 2 * k * sx]
    m[0, 1] = [0, sy, 0.75 * sy, 0]
    m[0, 2] = [0, 0, 1, 0]
    return m


def test_integer_translation_gives_shares_of_exactly_zero_and_one():
    depths = np.array([1.0, 2.0], np.float32)
    xf, yf = tc.tap_floor(translation_rel(1)[0], depths[0], np.arange(H), H, W)
    assert np.array_equal(xf, np.broadcast_to(np.arange(W, dtype=np.float32) + 2, (H, W)))
    assert np.array_equal(yf, np.broadcast_to(np.arange(H, dtype=np.float32)[:, None], (H, W)))
    still = tc.reload_shares(translation_rel(0), depths, H, W, 2)
    moved = tc.reload_shares(translation_rel(1), depths, H, W, 2)
    for k in ("lane", "quad", "wave"):
        assert still["all"][k] == 0.0 and still["views"][0][k] == 0.0, k
        assert moved["all"][k] == 1.0 and moved["views"][0][k] == 1.0, k
    assert still["followers"] == moved["followers"] == 1


def test_followers_are_counted_per_block_and_granularities_nest():
    """Planes 0, 1 | 2, 3 with 2 per thread: the step 1 -> 2 crosses a block and is not a
    follower step; one moved pixel reloads one lane, one quad and one wave."""
    depths = np.array([1.0, 1.0, 2.0, 2.0], np.float32)
    r = tc.reload_shares(translation_rel(1), depths, H, W, 2)
    assert r["followers"] == 2 and r["all"]["lane"] == 0.0
    r4 = tc.reload_shares(translation_rel(1), depths, H, W, 4)
    assert r4["followers"] == 3 and r4["all"]["lane"] == 1.0 / 3.0
    blocks = tc._any_blocks(np.eye(1, 40, 33, dtype=bool), 32)
    assert blocks.tolist() == [[False, True]]
    assert tc.loads_per_plane(0.3, 2) == (1 + 0.3) / 2 and tc.loads_per_plane(1.0, 4) == 1.0


def test_tap_floor_is_the_oracle_grid_floor():
    """The tool's fp32 restatement of the sampling position gives the floors of the oracle's
    grid (homography_grid, then grid_sample's unnormalisation) on the synthetic cameras."""
    from oracle import sweep_oracle as orc
    Hs, Ws, N = 24, 40, 4
    proj = torch.from_numpy(syn.camera_projections(N, Hs, Ws))
    depths = syn.depth_hypotheses(8)
    for v in range(1, N):
        rel = orc.relative_projection(proj[v:v + 1], proj[0:1])
        for d in depths[[0, 3, 7]]:
            gx, gy = orc.homography_grid(rel, torch.tensor([d]), Hs, Ws)
            ix = orc._fma(gx + 1, Ws / 2, torch.full_like(gx, -0.5))[0].numpy()
            iy = orc._fma(gy + 1, Hs / 2, torch.full_like(gy, -0.5))[0].numpy()
            xf, yf = tc.tap_floor(rel[0].numpy(), d, np.arange(Hs), Hs, Ws)
            assert np.array_equal(xf, np.floor(ix)) and np.array_equal(yf, np.floor(iy))
