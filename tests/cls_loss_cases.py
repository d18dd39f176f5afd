"""Inputs of the classification-loss tests, regenerated from seeds (numpy PCG64, as
aarmvs.synthetic) by both the fixture generator (tests/golden/make_cls_loss_golden.py, which runs
the reference on them) and the GPU tests; tests/golden/cls_loss.npz holds their digests.

Every case is the smallest shape at which a path of the kernels is taken: D below, at and past
the 8-plane unroll, one partly filled block, several blocks (the fixed-order reduce), per-element
depth lists and masks, a descending list, and the index rule's corner cases.
"""
from __future__ import annotations

import numpy as np

# name: (B, D, H, W, cost scale, seed, kind)
CASES = {
    "d1_4x4": (1, 1, 4, 4, 3.0, 11, "plain"),
    "d2_4x4": (1, 2, 4, 4, 3.0, 12, "plain"),
    "d5_4x4": (1, 5, 4, 4, 3.0, 13, "plain"),
    "d1_4x132": (1, 1, 4, 132, 3.0, 14, "plain"),
    "d2_4x132": (1, 2, 4, 132, 3.0, 15, "plain"),
    "d5_4x132": (1, 5, 4, 132, 3.0, 16, "plain"),
    "b2_d48_52x84": (2, 48, 52, 84, 8.0, 17, "plain"),       # 18 blocks per element
    "d192_8x12": (1, 192, 8, 12, 8.0, 18, "plain"),          # config 4's depth count
    "d37_16x20_descending": (1, 37, 16, 20, 8.0, 19, "descending"),
    "on_hypothesis": (1, 16, 8, 8, 10.0, 20, "on_hypothesis"),
    "midway": (1, 16, 8, 8, 3.0, 21, "midway"),              # first-minimum tie
    "out_of_range": (1, 16, 8, 8, 10.0, 22, "out_of_range"),
    "gt0_under_mask0": (1, 16, 8, 8, 3.0, 23, "gt0_under_mask0"),
    "all_zero_mask": (2, 9, 8, 12, 3.0, 24, "all_zero_mask"),   # element 1: no valid pixel
    "half_mask": (1, 16, 8, 8, 3.0, 25, "half_mask"),        # half-to-even index rounding
    "tied_maximum": (1, 12, 8, 8, 3.0, 26, "tied_maximum"),  # two bit-equal maxima per pixel
}
# the gradient of this case is kept in the fixture at every GRAD_STRIDE-th pixel only (all D
# planes of it, both batch elements, every block): the whole float64 volume is 3.4 MB
GRAD_STRIDE = {"b2_d48_52x84": 16}


def build(name: str) -> dict:
    """float32 inputs of a case: cost [B,D,H,W], depth_gt / mask [B,H,W], depth_values [B,D]."""
    B, D, H, W, scale, seed, kind = CASES[name]
    rng = np.random.default_rng(seed)
    cost = (rng.standard_normal((B, D, H, W)) * scale).astype(np.float32)
    # a different depth list per batch element; integers 8 apart: midpoints are exact in float32
    lo = 424.0 + 48.0 * np.arange(B)
    step = 8.0 + 2.0 * np.arange(B)
    dv = (lo[:, None] + step[:, None] * np.arange(D)[None, :]).astype(np.float32)
    if kind == "descending":   # inverse-depth sampling: 1 / linspace(1 / near, 1 / far) reversed
        inv = np.linspace(1.0 / 935.0, 1.0 / 425.0, D)
        dv = np.broadcast_to((1.0 / inv).astype(np.float32), (B, D)).copy()
        assert np.all(np.diff(dv, axis=1) < 0)
    near, far = dv.min(1)[:, None, None], dv.max(1)[:, None, None]
    gt = (near + (far - near) * rng.random((B, H, W))).astype(np.float32)
    mask = (rng.random((B, H, W)) < 0.7).astype(np.float32)
    idx = rng.integers(0, D, (B, H, W))
    pick = np.take_along_axis(dv, idx.reshape(B, -1), 1).reshape(B, H, W)
    if kind == "on_hypothesis":
        gt = pick.copy()
    elif kind == "midway":
        nxt = np.take_along_axis(dv, np.minimum(idx + 1, D - 1).reshape(B, -1), 1).reshape(B, H, W)
        gt = ((pick + nxt) * 0.5).astype(np.float32)
    elif kind == "out_of_range":
        gt = np.where(rng.random((B, H, W)) < 0.5, near - 100.0, far + 250.0).astype(np.float32)
    elif kind == "gt0_under_mask0":
        gt = np.where(mask > 0, gt, 0.0).astype(np.float32)
    elif kind == "all_zero_mask":
        mask[1] = 0.0
    elif kind == "half_mask":
        gt = pick.copy()    # argmin = idx: odd and even indices under mask 0.5
        mask = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), (B, H, W))
    elif kind == "tied_maximum":
        i, j = 3, 7
        top = np.abs(cost).max() + 1.0
        cost[:, i] = cost[:, j] = np.float32(top)
    return {"cost": cost, "depth_gt": gt, "mask": mask, "depth_values": dv}
