"""Adversarial camera geometry for the sweep tests, and a numpy qualifier that says which
regime of the cost-slice backward's source-box logic a set of cameras reaches.

``case(kind, H, W)`` is a pixel-space homography G (in the upper-left 3x3 block of a 4x4 M)
applied to a source view's projection as ``proj[:, v] = M @ proj[:, v]``: the source image is
then sampled at G(position) instead of at the plain rig's position.

``reach(rel, depths, H, W)`` describes the inputs only.  It works on the reference's sampling
positions (``oracle.sweep_oracle.homography_grid``) and the z row of ``rel``, and reads nothing
from the library.  The three constants below restate the tile logic it describes.
"""
from __future__ import annotations

import numpy as np
import torch

# the cost-slice backward's tile logic (cost_bwd.hip cbw_feat_kernel): kFbT, the tile edge in
# reference pixels; kFbBoxPx, the largest source box a block owns; kFbSlots, the reference
# pixels a box cell (a top-left tap position) holds per plane.  bptt.hip's kPlaneGroup is PLANES.
TILE = 16
BOX_PX = 768
SLOTS = 2
PLANES = 16

KINDS = ("minify", "magnify", "rotate", "behind", "shift")


def case(kind: str, H: int, W: int) -> torch.Tensor:
    """4x4 float32 M whose upper-left 3x3 block is the case's pixel-space homography."""
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0

    def about_centre(A):
        T = np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1.0]])
        Ti = np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1.0]])
        return T @ A @ Ti

    if kind == "minify":
        G = about_centre(np.diag([0.5, 0.5, 1.0]))
    elif kind == "magnify":
        G = about_centre(np.diag([1.7, 1.7, 1.0]))
    elif kind == "rotate":
        c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
        G = about_centre(np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]))
    elif kind == "behind":
        G = np.eye(3)
        G[2, 0] = -1.0 / (W / 2)
    elif kind == "shift":
        G = np.eye(3)
        G[0, 2], G[1, 2] = 0.75 * W, -0.4 * H
    else:
        raise ValueError(kind)
    M = np.eye(4)
    M[:3, :3] = G
    return torch.from_numpy(M.astype(np.float32))


def apply(proj: torch.Tensor, assignments, H: int, W: int) -> torch.Tensor:
    """A copy of proj [B,N,4,4] with ``proj[b, v] = case(kind) @ proj[b, v]`` for every
    ``(b, v, kind)`` of ``assignments`` (kind None: the view stays plain)."""
    out = proj.clone()
    for b, v, kind in assignments:
        if kind is not None:
            out[b, v] = case(kind, H, W) @ out[b, v]
    return out


def reach(rel, depths, H: int, W: int) -> dict:
    """Figures of one (view, batch element): rel [3,4], depths [D].

    Per 16x16 reference tile and 16-plane group (groups start at multiples of 16 planes, the
    last group possibly ragged; the backward walks them last to first):
      tiles        number of (tile, group) pairs
      behind       pairs with a tile corner at z <= 0 on some plane of the group
      empty        pairs, every corner in front, whose image-clamped bounding box of the
                   corners' bilinear taps is empty
      oversize     pairs, every corner in front, whose box holds more than BOX_PX pixels
    and per (pixel, plane), over every plane:
      overflow     share of pixels whose top-left tap is the top-left tap of more than SLOTS
                   pixels of their tile on that plane
      outside      share of the 4 bilinear taps that lie outside the image
      z_nonpos     share of positions with z <= 0
    """
    from oracle import sweep_oracle as orc
    rel = torch.as_tensor(rel, dtype=torch.float32).reshape(3, 4)
    dep = torch.as_tensor(np.asarray(depths, np.float32))
    D = dep.numel()
    gx, gy = orc.homography_grid(rel.unsqueeze(0).expand(D, 3, 4).contiguous(), dep, H, W)
    ix = (gx.double().numpy() + 1.0) * (W / 2.0) - 0.5      # [D,H,W] source pixel positions
    iy = (gy.double().numpy() + 1.0) * (H / 2.0) - 0.5
    m = rel.double().numpy()
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    z = (m[2, 0] * xs + m[2, 1] * ys + m[2, 2])[None] * dep.double().numpy()[:, None, None] + m[2, 3]
    fin = np.isfinite(ix) & np.isfinite(iy)
    x0 = np.floor(np.where(fin, np.clip(ix, -1e6, 1e6), -1e6)).astype(np.int64)
    y0 = np.floor(np.where(fin, np.clip(iy, -1e6, 1e6), -1e6)).astype(np.int64)

    out = {"tiles": 0, "behind": 0, "empty": 0, "oversize": 0}
    over = 0
    for ty in range(0, H, TILE):
        for tx in range(0, W, TILE):
            y1, x1 = min(ty + TILE, H), min(tx + TILE, W)
            # pixels of the tile sharing one top-left tap, per plane
            for d in range(D):
                key = (y0[d, ty:y1, tx:x1] * (4 * 10 ** 6) + x0[d, ty:y1, tx:x1]).ravel()
                _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
                over += int((cnt[inv] > SLOTS).sum())
            cys, cxs = [ty, y1 - 1], [tx, x1 - 1]
            for g0 in range(0, D, PLANES):
                sl = slice(g0, min(g0 + PLANES, D))
                out["tiles"] += 1
                if (z[sl][:, cys][:, :, cxs] <= 0).any():
                    out["behind"] += 1
                    continue
                bx = x0[sl][:, cys][:, :, cxs]
                by = y0[sl][:, cys][:, :, cxs]
                lx, hx = np.maximum(bx, 0).min(), np.minimum(bx + 1, W - 1).max()
                ly, hy = np.maximum(by, 0).min(), np.minimum(by + 1, H - 1).max()
                if hx < lx or hy < ly:
                    out["empty"] += 1
                elif (hx - lx + 1) * (hy - ly + 1) > BOX_PX:
                    out["oversize"] += 1
    taps_out = 0
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            taps_out += int(((xi < 0) | (xi >= W) | (yi < 0) | (yi >= H)).sum())
    n = D * H * W
    out["overflow"] = over / n
    out["outside"] = taps_out / (4 * n)
    out["z_nonpos"] = float((z <= 0).mean())
    return out
