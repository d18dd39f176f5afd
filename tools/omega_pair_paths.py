#!/usr/bin/env python3
"""Which path does each omega_conv item take, and how large is a plane pair's source box?

omega_mfma_kernel (AARMVS_OMEGA_PLANES=2) runs planes kp, kp + 1 of one (tile, view) as one item
on the union of their source boxes when both planes lie in the same block of ``ipb`` consecutive
items and the union fits the LDS box capacity; otherwise the planes run as single items, each in
LDS if its own box fits and on the global-gather path if not.  This tool restates that walk on
the CPU from the kernel's sampling arithmetic (tap_coincidence.tap_floor, box_extend's clamps,
16 x 16 haloed tiles with a 14 x 14 interior) and reports

* per (tile, view, pair): pair in LDS / pair split into singles, and per single item: LDS /
  global path (``omega_paths``),
* single and union box sizes in pixels (``box_sizes``; the table of DESIGN.md section 4).

Needs no GPU.

    python tools/omega_pair_paths.py dtu_eval_1600x1184_n7_d512
    python tools/omega_pair_paths.py --all --cap 300
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def _tap_coincidence():
    spec = importlib.util.spec_from_file_location("tap_coincidence",
                                                  os.path.join(_HERE, "tap_coincidence.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


tc = _tap_coincidence()

TILE, OUT = 16, 14          # haloed tile edge, its interior (OmegaTile<16>)
BOXPX = 2 * TILE * TILE     # the kernel's LDS box capacity in pixels
PLANE_GROUP = 16            # planes per launch (sweep_schedule.h's kPlaneGroup)
_BIG = 1 << 30


def tiles(H: int, W: int):
    """(tile rows, tile columns)."""
    return (H + OUT - 1) // OUT, (W + OUT - 1) // OUT


def tile_boxes(m, depth, H: int, W: int, tile_rows=None) -> np.ndarray:
    """Source boxes [rows, tiles_x, 4] = (x0, y0, x1, y1) int64 of one view and depth, for the
    tile rows ``tile_rows`` (default: all): box_extend over the tile's in-image haloed pixels.
    A tile with no in-image tap has x0 > x1."""
    ty_n, tx_n = tiles(H, W)
    rows = np.arange(ty_n) if tile_rows is None else np.asarray(tile_rows)
    xf, yf = tc.tap_floor(m, depth, np.arange(H), H, W)
    with np.errstate(invalid="ignore"):
        xl, xh = np.maximum(xf, 0), np.minimum(xf + 1, W - 1)
        yl, yh = np.maximum(yf, 0), np.minimum(yf + 1, H - 1)
        ok = ~(np.isnan(xf) | np.isnan(yf)) & (xl <= xh) & (yl <= yh)

    def grid(a, fill):
        # haloed pixel (hy, hx) of tile (ty, tx) is image pixel (14 ty - 1 + hy, 14 tx - 1 + hx)
        v = np.where(ok, np.where(ok, a, 0).astype(np.int64), fill)
        p = np.full((ty_n * OUT + 2, tx_n * OUT + 2), fill, np.int64)
        p[1:H + 1, 1:W + 1] = v
        w = np.lib.stride_tricks.sliding_window_view(p, (TILE, TILE))[::OUT, ::OUT]
        return w[rows]

    out = np.empty((len(rows), tx_n, 4), np.int64)
    out[..., 0] = grid(xl, _BIG).min(axis=(2, 3))
    out[..., 1] = grid(yl, _BIG).min(axis=(2, 3))
    out[..., 2] = grid(xh, -_BIG).max(axis=(2, 3))
    out[..., 3] = grid(yh, -_BIG).max(axis=(2, 3))
    return out


def box_union(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return np.concatenate([np.minimum(a[..., :2], b[..., :2]), np.maximum(a[..., 2:], b[..., 2:])], -1)


def box_px(b: np.ndarray) -> np.ndarray:
    """nx * ny as box_reduce returns them (an empty extent is 0)."""
    nx = np.where(b[..., 2] >= b[..., 0], b[..., 2] - b[..., 0] + 1, 0)
    ny = np.where(b[..., 3] >= b[..., 1], b[..., 3] - b[..., 1] + 1, 0)
    return nx * ny


def plane_groups(d_begin: int, d_end: int, G: int = PLANE_GROUP):
    """The (first plane, planes) launches of one sweep call over planes d_begin .. d_end - 1."""
    return [(g0, min(G, d_end - g0)) for g0 in range(d_begin, d_end, G)]


def omega_paths(rel, depths, H: int, W: int, cap: int | None = None, ipb: int = 8, groups=None,
                tile_row_step: int = 1, group_step: int = 1) -> dict:
    """Counts of the paths the items of a sweep take under AARMVS_OMEGA_PLANES=2.

    rel [nsrc,3,4], depths [D]; ``cap``: AARMVS_PIPE_BOX_CAP (default: the kernel's capacity);
    ``ipb``: items per block; ``groups``: the launches as (first plane, planes) (default: one
    call over all planes).  ``tile_row_step`` / ``group_step`` subsample tile rows and launches.
    Returns {"pair_lds", "pair_split", "single_lds", "single_global"}: plane pairs that ran as
    one item, pairs whose union exceeded the capacity (they ran as two singles), and the single
    items (those two, and every plane no pair could take) by their own path."""
    depths = np.asarray(depths, np.float32).reshape(-1)
    cap = min(BOXPX, max(4, cap)) if cap is not None else BOXPX
    ipb = max(1, ipb)
    groups = plane_groups(0, len(depths)) if groups is None else list(groups)
    ty_n, tx_n = tiles(H, W)
    rows = np.arange(0, ty_n, max(1, tile_row_step))
    nsrc = len(rel)
    cnt = {"pair_lds": 0, "pair_split": 0, "single_lds": 0, "single_global": 0}
    for g0, n in groups[::max(1, group_step)]:
        for v, m in enumerate(rel):
            bx = [tile_boxes(m, depths[g0 + k], H, W, rows) for k in range(n)]
            px1 = [box_px(b) for b in bx]
            px2 = [box_px(box_union(bx[k], bx[k + 1])) for k in range(n - 1)]
            for ri, ty in enumerate(rows):
                for tx in range(tx_n):
                    base = ((ty * tx_n + tx) * nsrc + v) * n
                    kp = 0
                    while kp < n:
                        run = 1
                        if (base + kp) % ipb + 1 < ipb and kp + 1 < n:
                            if px2[kp][ri, tx] <= cap:
                                cnt["pair_lds"] += 1
                                kp += 2
                                continue
                            cnt["pair_split"] += 1
                            run = 2
                        for k in range(kp, kp + run):
                            cnt["single_lds" if px1[k][ri, tx] <= cap else "single_global"] += 1
                        kp += run
    return cnt


def box_sizes(rel, depths, H: int, W: int, tile_row_step: int = 6, pair_step: int = 8) -> list:
    """Per view: single-box and pair-union sizes over planes (2 k, 2 k + 1), every
    ``pair_step``-th pair and ``tile_row_step``-th tile row: {"single_mean", "single_max",
    "union_mean", "union_max", "ratio", "over"} (ratio: union / single means; over: unions larger
    than the kernel's capacity)."""
    depths = np.asarray(depths, np.float32).reshape(-1)
    rows = np.arange(0, tiles(H, W)[0], max(1, tile_row_step))
    out = []
    for m in rel:
        s, u = [], []
        for k in range(0, len(depths) - 1, 2 * max(1, pair_step)):
            a, b = tile_boxes(m, depths[k], H, W, rows), tile_boxes(m, depths[k + 1], H, W, rows)
            s += [box_px(a).ravel(), box_px(b).ravel()]
            u.append(box_px(box_union(a, b)).ravel())
        s, u = np.concatenate(s), np.concatenate(u)
        out.append({"single_mean": float(s.mean()), "single_max": int(s.max()),
                    "union_mean": float(u.mean()), "union_max": int(u.max()),
                    "ratio": float(u.mean() / max(s.mean(), 1e-9)), "over": int((u > BOXPX).sum())})
    return out


def report(title, rel, depths, H, W, cap, ipb, tile_row_step, pair_step, out=sys.stdout):
    print(f"{title}: {W}x{H}, {len(rel)} source views, D={len(depths)}"
          f" (every {tile_row_step}. tile row, every {pair_step}. plane pair)", file=out)
    print("  view   single px mean / max   union px mean / max   union/single   over capacity",
          file=out)
    for v, r in enumerate(box_sizes(rel, depths, H, W, tile_row_step, pair_step)):
        print(f"  {v + 1:4d}   {r['single_mean']:9.1f} / {r['single_max']:4d}      "
              f"{r['union_mean']:8.1f} / {r['union_max']:4d}      {r['ratio']:6.3f}      {r['over']}",
              file=out)
    c = omega_paths(rel, depths, H, W, cap, ipb, tile_row_step=tile_row_step,
                    group_step=4 * max(1, pair_step))
    print(f"  paths at capacity {cap if cap is not None else BOXPX}, {ipb} items per block"
          f" (every {4 * max(1, pair_step)}. launch): "
          + ", ".join(f"{k} {n}" for k, n in c.items()), file=out)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("config", nargs="?", help="a bench.py configuration name")
    ap.add_argument("--all", action="store_true", help="every bench.py configuration")
    ap.add_argument("--cap", type=int, default=None, help="AARMVS_PIPE_BOX_CAP")
    ap.add_argument("--ipb", type=int, default=8, help="items per block")
    ap.add_argument("--tile-row-step", type=int, default=6)
    ap.add_argument("--pair-step", type=int, default=8)
    a = ap.parse_args(argv)
    if not a.all and not a.config:
        ap.error("give a configuration name or --all")
    for n in (list(tc.bench_configs()) if a.all else [a.config]):
        report(n, *tc.config_geometry(n), a.cap, a.ipb, a.tile_row_step, a.pair_step)
    return 0


if __name__ == "__main__":
    sys.exit(main())
