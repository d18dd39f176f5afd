#!/usr/bin/env python3
"""How often do consecutive depth planes of a sweep share their bilinear taps?

cost_x with PP planes per thread (cost_x_planes_kernel, AARMVS_COST_X_PLANES) reloads a
(pixel, view)'s four taps for plane d + 1 only where the tap floor (floor(ix), floor(iy)) differs
from plane d's.  This tool evaluates the kernel's sampling positions on the CPU (fp32, sample_pos's
operation order) and reports, per source view and overall, the share of follower-plane work that
must reload, at three granularities of the kernel's layout (two lanes per pixel, a wave = 32
pixels of one row):

* ``lane``  a pixel's lane pair (the floor differs),
* ``quad``  4 lanes = 2 neighbouring pixels, at least one of which reloads,
* ``wave``  32 pixels of a row (aligned to 32), at least one of which reloads.

Follower planes are planes 1 .. PP-1 of each PP-aligned block of the plane range (plane groups
are multiples of 4 planes long, so the blocks are the kernel's).  Needs no GPU.

    python tools/tap_coincidence.py dtu_eval_1600x1184_n7_d512
    python tools/tap_coincidence.py --all
    python tools/tap_coincidence.py --cams ref_cam.txt src1_cam.txt ... --height 128 --width 160 --planes 192
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "aa-rmvsnet_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

WAVE_PIXELS = 32
F32 = np.float32


def relative(ref_proj: np.ndarray, src_projs: np.ndarray) -> np.ndarray:
    """rows 0..2 of src @ inv(ref) in fp32, [nsrc,3,4] (aarmvs.ops.relative_projection)."""
    inv = np.linalg.inv(np.asarray(ref_proj, F32))
    return np.stack([(np.asarray(s, F32) @ inv)[:3, :4] for s in src_projs]).astype(F32)


def tap_floor(m: np.ndarray, depth, ys: np.ndarray, H: int, W: int):
    """(floor(ix), floor(iy)) [len(ys), W] fp32 of rows ``ys`` for one view's rel ``m`` [3,4] and
    one depth: sample_pos's operations, each rounded to fp32 (the fma in fp64, whose product is
    exact)."""
    m = np.asarray(m, F32)
    depth = F32(depth)
    x = np.arange(W, dtype=F32)[None, :]
    y = np.asarray(ys, F32)[:, None]
    with np.errstate(all="ignore"):
        p = []
        for k in range(3):
            rx = (m[k, 0] * x + m[k, 1] * y) + m[k, 2]
            p.append(rx * depth + m[k, 3])
        z = np.where(p[2] == 0, p[2] + F32(1e-4), p[2])
        gx = (p[0] / z) / F32((W - 1) * 0.5) - F32(1)
        gy = (p[1] / z) / F32((H - 1) * 0.5) - F32(1)
        ix = ((gx + F32(1)).astype(np.float64) * (W * 0.5) - 0.5).astype(F32)
        iy = ((gy + F32(1)).astype(np.float64) * (H * 0.5) - 0.5).astype(F32)
        return np.floor(ix), np.floor(iy)


def _any_blocks(r: np.ndarray, n: int) -> np.ndarray:
    """[rows, W] bool -> [rows, ceil(W / n)]: any() over aligned runs of n pixels."""
    rows, W = r.shape
    pad = (-W) % n
    if pad:
        r = np.concatenate([r, np.zeros((rows, pad), bool)], axis=1)
    return r.reshape(rows, -1, n).any(axis=2)


def reload_shares(rel: np.ndarray, depths, H: int, W: int, pp: int, row_step: int = 1,
                  block_step: int = 1) -> dict:
    """Reload shares of the follower planes for ``pp`` planes per thread.

    rel [nsrc,3,4], depths [D].  ``row_step`` / ``block_step`` subsample image rows and plane
    blocks (whole rows and whole blocks, so quads and waves stay what the kernel sees).
    Returns {"views": [{"lane", "quad", "wave"} per view], "all": {...}, "followers": count};
    a share is NaN when there is no follower plane."""
    depths = np.asarray(depths, F32).reshape(-1)
    ys = np.arange(0, H, max(1, row_step))
    views = []
    tot = np.zeros((3, 2))
    followers = 0
    for m in rel:
        cnt = np.zeros((3, 2))   # (reloading, all) for lane, quad, wave
        for d0 in range(0, len(depths), pp * max(1, block_step)):
            prev = tap_floor(m, depths[d0], ys, H, W)
            for d in range(d0 + 1, min(d0 + pp, len(depths))):
                cur = tap_floor(m, depths[d], ys, H, W)
                # the kernel's test: a NaN never compares equal and reloads
                r = ~((cur[0] == prev[0]) & (cur[1] == prev[1]))
                for i, n in enumerate((1, 2, WAVE_PIXELS)):
                    b = _any_blocks(r, n)
                    cnt[i] += (b.sum(), b.size)
                prev = cur
                followers += 1
        views.append({k: (cnt[i, 0] / cnt[i, 1] if cnt[i, 1] else float("nan"))
                      for i, k in enumerate(("lane", "quad", "wave"))})
        tot += cnt
    allv = {k: (tot[i, 0] / tot[i, 1] if tot[i, 1] else float("nan"))
            for i, k in enumerate(("lane", "quad", "wave"))}
    return {"views": views, "all": allv, "followers": followers // max(1, len(rel))}


def loads_per_plane(share: float, pp: int, followers_per_block: float | None = None) -> float:
    """Tap loads per plane against one plane per thread: (1 + followers * share) / planes."""
    f = pp - 1 if followers_per_block is None else followers_per_block
    return (1.0 + f * share) / (1.0 + f)


def bench_configs() -> dict:
    """bench.py's CONFIGS table, read without running the benchmark's imports."""
    with open(os.path.join(ROOT, "bench.py")) as f:
        src = f.read()
    start = src.index("CONFIGS = {")
    ns: dict = {}
    exec(src[start:src.index("}\n", start) + 1], ns)
    return ns["CONFIGS"]


def config_geometry(name: str):
    """(rel, depths, H, W) of a bench.py configuration (synthetic.scene's cameras and depths)."""
    from aarmvs import synthetic as syn
    c = bench_configs()[name]
    proj = syn.camera_projections(c["N"], c["H"], c["W"])
    return relative(proj[0], proj[1:]), syn.depth_hypotheses(c["D"]), c["H"], c["W"]


def cams_geometry(files, H: int, W: int, planes: int, interval_scale: float):
    """(rel, depths, H, W) from camera files (the first is the reference view), with the training
    loader's depth values of the reference camera."""
    from datasets import cams
    K, E, dmin, dint = cams.read_cam(files[0], interval_scale=interval_scale)[:4]
    ref = cams.projection(K, E)
    srcs = []
    for f in files[1:]:
        k, e = cams.read_cam(f, interval_scale=interval_scale)[:2]
        srcs.append(cams.projection(k, e))
    depths = cams.train_depth_values(dmin, dint, planes)[0]
    return relative(ref, np.stack(srcs)), depths, H, W


def report(title: str, rel, depths, H, W, pps, row_step, block_step, out=sys.stdout):
    print(f"{title}: {W}x{H}, {len(rel)} source views, D={len(depths)}"
          f" (every {row_step}. row, every {block_step}. plane block)", file=out)
    for pp in pps:
        r = reload_shares(rel, depths, H, W, pp, row_step, block_step)
        print(f"  {pp} planes per thread   lane   quad   wave", file=out)
        for v, s in enumerate(r["views"]):
            print(f"    view {v + 1:2d}            {s['lane']:6.3f} {s['quad']:6.3f} {s['wave']:6.3f}",
                  file=out)
        a = r["all"]
        print(f"    all views          {a['lane']:6.3f} {a['quad']:6.3f} {a['wave']:6.3f}"
              f"   tap loads per plane x{loads_per_plane(a['lane'], pp):.2f} (lanes)"
              f" x{loads_per_plane(a['quad'], pp):.2f} (quads)", file=out)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("config", nargs="?", help="a bench.py configuration name")
    ap.add_argument("--all", action="store_true", help="every bench.py configuration")
    ap.add_argument("--cams", nargs="+", help="camera files, the reference view first")
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=160)
    ap.add_argument("--planes", type=int, default=192)
    ap.add_argument("--interval-scale", type=float, default=1.06)
    ap.add_argument("--pp", type=int, nargs="+", default=[2, 4], help="planes per thread")
    ap.add_argument("--row-step", type=int, default=16, help="evaluate every n-th image row")
    ap.add_argument("--block-step", type=int, default=8, help="evaluate every n-th plane block")
    a = ap.parse_args(argv)
    if a.cams:
        g = cams_geometry(a.cams, a.height, a.width, a.planes, a.interval_scale)
        report("cameras " + os.path.dirname(a.cams[0]), *g, a.pp, a.row_step, a.block_step)
        return 0
    names = []
    if a.all:
        names = list(bench_configs())
    elif a.config:
        names = [a.config]
    else:
        ap.error("give a configuration name, --all or --cams")
    for n in names:
        report(n, *config_geometry(n), a.pp, a.row_step, a.block_step)
    return 0


if __name__ == "__main__":
    sys.exit(main())
