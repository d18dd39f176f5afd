"""Cases for the depth-map fusion step (csrc/fusion.hip, aarmvs/fusion.py) away from the benign scene of
``aarmvs.synthetic.fusion_views``: per-view intrinsics, cameras rotated about all three axes with a
z translation, a source camera that has part of the scene behind it, depth and confidence maps that
hold NaN, infinities, zeros of both signs, negative, huge, tiny and denormal values, and frames of
one row, one column and one pixel.

``edge_views`` is ``fusion_views``' ray cast -- the same world surface z = 600 + 0.05 x with bumps,
the same seeded noise, 2 % zero holes and random confidence, drawn in the same order -- with the
camera of every view chosen by ``kind`` (v = 0 .. nsrc, u = v - nsrc / 2):

    plain       fusion_views itself, bit for bit (tests/test_fusion_edge_cases.py asserts it)
    intrinsics  fx = 1.2 W (1 + 0.07 u), fy = 1.03 fx, cx = W / 2 + 3 v, cy = H / 2 - 2 v; poses as plain
    pose        K as plain; R = Rz(0.2 u) Rx(0.04 u) Ry(0.03 u), t = (-30 u, 12 u, 25 u)
    both        the intrinsics of ``intrinsics`` and the poses of ``pose``
    behind      plain, but the last view is R = Ry(1.45), t = 0: the surface is behind it for a part
                of the reference pixels (kz <= 0) and its own ray-cast depth map is negative there

``bad_maps`` scatters BAD_VALUES, ten times each at seeded positions, into every depth map and sets
the first four confidence values to BAD_CONFIDENCE (the threshold is PHOTO_THRESHOLD = 0.35, so they
are NaN, the threshold itself, the next float32 above it, and +inf).

There is no tolerance here: the kernels claim numpy's results bit for bit, so every comparison of
tests/test_gpu_fusion_edge.py is ``np.testing.assert_array_equal`` against oracle/fusion_oracle.py
and the restatements built on it.  tests/test_fusion_edge_cases.py asserts on the CPU what keeps
those comparisons meaningful.  ``inputs`` and ``reference`` are computed once per process and never
modified.  ``python tests/fusion_edge_cases.py`` prints the measured shares (profiles/
fusion_edge_cases.txt).
"""
from __future__ import annotations

import functools
import os
import sys
from typing import NamedTuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "aa-rmvsnet_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import fusion_oracle as fo  # noqa: E402

PHOTO_THRESHOLD = 0.35
KINDS = ("plain", "intrinsics", "pose", "both", "behind")
BEHIND_YAW = 1.45
# (1e-42 is a float32 denormal, 3.4e38 the largest decade below float32's maximum)
BAD_VALUES = (np.nan, np.inf, -np.inf, 0.0, -0.0, -600.0, 1e30, 1e-30, 3.4e38, 1e-42)
BAD_REPEAT = 10
BAD_CONFIDENCE = (np.float32(np.nan), np.float32(PHOTO_THRESHOLD),
                  np.nextafter(np.float32(PHOTO_THRESHOLD), np.float32(1)), np.float32(np.inf))


def _rx(th):
    return np.array([[1, 0, 0], [0, np.cos(th), -np.sin(th)], [0, np.sin(th), np.cos(th)]])


def _ry(th):
    return np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])


def _rz(th):
    return np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])


def cameras(H, W, nsrc, kind):
    """[(K float32 3x3, E float32 4x4)] of views 0 .. nsrc."""
    assert kind in KINDS
    cams = []
    for v in range(nsrc + 1):
        u = v - nsrc / 2
        if kind in ("intrinsics", "both"):
            fx = 1.2 * W * (1 + 0.07 * u)
            K = np.array([[fx, 0, W / 2 + 3 * v], [0, 1.03 * fx, H / 2 - 2 * v], [0, 0, 1]], np.float32)
        else:
            f = np.float32(1.2 * W)
            K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float32)
        if kind in ("pose", "both"):
            R = _rz(0.2 * u) @ _rx(0.04 * u) @ _ry(0.03 * u)
            t = np.array([-30.0 * u, 12.0 * u, 25.0 * u])
        elif kind == "behind" and v == nsrc:
            R, t = _ry(BEHIND_YAW), np.zeros(3)
        else:
            R = _ry(0.03 * u)
            t = np.array([-30.0 * u, 2.0 * v, 0.0])
        E = np.eye(4)
        E[:3, :3] = R
        E[:3, 3] = t
        cams.append((K, E.astype(np.float32)))
    return cams


def edge_views(H, W, nsrc, kind, seed=1):
    """(depths [nsrc + 1] float32 [H,W], cams, confidence float32 [H,W]): ``fusion_views`` with the
    cameras of ``kind``."""
    rng = np.random.default_rng(seed)
    cams = cameras(H, W, nsrc, kind)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    depths = []
    for K_, E_ in cams:
        Ki = np.linalg.inv(K_.astype(np.float64))
        rays = Ki @ np.stack([xs.ravel(), ys.ravel(), np.ones(H * W)])
        # camera -> world: X_w = R^T (X_c - t); surface z_w = 600 + 0.05 x_w (any rotation)
        R = E_[:3, :3].astype(np.float64)
        t = E_[:3, 3].astype(np.float64)
        o = -R.T @ t
        dvec = R.T @ rays
        lam = (600.0 + 0.05 * o[0] - o[2]) / (dvec[2] - 0.05 * dvec[0])
        pw = o[:, None] + dvec * lam
        bump = 4.0 * np.sin(pw[0] / 37.0) * np.cos(pw[1] / 23.0)
        depth = (lam * (1.0 + bump / 600.0)).reshape(H, W)
        noise = rng.normal(0, 0.3, (H, W))
        hole = rng.random((H, W)) < 0.02
        d = (depth + noise).astype(np.float32)
        d[hole] = 0.0
        depths.append(d)
    conf = rng.random((H, W)).astype(np.float32)
    return depths, cams, conf


def bad_maps(depths, conf, seed):
    """Copies with BAD_VALUES scattered into every depth map (BAD_REPEAT times each, at positions of
    their own per map) and BAD_CONFIDENCE at the head of the confidence map."""
    rng = np.random.default_rng(seed + 500)
    vals = np.repeat(np.array(BAD_VALUES, np.float32), BAD_REPEAT)
    out = []
    for d in depths:
        d = d.copy()
        assert d.size >= 2 * vals.size
        d.reshape(-1)[rng.choice(d.size, vals.size, replace=False)] = vals
        out.append(d)
    conf = conf.copy()
    conf.reshape(-1)[:len(BAD_CONFIDENCE)] = BAD_CONFIDENCE
    return out, conf


def holds(depth_map, value):
    """How often ``value`` occurs in a float32 map, by bit pattern (NaN, -0.0 and 0.0 told apart)."""
    bits = np.ascontiguousarray(depth_map, np.float32).view(np.uint32)
    if value != value:
        return int(np.isnan(depth_map).sum())
    return int((bits == np.float32(value).view(np.uint32)).sum())


class Case(NamedTuple):
    name: str
    H: int
    W: int
    nsrc: int
    kind: str
    bad: bool = False
    seed: int = 1


THIN_FRAMES = ((1, 1), (1, 7), (5, 1), (2, 3))
CASES = (
    Case("intrinsics", 40, 52, 4, "intrinsics"),
    Case("pose", 40, 52, 4, "pose"),
    Case("both", 40, 52, 4, "both"),
    Case("both_n10", 40, 52, 10, "both"),
    Case("both_75x101", 75, 101, 4, "both"),       # 7575 pixels: no multiple of 256
    Case("behind", 40, 52, 4, "behind"),
    Case("behind_n10", 40, 52, 10, "behind"),
    Case("bad_intrinsics", 40, 52, 4, "intrinsics", bad=True),
    Case("bad_both", 40, 52, 4, "both", bad=True),
    Case("bad_behind", 40, 52, 4, "behind", bad=True),
) + tuple(Case(f"thin_{h}x{w}_n{n}", h, w, n, "intrinsics") for h, w in THIN_FRAMES for n in (2, 1))
BY_NAME = {c.name: c for c in CASES}
# what tests/test_gpu_fusion_edge.py runs the plain filter on: every case
FILTER_CASES = tuple(c.name for c in CASES)
# the old scene at the same size: the shared-K blindness is measured on it
OLD_SCENE = (40, 52, 4, 1)


@functools.lru_cache(maxsize=None)
def inputs(case: Case):
    """(depths, cams, confidence): view 0 is the reference view."""
    depths, cams, conf = edge_views(case.H, case.W, case.nsrc, case.kind, case.seed)
    if case.bad:
        depths, conf = bad_maps(depths, conf, case.seed)
    for a in depths + [conf]:
        a.setflags(write=False)
    return depths, cams, conf


def oracle_filter(depths, cams, conf, core=fo.filter_depth_core):
    with np.errstate(all="ignore"):
        return core(depths[0], conf, cams[0], depths[1:], cams[1:], PHOTO_THRESHOLD)


@functools.lru_cache(maxsize=None)
def reference(case: Case):
    """The oracle's (photo, geo, final, depth_avg) of the case."""
    out = oracle_filter(*inputs(case))
    for a in out:
        a.setflags(write=False)
    return out


def source_coordinates(case: Case, v: int):
    """(kz float64 [H W], x_src, y_src float32 [H,W]) of the reference pixels in source view v
    (1 .. nsrc): fusion.py:75-87, as the oracle's reproject_with_depth forms them."""
    depths, cams, _ = inputs(case)
    (K_ref, E_ref), (K, E) = cams[0], cams[v]
    H, W = depths[0].shape
    x, y = np.meshgrid(np.arange(0, W), np.arange(0, H))
    x, y = x.reshape([-1]), y.reshape([-1])
    with np.errstate(all="ignore"):
        xyz_ref = np.matmul(np.linalg.inv(K_ref), np.vstack((x, y, np.ones_like(x))) * depths[0].reshape([-1]))
        xyz_src = np.matmul(np.matmul(E, np.linalg.inv(E_ref)), np.vstack((xyz_ref, np.ones_like(x))))[:3]
        kz = np.matmul(K, xyz_src)[2]
        _, _, _, x_src, y_src = fo.reproject_with_depth(depths[0], K_ref, E_ref, depths[v], K, E)
    return kz, x_src, y_src


def outside_fixed_point(coord):
    """Where a float32 source coordinate takes remap_linear's branch for non-finite values and for
    |32 v| >= 2^31 (csrc/fusion.hip to_fixed)."""
    with np.errstate(all="ignore"):
        t = np.asarray(coord, np.float32) * np.float32(32)
        return ~(np.abs(t) < np.float32(2147483520.0))


def swap_source_K(cams):
    """Every source view's K replaced by the reference view's."""
    return [cams[0]] + [(cams[0][0], E) for _, E in cams[1:]]


def swap_reference_K(cams):
    """The reference view's K replaced by source view 1's."""
    return [(cams[1][0], cams[0][1])] + list(cams[1:])


def changed(a, b):
    """Elements that differ, NaN equal to NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == bool:
        return int((a != b).sum())
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())


# ---------------------------------------------------------------------------------
# a scan for the drivers and fuse_views: `both` cameras, bad maps, a confidence map per view
# ---------------------------------------------------------------------------------
SCAN = (40, 52, 3, 5)   # H, W, nsrc, seed


@functools.lru_cache(maxsize=None)
def scan():
    """(pairs, depths, confidences, cams, images), dicts keyed by view id, as fusion_dedup_ref.scene
    gives them: every other view (ascending) is a source view."""
    H, W, nsrc, seed = SCAN
    d, cams, conf = edge_views(H, W, nsrc, "both", seed)
    n = nsrc + 1
    rng = np.random.default_rng(seed + 100)
    depths, confs = {}, {}
    for v in range(n):
        c = conf if v == 0 else rng.random((H, W)).astype(np.float32)
        dv, cv = bad_maps([d[v]], c, seed + 7 * v)
        depths[v], confs[v] = dv[0], cv
    irng = np.random.default_rng(seed + 200)
    images = {v: irng.integers(0, 256, (H, W, 3)).astype(np.float32) / np.float32(255.0) for v in range(n)}
    pairs = [(v, [s for s in range(n) if s != v]) for v in range(n)]
    return pairs, depths, confs, dict(enumerate(cams)), images


# ---------------------------------------------------------------------------------
# the measured shares
# ---------------------------------------------------------------------------------
def shares(case: Case) -> dict:
    depths, cams, conf = inputs(case)
    photo, geo, final, avg = reference(case)
    out = {"geo": float(geo.mean()), "photo": float(photo.mean()), "final": float(final.mean()),
           "avg_nan": int(np.isnan(avg).sum()), "avg_inf": int(np.isinf(avg).sum())}
    with np.errstate(invalid="ignore"):
        out["final_bad_avg"] = int((final & ~(np.isfinite(avg) & (avg >= 0))).sum())
    kz, xs, ys = source_coordinates(case, case.nsrc)
    with np.errstate(invalid="ignore"):
        out["kz_le_0_last"] = float((kz <= 0).mean())
    out["neg_depth_last"] = float((depths[case.nsrc] < 0).mean())
    out["outside_fixed"] = int(sum((outside_fixed_point(c)).sum() for v in range(1, case.nsrc + 1)
                                   for c in source_coordinates(case, v)[1:]))
    swapped = oracle_filter(depths, swap_source_K(cams), conf)
    out["srcK_geo"], out["srcK_avg"] = changed(swapped[1], geo), changed(swapped[3], avg)
    swapped = oracle_filter(depths, swap_reference_K(cams), conf)
    out["refK_geo"], out["refK_avg"] = changed(swapped[1], geo), changed(swapped[3], avg)
    return out


def report() -> str:
    from aarmvs import synthetic as syn
    keys = ("geo", "photo", "final", "avg_nan", "avg_inf", "final_bad_avg", "kz_le_0_last", "neg_depth_last",
            "outside_fixed", "srcK_geo", "srcK_avg", "refK_geo", "refK_avg")
    lines = [
        "Fusion edge cases (tests/fusion_edge_cases.py), oracle/fusion_oracle.py on the CPU, threshold 0.35.",
        "geo / photo / final: share of set pixels; avg_nan / avg_inf: NaN and infinite values of depth_avg;",
        "final_bad_avg: final pixels whose average is negative or not finite; kz_le_0_last: share of the",
        "reference pixels with kz <= 0 in the last source view; neg_depth_last: share of negative values in",
        "that view's depth map; outside_fixed: float32 source coordinates (x and y, all views) that are not",
        "finite or have |32 v| >= 2^31; srcK_*: pixels of geo / values of depth_avg that change when every",
        "source K is replaced by the reference K; refK_*: when the reference K is replaced by source 1's.",
        "",
        "case".ljust(18) + "pixels nsrc " + " ".join(k.rjust(14) for k in keys),
    ]

    def row(name, px, nsrc, s):
        cells = [(f"{s[k]:.4f}" if isinstance(s[k], float) else str(s[k])).rjust(14) for k in keys]
        return name.ljust(18) + f"{px:6d} {nsrc:4d} " + " ".join(cells)

    for case in CASES:
        lines.append(row(case.name, case.H * case.W, case.nsrc, shares(case)))
    # the old scene: one shared K, so neither replacement changes anything
    H, W, nsrc, seed = OLD_SCENE
    depths, cams, conf = syn.fusion_views(H, W, nsrc, seed=seed)
    ref = oracle_filter(depths, cams, conf)
    a, b = oracle_filter(depths, swap_source_K(cams), conf), oracle_filter(depths, swap_reference_K(cams), conf)
    lines += ["", f"synthetic.fusion_views({H}, {W}, {nsrc}, seed={seed}): geo {ref[1].mean():.4f}; source K <- reference K "
              f"changes {changed(a[1], ref[1])} geo pixels and {changed(a[3], ref[3])} averages; reference K <- source K "
              f"changes {changed(b[1], ref[1])} and {changed(b[3], ref[3])}."]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    sys.stdout.write(report())
