"""tools/omega_pair_paths.py (CPU): the source boxes and the plane-pair walk it restates from
omega_mfma_kernel, on small cameras where both can be counted by hand."""
import importlib.util
import os

import numpy as np

from conftest import ROOT
from aarmvs import synthetic as syn


def _tool():
    spec = importlib.util.spec_from_file_location(
        "omega_pair_paths", os.path.join(ROOT, "tools", "omega_pair_paths.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


opp = _tool()


def shift_rel(dx, dy):
    """A relative projection that moves every pixel by (dx, dy) at every depth."""
    return np.array([[1, 0, dx, 0], [0, 1, dy, 0], [0, 0, 1, 0]], np.float32)


def scene_rel(N, H, W):
    proj = syn.camera_projections(N, H, W, baseline=20.0 * 1600.0 / W)
    return opp.tc.relative(proj[0], proj[1:])


def test_tile_boxes_match_a_per_tile_restatement():
    """tile_boxes' sliding windows against box_extend written out per tile and pixel."""
    H, W = 40, 52
    rel = scene_rel(3, H, W)
    for m in rel:
        for depth in (425.0, 700.0):
            got = opp.tile_boxes(m, depth, H, W)
            xf, yf = opp.tc.tap_floor(m, depth, np.arange(H), H, W)
            ty_n, tx_n = opp.tiles(H, W)
            assert got.shape == (ty_n, tx_n, 4)
            for ty in range(ty_n):
                for tx in range(tx_n):
                    lo = [1 << 30, 1 << 30]
                    hi = [-(1 << 30), -(1 << 30)]
                    for y in range(max(0, 14 * ty - 1), min(H, 14 * ty + 15)):
                        for x in range(max(0, 14 * tx - 1), min(W, 14 * tx + 15)):
                            a, b = xf[y, x], yf[y, x]
                            if np.isnan(a) or np.isnan(b):
                                continue
                            xl, xh = max(a, 0), min(a + 1, W - 1)
                            yl, yh = max(b, 0), min(b + 1, H - 1)
                            if xl <= xh and yl <= yh:
                                lo = [min(lo[0], int(xl)), min(lo[1], int(yl))]
                                hi = [max(hi[0], int(xh)), max(hi[1], int(yh))]
                    assert list(got[ty, tx]) == lo + hi, (ty, tx)


def test_a_pure_shift_has_boxes_of_the_tile_plus_one_tap():
    H, W = 56, 56
    b = opp.tile_boxes(shift_rel(0.5, 0.5), 500.0, H, W)
    # tile (1, 1): haloed pixels 13 .. 28, taps floor(p + 0.5 ...) .. + 1: 17 x 17 pixels
    px = opp.box_px(b)
    assert px[1, 1] == 17 * 17, b[1, 1]
    # a shift of four image widths leaves no tap in the image
    assert (opp.box_px(opp.tile_boxes(shift_rel(4.0 * W, 0), 500.0, H, W)) == 0).all()


def test_union_and_box_px():
    a = np.array([[2, 3, 5, 6]])
    b = np.array([[4, 1, 9, 4]])
    u = opp.box_union(a, b)
    assert list(u[0]) == [2, 1, 9, 6]
    assert list(opp.box_px(np.concatenate([a, b, u]))) == [16, 24, 48]
    empty = np.array([[1 << 30, 1 << 30, -(1 << 30), -(1 << 30)]])
    assert opp.box_px(empty)[0] == 0
    assert list(opp.box_union(a, empty)[0]) == list(a[0])


def test_plane_groups():
    assert opp.plane_groups(0, 37) == [(0, 16), (16, 16), (32, 5)]
    assert opp.plane_groups(3, 16) == [(3, 13)]


def test_every_plane_is_counted_once_and_pairs_follow_the_blocks():
    H, W, N, D = 64, 96, 3, 6
    rel = scene_rel(N, H, W)
    dv = syn.depth_hypotheses(512)[:D]
    ty_n, tx_n = opp.tiles(H, W)
    tv = ty_n * tx_n * (N - 1)
    for cap in (None, 300, 4):
        for ipb in (1, 2, 3, 8):
            for groups in (None, [(0, 3), (3, 3)], [(1, 5)]):
                p = opp.omega_paths(rel, dv, H, W, cap, ipb, groups)
                planes = sum(n for _, n in (groups or [(0, D)]))
                assert 2 * p["pair_lds"] + p["single_lds"] + p["single_global"] == tv * planes
                if ipb == 1:
                    assert p["pair_lds"] == p["pair_split"] == 0
    # whole pairs in every block, everything fits: three pairs per (tile, view)
    assert opp.omega_paths(rel, dv, H, W, None, 2) == {
        "pair_lds": 3 * tv, "pair_split": 0, "single_lds": 0, "single_global": 0}
    # three items per block, six planes per (tile, view): a pair and a single per block
    assert opp.omega_paths(rel, dv, H, W, None, 3) == {
        "pair_lds": 2 * tv, "pair_split": 0, "single_lds": 2 * tv, "single_global": 0}
    # odd launches of 3 planes: wherever a block of 8 items ends, two of a (tile, view)'s three
    # planes are neighbours in one block, so each has one pair and one single
    assert opp.omega_paths(rel, dv, H, W, None, 8, [(0, 3), (3, 3)]) == {
        "pair_lds": 2 * tv, "pair_split": 0, "single_lds": 2 * tv, "single_global": 0}
    # blocks of 4 items over 6 planes per (tile, view): a (tile, view) starts at an even item of
    # a block, so its pairs (0,1) (2,3) (4,5) never straddle two blocks
    assert opp.omega_paths(rel, dv, H, W, None, 4)["pair_lds"] == 3 * tv
    # blocks of 3 items over launches of 5 planes: the blocks drift across (tile, view)s
    p = opp.omega_paths(rel, dv, H, W, None, 3, [(0, 5)])
    assert p["pair_lds"] < 2 * tv and 2 * p["pair_lds"] + p["single_lds"] == 5 * tv


def test_capacity_splits_pairs_and_sends_large_boxes_to_the_global_path():
    H, W = 56, 56
    rel = np.stack([shift_rel(0.5, 0.5)])
    dv = [500.0, 600.0]
    # interior tiles: 17 x 17 = 289 px single and union (the shift does not depend on depth)
    full = opp.omega_paths(rel, dv, H, W, None, 2)
    assert full == {"pair_lds": 16, "pair_split": 0, "single_lds": 0, "single_global": 0}
    p = opp.omega_paths(rel, dv, H, W, 288, 2)
    px = opp.box_px(opp.tile_boxes(rel[0], 500.0, H, W))
    big = int((px > 288).sum())
    assert 0 < big < 16
    assert p == {"pair_lds": 16 - big, "pair_split": big, "single_lds": 0, "single_global": 2 * big}
    # two planes whose boxes lie apart: the union exceeds a capacity both planes fit
    # (x + 0.5 + 1020 / depth, y + 0.5): shifts of 10.7 and 1.52 pixels, boxes 9 columns apart
    rel2 = np.stack([np.array([[1, 0, 0.5, 1020], [0, 1, 0.5, 0], [0, 0, 1, 0]], np.float32)])
    d2 = [100.0, 1000.0]
    a = opp.tile_boxes(rel2[0], d2[0], H, W)
    b = opp.tile_boxes(rel2[0], d2[1], H, W)
    assert opp.box_px(a)[1, 1] == 289 and opp.box_px(b)[1, 1] == 289
    u = opp.box_px(opp.box_union(a, b))
    assert u[1, 1] == 26 * 17
    cap = int(max(opp.box_px(a).max(), opp.box_px(b).max()))   # every single box fits
    assert u[1, 1] > cap
    q = opp.omega_paths(rel2, d2, H, W, cap, 2)
    assert q["pair_split"] == int((u > cap).sum()) > 0 and q["single_global"] == 0
    assert q["single_lds"] == 2 * q["pair_split"] and q["pair_lds"] == 16 - q["pair_split"]
