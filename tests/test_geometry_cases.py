"""Each camera case of tests/geometry_cases.py reaches its regime of the cost-slice backward's
source-box logic at the shapes tests/test_gpu_geometry.py runs, so that a case cannot silently
stop testing anything.  Conditions on the inputs only (numpy, no GPU, no library).

Figures (``reach``): per 16x16 tile and 16-plane group the tiles with a corner behind the
source camera, with an empty source box and with a box over 768 px; the share of pixels whose
top-left tap is shared by more than 2 pixels of their tile (a box cell overflows); the share of
taps outside the image.
"""
import numpy as np
import pytest
import torch

from aarmvs import synthetic as syn
from oracle import sweep_oracle as orc

import geometry_cases as gc


def _reach(kind, H, W, D, B=1, N=3, v=1, depths=None):
    sc = syn.scene(B, N, H, W, D, seed=0)
    proj = gc.apply(torch.from_numpy(sc["proj_matrices"]), [(0, v, kind)], H, W)
    rel = orc.relative_projection(proj[:, v], proj[:, 0])[0]
    return gc.reach(rel, sc["depth_values"][0] if depths is None else depths, H, W)


def test_case_matrices_are_pixel_space_homographies():
    H, W = 36, 52
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0, 1.0])
    for kind in gc.KINDS:
        M = gc.case(kind, H, W)
        assert M.dtype == torch.float32 and tuple(M.shape) == (4, 4)
        assert torch.equal(M[3], torch.tensor([0.0, 0.0, 0.0, 1.0])) and torch.equal(M[:3, 3], torch.zeros(3))
    for kind in ("minify", "magnify", "rotate"):   # the image centre stays put
        np.testing.assert_allclose(gc.case(kind, H, W)[:3, :3].double().numpy() @ c, c, atol=1e-5)
    p = gc.case("minify", H, W)[:3, :3].double().numpy() @ np.array([0.0, 0.0, 1.0])
    np.testing.assert_allclose(p[:2], c[:2] / 2, atol=1e-5)
    p = gc.case("rotate", H, W)[:3, :3].double().numpy() @ (c + np.array([10.0, 0.0, 0.0]))
    np.testing.assert_allclose(p[:2], c[:2] + 10.0 * np.array([np.cos(np.pi / 6), np.sin(np.pi / 6)]), atol=1e-4)
    assert float(gc.case("behind", H, W)[2, 0]) == pytest.approx(-1.0 / (W / 2))
    np.testing.assert_allclose(gc.case("shift", H, W)[:2, 2].numpy(), [0.75 * W, -0.4 * H], rtol=1e-6)


@pytest.mark.parametrize("H,W,D", [(36, 52, 18), (36, 52, 5), (44, 60, 5), (24, 40, 18)])
def test_plain_scene_reaches_only_the_in_box_gather(H, W, D):
    """The gap this module's cases close: on aarmvs.synthetic.scene's rig no tile has a corner
    behind the camera, an empty or an oversized box, and no box cell overflows."""
    for v in (1, 2):
        r = _reach(None, H, W, D, v=v)
        assert (r["behind"], r["empty"], r["oversize"], r["overflow"], r["z_nonpos"]) == (0, 0, 0, 0.0, 0.0), r


@pytest.mark.parametrize("D", [18, 5])
def test_minify_overflows_the_box_cells(D):
    r = _reach("minify", 36, 52, D)
    assert r["overflow"] >= 0.5 and r["outside"] == 0.0, r
    assert (r["behind"], r["empty"], r["oversize"]) == (0, 0, 0), r


def test_magnify_has_oversized_boxes_in_front_of_the_camera():
    r = _reach("magnify", 44, 60, 5)
    assert r["oversize"] >= 2 and r["behind"] == 0 and r["z_nonpos"] == 0.0, r


@pytest.mark.parametrize("D", [18, 5])
def test_rotate_puts_taps_outside_the_image(D):
    r = _reach("rotate", 36, 52, D)
    assert 0.1 <= r["outside"] <= 0.5 and r["behind"] == 0, r


@pytest.mark.parametrize("D", [18, 5])
def test_behind_puts_tile_corners_behind_the_camera(D):
    r = _reach("behind", 36, 52, D)
    assert 0.1 < r["z_nonpos"] < 0.9, r
    assert 2 * r["behind"] >= r["tiles"], r


@pytest.mark.parametrize("D", [18, 5])
def test_shift_empties_the_boxes(D):
    r = _reach("shift", 36, 52, D)
    assert 2 * r["empty"] >= r["tiles"] and r["behind"] == 0, r


def test_mixed_batch_views_keep_their_regimes():
    """The B = 2 case (24x40, D = 18: a 16-plane group and a ragged 2-plane one; element 1 on
    its own descending depths): minify, behind and shift reach their fallbacks there too, rotate
    and magnify put taps outside the image, and the plain view stays in the box."""
    H, W, D = 24, 40, 18
    d1 = np.linspace(1200.0, 600.0, D).astype(np.float32)
    r = _reach("minify", H, W, D, N=4, v=1)
    assert r["tiles"] == 12 and r["overflow"] >= 0.5, r
    r = _reach("rotate", H, W, D, N=4, v=2)
    assert 0.1 <= r["outside"] <= 0.5, r
    r = _reach(None, H, W, D, N=4, v=3)
    assert (r["behind"], r["empty"], r["oversize"], r["overflow"]) == (0, 0, 0, 0.0), r
    r = _reach("behind", H, W, D, N=4, v=1, depths=d1)
    assert 0.1 < r["z_nonpos"] < 0.9 and 2 * r["behind"] >= r["tiles"], r
    r = _reach("magnify", H, W, D, N=4, v=2, depths=d1)
    assert r["outside"] >= 0.5 and r["behind"] == 0, r
    r = _reach("shift", H, W, D, N=4, v=3, depths=d1)
    assert 2 * r["empty"] >= r["tiles"], r
