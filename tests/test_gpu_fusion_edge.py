"""Depth-map fusion on the GPU at the cases of tests/fusion_edge_cases.py: per-view intrinsics, cameras
rotated about all three axes, a source camera with part of the scene behind it, depth and confidence
maps with NaN, infinities, signed zeros, negative, huge and denormal values, and frames of one row,
one column and one pixel -- the filter (plain and de-duplicating), the point extraction (plain and
with normals), both file drivers and ``fuse_views``, and the argument checks of the entry points.

Every comparison is ``np.testing.assert_array_equal`` (NaN equal to NaN) against
oracle/fusion_oracle.py and the numpy restatements built on it: the kernels claim numpy's float64
results in numpy's order, so there is no tolerance.  tests/test_fusion_edge_cases.py asserts on the
CPU that the cases hold what they are named for and can tell a K taken from the wrong view.

The one-pixel frame and the single kept point send numpy through another BLAS routine (a matrix-
vector product) than every larger frame; its float64 last bit may differ, which the
float32 casts of the reprojected depth and of the points hide at these values.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "aa-rmvsnet_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fusion_dedup_ref as dr  # noqa: E402
import fusion_edge_cases as ec  # noqa: E402
import fusion_normals_ref as nr  # noqa: E402
import fusion_tnt_ref as tr  # noqa: E402
from oracle import fusion_oracle as fo  # noqa: E402
from test_gpu_fusion_dedup import _cam_text, _check_driver  # noqa: E402
from aarmvs import fusion  # noqa: E402
from aarmvs._lib import AarmvsError  # noqa: E402

pytestmark = pytest.mark.gpu

THR = ec.PHOTO_THRESHOLD
THIN = [c.name for c in ec.CASES if c.name.startswith("thin")]
_WANT = {}


def _once(key, make):
    """A restatement's answer: computed once, shared, never modified."""
    if key not in _WANT:
        with np.errstate(all="ignore"):
            _WANT[key] = make()
    return _WANT[key]


def _t(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _cuda(d):
    return {k: _t(v) for k, v in d.items()}


def _gpu_filter(case):
    depths, cams, conf = ec.inputs(case)
    t = [_t(d) for d in depths]
    return fusion.filter_depth_core(t[0], _t(conf), cams[0], t[1:], cams[1:], THR)


def _image(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3)).astype(np.float32) / np.float32(255.0)


# ---------------------------------------------------------------------------------
# 1. the plain filter
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.FILTER_CASES)
def test_filter_matches_oracle(name):
    case = ec.BY_NAME[name]
    want = ec.reference(case)
    got = [g.cpu().numpy() for g in _gpu_filter(case)]
    assert got[3].dtype == np.float64 and got[3].shape == (case.H, case.W)
    for k, g, w in zip(("photo", "geo", "final", "depth_avg"), got, want):
        print(f"{name} {k}: {ec.changed(g, w)} of {w.size} differ")
    for k, g, w in zip(("photo", "geo", "final", "depth_avg"), got, want):
        np.testing.assert_array_equal(g, w, err_msg=f"{name} {k}")


def test_filter_with_the_tnt_vote_rule_on_ten_views():
    """fusion_padding.py's fixed vote rule (tests/fusion_tnt_ref.py) on ``both`` with 10 source views."""
    case = ec.BY_NAME["both_n10"]
    want = _once("tnt_core", lambda: ec.oracle_filter(*ec.inputs(case), core=tr.filter_depth_core))
    for k, g, w in zip(("photo", "geo", "final", "depth_avg"), _gpu_filter(case), want):
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=k)


# ---------------------------------------------------------------------------------
# 2. the de-duplicating instantiation
# ---------------------------------------------------------------------------------
def _dedup_want(name, given):
    case = ec.BY_NAME[name]
    depths, cams, conf = ec.inputs(case)
    used_ref = (np.random.default_rng(4).random((case.H, case.W)) < 0.5).astype(np.uint8) if given else None
    marks = [np.zeros((case.H, case.W), np.uint8) for _ in range(case.nsrc)]
    out = dr.filter_depth_dedup(depths[0], conf, cams[0], depths[1:], cams[1:], THR, used_ref, marks)
    return used_ref, marks, out


@pytest.mark.parametrize("given", [True, False], ids=["used_ref", "no_used_ref"])
@pytest.mark.parametrize("name", ["both", "behind", "bad_both", "bad_behind"])
def test_dedup_matches_restatement_inside_guard_bytes(name, given):
    """The four plain outputs, ``emit`` and every source view's used map; the used and emit maps are
    carved out of one buffer filled with 0xAB, and nothing outside them is written: a mark computed
    from a NaN or infinite coordinate lands nowhere."""
    import torch
    case = ec.BY_NAME[name]
    depths, cams, conf = ec.inputs(case)
    used_ref, marks, want = _once(("dedup", name, given), lambda: _dedup_want(name, given))
    assert sum(int(m.sum()) for m in marks) > 100 and (not given or 0 < want[3].sum() < want[2].sum())
    for g, w in zip((want[0], want[1], want[2], want[4]), ec.reference(case)):
        np.testing.assert_array_equal(g, w)          # the restatement's four are the oracle's
    H, W, n = case.H, case.W, case.nsrc + 1          # nsrc used maps and the emit map
    HW, G = H * W, 67                                # 2080-byte maps at odd offsets
    buf = torch.full((n * (HW + G) + G,), 0xAB, dtype=torch.uint8, device="cuda")
    slot = lambda i: buf[G + i * (HW + G):G + i * (HW + G) + HW].view(H, W)  # noqa: E731
    used = [slot(i) for i in range(case.nsrc)]
    for u in used:
        u.zero_()
    t = [_t(d) for d in depths]
    got = fusion.filter_depth_dedup(t[0], _t(conf), cams[0], t[1:], cams[1:], THR,
                                    None if used_ref is None else _t(used_ref), used, emit_out=slot(case.nsrc))
    for k, g, w in zip(("photo", "geo", "final", "emit", "depth_avg"), got, want):
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=f"{name} {k}")
    if not given:
        np.testing.assert_array_equal(got[3].cpu().numpy(), want[2])     # emit = final
    host = buf.cpu().numpy()
    inside = np.zeros(host.shape, bool)
    for i in range(n):
        inside[G + i * (HW + G):G + i * (HW + G) + HW] = True
    assert (host[~inside] == 0xAB).all() and (~inside).sum() == (n + 1) * G
    assert set(np.unique(host[inside])) <= {0, 1}
    for v, (u, w) in enumerate(zip(used, marks)):
        np.testing.assert_array_equal(u.cpu().numpy(), w, err_msg=f"{name}: used map of source view {v}")
    np.testing.assert_array_equal(slot(case.nsrc).cpu().numpy(), want[3].astype(np.uint8))


# ---------------------------------------------------------------------------------
# 3. the points
# ---------------------------------------------------------------------------------
def _check_points(avg, keep, cam, img, least):
    """fuse_points_gpu of numpy inputs against the host fuse_points and fusion_padding.py's."""
    with np.errstate(all="ignore"):
        xyz_w, rgb_w = fusion.fuse_points(avg, keep, cam, img)
        xyz_t, rgb_t = tr.fuse_points(avg, keep, cam, img)
        xyz_t = xyz_t.astype(np.float32)
    n = int(keep.sum())
    assert xyz_w.shape == xyz_t.shape == (n, 3) and xyz_w.dtype == np.float32 and n >= least
    np.testing.assert_array_equal(xyz_w, xyz_t)
    np.testing.assert_array_equal(rgb_w, rgb_t)
    xyz, rgb = fusion.fuse_points_gpu(_t(avg), _t(keep), cam, _t(img))
    assert tuple(xyz.shape) == tuple(rgb.shape) == (n, 3)              # the count
    np.testing.assert_array_equal(xyz.cpu().numpy(), xyz_w)
    np.testing.assert_array_equal(rgb.cpu().numpy(), rgb_w)
    xyz2, none = fusion.fuse_points_gpu(_t(avg), _t(keep), cam)
    assert none is None
    np.testing.assert_array_equal(xyz2.cpu().numpy(), xyz_w)
    return xyz_w


@pytest.mark.parametrize("name", ["pose", "both", "both_75x101"])
def test_points_after_the_filter(name):
    """inv(E) with a full rotation, on the filter's own averaged depth and final mask."""
    case = ec.BY_NAME[name]
    _, cams, _ = ec.inputs(case)
    _, _, final, avg = _gpu_filter(case)
    final, avg = final.cpu().numpy(), avg.cpu().numpy()
    np.testing.assert_array_equal(final, ec.reference(case)[2])
    np.testing.assert_array_equal(avg, ec.reference(case)[3])
    _check_points(avg, final, cams[0], _image(case.H, case.W, 1), least=100)


def _bad_average():
    """bad_both's averaged depth with 1e300 and -1e300 planted, and a mask that keeps every value that
    is NaN, +-inf, negative or huge beside a tenth of the others."""
    case = ec.BY_NAME["bad_both"]
    avg = np.array(ec.reference(case)[3])
    rng = np.random.default_rng(8)
    spots = rng.choice(avg.size, 12, replace=False)
    avg.reshape(-1)[spots[:6]] = 1e300
    avg.reshape(-1)[spots[6:]] = -1e300
    with np.errstate(invalid="ignore"):
        odd = ~np.isfinite(avg) | (avg < 0) | (avg >= 1e300)
    return case, avg, odd | (rng.random(avg.shape) < 0.1), odd


def test_points_of_nan_infinite_negative_and_huge_averages():
    case, avg, keep, odd = _bad_average()
    assert np.isnan(avg[keep]).sum() >= 5 and np.isposinf(avg[keep]).sum() >= 5 and np.isneginf(avg[keep]).sum() >= 5
    assert (avg[keep] == 1e300).sum() == 6 and (avg[keep] == -1e300).sum() == 6 and (avg[keep] == -600).sum() >= 5
    assert odd.sum() >= 40 and (keep & ~odd).sum() >= 100
    xyz = _check_points(avg, keep, ec.inputs(case)[1][0], _image(case.H, case.W, 2), least=140)
    # the float32 cast of xyz overflows there, and 0 * inf is NaN
    assert np.isnan(xyz).any() and np.isposinf(xyz).any() and np.isneginf(xyz).any()
    assert np.isfinite(xyz[(avg[keep] >= 0) & (avg[keep] < 1e6)]).all()


@pytest.mark.parametrize("name", [n for n in THIN if n.endswith("_n2")])
def test_points_on_thin_frames(name):
    """One row, one column, one pixel: all kept (one point on 1 x 1), all dropped, and every other
    pixel."""
    import torch
    case = ec.BY_NAME[name]
    depths, cams, _ = ec.inputs(case)
    avg = depths[0].astype(np.float64)
    img = _image(case.H, case.W, 3)
    _check_points(avg, np.ones(avg.shape, bool), cams[0], img, least=1)
    _check_points(avg, np.zeros(avg.shape, bool), cams[0], img, least=0)
    if avg.size > 1:
        _check_points(avg, (np.arange(avg.size) % 2 == 1).reshape(avg.shape), cams[0], img, least=1)
    # and straight from the filter on that frame
    _, _, final, gavg = _gpu_filter(case)
    xyz, rgb = fusion.fuse_points_gpu(gavg, torch.ones_like(final), cams[0], _t(img))
    np.testing.assert_array_equal(xyz.cpu().numpy(), fusion.fuse_points(avg, np.ones(avg.shape, bool), cams[0])[0])


# ---------------------------------------------------------------------------------
# 4. the points with normals
# ---------------------------------------------------------------------------------
def test_points_with_normals_on_the_bad_averages():
    case, avg, keep, odd = _bad_average()
    cam = ec.inputs(case)[1][0]
    keep = keep | ec.reference(case)[2]
    want_n, want_h = _once("normals", lambda: nr.estimate_normals(avg, keep, cam))
    assert 100 <= want_h.sum() < keep.sum() and not want_h[odd].any()
    nmap, has = fusion.estimate_normals(_t(avg), _t(keep), cam)
    np.testing.assert_array_equal(has.cpu().numpy(), want_h)
    np.testing.assert_array_equal(nmap.cpu().numpy().view(np.uint32), want_n.view(np.uint32))
    img = _image(case.H, case.W, 4)
    with np.errstate(all="ignore"):
        xyz_w, rgb_w = dr.fuse_points(avg, keep, cam, img)
    xyz, rgb, nrm = fusion.fuse_points_normals_gpu(_t(avg), _t(keep), cam, _t(img), nmap)
    np.testing.assert_array_equal(xyz.cpu().numpy(), xyz_w)
    np.testing.assert_array_equal(rgb.cpu().numpy(), rgb_w)
    np.testing.assert_array_equal(nrm.cpu().numpy().view(np.uint32), want_n[keep].view(np.uint32))


# ---------------------------------------------------------------------------------
# 5. the drivers and fuse_views: ec.scan() (`both` cameras, bad maps), 4 views of 40 x 52
# ---------------------------------------------------------------------------------
def _write_scan(root, tnt):
    """ec.scan() as files.  DTU layout: images with 4 more rows above and below than the maps (the
    driver's crop; cy moves with them).  Tanks and Temples: intrinsics of the full-size image (2 K),
    images twice the maps' size, PFMs with 2 junk rows above and below."""
    from PIL import Image
    pairs, depths, confs, cams, _ = ec.scan()
    H, W, _, _ = ec.SCAN
    pad = 4
    scan, out = root / "scan1", root / "out" / "scan1"
    for d in ("cams", "images"):
        (scan / d).mkdir(parents=True, exist_ok=True)
    for d in ("depth_est_0", "confidence_0"):
        (out / d).mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(3)

    def stored(m):
        if not tnt:
            return m
        junk = rng.uniform(-1e6, 1e6, (H + 4, W)).astype(np.float32)
        junk[2:-2] = m
        return junk

    images, cam_texts, dmaps, cmaps = {}, {}, {}, {}
    for v in sorted(depths):
        K, E = cams[v]
        K = K.copy()
        if tnt:
            K[:2] *= 2
        else:
            K[1, 2] += pad
        cam_texts[v] = _cam_text(K, E)
        (scan / "cams" / "{:0>8}_cam.txt".format(v)).write_text(cam_texts[v])
        img = (rng.random((2 * H, 2 * W, 3) if tnt else (H + 2 * pad, W, 3)) * 255).astype(np.uint8)
        Image.fromarray(img).save(str(scan / "images" / "{:0>8}.jpg".format(v)), format="PNG")
        images[v] = np.array(Image.open(str(scan / "images" / "{:0>8}.jpg".format(v))), np.float32) / 255.0
        dmaps[v], cmaps[v] = stored(depths[v]), stored(confs[v])
        fusion.save_pfm(str(out / "depth_est_0" / "{:0>8}.pfm".format(v)), dmaps[v])
        fusion.save_pfm(str(out / "confidence_0" / "{:0>8}.pfm".format(v)), cmaps[v])
    with open(scan / "pair.txt", "w") as f:
        f.write(f"{len(pairs)}\n")
        for v, srcs in pairs:
            f.write(f"{v}\n{len(srcs)} " + " ".join(f"{s} {9.0 - s:.1f}" for s in srcs) + "\n")
    return scan, out, (pairs, images, cam_texts, dmaps, cmaps)


def _as_dict(scan_want):
    masks, xyz, rgb = scan_want
    return dict(xyz=xyz, rgb=rgb, masks={v: dict(photo=p, geo=g, final=f) for v, (p, g, f) in masks.items()})


def test_dtu_driver_on_per_view_cameras_and_bad_maps(tmp_path):
    scan, out, inputs = _write_scan(tmp_path, tnt=False)
    texts = inputs[2]
    for a in range(len(texts)):                      # the cam files differ in every intrinsic entry
        for b in range(a):
            ka, kb = (t.split("intrinsic\n")[1].split() for t in (texts[a], texts[b]))
            assert all(ka[i] != kb[i] for i in (0, 2, 4, 5))
    want = _once("dtu_scan", lambda: _as_dict(fo.filter_depth_scan(*inputs, THR)))
    assert sorted(want["masks"]) == [0, 1, 2, 3]
    ply = tmp_path / "scan1.ply"
    npts = fusion.filter_depth(str(scan), str(out), str(ply), THR)
    _check_driver(out, ply, npts, want, plain=True)


def test_tnt_driver_on_per_view_cameras_and_bad_maps(tmp_path):
    scan, out, inputs = _write_scan(tmp_path, tnt=True)
    want = _once("tnt_scan", lambda: _as_dict(tr.filter_depth_scan(*inputs, THR)))
    assert sorted(want["masks"]) == [0, 1, 2, 3]
    ply = tmp_path / "scan1.ply"
    npts = fusion.filter_depth_tnt(str(scan), str(out), str(ply), THR)
    _check_driver(out, ply, npts, want, plain=True)


@pytest.mark.parametrize("dedup", [False, True], ids=["plain", "dedup"])
def test_fuse_views_on_per_view_cameras_and_bad_maps(dedup):
    sc = ec.scan()
    pairs, depths, confs, cams, images = sc
    want = _once(("fuse_views", dedup), lambda: dr.fuse_views(*sc, THR, dedup=dedup))
    got = fusion.fuse_views(pairs, _cuda(depths), _cuda(confs), cams, _cuda(images), THR, dedup=dedup)
    assert sorted(got["masks"]) == sorted(want["masks"]) and got["counts"] == want["counts"]
    for v, m in want["masks"].items():
        assert sorted(got["masks"][v]) == sorted(m)
        for k in m:
            np.testing.assert_array_equal(got["masks"][v][k].cpu().numpy(), m[k], err_msg=f"view {v} {k}")
        np.testing.assert_array_equal(got["avg"][v].cpu().numpy(), want["avg"][v], err_msg=f"view {v} avg")
    if dedup:
        assert sorted(got["used"]) == sorted(want["used"])
        for v, u in want["used"].items():
            np.testing.assert_array_equal(got["used"][v].cpu().numpy(), u, err_msg=f"used map of view {v}")
    else:
        assert "used" not in got
    assert want["xyz"].shape[0] >= 100
    np.testing.assert_array_equal(got["xyz"].cpu().numpy(), want["xyz"])
    np.testing.assert_array_equal(got["rgb"].cpu().numpy(), want["rgb"])


# ---------------------------------------------------------------------------------
# 6. the argument checks (every call is rejected before anything is launched)
# ---------------------------------------------------------------------------------
def _filter_args(H, W, nsrc):
    """aarmvs_fusion_args of the given shape over 4 x 4 buffers (kept alive by the caller)."""
    import torch
    from aarmvs import _lib
    f32 = torch.ones(4, 4, dtype=torch.float32, device="cuda")
    u8 = [torch.zeros(4, 4, dtype=torch.uint8, device="cuda") for _ in range(3)]
    avg = torch.zeros(4, 4, dtype=torch.float64, device="cuda")
    cams = np.zeros(_lib.fusion_cam_floats(_lib.MAX_FUSION_SRC), np.float32)
    a = _lib.FusionArgs()
    a.H, a.W, a.nsrc = H, W, nsrc
    a.ref_depth = a.confidence = f32.data_ptr()
    for i in range(_lib.MAX_FUSION_SRC):
        a.src_depth[i] = f32.data_ptr()
    a.cams = cams.ctypes.data
    a.photo_threshold = 0.35
    a.photo_mask, a.geo_mask, a.final_mask = (m.data_ptr() for m in u8)
    a.depth_avg = avg.data_ptr()
    return a, (f32, u8, avg, cams)


@pytest.mark.parametrize("H,W,nsrc", [(0, 4, 2), (4, 0, 2), (0, 0, 2), (-1, 4, 2), (4, 4, 0), (4, 4, 11), (4, 4, -1)])
def test_filter_entry_points_reject_bad_shapes(H, W, nsrc):
    import torch
    from aarmvs import _lib, lib
    a, keep = _filter_args(H, W, nsrc)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib().aarmvs_fusion_filter(ctypes.byref(a), stream) != 0
    assert b"fusion_filter: need H, W >= 1 and 1 <= nsrc <= 10" in lib().aarmvs_last_error()
    d = _lib.FusionDedupArgs()
    emit = torch.full((4, 4), 0xAB, dtype=torch.uint8, device="cuda")
    d.emit_mask = emit.data_ptr()
    assert lib().aarmvs_fusion_filter_dedup(ctypes.byref(a), ctypes.byref(d), stream) != 0
    torch.cuda.synchronize()
    f32, u8, avg, _ = keep
    assert bool((emit == 0xAB).all()) and not any(bool(m.any()) for m in u8) and not bool(avg.any())
    # the same shapes through Python
    if H >= 0 and W >= 0 and nsrc >= 0:
        maps = torch.ones(H, W, dtype=torch.float32, device="cuda")
        cam = ec.cameras(4, 4, 1, "both")[0]
        with pytest.raises(AarmvsError):
            fusion.filter_depth_core(maps, maps, cam, [maps] * nsrc, [cam] * nsrc, THR)
        with pytest.raises(AarmvsError):
            fusion.filter_depth_dedup(maps, maps, cam, [maps] * nsrc, [cam] * nsrc, THR, None, [None] * nsrc)


@pytest.mark.parametrize("H,W", [(65536, 32768), (32768, 65536), (1 << 30, 2), (46341, 46341), (0, 4), (4, 0)])
def test_points_entry_points_reject_bad_shapes(H, W):
    """H W >= 2^31 (and H or W below 1) is rejected on the shape arguments alone: the buffers are tiny."""
    import torch
    from aarmvs import _lib, lib
    assert H < 1 or W < 1 or H * W >= 2 ** 31
    assert lib().aarmvs_fusion_points_workspace_bytes(H, W) == 0
    mask = torch.ones(4, 4, dtype=torch.uint8, device="cuda")
    depth = torch.ones(4, 4, dtype=torch.float64, device="cuda")
    xyz = torch.full((16, 3), -7.5, dtype=torch.float32, device="cuda")
    count = torch.full((1,), -3, dtype=torch.int64, device="cuda")
    work = torch.zeros(256, dtype=torch.uint8, device="cuda")
    cams = fusion.pack_point_cameras(ec.cameras(4, 4, 1, "both")[0])
    a = _lib.FusionPointsArgs()
    a.H, a.W = H, W
    a.mask, a.depth, a.color, a.cams = mask.data_ptr(), depth.data_ptr(), None, cams.ctypes.data
    a.xyz, a.rgb, a.capacity = xyz.data_ptr(), None, 16
    a.count, a.workspace = count.data_ptr(), work.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    assert lib().aarmvs_fusion_points(ctypes.byref(a), stream) != 0
    assert b"fusion_points: need H, W >= 1 and H * W < 2^31" in lib().aarmvs_last_error()
    nmap = torch.zeros(4, 4, 3, dtype=torch.float32, device="cuda")
    nxyz = torch.full((16, 3), -7.5, dtype=torch.float32, device="cuda")
    assert lib().aarmvs_fusion_points_normals(ctypes.byref(a), nmap.data_ptr(), nxyz.data_ptr(), stream) != 0
    torch.cuda.synchronize()
    assert int(count.item()) == -3 and bool((xyz == -7.5).all()) and bool((nxyz == -7.5).all())


def test_shapes_next_to_the_rejected_ones_are_accepted():
    """The smallest accepted filter call (1 x 1, one source view) and the largest accepted source
    count run: the rejections above are not a blanket refusal."""
    for name in ("thin_1x1_n1", "both_n10"):
        case = ec.BY_NAME[name]
        got = _gpu_filter(case)
        np.testing.assert_array_equal(got[0].cpu().numpy(), ec.reference(case)[0])
