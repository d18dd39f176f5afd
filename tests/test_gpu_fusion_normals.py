"""The per-point normals on the GPU (``aarmvs_fusion_normals``, ``aarmvs_fusion_points_normals``,
``fusion.fuse_views``, both file drivers), bit for bit against the numpy restatement
tests/fusion_normals_ref.py."""
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
import fusion_normals_ref as nr  # noqa: E402
import fusion_tnt_ref as tr  # noqa: E402
from test_gpu_fusion_dedup import H_SCAN, NSRC_SCAN, W_SCAN, _write_scan  # noqa: E402
from aarmvs import fusion  # noqa: E402

pytestmark = pytest.mark.gpu

# smaller than the r = 2 window; one pixel past a 16x64 tile each way; odd; exact tile multiples
SHAPES = [(3, 4), (17, 65), (37, 53), (64, 128)]
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _inputs(H, W):
    """(depth float64 [H,W], valid bool [H,W], (K, E)): a slanted plane with a sphere in front of it,
    0.2 % multiplicative noise, a 5 % step down the middle, about 40 % holes, a stripe whose only
    valid row is its middle one (where the image is tall enough), and NaN, +inf, 0 and a negative
    depth planted -- valid -- at corner, edge and interior pixels."""
    rng = np.random.default_rng(1000 * H + W)
    K, E = nr.camera(f=4.5 * W, cx=W / 2.0, cy=H / 2.0, seed=H)
    depth = nr.plane_depth(K, H, W, (0.3, -0.2, -1.0), 600.0)
    ball, _ = nr.sphere_depth(K, H, W, (0.0, 0.0, 640.0), 70.0)
    with np.errstate(invalid="ignore"):
        depth = np.where(ball < depth, ball, depth)
    depth = depth * (1.0 + 0.002 * rng.standard_normal((H, W)))
    depth[:, W // 2:] *= 1.05
    valid = rng.random((H, W)) > 0.4
    if H >= 16:
        valid[H - 10:H - 3] = False
        valid[H - 7] = True
    bad = [np.nan, np.inf, 0.0, -600.0]
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    edges = [(0, W // 2), (H // 2, 0), (H - 1, W // 3), (H // 3, W - 1)]
    inner = [(H // 2, W // 2), (H // 3, W // 3), (H // 2, W // 4), (H // 4, (2 * W) // 3)]
    for spots in (inner, edges, corners):
        for (y, x), b in zip(spots, bad):
            depth[y, x], valid[y, x] = b, True
    return depth, valid, (K, E)


def _case(H, W, r):
    if (H, W) not in _CACHE:
        _CACHE[(H, W)] = (_inputs(H, W), {})
    inp, want = _CACHE[(H, W)]
    if r not in want:
        want[r] = nr.estimate_normals(*inp, radius=r)
    return inp, want[r]


def _gpu(inp, **kw):
    import torch
    depth, valid, cam = inp
    n, h = fusion.estimate_normals(torch.from_numpy(depth).cuda(), torch.from_numpy(valid).cuda(), cam, **kw)
    return n.cpu().numpy(), h.cpu().numpy()


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_matches_restatement_bit_for_bit(shape, radius):
    """Every pixel, no exclusions: has_normal and the float32 normals are equal bit for bit (float64
    sqrt and division on the device are correctly rounded)."""
    inp, (want_n, want_h) = _case(*shape, radius)
    got_n, got_h = _gpu(inp, radius=radius)
    if min(shape) > 8:
        assert 0 < want_h.sum() < inp[1].sum()                     # some fits succeed, some windows fail
    np.testing.assert_array_equal(got_h, want_h)
    same = _bits(got_n) == _bits(want_n)
    print(f"{shape} r={radius}: {want_h.sum()} normals, {same.mean():.6f} of the components bit-equal, "
          f"max |diff| {np.abs(got_n - want_n).max():.3e}")
    assert same.all()
    assert not got_n[~got_h].any()


def test_the_inputs_hold_what_they_should():
    depth, valid, cam = _case(37, 53, 2)[0]
    assert np.isnan(depth).sum() == 3 and np.isposinf(depth).sum() == 3 and (depth == 0).sum() == 3 \
        and (depth < 0).sum() == 3
    assert 0.4 < valid.mean() < 0.7
    _, has = _case(37, 53, 3)[1]
    assert valid[37 - 7].all() and not has[37 - 7].any()           # the stripe's row is collinear
    assert not has[~valid].any()


def test_min_count_and_jump_reach_the_kernel():
    inp = _case(37, 53, 2)[0]
    for kw in (dict(radius=2, min_count=9), dict(radius=3, max_rel_jump=0.1, min_count=20),
               dict(radius=1, max_rel_jump=0.0)):
        want_n, want_h = nr.estimate_normals(*inp, **kw)
        got_n, got_h = _gpu(inp, **kw)
        np.testing.assert_array_equal(got_h, want_h)
        np.testing.assert_array_equal(_bits(got_n), _bits(want_n))


def test_null_has_normal_and_a_second_call():
    import torch
    from aarmvs import _lib, lib
    (depth, valid, cam), (want_n, want_h) = _case(17, 65, 2)
    H, W = depth.shape
    d, v = torch.from_numpy(depth).cuda(), torch.from_numpy(valid).cuda()
    cams = fusion.pack_normal_cameras(cam)
    out = torch.full((H, W, 3), 7.0, dtype=torch.float32, device="cuda")
    a = _lib.FusionNormalsArgs()
    a.H, a.W = H, W
    a.depth, a.valid, a.cams = d.data_ptr(), v.data_ptr(), cams.ctypes.data
    a.radius, a.min_count, a.max_rel_jump = 2, 3, 0.01
    a.normal, a.has_normal = out.data_ptr(), None
    _lib.check(lib().aarmvs_fusion_normals(ctypes.byref(a), torch.cuda.current_stream().cuda_stream),
               "fusion_normals")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(want_n))
    # twice more through Python: identical bits
    first = fusion.estimate_normals(d, v, cam)
    second = fusion.estimate_normals(d, v, cam)
    assert torch.equal(first[0].view(torch.int32), second[0].view(torch.int32)) and torch.equal(first[1], second[1])
    assert torch.equal(first[0].view(torch.int32), out.view(torch.int32))
    # a uint8 mask is a mask too
    third = fusion.estimate_normals(d, v.to(torch.uint8) * 3, cam)
    assert torch.equal(first[0].view(torch.int32), third[0].view(torch.int32))


def test_fuse_points_normals_gpu():
    import torch
    (depth, valid, cam), (want_n, want_h) = _case(64, 128, 2)
    H, W = depth.shape
    rng = np.random.default_rng(5)
    avg = torch.from_numpy(np.where(np.isfinite(depth) & (depth > 0), depth, 600.0)).cuda()
    mask = torch.from_numpy(valid).cuda()
    img = torch.from_numpy(rng.random((H, W, 3)).astype(np.float32)).cuda()
    nmap = torch.from_numpy(want_n).cuda()
    xyz0, rgb0 = fusion.fuse_points_gpu(avg, mask, cam, img)
    xyz, rgb, nrm = fusion.fuse_points_normals_gpu(avg, mask, cam, img, nmap)
    n = int(valid.sum())
    assert xyz.shape == nrm.shape == (n, 3) and n > 4 * 1024        # several blocks' chunks
    assert torch.equal(xyz.view(torch.int32), xyz0.view(torch.int32)) and torch.equal(rgb, rgb0)
    np.testing.assert_array_equal(_bits(nrm.cpu().numpy()), _bits(want_n[valid]))
    # without an image
    xyz1, none, nrm1 = fusion.fuse_points_normals_gpu(avg, mask, cam, None, nmap)
    assert none is None and torch.equal(xyz1, xyz0) and torch.equal(nrm1.view(torch.int32), nrm.view(torch.int32))
    # a capacity below the count: the first points, nothing past them, the full count
    cap = n // 2 + 1
    bx = torch.full((n, 3), -5.0, dtype=torch.float32, device="cuda")
    bn = torch.full((n, 3), -6.0, dtype=torch.float32, device="cuda")
    bc = torch.full((n, 3), 9, dtype=torch.uint8, device="cuda")
    count = fusion.fuse_points_into(avg, mask, cam, img, bx[:cap], bc[:cap], normal_map=nmap, nrm=bn[:cap])
    assert int(count.item()) == n
    assert torch.equal(bx[:cap], xyz0[:cap]) and torch.equal(bc[:cap], rgb0[:cap])
    assert torch.equal(bn[:cap].view(torch.int32), nrm[:cap].view(torch.int32))
    assert (bx[cap:] == -5.0).all() and (bn[cap:] == -6.0).all() and (bc[cap:] == 9).all()
    # an all-zero mask
    none_kept = torch.zeros_like(mask)
    x0, c0, n0 = fusion.fuse_points_normals_gpu(avg, none_kept, cam, img, nmap)
    assert x0.shape == n0.shape == (0, 3) and c0.shape == (0, 3)
    with pytest.raises(fusion.AarmvsError):
        fusion.fuse_points_into(avg, mask, cam, img, bx, bc, normal_map=nmap)          # normals out missing
    with pytest.raises(fusion.AarmvsError):
        fusion.fuse_points_normals_gpu(avg, mask, cam, img, nmap[:-1])                  # another size


def _cuda(d):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def _scan(case, dedup):
    key = ("scan", case, dedup)
    if key not in _CACHE:
        sc = dr.scene(*case)
        with np.errstate(all="ignore"):
            _CACHE[key] = (sc, nr.fuse_views_normals(*sc, dedup=dedup))
    return _CACHE[key]


@pytest.mark.parametrize("dedup", [False, True])
@pytest.mark.parametrize("case", [(40, 52, 2, 2), (75, 101, 4, 1)])
def test_fuse_views_with_normals_matches_restatement(case, dedup):
    import torch
    sc, want = _scan(case, dedup)
    pairs, depths, confs, cams, images = sc
    d, c, im = _cuda(depths), _cuda(confs), _cuda(images)
    got = fusion.fuse_views(pairs, d, c, cams, im, 0.35, dedup=dedup, normals=True)
    plain = fusion.fuse_views(pairs, d, c, cams, im, 0.35, dedup=dedup)
    assert "normals" not in plain and "normal_maps" not in plain and "has_normal" not in plain
    # everything the call returns without normals is bit-equal with them
    assert got["counts"] == plain["counts"] == want["counts"]
    assert torch.equal(got["xyz"].view(torch.int32), plain["xyz"].view(torch.int32))
    assert torch.equal(got["rgb"], plain["rgb"])
    for v in plain["masks"]:
        assert sorted(got["masks"][v]) == sorted(plain["masks"][v])
        for k in plain["masks"][v]:
            assert torch.equal(got["masks"][v][k], plain["masks"][v][k])
        assert torch.equal(got["avg"][v], plain["avg"][v])
    # and the restatement's
    np.testing.assert_array_equal(got["xyz"].cpu().numpy(), want["xyz"])
    np.testing.assert_array_equal(got["rgb"].cpu().numpy(), want["rgb"])
    assert sorted(got["normal_maps"]) == sorted(want["normal_maps"]) == sorted(got["has_normal"])
    for v in want["normal_maps"]:
        np.testing.assert_array_equal(got["has_normal"][v].cpu().numpy(), want["has_normal"][v], err_msg=f"view {v}")
        np.testing.assert_array_equal(_bits(got["normal_maps"][v].cpu().numpy()), _bits(want["normal_maps"][v]))
        # the fit's mask is the final mask, also under dedup
        final = want["masks"][v]["final"]
        assert not want["has_normal"][v][~final].any() and want["has_normal"][v][final].mean() > 0.99
    assert got["normals"].shape == got["xyz"].shape
    np.testing.assert_array_equal(_bits(got["normals"].cpu().numpy()), _bits(want["normals"]))
    if dedup:
        # a de-duplicated view keeps its neighbours: an emit-mask fit would lose normals
        later = pairs[-1][0]
        emit = want["masks"][later]["emit"]
        _, has_emit = nr.estimate_normals(want["avg"][later], emit, cams[later])
        assert emit.sum() > 0 and has_emit[emit].sum() < want["has_normal"][later][emit].sum()


def test_fuse_views_require_normal_and_parameters():
    sc, _ = _scan((40, 52, 2, 2), True)
    pairs, depths, confs, cams, images = sc
    params = dict(radius=3, min_count=30)
    with np.errstate(all="ignore"):
        want = nr.fuse_views_normals(*sc, dedup=True, normals=params, require_normal=True)
    got = fusion.fuse_views(pairs, _cuda(depths), _cuda(confs), cams, _cuda(images), 0.35, dedup=True,
                            normals=params, require_normal=True)
    assert got["counts"] == want["counts"] and 0 < want["xyz"].shape[0]
    np.testing.assert_array_equal(got["xyz"].cpu().numpy(), want["xyz"])
    np.testing.assert_array_equal(got["rgb"].cpu().numpy(), want["rgb"])
    np.testing.assert_array_equal(_bits(got["normals"].cpu().numpy()), _bits(want["normals"]))
    assert got["normals"].cpu().numpy().any(axis=1).all()
    loose = fusion.fuse_views(pairs, _cuda(depths), _cuda(confs), cams, _cuda(images), 0.35, dedup=True,
                              normals=params)
    assert loose["xyz"].shape[0] > got["xyz"].shape[0]


# ---------------------------------------------------------------------------------
# the file drivers, on the scan tree of tests/test_gpu_fusion_dedup.py (48x64 maps, 3 source views)
# ---------------------------------------------------------------------------------
def _read_ply(path):
    """(xyz, rgb, normals or None) of a PLY as the drivers write it."""
    head, body = path.read_bytes().split(b"end_header\n", 1)
    names = [ln.split()[2].decode() for ln in head.split(b"\n") if ln.startswith(b"property")]
    with_normals = ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert names in (with_normals, with_normals[:3] + with_normals[6:])
    v = np.frombuffer(body, dtype=[(n, "u1" if n in ("red", "green", "blue") else "<f4") for n in names])
    assert v.shape[0] == int(head.split(b"element vertex ")[1].split(b"\n")[0])
    nrm = np.stack([v["nx"], v["ny"], v["nz"]], 1) if "nx" in names else None
    return np.stack([v["x"], v["y"], v["z"]], 1), np.stack([v["red"], v["green"], v["blue"]], 1), nrm


def _plain_bytes(tmp_path, want):
    """The PLY the drivers have always written for this cloud."""
    fusion.write_ply(str(tmp_path / "want.ply"), want["xyz"], want["rgb"])
    return (tmp_path / "want.ply").read_bytes()


def _check_ply(ply, want, require=False):
    xyz, rgb, nrm = _read_ply(ply)
    np.testing.assert_array_equal(xyz, want["xyz"])
    np.testing.assert_array_equal(rgb, want["rgb"])
    np.testing.assert_array_equal(_bits(nrm), _bits(want["normals"]))
    assert xyz.shape[0] > 0
    if require:
        assert nrm.any(axis=1).all()


def test_dtu_driver_with_and_without_normals(tmp_path, capsys):
    pad = 4
    scan, out, (pair, images, cam_texts, dmaps, confs) = _write_scan(tmp_path, H_SCAN, W_SCAN, NSRC_SCAN, pad)
    cams = {}
    for v, txt in cam_texts.items():
        lines = [ln.rstrip() for ln in txt.splitlines()]
        E = np.array(" ".join(lines[1:5]).split(), dtype=np.float32).reshape((4, 4))
        K = np.array(" ".join(lines[7:10]).split(), dtype=np.float32).reshape((3, 3))
        K[1, 2] -= pad
        cams[v] = (K, E)
    cropped = {v: im[pad:-pad] for v, im in images.items()}
    with np.errstate(all="ignore"):
        want = nr.fuse_views_normals(pair, dmaps, confs, cams, cropped, 0.35)
        req = nr.fuse_views_normals(pair, dmaps, confs, cams, cropped, 0.35, dedup=True, normals=dict(radius=1),
                                    require_normal=True)
    # without the flags: the bytes it has always written
    ply = tmp_path / "plain.ply"
    assert fusion.filter_depth(str(scan), str(out), str(ply), 0.35) == want["xyz"].shape[0]
    assert ply.read_bytes() == _plain_bytes(tmp_path, want)
    # with normals: the same points, and nx ny nz
    ply = tmp_path / "normals.ply"
    capsys.readouterr()
    assert fusion.filter_depth(str(scan), str(out), str(ply), 0.35, normals=True) == want["xyz"].shape[0]
    _check_ply(ply, want)
    missing = int((~want["normals"].any(axis=1)).sum())
    assert "points without a normal: {} of {}".format(missing, want["xyz"].shape[0]) in capsys.readouterr().out
    # through the command line, with the other knobs
    (tmp_path / "list.txt").write_text("scan1\n")
    fusion.main(["--test_dataset", "dtu", "--testpath", str(tmp_path), "--testlist", str(tmp_path / "list.txt"),
                 "--outdir", str(tmp_path / "out"), "--dedup", "--normals", "--normal_radius", "1",
                 "--require_normal"])
    _check_ply(tmp_path / "out" / "mvsnet_001_l3.ply", req, require=True)
    assert req["xyz"].shape[0] < want["xyz"].shape[0]


def test_tnt_driver_with_and_without_normals(tmp_path):
    scan, out, (pair, images, cam_texts, dmaps, confs) = _write_scan(tmp_path, H_SCAN, W_SCAN, NSRC_SCAN, 0, tnt=True)
    cams = {v: tr.read_camera_parameters(txt) for v, txt in cam_texts.items()}      # the halved intrinsics
    halved = {v: tr.pyr_down(im) for v, im in images.items()}
    crop = lambda maps: {v: m[2:-2] for v, m in maps.items()}  # noqa: E731
    with np.errstate(all="ignore"):
        want = nr.fuse_views_normals(pair, crop(dmaps), crop(confs), cams, halved, 0.3, core=tr.filter_depth_core)
        req = nr.fuse_views_normals(pair, crop(dmaps), crop(confs), cams, halved, 0.3, core=tr.filter_depth_core,
                                    normals=dict(min_count=20), require_normal=True)
    ply = tmp_path / "plain.ply"
    assert fusion.filter_depth_tnt(str(scan), str(out), str(ply)) == want["xyz"].shape[0]
    assert ply.read_bytes() == _plain_bytes(tmp_path, want)
    ply = tmp_path / "normals.ply"
    assert fusion.filter_depth_tnt(str(scan), str(out), str(ply), normals=True) == want["xyz"].shape[0]
    _check_ply(ply, want)
    (tmp_path / "list.txt").write_text("scan1\n")
    fusion.main(["--test_dataset", "tnt", "--testpath", str(tmp_path), "--testlist", str(tmp_path / "list.txt"),
                 "--outdir", str(tmp_path / "out"), "--normals", "--normal_min_count", "20", "--require_normal"])
    _check_ply(tmp_path / "out" / "scan1.ply", req, require=True)
    assert 0 < req["xyz"].shape[0] < want["xyz"].shape[0]
