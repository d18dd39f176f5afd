"""Tanks and Temples fusion (fusion_padding.py): the pyrDown restatement's known answers, the
halved cameras, the vote-rule equivalence with fusion.py, the numpy matmul rounding the point
kernel rests on, the command line, and (GPU) ``pyr_down``, ``fuse_points_gpu`` and the
``filter_depth_tnt`` driver, bit for bit against numpy.

cv2 is not installed and the reference ships no fusion fixtures: parity is against the numpy
restatement tests/fusion_tnt_ref.py (cv2.pyrDown itself: parity unpinned)."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "aa-rmvsnet_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fusion_tnt_ref as tr  # noqa: E402
from oracle import fusion_oracle as fo  # noqa: E402
from aarmvs import fusion, synthetic as syn  # noqa: E402
from aarmvs._lib import AarmvsError  # noqa: E402

CAM_TXT = ("extrinsic\n1 0 0 10\n0 1 0 20\n0 0 1 30\n0 0 0 1\n\nintrinsic\n"
           "361.54 0 82.9\n0 360.4 66.4\n0 0 1\n\n425 2.5\n")


# ---------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------
def test_pyr_down_restatement_known_answers():
    # a constant image stays constant to the last bit: 6c, 8c, 14c, 15c, 16c and 256c / 256 are
    # exact for a constant with a few spare mantissa bits
    for c in (0.40625, 1.0, 201.0 / 256.0):
        out = tr.pyr_down(np.full((9, 12, 3), c, np.float32))
        assert out.shape == (5, 6, 3)
        np.testing.assert_array_equal(out, np.full((5, 6, 3), c, np.float32))
    # a unit impulse at an even interior pixel: the 5x5 kernel at its even taps
    img = np.zeros((12, 14), np.float32)
    img[4, 6] = 1.0
    out = tr.pyr_down(img)
    k = np.array([1, 4, 6, 4, 1], np.float64)
    want = np.zeros((6, 7), np.float32)
    want[1:4, 2:5] = (np.outer(k, k) / 256.0)[0::2, 0::2]
    np.testing.assert_array_equal(out, want)
    # REFLECT_101 corners of a 4x4 ramp s[i][j] = 4 i + j, by hand: at x = 0 the row pass is
    # 6 s0 + 4 (s1 + s1) + s2 + s2 = 64 i + 12, and down the rows at y = 0
    # 6 r0 + 4 (r1 + r1) + r2 + r2 = 72 + 608 + 280 = 960 -> 3.75; at x = 1 (tap 4 -> 2) the row
    # pass is 64 i + 30, at y = 1 (row 4 -> 2) 6*158 + 4 (94 + 222) + 30 + 158 = 2400 -> 9.375
    out = tr.pyr_down(np.arange(16, dtype=np.float32).reshape(4, 4))
    assert out.shape == (2, 2)
    assert out[0, 0] == np.float32(3.75) and out[1, 1] == np.float32(9.375)
    # odd sizes round up
    assert tr.pyr_down(np.zeros((9, 13, 3), np.float32)).shape == (5, 7, 3)
    assert tr.pyr_down(np.zeros((7, 4), np.float32)).shape == (4, 2)


def test_read_camera_parameters_tnt(tmp_path):
    (tmp_path / "00000000_cam.txt").write_text(CAM_TXT)
    K0, E0 = fusion.read_camera_parameters(str(tmp_path / "00000000_cam.txt"))
    K, E = fusion.read_camera_parameters_tnt(str(tmp_path / "00000000_cam.txt"))
    assert K.dtype == np.float32 and E.dtype == np.float32
    np.testing.assert_array_equal(K[:2], K0[:2] / np.float32(2))
    np.testing.assert_array_equal(K[2], K0[2])
    np.testing.assert_array_equal(E, E0)
    Kr, Er = tr.read_camera_parameters(CAM_TXT)
    np.testing.assert_array_equal(K, Kr)
    np.testing.assert_array_equal(E, Er)


@pytest.mark.parametrize("nsrc", [1, 4, 7, 10])
def test_fixed_vote_rule_equals_the_counted_one(nsrc):
    """fusion_padding.py counts all nine thresholds and asks >= 10, fusion.py counts i < nsrc + 1
    and asks >= nsrc + 1: threshold i can only collect i votes from nsrc >= i views, so up to 10
    source views the masks and averages are the same, and the filter kernel serves both."""
    depths, cams, conf = syn.fusion_views(36, 52, nsrc, seed=20 + nsrc)
    a = fo.filter_depth_core(depths[0], conf, cams[0], depths[1:], cams[1:], 0.3)
    b = tr.filter_depth_core(depths[0], conf, cams[0], depths[1:], cams[1:], 0.3)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert a[3].dtype == np.float64


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


@pytest.mark.parametrize("N", [2, 3, 5, 7, 13, 697])
def test_numpy_matmul_is_an_fma_chain_at_ragged_widths(N):
    """The point kernel's float64 products (csrc/fusion.hip mrow) assume numpy's matmul of a
    float32 3x3 / 4x4 matrix with a float64 [k, N] block rounds like fma(a_k, b_k, ... fma(a_1,
    b_1, a_0 * b_0)) whatever the number of kept pixels N (N = 1 takes another BLAS path and is
    kept out of the comparisons)."""
    rng = np.random.default_rng(N)
    for k in (3, 4):
        A = rng.standard_normal((k, k)).astype(np.float32)
        B = rng.standard_normal((k, N)) * 613.7
        C = np.matmul(A, B)
        for r in range(k):
            for j in range(N):
                s = float(A[r, 0]) * B[0, j]
                for q in range(1, k):
                    s = _fma(float(A[r, q]), B[q, j], s)
                assert s == C[r, j], (k, r, j)


def test_cli_arguments_and_defaults(tmp_path):
    base = ["--testpath", "/data", "--testlist", "list.txt", "--outdir", "/out"]
    a = fusion.parse_args(["--test_dataset", "tnt"] + base)
    assert (a.test_dataset, a.testpath, a.testlist, a.outdir) == ("tnt", "/data", "list.txt", "/out")
    assert a.photo_threshold == 0.3                       # fusion_padding.py:173
    assert fusion.parse_args(["--test_dataset", "dtu"] + base).photo_threshold == 0.35   # fusion.py:285
    assert fusion.parse_args(["--test_dataset", "dtu", "--photo_threshold", "0.5"] + base).photo_threshold == 0.5
    with pytest.raises(SystemExit):
        fusion.parse_args(["--test_dataset", "eth3d"] + base)
    with pytest.raises(SystemExit):
        fusion.parse_args(["--test_dataset", "tnt"])
    assert fusion.ply_path("/out", "Family", "tnt") == os.path.join("/out", "Family.ply")
    assert fusion.ply_path("/out", "scan9", "dtu") == os.path.join("/out", "mvsnet_009_l3.ply")
    # main() hands every scan of the list to the dataset's driver
    (tmp_path / "list.txt").write_text("Family\nHorse\n")
    calls = []
    saved = fusion.filter_depth_tnt, fusion.filter_depth
    fusion.filter_depth_tnt = lambda *a: calls.append(("tnt",) + a)
    fusion.filter_depth = lambda *a: calls.append(("dtu",) + a)
    try:
        fusion.main(["--test_dataset", "tnt", "--testpath", "/data", "--testlist", str(tmp_path / "list.txt"),
                     "--outdir", "/out"])
    finally:
        fusion.filter_depth_tnt, fusion.filter_depth = saved
    assert calls == [("tnt", "/data/Family", "/out/Family", "/out/Family.ply", 0.3, "cuda"),
                     ("tnt", "/data/Horse", "/out/Horse", "/out/Horse.ply", 0.3, "cuda")]


# ---------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("H,W,C", [(4, 4, 3), (8, 8, 3), (9, 13, 3), (67, 130, 3), (41, 1030, 3), (9, 13, 1)])
def test_gpu_pyr_down_matches_restatement(H, W, C):
    import torch
    rng = np.random.default_rng(H * 1000 + W)
    img = (rng.integers(0, 256, (H, W, C)).astype(np.float32) / np.float32(255.0))
    if C == 1:
        img = img[:, :, 0]
    out = fusion.pyr_down(torch.from_numpy(img).cuda())
    want = tr.pyr_down(img)
    assert out.dtype == torch.float32 and tuple(out.shape) == want.shape
    np.testing.assert_array_equal(out.cpu().numpy(), want)


@pytest.mark.gpu
def test_gpu_pyr_down_rejects_bad_input():
    import torch
    with pytest.raises(AarmvsError):
        fusion.pyr_down(torch.zeros(3, 8, 3, device="cuda"))          # H < 4
    with pytest.raises(AarmvsError):
        fusion.pyr_down(torch.zeros(8, 8, 3))                         # CPU tensor
    with pytest.raises(AarmvsError):
        fusion.pyr_down(torch.zeros(8, 8, 3, device="cuda", dtype=torch.float64))
    with pytest.raises(AarmvsError):
        fusion.pyr_down(torch.zeros(8, 8, 2, device="cuda"))


def _random_image(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3)).astype(np.float32) / np.float32(255.0)


def _check_points(avg, final, cam, img):
    """fuse_points_gpu against the host fuse_points on the same (numpy) inputs."""
    import torch
    xyz_w, rgb_w = fusion.fuse_points(avg, final, cam, img)
    assert xyz_w.shape[0] >= 100
    xyz, rgb = fusion.fuse_points_gpu(torch.from_numpy(avg).cuda(), torch.from_numpy(final).cuda(), cam,
                                      torch.from_numpy(img).cuda())
    assert xyz.is_cuda and xyz.dtype == torch.float32 and rgb.dtype == torch.uint8
    assert xyz.shape[0] == rgb.shape[0] == xyz_w.shape[0] == int(final.sum())
    np.testing.assert_array_equal(xyz.cpu().numpy(), xyz_w)
    np.testing.assert_array_equal(rgb.cpu().numpy(), rgb_w)
    # without an image: the same points, no colours
    xyz2, none = fusion.fuse_points_gpu(torch.from_numpy(avg).cuda(), torch.from_numpy(final).cuda(), cam)
    assert none is None
    np.testing.assert_array_equal(xyz2.cpu().numpy(), xyz_w)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,nsrc", [(36, 52, 10), (43, 61, 4)])
def test_gpu_points_after_the_filter(H, W, nsrc):
    import torch
    depths, cams, conf = syn.fusion_views(H, W, nsrc, seed=H)
    kept = fo.filter_depth_core(depths[0], conf, cams[0], depths[1:], cams[1:], 0.3)[2]
    assert kept.mean() >= 0.25
    t = [torch.from_numpy(d).cuda() for d in depths]
    _, _, final, avg = fusion.filter_depth_core(t[0], torch.from_numpy(conf).cuda(), cams[0], t[1:], cams[1:], 0.3)
    np.testing.assert_array_equal(final.cpu().numpy(), kept)
    img = _random_image(H, W, 1)
    xyz_w, rgb_w = fusion.fuse_points(avg, final, cams[0], img)
    assert xyz_w.shape[0] >= 100
    xyz, rgb = fusion.fuse_points_gpu(avg, final, cams[0], torch.from_numpy(img).cuda())
    np.testing.assert_array_equal(xyz.cpu().numpy(), xyz_w)
    np.testing.assert_array_equal(rgb.cpu().numpy(), rgb_w)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,p", [(600, 512, 0.5),     # more blocks than the scan's workgroup has threads
                                   (75, 101, 1.0)])     # all kept; 7575 pixels: no multiple of 64
def test_gpu_points_masks(H, W, p):
    rng = np.random.default_rng(H)
    _, cams, _ = syn.fusion_views(8, 8, 1, seed=2)
    avg = rng.uniform(400.0, 900.0, (H, W))
    final = rng.random((H, W)) < p
    assert final.all() == (p == 1.0)
    _check_points(avg, final, cams[0], _random_image(H, W, 5))


@pytest.mark.gpu
def test_gpu_points_empty_mask_and_capacity():
    import torch
    H, W = 75, 101
    rng = np.random.default_rng(9)
    _, cams, _ = syn.fusion_views(8, 8, 1, seed=2)
    avg = torch.from_numpy(rng.uniform(400.0, 900.0, (H, W))).cuda()
    img = torch.from_numpy(_random_image(H, W, 6)).cuda()

    def buffers(n):
        return (torch.full((n, 3), -7.5, dtype=torch.float32, device="cuda"),
                torch.full((n, 3), 0xA5, dtype=torch.uint8, device="cuda"))

    # nothing kept: count 0, the buffers keep their fill pattern
    xyz, rgb = buffers(64)
    none = torch.zeros(H, W, dtype=torch.bool, device="cuda")
    assert int(fusion.fuse_points_into(avg, none, cams[0], img, xyz, rgb).item()) == 0
    assert bool((xyz == -7.5).all()) and bool((rgb == 0xA5).all())
    x0, c0 = fusion.fuse_points_gpu(avg, none, cams[0], img)
    assert tuple(x0.shape) == (0, 3) and tuple(c0.shape) == (0, 3)
    # room for 7 points fewer than are kept, inside a larger buffer: exactly `capacity` points
    # written, the fill pattern intact after them, and the count still the total
    final = torch.from_numpy(rng.random((H, W)) < 0.5).cuda()
    xyz_w, rgb_w = fusion.fuse_points(avg, final, cams[0], img.cpu().numpy())
    n = xyz_w.shape[0]
    assert n >= 107
    xyz, rgb = buffers(n + 32)
    cap = n - 7
    count = fusion.fuse_points_into(avg, final, cams[0], img, xyz[:cap], rgb[:cap])
    assert int(count.item()) == n
    np.testing.assert_array_equal(xyz[:cap].cpu().numpy(), xyz_w[:cap])
    np.testing.assert_array_equal(rgb[:cap].cpu().numpy(), rgb_w[:cap])
    assert bool((xyz[cap:] == -7.5).all()) and bool((rgb[cap:] == 0xA5).all())


@pytest.mark.gpu
def test_gpu_points_reject_bad_input():
    import torch
    _, cams, _ = syn.fusion_views(8, 8, 1, seed=2)
    avg = torch.full((16, 16), 500.0, dtype=torch.float64)
    final = torch.ones(16, 16, dtype=torch.bool)
    with pytest.raises(AarmvsError):
        fusion.fuse_points_gpu(avg, final, cams[0])                               # CPU tensors
    with pytest.raises(AarmvsError):
        fusion.fuse_points_gpu(avg.cuda().float(), final.cuda(), cams[0])         # float32 average
    with pytest.raises(AarmvsError):
        fusion.fuse_points_gpu(avg.cuda(), final.cuda().float(), cams[0])         # float mask
    with pytest.raises(AarmvsError):
        fusion.fuse_points_gpu(avg.cuda(), final.cuda(), cams[0], torch.zeros(16, 16, 3, dtype=torch.float64,
                                                                              device="cuda"))
    with pytest.raises(AarmvsError):
        fusion.fuse_points_gpu(avg.cuda(), final.cuda(), cams[0], torch.zeros(20, 16, 3, device="cuda"))


# the scan: 12 views of 36x52 maps stored as 40x52 PFMs (2 junk rows above and below), 72x104
# images, cam files with 2 K.  Reference views 0 and 1 take 10 source views each from views
# 0 .. 10; view 11 is nobody's source view (the skip test lists it as a third reference view).
H_MAP, W_MAP, N_VIEWS = 36, 52, 12


def _write_tnt_scan(root, img_hw=(2 * H_MAP, 2 * W_MAP), with_view_11=False):
    from PIL import Image
    depths, cams, conf = syn.fusion_views(H_MAP, W_MAP, N_VIEWS - 1, seed=11)
    scan, out = root / "Family", root / "out" / "Family"
    for d in ("cams", "images"):
        (scan / d).mkdir(parents=True, exist_ok=True)
    for d in ("depth_est_0", "confidence_0"):
        (out / d).mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(3)
    images, cam_texts, dmaps, confs = {}, {}, {}, {}

    def padded(m):
        junk = rng.uniform(-1e6, 1e6, (H_MAP + 4, W_MAP)).astype(np.float32)
        junk[2:-2] = m
        return junk

    for v in range(N_VIEWS):
        K, E = cams[v]
        K = K.copy()
        K[:2] *= 2                              # the full-size image's intrinsics
        txt = ("extrinsic\n" + "\n".join(" ".join(repr(float(q)) for q in row) for row in E)
               + "\n\nintrinsic\n" + "\n".join(" ".join(repr(float(q)) for q in row) for row in K)
               + "\n\n425 2.5\n")
        (scan / "cams" / "{:0>8}_cam.txt".format(v)).write_text(txt)
        cam_texts[v] = txt
        img = (rng.random(tuple(img_hw) + (3,)) * 255).astype(np.uint8)
        Image.fromarray(img).save(str(scan / "images" / "{:0>8}.jpg".format(v)), format="PNG")
        images[v] = np.array(Image.open(str(scan / "images" / "{:0>8}.jpg".format(v))), np.float32) / 255.0
        dmaps[v] = padded(depths[v])
        confs[v] = padded(np.roll(conf, 7 * v, axis=1) if v else conf)
        fusion.save_pfm(str(out / "depth_est_0" / "{:0>8}.pfm".format(v)), dmaps[v])
        fusion.save_pfm(str(out / "confidence_0" / "{:0>8}.pfm".format(v)), confs[v])
    pair = [(0, list(range(1, 11))), (1, [0] + list(range(2, 11)))]
    if with_view_11:
        pair.append((11, list(range(1, 11))))
    with open(scan / "pair.txt", "w") as f:
        f.write(f"{len(pair)}\n")
        for v, srcs in pair:
            f.write(f"{v}\n{len(srcs)} " + " ".join(f"{s} {9.0 - 0.5 * s:.1f}" for s in srcs) + "\n")
    return scan, out, (pair, images, cam_texts, dmaps, confs)


_SCAN_WANT = {}


def _scan_want(inputs):
    """The restatement's answer for the scan (the inputs are seeded: computed once)."""
    if not _SCAN_WANT:
        _SCAN_WANT["v"] = tr.filter_depth_scan(*inputs, 0.3)
    return _SCAN_WANT["v"]


def _check_scan_outputs(out, ply, npts, want):
    from PIL import Image
    masks, xyz, rgb = want
    assert npts == xyz.shape[0]
    assert sorted(os.listdir(str(out / "mask"))) == sorted(
        "{:0>8}_{}.png".format(v, n) for v in masks for n in ("photo", "geo", "final"))
    for v, (photo, geo, final) in masks.items():
        assert final.mean() >= 0.25
        for name, m in (("photo", photo), ("geo", geo), ("final", final)):
            png = np.array(Image.open(str(out / "mask" / "{:0>8}_{}.png".format(v, name))))
            np.testing.assert_array_equal(png, m.astype(np.uint8) * 255)
    body = np.empty(npts, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                                 ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for i, f in enumerate(("x", "y", "z")):
        body[f] = xyz[:, i]
    for i, f in enumerate(("red", "green", "blue")):
        body[f] = rgb[:, i]
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex {}\nproperty float x\nproperty float y\n"
            "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
            "end_header\n").format(npts).encode("ascii")
    assert ply.read_bytes() == head + body.tobytes()


@pytest.mark.gpu
def test_gpu_filter_depth_tnt_scan_matches_restatement(tmp_path):
    """The per-scan driver through the command line's main(): masks and PLY byte for byte.
    (The images are 72x104, twice the cropped 36x52 maps, as 1080x1920 is of 540x960: an 80x104
    image halves to 40x52, which the driver rejects -- see the wrong-size test.)"""
    scan, out, inputs = _write_tnt_scan(tmp_path)
    want = _scan_want(inputs)
    assert sorted(want[0]) == [0, 1]
    (tmp_path / "list.txt").write_text("Family\n")
    fusion.main(["--test_dataset", "tnt", "--testpath", str(tmp_path), "--testlist", str(tmp_path / "list.txt"),
                 "--outdir", str(tmp_path / "out")])
    ply = tmp_path / "out" / "Family.ply"
    head = ply.read_bytes().split(b"end_header\n", 1)[0]
    npts = int(head.split(b"element vertex ")[1].split(b"\n")[0])
    _check_scan_outputs(out, ply, npts, want)


@pytest.mark.gpu
def test_gpu_filter_depth_tnt_skips_a_view_without_depth(tmp_path, capsys):
    scan, out, inputs = _write_tnt_scan(tmp_path, with_view_11=True)
    os.remove(str(out / "depth_est_0" / "{:0>8}.pfm".format(11)))
    ply = tmp_path / "Family.ply"
    npts = fusion.filter_depth_tnt(str(scan), str(out), str(ply))
    assert "skip 11" in capsys.readouterr().out
    pair, images, cam_texts, dmaps, confs = inputs
    _check_scan_outputs(out, ply, npts, _scan_want((pair[:2], images, cam_texts, dmaps, confs)))


@pytest.mark.gpu
def test_gpu_filter_depth_tnt_rejects_a_wrong_size_image(tmp_path):
    scan, out, _ = _write_tnt_scan(tmp_path, img_hw=(80, 104))
    with pytest.raises(AarmvsError, match=r"\(40, 52\).*\(36, 52\)"):
        fusion.filter_depth_tnt(str(scan), str(out), str(tmp_path / "Family.ply"))
