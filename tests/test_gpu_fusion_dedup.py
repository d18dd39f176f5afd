"""The visibility de-duplication on the GPU (``aarmvs_fusion_filter_dedup``, ``fusion.fuse_views``,
both file drivers), bit for bit against the numpy restatement tests/fusion_dedup_ref.py."""
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
import fusion_tnt_ref as tr  # noqa: E402
from oracle import fusion_oracle as fo  # noqa: E402
from aarmvs import fusion, synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(40, 52, 2, 2), (75, 101, 4, 1), (96, 128, 10, 0)]
_WANT = {}


def _want(key, make):
    """A scan and the restatement's answer for it: computed once, shared, never modified."""
    if key not in _WANT:
        sc = make()
        with np.errstate(all="ignore"):
            _WANT[key] = (sc, dr.fuse_views(*sc, dedup=True))
    return _WANT[key]


def _cuda(d):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def _gpu_scan(sc, dedup=True, photo_threshold=0.35):
    pairs, depths, confs, cams, images = sc
    return fusion.fuse_views(pairs, _cuda(depths), _cuda(confs), cams, _cuda(images), photo_threshold, dedup=dedup)


def _check_scan(got, want, sc):
    pairs, depths, confs, cams, _ = sc
    assert sorted(got["masks"]) == sorted(want["masks"]) and got["counts"] == want["counts"]
    for v, m in want["masks"].items():
        for k in ("photo", "geo", "final", "emit"):
            np.testing.assert_array_equal(got["masks"][v][k].cpu().numpy(), m[k], err_msg=f"view {v} {k}")
        np.testing.assert_array_equal(got["avg"][v].cpu().numpy(), want["avg"][v])
    assert sorted(got["used"]) == sorted(want["used"])
    for v, u in want["used"].items():
        np.testing.assert_array_equal(got["used"][v].cpu().numpy(), u, err_msg=f"used map of view {v}")
    np.testing.assert_array_equal(got["xyz"].cpu().numpy(), want["xyz"])
    np.testing.assert_array_equal(got["rgb"].cpu().numpy(), want["rgb"])


@pytest.mark.parametrize("case", CASES)
def test_fuse_views_dedup_matches_restatement(case):
    sc, want = _want(case, lambda: dr.scene(*case))
    got = _gpu_scan(sc)
    _check_scan(got, want, sc)
    # the three masks and the averaged depth are the plain filter's
    pairs, depths, confs, cams, _ = sc
    ref, srcs = pairs[-1]
    with np.errstate(all="ignore"):
        photo, geo, final, avg = fo.filter_depth_core(depths[ref], confs[ref], cams[ref], [depths[s] for s in srcs],
                                                      [cams[s] for s in srcs], 0.35)
    for k, w in (("photo", photo), ("geo", geo), ("final", final)):
        np.testing.assert_array_equal(got["masks"][ref][k].cpu().numpy(), w)
    np.testing.assert_array_equal(got["avg"][ref].cpu().numpy(), avg)
    assert 0 < got["xyz"].shape[0] <= 0.6 * sum(int(m["final"].sum()) for m in want["masks"].values())


def test_reversed_view_order():
    sc, want = _want("reversed", lambda: dr.scene(75, 101, 4, 1, reverse=True))
    assert want["xyz"].shape[0] == 8026
    _check_scan(_gpu_scan(sc), want, sc)


def _cyclic():
    _, depths, confs, cams, images = dr.scene(45, 61, 4, 7)
    return [(v, [(v + 1) % 5, (v + 2) % 5]) for v in range(5)], depths, confs, cams, images


def test_views_that_list_only_their_two_cyclic_successors():
    sc, want = _want("cyclic", _cyclic)
    assert 0 < want["xyz"].shape[0] < sum(int(m["final"].sum()) for m in want["masks"].values())
    _check_scan(_gpu_scan(sc), want, sc)


def _missing():
    pairs, depths, confs, cams, images = dr.scene(45, 61, 4, 7)
    # view 4 is a reference view but nobody's source view, and it has no depth map
    pairs = [(v, [s for s in range(4) if s != v]) for v in (0, 1)] + [(4, [0, 1])] + \
            [(v, [s for s in range(4) if s != v]) for v in (2, 3)]
    depths = {v: d for v, d in depths.items() if v != 4}
    return pairs, depths, confs, cams, images


def test_a_reference_view_without_a_depth_map_is_skipped():
    sc, want = _want("missing", _missing)
    assert sorted(want["masks"]) == [0, 1, 2, 3]
    got = _gpu_scan(sc)
    assert 4 not in got["masks"] and 4 not in got["used"]
    _check_scan(got, want, sc)


def _one_view(case=(40, 52, 2, 2)):
    import torch
    pairs, depths, confs, cams, _ = dr.scene(*case)
    ref, srcs = pairs[0]
    host = (depths[ref], confs[ref], cams[ref], [depths[s] for s in srcs], [cams[s] for s in srcs], 0.35)
    dev = (torch.from_numpy(depths[ref]).cuda(), torch.from_numpy(confs[ref]).cuda(), cams[ref],
           [torch.from_numpy(depths[s]).cuda() for s in srcs], [cams[s] for s in srcs], 0.35)
    return host, dev


def test_used_srcs_with_none_entries_and_a_used_reference_map():
    import torch
    host, dev = _one_view()
    H, W = host[0].shape
    used_ref = (np.random.default_rng(4).random((H, W)) < 0.5).astype(np.uint8)
    u_want = np.zeros((H, W), np.uint8)
    with np.errstate(all="ignore"):
        want = dr.filter_depth_dedup(*host, used_ref, [None, u_want])
    assert u_want.sum() > 100 and 0 < want[3].sum() < want[2].sum()
    u = torch.zeros(H, W, dtype=torch.uint8, device="cuda")
    got = fusion.filter_depth_dedup(*dev, torch.from_numpy(used_ref).cuda(), [None, u])
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g.cpu().numpy(), w)
    np.testing.assert_array_equal(u.cpu().numpy(), u_want)


def test_used_ref_none_emits_every_final_pixel():
    import torch
    host, dev = _one_view()
    H, W = host[0].shape
    u_want = [np.zeros((H, W), np.uint8) for _ in range(2)]
    with np.errstate(all="ignore"):
        want = dr.filter_depth_dedup(*host, None, u_want)
    u = [torch.zeros(H, W, dtype=torch.uint8, device="cuda") for _ in range(2)]
    got = fusion.filter_depth_dedup(*dev, None, u)
    np.testing.assert_array_equal(got[3].cpu().numpy(), got[2].cpu().numpy())
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g.cpu().numpy(), w)
    for g, w in zip(u, u_want):
        np.testing.assert_array_equal(g.cpu().numpy(), w)
    # and with nothing to mark at all, the masks are still the same
    none = fusion.filter_depth_dedup(*dev, None, [None, None])
    for g, w in zip(none, want):
        np.testing.assert_array_equal(g.cpu().numpy(), w)


def test_guard_bytes_around_the_used_and_emit_maps():
    """A scan whose used and emit maps are carved out of one buffer filled with 0xAB: nothing
    outside the maps is written, and the used maps hold only 0 and 1."""
    import torch
    case = (40, 52, 2, 2)
    sc, want = _want(case, lambda: dr.scene(*case))
    pairs, depths, confs, cams, _ = sc
    H, W = depths[0].shape
    HW, G, n = H * W, 67, len(depths)          # 2080-byte maps at odd offsets
    buf = torch.full((2 * n * (HW + G) + G,), 0xAB, dtype=torch.uint8, device="cuda")
    slot = lambda i: buf[G + i * (HW + G):G + i * (HW + G) + HW].view(H, W)  # noqa: E731
    used = {v: slot(v) for v in depths}
    emit = {v: slot(n + v) for v in depths}
    for u in used.values():
        u.zero_()
    d, c = _cuda(depths), _cuda(confs)
    for ref, srcs in pairs:
        out = fusion.filter_depth_dedup(d[ref], c[ref], cams[ref], [d[s] for s in srcs], [cams[s] for s in srcs],
                                        0.35, used[ref], [used[s] for s in srcs], emit_out=emit[ref])
        np.testing.assert_array_equal(out[3].cpu().numpy(), want["masks"][ref]["emit"])
    host = buf.cpu().numpy()
    inside = np.zeros(host.shape, bool)
    for i in range(2 * n):
        inside[G + i * (HW + G):G + i * (HW + G) + HW] = True
    assert (host[~inside] == 0xAB).all() and (~inside).sum() == (2 * n + 1) * G
    assert set(np.unique(host[inside])) <= {0, 1}
    for v in depths:
        np.testing.assert_array_equal(used[v].cpu().numpy(), want["used"][v])
        np.testing.assert_array_equal(emit[v].cpu().numpy(), want["masks"][v]["emit"].astype(np.uint8))


def test_two_runs_give_identical_bytes():
    import torch
    case = (75, 101, 4, 1)
    sc, _ = _want(case, lambda: dr.scene(*case))
    a, b = _gpu_scan(sc), _gpu_scan(sc)
    assert torch.equal(a["xyz"], b["xyz"]) and torch.equal(a["rgb"], b["rgb"]) and a["counts"] == b["counts"]
    for v in a["masks"]:
        assert torch.equal(a["masks"][v]["emit"], b["masks"][v]["emit"])
        assert torch.equal(a["used"][v], b["used"][v]) and torch.equal(a["avg"][v], b["avg"][v])


def test_null_dedup_arguments_are_the_plain_filter():
    import torch
    from aarmvs import _lib, lib
    _, dev = _one_view((75, 101, 4, 1))
    ref, conf, ref_cam, srcs, src_cams, thr = dev
    want = fusion.filter_depth_core(*dev)
    H, W = ref.shape
    cams = fusion.pack_cameras(ref_cam, src_cams)
    masks = [torch.full((H, W), 7, dtype=torch.uint8, device="cuda") for _ in range(3)]
    avg = torch.full((H, W), -1.0, dtype=torch.float64, device="cuda")
    a = _lib.FusionArgs()
    a.H, a.W, a.nsrc = H, W, len(srcs)
    a.ref_depth, a.confidence = ref.data_ptr(), conf.data_ptr()
    for i, t in enumerate(srcs):
        a.src_depth[i] = t.data_ptr()
    a.cams = cams.ctypes.data
    a.photo_threshold = float(np.float32(thr))
    a.photo_mask, a.geo_mask, a.final_mask = (m.data_ptr() for m in masks)
    a.depth_avg = avg.data_ptr()
    _lib.check(lib().aarmvs_fusion_filter_dedup(ctypes.byref(a), None, torch.cuda.current_stream().cuda_stream),
               "fusion_filter_dedup")
    torch.cuda.synchronize()
    for g, w in zip(masks, want[:3]):
        assert torch.equal(g.bool(), w) and int(g.max()) <= 1
    assert torch.equal(avg, want[3])


# ---------------------------------------------------------------------------------
# the file drivers (a scan written as in tests/test_fusion.py::_write_scan, and its Tanks and
# Temples form as in tests/test_fusion_tnt.py::_write_tnt_scan): 48x64 maps, 3 source views
# ---------------------------------------------------------------------------------
H_SCAN, W_SCAN, NSRC_SCAN = 48, 64, 3


def _cam_text(K, E):
    return ("extrinsic\n" + "\n".join(" ".join(repr(float(q)) for q in row) for row in E)
            + "\n\nintrinsic\n" + "\n".join(" ".join(repr(float(q)) for q in row) for row in K)
            + "\n\n425 2.5\n")


def _write_scan(root, H, W, nsrc, pad, tnt=False):
    """DTU layout: pair.txt, cams/, images/ (pad extra rows top and bottom: the driver's crop),
    depth_est_0/ and confidence_0/ PFMs.  tnt: full-size intrinsics (2 K), images twice the maps'
    size, PFMs with 2 junk rows above and below."""
    from PIL import Image
    depths, cams, conf = syn.fusion_views(H, W, nsrc, seed=11)
    n = nsrc + 1
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

    pair, images, cam_texts, dmaps, confs = [], {}, {}, {}, {}
    for v in range(n):
        K, E = cams[v]
        K = K.copy()
        if tnt:
            K[:2] *= 2
        else:
            K[1, 2] += pad                      # the image has pad more rows above the crop
        cam_texts[v] = _cam_text(K, E)
        (scan / "cams" / "{:0>8}_cam.txt".format(v)).write_text(cam_texts[v])
        img = (rng.random((2 * H, 2 * W, 3) if tnt else (H + 2 * pad, W, 3)) * 255).astype(np.uint8)
        Image.fromarray(img).save(str(scan / "images" / "{:0>8}.jpg".format(v)), format="PNG")
        images[v] = np.array(Image.open(str(scan / "images" / "{:0>8}.jpg".format(v))), np.float32) / 255.0
        dmaps[v] = stored(depths[v])
        confs[v] = stored(np.roll(conf, 7 * v, axis=1) if v else conf)
        fusion.save_pfm(str(out / "depth_est_0" / "{:0>8}.pfm".format(v)), dmaps[v])
        fusion.save_pfm(str(out / "confidence_0" / "{:0>8}.pfm".format(v)), confs[v])
        pair.append((v, [s for s in range(n) if s != v]))
    with open(scan / "pair.txt", "w") as f:
        f.write(f"{n}\n")
        for v, srcs in pair:
            f.write(f"{v}\n{len(srcs)} " + " ".join(f"{s} {9.0 - s:.1f}" for s in srcs) + "\n")
    return scan, out, (pair, images, cam_texts, dmaps, confs)


def _read_ply(path):
    head, body = path.read_bytes().split(b"end_header\n", 1)
    n = int(head.split(b"element vertex ")[1].split(b"\n")[0])
    v = np.frombuffer(body, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                                   ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    assert v.shape[0] == n
    return np.stack([v["x"], v["y"], v["z"]], 1), np.stack([v["red"], v["green"], v["blue"]], 1)


def _check_driver(out, ply, npts, want, plain):
    """The PLY and the mask PNGs of a driver run against a restatement's scan."""
    from PIL import Image
    xyz, rgb = _read_ply(ply)
    assert npts == xyz.shape[0] == want["xyz"].shape[0] > 0
    np.testing.assert_array_equal(xyz, want["xyz"])
    np.testing.assert_array_equal(rgb, want["rgb"])
    names = ("photo", "geo", "final") if plain else ("photo", "geo", "final", "emit")
    assert sorted(os.listdir(str(out / "mask"))) == sorted(
        "{:0>8}_{}.png".format(v, k) for v in want["masks"] for k in names)
    for v, m in want["masks"].items():
        for k in names:
            png = np.array(Image.open(str(out / "mask" / "{:0>8}_{}.png".format(v, k))))
            np.testing.assert_array_equal(png, m[k].astype(np.uint8) * 255, err_msg=f"view {v} {k}")


def test_dtu_driver_with_and_without_dedup(tmp_path):
    pad = 4
    scan, out, (pair, images, cam_texts, dmaps, confs) = _write_scan(tmp_path, H_SCAN, W_SCAN, NSRC_SCAN, pad)
    # what the driver makes of the files (fusion.py:157-171): scale 1, pad rows cropped, K re-centred
    assert fusion.crop_params(images[0].shape[:2], confs[0].shape) == (1.0, pad, pad, 1)
    cams = {}
    for v, txt in cam_texts.items():
        lines = [ln.rstrip() for ln in txt.splitlines()]                    # fusion.py:27-42
        E = np.array(" ".join(lines[1:5]).split(), dtype=np.float32).reshape((4, 4))
        K = np.array(" ".join(lines[7:10]).split(), dtype=np.float32).reshape((3, 3))
        K[:2, :] *= 1.0
        K[1, 2] -= pad
        cams[v] = (K, E)
    cropped = {v: im[pad:-pad] for v, im in images.items()}
    with np.errstate(all="ignore"):
        plain = dr.fuse_views(pair, dmaps, confs, cams, cropped, 0.35, dedup=False)
        want = dr.fuse_views(pair, dmaps, confs, cams, cropped, 0.35, dedup=True)
        masks, xyz, rgb = fo.filter_depth_scan(pair, images, cam_texts, dmaps, confs, 0.35)
    # the restatement's plain scan is the oracle's scan: the helper above reads the files right
    np.testing.assert_array_equal(plain["xyz"], xyz)
    np.testing.assert_array_equal(plain["rgb"], rgb)
    # without the flag: the cloud and the files it has always written
    ply = tmp_path / "plain.ply"
    npts = fusion.filter_depth(str(scan), str(out), str(ply), 0.35)
    _check_driver(out, ply, npts, plain, plain=True)
    # fuse_views(dedup=False) is that cloud too
    got = fusion.fuse_views(pair, _cuda(dmaps), _cuda(confs), cams, _cuda(cropped), 0.35)
    np.testing.assert_array_equal(got["xyz"].cpu().numpy(), xyz)
    np.testing.assert_array_equal(got["rgb"].cpu().numpy(), rgb)
    assert "used" not in got and "emit" not in got["masks"][0]
    # with it
    ply = tmp_path / "dedup.ply"
    npts = fusion.filter_depth(str(scan), str(out), str(ply), 0.35, dedup=True)
    assert npts < plain["xyz"].shape[0]
    _check_driver(out, ply, npts, want, plain=False)


def test_tnt_driver_with_and_without_dedup(tmp_path):
    scan, out, (pair, images, cam_texts, dmaps, confs) = _write_scan(tmp_path, H_SCAN, W_SCAN, NSRC_SCAN, 0, tnt=True)
    cams = {v: tr.read_camera_parameters(txt) for v, txt in cam_texts.items()}
    halved = {v: tr.pyr_down(im) for v, im in images.items()}
    crop = lambda maps: {v: m[2:-2] for v, m in maps.items()}  # noqa: E731
    with np.errstate(all="ignore"):
        plain = dr.fuse_views(pair, crop(dmaps), crop(confs), cams, halved, 0.3, dedup=False, core=tr.filter_depth_core)
        want = dr.fuse_views(pair, crop(dmaps), crop(confs), cams, halved, 0.3, dedup=True, core=tr.filter_depth_core)
        masks, xyz, rgb = tr.filter_depth_scan(pair, images, cam_texts, dmaps, confs, 0.3)
    np.testing.assert_array_equal(plain["xyz"], xyz)
    np.testing.assert_array_equal(plain["rgb"], rgb)
    ply = tmp_path / "plain.ply"
    npts = fusion.filter_depth_tnt(str(scan), str(out), str(ply))
    _check_driver(out, ply, npts, plain, plain=True)
    # through the command line
    (tmp_path / "list.txt").write_text("scan1\n")
    fusion.main(["--test_dataset", "tnt", "--testpath", str(tmp_path), "--testlist", str(tmp_path / "list.txt"),
                 "--outdir", str(tmp_path / "out"), "--dedup"])
    ply = tmp_path / "out" / "scan1.ply"
    npts = _read_ply(ply)[0].shape[0]
    assert npts < plain["xyz"].shape[0]
    _check_driver(out, ply, npts, want, plain=False)
