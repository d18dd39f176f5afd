"""The per-point normals' C ABI and Python surface without a GPU: the symbols, the structs, the
rejections that happen before any device work, the command line and the PLY writer."""
import ctypes
import inspect

import numpy as np
import pytest

INVALID = 1
H, W = 8, 8
# never dereferenced: validation fails first.  depth 512 B, valid 64 B, normal 768 B, has_normal 64 B
DEPTH, VALID, NORMAL, HAS = 0x10000, 0x20000, 0x30000, 0x40000


def _err():
    from aarmvs import lib
    return lib().aarmvs_last_error().decode()


def _args(cams):
    from aarmvs import _lib
    a = _lib.FusionNormalsArgs()
    a.H, a.W = H, W
    a.depth, a.valid = DEPTH, VALID
    a.cams = ctypes.addressof(cams)
    a.radius, a.min_count, a.max_rel_jump = 2, 3, 0.01
    a.normal, a.has_normal = NORMAL, HAS
    return a


def _cams():
    return (ctypes.c_float * 25)()


def _call(a):
    from aarmvs import lib
    return lib().aarmvs_fusion_normals(None if a is None else ctypes.byref(a), None)


def _points_args(cams):
    from aarmvs import _lib
    p = _lib.FusionPointsArgs()
    p.H, p.W = H, W
    p.mask, p.depth, p.color = VALID, DEPTH, None
    p.cams = ctypes.addressof(cams)
    p.xyz, p.rgb, p.capacity = 0x50000, None, 64
    p.count, p.workspace = 0x60000, 0x70000
    return p


def test_symbols_and_struct():
    from aarmvs import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("aarmvs_fusion_normals", "aarmvs_fusion_points_normals"):
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert [f[0] for f in _lib.FusionNormalsArgs._fields_] == [
        "H", "W", "depth", "valid", "cams", "radius", "min_count", "max_rel_jump", "normal", "has_normal"]
    p = ctypes.sizeof(ctypes.c_void_p)
    # 2 ints, 3 pointers, 2 ints and a float (+ padding), 2 pointers
    assert ctypes.sizeof(_lib.FusionNormalsArgs) == 8 + 3 * p + 16 + 2 * p == 64
    assert _lib.FusionNormalsArgs.has_normal.offset == 56
    assert _lib.MAX_NORMAL_RADIUS == 3 and _lib.FUSION_NORMAL_CAM_FLOATS == 25


def test_the_other_fusion_structs_did_not_change():
    from aarmvs import _lib
    assert [f[0] for f in _lib.FusionPointsArgs._fields_] == [
        "H", "W", "mask", "depth", "color", "cams", "xyz", "rgb", "capacity", "count", "workspace"]
    # 2 ints, 6 pointers, a long long, 2 pointers
    assert ctypes.sizeof(_lib.FusionPointsArgs) == 8 + 6 * 8 + 8 + 2 * 8 == 80
    assert _lib.FusionPointsArgs.workspace.offset == 72
    assert [f[0] for f in _lib.FusionArgs._fields_] == [
        "H", "W", "nsrc", "ref_depth", "confidence", "src_depth", "cams", "photo_threshold", "photo_mask",
        "geo_mask", "final_mask", "depth_avg"]
    assert ctypes.sizeof(_lib.FusionArgs) == 160 and _lib.FusionArgs.depth_avg.offset == 152


def test_the_profiler_list_did_not_change():
    """The new launches are timed under the existing "fusion_points" id."""
    from aarmvs import lib
    L = lib()
    names = [L.aarmvs_profile_kernel_name(i).decode() for i in range(L.aarmvs_profile_kernel_count())]
    assert len(names) == 58 and names[-1] == "refine" and "fusion_points" in names
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("field", ["depth", "valid", "cams", "normal"])
def test_rejects_a_null_pointer(field):
    a = _args(_cams())
    setattr(a, field, None)
    assert _call(a) == INVALID
    assert _err() == "fusion_normals: null pointer argument"


def test_rejects_null_args():
    assert _call(None) == INVALID and _err() == "fusion_normals: null args"


@pytest.mark.parametrize("hw", [(0, 8), (8, 0), (-1, 8), (1 << 16, 1 << 15), (46341, 46341)])
def test_rejects_bad_sizes(hw):
    a = _args(_cams())
    a.H, a.W = hw
    assert _call(a) == INVALID
    assert _err() == "fusion_normals: need H, W >= 1 and H * W < 2^31"


@pytest.mark.parametrize("radius", [0, -1, 4, 100])
def test_rejects_a_radius_outside_1_to_3(radius):
    a = _args(_cams())
    a.radius = radius
    assert _call(a) == INVALID and "radius" in _err()


@pytest.mark.parametrize("radius,min_count", [(1, 2), (1, 10), (2, 0), (2, 26), (3, 50), (3, -3)])
def test_rejects_a_min_count_outside_3_to_the_window(radius, min_count):
    a = _args(_cams())
    a.radius, a.min_count = radius, min_count
    assert _call(a) == INVALID and "min_count" in _err()


@pytest.mark.parametrize("jump", [-0.01, float("nan"), float("inf"), -float("inf")])
def test_rejects_a_negative_or_non_finite_max_rel_jump(jump):
    a = _args(_cams())
    a.max_rel_jump = jump
    assert _call(a) == INVALID and "max_rel_jump" in _err()


@pytest.mark.parametrize("field,where", [
    ("normal", DEPTH), ("normal", DEPTH + 8 * H * W - 4), ("normal", DEPTH - 12 * H * W + 4), ("normal", VALID),
    ("has_normal", DEPTH + 16), ("has_normal", VALID), ("has_normal", NORMAL + 100)])
def test_rejects_outputs_that_alias_the_inputs(field, where):
    a = _args(_cams())
    setattr(a, field, where)
    assert _call(a) == INVALID
    assert "fusion_normals" in _err() and "alias" in _err() and field in _err()


def test_points_normals_rejections():
    from aarmvs import lib
    L = lib()
    cams = _cams()
    p = _points_args(cams)
    # exactly one of normal_map and nxyz
    assert L.aarmvs_fusion_points_normals(ctypes.byref(p), NORMAL, None, None) == INVALID
    assert "fusion_points_normals" in _err() and "normal_map" in _err() and "nxyz" in _err()
    assert L.aarmvs_fusion_points_normals(ctypes.byref(p), None, 0x80000, None) == INVALID
    assert "fusion_points_normals" in _err()
    # everything aarmvs_fusion_points rejects, with its messages, with and without the new arguments
    for extra in ((NORMAL, 0x80000), (None, None)):
        assert L.aarmvs_fusion_points_normals(None, *extra, None) == INVALID and _err() == "fusion_points: null args"
        p = _points_args(cams)
        p.H = 0
        assert L.aarmvs_fusion_points_normals(ctypes.byref(p), *extra, None) == INVALID
        assert _err() == "fusion_points: need H, W >= 1 and H * W < 2^31"
        for field in ("mask", "depth", "cams", "count", "workspace"):
            p = _points_args(cams)
            setattr(p, field, None)
            assert L.aarmvs_fusion_points_normals(ctypes.byref(p), *extra, None) == INVALID
            assert _err() == "fusion_points: null pointer argument"
        p = _points_args(cams)
        p.capacity = -1
        assert L.aarmvs_fusion_points_normals(ctypes.byref(p), *extra, None) == INVALID
        assert _err() == "fusion_points: negative capacity"
        p = _points_args(cams)
        p.xyz = None
        assert L.aarmvs_fusion_points_normals(ctypes.byref(p), *extra, None) == INVALID
        assert _err() == "fusion_points: null xyz with capacity > 0"
        p = _points_args(cams)
        p.rgb = 0x90000
        assert L.aarmvs_fusion_points_normals(ctypes.byref(p), *extra, None) == INVALID
        assert _err() == "fusion_points: color and rgb must both be set or both be null"


def test_python_surface_and_defaults():
    import torch
    from aarmvs import AarmvsError, fusion
    sig = inspect.signature(fusion.estimate_normals).parameters
    assert list(sig) == ["depth_avg", "valid", "ref_cam", "radius", "max_rel_jump", "min_count"]
    assert (sig["radius"].default, sig["max_rel_jump"].default, sig["min_count"].default) == (2, 0.01, 3)
    assert list(inspect.signature(fusion.fuse_points_normals_gpu).parameters) == [
        "depth_avg", "final_mask", "ref_cam", "ref_img", "normal_map"]
    assert inspect.signature(fusion.fuse_views).parameters["normals"].default is False
    for fn in (fusion.filter_depth, fusion.filter_depth_tnt):
        assert inspect.signature(fn).parameters["normals"].default is None
    ply = inspect.signature(fusion.write_ply).parameters
    assert list(ply) == ["filename", "xyz", "rgb", "normals"] and ply["normals"].default is None
    # the camera packing: K, then the float32 inverse of E
    K = np.array([[290, 0, 32], [0, 292, 24], [0, 0, 1]], np.float64)
    E = np.eye(4)
    E[:3, 3] = (1, 2, 3)
    packed = fusion.pack_normal_cameras((K, E))
    assert packed.dtype == np.float32 and packed.shape == (25,)
    np.testing.assert_array_equal(packed[:9], K.astype(np.float32).ravel())
    np.testing.assert_array_equal(packed[9:], np.linalg.inv(E.astype(np.float32)).ravel())
    # the normals argument
    assert fusion.normal_params(False) is None and fusion.normal_params(None) is None
    assert fusion.normal_params(True) == dict(radius=2, max_rel_jump=0.01, min_count=3)
    assert fusion.normal_params(dict(radius=3)) == dict(radius=3, max_rel_jump=0.01, min_count=3)
    with pytest.raises(AarmvsError):
        fusion.normal_params(dict(window=3))
    # CPU tensors are refused: there is no CPU fallback
    cam = (np.eye(3), np.eye(4))
    with pytest.raises(AarmvsError):
        fusion.estimate_normals(torch.zeros(4, 4, dtype=torch.float64), torch.ones(4, 4, dtype=torch.bool), cam)
    with pytest.raises(AarmvsError):
        fusion.fuse_points_normals_gpu(torch.zeros(4, 4, dtype=torch.float64), torch.ones(4, 4, dtype=torch.bool),
                                       cam, None, torch.zeros(4, 4, 3))
    with pytest.raises(AarmvsError, match="require_normal"):
        fusion.fuse_views([], {}, {}, {}, require_normal=True)


def test_cli_hands_the_normals_to_the_drivers_only_when_asked(tmp_path):
    from aarmvs import fusion
    (tmp_path / "list.txt").write_text("scan1\n")
    calls = []
    saved = fusion.filter_depth_tnt, fusion.filter_depth
    fusion.filter_depth_tnt = lambda *a, **k: calls.append(("tnt", a, k))
    fusion.filter_depth = lambda *a, **k: calls.append(("dtu", a, k))
    base = ["--testpath", "/data", "--testlist", str(tmp_path / "list.txt"), "--outdir", "/out"]
    try:
        fusion.main(["--test_dataset", "dtu"] + base)
        fusion.main(["--test_dataset", "dtu", "--normal_radius", "3"] + base)      # without --normals: nothing
        fusion.main(["--test_dataset", "dtu", "--normals"] + base)
        fusion.main(["--test_dataset", "tnt", "--normals", "--normal_radius", "3", "--normal_max_rel_jump", "0.02",
                     "--normal_min_count", "6", "--require_normal", "--dedup"] + base)
    finally:
        fusion.filter_depth_tnt, fusion.filter_depth = saved
    dtu = ("/data/scan1", "/out/scan1", "/out/mvsnet_001_l3.ply", 0.35, "cuda")
    tnt = ("/data/scan1", "/out/scan1", "/out/scan1.ply", 0.3, "cuda")
    assert calls == [
        ("dtu", dtu, {}), ("dtu", dtu, {}),
        ("dtu", dtu, {"normals": dict(radius=2, max_rel_jump=0.01, min_count=3)}),
        ("tnt", tnt, {"dedup": True, "normals": dict(radius=3, max_rel_jump=0.02, min_count=6),
                      "require_normal": True})]
    args = fusion.parse_args(["--test_dataset", "dtu"] + base)
    assert (args.normals, args.normal_radius, args.normal_max_rel_jump, args.normal_min_count,
            args.require_normal) == (False, 2, 0.01, 3, False)
    with pytest.raises(SystemExit):
        fusion.parse_args(["--test_dataset", "dtu", "--normal_radius", "4"] + base)
    with pytest.raises(SystemExit):
        fusion.parse_args(["--test_dataset", "dtu", "--require_normal"] + base)


def _cloud(n=5):
    rng = np.random.default_rng(0)
    xyz = rng.standard_normal((n, 3)).astype(np.float32)
    nrm = rng.standard_normal((n, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    return xyz, rgb, nrm


def test_write_ply_round_trips_a_cloud_with_normals(tmp_path):
    from aarmvs import fusion
    xyz, rgb, nrm = _cloud()
    path = tmp_path / "n.ply"
    fusion.write_ply(str(path), xyz, rgb, nrm)
    head, body = path.read_bytes().split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 5"]
    props = [ln.split()[1:] for ln in lines[3:]]
    assert props == [["float", n] for n in ("x", "y", "z", "nx", "ny", "nz")] + \
        [["uchar", n] for n in ("red", "green", "blue")]
    dtype = [(name, "<f4" if kind == "float" else "u1") for kind, name in props]
    v = np.frombuffer(body, dtype=dtype)
    assert v.shape == (5,) and v.dtype.itemsize == 27
    np.testing.assert_array_equal(np.stack([v["x"], v["y"], v["z"]], 1), xyz)
    np.testing.assert_array_equal(np.stack([v["nx"], v["ny"], v["nz"]], 1), nrm)
    np.testing.assert_array_equal(np.stack([v["red"], v["green"], v["blue"]], 1), rgb)
    # normals without colours
    fusion.write_ply(str(path), xyz, None, nrm)
    head, body = path.read_bytes().split(b"end_header\n", 1)
    assert b"red" not in head and len(body) == 5 * 24
    with pytest.raises(ValueError):
        fusion.write_ply(str(path), xyz, rgb, nrm[:3])


@pytest.mark.parametrize("colours", [True, False])
def test_write_ply_without_normals_writes_the_bytes_it_always_wrote(tmp_path, colours):
    """The writer before the normals, restated: header and vertex layout."""
    from aarmvs import fusion
    xyz, rgb, _ = _cloud(7)
    rgb = rgb if colours else None
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")]
                                                          if colours else [])
    v = np.empty(7, dtype=fields)
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if colours:
        v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    header = "ply\nformat binary_little_endian 1.0\nelement vertex 7\n" + \
        "property float x\nproperty float y\nproperty float z\n" + \
        ("property uchar red\nproperty uchar green\nproperty uchar blue\n" if colours else "") + "end_header\n"
    want = header.encode("ascii") + v.tobytes()
    fusion.write_ply(str(tmp_path / "a.ply"), xyz, rgb)
    fusion.write_ply(str(tmp_path / "b.ply"), xyz, rgb, normals=None)
    assert (tmp_path / "a.ply").read_bytes() == want == (tmp_path / "b.ply").read_bytes()
