"""The point-cloud evaluation's C ABI and Python surface without a GPU: the symbols, the struct,
the rejections that happen before any device work, the profiler list and the PLY reader."""
import ctypes
import inspect

import numpy as np
import pytest

INVALID = 1
NQ, M = 100, 200
# never dereferenced: validation fails first.  query 1200 B, target 2400 B, keys 1600 B, ids 800 B,
# dist / index 400 B each
QUERY, TARGET, KEYS, IDS, DIST, INDEX = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
SYMBOLS = ("aarmvs_cloud_keys", "aarmvs_cloud_nn", "aarmvs_cloud_stats_scratch_bytes", "aarmvs_cloud_stats",
           "aarmvs_cloud_voxel_workspace_bytes", "aarmvs_cloud_voxel_centroids")


def _L():
    from aarmvs import lib
    return lib()


def _err():
    return _L().aarmvs_last_error().decode()


def _args():
    from aarmvs import _lib
    a = _lib.CloudNnArgs()
    a.query, a.target, a.target_keys, a.target_ids = QUERY, TARGET, KEYS, IDS
    a.nq, a.m = NQ, M
    a.origin[0], a.origin[1], a.origin[2] = 0.0, -1.0, 2.0
    a.cell, a.max_dist = 0.5, 2.0
    a.dist_out, a.index_out = DIST, INDEX
    return a


def _nn(a):
    return _L().aarmvs_cloud_nn(None if a is None else ctypes.byref(a), None)


def test_symbols_struct_and_constants():
    from aarmvs import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert [f[0] for f in _lib.CloudNnArgs._fields_] == [
        "query", "target", "target_keys", "target_ids", "nq", "m", "origin", "cell", "max_dist", "dist_out",
        "index_out"]
    # 4 pointers, 2 long longs, 4 doubles, a float (+ padding), 2 pointers
    assert ctypes.sizeof(_lib.CloudNnArgs) == 32 + 16 + 32 + 8 + 16 == 104
    A = _lib.CloudNnArgs
    assert (A.nq.offset, A.origin.offset, A.cell.offset, A.max_dist.offset, A.dist_out.offset, A.index_out.offset) == (
        32, 48, 72, 80, 88, 96)
    assert (_lib.CLOUD_MAX_RINGS, _lib.CLOUD_AXIS_BITS, _lib.MAX_THRESHOLDS) == (32, 21, 8)


def test_the_header_documents_the_definition():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "aarmvs.h")).read()
    for word in ("AARMVS_CLOUD_MAX_RINGS 32", "aarmvs_cloud_nn_args", "Stopping rule", "1 - 2^-20", "INT64_MAX",
                 "(i_z << 42) | (i_y << 21) | i_x") + SYMBOLS:
        assert word in text, word


def test_the_profiler_list_did_not_change():
    """The new launches are timed under the existing "fusion_points" id."""
    L = _L()
    names = [L.aarmvs_profile_kernel_name(i).decode() for i in range(L.aarmvs_profile_kernel_count())]
    assert len(names) == 58 and names[-1] == "refine" and "fusion_points" in names


def test_nn_accepts_nothing_to_do():
    a = _args()
    a.nq = 0
    a.query = a.dist_out = a.index_out = None
    assert _nn(a) == 0


def test_nn_rejects_null_args_and_null_pointers():
    assert _nn(None) == INVALID and _err() == "cloud_nn: null args"
    for field in ("query", "target", "target_keys", "dist_out"):
        a = _args()
        setattr(a, field, None)
        assert _nn(a) == INVALID and _err() == "cloud_nn: null pointer argument", field


@pytest.mark.parametrize("field,value", [("nq", -1), ("m", -1), ("nq", 1 << 31), ("m", 1 << 31), ("m", 1 << 40)])
def test_nn_rejects_bad_counts(field, value):
    a = _args()
    setattr(a, field, value)
    assert _nn(a) == INVALID and _err() == "cloud_nn: need 0 <= nq, m < 2^31"


@pytest.mark.parametrize("cell", [0.0, -1.0, float("nan"), float("inf")])
def test_nn_rejects_a_bad_cell(cell):
    a = _args()
    a.cell = cell
    assert _nn(a) == INVALID and _err() == "cloud_nn: cell must be finite and > 0"


@pytest.mark.parametrize("md", [-0.5, float("nan"), float("inf"), -float("inf")])
def test_nn_rejects_a_bad_max_dist(md):
    a = _args()
    a.max_dist = md
    assert _nn(a) == INVALID and _err() == "cloud_nn: max_dist must be finite and >= 0"


def test_nn_rejects_a_non_finite_origin():
    a = _args()
    a.origin[1] = float("nan")
    assert _nn(a) == INVALID and _err() == "cloud_nn: origin must be finite"


def test_nn_rejects_too_many_rings():
    a = _args()
    a.cell, a.max_dist = 1.0, 32.5
    assert _nn(a) == INVALID and _err() == "cloud_nn: max_dist / cell exceeds AARMVS_CLOUD_MAX_RINGS"
    a.cell, a.max_dist = 0.0625, 2.0   # exactly 32 rings pass (no query: nothing is launched)
    a.nq = 0
    assert _nn(a) == 0


@pytest.mark.parametrize("field,where", [
    ("dist_out", QUERY), ("dist_out", QUERY + 12 * NQ - 4), ("dist_out", QUERY - 4 * NQ + 4), ("dist_out", TARGET + 8),
    ("dist_out", KEYS + 8 * M - 1), ("dist_out", IDS), ("index_out", QUERY + 100), ("index_out", TARGET),
    ("index_out", KEYS), ("index_out", IDS + 4 * M - 4)])
def test_nn_rejects_outputs_that_overlap_inputs(field, where):
    a = _args()
    setattr(a, field, where)
    assert _nn(a) == INVALID and _err() == f"cloud_nn: {field} must not alias an input"


def test_nn_rejects_outputs_that_overlap_each_other():
    a = _args()
    a.index_out = DIST + 4 * NQ - 4
    assert _nn(a) == INVALID and _err() == "cloud_nn: dist_out and index_out must not alias"


def test_keys_rejections():
    L = _L()
    o = (ctypes.c_double * 3)(0, 0, 0)
    assert L.aarmvs_cloud_keys(QUERY, -1, o, 1.0, KEYS, None) == INVALID and "n < 2^31" in _err()
    assert L.aarmvs_cloud_keys(QUERY, 1 << 31, o, 1.0, KEYS, None) == INVALID and "n < 2^31" in _err()
    assert L.aarmvs_cloud_keys(None, 10, o, 1.0, KEYS, None) == INVALID and "null pointer" in _err()
    assert L.aarmvs_cloud_keys(QUERY, 10, None, 1.0, KEYS, None) == INVALID and "null pointer" in _err()
    assert L.aarmvs_cloud_keys(QUERY, 10, o, 1.0, None, None) == INVALID and "null pointer" in _err()
    for cell in (0.0, -2.0, float("nan"), float("inf")):
        assert L.aarmvs_cloud_keys(QUERY, 10, o, cell, KEYS, None) == INVALID and "cell" in _err()
    bad = (ctypes.c_double * 3)(0, float("inf"), 0)
    assert L.aarmvs_cloud_keys(QUERY, 10, bad, 1.0, KEYS, None) == INVALID and "origin" in _err()
    assert L.aarmvs_cloud_keys(QUERY, 10, o, 1.0, QUERY + 64, None) == INVALID and "alias" in _err()
    assert L.aarmvs_cloud_keys(None, 0, o, 1.0, None, None) == 0


def test_stats_rejections_and_scratch_size():
    L = _L()
    thr = (ctypes.c_float * 9)()
    assert L.aarmvs_cloud_stats(DIST, -1, thr, 1, INDEX, KEYS, None) == INVALID and "n < 2^31" in _err()
    assert L.aarmvs_cloud_stats(DIST, 10, thr, 9, INDEX, KEYS, None) == INVALID
    assert _err() == "cloud_stats: at most 8 thresholds"
    assert L.aarmvs_cloud_stats(DIST, 10, thr, -1, INDEX, KEYS, None) == INVALID
    for args in ((None, 10, thr, 1, INDEX, KEYS), (DIST, 10, None, 1, INDEX, KEYS), (DIST, 10, thr, 1, None, KEYS),
                 (DIST, 10, thr, 1, INDEX, None)):
        assert L.aarmvs_cloud_stats(*args, None) == INVALID and _err() == "cloud_stats: null pointer argument"
    # out [3 + k] doubles and the scratch must not overlap dist (40 B here), nor each other
    for args in ((DIST, 10, thr, 1, DIST + 36, KEYS), (DIST, 10, thr, 1, DIST - 31, KEYS),
                 (DIST, 10, thr, 1, INDEX, DIST + 8), (DIST, 10, thr, 1, INDEX, DIST - 255)):
        assert L.aarmvs_cloud_stats(*args, None) == INVALID and _err() == "cloud_stats: out and scratch must not alias dist"
    assert L.aarmvs_cloud_stats(DIST, 10, thr, 1, KEYS + 248, KEYS, None) == INVALID
    assert _err() == "cloud_stats: out must not alias scratch"
    # 11 doubles per block of 4096 values, rounded up to 256 bytes
    assert L.aarmvs_cloud_stats_scratch_bytes(1) == 256 == L.aarmvs_cloud_stats_scratch_bytes(0)
    assert L.aarmvs_cloud_stats_scratch_bytes(4096 * 100 + 1) == (101 * 88 + 255) // 256 * 256
    assert L.aarmvs_cloud_stats_scratch_bytes(-1) == 0 == L.aarmvs_cloud_stats_scratch_bytes(1 << 31)


def test_voxel_centroids_rejections_and_workspace_size():
    L = _L()
    call = L.aarmvs_cloud_voxel_centroids
    assert call(QUERY, KEYS, -1, TARGET, 10, DIST, INDEX, None) == INVALID and "n < 2^31" in _err()
    assert call(QUERY, KEYS, 10, TARGET, -1, DIST, INDEX, None) == INVALID and "negative capacity" in _err()
    for args in ((None, KEYS, 10, TARGET, 10, DIST, INDEX), (QUERY, None, 10, TARGET, 10, DIST, INDEX),
                 (QUERY, KEYS, 10, TARGET, 10, None, INDEX), (QUERY, KEYS, 10, TARGET, 10, DIST, None)):
        assert call(*args, None) == INVALID and _err() == "cloud_voxel_centroids: null pointer argument"
    assert call(QUERY, KEYS, 10, None, 10, DIST, INDEX, None) == INVALID and "null out_xyz" in _err()
    assert call(QUERY, KEYS, 10, QUERY + 60, 10, DIST, INDEX, None) == INVALID and "alias" in _err()
    assert call(QUERY, KEYS, 10, KEYS + 8, 10, DIST, INDEX, None) == INVALID and "alias" in _err()
    assert L.aarmvs_cloud_voxel_workspace_bytes(1) == 256
    assert L.aarmvs_cloud_voxel_workspace_bytes(1024 * 1000 + 1) == (1001 * 4 + 255) // 256 * 256
    assert L.aarmvs_cloud_voxel_workspace_bytes(-5) == 0


def test_python_surface():
    import torch
    from aarmvs import AarmvsError, cloud_eval, synthetic
    assert list(inspect.signature(cloud_eval.nn_distance).parameters) == ["query", "target", "max_dist", "cell"]
    assert inspect.signature(cloud_eval.nn_distance).parameters["cell"].default is None
    assert list(inspect.signature(cloud_eval.voxel_downsample).parameters) == ["xyz", "voxel"]
    ev = inspect.signature(cloud_eval.evaluate).parameters
    assert list(ev) == ["recon", "gt", "max_dist", "thresholds", "voxel"]
    assert ev["thresholds"].default == () and ev["voxel"].default is None
    assert list(inspect.signature(synthetic.fusion_ground_truth).parameters) == ["H", "W", "nsrc"]
    # CPU tensors are refused: there is no CPU fallback
    x = torch.zeros(4, 3)
    with pytest.raises(AarmvsError):
        cloud_eval.nn_distance(x, x, 1.0)
    with pytest.raises(AarmvsError):
        cloud_eval.voxel_downsample(x, 1.0)
    with pytest.raises(AarmvsError):
        cloud_eval.evaluate(x, x, 1.0)
    with pytest.raises(ValueError, match="tau"):
        cloud_eval.evaluate(x, x, 1.0, thresholds=(2.0,))
    args = cloud_eval.build_parser().parse_args(["--recon", "a.ply", "--gt", "b.ply", "--max_dist", "20", "--tau",
                                                 "1", "2", "5"])
    assert (args.recon, args.gt, args.max_dist, args.tau, args.voxel, args.json) == ("a.ply", "b.ply", 20.0,
                                                                                     [1.0, 2.0, 5.0], None, None)


def _cloud(n=9):
    rng = np.random.default_rng(0)
    return (rng.standard_normal((n, 3)).astype(np.float32), rng.integers(0, 256, (n, 3)).astype(np.uint8),
            rng.standard_normal((n, 3)).astype(np.float32))


@pytest.mark.parametrize("colours", [True, False])
@pytest.mark.parametrize("normals", [True, False])
def test_read_ply_round_trips_write_ply(tmp_path, colours, normals):
    from aarmvs import cloud_eval, fusion
    xyz, rgb, nrm = _cloud()
    xyz[3, 1] = np.float32("nan")      # bit patterns survive, too
    rgb, nrm = (rgb if colours else None), (nrm if normals else None)
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    fusion.write_ply(a, xyz, rgb, nrm)
    got = cloud_eval.read_ply(a)
    assert sorted(got) == ["normals", "rgb", "xyz"]
    assert got["xyz"].dtype == np.float32 and got["xyz"].tobytes() == xyz.tobytes()
    assert (got["rgb"] is None) == (not colours) and (got["normals"] is None) == (not normals)
    if colours:
        assert got["rgb"].dtype == np.uint8
        np.testing.assert_array_equal(got["rgb"], rgb)
    if normals:
        np.testing.assert_array_equal(got["normals"], nrm)
    fusion.write_ply(b, **got)
    assert open(a, "rb").read() == open(b, "rb").read()


def test_read_ply_reads_plain_xyz_in_ascii_and_binary(tmp_path):
    from aarmvs import cloud_eval
    xyz = np.float32([[0.5, -1.25, 3.0], [1e-3, 2.5e4, -7.0], [1, 2, 3]])
    head = "ply\nformat {} 1.0\ncomment made by hand\nelement vertex 3\nproperty float x\nproperty float y\n" \
           "property float z\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n"
    p = tmp_path / "a.ply"
    p.write_text(head.format("ascii") + "".join("{!r} {!r} {!r}\n".format(*map(float, r)) for r in xyz))
    got = cloud_eval.read_ply(str(p))
    np.testing.assert_array_equal(got["xyz"], xyz)
    assert got["rgb"] is None and got["normals"] is None
    p.write_bytes(head.format("binary_little_endian").encode() + xyz.astype("<f4").tobytes())
    np.testing.assert_array_equal(cloud_eval.read_ply(str(p))["xyz"], xyz)
    # an empty cloud, and what is not a PLY
    p.write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\n"
                  b"property float z\nend_header\n")
    assert cloud_eval.read_ply(str(p))["xyz"].shape == (0, 3)
    p.write_bytes(b"not a ply\n")
    with pytest.raises(ValueError):
        cloud_eval.read_ply(str(p))
    p.write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\n"
                  b"property float z\nend_header\n")
    with pytest.raises(ValueError):
        cloud_eval.read_ply(str(p))


def test_read_ply_header_and_short_files(tmp_path):
    from aarmvs import cloud_eval
    p = tmp_path / "a.ply"
    head = "ply\nformat {} 1.0\ncomment no end_header here yet\nelement vertex 2\nproperty float x\n" \
           "property float y\nproperty float z\nend_header\n"
    xyz = np.float32([[1, 2, 3], [4, 5, 6]])
    p.write_bytes(head.format("binary_little_endian").encode() + xyz.tobytes())
    np.testing.assert_array_equal(cloud_eval.read_ply(str(p))["xyz"], xyz)
    p.write_text(head.format("ascii") + "1 2 3\n4 5 6\n")
    np.testing.assert_array_equal(cloud_eval.read_ply(str(p))["xyz"], xyz)
    for body in ("1 2 3\n", "1 2 3\n4 5\n", ""):
        p.write_text(head.format("ascii") + body)
        with pytest.raises(ValueError, match="shorter than its header says"):
            cloud_eval.read_ply(str(p))
    p.write_bytes(head.format("binary_little_endian").encode() + xyz.tobytes()[:-1])
    with pytest.raises(ValueError, match="shorter than its header says"):
        cloud_eval.read_ply(str(p))
    p.write_bytes(b"ply\nformat ascii 1.0\ncomment end_header\nelement vertex 0\n")    # no end_header line
    with pytest.raises(ValueError, match="not a PLY"):
        cloud_eval.read_ply(str(p))
