"""The DTU protocol's C ABI and Python surface without a GPU: the symbols, the struct, the rejections
that happen before any device work, the profiler list and the Python argument errors."""
import ctypes
import inspect

import pytest

INVALID = 1
N = 100
# never dereferenced: validation fails first.  xyz 1200 B, keys 800 B, rank 400 B, the states 100 B
# each, remaining 16 B, scratch 256 B, a 7x5x3 mask 105 B, flags 100 B
XYZ, KEYS, RANK, S0, S1, REM, SCR, MASK, FLAGS = (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000,
                                                  0x80000, 0x90000)
SYMBOLS = ("aarmvs_cloud_thin_scratch_bytes", "aarmvs_cloud_thin", "aarmvs_cloud_regions")


def _L():
    from aarmvs import lib
    return lib()


def _err():
    return _L().aarmvs_last_error().decode()


def _args():
    from aarmvs import _lib
    a = _lib.CloudThinArgs()
    a.xyz, a.keys, a.rank, a.n = XYZ, KEYS, RANK, N
    a.origin[0], a.origin[1], a.origin[2] = 0.0, -1.0, 2.0
    a.cell, a.r = 0.5, 0.5
    a.init, a.which = 1, 0
    a.state[0], a.state[1] = S0, S1
    a.remaining, a.scratch = REM, SCR
    return a


def _thin(a, rounds=8):
    return _L().aarmvs_cloud_thin(None if a is None else ctypes.byref(a), rounds, None)


def test_symbols_struct_and_header():
    import os
    from aarmvs import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    A = _lib.CloudThinArgs
    assert [f[0] for f in A._fields_] == ["xyz", "keys", "rank", "n", "origin", "cell", "r", "init", "which", "state",
                                          "remaining", "scratch"]
    # 3 pointers, a long long, 4 doubles, a float and 2 ints (+ padding), 2 + 2 pointers
    assert ctypes.sizeof(A) == 24 + 8 + 32 + 16 + 16 + 16 == 112
    assert (A.n.offset, A.origin.offset, A.cell.offset, A.r.offset, A.init.offset, A.which.offset, A.state.offset,
            A.remaining.offset, A.scratch.offset) == (24, 32, 56, 64, 68, 72, 80, 96, 104)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "aarmvs.h")).read()
    for word in ("aarmvs_cloud_thin_args", "Round rule", "state[(which + rounds) & 1]", "round-half-to-even",
                 "BB[1][a] + 2 patch", "r (1 + 2^-40)") + SYMBOLS:
        assert word in text, word


def test_the_profiler_list_is_still_58_entries():
    L = _L()
    names = [L.aarmvs_profile_kernel_name(i).decode() for i in range(L.aarmvs_profile_kernel_count())]
    assert len(names) == 58 and names[-1] == "refine" and "fusion_points" in names


def test_thin_scratch_size():
    L = _L()
    # two ints per block of 256 points, rounded up to 256 bytes
    assert L.aarmvs_cloud_thin_scratch_bytes(0) == 256 == L.aarmvs_cloud_thin_scratch_bytes(256 * 32)
    assert L.aarmvs_cloud_thin_scratch_bytes(256 * 32 + 1) == 512
    assert L.aarmvs_cloud_thin_scratch_bytes(256 * 1000 + 1) == (1001 * 8 + 255) // 256 * 256
    assert L.aarmvs_cloud_thin_scratch_bytes(-1) == 0 == L.aarmvs_cloud_thin_scratch_bytes(1 << 31)


def test_thin_rejects_null_args_and_null_pointers():
    assert _thin(None) == INVALID and _err() == "cloud_thin: null args"
    for field in ("xyz", "keys", "rank", "remaining", "scratch"):
        a = _args()
        setattr(a, field, None)
        assert _thin(a) == INVALID and _err() == "cloud_thin: null pointer argument", field
    for k in (0, 1):
        a = _args()
        a.state[k] = None
        assert _thin(a) == INVALID and _err() == "cloud_thin: null pointer argument"
    a = _args()        # n == 0 still writes remaining
    a.n, a.remaining = 0, None
    assert _thin(a) == INVALID and _err() == "cloud_thin: null pointer argument"


@pytest.mark.parametrize("n", [-1, 1 << 31, 1 << 40])
def test_thin_rejects_bad_counts(n):
    a = _args()
    a.n = n
    assert _thin(a) == INVALID and _err() == "cloud_thin: need 0 <= n < 2^31"


@pytest.mark.parametrize("rounds", [0, -3])
def test_thin_rejects_no_rounds(rounds):
    assert _thin(_args(), rounds) == INVALID and _err() == "cloud_thin: need rounds >= 1"


@pytest.mark.parametrize("which", [-1, 2])
def test_thin_rejects_a_bad_buffer_index(which):
    a = _args()
    a.which = which
    assert _thin(a) == INVALID and _err() == "cloud_thin: which must be 0 or 1"


@pytest.mark.parametrize("cell", [0.0, -1.0, float("nan"), float("inf")])
def test_thin_rejects_a_bad_cell(cell):
    a = _args()
    a.cell = cell
    assert _thin(a) == INVALID and _err() == "cloud_thin: cell must be finite and > 0"


@pytest.mark.parametrize("r", [-0.5, float("nan"), float("inf"), -float("inf")])
def test_thin_rejects_a_bad_radius(r):
    a = _args()
    a.r = r
    assert _thin(a) == INVALID and _err() == "cloud_thin: r must be finite and >= 0"


def test_thin_rejects_a_cell_below_the_radius():
    a = _args()
    a.cell, a.r = 0.5, 0.75
    assert _thin(a) == INVALID and _err() == "cloud_thin: cell must be >= r"
    a.cell = 0.2      # the double 0.2 is below the float 0.2f
    a.r = 0.2
    assert _thin(a) == INVALID and _err() == "cloud_thin: cell must be >= r"


def test_thin_rejects_a_non_finite_origin():
    a = _args()
    a.origin[2] = float("inf")
    assert _thin(a) == INVALID and _err() == "cloud_thin: origin must be finite"


@pytest.mark.parametrize("field,k,where", [
    ("state", 0, XYZ), ("state", 0, XYZ + 12 * N - 1), ("state", 1, KEYS + 8), ("state", 1, RANK - N + 1),
    ("remaining", None, XYZ + 100), ("remaining", None, RANK + 4 * N - 8), ("scratch", None, KEYS - 255),
    ("scratch", None, RANK)])
def test_thin_rejects_outputs_that_overlap_inputs(field, k, where):
    a = _args()
    if k is None:
        setattr(a, field, where)
    else:
        a.state[k] = where
    assert _thin(a) == INVALID and _err() == "cloud_thin: an output must not alias an input"


@pytest.mark.parametrize("field,k,where", [
    ("state", 1, S0), ("state", 1, S0 + N - 1), ("remaining", None, S0 + 50), ("remaining", None, S1 - 15),
    ("scratch", None, S1 + N - 1), ("scratch", None, REM - 255), ("remaining", None, SCR + 248)])
def test_thin_rejects_outputs_that_overlap_each_other(field, k, where):
    a = _args()
    if k is None:
        setattr(a, field, where)
    else:
        a.state[k] = where
    assert _thin(a) == INVALID and _err() == "cloud_thin: the outputs must not alias each other"


# (thin with n == 0 writes remaining = {0, 0}, which is device work: tests/test_gpu_cloud_dtu.py)


# --------------------------------------------------------------------------------- regions
def _regions(xyz=XYZ, n=N, mask=MASK, dims=(7, 5, 3), bb=(0, 0, 0, 7, 5, 3), res=1.0, patch=60.0,
             plane=(0, 0, 1, 0), flags=FLAGS):
    d = None if dims is None else (ctypes.c_int * 3)(*dims)
    b = None if bb is None else (ctypes.c_double * 6)(*bb)
    p = None if plane is None else (ctypes.c_double * 4)(*plane)
    return _L().aarmvs_cloud_regions(xyz, n, mask, d, b, res, patch, p, flags, None)


def test_regions_rejections():
    nan, inf = float("nan"), float("inf")
    for n in (-1, 1 << 31):
        assert _regions(n=n) == INVALID and _err() == "cloud_regions: need 0 <= n < 2^31"
    for kw in (dict(xyz=None), dict(flags=None), dict(bb=None), dict(dims=None)):
        assert _regions(**kw) == INVALID and _err() == "cloud_regions: null pointer argument", kw
    for bad in ((0, nan, 0, 7, 5, 3), (0, 0, 0, 7, 5, inf)):
        assert _regions(bb=bad) == INVALID and _err() == "cloud_regions: bb must be finite"
    for patch in (-1.0, nan, inf):
        assert _regions(patch=patch) == INVALID and _err() == "cloud_regions: patch must be finite and >= 0"
    for res in (0.0, -2.0, nan, inf):
        assert _regions(res=res) == INVALID and _err() == "cloud_regions: res must be finite and > 0"
    for dims in ((0, 5, 3), (7, -1, 3), (7, 5, 0)):
        assert _regions(dims=dims) == INVALID and _err() == "cloud_regions: every mask dimension must be >= 1"
    for dims in ((1 << 11, 1 << 10, 1 << 10), (1 << 30, 2, 1), (1 << 30, 1 << 30, 1 << 30)):
        assert _regions(dims=dims) == INVALID and _err() == "cloud_regions: the mask has 2^31 voxels or more"
    for flags in (XYZ, XYZ + 12 * N - 1, XYZ - N + 1, MASK + 104, MASK - N + 1):
        assert _regions(flags=flags) == INVALID and _err() == "cloud_regions: flags_out must not alias an input"


def test_regions_with_no_points_is_a_no_op():
    assert _regions(n=0, xyz=None, flags=None) == 0
    assert _regions(n=0, xyz=None, flags=None, mask=None, dims=None, bb=None, plane=None) == 0
    # without a mask, res is not looked at
    assert _regions(n=0, mask=None, dims=None, res=float("nan")) == 0


# --------------------------------------------------------------------------------- Python
def test_python_surface_and_argument_errors():
    import torch
    from aarmvs import AarmvsError, cloud_eval as ce
    th = inspect.signature(ce.thin).parameters
    assert list(th) == ["xyz", "radius", "order", "seed", "rounds_per_call"]
    assert (th["order"].default, th["seed"].default, th["rounds_per_call"].default) == ("random", 0, 8)
    rg = inspect.signature(ce.regions).parameters
    assert list(rg) == ["xyz", "obs_mask", "bb", "res", "patch", "plane"] and rg["patch"].default == 60.0
    ev = inspect.signature(ce.evaluate_dtu).parameters
    assert list(ev) == ["recon", "gt", "obs_mask", "bb", "res", "plane", "thin", "patch", "max_dist", "seed", "order"]
    assert [ev[k].default for k in ("thin", "patch", "max_dist", "seed", "order")] == [0.2, 60.0, 20.0, 0, "random"]
    x = torch.zeros(4, 3)
    with pytest.raises(AarmvsError):          # CPU tensors are refused: there is no CPU fallback
        ce.thin(x, 0.5)
    with pytest.raises(AarmvsError):
        ce.regions(x, plane=[0, 0, 1, 0])
    with pytest.raises(AarmvsError):
        ce.evaluate_dtu(x, x, torch.ones(2, 2, 2), [[0, 0, 0], [1, 1, 1]], 1.0, [0, 0, 1, 0])
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            ce.thin(x, radius)
    with pytest.raises(ValueError, match="distinct"):
        ce.thin(x, 0.5, order=torch.tensor([0, 1, 1, 2], dtype=torch.int32))
    with pytest.raises(ValueError, match="int32"):
        ce.thin(x, 0.5, order=torch.tensor([0, 1, 2, 3]))
    with pytest.raises(ValueError, match="int32"):
        ce.thin(x, 0.5, order=torch.tensor([0, 1, 2], dtype=torch.int32))
    with pytest.raises(ValueError, match="order"):
        ce.thin(x, 0.5, order="sorted")
    with pytest.raises(ValueError, match="rounds_per_call"):
        ce.thin(x, 0.5, rounds_per_call=0)
    p = ce.build_parser()
    a = p.parse_args(["--protocol", "dtu", "--recon", "a.ply", "--gt", "b.ply", "--obs_mask", "m.mat", "--plane", "p.mat"])
    assert (a.protocol, a.obs_mask, a.plane, a.thin, a.patch, a.max_dist, a.seed) == ("dtu", "m.mat", "p.mat", 0.2,
                                                                                     60.0, None, 0)
    # the plain mode still requires --max_dist
    with pytest.raises(SystemExit):
        ce.main(["--recon", "a.ply", "--gt", "b.ply"])
    assert p.parse_args(["--recon", "a.ply", "--gt", "b.ply", "--max_dist", "20"]).protocol is None
