"""GPU tests of the DTU protocol (aarmvs_cloud_thin, aarmvs_cloud_regions; aarmvs/cloud_eval.py): the
kept set equals the literal sequential walk and the round count the round rule's, the region flags
and every field of evaluate_dtu equal the numpy restatement (tests/cloud_dtu_ref.py, itself checked
in test_cloud_dtu_ref.py)."""
import ctypes
import json
import math
import time

import numpy as np
import pytest

import cloud_dtu_ref as dtu

pytestmark = pytest.mark.gpu
R = dtu.R


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_WANT = {}


def _want(name, xyz, r, rank):
    """(kept by the sequential walk, rounds of the round rule), computed once per named case."""
    if name not in _WANT:
        seq = dtu.thin_sequential(xyz, r, rank)
        par, rounds = dtu.thin_rounds(xyz, r, rank)
        assert (par == seq).all()
        _WANT[name] = (seq, rounds)
    return _WANT[name]


def _check(torch, name, xyz, order, r=R, rounds_per_call=8):
    from aarmvs import cloud_eval as ce
    n = xyz.shape[0]
    rank = dtu.ranks_of(order, 0, n)
    want, want_rounds = _want(name, xyz, r, rank)
    given = order if isinstance(order, str) else torch.from_numpy(np.asarray(order, np.int32))
    idx, rounds = ce.thin(_dev(torch, xyz), r, given, seed=0, rounds_per_call=rounds_per_call)
    assert idx.dtype == torch.int64 and idx.is_cuda
    idx = idx.cpu().numpy()
    assert (np.diff(idx) > 0).all()                            # ascending, in the caller's order
    kept = np.zeros(n, bool)
    kept[idx] = True
    np.testing.assert_array_equal(kept, want)
    assert rounds == want_rounds
    return kept, rounds


@pytest.mark.parametrize("order", ["random", "input"])
@pytest.mark.parametrize("side", [12, 6])
def test_random_clouds_on_the_quarter_lattice(torch, side, order):
    """20,000 points, r = 0.75: ties at exactly r, duplicates, 19.5 (12^3) and 137 (6^3) neighbours
    per point."""
    xyz = dtu.lattice_cloud(side)
    kept, rounds = _check(torch, f"lattice{side}_{order}", xyz, order)
    a, _ = dtu.neighbour_pairs(xyz, R)
    assert (15 if side == 12 else 100) < a.size / xyz.shape[0] < (30 if side == 12 else 200)
    assert 100 < kept.sum() < xyz.shape[0] // 2 and rounds <= 40


@pytest.mark.parametrize("rounds_per_call", [8, 1, 64])
def test_the_raster_plane_in_input_order(torch, rounds_per_call):
    """A long chain of decisions (one row decides after the other): many calls at 8 rounds per call,
    and the same set and the same round count at 1 and 64."""
    kept, rounds = _check(torch, "raster", dtu.raster_plane(), "input", rounds_per_call=rounds_per_call)
    assert rounds > 100


def test_the_line_needs_n_rounds(torch):
    kept, rounds = _check(torch, "line", dtu.line(), "input", rounds_per_call=64)
    assert rounds == 256
    np.testing.assert_array_equal(kept, np.arange(256) % 2 == 0)
    _, few = _check(torch, "line_random", dtu.line(), "random")
    assert few <= 32


def test_copies_of_one_point(torch):
    xyz = np.tile(np.float32([[1.25, -2, 3]]), (1000, 1))
    kept, rounds = _check(torch, "copies", xyz, "random")
    assert kept.sum() == 1 and kept[np.argmin(dtu.ranks_of("random", 0, 1000))] and rounds == 2


def test_a_pair_exactly_at_r_and_one_just_beyond(torch):
    r = np.float32(0.75)
    beyond = np.nextafter(r, np.float32(2))
    for name, gap, n_kept in (("at_r", r, 1), ("beyond_r", beyond, 2)):
        for axis in range(3):
            xyz = np.float32([[1, 0, 3], [1, 0, 3]])
            xyz[:, axis] = [0, gap]                            # the difference is the gap itself, exactly
            kept, _ = _check(torch, f"{name}{axis}", xyz, "input", r=r)
            assert kept.sum() == n_kept and kept[0]
    # a 3-4-5 triangle scaled to r = 1.25: d2 == r r exactly, across a cell edge; the third point is
    # 1/16 beyond in d2
    xyz = np.float32([[0, 0, 0], [0.75, 1, 0], [-0.75, -1, 0.25]])
    kept, _ = _check(torch, "diagonal", xyz, "input", r=np.float32(1.25))
    np.testing.assert_array_equal(kept, [True, False, True])


def test_cell_faces_and_negative_coordinates(torch):
    """Multiples of 1/4 in [-2.25, 2.25] with cell = r = 0.75: every third lattice plane is a cell
    face, with points on it and on both sides; the grid's origin is negative."""
    xyz = (np.random.default_rng(5).integers(-9, 10, (3000, 3)) * 0.25).astype(np.float32)
    kept, _ = _check(torch, "faces", xyz, "random")
    assert 20 < kept.sum() < 1000
    # off the lattice, cell = r not a binary fraction: faces at no special coordinates
    xyz = (np.random.default_rng(6).random((3000, 3)) * 4 - 2).astype(np.float32)
    _check(torch, "faces_off", xyz, "random", r=np.float32(0.3))


def test_non_finite_and_huge_coordinates(torch):
    xyz = dtu.lattice_cloud(4, 600, seed=3)
    bad = [np.nan, np.inf, -np.inf]
    for k in range(30):
        xyz[7 * k, k % 3] = bad[k % 3]
    xyz[11] = np.nan
    kept, _ = _check(torch, "non_finite", xyz, "random")
    fin = np.isfinite(xyz).all(1)
    assert not kept[~fin].any() and kept[fin].sum() > 10
    # the finite points thin as if the others were not there: a dropped point hides no neighbour
    alone, _ = _check(torch, "non_finite_alone", xyz[fin], dtu.ranks_of("random", 0, 600)[fin].argsort().argsort())
    np.testing.assert_array_equal(kept[fin], alone)
    # 1e30 is a finite point: the grid grows to hold it (one cell holds all the others)
    xyz[3], xyz[4] = [1e30, 0, 0], [0, -1e30, 1]
    kept, _ = _check(torch, "huge", xyz, "random")
    assert kept[3] and kept[4]


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_small_sizes(torch, n):
    kept, rounds = _check(torch, f"small{n}", dtu.lattice_cloud(3, n, seed=n), "random")
    assert kept.sum() >= 1 and (n > 1 or rounds == 1)


def test_no_points(torch):
    from aarmvs import _lib, cloud_eval as ce, lib
    idx, rounds = ce.thin(torch.zeros(0, 3, device="cuda"), 0.5)
    assert idx.shape == (0,) and idx.dtype == torch.int64 and rounds == 0
    # all points dropped: nothing is ever undecided
    idx, rounds = ce.thin(torch.full((5, 3), float("nan"), device="cuda"), 0.5)
    assert idx.shape == (0,) and rounds == 0
    # the raw call with n == 0 writes remaining = {0, 0} and needs no cloud
    remaining = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    scratch = torch.zeros(lib().aarmvs_cloud_thin_scratch_bytes(0), dtype=torch.uint8, device="cuda")
    a = _lib.CloudThinArgs()
    a.n, a.cell, a.r, a.init = 0, 1.0, 0.5, 1
    a.remaining, a.scratch = remaining.data_ptr(), scratch.data_ptr()
    _lib.check(lib().aarmvs_cloud_thin(ctypes.byref(a), 3, torch.cuda.current_stream().cuda_stream), "cloud_thin")
    torch.cuda.synchronize()
    assert remaining.tolist() == [0, 0]
    assert ce.regions(torch.zeros(0, 3, device="cuda"), plane=[0, 0, 1, 0]).shape == (0,)


def _raw_thin(torch, xyz, r, rank, rounds_per_call):
    """aarmvs_cloud_thin through the Python plumbing's pieces, every output carved out of a 0xAB-filled
    buffer whose guard bytes are checked: (final state bytes in the sorted layout, kept in the
    caller's order, rounds, calls)."""
    from aarmvs import _lib, cloud_eval as ce, lib
    n, pad = xyz.shape[0], 64
    origin, cell = dtu.thin_grid(xyz, r)
    xd = _dev(torch, xyz)
    keys, perm = torch.sort(ce.cloud_keys(xd, origin, cell), stable=True)
    xs, rs = xd[perm].contiguous(), _dev(torch, np.asarray(rank, np.int32))[perm].contiguous()
    scr = lib().aarmvs_cloud_thin_scratch_bytes(n)
    sizes = [n, n, 16, scr]
    bufs = [torch.full((2 * pad + s,), 0xAB, dtype=torch.uint8, device="cuda") for s in sizes]
    a = _lib.CloudThinArgs()
    a.xyz, a.keys, a.rank, a.n = xs.data_ptr(), keys.data_ptr(), rs.data_ptr(), n
    a.origin[0], a.origin[1], a.origin[2] = (float(v) for v in origin)
    a.cell, a.r = float(cell), float(r)
    a.state[0], a.state[1] = bufs[0].data_ptr() + pad, bufs[1].data_ptr() + pad
    a.remaining, a.scratch = bufs[2].data_ptr() + pad, bufs[3].data_ptr() + pad
    a.init, a.which = 1, 0
    rounds = calls = 0
    while True:
        assert calls * rounds_per_call < n + rounds_per_call
        _lib.check(lib().aarmvs_cloud_thin(ctypes.byref(a), rounds_per_call, torch.cuda.current_stream().cuda_stream),
                   "cloud_thin")
        torch.cuda.synchronize()
        calls += 1
        a.init, a.which = 0, (a.which + rounds_per_call) & 1
        left, used = bufs[2].cpu().numpy()[pad:pad + 16].view(np.int64)
        assert 0 <= used <= rounds_per_call and (left == 0 or used == rounds_per_call)
        rounds += int(used)
        if left == 0:
            break
    raw = [b.cpu().numpy() for b in bufs]
    for b, s in zip(raw, sizes):
        assert (b[:pad] == 0xAB).all() and (b[pad + s:] == 0xAB).all()
    state = raw[a.which][pad:pad + n]
    assert set(np.unique(state)) <= {1, 2}
    kept = np.zeros(n, bool)
    kept[perm.cpu().numpy()[state == 1]] = True
    return state.tobytes(), kept, rounds, calls


@pytest.mark.parametrize("rounds_per_call", [3, 8])
def test_guard_bytes_and_two_identical_runs(torch, rounds_per_call):
    """An odd and an even number of rounds per call: the state ends in the buffer the header names."""
    xyz = dtu.lattice_cloud(5, 3001, seed=9)
    rank = dtu.ranks_of("random", 0, 3001)
    a = _raw_thin(torch, xyz, R, rank, rounds_per_call)
    b = _raw_thin(torch, xyz, R, rank, rounds_per_call)
    assert a[0] == b[0] and a[2:] == b[2:]
    want, want_rounds = _want("guard", xyz, R, rank)
    np.testing.assert_array_equal(a[1], want)
    assert a[2] == want_rounds and a[3] == -(-want_rounds // rounds_per_call)


def test_thin_on_a_side_stream(torch):
    """The contract tests/test_gpu_streams.py holds the other cloud ops to: the cloud is produced on a
    side stream behind a delay from a poisoned buffer, thin is called under that stream, and the
    poison is written back behind it.  A launch on any other stream would thin the poison."""
    import stream_cases as sc
    from aarmvs import cloud_eval as ce
    xyz, poison = _dev(torch, dtu.lattice_cloud(6, 5000, seed=21)), _dev(torch, dtu.lattice_cloud(6, 5000, seed=22))
    buf = xyz.clone()
    torch.cuda.synchronize()
    ce.thin(buf, R)                                            # warm
    t0 = time.perf_counter()
    want_idx, want_rounds = ce.thin(buf, R)
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    poison_idx, _ = ce.thin(poison, R)
    assert not torch.equal(poison_idx, want_idx)
    buf.copy_(poison)
    torch.cuda.synchronize()
    sc._sleep_cycles_per_ms()
    ms = sc.delay_ms(dt)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ev = sc.delay(s, ms)
        buf.copy_(xyz, non_blocking=True)
        # thin waits for the device inside: the precondition holds before it
        sc.require_pending(ev, "thin (before the call)", serial_call_ms=dt * 1e3, delay_ms=ms)
        idx, rounds = ce.thin(buf, R)
        idx = idx.clone()
        buf.copy_(poison, non_blocking=True)
    torch.cuda.synchronize()
    sc.same_bits({"idx": idx}, {"idx": want_idx}, "thin on a side stream")
    assert rounds == want_rounds


# --------------------------------------------------------------------------------- regions
def _regions_case():
    pts, _, bb, res, patch, plane, _ = dtu.hand_regions()
    rng = np.random.default_rng(31)
    mask = (rng.random((7, 5, 3)) < 0.6).astype(np.uint8)
    lo, hi = bb[0] - 4, bb[1] + 6
    cloud = (rng.random((1500, 3)) * (hi - lo) + lo).astype(np.float32)
    halves = (rng.integers(0, 40, (500, 3)) * 0.5 + (bb[0] - 2)).astype(np.float32)    # g at x.5, box faces
    xyz = np.concatenate([pts, cloud, halves])
    xyz[100::97, 2] = np.nan
    return xyz, mask, bb, res, patch, plane


def _flags(torch, xyz, *a, **kw):
    from aarmvs import cloud_eval as ce
    f = ce.regions(_dev(torch, xyz), *a, **kw)
    assert f.dtype == torch.uint8 and f.is_cuda and f.shape == (xyz.shape[0],)
    return f.cpu().numpy()


def test_regions_on_the_hand_worked_points(torch):
    pts, mask, bb, res, patch, plane, want = dtu.hand_regions()
    np.testing.assert_array_equal(_flags(torch, pts, mask, bb, res, patch, plane), want)
    np.testing.assert_array_equal(_flags(torch, pts, _dev(torch, mask), bb, res, patch, plane), want)


def test_regions_equal_the_restatement(torch):
    xyz, mask, bb, res, patch, plane = _regions_case()
    got = _flags(torch, xyz, mask, bb, res, patch, plane)
    assert got.tobytes() == dtu.regions(xyz, mask, bb, res, patch, plane).tobytes()
    assert set(np.unique(got)) == {0, 1, 3, 4, 5, 7} and np.bincount(got, minlength=8)[[0, 1, 3, 4, 5, 7]].min() >= 10
    assert (got[np.isnan(xyz).any(1)] == 0).all()
    # the forms without a mask, a box or a plane: the bit of a missing input is 0
    assert _flags(torch, xyz, None, bb, None, patch, plane).tobytes() == (got & 5).tobytes()
    assert _flags(torch, xyz, mask, bb, res, patch).tobytes() == (got & 3).tobytes()
    assert _flags(torch, xyz, plane=plane).tobytes() == (got & 4).tobytes()
    assert not _flags(torch, xyz).any()
    assert _flags(torch, xyz, mask, bb, res, patch, plane).tobytes() == got.tobytes()
    # another patch moves the box, a patch of 0 is allowed
    for p in (0.0, 3.5):
        assert _flags(torch, xyz, mask, bb, res, p, plane).tobytes() == dtu.regions(xyz, mask, bb, res, p, plane).tobytes()


def test_regions_guard_bytes(torch):
    from aarmvs import _lib, lib
    xyz, mask, bb, res, patch, plane = _regions_case()
    n, pad = xyz.shape[0], 64
    buf = torch.full((2 * pad + n,), 0xAB, dtype=torch.uint8, device="cuda")
    xd, md = _dev(torch, xyz), _dev(torch, mask)
    _lib.check(lib().aarmvs_cloud_regions(xd.data_ptr(), n, md.data_ptr(), (ctypes.c_int * 3)(7, 5, 3),
                                          (ctypes.c_double * 6)(*bb.reshape(6)), res, patch,
                                          (ctypes.c_double * 4)(*plane), buf.data_ptr() + pad,
                                          torch.cuda.current_stream().cuda_stream), "cloud_regions")
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[:pad] == 0xAB).all() and (raw[pad + n:] == 0xAB).all()
    assert raw[pad:pad + n].tobytes() == dtu.regions(xyz, mask, bb, res, patch, plane).tobytes()


# --------------------------------------------------------------------------------- end to end
THIN, MAX_DIST = 5.0, 6.0    # scene units: the fused points are 2 to 8 apart (60 % survive 5.0)


@pytest.fixture(scope="module")
def scan(torch):
    """The fused synthetic scan at 40x52 with 2 source views (plain), its ground-truth cloud, a
    synthetic observation mask (about 24^3, a seeded pattern that leaves part of the surface
    unobserved) and a plane that cuts the ground truth roughly in half.  The mask's box is the
    ground truth's bounds drawn in by a tenth of the extent per side in x and y: the fused cloud
    lies inside the ground truth's own bounds, which would make IN_BOX a step that drops nothing."""
    from aarmvs import fusion, synthetic as syn
    H, W, nsrc = 40, 52, 2
    depths, cams, _ = syn.fusion_views(H, W, nsrc, seed=0)
    rng = np.random.default_rng(100)
    n = nsrc + 1
    confs = {v: torch.from_numpy(rng.random((H, W)).astype(np.float32)).cuda() for v in range(n)}
    depths = {v: torch.from_numpy(d).cuda() for v, d in enumerate(depths)}
    pairs = [(v, [s for s in range(n) if s != v]) for v in range(n)]
    recon = fusion.fuse_views(pairs, depths, confs, dict(enumerate(cams)), None, 0.35)["xyz"]
    gt = syn.fusion_ground_truth(H, W, nsrc)
    bb = np.stack([gt.min(0), gt.max(0)]).astype(np.float64)
    inset = 0.1 * (bb[1] - bb[0]) * [1, 1, 0]
    bb = np.stack([bb[0] + inset, bb[1] - inset])
    res = float((bb[1] - bb[0]).max() / 23.0)
    dims = (np.floor((bb[1] - bb[0]) / res) + 1).astype(int)
    mask = (np.random.default_rng(101).random(tuple(dims)) < 0.7).astype(np.uint8)
    axis = int(np.argmax(bb[1] - bb[0]))
    plane = np.zeros(4)
    plane[axis], plane[3] = 1.0, -float(np.median(gt[:, axis]))
    return dict(recon=recon, gt=torch.from_numpy(gt).cuda(), mask=mask, bb=bb, res=res, plane=plane,
                kw=dict(thin=THIN, patch=0.0, max_dist=MAX_DIST, seed=3))


def _same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        g, w = got[k], want[k]
        assert type(g) is type(w) and (g == w or (isinstance(w, float) and math.isnan(w) and math.isnan(g))), (k, g, w)


FIELDS = ["n_recon", "n_thinned", "n_in_box", "n_in_obs", "n_gt", "n_gt_above", "thin_rounds", "accuracy_mean",
          "accuracy_median", "completeness_mean", "completeness_median", "overall", "recon_beyond_max_dist",
          "gt_beyond_max_dist", "recon_nonfinite", "gt_nonfinite", "thin", "patch", "max_dist", "seed", "order"]


def test_evaluate_dtu_end_to_end(torch, scan):
    """Every field equals the restatement's: counts exactly, means in the fixed-order form, medians
    the lower middle value.  No step of the protocol is a no-op on this scan."""
    from aarmvs import cloud_eval as ce
    got = ce.evaluate_dtu(scan["recon"], scan["gt"], scan["mask"], scan["bb"], scan["res"], scan["plane"], **scan["kw"])
    print(json.dumps(got))
    assert sorted(got) == sorted(FIELDS)
    assert 0.25 * got["n_recon"] < got["n_thinned"] < 0.75 * got["n_recon"]
    assert 0 < got["n_in_obs"] < got["n_in_box"] < got["n_thinned"] < got["n_recon"]
    assert 0 < got["n_gt_above"] < got["n_gt"] and 0.3 < got["n_gt_above"] / got["n_gt"] < 0.7
    assert 0 < got["accuracy_mean"] < MAX_DIST and 0 < got["completeness_mean"] < MAX_DIST
    assert got["thin_rounds"] >= 2 and got["gt_beyond_max_dist"] > 0
    want = dtu.evaluate_dtu(scan["recon"].cpu().numpy(), scan["gt"].cpu().numpy(), scan["mask"], scan["bb"],
                            scan["res"], scan["plane"], **scan["kw"])
    _same(got, want)
    again = ce.evaluate_dtu(scan["recon"], scan["gt"], scan["mask"], scan["bb"], scan["res"], scan["plane"], **scan["kw"])
    assert json.dumps(again) == json.dumps(got)


def test_the_command_line_gives_the_same_dict(torch, scan, tmp_path):
    from scipy.io import savemat
    from aarmvs import cloud_eval as ce, fusion
    a, b, j = str(tmp_path / "recon.ply"), str(tmp_path / "stl.ply"), str(tmp_path / "out.json")
    m, p = str(tmp_path / "ObsMask1_10.mat"), str(tmp_path / "Plane1.mat")
    fusion.write_ply(a, scan["recon"].cpu().numpy())
    fusion.write_ply(b, scan["gt"].cpu().numpy())
    savemat(m, {"ObsMask": np.asfortranarray(scan["mask"].astype(bool)), "BB": scan["bb"],
                "Res": np.float64([[scan["res"]]])})
    savemat(p, {"P": scan["plane"].reshape(4, 1)})
    kw = scan["kw"]
    res = ce.main(["--protocol", "dtu", "--recon", a, "--gt", b, "--obs_mask", m, "--plane", p, "--thin", repr(kw["thin"]),
                   "--patch", repr(kw["patch"]), "--max_dist", repr(kw["max_dist"]), "--seed", str(kw["seed"]),
                   "--json", j])
    want = ce.evaluate_dtu(scan["recon"], scan["gt"], scan["mask"], scan["bb"], scan["res"], scan["plane"], **kw)
    _same(res, want)
    _same(json.load(open(j)), want)
