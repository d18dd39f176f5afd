"""GPU tests of the point-cloud evaluation (aarmvs_cloud_*; aarmvs/cloud_eval.py): every output is
compared bit for bit with the numpy restatement of the definition (tests/cloud_eval_ref.py, itself
checked against cKDTree in test_cloud_eval_ref.py)."""
import ctypes
import json
import math

import numpy as np
import pytest

import cloud_eval_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw_nn(torch, q, t, origin, cell, max_dist, ids=None, want_index=True, guard=False):
    """aarmvs_cloud_nn through the Python plumbing's pieces: keys, a stable sort, the kernel.  With
    ``guard`` the outputs are carved out of 0xAB-filled buffers and the guard bytes are checked."""
    from aarmvs import cloud_eval as ce
    qd, td = _dev(torch, q), _dev(torch, t)
    keys, perm = torch.sort(ce.cloud_keys(td, origin, cell), stable=True)
    np.testing.assert_array_equal(keys.cpu().numpy(), np.sort(ref.keys(t, origin, cell), kind="stable"))
    ts = td[perm].contiguous()
    tid = perm.to(torch.int32) if ids is None else _dev(torch, np.asarray(ids, np.int32))[perm].contiguous()
    if not guard:
        d, i = ce.nn_sorted(qd, ts, keys, tid, origin, cell, max_dist, want_index)
        torch.cuda.synchronize()
        return d.cpu().numpy(), (None if i is None else i.cpu().numpy())
    from aarmvs import _lib, lib
    nq, pad = q.shape[0], 64
    bufs = [torch.full((2 * pad + 4 * nq,), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(2)]
    a = _lib.CloudNnArgs()
    a.query, a.target, a.target_keys, a.target_ids = qd.data_ptr(), ts.data_ptr(), keys.data_ptr(), tid.data_ptr()
    a.nq, a.m = nq, t.shape[0]
    a.origin[0], a.origin[1], a.origin[2] = (float(v) for v in origin)
    a.cell, a.max_dist = float(cell), float(max_dist)
    a.dist_out, a.index_out = bufs[0].data_ptr() + pad, bufs[1].data_ptr() + pad
    _lib.check(lib().aarmvs_cloud_nn(ctypes.byref(a), torch.cuda.current_stream().cuda_stream), "cloud_nn")
    torch.cuda.synchronize()
    raw = [b.cpu().numpy() for b in bufs]
    for r in raw:
        assert (r[:pad] == 0xAB).all() and (r[pad + 4 * nq:] == 0xAB).all()
    return raw[0][pad:pad + 4 * nq].view(np.float32), raw[1][pad:pad + 4 * nq].view(np.int32)


def _check(torch, q, t, origin, cell, max_dist, ids=None, **kw):
    d, i = _raw_nn(torch, q, t, origin, cell, max_dist, ids, **kw)
    want_d, want_i = ref.nn(q, t, origin, cell, max_dist, target_ids=ids)
    np.testing.assert_array_equal(d, want_d)
    np.testing.assert_array_equal(i, want_i)
    return d, i


def _uniform(seed, n, scale=8.0):
    return (np.random.default_rng(seed).random((n, 3)) * scale).astype(np.float32)


@pytest.mark.parametrize("rings", [1, 8])
def test_uniform_clouds_one_ring_and_eight(torch, rings):
    q, t = _uniform(1, 2000), _uniform(2, 3000)
    max_dist = 0.5
    d, _ = _check(torch, q, t, np.zeros(3), max_dist / rings, max_dist)
    assert 100 < np.isfinite(d).sum() < q.shape[0]   # both outcomes occur


@pytest.mark.parametrize("nq,m", [(1, 4097), (63, 1), (64, 2), (65, 4097), (257, 2), (4097, 1), (4097, 4097)])
def test_sizes(torch, nq, m):
    q, t = _uniform(10 + nq, nq, 4.0), _uniform(20 + m, m, 4.0)
    _check(torch, q, t, np.zeros(3), 0.25, 1.0)


def test_two_tight_clusters_far_apart(torch):
    rng = np.random.default_rng(3)
    t = np.concatenate([rng.normal(0, 0.02, (1500, 3)) + 5, rng.normal(0, 0.02, (1500, 3)) + 60]).astype(np.float32)
    # queries: most far from both clusters, some a few rings out, some inside
    q = np.concatenate([rng.random((1500, 3)) * 64, rng.normal(0, 1.0, (400, 3)) + 5,
                        rng.normal(0, 0.05, (100, 3)) + 60]).astype(np.float32)
    d, _ = _check(torch, q, t, np.zeros(3) - 4.0, 0.5, 3.0)
    assert np.isinf(d).sum() > q.shape[0] // 2 and ((d > 1.5) & np.isfinite(d)).sum() > 20


@pytest.mark.parametrize("cell", [0.5, 0.1, 1.0 / 3.0])
def test_coordinates_on_exact_multiples_of_the_cell(torch, cell):
    """Targets on the lattice, queries on lattice points, face centres and corners: an early stop,
    or a neighbour cell skipped at a face, shows here."""
    rng = np.random.default_rng(4)
    lat = rng.integers(0, 12, (1500, 3))
    t = (lat * np.float64(cell)).astype(np.float32)
    ql = rng.integers(0, 24, (2000, 3)) / 2.0          # lattice points and half-way points
    q = (ql * np.float64(cell)).astype(np.float32)
    for max_dist in (cell, 2 * cell, 2.5 * cell):
        _check(torch, q, t, np.zeros(3), cell, np.float32(max_dist))
    _check(torch, q, t, np.float64([-cell, -2 * cell, 0.0]), cell, np.float32(3 * cell))


def test_ties_with_and_without_ids(torch):
    rng = np.random.default_rng(5)
    base = rng.integers(0, 6, (300, 3)).astype(np.float32)
    t = np.concatenate([base, base, base[::-1]])            # every target three times
    # symmetric pairs: queries half-way between lattice points, and on the targets themselves
    q = np.concatenate([base + np.float32([0.5, 0, 0]), base, rng.integers(0, 12, (400, 3)).astype(np.float32) / 2])
    m = t.shape[0]
    for ids in (None, np.arange(m)[::-1].copy(), rng.permutation(m)):
        d, i = _check(torch, q, t, np.zeros(3), 0.5, 1.5, ids=ids)
        assert (d[300:600] == 0).all()
    d, i = _raw_nn(torch, q, t, np.zeros(3), 0.5, 1.5, want_index=False)
    assert i is None
    np.testing.assert_array_equal(d, ref.nn(q, t, np.zeros(3), 0.5, 1.5)[0])


@pytest.mark.parametrize("raw", [False, True])
def test_ties_with_target_ids_null(torch, raw):
    """target_ids == NULL: the id is the position in the key-sorted target, so the index is a sorted
    position and ties go to the lowest one.  Through nn_sorted(ids=None) and through the raw struct."""
    from aarmvs import _lib, cloud_eval as ce, lib
    rng = np.random.default_rng(5)
    base = rng.integers(0, 6, (300, 3)).astype(np.float32)
    t = np.concatenate([base, base, base[::-1]])            # duplicates: every target three times
    q = np.concatenate([base + np.float32([0.5, 0, 0]), base, rng.integers(0, 12, (400, 3)).astype(np.float32) / 2])
    t[7, 1], t[11, 0] = np.nan, -3.0                        # not in the grid: sorted last, never a neighbour
    origin, cell, max_dist = np.zeros(3), 0.5, 1.5
    qd, td = _dev(torch, q), _dev(torch, t)
    keys, perm = torch.sort(ce.cloud_keys(td, origin, cell), stable=True)
    ts = td[perm].contiguous()
    t_sorted = ts.cpu().numpy()
    want_d, want_i = ref.nn(q, t_sorted, origin, cell, max_dist)     # no ids: positions in t_sorted
    if not raw:
        d, i = ce.nn_sorted(qd, ts, keys, None, origin, cell, max_dist)
    else:
        d = torch.empty(q.shape[0], dtype=torch.float32, device="cuda")
        i = torch.empty(q.shape[0], dtype=torch.int32, device="cuda")
        a = _lib.CloudNnArgs()
        a.query, a.target, a.target_keys, a.target_ids = qd.data_ptr(), ts.data_ptr(), keys.data_ptr(), None
        a.nq, a.m = q.shape[0], t.shape[0]
        a.cell, a.max_dist = cell, max_dist
        a.dist_out, a.index_out = d.data_ptr(), i.data_ptr()
        assert not a.target_ids
        _lib.check(lib().aarmvs_cloud_nn(ctypes.byref(a), torch.cuda.current_stream().cuda_stream), "cloud_nn")
    torch.cuda.synchronize()
    d, i = d.cpu().numpy(), i.cpu().numpy()
    np.testing.assert_array_equal(d, want_d)
    np.testing.assert_array_equal(i, want_i)
    # the ties are real: mapped back to the caller's numbering, the lowest sorted position is not always
    # the lowest original index (a symmetric pair's two targets lie in different cells)
    found = i >= 0
    assert found.sum() > 600 and (i[found] < t.shape[0] - 2).all()
    assert (perm.cpu().numpy()[i[found]] != ref.nn(q, t, origin, cell, max_dist)[1][found]).any()


def test_a_target_exactly_at_max_dist_is_included(torch):
    t = np.float32([[4, 4, 4], [10, 4, 4]])
    q = np.float32([[4, 4, 6], [4, 2, 4], [2, 4, 4], [4, 4, 6.000001], [7, 8, 4], [12.5, 4, 4]])
    for cell in (2.0, 0.5, 0.25):
        d, i = _check(torch, q, t, np.zeros(3), cell, 2.0)
        np.testing.assert_array_equal(d[:3], [2, 2, 2])
        assert np.isposinf(d[3]) and np.isposinf(d[4]) and np.isposinf(d[5]) and (i[3:] == -1).all()
    d, _ = _check(torch, np.float32([[7, 8, 4]]), t, np.zeros(3), 1.0, 5.0)    # a 3-4-5 triangle, both sides
    assert d[0] == 5.0
    _check(torch, q, t, np.zeros(3), 1.0, 0.0)                                  # max_dist 0: only coincident points


def test_non_finite_and_huge_coordinates(torch):
    q, t = _uniform(6, 500, 4.0), _uniform(7, 700, 4.0)
    bad = np.float32([np.nan, np.inf, -np.inf, 1e30, -1e30])
    for k, v in enumerate(bad):
        q[3 * k, k % 3] = v
        t[5 * k + 1, (k + 1) % 3] = v
    q[40] = np.nan
    d, i = _check(torch, q, t, np.zeros(3), 0.25, 1.0)
    assert np.isnan(d[[0, 3, 6, 40]]).all() and np.isposinf(d[[9, 12]]).all() and (i[[0, 3, 6, 9, 12, 40]] == -1).all()
    # a finite query outside the grid, through the raw ABI: +inf / -1
    d, i = _check(torch, np.float32([[-0.5, 1, 1], [1, 1, 1]]), t, np.zeros(3), 0.25, 1.0)
    assert np.isposinf(d[0]) and i[0] == -1 and np.isfinite(d[1])
    # no target in the grid at all, and no target
    d, i = _check(torch, q, np.full((5, 3), np.nan, np.float32), np.zeros(3), 0.25, 1.0)
    assert not np.isfinite(d).any()
    from aarmvs import cloud_eval as ce
    empty = torch.zeros(0, 3, device="cuda")
    d, i = ce.nn_distance(_dev(torch, q), empty, 1.0)
    np.testing.assert_array_equal(d.cpu().numpy(), np.where(np.isfinite(q).all(1), np.float32(np.inf), np.float32(np.nan)))
    assert (i.cpu().numpy() == -1).all()
    d, i = ce.nn_distance(empty, _dev(torch, t), 1.0)
    assert d.shape == (0,) and i.shape == (0,)


def test_huge_coordinates_through_the_python_layer(torch):
    """1e30 is a finite point: the grid grows to hold it (a few cells in all), the result stays exact."""
    from aarmvs import cloud_eval as ce
    q, t = _uniform(8, 300, 4.0), _uniform(9, 400, 4.0)
    q[7, 0], t[11, 2], t[12, 1] = 1e30, 1e30, np.nan
    origin, cell = ref.grid_for([q, t], 1.0)
    d, i = ce.nn_distance(_dev(torch, q), _dev(torch, t), 1.0)
    want_d, want_i = ref.nn(q, t, origin, cell, 1.0)
    np.testing.assert_array_equal(d.cpu().numpy(), want_d)
    np.testing.assert_array_equal(i.cpu().numpy(), want_i)
    q, t = _uniform(8, 30, 4.0), _uniform(9, 40, 4.0)
    with pytest.raises(ValueError, match="ring limit"):
        ce.nn_distance(_dev(torch, q), _dev(torch, t), 1.0, cell=0.01)


def test_the_grid_edges_clamp_and_do_not_wrap(torch):
    """Clouds in the cells i_a = 0 and i_a = 2^21 - 1: a row left of x = 0 or right of x = 2^21 - 1 is
    another row's key range and must not be scanned as a neighbour."""
    top = float((1 << 21) - 1)
    rng = np.random.default_rng(11)
    corner = rng.integers(0, 3, (400, 3)).astype(np.float64)
    # x at the far edge with y one row further: its key follows (x = 0, y + 1)'s directly
    t = np.concatenate([corner, [top, top, top] - corner, [[top, 0, 0], [0, 1, 0], [0, 0, 1], [top, top - 1, top]]])
    q = np.concatenate([corner[:200] + 0.5, [top, top, top] - corner[:200] - 0.25,
                        [[0, 1, 0], [top, 0, 0], [0.5, 0.5, 0.5], [top, top, top], [0, 0, 0]]])
    t, q = t.astype(np.float32), q.astype(np.float32)
    for max_dist in (1.0, 3.0):
        _check(torch, q, t, np.zeros(3), 1.0, max_dist)
    k = ref.keys(t, np.zeros(3), 1.0)
    assert k.max() == (((1 << 21) - 1) << 42) | (((1 << 21) - 1) << 21) | ((1 << 21) - 1) and k.min() == 0


def test_guard_bytes_and_two_identical_runs(torch):
    q, t = _uniform(12, 1000), _uniform(13, 1500)
    a = _raw_nn(torch, q, t, np.zeros(3), 0.125, 0.5, guard=True)
    b = _raw_nn(torch, q, t, np.zeros(3), 0.125, 0.5, guard=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    want = ref.nn(q, t, np.zeros(3), 0.125, 0.5)
    np.testing.assert_array_equal(a[0], want[0])
    np.testing.assert_array_equal(a[1], want[1])


def test_nn_distance_picks_the_grid_and_restores_the_order(torch):
    from aarmvs import cloud_eval as ce
    q, t = _uniform(14, 1200) - 3, _uniform(15, 900) - 3
    for max_dist, cell in ((0.4, None), (0.4, 0.4), (1.0, 0.05)):
        origin, c = ref.grid_for([q, t], max_dist, cell)
        d, i = ce.nn_distance(_dev(torch, q), _dev(torch, t), max_dist, cell)
        want = ref.nn(q, t, origin, c, max_dist)
        np.testing.assert_array_equal(d.cpu().numpy(), want[0])
        np.testing.assert_array_equal(i.cpu().numpy(), want[1])


# --------------------------------------------------------------------------------- statistics
def _stats_case(name):
    rng = np.random.default_rng(16)
    if name == "mixed":
        d = (rng.random(9001) * 3).astype(np.float32)
        d[::5], d[::13] = np.inf, np.nan
    elif name == "all_nan":
        d = np.full(300, np.nan, np.float32)
    elif name == "all_inf":
        d = np.full(4097, np.inf, np.float32)
    elif name == "one":
        d = np.float32([1.5])
    else:
        d = np.zeros(0, np.float32)
    return d


@pytest.mark.parametrize("name", ["mixed", "all_nan", "all_inf", "one", "empty"])
def test_cloud_stats(torch, name):
    from aarmvs import cloud_eval as ce
    d = _stats_case(name)
    thr = (0.5, 1.5, 3.5)
    got = ce.distance_stats(_dev(torch, d), thr)
    again = ce.distance_stats(_dev(torch, d), thr)
    want = ref.stats(d, thr)
    assert got[0] == want[0] and got[2] == want[2] and got[3:] == want[3:]          # the counts are exact
    assert abs(got[1] - want[1]) <= 1e-12 * abs(want[1])                            # math.fsum
    assert got[1] == ref.fixed_order_sum(d)                                         # and the stated order
    assert [math.copysign(1, v) for v in got] == [1.0] * 6
    assert np.float64(got).tobytes() == np.float64(again).tobytes()
    assert ce.distance_stats(_dev(torch, d)) == got[:3]


# --------------------------------------------------------------------------------- voxel centroids
def _voxel_case(name):
    rng = np.random.default_rng(17)
    if name == "random":
        return (rng.random((3000, 3)) * 5).astype(np.float32), 0.5
    if name == "clustered":
        c = rng.random((20, 3)) * 10
        return (c[rng.integers(0, 20, 5000)] + rng.normal(0, 0.2, (5000, 3))).astype(np.float32), 0.25
    if name == "one_point":
        return np.float32([[1.5, -2, 7]]), 1.0
    if name == "all_in_one":
        return (rng.random((4500, 3)) * 0.99).astype(np.float32), 1.0
    if name == "faces":    # points exactly on voxel faces and corners, and duplicates
        return (rng.integers(0, 9, (2000, 3)) * 0.5).astype(np.float32), 1.0
    x = (rng.random((600, 3)) * 3).astype(np.float32)      # "non_finite"
    x[::50, 1] = np.nan
    x[7, 0] = np.inf
    return x, 0.75


@pytest.mark.parametrize("name", ["random", "clustered", "one_point", "all_in_one", "faces", "non_finite"])
def test_voxel_downsample(torch, name):
    from aarmvs import cloud_eval as ce
    x, voxel = _voxel_case(name)
    fin = x[np.isfinite(x).all(1)]
    origin = fin.min(0).astype(np.float64)
    want = ref.voxel_centroids(x, origin, voxel)
    got = ce.voxel_downsample(_dev(torch, x), voxel).cpu().numpy()
    k = ref.keys(x, origin, voxel)
    assert got.shape[0] == np.unique(k[k != ref.NO_KEY]).size == want.shape[0]
    assert got.tobytes() == want.tobytes()
    if name == "all_in_one":
        assert got.shape[0] == 1
    assert ce.voxel_downsample(_dev(torch, x), voxel).cpu().numpy().tobytes() == got.tobytes()


# --------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def scan(torch):
    """The fused synthetic scan at 40x52 with 2 source views, plain and de-duplicated, and its
    ground-truth cloud."""
    from aarmvs import fusion, synthetic as syn
    H, W, nsrc = 40, 52, 2
    depths, cams, _ = syn.fusion_views(H, W, nsrc, seed=0)
    rng = np.random.default_rng(100)
    n = nsrc + 1
    confs = {v: torch.from_numpy(rng.random((H, W)).astype(np.float32)).cuda() for v in range(n)}
    depths = {v: torch.from_numpy(d).cuda() for v, d in enumerate(depths)}
    pairs = [(v, [s for s in range(n) if s != v]) for v in range(n)]
    out = {}
    for form, dedup in (("plain", False), ("dedup", True)):
        out[form] = fusion.fuse_views(pairs, depths, confs, dict(enumerate(cams)), None, 0.35, dedup=dedup)["xyz"]
    out["gt"] = torch.from_numpy(syn.fusion_ground_truth(H, W, nsrc)).cuda()
    assert out["plain"].shape[0] > out["dedup"].shape[0] > 500
    return out


def _same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        g, w = got[k], want[k]
        assert g == w or (isinstance(w, float) and math.isnan(w) and math.isnan(g)), (k, g, w)


@pytest.mark.parametrize("form", ["plain", "dedup"])
@pytest.mark.parametrize("voxel", [None, 1.0])
def test_evaluate_end_to_end(torch, scan, form, voxel):
    """Every field equals the restatement's.  Medians follow torch.median: of an even number of
    values, the LOWER of the two middle ones (the restatement takes that one too)."""
    from aarmvs import cloud_eval as ce
    max_dist, taus = 2.0, (0.25, 0.5, 1.0)
    got = ce.evaluate(scan[form], scan["gt"], max_dist, taus, voxel)
    want = ref.evaluate(scan[form].cpu().numpy(), scan["gt"].cpu().numpy(), max_dist, taus, voxel)
    _same(got, want)
    assert 0 < got["accuracy_mean"] < max_dist and 0 < got["completeness_mean"] < max_dist
    assert 0 < got["fscore@1"] <= 1 and got["recon_nonfinite"] == 0


def test_the_command_line_gives_the_same_dict(torch, scan, tmp_path):
    from aarmvs import cloud_eval as ce, fusion
    a, b, j = str(tmp_path / "recon.ply"), str(tmp_path / "gt.ply"), str(tmp_path / "out.json")
    fusion.write_ply(a, scan["dedup"].cpu().numpy())
    fusion.write_ply(b, scan["gt"].cpu().numpy())
    res = ce.main(["--recon", a, "--gt", b, "--max_dist", "2", "--tau", "0.25", "0.5", "1", "--json", j])
    want = ce.evaluate(scan["dedup"], scan["gt"], 2.0, (0.25, 0.5, 1.0))
    _same(res, want)
    _same(json.load(open(j)), want)


def test_evaluate_on_a_case_worked_out_by_hand(torch):
    """The figures' formulas against numbers worked out by hand (tests/cloud_eval_ref.hand_case), not
    against the restatement's copy of them."""
    from aarmvs import cloud_eval as ce
    recon, gt, max_dist, taus, want = ref.hand_case()
    got = ce.evaluate(_dev(torch, recon), _dev(torch, gt), max_dist, taus)
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-15, abs=0), k
    far = ce.evaluate(_dev(torch, np.float32([[0, 0, 0]])), _dev(torch, np.float32([[50, 0, 0]])), 2.0, (1.0,))
    assert far["precision@1"] == far["recall@1"] == far["fscore@1"] == 0.0
    assert math.isnan(far["accuracy_mean"]) and far["recon_beyond_max_dist"] == far["gt_beyond_max_dist"] == 1
