"""Point-cloud evaluation on the GPU (include/aarmvs.h, "Point-cloud evaluation"):
nearest-neighbour distances between two clouds, voxel down-sampling, and the plain accuracy /
completeness (DTU-style) and precision / recall / F-score (Tanks-and-Temples-style) figures.

``evaluate_dtu`` adds the DTU protocol (include/aarmvs.h, "DTU protocol"):
``reducePts`` as ``thin`` (the greedy walk run as parallel rounds), the observation mask and the
ground-plane cut as ``regions``, from the scan's ``ObsMask`` / ``Plane`` files.  NOT implemented:
Tanks and Temples' alignment and cropping, which need that dataset's files.  Sorting is
``torch.sort`` (plumbing); the keys, the query, the statistics, the centroids, the thinning rounds
and the region flags are HIP kernels, and there is no CPU fallback: CPU tensors are refused.

    python -m aarmvs.cloud_eval --recon A.ply --gt B.ply --max_dist 20 --tau 1 2 5 [--voxel V] [--json out.json]
    python -m aarmvs.cloud_eval --protocol dtu --recon A.ply --gt stl.ply --obs_mask M.mat --plane P.mat
                                [--thin 0.2 --patch 60 --max_dist 20 --seed 0 --json out.json]
"""
from __future__ import annotations

import ctypes
import json
import math
import re

import numpy as np
import torch

from . import _lib
from ._lib import AarmvsError, check, lib

AXIS_CELLS = 1 << _lib.CLOUD_AXIS_BITS


def _cloud(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2
            and t.shape[1] == 3):
        raise AarmvsError(f"aarmvs: {what} must be a CUDA float32 [n,3] tensor (there is no CPU fallback)")
    if t.shape[0] >= 1 << 31:
        raise ValueError(f"aarmvs: {what} has 2^31 points or more")
    return t.contiguous()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bounds(clouds):
    """Per-axis (min, max) of the finite points of the clouds as float64 numpy [3] (zeros if none)."""
    lo, hi = None, None
    for c in clouds:
        fin = c[torch.isfinite(c).all(1)]
        if fin.shape[0] == 0:
            continue
        a, b = fin.min(0).values.double().cpu().numpy(), fin.max(0).values.double().cpu().numpy()
        lo = a if lo is None else np.minimum(lo, a)
        hi = b if hi is None else np.maximum(hi, b)
    if lo is None:
        lo = hi = np.zeros(3)
    return lo, hi


def pick_grid(clouds, max_dist, cell=None):
    """(origin float64 [3], cell): every finite point of the clouds is in the grid.  origin = the
    per-axis minimum; cell = max_dist / 4 unless given, enlarged to extent / (2^21 - 2) where the
    2^21-cells-per-axis limit requires it (1.0 if that is still 0)."""
    lo, hi = _bounds(clouds)
    cell = float(max_dist) / 4.0 if cell is None else float(cell)
    if not (math.isfinite(cell) and cell >= 0.0):
        raise ValueError("aarmvs: cell must be finite and >= 0")
    cell = max(cell, float((hi - lo).max()) / (AXIS_CELLS - 2))
    if not cell > 0.0:
        cell = 1.0
    return lo, cell


def cloud_keys(xyz, origin, cell):
    """int64 [n] grid keys of a CUDA float32 [n,3] cloud (``aarmvs_cloud_keys``)."""
    xyz = _cloud(xyz, "xyz")
    keys = torch.empty(xyz.shape[0], dtype=torch.int64, device=xyz.device)
    o = (ctypes.c_double * 3)(*[float(v) for v in origin])
    with torch.cuda.device(xyz.device):
        check(lib().aarmvs_cloud_keys(xyz.data_ptr(), xyz.shape[0], o, float(cell), keys.data_ptr(), _stream()),
              "cloud_keys")
    return keys


def _sorted_by_key(xyz, origin, cell):
    keys, perm = torch.sort(cloud_keys(xyz, origin, cell), stable=True)
    return xyz[perm].contiguous(), keys, perm


def nn_sorted(query, target_sorted, target_keys, target_ids, origin, cell, max_dist, want_index=True):
    """``aarmvs_cloud_nn`` on a key-sorted target: (dist float32 [nq], index int32 [nq] or None), in
    the order of ``query``."""
    dev = query.device
    nq = query.shape[0]
    dist = torch.empty(nq, dtype=torch.float32, device=dev)
    index = torch.empty(nq, dtype=torch.int32, device=dev) if want_index else None
    a = _lib.CloudNnArgs()
    a.query, a.target, a.target_keys = query.data_ptr(), target_sorted.data_ptr(), target_keys.data_ptr()
    a.target_ids = None if target_ids is None else target_ids.data_ptr()
    a.nq, a.m = nq, target_sorted.shape[0]
    a.origin[0], a.origin[1], a.origin[2] = (float(v) for v in origin)
    a.cell, a.max_dist = float(cell), float(max_dist)
    a.dist_out = dist.data_ptr()
    a.index_out = None if index is None else index.data_ptr()
    with torch.cuda.device(dev):
        check(lib().aarmvs_cloud_nn(ctypes.byref(a), _stream()), "cloud_nn")
    return dist, index


def _checked_grid(a, b, max_dist, cell=None):
    """(max_dist rounded to float32, origin, cell) for two clouds on one device, or an error."""
    if a.device != b.device:
        raise AarmvsError("aarmvs: the two clouds are on different devices")
    max_dist = float(np.float32(max_dist))
    if not (math.isfinite(max_dist) and max_dist >= 0.0):
        raise ValueError("aarmvs: max_dist must be finite and >= 0")
    origin, cell = pick_grid([a, b], max_dist, cell)
    if max_dist / cell > _lib.CLOUD_MAX_RINGS:
        raise ValueError(f"aarmvs: max_dist / cell = {max_dist / cell:g} exceeds the ring limit "
                         f"{_lib.CLOUD_MAX_RINGS}")
    return max_dist, origin, cell


def nn_distance(query, target, max_dist, cell=None):
    """For every point of ``query`` the distance to its nearest point of ``target`` within
    ``max_dist`` and that point's index in ``target``: (dist float32 [nq], index int32 [nq]); +inf /
    -1 where there is none, NaN / -1 for a query with a non-finite coordinate.  Exact, ties to the
    lowest index.  The grid holds every finite point of both clouds; ``cell`` defaults to
    ``max_dist / 4`` and grows where the 2^21-cells-per-axis limit requires; ValueError when
    ``max_dist / cell`` would exceed the ring limit."""
    query, target = _cloud(query, "query"), _cloud(target, "target")
    max_dist, origin, cell = _checked_grid(query, target, max_dist, cell)
    t_sorted, t_keys, t_perm = _sorted_by_key(target, origin, cell)
    q_sorted, _, q_perm = _sorted_by_key(query, origin, cell)
    d_s, i_s = nn_sorted(q_sorted, t_sorted, t_keys, t_perm.to(torch.int32), origin, cell, max_dist)
    dist, index = torch.empty_like(d_s), torch.empty_like(i_s)
    dist[q_perm] = d_s
    index[q_perm] = i_s
    return dist, index


def distance_stats(dist, thresholds=()):
    """``aarmvs_cloud_stats`` of a CUDA float32 [n] tensor as a list of floats: the number of finite
    values, their fixed-order fp64 sum, the number of NaN, then per threshold the number of finite
    values below it."""
    if not (isinstance(dist, torch.Tensor) and dist.is_cuda and dist.dtype == torch.float32 and dist.dim() == 1):
        raise AarmvsError("aarmvs: dist must be a CUDA float32 [n] tensor")
    thresholds = [float(t) for t in thresholds]
    if len(thresholds) > _lib.MAX_THRESHOLDS:
        raise ValueError(f"aarmvs: at most {_lib.MAX_THRESHOLDS} thresholds")
    dist = dist.contiguous()
    n, dev = dist.shape[0], dist.device
    out = torch.empty(3 + len(thresholds), dtype=torch.float64, device=dev)
    scratch = torch.empty(max(1, lib().aarmvs_cloud_stats_scratch_bytes(n)), dtype=torch.uint8, device=dev)
    thr = (ctypes.c_float * max(1, len(thresholds)))(*thresholds)
    with torch.cuda.device(dev):
        check(lib().aarmvs_cloud_stats(dist.data_ptr(), n, thr, len(thresholds), out.data_ptr(),
                                       scratch.data_ptr(), _stream()), "cloud_stats")
    return out.cpu().tolist()


def voxel_downsample(xyz, voxel):
    """One point per occupied voxel of side ``voxel`` (grid origin: the per-axis minimum of the finite
    points): the float64 mean of the voxel's points in their original order, as float32 [n',3], in
    key order (z-major).  Points with a non-finite coordinate are dropped."""
    xyz = _cloud(xyz, "xyz")
    voxel = float(voxel)
    if not (math.isfinite(voxel) and voxel > 0.0):
        raise ValueError("aarmvs: voxel must be finite and > 0")
    lo, hi = _bounds([xyz])
    if float((hi - lo).max()) / voxel >= AXIS_CELLS - 1:
        raise ValueError("aarmvs: the cloud spans 2^21 voxels or more along an axis")
    s_xyz, s_keys, _ = _sorted_by_key(xyz, lo, voxel)
    n, dev = xyz.shape[0], xyz.device
    out = torch.empty(n, 3, dtype=torch.float32, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    work = torch.empty(max(1, lib().aarmvs_cloud_voxel_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib().aarmvs_cloud_voxel_centroids(s_xyz.data_ptr(), s_keys.data_ptr(), n, out.data_ptr(), n,
                                                 count.data_ptr(), work.data_ptr(), _stream()),
              "cloud_voxel_centroids")
    return out[:int(count.item())]


def _median(dist):
    fin = dist[torch.isfinite(dist)]
    return float(torch.median(fin)) if fin.shape[0] else float("nan")   # the lower middle value


def evaluate(recon, gt, max_dist, thresholds=(), voxel=None):
    """Compare a reconstructed cloud with a ground-truth cloud (CUDA float32 [n,3] each).  ``voxel``:
    down-sample ``recon`` first.  Distances are truncated at ``max_dist`` in both directions.
    DTU-style, over the distances <= max_dist: ``accuracy_mean`` / ``accuracy_median`` (recon -> gt),
    ``completeness_mean`` / ``completeness_median`` (gt -> recon), ``overall`` = the mean of the two
    means.  Tanks-and-Temples-style, per tau (<= max_dist): ``precision@tau`` = the share of recon
    points nearer than tau to gt, ``recall@tau`` = the share of gt points nearer than tau to recon,
    ``fscore@tau`` = 2PR / (P + R) (0 when P + R == 0); the denominators count all points with finite
    coordinates.  Also ``n_recon`` (after the down-sampling), ``n_gt``, ``recon_beyond_max_dist``,
    ``gt_beyond_max_dist``, ``recon_nonfinite`` and ``gt_nonfinite``.  Plain figures, not the
    official protocols (module docstring)."""
    thresholds = [float(t) for t in thresholds]
    if any(not t <= float(max_dist) for t in thresholds):
        raise ValueError("aarmvs: every tau must be <= max_dist (distances are truncated there)")
    recon, gt = _cloud(recon, "recon"), _cloud(gt, "gt")
    if voxel is not None:
        recon = voxel_downsample(recon, voxel)
    out = dict(n_recon=int(recon.shape[0]), n_gt=int(gt.shape[0]), max_dist=float(max_dist))
    # one grid for both directions, and each cloud keyed and sorted once
    md, origin, cell = _checked_grid(recon, gt, max_dist)
    r_sorted, r_keys, r_perm = _sorted_by_key(recon, origin, cell)
    g_sorted, g_keys, g_perm = _sorted_by_key(gt, origin, cell)
    sides = {}
    for name, q_sorted, q_perm, t_sorted, t_keys in (("accuracy", r_sorted, r_perm, g_sorted, g_keys),
                                                     ("completeness", g_sorted, g_perm, r_sorted, r_keys)):
        d_s, _ = nn_sorted(q_sorted, t_sorted, t_keys, None, origin, cell, md, want_index=False)
        dist = torch.empty_like(d_s)
        dist[q_perm] = d_s       # the caller's order: the statistics' sum order is defined on it
        st = distance_stats(dist, thresholds)
        out[name + "_mean"] = st[1] / st[0] if st[0] else float("nan")
        out[name + "_median"] = _median(dist)
        sides[name] = (st, int(dist.shape[0]))
    out["overall"] = 0.5 * (out["accuracy_mean"] + out["completeness_mean"])
    for which, name in (("recon", "accuracy"), ("gt", "completeness")):
        st, n = sides[name]
        out[which + "_nonfinite"] = int(st[2])
        out[which + "_beyond_max_dist"] = int(n - st[2] - st[0])
    for k, tau in enumerate(thresholds):
        pr = []
        for name in ("accuracy", "completeness"):
            st, n = sides[name]
            den = n - st[2]
            pr.append(st[3 + k] / den if den else 0.0)
        p, r = pr
        out[f"precision@{tau:g}"], out[f"recall@{tau:g}"] = p, r
        out[f"fscore@{tau:g}"] = 2.0 * p * r / (p + r) if p + r > 0 else 0.0
    return out


# ---------------------------------------------------------------------------------
# The DTU protocol (include/aarmvs.h, "DTU protocol")
# ---------------------------------------------------------------------------------
IN_BOX, IN_OBS, ABOVE = 1, 2, 4


def _ranks(order, seed, n):
    """The int32 [n] ranks of ``thin``: a seeded permutation, the input order, or the caller's own."""
    if isinstance(order, str):
        if order == "random":
            return torch.from_numpy(np.random.default_rng(seed).permutation(n).astype(np.int32))
        if order == "input":
            return torch.arange(n, dtype=torch.int32)
        raise ValueError('aarmvs: order must be "random", "input" or an int32 rank tensor')
    rank = torch.as_tensor(order)
    if rank.dtype != torch.int32 or rank.dim() != 1 or rank.shape[0] != n:
        raise ValueError("aarmvs: the ranks must be an int32 [n] tensor")
    if torch.unique(rank).shape[0] != n:
        raise ValueError("aarmvs: the ranks must be distinct")
    return rank


def thin(xyz, radius, order="random", seed=0, rounds_per_call=8):
    """DTU's ``reducePts``: walk the points in ascending rank, keep a point, drop every point within
    ``radius`` of it (inclusive).  Returns (kept_index int64 [n'] ascending, in the caller's order;
    the number of rounds to the fixpoint).  ``order``: "random" (ranks =
    ``numpy.random.default_rng(seed).permutation(n)``), "input" (``arange(n)``) or an int32 [n]
    tensor of distinct ranks.  Points with a non-finite coordinate are dropped.  The walk runs as
    parallel rounds (``aarmvs_cloud_thin``, ``rounds_per_call`` per call) whose fixpoint IS the
    sequential result; the round count does not depend on ``rounds_per_call``.  The host reads the
    number of undecided points back after each call."""
    radius = float(np.float32(radius))
    if not (math.isfinite(radius) and radius > 0.0):
        raise ValueError("aarmvs: radius must be finite and > 0")
    rounds_per_call = int(rounds_per_call)
    if rounds_per_call < 1:
        raise ValueError("aarmvs: rounds_per_call must be >= 1")
    if isinstance(xyz, torch.Tensor) and xyz.dim() == 2:
        rank = _ranks(order, seed, xyz.shape[0])
    xyz = _cloud(xyz, "xyz")
    n, dev = xyz.shape[0], xyz.device
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=dev), 0
    lo, hi = _bounds([xyz])
    cell = max(radius, float((hi - lo).max()) / (AXIS_CELLS - 2))
    s_xyz, s_keys, perm = _sorted_by_key(xyz, lo, cell)
    state, rounds = thin_sorted(s_xyz, s_keys, rank.to(dev)[perm].contiguous(), lo, cell, radius, rounds_per_call)
    return torch.sort(perm[state == 1]).values, rounds


def thin_sorted(s_xyz, s_keys, s_rank, origin, cell, radius, rounds_per_call=8, log=None):
    """``aarmvs_cloud_thin`` on a key-sorted cloud until nothing is undecided: (state uint8 [n] in the
    sorted layout, 1 kept / 2 removed; the number of rounds to the fixpoint).  ``log``: a list that
    receives per call (rounds run, undecided points left, device milliseconds of the call)."""
    n, dev = s_xyz.shape[0], s_xyz.device
    state =[torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2)]
    remaining = torch.empty(2, dtype=torch.int64, device=dev)
    scratch = torch.empty(max(1, lib().aarmvs_cloud_thin_scratch_bytes(n)), dtype=torch.uint8, device=dev)
    a = _lib.CloudThinArgs()
    a.xyz, a.keys, a.rank, a.n = s_xyz.data_ptr(), s_keys.data_ptr(), s_rank.data_ptr(), n
    a.origin[0], a.origin[1], a.origin[2] = (float(v) for v in origin)
    a.cell, a.r = float(cell), float(radius)
    a.state[0], a.state[1] = state[0].data_ptr(), state[1].data_ptr()
    a.remaining, a.scratch = remaining.data_ptr(), scratch.data_ptr()
    a.init, a.which = 1, 0
    rounds = launched = 0
    with torch.cuda.device(dev):
        while True:
            if launched >= n:
                raise AarmvsError(f"aarmvs: thinning did not reach its fixpoint in n = {n} rounds")
            k = min(rounds_per_call, n - launched)
            if log is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            check(lib().aarmvs_cloud_thin(ctypes.byref(a), k, _stream()), "cloud_thin")
            if log is not None:
                e1.record()
            launched += k
            a.init, a.which = 0, (a.which + k) & 1
            left, used = remaining.cpu().tolist()      # the one wait for the device per call
            rounds += used
            if log is not None:
                log.append((k, left, e0.elapsed_time(e1)))
            if left == 0:
                break
    return state[a.which], rounds


_thin_points = thin   # evaluate_dtu's ``thin`` parameter is the radius


def regions(xyz, obs_mask=None, bb=None, res=None, patch=60.0, plane=None):
    """uint8 [n] flags of a CUDA float32 [n,3] cloud (``aarmvs_cloud_regions``): ``IN_BOX`` (1) inside
    ``bb`` [2,3] widened by ``patch`` below and ``2 * patch`` above, ``IN_OBS`` (2) in the box and on a
    set voxel of ``obs_mask`` (uint8 [nx,ny,nz], voxel = rint((p - bb[0]) / res)), ``ABOVE`` (4)
    on the positive side of ``plane`` [4].  A bit whose input is None is 0; points with a non-finite
    coordinate get 0."""
    xyz = _cloud(xyz, "xyz")
    n, dev = xyz.shape[0], xyz.device
    if obs_mask is not None and (bb is None or res is None):
        raise ValueError("aarmvs: obs_mask needs bb and res")
    mask = dims = None
    if obs_mask is not None:
        mask = torch.as_tensor(obs_mask)
        if mask.dim() != 3:
            raise ValueError("aarmvs: obs_mask must be [nx,ny,nz]")
        mask = (mask != 0).to(device=dev, dtype=torch.uint8).contiguous()
        dims = (ctypes.c_int * 3)(*mask.shape)
    bbv = None if bb is None else (ctypes.c_double * 6)(*np.asarray(bb, np.float64).reshape(6).tolist())
    pv = None if plane is None else (ctypes.c_double * 4)(*np.asarray(plane, np.float64).reshape(4).tolist())
    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib().aarmvs_cloud_regions(xyz.data_ptr(), n, None if mask is None else mask.data_ptr(), dims, bbv,
                                         1.0 if res is None else float(res), float(patch), pv, flags.data_ptr(),
                                         _stream()), "cloud_regions")
    return flags


def _load(path, names):
    if str(path).endswith(".npz"):
        with np.load(path) as f:
            return {k: f[k] for k in names}
    try:
        from scipy.io import loadmat
    except ImportError as e:
        raise ImportError("aarmvs: reading a .mat file needs scipy (scipy.io.loadmat); convert the file to "
                          ".npz with the same field names to do without it") from e
    f = loadmat(path)
    return {k: f[k] for k in names}


def read_dtu_mask(path):
    """DTU's ``ObsMask/ObsMaskN_10.mat`` (or an .npz with the same fields ``ObsMask``, ``BB``, ``Res``):
    a dict of ``obs_mask`` uint8 [nx,ny,nz] C-contiguous (0/1), ``bb`` float64 [2,3], ``res`` float."""
    f = _load(path, ("ObsMask", "BB", "Res"))
    m = np.asarray(f["ObsMask"])
    if m.ndim != 3:
        raise ValueError(f"read_dtu_mask: ObsMask of {path} is not 3-D")
    return dict(obs_mask=np.ascontiguousarray(m != 0).astype(np.uint8),
                bb=np.ascontiguousarray(np.asarray(f["BB"], np.float64).reshape(2, 3)),
                res=float(np.asarray(f["Res"], np.float64).reshape(-1)[0]))


def read_dtu_plane(path):
    """DTU's ``ObsMask/PlaneN.mat`` (or an .npz with the field ``P``): the plane as float64 [4]."""
    return np.ascontiguousarray(np.asarray(_load(path, ("P",))["P"], np.float64).reshape(4))


def _nn_in_order(query, target, origin, cell, max_dist):
    """Distances of ``nn_sorted`` in the order of ``query`` with those == max_dist set to +inf: the
    protocol's truncation is strict."""
    t_sorted, t_keys, _ = _sorted_by_key(target, origin, cell)
    q_sorted, _, q_perm = _sorted_by_key(query, origin, cell)
    d_s, _ = nn_sorted(q_sorted, t_sorted, t_keys, None, origin, cell, max_dist, want_index=False)
    dist = torch.empty_like(d_s)
    dist[q_perm] = d_s
    return torch.where(dist >= max_dist, torch.full_like(dist, float("inf")), dist)


def evaluate_dtu(recon, gt, obs_mask, bb, res, plane, thin=0.2, patch=60.0, max_dist=20.0, seed=0, order="random"):
    """The DTU evaluation protocol (include/aarmvs.h, "DTU protocol") of a reconstructed cloud
    against a scan's ground truth (CUDA float32 [n,3] each) with the scan's observation mask
    (``obs_mask``, ``bb``, ``res``: ``read_dtu_mask``) and ground plane (``read_dtu_plane``):
      1. ``recon`` is thinned at radius ``thin`` (``thin(recon, thin, order, seed)``);
      2. ``n_in_box`` / ``n_in_obs`` of the thinned points are IN_BOX / IN_OBS;
      3. accuracy: from every IN_OBS point the distance to ``gt``; mean and median over the distances
         strictly below ``max_dist``;
      4. completeness: from every ABOVE point of ``gt`` the distance to the IN_BOX points; the same;
      5. ``overall`` = the mean of the two means.
    The means are ``aarmvs_cloud_stats``' fixed-order sums over the counts in the caller's point
    order, the medians the lower middle value.  Restates the published MATLAB evaluation as its
    common Python port does; parity with the MATLAB code itself is not pinned."""
    recon, gt = _cloud(recon, "recon"), _cloud(gt, "gt")
    kept, rounds = _thin_points(recon, thin, order, seed)
    down = recon[kept]
    flags = regions(down, obs_mask, bb, res, patch)
    data_in, data_in_obs = down[(flags & IN_BOX) != 0], down[(flags & IN_OBS) != 0]
    gt_above = gt[(regions(gt, plane=plane) & ABOVE) != 0]
    out = dict(n_recon=int(recon.shape[0]), n_thinned=int(down.shape[0]), n_in_box=int(data_in.shape[0]),
               n_in_obs=int(data_in_obs.shape[0]), n_gt=int(gt.shape[0]), n_gt_above=int(gt_above.shape[0]),
               thin_rounds=int(rounds))
    md, origin, cell = _checked_grid(data_in, gt, max_dist)
    for name, which, query, target in (("accuracy", "recon", data_in_obs, gt), ("completeness", "gt", gt_above, data_in)):
        dist = _nn_in_order(query, target, origin, cell, md)
        st = distance_stats(dist)
        out[name + "_mean"] = st[1] / st[0] if st[0] else float("nan")
        out[name + "_median"] = _median(dist)
        out[which + "_beyond_max_dist"] = int(dist.shape[0] - st[2] - st[0])
    out["overall"] = 0.5 * (out["accuracy_mean"] + out["completeness_mean"])
    out["recon_nonfinite"] = int((~torch.isfinite(recon).all(1)).sum())
    out["gt_nonfinite"] = int((~torch.isfinite(gt).all(1)).sum())
    out.update(thin=float(np.float32(thin)), patch=float(patch), max_dist=float(max_dist), seed=int(seed),
               order=order if isinstance(order, str) else "ranks")
    return out


# ---------------------------------------------------------------------------------
# PLY reader (numpy only): what aarmvs.fusion.write_ply writes, and plain ascii / binary x y z
# ---------------------------------------------------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2",
              "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4",
              "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path):
    """Read the vertices of an ascii or binary little-endian PLY: a dict of ``xyz`` float32 [n,3],
    ``normals`` float32 [n,3] or None (nx, ny, nz) and ``rgb`` uint8 [n,3] or None (red, green,
    blue).  ``write_ply(path, **read_ply(path))`` rewrites a file of ``aarmvs.fusion.write_ply``
    byte for byte.  Elements after the vertices (faces) are ignored; list properties in the vertex
    element are not supported."""
    with open(path, "rb") as f:
        data = f.read()
    # the header ends at a LINE that is end_header (the word may also occur in a comment)
    m = re.search(rb"^end_header[ \t]*\r?\n", data, re.MULTILINE)
    if not data.startswith(b"ply") or m is None:
        raise ValueError(f"read_ply: {path} is not a PLY file")
    end, body = m.start(), data[m.end():]
    fmt, n, props, element = None, 0, [], None
    for line in data[:end].decode("ascii").splitlines()[1:]:
        w = line.split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            if element is None and w[1] != "vertex":
                raise ValueError("read_ply: the vertex element must come first")
            element = w[1]
            if element == "vertex":
                n = int(w[2])
        elif w[0] == "property" and element == "vertex":
            if w[1] == "list" or w[1] not in _PLY_TYPES:
                raise ValueError(f"read_ply: unsupported vertex property: {line}")
            props.append((w[2], _PLY_TYPES[w[1]]))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"read_ply: unsupported format {fmt!r}")
    names = [p[0] for p in props]
    if not all(a in names for a in "xyz"):
        raise ValueError("read_ply: the vertices have no x, y, z")
    if fmt == "ascii":
        rows = [r for r in body.decode("ascii").split("\n") if r.strip()][:n]
        if len(rows) < n or any(len(r.split()) < len(props) for r in rows):
            raise ValueError("read_ply: the file is shorter than its header says")
        tab = np.array([r.split()[:len(props)] for r in rows], dtype=np.float64).reshape(n, len(props))
        col = {name: tab[:, k].astype(t) for k, (name, t) in enumerate(props)}
    else:
        dt = np.dtype([(name, "<" + t) for name, t in props])
        if len(body) < n * dt.itemsize:
            raise ValueError("read_ply: the file is shorter than its header says")
        v = np.frombuffer(body, dtype=dt, count=n)
        col = {name: v[name] for name in names}

    def take(fields, dtype):
        if not all(a in col for a in fields):
            return None
        return np.ascontiguousarray(np.stack([col[a] for a in fields], 1).astype(dtype, copy=False))

    return dict(xyz=take(("x", "y", "z"), np.float32), normals=take(("nx", "ny", "nz"), np.float32),
                rgb=take(("red", "green", "blue"), np.uint8))


# ---------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------
def build_parser():
    import argparse
    p = argparse.ArgumentParser(prog="python -m aarmvs.cloud_eval",
                                description="Accuracy, completeness and F-score of a reconstructed cloud against "
                                            "a ground-truth cloud: plain figures, or with --protocol dtu the DTU "
                                            "protocol (not Tanks and Temples' alignment and cropping)")
    p.add_argument("--recon", required=True, help="the reconstructed cloud (PLY)")
    p.add_argument("--gt", required=True, help="the ground-truth cloud (PLY)")
    p.add_argument("--max_dist", type=float, default=None,
                   help="distances are truncated here (required; with --protocol dtu: default 20)")
    p.add_argument("--tau", type=float, nargs="*", default=[], help="F-score thresholds (<= max_dist)")
    p.add_argument("--voxel", type=float, default=None, help="down-sample the reconstruction to this voxel size")
    p.add_argument("--json", default=None, help="also write the result here")
    p.add_argument("--device", default="cuda")
    p.add_argument("--protocol", choices=["dtu"], default=None,
                   help="dtu: the DTU protocol (thinning, observation mask, plane cut) instead of the plain figures")
    p.add_argument("--obs_mask", default=None, help="dtu: ObsMask/ObsMaskN_10.mat (or .npz: ObsMask, BB, Res)")
    p.add_argument("--plane", default=None, help="dtu: ObsMask/PlaneN.mat (or .npz: P)")
    p.add_argument("--thin", type=float, default=0.2, help="dtu: the thinning radius")
    p.add_argument("--patch", type=float, default=60.0, help="dtu: the margin around the mask's box")
    p.add_argument("--seed", type=int, default=0, help="dtu: the seed of the thinning order")
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.protocol is None and args.max_dist is None:
        parser.error("the following arguments are required: --max_dist")
    if args.protocol == "dtu" and (args.obs_mask is None or args.plane is None):
        parser.error("--protocol dtu needs --obs_mask and --plane")
    dev = torch.device(args.device)
    recon = torch.from_numpy(read_ply(args.recon)["xyz"]).to(dev)
    gt = torch.from_numpy(read_ply(args.gt)["xyz"]).to(dev)
    if args.protocol == "dtu":
        m = read_dtu_mask(args.obs_mask)
        res = evaluate_dtu(recon, gt, m["obs_mask"], m["bb"], m["res"], read_dtu_plane(args.plane), thin=args.thin,
                           patch=args.patch, max_dist=20.0 if args.max_dist is None else args.max_dist,
                           seed=args.seed)
    else:
        res = evaluate(recon, gt, args.max_dist, args.tau, args.voxel)
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    main()
