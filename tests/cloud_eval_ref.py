"""numpy float64 restatement of the point-cloud evaluation's definition (include/aarmvs.h,
"Point-cloud evaluation"): the grid keys, the brute-force truncated nearest neighbour with its tie
rule, the distance statistics and the voxel centroids summed in index order.  No grid search here:
the neighbour is the minimum over ALL in-grid targets, which is what the kernel must equal."""
import math

import numpy as np

NO_KEY = np.iinfo(np.int64).max
AXIS_CELLS = 1 << 21


def cells(xyz, origin, cell):
    """(i [n,3] int64, in_grid [n] bool): i_a = floor(((double)p_a - origin_a) / cell)."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor((p - np.asarray(origin, np.float64)[None, :]) / np.float64(cell))
        ok = np.isfinite(p).all(1) & (t >= 0).all(1) & (t < AXIS_CELLS).all(1)
    i = np.where(ok[:, None], t, 0).astype(np.int64)
    return i, ok


def keys(xyz, origin, cell):
    i, ok = cells(xyz, origin, cell)
    k = (i[:, 2] << 42) | (i[:, 1] << 21) | i[:, 0]
    return np.where(ok, k, NO_KEY).astype(np.int64)


def nn(query, target, origin, cell, max_dist, target_ids=None, chunk=512):
    """(dist float32 [nq], index int32 [nq]) of the definition, by brute force."""
    q = np.asarray(query, np.float32).reshape(-1, 3).astype(np.float64)
    t = np.asarray(target, np.float32).reshape(-1, 3).astype(np.float64)
    ids = np.arange(t.shape[0], dtype=np.int64) if target_ids is None else np.asarray(target_ids, np.int64)
    _, t_in = cells(target, origin, cell)
    _, q_in = cells(query, origin, cell)
    t, ids = t[t_in], ids[t_in]
    md2 = np.float64(np.float32(max_dist)) * np.float64(np.float32(max_dist))
    dist = np.full(q.shape[0], np.inf, np.float32)
    index = np.full(q.shape[0], -1, np.int32)
    q_finite = np.isfinite(q).all(1)
    dist[~q_finite] = np.nan
    rows = np.nonzero(q_in)[0]
    if t.shape[0] == 0:
        return dist, index
    for s in range(0, rows.size, chunk):
        r = rows[s:s + chunk]
        d = q[r, None, :] - t[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        best = d2.min(1)
        # the smallest id among the targets at the minimum
        tie = np.where(d2 == best[:, None], ids[None, :], np.iinfo(np.int64).max).min(1)
        keep = best <= md2
        dist[r[keep]] = np.sqrt(best[keep]).astype(np.float32)
        index[r[keep]] = tie[keep].astype(np.int32)
    return dist, index


def stats(dist, thresholds=()):
    """[finite count, fsum of the finite values, NaN count, counts of finite values < threshold]."""
    d = np.asarray(dist, np.float32)
    fin = np.isfinite(d)
    out = [float(fin.sum()), math.fsum(d[fin].astype(np.float64).tolist()), float(np.isnan(d).sum())]
    for thr in thresholds:
        out.append(float((d[fin] < np.float32(thr)).sum()))
    return out


def _block_sum(v):
    """v [..., 256] float64 -> the block sum as aarmvs_cloud_stats forms it: an xor butterfly inside
    each 64-lane wave (lane 0's value), then the four waves in index order."""
    w = v.reshape(v.shape[:-1] + (4, 64)).copy()
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lane ^ o]
    w = w[..., 0]
    s = w[..., 0]
    for k in range(1, 4):
        s = s + w[..., k]
    return s


def fixed_order_sum(dist):
    """The fp64 sum of the finite values of dist in aarmvs_cloud_stats' order (include/aarmvs.h)."""
    d = np.asarray(dist, np.float32)
    v = np.where(np.isfinite(d), d, np.float32(0)).astype(np.float64)
    nblk = (v.size + 4095) // 4096
    if nblk == 0:
        return 0.0
    v = np.concatenate([v, np.zeros(nblk * 4096 - v.size)]).reshape(nblk, 16, 256)
    acc = np.zeros((nblk, 256))
    for r in range(16):
        acc = acc + v[:, r, :]
    part = _block_sum(acc)                                   # [nblk]
    rounds = (nblk + 255) // 256
    part = np.concatenate([part, np.zeros(rounds * 256 - nblk)]).reshape(rounds, 256)
    acc = np.zeros(256)
    for r in range(rounds):
        acc = acc + part[r]
    return float(_block_sum(acc))


def voxel_centroids(xyz, origin, cell):
    """One point per occupied cell, in key order: the float64 sum of the cell's points in index
    order over their number, cast to float32."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    k = keys(p, origin, cell)
    order = np.argsort(k, kind="stable")
    order = order[k[order] != NO_KEY]
    out = []
    i = 0
    while i < order.size:
        j = i
        s = np.zeros(3, np.float64)
        while j < order.size and k[order[j]] == k[order[i]]:
            s = s + p[order[j]].astype(np.float64)
            j += 1
        out.append((s / np.float64(j - i)).astype(np.float32))
        i = j
    return np.stack(out) if out else np.zeros((0, 3), np.float32)


def grid_for(clouds, max_dist, cell=None):
    """The grid aarmvs.cloud_eval picks, restated: origin = the per-axis minimum of the finite
    points (exact float32 values), cell = max_dist / 4 unless given, enlarged to extent / (2^21 - 2)
    where the extent needs it, 1.0 if that is still 0."""
    pts = [np.asarray(c, np.float32).reshape(-1, 3) for c in clouds]
    pts = [c[np.isfinite(c).all(1)] for c in pts]
    pts = [c for c in pts if c.shape[0]]
    if pts:
        lo = np.min([c.min(0) for c in pts], 0).astype(np.float64)
        hi = np.max([c.max(0) for c in pts], 0).astype(np.float64)
    else:
        lo = hi = np.zeros(3)
    cell = float(np.float32(max_dist)) / 4.0 if cell is None else float(cell)
    cell = max(cell, float((hi - lo).max()) / (AXIS_CELLS - 2))
    if not cell > 0.0:
        cell = 1.0
    return lo, cell


def evaluate(recon, gt, max_dist, thresholds=(), voxel=None):
    """aarmvs.cloud_eval.evaluate restated (medians: the lower middle value, torch.median's)."""
    recon = np.asarray(recon, np.float32).reshape(-1, 3)
    gt = np.asarray(gt, np.float32).reshape(-1, 3)
    if voxel is not None:
        fin = recon[np.isfinite(recon).all(1)]
        origin = fin.min(0).astype(np.float64) if fin.shape[0] else np.zeros(3)
        recon = voxel_centroids(recon, origin, voxel)
    origin, cell = grid_for([recon, gt], max_dist)
    out = dict(n_recon=int(recon.shape[0]), n_gt=int(gt.shape[0]), max_dist=float(max_dist))
    sides = {}
    for name, a, b in (("accuracy", recon, gt), ("completeness", gt, recon)):
        d, _ = nn(a, b, origin, cell, max_dist)
        st = stats(d, thresholds)
        fin = np.sort(d[np.isfinite(d)])
        out[name + "_mean"] = fixed_order_sum(d) / st[0] if st[0] else float("nan")
        out[name + "_median"] = float(fin[(fin.size - 1) // 2]) if fin.size else float("nan")
        sides[name] = (st, d.shape[0])
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


def hand_case():
    """A case small enough to work out by hand: (recon, gt, max_dist, thresholds, expected fields).
    recon -> gt: 0.5, 0, beyond (6 > 2), NaN.  gt -> recon: 0.5, 0, beyond (3 > 2), 0.125."""
    recon = np.float32([[0, 0, 0], [1, 0, 0], [10, 0, 0], [np.nan, 0, 0]])
    gt = np.float32([[0, 0, 0.5], [1, 0, 0], [4, 0, 0], [1, 0, 0.125]])
    p25, r25, p1, r1 = 1 / 3, 2 / 4, 2 / 3, 3 / 4          # of 3 finite recon points, of 4 gt points
    want = {"n_recon": 4, "n_gt": 4, "max_dist": 2.0,
            "accuracy_mean": 0.25, "accuracy_median": 0.0,              # of {0, 0.5}: the lower middle value
            "completeness_mean": 0.625 / 3, "completeness_median": 0.125,
            "overall": 0.5 * (0.25 + 0.625 / 3),
            "recon_nonfinite": 1, "recon_beyond_max_dist": 1, "gt_nonfinite": 0, "gt_beyond_max_dist": 1,
            "precision@0.25": p25, "recall@0.25": r25, "fscore@0.25": 0.4,
            "precision@1": p1, "recall@1": r1, "fscore@1": 12 / 17}
    return recon, gt, 2.0, (0.25, 1.0), want
