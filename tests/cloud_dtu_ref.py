"""numpy float64 restatement of the DTU protocol's definition (include/aarmvs.h, "DTU protocol"): the
greedy thinning as the literal sequential walk and as the round rule, the region tests, and
evaluate_dtu on top of cloud_eval_ref's brute-force nearest neighbour and fixed-order sum."""
import numpy as np

import cloud_eval_ref as ref

UNDECIDED, KEPT, REMOVED = 0, 1, 2


def thin_grid(xyz, r):
    """The grid aarmvs.cloud_eval.thin picks: origin = the per-axis minimum of the finite points,
    cell = max(r, extent / (2^21 - 2))."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    fin = p[np.isfinite(p).all(1)]
    if fin.shape[0] == 0:
        return np.zeros(3), float(np.float32(r))
    lo, hi = fin.min(0).astype(np.float64), fin.max(0).astype(np.float64)
    return lo, max(float(np.float32(r)), float((hi - lo).max()) / (ref.AXIS_CELLS - 2))


def in_grid(xyz, r):
    origin, cell = thin_grid(xyz, r)
    return ref.cells(xyz, origin, cell)[1]


_PAIRS = {}


def neighbour_pairs(xyz, r, chunk=256):
    """(a, b) int64 arrays: every ordered pair a != b of in-grid points with d2 <= (double)r (double)r,
    by brute force on float64 (d2 = (dx dx + dy dy) + dz dz).  The points are visited in x order and a
    chunk is compared with the slab of points whose x lies within r (1 + 1e-9) of the chunk's: a pair
    outside the slab has dx dx > r r already.  Cached per (cloud, r): the tests share it."""
    p32 = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
    key = (p32.tobytes(), float(np.float32(r)))
    if key in _PAIRS:
        return _PAIRS[key]
    r64 = np.float64(np.float32(r))
    r2, slack = r64 * r64, r64 * (1 + 1e-9)
    ids = np.nonzero(in_grid(p32, r))[0]
    p = p32[ids].astype(np.float64)
    order = np.argsort(p[:, 0], kind="stable")
    p, ids = p[order], ids[order]
    x = p[:, 0]
    out_a, out_b = [], []
    for s in range(0, p.shape[0], chunk):
        e = min(s + chunk, p.shape[0])
        lo, hi = np.searchsorted(x, x[s] - slack, "left"), np.searchsorted(x, x[e - 1] + slack, "right")
        d = p[s:e, None, :] - p[None, lo:hi, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        a, b = np.nonzero(d2 <= r2)
        a, b = a + s, b + lo
        keep = a != b
        out_a.append(ids[a[keep]])
        out_b.append(ids[b[keep]])
    a = np.concatenate(out_a) if out_a else np.zeros(0, np.int64)
    b = np.concatenate(out_b) if out_b else np.zeros(0, np.int64)
    if len(_PAIRS) > 16:
        _PAIRS.clear()
    _PAIRS[key] = (a, b)
    return a, b


def _ranks(rank, n):
    rank = np.asarray(rank, np.int64).reshape(-1)
    assert rank.shape[0] == n and np.unique(rank).size == n
    return rank


def thin_sequential(xyz, r, rank):
    """kept bool [n]: the literal walk in ascending rank -- keep a point that is still there, delete
    every neighbour of it."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = p.shape[0]
    rank = _ranks(rank, n)
    a, b = neighbour_pairs(p, r)
    order = np.argsort(a, kind="stable")
    a, b = a[order], b[order]
    start = np.searchsorted(a, np.arange(n + 1))
    gone = ~in_grid(p, r)
    kept = np.zeros(n, bool)
    for i in np.argsort(rank, kind="stable"):
        if gone[i]:
            continue
        kept[i] = True
        gone[b[start[i]:start[i + 1]]] = True
    return kept


def round_step(state, a, b, n, rule="definition"):
    """One round of the rule on the lower-ranked-neighbour pairs (a: the point, b: its lower-ranked
    neighbour): reads `state`, returns the new array.  `rule` selects a MUTANT for the tests:
    "undecided_as_removed" keeps a point whose lower neighbours are merely not kept."""
    has_kept = np.bincount(a[state[b] == KEPT], minlength=n) > 0
    has_und = np.bincount(a[state[b] == UNDECIDED], minlength=n) > 0
    if rule == "undecided_as_removed":
        has_und[:] = False
    new = state.copy()
    und = state == UNDECIDED
    new[und & has_kept] = REMOVED
    new[und & ~has_kept & ~has_und] = KEPT
    return new


def thin_rounds(xyz, r, rank, rule="definition", max_rounds=None):
    """(kept bool [n], rounds): the round rule with ping-pong state until nothing is undecided.
    `rule`: "definition", or a mutant -- "ignore_rank" takes every neighbour for a lower-ranked one
    (it need not reach a fixpoint: `max_rounds` stops it), "undecided_as_removed" (round_step)."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = p.shape[0]
    rank = _ranks(rank, n)
    a, b = neighbour_pairs(p, r)
    if rule != "ignore_rank":
        lower = rank[b] < rank[a]
        a, b = a[lower], b[lower]
    state = np.where(in_grid(p, r), UNDECIDED, REMOVED).astype(np.uint8)
    rounds = 0
    while (state == UNDECIDED).any() and (max_rounds is None or rounds < max_rounds):
        state = round_step(state, a, b, n, rule)
        rounds += 1
    return state == KEPT, rounds


def regions(xyz, obs_mask=None, bb=None, res=None, patch=60.0, plane=None):
    """uint8 [n]: bit 0 IN_BOX, bit 1 IN_OBS, bit 2 ABOVE; a bit whose input is None is 0."""
    p32 = np.asarray(xyz, np.float32).reshape(-1, 3)
    fin = np.isfinite(p32).all(1)
    p = np.where(fin[:, None], p32, np.float32(0)).astype(np.float64)
    flags = np.zeros(p.shape[0], np.uint8)
    if bb is not None:
        bb = np.asarray(bb, np.float64).reshape(2, 3)
        patch = np.float64(patch)
        in_box = fin & (p >= bb[0] - patch).all(1) & (p < bb[1] + np.float64(2.0) * patch).all(1)
        flags |= in_box.astype(np.uint8)
        if obs_mask is not None:
            m = np.asarray(obs_mask)
            g = np.rint((p - bb[0]) / np.float64(res))                        # half to even
            ok = in_box & (g >= 0).all(1) & (g < np.float64(m.shape)).all(1)
            gi = np.where(ok[:, None], g, 0).astype(np.int64)
            flags |= ((ok & (m[gi[:, 0], gi[:, 1], gi[:, 2]] != 0)).astype(np.uint8) << 1)
    if plane is not None:
        P = np.asarray(plane, np.float64).reshape(4)
        s = ((P[0] * p[:, 0] + P[1] * p[:, 1]) + P[2] * p[:, 2]) + P[3]
        flags |= ((fin & (s > 0)).astype(np.uint8) << 2)
    return flags


def hand_regions():
    """Points worked out by hand on a 7x5x3 mask: (points, mask, bb, res, patch, plane, expected flags).
    BB0 = (10, 20, 30), Res = 2, patch = 1: the box is [9, 24) x [19, 30) x [29, 36); above: z > 30.5."""
    bb = np.float64([[10, 20, 30], [22, 28, 34]])
    mask = np.ones((7, 5, 3), np.uint8)
    mask[1, 1, 1] = 0
    pts = np.float32([
        [11, 22, 30],      # (p - BB0) / Res = (0.5, 1, 0) -> g = (0, 1, 0): half to even; set        -> 3
        [13, 22, 30],      # 1.5 -> 2                                                                 -> 3
        [15, 22, 30],      # 2.5 -> 2                                                                 -> 3
        [13, 21, 31],      # (1.5, 0.5, 0.5) -> (2, 0, 0); above                                      -> 7
        [12, 22, 32],      # g = (1, 1, 1): the cleared voxel; in the box, above                      -> 5
        [9, 19, 29],       # p == BB0 - patch on every axis: in; g = rint(-0.5) = -0 -> 0             -> 3
        [8.5, 22, 30],     # below BB0 - patch                                                        -> 0
        [24, 22, 30],      # p_x == BB1 + 2 patch: out                                                -> 0
        [23.5, 22, 30],    # in the box; g_x = rint(6.75) = 7 == n_x: not observed                    -> 1
        [23, 22, 30],      # g_x = rint(6.5) = 6: half to even keeps it inside                        -> 3
        [12, 29.5, 30],    # g_y = rint(4.75) = 5 == n_y                                              -> 1
        [12, 22, 35.5],    # g_z = rint(2.75) = 3 == n_z; above                                       -> 5
        [np.nan, 22, 30], [12, np.inf, 31]])
    return pts, mask, bb, 2.0, 1.0, np.float64([0, 0, 1, -30.5]), np.uint8([3, 3, 3, 7, 5, 3, 0, 0, 1, 3, 1, 5, 0, 0])


def ranks_of(order, seed, n):
    if isinstance(order, str):
        return np.random.default_rng(seed).permutation(n) if order == "random" else np.arange(n)
    return np.asarray(order)


def _side(query, target, origin, cell, max_dist):
    d, _ = ref.nn(query, target, origin, cell, max_dist)
    d = np.where(d >= np.float32(max_dist), np.float32(np.inf), d)            # strict truncation (NaN stays)
    st = ref.stats(d)
    fin = np.sort(d[np.isfinite(d)])
    mean = ref.fixed_order_sum(d) / st[0] if st[0] else float("nan")
    median = float(fin[(fin.size - 1) // 2]) if fin.size else float("nan")
    return mean, median, int(d.shape[0] - st[2] - st[0])


def evaluate_dtu(recon, gt, obs_mask, bb, res, plane, thin=0.2, patch=60.0, max_dist=20.0, seed=0, order="random"):
    """aarmvs.cloud_eval.evaluate_dtu restated."""
    recon = np.asarray(recon, np.float32).reshape(-1, 3)
    gt = np.asarray(gt, np.float32).reshape(-1, 3)
    kept, rounds = thin_rounds(recon, thin, ranks_of(order, seed, recon.shape[0]))
    assert (kept == thin_sequential(recon, thin, ranks_of(order, seed, recon.shape[0]))).all()
    down = recon[kept]
    flags = regions(down, obs_mask, bb, res, patch)
    data_in, data_in_obs = down[(flags & 1) != 0], down[(flags & 2) != 0]
    gt_above = gt[(regions(gt, plane=plane) & 4) != 0]
    out = dict(n_recon=int(recon.shape[0]), n_thinned=int(down.shape[0]), n_in_box=int(data_in.shape[0]),
               n_in_obs=int(data_in_obs.shape[0]), n_gt=int(gt.shape[0]), n_gt_above=int(gt_above.shape[0]),
               thin_rounds=int(rounds))
    origin, cell = ref.grid_for([data_in, gt], max_dist)
    out["accuracy_mean"], out["accuracy_median"], out["recon_beyond_max_dist"] = _side(data_in_obs, gt, origin, cell,
                                                                                     max_dist)
    out["completeness_mean"], out["completeness_median"], out["gt_beyond_max_dist"] = _side(gt_above, data_in, origin,
                                                                                          cell, max_dist)
    out["overall"] = 0.5 * (out["accuracy_mean"] + out["completeness_mean"])
    out["recon_nonfinite"] = int((~np.isfinite(recon).all(1)).sum())
    out["gt_nonfinite"] = int((~np.isfinite(gt).all(1)).sum())
    out.update(thin=float(np.float32(thin)), patch=float(patch), max_dist=float(max_dist), seed=int(seed),
               order=order if isinstance(order, str) else "ranks")
    return out


# --------------------------------------------------------------------------------- the shared cases
R = 0.75   # with coordinates on multiples of 1/4: d2 is exact, and ties at exactly r occur


def lattice_cloud(side, n=20000, seed=0):
    """n random points on the quarter lattice in a side^3 cube (duplicates included)."""
    return (np.random.default_rng(seed).integers(0, 4 * side + 1, (n, 3)) * 0.25).astype(np.float32)


def raster_plane(w=160, h=120, pitch=0.25):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x.ravel() * pitch, y.ravel() * pitch, np.zeros(w * h)], 1).astype(np.float32)


def line(n=256, spacing=0.5):
    return np.stack([np.arange(n) * spacing, np.zeros(n), np.zeros(n)], 1).astype(np.float32)
