"""CPU restatement of the fusion step's opt-in visibility de-duplication -- TEST INFRASTRUCTURE.
Only tests/ and the timing tools may import this module; the product path (aarmvs.fusion) runs
the HIP kernel and never falls back to it.

The contract (include/aarmvs.h, aarmvs_fusion_filter_dedup): a scan keeps one used map per view
(uint8 [H,W], zero at the start), reference views go in pair-file order, and for reference view r
with sources s_0 .. s_{k-1}
  emit(p) = final(p) and used[r][p] == 0
  for every final p (emitted or not) and every source v whose i = 10 mask holds at p:
      X, Y = rint(x2d_src), rint(y2d_src)   (the float32 coordinates given to remap; ties to even)
      used[s_v][Y, X] = 1 if 0 <= X < W and 0 <= Y < H   (non-finite coordinates mark nothing)
The masks and the averaged depth are oracle.fusion_oracle.filter_depth_core's (or, for Tanks and
Temples, tests/fusion_tnt_ref.py's: the same values up to 10 source views), the mask and the
coordinates come from oracle.fusion_oracle.check_geometric_consistency, and the points are
fusion.py:235-246 on ``emit`` instead of ``final``.
"""
import numpy as np

from oracle import fusion_oracle as fo


def filter_depth_dedup(ref_depth, confidence, ref_cam, src_depths, src_cams, photo_threshold, used_ref,
                       used_srcs, core=fo.filter_depth_core, mark_from_emit=False):
    """One reference view: (photo, geo, final, emit, avg).  ``used_ref``: uint8 [H,W] or None
    (nothing used yet); ``used_srcs``: one uint8 [H,W] per source view, marked in place, or None
    (that view is not marked).  ``mark_from_emit``: the other reading of the contract (marks from
    emitted pixels only), kept to show that the known answers tell the two apart."""
    photo, geo, final, avg = core(ref_depth, confidence, ref_cam, src_depths, src_cams, photo_threshold)
    emit = final.copy() if used_ref is None else np.logical_and(final, used_ref == 0)
    H, W = ref_depth.shape
    marking = emit if mark_from_emit else final
    for src_depth, (K, E), used in zip(src_depths, src_cams, used_srcs):
        if used is None:
            continue
        _, mask, _, x2d_src, y2d_src, _ = fo.check_geometric_consistency(
            ref_depth, ref_cam[0], ref_cam[1], src_depth, K, E)
        assert x2d_src.dtype == np.float32 and y2d_src.dtype == np.float32
        sel = np.logical_and(marking, mask)
        X, Y = np.rint(x2d_src[sel]), np.rint(y2d_src[sel])
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(X) & np.isfinite(Y) & (X >= 0) & (X < W) & (Y >= 0) & (Y < H)
        used[Y[ok].astype(np.int64), X[ok].astype(np.int64)] = 1
    return photo, geo, final, emit, avg


def fuse_points(depth_est_averaged, valid, ref_cam, ref_img=None):
    """fusion.py:235-246: (xyz float32 [n,3], rgb uint8 [n,3] or None) of the pixels of ``valid``."""
    K, E = ref_cam
    height, width = depth_est_averaged.shape[:2]
    x, y = np.meshgrid(np.arange(0, width), np.arange(0, height))
    x, y, depth = x[valid], y[valid], depth_est_averaged[valid]
    xyz_ref = np.matmul(np.linalg.inv(K), np.vstack((x, y, np.ones_like(x))) * depth)
    xyz_world = np.matmul(np.linalg.inv(E), np.vstack((xyz_ref, np.ones_like(x))))[:3]
    rgb = None if ref_img is None else (ref_img[valid] * 255).astype(np.uint8)
    return xyz_world.transpose((1, 0)).astype(np.float32), rgb


def fuse_views(pairs, depths, confidences, cams, images=None, photo_threshold=0.35, dedup=True,
               core=fo.filter_depth_core, mark_from_emit=False):
    """A scan in memory (dicts keyed by view id; reference views without a depth map are skipped):
    dict(xyz, rgb, masks {view: dict(photo, geo, final, emit)}, avg {view}, counts {view}, used
    {view: uint8 [H,W]}).  With ``dedup=False`` the points are those of ``final``, there are no
    ``emit`` masks and no used maps."""
    used, masks, avgs, counts, verts, cols = {}, {}, {}, {}, [], []

    def used_of(v):
        if v not in used:
            used[v] = np.zeros(depths[v].shape, np.uint8)
        return used[v]

    for ref, srcs in pairs:
        if ref not in depths:
            continue
        src_d, src_c = [depths[s] for s in srcs], [cams[s] for s in srcs]
        if dedup:
            photo, geo, final, emit, avg = filter_depth_dedup(
                depths[ref], confidences[ref], cams[ref], src_d, src_c, photo_threshold, used_of(ref),
                [used_of(s) for s in srcs], core=core, mark_from_emit=mark_from_emit)
            masks[ref] = dict(photo=photo, geo=geo, final=final, emit=emit)
        else:
            photo, geo, final, avg = core(depths[ref], confidences[ref], cams[ref], src_d, src_c, photo_threshold)
            emit = final
            masks[ref] = dict(photo=photo, geo=geo, final=final)
        xyz, rgb = fuse_points(avg, emit, cams[ref], None if images is None else images[ref])
        avgs[ref], counts[ref] = avg, xyz.shape[0]
        verts.append(xyz)
        cols.append(rgb)
    xyz = np.concatenate(verts) if verts else np.zeros((0, 3), np.float32)
    rgb = None if images is None else (np.concatenate(cols) if cols else np.zeros((0, 3), np.uint8))
    return dict(xyz=xyz, rgb=rgb, masks=masks, avg=avgs, counts=counts, used=used)


def scene(H, W, nsrc, seed, reverse=False):
    """The tests' scan: synthetic.fusion_views(H, W, nsrc, seed), per-view confidences drawn in
    view order from default_rng(seed + 100), every other view (ascending) as a source view, seeded
    images.  Returns (pairs, depths, confidences, cams, images), dicts keyed by view id."""
    from aarmvs import synthetic as syn
    d, c, _ = syn.fusion_views(H, W, nsrc, seed=seed)
    n = nsrc + 1
    rng = np.random.default_rng(seed + 100)
    confs = {v: rng.random((H, W)).astype(np.float32) for v in range(n)}
    irng = np.random.default_rng(seed + 200)
    images = {v: irng.integers(0, 256, (H, W, 3)).astype(np.float32) / np.float32(255.0) for v in range(n)}
    order = range(n - 1, -1, -1) if reverse else range(n)
    pairs = [(v, [s for s in range(n) if s != v]) for v in order]
    return pairs, dict(enumerate(d)), confs, dict(enumerate(c)), images


def footprint(W):
    """The world size of a pixel at the scene's depth: 600 / f, f = 1.2 W (synthetic.fusion_views)."""
    return 600.0 / (1.2 * W)


def largest_gap(full_xyz, kept_xyz, chunk=512):
    """max over the points of ``full_xyz`` of the distance to the nearest point of ``kept_xyz``
    (brute force, float64)."""
    kept = kept_xyz.astype(np.float64)
    worst = 0.0
    for i in range(0, full_xyz.shape[0], chunk):
        a = full_xyz[i:i + chunk].astype(np.float64)
        d2 = ((a[:, None, :] - kept[None, :, :]) ** 2).sum(-1)
        worst = max(worst, float(np.sqrt(d2.min(1).max())))
    return worst
