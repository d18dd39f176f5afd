"""CPU restatement of the fusion step's opt-in per-point normals -- TEST INFRASTRUCTURE.  Only tests/
and the timing tools may import this module; the product path (aarmvs.fusion) runs the HIP kernel
and never falls back to it.

The contract (include/aarmvs.h, aarmvs_fusion_normals), op for op in float64, vectorised over the
pixels, the window offsets in row-major order (v outer, u inner):
  centre p usable: valid[p] != 0 and d0 = depth[p] finite and > 0
  neighbour q = p + (u, v), |u|, |v| <= r, usable: inside, valid, depth finite and > 0, and
      |depth[q] - d0| <= float64(float32(max_rel_jump)) * d0      (the centre counts)
  w = 1.0 / depth[q];  A = sum u^2, B = sum u v, C = sum v^2, D = sum u, E = sum v, N = sum 1,
      Suw = sum (u w), Svw = sum (v w), Sw = sum w
  c00 = C N - E E, c01 = D E - B N, c02 = B E - C D, c11 = A N - D D, c12 = B D - A E,
      c22 = A C - B B, det = (A c00 + B c01) + D c02
  a = (c00 Suw + c01 Svw) + c02 Sw, b = (c01 Suw + c11 Svw) + c12 Sw, c = (c02 Suw + c12 Svw) + c22 Sw
  cabs = (c - a x0) - b y0
  m_i = (K[0][i] a + K[1][i] b) + K[2][i] cabs, len = sqrt((m0^2 + m1^2) + m2^2), n_cam = -(m / len)
  n_i = (R[i][0] n0 + R[i][1] n1) + R[i][2] n2, R = inv(E)[:3, :3] (float32 inverse), cast to float32
  has = usable and N >= min_count and det > 0 and len finite and > 0; else normal = 0.
numpy rounds every float64 operation on its own (no fused multiply-add), as the contract asks.
"""
import numpy as np

import fusion_dedup_ref as dr

DEFAULTS = dict(radius=2, max_rel_jump=0.01, min_count=3)


def estimate_normals(depth, valid, ref_cam, radius=2, max_rel_jump=0.01, min_count=3, origin=(0, 0)):
    """(normal float32 [H,W,3], has bool [H,W]) of a float64 depth map and a mask; ref_cam = (K, E).
    ``origin`` = (x, y): the pixel coordinates of depth[0, 0], for a test that looks at a window of a
    larger frame (a fit depends only on its window; the crop's borders are image borders)."""
    depth = np.asarray(depth, np.float64)
    H, W = depth.shape
    r = int(radius)
    K = np.asarray(ref_cam[0], np.float32).astype(np.float64)
    R = np.linalg.inv(np.asarray(ref_cam[1], np.float32))[:3, :3].astype(np.float64)
    jump = np.float64(np.float32(max_rel_jump))
    with np.errstate(all="ignore"):
        usable = (np.asarray(valid) != 0) & np.isfinite(depth) & (depth > 0)
        # padded by r: the out-of-image taps are unusable
        dpad = np.full((H + 2 * r, W + 2 * r), np.nan)
        dpad[r:r + H, r:r + W] = np.where(usable, depth, np.nan)
        upad = np.zeros((H + 2 * r, W + 2 * r), bool)
        upad[r:r + H, r:r + W] = usable
        lim = jump * depth
        A, B, C, D, E, N = (np.zeros((H, W)) for _ in range(6))
        Suw, Svw, Sw = (np.zeros((H, W)) for _ in range(3))
        for v in range(-r, r + 1):
            for u in range(-r, r + 1):
                dq = dpad[r + v:r + v + H, r + u:r + u + W]
                ok = usable & upad[r + v:r + v + H, r + u:r + u + W] & (np.abs(dq - depth) <= lim)
                w = 1.0 / dq
                A, B, C = A + ok * (u * u), B + ok * (u * v), C + ok * (v * v)
                D, E, N = D + ok * u, E + ok * v, N + ok
                Suw = np.where(ok, Suw + np.float64(u) * w, Suw)
                Svw = np.where(ok, Svw + np.float64(v) * w, Svw)
                Sw = np.where(ok, Sw + w, Sw)
        c00, c01, c02 = C * N - E * E, D * E - B * N, B * E - C * D
        c11, c12, c22 = A * N - D * D, B * D - A * E, A * C - B * B
        det = (A * c00 + B * c01) + D * c02
        a = (c00 * Suw + c01 * Svw) + c02 * Sw
        b = (c01 * Suw + c11 * Svw) + c12 * Sw
        c = (c02 * Suw + c12 * Svw) + c22 * Sw
        y0, x0 = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        x0, y0 = x0 + np.float64(origin[0]), y0 + np.float64(origin[1])
        cabs = (c - a * x0) - b * y0
        m = [(K[0, i] * a + K[1, i] * b) + K[2, i] * cabs for i in range(3)]
        length = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        n = [-(mi / length) for mi in m]
        world = [(R[i, 0] * n[0] + R[i, 1] * n[1]) + R[i, 2] * n[2] for i in range(3)]
        has = usable & (N >= min_count) & (det > 0) & np.isfinite(length) & (length > 0)
        normal = np.stack([np.where(has, wi, 0.0) for wi in world], axis=-1).astype(np.float32)
    return normal, has


def fuse_views_normals(pairs, depths, confidences, cams, images=None, photo_threshold=0.35, dedup=False,
                       normals=True, require_normal=False, core=dr.fo.filter_depth_core):
    """fusion_dedup_ref.fuse_views with normals: per view the fit on the averaged depth and the FINAL
    mask (also under dedup), the points those of final / emit (and has, with require_normal).  The
    dict gains ``normals`` [n,3], ``normal_maps`` and ``has_normal`` {view}."""
    params = dict(DEFAULTS) if normals is True else {**DEFAULTS, **normals}
    out = dr.fuse_views(pairs, depths, confidences, cams, images, photo_threshold, dedup=dedup, core=core)
    nmaps, has_maps, verts, cols, nrms, counts = {}, {}, [], [], [], {}
    for ref, _ in pairs:
        if ref not in depths:
            continue
        m = out["masks"][ref]
        nmaps[ref], has_maps[ref] = estimate_normals(out["avg"][ref], m["final"], cams[ref], **params)
        keep = m["emit"] if dedup else m["final"]
        if require_normal:
            keep = keep & has_maps[ref]
        xyz, rgb = dr.fuse_points(out["avg"][ref], keep, cams[ref], None if images is None else images[ref])
        verts.append(xyz)
        cols.append(rgb)
        nrms.append(nmaps[ref][keep])
        counts[ref] = xyz.shape[0]
    out["xyz"] = np.concatenate(verts) if verts else np.zeros((0, 3), np.float32)
    if images is not None:
        out["rgb"] = np.concatenate(cols) if cols else np.zeros((0, 3), np.uint8)
    out["counts"] = counts
    out["normals"] = np.concatenate(nrms) if nrms else np.zeros((0, 3), np.float32)
    out["normal_maps"], out["has_normal"] = nmaps, has_maps
    return out


# ---------------------------------------------------------------------------------
# analytic scenes for the tests: a camera (K, E), a depth map, the true world normals
# ---------------------------------------------------------------------------------
def camera(f=290.0, cx=32.0, cy=24.0, seed=0):
    """(K float32 3x3, E float32 4x4 world -> camera): a seeded rotation and translation."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = q, rng.uniform(-50, 50, 3)
    K = np.array([[f, 0, cx], [0, f * 1.01, cy], [0, 0, 1]])
    return K.astype(np.float32), E.astype(np.float32)


def rays(K, H, W, origin=(0, 0)):
    """inv(K) (x, y, 1) per pixel, float64 [H,W,3]; ``origin``: the pixel coordinates of [0, 0]."""
    y, x = np.meshgrid(np.arange(H, dtype=np.float64) + origin[1], np.arange(W, dtype=np.float64) + origin[0],
                       indexing="ij")
    pix = np.stack([x, y, np.ones_like(x)], -1)
    return pix @ np.linalg.inv(np.asarray(K, np.float64)).T


def plane_depth(K, H, W, n_cam, dist, origin=(0, 0)):
    """Depth map of the camera-space plane n_cam . P = -dist (dist > 0: the unit normal n_cam faces
    the camera at the origin; every ray must meet it, n_cam . ray < 0)."""
    n_cam = np.asarray(n_cam, np.float64) / np.linalg.norm(n_cam)
    return -dist / (rays(K, H, W, origin) @ n_cam)


def world_normal(E, n_cam):
    """The camera-space unit normal in world coordinates (float64), as the contract rotates it."""
    n_cam = np.asarray(n_cam, np.float64) / np.linalg.norm(n_cam)
    return np.linalg.inv(np.asarray(E, np.float32))[:3, :3].astype(np.float64) @ n_cam


def sphere_depth(K, H, W, centre, radius):
    """(depth [H,W] (NaN off the sphere), camera-space outward normals [H,W,3]) of a sphere."""
    ray = rays(K, H, W)
    c = np.asarray(centre, np.float64)
    aa = (ray * ray).sum(-1)
    bb = ray @ c
    with np.errstate(invalid="ignore"):
        t = (bb - np.sqrt(bb * bb - aa * (c @ c - radius * radius))) / aa
    P = ray * t[..., None]
    return t, (P - c) / radius


def angle_deg(n, truth):
    """Angle between unit vectors [..., 3], degrees."""
    return np.degrees(np.arccos(np.clip((np.asarray(n, np.float64) * truth).sum(-1), -1.0, 1.0)))


def cross_product_normals(depth, K):
    """The estimator the fit replaces: back-project, central differences, cross product, faced to the
    camera.  Camera-space unit normals [H,W,3] (NaN on the border)."""
    H, W = depth.shape
    P = rays(K, H, W) * depth[..., None]
    out = np.full((H, W, 3), np.nan)
    dx = P[1:-1, 2:] - P[1:-1, :-2]
    dy = P[2:, 1:-1] - P[:-2, 1:-1]
    n = np.cross(dx, dy)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    flip = (n * P[1:-1, 1:-1]).sum(-1) > 0
    n[flip] = -n[flip]
    out[1:-1, 1:-1] = n
    return out
