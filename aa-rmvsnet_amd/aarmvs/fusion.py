"""Depth-map fusion (the reference's fusion.py) on the HIP library.

``filter_depth_core`` is the per-reference-view core of ``filter_depth``
(fusion.py:174-220): photometric mask, geometric consistency against every source view
(``reproject_with_depth`` / ``check_geometric_consistency``, fusion.py:71-133), the
per-threshold votes, the geometric and final masks and the averaged depth -- one HIP
launch (``aarmvs_fusion_filter``).  ``fuse_points`` back-projects the kept pixels to world
points (fusion.py:235-246), and ``filter_depth`` is the per-scan driver (fusion.py:135-273):
pair file, per reference view the image rescale/crop and camera re-centring, the GPU core
against every source view, the three mask PNGs and the scan's PLY.  The file helpers
read/write the formats the fusion step consumes: PFM maps (``datasets.data_io``, the
reference's datasets/data_io.py:9-74, re-exported here), cam files (fusion.py:27-42), pair files (fusion.py:57-68), images (fusion.py:45-50), masks
(fusion.py:52-56) and a binary PLY writer for the point cloud.
Depth maps must be CUDA float32 tensors; there is no CPU fallback.

Tanks and Temples goes through the reference's fusion_padding.py instead: ``filter_depth_tnt``
is that per-scan driver (halved intrinsics, rows [2:-2] of the maps, ``pyr_down`` of the image
(``aarmvs_pyr_down``), the same filter core, and ``fuse_points_gpu`` (``aarmvs_fusion_points``)
for the kept pixels' points).  ``python -m aarmvs.fusion --test_dataset {dtu,tnt} ...`` runs
either driver over a scan list.

Opt-in, beyond the reference: the visibility de-duplication (``--dedup``, ``dedup=True`` on both
drivers and on ``fuse_views``, which fuses a scan held in memory; ``filter_depth_dedup`` per
reference view, ``aarmvs_fusion_filter_dedup``).  A scan keeps one used map per view; a final pixel
marks the pixel it projects to in every source view it is consistent with, and a later view emits
only its final pixels that are not marked, so a surface patch seen from k views is emitted about
once instead of k times.  Off (the default) nothing changes.  Its effect on DTU and Tanks and
Temples scores is not measured.

Opt-in, beyond the reference: per-point normals (``--normals``, ``normals=True`` or a dict of
``radius`` / ``max_rel_jump`` / ``min_count`` on both drivers and on ``fuse_views``;
``estimate_normals`` per view, ``aarmvs_fusion_normals``).  A view's normal map is a least-squares fit
of 1/d = a x + b y + c over a window of its averaged depth map, restricted to the view's final mask
and to neighbours within ``max_rel_jump`` of the centre's depth; the normals face the camera, travel
with the kept pixels (``fuse_points_normals_gpu``, ``aarmvs_fusion_points_normals``) and go to the
PLY as nx ny nz.  Off (the default) nothing changes.  The effect on meshes of DTU and Tanks and
Temples clouds is not measured.
"""
from __future__ import annotations

import os

import ctypes

import numpy as np
import torch

from datasets.data_io import read_pfm, save_pfm  # noqa: F401  (fusion.read_pfm / save_pfm)

from . import _lib
from ._lib import AarmvsError, check, lib

# the per-scan folders the drivers read the maps from (the reference's names, eval.py)
DEFAULT_DEPTH_DIR, DEFAULT_CONF_DIR = "depth_est_0", "confidence_0"


def pack_cameras(ref_cam, src_cams) -> np.ndarray:
    """float32 matrices exactly as numpy forms them in fusion.py:71-108 (float32 inverses
    and float32 products), packed for ``aarmvs_fusion_filter`` (include/aarmvs.h)."""
    K_ref = np.asarray(ref_cam[0], np.float32)
    E_ref = np.asarray(ref_cam[1], np.float32)
    parts = [np.linalg.inv(K_ref).ravel(), K_ref.ravel()]
    for K, E in src_cams:
        K = np.asarray(K, np.float32)
        E = np.asarray(E, np.float32)
        parts += [K.ravel(), np.linalg.inv(K).ravel(),
                  np.matmul(E, np.linalg.inv(E_ref))[:3].ravel(),
                  np.matmul(E_ref, np.linalg.inv(E))[:3].ravel()]
    out = np.concatenate(parts).astype(np.float32)
    assert out.size == _lib.fusion_cam_floats(len(src_cams))
    return np.ascontiguousarray(out)


def filter_depth_core(ref_depth: torch.Tensor, confidence: torch.Tensor, ref_cam, src_depths,
                      src_cams, photo_threshold: float):
    """(photo_mask, geo_mask, final_mask [H,W] bool, depth_est_averaged [H,W] float64)."""
    return _filter_launch(ref_depth, confidence, ref_cam, src_depths, src_cams, photo_threshold, None)


def _used_map(t, ref_depth, what):
    if not (isinstance(t, torch.Tensor) and t.device == ref_depth.device and t.dtype == torch.uint8
            and t.shape == ref_depth.shape and t.is_contiguous()):
        raise AarmvsError(f"aarmvs: fusion {what} must be a contiguous CUDA uint8 [H,W] tensor of the depth "
                          "map's size, on its device")
    return t


def filter_depth_dedup(ref_depth: torch.Tensor, confidence: torch.Tensor, ref_cam, src_depths, src_cams,
                       photo_threshold: float, used_ref, used_srcs, emit_out=None):
    """``filter_depth_core`` with the visibility de-duplication (``aarmvs_fusion_filter_dedup``,
    include/aarmvs.h): (photo_mask, geo_mask, final_mask, emit_mask [H,W] bool,
    depth_est_averaged [H,W] float64).  ``used_ref``: the reference view's used map, a CUDA uint8
    [H,W] tensor, or None (nothing used yet: emit = final).  ``used_srcs``: one used map per source
    view, marked IN PLACE; an entry may be None (that view is not marked).  emit = final and not
    used_ref; every final pixel marks the nearest pixel of each source view it is consistent with.
    The other four outputs are ``filter_depth_core``'s, bit for bit.  The calls of one scan must be
    ordered on one stream.  ``emit_out``: a CUDA uint8 [H,W] tensor to write the emit mask into."""
    if len(used_srcs) != len(src_depths):
        raise AarmvsError(f"aarmvs: fusion got {len(src_depths)} source views but {len(used_srcs)} used maps")
    return _filter_launch(ref_depth, confidence, ref_cam, src_depths, src_cams, photo_threshold,
                          (used_ref, list(used_srcs), emit_out))


def _filter_launch(ref_depth, confidence, ref_cam, src_depths, src_cams, photo_threshold, dedup):
    """The filter launch behind ``filter_depth_core`` (dedup None) and ``filter_depth_dedup``
    (dedup = (used_ref, used_srcs, emit_out))."""
    nsrc = len(src_depths)
    if not 1 <= nsrc <= _lib.MAX_FUSION_SRC:
        raise AarmvsError(f"aarmvs: fusion needs 1..{_lib.MAX_FUSION_SRC} source views, got {nsrc}")
    maps = [ref_depth, confidence, *src_depths]
    for t in maps:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
            raise AarmvsError("aarmvs: fusion depth maps / confidence must be CUDA float32 tensors")
        if t.shape != ref_depth.shape or t.dim() != 2:
            raise AarmvsError("aarmvs: fusion maps must all be [H,W] of the same size")
    maps = [t.contiguous() for t in maps]
    H, W = ref_depth.shape
    dev = ref_depth.device
    cams = pack_cameras(ref_cam, src_cams)
    photo = torch.empty(H, W, dtype=torch.uint8, device=dev)
    geo = torch.empty_like(photo)
    final = torch.empty_like(photo)
    avg = torch.empty(H, W, dtype=torch.float64, device=dev)
    a = _lib.FusionArgs()
    a.H, a.W, a.nsrc = H, W, nsrc
    a.ref_depth = maps[0].data_ptr()
    a.confidence = maps[1].data_ptr()
    for i, t in enumerate(maps[2:]):
        a.src_depth[i] = t.data_ptr()
    a.cams = cams.ctypes.data
    a.photo_threshold = float(np.float32(photo_threshold))
    a.photo_mask, a.geo_mask, a.final_mask = photo.data_ptr(), geo.data_ptr(), final.data_ptr()
    a.depth_avg = avg.data_ptr()
    if dedup is None:
        check(lib().aarmvs_fusion_filter(ctypes.byref(a), torch.cuda.current_stream().cuda_stream),
              "fusion_filter")
        return photo.bool(), geo.bool(), final.bool(), avg
    used_ref, used_srcs, emit = dedup
    d = _lib.FusionDedupArgs()
    if used_ref is not None:
        d.used_ref = _used_map(used_ref, ref_depth, "used_ref").data_ptr()
    for i, t in enumerate(used_srcs):
        if t is not None:
            d.used_src[i] = _used_map(t, ref_depth, "used_srcs").data_ptr()
    emit = torch.empty_like(photo) if emit is None else _used_map(emit, ref_depth, "emit_out")
    d.emit_mask = emit.data_ptr()
    with torch.cuda.device(dev):
        check(lib().aarmvs_fusion_filter_dedup(ctypes.byref(a), ctypes.byref(d),
                                               torch.cuda.current_stream().cuda_stream), "fusion_filter_dedup")
    return photo.bool(), geo.bool(), final.bool(), emit.bool(), avg


def fuse_points(depth_est_averaged, final_mask, ref_cam, ref_img=None):
    """World points (float32 [n,3]) and colours (uint8 [n,3] or None) of the kept pixels
    (fusion.py:235-246), host numpy."""
    depth = depth_est_averaged.cpu().numpy() if isinstance(depth_est_averaged, torch.Tensor) else depth_est_averaged
    valid = final_mask.cpu().numpy() if isinstance(final_mask, torch.Tensor) else final_mask
    K, E = (np.asarray(m, np.float32) for m in ref_cam)
    height, width = depth.shape[:2]
    x, y = np.meshgrid(np.arange(0, width), np.arange(0, height))
    x, y, d = x[valid], y[valid], depth[valid]
    xyz_ref = np.matmul(np.linalg.inv(K), np.vstack((x, y, np.ones_like(x))) * d)
    xyz_world = np.matmul(np.linalg.inv(E), np.vstack((xyz_ref, np.ones_like(x))))[:3]
    colors = None if ref_img is None else (np.asarray(ref_img)[valid] * 255).astype(np.uint8)
    return xyz_world.transpose((1, 0)).astype(np.float32), colors


def crop_params(img_hw, depth_hw):
    """(scale, index, index_p, flag) that map an image of size img_hw onto a depth map of size
    depth_hw: resize by scale, then crop index / index_p columns (flag 0) or rows (flag 1)
    (fusion.py:157-165)."""
    (ih, iw), (dh, dw) = img_hw, depth_hw
    scale = float(dh) / ih
    index = int((int(iw * scale) - dw) / 2)
    index_p = (int(iw * scale) - dw) - index
    flag = 0
    if dw / iw > scale:
        scale = float(dw) / iw
        index = int((int(ih * scale) - dh) / 2)
        index_p = (int(ih * scale) - dh) - index
        flag = 1
    return scale, index, index_p, flag


def resize_linear(img, width, height):
    """cv2.resize(img, (width, height)) with the default INTER_LINEAR on a float32 [H,W,C]
    image, restated from OpenCV's published algorithm (imgproc/src/resize.cpp): source
    coordinate (d + 0.5) / scale - 0.5, clamped taps, float32 horizontal then vertical
    passes; an exact 2x downscale takes OpenCV's INTER_AREA path (2x2 mean).  cv2 is not
    installed here, so agreement with cv2 itself is parity unpinned; the common DTU / T&T
    case is scale 1 (the identity)."""
    img = np.asarray(img, np.float32)
    ih, iw = img.shape[:2]
    if (iw, ih) == (width, height):
        return img.copy()
    if iw == 2 * width and ih == 2 * height:
        q = img[0::2, 0::2] + img[0::2, 1::2]
        q = q + img[1::2, 0::2]
        q = q + img[1::2, 1::2]
        return (q * np.float32(0.25)).astype(np.float32)

    def taps(n_src, n_dst):
        scale = float(n_src) / n_dst   # 1 / inv_scale (double), resize.cpp
        d = np.arange(n_dst, dtype=np.float64)
        f = ((d + 0.5) * scale - 0.5).astype(np.float32)
        s0 = np.floor(f).astype(np.int64)
        f = (f - s0.astype(np.float32)).astype(np.float32)
        lo = s0 < 0
        f[lo], s0[lo] = 0.0, 0
        hi = s0 >= n_src - 1
        f[hi], s0[hi] = 0.0, n_src - 1
        s1 = np.minimum(s0 + 1, n_src - 1)
        return s0, s1, (np.float32(1) - f).astype(np.float32), f

    x0, x1, ax0, ax1 = taps(iw, width)
    y0, y1, by0, by1 = taps(ih, height)
    ex = (slice(None), None) if img.ndim == 3 else (slice(None),)
    rows = img[:, x0] * ax0[ex] + img[:, x1] * ax1[ex]          # horizontal pass, float32
    ey = (slice(None), None, None) if img.ndim == 3 else (slice(None), None)
    out = by0[ey] * rows[y0] + by1[ey] * rows[y1]                # vertical pass
    return out.astype(np.float32)


def filter_depth(scan_folder, out_folder, plyfilename, photo_threshold, device="cuda",
                 depth_dir=DEFAULT_DEPTH_DIR, conf_dir=DEFAULT_CONF_DIR, dedup=False, normals=None,
                 require_normal=False):
    """fusion.py:135-273 for one scan: for every (ref_view, src_views) of pair.txt with an
    estimated depth map, the geometric / photometric filtering on the GPU
    (``filter_depth_core``), the three mask PNGs under out_folder/mask, and the kept pixels'
    world points (coloured from the rescaled, cropped reference image) written to
    plyfilename.  Returns the number of points written.  ``depth_dir`` / ``conf_dir``: the
    folders under out_folder the depth and confidence maps are read from (the reference's
    depth_est_0 / confidence_0; e.g. eval_sharded --refine_depth's depth_refined_0 /
    confidence_window_0).  ``dedup``: the opt-in visibility de-duplication
    (``filter_depth_dedup``): every view's depth map (read once) and used map stay on the GPU for
    the whole scan, the points are those of the emit mask, and mask/{view}_emit.png is written
    beside the other three.  ``normals`` (None / False, True, or a dict of ``radius`` /
    ``max_rel_jump`` / ``min_count``): the opt-in per-point normals (``estimate_normals`` on the
    averaged depth and the final mask), written to the PLY as nx ny nz; ``require_normal`` (with
    ``normals``): only the pixels that have a normal are extracted."""
    vertexs, vertex_colors, vertex_normals = [], [], []
    nparams = normal_params(normals)
    if require_normal and nparams is None:
        raise AarmvsError("aarmvs: require_normal needs normals")
    dev = torch.device(device)
    depth_file = os.path.join(out_folder, depth_dir, "{:0>8}.pfm")
    cache, used = {}, _UsedMaps()

    def depth_of(view):   # dedup only: a PFM is read once per scan
        if view not in cache:
            cache[view] = torch.from_numpy(np.ascontiguousarray(read_pfm(depth_file.format(view))[0])).to(dev)
        return cache[view]

    for ref_view, src_views in read_pair_file(os.path.join(scan_folder, "pair.txt")):
        dpath = depth_file.format(ref_view)
        if not os.path.exists(dpath):
            print("skip", ref_view)
            continue
        ref_img = read_img(os.path.join(scan_folder, "images/{:0>8}.jpg".format(ref_view)))
        ref_depth_est = None if dedup else read_pfm(dpath)[0]
        confidence = read_pfm(os.path.join(out_folder, conf_dir, "{:0>8}.pfm".format(ref_view)))[0]
        scale, index, index_p, flag = crop_params(ref_img.shape[:2], confidence.shape[:2])
        ref_img = resize_linear(ref_img, int(ref_img.shape[1] * scale), int(ref_img.shape[0] * scale))
        if flag == 0:
            ref_img = ref_img[:, index:ref_img.shape[1] - index_p, :]
        else:
            ref_img = ref_img[index:ref_img.shape[0] - index_p, :, :]
        cam_file = os.path.join(scan_folder, "cams/{:0>8}_cam.txt")
        ref_cam = read_camera_parameters(cam_file.format(ref_view), scale, index, flag)
        src_depths, src_cams = [], []
        for src_view in src_views:
            src_depths.append(depth_of(src_view) if dedup else torch.from_numpy(np.ascontiguousarray(read_pfm(
                depth_file.format(src_view))[0])).to(dev))
            src_cams.append(read_camera_parameters(cam_file.format(src_view), scale, index, flag))
        if dedup:
            ref_depth = depth_of(ref_view)
            photo, geo, final, emit, avg = filter_depth_dedup(
                ref_depth, torch.from_numpy(np.ascontiguousarray(confidence)).to(dev), ref_cam, src_depths,
                src_cams, photo_threshold, used.of(ref_view, ref_depth),
                [used.of(v, d) for v, d in zip(src_views, src_depths)])
            emit = emit.cpu().numpy()
        else:
            photo, geo, final, avg = filter_depth_core(
                torch.from_numpy(np.ascontiguousarray(ref_depth_est)).to(dev),
                torch.from_numpy(np.ascontiguousarray(confidence)).to(dev), ref_cam, src_depths, src_cams,
                photo_threshold)
        if nparams is not None:
            nmap, has = estimate_normals(avg, final, ref_cam, **nparams)
        photo, geo, final = (m.cpu().numpy() for m in (photo, geo, final))
        os.makedirs(os.path.join(out_folder, "mask"), exist_ok=True)
        save_mask(os.path.join(out_folder, "mask/{:0>8}_photo.png".format(ref_view)), photo)
        save_mask(os.path.join(out_folder, "mask/{:0>8}_geo.png".format(ref_view)), geo)
        save_mask(os.path.join(out_folder, "mask/{:0>8}_final.png".format(ref_view)), final)
        print("processing {}, ref-view{:0>2}, photo/geo/final-mask:{}/{}/{}".format(
            scan_folder, ref_view, photo.mean(), geo.mean(), final.mean()))
        if dedup:
            save_mask(os.path.join(out_folder, "mask/{:0>8}_emit.png".format(ref_view)), emit)
            print("  emit-mask:{}".format(emit.mean()))
        keep = emit if dedup else final
        if nparams is not None:
            if require_normal:
                keep = np.logical_and(keep, has.cpu().numpy())
            vertex_normals.append(nmap.cpu().numpy()[keep])
        xyz, rgb = fuse_points(avg.cpu().numpy(), keep, ref_cam, ref_img)
        vertexs.append(xyz)
        vertex_colors.append(rgb)
    return _write_scan_ply(plyfilename, vertexs, vertex_colors, vertex_normals if nparams is not None else None)


# ---------------------------------------------------------------------------------
# Tanks and Temples (the reference's fusion_padding.py)
# ---------------------------------------------------------------------------------
def pyr_down(img: torch.Tensor) -> torch.Tensor:
    """cv2.pyrDown(img) of a CUDA float32 [H,W] or [H,W,3] image (fusion_padding.py:166):
    [(H+1)//2, (W+1)//2(, 3)], one ``aarmvs_pyr_down`` launch.  OpenCV's scalar float path
    (imgproc/src/pyramids.cpp) restated op for op; cv2 is not installed here and its SIMD paths
    may associate the sums differently, so agreement with cv2 itself is parity unpinned."""
    if not (isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == torch.float32):
        raise AarmvsError("aarmvs: pyr_down needs a CUDA float32 tensor")
    if not (img.dim() == 2 or (img.dim() == 3 and img.shape[2] == 3)):
        raise AarmvsError(f"aarmvs: pyr_down needs an [H,W] or [H,W,3] image, got {tuple(img.shape)}")
    img = img.contiguous()
    H, W = img.shape[:2]
    out = torch.empty(((H + 1) // 2, (W + 1) // 2) + tuple(img.shape[2:]), dtype=torch.float32,
                      device=img.device)
    with torch.cuda.device(img.device):
        check(lib().aarmvs_pyr_down(img.data_ptr(), H, W, 1 if img.dim() == 2 else 3, out.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream), "pyr_down")
    return out


def pack_point_cameras(ref_cam) -> np.ndarray:
    """inv(K) 3x3 then inv(E) 4x4 as numpy forms them in float32 (fusion_padding.py:246-249),
    packed for ``aarmvs_fusion_points``."""
    K, E = (np.asarray(m, np.float32) for m in ref_cam)
    return np.ascontiguousarray(np.concatenate([np.linalg.inv(K).ravel(), np.linalg.inv(E).ravel()])
                                .astype(np.float32))


def fuse_points_into(depth_avg, final_mask, ref_cam, ref_img, xyz, rgb, *, normal_map=None, nrm=None) -> torch.Tensor:
    """The kept pixels' world points into the caller's buffers: xyz float32 [capacity,3], rgb
    uint8 [capacity,3] (None if and only if ref_img is), in pixel order; points past the
    capacity are dropped.  Returns the number of kept pixels as a CUDA int64 [1] tensor,
    without waiting for the device.  ``normal_map`` (CUDA float32 [H,W,3], ``estimate_normals``)
    and ``nrm`` (float32 [capacity,3]), both or neither: the kept pixels' normals go to ``nrm``
    (``aarmvs_fusion_points_normals``)."""
    if not (isinstance(depth_avg, torch.Tensor) and depth_avg.is_cuda and depth_avg.dtype == torch.float64
            and depth_avg.dim() == 2):
        raise AarmvsError("aarmvs: fuse_points_gpu needs the averaged depth as a CUDA float64 [H,W] tensor")
    dev = depth_avg.device
    if not (isinstance(final_mask, torch.Tensor) and final_mask.device == dev
            and final_mask.dtype in (torch.bool, torch.uint8) and final_mask.shape == depth_avg.shape):
        raise AarmvsError("aarmvs: fuse_points_gpu needs the mask as a CUDA bool / uint8 [H,W] tensor "
                          "of the depth map's size")
    H, W = depth_avg.shape
    if (ref_img is None) != (rgb is None):
        raise AarmvsError("aarmvs: fuse_points_gpu: colours out need an image, and an image colours out")
    if ref_img is not None:
        if not (isinstance(ref_img, torch.Tensor) and ref_img.device == dev and ref_img.dtype == torch.float32):
            raise AarmvsError("aarmvs: fuse_points_gpu needs the image as a CUDA float32 tensor")
        if tuple(ref_img.shape) != (H, W, 3):
            raise AarmvsError(f"aarmvs: image {tuple(ref_img.shape[:2])} and depth map {(H, W)} differ in size")
        ref_img = ref_img.contiguous()
    for t, dt, what in ((xyz, torch.float32, "xyz"), (rgb, torch.uint8, "rgb")):
        if t is not None and not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dt
                                  and t.dim() == 2 and t.shape[1] == 3 and t.is_contiguous()):
            raise AarmvsError(f"aarmvs: fuse_points_gpu: {what} must be a contiguous CUDA [n,3] tensor")
    if rgb is not None and rgb.shape[0] != xyz.shape[0]:
        raise AarmvsError("aarmvs: fuse_points_gpu: xyz and rgb differ in capacity")
    if (normal_map is None) != (nrm is None):
        raise AarmvsError("aarmvs: fuse_points_gpu: normals out need a normal map, and a normal map normals out")
    if normal_map is not None:
        if not (isinstance(normal_map, torch.Tensor) and normal_map.device == dev
                and normal_map.dtype == torch.float32 and tuple(normal_map.shape) == (H, W, 3)):
            raise AarmvsError("aarmvs: fuse_points_gpu needs the normal map as a CUDA float32 [H,W,3] tensor "
                              "of the depth map's size")
        normal_map = normal_map.contiguous()
        if not (isinstance(nrm, torch.Tensor) and nrm.device == dev and nrm.dtype == torch.float32
                and nrm.dim() == 2 and nrm.shape[1] == 3 and nrm.is_contiguous()):
            raise AarmvsError("aarmvs: fuse_points_gpu: nrm must be a contiguous CUDA [n,3] tensor")
        if nrm.shape[0] != xyz.shape[0]:
            raise AarmvsError("aarmvs: fuse_points_gpu: xyz and nrm differ in capacity")
    depth_avg, final_mask = depth_avg.contiguous(), final_mask.contiguous()
    cams = pack_point_cameras(ref_cam)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    work = torch.empty(max(1, lib().aarmvs_fusion_points_workspace_bytes(H, W)), dtype=torch.uint8, device=dev)
    a = _lib.FusionPointsArgs()
    a.H, a.W = H, W
    a.mask, a.depth = final_mask.data_ptr(), depth_avg.data_ptr()
    a.color = None if ref_img is None else ref_img.data_ptr()
    a.cams = cams.ctypes.data
    a.xyz = xyz.data_ptr()
    a.rgb = None if rgb is None else rgb.data_ptr()
    a.capacity = xyz.shape[0]
    a.count, a.workspace = count.data_ptr(), work.data_ptr()
    with torch.cuda.device(dev):
        if normal_map is None:
            check(lib().aarmvs_fusion_points(ctypes.byref(a), torch.cuda.current_stream().cuda_stream),
                  "fusion_points")
        else:
            check(lib().aarmvs_fusion_points_normals(ctypes.byref(a), normal_map.data_ptr(), nrm.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream),
                  "fusion_points_normals")
    return count


def fuse_points_gpu(depth_avg, final_mask, ref_cam, ref_img=None):
    """``fuse_points`` on the GPU (``aarmvs_fusion_points``): CUDA float64 averaged depth, CUDA
    bool mask and (optionally) a CUDA float32 [H,W,3] image in, (xyz float32 [n,3], rgb uint8
    [n,3] or None) out as CUDA tensors, the points in pixel order and bit-equal to numpy's."""
    if not (isinstance(depth_avg, torch.Tensor) and depth_avg.is_cuda and depth_avg.dim() == 2):
        raise AarmvsError("aarmvs: fuse_points_gpu needs the averaged depth as a CUDA float64 [H,W] tensor")
    (H, W), dev = depth_avg.shape, depth_avg.device
    xyz = torch.empty(H * W, 3, dtype=torch.float32, device=dev)
    rgb = None if ref_img is None else torch.empty(H * W, 3, dtype=torch.uint8, device=dev)
    n = int(fuse_points_into(depth_avg, final_mask, ref_cam, ref_img, xyz, rgb).item())
    return xyz[:n], (None if rgb is None else rgb[:n])


# ---------------------------------------------------------------------------------
# opt-in per-point normals (not in the reference; include/aarmvs.h)
# ---------------------------------------------------------------------------------
NORMAL_DEFAULTS = dict(radius=2, max_rel_jump=0.01, min_count=3)


def normal_params(normals):
    """The ``normals`` argument of ``fuse_views`` and the drivers as ``estimate_normals``' keywords:
    None for False / None, the defaults for True, a dict of ``radius`` / ``max_rel_jump`` /
    ``min_count`` over the defaults."""
    if normals is None or normals is False:
        return None
    if normals is True:
        return dict(NORMAL_DEFAULTS)
    if not isinstance(normals, dict) or set(normals) - set(NORMAL_DEFAULTS):
        raise AarmvsError(f"aarmvs: normals must be a bool or a dict of {sorted(NORMAL_DEFAULTS)}, got {normals!r}")
    return {**NORMAL_DEFAULTS, **normals}


def pack_normal_cameras(ref_cam) -> np.ndarray:
    """K 3x3 (of the depth map's pixel grid) then inv(E) 4x4 as numpy forms it in float32, packed for
    ``aarmvs_fusion_normals``."""
    K, E = (np.asarray(m, np.float32) for m in ref_cam)
    out = np.ascontiguousarray(np.concatenate([K.ravel(), np.linalg.inv(E).ravel()]).astype(np.float32))
    assert out.size == _lib.FUSION_NORMAL_CAM_FLOATS
    return out


def estimate_normals(depth_avg, valid, ref_cam, radius=2, max_rel_jump=0.01, min_count=3):
    """Per-pixel world normals of a view's averaged depth map (``aarmvs_fusion_normals``,
    include/aarmvs.h): a float64 least-squares fit of 1/d = a x + b y + c over the (2 radius + 1)^2
    window's usable pixels -- those of ``valid`` with a finite depth > 0 within ``max_rel_jump``
    (relative) of the centre's -- needing ``min_count`` of them, not collinear.  ``depth_avg``: CUDA
    float64 [H,W]; ``valid``: CUDA bool / uint8 [H,W]; ``ref_cam``: (K, E) of the depth map's grid.
    ``max_rel_jump``'s default is the reference's relative depth threshold in
    check_geometric_consistency; ``min_count``'s is every solvable fit.  Returns (normal float32
    [H,W,3]: unit, facing the camera, (0,0,0) where there is none; has bool [H,W]) as CUDA tensors."""
    if not (isinstance(depth_avg, torch.Tensor) and depth_avg.is_cuda and depth_avg.dtype == torch.float64
            and depth_avg.dim() == 2):
        raise AarmvsError("aarmvs: estimate_normals needs the averaged depth as a CUDA float64 [H,W] tensor")
    dev = depth_avg.device
    if not (isinstance(valid, torch.Tensor) and valid.device == dev and valid.dtype in (torch.bool, torch.uint8)
            and valid.shape == depth_avg.shape):
        raise AarmvsError("aarmvs: estimate_normals needs the mask as a CUDA bool / uint8 [H,W] tensor of the "
                          "depth map's size")
    H, W = depth_avg.shape
    depth_avg, valid = depth_avg.contiguous(), valid.contiguous()
    cams = pack_normal_cameras(ref_cam)
    normal = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    has = torch.empty(H, W, dtype=torch.uint8, device=dev)
    a = _lib.FusionNormalsArgs()
    a.H, a.W = H, W
    a.depth, a.valid = depth_avg.data_ptr(), valid.data_ptr()
    a.cams = cams.ctypes.data
    a.radius, a.min_count = int(radius), int(min_count)
    a.max_rel_jump = float(max_rel_jump)
    a.normal, a.has_normal = normal.data_ptr(), has.data_ptr()
    with torch.cuda.device(dev):
        check(lib().aarmvs_fusion_normals(ctypes.byref(a), torch.cuda.current_stream().cuda_stream),
              "fusion_normals")
    return normal, has.bool()


def fuse_points_normals_gpu(depth_avg, final_mask, ref_cam, ref_img, normal_map):
    """``fuse_points_gpu`` with the kept pixels' normals (``aarmvs_fusion_points_normals``): (xyz
    float32 [n,3], rgb uint8 [n,3] or None, nrm float32 [n,3]), ``nrm`` = ``normal_map[mask]`` in
    pixel order, lined up with ``xyz`` and ``rgb``, which are ``fuse_points_gpu``'s bit for bit."""
    if not (isinstance(depth_avg, torch.Tensor) and depth_avg.is_cuda and depth_avg.dim() == 2):
        raise AarmvsError("aarmvs: fuse_points_gpu needs the averaged depth as a CUDA float64 [H,W] tensor")
    (H, W), dev = depth_avg.shape, depth_avg.device
    xyz = torch.empty(H * W, 3, dtype=torch.float32, device=dev)
    nrm = torch.empty(H * W, 3, dtype=torch.float32, device=dev)
    rgb = None if ref_img is None else torch.empty(H * W, 3, dtype=torch.uint8, device=dev)
    n = int(fuse_points_into(depth_avg, final_mask, ref_cam, ref_img, xyz, rgb, normal_map=normal_map,
                             nrm=nrm).item())
    return xyz[:n], (None if rgb is None else rgb[:n]), nrm[:n]


def _write_scan_ply(plyfilename, vertexs, vertex_colors, vertex_normals=None):
    """The drivers' last step: the views' points, colours and (with normals) normals, concatenated,
    to the PLY.  Returns the number of points."""
    xyz = np.concatenate(vertexs, axis=0) if vertexs else np.zeros((0, 3), np.float32)
    rgb = np.concatenate(vertex_colors, axis=0) if vertex_colors else np.zeros((0, 3), np.uint8)
    if vertex_normals is None:
        write_ply(plyfilename, xyz, rgb)
    else:
        nrm = np.concatenate(vertex_normals, axis=0) if vertex_normals else np.zeros((0, 3), np.float32)
        write_ply(plyfilename, xyz, rgb, nrm)
        print("points without a normal: {} of {}".format(int((~nrm.any(axis=1)).sum()), nrm.shape[0]))
    print("saving the final model to", plyfilename)
    return xyz.shape[0]


class _UsedMaps:
    """A scan's used maps (the visibility de-duplication's state): one zeroed CUDA uint8 map per
    view id, allocated when the view is first a reference or a source view."""

    def __init__(self):
        self.maps = {}

    def of(self, view, depth):
        if view not in self.maps:
            self.maps[view] = torch.zeros(depth.shape, dtype=torch.uint8, device=depth.device)
        return self.maps[view]


def fuse_views(pairs, depths, confidences, cams, images=None, photo_threshold=0.35, dedup=False, normals=False,
               require_normal=False):
    """Filter and fuse a scan held in memory.  ``pairs``: [(ref_view, [src_view, ...]), ...] in
    pair-file order; ``depths`` / ``confidences``: {view: CUDA float32 [H,W]}; ``cams``: {view: (K,
    E)}; ``images``: {view: CUDA float32 [H,W,3] in [0,1]} or None.  Reference views absent from
    ``depths`` are skipped.  Per reference view ``filter_depth_core`` (``dedup=False``: the cloud is
    the concatenation the file drivers write) or ``filter_depth_dedup`` on the scan's used maps
    (``dedup=True``: a view emits only the final pixels that no earlier view's consistent match
    marked), then ``fuse_points_gpu`` on the final / emit mask.  Returns a dict: ``xyz`` float32
    [n,3] and ``rgb`` uint8 [n,3] (None without images) CUDA tensors, ``masks`` {view: {"photo",
    "geo", "final"(, "emit"): bool [H,W]}}, ``avg`` {view: float64 [H,W]}, ``counts`` {view: points
    emitted} and, with ``dedup``, ``used`` {view: uint8 [H,W]} after the scan.  ``normals`` (True, or
    a dict of ``radius`` / ``max_rel_jump`` / ``min_count``): per view ``estimate_normals`` on the
    averaged depth and the FINAL mask -- also under ``dedup``: the emit mask only selects what is
    extracted, a de-duplicated view keeps its neighbours for the fit -- and the dict gains
    ``normals`` float32 [n,3] lined up with ``xyz``, ``normal_maps`` {view: float32 [H,W,3]} and
    ``has_normal`` {view: bool [H,W]}; everything else is bit for bit what it is without.
    ``require_normal`` (with ``normals``): extract only the pixels that have a normal."""
    used = _UsedMaps()
    masks, avgs, counts, verts, cols = {}, {}, {}, [], []
    nparams = normal_params(normals)
    if require_normal and nparams is None:
        raise AarmvsError("aarmvs: require_normal needs normals")
    nmaps, has_maps, nrms = {}, {}, []
    dev = None
    for ref_view, src_views in pairs:
        if ref_view not in depths:
            continue
        ref_depth = depths[ref_view]
        dev = ref_depth.device
        src_depths = [depths[v] for v in src_views]
        src_cams = [cams[v] for v in src_views]
        if dedup:
            photo, geo, final, emit, avg = filter_depth_dedup(
                ref_depth, confidences[ref_view], cams[ref_view], src_depths, src_cams, photo_threshold,
                used.of(ref_view, ref_depth), [used.of(v, depths[v]) for v in src_views])
            masks[ref_view] = dict(photo=photo, geo=geo, final=final, emit=emit)
        else:
            photo, geo, final, avg = filter_depth_core(ref_depth, confidences[ref_view], cams[ref_view],
                                                       src_depths, src_cams, photo_threshold)
            emit = final
            masks[ref_view] = dict(photo=photo, geo=geo, final=final)
        img = None if images is None else images[ref_view]
        if nparams is None:
            xyz, rgb = fuse_points_gpu(avg, emit, cams[ref_view], img)
        else:
            nmap, has = estimate_normals(avg, final, cams[ref_view], **nparams)
            nmaps[ref_view], has_maps[ref_view] = nmap, has
            xyz, rgb, nrm = fuse_points_normals_gpu(avg, emit & has if require_normal else emit, cams[ref_view],
                                                    img, nmap)
            nrms.append(nrm)
        avgs[ref_view], counts[ref_view] = avg, int(xyz.shape[0])
        verts.append(xyz)
        cols.append(rgb)
    if verts:
        xyz = torch.cat(verts)
        rgb = None if images is None else torch.cat(cols)
    else:
        xyz = torch.zeros(0, 3, dtype=torch.float32, device=dev)
        rgb = None if images is None else torch.zeros(0, 3, dtype=torch.uint8, device=dev)
    out = dict(xyz=xyz, rgb=rgb, masks=masks, avg=avgs, counts=counts)
    if dedup:
        out["used"] = used.maps
    if nparams is not None:
        out["normals"] = torch.cat(nrms) if nrms else torch.zeros(0, 3, dtype=torch.float32, device=dev)
        out["normal_maps"], out["has_normal"] = nmaps, has_maps
    return out


def read_camera_parameters_tnt(filename):
    """(intrinsics float32 3x3, extrinsics float32 4x4) of a cam.txt with intrinsics rows 0
    and 1 halved in float32 (fusion_padding.py:29-39: the maps are half the image's size)."""
    intrinsics, extrinsics = read_camera_parameters(filename)
    intrinsics[:2] /= 2
    return intrinsics, extrinsics


def filter_depth_tnt(scan_folder, out_folder, plyfilename, photo_threshold=0.3, device="cuda",
                     depth_dir=DEFAULT_DEPTH_DIR, conf_dir=DEFAULT_CONF_DIR, dedup=False, normals=None,
                     require_normal=False):
    """fusion_padding.py:137-266 for one scan.  Per reference view of pair.txt: the image goes
    to the GPU and through ``pyr_down``; rows [2:-2] are cropped from the reference and source
    depth maps and the confidence map (the padding loader's extra rows); ``filter_depth_core``
    runs with the halved cameras (with up to 10 source views its vote rule is
    fusion_padding.py's fixed one); ``fuse_points_gpu`` extracts the kept
    points.  Only the three masks (for the PNGs under out_folder/mask) and the kept points come
    back to the host.  Writes plyfilename and returns the number of points.  A reference view
    without a depth map is skipped (the reference stops with an error there).  ``depth_dir`` /
    ``conf_dir``, ``dedup``: as for ``filter_depth`` (the cropped depth maps stay on the GPU for the
    whole scan either way; with ``dedup`` the used maps do too).  ``normals``, ``require_normal``: as
    for ``filter_depth``; the fit runs on the cropped half-size maps with the halved intrinsics, the
    grid the points come from."""
    vertexs, vertex_colors, vertex_normals = [], [], []
    nparams = normal_params(normals)
    if require_normal and nparams is None:
        raise AarmvsError("aarmvs: require_normal needs normals")
    dev = torch.device(device)
    cam_file = os.path.join(scan_folder, "cams/{:0>8}_cam.txt")
    depth_file = os.path.join(out_folder, depth_dir, "{:0>8}.pfm")
    cache, used = {}, _UsedMaps()

    def cropped(path):
        return torch.from_numpy(np.ascontiguousarray(read_pfm(path)[0])).to(dev)[2:-2]

    def depth_of(view):
        if view not in cache:
            cache[view] = cropped(depth_file.format(view))
        return cache[view]

    for ref_view, src_views in read_pair_file(os.path.join(scan_folder, "pair.txt")):
        if not os.path.exists(depth_file.format(ref_view)):
            print("skip", ref_view)
            continue
        ref_cam = read_camera_parameters_tnt(cam_file.format(ref_view))
        ref_img = pyr_down(torch.from_numpy(
            read_img(os.path.join(scan_folder, "images/{:0>8}.jpg".format(ref_view)))).to(dev))
        ref_depth_est = depth_of(ref_view)
        confidence = cropped(os.path.join(out_folder, conf_dir, "{:0>8}.pfm".format(ref_view)))
        if tuple(ref_img.shape[:2]) != tuple(ref_depth_est.shape):
            raise AarmvsError(f"aarmvs: view {ref_view}: the halved image is {tuple(ref_img.shape[:2])} "
                              f"but the cropped depth map is {tuple(ref_depth_est.shape)}")
        src_cams = [read_camera_parameters_tnt(cam_file.format(v)) for v in src_views]
        if dedup:
            photo, geo, final, emit, avg = filter_depth_dedup(
                ref_depth_est, confidence, ref_cam, [depth_of(v) for v in src_views], src_cams, photo_threshold,
                used.of(ref_view, ref_depth_est), [used.of(v, depth_of(v)) for v in src_views])
            keep = emit
            emit = emit.cpu().numpy()
        else:
            photo, geo, final, avg = filter_depth_core(ref_depth_est, confidence, ref_cam,
                                                       [depth_of(v) for v in src_views], src_cams, photo_threshold)
            keep = final
        if nparams is None:
            xyz, rgb = fuse_points_gpu(avg, keep, ref_cam, ref_img)
        else:
            nmap, has = estimate_normals(avg, final, ref_cam, **nparams)
            xyz, rgb, nrm = fuse_points_normals_gpu(avg, keep & has if require_normal else keep, ref_cam, ref_img,
                                                    nmap)
            vertex_normals.append(nrm.cpu().numpy())
        photo, geo, final = (m.cpu().numpy() for m in (photo, geo, final))
        os.makedirs(os.path.join(out_folder, "mask"), exist_ok=True)
        save_mask(os.path.join(out_folder, "mask/{:0>8}_photo.png".format(ref_view)), photo)
        save_mask(os.path.join(out_folder, "mask/{:0>8}_geo.png".format(ref_view)), geo)
        save_mask(os.path.join(out_folder, "mask/{:0>8}_final.png".format(ref_view)), final)
        print("processing {}, ref-view{:0>2}, photo/geo/final-mask:{}/{}/{}".format(
            scan_folder, ref_view, photo.mean(), geo.mean(), final.mean()))
        if dedup:
            save_mask(os.path.join(out_folder, "mask/{:0>8}_emit.png".format(ref_view)), emit)
            print("  emit-mask:{}".format(emit.mean()))
        vertexs.append(xyz.cpu().numpy())
        vertex_colors.append(rgb.cpu().numpy())
    return _write_scan_ply(plyfilename, vertexs, vertex_colors, vertex_normals if nparams is not None else None)


# ---------------------------------------------------------------------------------
# file formats
# ---------------------------------------------------------------------------------
def read_img(filename):
    """float32 image in [0, 1] (fusion.py:45-50)."""
    from PIL import Image
    return np.array(Image.open(filename), dtype=np.float32) / 255.0


def save_mask(filename, mask):
    """8-bit PNG, 255 where the mask is set (fusion.py:52-56)."""
    from PIL import Image
    mask = np.asarray(mask)
    if mask.dtype != np.bool_:
        raise ValueError("save_mask: mask must be boolean")
    Image.fromarray(mask.astype(np.uint8) * 255).save(filename)
def read_camera_parameters(filename, scale=1.0, index=0, flag=0):
    """(intrinsics float32 3x3, extrinsics float32 4x4) of a cam.txt, intrinsics scaled and
    shifted for the resized / cropped image (fusion.py:27-42)."""
    with open(filename) as f:
        lines = [line.rstrip() for line in f.readlines()]
    extrinsics = np.array(" ".join(lines[1:5]).split(), dtype=np.float32).reshape((4, 4))
    intrinsics = np.array(" ".join(lines[7:10]).split(), dtype=np.float32).reshape((3, 3))
    intrinsics[:2, :] *= scale
    if flag == 0:
        intrinsics[0, 2] -= index
    else:
        intrinsics[1, 2] -= index
    return intrinsics, extrinsics


def read_pair_file(filename):
    """[(ref_view, [src_view, ...]), ...] (fusion.py:57-68)."""
    data = []
    with open(filename) as f:
        num_viewpoint = int(f.readline())
        for _ in range(num_viewpoint):
            ref_view = int(f.readline().rstrip())
            src_views = [int(x) for x in f.readline().rstrip().split()[1::2]]
            data.append((ref_view, src_views))
    return data


def write_ply(filename, xyz, rgb=None, normals=None):
    """Binary little-endian PLY of float32 x, y, z (+ float32 nx, ny, nz) (+ uint8 red, green, blue)
    vertices, the property order that MeshLab, Open3D and COLMAP read."""
    xyz = np.asarray(xyz, np.float32)
    n = xyz.shape[0]
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if rgb is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    v = np.empty(n, dtype=fields)
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if normals is not None:
        normals = np.asarray(normals, np.float32)
        if normals.shape != xyz.shape:
            raise ValueError("write_ply: normals must have xyz's shape")
        v["nx"], v["ny"], v["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
    if rgb is not None:
        rgb = np.asarray(rgb, np.uint8)
        v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    props = "".join(f"property {'float' if t == '<f4' else 'uchar'} {name}\n" for name, t in fields)
    header = f"ply\nformat binary_little_endian 1.0\nelement vertex {n}\n{props}end_header\n"
    with open(filename, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(v.tobytes())


# ---------------------------------------------------------------------------------
# command line (scripts/fusion_dtu.sh -> fusion.py, scripts/fusion_tnt.sh -> fusion_padding.py)
# ---------------------------------------------------------------------------------
DEFAULT_PHOTO_THRESHOLD = {"dtu": 0.35, "tnt": 0.3}   # fusion.py:285, fusion_padding.py:173


def build_parser():
    import argparse
    p = argparse.ArgumentParser(prog="python -m aarmvs.fusion",
                                description="Filter and fuse the depth maps of every scan of a list")
    p.add_argument("--test_dataset", choices=["dtu", "tnt"], required=True,
                   help="dtu: fusion.py's filter_depth; tnt: fusion_padding.py's")
    p.add_argument("--testpath", required=True, help="folder of the scans (pair.txt, cams/, images/)")
    p.add_argument("--testlist", required=True, help="text file, one scan name per line")
    p.add_argument("--outdir", required=True, help="folder of the per-scan depth_est_0/ and confidence_0/")
    p.add_argument("--photo_threshold", type=float, default=None,
                   help="confidence threshold (default: 0.35 for dtu, 0.3 for tnt)")
    p.add_argument("--depth_dir", default=DEFAULT_DEPTH_DIR,
                   help="per-scan folder of the depth maps (e.g. depth_refined_0 of eval_sharded --refine_depth)")
    p.add_argument("--conf_dir", default=DEFAULT_CONF_DIR,
                   help="per-scan folder of the confidence maps (e.g. confidence_window_0)")
    p.add_argument("--dedup", action="store_true",
                   help="visibility de-duplication: a view emits only the final pixels that no earlier view's "
                        "consistent match marked (off: the reference's cloud; DESIGN.md §4b)")
    p.add_argument("--normals", action="store_true",
                   help="per-point normals (nx ny nz in the PLY) from a window fit of every view's averaged depth "
                        "(off: the reference's cloud; DESIGN.md §4c)")
    p.add_argument("--normal_radius", type=int, choices=[1, 2, 3], default=NORMAL_DEFAULTS["radius"],
                   help="--normals: the fit's window is (2 r + 1)^2 pixels")
    p.add_argument("--normal_max_rel_jump", type=float, default=NORMAL_DEFAULTS["max_rel_jump"],
                   help="--normals: a neighbour takes part when its depth is within this (relative) of the centre's")
    p.add_argument("--normal_min_count", type=int, default=NORMAL_DEFAULTS["min_count"],
                   help="--normals: usable pixels a fit needs (3 .. (2 r + 1)^2)")
    p.add_argument("--require_normal", action="store_true",
                   help="--normals: emit only the pixels that have a normal (off: the point set does not change)")
    p.add_argument("--device", default="cuda")
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    if args.photo_threshold is None:
        args.photo_threshold = DEFAULT_PHOTO_THRESHOLD[args.test_dataset]
    if args.require_normal and not args.normals:
        build_parser().error("--require_normal needs --normals")
    return args


def ply_path(outdir, scan, test_dataset):
    """Where the scan's point cloud goes: outdir/<scan>.ply (fusion_padding.py:278,
    fusion.py:289), but for DTU's scanN folders the name the DTU evaluation reads,
    outdir/mvsnet_NNN_l3.ply (fusion.py:284-286)."""
    if test_dataset == "dtu" and scan.startswith("scan") and scan[4:].isdigit():
        return os.path.join(outdir, "mvsnet_{:0>3}_l3.ply".format(int(scan[4:])))
    return os.path.join(outdir, scan + ".ply")


def main(argv=None):
    args = parse_args(argv)
    with open(args.testlist) as f:
        scans = [line.rstrip() for line in f if line.strip()]
    for scan in scans:
        scan_folder = os.path.join(args.testpath, scan)
        out_folder = os.path.join(args.outdir, scan)
        ply = ply_path(args.outdir, scan, args.test_dataset)
        # (the folders, --dedup and --normals are passed on only when they are not the defaults: the default
        # call is the five-argument one it has always been)
        dirs = {}
        if (args.depth_dir, args.conf_dir) != (DEFAULT_DEPTH_DIR, DEFAULT_CONF_DIR):
            dirs = dict(depth_dir=args.depth_dir, conf_dir=args.conf_dir)
        if args.dedup:
            dirs["dedup"] = True
        if args.normals:
            dirs["normals"] = dict(radius=args.normal_radius, max_rel_jump=args.normal_max_rel_jump,
                                   min_count=args.normal_min_count)
            if args.require_normal:
                dirs["require_normal"] = True
        if args.test_dataset == "tnt":
            filter_depth_tnt(scan_folder, out_folder, ply, args.photo_threshold, args.device, **dirs)
        else:
            filter_depth(scan_folder, out_folder, ply, args.photo_threshold, args.device, **dirs)


if __name__ == "__main__":
    main()
