"""CPU restatement of the Tanks and Temples fusion step (fusion_padding.py) -- TEST
INFRASTRUCTURE.  Only tests/ and the timing tools may import this module; the product path
(aarmvs.fusion) runs the HIP kernels and never falls back to it.

Follows, part by part:
  pyr_down                    cv2.pyrDown(img) on a float32 image, restated from OpenCV's
                              published scalar algorithm (imgproc/src/pyramids.cpp, PyrDownInvoker
                              with FltCast<float, 8>): per source row r[x] = s[2x]*6 + (s[2x-1] +
                              s[2x+1])*4 + s[2x-2] + s[2x+2], the same down the rows, * (1/256), sums
                              left to right in float32, BORDER_REFLECT_101.  cv2 is not installed
                              and its SIMD paths may associate the sums differently: agreement with
                              cv2 itself is parity unpinned.
  read_camera_parameters      fusion_padding.py:29-39 (intrinsics rows 0 and 1 halved)
  filter_depth_core           fusion_padding.py:173-218 (all nine thresholds counted, >= 10)
  fuse_points                 fusion_padding.py:239-251
  filter_depth_scan           fusion_padding.py:137-266 on in-memory inputs
check_geometric_consistency is the same function in fusion.py and fusion_padding.py: it comes
from oracle.fusion_oracle.
"""
import numpy as np

from oracle import fusion_oracle as fo


def _reflect101(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def _taps(at):
    six, four = np.float32(6), np.float32(4)
    v = at(0) * six + (at(-1) + at(1)) * four
    v = v + at(-2)
    return v + at(2)


def pyr_down(img):
    """cv2.pyrDown(img): float32 [H,W] or [H,W,C] -> [(H+1)//2, (W+1)//2(, C)]."""
    img = np.asarray(img, np.float32)
    H, W = img.shape[:2]
    assert H >= 4 and W >= 4
    xs = 2 * np.arange((W + 1) // 2)
    rows = _taps(lambda k: img[:, _reflect101(xs + k, W)])
    ys = 2 * np.arange((H + 1) // 2)
    out = _taps(lambda k: rows[_reflect101(ys + k, H)]) * np.float32(1.0 / 256.0)
    assert out.dtype == np.float32
    return out


def read_camera_parameters(text):
    """fusion_padding.py:29-39 on the text of a cam.txt."""
    lines = [ln.rstrip() for ln in text.splitlines()]
    extrinsics = np.array(" ".join(lines[1:5]).split(), dtype=np.float32).reshape((4, 4))
    intrinsics = np.array(" ".join(lines[7:10]).split(), dtype=np.float32).reshape((3, 3))
    intrinsics[:2][:] /= 2
    return intrinsics, extrinsics


def filter_depth_core(ref_depth, confidence, ref_cam, src_depths, src_cams, photo_threshold=0.3):
    """fusion_padding.py:173-218 for one reference view: (photo_mask, geo_mask, final_mask,
    depth_est_averaged)."""
    ref_K, ref_E = ref_cam
    photo_mask = confidence > np.float32(photo_threshold)
    geo_mask_sum = 0
    geo_mask_sums = []
    all_srcview_depth_ests = []
    ct = 0
    for src_depth, (K, E) in zip(src_depths, src_cams):
        ct = ct + 1
        masks, geo_mask, depth_reprojected, _, _, _ = fo.check_geometric_consistency(
            ref_depth, ref_K, ref_E, src_depth, K, E)
        if ct == 1:
            for i in range(2, 11):
                geo_mask_sums.append(masks[i - 2].astype(np.int32))
        else:
            for i in range(2, 11):
                geo_mask_sums[i - 2] += masks[i - 2].astype(np.int32)
        geo_mask_sum += geo_mask.astype(np.int32)
        all_srcview_depth_ests.append(depth_reprojected)
    geo_mask = geo_mask_sum >= 10
    for i in range(2, 11):
        geo_mask = np.logical_or(geo_mask, geo_mask_sums[i - 2] >= i)
    depth_est_averaged = (sum(all_srcview_depth_ests) + ref_depth) / (geo_mask_sum + 1)
    final_mask = np.logical_and(photo_mask, geo_mask)
    return photo_mask, geo_mask, final_mask, depth_est_averaged


def fuse_points(depth_est_averaged, final_mask, ref_cam, ref_img):
    """fusion_padding.py:239-251: (xyz_world float64 [n,3], colours uint8 [n,3])."""
    ref_intrinsics, ref_extrinsics = ref_cam
    height, width = depth_est_averaged.shape[:2]
    x, y = np.meshgrid(np.arange(0, width), np.arange(0, height))
    valid_points = final_mask
    x, y, depth = x[valid_points], y[valid_points], depth_est_averaged[valid_points]
    color = ref_img[:, :, :][valid_points]
    xyz_ref = np.matmul(np.linalg.inv(ref_intrinsics), np.vstack((x, y, np.ones_like(x))) * depth)
    xyz_world = np.matmul(np.linalg.inv(ref_extrinsics), np.vstack((xyz_ref, np.ones_like(x))))[:3]
    return xyz_world.transpose((1, 0)), (color * 255).astype(np.uint8)


def filter_depth_scan(pair_data, images, cam_texts, depth_ests, confidences, photo_threshold=0.3):
    """fusion_padding.py:137-266 on in-memory inputs: pair_data [(ref, [src...])], images {view:
    float32 [H,W,3] in [0,1]}, cam_texts {view: cam.txt text}, depth_ests / confidences {view:
    float32 maps as stored, with the padding loader's 2 extra rows above and below}.  Reference
    views without a depth map are skipped (the driver's documented deviation).  Returns (masks
    {ref: (photo, geo, final)}, xyz float32 [n,3] as the PLY's 'f4' fields store it, rgb uint8
    [n,3])."""
    masks, verts, cols = {}, [], []
    for ref_view, src_views in pair_data:
        if ref_view not in depth_ests:
            continue
        ref_cam = read_camera_parameters(cam_texts[ref_view])
        ref_img = pyr_down(images[ref_view])
        ref_depth = depth_ests[ref_view][2:-2, :]
        conf = confidences[ref_view][2:-2, :]
        src_d = [depth_ests[s][2:-2, :] for s in src_views]
        src_c = [read_camera_parameters(cam_texts[s]) for s in src_views]
        photo, geo, final, avg = filter_depth_core(ref_depth, conf, ref_cam, src_d, src_c, photo_threshold)
        masks[ref_view] = (photo, geo, final)
        xyz, rgb = fuse_points(avg, final, ref_cam, ref_img)
        verts.append(xyz)
        cols.append(rgb)
    return masks, np.concatenate(verts).astype(np.float32), np.concatenate(cols)
