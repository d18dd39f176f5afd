"""Times the Tanks and Temples fusion additions at the T&T frame (1080x1920 image, 540x960
maps, 10 source views): ``pyr_down`` and ``aarmvs_fusion_points`` per reference view (device
events), the whole GPU path to host arrays (upload, kernels, count, kept points back), and the
host path the DTU driver's way would need for the same output (D2H of the float64 average and
the mask, numpy ``fuse_points``, the numpy pyrDown restatement).  Prints one JSON line and,
with an output folder, writes it to <out>/fusion_tnt_time.json.
usage: python tools/fusion_tnt_time.py [reps] [out_folder]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "aa-rmvsnet_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fusion_tnt_ref as tr  # noqa: E402
from aarmvs import fusion, synthetic as syn  # noqa: E402

HBM_PEAK_GBS = 8000.0     # HBM3E spec, as bench.py
IMG_H, IMG_W, H, W, NSRC = 1080, 1920, 540, 960, 10


def device_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def host_ms(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    out_dir = sys.argv[2] if len(sys.argv) > 2 else None
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    dev = torch.device("cuda", 0)
    depths, cams, conf = syn.fusion_views(H, W, NSRC, seed=7)
    t = [torch.from_numpy(d).to(dev) for d in depths]
    _, _, final, avg = fusion.filter_depth_core(t[0], torch.from_numpy(conf).to(dev), cams[0], t[1:], cams[1:], 0.3)
    img_np = np.random.default_rng(0).integers(0, 256, (IMG_H, IMG_W, 3)).astype(np.float32) / np.float32(255)
    img = torch.from_numpy(img_np).to(dev)
    half = fusion.pyr_down(img)
    xyz = torch.empty(H * W, 3, dtype=torch.float32, device=dev)
    rgb = torch.empty(H * W, 3, dtype=torch.uint8, device=dev)
    kept = int(fusion.fuse_points_into(avg, final, cams[0], half, xyz, rgb).item())

    pyr_ms = device_ms(lambda: fusion.pyr_down(img), reps)
    pts_ms = device_ms(lambda: fusion.fuse_points_into(avg, final, cams[0], half, xyz, rgb), reps)

    def gpu_path():       # image up, pyramid, points, kept points back
        h = fusion.pyr_down(torch.from_numpy(img_np).to(dev))
        p, c = fusion.fuse_points_gpu(avg, final, cams[0], h)
        return p.cpu().numpy(), c.cpu().numpy()

    def host_path():      # average and mask down, numpy pyramid and points
        h = tr.pyr_down(img_np)
        return fusion.fuse_points(avg.cpu().numpy(), final.cpu().numpy(), cams[0], h)

    gp, gc = gpu_path()
    hp, hc = host_path()
    same = bool(np.array_equal(gp, hp) and np.array_equal(gc, hc))
    host_reps = max(1, reps // 10)
    gpu_wall = host_ms(gpu_path, host_reps)
    host_wall = host_ms(host_path, host_reps)
    host_d2h = host_ms(lambda: (avg.cpu(), final.cpu()), host_reps)
    host_pyr = host_ms(lambda: tr.pyr_down(img_np), host_reps)
    avg_np, final_np = avg.cpu().numpy(), final.cpu().numpy()
    half_np = half.cpu().numpy()
    host_pts = host_ms(lambda: fusion.fuse_points(avg_np, final_np, cams[0], half_np), host_reps)

    pyr_bytes = 4.0 * 3 * (IMG_H * IMG_W + IMG_H * IMG_W / 4)
    pts_bytes = 1.0 * H * W + (8 + 12 + 12 + 3) * kept
    res = dict(
        workload=f"{IMG_H}x{IMG_W} image, {H}x{W} maps, {NSRC} source views", reps=reps, kept_points=kept,
        kept_share=round(kept / (H * W), 4), gpu_equals_host=same,
        pyr_down_ms=round(pyr_ms, 4), pyr_down_bytes=pyr_bytes,
        pyr_down_hbm_frac=round(pyr_bytes / (pyr_ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4),
        fusion_points_ms=round(pts_ms, 4), fusion_points_bytes=pts_bytes,
        fusion_points_hbm_frac=round(pts_bytes / (pts_ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4),
        gpu_path_wall_ms=round(gpu_wall, 3), host_path_wall_ms=round(host_wall, 3),
        host_d2h_ms=round(host_d2h, 3), host_numpy_pyr_down_ms=round(host_pyr, 3),
        host_numpy_fuse_points_ms=round(host_pts, 3), hbm_peak_gbs=HBM_PEAK_GBS)
    line = json.dumps(res)
    print(line, flush=True)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "fusion_tnt_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
