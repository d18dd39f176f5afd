"""Point-cloud evaluation on the synthetic scan: throughput of the GPU nearest-neighbour query beside
scipy's cKDTree on the same arrays, and the accuracy / completeness / F-score figures of the plain
and the de-duplicated fused cloud (``aarmvs.cloud_eval``).  Seeded, no files.

The scan is synthetic.fusion_views at 1184x1600 with 11 views, fused as tools/fusion_dedup_ab.py does
(every view lists the 10 others, per-view confidences from default_rng(seed + 100), threshold 0.35),
without and with ``dedup``.  The ground-truth cloud is synthetic.fusion_ground_truth of the same
views, every ``--gt-stride``-th point.  ONE child process
  (a) times ``aarmvs_cloud_nn`` alone (sorted inputs prepared once) and ``nn_distance`` whole (grid,
      keys, two sorts, gathers, query, un-permute) in both directions for both clouds: after a
      warm-up, ``--rounds`` windows of back-to-back calls, a device-event pair around each window, the
      calls per window chosen so that a window lasts about ``--window-s`` seconds;
  (b) times ``cKDTree(target).query(query, distance_upper_bound=max_dist, workers=16)`` on the same
      arrays with a host clock (build and query apart), and counts how many distances agree with the
      GPU's after the float32 cast;
  (c) records ``cloud_eval.evaluate`` of the plain and the de-duplicated cloud (and of the plain cloud
      down-sampled to ``--voxel``).
The bytes a query moves are ESTIMATED from the span sizes: over a sample of queries, the targets in
the 3x3 rows of rings 0 and 1 (what a query scans when it stops after ring 1, as most do here).

The parent process never opens the GPU; the child runs under its own ``timeout`` and nothing is
started after it fails.  Writes ``--out`` (default profiles/cloud_eval_ab.json) and prints it.

usage: python tools/cloud_eval_ab.py [--rounds 5] [--window-s 0.6] [--no-kdtree] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "aa-rmvsnet_amd")]

NSRC, THRESHOLD = 10, 0.35


def _window_us(fn, torch, rounds, window_s):
    """us per call of fn: warm-up, then `rounds` event-timed windows of back-to-back calls."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(3, min(500, int(math.ceil(window_s * 1e3 / max(1e-3, e0.elapsed_time(e1))))))
    us = []
    for _ in range(max(1, rounds)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1) / reps)
    med = statistics.median(us)
    return dict(median_us=round(med, 1), min_us=round(min(us), 1), max_us=round(max(us), 1), calls_per_window=reps,
                window_ms=round(med * reps / 1e3, 1))


def _span_estimate(torch, q_sorted, t_keys, origin, cell, sample=200000):
    """Mean number of targets in the 3x3 rows (x-span of 3 cells) around a query's cell, over a
    sample of in-grid queries, and the mean occupancy of an occupied target cell."""
    from aarmvs import cloud_eval as ce
    step = max(1, q_sorted.shape[0] // sample)
    qk = ce.cloud_keys(q_sorted[::step].contiguous(), origin, cell)
    qk = qk[qk != torch.iinfo(torch.int64).max]
    top = (1 << 21) - 1
    ix, iy, iz = qk & top, (qk >> 21) & top, qk >> 42
    total = torch.zeros_like(qk)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            y, z = iy + dy, iz + dz
            ok = (y >= 0) & (y <= top) & (z >= 0) & (z <= top)
            base = (z << 42) | (y << 21)
            lo = torch.searchsorted(t_keys, base | (ix - 1).clamp(min=0))
            hi = torch.searchsorted(t_keys, base | (ix + 1).clamp(max=top), right=True)
            total += torch.where(ok, hi - lo, torch.zeros_like(lo))
    in_grid = t_keys[t_keys != torch.iinfo(torch.int64).max]
    cells = int(torch.unique_consecutive(in_grid).shape[0])
    return float(total.double().mean()), (in_grid.shape[0] / max(1, cells)), int(qk.shape[0])


def child(args):
    import numpy as np
    import torch

    from aarmvs import cloud_eval as ce, fusion, synthetic as syn

    H, W = args.height, args.width
    dev = torch.device("cuda", 0)
    n = NSRC + 1
    depths, cams, _ = syn.fusion_views(H, W, NSRC, seed=args.seed)
    rng = np.random.default_rng(args.seed + 100)
    confs = {v: torch.from_numpy(rng.random((H, W)).astype(np.float32)).to(dev) for v in range(n)}
    depths = {v: torch.from_numpy(d).to(dev) for v, d in enumerate(depths)}
    pairs = [(v, [s for s in range(n) if s != v]) for v in range(n)]
    clouds = {}
    for form, dedup in (("plain", False), ("dedup", True)):
        clouds[form] = fusion.fuse_views(pairs, depths, confs, dict(enumerate(cams)), None, THRESHOLD,
                                         dedup=dedup)["xyz"].contiguous()
    del depths, confs
    gt_full = syn.fusion_ground_truth(H, W, NSRC)
    gt = torch.from_numpy(np.ascontiguousarray(gt_full[::args.gt_stride])).to(dev)
    res = dict(shape=dict(H=H, W=W, views=n, seed=args.seed, photo_threshold=THRESHOLD),
               clouds=dict(plain=int(clouds["plain"].shape[0]), dedup=int(clouds["dedup"].shape[0]),
                           ground_truth_full=int(gt_full.shape[0]), ground_truth=int(gt.shape[0]),
                           ground_truth_note=f"every {args.gt_stride}th point of fusion_ground_truth"),
               max_dist=args.max_dist, tau=list(args.tau))
    del gt_full
    max_dist = args.max_dist

    # (a) the GPU query, and (b) cKDTree on the same arrays
    timing = {}
    for form in ("plain", "dedup"):
        for direction, q, t in (("recon_to_gt", clouds[form], gt), ("gt_to_recon", gt, clouds[form])):
            origin, cell = ce.pick_grid([q, t], max_dist)
            t_sorted, t_keys, t_perm = ce._sorted_by_key(t, origin, cell)
            q_sorted, _, _ = ce._sorted_by_key(q, origin, cell)
            t_ids = t_perm.to(torch.int32)
            kern = _window_us(lambda: ce.nn_sorted(q_sorted, t_sorted, t_keys, t_ids, origin, cell, max_dist),
                              torch, args.rounds, args.window_s)
            whole = _window_us(lambda: ce.nn_distance(q, t, max_dist), torch, args.rounds, args.window_s)
            scanned, occupancy, sampled = _span_estimate(torch, q_sorted, t_keys, origin, cell)
            nq, m = int(q.shape[0]), int(t.shape[0])
            levels = math.log2(max(2, m))
            entry = dict(nq=nq, m=m, cell=cell, rings=math.ceil(max_dist / cell),
                         kernel=dict(**kern, queries_per_s=round(nq / (kern["median_us"] * 1e-6))),
                         nn_distance=dict(**whole, queries_per_s=round(nq / (whole["median_us"] * 1e-6))),
                         span_estimate=dict(
                             queries_sampled=sampled, mean_targets_in_rings_0_1=round(scanned, 2),
                             mean_targets_per_occupied_cell=round(occupancy, 2),
                             bytes_per_query_streamed=20,
                             bytes_per_query_scanned=round(24 * scanned, 1),
                             bytes_per_query_binary_search_keys=round(11 * 8 * levels, 1),
                             note="streamed: the query (12) and dist + index (8); scanned: key + point + id "
                                  "(24) per target of the 9 rows of rings 0 and 1; binary search: 11 searches of "
                                  "log2(m) keys, the upper levels shared by a wave and served from cache.  Queries "
                                  "that go beyond ring 1 scan more."))
            d_gpu, _ = ce.nn_distance(q, t, max_dist)
            d_gpu = d_gpu.cpu().numpy()
            del t_sorted, t_keys, t_perm, q_sorted, t_ids
            if not args.no_kdtree:
                from scipy.spatial import cKDTree
                qa, ta = q.cpu().numpy().astype(np.float64), t.cpu().numpy().astype(np.float64)
                t0 = time.perf_counter()
                tree = cKDTree(ta)
                t1 = time.perf_counter()
                d_kd, _ = tree.query(qa, k=1, distance_upper_bound=max_dist, workers=16)
                t2 = time.perf_counter()
                same = d_kd.astype(np.float32) == d_gpu
                entry["ckdtree"] = dict(workers=16, build_s=round(t1 - t0, 3), query_s=round(t2 - t1, 3),
                                        queries_per_s=round(nq / (t2 - t1)),
                                        queries_per_s_with_build=round(nq / (t2 - t0)),
                                        distances_equal_after_float32_cast=int(same.sum()), of=nq)
                entry["gpu_kernel_over_ckdtree_query"] = round((t2 - t1) / (kern["median_us"] * 1e-6), 1)
                entry["gpu_nn_distance_over_ckdtree_build_and_query"] = round(
                    (t2 - t0) / (whole["median_us"] * 1e-6), 1)
                del tree, qa, ta, d_kd
            timing[f"{form}.{direction}"] = entry
            print("TIMED " + json.dumps({f"{form}.{direction}": entry}), flush=True)
    res["nn"] = timing

    # (c) the figures this exists for (synthetic)
    ev = {}
    for name, cloud, voxel in (("plain", clouds["plain"], None), ("dedup", clouds["dedup"], None),
                               (f"plain_voxel_{args.voxel:g}", clouds["plain"], args.voxel)):
        t0 = time.perf_counter()
        ev[name] = ce.evaluate(cloud, gt, max_dist, args.tau, voxel)
        torch.cuda.synchronize()
        ev[name]["evaluate_wall_s"] = round(time.perf_counter() - t0, 3)
    res["evaluate"] = ev
    res["evaluate_note"] = ("SYNTHETIC scan and ground truth; plain figures, not the official DTU / Tanks and "
                            "Temples protocols (no masks, plane cut, reducePts, alignment or cropping)")
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--height", type=int, default=1184)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--gt-stride", type=int, default=8, help="keep every n-th ground-truth point")
    ap.add_argument("--max_dist", type=float, default=2.0)
    ap.add_argument("--tau", type=float, nargs="*", default=[0.25, 0.5, 1.0])
    ap.add_argument("--voxel", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per form")
    ap.add_argument("--window-s", type=float, default=0.6, help="aimed length of a window")
    ap.add_argument("--no-kdtree", action="store_true", help="skip the cKDTree comparison")
    ap.add_argument("--timeout", type=int, default=900, help="seconds for the child (its own `timeout`)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_eval_ab.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(child(args)))
        return
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:]
    line = []
    with subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True) as r:
        for ln in r.stdout:   # passed on as it comes: the child works for minutes
            if ln.startswith("RESULT "):
                line.append(ln)
            else:
                sys.stdout.write(ln)
                sys.stdout.flush()
    if r.returncode != 0 or not line:   # nothing more is started on the GPU after a failure
        raise SystemExit(f"cloud_eval_ab: the child failed (exit status {r.returncode})")
    res = dict(tool="cloud_eval_ab",
               timing="GPU: device events around windows of back-to-back calls after a warm-up; cKDTree: a host "
                      "clock around build and query, same arrays, same machine, 16 workers",
               **json.loads(line[-1][len("RESULT "):]))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
