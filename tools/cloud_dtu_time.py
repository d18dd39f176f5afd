"""The DTU protocol on the synthetic scan: rounds and time of the GPU thinning (``aarmvs.cloud_eval.thin``)
beside the sequential walk on the host, and the time of ``regions`` and of the whole ``evaluate_dtu``
(DESIGN.md §4e).  Seeded, no files.

The scan is tools/cloud_eval_ab.py's: synthetic.fusion_views at 1184x1600 with 11 views fused plain
(every view lists the 10 others, confidences from default_rng(seed + 100), threshold 0.35), against
every ``--gt-stride``-th point of synthetic.fusion_ground_truth.  ONE child process
  (a) estimates the scan's point spacing: the median distance from every 16th point to its nearest
      point among the others (``nn_distance``); the thinning radius is ``--spacing-factor`` times that;
  (b) times ``thin`` whole (bounds, keys, the sort, the gathers, the rounds, the final sort of the kept
      indices; host clock around a synchronised call, median of ``--rounds`` calls after a warm-up) and
      the rounds alone on the prepared key-sorted cloud (``thin_sorted``: device events around each
      ``aarmvs_cloud_thin`` call, at 8 rounds per call and at 1 round per call for the per-round times
      and the number of undecided points after each round);
  (c) times ``regions`` (device events around windows of back-to-back calls) and ``evaluate_dtu`` (host
      clock) with a synthetic observation mask on the ground truth's bounds and a plane through the
      ground truth's median depth;
  (d) walks a spatial crop of the scan (the ``--crop`` points nearest the scan's centre in x, so the
      density is the scan's) sequentially on the host: ``cKDTree.query_ball_point`` of all its points
      with 16 workers, then the walk in rank order in Python; the same crop with the same ranks goes
      through ``thin`` and the two kept sets are compared.  The host time for the full cloud is NOT
      measured; ``host_full_cloud_extrapolated_s`` scales the crop's time by the point counts.

The parent process never opens the GPU; the child runs under its own ``timeout`` and nothing is
started after it fails.  Writes ``--out`` (default profiles/cloud_dtu_ab.json) and prints it.

usage: python tools/cloud_dtu_time.py [--rounds 5] [--crop 400000] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "aa-rmvsnet_amd"), os.path.join(ROOT, "tools")]

NSRC, THRESHOLD = 10, 0.35


def _host_ms(fn, torch, rounds):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(max(1, rounds)):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return dict(median_ms=round(statistics.median(ms), 2), min_ms=round(min(ms), 2), max_ms=round(max(ms), 2),
                calls=len(ms))


def child(args):
    import numpy as np
    import torch

    from aarmvs import cloud_eval as ce, fusion, synthetic as syn
    from cloud_eval_ab import _window_us

    H, W = args.height, args.width
    dev = torch.device("cuda", 0)
    n = NSRC + 1
    depths, cams, _ = syn.fusion_views(H, W, NSRC, seed=args.seed)
    rng = np.random.default_rng(args.seed + 100)
    confs = {v: torch.from_numpy(rng.random((H, W)).astype(np.float32)).to(dev) for v in range(n)}
    depths = {v: torch.from_numpy(d).to(dev) for v, d in enumerate(depths)}
    pairs = [(v, [s for s in range(n) if s != v]) for v in range(n)]
    recon = fusion.fuse_views(pairs, depths, confs, dict(enumerate(cams)), None, THRESHOLD)["xyz"].contiguous()
    del depths, confs
    gt = torch.from_numpy(np.ascontiguousarray(syn.fusion_ground_truth(H, W, NSRC)[::args.gt_stride])).to(dev)
    nr = int(recon.shape[0])
    res = dict(shape=dict(H=H, W=W, views=n, seed=args.seed, photo_threshold=THRESHOLD),
               clouds=dict(recon=nr, ground_truth=int(gt.shape[0]),
                           ground_truth_note=f"every {args.gt_stride}th point of fusion_ground_truth"))

    # (a) the spacing and the radius
    pick = torch.zeros(nr, dtype=torch.bool, device=dev)
    pick[::16] = True
    d, _ = ce.nn_distance(recon[pick], recon[~pick], args.max_dist)
    spacing = float(d[torch.isfinite(d)].median())
    radius = float(np.float32(args.spacing_factor * spacing))
    res["spacing"] = dict(median_nn_of_every_16th_point_to_the_others=spacing, factor=args.spacing_factor,
                          radius=radius)
    print("SPACING " + json.dumps(res["spacing"]), flush=True)
    del pick, d

    # (b) thin: whole, and the rounds alone
    kept, rounds = ce.thin(recon, radius, seed=args.seed)
    whole = _host_ms(lambda: ce.thin(recon, radius, seed=args.seed), torch, args.rounds)
    rank = torch.from_numpy(np.random.default_rng(args.seed).permutation(nr).astype(np.int32)).to(dev)
    lo, hi = ce._bounds([recon])
    cell = max(radius, float((hi - lo).max()) / (ce.AXIS_CELLS - 2))
    t0 = time.perf_counter()
    s_xyz, s_keys, perm = ce._sorted_by_key(recon, lo, cell)
    s_rank = rank[perm].contiguous()
    torch.cuda.synchronize()
    prepare_ms = 1e3 * (time.perf_counter() - t0)
    by8 = []
    ce.thin_sorted(s_xyz, s_keys, s_rank, lo, cell, radius, 8)
    state8, rounds8 = ce.thin_sorted(s_xyz, s_keys, s_rank, lo, cell, radius, 8, log=by8)
    loop8 = _host_ms(lambda: ce.thin_sorted(s_xyz, s_keys, s_rank, lo, cell, radius, 8), torch, args.rounds)
    by1 = []
    state1, rounds1 = ce.thin_sorted(s_xyz, s_keys, s_rank, lo, cell, radius, 1, log=by1)
    assert rounds8 == rounds1 == rounds and torch.equal(state8, state1)
    assert torch.equal(torch.sort(perm[state1 == 1]).values, kept)
    in_grid = int((s_keys != torch.iinfo(torch.int64).max).sum())
    res["thin"] = dict(
        radius=radius, cell=cell, kept=int(kept.shape[0]), of=nr, rounds=int(rounds),
        whole_call_host=whole, keys_sort_gathers_host_ms=round(prepare_ms, 2),
        rounds_alone_at_8_per_call=dict(host=loop8, calls=len(by8),
                                        device_ms_per_call=[round(c[2], 3) for c in by8],
                                        device_ms_total=round(sum(c[2] for c in by8), 3)),
        rounds_alone_at_1_per_call=dict(device_ms_per_round=[round(c[2], 3) for c in by1],
                                        undecided_after_round=[int(c[1]) for c in by1],
                                        undecided_before_round_1=in_grid,
                                        device_ms_total=round(sum(c[2] for c in by1), 3)),
        note="whole_call: bounds, keys, the stable sort, two gathers, the rounds (8 per call, one readback per "
             "call), the final sort of the kept indices; a call's device time covers the init kernel (first "
             "call), its rounds and the one-block reduce")
    print("THIN " + json.dumps(res["thin"]), flush=True)
    del s_xyz, s_keys, s_rank, perm, state8, state1

    # (c) regions and evaluate_dtu on a synthetic mask and plane
    g = gt.cpu().numpy()
    bb = np.stack([g.min(0), g.max(0)]).astype(np.float64)
    mres = float((bb[1] - bb[0]).max() / 255.0)
    dims = (np.floor((bb[1] - bb[0]) / mres) + 1).astype(int)
    mask = (np.random.default_rng(args.seed + 1).random(tuple(dims)) < 0.7).astype(np.uint8)
    plane = np.float64([0, 0, 1, -float(np.median(g[:, 2]))])
    md = torch.from_numpy(mask).to(dev)
    reg = _window_us(lambda: ce.regions(recon, md, bb, mres, args.patch, plane), torch, args.rounds, 0.3)
    res["regions"] = dict(points=nr, mask_dims=[int(v) for v in dims], **reg,
                          points_per_s=round(nr / (reg["median_us"] * 1e-6)))
    ev_kw = dict(thin=radius, patch=args.patch, max_dist=args.max_dist, seed=args.seed)
    out = ce.evaluate_dtu(recon, gt, md, bb, mres, plane, **ev_kw)
    res["evaluate_dtu"] = dict(result=out, host=_host_ms(lambda: ce.evaluate_dtu(recon, gt, md, bb, mres, plane, **ev_kw),
                                                         torch, max(1, args.rounds // 2)),
                               note="SYNTHETIC scan, ground truth, mask (a seeded pattern, 70 % set) and plane: the "
                                    "figures exercise the protocol and are not DTU scores")
    print("EVAL " + json.dumps(res["evaluate_dtu"]), flush=True)

    # (d) the sequential walk on the host, on a spatial crop
    if not args.no_host:
        from scipy.spatial import cKDTree
        x = recon[:, 0]
        order = torch.argsort((x - x.median()).abs())[:min(args.crop, nr)]
        crop = recon[torch.sort(order).values].contiguous()
        nc = int(crop.shape[0])
        crank = np.random.default_rng(args.seed).permutation(nc)
        p = crop.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        tree = cKDTree(p)
        t1 = time.perf_counter()
        balls = tree.query_ball_point(p, radius, workers=16)
        t2 = time.perf_counter()
        gone, want = np.zeros(nc, bool), np.zeros(nc, bool)
        for i in np.argsort(crank):
            if not gone[i]:
                want[i] = True
                gone[balls[i]] = True
        t3 = time.perf_counter()
        neighbours = float(np.mean([len(b) for b in balls[::97]]) - 1)
        del balls, tree
        gpu = _host_ms(lambda: ce.thin(crop, radius, order=torch.from_numpy(crank.astype(np.int32))), torch, args.rounds)
        idx, crounds = ce.thin(crop, radius, order=torch.from_numpy(crank.astype(np.int32)))
        got = np.zeros(nc, bool)
        got[idx.cpu().numpy()] = True
        host_s = t3 - t0
        res["host_walk"] = dict(
            crop_points=nc, crop_note="the points nearest the scan's median x: a slab at the scan's own density",
            mean_neighbours_within_radius=round(neighbours, 1),
            ckdtree_build_s=round(t1 - t0, 3), query_ball_point_16_workers_s=round(t2 - t1, 3),
            python_walk_s=round(t3 - t2, 3), host_total_s=round(host_s, 3),
            gpu_thin_same_crop=gpu, gpu_rounds=int(crounds),
            host_over_gpu=round(host_s / (gpu["median_ms"] * 1e-3), 1),
            kept_host=int(want.sum()), kept_gpu=int(got.sum()), kept_sets_differ_at=int((want != got).sum()),
            host_full_cloud_extrapolated_s=round(host_s * nr / nc, 1),
            note="cKDTree compares float64 distances it forms its own way; a point within an ulp of the radius "
                 "may fall on the other side (kept_sets_differ_at counts the points whose fate differs)")
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--height", type=int, default=1184)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--gt-stride", type=int, default=8, help="keep every n-th ground-truth point")
    ap.add_argument("--max_dist", type=float, default=2.0)
    ap.add_argument("--patch", type=float, default=6.0)
    ap.add_argument("--spacing-factor", type=float, default=2.0, help="radius = this times the median spacing")
    ap.add_argument("--crop", type=int, default=400000, help="points of the host walk's crop")
    ap.add_argument("--rounds", type=int, default=5, help="timed calls per figure")
    ap.add_argument("--no-host", action="store_true", help="skip the host walk")
    ap.add_argument("--timeout", type=int, default=540, help="seconds for the child (its own `timeout`)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_dtu_ab.json"))
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
        raise SystemExit(f"cloud_dtu_time: the child failed (exit status {r.returncode})")
    res = dict(tool="cloud_dtu_time",
               timing="thin and evaluate_dtu: a host clock around synchronised calls after a warm-up; the rounds: "
                      "device events around each aarmvs_cloud_thin call; regions: device events around windows of "
                      "back-to-back calls; the host walk: a host clock, same machine, 16 workers for the tree",
               **json.loads(line[-1][len("RESULT "):]))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
