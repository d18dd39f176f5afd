"""A/B of the fusion filter with and without the visibility de-duplication
(``aarmvs_fusion_filter`` / ``aarmvs_fusion_filter_dedup``).  Seeded, no files.

The scan is synthetic.fusion_views at 1184x1600 with 11 views (every view lists the 10 others,
ascending, as source views; per-view confidences from default_rng(seed + 100); threshold 0.35).
ONE child process
  * fuses the scan with ``fusion.fuse_views`` without and with ``dedup`` and records the point
    counts (per view and in all);
  * times the two launches of reference view 0 through the C ABI on preallocated buffers: after
    ``--warmup`` launches of each, ``--rounds`` rounds alternate a window of ``--reps`` plain
    launches and a window of ``--reps`` de-duplicating ones, a hipEvent pair around each window
    (at ~0.17 ms a launch, 5000 launches make a window of more than 0.8 s).  Recorded: us
    per launch of every window, the median and the spread (min, max) per form, and the ratio of
    the medians;
  * states the bytes the mode adds, from the shapes.
With ``--parent-lib FILE`` (a build of the parent commit's library) further children run bench.py's
``fusion_bench`` -- the ``fusion`` figure of ``bench.py --full`` -- alternately on that library and
on the in-tree one, ``--bench-runs`` times each: the off path launches the unchanged kernel, and the
two sets of figures are recorded side by side.

The parent process never opens the GPU: every child runs under its own ``timeout``, and nothing
more is started after a child that fails.  Writes ``--out`` (default
profiles/fusion_dedup_ab.json) and prints the same JSON on one line.

usage: python tools/fusion_dedup_ab.py [--rounds 7] [--reps 5000] [--parent-lib FILE] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "aa-rmvsnet_amd")]

H, W, NSRC, THRESHOLD = 1184, 1600, 10, 0.35


def child_kernels(seed, rounds, reps, warmup):
    import numpy as np
    import torch

    from aarmvs import _lib, fusion, lib, synthetic as syn

    dev = torch.device("cuda", 0)
    n = NSRC + 1
    depths, cams, _ = syn.fusion_views(H, W, NSRC, seed=seed)
    rng = np.random.default_rng(seed + 100)
    confs = {v: torch.from_numpy(rng.random((H, W)).astype(np.float32)).to(dev) for v in range(n)}
    depths = {v: torch.from_numpy(d).to(dev) for v, d in enumerate(depths)}
    cams = dict(enumerate(cams))
    pairs = [(v, [s for s in range(n) if s != v]) for v in range(n)]

    # the scan's point counts
    counts = {}
    for form, dedup in (("off", False), ("on", True)):
        out = fusion.fuse_views(pairs, depths, confs, cams, None, THRESHOLD, dedup=dedup)
        counts[form] = dict(points=int(out["xyz"].shape[0]), per_view=[out["counts"][v] for v in range(n)])
        if dedup:
            used_share = [round(float(out["used"][v].float().mean()), 4) for v in range(n)]
    del out
    torch.cuda.synchronize()

    # the two launches of reference view 0, on preallocated buffers
    ref, srcs = pairs[0]
    packed = fusion.pack_cameras(cams[ref], [cams[s] for s in srcs])
    u8 = lambda: torch.empty(H, W, dtype=torch.uint8, device=dev)  # noqa: E731
    photo, geo, final, emit = u8(), u8(), u8(), u8()
    avg = torch.empty(H, W, dtype=torch.float64, device=dev)
    used = [torch.zeros(H, W, dtype=torch.uint8, device=dev) for _ in range(n)]
    a = _lib.FusionArgs()
    a.H, a.W, a.nsrc = H, W, NSRC
    a.ref_depth, a.confidence = depths[ref].data_ptr(), confs[ref].data_ptr()
    for i, s in enumerate(srcs):
        a.src_depth[i] = depths[s].data_ptr()
    a.cams = packed.ctypes.data
    a.photo_threshold = float(np.float32(THRESHOLD))
    a.photo_mask, a.geo_mask, a.final_mask, a.depth_avg = (photo.data_ptr(), geo.data_ptr(), final.data_ptr(),
                                                           avg.data_ptr())
    d = _lib.FusionDedupArgs()
    d.used_ref = used[ref].data_ptr()
    for i, s in enumerate(srcs):
        d.used_src[i] = used[s].data_ptr()
    d.emit_mask = emit.data_ptr()
    L = lib()
    stream = torch.cuda.current_stream().cuda_stream
    launch = {"off": lambda: _lib.check(L.aarmvs_fusion_filter(ctypes.byref(a), stream), "fusion_filter"),
              "on": lambda: _lib.check(L.aarmvs_fusion_filter_dedup(ctypes.byref(a), ctypes.byref(d), stream),
                                       "fusion_filter_dedup")}
    # the mode leaves the plain outputs alone (view 0: nothing used yet, emit = final)
    launch["off"]()
    plain = [t.clone() for t in (photo, geo, final, avg)]
    launch["on"]()
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(plain, (photo, geo, final, avg))) and torch.equal(emit, final)
    final_px = int(final.sum())
    for f in ("off", "on"):
        for _ in range(max(1, warmup)):
            launch[f]()
    torch.cuda.synchronize()
    us = {"off": [], "on": []}
    for _ in range(max(1, rounds)):
        for f in ("off", "on"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                launch[f]()
            e1.record()
            torch.cuda.synchronize()
            us[f].append(1e3 * e0.elapsed_time(e1) / reps)
    med = {f: statistics.median(us[f]) for f in us}
    px = H * W
    return dict(
        shape=dict(H=H, W=W, views=n, nsrc=NSRC, seed=seed, photo_threshold=THRESHOLD),
        scan_points=dict(off=counts["off"]["points"], on=counts["on"]["points"],
                         ratio=round(counts["on"]["points"] / max(1, counts["off"]["points"]), 4),
                         per_view_off=counts["off"]["per_view"], per_view_on=counts["on"]["per_view"],
                         used_share_per_view=used_share),
        kernel_us_per_launch={f: dict(median=round(med[f], 2), min=round(min(us[f]), 2), max=round(max(us[f]), 2),
                                      windows=[round(v, 2) for v in us[f]]) for f in us},
        window_ms={f: round(med[f] * reps / 1e3, 1) for f in us},
        dedup_over_plain=round(med["on"] / med["off"], 4),
        extra_us_per_launch=round(med["on"] - med["off"], 2),
        plain_outputs_bit_identical=bool(same), final_pixels_view0=final_px,
        bytes_added=dict(
            per_launch_streamed=2 * px, per_launch_streamed_note="used_ref read + emit_mask written, 1 B per pixel each",
            per_launch_mark_stores_at_most=NSRC * final_px,
            per_launch_mark_stores_note="one 1-byte store per final pixel and consistent source view",
            plain_algorithmic_bytes_per_launch=(19 + 4 * NSRC) * px,
            per_scan_used_maps=n * px, per_scan_resident_depth_maps=4 * n * px))


def child_bench(reps, parent):
    import torch

    import bench
    if parent:   # the parent commit's library has no de-duplicating entry point to bind
        from aarmvs import _lib
        _lib.SIGNATURES.pop("aarmvs_fusion_filter_dedup")
    r = bench.fusion_bench(H, W, NSRC, torch.device("cuda", 0), False, reps=reps)
    return dict(ms_per_view=r["ms_per_view"], frac=r["frac"])


def run_child(argv, seconds, env=None):
    cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__)] + argv
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:   # nothing more is started on the GPU after a failure
        sys.stdout.write(r.stdout)
        raise SystemExit(f"fusion_dedup_ab: {' '.join(argv)} failed (exit status {r.returncode})")
    return json.loads(line[-1][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=7, help="timed windows per form")
    ap.add_argument("--reps", type=int, default=5000, help="launches per window")
    ap.add_argument("--warmup", type=int, default=50, help="warm-up launches per form")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libaarmvs.so, for the bench.py figure")
    ap.add_argument("--bench-runs", type=int, default=4, help="fusion_bench runs per library")
    ap.add_argument("--bench-reps", type=int, default=200, help="launches per fusion_bench run")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child (its own `timeout`)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fusion_dedup_ab.json"))
    ap.add_argument("--child", choices=["kernels", "bench", "bench_parent"], default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child == "kernels":
        print("RESULT " + json.dumps(child_kernels(args.seed, args.rounds, args.reps, args.warmup)))
        return
    if args.child in ("bench", "bench_parent"):
        print("RESULT " + json.dumps(child_bench(args.bench_reps, args.child == "bench_parent")))
        return
    common = ["--seed", str(args.seed), "--rounds", str(args.rounds), "--reps", str(args.reps), "--warmup",
              str(args.warmup), "--bench-reps", str(args.bench_reps)]
    res = dict(tool="fusion_dedup_ab",
               timing="kernels: hipEvents around windows of back-to-back launches through the C ABI, plain and "
                      "de-duplicating windows alternated in one process; bench: bench.py fusion_bench, one process "
                      "per run, the two libraries alternated",
               **run_child(["--child", "kernels"] + common, args.timeout))
    print(json.dumps(res), flush=True)
    if args.parent_lib:
        env_parent = dict(os.environ, AARMVS_LIB=os.path.abspath(args.parent_lib))
        env_tree = {k: v for k, v in os.environ.items() if k != "AARMVS_LIB"}
        runs = {"parent": [], "this": []}
        for _ in range(max(1, args.bench_runs)):
            runs["parent"].append(run_child(["--child", "bench_parent"] + common, args.timeout, env_parent)["ms_per_view"])
            runs["this"].append(run_child(["--child", "bench"] + common, args.timeout, env_tree)["ms_per_view"])
        res["bench_fusion_ms_per_view"] = dict(
            what="bench.py fusion_bench (the `fusion` figure of bench.py --full; the plain filter) at "
                 f"{W}x{H}, {NSRC} source views, {args.bench_reps} launches per run",
            parent=dict(runs=runs["parent"], median=round(statistics.median(runs["parent"]), 4)),
            this=dict(runs=runs["this"], median=round(statistics.median(runs["this"]), 4)),
            this_within_parent_spread=bool(min(runs["parent"]) <= statistics.median(runs["this"]) <= max(runs["parent"])))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
