"""Timing of the fusion step's opt-in per-point normals (``aarmvs_fusion_normals``,
``aarmvs_fusion_points_normals``).  Seeded, no files.

The view is reference view 0 of synthetic.fusion_views at 1184x1600 with 10 source views
(confidences from default_rng(seed + 100), threshold 0.35): its averaged depth and final mask come
from one ``aarmvs_fusion_filter`` launch.  ONE child process
  * times, through the C ABI on preallocated buffers, the normals launch for r = 1, 2, 3 and -- as
    the yardstick of the same session -- the plain filter launch: after ``--warmup`` launches of
    each, ``--rounds`` rounds take the four forms in turn, a window of ``--reps`` back-to-back
    launches each, a hipEvent pair around every window.  Recorded: us per launch of every window,
    the median and the spread (min, max) per form, the algorithmic bytes and the rate they imply;
  * times ``aarmvs_fusion_points`` against ``aarmvs_fusion_points_normals`` the same way (same
    mask, same rounds, alternating), and checks that xyz and rgb are the same bits;
  * records how many final pixels get a normal per radius.
With ``--parent-lib FILE`` (a build of the parent commit's library) further children run bench.py's
``fusion_bench`` -- the ``fusion`` figure of ``bench.py --full`` -- alternately on that library and
on the in-tree one, ``--bench-runs`` times each: with the normals off the filter launch is the
unchanged kernel, and the two sets of figures are recorded side by side.

The parent process never opens the GPU: every child runs under its own ``timeout``, and nothing
more is started after a child that fails.  Writes ``--out`` (default
profiles/fusion_normals_ab.json) and prints the same JSON on one line.

usage: python tools/fusion_normals_ab.py [--rounds 7] [--reps 2000] [--parent-lib FILE] [--out FILE]
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
NEW_SYMBOLS = ("aarmvs_fusion_normals", "aarmvs_fusion_points_normals")


def _windows(launch, forms, rounds, reps, warmup):
    """{form: [us per launch of every window]}: the forms in turn, ``rounds`` times."""
    import torch
    for f in forms:
        for _ in range(max(1, warmup)):
            launch[f]()
    torch.cuda.synchronize()
    us = {f: [] for f in forms}
    for _ in range(max(1, rounds)):
        for f in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                launch[f]()
            e1.record()
            torch.cuda.synchronize()
            us[f].append(1e3 * e0.elapsed_time(e1) / reps)
    return us


def _stats(us, reps, nbytes=None):
    med = statistics.median(us)
    out = dict(median=round(med, 2), min=round(min(us), 2), max=round(max(us), 2), windows=[round(v, 2) for v in us],
               window_ms=round(med * reps / 1e3, 1))
    if nbytes is not None:
        out["algorithmic_bytes"] = int(nbytes)
        out["algorithmic_TB_per_s"] = round(nbytes / (med * 1e-6) / 1e12, 3)
    return out


def child_kernels(seed, rounds, reps, warmup):
    import numpy as np
    import torch

    from aarmvs import _lib, fusion, lib, synthetic as syn

    dev = torch.device("cuda", 0)
    n = NSRC + 1
    depths, cams, _ = syn.fusion_views(H, W, NSRC, seed=seed)
    rng = np.random.default_rng(seed + 100)
    conf = torch.from_numpy(rng.random((H, W)).astype(np.float32)).to(dev)
    depths = [torch.from_numpy(d).to(dev) for d in depths]
    img = torch.from_numpy(np.random.default_rng(seed + 200).random((H, W, 3)).astype(np.float32)).to(dev)
    L = lib()
    stream = torch.cuda.current_stream().cuda_stream
    px = H * W

    # the plain filter launch of view 0: the yardstick, and the normals' inputs
    packed = fusion.pack_cameras(cams[0], cams[1:])
    u8 = lambda: torch.empty(H, W, dtype=torch.uint8, device=dev)  # noqa: E731
    photo, geo, final = u8(), u8(), u8()
    avg = torch.empty(H, W, dtype=torch.float64, device=dev)
    fa = _lib.FusionArgs()
    fa.H, fa.W, fa.nsrc = H, W, NSRC
    fa.ref_depth, fa.confidence = depths[0].data_ptr(), conf.data_ptr()
    for i in range(NSRC):
        fa.src_depth[i] = depths[1 + i].data_ptr()
    fa.cams = packed.ctypes.data
    fa.photo_threshold = float(np.float32(THRESHOLD))
    fa.photo_mask, fa.geo_mask, fa.final_mask, fa.depth_avg = (photo.data_ptr(), geo.data_ptr(), final.data_ptr(),
                                                               avg.data_ptr())
    launch = {"filter": lambda: _lib.check(L.aarmvs_fusion_filter(ctypes.byref(fa), stream), "fusion_filter")}
    launch["filter"]()
    torch.cuda.synchronize()
    final_px = int(final.sum())

    # the normals launches
    ncams = fusion.pack_normal_cameras(cams[0])
    normal = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    has = u8()
    share = {}
    for r in (1, 2, 3):
        a = _lib.FusionNormalsArgs()
        a.H, a.W = H, W
        a.depth, a.valid, a.cams = avg.data_ptr(), final.data_ptr(), ncams.ctypes.data
        a.radius, a.min_count, a.max_rel_jump = r, 3, 0.01
        a.normal, a.has_normal = normal.data_ptr(), has.data_ptr()
        launch[f"normals_r{r}"] = (lambda a=a: _lib.check(L.aarmvs_fusion_normals(ctypes.byref(a), stream),
                                                          "fusion_normals"))
        launch[f"normals_r{r}"]()
        torch.cuda.synchronize()
        share[f"r{r}"] = round(int(has.sum()) / max(1, final_px), 5)
    launch["normals_r2"]()          # the map the points pass copies from: r = 2
    torch.cuda.synchronize()
    forms = ["filter", "normals_r1", "normals_r2", "normals_r3"]
    us = _windows(launch, forms, rounds, reps, warmup)
    nbytes = {"filter": (19 + 4 * NSRC) * px}
    for r in (1, 2, 3):
        nbytes[f"normals_r{r}"] = (9 + 13) * px          # halo re-reads not counted
    kernels = {f: _stats(us[f], reps, nbytes[f]) for f in forms}

    # the points pass without and with the normals
    pcams = fusion.pack_point_cameras(cams[0])
    cap = px
    xyz = [torch.empty(cap, 3, dtype=torch.float32, device=dev) for _ in range(2)]
    rgb = [torch.empty(cap, 3, dtype=torch.uint8, device=dev) for _ in range(2)]
    nxyz = torch.empty(cap, 3, dtype=torch.float32, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    work = torch.empty(max(1, L.aarmvs_fusion_points_workspace_bytes(H, W)), dtype=torch.uint8, device=dev)
    pa = []
    for i in range(2):
        p = _lib.FusionPointsArgs()
        p.H, p.W = H, W
        p.mask, p.depth, p.color = final.data_ptr(), avg.data_ptr(), img.data_ptr()
        p.cams = pcams.ctypes.data
        p.xyz, p.rgb, p.capacity = xyz[i].data_ptr(), rgb[i].data_ptr(), cap
        p.count, p.workspace = count.data_ptr(), work.data_ptr()
        pa.append(p)
    plaunch = {
        "points": lambda: _lib.check(L.aarmvs_fusion_points(ctypes.byref(pa[0]), stream), "fusion_points"),
        "points_normals": lambda: _lib.check(L.aarmvs_fusion_points_normals(
            ctypes.byref(pa[1]), normal.data_ptr(), nxyz.data_ptr(), stream), "fusion_points_normals")}
    plaunch["points"]()
    plaunch["points_normals"]()
    torch.cuda.synchronize()
    kept = int(count.item())
    same = bool(torch.equal(xyz[0][:kept].view(torch.int32), xyz[1][:kept].view(torch.int32))
                and torch.equal(rgb[0][:kept], rgb[1][:kept])
                and torch.equal(nxyz[:kept].view(torch.int32), normal[final.bool()].view(torch.int32)))
    pus = _windows(plaunch, ["points", "points_normals"], rounds, reps, warmup)
    pbytes = {"points": px + 35 * kept, "points_normals": px + 59 * kept}
    points = {f: _stats(pus[f], reps, pbytes[f]) for f in pus}
    return dict(
        shape=dict(H=H, W=W, nsrc=NSRC, seed=seed, photo_threshold=THRESHOLD, final_pixels=final_px,
                   final_share=round(final_px / px, 4)),
        normals_parameters=dict(max_rel_jump=0.01, min_count=3, valid="the final mask"),
        final_pixels_with_a_normal=share,
        kernel_us_per_launch=kernels,
        normals_r2_over_filter=round(kernels["normals_r2"]["median"] / kernels["filter"]["median"], 4),
        points_us_per_launch=points,
        points_normals_over_points=round(points["points_normals"]["median"] / points["points"]["median"], 4),
        points_extra_us=round(points["points_normals"]["median"] - points["points"]["median"], 2),
        points_outputs_bit_identical=same, kept_pixels=kept)


def child_bench(reps, parent):
    import torch

    import bench
    if parent:   # the parent commit's library has no normals entry points to bind
        from aarmvs import _lib
        for name in NEW_SYMBOLS:
            _lib.SIGNATURES.pop(name)
    r = bench.fusion_bench(H, W, NSRC, torch.device("cuda", 0), False, reps=reps)
    return dict(ms_per_view=r["ms_per_view"], frac=r["frac"])


def run_child(argv, seconds, env=None):
    cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__)] + argv
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:   # nothing more is started on the GPU after a failure
        sys.stdout.write(r.stdout)
        raise SystemExit(f"fusion_normals_ab: {' '.join(argv)} failed (exit status {r.returncode})")
    return json.loads(line[-1][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=7, help="timed windows per form")
    ap.add_argument("--reps", type=int, default=2000, help="launches per window")
    ap.add_argument("--warmup", type=int, default=50, help="warm-up launches per form")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libaarmvs.so, for the bench.py figure")
    ap.add_argument("--bench-runs", type=int, default=4, help="fusion_bench runs per library")
    ap.add_argument("--bench-reps", type=int, default=200, help="launches per fusion_bench run")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child (its own `timeout`)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fusion_normals_ab.json"))
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
    res = dict(tool="fusion_normals_ab",
               timing="kernels and points: hipEvents around windows of back-to-back launches through the C ABI, the "
                      "forms taken in turn in one process; bench: bench.py fusion_bench, one process per run, the "
                      "two libraries alternated",
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
            what="bench.py fusion_bench (the `fusion` figure of bench.py --full; the plain filter, normals off) at "
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
