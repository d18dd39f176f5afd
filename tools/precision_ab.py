"""A/B of the inference sweep's precision modes (``DepthSweep.precision``: "split", the parity
mode, against "fp16", one matrix product per fp32 product in the cells and deconvs).

Per config (default: the headline, 1600x1184, N = 7, D = 512, and config 2, 800x600, N = 5,
D = 256; bench.py's seeded inputs and the real weights) ONE process runs both modes alternately on
ONE DepthSweep (the same packed weights and workspace): ``--warmup`` rounds split/fp16, then
``--steps`` timed rounds (a host clock around a device synchronise per sweep, both streams on),
then one sweep of each mode under the library's event profiler on one stream (each figure is the
kernel's isolated duration, as in bench.py's timing pass).  Recorded per config: ms per sweep
(median; every sample listed), the per-kernel us per launch of the five cells and the two deconvs
in both modes and their ratios, the sum over a plane, and the depth rel-L1 / share of pixels whose
plane changed / largest confidence difference between the two modes' outputs.

The parent process never opens the GPU: it runs each config as a child under its own
``timeout`` and stops at the first child that fails.  Writes ``--out`` (default
profiles/fp16_mode_ab.json) and prints the same JSON on one line.

usage: python tools/precision_ab.py [--steps 3] [--warmup 1] [--planes 0] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "aa-rmvsnet_amd")]

CONFIGS = ("dtu_eval_1600x1184_n7_d512", "dtu_eval_800x600_n5_d256")
MODES = ("split", "fp16")
UNITS = ["lstm_cell0", "lstm_cell1", "lstm_cell2", "lstm_cell3", "lstm_cell4", "deconv0", "deconv1"]


def child(config, steps, warmup, planes):
    import torch

    import bench
    from aarmvs import ops

    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = dict(bench.CONFIGS[config])
    if planes:
        cfg["D"] = min(cfg["D"], planes)
    N, H, W, D = cfg["N"], cfg["H"], cfg["W"], cfg["D"]
    P = {k: torch.from_numpy(v).to(dev) for k, v in bench.real_weights().items()}
    _, proj, dv, feats = bench.make_inputs(cfg, 1, seed=0, device=dev)
    sweep = ops.DepthSweep(P, dev)
    ref, srcs, src_proj = feats[0], list(feats[1:]), list(proj[:, 1:].unbind(1))

    def step(mode):
        sweep.precision = mode
        return sweep(ref, srcs, proj[:, 0], src_proj, dv, want_depth=True)

    for _ in range(max(1, warmup)):
        for m in MODES:
            step(m)
    torch.cuda.synchronize()
    ms = {m: [] for m in MODES}
    outs = {}
    for _ in range(max(1, steps)):
        for m in MODES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = step(m)
            torch.cuda.synchronize()
            ms[m].append((time.perf_counter() - t0) * 1e3)
            outs[m] = (out["depth"].clone(), out["conf"].clone())
    # per-kernel pass: one stream, an event pair around every launch
    sweep.overlap = False
    prof = {}
    ops.profile_enable(True)
    try:
        for m in MODES:
            ops.profile_reset()
            step(m)
            torch.cuda.synchronize()
            prof[m] = ops.profile_read()
    finally:
        ops.profile_enable(False)
        ops.profile_reset()
    sweep.overlap = True

    def us(m, name):
        n, total = prof[m].get(name + ("_fp16" if m == "fp16" else ""), (0, 0.0))
        return 1e3 * total / n if n else None

    kernels = {}
    for name in UNITS:
        a, b = us("split", name), us("fp16", name)
        kernels[name] = dict(split_us=round(a, 2), fp16_us=round(b, 2), ratio=round(b / a, 3))
    per_plane = {m: {} for m in MODES}
    for m in MODES:   # cells 3 and 4 are launched per batch element (B = 1 here): one launch per plane
        cells = sum(us(m, f"lstm_cell{k}") for k in range(5))
        dec = us(m, "deconv0") + us(m, "deconv1")
        other = sum(1e3 * t for k, (n, t) in prof[m].items() if k.split("_fp16")[0] not in UNITS) / D
        per_plane[m] = dict(cells_us=round(cells, 1), deconvs_us=round(dec, 1), other_us=round(other, 1))
    d3, c3 = outs["split"]
    d16, c16 = outs["fp16"]
    med = {m: statistics.median(ms[m]) for m in MODES}
    return dict(
        config=config, shape=dict(B=1, N=N, H=H, W=W, D=D),
        ms_per_sweep={m: round(med[m], 2) for m in MODES},
        ms_samples={m: [round(v, 2) for v in ms[m]] for m in MODES},
        sweep_ratio=round(med["fp16"] / med["split"], 3),
        ghyp_per_s={m: round(H * W * D / med[m] / 1e6, 4) for m in MODES},
        kernels_us_per_launch=kernels, per_plane_us=per_plane,
        cells_ratio=round(per_plane["fp16"]["cells_us"] / per_plane["split"]["cells_us"], 3),
        cells_and_deconvs_ratio=round(
            (per_plane["fp16"]["cells_us"] + per_plane["fp16"]["deconvs_us"])
            / (per_plane["split"]["cells_us"] + per_plane["split"]["deconvs_us"]), 3),
        outputs=dict(
            depth_rel_l1=float((d16 - d3).abs().sum() / d3.abs().sum()),
            pixels_that_change_plane=float((d16 != d3).float().mean()),
            conf_max_abs_diff=float((c16 - c3).abs().max()),
            finite=bool(torch.isfinite(d16).all() and torch.isfinite(c16).all())))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=3, help="timed rounds per mode")
    ap.add_argument("--warmup", type=int, default=1, help="warm-up rounds per mode")
    ap.add_argument("--planes", type=int, default=0, help="limit D (0: the config's)")
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per config (its own `timeout`)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp16_mode_ab.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(child(args.child, args.steps, args.warmup, args.planes)))
        return
    results = []
    for config in args.configs:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", config,
               "--steps", str(args.steps), "--warmup", str(args.warmup), "--planes", str(args.planes)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:   # nothing more is started on the GPU after a failure
            sys.stdout.write(r.stdout)
            raise SystemExit(f"precision_ab: {config} failed (exit status {r.returncode})")
        results.append(json.loads(line[-1][len("RESULT "):]))
    res = dict(tool="precision_ab", modes=list(MODES), timed_rounds=max(1, args.steps), warmup_rounds=max(1, args.warmup),
               timing="ms_per_sweep: host clock around a device synchronise, both modes alternated in one process on "
                      "one DepthSweep; kernels: one sweep per mode on one stream, hipEvents per launch",
               weights="tests/golden/real_weights_sweep.npz", configs=results)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
