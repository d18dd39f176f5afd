"""A/B of the inference sweep with and without the depth-posterior statistics
(``DepthSweep.__call__(want_posterior=...)``, aarmvs_sweep_ex).

Per config (default: the headline, 1600x1184, N = 7, D = 512; bench.py's seeded inputs and the
real weights) ONE process runs both forms alternately on ONE DepthSweep (the same packed weights,
workspace and state buffer): ``--warmup`` rounds off/on, then ``--steps`` timed rounds (a host
clock around a device synchronise per sweep, both streams on), then one sweep of each form under
the library's event profiler on one stream (each figure is the kernel's isolated duration, as in
bench.py's timing pass).  Recorded per config: ms per sweep (median; every sample listed), the
head kernel's us per launch in both forms, the statistics' finalize's us (counted under the
profiler's "refine" id), and a description of the four maps (their means, the share of NaN
pixels, whether the mean lies inside the depth range) -- not an accuracy figure: there is no
ground truth here.

The parent process never opens the GPU: it runs each config as a child under its own ``timeout``
and stops at the first child that fails.  Writes ``--out`` (default profiles/posterior_ab.json) and
prints the same JSON on one line.

usage: python tools/posterior_ab.py [--steps 3] [--warmup 1] [--planes 0] [--out FILE]
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

CONFIGS = ("dtu_eval_1600x1184_n7_d512",)
FORMS = ("off", "on")


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

    def step(form):
        return sweep(ref, srcs, proj[:, 0], src_proj, dv, want_depth=True, want_posterior=form == "on")

    for _ in range(max(1, warmup)):
        for f in FORMS:
            step(f)
    torch.cuda.synchronize()
    ms = {f: [] for f in FORMS}
    outs = {}
    for _ in range(max(1, steps)):
        for f in FORMS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = step(f)
            torch.cuda.synchronize()
            ms[f].append((time.perf_counter() - t0) * 1e3)
            outs[f] = {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}
    # per-kernel pass: one stream, an event pair around every launch
    sweep.overlap = False
    prof = {}
    ops.profile_enable(True)
    try:
        for f in FORMS:
            ops.profile_reset()
            step(f)
            torch.cuda.synchronize()
            prof[f] = ops.profile_read()
    finally:
        ops.profile_enable(False)
        ops.profile_reset()
    sweep.overlap = True

    def us(f, name):
        n, total = prof[f].get(name, (0, 0.0))
        return round(1e3 * total / n, 2) if n else None

    plane_us = {f: round(sum(1e3 * t for _, t in prof[f].values()) / D, 1) for f in FORMS}
    on, off = outs["on"], outs["off"]
    nan = torch.isnan(on["depth_std"])
    ok = ~nan
    lo, hi = float(dv.min()), float(dv.max())
    med = {f: statistics.median(ms[f]) for f in FORMS}
    return dict(
        config=config, shape=dict(B=1, N=N, H=H, W=W, D=D),
        ms_per_sweep={f: round(med[f], 2) for f in FORMS},
        ms_samples={f: [round(v, 2) for v in ms[f]] for f in FORMS},
        sweep_ratio=round(med["on"] / med["off"], 4),
        head_wta_us_per_launch={f: us(f, "head_wta") for f in FORMS},
        posterior_finalize_us=us("on", "refine"), finalize_us=us("on", "finalize"),
        kernels_us_per_plane=plane_us,
        outputs=dict(
            wta_outputs_bit_identical=bool(torch.equal(on["depth"], off["depth"]) and torch.equal(on["conf"], off["conf"])),
            nan_pixels=float(nan.float().mean()),
            nan_exactly_where_conf_is=bool(all(torch.equal(torch.isnan(on[k]), torch.isnan(on["conf"]))
                                               for k in ops.POSTERIOR_KEYS)),
            mean_inside_depth_range=bool(((on["depth_mean"][ok] >= lo) & (on["depth_mean"][ok] <= hi)).all()),
            depth_range=[lo, hi], mean_depth_std=float(on["depth_std"][ok].mean()),
            mean_abs_mean_minus_wta=float((on["depth_mean"][ok] - on["depth"][ok]).abs().mean()),
            mean_entropy_nats=float(on["entropy"][ok].mean()), ln_D=round(float(torch.tensor(float(D)).log()), 4),
            mean_conf=float(on["conf"][ok].mean()), mean_runner_up=float(on["runner_up"][ok].mean())))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=3, help="timed rounds per form")
    ap.add_argument("--warmup", type=int, default=1, help="warm-up rounds per form")
    ap.add_argument("--planes", type=int, default=0, help="limit D (0: the config's)")
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per config (its own `timeout`)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_ab.json"))
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
            raise SystemExit(f"posterior_ab: {config} failed (exit status {r.returncode})")
        results.append(json.loads(line[-1][len("RESULT "):]))
    res = dict(tool="posterior_ab", forms=list(FORMS), timed_rounds=max(1, args.steps), warmup_rounds=max(1, args.warmup),
               timing="ms_per_sweep: host clock around a device synchronise, both forms alternated in one process on "
                      "one DepthSweep; kernels: one sweep per form on one stream, hipEvents per launch",
               weights="tests/golden/real_weights_sweep.npz", configs=results)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
