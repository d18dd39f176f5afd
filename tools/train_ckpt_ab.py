"""Time and peak memory of the training step with and without plane-segment checkpointing
(``EMVSNet(checkpoint_planes=S)``), in one process.

Default: config 4's frame and planes (640x512, N = 3, D = 192, one sample), the seeded synthetic
inputs of ``bench.train_bench``, ONE model whose ``checkpoint_planes`` is switched between steps
(the same weights, sweep workspace and backward scratch for every variant).  Variants 0 (the
whole record, the un-checkpointed path as it is), 16, 48 and 96, alternated 0/16/48/96/0/...:
``--warmup`` rounds first, then ``--steps`` timed rounds (at least 5).  Per step: a host clock
around a device synchronise, and torch.cuda.max_memory_allocated from a peak reset before the
step.  Per variant the JSON has ms_per_step (median; every sample is listed) and peak_bytes (max),
K = ceil(D / S) and the derived bound step(0) + 1.15 (K - 1) / K F, with F the recorded forward
alone: device events around ``_SweepTrain.forward`` in extra variant-0 steps after the timed ones.

``--frame 1184x1600 --planes 192 --checkpoint_planes 32``: one timed step at that frame with that
segment length only, after one warm-up step whose time (the process's one-time initialisation:
code objects, MIOpen's search for FeatNet's convolutions at the new shape) is reported beside it.
The un-checkpointed variant is not tried there: its record's bytes come from the size helper and
are printed beside the device's memory.

Prints one JSON line; ``--out FILE`` also writes it (indented).
usage: python tools/train_ckpt_ab.py [--steps 5] [--warmup 1] [--out FILE]
       python tools/train_ckpt_ab.py --frame 1184x1600 --planes 192 --checkpoint_planes 32 [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "aa-rmvsnet_amd")]
import torch  # noqa: E402

from aarmvs import ops, synthetic as syn  # noqa: E402
from models import drmvsnet  # noqa: E402

VARIANTS = (0, 16, 48, 96)
N = 3


def make_step(dev, H, W, D):
    """bench.train_bench's step: seeded images and scene, random-init weights, mvsnet_cls_loss"""
    B = 1
    g = torch.Generator(device="cpu").manual_seed(0)
    imgs = torch.randn(B, N, 3, H, W, generator=g).to(dev)
    sc = syn.scene(B, N, H, W, D, seed=0)
    proj = torch.from_numpy(sc["proj_matrices"]).to(dev)
    torch.manual_seed(0)
    model = drmvsnet.EMVSNet(D, image_scale=1.0, max_h=H, max_w=W, evidential=False).to(dev).train()
    dv = torch.from_numpy(sc["depth_values"]).to(dev)
    depth_gt = dv[:, D // 2].reshape(B, 1, 1).expand(B, H, W).contiguous()
    mask = torch.ones(B, H, W, device=dev)

    def step(S):
        model.checkpoint_planes = S
        model.zero_grad(set_to_none=True)
        prob, _, _ = model(imgs, proj, dv)
        loss = drmvsnet.mvsnet_cls_loss(prob, depth_gt, mask, dv)[0]
        loss.backward()
        return loss

    return model, step


def measured(step, S, dev):
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    t0 = time.perf_counter()
    loss = step(S)
    torch.cuda.synchronize(dev)
    ms = (time.perf_counter() - t0) * 1e3
    return ms, torch.cuda.max_memory_allocated(dev), float(loss.detach())


def recorded_forward_ms(step, dev, reps=3):
    """F: device time of _SweepTrain.forward alone (events around it) in variant-0 steps"""
    orig = drmvsnet._SweepTrain.forward
    spans = []

    def timed(ctx, *args):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = orig(ctx, *args)
        b.record()
        spans.append((a, b))
        return out

    drmvsnet._SweepTrain.forward = staticmethod(timed)
    try:
        for _ in range(reps):
            step(0)
        torch.cuda.synchronize(dev)
    finally:
        drmvsnet._SweepTrain.forward = staticmethod(orig)
    return statistics.median(a.elapsed_time(b) for a, b in spans)


def sizes(H, W, D, S):
    rec, ck = ops.DepthSweep.record_bytes(1, H, W, min(S, D) if S else D, nsrc=N - 1)
    K = -(-D // S) if S else 1
    return dict(record_bytes=rec, checkpoint_bytes=ck if S else 0, checkpoints=K - 1, segments=K)


def run_ab(dev, H, W, D, steps, warmup):
    model, step = make_step(dev, H, W, D)
    for _ in range(max(1, warmup)):
        for S in VARIANTS:
            step(S)
    samples = {S: [] for S in VARIANTS}
    for _ in range(max(5, steps)):
        for S in VARIANTS:
            samples[S].append(measured(step, S, dev))
    F = recorded_forward_ms(step, dev)
    base = statistics.median(m for m, _, _ in samples[0])
    losses = {l for v in samples.values() for _, _, l in v}
    out = dict(tool="train_ckpt_ab", config=f"{W}x{H}, N={N}, D={D}, 1 sample", timed_steps=max(5, steps),
               warmup_rounds=max(1, warmup), timing="host clock around a device synchronise, per step",
               recorded_forward_ms=round(F, 2), same_loss_every_step=len(losses) == 1, variants=[])
    for S in VARIANTS:
        ms = [m for m, _, _ in samples[S]]
        sz = sizes(H, W, D, S)
        K = sz["segments"]
        v = dict(checkpoint_planes=S, ms_per_step=round(statistics.median(ms), 2),
                 ms_samples=[round(m, 2) for m in ms], peak_bytes=max(p for _, p, _ in samples[S]), **sz)
        if S:
            v["bound_ms"] = round(base + 1.15 * (K - 1) / K * F, 2)
            v["within_bound"] = v["ms_per_step"] <= v["bound_ms"]
        out["variants"].append(v)
    return out


def run_single(dev, H, W, D, S):
    """one timed step (after one warm-up step) at a frame where only the checkpointed variant is tried"""
    if S <= 0:
        raise SystemExit("--frame needs --checkpoint_planes S > 0: the un-checkpointed variant is not tried there")
    total = torch.cuda.get_device_properties(dev).total_memory
    whole = sizes(H, W, D, 0)["record_bytes"]
    model, step = make_step(dev, H, W, D)
    first_ms, first_peak, _ = measured(step, S, dev)   # the process's first step: one-time initialisation
    ms, peak, loss = measured(step, S, dev)
    finite = all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    return dict(tool="train_ckpt_ab", config=f"{W}x{H}, N={N}, D={D}, 1 sample", timed_steps=1, warmup_rounds=1,
                timing="host clock around a device synchronise; one step after one warm-up step",
                first_step_ms=round(first_ms, 2),
                variants=[dict(checkpoint_planes=S, ms_per_step=round(ms, 2), peak_bytes=max(peak, first_peak),
                               **sizes(H, W, D, S))],
                loss=loss, loss_and_grads_finite=finite and loss == loss,
                unchecked_variant=dict(checkpoint_planes=0, record_bytes=whole, device_bytes=total,
                                       fits=whole < total,
                                       note=f"not run: its record alone is {whole / 1e9:.1f} GB against the "
                                            f"device's {total / 1e9:.1f} GB"
                                            + ("" if whole < total else ", it does not fit")))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5, help="timed rounds (at least 5)")
    ap.add_argument("--warmup", type=int, default=1, help="warm-up rounds (at least 1)")
    ap.add_argument("--frame", default=None, help="HxW of a single checkpointed step, e.g. 1184x1600")
    ap.add_argument("--planes", type=int, default=192)
    ap.add_argument("--checkpoint_planes", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    if args.frame:
        H, W = (int(v) for v in args.frame.lower().split("x"))
        res = run_single(dev, H, W, args.planes, args.checkpoint_planes)
        if not res["unchecked_variant"]["fits"]:
            print(f"checkpoint_planes=0 at {W}x{H}, D={args.planes}: {res['unchecked_variant']['note']}",
                  file=sys.stderr)
    else:
        res = run_ab(dev, 512, 640, args.planes, args.steps, args.warmup)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
