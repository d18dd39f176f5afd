"""Times the training loss at the cost-volume shape of config 4's training step (B = 1,
D = 192, 512x640, as ``bench.py --train``): the unfused chain (``softmax_depth`` +
``mvsnet_cls_loss`` + backward to dL/dcost, the path of ``EMVSNet`` + ``mvsnet_cls_loss``) against
the fused one (``mvsnet_cls_loss_from_cost``: aarmvs_cls_loss + aarmvs_cls_loss_backward), in one
process, alternated A/B/A/B.  Per path: the time per call from device events around ``reps``
back-to-back calls after a warm-up, and torch.cuda.max_memory_allocated over one call from a
reset peak (above what the inputs hold).  For the fused kernels: the library's per-kernel event
times and their achieved bytes/s against the algorithmic bytes (forward 4 B D HW read, backward
8 B D HW) and the HBM peak.  Before timing, both paths are checked against a float64 evaluation
of the same inputs on the CPU with the tests' bounds (loss: max(2 x the unfused path's error,
1e-6 relative); dL/dcost: relative L2 max(2 x the unfused path's, 1e-6)), at a smaller frame so
the CPU autograd stays short, and for equality of loss and WTA depth at the timed frame.
Prints one JSON line and, with an output folder, writes it to <out>/cls_loss_time.json.
usage: python tools/cls_loss_time.py [reps] [out_folder]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "aa-rmvsnet_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from aarmvs import ops, synthetic as syn  # noqa: E402
from models.drmvsnet import _SoftmaxDepth, mvsnet_cls_loss, mvsnet_cls_loss_from_cost  # noqa: E402

HBM_PEAK_GBS = 8000.0     # HBM3E spec, as bench.py
B, D, H, W = 1, 192, 512, 640
ROUNDS = 3                # A/B/A/B...: the reported time of a path is the median of its rounds


def inputs(h, w, dev, seed=0):
    dv = np.broadcast_to(syn.depth_hypotheses(D), (B, D)).copy()
    gt, mask = syn.depth_targets(dv, h, w, seed)
    cost = (np.random.default_rng(seed).standard_normal((B, D, h, w)) * 3.0).astype(np.float32)
    return [torch.from_numpy(a).to(dev) for a in (cost, gt, mask, dv)]


def unfused(cost, gt, mask, dv):
    c = cost.detach().requires_grad_(True)
    loss, wta = mvsnet_cls_loss(_SoftmaxDepth.apply(c), gt, mask, dv)
    loss.backward()
    return loss.detach(), wta, c.grad


def fused(cost, gt, mask, dv):
    c = cost.detach().requires_grad_(True)
    loss, wta = mvsnet_cls_loss_from_cost(c, gt, mask, dv)
    loss.backward()
    return loss.detach(), wta, c.grad


def rel_l2(a, ref):
    return float(np.linalg.norm(a.ravel() - ref.ravel()) / np.linalg.norm(ref.ravel()))


def check(dev):
    """Both paths against float64 on the CPU at 64x80, with the tests' bounds."""
    t = inputs(64, 80, dev, seed=1)
    c64 = t[0].cpu().double().requires_grad_(True)
    l64, w64 = mvsnet_cls_loss(torch.softmax(c64, 1), *(a.cpu().double() for a in t[1:]))
    l64.backward()
    l64, g64 = l64.item(), c64.grad.numpy()
    lu, wu, gu = unfused(*t)
    lf, wf, gf = fused(*t)
    eu, ef = abs(lu.item() - l64), abs(lf.item() - l64)
    ru, rf = rel_l2(gu.cpu().double().numpy(), g64), rel_l2(gf.cpu().double().numpy(), g64)
    assert ef <= max(2 * eu, 1e-6 * abs(l64)), (ef, eu, l64)
    assert rf <= max(2 * ru, 1e-6), (rf, ru)
    assert torch.equal(wf.cpu().double(), w64) and torch.equal(wu, wf)
    return dict(loss_err_fused=ef, loss_err_unfused=eu, grad_rel_l2_fused=rf, grad_rel_l2_unfused=ru)


def device_ms(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    out_dir = sys.argv[2] if len(sys.argv) > 2 else None
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    dev = torch.device("cuda", 0)
    agree = check(dev)
    t = inputs(H, W, dev)
    paths = {"unfused": lambda: unfused(*t), "fused": lambda: fused(*t)}
    lu, wu, _ = paths["unfused"]()     # warm-up of every shape, both paths
    lf, wf, _ = paths["fused"]()
    assert torch.equal(wu, wf) and abs(lu.item() - lf.item()) <= 1e-6 * abs(lu.item()), (lu, lf)
    for fn in paths.values():
        for _ in range(3):
            fn()
    ms = {k: [] for k in paths}
    for _ in range(ROUNDS):
        for k, fn in paths.items():
            ms[k].append(device_ms(fn, reps))
    peak = {k: peak_bytes(fn) for k, fn in paths.items()}

    ops.profile_reset()
    ops.profile_enable(True)
    for _ in range(reps):
        paths["fused"]()
    torch.cuda.synchronize()
    prof = ops.profile_read()
    ops.profile_enable(False)
    vol = 4.0 * B * D * H * W
    kern = {}
    for name, nbytes in (("cls_loss_fwd", vol), ("cls_loss_reduce", None), ("cls_loss_bwd", 2 * vol)):
        n, total = prof[name]
        row = dict(launches=n, ms_per_launch=round(total / n, 4))
        if nbytes:
            gbs = nbytes / (total / n / 1e3) / 1e9
            row.update(algorithmic_bytes=nbytes, gb_per_s=round(gbs, 1), hbm_frac=round(gbs / HBM_PEAK_GBS, 4))
        kern[name] = row
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = dict(workload=f"cost volume B={B} D={D} {H}x{W} (config 4's training step)", reps=reps,
               rounds=ROUNDS, volume_mb=round(vol / 2 ** 20, 1),
               unfused_ms=round(med["unfused"], 4), fused_ms=round(med["fused"], 4),
               unfused_ms_rounds=[round(v, 4) for v in ms["unfused"]],
               fused_ms_rounds=[round(v, 4) for v in ms["fused"]],
               speedup=round(med["unfused"] / med["fused"], 2),
               unfused_peak_mb=round(peak["unfused"] / 2 ** 20, 1), fused_peak_mb=round(peak["fused"] / 2 ** 20, 1),
               fused_kernels=kern, agreement_64x80=agree, hbm_peak_gbs=HBM_PEAK_GBS)
    line = json.dumps(res)
    print(line, flush=True)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "cls_loss_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
