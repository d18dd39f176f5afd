"""Depth-sweep throughput benchmark (BASELINE.json metric: depth-hypotheses/s).

One "step" = one full D-plane sweep (EMVSNet's eval depth loop, drmvsnet.py:306-342:
warp x (N-1), omega aggregation, ConvLSTM U-Net step, online WTA) over B reference
views per GPU, with the per-view features already resident in HBM (FeatNet is out of
scope).  ``value`` = ref-views x H x W x D x steps (all ranks) / max-over-ranks
wall time of the timed region.

Multi-GPU: one process per GPU (torchrun), reference views sharded across ranks, no
data-path collective; the only collectives are the timing barrier and the
max-over-ranks reduction of the elapsed time.

A plain run (``--gpus 1 --steps N --warmup W``) sets up, warms up, times the N steps, writes
the last step's outputs if ``--dump-outputs DIR`` is given, and prints the JSON line with the
headline figure alone.  Everything else is measured only with ``--full`` (each leg can still be
switched off with its ``--no-*`` option).

With ``--full``, also reported on the same JSON line:
  roofline      the dominant kernel's achieved algorithmic bytes (HBM-bound) or flops
                (MFMA-bound) per launch / its average launch time, from hipEvents
                recorded on the launch stream over the timed region;
  kernels       the same figures for every kernel of the sweep;
  cpu_baseline  the CPU oracle (oracle/sweep_oracle.py, a from-scratch fp32 restatement
                of the reference, pinned to fixtures made by running the reference) timed
                on this host's cores on a bounded sample (the first planes of the same
                workload), rank 0 at N=1 only;
  parity        HIP vs the oracle on that sample (cost max|err|, depth rel-L1);
  fusion        the depth-map fusion core (§8f-2) at the same resolution;
  e2e           the end-to-end models.EMVSNet eval forward on images (FeatNet in PyTorch
                + the sweep) at the same config, reported beside the headline (§8d).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "aa-rmvsnet_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from aarmvs import ops, synthetic as syn  # noqa: E402
from aarmvs.dist import env, init_process_group, local_device_index, max_over_ranks  # noqa: E402

HBM_PEAK_GBS = 8000.0     # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: f32 MFMA (= vector) dense peak
F16_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense f16/bf16 MFMA peak
# The ConvLSTM cells run each fp32 product as three f16 MFMA products (split-fp16,
# DESIGN.md §7): their fp32-equivalent ceiling is the f16 peak / 3.
CELL_PEAK_TFLOPS = F16_PEAK_TFLOPS / 3

# BASELINE.json configs (name -> views N, H, W, D)
CONFIGS = {
    "plumbing_160x128_n3_d48": dict(N=3, H=128, W=160, D=48),       # configs[0]
    "dtu_eval_800x600_n5_d256": dict(N=5, H=600, W=800, D=256),     # configs[1]
    "dtu_eval_1600x1184_n7_d512": dict(N=7, H=1184, W=1600, D=512),  # configs[2] (headline)
    "dtu_train_640x512_n3_d192": dict(N=3, H=512, W=640, D=192),    # configs[3] (sweep only)
    "tnt_1920x1056_n11_d898": dict(N=11, H=1056, W=1920, D=898),    # configs[4]
}
DEFAULT_CONFIG = "dtu_eval_1600x1184_n7_d512"

# ConvLSTM cells (drmvsnet.py:241-244): (input ch incl. hidden, 4*hid, resolution divisor)
CELL_GEOM = {0: (48, 64, 1), 1: (32, 64, 2), 2: (32, 64, 4), 3: (48, 64, 2), 4: (40, 32, 1)}


def algorithmic_work(name: str, B: int, N: int, H: int, W: int, launches_per_plane: int):
    """(kind, amount per launch) of a sweep kernel; kind 'bytes' (HBM) or 'flops' (MFMA).

    Per-unit figures:
      cost_x       128*(N+1) B per hypothesis: ref + N-1 source features read once,
                   the 32-ch cost slice written once (fp32);
      omega_conv   128*N + 16*(N-1) B per hypothesis: ref + N-1 source features read
                   once, the 4-ch omega conv output written once per source view;
      omega_stats  16*(N-1) B per hypothesis (the omega conv output, 4 ch per view);
      lstm_cell k  2*9*Cin*Cout FLOP per cell pixel;
      deconv       2*16*16*9 FLOP per deconv input pixel (each input pixel meets the 3x3 kernel once);
      head_wta     8*9*2 FLOP per pixel.
    """
    HW = H * W
    nsrc = N - 1
    if name == "cost_x":
        return "bytes", 128.0 * (N + 1) * B * HW / launches_per_plane
    if name == "omega_conv":
        return "bytes", (128.0 * N + 16.0 * nsrc) * B * HW / launches_per_plane
    if name in ("omega_stats1", "omega_stats2"):
        return "bytes", 16.0 * nsrc * B * HW / launches_per_plane
    if name.startswith("lstm_cell"):
        k = int(name[-1])
        cin, cout, sc = CELL_GEOM[k]
        return "flops", 2.0 * 9 * cin * cout * B * HW / (sc * sc) / launches_per_plane
    if name == "deconv0":
        return "flops", 2.0 * 16 * 16 * 9 * B * HW / 16 / launches_per_plane
    if name == "deconv1":
        return "flops", 2.0 * 16 * 16 * 9 * B * HW / 4 / launches_per_plane
    if name == "head_wta":
        return "flops", 2.0 * 8 * 9 * B * HW / launches_per_plane
    return "bytes", 0.0


def kernel_table(prof: dict, planes: int, B: int, N: int, H: int, W: int):
    rows = {}
    total = sum(ms for _, ms in prof.values()) or 1.0
    for name, (n, ms) in prof.items():
        # launches per plane: 1/G for the cost-slice kernels (one launch covers a group of G
        # planes), 1 for the regulariser's
        per_plane = n / planes
        kind, amount = algorithmic_work(name, B, N, H, W, per_plane)
        avg_s = ms / n / 1e3
        if kind == "bytes":
            ach = amount / avg_s / 1e9 if amount else 0.0
            rows[name] = dict(launches=n, avg_us=round(avg_s * 1e6, 2), share=round(ms / total, 4),
                              bound="hbm", achieved=round(ach, 1), unit="GB/s",
                              frac=round(ach / HBM_PEAK_GBS, 4), per_launch=amount)
        else:
            ach = amount / avg_s / 1e12
            peak = CELL_PEAK_TFLOPS if name.startswith("lstm_cell") else FP32_PEAK_TFLOPS
            rows[name] = dict(launches=n, avg_us=round(avg_s * 1e6, 2), share=round(ms / total, 4),
                              bound="mfma", achieved=round(ach, 2), unit="TFLOP/s",
                              peak=round(peak, 1), frac=round(ach / peak, 4), per_launch=amount)
    return rows


def load_traffic(workload: str, kernel: str):
    """(HBM bytes per launch of `kernel`, the PMC run they come from) from the committed
    rocprofv3 --pmc summary (tools/pmc_summarize.py), or (None, None).  Not measured in this
    run: PMC passes need their own rocprofv3 runs (MI355X_MICROARCH.md §HBM)."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        with open(path) as f:
            tab = json.load(f)
        v = tab.get(workload, {}).get(kernel)
        return v, (f"profiles/pmc_traffic.json: {tab.get('_source', 'unlabelled PMC run')}"
                   if v is not None else None)
    except (OSError, ValueError):
        return None, None


def make_inputs(cfg, B, seed, device):
    N, H, W, D = cfg["N"], cfg["H"], cfg["W"], cfg["D"]
    sc = syn.scene(B, N, H, W, D, seed=seed)
    feats = torch.from_numpy(sc["features"])           # [N,B,32,H,W]
    proj = torch.from_numpy(sc["proj_matrices"])       # [B,N,4,4]
    dv = torch.from_numpy(sc["depth_values"])          # [B,D]
    return feats, proj, dv, feats.to(device)


def cpu_model() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def real_weights():
    """The reference's model_dtu_v2 omega/regulariser tensors, as committed in
    tests/golden/real_weights_sweep.npz (read from the checkpoint with weights_only=True by
    tests/golden/make_golden.py)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "real_weights_sweep.npz"), allow_pickle=False)
    return {k[2:]: g[k] for k in g.files if k.startswith("w:")}


def cpu_baseline(feats, proj, dv, P, planes: int):
    """SURVEY §8d's CPU baseline: the CPU restatement (oracle/sweep_oracle.py with its
    F.grid_sample warp, the reference's own ATen kernels; measured beside the imported
    reference in profiles/r02_cpu_restatement_vs_reference.json) on this host's cores, one
    warm-up plane then `planes` timed planes of the same inputs.  Returns the oracle's
    output over planes 0..planes (the parity leg) and the baseline record."""
    from oracle import sweep_oracle as orc
    threads = int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))
    threads = max(1, min(threads, os.cpu_count() or 1))
    torch.set_num_threads(threads)
    N = feats.shape[0]
    B, _, H, W = feats.shape[1:]
    times = []
    ref = orc.sweep(feats[0], list(feats[1:]), proj[:, 0], list(proj[:, 1:].unbind(1)),
                    dv[:, :planes + 1], P, want_volume=True, fast=True, plane_times=times)
    dt = sum(times[1:])   # plane 0 is the warm-up
    hyp = B * H * W * planes
    return ref, dict(value=hyp / dt, unit="depth-hypotheses/s", cores=torch.get_num_threads(),
                     kind="port", cpu=cpu_model(), s_per_plane=round(dt / planes, 3),
                     sample=f"oracle/sweep_oracle.py (fast: F.grid_sample warp), 1 warm-up plane + "
                            f"{planes} timed planes of D, B={B}, N={N}, {W}x{H}, model_dtu_v2 weights, "
                            f"{dt:.1f} s timed, torch CPU threads={torch.get_num_threads()}, "
                            f"CPU: {cpu_model()}")


def fusion_bench(H: int, W: int, nsrc: int, dev, cpu_leg: bool, reps: int = 10):
    """The depth-map fusion core (aarmvs.fusion.filter_depth_core, fusion.py:174-220) on one
    reference view with nsrc source views at the sweep's resolution: GPU time per view with
    hipEvents, HBM roofline on its algorithmic bytes ((19 + 4 nsrc) B per reference pixel:
    depth + confidence + one depth read per source view + three masks + the float64
    average), and the CPU oracle on a 2-source-view sample of the same maps."""
    from aarmvs import fusion
    depths, cams, conf = syn.fusion_views(H, W, nsrc, seed=7)
    t = [torch.from_numpy(d).to(dev) for d in depths]
    c = torch.from_numpy(conf).to(dev)
    run = lambda: fusion.filter_depth_core(t[0], c, cams[0], t[1:], cams[1:], 0.35)  # noqa: E731
    run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    px = H * W
    bytes_ = (19.0 + 4.0 * nsrc) * px
    ach = bytes_ / (ms / 1e3) / 1e9
    res = dict(metric="fusion ref-view pixels/s (nsrc source views each)", value=round(px / (ms / 1e3), 1),
               ms_per_view=round(ms, 4), H=H, W=W, nsrc=nsrc, achieved_gbs=round(ach, 1),
               peak_gbs=HBM_PEAK_GBS, frac=round(ach / HBM_PEAK_GBS, 4),
               geo_mask_mean=round(float(out[1].float().mean()), 4))
    if cpu_leg:
        from oracle import fusion_oracle as fo
        k = 2
        t0 = time.perf_counter()
        fo.filter_depth_core(depths[0], conf, cams[0], depths[1:1 + k], cams[1:1 + k], 0.35)
        dt = time.perf_counter() - t0
        res["cpu_baseline"] = dict(value=round(px * k / nsrc / dt, 1), unit="ref-view pixels/s",
                                   cores=1, kind="port",
                                   sample=f"oracle/fusion_oracle.py filter_depth_core, {k} of {nsrc} "
                                          f"source views ({dt:.1f} s), scaled to {nsrc}")
    return res


def e2e_bench(N: int, H: int, W: int, D: int, B: int, dev, reps: int = 2):
    """End-to-end figure (reported beside the headline): the drop-in
    `models.EMVSNet` eval forward (drmvsnet.py:255-345) on images, FeatNet (PyTorch on the
    GPU) for all N views plus the HIP sweep, random-init weights; FeatNet alone is timed
    too.  Wall time with the device synchronised, `reps` forwards after one warm-up."""
    from models.drmvsnet import EMVSNet
    torch.manual_seed(0)
    model = EMVSNet(D, image_scale=1.0, max_h=H, max_w=W, return_depth=True).to(dev).eval()
    g = torch.Generator(device="cpu").manual_seed(0)
    imgs = torch.randn(B, N, 3, H, W, generator=g).to(dev)
    sc = syn.scene(B, N, H, W, D, seed=0)
    proj = torch.from_numpy(sc["proj_matrices"]).to(dev)
    dv = torch.from_numpy(sc["depth_values"]).to(dev)
    with torch.no_grad():
        out = model(imgs, proj, dv)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = model(imgs, proj, dv)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        views = torch.unbind(imgs, 1)
        t0 = time.perf_counter()
        for _ in range(reps):
            feats = [model.feature(v) for v in views]
        torch.cuda.synchronize()
        ft = (time.perf_counter() - t0) / reps
    ok = bool(torch.isfinite(out["depth"]).all())
    del feats, out, model
    return dict(metric="end-to-end depth-hypotheses/s (EMVSNet.forward: FeatNet + sweep)",
                value=round(B * H * W * D / dt, 1), s_per_step=round(dt, 4),
                featnet_s=round(ft, 4), featnet="PyTorch (MIOpen) fp32 convs + the HIP deformable-conv sampling (aarmvs_deform_sample); outside the §8 scope",
                images=f"[{B},{N},3,{H},{W}] ~N(0,1)", depth_finite=ok)


def backward_work(name: str, B: int, N: int, H: int, W: int, D: int, launches: int):
    """(kind, amount per launch, peak) of a training-backward kernel (bptt.hip, warp_cost.hip
    cbw_*), per DESIGN.md §6's per-unit figures, for `launches` launches over D planes:
      gate_bwd k   52 hid B per cell pixel and plane (z, gz: 4 hid floats each; c, c', dL/dh,
                   dL/dc read and dL/dc written: hid floats each);
      dgrad k      2*9*Cin*4hid FLOP per cell pixel and plane (the forward conv transposed;
                   three split-fp16 products: the cells' ceiling, f16 peak / 3);
      wgrad k      the same FLOP (four split products: f16 peak / 4);
      gnb_partial  128 B per deconv output pixel and plane (dL/dr and u, 16 ch each), both deconvs;
      deconv_bwd   2*16*16*9 FLOP per deconv input pixel and plane (VALU fp32), both deconvs;
      cbw_feat     per hypothesis: the reference and source features (128 (N) B), dL/dx (128 B),
                   dL/dt1 and the omega weight per view (20 (N-1) B);
      cbw_chain    per hypothesis and view: the omega conv output t1 (16 B) per stage (4), the
                   stage-1 warp and dL/dx (3 x 128 B), dL/do / w / dL/dt1 out (24 B);
      deconv_wgrad 2*16*16*9 FLOP per deconv input pixel and plane (fp32 MFMA), both deconvs;
      head_wgrad   the head's h4 (8 ch) and dL/dcost per pixel and plane: 36 B."""
    HW = H * W
    nsrc = N - 1
    cell = {0: (48, 16, 1), 1: (32, 16, 2), 2: (32, 16, 4), 3: (48, 16, 2), 4: (40, 8, 1)}
    if name[:-1] in ("gate_bwd", "dgrad", "wgrad") and name[-1].isdigit():
        cin, hid, sc = cell[int(name[-1])]
        px = B * HW / (sc * sc) * D
        if name.startswith("gate_bwd"):
            return "bytes", 52.0 * hid * px / launches, HBM_PEAK_GBS
        peak = CELL_PEAK_TFLOPS if name.startswith("dgrad") else F16_PEAK_TFLOPS / 4
        return "flops", 2.0 * 9 * cin * 4 * hid * px / launches, peak
    if name == "gnb_partial":
        return "bytes", 128.0 * B * (HW + HW / 4) * D / launches, HBM_PEAK_GBS
    if name == "deconv_bwd":
        return "flops", 2.0 * 16 * 16 * 9 * B * (HW / 4 + HW / 16) * D / launches, FP32_PEAK_TFLOPS
    if name == "cbw_feat":
        return "bytes", (128.0 * N + 128.0 + 20.0 * nsrc) * B * HW * D / launches, HBM_PEAK_GBS
    if name == "deconv_wgrad":
        return "flops", 2.0 * 16 * 16 * 9 * B * (HW / 4 + HW / 16) * D / launches, FP32_PEAK_TFLOPS
    if name == "head_wgrad":
        return "bytes", 36.0 * B * HW * D / launches, HBM_PEAK_GBS
    if name == "cbw_chain":
        return "bytes", (16.0 * 4 + 3 * 128.0 + 24.0) * nsrc * B * HW * D / launches, HBM_PEAK_GBS
    return None, 0.0, None


def train_kernel_table(prof: dict, B: int, N: int, H: int, W: int, D: int):
    """Per-kernel rows of one profiled training step: the forward sweep's kernels as in the
    headline table (kernel_table), the backward's with backward_work's algorithmic work."""
    fwd = {k: v for k, v in prof.items() if backward_work(k, B, N, H, W, D, 1)[0] is None
           and k not in ("bwd_small", "cbw_small")}
    rows = kernel_table(fwd, D, B, N, H, W)
    total = sum(ms for _, ms in prof.values()) or 1.0
    for name, (n, ms) in prof.items():
        kind, amount, peak = backward_work(name, B, N, H, W, D, n)
        avg_s = ms / n / 1e3
        row = dict(launches=n, avg_us=round(avg_s * 1e6, 2), share=round(ms / total, 4))
        if kind == "bytes":
            ach = amount / avg_s / 1e9
            row.update(bound="hbm", achieved=round(ach, 1), unit="GB/s", peak=peak, frac=round(ach / peak, 4))
        elif kind == "flops":
            ach = amount / avg_s / 1e12
            row.update(bound="mfma" if name[:-1] in ("dgrad", "wgrad") or name == "deconv_wgrad" else "valu",
                       achieved=round(ach, 2),
                       unit="TFLOP/s", peak=round(peak, 1), frac=round(ach / peak, 4))
        elif name in ("bwd_small", "cbw_small"):
            row.update(bound=None, note="fixed-order reductions / small per-group kernels")
        else:
            continue
        rows[name] = row
    for r in rows.values():
        r.pop("per_launch", None)
    return rows


def ceiling_limits():
    """What binds the cost-slice kernels besides HBM, from the committed rocprofv3 counter passes
    (tools/gpu_ceiling.sh -> tools/ceiling_summary.py, one 16-plane group at the headline): the
    fraction of wave cycles issuing / dependency-stalled / parked for omega_conv (issue- and
    latency-bound) and the texture-unit (TA, TD) busy fractions and L1 hit rate for cost_x
    (bound by its gathers through the vector L1)."""
    here = os.path.dirname(os.path.abspath(__file__))
    for name in ("r06_ceiling_pmc.json", "r05_ceiling_pmc.json", "r04_ceiling_pmc.json", "r03_ceiling_pmc.json"):
        path = os.path.join(here, "profiles", name)
        if not os.path.exists(path):
            continue
        with open(path) as fh:
            d = json.load(fh)
        if not (d.get("omega_conv") or d.get("cost_x")):
            continue
        out = {"source": "profiles/" + name}
        om, cx = d.get("omega_conv") or {}, d.get("cost_x") or {}

        def valu_pipe(k):
            # share of the launch's GPU-active cycles a SIMD's VALU is busy: 4 cycles per wave64
            # VALU instruction, the waves spread over 256 CUs x 4 SIMDs (MI355X)
            if not (k.get("per_wave_valu") and k.get("waves") and k.get("gui_active_cycles")):
                return None
            return round(k["per_wave_valu"] * 4.0 * k["waves"] / 1024.0 / k["gui_active_cycles"], 4)

        if om:
            out["omega_conv"] = {k: om[k] for k in ("issue_frac", "dep_stall_frac", "parked_frac", "per_wave_valu")
                                 if k in om}
            out["omega_conv"]["valu_pipe_frac"] = valu_pipe(om)
            out["omega_conv"]["bound"] = "VALU issue" if (valu_pipe(om) or 0) > 0.75 else "issue/latency"
        if cx:
            l1 = 1.0 - cx["tcp_to_l2_read_req"] / cx["tcp_accesses"] if cx.get("tcp_accesses") else None
            out["cost_x"] = {k: cx[k] for k in ("ta_busy_frac", "td_busy_frac", "issue_frac", "parked_frac")
                             if k in cx}
            out["cost_x"]["l1_hit_frac"] = round(l1, 4) if l1 is not None else None
            out["cost_x"]["valu_pipe_frac"] = valu_pipe(cx)
            out["cost_x"]["bound"] = "L1 gather (TD)"
        return out
    return None


def train_bench(dev, D: int = 192, reps: int = 2):
    """Training-step time at config 4 as stated (BASELINE configs[3]: 640x512, N=3, D=192, one
    sample per GPU; train.py:288-307): the drop-in EMVSNet train forward (FeatNet + the HIP
    sweep), softmax, mvsnet_cls_loss and the backward through the whole 192-plane recurrence,
    random-init weights, synthetic images.  Wall time with the device synchronised, `reps`
    steps after one warm-up step; peak device memory of the step."""
    from models.drmvsnet import EMVSNet, mvsnet_cls_loss
    B, N, H, W = 1, 3, 512, 640
    g = torch.Generator(device="cpu").manual_seed(0)
    imgs = torch.randn(B, N, 3, H, W, generator=g).to(dev)
    sc = syn.scene(B, N, H, W, D, seed=0)
    proj = torch.from_numpy(sc["proj_matrices"]).to(dev)
    torch.manual_seed(0)
    model = EMVSNet(D, image_scale=1.0, max_h=H, max_w=W, evidential=False).to(dev).train()
    dv = torch.from_numpy(sc["depth_values"]).to(dev)
    depth_gt = dv[:, D // 2].reshape(B, 1, 1).expand(B, H, W).contiguous()
    mask = torch.ones(B, H, W, device=dev)

    def step():
        model.zero_grad(set_to_none=True)
        prob, _, _ = model(imgs, proj, dv)
        loss = mvsnet_cls_loss(prob, depth_gt, mask, dv)[0]
        loss.backward()
        return loss

    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    peak = torch.cuda.max_memory_allocated(dev)
    # the same steps with the backward on one stream (AARMVS_BWD_PIPE=0; the default schedule 1
    # overlaps the plane pipeline and the group stage, bit-identical to it)
    prev = os.environ.get("AARMVS_BWD_PIPE")
    os.environ["AARMVS_BWD_PIPE"] = "0"
    step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        step()
    torch.cuda.synchronize()
    dt_ov = (time.perf_counter() - t0) / reps
    if prev is None:
        del os.environ["AARMVS_BWD_PIPE"]
    else:
        os.environ["AARMVS_BWD_PIPE"] = prev
    ok = bool(torch.isfinite(loss)) and all(
        p.grad is None or bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    # one more step with a hipEvent pair around every library launch (the forward's and the
    # backward's two-stream schedules serialised onto one stream): per-kernel rooflines
    sw = model._sweep(dev)
    sw.overlap = False
    ops.profile_enable(True)
    ops.profile_reset()
    step()
    torch.cuda.synchronize()
    prof = ops.profile_read()
    ops.profile_enable(False)
    sw.overlap = True
    kern = train_kernel_table(prof, B, N, H, W, D)
    lib_ms = sum(ms for _, ms in prof.values())
    del model
    return dict(metric="training step (forward + mvsnet_cls_loss + backward), 1 sample / GPU",
                config="dtu_train_640x512_n3_d192", D=D, s_per_step=round(dt, 4),
                ms_per_plane=round(dt / D * 1e3, 3), steps_timed=reps,
                backward_schedule="plane pipeline + group-stage overlap on three streams (AARMVS_BWD_PIPE=1, "
                                  "default; bit-identical to one stream)",
                s_per_step_one_stream=round(dt_ov, 4), ms_per_plane_one_stream=round(dt_ov / D * 1e3, 3),
                peak_device_gb=round(peak / 1e9, 2),
                backward=getattr(EMVSNet, "BACKWARD_PATH", "see DESIGN.md §6"),
                loss_and_grads_finite=ok,
                kernels_timing="separate profiled step, one stream, hipEvents per launch",
                library_ms_per_step=round(lib_ms, 2), kernels=kern)


def train_cpu_baseline(planes: int = 6):
    """CPU leg of the training mode: float32 autograd of the oracle (the reference's own ATen
    arithmetic) through `planes` planes of config 4's 640x512, N=3 sweep plus the softmax loss,
    on this host's cores; scaled to one D=192 sample (the sweep's cost is uniform per plane)."""
    from oracle import sweep_oracle as orc
    threads = int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))
    torch.set_num_threads(max(1, min(threads, os.cpu_count() or 1)))
    B, N, H, W, D = 1, 3, 512, 640, 192
    sc = syn.scene(B, N, H, W, D, seed=0)
    feats = torch.from_numpy(sc["features"]).requires_grad_(True)
    proj = torch.from_numpy(sc["proj_matrices"])
    dv = torch.from_numpy(sc["depth_values"][:, :planes].copy())
    P = {k: torch.from_numpy(v).requires_grad_(True) for k, v in syn.sweep_weights(1).items()}
    rels = [orc.relative_projection(proj[:, v], proj[:, 0]) for v in range(1, N)]
    t0 = time.perf_counter()
    state = orc.init_state(B, H, W)
    costs = []
    for d in range(planes):
        x = orc.cost_slice(feats[0], [feats[v] for v in range(1, N)], rels, dv[:, d], P, fast=True)
        cost, state = orc.unet_step(x, state, P)
        costs.append(cost)
    prob = torch.softmax(torch.stack(costs, 1).squeeze(2), dim=1)
    (-(prob.clamp_min(1e-12).log()[:, 0]).mean()).backward()
    dt = time.perf_counter() - t0
    s_per_sample = dt / planes * D
    return dict(value=round(1.0 / s_per_sample, 6), unit="training samples/s", cores=torch.get_num_threads(),
                kind="port", cpu=cpu_model(), s_per_plane=round(dt / planes, 3),
                sample=f"oracle/sweep_oracle.py float32 autograd, forward + backward of {planes} planes of "
                       f"640x512, N=3 (no FeatNet), {dt:.1f} s, scaled x{D // planes} to one D={D} sample; "
                       f"torch CPU threads={torch.get_num_threads()}, CPU: {cpu_model()}")


def train_main(args, rank: int, world: int, dev) -> None:
    """``--train``: BASELINE configs[3] as a data-parallel training step (train.py:172 wraps the
    model for all GPUs, train.py:288-307 is the step): one 640x512, N=3, D=192 sample per rank
    through the drop-in models.EMVSNet (FeatNet in PyTorch, the HIP sweep and its HIP backward),
    mvsnet_cls_loss, DDP's gradient all-reduce over RCCL (gloo in a shared-GPU rehearsal) and
    Adam.  value = samples of all ranks / max-over-ranks wall time of the K timed steps; the
    all-reduce is timed on its own (the DDP bucket's size, 20 repetitions) to give its share."""
    from models.drmvsnet import EMVSNet, mvsnet_cls_loss
    B, N, H, W, D = 1, 3, 512, 640, args.train_planes
    g = torch.Generator(device="cpu").manual_seed(rank)
    imgs = torch.randn(B, N, 3, H, W, generator=g).to(dev)
    sc = syn.scene(B, N, H, W, D, seed=rank)
    proj = torch.from_numpy(sc["proj_matrices"]).to(dev)
    dv = torch.from_numpy(sc["depth_values"]).to(dev)
    depth_gt = dv[:, D // 2].reshape(B, 1, 1).expand(B, H, W).contiguous()
    mask = torch.ones(B, H, W, device=dev)
    torch.manual_seed(0)   # one initial model on every rank (DDP also broadcasts rank 0's)
    core = EMVSNet(D, image_scale=1.0, max_h=H, max_w=W, evidential=False).to(dev).train()
    model = core
    if world > 1:
        nccl = torch.distributed.get_backend() == "nccl"
        model = torch.nn.parallel.DistributedDataParallel(core, device_ids=[dev.index] if nccl else None)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)

    def step():
        opt.zero_grad(set_to_none=True)
        prob, _, _ = model(imgs, proj, dv)
        loss = mvsnet_cls_loss(prob, depth_gt, mask, dv)[0]
        loss.backward()
        opt.step()
        return loss

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    barrier()
    elapsed = max_over_ranks(time.perf_counter() - t0, dev)
    if args.dump_outputs:   # the step's loss and the gradients it left (a seeded sample if large)
        grads = torch.cat([p.grad.reshape(-1) for p in core.parameters() if p.grad is not None])
        dump_outputs(args.dump_outputs, {"loss": loss.reshape(1), "grads": grads}, rank, world)
    ok = bool(torch.isfinite(loss)) and all(p.grad is None or bool(torch.isfinite(p.grad).all())
                                            for p in core.parameters())
    nparam = sum(p.numel() for p in core.parameters() if p.requires_grad)
    ar_ms = 0.0
    if world > 1:   # the gradient all-reduce alone: one flat bucket of every trained parameter
        flat = torch.zeros(nparam, device=dev if torch.distributed.get_backend() == "nccl" else "cpu")
        for _ in range(3):
            torch.distributed.all_reduce(flat)
        barrier()
        t1 = time.perf_counter()
        for _ in range(20):
            torch.distributed.all_reduce(flat)
        barrier()
        ar_ms = max_over_ranks((time.perf_counter() - t1) / 20 * 1e3, dev)
    cpu = train_cpu_baseline() if (rank == 0 and world == 1 and not args.no_cpu) else None
    # the training backward's dominant kernel over one profiled step (one stream, hipEvents)
    roofline, kern = None, None
    if rank == 0 and not args.no_kernel_timing:
        sw = core._sweep(dev)
        sw.overlap = False
        ops.profile_enable(True)
        ops.profile_reset()
        step()
        torch.cuda.synchronize()
        prof = ops.profile_read()
        ops.profile_enable(False)
        sw.overlap = True
        kern = train_kernel_table(prof, B, N, H, W, D)
        cand = {k: v for k, v in kern.items() if v.get("bound") in ("hbm", "mfma", "valu")}
        if cand:
            dom = max(cand, key=lambda k: cand[k]["share"])
            r = cand[dom]
            roofline = dict(kernel=dom, bound=r["bound"], achieved=r["achieved"],
                            peak=r.get("peak", HBM_PEAK_GBS), unit=r["unit"], frac=r["frac"], traffic=None,
                            avg_us=r["avg_us"], timing="separate profiled step, one stream, hipEvents per launch")
    if rank == 0:
        ms = elapsed / args.steps * 1e3
        line = {
            "metric": "training samples/sec (config 4 DDP step: EMVSNet forward + mvsnet_cls_loss + backward "
                      "+ gradient all-reduce + Adam)",
            "value": round(world * args.steps / elapsed, 4),
            "unit": "samples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "fp32-class split-fp16 (3 products; weight gradients 4) on the sweep, fp32 elsewhere",
            "data": "synthetic images ~N(0,1), SURVEY 8d cameras, random-init weights",
            "config": {"workload": "dtu_train_640x512_n3_d192", "views": N, "H": H, "W": W, "D": D,
                       "global_batch": B * world, "parallelism": f"ddp x{world}"},
            "hyp_per_s": round(world * args.steps * B * H * W * D / elapsed, 1),
            "allreduce": dict(params=nparam, bytes=nparam * 4, ms=round(ar_ms, 4),
                              share_of_step=round(ar_ms / ms, 5) if world > 1 else 0.0,
                              backend=torch.distributed.get_backend() if world > 1 else None,
                              note="timed alone; DDP overlaps it with the backward"),
            "loss_and_grads_finite": ok,
            "roofline": roofline,
            "cpu_baseline": cpu,
            "train_kernels": kern,
        }
        print(json.dumps(line), flush=True)


DUMP_LIMIT_BYTES = 64 << 20   # --dump-outputs: at most this much in all
DUMP_SAMPLE_SEED = 20240607


def dump_outputs(directory: str, arrays: dict, rank: int, world: int) -> None:
    """``--dump-outputs``: write the last timed step's outputs as ``DIR/<name>.npy`` (float32;
    ``<name>_rank<r>`` when several ranks run).  An array that would take the total past
    DUMP_LIMIT_BYTES is stored as a fixed, seeded sample of its elements (the same indices in
    every run, so that two builds compare element for element)."""
    os.makedirs(directory, exist_ok=True)
    budget = DUMP_LIMIT_BYTES // max(1, world)
    share = budget // max(1, len(arrays)) - 4096   # room for the .npy header
    for name, t in arrays.items():
        flat = t.detach().reshape(-1)
        if flat.numel() * 4 > share:
            n = share // 4
            idx = np.random.default_rng(DUMP_SAMPLE_SEED).choice(flat.numel(), size=n, replace=False)
            idx.sort()
            a = flat[torch.from_numpy(idx).to(flat.device)].float().cpu().numpy()
        else:
            a = t.detach().float().cpu().numpy()
        suffix = f"_rank{rank}" if world > 1 else ""
        np.save(os.path.join(directory, f"{name}{suffix}.npy"), np.ascontiguousarray(a, dtype=np.float32))


def spawn_ranks(n: int) -> int:
    """``--gpus N`` without a launcher: start N rank processes (one per GPU, the torchrun
    environment set by hand) from this parent, which never initialises the GPU
    (torch.cuda.device_count() does not, on this image), and exit with the worst code."""
    import signal
    import socket
    import subprocess
    visible = torch.cuda.device_count()
    if n > visible and not os.environ.get("AARMVS_SHARED_GPU") == "1":
        print(f"bench.py: --gpus {n} but only {visible} GPU(s) are visible", file=sys.stderr)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n),
                   LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:],
                                      env=env))
    rc = 0
    live = list(procs)
    while live:   # a failed rank would leave the others waiting at a barrier: stop them
        time.sleep(0.5)
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            if code != 0:
                rc = rc or (code if code > 0 else 128 - code)
                for q in live:
                    q.send_signal(signal.SIGTERM)
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", default=DEFAULT_CONFIG, choices=sorted(CONFIGS))
    ap.add_argument("--batch", type=int, default=1, help="reference views per GPU per step")
    ap.add_argument("--cpu-planes", type=int, default=8,
                    help="CPU baseline: timed planes after one warm-up plane (SURVEY 8d: 8)")
    ap.add_argument("--random-weights", action="store_true",
                    help="random-init sweep weights instead of the reference's model_dtu_v2")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-kernel-timing", action="store_true")
    ap.add_argument("--no-overlap", action="store_true",
                    help="run the omega pipeline on the main stream (no second stream)")
    ap.add_argument("--high-priority", action="store_true",
                    help="run the sweep's main stream at high priority (aux stream normal)")
    ap.add_argument("--no-fusion", action="store_true",
                    help="skip the depth-map fusion measurement (the next §8 row)")
    ap.add_argument("--no-train", action="store_true",
                    help="skip the config-4 training step (train_bench, D=192)")
    ap.add_argument("--train-planes", type=int, default=192,
                    help="depth planes of the training step (BASELINE configs[3]: 192)")
    ap.add_argument("--no-e2e", action="store_true",
                    help="skip the end-to-end EMVSNet.forward figure (FeatNet + sweep)")
    ap.add_argument("--train", action="store_true",
                    help="measure config 4's DDP training step (one sample per rank) instead of the "
                         "inference sweep; --train-planes sets D")
    ap.add_argument("--planes", type=int, default=0,
                    help="profiling aid: sweep only the first P depth planes (0 = all D); "
                         "per-launch figures are unchanged, the headline value is not comparable")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline figure: per-kernel timing and "
                         "roofline, CPU baseline and parity, fusion, end-to-end forward, training step "
                         "(each leg can be left out with its --no-* option)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned as "
                         "DIR/<name>.npy (float32, at most 64 MB in all)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:   # a plain run measures the headline figure only
        args.no_cpu = args.no_kernel_timing = args.no_fusion = args.no_e2e = args.no_train = True

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args.gpus))
    rank, local, world = env()
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world} ranks were launched",
              file=sys.stderr)
        sys.exit(2)
    dev = torch.device("cuda", local_device_index(local))
    torch.cuda.set_device(dev)
    init_process_group(dev)
    if args.train:
        train_main(args, rank, world, dev)
        if world > 1:
            torch.distributed.destroy_process_group()
        return

    cfg = dict(CONFIGS[args.config])
    if args.planes:
        cfg["D"] = min(cfg["D"], args.planes)
    N, H, W, D, B = cfg["N"], cfg["H"], cfg["W"], cfg["D"], args.batch
    wts = syn.sweep_weights(1) if args.random_weights else real_weights()
    P = {k: torch.from_numpy(v) for k, v in wts.items()}
    feats_h, proj, dv, feats = make_inputs(cfg, B, seed=rank, device=dev)
    sweep = ops.DepthSweep({k: v.to(dev) for k, v in P.items()}, dev, overlap=not args.no_overlap)
    if args.high_priority:
        torch.cuda.set_stream(torch.cuda.Stream(device=dev, priority=-1))
    ref, srcs = feats[0], list(feats[1:])
    src_proj = list(proj[:, 1:].unbind(1))

    def step():
        return sweep(ref, srcs, proj[:, 0], src_proj, dv, want_depth=True)

    timing = not args.no_kernel_timing
    ops.profile_enable(False)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    # headline region: no per-launch events (they serialise the two streams' launches)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    barrier()
    elapsed = time.perf_counter() - t0
    elapsed = max_over_ranks(elapsed, dev)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"depth": out["depth"], "conf": out["conf"]}, rank, world)

    # separate kernel-timing pass over the same workload: one step with a hipEvent pair
    # around every launch and the two streams serialised (one stream), so each average is
    # the kernel's isolated duration -> per-kernel figures for `roofline`.  Concurrent
    # kernels would share the CUs and stretch each other's event spans.
    prof, prof_steps = {}, 0
    if timing:
        sweep.overlap = False
        ops.profile_enable(True)
        ops.profile_reset()
        prof_steps = 1
        barrier()
        for _ in range(prof_steps):
            step()
        barrier()
        prof = ops.profile_read()
        ops.profile_enable(False)

    hyp = world * B * H * W * D * args.steps
    value = hyp / elapsed
    kernels = kernel_table(prof, D * prof_steps, B, N, H, W) if prof else {}
    roofline = None
    if kernels:
        dom = max(kernels, key=lambda k: kernels[k]["share"])
        r = kernels[dom]
        traffic, traffic_src = load_traffic(args.config, dom)
        roofline = dict(kernel=dom, bound=r["bound"], achieved=r["achieved"],
                        peak=HBM_PEAK_GBS if r["bound"] == "hbm" else r["peak"],
                        unit=r["unit"], frac=r["frac"], traffic=traffic,
                        traffic_source=traffic_src,
                        per_launch=r["per_launch"], avg_us=r["avg_us"],
                        timing=f"separate pass, {prof_steps} step(s), one stream, hipEvents per launch")
        # the warp + aggregation path as a whole (every launch that produces the cost
        # slice): 128*(N+1) algorithmic B/hyp over the summed device time of its kernels
        group = [k for k in ("cost_x", "omega_conv", "omega_stats1", "omega_stats2", "omega_stat_reduce")
                 if k in prof]
        if group:
            ms = sum(prof[k][1] for k in group)
            planes = D * prof_steps
            ach = 128.0 * (N + 1) * B * H * W * planes / (ms / 1e3) / 1e9
            roofline["warp_aggregation"] = dict(kernels=group, achieved=round(ach, 1), unit="GB/s",
                                                peak=HBM_PEAK_GBS, frac=round(ach / HBM_PEAK_GBS, 4),
                                                us_per_plane=round(ms / planes * 1e3, 2))
        lim = ceiling_limits()
        if lim:
            roofline["limits"] = lim
            # what binds the dominant kernel by its counters (the HBM ratio stays in frac):
            # omega_conv the VALU pipe (87% busy), cost_x the vector-L1 gather path
            if dom in lim and lim[dom].get("bound"):
                roofline["roofline_model"] = r["bound"]
                roofline["bound"] = lim[dom]["bound"]

    cpu = None
    parity = None
    if rank == 0 and world == 1 and not args.no_cpu:
        planes = max(1, min(args.cpu_planes, D - 1))
        orc_out, cpu = cpu_baseline(feats_h, proj, dv, P, planes)
        g = sweep(ref, srcs, proj[:, 0], src_proj, dv[:, :planes + 1].contiguous(), want_depth=True,
                  want_cost=True)
        torch.cuda.synchronize()
        cost_err = float((g["cost"].cpu() - orc_out["cost"]).abs().max())
        dref = orc_out["depth"]
        rl1 = float((g["depth"].cpu() - dref).abs().sum() / dref.abs().sum())
        parity = dict(sample_planes=planes + 1, cost_max_abs_err=cost_err, depth_rel_l1=rl1)
        cpu["value"] = round(cpu["value"], 1)

    fusion_res = None
    if rank == 0 and world == 1 and not args.no_fusion:
        fusion_res = fusion_bench(H, W, 10, dev, cpu_leg=not args.no_cpu)

    e2e = None
    if rank == 0 and world == 1 and not args.no_e2e:
        e2e = e2e_bench(N, H, W, D, B, dev)

    train = None
    if rank == 0 and world == 1 and not args.no_train:
        train = train_bench(dev, D=args.train_planes)

    if rank == 0:
        line = {
            "metric": "depth-hypotheses/sec (ref-views x H x W x D / s)",
            "value": round(value, 1),
            "unit": "depth-hypotheses/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "full": args.full,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "fp32-class split-fp16 (3 products: cells, deconvs, omega conv on f16 MFMA, lo*lo "
                     "dropped, fp32 accumulate; fp32 elsewhere)",
            "data": "synthetic (seeded numpy features ~N(0,1), SURVEY 8d cameras, "
                    + ("random-init weights)" if args.random_weights else "model_dtu_v2 weights)"),
            "config": {"workload": args.config, "ref_views_per_gpu": B, "views": N, "H": H, "W": W,
                       "D": D, "global_batch": B * world, "parallelism": f"ref-view shard x{world}"},
            "roofline": roofline,
            "warp_aggregation": (roofline or {}).get("warp_aggregation"),
            "cpu_baseline": cpu,
            "parity": parity,
            "fusion": fusion_res,
            "e2e": e2e,
            "train": train,
            "kernels": {k: {kk: vv for kk, vv in v.items() if kk != "per_launch"}
                        for k, v in kernels.items()},
        }
        print(json.dumps(line), flush=True)
    del out
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
