"""Multi-GPU training driver: the reference's train.py loop (train.py:147-262) as one
process per GPU with DistributedDataParallel.

Each rank takes its shard of the training set (DistributedSampler, one or more samples per
GPU), runs the drop-in ``EMVSNet`` train forward (FeatNet + the HIP sweep), the loss, and the
backward; DDP's gradient all-reduce (``nccl`` = RCCL over xGMI; ``gloo`` in the shared-GPU
rehearsal, ``aarmvs.dist.shared_gpu``) is the only exchange.  As in train.py: Adam at
``--lr``, CosineAnnealingLR(T_max=epochs, eta_min=2e-6) stepped per epoch, checkpoints
``{'epoch', 'model', 'optimizer'}`` as ``logdir/model_{epoch:0>6}.ckpt`` (rank 0; the
wrapped model's keys, ``module.``-prefixed under DDP as under train.py's DataParallel), and
``--resume`` from the latest of them.

Loss: ``loss_der`` on the evidential outputs where the head runs (B = 1, D = 32: train.py:297-
304), otherwise the core ``mvsnet_cls_loss`` (the head cannot train at D = 192);
with ``--fused_loss`` the model hands over the raw cost volume and the loss is
``mvsnet_cls_loss_from_cost`` (HIP: no probability volume).

``--testpath/--testlist`` add train.py's per-epoch test pass (train.py:259-285, test_sample):
eval mode, no grad, the same loss as training and the six masked depth metrics
(``aarmvs.ops.depth_metrics``) of the loss's depth map, averaged over batches as
DictAverageMeter does.  Each rank takes its contiguous shard of the test samples
(``aarmvs.dist.shard_range``); the per-batch sums and batch counts are all-reduced, rank 0
prints ``avg_test_scalars:``.  ``--refine_metrics`` adds the same six metrics of the sub-plane
refined depth (``aarmvs.ops.refine_from_cost`` on the pass's cost volume; not in train.py) on a
line of their own, ``avg_test_scalars_refined:``.  ``--uncertainty_metrics`` adds, on the line
``avg_test_scalars_uncertainty:``, the sparsification error (AUSE) of the depth map's absolute
error ranked by 1 - confidence and by the depth posterior's standard deviation, entropy and
runner-up probability (``aarmvs.ops.posterior_from_cost``; not in train.py).  The evidential scalars, tensorboard summaries and the image /
.pt dumps of test_sample are not reproduced.

usage: python -m torch.distributed.run --nproc-per-node 8 -m aarmvs.train_ddp \\
           --trainpath DTU --trainlist lists/train.txt --numdepth 192 --logdir ckpt
"""
from __future__ import annotations

import argparse
import ast
import os
import sys
import time
from collections import OrderedDict

import torch
from torch.utils.data import DataLoader
from torch.utils.data.distributed import DistributedSampler

from .dist import env, init_process_group, local_device_index, shard_range, sum_over_ranks


def parse_args(argv=None):
    """train.py's arguments (train.py:28-68) that the loop uses, plus --max_steps."""
    ap = argparse.ArgumentParser(description="AA-RMVSNet training (DDP, one process per GPU)")
    ap.add_argument("--inverse_depth", type=ast.literal_eval, default=False)
    ap.add_argument("--origin_size", type=ast.literal_eval, default=False)
    ap.add_argument("--max_h", type=int, default=512)
    ap.add_argument("--max_w", type=int, default=640)
    ap.add_argument("--view_num", type=int, default=3)
    ap.add_argument("--image_scale", type=float, default=0.25)
    ap.add_argument("--dataset", default="dtu_yao")
    ap.add_argument("--trainpath")
    ap.add_argument("--trainlist")
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--lr", type=float, default=0.001)
    ap.add_argument("--batch_size", type=int, default=1, help="samples per GPU per step")
    ap.add_argument("--numdepth", type=int, default=192)
    ap.add_argument("--interval_scale", type=float, default=1.06)
    ap.add_argument("--loadckpt", default=None)
    ap.add_argument("--logdir", default="./checkpoints/debug")
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--summary_freq", type=int, default=20)
    ap.add_argument("--save_freq_checkpoint", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max_steps", type=int, default=0, help="stop each epoch after this many steps (0: all)")
    ap.add_argument("--train_light_idx", type=int, default=-1,
                    help="light index of the training images (train.py: -1, all seven)")
    ap.add_argument("--fused_loss", action="store_true",
                    help="loss from the raw cost volume on the HIP kernels (where the evidential "
                         "head does not run)")
    ap.add_argument("--checkpoint_planes", type=int, default=0,
                    help="plane-segment checkpointing of the sweep's BPTT: keep a record of this many "
                         "planes (a multiple of 16) and recompute each segment's forward before its "
                         "backward; same gradients, bit for bit (0: the whole record)")
    ap.add_argument("--testpath", default=None, help="test datapath: run train.py's per-epoch test pass")
    ap.add_argument("--testlist", default=None, help="test list")
    ap.add_argument("--test_light_idx", type=int, default=3,
                    help="light index of the test images (train.py --light_idx: 3)")
    ap.add_argument("--refine_metrics", action="store_true",
                    help="with --testpath: also report the depth metrics of the sub-plane refined depth "
                         "(the local expectation over the winning plane and its neighbours)")
    ap.add_argument("--uncertainty_metrics", action="store_true",
                    help="with --testpath: also report how well 1 - confidence and the depth posterior's "
                         "standard deviation, entropy and runner-up probability rank the depth error (AUSE)")
    return ap.parse_args(argv)


def _strip_module(state):
    return OrderedDict((k[7:] if k.startswith("module.") else k, v) for k, v in state.items())


TEST_THRESHOLDS = (2, 4, 8, 16, 32)


def _loss_and_depth(out, s, fused: bool):
    """The training loss of one batch and the depth map it comes with (train.py:297-304)."""
    from evidential.models import loss_der
    from models import mvsnet_cls_loss, mvsnet_cls_loss_from_cost
    first, evidential, _ = out
    if evidential is not None:   # loss_der reads the evidential prediction only
        return loss_der({"probability_volume": first, "evidential_prediction": evidential},
                        s["depth"], s["mask"], s["depth_values"])[:2]
    if fused:
        return mvsnet_cls_loss_from_cost(first, s["depth"], s["mask"], s["depth_values"])
    return mvsnet_cls_loss(first, s["depth"], s["mask"], s["depth_values"])


REFINED = "refined_"   # prefix of --refine_metrics' keys in run_test_pass's result


AUSE = "ause_"         # prefix of --uncertainty_metrics' keys in run_test_pass's result
RANKINGS = ("conf", "depth_std", "entropy", "runner_up")
AUSE_STEPS = 50


def _ause(err: torch.Tensor, unc: torch.Tensor) -> torch.Tensor:
    """AUSE of one image's valid pixels (1-D tensors): sort by uncertainty, descending and stable
    (NaN counts as the most uncertain); for k = 0..49 drop the first floor(k n / 50) pixels and
    average the error of the rest; the same ranked by the error itself (the oracle); the mean
    difference of the two curves over the mean error.  0 for an image with no valid pixel or no
    error."""
    n = err.numel()
    e = err.double()
    if n == 0 or float(e.sum()) == 0.0:
        return torch.zeros((), dtype=torch.float64, device=err.device)
    u = unc.double()
    u = torch.where(torch.isnan(u), torch.full_like(u, float("inf")), u)
    drop = (torch.arange(AUSE_STEPS, device=err.device) * n) // AUSE_STEPS

    def curve(rank):
        s = e[torch.sort(rank, descending=True, stable=True).indices]
        tail = torch.cat([s.flip(0).cumsum(0).flip(0), s.new_zeros(1)])   # tail[i] = sum s[i:]
        return tail[drop] / (n - drop)

    return (curve(u) - curve(e)).mean() / e.mean()


def sparsification_errors(depth_est, depth_gt, mask, cost, depth_values) -> dict:
    """{ranking: [B] float64 AUSE per image} of |depth_est - depth_gt| over mask > 0.5 under the
    RANKINGS: 1 - max softmax probability, and ops.posterior_from_cost's depth_std, entropy and
    runner_up of ``cost`` [B,D,H,W] (a log-probability volume serves as well: the statistics do
    not see a per-pixel shift of every plane)."""
    from . import ops
    post = ops.posterior_from_cost(cost.float().contiguous(), depth_values.float())
    unc = {"conf": 1.0 - torch.softmax(cost.float(), 1).amax(1), "depth_std": post["depth_std"],
           "entropy": post["entropy"], "runner_up": post["runner_up"]}
    err = (depth_est.float() - depth_gt.float()).abs()
    out = {k: [] for k in RANKINGS}
    for b in range(err.shape[0]):
        valid = mask[b] > 0.5
        for k in RANKINGS:
            out[k].append(_ause(err[b][valid], unc[k][b][valid]))
    return {k: torch.stack(v) for k, v in out.items()}


def run_test_pass(model, loader, device, fused: bool, rank: int = 0, log=print, refine: bool = False,
                  uncertainty: bool = False) -> dict:
    """train.py:259-285 on this rank's loader: per batch the loss and the masked metrics of its
    depth map, summed over batches and ranks, divided by the batch count.  ``uncertainty``: also
    the batch's mean AUSE per ranking (sparsification_errors), under AUSE-prefixed keys, from the
    same cost volume as ``refine`` uses.  ``refine``: also the
    metrics of ops.refine_from_cost's depth, under REFINED-prefixed keys.  Its cost volume is the
    model's with --fused_loss and the log of the probability volume otherwise (the same per-pixel
    shift on every plane, which the refinement's quotient cancels)."""
    from . import ops
    keys = ["loss", "abs_depth_error"] + [f"thres{t}mm_error" for t in TEST_THRESHOLDS]
    base = len(keys)
    if refine:
        keys = keys + [REFINED + k for k in keys[1:]]
    if uncertainty:
        keys = keys + [AUSE + k for k in RANKINGS]
    sums, count = [0.0] * len(keys), 0
    model.eval()
    with torch.no_grad():
        for sample in loader:
            s = {k: v.to(device) if torch.is_tensor(v) else v for k, v in sample.items()}
            out = model(s["imgs"], s["proj_matrices"], s["depth_values"])
            loss, depth_est = _loss_and_depth(out, s, fused)
            m = ops.depth_metrics(depth_est.float(), s["depth"].float(), s["mask"].float(),
                                  TEST_THRESHOLDS)
            cells = [loss.double().reshape(())] + [m[k] for k in keys[1:base]]
            if refine:
                cost = out[0] if getattr(model, "return_cost", False) else torch.log(out[0])
                r = ops.refine_from_cost(cost.float(), s["depth_values"].float())
                mr = ops.depth_metrics(r["depth_refined"], s["depth"].float(), s["mask"].float(),
                                       TEST_THRESHOLDS)
                cells += [mr[k[len(REFINED):]] for k in keys[base:] if k.startswith(REFINED)]
            if uncertainty:
                cost = out[0] if getattr(model, "return_cost", False) else torch.log(out[0])
                au = sparsification_errors(depth_est, s["depth"], s["mask"], cost, s["depth_values"])
                cells += [au[k].mean() for k in RANKINGS]
            row = torch.stack(cells).tolist()
            sums = [a + b for a, b in zip(sums, row)]
            count += 1
    total = sum_over_ranks(sums + [float(count)], device)
    log(f"test pass: rank {rank} ran {count} of {int(total[-1])} test batches")
    return {k: v / total[-1] for k, v in zip(keys, total)} if total[-1] else {}


def train(args, rank: int = 0, world: int = 1, device=None, log=print) -> dict:
    """Runs train.py's epochs on this rank's shard; returns {'losses', 'checkpoints',
    'test_scalars' (one dict per epoch when --testpath is given, else empty)[,
    'test_scalars_refined' likewise with --refine_metrics][, 'test_scalars_uncertainty' likewise
    with --uncertainty_metrics]}."""
    from datasets import find_dataset_def
    from models import EMVSNet
    device = torch.device(device or f"cuda:{local_device_index(env()[1])}")
    if device.type == "cuda":
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        # libaarmvs launches on the current device's stream: make it this rank's GPU
        torch.cuda.set_device(device)
    torch.manual_seed(args.seed)
    init_process_group(device)
    ds = find_dataset_def(args.dataset)(args.trainpath, args.trainlist, "train", args.view_num,
                                        args.numdepth, args.interval_scale, args.inverse_depth,
                                        args.origin_size, args.train_light_idx, args.image_scale)
    sampler = DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=True, seed=args.seed,
                                 drop_last=True)
    loader = DataLoader(ds, args.batch_size, sampler=sampler, num_workers=0, drop_last=True)
    test_loader = None
    if args.testpath:
        tds = find_dataset_def(args.dataset)(args.testpath, args.testlist, "test", args.view_num,
                                             args.numdepth, args.interval_scale, args.inverse_depth,
                                             args.origin_size, args.test_light_idx, args.image_scale)
        shard = torch.utils.data.Subset(tds, list(shard_range(len(tds), rank, world)))
        test_loader = DataLoader(shard, args.batch_size, shuffle=False, num_workers=0, drop_last=False)
    model = EMVSNet(disparity_level=args.numdepth, image_scale=args.image_scale,
                    max_h=args.max_h, max_w=args.max_w, return_cost=args.fused_loss,
                    checkpoint_planes=args.checkpoint_planes)
    if args.loadckpt:   # train.py:150-170: tensors only, any 'module.' prefix removed
        state = torch.load(args.loadckpt, map_location="cpu", weights_only=True)["model"]
        model.load_state_dict(_strip_module(state), strict=True)
    model = model.to(device)
    head_runs = args.batch_size == 1 and args.numdepth == 32
    if world > 1:
        # the evidential head's parameters get no gradient where it does not run
        model = torch.nn.parallel.DistributedDataParallel(
            model, device_ids=[device.index] if torch.distributed.get_backend() == "nccl" else None,
            find_unused_parameters=not head_runs)
    optimizer = torch.optim.Adam(model.parameters(), lr=args.lr)
    start_epoch = 0
    if args.resume:   # train.py:186-197
        saved = sorted((f for f in os.listdir(args.logdir) if f.endswith(".ckpt")),
                       key=lambda f: int(f.split("_")[-1].split(".")[0]))
        state = torch.load(os.path.join(args.logdir, saved[-1]), map_location="cpu", weights_only=True)
        # a checkpoint saved at another world size has (or lacks) DDP's 'module.' prefix
        core = model.module if isinstance(model, torch.nn.parallel.DistributedDataParallel) else model
        core.load_state_dict(_strip_module(state["model"]))
        optimizer.load_state_dict(state["optimizer"])
        start_epoch = state["epoch"] + 1
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=args.epochs, eta_min=2e-06)
    for _ in range(start_epoch):
        sched.step()
    if rank == 0:
        os.makedirs(args.logdir, exist_ok=True)
    losses, ckpts, test_scalars, test_scalars_refined, test_scalars_uncertainty = [], [], [], [], []
    for epoch in range(start_epoch, args.epochs):
        sampler.set_epoch(epoch)
        for step, sample in enumerate(loader):
            if args.max_steps and step >= args.max_steps:
                break
            t0 = time.time()
            model.train()
            optimizer.zero_grad()
            s = {k: v.to(device) if torch.is_tensor(v) else v for k, v in sample.items()}
            loss = _loss_and_depth(model(s["imgs"], s["proj_matrices"], s["depth_values"]), s,
                                   args.fused_loss)[0]
            loss.backward()
            optimizer.step()
            losses.append(float(loss))
            if rank == 0 and step % args.summary_freq == 0:
                log("Epoch {}/{}, Iter {}/{}, LR {}, train loss = {:.3f}, time = {:.3f}".format(
                    epoch, args.epochs, step, len(loader), optimizer.param_groups[0]["lr"],
                    losses[-1], time.time() - t0))
        sched.step()
        if rank == 0 and (epoch + 1) % args.save_freq_checkpoint == 0:   # train.py:232-237
            path = "{}/model_{:0>6}.ckpt".format(args.logdir, epoch)
            torch.save({"epoch": epoch, "model": model.state_dict(),
                        "optimizer": optimizer.state_dict()}, path)
            ckpts.append(path)
        if test_loader is not None:   # train.py:259-285
            # the bare module: ranks may hold different numbers of test batches, and DDP's
            # forward synchronises buffers across ranks
            core = model.module if isinstance(model, torch.nn.parallel.DistributedDataParallel) else model
            scalars = run_test_pass(core, test_loader, device, args.fused_loss, rank, log,
                                    refine=getattr(args, "refine_metrics", False),
                                    uncertainty=getattr(args, "uncertainty_metrics", False))
            test_scalars.append({k: v for k, v in scalars.items() if not k.startswith((REFINED, AUSE))})
            ause = {k[len(AUSE):]: v for k, v in scalars.items() if k.startswith(AUSE)}
            if ause:
                test_scalars_uncertainty.append(ause)
            refined = {k[len(REFINED):]: v for k, v in scalars.items() if k.startswith(REFINED)}
            if refined:
                test_scalars_refined.append(refined)
            if rank == 0:
                log("avg_test_scalars:", test_scalars[-1])
                if refined:
                    log("avg_test_scalars_refined:", refined)
                if ause:
                    log("avg_test_scalars_uncertainty:", ause)
    out = {"losses": losses, "checkpoints": ckpts, "test_scalars": test_scalars}
    if test_scalars_refined:
        out["test_scalars_refined"] = test_scalars_refined
    if test_scalars_uncertainty:
        out["test_scalars_uncertainty"] = test_scalars_uncertainty
    return out


def main(argv=None) -> int:
    args = parse_args(argv)
    rank, _, world = env()
    out = train(args, rank, world)
    print(f"rank {rank}/{world}: {len(out['losses'])} steps, last loss "
          f"{out['losses'][-1] if out['losses'] else float('nan'):.4f}", file=sys.stderr)
    if world > 1:
        torch.distributed.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
