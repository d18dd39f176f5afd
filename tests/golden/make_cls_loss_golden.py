"""Generate tests/golden/cls_loss.npz by importing and RUNNING the reference's mvsnet_cls_loss
(models/drmvsnet.py:347-381) on the CPU, on torch.softmax of the seeded cost volumes of
tests/cls_loss_cases.py, in float32 and in float64.

Runs only where the reference is mounted (see make_golden.py, whose import_reference this
uses).  Nothing of the reference is copied: the fixture holds input digests and reference
OUTPUTS.  Per case ``<name>/...``:

  digest                 aarmvs.synthetic.array_digest of the four inputs
  loss32, loss64         the loss
  wta32, wta64           the winner-take-all depth map
  prob32, prob64         the max-probability map
  grad64                 dL/dcost (autograd through torch.softmax) in float64; for the cases
                         of cls_loss_cases.GRAD_STRIDE at every n-th pixel only (file size)
  grad32_rel_l2          relative L2 error of the float32 autograd gradient against grad64
                         (over the kept pixels; the float32 volume itself is not stored)
  gt64                   the ground-truth plane index of the float64 run, read off its gradient
                         (the one negative entry along D; 0 under a zero mask, where the
                         reference's index rule gives round(0 * argmin) = 0)
  gap64                  per pixel (p1 - p2) / p1 of the float64 top-two probabilities

Asserted here, so the tests may rely on it: no float32 probability is below 1e-30 (the
reference is outside its 0 * log(0) = NaN regime), no pixel's gap is below 1e-6 and the float32
and float64 WTA depths agree everywhere -- except in the deliberate tied_maximum case.

usage: python tests/golden/make_cls_loss_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cls_loss_cases as cases  # noqa: E402
import make_golden  # noqa: E402
from make_golden import syn  # noqa: E402


def run(drm, inp, dtype):
    t = {k: torch.from_numpy(v).to(dtype) for k, v in inp.items()}
    cost = t["cost"].clone().requires_grad_(True)
    prob = torch.softmax(cost, dim=1)
    loss, wta, pmap = drm.mvsnet_cls_loss(prob, t["depth_gt"], t["mask"], t["depth_values"],
                                          return_prob_map=True)
    loss.backward()
    return {"loss": loss.detach().numpy(), "wta": wta.numpy(), "pmap": pmap.detach().numpy(),
            "grad": cost.grad.numpy(), "prob": prob.detach().numpy()}


def main():
    drm, _ = make_golden.import_reference()
    out = {}
    for name in cases.CASES:
        inp = cases.build(name)
        r32, r64 = run(drm, inp, torch.float32), run(drm, inp, torch.float64)
        assert np.isfinite(r32["loss"]) and np.isfinite(r64["loss"]), name
        assert r32["prob"].min() >= 1e-30, (name, r32["prob"].min())
        B, D, H, W = inp["cost"].shape
        top = np.sort(r64["prob"], axis=1)[:, ::-1]
        gap = (top[:, 0] - top[:, 1]) / top[:, 0] if D > 1 else np.ones((B, H, W))
        if name != "tied_maximum":
            assert (gap < 1e-6).sum() == 0, name
            assert np.array_equal(r32["wta"].astype(np.float64), r64["wta"]), name
        gt = np.where(inp["mask"] != 0, np.argmin(r64["grad"], axis=1), 0).astype(np.int32)
        sel = slice(None, None, cases.GRAD_STRIDE.get(name, 1))
        g64 = r64["grad"].reshape(B, D, H * W)[:, :, sel]
        g32 = r32["grad"].reshape(B, D, H * W)[:, :, sel].astype(np.float64)
        den = np.sqrt((g64 ** 2).sum())
        rel = np.sqrt(((g32 - g64) ** 2).sum()) / den if den > 0 else 0.0
        fields = {"digest": np.array(syn.array_digest(*(inp[k] for k in sorted(inp)))),
                  "loss32": r32["loss"], "loss64": r64["loss"], "wta32": r32["wta"],
                  "wta64": r64["wta"], "prob32": r32["pmap"], "prob64": r64["pmap"],
                  "grad64": np.ascontiguousarray(g64), "grad32_rel_l2": np.float64(rel),
                  "gt64": gt, "gap64": gap}
        for k, v in fields.items():
            out[f"{name}/{k}"] = v
        print(f"{name}: loss64 {float(r64['loss']):.9g} |loss32 - loss64|/loss64 "
              f"{abs(float(r32['loss']) - float(r64['loss'])) / max(abs(float(r64['loss'])), 1e-300):.2e} "
              f"grad32 rel L2 {rel:.2e} prob32 err {np.abs(r32['pmap'] - r64['pmap']).max():.2e} "
              f"min p32 {r32['prob'].min():.2e}")
    path = os.path.join(HERE, "cls_loss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
