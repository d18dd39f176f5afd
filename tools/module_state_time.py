"""Host + device time of one EMVSNet forward, for the cost of repacking the sweep parameters on
every call (profiles/module_state.txt).

    python tools/module_state_time.py [TREE] [LABEL]

The model forward under no_grad with return_depth=True and feature = nn.Identity(), at the
frame of BASELINE.json's first config (3 views, 160x128, D = 48): 3 warm-up calls, 200 timed
calls, one synchronise at the end; then 200 calls of ``EMVSNet._sweep`` alone (host time of
the enqueue, and with the final synchronise).  TREE is the checkout whose package is imported (default:
this one), so that two commits can be timed in turn in one session; LABEL names the line.
"""
import os
import sys
import time

root = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), ".."))
label = sys.argv[2] if len(sys.argv) > 2 else "this"
sys.path[:0] = [root, os.path.join(root, "aa-rmvsnet_amd")]

import numpy as np   # noqa: E402
import torch   # noqa: E402
import torch.nn as nn   # noqa: E402

from aarmvs import synthetic as syn   # noqa: E402
from models import EMVSNet   # noqa: E402

WARMUP, CALLS = 3, 200
B, N, H, W, D = 1, 3, 128, 160, 48


def main():
    assert torch.cuda.is_available(), "needs a ROCm device"
    m = EMVSNet(disparity_level=D, image_scale=1.0, max_h=H, max_w=W, return_depth=True)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.init_weights(shapes, seed=2).items()})
    m.feature = nn.Identity()
    m = m.cuda()
    sc = syn.scene(B, N, H, W, D, seed=5)
    imgs = torch.from_numpy(np.moveaxis(sc["features"], 0, 1).copy()).cuda()
    proj = torch.from_numpy(sc["proj_matrices"]).cuda()
    dv = torch.from_numpy(sc["depth_values"]).cuda()
    with torch.no_grad():
        for _ in range(WARMUP):
            m(imgs, proj, dv)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            out = m(imgs, proj, dv)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / CALLS
        # the share of EMVSNet._sweep (the parameters' way into the library) in that time
        t0 = time.perf_counter()
        for _ in range(CALLS):
            m._sweep(imgs.device)
        t_host = (time.perf_counter() - t0) / CALLS
        torch.cuda.synchronize()
        t_all = (time.perf_counter() - t0) / CALLS
    # the digest shows that the trees being compared computed the same depth map
    print(f"TIME {label} ms_per_forward {dt * 1e3:.4f} sweep_host_ms {t_host * 1e3:.4f} "
          f"sweep_synced_ms {t_all * 1e3:.4f} depth_digest "
          f"{syn.array_digest(out['depth'].cpu().numpy())}")


if __name__ == "__main__":
    main()
