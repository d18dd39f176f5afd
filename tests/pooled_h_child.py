"""Child process of test_gpu_pooled_h.py: runs the eval sweeps of that test under the
AARMVS_CELL_POOL setting of its environment (the library reads it once) and saves every output
and state tensor to the file given as argv[1] (torch.save of a flat dict of CPU tensors)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "aa-rmvsnet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from aarmvs import ops, synthetic as syn  # noqa: E402

DEV = "cuda"
REG_ENV = ("AARMVS_REG_STREAMS", "AARMVS_REG_MAP")


def scene_args(B, N, H, W, D, seed):
    sc = syn.scene(B, N, H, W, D, seed=seed)
    feats = torch.from_numpy(sc["features"]).to(DEV)
    proj = torch.from_numpy(sc["proj_matrices"])
    return (feats[0], [feats[v] for v in range(1, N)], proj[:, 0],
            [proj[:, v] for v in range(1, N)], torch.from_numpy(sc["depth_values"]))


def collect(out, tag, sw, res, cost, B, N, H, W, D):
    out[f"{tag}/depth"] = res["depth"].cpu()
    out[f"{tag}/conf"] = res["conf"].cpu()
    out[f"{tag}/cost"] = cost.cpu()
    for cell in range(5):
        for which, nm in ((0, "h"), (1, "c")):
            out[f"{tag}/{nm}{cell}"] = sw.state(B, H, W, N - 1, D, cell, which).contiguous().cpu()


def main(path):
    P = {k: torch.from_numpy(v).to(DEV) for k, v in syn.sweep_weights(11).items()}
    out = {}
    # default stream plan, D = 5: more than two wraps of the h2 and h3 rings (3 slots each)
    for tag, (B, N, H, W, D) in (("36x40", (1, 3, 36, 40, 5)), ("68x100", (2, 3, 68, 100, 5))):
        sw = ops.DepthSweep(P, DEV)
        res = sw(*scene_args(B, N, H, W, D, seed=31), want_cost=True)
        collect(out, tag, sw, res, res["cost"], B, N, H, W, D)
    # 36 x 40, D = 7 (past one wrap of h0's 6 slots): other stream plans, and a cut d_range
    B, N, H, W, D = 1, 3, 36, 40, 7
    args = scene_args(B, N, H, W, D, seed=32)
    for tag, env in (("one", {"AARMVS_REG_STREAMS": "1"}), ("five", {"AARMVS_REG_STREAMS": "5"}),
                     ("five_map", {"AARMVS_REG_STREAMS": "5", "AARMVS_REG_MAP": "02121"}), ("full", {})):
        for k in REG_ENV:
            os.environ.pop(k, None)
        os.environ.update(env)   # read per call by the library
        sw = ops.DepthSweep(P, DEV)
        res = sw(*args, want_cost=True)
        collect(out, tag, sw, res, res["cost"], B, N, H, W, D)
    for k in REG_ENV:
        os.environ.pop(k, None)
    sw = ops.DepthSweep(P, DEV)
    cost = torch.empty(B, D, H, W, device=DEV)
    sw(*args, d_range=(0, 3), cost_out=cost)
    res = sw(*args, d_range=(3, D), cost_out=cost)
    collect(out, "cut", sw, res, cost, B, N, H, W, D)
    torch.cuda.synchronize()
    torch.save(out, path)


if __name__ == "__main__":
    main(sys.argv[1])
