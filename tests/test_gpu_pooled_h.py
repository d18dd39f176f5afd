"""The pooled hidden state handed from cell 0 to cell 1 and from cell 1 to cell 2 (convlstm.hip
CellDef<5..7>: the producer stores maxpool2x2(h') from its accumulator registers, the consumer
stages that quarter-size image) against the cells that pool the fine image while staging it
(AARMVS_CELL_POOL=0): the same fmaxf tree on the same fp32 values and the same accumulation order
per pixel, so every output of the sweep must be bit-identical.

The library reads AARMVS_CELL_POOL once, so each setting runs in a child process of its own
(pooled_h_child.py), once for the whole module.  Shapes: 36x40 has partial tiles in both
directions and a partial 16-column half of a wave patch; 68x100 (B=2) adds a full tile, a tile
cut in x inside the second column half (cell 1: 50 columns) and one cut in y inside a row pair
(cell 1: 34 rows).  D=5 wraps the 3-slot rings of h2 and h3 more than once, D=7 the 6-slot ring of
h0 that the pooled image follows."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ["depth", "conf", "cost"] + [f"{nm}{cell}" for cell in range(5) for nm in ("h", "c")]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    d = tmp_path_factory.mktemp("pooled_h")
    out = {}
    for pool in ("1", "0"):
        env = {k: v for k, v in os.environ.items()
               if k not in ("AARMVS_REG_STREAMS", "AARMVS_REG_MAP", "AARMVS_CELL_MS", "AARMVS_CELL_SKEW")}
        env["AARMVS_CELL_POOL"] = pool
        f = str(d / f"pool{pool}.pt")
        r = subprocess.run([sys.executable, os.path.join(HERE, "pooled_h_child.py"), f], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
        out[pool] = torch.load(f)
    return out


def _same(a, b, tag_a, tag_b):
    for k in KEYS:
        x, y = a[f"{tag_a}/{k}"], b[f"{tag_b}/{k}"]
        assert torch.isfinite(x).all(), (tag_a, k)
        assert torch.equal(x, y), (tag_a, tag_b, k, float((x - y).abs().max()))


@pytest.mark.parametrize("tag", ["36x40", "68x100"])
def test_pooled_h_is_bit_identical(runs, tag):
    """Depth, confidence, cost volume and every cell's h and c after D=5 planes."""
    _same(runs["1"], runs["0"], tag, tag)
    assert float(runs["1"][f"{tag}/h2"].abs().max()) > 0.0   # cell 2 saw a non-trivial pooled input


@pytest.mark.parametrize("tag", ["one", "five", "five_map"])
def test_pooled_h_follows_the_ring_under_other_stream_plans(runs, tag):
    """36x40, D=7 with the regulariser on one stream and with one unit per stream (in unit order
    and in the out-of-order assignment 02121): the pooled slots are written and waited on with
    their h slots, so each plan matches AARMVS_CELL_POOL=0 under the same plan and the pooled
    one-stream run."""
    _same(runs["1"], runs["0"], tag, tag)
    _same(runs["1"], runs["1"], tag, "one")


def test_pooled_h_survives_a_d_range_cut(runs):
    """Planes 0..3 then 3..7 in two calls against 0..7 in one."""
    _same(runs["1"], runs["1"], "cut", "full")
    _same(runs["1"], runs["0"], "cut", "cut")
