"""The figures of profiles/epilogue_errors.txt (needs a GPU): the SHA-256 over the output bytes of
ops.softmax_depth on the finite cases of tests/epilogue_cases.py (run it once under AARMVS_LIB = a
build of the commit to compare with and once without, to see whether a kernel change keeps the
bits), then, with ``rows``, one line per evidential case and tensor: the library's m, float32 CPU
torch's m_f32 and the bound, as tests/test_gpu_epilogue.py forms them.

    python tools/epilogue_profile.py [rows]
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "aa-rmvsnet_amd"), ROOT]
import epilogue_cases as ec  # noqa: E402
import test_gpu_epilogue as t  # noqa: E402
from aarmvs import _lib  # noqa: E402

h = hashlib.sha256()
for cost in [ec.sm_random(D) for D in ec.SM_UNROLL_D] + [ec.sm_volume(c) for c in ec.SM_FINITE.values()]:
    h.update(t._softmax(cost).contiguous().numpy().tobytes())
print(f"softmax_depth finite cases, {os.path.basename(_lib.LIB_PATH)}: sha256 {h.hexdigest()}")

if "rows" in sys.argv[1:]:
    print(f"{'case':28s} {'tensor':9s} {'m':>10s} {'m_f32':>10s} {'bound':>10s}  m/bound")
    worst = []
    for case in ec.EV_CASES:
        rows, bad = t.ev_rows(case, t._ev_run(case))
        for k, m, m32, b in rows:
            print(f"{case.name:28s} {k:9s} {m:10.3e} {m32:10.3e} {b:10.3e}  {m / b:.3f}")
            worst.append((m / b, m / ec.FLOOR, case.name, k))
        if bad:
            print(f"FAILED {case.name}: " + "; ".join(bad))
    print("largest m / bound:", [(f"{r:.3f}", c, k) for r, _, c, k in sorted(worst, reverse=True)[:6]])
