"""CPU check of the sweep's stream schedule (aa-rmvsnet_amd/csrc/sweep_schedule.h).

tests/sweep_schedule_check.cpp is a stand-alone host program that includes only that header:
it walks the plan of every unit -> stream map (and of the default plans) with a recording
sink, simulates happens-before between streams and events, and fails on a pair of conflicting
buffer accesses left unordered, on an event wait that resolves to another record than the one
it means, or on a call that returns with work not ordered on the caller's stream; the same for
two sweeps with their own buffers and caller streams whose calls alternate on the shared library
streams and one event array (and two sweeps on ONE buffer set must race).  It also
shows itself not vacuous: with all waits of one class dropped, some map must race.  Built with
AddressSanitizer and UBSan, like tools/asan/abi_host.cpp; no GPU, nothing loaded into Python.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM_CLANG = "/opt/rocm/lib/llvm/bin/clang++"
CXX = ROCM_CLANG if os.path.exists(ROCM_CLANG) else shutil.which("clang++") or shutil.which("g++")


@pytest.mark.skipif(CXX is None, reason="needs a host C++17 compiler")
def test_sweep_schedule_orders_every_hazard(tmp_path):
    exe = str(tmp_path / "sweep_schedule_check")
    r = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer",
                        os.path.join(ROOT, "tests", "sweep_schedule_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "sweep_schedule_check: ok" in out
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out
