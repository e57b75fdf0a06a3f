"""What the persistent closed loop needs on the host for solve_every > 1, without a GPU: tests/cl_hold_loop_check_main.cpp, a stand-alone program with its
own main around csrc/cl_hold.hpp's schedule and csrc/slsqp_api.hip's option and argument builders (compiled for the host only), built with the address
and undefined-behaviour sanitizers."""
import os
import subprocess

from conftest import ROOT


def test_schedule_option_states_and_block_layout_under_sanitizers():
    """The solve / hold schedule for every M in 1..N and run lengths that end on a solve, on a first hold and on a last hold; cl_options in the 16
    states of (reference, parameters, bounds, hold): var in {0, 1, 3, 5, 7} without hold, {9, 11, 13, 15} with it and never another value, the hold
    sets found by k_cl_loop's dispatch alone, slsqp_cl_set_solve_every's range with refusals that change nothing; ScpLoopArgs with the size and every
    field offset it had before, the hold block behind it, and a staged block that does not depend on M."""
    exe = os.path.join(ROOT, "tests", "_build", "cl_hold_loop_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-fuse-cuid=none", "-O1", "-g", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", "-Wno-pass-failed",
                           "-Wno-invalid-offsetof", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cl_hold_loop_check_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cl_hold_loop_check ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
