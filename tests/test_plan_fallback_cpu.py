"""Plan fallback without a GPU: tests/cl_plan_fallback_check_main.cpp, a stand-alone program with its own main around
csrc/cl_hold.hpp's age rule and csrc/slsqp_api.hip's setter and argument-block builders (compiled for the host only), built with the address and
undefined-behaviour sanitizers; and tests/plan_fallback_ref.py, the numpy restatement the GPU tests compare against, on a hand-written run."""
import os
import subprocess

import plan_fallback_ref as P
from conftest import ROOT


def test_age_rule_setter_and_argument_block_under_sanitizers():
    """cl_hold::fallback_index / plan_age_after / policy_code over hand-written sequences; slsqp_cl_set_plan_fallback's values with refusals that
    change nothing; every field the argument block had at its offset, the new ones behind the hold block inside the handle's buffer; make_hold_block
    byte-identical with the option off."""
    exe = os.path.join(ROOT, "tests", "_build", "cl_plan_fallback_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-fuse-cuid=none", "-O1", "-g", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", "-Wno-pass-failed",
                           "-Wno-invalid-offsetof", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cl_plan_fallback_check_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cl_plan_fallback_check ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_helper_on_a_hand_written_run():
    """One instance, N = 4, M = 2, eight steps.  Solves at 0, 2, 4, 6; those at 2 and 4 fail.
        s = 0  solve ok            age 0
        s = 1  hold                k = 1, code 1, age 1
        s = 2  solve fails         k = 2, code 2, age 2
        s = 3  hold                k = 3 = N - 1, code 1, age 3
        s = 4  solve fails         k = 4 > N - 1: no row left, code 0, age -1
        s = 5  hold                no backup: code 0, age -1
        s = 6  solve ok            age 0
        s = 7  hold                k = 1, code 1, age 1"""
    hold_index = [[0, 1, 0, 1, 0, 1, 0, 1]]
    success = [[1, 1, 0, 0, 0, 0, 1, 1]]      # (a hold step's entry repeats the last solve's)
    k, code, age = P.run(4, hold_index, success)
    assert k.tolist() == [[0, 1, 2, 3, 0, 0, 0, 1]]
    assert code.tolist() == [[0, 1, 2, 1, 0, 0, 0, 1]]
    assert age.tolist() == [[0, 1, 2, 3, -1, -1, 0, 1]]
    # M = 1, a failure before any success; the cap
    k, code, age = P.run(3, [[0] * 6], [[0, 1, 0, 0, 0, 1]])
    assert code.tolist() == [[0, 0, 2, 2, 0, 0]] and age.tolist() == [[-1, 0, 1, 2, -1, 0]] and k.tolist() == [[0, 0, 1, 2, 0, 0]]
    assert P.fallback_index(-1, 4) == 0 and P.fallback_index(2, 4) == 3 and P.fallback_index(3, 4) == 0 and P.fallback_index(0, 1) == 0
    assert P.step(5, 8, False, False) == (6, P.HOLD, 6) and P.step(5, 8, True, False) == (6, P.FALLBACK, 6) and P.step(5, 8, True, True) == (0, P.NOMINAL, 0)
