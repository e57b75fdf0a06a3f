"""The event-triggered hold schedule without a GPU: tests/cl_hold_trigger_check_main.cpp, a stand-alone program with its own
main around csrc/cl_hold.hpp's decision and csrc/slsqp_api.hip's hold-block builder (compiled for the host only), built with the address and
undefined-behaviour sanitizers; and tests/hold_trigger_ref.py, the numpy restatement the GPU tests compare against, on a hand-written example."""
import os
import subprocess

import numpy as np

import hold_trigger_ref as T
from conftest import ROOT


def test_decision_setter_and_hold_block_under_sanitizers():
    """cl_hold::tube_term and cl_hold::decide in every precedence case, theta in {0, 0.5, inf}, a NaN ratio, M in 1..N; slsqp_cl_set_hold_trigger's
    range with refusals that change nothing; HoldLoopArgs with the offsets its fields had, the new ones behind M, inside the handle's buffer, and
    make_hold_block byte-identical for two calls."""
    exe = os.path.join(ROOT, "tests", "_build", "cl_hold_trigger_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-fuse-cuid=none", "-O1", "-g", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", "-Wno-pass-failed",
                           "-Wno-invalid-offsetof", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cl_hold_trigger_check_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cl_hold_trigger_check ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_tube_ratio_and_decide_of_the_helper():
    inf, nan = np.inf, np.nan
    assert T.tube_ratio([1.0, 2.0], [0.75, 2.0], [0.5, 0.1]) == 0.5
    assert T.tube_ratio([1.0, 2.0], [1.0, 2.5], [0.0, 1.0]) == 0.5 and T.tube_ratio([1.0, 2.0], [1.5, 2.0], [0.0, 1.0]) == inf      # a tube of zero width
    assert T.tube_ratio([nan, 2.0], [1.0, 2.0], [1.0, 1.0]) == inf and T.tube_ratio([1.0], [2.0], [nan]) == inf
    assert T.tube_ratio([0.3], [0.1], [0.1]) == abs(0.3 - 0.1) / 0.1
    assert T.tube_ratio(np.zeros((3, 2)), np.ones((3, 2)), np.array([2.0, 4.0])).tolist() == [0.5, 0.5, 0.5]
    for theta in (0.0, 0.5, inf):
        assert T.decide(0, 0, 3, False, nan, theta) == T.SCHEDULED
        assert T.decide(5, 2, 3, True, 0.0, theta) == T.SCHEDULED      # the cap
        assert T.decide(5, 1, 3, False, 0.0, theta) == T.FAILED
        assert T.decide(5, 1, 3, True, nan, theta) == T.TUBE
        assert T.decide(5, 1, 3, True, 0.25, theta) == (T.TUBE if theta == 0.0 else T.HOLD)
        assert T.decide(5, 0, 1, True, 0.0, theta) == T.SCHEDULED      # M = 1
    assert T.decide(5, 0, 3, True, 0.5, 0.5) == T.HOLD and T.decide(5, 0, 3, True, 0.5000001, 0.5) == T.TUBE


def test_schedule_from_log_on_a_hand_written_run():
    """One instance, one state component, N = 3, six steps, M = 3, theta = 0.5.  The logged plans (stage 0 .. 3) and back-offs per step:
        s = 0  a solve                      plan 0, 1, 2, 3     back-offs 0, .2, .4, .8
        s = 1  x = 1.05: r = .05/.2  = .25  hold 1              plan (shifted) 1, 2, 3, 3
        s = 2  x = 2.1 : r = .1/.4   = .25  k = 2 < M: hold 2   plan 2, 3, 3, 3
        s = 3  x = 3.8 : r = .8/.8   = 1    k = 3 >= M: a scheduled solve, the ratio still on record; new plan 3.8, 5, 6, 7, back-offs 0, .5, 1, 2
        s = 4  x = 5.5 : r = .5/.5   = 1    left half the tube: solve (2); the solve fails: the plan stays, success 0
        s = 5  the last solve failed: solve (3), no ratio"""
    state = [0.0, 1.05, 2.1, 3.8, 5.5, 9.0]
    plans = [[0, 1, 2, 3], [1, 2, 3, 3], [2, 3, 3, 3], [3.8, 5, 6, 7], [5, 6, 7, 7], [9.0, 9, 9, 9]]
    backs = [[0, .2, .4, .8]] * 3 + [[0, .5, 1, 2]] * 2 + [[0, 0, 0, 0]]
    out = dict(state_trajectory=np.array(state)[None, None, :], nominal_trajectory_x=np.array(plans, dtype=float).T[None, None, :, :],
               backoff_trajectory_x=np.array(backs, dtype=float).T[None, None, :, :], success=np.array([[1, 1, 1, 1, 0, 1]], dtype=bool))
    ratio, reason, hold = T.schedule_from_log(out, 3, 0.5)
    assert reason.tolist() == [[1, 0, 0, 1, 2, 3]] and hold.tolist() == [[0, 1, 2, 0, 0, 0]]
    assert np.allclose(ratio, [[0, .25, .25, 1.0, 1.0, 0]], rtol=1e-14, atol=0) and ratio[0, 1] == abs(1.05 - 1) / .2
    # the fixed period is theta = inf; theta = 0 solves at every step the state is off its plan
    _, reason, hold = T.schedule_from_log(out, 3, np.inf)
    assert reason.tolist() == [[1, 0, 0, 1, 0, 3]] and hold.tolist() == [[0, 1, 2, 0, 1, 0]]
    _, reason, hold = T.schedule_from_log(out, 3, 0.0)
    assert reason.tolist() == [[1, 2, 2, 2, 2, 3]] and not hold.any()
    _, reason, hold = T.schedule_from_log(out, 1, 0.5)
    assert reason.tolist() == [[1] * 6] and not hold.any()
