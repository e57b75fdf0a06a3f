"""The per-handle closed-loop options in every combination: a reference, plant parameters and bounds each on or off (8 states), at the pendulum's
smallest shape (tests/loop_args_runs.py: N = 3, B = 5, 3 steps, SLSQP_LOOP_WAVES = 2) with per-instance tables of 2 rows, so every window holds the
last row.  One description of the handle's options (cl_options, csrc/slsqp_api.hip) chooses the kernels of every route; here the routes of a state
are compared with each other bit for bit.  States (0, 1, 0), (0, 0, 1) and (0, 1, 1) run the persistent kernels with the handle's own zero reference."""
import numpy as np
import pytest

import loop_args_runs as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plain_states():
    return R.option_state_runs((0, 0, 0))["step0"][0]["state_trajectory"]


@pytest.mark.parametrize("state", R.STATES, ids=lambda s: "".join(map(str, s)))
def test_every_route_of_an_option_state_is_bitwise_the_step_by_step_loop(state, plain_states):
    """The persistent launch, the round-based loop and slsqp_cl_step through the fused chain equal slsqp_cl_step through the separate launches in
    every LOG_KEYS / FIN_KEYS array; slsqp_cl_run_scp (rti = 2, two fast-SLS steps) equals its own step-by-step loop; every run did block solves, and
    every state but the plain one moves the closed loop (the options are in use: the bounds' input limit is active)."""
    runs = R.option_state_runs(state)
    for route, (out, _) in runs.items():
        assert R.real_work(out), (state, route)
    for route in ("step2", "persistent", "rounds"):
        R.assert_same(*runs[route], *runs["step0"], what=(state, route))
    R.assert_same(*runs["scp"], *runs["scp_step"], what=(state, "scp"))
    assert np.array_equal(runs["step0"][0]["state_trajectory"], plain_states) == (state == (0, 0, 0))
    assert runs["persistent"][0]["loop_stats"]["waves"] == R.WAVES and runs["scp"][0]["loop_stats"]["waves"] == R.WAVES
