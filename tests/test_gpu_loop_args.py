"""The closed-loop kernels' arguments: one QpArgs per chain (the last QP of a call runs on the first one's with three ints overridden,
qp_second_args) and the persistent kernels' argument block in device memory, one per handle, rewritten before every launch.  Everything is compared
bit for bit (np.array_equal with equal_nan) on the logged trajectories, qp_stats and the final x_meas / nominal_* / primal_vec, at the smallest shapes
(tests/loop_args_runs.py: pendulum N = 3, quadrotor N = 8, rocket N = 5 from x0 scaled to 0.3, B = 5) with SLSQP_LOOP_WAVES = 2, so every instance
changes hands between the waves; every run must show block solves in both statistics slots."""
import os
import subprocess
import sys

import numpy as np
import pytest

import loop_args_runs as R
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def separate_launches(tmp_path_factory):
    """The step-by-step loop of every plant with SLSQP_FUSE_RTI=0, from a fresh child process: k_qp_solve launched twice per step with arguments made
    by two independent make_qp_args calls -- no code of the fused chain in it."""
    path = str(tmp_path_factory.mktemp("loop_args") / "separate.npz")
    env = dict(os.environ, SLSQP_FUSE_RTI="0")
    env.pop("SLSQP_LOOP_WAVES", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "loop_args_runs.py"), path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "loop_args_runs ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return dict(np.load(path))


def _force_chain(o):
    o.fuse_rti = 2      # k_rti_chain although the batch is small


def _rounds(o):
    o.cl_persistent = 0


# ---- 1: the independent yardstick -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.SHAPES))
def test_all_three_loops_are_bitwise_the_separate_launches(name, separate_launches):
    """slsqp_cl_step through k_rti_chain, the round-based slsqp_cl_run and the persistent launch all run the changed rti_chain_dev: a comparison
    between them is blind to a lost override of (warm, stat_slot, snap_use).  The yardstick is the loop of separate launches."""
    ref = {k: separate_launches[f"{name}/{k}"] for k in R.LOG_KEYS}
    ref_fin = {k: separate_launches[f"{name}/fin/{k}"] for k in R.FIN_KEYS}
    q = ref["qp_stats"]
    print(name, "separate launches: success", ref["success"].mean(), "block solves slot 0 / 1", q[:, :, 0, 1].sum(), q[:, :, 1, 1].sum(), "warm starts slot 0 / 1",
          q[:, :, 0, 4].sum(), q[:, :, 1, 4].sum())
    assert R.real_work(ref), q[:, :, :, 1]
    assert (q[:, :, 1, 4] == 1).any()      # the last QP of a call starts warm in the separate launches: the fused ones must report the same
    m, N, B, steps, x0, W, kw = R.setup(name)
    for what, run, tune in (("stepwise chain", R.stepwise, _force_chain), ("rounds", R.decoupled, _rounds), ("persistent", R.decoupled, None)):
        out, fin = run(R.make(m, N, B, tune), steps, x0, W, **kw)
        assert R.real_work(out), what
        R.assert_same(out, fin, ref, ref_fin, (name, what))
        assert np.array_equal(out["qp_stats"][:, :, 1, 4], q[:, :, 1, 4]), what
        if what == "persistent":
            assert out["loop_stats"]["waves"] == R.WAVES and out["loop_stats"]["mpc_steps"] == B * steps


# ---- 2: reuse of a handle -----------------------------------------------------------------------------------------------------------------
def test_block_is_rewritten_for_every_launch_of_a_handle():
    """4 steps then 2 with the log on (steps, log_steps), then warm_rounds, as_first and warm_start changed between two runs: each run of the reused handle
    equals a fresh handle's run and the step-by-step loop with the same options."""
    m, N, B, _, x0, W4, kw = R.setup("pendulum", steps=4)
    W2 = W4[:2]
    cl = R.make(m, N, B)
    for steps, W in ((4, W4), (2, W2)):
        out, fin = R.decoupled(cl, steps, x0, W, close=False, **kw)
        ref, ref_fin = R.decoupled(R.make(m, N, B), steps, x0, W, **kw)
        assert R.real_work(out) and out["state_trajectory"].shape[2] == steps and out["loop_stats"]["mpc_steps"] == B * steps
        R.assert_same(out, fin, ref, ref_fin, ("reused", steps))
        ref, ref_fin = R.stepwise(R.make(m, N, B), steps, x0, W, **kw)
        R.assert_same(out, fin, ref, ref_fin, ("stepwise", steps))
    seen = []
    for warm_rounds, as_first, warm_start in ((1, 0, 1), (6, 1, 0)):      # (warm_start with them: its trace in qp_stats does not depend on the shape)
        def tune(o):
            o.warm_rounds, o.as_first, o.warm_start = warm_rounds, as_first, warm_start
        tune(cl.f.opts)
        out, fin = R.decoupled(cl, 4, x0, W4, close=False, **kw)
        ref, ref_fin = R.stepwise(R.make(m, N, B, tune), 4, x0, W4, **kw)
        assert R.real_work(out)
        R.assert_same(out, fin, ref, ref_fin, ("options", warm_rounds, as_first, warm_start))
        seen.append(out["qp_stats"])
    cl.close()
    assert seen[0][:, :, 0, 4].any() and not seen[1][:, :, 0, 4].any()      # the options reached the kernel: first QPs started warm / never did


# ---- 3: two handles alive -----------------------------------------------------------------------------------------------------------------
def test_blocks_are_per_handle():
    """A pendulum and a quadrotor handle (other plant, N and B) alive together and run alternately, each run against the handle's solo run."""
    sp = R.setup("pendulum", B=4)
    sq = R.setup("quadrotor", N=6, B=5)
    solo = {}
    for key, (m, N, B, steps, x0, W, kw) in (("p", sp), ("q", sq)):
        solo[key] = R.decoupled(R.make(m, N, B), steps, x0, W, **kw)
        assert R.real_work(solo[key][0])
    hp, hq = R.make(*sp[:3]), R.make(*sq[:3])
    for key, cl, (m, N, B, steps, x0, W, kw) in (("p", hp, sp), ("q", hq, sq), ("p", hp, sp), ("q", hq, sq)):
        out, fin = R.decoupled(cl, steps, x0, W, close=False, **kw)
        R.assert_same(out, fin, *solo[key], what=("alternating", key))
    hp.close()
    hq.close()


# ---- 4: the other loop kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ref", "pp", "scp"])
def test_the_other_loop_kernels_are_bitwise_the_step_by_step_loop(kind):
    """k_cl_loop<M, 1> (a reference), k_cl_loop<M, 3> (plant parameters: VAR = REF | PP) and k_cl_loop_scp<M, 0> (slsqp_cl_run_scp with rti = 2) at the pendulum shape."""
    from robust_nonlinear_mpc_amd import plant_param_defaults
    m, N, B, steps, x0, W, kw = R.setup("pendulum")
    mk = dict(rti=2) if kind == "scp" else {}
    if kind == "ref":
        Xref = np.tile(np.asarray(m.x_ref, dtype=float), (B, steps + 2, 1))
        Xref[:, :, 0] += 0.2 * np.sin(0.35 * np.arange(steps + 2)[None, :] + 0.7 * np.arange(B)[:, None])
        mk["reference"] = (Xref, np.tile(np.asarray(m.u_ref, dtype=float), (B, steps + 2, 1)))
    if kind == "pp":
        mk["plant_params"] = plant_param_defaults(m)[None, :] * (1.0 + 0.1 * np.linspace(-1, 1, B)[:, None] * np.array([1.0, -1.0, 0.5, 0.0]))
    ref, ref_fin = R.stepwise(R.make(m, N, B, **mk), steps, x0, W, **kw)
    out, fin = R.decoupled(R.make(m, N, B, **mk), steps, x0, W, **kw)
    assert R.real_work(out) and out["loop_stats"]["waves"] == R.WAVES
    R.assert_same(out, fin, ref, ref_fin, kind)
    if kind == "pp":
        assert np.array_equal(out["model_error"], ref["model_error"]) and out["model_error"].any()
    if kind != "scp":      # the reference / the parameters are in use
        plain, _ = R.decoupled(R.make(m, N, B), steps, x0, W, **kw)
        assert not np.array_equal(plain["state_trajectory"], out["state_trajectory"])
