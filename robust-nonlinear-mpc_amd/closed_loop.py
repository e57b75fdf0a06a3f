"""Batched closed-loop robust MPC driver on the GPU.

Mirrors what the reference's closed-loop scripts do around `SCP_SLS` for ONE instance
(expe/main_rocket_robust_closed_loop.py:128-206, main_pendulum...:62-121, main_quadrotor...:98-158), for B instances at once:

    for i in range(steps):
        if i > 0: solver.reset_warm_start()            SCP_SLS_jit.py:500-551   (shift + solver reset)
        solution = solver.solve(x0)                     SCP_SLS_jit.py:65-152    (rti x [linearise, fast-SLS, nominal += delta])
        u0 = solution['primal_u'][:, 0]
        x0 = m.ddyn(x0, u0) + m.E @ w_i                 plant + bounded noise (rocket only)

Everything between `reset(...)` and the result arrays stays on the device (slsqp_cl_step); the host only supplies the
disturbance samples.  The reference obtains the very first nominal trajectory from IPOPT (out of scope): pass it as
`X_nom, U_nom`, or let the driver roll the plant out from x0 under a constant input.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .fast_sls import BatchedFastSLS, _c, _ptr


class ClosedLoopMPC:
    def __init__(self, model, N, batch, rti=None, fast_sls_rti_steps=None, device=0, x0_box_tol=0.0, solve_waves=1, reference=None, plant_params=None, bounds=None, solve_every=1, hold_trigger=None, plan_fallback=False,
                 adversary=None, adversary_amp=1.0, adversary_mask=None, meas_noise=None):
        """x0_box_tol: how far the measured state may lie outside its own stage-0 box (the tightened QP's included) before an MPC step is
        refused as infeasible; 0 = strict (1e-9), X0_BOX_TOL_OSQP_DEFAULT = what the reference's OSQP settings let through, inf = a measured
        state never fails a step on its own (slsqp_set_x0_box_tol).
        solve_waves: 1, or 2 / 4 / 8 waves per instance for the QP solves (slsqp_set_solve_waves: for one plant or a handful); run_decoupled then
        takes the step-by-step loop, the persistent kernels being one wave per instance.
        reference: see set_reference (None: the cost is around the origin of the raw state, as in the reference's scripts).
        plant_params: see set_plant_params (None: the true plant is the controller's model).
        bounds: see set_bounds (None: the model's box, the same for every instance and every step).
        solve_every: M of run / run_on_device / run_decoupled: the controller solves at steps 0, M, 2M, ... and holds its plan in between
        (hold_step: the tube policy of the last solve acts on the measured state); 1 <= M <= N; 1 (default): a solve at every step.
        hold_trigger: theta of run_decoupled(..., persistent_hold=True): an instance holds while its measured state stays inside theta x the tube of
        its plan and solves when it does not, or after M steps at the latest; None or inf (default): off, the fixed period.
        plan_fallback: True: a step that applies no freshly certified plan (a solve that failed, a hold step) runs the tube policy of the instance's
        last plan that succeeded, from a per-instance backup, while that plan has rows left (BatchedFastSLS.set_plan_fallback; rti = 1 with one
        fast-SLS step).  Honoured by step / hold_step, run, run_on_device and run_decoupled (the persistent launch with persistent_hold=True or M = 1,
        else step by step); their results then hold `plan_age` (B, steps), `hold_index` and `hold_policy` (B, steps) as int32 codes: 2 a failed solve
        that ran the backup's policy, 1 a hold step that ran it, 0 the nominal input.  False (default): every launch and every bit as before.
        adversary, adversary_amp, adversary_mask: see set_adversary (None: the disturbance is the caller's W, as before).
        meas_noise: see set_meas_noise (None: the controller is given the true plant state, as before)."""
        m = model
        self.m, self.N, self.B = m, int(N), int(batch)
        self.rti = int(m.rti if rti is None else rti)
        self.f = BatchedFastSLS(self.N, m.Q, m.R, m, m.Qf, m.Q_reg, m.R_reg, m.Q_reg_f, batch=self.B, device=device)
        # rti > 0: that many SCP iterations per MPC step (scripts); rti <= 0: SCP_SLS's default converge mode (SCP_SLS_jit.py:20-21).
        # fast_sls_rti_steps: None -> the script's value when rti is the script's, the reference default (converge, None) otherwise
        if fast_sls_rti_steps is None and rti is None:
            fast_sls_rti_steps = m.fast_sls_rti_steps
        self.f.set_rti_steps(fast_sls_rti_steps)
        self.f.opts.x0_box_tol = float(x0_box_tol)
        if solve_waves != 1:
            self.f.opts.solve_waves = int(solve_waves)
        self.steps_done = 0
        self.solve_every = self._check_solve_every(solve_every)
        self.hold_trigger = self._check_hold_trigger(hold_trigger, first=True)
        self.plan_fallback = bool(plan_fallback)
        if self.plan_fallback:
            self.f.set_plan_fallback(True)
        if reference is not None:
            self.set_reference(reference)
        if plant_params is not None:
            self.set_plant_params(plant_params)
        if bounds is not None:
            self.set_bounds(bounds)
        if adversary is not None:
            self.set_adversary(adversary, adversary_amp, adversary_mask)
        self._mn = None      # the measurement-noise table the loop in progress runs under (latched by reset)
        if meas_noise is not None:
            self.set_meas_noise(meas_noise)

    def set_meas_noise(self, Nm):
        """Measurement noise from the next reset() on (BatchedFastSLS.set_meas_noise): Nm (T,nx) or (B,T,nx), the error of the measurement in state
        coordinates, row min(s, T - 1) for MPC step s, last row held; None clears it.  The controller is then pinned to x_meas = x_plant + n_s while
        the plant (and the adversary) run on x_plant.  Honoured by run, run_on_device, run_decoupled, step and hold_step.  Their results change only
        while the option is on: `state_trajectory` is the TRUE plant trajectory (so `constraint_margin`, `disturbance_used` and `model_error` audit the
        real system), `measured_trajectory` (B,nx,steps) what the controller saw, `meas_noise` the table; `x0_violation`, `tube_ratio` and
        `solve_trigger` stay what the controller computed from its measurement.  step / hold_step return `x_plant` (the true state after the plant
        step) beside `x_next` (the next measurement)."""
        self.f.set_meas_noise(Nm)

    def _meas_row(self, s):
        """(B,nx) or (nx,): the latched table's row for MPC step s."""
        return self._mn[..., min(int(s), self._mn.shape[-2] - 1), :]

    def _meas_keys(self):
        """What a step under measurement noise adds: the true state its plant step left; nothing without the option."""
        return {} if self._mn is None else dict(x_plant=self.f.get("x_plant", (self.m.nx,)))

    def set_adversary(self, policy, amp=1.0, mask=None):
        """State-feedback disturbance adversary from the next plant step on (BatchedFastSLS.set_adversary): "nearest_bound" pushes every state towards
        the nearer side of its box in force (set_bounds, else the model's), "away_from_target" away from the reference (set_reference, else the
        origin), as w_j = amp sign(sum_i d_i E_ij) on the channels of `mask` ((nx,), None: all); the other channels keep the W the run was given.
        None / "off" / 0 clears it.  step, hold_step and every run method then return `w_applied` -- (B,nx) per step, (steps,B,nx) per run -- and
        the runs `disturbance_used` (steps,B), computed from it; amp > 1 shows there as values above 1."""
        self.f.set_adversary(policy, amp, mask)

    def _adversary_keys(self):
        """What a step under the adversary adds: the sample its plant step used; nothing without the option."""
        return {} if self.f.adversary is None else dict(w_applied=self.f.get("w_applied", (self.m.nx,)))

    def _check_solve_every(self, M):
        M = self.solve_every if M is None else int(M)
        if not 1 <= M <= self.N:
            raise ValueError(f"solve_every must lie in 1..N = {self.N} (K has N rows: at most N - 1 hold steps between two solves), got {M}")
        return M

    def _check_hold_trigger(self, theta, first=False):
        theta = (float("inf") if first else self.hold_trigger) if theta is None else float(theta)
        if not theta >= 0.0:
            raise ValueError(f"hold_trigger must lie in [0, inf] (a fraction of the tube; inf = off), got {theta}")
        return theta

    def _no_trigger(self, theta, who):
        if self._check_hold_trigger(theta) < float("inf"):
            raise ValueError(f"{who}: hold_trigger runs in the persistent launch only: run_decoupled(..., solve_every=M, persistent_hold=True, hold_trigger=theta) "
                             "(a batch that steps together has one schedule; tube_ratio() gives a step-by-step caller the quantity to decide on)")

    def tube_ratio(self):
        """(B,) the tube ratio of every instance for the hold step that hold_step() would run next (BatchedFastSLS.tube_ratio)."""
        return self.f.tube_ratio()

    def set_bounds(self, bounds, gf=None):
        """The box in force from the next reset() on: a pair (g, gf) (tuple or list) or g, gf -- rows over MPC time in the model's layout [hi; -lo], (T,ni) / (T,ni_f)
        shared by the batch or (B,T,ni) / (B,T,ni_f) per instance, row t for MPC step t after reset(), last row held (BatchedFastSLS.set_bounds;
        bounds.box_bounds builds them from per-component limits); gf None: the model's terminal box; None: the model's box again.  Logged runs then
        hold `constraint_margin` (steps, B): the smallest distance of the measured state and applied input to the box in force at that time (negative:
        outside)."""
        if isinstance(bounds, (tuple, list)) and len(bounds) == 2 and gf is None and np.ndim(bounds[0]) >= 2:      # (a pair, not two rows of one g)
            bounds, gf = bounds
        self.f.set_bounds(bounds, gf)

    def _add_margin(self, out):
        if self.f.bounds is not None:
            from .bounds import constraint_margin
            out.update(constraint_margin=constraint_margin(self.m, self.f.bounds[0], out["state_trajectory"], out["input_trajectory"]),
                       bounds_g=np.array(self.f.bounds[0]), bounds_gf=np.array(self.f.bounds[1]))
        return out

    def set_plant_params(self, plant_params):
        """Physical parameters of the TRUE plant from the next step on: a dict {name: scalar or (B,)}, an array (np,) or (B,np)
        (models.pack_plant_params), None: the plant is the controller's model again.  Only the plant step x+ = ddyn_p(x, u0) + E w uses them; the
        linearisation, the warm-start shift and the nominal initialiser keep the model's constants.  Logged runs then hold `model_error`
        (ddyn_p - ddyn of every plant step) and `disturbance_used`."""
        self.f.set_plant_params(plant_params)

    def set_reference(self, reference, Uref=None):
        """What the closed loop tracks from the next reset() on: a tuple (Xref, Uref) or Xref, Uref -- arrays (T,nx), (T,nu) shared by the batch or
        (B,T,nx), (B,T,nu) per instance, row t for MPC step t after reset(), last row held (BatchedFastSLS.set_reference); "neutral": the
        setpoint (model.x_ref, model.u_ref), the plant's own neutral point; None: no reference."""
        if isinstance(reference, str):
            if reference != "neutral":
                raise ValueError(f"reference: unknown shorthand {reference!r} (only \"neutral\")")
            reference, Uref = np.asarray(self.m.x_ref, dtype=float)[None, :], np.asarray(self.m.u_ref, dtype=float)[None, :]
        elif isinstance(reference, tuple) and len(reference) == 2 and Uref is None:
            reference, Uref = reference
        self.f.set_reference(reference, Uref)

    def close(self):
        self.f.close()

    def reset(self, x_meas, X_nom=None, U_nom=None, u_init=None, solve_nominal=False, max_qp=120, tol=1e-7, rho=1e3, continuation=1):
        """x_meas (B,nx).  X_nom (B,N+1,nx), U_nom (B,N,nu) optional initial nominal; else roll-out under `u_init` (default: the
        model's neutral input).  solve_nominal=True then solves the nominal NLP from that guess on the GPU (the role IPOPT has in
        SCP_SLS.solve_nominal_trajectory, SCP_SLS_jit.py:161-188); per-instance outcome in self.nlp_status (0 = KKT point found).
        continuation=K > 1 (far-away states): the NLP is solved for x_ref + s (x_meas - x_ref), s = 1/K, 2/K, ..., 1, each stage from the
        previous stage's trajectory (the initial-state constraint is damped like the others, so a stage moves x_0 gradually)."""
        f, m = self.f, self.m
        x_meas = _c(x_meas)
        assert x_meas.shape == (self.B, m.nx)
        Xn = None if X_nom is None else _c(X_nom)
        Un = None if U_nom is None else _c(U_nom)
        ui = _c(m.u_ref if u_init is None else u_init)
        K = max(1, int(continuation)) if solve_nominal and Xn is None else 1
        x_first = x_meas if K == 1 else _c(m.x_ref + (x_meas - m.x_ref) / K)
        L.check(f.lib.slsqp_cl_init(f.h, _ptr(x_first), _ptr(Xn), _ptr(Un), _ptr(ui), L.HOST))
        self._mn = f.meas_noise      # (slsqp_cl_init has latched it: x_plant <- x_first, x_meas <- x_first + n_0)
        self.steps_done = 0
        self._W_log = []      # the disturbance samples of the run's steps (disturbance_used)
        self.nlp_status = None
        if solve_nominal:
            L.check(f.lib.slsqp_nominal_solve(f.h, int(max_qp), float(tol), float(rho), C.byref(f.opts)))
            for k in range(2, K + 1):
                xs = _c(m.x_ref + (x_meas - m.x_ref) * (k / K))
                if self._mn is not None:      # (the stages are the controller's: each is pinned to what it would measure there; the truth ends at x_meas)
                    L.check(f.lib.slsqp_set(f.h, b"x_plant", _ptr(xs), L.HOST))
                    xs = _c(xs + self._meas_row(0))
                L.check(f.lib.slsqp_set(f.h, b"x_meas", _ptr(xs), L.HOST))
                L.check(f.lib.slsqp_nominal_solve(f.h, int(max_qp), float(tol), float(rho), C.byref(f.opts)))
            self.nlp_status = f.get("nlp_status", (), np.int32)
            self.nlp_iterations = f.get("nlp_iterations", (), np.int32)
            self.nlp_info = f.get("nlp_info", (12,))

    def step(self, w=None, fetch=True):
        """One MPC step of the whole batch.  w (B,nx): disturbance sample in [-1,1]^nx (x+ = ddyn(x,u0) + E w), or None."""
        f = self.f
        wv = None if w is None else _c(w)
        L.check(f.lib.slsqp_cl_step(f.h, self.rti, _ptr(wv), L.HOST, C.byref(f.opts)))
        self.steps_done += 1
        self._W_log.append(wv)
        if not fetch:
            return None
        m, N = self.m, self.N
        return dict(
            u0=f.get("u0", (m.nu,)), x_next=f.get("x_meas", (m.nx,)),
            nominal_x=f.get("nominal_x", (N + 1, m.nx)), nominal_u=f.get("nominal_u", (N, m.nu)),
            backoff_x=f.get("backoff_x", (N + 1, m.nx)), backoff_u=f.get("backoff_u", (N, m.nu)),
            success=f.get("scp_success", (), np.int32).astype(bool), status=f.get("status", (), np.int32),
            scp_iterations=f.get("scp_iterations", (), np.int32), primal_infeasibility=f.get("primal_infeasibility", ()),
            x0_violation=np.where(f.get("qp_stats", (2, 8), np.int32)[:, :, 6] == -1, 0.0, f.get("x0_viol", (2,))),      # (0 where the QP took no part, as in the log)
            t_qp_ms=f.timing_ms()["qp"], t_riccati_ms=f.timing_ms()["sweep"], t_jac_ms=f.timing_ms()["jac"],
            **self._fallback_keys(solved=True), **self._adversary_keys(), **self._meas_keys(),
        )

    def _fallback_keys(self, solved):
        """plan_fallback: what the step left -- `plan_age`, and on a solved step `hold_policy` (2 where a failed solve ran the backup's policy) and the
        measured state the input was computed for is the caller's to keep; nothing without the option."""
        if not self.plan_fallback:
            return {}
        f = self.f
        out = dict(plan_age=f.get("plan_age", (), np.int32))
        if solved:
            out.update(hold_index=np.zeros(self.B, dtype=np.int32), hold_policy=np.where(f.get("scp_success", (), np.int32) != 0, 0, f.get("hold_policy", (), np.int32)).astype(np.int32))
        else:
            out.update(hold_policy=f.get("hold_policy", (), np.int32))
        return out

    def hold_step(self, w=None, fetch=True):
        """One closed-loop step of the whole batch without a solve (BatchedFastSLS.hold_step): the plan of the last step() is held, its tube policy
        gives the input from the measured state.  The keys of step(); `nominal_x` / `nominal_u` are the plan moved to this step, the back-offs and
        `success` the last solve's, plus `state` (the measured state the input was computed for), `hold_index` and `hold_policy` (False: the instance
        has no valid plan and applied the nominal input)."""
        f, m, N = self.f, self.m, self.N
        wv = None if w is None else _c(w)
        state = f.get("x_meas", (m.nx,)) if fetch else None
        f.hold_step(wv)
        self.steps_done += 1
        self._W_log.append(wv)
        if not fetch:
            return None
        out = dict(
            u0=f.get("u0", (m.nu,)), x_next=f.get("x_meas", (m.nx,)), state=state,
            nominal_x=f.get("nominal_x", (N + 1, m.nx)), nominal_u=f.get("nominal_u", (N, m.nu)),
            backoff_x=f.get("backoff_x", (N + 1, m.nx)), backoff_u=f.get("backoff_u", (N, m.nu)),
            success=f.get("scp_success", (), np.int32).astype(bool), status=f.get("status", (), np.int32),
            scp_iterations=np.zeros(self.B, dtype=np.int32), primal_infeasibility=f.get("primal_infeasibility", ()),
            x0_violation=np.zeros((self.B, 2)), hold_index=f.get("hold_index", (), np.int32), hold_policy=f.get("hold_policy", (), np.int32).astype(bool),
            t_qp_ms=0.0, t_riccati_ms=0.0, t_jac_ms=0.0,
        )
        out.update(self._fallback_keys(solved=False))      # (plan_fallback: the policy as its code, and plan_age)
        out.update(self._adversary_keys())
        out.update(self._meas_keys())
        return out

    def run_on_device(self, x0, steps, W=None, X_nom=None, U_nom=None, solve_nominal=False, continuation=1, solve_every=None, hold_trigger=None):
        """Same result as run(), but the per-step records stay in device buffers (slsqp_cl_log) and are read back once at the end: the only
        host -> device traffic per MPC step is the disturbance sample (B,nx).  solve_every = M > 1 (None: the constructor's): see run()."""
        f, m, N, B = self.f, self.m, self.N, self.B
        M = self._check_solve_every(solve_every)
        self._no_trigger(hold_trigger, "run_on_device")
        L.check(f.lib.slsqp_cl_log(f.h, int(steps)))
        self.reset(x0, X_nom, U_nom, solve_nominal=solve_nominal, continuation=continuation)
        t_qp, t_ric, t_jac = np.zeros((steps, 1)), np.zeros((steps, 1)), np.zeros((steps, 1))
        for i in range(steps):
            if i % M:
                self.hold_step(None if W is None else W[i], fetch=False)
            else:
                self.step(None if W is None else W[i], fetch=False)
            t = f.timing_ms()
            t_qp[i], t_ric[i], t_jac[i] = t["qp"], t["sweep"], t["jac"]
        out = self._log_result(steps, t_jac, t_qp, t_ric)
        if M > 1 or self.plan_fallback:
            out.update(self._hold_log(steps))
        return out

    def _hold_log(self, steps):
        """`hold_index` and `hold_policy` (B, steps) of a logged run; with plan_fallback the policy as its int32 code, and `plan_age`."""
        f = self.f
        pol = f.get("log_hold_policy", (steps,), np.int32)
        out = dict(hold_index=f.get("log_hold", (steps,), np.int32), hold_policy=pol if self.plan_fallback else pol.astype(bool))
        if self.plan_fallback:
            out["plan_age"] = f.get("log_plan_age", (steps,), np.int32)
        return out

    def _log_result(self, steps, t_jac, t_qp, t_ric):
        """The arrays of the device-side log (slsqp_cl_log) laid out like the reference's npz, batch axis first."""
        f, m, N = self.f, self.m, self.N
        lx = f.get("log_nominal_x", (steps, N + 1, m.nx)); lu = f.get("log_nominal_u", (steps, N, m.nu))
        lbx = f.get("log_backoff_x", (steps, N + 1, m.nx)); lbu = f.get("log_backoff_u", (steps, N, m.nu))
        u0 = f.get("log_u0", (steps, m.nu))
        out = dict(
            state_trajectory=f.get("log_state", (steps, m.nx)).transpose(0, 2, 1).copy(),
            input_trajectory=u0[:, :max(steps - 1, 0)].transpose(0, 2, 1).copy(),
            nominal_trajectory_x=lx.transpose(0, 3, 2, 1).copy(), nominal_trajectory_u=lu.transpose(0, 3, 2, 1).copy(),
            backoff_trajectory_x=lbx.transpose(0, 3, 2, 1).copy(), backoff_trajectory_u=lbu.transpose(0, 3, 2, 1).copy(),
            t_jac=t_jac, t_qp=t_qp, t_riccati=t_ric,
            success=f.get("log_success", (steps,), np.int32).astype(bool), scp_iterations=f.get("log_scp_iterations", (steps,), np.int32),
            primal_infeasibility=f.get("log_primal_infeasibility", (steps,)),
            x0_violation=f.get("log_x0_viol", (steps, 2)),
        )
        if self._mn is not None:      # measurement noise: the audit keys below are computed from the TRUE trajectory
            out.update(state_trajectory=f.get("log_plant_state", (steps, m.nx)).transpose(0, 2, 1).copy(),
                       measured_trajectory=f.get("log_measured_state", (steps, m.nx)).transpose(0, 2, 1).copy(), meas_noise=np.array(self._mn))
        wa = None if f.adversary is None else f.get("log_w_applied", (steps, m.nx)).transpose(1, 0, 2).copy()      # (steps, B, nx)
        if f.plant_params is not None:
            me = f.get("log_model_error", (steps, m.nx))
            out.update(model_error=me.transpose(0, 2, 1).copy(), disturbance_used=self._disturbance_used(me, wa), plant_params=np.array(f.plant_params))
        if wa is not None:
            out["w_applied"] = wa
            out.setdefault("disturbance_used", self._disturbance_used(np.zeros((self.B, steps, m.nx)), wa))
        return self._add_margin(out)

    def _disturbance_used(self, me, w_applied=None):
        """me (B,steps,nx): ddyn_p - ddyn of every plant step; w_applied (steps,B,nx): the samples the plant steps used where an adversary chose
        them (None: the W the run was given).  (steps,B): max_i |(E^-1 me)_i + w_i|, how much of the unit box the tubes assume the
        mismatch and the noise sample of the step used together (> 1: outside what the tubes were designed for); NaN when E is not square and
        nonsingular."""
        m, B, steps = self.m, me.shape[0], me.shape[1]
        E = np.asarray(m.E, dtype=float)
        if E.ndim != 2 or E.shape[0] != E.shape[1] or np.linalg.matrix_rank(E) < E.shape[0]:
            return np.full((steps, B), np.nan)
        wm = np.linalg.solve(E, me.reshape(-1, m.nx).T).T.reshape(B, steps, m.nx)
        for i, w in enumerate(self._W_log[:steps] if w_applied is None else w_applied[:steps]):
            if w is not None:
                wm[:, i] += w
        return np.max(np.abs(wm), axis=2).T.copy()

    def run_decoupled(self, x0, steps, W=None, X_nom=None, U_nom=None, solve_nominal=False, continuation=1, budget_ms=8.0, cut_frac=0.0, solve_every=None, persistent_hold=False, hold_trigger=None, persistent_converge=False):
        """Same results as run_on_device() -- bit for bit -- with the instances advancing through their MPC steps independently, so nobody waits for
        the slowest instance of a step.
        rti = 1 with one fast-SLS step (the rocket script's setting): slsqp_cl_run.  With opts.cl_persistent (the default) the whole loop is ONE launch:
        waves take instances from a device-side FIFO and run one MPC step each time; with opts.cl_persistent = 0 it runs in rounds (a chain of QP
        solves that is not done budget_ms after its launch started suspends itself and resumes in the next round; cut_frac: see slsqp_cl_run).
        Every other setting slsqp_cl_step takes with a fixed number of fast-SLS steps (rti > 1, SCP converge mode rti <= 0, rti_steps > 1: the
        pendulum and quadrotor scripts, SCP_SLS's default): slsqp_cl_run_scp, always one persistent launch (budget_ms / cut_frac ignored).  Fast-SLS
        converge mode (fast_sls_rti_steps None; but see persistent_converge), precision = 1 and SLSQP_FUSE_RTI=0 are refused with the library's message.
        solve_every = M > 1 (None: the constructor's): by default the run takes the step-by-step loop (run_on_device), as it does for solve_waves > 1.
        persistent_hold=True runs it as the persistent launch instead, the hold steps of an instance inside the loop of the wave that solved for it
        (BatchedFastSLS.set_solve_every; rti = 1 with one fast-SLS step and opts.cl_persistent only, every other setting raises with the library's
        message): the same bits, what a persistent run returns, plus `hold_index` and `hold_policy`.
        hold_trigger = theta < inf (None: the constructor's; with persistent_hold and M > 1 only, anything else raises): event-triggered solves -- an
        instance holds while its tube ratio is <= theta and solves when it is not, or after M steps at the latest (slsqp_cl_set_hold_trigger); the result
        then also holds `tube_ratio` (B, steps) and `solve_trigger` (B, steps) (0 hold, 1 scheduled, 2 left theta x tube, 3 the last solve had failed).
        persistent_converge=True with fast-SLS converge mode (fast_sls_rti_steps None): the run is taken as one persistent launch in which every
        instance iterates its fast-SLS solves to convergence on its own (BatchedFastSLS.set_sls_converge, set for this call and cleared afterwards;
        at most opts.max_sls_iter iterations per solve); the result then also holds `sls_iterations` (B, steps), iteration_number as each step left
        it.  With a fixed number of fast-SLS steps it changes nothing.  False (default): that mode raises with the library's message, as before.
        Adds `qp_stats` (B, steps, 2, 8) (next to `x0_violation` (B, steps, 2), which every logged run has), `rounds` and (persistent) `loop_stats`; the t_* arrays hold the run's totals in their first entry."""
        f, m, N, B = self.f, self.m, self.N, self.B
        M = self._check_solve_every(solve_every)
        hold = M > 1 and persistent_hold
        theta = self._check_hold_trigger(hold_trigger)
        if not persistent_hold:
            self._no_trigger(theta, "run_decoupled without persistent_hold")
        if f.opts.solve_waves > 1 or (M > 1 and not hold):      # the persistent kernels are one wave per instance; M > 1 without persistent_hold: the same loop, step by step (no qp_stats / loop_stats)
            out = self.run_on_device(x0, steps, W, X_nom, U_nom, solve_nominal=solve_nominal, continuation=continuation, solve_every=M, hold_trigger=theta)      # (a finite theta raises there)
            out["rounds"] = steps
            return out
        if hold and not (self.rti == 1 and f.opts.rti_steps == 1):      # (asked here, before anything is reset: the library's words)
            raise RuntimeError(f"slsqp: slsqp_cl_run_scp: solve_every = {M} needs rti = 1 with one fast-SLS step (slsqp_cl_run's kernel): the general "
                               "persistent loop keeps its gains per SCP iteration and solves at every step (use slsqp_cl_step / slsqp_cl_hold_step)")
        conv = bool(persistent_converge) and f.opts.rti_steps <= 0
        f.set_solve_every(M if hold else 1)
        f.set_hold_trigger(theta if hold else None)
        f.set_sls_converge(conv)
        try:
            return self._run_persistent(x0, steps, W, X_nom, U_nom, solve_nominal, continuation, budget_ms, cut_frac, hold, conv)
        finally:
            f.set_solve_every(1)      # (the handle's M, theta and converge option are this call's: the next run says what it wants)
            f.set_hold_trigger(None)
            f.set_sls_converge(False)

    def _run_persistent(self, x0, steps, W, X_nom, U_nom, solve_nominal, continuation, budget_ms, cut_frac, hold, conv=False):
        f, m, N, B = self.f, self.m, self.N, self.B
        L.check(f.lib.slsqp_cl_log(f.h, int(steps)))
        self.reset(x0, X_nom, U_nom, solve_nominal=solve_nominal, continuation=continuation)
        Wc = None if W is None else _c(W)
        assert Wc is None or Wc.shape == (steps, B, m.nx)
        self._W_log = [None] * steps if Wc is None else list(Wc)
        rounds = C.c_int(0)
        one_by_one = self.rti == 1 and f.opts.rti_steps == 1
        if one_by_one:
            L.check(f.lib.slsqp_cl_run(f.h, int(steps), _ptr(Wc), L.HOST, C.byref(f.opts), float(budget_ms), float(cut_frac), C.byref(rounds)))
        else:
            L.check(f.lib.slsqp_cl_run_scp(f.h, int(steps), self.rti, _ptr(Wc), L.HOST, C.byref(f.opts)))
            rounds.value = 1
        self.steps_done = steps
        t = f.timing_ms()
        t_qp, t_ric, t_jac = np.zeros((steps, 1)), np.zeros((steps, 1)), np.zeros((steps, 1))
        t_qp[0], t_ric[0], t_jac[0] = t["qp"], t["sweep"], t["jac"]
        out = self._log_result(steps, t_jac, t_qp, t_ric)
        out["qp_stats"] = f.get("log_qp_stats", (steps, 2, 8), np.int32)
        out["rounds"] = rounds.value
        if f.opts.cl_persistent or not one_by_one:      # one persistent launch: how busy the instance queue kept the waves
            st = (C.c_double * L.CL_RUN_STATS_LEN)()
            L.check(f.lib.slsqp_cl_run_stats(f.h, st, L.CL_RUN_STATS_LEN))
            out["loop_stats"] = dict(waves=int(st[0]), busy_ms=float(st[1]), mpc_steps=int(st[2]), launch_ms=float(st[3]))
        if conv:
            out["sls_iterations"] = f.get("log_sls_iterations", (steps,), np.int32)
        if hold or self.plan_fallback:
            out.update(self._hold_log(steps))
        if hold:
            if f.get_hold_trigger() < float("inf"):
                out.update(tube_ratio=f.get("log_tube_ratio", (steps,)), solve_trigger=f.get("log_solve_trigger", (steps,), np.int32))
        return out

    def run(self, x0, steps, W=None, X_nom=None, U_nom=None, solve_nominal=False, solve_every=None, hold_trigger=None):
        """Closed loop of `steps` MPC steps from x0 (B,nx); W (steps,B,nx) disturbance samples or None.  Returns arrays laid out
        like the reference's npz (expe/main_rocket_robust_closed_loop.py:189-206) with a leading batch axis.
        solve_every = M > 1 (None: the constructor's): a solve at steps 0, M, 2M, ..., hold_step() in between; the result then also holds `hold_index`
        (B, steps) (0: a solved step, k: the k-th hold step since the solve) and `hold_policy` (B, steps) (the tube policy ran)."""
        m, N, B = self.m, self.N, self.B
        M = self._check_solve_every(solve_every)
        self._no_trigger(hold_trigger, "run")
        self.reset(x0, X_nom, U_nom, solve_nominal=solve_nominal)
        out = dict(
            state_trajectory=np.zeros((B, m.nx, steps)), input_trajectory=np.zeros((B, m.nu, max(steps - 1, 0))),
            nominal_trajectory_x=np.zeros((B, m.nx, N + 1, steps)), nominal_trajectory_u=np.zeros((B, m.nu, N, steps)),
            backoff_trajectory_x=np.zeros((B, m.nx, N + 1, steps)), backoff_trajectory_u=np.zeros((B, m.nu, N, steps)),
            t_jac=np.zeros((steps, 1)), t_qp=np.zeros((steps, 1)), t_riccati=np.zeros((steps, 1)),
            success=np.zeros((B, steps), dtype=bool), scp_iterations=np.zeros((B, steps), dtype=np.int32),
            primal_infeasibility=np.full((B, steps), np.nan), x0_violation=np.zeros((B, steps, 2)),
        )
        if M > 1 or self.plan_fallback:
            out.update(hold_index=np.zeros((B, steps), dtype=np.int32), hold_policy=np.zeros((B, steps), dtype=np.int32 if self.plan_fallback else bool))
        if self.plan_fallback:
            out.update(plan_age=np.zeros((B, steps), dtype=np.int32))
        if self._mn is not None:
            out.update(measured_trajectory=np.zeros((B, m.nx, steps)), meas_noise=np.array(self._mn))
        for i in range(steps):
            if self._mn is not None:
                xp_i, xm_i = self.f.get("x_plant", (m.nx,)), self.f.get("x_meas", (m.nx,))
            if i % M:
                r = self.hold_step(None if W is None else W[i])
                out["hold_index"][:, i] = r["hold_index"]
            else:
                r = self.step(None if W is None else W[i])
            if "hold_policy" in r and "hold_policy" in out:
                out["hold_policy"][:, i] = r["hold_policy"]
            if self.plan_fallback:
                out["plan_age"][:, i] = r["plan_age"]
            out["state_trajectory"][:, :, i] = r["state"] if i % M else r["nominal_x"][:, 0, :]
            if self._mn is not None:      # (the true state and the measurement at the top of the step)
                out["state_trajectory"][:, :, i], out["measured_trajectory"][:, :, i] = xp_i, xm_i
            if i < steps - 1:
                out["input_trajectory"][:, :, i] = r["u0"]
            out["nominal_trajectory_x"][:, :, :, i] = r["nominal_x"].transpose(0, 2, 1)
            out["nominal_trajectory_u"][:, :, :, i] = r["nominal_u"].transpose(0, 2, 1)
            out["backoff_trajectory_x"][:, :, :, i] = r["backoff_x"].transpose(0, 2, 1)
            out["backoff_trajectory_u"][:, :, :, i] = r["backoff_u"].transpose(0, 2, 1)
            out["t_qp"][i], out["t_riccati"][i], out["t_jac"][i] = r["t_qp_ms"], r["t_riccati_ms"], r["t_jac_ms"]
            out["primal_infeasibility"][:, i] = r["primal_infeasibility"]
            out["success"][:, i] = r["success"]
            out["scp_iterations"][:, i] = r["scp_iterations"]
            out["x0_violation"][:, i] = r["x0_violation"]
            if self.f.plant_params is not None:
                out.setdefault("model_error", np.zeros((B, m.nx, steps)))[:, :, i] = self.f.get("model_err", (m.nx,))
            if "w_applied" in r:
                out.setdefault("w_applied", np.zeros((steps, B, m.nx)))[i] = r["w_applied"]
        wa = out.get("w_applied")
        if "model_error" in out:
            out.update(disturbance_used=self._disturbance_used(out["model_error"].transpose(0, 2, 1), wa), plant_params=np.array(self.f.plant_params))
        elif wa is not None:
            out["disturbance_used"] = self._disturbance_used(np.zeros((B, steps, m.nx)), wa)
        return self._add_margin(out)

    def save_npz(self, path, out, b=0):
        """Write instance b with exactly the key set the reference's plot()/loaders read (main_rocket...:189-206, 218-241); what the result
        dictionary holds beyond that (success, qp_stats, x0_violation, ...) is not written."""
        m = self.m
        steps = out["state_trajectory"].shape[2]
        np.savez(path, state_trajectory=out["state_trajectory"][b], input_trajectory=out["input_trajectory"][b],
                 nominal_trajectory_x=out["nominal_trajectory_x"][b], nominal_trajectory_u=out["nominal_trajectory_u"][b],
                 backoff_trajectory_x=out["backoff_trajectory_x"][b], backoff_trajectory_u=out["backoff_trajectory_u"][b],
                 dt=0.05, g=m.g, nx=m.nx, nu=m.nu, simulation_time_steps=steps, N=self.N,
                 t_jac=out["t_jac"], t_qp=out["t_qp"], t_riccati=out["t_riccati"],
                 **({} if "model_error" not in out else dict(      # (only a run with plant parameters: the key set of every other run is unchanged)
                     plant_params=out["plant_params"] if out["plant_params"].ndim == 1 else out["plant_params"][b], model_error=out["model_error"][b],
                     disturbance_used=out["disturbance_used"][:, b])),
                 **({} if "constraint_margin" not in out else dict(      # (only a run with bounds, likewise)
                     constraint_margin=out["constraint_margin"][:, b], bounds_g=out["bounds_g"] if out["bounds_g"].ndim == 2 else out["bounds_g"][b],
                     bounds_gf=out["bounds_gf"] if out["bounds_gf"].ndim == 2 else out["bounds_gf"][b])),
                 **({} if "measured_trajectory" not in out else dict(      # (only a run with measurement noise, likewise: state_trajectory is the truth there)
                     measured_trajectory=out["measured_trajectory"][b], meas_noise=out["meas_noise"] if out["meas_noise"].ndim == 2 else out["meas_noise"][b])))
