/*
 * slsqp.h -- C ABI of the MI355X-native batched fast-SLS QP path (libslsqp_hip.so).
 *
 * Every entry point replaces a call the reference makes on its hot path (citations relative to the
 * reference repository antoineleeman/robust-nonlinear-mpc):
 *
 *   slsqp_create / destroy          fast_SLS.__init__                 solver/fast_SLS_jit.py:202-241
 *                                   (QP._assemble_structures + first OSQP setup, solver/qp_jit.py:77-192, 278-306)
 *   slsqp_set_costs                 OCP.__init__ weights              solver/ocp.py:8-38; SCP_SLS_jit.py:386-388
 *   slsqp_set_constraints           LTV(m,N) G,Gf,gf copies           dyn/LTV.py:17-32
 *   slsqp_update_dynamics           fast_SLS.update_dynamics_list     solver/fast_SLS_jit.py:250-273
 *                                   (QP.update_dynamics :518-576, offset_constraints :595-610)
 *   slsqp_update_linear_cost        fast_SLS.update_linear_cost       solver/fast_SLS_jit.py:575-576
 *   slsqp_solve                     fast_SLS.solve                    solver/fast_SLS_jit.py:278-312
 *   slsqp_get                       post_processing_solution          solver/fast_SLS_jit.py:602-646
 *   slsqp_reset                     reset_solver_to_zeros             solver/fast_SLS_jit.py:424-442
 *   slsqp_qp_update_data_mat/_vec,  module `osqp_generated`           solver/qp_jit.py:671-698 (push), :449-470 (solve)
 *   slsqp_qp_solve                  (update_data_mat / update_data_vec / solve)
 *   slsqp_sweep                     backward_solve + update_tightening kernels  solver/fast_SLS_jit.py:489-571
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures; all arrays are C-contiguous fp64 (int32 for status/iter).
 *   - `loc` says where caller buffers live: SLSQP_HOST (library copies over PCIe) or SLSQP_DEVICE (device
 *     pointers on the handle's GPU, consumed/produced in place on the handle's stream).
 *   - the batch axis B (independent MPC instances) is always the leading axis.
 *   - return value: 0 ok, <0 API misuse / unsupported configuration (message via slsqp_last_error()).
 *     Per-instance outcomes never fail the call: see status[B] (SLSQP_ST_*).
 *   - one handle = one GPU + one HIP stream; distinct handles may be used from distinct threads.
 */
#ifndef SLSQP_H
#define SLSQP_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct slsqp_handle slsqp_handle;

typedef struct {
    int nx, nu, nw; /* state / input / disturbance dims */
    int N;          /* horizon */
    int ni, ni_f;   /* stage / terminal inequality rows; must be 2(nx+nu) and 2nx (G=[I;-I], Gf=[I;-I]) */
} slsqp_dims;

enum { SLSQP_HOST = 0, SLSQP_DEVICE = 1 };

/* per-instance status */
enum {
    SLSQP_ST_SOLVED = 0,      /* KKT certificate met (polished active-set solution) */
    SLSQP_ST_SOLVED_IPM = 4,  /* interior-point tolerance met, polish rejected (solution accurate to opts.eps) */
    SLSQP_ST_MAX_ITER = 1,
    SLSQP_ST_INFEASIBLE = 2,  /* primal infeasible, seen before any work: the pinned x0 lies outside its own stage-0 box */
    SLSQP_ST_NUMERICAL = 3,   /* no finite answer: the interior point's residual went NaN / beyond 1e30, or the instance's data holds a NaN (q, box or
                                 dynamics rows, A, B) or an infinite entry of q, a dynamics row, A or B (checked around every QP launch of slsqp_qp_solve /
                                 slsqp_solve; the closed-loop entry points build their own data and rely on the certificate, which never accepts NaN).
                                 An instance whose x0 is NaN is status 2 */
    SLSQP_ST_INFEASIBLE_CERT = 5 /* primal infeasible, certified by the interior point's multipliers (Farkas ray; the test OSQP applies for the
                                    reference, eps_prim_inf = 1e-4): E'nu + lambda_u - lambda_l ~ 0 with a negative support value */
};

typedef struct {
    int rti_steps;       /* >0: RTI mode, exactly that many fast-SLS steps then one final QP (fast_SLS_jit.py:280-296);
                            <=0: converge mode, up to max_sls_iter steps (:298-312) */
    int max_sls_iter;    /* MAX_ITER (30, fast_SLS_jit.py:206) */
    int qp_max_iter;     /* interior-point iteration cap per QP (default 60) */
    double qp_eps;       /* interior-point residual / complementarity tolerance before the polish (default 1e-6, relative to max(1,|q|inf));
                            if the polish then fails to certify, the interior point resumes down to 1e-9 and the polish is repeated */
    double conv_tol;     /* primal convergence test of check_convergence_socp (1e-3, fast_SLS_jit.py:594) */
    double eps_backoff;  /* epsilon_backoff (1e-10, fast_SLS_jit.py:205) */
    int want_K;          /* accepted and ignored: K (N,N+1,nu,nx) is always kept (the propagation of the sweep reads it back) */
    int warm_start;      /* 1 (default): the first QP of a call first tries an active-set polish from the instance's previous
                            certified solution (KKT-verified, falls back to the interior point); later QPs of a call always do */
    int warm_rounds;     /* active-set correction rounds a warm attempt may use before falling back (default 20) */
    int max_scp_iter;    /* MAX_ITER_SCP (100, SCP_SLS_jit.py:47): cap of the SCP loop of slsqp_cl_step in converge mode (rti <= 0) */
    double scp_eps;      /* epsilon_convergence (1e-10, SCP_SLS_jit.py:29): SCP converged when |delta_vec|inf < scp_eps */
    int precision;       /* 0 (default): fp64 throughout.  1: mixed -- block factorisations, stored inverses and substitutions in fp32,
                            right-hand sides / residuals / KKT certificate in fp64, two more refinement solves per polish; instances
                            that do not certify are solved again in fp64 (BASELINE config 3, "fp32 vs fp64") */
    int as_first;        /* 1: a cold QP solve first runs the active-set iteration from the empty set (round 0 = the equality-constrained
                            optimum), certificate-checked like every polish, and only falls back to the interior point when that fails; a failed warm
                            attempt is followed by that attempt from the empty set too.  2 (default): as 1, but a failed warm attempt goes straight to
                            the interior point (the retry from the empty set rescued 0.08 % of the failed warm attempts where it was measured).
                            0: no active-set attempt before the interior point */
    int as_rounds;       /* correction rounds such an attempt may use (default 24) */
    int as_max_viol;     /* an active-set attempt is abandoned when one of its solves leaves more violated bounds than this (default 64), or more
                            than twice the previous round's + 8: a set that pins both ends of a dynamics row makes the solve blow up */
    int ipm_restart;     /* 1 (default): QPs after the first of a fast-SLS call (same A, B, q, tightened bounds) whose warm active-set attempt
                            fails restart the interior point from a copy of the first QP's iterate at mu ~ 1e-3 |q|inf instead of from scratch */
    int time_kernels;    /* 0 (default): no per-launch timing.  1: HIP event pairs around every launch of the dominant QP kernel on the
                            handle's stream, read with slsqp_kernel_timing (bench.py's roofline leg) */
    int as_warm_max_set; /* 28 (default): the last QP of a call does not start its warm active-set attempt from the first QP's set when that set has more
                            active bounds than this (0 = no limit): it starts from the previous call's last set (as_warm_last) or, without one, the interior point */
    int as_warm_last;    /* 1 (default): where as_warm_max_set rules out the first QP's set (or the first QP left no certified set), the last QP of a call starts
                            from the certified active set of the PREVIOUS call's last QP, moved one stage with the horizon after slsqp_cl_step's shift;
                            2: whenever such a set exists; 0: never */
    int fuse_rti;        /* 1 (default): an RTI solve with rti_steps = 1 in fp64 (the rocket script's setting) of a batch with B (N+1) >= 3072 runs as ONE launch
                            in which every wavefront takes its instance through QP -> eta -> Riccati / propagation -> tightened bounds -> QP (k_rti_chain): no
                            batch-wide barrier behind a QP, so a slow instance only delays itself.  Smaller batches keep the separate launches (their SLS
                            propagation runs N+1 columns of an instance side by side: lower latency).  2: the chain whatever the batch; 0: never.
                            Same arithmetic, same results bit for bit. */
    int cl_persistent;   /* 1 (default): slsqp_cl_run is ONE persistent launch (k_cl_loop): wavefronts take instances from a device-side FIFO and run one
                            whole MPC step each time (shift, linearisation, RTI chain, nominal update, plant), so no wave slot ever waits for a round or
                            for another instance; budget_ms / cut_frac are ignored and *rounds_out = 1.  0: the round-based loop described at
                            slsqp_cl_run.  Same results bit for bit either way. */
} slsqp_opts;
#define SLSQP_X0_BOX_TOL_OSQP_DEFAULT 1e-3

void slsqp_default_opts(slsqp_opts *o);
const char *slsqp_last_error(void);
const char *slsqp_version(void);

slsqp_handle *slsqp_create(const slsqp_dims *d, int batch, int device);
void slsqp_destroy(slsqp_handle *h);

/* Q (nx,nx) R (nu,nu) Qf (nx,nx): must be diagonal (all reference scripts use np.diag); Q_reg/R_reg/Q_reg_f likewise.
   Host pointers. Batch-constant. */
int slsqp_set_costs(slsqp_handle *h, const double *Q, const double *R, const double *Qf, const double *Q_reg,
                    const double *R_reg, const double *Q_reg_f);
/* G (ni,nx+nu), Gf (ni_f,nx), gf (ni_f): host pointers.  G = [I;-I], Gf = [I;-I] (every plant of the reference) enables all entry points;
   any other G / Gf is accepted for the sweep-level boundary (slsqp_sweep) only -- the QP-level entry points then refuse.  gf is the RAW terminal bound that the
   tightened QP uses (fast_SLS_jit.py:524,568). */
int slsqp_set_constraints(slsqp_handle *h, const double *G, const double *Gf, const double *gf);

/* A (B,N,nx,nx)  Bm (B,N,nx,nu)  E (N+1,nx,nw) shared by the batch (NULL keeps the previous one)
   g (B,N,ni) shifted stage bounds g_k = g - G [z_k;v_k];  g_N (B,ni_f) shifted terminal bound gf - Gf z_N
   c (B,N,nx) dynamics offsets c_k = f(z_k,v_k) - z_{k+1}.
   Effect = QP.update_dynamics + offset_constraints: ubg <- [-c_k + eps ; g_k + eps]..., g_N + eps ; lbg <- [-c_k - eps ; -inf]. */
int slsqp_update_dynamics(slsqp_handle *h, const double *A, const double *Bm, const double *E, const double *g,
                          const double *g_N, const double *c, int loc);
int slsqp_update_linear_cost(slsqp_handle *h, const double *q, int loc); /* q (B,n) */

/* x0 (B,nx): the argument of fast_SLS.solve, i.e. x_nom0 - x_meas.  Runs the whole fast-SLS iteration on the GPU. */
int slsqp_solve(slsqp_handle *h, const double *x0, int loc, const slsqp_opts *opts);

/* Fetch a result array by name into `out` (host or device).  Names and shapes (B leading):
   primal_vec (n) dual_vec (m-nx) cost_nominal (1) cost_tube (1; SLS.eval_cost of the last sweep, util/SLS.py:38-46) status[int32] (1) qp_iters[int32] (1) iteration_number[int32] (1)
   beta (N,N,ni) beta_f (N+1,ni_f) backoff (N,ni) backoff_f (ni_f) backoff_x (N+1,nx) backoff_u (N,nu)
   eta (N,N,ni) eta_f (N+1,ni_f) K (N,N+1,nu,nx) ubg (m-nx) lbg (m-nx) kkt (8) pin_dual (nx) success[int32] (1)
   x0_viol (2): largest amount by which the pinned x_0 lay outside its stage-0 box in the instance's last first / last QP (<= 0: inside; +inf: NaN
   state), written for accepted and refused solves alike (slsqp_set_x0_box_tol); a QP the instance took no part in (qp_stats status -1) leaves its entry as it was
   and the current problem data: A (N,nx,nx) Bm (N,nx,nu) c (N,nx) g (N,ni) gN (ni_f) q (n) */
int slsqp_get(slsqp_handle *h, const char *name, void *out, int loc);
/* bytes slsqp_get copies per instance for `name` (the caller's buffer must hold batch x that), or -1 for an unknown name */
long long slsqp_result_bytes(slsqp_handle *h, const char *name);
/* Overwrite a named array: ubg, lbg (QP.update_ubg / reset_lbg, qp_jit.py:578-593, poked by SCP_SLS_jit.py:86-99), q, nominal_x, nominal_u,
   x_meas.  Same shapes as slsqp_get. */
int slsqp_set(slsqp_handle *h, const char *name, const void *src, int loc);
int slsqp_reset(slsqp_handle *h);
/* Tolerance of the measured state against its own stage-0 box, kept by the handle for every following call (slsqp_opts keeps its layout: the value
   is a property of the handle, like the costs).  0 (default): strict -- a QP whose pinned x_0 lies more than 1e-9 outside its own stage-0 box (the rows
   of G [x_0;u_0] <= g that touch the state; the tightened QP moves them inwards by the back-off) ends with SLSQP_ST_INFEASIBLE and no work.  > 0: the
   gate is max(1e-9, tol); INFINITY: the stage-0 state rows never gate (a measured state is data, not a decision variable).  A NaN or infinite state
   is refused whatever the value; a negative or NaN tol is an error.  An accepted solve returns the exact optimum of the QP WITHOUT its stage-0 state
   rows (their multipliers are 0; the stage-0 input rows stay constraints), certified like every other solve; if the rest of the QP is infeasible the
   Farkas test answers (SLSQP_ST_INFEASIBLE_CERT).  Stands for what the reference gets from OSQP at eps_abs = eps_rel = 1e-3 with "solved inaccurate"
   accepted (solver/qp_jit.py:370-400 solve and status check, :537-548 settings): violations below its primal tolerance pass unseen there.
   SLSQP_X0_BOX_TOL_OSQP_DEFAULT lies where that solver accepted every QP measured; its iterate then moves x_0 itself by about
   half the violation, which this library does not imitate.  Applies to every QP of slsqp_solve, slsqp_qp_solve, slsqp_cl_step, slsqp_cl_run and
   slsqp_cl_run_scp; the QPs of slsqp_nominal_solve stay strict (their x_0 deviation is 0 by construction).  The largest violation of each solve can
   be read afterwards: slsqp_get "x0_viol", "log_x0_viol". */
int slsqp_set_x0_box_tol(slsqp_handle *h, double tol);
double slsqp_get_x0_box_tol(slsqp_handle *h);

/* Waves per MPC instance of the QP solves (a property of the handle, like the tolerance above; slsqp_opts keeps its layout).
   1 (default): the single-wave kernels -- one wavefront owns one instance, the right mapping for large batches.
   2, 4, 8: every QP that slsqp_qp_solve, slsqp_solve, slsqp_cl_step and slsqp_nominal_solve run is solved by one workgroup of that many waves
   per instance, the block-tridiagonal system by block cyclic reduction (a dependent chain of log2 N levels instead of N stages): for a caller
   with one plant or a handful.  fp64 only (opts.precision = 1 is refused); the fused RTI chain is not used; slsqp_cl_run and slsqp_cl_run_scp
   (one wave per instance by construction) refuse.  Every answer passes the same KKT certificate as with 1.
   Any other value is an error (< 0, slsqp_last_error) and leaves the setting as it was.  Changing the value makes the next solve of every instance
   factorise afresh (the two paths do not read each other's stored factors); warm-start sets and results stay valid. */
int slsqp_set_solve_waves(slsqp_handle *h, int waves);
int slsqp_get_solve_waves(slsqp_handle *h);

/* Reference trajectory of the closed loop (a property of the handle, like the two settings above; slsqp_opts keeps its layout).
   Xref (T,nx), Uref (T,nu) shared by the batch (per_instance = 0), or (B,T,nx), (B,T,nu) (per_instance = 1); T >= 1; host or device buffers (`loc`),
   copied by the call.  Row t belongs to absolute MPC time t, counted from the slsqp_cl_init that starts a run: at MPC step s (completed steps of the
   instance since slsqp_cl_init) stage k = 0..N of the horizon uses row min(s + k, T - 1) -- the last row is held, T = 1 is a setpoint.  The step's cost is
       sum_k (x_k - xr)'Q(x_k - xr) + (u_k - ur)'R(u_k - ur) + (x_N - xr_N)'Qf(x_N - xr_N),
   i.e. the linear cost of every SCP iteration of the step becomes q = 2 H (y_nom - y_ref window); H, the bounds, c, A, B and the tubes do not depend
   on it.  The reference need not be feasible or dynamically consistent.  Uref = NULL: zero input reference.  Xref = NULL with T = 0 clears the
   reference (the default: q = 2 H y_nom); a zero reference gives the same bits as none.
   Errors (< 0, slsqp_last_error; the previous reference stays in force): T < 0, T = 0 with Xref, T > 0 without, a NaN or infinite entry,
   per_instance outside {0, 1}.
   Reaches every place where the library forms the cost: slsqp_linearize (window of the handle's step count: 0 after slsqp_cl_init, + 1 per
   slsqp_cl_step, + steps per slsqp_cl_run / slsqp_cl_run_scp), slsqp_cl_step, slsqp_cl_run (persistent and round-based: every instance reads the window
   of its own step), slsqp_cl_run_scp, and slsqp_nominal_solve (objective and QPs use the window of step 0, so the first nominal minimises the tracked
   cost).  Survives slsqp_cl_init (which only restarts the step count); may be replaced between runs.  slsqp_update_linear_cost, slsqp_solve and
   slsqp_qp_* bring their own q and are not affected. */
int slsqp_cl_set_reference(slsqp_handle *h, const double *Xref, const double *Uref, int T, int per_instance, int loc);

/* Plant parameters of the closed loop: a true plant that differs from the controller's model (a property of the handle, like the settings above;
   slsqp_opts keeps its layout).  What a user of the reference does by editing `m.params` before the loop of expe/main_*_closed_loop.py -- except
   that there the controller changes with the plant; here ONLY the plant step x_meas <- ddyn_p(x_meas, u0) + E w of slsqp_cl_step, slsqp_cl_run
   (persistent and round-based) and slsqp_cl_run_scp uses the parameters.  The linearisation, the predicted last state of the shifted nominal and
   the nominal initialiser keep the model's constants: controller != plant is the point.
   Parameter vectors, in this order (quadrotor, rocket: the reference's dict order, dyn/quadrotor.py:32-40, dyn/rocket.py:25-39):
       model 0 pendulum   4: m1, m2, l, g
       model 1 quadrotor  7: m, g, l, Jx, Jy, Jz, kM
       model 2 rocket    13: mass, gravity_constant, inertia_xx, inertia_yy, inertia_zz, thrust_cog_offset, thrust_magnitude_time_constant,
                             servo_angle_time_constant, gimbal_a, gimbal_b, gimbal_c, gimbal_d, gimbal_e
   (the rocket's thrust offset 11.3796 is a literal of the reference's ODE, not a parameter: a heavier rocket sags).
   slsqp_plant_param_count: the length for a model id (-1: unknown id).  slsqp_plant_param_name: entry i's name (NULL outside the range).
   slsqp_plant_param_defaults: the model's constants into out[0..count) (len >= count); returns the count, < 0 on error.
   slsqp_cl_set_plant_params: P (np) shared by the batch (per_instance = 0) or (B,np) (per_instance = 1), host or device (`loc`), copied by the call;
   np must be the count of the handle's model; np = 0 with P = NULL clears (the default: the plant is the model).  Survives slsqp_cl_init; may be
   replaced between runs, not during one.  A row holding the defaults bit for bit takes the model's own step: its model_err is exactly 0 (the closed loop then has the bits of no parameters at
   the tested sizes; at rocket B = 4096 rounding-level differences remain).
   Errors (< 0, slsqp_last_error; the previous parameters stay in force): no slsqp_set_model yet, np not the model's count, a NaN or infinite entry, an
   entry <= 0 among the masses, inertias, lengths, time constants, g and the gimbal lengths (everything but the quadrotor's kM), per_instance
   outside {0, 1}.
   Results (slsqp_get): "plant_params" (np) per instance (a shared row repeated; the defaults without parameters); "model_err" (nx):
   ddyn_p(x,u0) - ddyn(x,u0) of the last plant step, before the noise is added (zeros without parameters); "log_model_error" (S,nx) with
   slsqp_cl_log: the same for every MPC step, in the layout of log_state (zeros without parameters). */
int slsqp_plant_param_count(int model_id);
const char *slsqp_plant_param_name(int model_id, int i);
int slsqp_plant_param_defaults(int model_id, double *out, int len);
int slsqp_cl_set_plant_params(slsqp_handle *h, const double *P, int np, int per_instance, int loc);

/* Box bounds over MPC time in the on-device closed loops: a property of the handle (like the reference and the plant parameters: slsqp_opts keeps its
   layout).  slsqp_set_model / slsqp_set_constraints give ONE box for the batch that never changes; this call gives its right-hand sides as rows over
   MPC time, shared by the batch or one set per instance: an actuator limit per vehicle, a corridor along a tracked path, a rate limit that closes in
   near touchdown -- the reference's update_dynamics_list(..., g_list, ...) hook.  G = [I; -I] stays; the rows are in the model's own layout:
       g  (T, ni)   = [hi; -lo] over [x; u]      gf (T, ni_f) = [hi; -lo] over x        (per_instance = 0)
       g  (B,T,ni), gf (B,T,ni_f)                                                      (per_instance = 1)
   host or device (`loc`), copied by the call.  gf = NULL: every terminal row is the model's own gf.  Row t belongs to MPC time t counted from
   slsqp_cl_init: at MPC step s stage k < N uses g row min(s + k, T - 1) and the terminal stage gf row min(s + N, T - 1) -- the last row is held, so
   T = 1 is a constant box (per instance: a parameter study) -- and all SCP iterations of one step use the same window.  What changes: the stage rows
   g_k = g_row - G [x_k; u_k], the terminal row g_N = gf_row - Gf x_N of QP #1, and the terminal row gf_row - backoff_f of the tightened QP (un-shifted,
   as the model's gf is today).  H, q, A, B, c, E, the sweeps and the QP kernels do not see it; the stage-0 gate (slsqp_set_x0_box_tol, "x0_viol")
   reads the stage-0 rows of the step's own window.  Honoured by slsqp_linearize (the handle's step count), slsqp_cl_step, slsqp_cl_run (persistent and
   round-based), slsqp_cl_run_scp and slsqp_nominal_solve (window of step 0); slsqp_solve, slsqp_update_dynamics and slsqp_qp_* bring their own g and
   are not affected.  Survives slsqp_cl_init; may be replaced between runs and between two slsqp_cl_step calls (the setter waits for the handle's stream; the step
   count goes on), not while a call is in flight; T = 0 with g = NULL clears (the default: the model's box,
   and the kernels of a handle that never had bounds).  With gf = NULL the model's gf is read at the call: set the constraints first.
   Errors (< 0, slsqp_last_error; the previous bounds stay in force): no slsqp_set_model yet, a handle with a general G, T < 0, T = 0 with g, T > 0
   without g, per_instance outside {0, 1}, a NaN or -inf entry, a row with hi < lo in any component (g[i] + g[nz+i] < 0, likewise gf).  +inf is
   allowed and is "no bound", exactly as 1e20 is.
   Results (slsqp_get, slsqp_result_bytes): "bounds_g" (T, ni) and "bounds_gf" (T, ni_f) per instance (a shared set repeated; without bounds the model's
   box with T = 1). */
int slsqp_cl_set_bounds(slsqp_handle *h, const double *g, const double *gf, int T, int per_instance, int loc);
int slsqp_sync(slsqp_handle *h);

/* ---- the step in front of the path: batched linearisation (SCP_SLS.update_jacobian, solver/SCP_SLS_jit.py:251-366) ---------
   model_id: 0 pendulum, 1 quadrotor, 2 rocket (ODEs of dyn/{pendulum,quadrotor,rocket}.py, RK4 h=0.05, dyn/model.py:15-34); g_raw (ni): the plant's stage bound g.
   slsqp_linearize: X (B,N+1,nx), U (B,N,nu) nominal trajectories (stage-major) -> A,B (forward-mode AD through RK4),
   c_k = f(x_k,u_k) - x_{k+1}, g_k = g - G[x_k;u_k], g_N = gf - Gf x_N, q = 2 H y_nom (2 H (y_nom - y_ref) with slsqp_cl_set_reference), then the un-tightened bounds; E is untouched
   (set it once with slsqp_update_dynamics or slsqp_set_E). Equivalent to update_dynamics + update_linear_cost. */
int slsqp_set_model(slsqp_handle *h, int model_id, const double *g_raw);
int slsqp_set_E(slsqp_handle *h, const double *E, int loc);   /* E (N+1,nx,nw) */
int slsqp_linearize(slsqp_handle *h, const double *X, const double *U, int loc);

/* ---- the caller after the path: SCP update, warm-start shift, plant step (SCP_SLS.socp_step solver/SCP_SLS_jit.py:404-473,
   reset_warm_start :500-551, expe/main_rocket_robust_closed_loop.py:149-182) -- a whole closed-loop MPC step with no host round trip.
   slsqp_cl_init: x_meas (B,nx); X_nom (B,N+1,nx), U_nom (B,N,nu) initial nominal, or NULL,NULL -> roll-out of the plant from x_meas
   under the constant input u_init (nu) (the reference's IPOPT initialiser is out of scope; pass its result here to reproduce it).
   slsqp_cl_step: rti > 0: exactly rti SCP iterations (scripts: rocket 1, pendulum/quadrotor 3); rti <= 0: SCP_SLS's default
   converge mode (rti = -1, SCP_SLS_jit.py:20-21,113-135): iterate every instance until |delta_vec|inf < opts.scp_eps, at most
   opts.max_scp_iter times; an instance whose fast-SLS step fails leaves the loop (:118-119).  w (B,nx) disturbance sample or NULL.
   Results via slsqp_get: nominal_x (N+1,nx) nominal_u (N,nu) x_meas (nx) u0 (nu) scp_success[int32] (1) scp_iterations[int32] (1)
   scp_delta_max (1) primal_infeasibility (1; max_k,i (ddyn(x_k,u_k) - x_{k+1})_i of the updated nominal, SCP_SLS_jit.py:449-456) + all names of the fast-SLS result (for each instance: of its last fast-SLS solve). */
int slsqp_cl_init(slsqp_handle *h, const double *x_meas, const double *X_nom, const double *U_nom, const double *u_init, int loc);
int slsqp_cl_step(slsqp_handle *h, int rti, const double *w, int loc, const slsqp_opts *opts);
/* One closed-loop step WITHOUT a solve: the plan of the last slsqp_cl_step is held and its tube policy acts on the measured state -- the
   disturbance-feedback gains K[k,j] of the Riccati sweep (Phi_u = K Phi_x, fast_SLS_jit.py:87-117) that the tightened QP assumed along the horizon.
   Hold step k = 1, 2, ... is the k-th plant step since that solve (stage 0 of the plan was pinned to the state measured then); z_k, v_k the plan's
   nominal at stage k, A_j, B_j the handle's linearisation and K what slsqp_get "K" returns, all as they stand after the solve.  Per instance, column
   states xi_j (nx), j = 1..k:
       e     = x_meas - z_k
       xi_j <- (A_{k-1} + B_{k-1} K[k-1,j]) xi_j     1 <= j < k       the plan's prediction of the old columns
       xi_k  = e - sum_{j<k} xi_j                                     what the plan did not predict: disturbance + model defect
       u     = v_k + sum_{1<=j<=k} K[k,j] xi_j
       x_meas <- plant(x_meas, u) + E w                               the plant step of slsqp_cl_step (plant parameters included)
   The call shifts the nominal by one stage (the warm-start shift slsqp_cl_step applies at its top), so afterwards stage 0 of nominal_x / nominal_u is
   z_k, v_k; the nominal is never overwritten with u.  It counts as a closed-loop step: the step count of the reference / bounds windows and the log
   entry advance.  An instance whose last slsqp_cl_step ended with scp_success = 0 has no valid plan: it applies u = v_k (what a failed solved step
   applies), keeps its xi, and reports hold_policy = 0.  The input is not clipped to the box.  k <= N - 1 (K has N rows).  The next slsqp_cl_step
   solves from the held nominal; its QP warm sets move one stage while the horizon moved k + 1 (speed only: every answer is certified).
   w (B,nx) disturbance sample or NULL.
   Errors (< 0, slsqp_last_error; nothing changed): no slsqp_set_model; no slsqp_cl_step since slsqp_cl_init; the hold index would exceed N - 1; a
   slsqp_cl_run / slsqp_cl_run_scp since the last slsqp_cl_step (they leave no per-batch plan); loc outside {SLSQP_HOST, SLSQP_DEVICE}.
   slsqp_cl_init and slsqp_cl_step set the hold index back to 0.
   Results (slsqp_get, slsqp_result_bytes): hold_index[int32] (1) hold steps since the last solve; hold_xi (N+1,nx) row j = xi_j, rows above the index
   zero; hold_policy[int32] (1) of the last hold step: 1 the policy ran, 0 the nominal input was applied; u0, x_meas, model_err as after
   slsqp_cl_step.  With slsqp_cl_log: log_hold[int32] (S) 0 for a solved step, k for hold step k; log_hold_policy[int32] (S); the entry's log_state and
   log_u0 are the measured state and the applied input, log_nominal_* the shifted plan, log_backoff_* and log_success the last solve's,
   log_scp_iterations 0 and log_x0_viol 0.
   The call does not read slsqp_cl_set_solve_every: a step-by-step caller decides itself which of its steps are solves.  The same hold step runs
   inside the persistent launch of slsqp_cl_run for a handle with solve_every > 1 (below); after such a run the call is still refused until a
   slsqp_cl_step. */
int slsqp_cl_hold_step(slsqp_handle *h, const double *w, int loc);
/* M of slsqp_cl_run: the controller of every instance solves at its steps 0, M, 2M, ... and holds its plan at the others (the hold step above).  A
   property of the handle like x0_box_tol (slsqp_opts keeps its layout), default 1 = a solve at every step.  1 <= M <= N; anything else is refused
   (< 0, slsqp_last_error) and changes nothing.  slsqp_cl_step and slsqp_cl_hold_step ignore it. */
int slsqp_cl_set_solve_every(slsqp_handle *h, int M);
int slsqp_cl_get_solve_every(slsqp_handle *h);
/* Event-triggered solves: theta of slsqp_cl_run with M > 1 (persistent launch).  An instance holds its plan while its measured state stays inside the
   fraction theta of the tube that plan computed and solves as soon as it does not, or after M steps at the latest (M is then a cap, not a period).
   A property of the handle, default +INFINITY = off: the fixed period above, the same launch and the same bits.  theta in [0, +INFINITY]; a negative
   or NaN theta is refused (< 0, slsqp_last_error) and changes nothing.  slsqp_cl_step and slsqp_cl_hold_step do not read it; M = 1 ignores it.
   Per instance, about to begin its closed-loop step s >= 1, with k_prev the hold index of step s - 1 (0: a solve), k = k_prev + 1, x = x_meas, z =
   stage 1 of its nominal (z_k of the plan: a hold step shifts before it acts), bo = row k of the last solve's backoff_x, plan_ok = its scp_success:
       r = max_i |x_i - z_i| / bo_i      plain fp64; bo_i = 0: 0 if x_i == z_i, else +inf; a NaN term counts as +inf
       solve_trigger 1  s == 0 or k >= M     a scheduled solve
                     3  !plan_ok             the last solve failed, there is no tube to hold: solve again now
                     2  !(r <= theta)        the state left theta x tube: solve
                     0  otherwise            hold step k
   in this precedence.  With slsqp_cl_log the run fills log_tube_ratio (S): r where it was evaluated (s >= 1 and plan_ok), else 0, and
   log_solve_trigger[int32] (S): the code; both are zeros after every other kind of run.  After an event-triggered run hold_index is per instance. */
int slsqp_cl_set_hold_trigger(slsqp_handle *h, double theta);
double slsqp_cl_get_hold_trigger(slsqp_handle *h);
/* out (B): the tube ratio r above of every instance for the hold step slsqp_cl_hold_step would run next; +INFINITY for an instance without a valid
   plan (scp_success = 0).  For a step-by-step caller that decides itself (for the whole batch) when to solve.  The refusals are those of
   slsqp_cl_hold_step; the call changes nothing in the handle. */
int slsqp_cl_tube_ratio(slsqp_handle *h, double *out, int loc);
/* Plan fallback: what a closed-loop step does when it applies no freshly certified plan.  A property of the handle, default 0 = off: every launch and
   every bit as without the call.  on = 1: per instance a BACKUP of its last plan that succeeded (A, Bm, the compact gains Kc, backoff_x) and plan_age,
   the plant steps since that plan pinned its stage 0 (-1: no backup, the state after slsqp_cl_init; 0 right after a solve with scp_success = 1).
       a solve that succeeds      applies nominal_u[0] as ever; the plan is copied into the backup, plan_age = 0
       a solve that fails, or     k = plan_age + 1.  Backup present and k <= N - 1 (K has N rows): hold step k of the BACKUP -- the formulas of
       a hold step                slsqp_cl_hold_step with the backup's A_{k-1}, B_{k-1}, K[k-1,j], K[k,j]; z_k, v_k are stage 0 of the live nominal (a failed
                                  step leaves the shifted plan untouched); plan_age = k.  Otherwise the nominal input, xi as without the option,
                                  plan_age = -1.
   The schedule (solve_every, hold_trigger, hold_index, the solve_trigger codes) does not change; after a solve that succeeded the backup equals the live
   arrays and plan_age the hold index, so those hold steps keep their bits.  The input is not clipped.  hold_policy / log_hold_policy: 2 on a failed
   solve that ran the backup's policy, 1 on a hold step that ran it, 0 where the nominal input was applied.
   Read by slsqp_cl_step and slsqp_cl_hold_step (one more launch; the hold index of slsqp_cl_hold_step's refusals stays the batch's) and by slsqp_cl_run
   in the persistent launch, M = 1 included.  It needs rti = 1 with one fast-SLS step (the gains are then the compact ones; the full K is not kept):
   slsqp_cl_step and slsqp_cl_run_scp with other settings and the round-based slsqp_cl_run refuse while it is on (< 0, slsqp_last_error).
   Values other than 0 / 1 are refused and change nothing.
   Results (slsqp_get): plan_age[int32] (1), plan_A (N,nx,nx), plan_Bm (N,nx,nu), plan_Kc (N,nu,nx), plan_backoff_x (N+1,nx); with slsqp_cl_log
   log_plan_age[int32] (S): the age every step left behind (zeros from a handle with the option off). */
int slsqp_cl_set_plan_fallback(slsqp_handle *h, int on);
int slsqp_cl_get_plan_fallback(slsqp_handle *h);
/* The whole closed loop with the instances advancing INDEPENDENTLY (rti = 1, one fast-SLS step, fp64, fuse_rti: the rocket script's setting):
   `steps` MPC steps of every instance, W (steps,B,nx) disturbance samples or NULL.  Per instance the same operations in the same order as `steps`
   calls of slsqp_cl_step (identical results), but in rounds: in a round an instance begins its next MPC step or resumes the QP solve that the
   previous round's deadline suspended; a chain still running budget_ms after its launch started (budget_ms <= 0: no time limit), or still running when
   cut_frac of the round's participants have finished (0 < cut_frac < 1; else off), suspends itself and continues in the next round.
   No instance waits for the slowest one of its step.  Call after slsqp_cl_init (+ slsqp_nominal_solve); per-step results through the device-side
   log (slsqp_cl_log with max_steps >= steps, before slsqp_cl_init), `log_qp_stats`[int32] (steps,2,8) and `log_x0_viol` (steps,2), the per-step
   copies of qp_stats and x0_viol (0 where the QP took no part).  *rounds_out (may be NULL): rounds taken.
   With opts.cl_persistent (the default) there are no rounds at all: see slsqp_opts.
   slsqp_cl_set_solve_every with M > 1 (persistent launch only; the round-based loop refuses, as does slsqp_cl_run_scp for any setting but rti = 1 with
   rti_steps = 1): step s of an instance with s % M != 0 is the hold step k = s % M of slsqp_cl_hold_step, run by the wave that holds the instance --
   the same device functions in the same order as that call's launches, same bits as a step-by-step loop of slsqp_cl_step / slsqp_cl_hold_step.  A wave
   that has solved for an instance runs its following hold steps at once, before the instance goes back to the queue.  The entry of `log_qp_stats`
   of a hold step says "took no part": status -1 in both slots, 0 everywhere else.  With slsqp_cl_log the run fills log_hold and log_hold_policy;
   afterwards hold_index, hold_policy, hold_xi and u0 hold the state after the last step.  With M = 1 the call launches exactly what it always did. */
int slsqp_cl_run(slsqp_handle *h, int steps, const double *W, int loc, const slsqp_opts *opts, double budget_ms, double cut_frac, int *rounds_out);
/* `steps` MPC steps of every instance as ONE persistent launch, for any SCP setting of slsqp_cl_step (SCP_SLS.solve, SCP_SLS_jit.py:103-135):
   rti > 0: exactly rti SCP iterations per MPC step; rti <= 0: converge mode (opts.scp_eps, opts.max_scp_iter), every instance leaving the loop at
   its own iteration.  opts.rti_steps >= 1 fast-SLS steps per solve (fast_SLS.solve in RTI mode, fast_SLS_jit.py:278-296; fp64, box constraints,
   fused chain allowed); fast-SLS converge mode (rti_steps <= 0) and precision = 1 are refused.
   Same operations per instance in the same order as `steps` calls of slsqp_cl_step(h, rti, ...): same bits.  rti = 1 with rti_steps = 1 runs
   slsqp_cl_run's persistent kernel.  Results as for slsqp_cl_run: the device-side log, the final state, slsqp_cl_run_stats and `log_qp_stats`
   (steps,2,8), which holds per MPC step what `qp_stats` holds after the corresponding slsqp_cl_step (converge mode: an instance that left the SCP
   loop before the last instance of the batch did has its slots marked "took no part", status -1, as the batch-wide launches leave them). */
int slsqp_cl_run_scp(slsqp_handle *h, int steps, int rti, const double *W, int loc, const slsqp_opts *opts);
/* Fast-SLS converge mode inside slsqp_cl_run_scp's persistent launch.  A property of the handle, default 0 = off: the call refuses opts.rti_steps <= 0
   as above and launches what it always did.  on = 1: slsqp_cl_run_scp accepts opts.rti_steps <= 0, for every rti, with opts.max_sls_iter >= 1 (a
   smaller value is refused), and runs the steps as ONE launch in which every instance iterates fast_SLS.solve's default loop
   (fast_SLS_jit.py:298-312) on its own: QP, eta and the convergence test, then either it leaves (converged: success; its QP failed: not) or it sweeps
   and tightens and goes on, up to max_sls_iter times; an instance that hits the cap solves the last QP and fails, and its solver state is reset at
   the top of its next solve (_finish_failure), as slsqp_cl_step does.  Same operations per instance in the same order as `steps` calls of
   slsqp_cl_step(h, rti, ...) with the same options: same bits, `log_qp_stats` and `log_x0_viol` included (slot 0 of an instance that left a step's
   last solve while another instance of the batch iterated on says "took no part", as the batch-wide launches leave it).  The other refusals of
   slsqp_cl_run_scp stand (precision = 1, general G, solve_waves > 1, the fused chain switched off, solve_every > 1, plan fallback).  With the option
   on and opts.rti_steps >= 1 the call launches exactly what it launches with the option off.  Values other than 0 / 1 are refused and change nothing.
   Result (slsqp_get): log_sls_iterations[int32] (steps), iteration_number as each MPC step of the run left it (the sweeps the step ran); registered
   by every slsqp_cl_run / slsqp_cl_run_scp, zeros from every run but these. */
int slsqp_cl_set_sls_converge(slsqp_handle *h, int on);
int slsqp_cl_get_sls_converge(slsqp_handle *h);
/* State-feedback disturbance adversary of the closed loops.  A property of the handle, default off: every call launches what it always did.  With a
   policy on, the sample w of every plant step x+ = ddyn(x, u0) + E w of slsqp_cl_step, slsqp_cl_hold_step, slsqp_cl_run and slsqp_cl_run_scp is decided
   on the device from the measured state x of the instance at that step (its entry of log_state), per state component i a direction d_i:
     SLSQP_ADV_NEAREST_BOUND     towards the nearer side of the state's box in force at the step -- row min(s, T - 1) of slsqp_cl_set_bounds' table, else
                                 the model's g; d_i = +1 when hi_i - x_i <= x_i - lo_i, else -1; a side that is +inf or >= 1e20 is absent: the other one
                                 pulls, and without either d_i = 0;
     SLSQP_ADV_AWAY_FROM_TARGET  away from what the loop tracks: d_i = +1 if x_i >= xref_i, else -1, xref the state part of row min(s, T - 1) of
                                 slsqp_cl_set_reference's table, or zero.
   A NaN x_i gives d_i = 0.  Channel j gets s_j = sum_i d_i E_ij and w_j = amp sign(s_j) where mask[j] != 0 and s_j != 0; every other channel keeps the
   caller's W_j (0 where the caller passed none).  For a diagonal E: w_j = amp d_j sign(E_jj).  mask (nx) bytes on the host, NULL = every channel.
   amp > 1 is accepted: it is outside the box the tubes were designed for.  policy = SLSQP_ADV_OFF clears the option (amp and mask are not read).
   Refused, with a message that names the argument and the previous setting left in force: an unknown policy; amp NaN, infinite or <= 0; a handle
   without slsqp_set_model; a general G.  The option changes nothing but the sample the plant step reads: a run with the option off and W = the
   applied samples gives the same bits.
   Results (slsqp_get): w_applied (nx), the sample the last plant step used; with slsqp_cl_log, log_w_applied (S,nx), one entry per MPC step (zeros
   while the option is off). */
#define SLSQP_ADV_OFF 0
#define SLSQP_ADV_NEAREST_BOUND 1
#define SLSQP_ADV_AWAY_FROM_TARGET 2
int slsqp_cl_set_adversary(slsqp_handle *h, int policy, double amp, const unsigned char *mask /* (nx) host, NULL = every channel */);
int slsqp_cl_get_adversary(slsqp_handle *h, int *policy, double *amp);
/* Measurement noise of the closed loops.  A property of the handle, default off: every call launches what it always did.  With a table on, the handle
   keeps two states per instance: x_plant (B,nx), the true state -- the plant step x_plant <- ddyn_p(x_plant, u) + E w reads and writes it, the adversary
   reads it (its "entry of log_state" becomes "entry of log_plant_state"), model_err / log_model_error are computed from it -- and x_meas = x_plant + n_s,
   what the controller sees: the pin x_nom0 - x_meas of every solve of the step, the stage-0 gate and x0_viol, the hold policy's e = x_meas - z_k,
   slsqp_cl_tube_ratio and the event trigger, slsqp_nominal_solve's pin and the roll-out of slsqp_cl_init.  One fp64 addition per component.
   n_s is row min(s, T - 1) of Nm, s the MPC step counted from slsqp_cl_init (the instance's own count in slsqp_cl_run / slsqp_cl_run_scp); the last row
   is held, T = 1 is a constant bias.  Nm (T,nx) shared by the batch (per_instance = 0) or (B,T,nx) (per_instance = 1), host or device (`loc`), copied by
   the call: the error itself, in state coordinates.  The measurement of step s + 1 is formed directly behind the plant step of step s (in the
   persistent launches before the event-trigger decision that follows it).  slsqp_cl_init(h, x, ...) takes x as the TRUE state: x_plant <- x,
   x_meas <- x + n_0.
   slsqp_cl_init LATCHES the table in force: a call of this setter between two slsqp_cl_init calls takes effect at the next slsqp_cl_init and changes
   nothing in the loop in progress.  The option survives slsqp_cl_init.  T = 0 with Nm = NULL clears it.
   Refused, with a message that names the argument and the previous table left in force: T < 0; T = 0 with a table; T > 0 without one; a NaN or
   infinite entry; per_instance outside {0,1}; loc outside {SLSQP_HOST, SLSQP_DEVICE}; a handle without slsqp_set_model.
   Results (slsqp_get, slsqp_result_bytes): x_plant (nx), equal to x_meas on a handle with the option off; meas_noise (T,nx) per instance, the latched
   table (a shared one repeated; 0 bytes while off); with slsqp_cl_log: log_plant_state (S,nx), the true state at the top of every step, and
   log_measured_state (S,nx), x_meas at the top of every step, both in the layout of log_state and, with the option off, copies of it.  log_state
   keeps its meaning: the state the step's solve was pinned to (stage 0 of the nominal after the step).  slsqp_set takes "x_plant"; with the option on
   slsqp_set "x_meas" writes the measurement only (with it off both names are the one state). */
int slsqp_cl_set_meas_noise(slsqp_handle *h, const double *Nm, int T, int per_instance, int loc);
/* wave statistics of the last persistent slsqp_cl_run / slsqp_cl_run_scp: [0] wavefronts launched, [1] sum over the MPC steps of the time a wavefront spent on them (ms),
   [2] MPC steps run, [3] duration of the launch (ms, HIP events; 0 without opts.time_kernels).  [1] / ([0] x [3]) = how busy the queue kept the waves. */
#define SLSQP_CL_RUN_STATS_LEN 4
int slsqp_cl_run_stats(slsqp_handle *h, double *out, int len);
/* Device-side log of the closed loop: every following slsqp_cl_step stores what the scripts keep per MPC step
   (expe/main_rocket_robust_closed_loop.py:160-178) in entry `step` of (B, max_steps, ...) device buffers, so a Monte-Carlo run makes no
   host round trip per step.  slsqp_get names (per instance): log_state (S,nx) log_u0 (S,nu) log_nominal_x (S,N+1,nx) log_nominal_u (S,N,nu)
   log_backoff_x (S,N+1,nx) log_backoff_u (S,N,nu) log_success[int32] (S) log_scp_iterations[int32] (S) log_primal_infeasibility (S)
   log_x0_viol (S,2) (x0_viol after the step, 0 where the QP took no part; after a slsqp_cl_run / slsqp_cl_run_scp the name holds that run's (steps,2) instead).
   slsqp_cl_init restarts at entry 0. */
int slsqp_cl_log(slsqp_handle *h, int max_steps);

/* ---- nominal-trajectory initialiser: replaces the reference's IPOPT call for the first MPC step
   (SCP_SLS.solve_nominal_trajectory solver/SCP_SLS_jit.py:161-188, NLP of solver/nlp.py:158-217:
   min sum x'Qx + u'Ru + xN'Qf xN  s.t. x+ = ddyn(x,u), G[x;u] <= g, Gf xN <= gf, x0 = x_meas).
   Improves the nominal held by the handle (slsqp_cl_init: the caller's guess or the roll-out) for every instance by trust-region
   sequential convex programming on the path's own QP kernel, until the step is below tol (default 1e-7) with feasible dynamics and
   box, at most max_qp QP solves (default 120); rho (default 1e3) weighs constraint violation in the merit function.
   Results via slsqp_get: nominal_x, nominal_u, nlp_status[int32] (0 converged to a KKT point, 1 max_qp reached, 2 failed:
   no acceptable step / QP infeasible), nlp_iterations[int32] (accepted steps), nlp_info (12): w, kappa, kappa0, cost, defect l1, box
   violation l1, last ratio, last |step|inf.  IPOPT output is not available offline: parity for this entry point is "unpinned";
   tests certify the NLP's KKT conditions independently. */
int slsqp_nominal_solve(slsqp_handle *h, int max_qp, double tol, double rho, const slsqp_opts *opts);

/* ---- QP-level boundary: mirrors the three calls of the reference's generated module ----------------------- */
/* P_x (B,nnzP): CSC data of triu(2P) (diagonal => nnzP = n);  A_x (B,nnzA): CSC data of the (m x n) constraint
   matrix INCLUDING the x0-pin rows, sorted indices, pattern of qp_jit.py:77-192 with G=[I;-I]. */
int slsqp_qp_nnz(const slsqp_dims *d, int *n, int *m, int *nnzP, int *nnzA);
int slsqp_qp_update_data_mat(slsqp_handle *h, const double *P_x, const double *A_x, int loc);
int slsqp_qp_update_data_vec(slsqp_handle *h, const double *q, const double *l, const double *u, int loc); /* (B,n) (B,m) (B,m) */
/* x (B,n), y (B,m) OSQP sign convention, status (B), iters (B) */
int slsqp_qp_solve(slsqp_handle *h, double *x, double *y, int *status, int *iters, int loc, const slsqp_opts *opts);

/* ---- sweep-level boundary ---------------------------------------------------------------------------------- */
/* eta (B,N,N,ni) eta_f (B,N+1,ni_f) in; K/beta/beta_f/backoff/backoff_f out (any may be NULL). Uses the handle's A,B,E. */
int slsqp_sweep(slsqp_handle *h, const double *eta, const double *eta_f, double *K, double *beta, double *beta_f,
                double *backoff, double *backoff_f, int loc);

/* Both timing queries take the LENGTH of the caller's buffer and refuse (return < 0, nothing written) a buffer shorter than what they
   write: SLSQP_TIMING_LEN / SLSQP_KERNEL_TIMING_LEN doubles.  (Round 2 took bare pointers; a caller that still sized its buffer for four
   values when a fifth was added corrupted its own heap.)  Longer buffers are fine: only the first SLSQP_*_LEN entries are written. */
#define SLSQP_TIMING_LEN 5
#define SLSQP_KERNEL_TIMING_LEN 8
/* elapsed GPU time (ms) of the kernels launched by the last slsqp_solve / slsqp_qp_solve / slsqp_sweep / slsqp_cl_step call,
   measured with HIP events on the handle's stream: [0] total, [1] QP kernel (k_qp_solve), [2] sweep kernels, [3] other,
   [4] linearisation of the last slsqp_cl_step (the reference's t_jac, SCP_SLS_jit.py:268,339-341). */
int slsqp_last_timing(slsqp_handle *h, double *ms, int len);
/* accumulated since the last call (opts.time_kernels = 1 for [0], [1]): [0] total ms of the launches of the dominant QP kernel (k_qp_solve: one
   launch per QP solve) from HIP events around each launch on the handle's stream, [1] number of those launches, [2] instances re-solved in fp64
   after a mixed-precision attempt, and device counters of the work done: [3] instance forward sweeps, [4] how many of them factorised,
   [5] stages factorised (a factorising sweep of an active-set round re-does only the stages from the first changed one on), [6] QP solves that
   ran at least one block solve, [7] block solves that ended after their forward sweep (residual check of an already certified solve: no
   backward sweep); resets the accumulators. */
int slsqp_kernel_timing(slsqp_handle *h, double *out, int len);
void *slsqp_stream(slsqp_handle *h); /* hipStream_t, for callers that share device buffers */
/* Diagnostic: one wavefront runs one of the wave-level building blocks of the kernels (csrc/wave_la.hpp: the MFMA block products, the fused
   product pair of the SLS propagation, the Gauss-Jordan SPD inverse, the D_k assembly) on packed row-major host operands; (nx,nu) = (17,4)
   or (13,4).  Cases and operand order: slsqp_api.hip, k_selftest.  Used by tests/test_gpu_parity.py::test_wave_level_building_blocks. */
int slsqp_selftest(int nx, int nu, int which, const double *in, int n_in, double *out, int n_out);

/* Diagnostic: ONE block solve  Y nu = b  of the solver's normal equations for every instance, on the handle's current A_k, B_k and weights the
   caller gives:  Y = E diag(PI) E' + delta I,  b = E V  (E: the dynamics rows [A_k B_k -I]; no dynamics offsets).
   PI, V: (B,n).  W: (B,N nx) = nu.  G: (B,n) = E' nu.  bmax: (B) max|b| with waves > 1, the largest forward-eliminated entry with waves = 1 (may be NULL).
   fail: (B) 1 = a block was not positive definite (may be NULL).
   waves = 1: the sequential block LDL' sweeps of the single-wave kernels (full factorisation).  2, 4, 8: the block cyclic reduction of the multi-wave kernel.
   factor = 0: substitution only, with the factors the previous factorising call with the same `waves` left; refused when there is none, or when a QP
   solve of the handle ran in between (it overwrites the factor buffers).  update_dynamics must have been called.
   The stored factorisations of the handle's QP solves are discarded (their next solve factorises).  Used by tests/test_gpu_multiwave.py. */
int slsqp_ne_solve(slsqp_handle *h, int waves, int factor, const double *PI, const double *V, double delta, double *W, double *G, double *bmax, int *fail, int loc);

#ifdef __cplusplus
}
#endif
#endif
