// slsqp_api.hip -- C-ABI host side of libslsqp_hip.so (see include/slsqp.h for the contract and the reference
// call sites each entry point replaces).  The fast-SLS control flow of fast_SLS.solve
// (solver/fast_SLS_jit.py:278-327) is run here as a short sequence of batched kernel launches with
// per-instance masks, so one infeasible or converged instance never stalls or fails the batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/slsqp.h"
#include "slsqp_kernels.hpp"
#include "slsqp_mw.hpp"
#include "plant_params.hpp"
#include "cl_bounds.hpp"
#include "cl_hold.hpp"
#include "cl_hold_kernel.hpp"
#include "cl_sls_conv.hpp"

using namespace slsqp;

static thread_local std::string g_err;
static int fail(const std::string &m) { g_err = m; return -1; }
#define HIPCHK(x)                                                                                  \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(e_));         \
    } while (0)

extern "C" const char *slsqp_last_error(void) { return g_err.c_str(); }
extern "C" const char *slsqp_version(void) { return "slsqp-hip 0.1 (gfx950)"; }

extern "C" void slsqp_default_opts(slsqp_opts *o) {
    o->rti_steps = 1; o->max_sls_iter = 30; o->qp_max_iter = 60; o->qp_eps = 1e-6; o->conv_tol = 1e-3;
    o->eps_backoff = 1e-10; o->want_K = 1; o->warm_start = 1; o->warm_rounds = 20;
    o->max_scp_iter = 100; o->scp_eps = 1e-10; o->precision = 0; o->time_kernels = 0; o->as_first = 2; o->as_rounds = 24; o->as_max_viol = 64; o->ipm_restart = 1; o->as_warm_max_set = 28; o->as_warm_last = 1; o->fuse_rti = 1; o->cl_persistent = 1;
}

struct slsqp_handle {
    slsqp_dims d;
    int B, dev, n, m, mb, nz;
    hipStream_t st;
    // problem data
    double *A, *Bm, *E, *g, *gN, *c, *q, *x0val, *gf_raw, *g_raw, *cst;
    int model_id;
    double *Xn, *Un, *xmeas, *x0arg, *u0, *wbuf, *u_init; int cl_steps;  // cst: Qd Rd Qfd Qregd Rregd Qregfd packed
    double *ubg, *lbg;
    // results / state
    double *primal, *dual, *cost, *pin_dual, *kkt, *prev_primal, *Linv, *ws, *qpstate;
    double *eta, *eta_f, *beta, *beta_f, *backoff, *backoff_f, *backoff_x, *backoff_u, *K;
    int *status, *iters, *itnum, *has_prev, *conv, *alive, *mask, *success, *infeas, *counter;
    int *scp_active, *scp_success, *scp_iters, *pending_reset, *scp_upd; double *scp_dmax;
    int horizon_shifted = 0;
    // timeline: event pairs recorded on the stream with a role (0 QP, 1 sweep, 2 whole solve, 3 linearisation, 4 fused RTI chain); read after a synchronisation
    std::vector<hipEvent_t> tl; std::vector<int> tl_role; int tl_n = 0; double tl_acc[5] = {0, 0, 0, 0, 0};     // role 4: fused RTI chain launches (k_rti_chain)
    // slsqp_cl_run: per-instance progress through the closed loop (step counter, suspended-solve state, round masks), per-instance call ids, the launch's
    // start-time word, the per-step copy of qp_stats
    int *cl_stepno = nullptr, *cl_lag = nullptr, *cl_begin = nullptr, *cl_runm = nullptr, *cl_done = nullptr, *cl_skipb = nullptr, *cl_skip_begin = nullptr, *qplog = nullptr;
    double *call_ids = nullptr, *cl_W = nullptr; size_t cl_W_doubles = 0; unsigned long long *t0word = nullptr; int qplog_steps = 0, qplog_cap = 0, *qplog_nsolves = nullptr;      // qplog: capacity in steps, steps of the current run; solves per (instance, step) (k_cl_loop_scp)
    int *clq_slots = nullptr, *clq_ctl = nullptr; unsigned clq_cap = 0; int cl_loop_waves = 0; double cl_loop_ms = 0.0; unsigned long long *cl_busy = nullptr, *cl_tbegin = nullptr, cl_busy_host[16] = {};      // k_cl_loop: instance FIFO (slots; head, tail, avail, err), wave life-time counters
    unsigned char *loop_blk = nullptr; std::vector<unsigned char> loop_blk_host;      // the persistent kernels' argument block (ScpLoopArgs) of this handle and what the host last wrote to it
    bool cl_round = false; unsigned long long cl_budget = 0; int cl_total_steps = 0; unsigned cl_cut_count = 0xFFFFFFFFu;
    unsigned long long *chain_times = nullptr, *chain_times_host = nullptr;   // (B,4) in-kernel wall-clock ticks per instance; pinned copy of instance 0's
    int *qp_diag = nullptr;     // QP_DIAG_SPAN builds only
    double *nom_st; int *nom_need_lin, *nom_status, *nom_iters;
    int *retry; int mx_retry, mx_retry_total;
    int *databad, *runq;        // (B) 1 = the QP data of the instance holds a non-finite value (k_flag_nonfinite); the launch's run mask without those
    double *Kc, *Aclc;          // (B,N,nu,nx), (B,N,nx,nx): K_k and A_k + B_k K_k of the shared Riccati recursion (k_sweep_ric1 -> k_sweep_prop)
    double *lin_stage, *lin_tape;   // (B,N,3,nx) intermediate RK4 stage points of the linearisation (k_lin_val -> k_lin_tan); (B,N,4,NT_MAX) its transcendental values
    double call_id;             // counts fast-SLS calls (validity of the interior-point iterate copies, QpArgs::call_id)
    int *qpstat;                // (B,2,8) per-QP statistics, see QpArgs::qpstat
    double *x0viol;             // (B,2) largest stage-0 violation of the instance's last first / last QP: part of the kkt allocation (x0_record, slsqp_kernels.hpp)
    double x0_box_tol = 0.0;    // slsqp_set_x0_box_tol: the tolerance the following launches ask for
    int solve_every = 1;        // slsqp_cl_set_solve_every: M of slsqp_cl_run -- a solve at steps 0, M, 2M, ... of every instance, hold steps in between (1: a solve at every step)
    double hold_trigger = INFINITY;      // slsqp_cl_set_hold_trigger: theta of slsqp_cl_run with solve_every > 1 -- an instance holds while its tube ratio is <= theta (+inf: off, the fixed period)
    int *hold_k = nullptr, *lg_trig = nullptr; double *lg_ratio = nullptr;      // (B) per-instance hold index of an event-triggered run (ensure_hold); its per-step reason codes and ratios (slsqp_cl_log)
    // slsqp_cl_set_plan_fallback: the backup of every instance's last plan that succeeded, one buffer
    // [A (B,N,nx,nx) | Bm (B,N,nx,nu) | Kc (B,N,nu,nx) | backoff_x (B,N+1,nx)] allocated by the first step that needs it (ensure_plan), its age, the age's log
    int plan_fallback = 0; double *plan_bk = nullptr; int *plan_age = nullptr, *lg_age = nullptr;
    // slsqp_cl_set_sls_converge: slsqp_cl_run_scp takes fast-SLS converge mode (opts.rti_steps <= 0).  sls_itlog: one allocation
    // [log_sls_iterations (B, qplog_cap) | the sweeps of each step's last solve (B, qplog_cap)], made with qplog
    int sls_converge = 0, *sls_itlog = nullptr; std::vector<unsigned char> conv_blk_host;
    int plan_blk_dev = 0; std::vector<unsigned char> plan_blk_host;      // whether the PlanArgs in loop_blk (PLAN_BLK_OFFSET) say "on"; the bytes the host last wrote there
    std::vector<unsigned char> hold_blk_host;    // the HoldLoopArgs the host last wrote behind the ScpLoopArgs of loop_blk (runs with solve_every > 1 only)
    int solve_waves = 1;        // slsqp_set_solve_waves: 1 = the single-wave QP kernels, 2 / 4 / 8 = k_qp_solve_mw (one workgroup of that many waves per instance)
    double *ref_Y = nullptr; int ref_T = 0; size_t ref_stride = 0;      // slsqp_cl_set_reference: packed rows [x_ref; u_ref] (T, nz), per instance with ref_stride = T nz, shared with 0; ref_T = 0: none
    double *zero_ref = nullptr;      // (nz) zeros: the one-row reference the persistent kernels take for a handle with parameters or bounds and no reference (cl_options)
    // slsqp_cl_set_plant_params: one allocation [P (rows, np) | model_err (B, nx)]: parameter rows (pp_stride = np per instance, 0 shared; pp_P NULL: none)
    // and ddyn_p - ddyn of the last plant step
    double *pp_P = nullptr, *pp_merr = nullptr, *lg_merr = nullptr; int pp_np = 0, pp_stride = 0; std::vector<double> pp_host;
    // slsqp_cl_set_bounds: the packed rows (sets, T, ni + ni_f) (bnd_stride = T (ni + ni_f) per instance, 0 shared; bnd_rows NULL: none).  bnd_host: the packed
    // rows on the host (slsqp_get "bounds_g" / "bounds_gf"); g_raw_host / gf_raw_host: the model's box, served where no bounds are set.
    double *bnd_rows = nullptr; int bnd_T = 0; size_t bnd_stride = 0; std::vector<double> bnd_host, g_raw_host, gf_raw_host;
    // slsqp_cl_set_adversary (cl_adversary.hpp): policy (0 = off), amp, the channel mask as a bit set; one allocation made by the
    // first call that switches it on, [the model's plant parameters (np) | model_err (B, nx) | adv_w (B, nx)]: the row of defaults and the model error
    // the persistent kernels' PP variants take for a handle without parameters of its own, and the sample every instance's last plant step used.
    // lg_wadv: its per-step log (part of the slsqp_cl_log buffers).  adv_blk_*: as plan_blk_* for the AdvArgs in loop_blk (ADV_BLK_OFFSET).
    int adv_policy = 0; double adv_amp = 1.0; unsigned adv_mask = 0u; double *adv_buf = nullptr, *adv_merr = nullptr, *adv_w = nullptr, *lg_wadv = nullptr;
    int adv_blk_dev = 0; std::vector<unsigned char> adv_blk_host;
    // slsqp_cl_set_meas_noise (cl_meas.hpp): the table the setter last accepted (mn_next: rows on the device, T = 0: none,
    // stride = T nx per instance or 0 shared, its host copy) and the one slsqp_cl_init latched for the loop in progress (mn); both may name the same
    // buffer.  x_plant (B, nx): the true state, allocated by the first call that sets a table.  lg_plant / lg_meas: the per-step logs of the truth and of
    // the measurement (part of the slsqp_cl_log buffers).  mn_blk_*: as adv_blk_* for the cl_meas::Args in loop_blk (MEAS_BLK_OFFSET).
    struct MeasTab { double *rows = nullptr; int T = 0; size_t stride = 0; std::vector<double> host; } mn, mn_next;
    double *x_plant = nullptr, *lg_plant = nullptr, *lg_meas = nullptr;
    int mn_blk_dev = 0; std::vector<unsigned char> mn_blk_host;
    // slsqp_cl_hold_step: which hold step comes next (cl_hold.hpp) and, allocated by the first hold step, one buffer [xi (B,N+1,nx) | u (B,nu)] of the
    // column states and the applied input, and the per-instance flag "the policy ran"; lg_hold / lg_hpol: their per-step log (part of the slsqp_cl_log buffers)
    cl_hold::State hold; double *hold_xi = nullptr, *hold_u = nullptr; int *hold_policy = nullptr, *lg_hold = nullptr, *lg_hpol = nullptr;
    double *cr = nullptr;       // (B,N,3,nx,nx) scratch of the cyclic reduction (slsqp_mw.hpp), allocated by the first launch that needs it
    int ne_waves = 0;           // slsqp_ne_solve: the path whose factors the last factorising call left (0 = none)
    double x0_tol_dev = 0.0;    // the tolerance of the x0 gate the device currently holds (kkt[8 B]; written when a launch asks for another one)
    double *x0vlog = nullptr;   // (B, qplog_steps, 2) per-step copy of x0viol of a slsqp_cl_run / slsqp_cl_run_scp (allocated with qplog)
    double *lg_x0v = nullptr;   // (B, log_steps, 2) the same for slsqp_cl_step loops (part of the slsqp_cl_log buffers)
    int *stale;                 // (B) bit 0: eta / eta_f, bit 1: K hold values from before the last slsqp_reset (zeroed lazily on slsqp_get)
    double *pinf; double t_jac;  // primal_infeasibility of the last SCP update (SCP_SLS_jit.py:449-456); linearisation time of the last cl_step
    // qp-level CSC maps
    int *mapA, *mapB;  // CSC offsets of A_k[i][j] / B_k[i][j]
    double *stage;     // staging buffer for host<->device transfers
    size_t stage_bytes;
    bool have_costs, have_cons, have_dyn;
    bool beta_inited;           // beta / beta_f have been filled with eps once (k_init_backoff); later solves only repair swept instances (last part of k_after_qp)
    bool general_G;             // G, Gf are not [I;-I]: only the sweep-level boundary (slsqp_sweep) is available
    double *Gd, *Gfd;           // device copies of G (ni, nx+nu) and Gf (ni_f, nx) when general_G
    hipEvent_t ev[10];
    std::vector<hipEvent_t> kev;   // event pairs around every k_qp_solve launch since the last harvest (only with opts.time_kernels)
    int n_kev; bool time_kernels;
    double t_total, t_qp, t_sweep, t_fwd; int n_fwd; double fwd_inst;   // fwd_inst: sum over launches of instances that did work
    std::map<std::string, std::pair<void *, size_t>> named;  // name -> (device ptr, bytes per instance)
    unsigned long long *inst_launches;                       // device counters of k_qp_solve's work (QpArgs::inst_launches; roofline accounting)
    double *ct_part, *cost_tube;                             // sweep's per-column parts of cost_tube^2 and the result
    std::vector<void *> owned, log_owned;                    // device buffers of the handle / of its closed-loop log
    int log_steps;                                           // device-side closed-loop log (slsqp_cl_log): capacity in MPC steps, 0 = off
    double *lg_x, *lg_u, *lg_bx, *lg_bu, *lg_state, *lg_u0, *lg_pinf; int *lg_succ, *lg_it;
};

// The per-handle closed-loop options.  The persistent kernels' variant VAR is a set of these bits; the instantiated sets are
// the five of with_loop_var: an option that needs the tracked cost's code path (parameters, bounds) carries the REF bit, and a handle without a
// reference then passes one row of zeros, which tests/test_gpu_reference.py holds to be the bits of no reference.  HOLD (slsqp_cl_set_solve_every
// with M > 1) comes with REF too and exists for k_cl_loop only: the sets 9, 11, 13, 15.
constexpr int VAR_REF = 1, VAR_PP = 2, VAR_BND = 4, VAR_HOLD = 8;
constexpr bool var_ref(int VAR) { return VAR & VAR_REF; }
constexpr bool var_pp(int VAR) { return VAR & VAR_PP; }
constexpr bool var_bnd(int VAR) { return VAR & VAR_BND; }
constexpr bool var_hold(int VAR) { return VAR & VAR_HOLD; }
// What a handle has set, asked by every launch site: ref / pp / bnd are the handle's own (the flags of the batch-wide kernels: REF and BND of k_lin_vec
// and k_nom_eval, BND of k_tighten and k_rti_chain, pp for the plant step) and own_rf the handle's own reference, empty without one (what those two
// kernels take); var, rf, pa are what the persistent kernels take (rf: own_rf, else the zero row where var has the REF bit, else empty; pa: empty
// without parameters).  hold: the handle's solve_every is above 1 (read by slsqp_cl_run alone: slsqp_cl_step and slsqp_cl_hold_step ignore the setting)
// or plan fallback is on.
// fallback: slsqp_cl_set_plan_fallback is on -- a run-time branch inside the HOLD variants, which a run with M = 1 then launches too.
// adv: slsqp_cl_set_adversary is on -- the stepped paths launch k_cl_adversary with aa in front of their plant launch; the persistent
// kernels branch on the AdvArgs of their block inside the instantiations with the PP bit, so var carries that bit, and a handle without parameters of its
// own passes the model's row of defaults as pa (cl_plant_one's is_model rule: the model's step, a model error of exactly zero).  pp stays the handle's own.
// mn: slsqp_cl_set_meas_noise is on for the loop in progress -- the stepped paths launch k_cl_meas with ma in front of and behind
// their plant launch; the persistent kernels branch on the cl_meas::Args of their block inside the instantiations with the PP bit, as for adv.
struct ClOptions { bool ref, pp, bnd; RefArgs own_rf; int var; RefArgs rf; PlantArgs pa; bool hold; bool fallback; bool adv; cl_adversary::Args aa; bool mn; cl_meas::Args ma; };
// what the two halves of the measurement rule read (no HIP call in here): the latched table, the true state and the logs
static cl_meas::Args meas_args(const slsqp_handle *h) {
    cl_meas::Args A;
    memset(&A, 0, sizeof A);
    A.rows = h->mn.rows; A.T = h->mn.T; A.stride = h->mn.stride; A.x_plant = h->x_plant;
    if (h->log_steps > 0) { A.S = h->log_steps; A.lg_plant = h->lg_plant; A.lg_meas = h->lg_meas; }
    return A;
}
// what the adversary reads at the plant step (no HIP call in here): the bounds in force -- the handle's table, or the model's g as one shared row --
// and the reference, or one shared row of zeros
static cl_adversary::Args adv_args(const slsqp_handle *h) {
    cl_adversary::Args A;
    memset(&A, 0, sizeof A);
    A.policy = h->adv_policy; A.nz = h->d.nx + h->d.nu; A.mask = h->adv_mask; A.amp = h->adv_amp;
    A.adv_w = h->adv_w; A.lg = h->log_steps > 0 ? h->lg_wadv : nullptr; A.S = h->log_steps;
    if (h->bnd_rows) { A.bd.rows = h->bnd_rows; A.bd.T = h->bnd_T; A.bd.stride = h->bnd_stride; A.bdW = h->d.ni + h->d.ni_f; }
    else { A.bd.rows = h->g_raw; A.bd.T = 1; A.bd.stride = 0; A.bdW = h->d.ni; }
    if (h->ref_T > 0) { A.rf.rows = h->ref_Y; A.rf.T = h->ref_T; A.rf.stride = h->ref_stride; }
    else { A.rf.rows = h->zero_ref; A.rf.T = 1; A.rf.stride = 0; }
    return A;
}
static ClOptions cl_options(const slsqp_handle *h) {
    ClOptions o{};
    o.ref = h->ref_T > 0; o.pp = h->pp_P != nullptr; o.bnd = h->bnd_rows != nullptr;
    o.fallback = h->plan_fallback != 0;
    o.hold = h->solve_every > 1 || o.fallback;
    o.adv = h->adv_policy != cl_adversary::OFF;
    o.mn = h->mn.T > 0;
    const bool ppk = o.pp || o.adv || o.mn;      // the PP bit of the persistent kernels
    o.var = ((o.ref || ppk || o.bnd || o.hold) ? VAR_REF : 0) | (ppk ? VAR_PP : 0) | (o.bnd ? VAR_BND : 0) | (o.hold ? VAR_HOLD : 0);
    if (o.ref) o.own_rf = RefArgs{h->ref_Y, h->ref_T, h->ref_stride};
    o.rf = (o.var && !o.ref) ? RefArgs{h->zero_ref, 1, 0} : o.own_rf;
    if (o.pp) o.pa = PlantArgs{h->pp_P, h->pp_stride, h->pp_merr, h->log_steps > 0 ? h->lg_merr : nullptr, h->log_steps};
    else if (o.adv || o.mn) o.pa = PlantArgs{h->adv_buf, 0, h->adv_merr, h->log_steps > 0 ? h->lg_merr : nullptr, h->log_steps};
    if (o.adv) o.aa = adv_args(h);
    if (o.mn) o.ma = meas_args(h);
    return o;
}
// the bounds' table (empty without bounds) and the MPC step whose window a batch-wide launch reads, of the reference too: `step`, or stepno[b]
static BndArgs bnd_args(const slsqp_handle *h, int step, const int *stepno) { return BndArgs{{h->bnd_rows, h->bnd_T, h->bnd_stride}, stepno, step}; }
// A run-time choice among three as a template argument: f(std::integral_constant<int, i>) for i in 0..2, false for any other i.  f is a generic
// lambda and names the constant as M() / V(); an instantiation that is missing stops the build.
template <class F>
static bool dispatch3(int i, F &&f) {
    switch (i) {
    case 0: f(std::integral_constant<int, 0>{}); return true;
    case 1: f(std::integral_constant<int, 1>{}); return true;
    case 2: f(std::integral_constant<int, 2>{}); return true;
    }
    return false;
}
// the same among the instantiated variants of the persistent kernels; hold_sets: those of k_cl_loop alone as well (f then guards what it
// instantiates with var_hold(V()))
template <class F>
static bool with_loop_var(int var, F &&f, bool hold_sets = false) {
    if (hold_sets) switch (var) {
    case VAR_HOLD | VAR_REF: f(std::integral_constant<int, VAR_HOLD | VAR_REF>{}); return true;
    case VAR_HOLD | VAR_REF | VAR_PP: f(std::integral_constant<int, VAR_HOLD | VAR_REF | VAR_PP>{}); return true;
    case VAR_HOLD | VAR_REF | VAR_BND: f(std::integral_constant<int, VAR_HOLD | VAR_REF | VAR_BND>{}); return true;
    case VAR_HOLD | VAR_REF | VAR_PP | VAR_BND: f(std::integral_constant<int, VAR_HOLD | VAR_REF | VAR_PP | VAR_BND>{}); return true;
    }
    switch (var) {
    case 0: f(std::integral_constant<int, 0>{}); return true;
    case VAR_REF: f(std::integral_constant<int, VAR_REF>{}); return true;
    case VAR_REF | VAR_PP: f(std::integral_constant<int, VAR_REF | VAR_PP>{}); return true;
    case VAR_REF | VAR_BND: f(std::integral_constant<int, VAR_REF | VAR_BND>{}); return true;
    case VAR_REF | VAR_PP | VAR_BND: f(std::integral_constant<int, VAR_REF | VAR_PP | VAR_BND>{}); return true;
    }
    return false;
}
// a flag as a template argument: f(std::true_type / std::false_type), named B() in the generic lambda
template <class F>
static void with_flag(bool on, F &&f) { if (on) f(std::true_type{}); else f(std::false_type{}); }
// the handle's own (REF, BND), for k_lin_vec and k_nom_eval
template <class F>
static void with_ref_bnd(const ClOptions &op, F &&f) { with_flag(op.ref, [&](auto REF) { with_flag(op.bnd, [&](auto BND) { f(REF, BND); }); }); }
// the handle's plant model (0 pendulum, 1 quadrotor, 2 rocket): every launch of a kernel that is a template of the model goes through here
template <class F>
static int with_model(const slsqp_handle *h, F &&f) {
    return dispatch3(h->model_id, f) ? 0 : fail("no kernels for model id " + std::to_string(h->model_id) + " (0 pendulum, 1 quadrotor, 2 rocket)");
}

template <typename T>
static int dalloc(std::vector<void *> &owned, T **p, size_t count) {
    *p = nullptr;
    HIPCHK(hipMalloc((void **)p, count * sizeof(T) + 64));
    owned.push_back((void *)*p);
    HIPCHK(hipMemset(*p, 0, count * sizeof(T)));
    return 0;
}
static void free_all(std::vector<void *> &owned) { for (void *p : owned) if (p) hipFree(p); owned.clear(); }
// The device buffer of a per-handle closed-loop option (slsqp_cl_set_reference / _plant_params / _bounds), one path for all of them.
// opt_install: a new buffer of `up` followed by n_zero zeros; only when it is complete the previous buffer is freed and *slot (and *keep, the host
// copy a getter serves, where given) replaced -- on failure both stay as they were.  opt_clear: no buffer.  opt_fetch: the caller's array to the host.
static int opt_install(const char *who, double **slot, std::vector<double> &up, size_t n_zero = 0, std::vector<double> *keep = nullptr) {
    double *buf = nullptr;
    HIPCHK(hipMalloc((void **)&buf, sizeof(double) * (up.size() + n_zero) + 64));
    if ((n_zero && hipMemset(buf, 0, sizeof(double) * (up.size() + n_zero)) != hipSuccess) || hipMemcpy(buf, up.data(), sizeof(double) * up.size(), hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(buf);
        return fail(std::string(who) + ": upload failed");
    }
    if (*slot) hipFree(*slot);
    *slot = buf;
    if (keep) keep->swap(up);
    return 0;
}
static void opt_clear(double **slot, std::vector<double> *keep = nullptr) {
    if (*slot) hipFree(*slot);
    *slot = nullptr;
    if (keep) keep->clear();
}
static int opt_fetch(std::vector<double> &dst, const double *src, int loc) {
    HIPCHK(hipMemcpy(dst.data(), src, sizeof(double) * dst.size(), loc == SLSQP_HOST ? hipMemcpyHostToHost : hipMemcpyDeviceToHost));
    return 0;
}

// (nx, nu) pairs the QP / sweep kernels are instantiated for: the reference's three plants, plus whatever the build adds with
//   -DSLSQP_EXTRA_DIMS="X(6,2) X(9,3)"      (limits of the single-wave kernels: nx <= 17, nu <= 4, nx + nu <= 21)
// The plant-specific entry points (slsqp_set_model / slsqp_linearize / slsqp_cl_*) exist for the three plants only.
#ifndef SLSQP_EXTRA_DIMS
#define SLSQP_EXTRA_DIMS
#endif
#define SLSQP_DIM_LIST X(4, 1) X(13, 4) X(17, 4) SLSQP_EXTRA_DIMS
static bool supported_dims(int nx, int nu) {
#define X(NX_, NU_) if (nx == NX_ && nu == NU_) return true;
    SLSQP_DIM_LIST
#undef X
    return false;
}
static std::string dims_list() {
    std::string r;
#define X(NX_, NU_) r += " (" #NX_ "," #NU_ ")";
    SLSQP_DIM_LIST
#undef X
    return r;
}
// the (nx, nu) pair as template arguments, as with_model gives the plant: every launch of a kernel that is a template of the pair goes through here.
// f(std::integral_constant<int, NX>, std::integral_constant<int, NU>), NX() / NU() in the generic lambda, returns an int; no such pair in the build is an error that says so
template <class F>
static int with_dims(int nx, int nu, F &&f) {
#define X(NX_, NU_) if (nx == NX_ && nu == NU_) return f(std::integral_constant<int, NX_>{}, std::integral_constant<int, NU_>{});
    SLSQP_DIM_LIST
#undef X
    return fail("no kernels for (nx, nu) = (" + std::to_string(nx) + "," + std::to_string(nu) + "); built for" + dims_list());
}
template <class F>
static int with_dims(const slsqp_handle *h, F &&f) { return with_dims(h->d.nx, h->d.nu, f); }

extern "C" int slsqp_qp_nnz(const slsqp_dims *d, int *n, int *m, int *nnzP, int *nnzA) {
    const int nz = d->nx + d->nu;
    *n = nz * d->N + d->nx;
    *m = d->N * (d->nx + d->ni) + d->ni_f + d->nx;
    *nnzP = *n;
    *nnzA = d->N * (d->nx * (nz + 1) + 2 * nz) + 3 * d->nx;
    return 0;
}

extern "C" slsqp_handle *slsqp_create(const slsqp_dims *d, int batch, int device) {
    if (!supported_dims(d->nx, d->nu)) { fail("unsupported (nx,nu): this build instantiates the kernels for" + dims_list() + " (add pairs with -DSLSQP_EXTRA_DIMS)"); return nullptr; }
    if (d->ni < 1 || d->ni_f < 1 || d->ni > 4096 || d->ni_f > 4096) { fail("need 1 <= ni, ni_f <= 4096"); return nullptr; }
    if (d->nw < 1 || d->nw > d->nx) { fail("need 1 <= nw <= nx (E is kept zero-padded to nx columns: the padding adds nothing to any row norm of Phi)"); return nullptr; }
    if (d->N < 1 || d->N > 64 || batch < 1) { fail("need 1 <= N <= 64 and batch >= 1"); return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { fail("no HIP device visible: libslsqp_hip has no CPU fallback"); return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { fail("hipSetDevice failed"); return nullptr; }
    slsqp_handle *h = new slsqp_handle();
    h->d = *d; h->B = batch; h->dev = device;
    const int nx = d->nx, nu = d->nu, N = d->N, ni = d->ni, nif = d->ni_f, nw = d->nw;
    h->nz = nx + nu; h->n = h->nz * N + nx; h->mb = N * (nx + ni) + nif; h->m = h->mb + nx;
    const size_t B = batch;
    if (hipStreamCreate(&h->st) != hipSuccess) { fail("hipStreamCreate"); delete h; return nullptr; }
    int rc = 0;
    rc |= dalloc(h->owned, &h->A, B * N * nx * nx); rc |= dalloc(h->owned, &h->Bm, B * N * nx * nu); rc |= dalloc(h->owned, &h->E, (size_t)(N + 1) * nx * nx);     // (N+1, nx, nx): E (N+1, nx, nw) zero-padded to nx columns
    (void)nw;
    rc |= dalloc(h->owned, &h->g, B * N * ni); rc |= dalloc(h->owned, &h->gN, B * nif); rc |= dalloc(h->owned, &h->c, B * N * nx); rc |= dalloc(h->owned, &h->q, B * h->n);
    rc |= dalloc(h->owned, &h->x0val, B * nx); rc |= dalloc(h->owned, &h->gf_raw, (size_t)nif); rc |= dalloc(h->owned, &h->g_raw, (size_t)ni);
    rc |= dalloc(h->owned, &h->Xn, B * (N + 1) * nx); rc |= dalloc(h->owned, &h->Un, B * N * nu); rc |= dalloc(h->owned, &h->xmeas, B * nx); rc |= dalloc(h->owned, &h->x0arg, B * nx);
    rc |= dalloc(h->owned, &h->u0, B * nu); rc |= dalloc(h->owned, &h->wbuf, B * nx); rc |= dalloc(h->owned, &h->u_init, (size_t)nu); rc |= dalloc(h->owned, &h->zero_ref, (size_t)(nx + nu)); h->cl_steps = 0; rc |= dalloc(h->owned, &h->cst, (size_t)(3 * nx + 2 * nu) * 2);
    rc |= dalloc(h->owned, &h->ubg, B * h->mb); rc |= dalloc(h->owned, &h->lbg, B * h->mb);
    rc |= dalloc(h->owned, &h->primal, B * h->n); rc |= dalloc(h->owned, &h->dual, B * h->mb); rc |= dalloc(h->owned, &h->cost, B); rc |= dalloc(h->owned, &h->pin_dual, B * nx);
    rc |= dalloc(h->owned, &h->kkt, kkt_doubles(B)); rc |= dalloc(h->owned, &h->prev_primal, B * h->n); rc |= dalloc(h->owned, &h->Linv, B * N * nx * nx); rc |= dalloc(h->owned, &h->ws, B * qp_ws_doubles(h->n, N, nx)); rc |= dalloc(h->owned, &h->qpstate, B * 40);
    rc |= dalloc(h->owned, &h->eta, B * N * N * ni); rc |= dalloc(h->owned, &h->eta_f, B * (N + 1) * nif); rc |= dalloc(h->owned, &h->beta, B * N * N * ni);
    rc |= dalloc(h->owned, &h->beta_f, B * (N + 1) * nif); rc |= dalloc(h->owned, &h->backoff, B * N * ni); rc |= dalloc(h->owned, &h->backoff_f, B * nif);
    rc |= dalloc(h->owned, &h->backoff_x, B * (N + 1) * nx); rc |= dalloc(h->owned, &h->backoff_u, B * N * nu); rc |= dalloc(h->owned, &h->K, B * N * (N + 1) * nu * nx);
    rc |= dalloc(h->owned, &h->status, B); rc |= dalloc(h->owned, &h->iters, B); rc |= dalloc(h->owned, &h->itnum, B); rc |= dalloc(h->owned, &h->has_prev, B); rc |= dalloc(h->owned, &h->conv, B);
    rc |= dalloc(h->owned, &h->alive, B); rc |= dalloc(h->owned, &h->mask, B); rc |= dalloc(h->owned, &h->success, B); rc |= dalloc(h->owned, &h->infeas, B); rc |= dalloc(h->owned, &h->counter, (size_t)4);
    rc |= dalloc(h->owned, &h->scp_active, B); rc |= dalloc(h->owned, &h->scp_success, B); rc |= dalloc(h->owned, &h->scp_iters, B); rc |= dalloc(h->owned, &h->pending_reset, B); rc |= dalloc(h->owned, &h->scp_dmax, B);
    rc |= dalloc(h->owned, &h->retry, B); h->mx_retry = 0; h->mx_retry_total = 0; rc |= dalloc(h->owned, &h->databad, B); rc |= dalloc(h->owned, &h->runq, B);
    rc |= dalloc(h->owned, &h->nom_st, B * 12); rc |= dalloc(h->owned, &h->nom_need_lin, B); rc |= dalloc(h->owned, &h->nom_status, B); rc |= dalloc(h->owned, &h->nom_iters, B);
    rc |= dalloc(h->owned, &h->mapA, (size_t)N * nx * nx); rc |= dalloc(h->owned, &h->mapB, (size_t)N * nx * nu);
    rc |= dalloc(h->owned, &h->inst_launches, (size_t)8); rc |= dalloc(h->owned, &h->chain_times, B * 4);
    rc |= dalloc(h->owned, &h->cl_stepno, B); rc |= dalloc(h->owned, &h->cl_lag, B); rc |= dalloc(h->owned, &h->cl_begin, B); rc |= dalloc(h->owned, &h->cl_runm, B); rc |= dalloc(h->owned, &h->cl_done, B);
    { unsigned cap = 1; while (cap < 4u * (unsigned)B) cap <<= 1; h->clq_cap = cap; rc |= dalloc(h->owned, &h->clq_slots, (size_t)cap); rc |= dalloc(h->owned, &h->clq_ctl, (size_t)8); rc |= dalloc(h->owned, &h->cl_busy, (size_t)16); rc |= dalloc(h->owned, &h->cl_tbegin, (size_t)B); rc |= dalloc(h->owned, &h->loop_blk, (size_t)4096); }
    rc |= dalloc(h->owned, &h->cl_skipb, B); rc |= dalloc(h->owned, &h->call_ids, B); rc |= dalloc(h->owned, &h->t0word, (size_t)2); rc |= dalloc(h->owned, &h->ct_part, B * (N + 1)); rc |= dalloc(h->owned, &h->cost_tube, B);
    rc |= dalloc(h->owned, &h->lin_stage, B * N * 3 * nx); rc |= dalloc(h->owned, &h->lin_tape, B * N * 4 * dyn::NT_MAX); rc |= dalloc(h->owned, &h->Kc, B * N * nu * nx); rc |= dalloc(h->owned, &h->Aclc, B * N * nx * nx); rc |= dalloc(h->owned, &h->qpstat, B * 16); rc |= dalloc(h->owned, &h->Gd, (size_t)ni * (nx + nu)); rc |= dalloc(h->owned, &h->Gfd, (size_t)nif * nx); h->general_G = false; h->beta_inited = false; rc |= dalloc(h->owned, &h->stale, B); rc |= dalloc(h->owned, &h->pinf, B); rc |= dalloc(h->owned, &h->scp_upd, B); h->t_jac = 0;
    h->log_steps = 0; h->lg_x = h->lg_u = h->lg_bx = h->lg_bu = h->lg_state = h->lg_u0 = h->lg_pinf = nullptr; h->lg_succ = h->lg_it = nullptr;
    if (rc) { free_all(h->owned); hipStreamDestroy(h->st); delete h; return nullptr; }
    if (hipHostMalloc((void **)&h->chain_times_host, 4 * sizeof(unsigned long long)) != hipSuccess) h->chain_times_host = nullptr;
    else memset(h->chain_times_host, 0, 4 * sizeof(unsigned long long));
    for (auto &e : h->ev) hipEventCreate(&e);
    h->tl.resize(2 * 256); for (auto &e : h->tl) hipEventCreate(&e);
    h->tl_role.assign(256, 0); h->tl_n = 0;
    h->kev.resize(2 * 256); for (auto &e : h->kev) hipEventCreate(&e);
    h->n_kev = 0; h->t_fwd = 0; h->n_fwd = 0; h->fwd_inst = 0; h->time_kernels = false; h->call_id = 0;
    // CSC offsets of the reference's frozen pattern (qp_jit.py:101-123,178-186; columns sorted by row)
    {
        std::vector<int> mA((size_t)N * nx * nx), mB((size_t)N * nx * nu);
        int p = 0;
        for (int k = 0; k <= N; k++) {
            for (int j = 0; j < nx; j++) {      // column of x_k[j]
                if (k >= 1) p += 1;              // -I entry in dynamics row block k-1
                if (k < N) { for (int i = 0; i < nx; i++) mA[((size_t)k * nx + i) * nx + j] = p + i; p += nx; p += 2; }
                else p += 2;                     // terminal +1 / -1
                if (k == 0) p += 1;              // x0 pin row (last rows of the matrix)
            }
            if (k < N)
                for (int a = 0; a < nu; a++) {   // column of u_k[a]
                    for (int i = 0; i < nx; i++) mB[((size_t)k * nx + i) * nu + a] = p + i;
                    p += nx; p += 2;
                }
        }
        hipMemcpyAsync(h->mapA, mA.data(), mA.size() * sizeof(int), hipMemcpyHostToDevice, h->st);
        hipMemcpyAsync(h->mapB, mB.data(), mB.size() * sizeof(int), hipMemcpyHostToDevice, h->st);
        hipStreamSynchronize(h->st);
    }
    h->stage = nullptr; h->stage_bytes = 0;
    h->have_costs = h->have_cons = h->have_dyn = false; h->model_id = -1;
    h->t_total = h->t_qp = h->t_sweep = 0;
    auto reg = [&](const char *nm, void *p, size_t bytes) { h->named[nm] = {p, bytes}; };
    reg("primal_vec", h->primal, sizeof(double) * h->n); reg("dual_vec", h->dual, sizeof(double) * h->mb); reg("cost_nominal", h->cost, sizeof(double));
    reg("status", h->status, sizeof(int)); reg("qp_iters", h->iters, sizeof(int)); reg("iteration_number", h->itnum, sizeof(int));
    reg("success", h->success, sizeof(int)); reg("scp_success", h->scp_success, sizeof(int)); reg("scp_iterations", h->scp_iters, sizeof(int));
    reg("scp_delta_max", h->scp_dmax, sizeof(double));
    reg("nlp_status", h->nom_status, sizeof(int)); reg("nlp_iterations", h->nom_iters, sizeof(int)); reg("nlp_info", h->nom_st, sizeof(double) * 12);
    reg("beta", h->beta, sizeof(double) * N * N * ni); reg("beta_f", h->beta_f, sizeof(double) * (N + 1) * nif);
    reg("backoff", h->backoff, sizeof(double) * N * ni); reg("backoff_f", h->backoff_f, sizeof(double) * nif);
    reg("backoff_x", h->backoff_x, sizeof(double) * (N + 1) * nx); reg("backoff_u", h->backoff_u, sizeof(double) * N * nu);
    reg("eta", h->eta, sizeof(double) * N * N * ni); reg("eta_f", h->eta_f, sizeof(double) * (N + 1) * nif);
    reg("K", h->K, sizeof(double) * N * (N + 1) * nu * nx); reg("ubg", h->ubg, sizeof(double) * h->mb); reg("lbg", h->lbg, sizeof(double) * h->mb);
    reg("kkt", h->kkt, sizeof(double) * 8); reg("cost_tube", h->cost_tube, sizeof(double));
    reg("nominal_x", h->Xn, sizeof(double) * (N + 1) * nx); reg("nominal_u", h->Un, sizeof(double) * N * nu); reg("x_meas", h->xmeas, sizeof(double) * nx); reg("u0", h->u0, sizeof(double) * nu);
    reg("Kc", h->Kc, sizeof(double) * N * nu * nx);      // the compact gains of the shared Riccati recursion (K[k,j] = Kc[k], j <= k, where stale has bit 32)
    reg("A", h->A, sizeof(double) * N * nx * nx); reg("Bm", h->Bm, sizeof(double) * N * nx * nu); reg("c", h->c, sizeof(double) * N * nx);
    reg("g", h->g, sizeof(double) * N * ni); reg("gN", h->gN, sizeof(double) * nif); reg("q", h->q, sizeof(double) * h->n); reg("pin_dual", h->pin_dual, sizeof(double) * nx);
    reg("chain_times", h->chain_times, sizeof(unsigned long long) * 4); reg("primal_infeasibility", h->pinf, sizeof(double)); reg("qp_stats", h->qpstat, sizeof(int) * 16); h->x0viol = x0_record(h->kkt, h->B) + 2; reg("x0_viol", h->x0viol, sizeof(double) * 2); reg("x0_arg", h->x0arg, sizeof(double) * nx);
#ifdef QP_DIAG_SPAN
    if (dalloc(h->owned, &h->qp_diag, B * 64)) return nullptr;
    reg("qp_diag", h->qp_diag, sizeof(int) * 64);
#endif
    return h;
}

extern "C" void slsqp_destroy(slsqp_handle *h) {
    if (!h) return;
    hipSetDevice(h->dev);
    hipStreamSynchronize(h->st);
    free_all(h->log_owned);
    free_all(h->owned);
    if (h->stage) hipFree(h->stage);
    if (h->cl_W) hipFree(h->cl_W);
    opt_clear(&h->ref_Y); opt_clear(&h->pp_P); opt_clear(&h->bnd_rows); opt_clear(&h->adv_buf);
    if (h->mn_next.rows && h->mn_next.rows != h->mn.rows) hipFree(h->mn_next.rows);
    if (h->mn.rows) hipFree(h->mn.rows);
    if (h->x_plant) hipFree(h->x_plant);
    if (h->hold_xi) hipFree(h->hold_xi);
    if (h->hold_policy) hipFree(h->hold_policy);
    if (h->plan_bk) hipFree(h->plan_bk);
    if (h->plan_age) hipFree(h->plan_age);
    if (h->qplog) hipFree(h->qplog);
    if (h->x0vlog) hipFree(h->x0vlog);
    if (h->qplog_nsolves) hipFree(h->qplog_nsolves);
    if (h->sls_itlog) hipFree(h->sls_itlog);
    if (h->chain_times_host) hipHostFree(h->chain_times_host);
    for (auto &e : h->ev) hipEventDestroy(e);
    for (auto &e : h->tl) hipEventDestroy(e);
    for (auto &e : h->kev) hipEventDestroy(e);
    hipStreamDestroy(h->st);
    delete h;
}

extern "C" void *slsqp_stream(slsqp_handle *h) { return (void *)h->st; }
extern "C" int slsqp_sync(slsqp_handle *h) { hipSetDevice(h->dev); HIPCHK(hipStreamSynchronize(h->st)); return 0; }

static int put(slsqp_handle *h, void *dst, const void *src, size_t bytes, int loc) {
    if (!src) return 0;
    HIPCHK(hipMemcpyAsync(dst, src, bytes, loc == SLSQP_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, h->st));
    if (loc == SLSQP_HOST) HIPCHK(hipStreamSynchronize(h->st));  // caller's buffer may be reused on return
    return 0;
}

// Device staging area for host-buffer (SLSQP_HOST) entry points: grown on demand, reused, filled with async copies on the handle's stream --
// no hipMalloc / null-stream hipMemcpy per call (those serialise against every other handle's stream).
static double *stage_buf(slsqp_handle *h, size_t bytes) {
    if (bytes > h->stage_bytes) {
        hipStreamSynchronize(h->st);
        if (h->stage) { hipFree(h->stage); h->stage = nullptr; h->stage_bytes = 0; }
        if (hipMalloc((void **)&h->stage, bytes + 64) != hipSuccess) { h->stage = nullptr; fail("hipMalloc (staging buffer)"); return nullptr; }
        h->stage_bytes = bytes;
    }
    return h->stage;
}

// E (N+1, nx, nw), nw <= nx, into the handle's (N+1, nx, nx) buffer: Phi_x[j,j] = E_j (fast_SLS_jit.py:104-108) with nw < nx (dyn/LTV.py:17-32
// allows any nw) propagates as an nx x nx block whose last nx - nw columns are and stay zero -- every row norm, hence beta, the back-offs and
// cost_tube, is the one of the nx x nw block.
__global__ void k_pad_cols(int rows, int nw, int nx, const double *src, double *dst) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rows * nx; i += gridDim.x * blockDim.x) { const int r = i / nx, c = i % nx; dst[i] = c < nw ? src[r * nw + c] : 0.0; }
}
static int put_E(slsqp_handle *h, const double *E, int loc) {
    if (!E) return 0;
    const slsqp_dims &d = h->d;
    const size_t rows = (size_t)(d.N + 1) * d.nx;
    if (d.nw == d.nx) return put(h, h->E, E, sizeof(double) * rows * d.nx, loc);
    const double *src = E;
    if (loc == SLSQP_HOST) {
        double *tmp = stage_buf(h, sizeof(double) * rows * d.nw);
        if (!tmp) return -1;
        HIPCHK(hipMemcpyAsync(tmp, E, sizeof(double) * rows * d.nw, hipMemcpyHostToDevice, h->st));
        src = tmp;
    }
    hipLaunchKernelGGL(k_pad_cols, dim3(64), dim3(256), 0, h->st, (int)rows, d.nw, d.nx, src, h->E);
    HIPCHK(hipGetLastError());
    if (loc == SLSQP_HOST) HIPCHK(hipStreamSynchronize(h->st));
    return 0;
}

static bool is_diag(const double *M, int n) {
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) if (i != j && M[i * n + j] != 0.0) return false;
    return true;
}

extern "C" int slsqp_set_costs(slsqp_handle *h, const double *Q, const double *R, const double *Qf, const double *Q_reg, const double *R_reg,
                               const double *Q_reg_f) {
    hipSetDevice(h->dev);
    const int nx = h->d.nx, nu = h->d.nu;
    if (!is_diag(Q, nx) || !is_diag(R, nu) || !is_diag(Qf, nx) || !is_diag(Q_reg, nx) || !is_diag(R_reg, nu) || !is_diag(Q_reg_f, nx))
        return fail("Q,R,Qf,Q_reg,R_reg,Q_reg_f must be diagonal (HIP path); dense weights are not supported");
    std::vector<double> v;
    auto push = [&](const double *M, int n) { for (int i = 0; i < n; i++) v.push_back(M[i * n + i]); };
    push(Q, nx); push(R, nu); push(Qf, nx); push(Q_reg, nx); push(R_reg, nu); push(Q_reg_f, nx);
    for (int i = 0; i < nx + nu + nx; i++) if (!(v[i] > 0.0)) return fail("Q,R,Qf must be positive definite");
    HIPCHK(hipMemcpy(h->cst, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
    h->have_costs = true;
    return 0;
}

extern "C" int slsqp_set_constraints(slsqp_handle *h, const double *G, const double *Gf, const double *gf) {
    hipSetDevice(h->dev);
    const int nx = h->d.nx, nz = h->nz, ni = h->d.ni, nif = h->d.ni_f;
    bool box = (ni == 2 * nz) && (nif == 2 * nx);
    for (int i = 0; box && i < 2 * nz; i++) for (int j = 0; j < nz; j++) {
        const double want = (i % nz == j) ? (i < nz ? 1.0 : -1.0) : 0.0;
        if (G[i * nz + j] != want) { box = false; break; }
    }
    for (int i = 0; box && i < 2 * nx; i++) for (int j = 0; j < nx; j++) {
        const double want = (i % nx == j) ? (i < nx ? 1.0 : -1.0) : 0.0;
        if (Gf[i * nx + j] != want) { box = false; break; }
    }
    // general G (fast_SLS_jit.py:76-79, 138-170; Pendulum.replace_constraints): the SLS sweep takes it (k_sweep_gen); the QP solver eliminates box
    // constraints through a diagonal Pi and does not -- slsqp_solve / slsqp_qp_* / slsqp_cl_* refuse such a handle
    h->general_G = !box;
    HIPCHK(hipMemcpy(h->Gd, G, sizeof(double) * (size_t)ni * nz, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->Gfd, Gf, sizeof(double) * (size_t)nif * nx, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->gf_raw, gf, sizeof(double) * nif, hipMemcpyHostToDevice));
    h->gf_raw_host.assign(gf, gf + nif);
    h->have_cons = true;
    return 0;
}

static BoundsArgs bounds_args(slsqp_handle *h, const int *run);      // (with the other argument builders, below)
extern "C" int slsqp_update_dynamics(slsqp_handle *h, const double *A, const double *Bm, const double *E, const double *g, const double *g_N,
                                     const double *c, int loc) {
    hipSetDevice(h->dev);
    const slsqp_dims &d = h->d;
    const size_t B = h->B;
    if (!A || !Bm || !g || !g_N || !c) return fail("A, B, g, g_N, c are required");
    if (put(h, h->A, A, sizeof(double) * B * d.N * d.nx * d.nx, loc)) return -1;
    if (put(h, h->Bm, Bm, sizeof(double) * B * d.N * d.nx * d.nu, loc)) return -1;
    if (put_E(h, E, loc)) return -1;
    if (put(h, h->g, g, sizeof(double) * B * d.N * d.ni, loc)) return -1;
    if (put(h, h->gN, g_N, sizeof(double) * B * d.ni_f, loc)) return -1;
    if (put(h, h->c, c, sizeof(double) * B * d.N * d.nx, loc)) return -1;
    hipLaunchKernelGGL(k_set_bounds, dim3(1024), dim3(256), 0, h->st, bounds_args(h, nullptr));
    HIPCHK(hipGetLastError());
    h->have_dyn = true;
    return 0;
}

extern "C" int slsqp_update_linear_cost(slsqp_handle *h, const double *q, int loc) {
    hipSetDevice(h->dev);
    return put(h, h->q, q, sizeof(double) * (size_t)h->B * h->n, loc);
}

// ---- small mask kernels ------------------------------------------------------------------------------------
__global__ void k_fill_int(int *p, int v, int n) { int i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) p[i] = v; }
__global__ void k_fill_doubles(double *p, double v, size_t n) { for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v; }
__global__ void k_negate(const double *x, double *y, int n) { int i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) y[i] = -x[i]; }
__global__ void k_finish(int B, int rti, const int *alive, const int *infeas, int *success, const int *active, int *pending_reset) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (active && !active[b]) { success[b] = 0; return; }       // not part of this call
    if (rti) success[b] = (!infeas[b]) || success[b];           // fast_SLS_jit.py:295
    else if (alive[b] || infeas[b]) { success[b] = 0; pending_reset[b] = 1; }   // hit MAX_ITER or infeasible (:304, :312) -> _finish_failure
}
// _finish_failure (fast_SLS_jit.py:334-341) resets the solver AFTER the result dict has been built: the reset (eta, eta_f,
// iteration_number -> 0; bounds and linear cost are rewritten by the caller's next update anyway) is applied at the top of the
// instance's next solve, so that slsqp_get still returns the failed call's arrays.
__global__ void k_apply_pending_reset(int B, int *pending, const int *active, int *itnum, double *eta, size_t neta, double *eta_f, size_t netaf, int *stale) {
    const int b = blockIdx.x;
    if (!pending[b] || (active && !active[b])) return;
    for (size_t o = threadIdx.x; o < neta; o += blockDim.x) eta[(size_t)b * neta + o] = 0.0;
    for (size_t o = threadIdx.x; o < netaf; o += blockDim.x) eta_f[(size_t)b * netaf + o] = 0.0;
    __syncthreads();
    if (threadIdx.x == 0) { itnum[b] = 0; pending[b] = 0; stale[b] &= ~16; }
}
// The elementwise work between the first QP of a fast-SLS iteration and its sweep in ONE launch (one workgroup per instance), in the reference's order:
//   a failed QP drops the instance (forward_solve -> False, fast_SLS_jit.py:461-464);
//   evaluate_dual_eta (:475-487) -- in the first iteration of a solve beta = eps everywhere, eta[k,j] = mu_k / (2 sqrt(eps)) for every j <= k and only
//     column 0 is written (all the shared Riccati recursion reads; slsqp_get broadcasts it on demand);
//   check_convergence_socp (:581-600, its state persists across calls: quirk q5);
//   the mask of the instances that go on to Riccati + tightening (_step :318-326);
//   first iteration only: instances that are NOT swept but whose beta still holds an earlier solve's values get initialize_backoff's eps (the solve
//     start no longer writes beta for everybody: 1.1 GB per 4096 rocket instances).
// Five launches before; a pendulum closed-loop step is launch-bound and 30 of its ~120 launches were these.
struct AfterQpArgs {
    int B, rti, first_iter;
    const int *status, *active;
    int *alive, *infeas, *mask, *success, *itnum, *counter, *stale, *conv;
    EtaArgs ea; ConvArgs ca;
    double *beta_w, *beta_f_w;     // the same arrays as ea.beta / ea.beta_f, writable (the beta repair)
};
__global__ __launch_bounds__(256) void k_after_qp(AfterQpArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ int s_alive, s_m, s_stale;
    if (tid == 0) {
        int al = a.alive[b];
        if (al) { const int st = a.status[b]; if (!(st == 0 || st == 4)) { al = 0; a.alive[b] = 0; a.infeas[b] = 1; } }
        s_alive = al;
    }
    __syncthreads();
    const int alive = s_alive;
    if (alive) {       // ---- evaluate_dual_eta
        const EtaArgs &e = a.ea;
        const int SR = e.NX + e.NI, mb = e.N * SR + e.NIF;
        const double *du = e.dual + (size_t)b * mb;
        double *et = e.eta + (size_t)b * e.N * e.N * e.NI, *ef = e.eta_f + (size_t)b * (e.N + 1) * e.NIF;
        if (e.first_iter) {
            const double s0 = 2.0 * sqrt(e.eps);
            for (int o = tid; o < e.N * e.NI; o += blockDim.x) { const int i = o % e.NI, k = o / e.NI; et[((size_t)k * e.N) * e.NI + i] = du[k * SR + e.NX + i] / s0; }
            for (int o = tid; o < e.NIF; o += blockDim.x) ef[o] = du[e.N * SR + o] / s0;
        } else {
            const double *be = e.beta + (size_t)b * e.N * e.N * e.NI, *bf = e.beta_f + (size_t)b * (e.N + 1) * e.NIF;
            for (int o = tid; o < e.N * e.N * e.NI; o += blockDim.x) {
                const int i = o % e.NI, j = (o / e.NI) % e.N, k = o / (e.NI * e.N);
                if (j <= k) et[o] = du[k * SR + e.NX + i] / (2.0 * sqrt(fmax(be[o], e.eps)));
            }
            for (int o = tid; o < (e.N + 1) * e.NIF; o += blockDim.x) ef[o] = du[e.N * SR + (o % e.NIF)] / (2.0 * sqrt(fmax(bf[o], e.eps)));
        }
    }
    int cv = 0;
    if (tid < 64) {    // ---- check_convergence_socp (first wave)
        const ConvArgs &c = a.ca;
        if (alive) {
            const double *p = c.primal + (size_t)b * c.n;
            double *q = c.prev + (size_t)b * c.n;
            double d = 0.0;
            for (int o = tid; o < c.n; o += 64) { d = fmax(d, fabs(p[o] - q[o])); q[o] = p[o]; }
            d = wla::wave_max(d);
            if (tid == 0) { cv = (c.has_prev[b] && d <= c.tol) ? 1 : 0; c.has_prev[b] = 1; }
        }
        if (tid == 0) {
            a.conv[b] = cv;
            int st = a.stale[b];
            if (alive) st = a.ea.first_iter ? ((st & ~1) | 16) : (st & ~(1 | 16));      // state of the eta array: column 0 only / complete
            int m = 0;                                                                    // ---- mask
            if (alive) {
                if (cv) { a.success[b] = 1; if (!a.rti) a.alive[b] = 0; }
                else m = 1;
            }
            a.mask[b] = m;
            if (m) { a.itnum[b] += 1; st = (st & ~(2 | 32)) | 8; if (!a.rti) atomicAdd(a.counter, 1); }
            s_m = m; s_stale = st;
            a.stale[b] = st;
        }
    }
    __syncthreads();
    if (a.first_iter && !((a.active && !a.active[b]) || s_m || !(s_stale & 8))) {      // ---- beta repair
        const EtaArgs &e = a.ea;
        double *be = a.beta_w + (size_t)b * e.N * e.N * e.NI, *bf = a.beta_f_w + (size_t)b * (e.N + 1) * e.NIF;
        for (int o = tid; o < e.N * e.N * e.NI; o += blockDim.x) be[o] = e.eps;
        for (int o = tid; o < (e.N + 1) * e.NIF; o += blockDim.x) bf[o] = e.eps;
        if (tid == 0) a.stale[b] = s_stale & ~8;
    }
}

// The start of a fast-SLS solve in one launch (one workgroup per instance): x_0 pin value, alive mask, the pending solver reset of an instance
// whose last converge-mode solve failed, cleared flags, initialize_backoff.  Replaces seven launches.
struct SolveBeginArgs {
    int B, NX;
    const double *x0;            // (B,NX) device, or NULL when the pin value has already been written
    double *x0val;
    const int *active; int *alive, *infeas, *success, *pending, *itnum, *stale;
    double *eta, *eta_f; size_t neta, netaf;
    InitBackoffArgs ib;          // run = the instances whose back-offs are reset
    const int *skip;             // (B) or NULL: instances that are in the middle of a solve (slsqp_cl_run) and must not be touched at all
};
__global__ __launch_bounds__(256) void k_solve_begin(SolveBeginArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (a.skip && a.skip[b]) return;
    const int act = a.active ? a.active[b] : 1;
    if (a.x0 && tid < a.NX) a.x0val[(size_t)b * a.NX + tid] = -a.x0[(size_t)b * a.NX + tid];
    if (tid == 0) { a.alive[b] = act; a.infeas[b] = 0; a.success[b] = 0; }
    if (a.pending[b] && act) {       // _finish_failure of the previous call (_finish_failure, fast_SLS_jit.py:334-341)
        for (size_t o = tid; o < a.neta; o += blockDim.x) a.eta[(size_t)b * a.neta + o] = 0.0;
        for (size_t o = tid; o < a.netaf; o += blockDim.x) a.eta_f[(size_t)b * a.netaf + o] = 0.0;
        __syncthreads();
        if (tid == 0) { a.itnum[b] = 0; a.pending[b] = 0; a.stale[b] &= ~16; }
    }
    const InitBackoffArgs &i = a.ib;
    if (i.run && !i.run[b]) return;
    const int NZ = i.NX + i.NU, NI = 2 * NZ, NIF = 2 * i.NX, N = i.N;
    const double sq = sqrt(i.eps);
    for (int o = tid; o < N * NI; o += blockDim.x) i.backoff[(size_t)b * N * NI + o] = N * sq;
    for (int o = tid; o < NIF; o += blockDim.x) i.backoff_f[(size_t)b * NIF + o] = (N + 1) * sq;
    for (int o = tid; o < (N + 1) * i.NX; o += blockDim.x) i.backoff_x[(size_t)b * (N + 1) * i.NX + o] = 0.0;
    for (int o = tid; o < N * i.NU; o += blockDim.x) i.backoff_u[(size_t)b * N * i.NU + o] = 0.0;
}

// k_after_qp for ONE wave (the fused chain kernel below): the same steps in the same order, reductions through the wave instead of LDS.
__device__ __forceinline__ int after_qp_wave(const AfterQpArgs &a, int b, int lane) {
    int alive = a.alive[b];
    if (alive) { const int st = a.status[b]; if (!(st == 0 || st == 4)) { alive = 0; if (lane == 0) { a.alive[b] = 0; a.infeas[b] = 1; } } }
    const EtaArgs &e = a.ea;
    if (alive) {       // ---- evaluate_dual_eta
        const int SR = e.NX + e.NI, mb = e.N * SR + e.NIF;
        const double *du = e.dual + (size_t)b * mb;
        double *et = e.eta + (size_t)b * e.N * e.N * e.NI, *ef = e.eta_f + (size_t)b * (e.N + 1) * e.NIF;
        if (e.first_iter) {
            const double s0 = 2.0 * sqrt(e.eps);
            for (int o = lane; o < e.N * e.NI; o += 64) { const int i = o % e.NI, k = o / e.NI; et[((size_t)k * e.N) * e.NI + i] = du[k * SR + e.NX + i] / s0; }
            for (int o = lane; o < e.NIF; o += 64) ef[o] = du[e.N * SR + o] / s0;
        } else {
            const double *be = e.beta + (size_t)b * e.N * e.N * e.NI, *bf = e.beta_f + (size_t)b * (e.N + 1) * e.NIF;
            for (int o = lane; o < e.N * e.N * e.NI; o += 64) {
                const int i = o % e.NI, j = (o / e.NI) % e.N, k = o / (e.NI * e.N);
                if (j <= k) et[o] = du[k * SR + e.NX + i] / (2.0 * sqrt(fmax(be[o], e.eps)));
            }
            for (int o = lane; o < (e.N + 1) * e.NIF; o += 64) ef[o] = du[e.N * SR + (o % e.NIF)] / (2.0 * sqrt(fmax(bf[o], e.eps)));
        }
    }
    int cv = 0;
    const ConvArgs &c = a.ca;
    if (alive) {       // ---- check_convergence_socp
        const double *p = c.primal + (size_t)b * c.n;
        double *q = c.prev + (size_t)b * c.n;
        double d = 0.0;
        for (int o = lane; o < c.n; o += 64) { d = fmax(d, fabs(p[o] - q[o])); q[o] = p[o]; }
        d = wla::wave_max(d);
        cv = (c.has_prev[b] && d <= c.tol) ? 1 : 0;
    }
    int st = a.stale[b];
    if (alive) st = e.first_iter ? ((st & ~1) | 16) : (st & ~(1 | 16));
    int m = 0;                                                                        // ---- mask
    if (alive && !cv) m = 1;
    if (m) st = (st & ~(2 | 32)) | 8;
    const bool repair = a.first_iter && !((a.active && !a.active[b]) || m || !(st & 8));
    wla::wsync_mem();                  // every lane has read has_prev / stale / alive before lane 0 rewrites them
    if (lane == 0) {
        if (alive) c.has_prev[b] = 1;
        a.conv[b] = cv;
        if (alive && cv) { a.success[b] = 1; if (!a.rti) a.alive[b] = 0; }
        a.mask[b] = m;
        if (m) { a.itnum[b] += 1; if (!a.rti) atomicAdd(a.counter, 1); }
        a.stale[b] = repair ? (st & ~8) : st;
    }
    if (repair) {      // ---- beta repair
        double *be = a.beta_w + (size_t)b * e.N * e.N * e.NI, *bf = a.beta_f_w + (size_t)b * (e.N + 1) * e.NIF;
        for (int o = lane; o < e.N * e.N * e.NI; o += 64) be[o] = e.eps;
        for (int o = lane; o < (e.N + 1) * e.NIF; o += 64) bf[o] = e.eps;
    }
    return m;
}

// One RTI fast-SLS solve (fast_SLS.solve with rti_steps = 1, the rocket script's setting: QP -> eta -> Riccati / propagation / back-offs ->
// tightened bounds -> QP) of one instance by ONE wave in ONE launch.  The separate launches (k_qp_solve, k_after_qp, k_sweep_ric1, k_sweep_prop,
// k_tighten, k_qp_solve) put a batch-wide barrier behind each QP: every launch lasts as long as its slowest instance (a failed warm attempt
// followed by the interior point: 50-90 block solves against a mean of 10), so the step pays max(QP #1) + max(QP #2).  Here an instance that is
// slow in one QP only delays itself and the step pays max over the instances of their own sums.  Same device functions, same arithmetic, same bits.
struct ChainArgs {
    QpArgs q;                       // QP #1's arguments; QP #2's are these with the three ints of q2 (qp_second_args)
    Qp2Ints q2;
    AfterQpArgs aq;
    SweepSharedArgs sw;
    TightenArgs ta;
    const int *active; int *success; const int *infeas;      // k_finish
    unsigned long long *times;      // (B,4) or NULL: wall_clock64 ticks (100 MHz) of QP #1, the sweep part, QP #2 of each instance
    int max_ticks;
    // slsqp_cl_run (all NULL / 0 otherwise): instances advance through their MPC steps independently
    int *lag;                       // (B) 0: the instance starts its chain in this launch; 1 / 2: it was suspended inside QP #1 / QP #2 and resumes there
    const int *runm;                // (B) 0: the instance takes no part in this launch (it has finished all its steps)
    int *done;                      // (B) out: 1 = the chain of the instance ended in this launch
    unsigned long long *t0word;     // start time of the launch (first wave to arrive writes it), zeroed by the host before the launch
    unsigned long long budget;      // wall-clock ticks (100 MHz) after the start at which unfinished solves suspend themselves
    unsigned *fin_count; unsigned cut_count;      // chains of this launch that have ended (device counter, zeroed by the host); solves suspend once it reaches cut_count
    int *qplog; const int *stepno; int log_steps;      // (B, log_steps, 16) per-step copy of the instance's qp_stats, entry stepno[b]
    double *x0vlog;                 // (B, log_steps, 2) per-step copy of the instance's x0_viol, kept wherever qplog is
};
// BLK: c_ lies in the argument block of a persistent closed-loop kernel (args_here, slsqp_kernels.hpp): the head of the chain, of each pass, of the
// part behind QP #1 and of the tail read what they use afresh.
// BND: the tightening reads the terminal row of the instance's window of the bounds (bdp: in the block too with BLK, else the kernel's parameter).
template <int NX, int NU, bool BLK = false, bool BND = false>
__device__ __forceinline__ int rti_chain_dev(const ChainArgs &c_, int b, int lane, double *sm, const BndArgs *bdp = nullptr) {
    const ChainArgs *cp = &c_;
    unsigned long long t0 = wall_clock64(), t1 = t0, t2 = t0, deadline = ~0ULL;
    int lg = 0;
    const int have_lag = args_here<BLK>(cp).lag ? 1 : 0;
    if (have_lag) {
        const ChainArgs &c = args_here<BLK>(cp);
        lg = __builtin_amdgcn_readfirstlane(c.lag[b]);
        unsigned long long first = 0ULL;
        if (lane == 0) { first = atomicCAS(c.t0word, 0ULL, t0); if (first == 0ULL) first = t0; }
        first = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(first >> 32)) << 32) | (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)first);      // (the builtin returns a signed int: no sign extension)
        deadline = first + c.budget;
        if (lane == 0) c.done[b] = 0;
    }
    int fin = 1;
#pragma unroll 1
    for (int pass = (lg == 2 ? 1 : 0); pass < 2; pass++) {
        asm volatile("" : "+v"(lane));
        {
            const ChainArgs &c = args_here<BLK>(cp);
            Qp2Ints qi{c.q.warm, c.q.stat_slot, c.q.snap_use};
            if (pass) qi = c.q2;
            if constexpr (BLK) fin = __builtin_amdgcn_readfirstlane(qp_solve_dev<NX, NU, false, true>(c.q, b, lane, sm, c.max_ticks, (lg == pass + 1) ? 1 : 0, deadline, c.lag ? c.fin_count : nullptr, c.cut_count, qi));
            else fin = __builtin_amdgcn_readfirstlane(qp_solve_dev<NX, NU, false>(qp_second_args(c.q, qi), b, lane, sm, c.max_ticks, (lg == pass + 1) ? 1 : 0, deadline, c.lag ? c.fin_count : nullptr, c.cut_count));
        }
        wla::wsync_mem();
        const ChainArgs &c = args_here<BLK>(cp);
        if (!fin) { if (lane == 0) c.lag[b] = pass + 1; break; }      // suspended at the deadline: the next launch resumes this solve
        if (pass == 1) break;
        t1 = wall_clock64();
        asm volatile("" : "+v"(lane));
        const int m = __builtin_amdgcn_readfirstlane(after_qp_wave(c.aq, b, lane));      // (wave-uniform by construction; said so to the compiler)
        wla::wsync_mem();
        if (m) {       // Riccati + tightening for this instance (fast_SLS_jit.py:321-322)
            sweep_ric1_dev<NX, NU>(c.sw, b, lane, sm);
            wla::wsync_mem();
#pragma unroll 1
            for (int j = 0; j <= c.sw.s.N; j += 2) {      // two disturbance columns per pass
                asm volatile("" : "+v"(lane));
                sweep_prop_dev<NX, NU>(c.sw, b, j, min(2, c.sw.s.N + 1 - j), lane, sm);
                wla::wsync();
            }
            wla::wsync_mem();
            tighten_dev<BND, BLK>(c.ta, b, lane, 64, bdp);
            wla::wsync_mem();
        }
        t2 = wall_clock64();
    }
    if (!fin) return 0;
    const ChainArgs &c = args_here<BLK>(cp);
    if (lane == 0) {
        if (c.active && !c.active[b]) c.success[b] = 0;
        else c.success[b] = (!c.infeas[b]) || c.success[b];           // fast_SLS_jit.py:295 (k_finish, RTI)
        if (c.times) { const unsigned long long t3 = wall_clock64(); unsigned long long *t = c.times + (size_t)b * 4; t[0] = t1 - t0; t[1] = t2 - t1; t[2] = t3 - t2; t[3] = t3 - t0; }
        if (c.lag) { c.lag[b] = 0; c.done[b] = 1; atomicAdd(c.fin_count, 1u); }
    }
    if (c.qplog && lane < 16) c.qplog[((size_t)b * c.log_steps + min(c.stepno[b], c.log_steps - 1)) * 16 + lane] = c.q.qpstat[(size_t)b * 16 + lane];
    if (c.qplog && lane >= 16 && lane < 18)      // per-step copy of x0_viol; a QP that took no part (qp_stats status -1) records 0
        c.x0vlog[((size_t)b * c.log_steps + min(c.stepno[b], c.log_steps - 1)) * 2 + lane - 16] = c.q.qpstat[(size_t)b * 16 + (lane - 16) * 8 + 6] == -1 ? 0.0 : x0_record(c.q.kkt, c.q.B)[2 + (size_t)b * 2 + lane - 16];
    return 1;
}
// BND: a handle with bounds (slsqp_cl_step at large batches, the rounds of slsqp_cl_run); without, bd is empty and never read
template <int NX, int NU, bool BND>
__global__ __launch_bounds__(64, QP_PERSIST_WAVES_PER_SIMD) void k_rti_chain(ChainArgs c, BndArgs bd) {
    int b = blockIdx.x, lane = threadIdx.x;
    if (b >= c.q.B) return;
    if (c.runm && !c.runm[b]) return;
    extern __shared__ double sm[];
    rti_chain_dev<NX, NU, false, BND>(c, b, lane, sm, &bd);
}

// ---- the whole closed loop as ONE persistent launch (slsqp_cl_run, opts.cl_persistent) ------------------------------------------------
// A wave takes an instance from a device-side FIFO, runs ONE complete MPC step of it -- warm-start shift, solver reset, linearisation, x0 pin,
// solve start, the RTI chain (QP #1 -> eta -> Riccati / propagation -> tightened bounds -> QP #2), nominal update, primal infeasibility, log
// entry, plant step with the disturbance sample of that step -- and puts the instance back while it has steps left.  Every step of every
// instance is the same sequence of device functions the launches of slsqp_cl_step run (same arithmetic, same bits); what is gone is every
// barrier between instances: no wave slot waits for a round, a deadline or the slowest instance of a batch, and the FIFO order keeps the
// instances' step counters together so the run has no long tail.  The queue: slots[cap] (0 = empty, else instance + 1), tail / head
// tickets, `avail` = published items not yet claimed.  A wave that finds avail <= 0 EXITS (an instance is always either in the queue or
// held by a running wave, which will push and then pop again; so nothing is stranded); the only waits are for the slot of a ticket already
// taken to be published / cleared by a wave that is a few instructions away from doing so, and they are bounded (err flag instead of a hang).
// Hand-over between waves on different XCDs (own L2 each): agent-scope release before the push, acquire after the pop.
struct ClQueue { int *slots; unsigned mask; unsigned *head, *tail; int *avail, *err; };
__device__ __forceinline__ int clq_pop(const ClQueue &q, int lane) {
    int v = -1;
    if (lane == 0) {
        // a claim given back hides, while it lasts, an item published meanwhile: look again when the give-back leaves avail > 0, or this wave
        // and the publisher of that item could both exit with the item stranded in the queue
        bool claimed = true;
        while (atomicSub(q.avail, 1) <= 0)
            if (atomicAdd(q.avail, 1) + 1 <= 0) { claimed = false; break; }
        if (claimed) {
            const unsigned t = atomicAdd(q.head, 1u);
            int *slot = q.slots + (t & q.mask);
            int got = 0;
            for (int spin = 0; spin < (1 << 22) && !got; spin++) {
                got = __hip_atomic_exchange(slot, 0, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                if (!got) __builtin_amdgcn_s_sleep(4);
            }
            if (got) v = got - 1; else atomicExch(q.err, 1);
        }
    }
    return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ void clq_push(const ClQueue &q, int b, int lane) {
    if (lane == 0) {
        const unsigned p = atomicAdd(q.tail, 1u);
        int *slot = q.slots + (p & q.mask);
        bool ok = false;
        for (int spin = 0; spin < (1 << 22) && !ok; spin++) {
            int expected = 0;
            ok = __hip_atomic_compare_exchange_strong(slot, &expected, b + 1, __ATOMIC_RELEASE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!ok) __builtin_amdgcn_s_sleep(4);
        }
        if (ok) atomicAdd(q.avail, 1); else atomicExch(q.err, 2);
    }
}
__global__ void k_clq_init(int B, ClQueue q) {
    const unsigned cap = q.mask + 1u;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += gridDim.x * blockDim.x) q.slots[i] = (i < (unsigned)B) ? (int)i + 1 : 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) { *q.head = 0u; *q.tail = (unsigned)B; *q.avail = B; *q.err = 0; }
}
// k_solve_begin for one wave
__device__ __forceinline__ void solve_begin_wave(const SolveBeginArgs &a, int b, int lane) {
    const int act = a.active ? a.active[b] : 1;
    if (a.x0 && lane < a.NX) a.x0val[(size_t)b * a.NX + lane] = -a.x0[(size_t)b * a.NX + lane];
    const int pend = a.pending[b];
    wla::wsync_mem();
    if (lane == 0) { a.alive[b] = act; a.infeas[b] = 0; a.success[b] = 0; }
    if (pend && act) {       // _finish_failure of the previous call (fast_SLS_jit.py:334-341)
        for (size_t o = lane; o < a.neta; o += 64) a.eta[(size_t)b * a.neta + o] = 0.0;
        for (size_t o = lane; o < a.netaf; o += 64) a.eta_f[(size_t)b * a.netaf + o] = 0.0;
        const int st = a.stale[b];
        wla::wsync_mem();
        if (lane == 0) { a.itnum[b] = 0; a.pending[b] = 0; a.stale[b] = st & ~16; }
    }
    const InitBackoffArgs &i = a.ib;
    if (i.run && !i.run[b]) return;
    const int NZ = i.NX + i.NU, NI = 2 * NZ, NIF = 2 * i.NX, N = i.N;
    const double sq = sqrt(i.eps);
    for (int o = lane; o < N * NI; o += 64) i.backoff[(size_t)b * N * NI + o] = N * sq;
    for (int o = lane; o < NIF; o += 64) i.backoff_f[(size_t)b * NIF + o] = (N + 1) * sq;
    for (int o = lane; o < (N + 1) * i.NX; o += 64) i.backoff_x[(size_t)b * (N + 1) * i.NX + o] = 0.0;
    for (int o = lane; o < N * i.NU; o += 64) i.backoff_u[(size_t)b * N * i.NU + o] = 0.0;
}
struct LoopArgs {
    ChainArgs c; ClArgs cl; LinArgs lin; BoundsArgs ba; SolveBeginArgs sb; ClLogArgs lg; ScpArgs sa;
    int steps, n, have_log, fence, keep_laggards;
    int *stepno; double *call_ids, *q; int *stale, *itnum, *pending, *scp_active;
    const double *W_all; double *pinf;
    ClQueue Q;
    unsigned long long *busy, *t_begin;      // busy[0] sum over the MPC steps of the time a wave spent on them (100 MHz ticks), [2] MPC steps run; t_begin (B): start of the instance's current step
};
// The argument block of the two persistent kernels, whatever their variant (k_cl_loop uses L only; the fields behind it are k_cl_loop_scp's).  It lives in device
// memory, one block per handle (slsqp_handle::loop_blk), written by cl_run_persistent on the handle's stream before every launch; the kernels
// take its address and read it through args_here<true> (slsqp_kernels.hpp): the heads of cl_step_begin, of the chain's parts, of cl_step_end and of
// every part of qp_solve_dev's tick loop each read the fields they use.  What may go into it: anything -- a field costs a scalar load where it is
// used, not a register for the life of the kernel.
struct ScpLoopArgs {
    LoopArgs L;
    int max_it, converge, rti_steps;
    int *nsolves;
    BndArgs bd;      // slsqp_cl_set_bounds (the variants with VAR_BND only; behind everything else, so no other field moves)
};
// What the HOLD variants of k_cl_loop read besides: the arguments of the hold function (a.k and a.step are not read: every
// instance is at its own step) and M.  It lies in the same device block BEHIND the ScpLoopArgs, at HOLD_BLK_OFFSET: ScpLoopArgs keeps its size and
// every offset (bd stays its last field, tests/loop_args_check_main.cpp), and a run with M = 1 writes and reads the bytes it always did.
// Event-triggered runs (slsqp_cl_set_hold_trigger) read the fields behind M: theta (+inf: off -- none of the others is read),
// the last solve's backoff_x, the per-instance hold index that replaces hold_index_at(stepno, M), and the log of ratio and reason code.
// Plan fallback (slsqp_cl_set_plan_fallback) reads a PlanArgs BEHIND this struct in the same block, at PLAN_BLK_OFFSET: this struct
// keeps its size and every offset.  on = 0 (the default): none of its other fields is read.  With it on, a.A / a.Bm / a.Kc and backoff_x here are the
// backup's: every policy step and the trigger's ratio read the backup store.
struct HoldLoopArgs { HoldArgs a; int M; double theta; const double *backoff_x; int *hold_k; double *lratio; int *ltrig; };
// the hold index of instance b at its step s: the one the wave that ran step s - 1 decided, or the fixed period's (wave-uniform)
__device__ __forceinline__ int loop_hold_index(const HoldLoopArgs &H, int b, int s) { return cl_hold::trigger_on(H.theta, H.M) ? H.hold_k[b] : cl_hold::hold_index_at(s, H.M); }
constexpr size_t HOLD_BLK_OFFSET = (sizeof(ScpLoopArgs) + 15) & ~(size_t)15, LOOP_BLK_BYTES = 4096;
static_assert(HOLD_BLK_OFFSET + sizeof(HoldLoopArgs) <= LOOP_BLK_BYTES, "slsqp_handle::loop_blk is 4096 bytes");
__device__ __forceinline__ const HoldLoopArgs *hold_blk(const ScpLoopArgs *blk) { return (const HoldLoopArgs *)((const unsigned char *)blk + HOLD_BLK_OFFSET); }
constexpr size_t PLAN_BLK_OFFSET = (HOLD_BLK_OFFSET + sizeof(HoldLoopArgs) + 15) & ~(size_t)15;
static_assert(PLAN_BLK_OFFSET + sizeof(PlanArgs) <= LOOP_BLK_BYTES, "slsqp_handle::loop_blk is 4096 bytes");
__device__ __forceinline__ const PlanArgs *plan_blk_of(const HoldLoopArgs *hp) { return (const PlanArgs *)((const unsigned char *)hp + (PLAN_BLK_OFFSET - HOLD_BLK_OFFSET)); }
// What the CONV variants of k_cl_loop_scp read besides (slsqp_cl_set_sls_converge): per (instance, step) of the run's log the
// sweeps of the step's last fast-SLS solve (from which k_cl_qplog_sls_conv reproduces the batch-wide launches' "took no part") and iteration_number
// as the step leaves it (log_sls_iterations).  BEHIND the plan block in the same device block: nothing in front of it moves, no other kernel reads it.
struct SlsConvArgs { int *lastit, *itlog; int log_steps; };
constexpr size_t CONV_BLK_OFFSET = (PLAN_BLK_OFFSET + sizeof(PlanArgs) + 15) & ~(size_t)15;
static_assert(CONV_BLK_OFFSET + sizeof(SlsConvArgs) <= LOOP_BLK_BYTES, "slsqp_handle::loop_blk is 4096 bytes");
__device__ __forceinline__ const SlsConvArgs *conv_blk(const ScpLoopArgs *blk) { return (const SlsConvArgs *)((const unsigned char *)blk + CONV_BLK_OFFSET); }
// What the instantiations with the PP bit read at their plant step besides (slsqp_cl_set_adversary): the adversary's arguments
// (cl_adversary.hpp), BEHIND the CONV block in the same device block -- nothing in front of it moves.  policy = 0 (the zero bytes of a handle that never
// set the option): none of its other fields is read.  The block starts with the LoopArgs (L is ScpLoopArgs' first member), so both step-end functions
// reach it from the pointer they hold.
using AdvArgs = cl_adversary::Args;
constexpr size_t ADV_BLK_OFFSET = (CONV_BLK_OFFSET + sizeof(SlsConvArgs) + 15) & ~(size_t)15;
static_assert(ADV_BLK_OFFSET + sizeof(AdvArgs) <= LOOP_BLK_BYTES && sizeof(AdvArgs) % 8 == 0, "slsqp_handle::loop_blk is 4096 bytes");
__device__ __forceinline__ const AdvArgs *adv_blk(const LoopArgs *blk) { return (const AdvArgs *)((const unsigned char *)blk + ADV_BLK_OFFSET); }
// What the same instantiations read around their plant step for slsqp_cl_set_meas_noise: the arguments of the measurement rule
// (cl_meas.hpp), BEHIND the adversary's block -- nothing in front of it moves.  T = 0 (the zero bytes of a handle that never set the option): none of
// its other fields is read.
using MeasArgs = cl_meas::Args;
constexpr size_t MEAS_BLK_OFFSET = (ADV_BLK_OFFSET + sizeof(AdvArgs) + 15) & ~(size_t)15;
static_assert(MEAS_BLK_OFFSET + sizeof(MeasArgs) <= LOOP_BLK_BYTES && sizeof(MeasArgs) % 8 == 0, "slsqp_handle::loop_blk is 4096 bytes");
__device__ __forceinline__ const MeasArgs *meas_blk(const LoopArgs *blk) { return (const MeasArgs *)((const unsigned char *)blk + MEAS_BLK_OFFSET); }
// the two halves of an MPC step around the RTI chain, as functions of their own: what they keep in registers (dual numbers of the linearisation, the
// plant's RK4 stages) stays out of the register allocation of the QP loops, and nothing of theirs is live across the chain
// HOLD (k_cl_loop's hold variants): held != 0 is a hold step of the instance, which takes the shift alone -- no solver reset, so stale, itnum, q
// and call_ids stay and K stays valid; the rest of the hold step is cl_step_end's
template <int MODEL, bool REF = false, bool BND = false, bool HOLD = false>
__device__ CLW_FN void cl_step_begin(const LoopArgs &L_, int b, int lane, const RefArgs *rf = nullptr, const BndArgs *bd = nullptr, int held = 0) {
    const LoopArgs *Lp = &L_;
    const LoopArgs &L = args_here<true>(Lp);
    constexpr int NX = dyn::Dims<MODEL>::NX;
    const int s = L.stepno[b];
    if (lane == 0) L.t_begin[b] = wall_clock64();
#ifdef CL_LOOP_STAMP
    unsigned long long ts_ = wall_clock64();
#define CLSTAMP(i) do { wla::wsync_mem(); const unsigned long long t_ = wall_clock64(); if (lane == 0) atomicAdd(L.busy + (i), t_ - ts_); ts_ = t_; } while (0)
#else
#define CLSTAMP(i) do {} while (0)
#endif
    // reset_warm_start (shift + solver reset) past the first step, call id, flags
    if (s > 0) {
        cl_shift_wave<MODEL>(L.cl, b, lane);
        if constexpr (HOLD) { if (held) return; }
        for (int o = lane; o < L.n; o += 64) L.q[(size_t)b * L.n + o] = 0.0;
        const int st = L.stale[b];
        wla::wsync_mem();
        if (lane == 0) { L.stale[b] = (st & 8) | 3; L.itnum[b] = 0; L.pending[b] = 0; }
    }
    if (lane == 0) { L.call_ids[b] += 1.0; L.sa.scp_success[b] = 0; L.sa.scp_iters[b] = 0; }
    wla::wsync_mem();
    CLSTAMP(4);
    lin_wave<MODEL, REF, BND>(L.lin, L.ba, b, lane, rf, s, bd);      // (REF, BND: the window of the instance's OWN step count)
    CLSTAMP(5);
    if (lane < NX) L.cl.x0arg[(size_t)b * NX + lane] = L.cl.Xn[(size_t)b * (L.cl.N + 1) * NX + lane] - L.cl.xmeas[(size_t)b * NX + lane];
    wla::wsync_mem();
    solve_begin_wave(L.sb, b, lane);
    wla::wsync_mem();
    CLSTAMP(6);
}
// nominal += delta, primal infeasibility, log entry, plant + noise, step counter; returns the instance's new step count while it has steps left, else 0
// HOLD: at a step s of the instance that is no solve (cl_hold::hold_index_at(s, M) = k > 0; cl_step_begin has shifted the plan) the stages of
// slsqp_cl_hold_step's launches in their order instead -- the log items of the entry (the shifted plan, the last solve's back-offs and success), the
// hold function (xi, the policy's input u, hold_policy) in the LDS `sm`, the log fields k_cl_hold writes, "took no part" as the entry of log_qp_stats --
// and then the SAME plant step, one call site, with u in the place of the first nominal input
template <int MODEL, bool PP = false, bool HOLD = false>
__device__ CLW_FN int cl_step_end(const LoopArgs &L_, int b, int lane, const PlantArgs *pa = nullptr, const HoldLoopArgs *hp = nullptr, double *sm = nullptr, int *knext = nullptr) {
    const LoopArgs *Lp = &L_;
    const LoopArgs &L = args_here<true>(Lp);
    constexpr int NX = dyn::Dims<MODEL>::NX;
    const int s = L.stepno[b];
#ifdef CL_LOOP_STAMP
    unsigned long long ts_ = wall_clock64();
#endif
    bool held = false, fb = false;      // HOLD: a hold step; plan fallback is on (wave-uniform)
    int kprev = 0;      // HOLD: the hold index of this step
    if constexpr (HOLD) {
        const HoldLoopArgs &H = args_here<true>(hp);
        kprev = loop_hold_index(H, b, s);
        held = kprev != 0;
        fb = args_here<true>(plan_blk_of(hp)).on != 0;
        if (held && L.have_log) {
            const int per = 2 * ((L.lg.N + 1) * L.lg.NX + L.lg.N * L.lg.NU);
            for (int o = lane; o < per; o += 64) cl_log_item(L.lg, b, o);
            wla::wsync_mem();      // (lu0 of the entry is written again below, by other lanes)
        }
    }
    if (!held) {
        if (lane == 0) L.scp_active[b] = 1;
        wla::wsync_mem();
        cl_scp_update_wave(L.cl, L.sa, b, lane);
        wla::wsync_mem();
        CLSTAMP(7);
        if (L.sa.updated[b]) cl_infeas_wave<MODEL>(L.cl, L.pinf, b, lane);
        wla::wsync_mem();
        CLSTAMP(8);
        if (L.have_log) {
            const int per = 2 * ((L.lg.N + 1) * L.lg.NX + L.lg.N * L.lg.NU);
            for (int o = lane; o < per; o += 64) cl_log_item(L.lg, b, o);
            if constexpr (HOLD) { if (fb) wla::wsync_mem(); }      // (lu0 of the entry is written again below, by other lanes)
        }
    }
    if constexpr (HOLD) {
        // the hold function, ONE call site: a hold step runs it on the plan of the last solve; under plan fallback a solved step that failed runs it too,
        // and both on the backup, at the index the backup's age gives (after a solve that succeeded: the schedule's index and the live plan's bits)
        if (held || fb) {
            const HoldLoopArgs &H = args_here<true>(hp);
            int kk = kprev, plan = 0, age = -1, code = 0;
            bool run = held;
            if (fb) run = cl_fallback_begin<MODEL>(H.a, args_here<true>(plan_blk_of(hp)), b, lane, kprev, &kk, &plan, &age, &code);
            if (run) cl_hold_wave<MODEL>(H.a, b, lane, kk, sm, plan);
            if (held) {
                cl_hold_log<MODEL>(H.a, b, lane, kprev, s);
                if (L.c.qplog && s < L.c.log_steps) {      // no QP took part in this step: status -1 in both slots, 0 everywhere else, no stage-0 record
                    if (lane < 16) L.c.qplog[((size_t)b * L.c.log_steps + s) * 16 + lane] = (lane & 7) == 6 ? -1 : 0;
                    if (lane >= 16 && lane < 18) L.c.x0vlog[((size_t)b * L.c.log_steps + s) * 2 + (lane - 16)] = 0.0;
                }
            }
            if (fb) cl_fallback_log<MODEL>(H.a, args_here<true>(plan_blk_of(hp)), b, lane, s, held, age, code);
        }
    }
    CLSTAMP(9);
    if (lane == 0) {
        const double *w = L.W_all ? L.W_all + (size_t)s * L.cl.B * NX : nullptr;
        if constexpr (PP) cl_meas_lane<NX>(meas_blk(Lp), L.cl, b, s, false);      // slsqp_cl_set_meas_noise: the controller is done with its measurement; x_meas <- x_plant
        if constexpr (PP) w = cl_adversary_lane<NX>(adv_blk(Lp), L.cl, b, s, w);      // slsqp_cl_set_adversary: the sample is decided here, from x_meas as the plant step reads it
        if constexpr (HOLD) {
            ClArgs c = L.cl;
            if (held || fb) { c.N = 1; c.Un = args_here<true>(hp).a.u; }      // "the first nominal input" of instance b is u[b], as in k_cl_hold: the nominal itself stays the plan
            cl_plant_one<MODEL, PP>(c, b, w, pa, s);
        } else cl_plant_one<MODEL, PP>(L.cl, b, w, pa, s);
        if constexpr (PP) cl_meas_lane<NX>(meas_blk(Lp), L.cl, b, s, true);      // x_plant <- x_meas, x_meas <- x_meas + n_{s+1}: the trigger's decision below reads the new measurement
        L.stepno[b] = s + 1;
        if (L.busy) { atomicAdd(L.busy, wall_clock64() - L.t_begin[b]); atomicAdd(L.busy + 2, 1ULL); }
    }
    wla::wsync_mem();
    CLSTAMP(10);
    const int next = (s + 1 < L.steps) ? s + 1 : 0;
    if constexpr (HOLD) {
        // what the instance does at its next step, decided here: x_meas is new and the plan not yet shifted again.  Event-triggered: the tube ratio
        // of the hold step that would come next and cl_hold::decide, stored per instance for the loop top and for this function at step s + 1
        const HoldLoopArgs &H = args_here<true>(hp);
        if (!cl_hold::trigger_on(H.theta, H.M)) *knext = cl_hold::hold_index_at(next, H.M);
        else {
            *knext = 0;
            const bool lg = H.a.S > 0;
            if (s == 0 && lg && lane == 0) { H.ltrig[(size_t)b * H.a.S] = cl_hold::TRIG_SCHEDULED; H.lratio[(size_t)b * H.a.S] = 0.0; }
            if (next) {
                const bool ok = H.a.scp_success[b] != 0;
                const int kn = kprev + 1;
                double r = 0.0;
                if (ok && kn <= H.a.cl.N) r = cl_tube_ratio_wave<MODEL>(H.a.cl, H.backoff_x, b, lane, kn);
                const int code = cl_hold::decide(next, kprev, H.M, ok, r, H.theta);
                *knext = code == cl_hold::TRIG_HOLD ? kn : 0;
                if (lane == 0) {
                    H.hold_k[b] = *knext;
                    if (lg && next < H.a.S) { H.ltrig[(size_t)b * H.a.S + next] = code; H.lratio[(size_t)b * H.a.S + next] = r; }
                }
                wla::wsync_mem();
            }
        }
    }
    return next;
}
// The persistent closed loop, ONE body with five variants, VAR a set of the bits VAR_REF / VAR_PP / VAR_BND (cl_options).  0: plain; REF: tracks a
// reference (slsqp_cl_set_reference: the linear cost of cl_step_begin reads rf); PP: steps the plant with the instance's own parameters
// (slsqp_cl_set_plant_params: cl_step_end reads pa); BND: the box bounds of slsqp_cl_set_bounds (the linearisation's g_k / g_N and the chain's terminal
// tightened row read blk->bd).  PP and BND come with REF only (1, 3, 5, 7: a handle without a reference passes one row of zeros).  A variant is passed
// empty rf / pa where it reads none.  The three calls that name VAR, through var_ref / var_pp / var_bnd, are all that depends on it.  The statements
// stand in the kernel, not in a function it calls, and the next per-handle option is a further VAR bit, not a further kernel (DESIGN.md sections 14, 16).
// HOLD (9, 11, 13, 15; slsqp_cl_set_solve_every): the instance solves at its steps 0, M, 2M, ... only; at the others the loop
// body runs the shift of cl_step_begin, no chain, and the hold path of cl_step_end.  Every statement HOLD adds is under if constexpr (var_hold(VAR)).
template <int MODEL, int VAR>
__global__ __launch_bounds__(64, QP_PERSIST_WAVES_PER_SIMD) void k_cl_loop(const ScpLoopArgs *blk, RefArgs rf, PlantArgs pa) {
    constexpr int NX = dyn::Dims<MODEL>::NX, NU = dyn::Dims<MODEL>::NU;
    int lane = threadIdx.x;
    extern __shared__ double sm[];
    int b = -1;
#ifdef CL_LOOP_STAMP
    const unsigned long long tw0_ = wall_clock64();
    if (lane == 0) atomicMin(args_here<true>(blk).L.busy + 14, tw0_);
#endif
#pragma unroll 1
    for (;;) {
        asm volatile("" : "+v"(lane));
        const LoopArgs &L = args_here<true>(blk).L;
        if (b < 0) {
#ifdef CL_LOOP_STAMP
            const unsigned long long tp_ = wall_clock64();
#endif
            b = clq_pop(L.Q, lane);
            if (b < 0) break;
            if (L.fence & 1) __threadfence();      // acquire: what the wave that ran this instance's previous step wrote (possibly through another XCD's L2)
#ifdef CL_LOOP_STAMP
            if (lane == 0) atomicAdd(L.busy + 11, wall_clock64() - tp_);
#endif
        }
        bool solve = true;      // HOLD: the instance's step is a solve or a hold step (read again in cl_step_end: nothing of it is live across the chain)
        if constexpr (var_hold(VAR)) solve = __builtin_amdgcn_readfirstlane(loop_hold_index(args_here<true>(hold_blk(blk)), b, L.stepno[b])) == 0;
        cl_step_begin<MODEL, var_ref(VAR), var_bnd(VAR), var_hold(VAR)>(L, b, lane, var_ref(VAR) ? &rf : nullptr, var_bnd(VAR) ? &blk->bd : nullptr, solve ? 0 : 1);
        b = __builtin_amdgcn_readfirstlane(b);      // (across a call the compiler may park it in a vector register)
        asm volatile("" : "+v"(lane));
        if (solve) {
            rti_chain_dev<NX, NU, true, var_bnd(VAR)>(L.c, b, lane, sm, var_bnd(VAR) ? &blk->bd : nullptr);
            wla::wsync_mem();
        }
        asm volatile("" : "+v"(lane));
        int knext = 0;      // HOLD: the hold index of the instance's next step (0: a solve)
        const int next = __builtin_amdgcn_readfirstlane(cl_step_end<MODEL, var_pp(VAR), var_hold(VAR)>(L, b, lane, var_pp(VAR) ? &pa : nullptr, var_hold(VAR) ? hold_blk(blk) : nullptr, sm, &knext));
        b = __builtin_amdgcn_readfirstlane(b);
        if (!next) { b = -1; continue; }
        // HOLD: the hold steps that follow a solve (at most M - 1, fewer at the end of the run) run at once on this wave, without a queue round trip;
        // the tail below then sees the step count the instance has reached
        if constexpr (var_hold(VAR)) { if (__builtin_amdgcn_readfirstlane(knext)) continue; }
        const LoopArgs &Lt = args_here<true>(blk).L;      // (the tail's few fields, read here and not held across the step)
        // An instance that is behind the batch's mean progress keeps its wave and goes straight on (a few instances are slow in MANY of their
        // steps: queueing after each of them they would finish long after the others, with the GPU nearly empty); the others queue up, so the
        // waves are shared fairly among the instances that are level
        const unsigned long long done_steps = __hip_atomic_load(Lt.busy + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int behind = __builtin_amdgcn_readfirstlane(((unsigned long long)next * (unsigned long long)Lt.cl.B < done_steps) ? 1 : 0);
        if (behind && Lt.keep_laggards) continue;
#ifdef CL_LOOP_STAMP
        const unsigned long long tq_ = wall_clock64();
#endif
        if (Lt.fence & 2) __threadfence();      // release: the next step of this instance may run anywhere
        clq_push(Lt.Q, b, lane);
        b = -1;
#ifdef CL_LOOP_STAMP
        if (lane == 0) atomicAdd(L.busy + 12, wall_clock64() - tq_);
#endif
    }
#ifdef CL_LOOP_STAMP
    if (lane == 0) { const LoopArgs &L = args_here<true>(blk).L; const unsigned long long te_ = wall_clock64(); atomicAdd(L.busy + 13, te_ - tw0_); atomicMax(L.busy + 15, te_); atomicAdd(L.busy + 1, 1ULL); }
#endif
}

// ---- the persistent loop for any SCP setting of slsqp_cl_step (slsqp_cl_run_scp) -------------------------------------------------------
// One queue item is still one whole MPC step of one instance, but the step is the general one: max_it SCP iterations (SCP_SLS.solve,
// SCP_SLS_jit.py:103-135), each a fast-SLS solve of rti_steps steps (fast_SLS.solve, fast_SLS_jit.py:278-296) -- what slsqp_cl_step and solve_impl
// launch for the batch, here per instance by the wave that holds it, same device functions in the same order.  A kernel of its own: k_cl_loop
// (one iteration, one step) keeps its code object.
//   fixed rti: every instance runs its rti iterations; one whose step failed is masked through scp_active for the remaining ones exactly as the
//     launches mask it (linearisation skipped, solve start / QPs / finish see it as "takes no part", no nominal update);
//   converge mode (rti <= 0): an instance leaves as soon as cl_scp_update_wave clears its scp_active (converged or failed) -- the batch-wide
//     launches go on until the last instance has left and, for the ones that left earlier, only rewrite their qp_stats slots as "took no part".
//     nsolves (B, steps) keeps the number of solves each step of each instance ran, from which k_cl_qplog_masked reproduces that afterwards.
// shift + solver reset past the first step, SCP flags of the step (slsqp_cl_step's preamble)
template <int MODEL>
__device__ CLW_FN void cl_scp_step_begin(const LoopArgs &L_, int b, int lane) {
    const LoopArgs *Lp = &L_;
    const LoopArgs &L = args_here<true>(Lp);
    const int s = L.stepno[b];
    if (lane == 0) L.t_begin[b] = wall_clock64();
    if (s > 0) {
        cl_shift_wave<MODEL>(L.cl, b, lane);
        for (int o = lane; o < L.n; o += 64) L.q[(size_t)b * L.n + o] = 0.0;
        const int st = L.stale[b];
        wla::wsync_mem();
        if (lane == 0) { L.stale[b] = (st & 8) | 3; L.itnum[b] = 0; L.pending[b] = 0; }
    }
    if (lane == 0) { L.scp_active[b] = 1; L.sa.scp_success[b] = 0; L.sa.scp_iters[b] = 0; }
    wla::wsync_mem();
}
// start of SCP iteration ii: linearisation (instances still iterating), x0 pin, call id, solve start
template <int MODEL, bool REF = false, bool BND = false>
__device__ CLW_FN void cl_scp_iter_begin(const LoopArgs &L_, int b, int lane, int ii, const RefArgs *rf = nullptr, const BndArgs *bd = nullptr) {
    const LoopArgs *Lp = &L_;
    const LoopArgs &L = args_here<true>(Lp);
    constexpr int NX = dyn::Dims<MODEL>::NX;
    const int act = __builtin_amdgcn_readfirstlane(L.scp_active[b]);
    if (ii == 0 || act) lin_wave<MODEL, REF, BND>(L.lin, L.ba, b, lane, rf, (REF || BND) ? L.stepno[b] : 0, bd);      // (REF, BND: every iteration of the step uses the window of the instance's own step count)
    if (lane < NX) L.cl.x0arg[(size_t)b * NX + lane] = L.cl.Xn[(size_t)b * (L.cl.N + 1) * NX + lane] - L.cl.xmeas[(size_t)b * NX + lane];
    if (lane == 0) L.call_ids[b] += 1.0;
    wla::wsync_mem();
    solve_begin_wave(L.sb, b, lane);
    wla::wsync_mem();
}
// end of SCP iteration ii: nominal += delta / the instance leaves the loop, primal infeasibility; returns 1 while the instance is still iterating
template <int MODEL>
__device__ CLW_FN int cl_scp_iter_end(const LoopArgs &L_, int b, int lane, int ii, int converge) {
    const LoopArgs *Lp = &L_;
    const LoopArgs &L = args_here<true>(Lp);
    ScpArgs sa = L.sa;
    sa.ii = ii; sa.converge = converge;
    cl_scp_update_wave(L.cl, sa, b, lane);
    wla::wsync_mem();
    if (L.sa.updated[b]) cl_infeas_wave<MODEL>(L.cl, L.pinf, b, lane);
    wla::wsync_mem();
    return L.scp_active[b];
}
// log entries, plant step + noise, step counter; returns the instance's new step count while it has steps left, else 0
template <int MODEL, bool PP = false>
__device__ CLW_FN int cl_scp_step_end(const ScpLoopArgs &S_, int b, int lane, int nsolves, const PlantArgs *pa = nullptr) {
    const ScpLoopArgs *Sp = &S_;
    const ScpLoopArgs &S = args_here<true>(Sp);
    const LoopArgs &L = S.L;
    constexpr int NX = dyn::Dims<MODEL>::NX;
    const int s = L.stepno[b];
    if (L.have_log) {
        const int per = 2 * ((L.lg.N + 1) * L.lg.NX + L.lg.N * L.lg.NU);
        for (int o = lane; o < per; o += 64) cl_log_item(L.lg, b, o);
    }
    if (L.c.qplog && s < L.c.log_steps) {
        if (lane < 16) L.c.qplog[((size_t)b * L.c.log_steps + s) * 16 + lane] = L.c.q.qpstat[(size_t)b * 16 + lane];
        else if (lane < 18) L.c.x0vlog[((size_t)b * L.c.log_steps + s) * 2 + lane - 16] = L.c.q.qpstat[(size_t)b * 16 + (lane - 16) * 8 + 6] == -1 ? 0.0 : x0_record(L.c.q.kkt, L.c.q.B)[2 + (size_t)b * 2 + lane - 16];
        if (lane == 0) S.nsolves[(size_t)b * L.c.log_steps + s] = nsolves;
    }
    if (lane == 0) {
        const double *w = L.W_all ? L.W_all + (size_t)s * L.cl.B * NX : nullptr;
        if constexpr (PP) cl_meas_lane<NX>(meas_blk(&Sp->L), L.cl, b, s, false);      // slsqp_cl_set_meas_noise, as in cl_step_end
        if constexpr (PP) w = cl_adversary_lane<NX>(adv_blk(&Sp->L), L.cl, b, s, w);      // slsqp_cl_set_adversary, as in cl_step_end
        cl_plant_one<MODEL, PP>(L.cl, b, w, pa, s);
        if constexpr (PP) cl_meas_lane<NX>(meas_blk(&Sp->L), L.cl, b, s, true);
        L.stepno[b] = s + 1;
        if (L.busy) { atomicAdd(L.busy, wall_clock64() - L.t_begin[b]); atomicAdd(L.busy + 2, 1ULL); }
    }
    wla::wsync_mem();
    return (s + 1 < L.steps) ? s + 1 : 0;
}
// one fast-SLS solve of rti_steps steps of one instance by one wave: what solve_impl launches (fast_SLS_jit.py:278-296).  QP i of the call gets the
// arguments launch_qp builds for it: the first one q1's (warm per opts.warm_start, slot 0, no iterate copy to restart from), the middle ones warm,
// slot 0, restart allowed, the last one q2's; the horizon shift only reaches the first and the last QP of the first solve after the shift
// CONV (the CONV variants of k_cl_loop_scp): fast-SLS converge mode (fast_SLS_jit.py:298-312), what solve_impl launches with
// rti_steps <= 0.  rti_steps is the cap max_sls_iter here; QP i = 0 .. cap - 1 with the first call's arguments (warm and restart past the first),
// after_qp_wave with rti = 0 (it clears `alive` on convergence); the instance leaves at the first iteration that returns no mask -- converged, or its
// QP failed -- else sweep and tightening; then the last QP, which solves for an instance still alive (it hit the cap, :311) and writes "took no part"
// for every other, as the batch-wide launch on `alive` does; then k_finish's converge branch (pending: the solver reset of the instance's next solve,
// applied by solve_begin_wave).  *nsweeps: the sweeps of this solve.  No exit depends on another instance; every bound is wave-uniform.
template <int NX, int NU, bool BND = false, bool CONV = false>
__device__ __forceinline__ void sls_solve_dev(const ChainArgs &c_, int b, int lane, double *sm, int rti_steps, int shifted, const BndArgs *bdp = nullptr, int *pending = nullptr, int *nsweeps = nullptr) {
    const ChainArgs *cp = &c_;
    [[maybe_unused]] int left = 0, swept = 0;      // CONV: the instance has left the loop (the pass that follows is its last QP); sweeps so far
#pragma unroll 1
    for (int i = 0; i <= rti_steps; i++) {
        asm volatile("" : "+v"(lane));
        {
            const ChainArgs &c = args_here<true>(cp);
            QpArgs q = c.q;
            q.warm = i > 0 ? 1 : c.q.warm;
            q.stat_slot = i == rti_steps ? 1 : 0;
            q.snap_use = i > 0 ? c.q2.snap_use : 0;
            q.warm_shift = (shifted && (i == 0 || i == rti_steps)) ? c.q.warm_shift : 0;
            if constexpr (CONV) { if (left) { q.stat_slot = 1; q.warm_shift = shifted ? c.q.warm_shift : 0; } }
            qp_solve_dev<NX, NU, false>(q, b, lane, sm, c.max_ticks);
        }
        wla::wsync_mem();
        if (i == rti_steps) break;
        if constexpr (CONV) { if (left) break; }
        asm volatile("" : "+v"(lane));
        const ChainArgs &c = args_here<true>(cp);
        AfterQpArgs aq = c.aq;
        aq.first_iter = i == 0 ? 1 : 0; aq.ea.first_iter = aq.first_iter;
        if constexpr (CONV) aq.rti = 0;
        const int m = __builtin_amdgcn_readfirstlane(after_qp_wave(aq, b, lane));
        wla::wsync_mem();
        if constexpr (CONV) { if (!m) { left = 1; continue; } swept++; }
        if (!m) continue;
        if (i == 0) {      // beta = eps in every column: one Riccati recursion for all of them
            sweep_ric1_dev<NX, NU>(c.sw, b, lane, sm);
            wla::wsync_mem();
#pragma unroll 1
            for (int j = 0; j <= c.sw.s.N; j += 2) {
                asm volatile("" : "+v"(lane));
                sweep_prop_dev<NX, NU>(c.sw, b, j, min(2, c.sw.s.N + 1 - j), lane, sm);
                wla::wsync();
            }
        } else {
#pragma unroll 1
            for (int j = 0; j <= c.sw.s.N; j++) {      // the general sweep, column by column
                asm volatile("" : "+v"(lane));
                sweep_col_dev<NX, NU>(c.sw.s, b, j, lane, sm);
                wla::wsync();
            }
        }
        wla::wsync_mem();
        tighten_dev<BND, true>(c.ta, b, lane, 64, bdp);
        wla::wsync_mem();
    }
    const ChainArgs &c = args_here<true>(cp);
    if (lane == 0) {
        if (c.active && !c.active[b]) c.success[b] = 0;
        else if constexpr (CONV) { if (c.aq.alive[b] || c.infeas[b]) { c.success[b] = 0; pending[b] = 1; } }      // hit the cap or infeasible (k_finish, converge mode: :304, :312)
        else c.success[b] = (!c.infeas[b]) || c.success[b];           // fast_SLS_jit.py:295 (k_finish, RTI)
    }
    if constexpr (CONV) *nsweeps = swept;
    wla::wsync_mem();
}
// one body for the five variants, as k_cl_loop above: var_ref reads the tracked linear cost in cl_scp_iter_begin, var_pp the plant parameters in
// cl_scp_step_end, var_bnd the bounds in cl_scp_iter_begin and sls_solve_dev
// CONV (slsqp_cl_set_sls_converge): every fast-SLS solve of the step runs in converge mode (sls_solve_dev's CONV, S.rti_steps the
// cap max_sls_iter), and the step's entry of the two per-step arrays behind the block is written.  A flag of its own, not a VAR bit: the five
// variants exist with and without it, and every statement it adds is under if constexpr (CONV).
template <int MODEL, int VAR, bool CONV = false>
__global__ __launch_bounds__(64, QP_PERSIST_WAVES_PER_SIMD) void k_cl_loop_scp(const ScpLoopArgs *blk, RefArgs rf, PlantArgs pa) {
    constexpr int NX = dyn::Dims<MODEL>::NX, NU = dyn::Dims<MODEL>::NU;
    int lane = threadIdx.x;
    extern __shared__ double sm[];
    int b = -1;
#pragma unroll 1
    for (;;) {
        asm volatile("" : "+v"(lane));
        const ScpLoopArgs &S = args_here<true>(blk);
        const LoopArgs &L = S.L;
        if (b < 0) {
            b = clq_pop(L.Q, lane);
            if (b < 0) break;
            if (L.fence & 1) __threadfence();
        }
        cl_scp_step_begin<MODEL>(L, b, lane);
        b = __builtin_amdgcn_readfirstlane(b);
        int nsolves = 0;
        [[maybe_unused]] int nsweeps = 0;      // CONV: the sweeps of the step's last solve
#pragma unroll 1
        for (int ii = 0; ii < S.max_it; ii++) {
            asm volatile("" : "+v"(lane));
            cl_scp_iter_begin<MODEL, var_ref(VAR), var_bnd(VAR)>(L, b, lane, ii, var_ref(VAR) ? &rf : nullptr, var_bnd(VAR) ? &blk->bd : nullptr);
            b = __builtin_amdgcn_readfirstlane(b);
            asm volatile("" : "+v"(lane));
            if constexpr (CONV) {
                sls_solve_dev<NX, NU, var_bnd(VAR), true>(L.c, b, lane, sm, S.rti_steps, ii == 0 ? 1 : 0, var_bnd(VAR) ? &blk->bd : nullptr, L.pending, &nsweeps);
                nsweeps = __builtin_amdgcn_readfirstlane(nsweeps);
            } else sls_solve_dev<NX, NU, var_bnd(VAR)>(L.c, b, lane, sm, S.rti_steps, ii == 0 ? 1 : 0, var_bnd(VAR) ? &blk->bd : nullptr);
            asm volatile("" : "+v"(lane));
            const int act = __builtin_amdgcn_readfirstlane(cl_scp_iter_end<MODEL>(L, b, lane, ii, S.converge));
            b = __builtin_amdgcn_readfirstlane(b);
            nsolves = ii + 1;
            if (S.converge && !act) break;
        }
        if constexpr (CONV) {
            const SlsConvArgs &V = args_here<true>(conv_blk(blk));
            const LoopArgs &Lc = args_here<true>(blk).L;
            const int s = Lc.stepno[b];
            if (lane == 0 && s < V.log_steps) { V.lastit[(size_t)b * V.log_steps + s] = nsweeps; V.itlog[(size_t)b * V.log_steps + s] = Lc.itnum[b]; }
        }
        asm volatile("" : "+v"(lane));
        const int next = __builtin_amdgcn_readfirstlane(cl_scp_step_end<MODEL, var_pp(VAR)>(S, b, lane, nsolves, var_pp(VAR) ? &pa : nullptr));
        b = __builtin_amdgcn_readfirstlane(b);
        if (!next) { b = -1; continue; }
        const LoopArgs &Lt = args_here<true>(blk).L;      // (the tail's few fields, read here and not held across the step)
        const unsigned long long done_steps = __hip_atomic_load(Lt.busy + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int behind = __builtin_amdgcn_readfirstlane(((unsigned long long)next * (unsigned long long)Lt.cl.B < done_steps) ? 1 : 0);
        if (behind && Lt.keep_laggards) continue;
        if (Lt.fence & 2) __threadfence();
        clq_push(Lt.Q, b, lane);
        b = -1;
    }
}
// converge mode: the batch-wide launches of step s run max over the instances of their solves; an instance that left earlier has its qp_stats
// slots rewritten as "took no part" (status -1) by the QP launches that follow.  One block per step.
__global__ void k_cl_qplog_masked(int B, int steps, int log_steps, const int *nsolves, int *qplog, double *x0vlog) {
    const int s = blockIdx.x;
    __shared__ int smax;
    if (threadIdx.x == 0) smax = 0;
    __syncthreads();
    int mx = 0;
    for (int b = threadIdx.x; b < B; b += blockDim.x) mx = max(mx, nsolves[(size_t)b * log_steps + s]);
    atomicMax(&smax, mx);
    __syncthreads();
    mx = smax;
    for (int b = threadIdx.x; b < B; b += blockDim.x)
        if (nsolves[(size_t)b * log_steps + s] < mx) {
            int *qs = qplog + ((size_t)b * log_steps + s) * 16;
            for (int i = 0; i < 16; i++) qs[i] = (i % 8 == 6) ? -1 : 0;
            x0vlog[((size_t)b * log_steps + s) * 2] = 0.0; x0vlog[((size_t)b * log_steps + s) * 2 + 1] = 0.0;      // (a QP that took no part records 0)
        }
}
// fast-SLS converge mode (the CONV variants; cl_sls_conv.hpp): among the instances that took part in the last solve the batch-wide launches of step s
// run -- the ones with the step's largest number of solves -- an instance that left the fast-SLS loop before the last loop QP was launched has its
// slot 0 rewritten as "took no part" by the launches that follow.  lastit (B, log_steps): the sweeps of each instance's last solve of the step.
// One block per step, behind k_cl_qplog_masked (which has dealt with the instances that ran fewer solves).
__global__ void k_cl_qplog_sls_conv(int B, int steps, int log_steps, int cap, const int *nsolves, const int *lastit, int *qplog, double *x0vlog) {
    const int s = blockIdx.x;
    __shared__ int smax, nmax;
    if (threadIdx.x == 0) { smax = 0; nmax = 0; }
    __syncthreads();
    int mx = 0;
    for (int b = threadIdx.x; b < B; b += blockDim.x) mx = max(mx, nsolves[(size_t)b * log_steps + s]);
    atomicMax(&smax, mx);
    __syncthreads();
    mx = smax;
    int nm = 0;
    for (int b = threadIdx.x; b < B; b += blockDim.x) if (nsolves[(size_t)b * log_steps + s] == mx) nm = max(nm, lastit[(size_t)b * log_steps + s]);
    atomicMax(&nmax, nm);
    __syncthreads();
    nm = nmax;
    for (int b = threadIdx.x; b < B; b += blockDim.x)
        if (nsolves[(size_t)b * log_steps + s] == mx && cl_sls_conv::slot0_took_no_part(lastit[(size_t)b * log_steps + s], nm, cap)) {
            int *qs = qplog + ((size_t)b * log_steps + s) * 16;
            for (int i = 0; i < 8; i++) qs[i] = (i == 6) ? -1 : 0;
            x0vlog[((size_t)b * log_steps + s) * 2] = 0.0;      // (a QP that took no part records 0)
        }
}

// ---- masked pieces of a closed-loop round (slsqp_cl_run) ----
// cl_stage[b]: what the instance does in this round -- begin = it starts its next MPC step (shift, reset, linearise, x0 pin, solve start), runm = it runs
// the chain (begins or resumes), from its step counter and lag state
__global__ void k_cl_round_masks(int B, int steps, const int *stepno, const int *lag, int *begin, int *runm, int *skip_begin, int *done, int *n_unfinished) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int unfinished = stepno[b] < steps;
    const int bg = unfinished && lag[b] == 0;
    begin[b] = bg; runm[b] = unfinished; skip_begin[b] = !bg;
    done[b] = 0;       // (set by the chain kernel for the instances whose chain ends in this round; instances that take no part must not keep an old 1)
    if (unfinished) atomicAdd(n_unfinished, 1);
}
// reset_solver_to_zeros of slsqp_reset for the instances that begin a step (the others are in the middle of theirs)
__global__ void k_cl_reset_masked(int B, int n, const int *begin, const int *stepno, int *stale, int *itnum, int *pending, double *q) {
    const int b = blockIdx.x;
    if (!begin[b] || stepno[b] == 0) return;
    for (int o = threadIdx.x; o < n; o += blockDim.x) q[(size_t)b * n + o] = 0.0;
    if (threadIdx.x == 0) { stale[b] = (stale[b] & 8) | 3; itnum[b] = 0; pending[b] = 0; }
}
__global__ void k_cl_advance(int B, const int *done, int *stepno, double *call_ids, const int *begin) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (done[b]) stepno[b] += 1;
}
__global__ void k_cl_bump_call(int B, const int *begin, double *call_ids) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && begin[b]) call_ids[b] += 1.0;
}

__global__ void k_reset_stale(int *p, int n) { int i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) p[i] = (p[i] & 8) | 3; }   // eta, K: zero on demand; beta keeps its state
// instances whose `bit` is set in stale[]: zero their slice of arr1 (and arr2), then clear the bit (last use decides: clear_bit)
__global__ void k_zero_stale(int *stale, int bit, double *arr1, size_t n1, double *arr2, size_t n2) {
    const int b = blockIdx.x;
    if (!(stale[b] & bit)) return;
    for (size_t o = threadIdx.x; o < n1; o += blockDim.x) arr1[(size_t)b * n1 + o] = 0.0;
    if (arr2) for (size_t o = threadIdx.x; o < n2; o += blockDim.x) arr2[(size_t)b * n2 + o] = 0.0;
    __syncthreads();
    if (threadIdx.x == 0) stale[b] &= ~bit;
}
// beta[k,j] = 0 (j > k) for the instances whose beta holds a sweep's values (stale bit 8): the sweeps write the entries j <= k only and what lies above the
// diagonal is still initialize_backoff's eps, where the reference returns the zeros of _backoff_from_phi (fast_SLS_jit.py:141).  Nothing on the device reads
// those entries (evaluate_dual_eta and the back-off sums stop at j = k), so they are cleared only when the array is handed out.
__global__ void k_beta_upper_zero(int N, int NI, const int *stale, double *beta) {
    const int b = blockIdx.x;
    if (!(stale[b] & 8)) return;
    double *be = beta + (size_t)b * N * N * NI;
    for (int o = threadIdx.x; o < N * N * NI; o += blockDim.x) {
        const int j = (o / NI) % N, k = o / (NI * N);
        if (j > k) be[o] = 0.0;
    }
}
__global__ void k_copy_int(const int *src, int *dst, int n) { int i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) dst[i] = src[i]; }
__global__ void k_split_lu(int B, int mb, int nx, const double *l, const double *u, double *lbg, double *ubg, double *x0val) {
    const int m = mb + nx;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < (size_t)B * m; idx += (size_t)gridDim.x * blockDim.x) {
        const int b = idx / m, r = idx % m;
        if (r < mb) { lbg[(size_t)b * mb + r] = l[idx]; ubg[(size_t)b * mb + r] = u[idx]; }
        else x0val[(size_t)b * nx + (r - mb)] = 0.5 * (l[idx] + u[idx]);
    }
}
__global__ void k_gather_csc(int B, int cnt, int nnz, const int *map, const double *Ax, double *dst) {
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < (size_t)B * cnt; idx += (size_t)gridDim.x * blockDim.x) {
        const int b = idx / cnt, o = idx % cnt;
        dst[idx] = Ax[(size_t)b * nnz + map[o]];
    }
}
__global__ void k_join_y(int B, int mb, int nx, const double *dual, const double *pin, double *y) {
    const int m = mb + nx;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < (size_t)B * m; idx += (size_t)gridDim.x * blockDim.x) {
        const int b = idx / m, r = idx % m;
        y[idx] = r < mb ? dual[(size_t)b * mb + r] : pin[(size_t)b * nx + (r - mb)];
    }
}

// ---- kernel argument builders ---------------------------------------------------------
// One builder per argument struct: the handle and, by name, what varies between the launch sites.  Every site calls it; no HIP call in any of them.
static Costs costs_of(slsqp_handle *h) {
    const int nx = h->d.nx, nu = h->d.nu;
    Costs c;
    c.Qd = h->cst; c.Rd = c.Qd + nx; c.Qfd = c.Rd + nu; c.Qregd = c.Qfd + nx; c.Rregd = c.Qregd + nx; c.Qregfd = c.Rregd + nu; c.prox = 0.0;
    return c;
}
static ClArgs cl_args(slsqp_handle *h, const double *w) {
    ClArgs a;
    a.B = h->B; a.N = h->d.N; a.NX = h->d.nx; a.NU = h->d.nu; a.Xn = h->Xn; a.Un = h->Un; a.xmeas = h->xmeas; a.primal = h->primal;
    a.success = h->success; a.x0arg = h->x0arg; a.E = h->E; a.w = w; a.u0 = h->u0; a.u_init = h->u_init;
    return a;
}
// run: the instances that are tightened (NULL = all); write_ubg: the tightened rows go into the QP's bounds (a solve) or only into the back-offs (slsqp_sweep)
static TightenArgs tighten_args(slsqp_handle *h, const int *run, int write_ubg) {
    return TightenArgs{h->B, h->d.N, h->d.nx, h->d.nu, h->d.ni, h->d.ni_f, h->beta, h->beta_f, h->g, h->gf_raw, h->c, run, h->backoff, h->backoff_f, h->backoff_x, h->backoff_u, h->ubg, write_ubg, h->ct_part, h->cost_tube};
}
static SweepArgs sweep_args(slsqp_handle *h, const int *run, const double *eta, const double *eta_f, double eps) {
    return SweepArgs{h->B, h->d.N, h->d.nw, h->A, h->Bm, h->E, 0, eta, eta_f, run, costs_of(h), h->K, h->beta, h->beta_f, h->ct_part, eps};
}
// rti: RTI mode (no count of the instances that go on); first: first iteration of the solve (the beta repair); shared_cols: beta = eps in every
// column, evaluate_dual_eta writes column 0 only
static AfterQpArgs after_qp_args(slsqp_handle *h, const slsqp_opts &o, const int *active, int rti, int first, int shared_cols) {
    const EtaArgs ea{h->B, h->d.N, h->d.nx, h->d.ni, h->d.ni_f, h->dual, h->beta, h->beta_f, h->alive, h->eta, h->eta_f, o.eps_backoff, h->stale, shared_cols};
    const ConvArgs ca{h->B, h->n, h->primal, h->prev_primal, h->has_prev, h->alive, h->conv, o.conv_tol};
    return AfterQpArgs{h->B, rti, first, h->status, active, h->alive, h->infeas, h->mask, h->success, h->itnum, h->counter, h->stale, h->conv, ea, ca, h->beta, h->beta_f};
}
// run: the instances whose back-offs are reset (NULL = all); fill_beta: beta = eps too (the handle's first solve)
static InitBackoffArgs init_backoff_args(slsqp_handle *h, const slsqp_opts &o, const int *run, int fill_beta) {
    return InitBackoffArgs{h->B, h->d.N, h->d.nx, h->d.nu, o.eps_backoff, run, h->beta, h->beta_f, h->backoff, h->backoff_f, h->backoff_x, h->backoff_u, fill_beta};
}
// x0: the device array the pin value is taken from, or NULL when it has been written already; skip_begin: instances in the middle of a solve (slsqp_cl_run's rounds)
static SolveBeginArgs solve_begin_args(slsqp_handle *h, const slsqp_opts &o, const double *x0, const int *active, const int *skip_begin) {
    return SolveBeginArgs{h->B, h->d.nx, x0, h->x0val, active, h->alive, h->infeas, h->success, h->pending_reset, h->itnum, h->stale,
                          h->eta, h->eta_f, (size_t)h->d.N * h->d.N * h->d.ni, (size_t)(h->d.N + 1) * h->d.ni_f, init_backoff_args(h, o, active, 0), skip_begin};
}
// X, U: the device trajectory that is linearised; run: the instances it is done for (NULL = all)
static LinArgs lin_args(slsqp_handle *h, const double *X, const double *U, const int *run) {
    return LinArgs{h->B, h->d.N, X, U, h->g_raw, h->gf_raw, costs_of(h), h->A, h->Bm, h->c, h->g, h->gN, h->q, run, h->lin_stage, h->lin_tape};
}
static BoundsArgs bounds_args(slsqp_handle *h, const int *run) {
    return BoundsArgs{h->B, h->d.N, h->d.nx, h->d.ni, h->d.ni_f, h->g, h->gN, h->c, h->ubg, h->lbg, 1e-10, run};
}
// the log entry: stepno[b] for the instances of mask (NULL = all), or `step` for everybody with stepno = NULL
static ClLogArgs cl_log_args(slsqp_handle *h, const int *stepno, const int *mask, int step) {
    return ClLogArgs{stepno, mask, h->B, h->d.N, h->d.nx, h->d.nu, h->log_steps, step, h->Xn, h->Un, h->backoff_x, h->backoff_u, h->scp_success, h->scp_iters,
                     h->pinf, h->lg_x, h->lg_u, h->lg_bx, h->lg_bu, h->lg_state, h->lg_u0, h->lg_pinf, h->lg_succ, h->lg_it};
}
static ScpArgs scp_args(slsqp_handle *h, const slsqp_opts &o, int it, int converge) {
    return ScpArgs{it, converge, o.scp_eps, h->scp_active, h->scp_success, h->scp_iters, h->counter + 2, h->scp_dmax, h->scp_upd};
}
// dynamic LDS of a wave that runs a whole chain (k_rti_chain, the persistent loops): the largest of its parts' work areas
template <int NX, int NU>
static size_t chain_lds_bytes(const slsqp_handle *h) {
    return sizeof(double) * std::max({(size_t)qp_lds_doubles<NX, NU>(h->d.N), (size_t)(2 * h->n + 8), (size_t)sweep_lds_doubles<NX, NU>(), (size_t)sweep_prop_lds_doubles<NX, NU>()});
}
// a launch between a pair of kev events, when opts.time_kernels asks for it and there is room (harvest_kernel_events reads them)
template <class F>
static void timed_launch(slsqp_handle *h, F &&launch) {
    const bool timed = h->time_kernels && h->n_kev + 2 <= (int)h->kev.size();
    if (timed) hipEventRecord(h->kev[h->n_kev], h->st);
    launch();
    if (timed) { hipEventRecord(h->kev[h->n_kev + 1], h->st); h->n_kev += 2; }
}

// ---- kernel dispatch ---------------------------------------------------------------------------------------
// ticks a QP solve may take: 1 (start) + 2 per interior-point iteration + (1 + n_refine) per polish round, after at most warm_rounds + as_rounds
// active-set rounds of the attempts that precede the interior point
static int qp_max_ticks(const QpArgs &a, int max_iter) { return 1 + 2 * max_iter + 3 + 2 * 10 + 8 + 2 + 16 + 2 * (a.warm_rounds + a.as_rounds + 2); }
template <int NX, int NU>
static int launch_qp_t(slsqp_handle *h, const QpArgs &a, int max_iter, bool mx) {
    // the LDS of a QP wave also holds two n-vectors of the phase logic between the sweeps (phase_update, fused look)
    const size_t lds = std::max(mx ? QpLdsMx<NX, NU>::BYTES : sizeof(double) * (size_t)qp_lds_doubles<NX, NU>(h->d.N), sizeof(double) * (size_t)(2 * h->n + 8));
    const dim3 grid(h->B), blk(64);
    const int max_ticks = qp_max_ticks(a, max_iter);
    // one launch per QP solve: every wave runs its instance to completion (k_qp_solve)
    timed_launch(h, [&] { with_flag(mx, [&](auto MX) { hipLaunchKernelGGL((k_qp_solve<NX, NU, MX()>), grid, blk, lds, h->st, a, max_ticks); }); });
    HIPCHK(hipGetLastError());
    return 0;
}

// kernel events recorded by launches that did not wait for their kernels (k_qp_solve): read once the stream has been synchronised
static void harvest_kernel_events(slsqp_handle *h) {
    for (int i = 0; i + 1 < h->n_kev; i += 2) { float ms = 0; if (hipEventElapsedTime(&ms, h->kev[i], h->kev[i + 1]) == hipSuccess) { h->t_fwd += ms; h->n_fwd++; } }
    h->n_kev = 0;
}

// Non-finite QP data of an instance, checked by passes of their own around a QP launch (folded into the QP kernels' setup, the check cost them
// registers and 7 % of the closed-loop step): a NaN in q, in a box row or in a dynamics row, or +-inf in q or in a dynamics row (c).  +-inf in a box
// row is no bound, like 1e20.  A NaN or +-inf in A or B as well.  Such an instance cannot certify (its solve is NaN, and the look and the certificate keep NaN), so it ends
// unsolved and takes no part in the launch (its previous primal / dual stay); k_apply_nonfinite then records it as status 3, with the qp_stats of a flagged instance.  With a
// NaN or infinite |q|inf every tolerance max(1,|q|inf) would be meaningless.
__global__ __launch_bounds__(64) void k_flag_nonfinite(int n, int mb, int NX, int SR, int Ndyn, int nAB, const double *q, const double *ubg, const double *lbg,
                                                        const double *A, const double *Bm, int nA, const int *run, int *bad, int *runq, int *alive, int *infeas) {
    const int b = blockIdx.x;
    int f = 0;
    for (int e = threadIdx.x; e < n; e += 64) f |= !(fabs(q[(size_t)b * n + e]) < INFINITY);
    for (int e = threadIdx.x; e < nAB; e += 64) f |= !(fabs(e < nA ? A[(size_t)b * nA + e] : Bm[(size_t)b * (nAB - nA) + e - nA]) < INFINITY);
    for (int r = threadIdx.x; r < mb; r += 64) {
        const double u = ubg[(size_t)b * mb + r], l = lbg[(size_t)b * mb + r];
        if (r < Ndyn && r % SR < NX) f |= !(fabs(u) < INFINITY) | !(fabs(l) < INFINITY);
        else f |= (u != u) | (l != l);
    }
    f = __syncthreads_or(f);
    if (threadIdx.x == 0) {
        bad[b] = f; runq[b] = (run ? run[b] : 1) && !f;
        if (f && alive) { alive[b] = 0; infeas[b] = 1; }      // (the fused chain: the instance takes no part, its call fails)
    }
}
__global__ void k_apply_nonfinite(int B, const int *bad, const int *run, int *status, int *qpstat, int stat_slot) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || !bad[b] || (run && !run[b])) return;
    status[b] = 3;
    int *qs = qpstat + ((size_t)b * 2 + stat_slot) * 8;
    for (int i = 0; i < 8; i++) qs[i] = 0;
    qs[6] = 3;
}
static void apply_nonfinite(slsqp_handle *h, const int *run, int stat_slot) {
    hipLaunchKernelGGL(k_apply_nonfinite, dim3((h->B + 255) / 256), dim3(256), 0, h->st, h->B, h->databad, run, h->status, h->qpstat, stat_slot);
}
static void flag_nonfinite(slsqp_handle *h, const int *run, int *alive = nullptr, int *infeas = nullptr) {
    const int SR = h->d.nx + h->d.ni;
    const int nA = h->d.N * h->d.nx * h->d.nx, nAB = nA + h->d.N * h->d.nx * h->d.nu;
    hipLaunchKernelGGL(k_flag_nonfinite, dim3(h->B), dim3(64), 0, h->st, h->n, h->mb, h->d.nx, SR, h->d.N * SR, nAB, h->q, h->ubg, h->lbg, h->A, h->Bm, nA, run, h->databad, h->runq, alive, infeas);
}

// instances of `run` whose mixed-precision solve did not end on the KKT certificate are solved again in fp64
__global__ void k_mark_retry(int B, const int *run, const int *status, int *retry, int *count) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int r = (!run || run[b]) && status[b] != 0 && status[b] != 2 && status[b] != 5;      // (2, 5: infeasible for either arithmetic)
    retry[b] = r;
    if (r) atomicAdd(count, 1);
}

// the tolerance of the x0 gate (slsqp_set_x0_box_tol) goes to the device word the QP kernels read it from (x0_record), on the handle's stream, when
// it differs from what is there: the default (0, what the allocation holds) never launches anything
static void set_x0_tol(slsqp_handle *h, double tol) {
    if (!(tol > 0.0)) tol = 0.0;      // (negative or NaN: strict)
    if (tol == h->x0_tol_dev) return;
    hipLaunchKernelGGL(k_fill_doubles, dim3(1), dim3(64), 0, h->st, x0_record(h->kkt, h->B), tol, (size_t)1);
    h->x0_tol_dev = tol;
}

// What one QP of a call asks for: warm start, the nominal initialiser's proximal weights (B, 12) or NULL, the statistics slot, whether the interior point's iterate
// is copied (snap_take) and may be restarted from (snap_use), whether the warm set moves one stage on with the horizon
struct QpCall { int warm = 0; const double *prox = nullptr; int stat_slot = 0, snap_take = 0, snap_use = 0, warm_shift = 0; };
// the first and the last QP of a fast-SLS call
static QpCall qp_first_call(int warm, int warm_shift) { QpCall c; c.warm = warm; c.snap_take = 1; c.warm_shift = warm_shift; return c; }
static QpCall qp_last_call(int warm_shift) { QpCall c; c.warm = 1; c.stat_slot = 1; c.snap_take = 1; c.snap_use = 1; c.warm_shift = warm_shift; return c; }
// what the last QP of a call changes in the first one's arguments (make_qp_args with qp_last_call: warm, statistics slot 1, restart from the first QP's iterate copy)
static Qp2Ints qp_second_ints(const slsqp_opts &o) { const QpCall l = qp_last_call(0); return Qp2Ints{l.warm, l.stat_slot, (l.snap_use && o.ipm_restart) ? 1 : 0}; }
// the tolerance of the x0 gate a launch with these arguments asks for (set_x0_tol): the nominal initialiser's QPs (prox) stay strict
static double qp_x0_tol(const slsqp_handle *h, const QpCall &c) { return c.prox ? 0.0 : h->x0_box_tol; }

static QpArgs make_qp_args(slsqp_handle *h, const int *run, const slsqp_opts *o, const QpCall &c) {
    QpArgs a;
    memset(&a, 0, sizeof a);      // (padding too: the closed-loop kernels' argument block is compared and copied as bytes)
    a.qpstat = h->qpstat; a.stat_slot = c.stat_slot; a.diag = h->qp_diag;
    static const double snap_mu = getenv("SLSQP_SNAP_MU") ? atof(getenv("SLSQP_SNAP_MU")) : 1e-3;
    a.snap_take = c.snap_take; a.snap_use = c.snap_use && o->ipm_restart; a.snap_mu = snap_mu; a.call_id = h->call_id; a.call_ids = h->cl_round ? h->call_ids : nullptr; a.as_first = o->as_first; a.as_rounds = o->as_rounds; a.as_max_viol = o->as_max_viol; a.as_warm_max_set = o->as_warm_max_set; a.as_warm_last = o->as_warm_last;
    { static const double pe = getenv("SLSQP_PINF_EPS") ? atof(getenv("SLSQP_PINF_EPS")) : 1e-4; a.pinf_eps = pe; }
    { static const int ws = getenv("SLSQP_WARM_SHIFT") ? atoi(getenv("SLSQP_WARM_SHIFT")) : 1; a.warm_shift = ws ? c.warm_shift : 0; a.shift_stepno = nullptr; }
    a.prox = c.prox; a.prox_stride = 12; a.inst_launches = h->inst_launches;
    a.B = h->B; a.N = h->d.N; a.A = h->A; a.Bm = h->Bm; a.q = h->q; a.ubg = h->ubg; a.lbg = h->lbg; a.x0val = h->x0val; a.run = run;
    a.cst = costs_of(h); a.Linv = h->Linv; a.ws = h->ws; a.primal = h->primal; a.dual = h->dual; a.cost = h->cost; a.pin_dual = h->pin_dual; a.kkt = h->kkt;
    a.status = h->status; a.iters = h->iters; a.max_iter = o->qp_max_iter; a.eps = o->qp_eps;
    a.state = h->qpstate; a.warm = c.warm; a.warm_rounds = o->warm_rounds;
    a.init_s = getenv("SLSQP_INIT_S") ? atof(getenv("SLSQP_INIT_S")) : 1.0; a.init_lam = getenv("SLSQP_INIT_LAM") ? atof(getenv("SLSQP_INIT_LAM")) : 0.0;
    const bool mx = o->precision == 1;
    a.n_refine = mx ? 3 : 1;   // fp64: one refinement solve; its forward sweep measures the dynamics residual of the first solve (certificate)
    if (getenv("SLSQP_NREFINE")) a.n_refine = atoi(getenv("SLSQP_NREFINE"));
    // tolerance (relative to max(1, |q|inf)) of the look at an un-refined active-set solve.  fp64: the un-refined solve is good to ~1e-11, so the look can
    // use nearly the certificate's own 1e-9 -- with 1e-6 (rounds 1 and 2) violations and wrong-sign multipliers between 1e-9 and 1e-6 went unnoticed until
    // the refined solve's certificate check, and each of those late corrections cost a refinement solve and a fresh factorisation: 9.2 / 11.0 block solves per
    // QP of the rocket loop against 5.9 / 8.0 with 1e-8 (same certified fractions; the numpy prototype of the iteration needs 3.95 rounds, the GPU now 3.8 / 4.7)
    a.early_ctol = mx ? 1e-2 : 1e-8;
    if (!mx && getenv("SLSQP_EARLY_CTOL")) a.early_ctol = atof(getenv("SLSQP_EARLY_CTOL"));      // (experiments)
    return a;
}

// ---- the multi-wave path (slsqp_mw.hpp): one workgroup of solve_waves waves per instance -------------------------
static int ensure_cr(slsqp_handle *h) {
    if (h->cr) return 0;
    return dalloc(h->owned, &h->cr, (size_t)h->B * h->d.N * 3 * h->d.nx * h->d.nx);
}
// LDS of a multi-wave workgroup: the work areas of the reduction, or the two n-vectors of the phase logic (wave 0, between the block solves)
template <int NX, int NU>
static size_t mw_lds_bytes(const slsqp_handle *h, int W) {
    return sizeof(double) * std::max((size_t)MwLds<NX, NU>::total(h->d.N, W), (size_t)(2 * h->n + 8));
}
// more than 64 KB of dynamic LDS (quadrotor and rocket with 8 waves) has to be asked for.  The attribute belongs to the function on the CURRENT device, so it
// is set before every launch (a host-side table write), not once per process: handles on several devices share this code
template <typename K>
static int allow_lds(K kernel) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    return 0;
}
template <int NX, int NU>
static int launch_qp_mw_t(slsqp_handle *h, const QpArgs &a, int max_iter) {
    if (ensure_cr(h) || allow_lds(k_qp_solve_mw<NX, NU>)) return -1;
    const int W = h->solve_waves;
    const size_t lds = mw_lds_bytes<NX, NU>(h, W);
    if (lds > 160 * 1024) return fail("solve_waves: the work areas of that many waves do not fit the LDS for this horizon");
    const int max_ticks = qp_max_ticks(a, max_iter);
    timed_launch(h, [&] { hipLaunchKernelGGL((k_qp_solve_mw<NX, NU>), dim3(h->B), dim3(64 * W), lds, h->st, a, max_ticks, h->cr, W); });
    HIPCHK(hipGetLastError());
    return 0;
}
// the stored factorisations of every instance are forgotten (the two paths keep theirs in different scratch buffers and layouts): the next
// solve of each instance factorises.  Warm sets and everything else in QpState stay.
__global__ void k_forget_factors(int B, double *state) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    QpState *st = (QpState *)state + b;
    st->fact_call = 0.0; st->uf_valid = 0.0;
}
static void forget_factors(slsqp_handle *h) { hipLaunchKernelGGL(k_forget_factors, dim3((h->B + 255) / 256), dim3(256), 0, h->st, h->B, h->qpstate); }

// what the multi-wave path does not serve is refused at the entry points, before anything is launched or a timeline interval is begun
static int mw_refuse(const slsqp_handle *h, const slsqp_opts &o) {
    if (h->solve_waves > 1 && o.precision == 1) return fail("solve_waves > 1: the multi-wave QP kernel is fp64 only (precision = 1 needs solve_waves = 1)");
    return 0;
}

// one QP solve of the instances of `run` (NULL = all), on the multi-wave or the single-wave kernel
static int launch_qp(slsqp_handle *h, const int *run, const slsqp_opts *o, const QpCall &c) {
    h->ne_waves = 0;      // (this launch overwrites the factor buffers: slsqp_ne_solve(factor = 0) may not substitute with them)
    if (mw_refuse(h, *o)) return -1;
    flag_nonfinite(h, run);
    set_x0_tol(h, qp_x0_tol(h, c));
    const QpArgs a = make_qp_args(h, h->runq, o, c);
    h->time_kernels = o->time_kernels != 0;
    h->mx_retry = 0;
    const bool mw = h->solve_waves > 1, mx = o->precision == 1;      // (never both: mw_refuse)
    auto go = [&](const QpArgs &q, bool m) {
        return with_dims(h, [&](auto NX, auto NU) { return mw ? launch_qp_mw_t<NX(), NU()>(h, q, o->qp_max_iter) : launch_qp_t<NX(), NU()>(h, q, o->qp_max_iter, m); });
    };
    if (go(a, mx)) return -1;
    if (mx) {
        HIPCHK(hipMemsetAsync(h->counter + 3, 0, sizeof(int), h->st));
        hipLaunchKernelGGL(k_mark_retry, dim3((h->B + 255) / 256), dim3(256), 0, h->st, h->B, a.run, h->status, h->retry, h->counter + 3);
        int nretry = 0;
        HIPCHK(hipMemcpyAsync(&nretry, h->counter + 3, sizeof(int), hipMemcpyDeviceToHost, h->st));
        HIPCHK(hipStreamSynchronize(h->st));
        h->mx_retry = nretry; h->mx_retry_total += nretry;
        if (nretry > 0) {
            QpArgs r = a;
            r.run = h->retry; r.warm = 0; r.n_refine = 1; r.early_ctol = 1e-6; r.snap_take = 0; r.snap_use = 0;
            if (go(r, false)) return -1;
        }
    }
    apply_nonfinite(h, run, c.stat_slot);
    return 0;
}

template <int NX, int NU>
static int launch_sweep_gen_t(slsqp_handle *h, const SweepArgs &a) {
    const size_t lds = sizeof(double) * sweep_gen_lds_doubles<NX, NU>();
    hipLaunchKernelGGL((k_sweep_gen<NX, NU>), dim3(h->B * (h->d.N + 1)), dim3(64), lds, h->st, (SweepGenArgs{a, h->Gd, h->Gfd, h->d.ni, h->d.ni_f}));
    HIPCHK(hipGetLastError());
    return 0;
}
template <int NX, int NU>
static int launch_sweep_t(slsqp_handle *h, const SweepArgs &a) {
    const size_t lds = sizeof(double) * sweep_lds_doubles<NX, NU>();
    hipLaunchKernelGGL((k_sweep<NX, NU>), dim3(h->B * (h->d.N + 1)), dim3(64), lds, h->st, a);
    HIPCHK(hipGetLastError());
    return 0;
}
template <int NX, int NU>
static int launch_sweep_shared_t(slsqp_handle *h, const SweepArgs &a) {
    SweepSharedArgs aa{a, h->Kc, h->Aclc, h->stale};
    const size_t lds_ric = sizeof(double) * sweep_lds_doubles<NX, NU>(), lds_prop = sizeof(double) * sweep_prop_lds_doubles<NX, NU>();
    hipLaunchKernelGGL((k_sweep_ric1<NX, NU>), dim3(h->B), dim3(64), lds_ric, h->st, aa);
    hipLaunchKernelGGL((k_sweep_prop<NX, NU>), dim3(h->B * ((h->d.N + 2) / 2)), dim3(64), lds_prop, h->st, aa);      // one wave per pair of disturbance columns
    HIPCHK(hipGetLastError());
    return 0;
}
static bool sweep_shared_allowed() { static const bool v = getenv("SLSQP_SWEEP_SHARED") ? atoi(getenv("SLSQP_SWEEP_SHARED")) != 0 : true; return v; }
// shared_cols: every column's eta is the same (first fast-SLS iteration after initialize_backoff): one Riccati recursion per instance
static int launch_sweep(slsqp_handle *h, const int *run, const double *eta, const double *eta_f, double eps, bool shared_cols = false) {
    const SweepArgs a = sweep_args(h, run, eta, eta_f, eps);
    return with_dims(h, [&](auto NX, auto NU) {
        if (h->general_G) return launch_sweep_gen_t<NX(), NU()>(h, a);
        if (shared_cols && sweep_shared_allowed()) return launch_sweep_shared_t<NX(), NU()>(h, a);
        return launch_sweep_t<NX(), NU()>(h, a);
    });
}

// arguments of one RTI chain (k_rti_chain / k_cl_loop): QP #1, what follows it, the sweep, the tightening, QP #2 (memset first: part of the persistent kernels' block)
static ChainArgs make_chain_args(slsqp_handle *h, const slsqp_opts &o, const int *active, int wshift) {
    ChainArgs c;
    memset(&c, 0, sizeof c);
    c.q = make_qp_args(h, h->alive, &o, qp_first_call(o.warm_start ? 1 : 0, wshift));
    c.q2 = qp_second_ints(o);
    c.aq = after_qp_args(h, o, active, /* rti */ 1, /* first */ 1, /* shared_cols */ 1);
    c.sw = SweepSharedArgs{sweep_args(h, h->mask, h->eta, h->eta_f, o.eps_backoff), h->Kc, h->Aclc, h->stale};
    c.ta = tighten_args(h, h->mask, 1);
    c.active = active; c.success = h->success; c.infeas = h->infeas; c.times = h->chain_times;
    c.max_ticks = qp_max_ticks(c.q, o.qp_max_iter);
    c.cut_count = 0xFFFFFFFFu;      // (lag, runm, done, t0word, budget, fin_count, the per-step log: NULL / 0, slsqp_cl_run's callers set them)
    return c;
}

// the fused RTI chain (k_rti_chain): one launch for QP #1 -> eta -> shared Riccati + propagation -> tightened bounds -> QP #2
template <int NX, int NU>
static int launch_chain_t(slsqp_handle *h, ChainArgs &c, const BndArgs *bd) {
    const size_t lds = chain_lds_bytes<NX, NU>(h);
    h->ne_waves = 0;      // (slsqp_ne_solve's factors do not survive a QP solve)
    timed_launch(h, [&] { with_flag(bd != nullptr, [&](auto BND) { hipLaunchKernelGGL((k_rti_chain<NX, NU, BND()>), dim3(h->B), dim3(64), lds, h->st, c, bd ? *bd : BndArgs{}); }); });
    HIPCHK(hipGetLastError());
    return 0;
}
// the tightening as a launch of its own: bd as for launch_chain_t
static void launch_tighten(slsqp_handle *h, const TightenArgs &ta, const BndArgs *bd) {
    with_flag(bd != nullptr, [&](auto BND) { hipLaunchKernelGGL((k_tighten<BND()>), dim3(h->B), dim3(128), 0, h->st, ta, bd ? *bd : BndArgs{}); });
}
static bool chain_allowed() { static const bool v = getenv("SLSQP_FUSE_RTI") ? atoi(getenv("SLSQP_FUSE_RTI")) != 0 : true; return v; }

static float ev_ms(hipEvent_t a, hipEvent_t b) { float ms = 0; hipEventElapsedTime(&ms, a, b); return ms; }

// `active` (device, B ints or NULL = all): instances that take part in this call; the others keep every result array untouched.
// ---- timeline of a solve / closed-loop step: event pairs with a role, summed once the stream has been synchronised ----
static int tl_begin(slsqp_handle *h, int role) {
    if (h->tl_n >= (int)h->tl_role.size()) return -1;          // full: this interval goes untimed (flush points keep that from happening)
    const int i = h->tl_n++;
    h->tl_role[i] = role;
    hipEventRecord(h->tl[2 * i], h->st);
    return i;
}
static void tl_end(slsqp_handle *h, int i) { if (i >= 0) hipEventRecord(h->tl[2 * i + 1], h->st); }
// only right after a stream synchronisation: add the recorded intervals to the accumulators, recycle the events
static void tl_flush(slsqp_handle *h) {
    for (int i = 0; i < h->tl_n; i++) { float ms = 0; if (hipEventElapsedTime(&ms, h->tl[2 * i], h->tl[2 * i + 1]) == hipSuccess) h->tl_acc[h->tl_role[i]] += ms; }
    h->tl_n = 0;
    harvest_kernel_events(h);
}
static void tl_take(slsqp_handle *h) {     // accumulators -> the handle's timing fields (what slsqp_last_timing reports)
    tl_flush(h);
    h->t_qp = h->tl_acc[0]; h->t_sweep = h->tl_acc[1]; h->t_total = h->tl_acc[2]; h->t_jac = h->tl_acc[3];
    if (h->tl_acc[4] > 0.0) {
        // fused RTI chain launches: no batch-wide "QP time" / "sweep time" exists any more.  Reported: the sweep part as instance 0 spent it inside
        // the kernel (wall clock, 100 MHz; what the reference's single-instance t_backward_ms measures), the rest of the launches' duration as QP time
        double sw = 0.0;
        if (h->chain_times_host) sw = std::min(h->tl_acc[4], (double)h->chain_times_host[1] * 1e-5);
        h->t_sweep += sw; h->t_qp += h->tl_acc[4] - sw;
    }
    h->tl_acc[0] = h->tl_acc[1] = h->tl_acc[2] = h->tl_acc[3] = h->tl_acc[4] = 0;
}
// the tail of an entry point whose work is enqueued: return (no_sync: the caller synchronises the stream later and then calls tl_take), or wait and take the timeline
static int finish_enqueued(slsqp_handle *h, bool no_sync) {
    if (no_sync) return 0;
    HIPCHK(hipStreamSynchronize(h->st));
    tl_take(h);
    return 0;
}

// no_sync: finish_enqueued
// bd: the bounds whose window gives the tightening's terminal row (the closed-loop entry points of a handle with bounds), or NULL: the model's gf
// (slsqp_solve brings its own g and always passes NULL)
static int solve_impl(slsqp_handle *h, const double *x0, int loc, const slsqp_opts *opts, const int *active, bool no_sync = false, const BndArgs *bd = nullptr) {
    hipSetDevice(h->dev);
    if (h->general_G) return fail("general G: only the sweep-level boundary (slsqp_sweep) is available; the QP solver needs box constraints G = [I;-I]");
    if (!h->have_costs || !h->have_cons || !h->have_dyn) return fail("set_costs, set_constraints and update_dynamics must be called first");
    slsqp_opts o;
    if (opts) o = *opts; else slsqp_default_opts(&o);
    if (mw_refuse(h, o)) return -1;
    const slsqp_dims &d = h->d;
    const int B = h->B, gb = (B + 255) / 256;
    // x_0 is pinned to -x0 (qp_jit.py:376-379)
    if (loc == SLSQP_HOST) {
        std::vector<double> neg((size_t)B * d.nx);
        for (size_t i = 0; i < neg.size(); i++) neg[i] = -x0[i];
        HIPCHK(hipMemcpyAsync(h->x0val, neg.data(), neg.size() * sizeof(double), hipMemcpyHostToDevice, h->st));
        HIPCHK(hipStreamSynchronize(h->st));
    } else if (!h->beta_inited) {
        hipLaunchKernelGGL(k_negate, dim3((B * d.nx + 255) / 256), dim3(256), 0, h->st, x0, h->x0val, B * d.nx);
    }
    const bool rti = o.rti_steps > 0;
    const int steps = rti ? o.rti_steps : o.max_sls_iter;
    h->call_id += 1.0;
    // the caller moved the horizon one stage on since the last solve (slsqp_cl_step's reset_warm_start): the first QP's warm set moves with it
    const int wshift = h->horizon_shifted; h->horizon_shifted = 0;
    const int tl_tot = tl_begin(h, 2);
    if (h->beta_inited) {     // every solve but the handle's first: the whole preamble in one launch
        hipLaunchKernelGGL(k_solve_begin, dim3(B), dim3(256), 0, h->st, solve_begin_args(h, o, loc == SLSQP_HOST ? nullptr : x0, active, h->cl_skip_begin));
    } else {
        if (active) hipLaunchKernelGGL(k_copy_int, dim3(gb), dim3(256), 0, h->st, active, h->alive, B);
        else hipLaunchKernelGGL(k_fill_int, dim3(gb), dim3(256), 0, h->st, h->alive, 1, B);
        hipLaunchKernelGGL(k_apply_pending_reset, dim3(B), dim3(256), 0, h->st, B, h->pending_reset, active, h->itnum, h->eta, (size_t)d.N * d.N * d.ni, h->eta_f,
                           (size_t)(d.N + 1) * d.ni_f, h->stale);
        hipLaunchKernelGGL(k_fill_int, dim3(gb), dim3(256), 0, h->st, h->infeas, 0, B);
        hipLaunchKernelGGL(k_fill_int, dim3(gb), dim3(256), 0, h->st, h->success, 0, B);
        // initialize_backoff at the top of every solve (fast_SLS_jit.py:281,299).  The first solve of a handle fills beta for every instance (also the
        // ones outside `active`: later calls rely on it), but their back-off arrays must stay untouched: the fill is launches of its own then
        if (active) {
            hipLaunchKernelGGL(k_fill_doubles, dim3(1024), dim3(256), 0, h->st, h->beta, o.eps_backoff, (size_t)B * d.N * d.N * d.ni);
            hipLaunchKernelGGL(k_fill_doubles, dim3(1024), dim3(256), 0, h->st, h->beta_f, o.eps_backoff, (size_t)B * (d.N + 1) * d.ni_f);
            hipLaunchKernelGGL(k_init_backoff, dim3(B), dim3(256), 0, h->st, init_backoff_args(h, o, active, 0));
        } else hipLaunchKernelGGL(k_init_backoff, dim3(B), dim3(256), 0, h->st, init_backoff_args(h, o, nullptr, 1));
        h->beta_inited = true;
    }
    // (small batches keep the separate launches: there the SLS propagation of an instance runs as N + 1 waves side by side, which is what a B = 1 caller
    // waits for -- 1.1 against 1.6 ms per rocket RTI step -- while from ~150 instances on the columns of one instance would only compete with other
    // instances' for the same SIMDs.  fuse_rti = 2 forces the chain, slsqp_cl_run always uses it.)
    const bool fuse_here = o.fuse_rti == 2 || h->cl_round || (o.fuse_rti == 1 && (long)B * (d.N + 1) >= 3072);
    if (rti && steps == 1 && o.precision == 0 && fuse_here && h->solve_waves == 1 && chain_allowed() && sweep_shared_allowed() && !h->general_G) {
        // fast_SLS.solve with rti_steps = 1 (the rocket script's setting) as ONE launch: every wave takes its instance through the whole chain
        h->time_kernels = o.time_kernels != 0;
        set_x0_tol(h, h->x0_box_tol);
        ChainArgs c = make_chain_args(h, o, active, wshift);
        if (h->cl_round) {      // a round of slsqp_cl_run: suspended solves resume, unfinished ones suspend at the deadline
            c.lag = h->cl_lag; c.runm = h->cl_runm; c.done = h->cl_done; c.t0word = h->t0word; c.budget = h->cl_budget;
            c.qplog = h->qplog; c.x0vlog = h->x0vlog; c.stepno = h->cl_stepno; c.log_steps = h->qplog_steps;
            c.fin_count = (unsigned *)(h->t0word + 1); c.cut_count = h->cl_cut_count;
            HIPCHK(hipMemsetAsync(h->t0word, 0, 2 * sizeof(unsigned long long), h->st));
        } else flag_nonfinite(h, active, h->alive, h->infeas);      // (slsqp_cl_run's rounds and k_cl_loop linearise their own data; the NaN-keeping certificate guards them)
        const int tl_c = tl_begin(h, 4);
        if (with_dims(h, [&](auto NX, auto NU) { return launch_chain_t<NX(), NU()>(h, c, bd); })) return -1;
        if (!h->cl_round) apply_nonfinite(h, active, 0);      // (an instance flagged at QP #1 never reaches QP #2)
        tl_end(h, tl_c);
        if (h->chain_times_host) HIPCHK(hipMemcpyAsync(h->chain_times_host, h->chain_times, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->st));
        tl_end(h, tl_tot);
        return finish_enqueued(h, no_sync);
    }
    for (int i = 0; i < steps; i++) {
        const int tl_q = tl_begin(h, 0);
        QpCall qc = qp_first_call((i > 0 || o.warm_start) ? 1 : 0, i == 0 ? wshift : 0);
        qc.snap_use = i > 0 ? 1 : 0;
        if (launch_qp(h, h->alive, &o, qc)) return -1;
        tl_end(h, tl_q);
        // flags after the QP, evaluate_dual_eta, check_convergence_socp, masks and (first iteration) the beta repair: one launch
        if (!rti) HIPCHK(hipMemsetAsync(h->counter, 0, sizeof(int), h->st));      // (the count of instances that go on is only read in converge mode)
        hipLaunchKernelGGL(k_after_qp, dim3(B), dim3(256), 0, h->st, after_qp_args(h, o, active, rti ? 1 : 0, i == 0 ? 1 : 0, (i == 0 && sweep_shared_allowed()) ? 1 : 0));
        const int tl_s = tl_begin(h, 1);
        if (launch_sweep(h, h->mask, h->eta, h->eta_f, o.eps_backoff, /* beta == eps for every column right after initialize_backoff */ i == 0)) return -1;
        tl_end(h, tl_s);
        launch_tighten(h, tighten_args(h, h->mask, 1), bd);
        if (rti) continue;      // RTI mode (every closed-loop script): nothing to decide on the host, the stream runs on
        int nmask = 0;
        HIPCHK(hipMemcpyAsync(&nmask, h->counter, sizeof(int), hipMemcpyDeviceToHost, h->st));
        HIPCHK(hipStreamSynchronize(h->st));
        if (nmask == 0) break;   // every instance converged or failed
    }
    // final QP: RTI always (fast_SLS_jit.py:293); converge mode only for instances that hit MAX_ITER (:311)
    const int tl_q2 = tl_begin(h, 0);
    if (launch_qp(h, h->alive, &o, qp_last_call(wshift))) return -1;
    tl_end(h, tl_q2);
    hipLaunchKernelGGL(k_finish, dim3(gb), dim3(256), 0, h->st, B, rti ? 1 : 0, h->alive, h->infeas, h->success, active, h->pending_reset);
    tl_end(h, tl_tot);
    return finish_enqueued(h, no_sync);
}

extern "C" int slsqp_solve(slsqp_handle *h, const double *x0, int loc, const slsqp_opts *opts) { return solve_impl(h, x0, loc, opts, nullptr); }

extern "C" int slsqp_last_timing(slsqp_handle *h, double *ms5, int len) {
    if (!ms5 || len < SLSQP_TIMING_LEN) return fail("slsqp_last_timing: the buffer must hold SLSQP_TIMING_LEN (5) doubles");
    if (h->tl_n > 0) { hipSetDevice(h->dev); hipStreamSynchronize(h->st); tl_take(h); }
    ms5[0] = h->t_total; ms5[1] = h->t_qp; ms5[2] = h->t_sweep; ms5[3] = h->t_total - h->t_qp - h->t_sweep; ms5[4] = h->t_jac;
    return 0;
}
extern "C" int slsqp_kernel_timing(slsqp_handle *h, double *out8, int len) {
    if (!out8 || len < SLSQP_KERNEL_TIMING_LEN) return fail("slsqp_kernel_timing: the buffer must hold SLSQP_KERNEL_TIMING_LEN (8) doubles");
    unsigned long long il[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    hipSetDevice(h->dev);
    hipMemcpyAsync(il, h->inst_launches, sizeof(il), hipMemcpyDeviceToHost, h->st);
    hipMemsetAsync(h->inst_launches, 0, sizeof(il), h->st);
    hipStreamSynchronize(h->st);
    if (h->tl_n > 0) tl_take(h); else harvest_kernel_events(h);
    out8[0] = h->t_fwd; out8[1] = (double)h->n_fwd; out8[2] = (double)h->mx_retry_total; out8[3] = (double)il[0]; out8[4] = (double)il[1];
    out8[5] = (double)il[2]; out8[6] = (double)il[3]; out8[7] = (double)il[4];
    h->t_fwd = 0; h->n_fwd = 0; h->mx_retry_total = 0;
    return 0;
}

// Plan fallback: the backup store, one buffer [A | Bm | Kc | backoff_x] with the shapes of the live arrays
static size_t plan_doubles(const slsqp_handle *h, int part) {      // doubles per instance of part 0..3
    const slsqp_dims &d = h->d;
    return part == 0 ? (size_t)d.N * d.nx * d.nx : part == 3 ? (size_t)(d.N + 1) * d.nx : (size_t)d.N * d.nx * d.nu;
}
static double *plan_part(const slsqp_handle *h, int part) {
    double *p = h->plan_bk;
    for (int i = 0; i < part; i++) p += (size_t)h->B * plan_doubles(h, i);
    return p;
}
static int plan_part_named(const char *name) {
    static const char *names[] = {"plan_A", "plan_Bm", "plan_Kc", "plan_backoff_x"};
    for (int i = 0; i < 4; i++) if (!strcmp(name, names[i])) return i;
    return -1;
}
// bytes per instance of a named result (what slsqp_get copies for each instance), or -1 for an unknown name
extern "C" long long slsqp_result_bytes(slsqp_handle *h, const char *name) {
    if (!strcmp(name, "plant_params")) return h->model_id < 0 ? -1LL : (long long)sizeof(double) * plant_params::count(h->model_id);
    if (!strcmp(name, "model_err")) return (long long)sizeof(double) * h->d.nx;
    if (!strcmp(name, "w_applied")) return (long long)sizeof(double) * h->d.nx;
    if (!strcmp(name, "x_plant")) return (long long)sizeof(double) * h->d.nx;
    if (!strcmp(name, "meas_noise")) return (long long)sizeof(double) * h->d.nx * h->mn.T;
    if (!strcmp(name, "bounds_g")) return (long long)sizeof(double) * h->d.ni * (h->bnd_rows ? h->bnd_T : 1);
    if (!strcmp(name, "bounds_gf")) return (long long)sizeof(double) * h->d.ni_f * (h->bnd_rows ? h->bnd_T : 1);
    if (!strcmp(name, "hold_index") || !strcmp(name, "hold_policy")) return (long long)sizeof(int);
    if (!strcmp(name, "hold_xi")) return (long long)sizeof(double) * (h->d.N + 1) * h->d.nx;
    if (!strcmp(name, "plan_age")) return (long long)sizeof(int);
    if (const int part = plan_part_named(name); part >= 0) return (long long)sizeof(double) * plan_doubles(h, part);
    auto it = h->named.find(name);
    return it == h->named.end() ? -1LL : (long long)it->second.second;
}

extern "C" int slsqp_set_x0_box_tol(slsqp_handle *h, double tol) {
    if (!(tol >= 0.0)) return fail("slsqp_set_x0_box_tol: the tolerance must be >= 0 (0 = strict, INFINITY = the stage-0 state rows never gate)");
    h->x0_box_tol = tol;
    return 0;
}
extern "C" double slsqp_get_x0_box_tol(slsqp_handle *h) { return h->x0_box_tol; }

extern "C" int slsqp_set_solve_waves(slsqp_handle *h, int waves) {
    if (waves != 1 && waves != 2 && waves != 4 && waves != 8) return fail("slsqp_set_solve_waves: waves must be 1 (the single-wave kernels), 2, 4 or 8");
    if (waves == h->solve_waves) return 0;
    hipSetDevice(h->dev);
    forget_factors(h);      // neither path may read the factors the other one stored
    HIPCHK(hipGetLastError());
    h->solve_waves = waves;
    return 0;
}
extern "C" int slsqp_get_solve_waves(slsqp_handle *h) { return h->solve_waves; }

// Reference of the tracked cost: validated and packed on the host into rows [x_ref(t); u_ref(t)], then one upload; the previous reference stays in
// force until the new one is complete.
extern "C" int slsqp_cl_set_reference(slsqp_handle *h, const double *Xref, const double *Uref, int T, int per_instance, int loc) {
    hipSetDevice(h->dev);
    if (per_instance != 0 && per_instance != 1) return fail("slsqp_cl_set_reference: per_instance must be 0 (one reference for the batch) or 1 (Xref (B,T,nx), Uref (B,T,nu))");
    if (T < 0) return fail("slsqp_cl_set_reference: T must be >= 1 (or 0 with Xref = NULL to clear the reference)");
    if (T == 0 && Xref) return fail("slsqp_cl_set_reference: T = 0 clears the reference and takes Xref = NULL; a reference has T >= 1 rows");
    if (T > 0 && !Xref) return fail("slsqp_cl_set_reference: Xref is NULL with T > 0 (T = 0 clears the reference)");
    if (loc != SLSQP_HOST && loc != SLSQP_DEVICE) return fail("slsqp_cl_set_reference: loc must be SLSQP_HOST or SLSQP_DEVICE");
    HIPCHK(hipStreamSynchronize(h->st));      // no launch may still read the buffer that is replaced
    if (T == 0) {
        opt_clear(&h->ref_Y);
        h->ref_T = 0; h->ref_stride = 0;
        return 0;
    }
    const size_t nx = h->d.nx, nu = h->d.nu, nz = nx + nu, rows = (size_t)(per_instance ? h->B : 1) * T;
    std::vector<double> X(rows * nx), U(rows * nu, 0.0), Y(rows * nz);
    if (opt_fetch(X, Xref, loc) || (Uref && opt_fetch(U, Uref, loc))) return -1;
    for (size_t r = 0; r < rows; r++) {
        for (size_t i = 0; i < nx; i++) Y[r * nz + i] = X[r * nx + i];
        for (size_t i = 0; i < nu; i++) Y[r * nz + nx + i] = U[r * nu + i];
    }
    for (double v : Y) if (!std::isfinite(v)) return fail("slsqp_cl_set_reference: the reference holds a NaN or infinite entry");
    if (opt_install("slsqp_cl_set_reference", &h->ref_Y, Y)) return -1;
    h->ref_T = T; h->ref_stride = per_instance ? (size_t)T * nz : 0;
    return 0;
}

// Plant parameters: names and defaults per model, and the setter -- validated on the host (plant_params.hpp), uploaded into a new buffer, and only
// then the previous buffer is dropped: a refused call leaves the previous parameters in force.
extern "C" int slsqp_plant_param_count(int model_id) { return plant_params::count(model_id); }
extern "C" const char *slsqp_plant_param_name(int model_id, int i) { return plant_params::name(model_id, i); }
extern "C" int slsqp_plant_param_defaults(int model_id, double *out, int len) {
    const int np = plant_params::count(model_id);
    if (np < 0) return fail("slsqp_plant_param_defaults: unknown model id (0 pendulum, 1 quadrotor, 2 rocket)");
    if (!out || len < np) return fail("slsqp_plant_param_defaults: the buffer must hold slsqp_plant_param_count(model_id) doubles");
    for (int i = 0; i < np; i++) out[i] = plant_params::default_value(model_id, i);
    return np;
}
extern "C" int slsqp_cl_set_plant_params(slsqp_handle *h, const double *P, int np, int per_instance, int loc) {
    hipSetDevice(h->dev);
    if (h->model_id < 0) return fail("slsqp_cl_set_plant_params: slsqp_set_model must be called first");
    if (per_instance != 0 && per_instance != 1) return fail("slsqp_cl_set_plant_params: per_instance must be 0 (one row for the batch) or 1 (P (B,np))");
    if (loc != SLSQP_HOST && loc != SLSQP_DEVICE) return fail("slsqp_cl_set_plant_params: loc must be SLSQP_HOST or SLSQP_DEVICE");
    if (np < 0) return fail("slsqp_cl_set_plant_params: np must be the model's parameter count (or 0 with P = NULL to clear the parameters)");
    if (np == 0 && P) return fail("slsqp_cl_set_plant_params: np = 0 clears the parameters and takes P = NULL");
    if (np > 0 && !P) return fail("slsqp_cl_set_plant_params: P is NULL with np > 0 (np = 0 clears the parameters)");
    HIPCHK(hipStreamSynchronize(h->st));      // no launch may still read the buffer that is replaced
    if (np == 0) {
        opt_clear(&h->pp_P, &h->pp_host);
        h->pp_merr = nullptr; h->pp_np = 0; h->pp_stride = 0;
        return 0;
    }
    if (np != plant_params::count(h->model_id)) { std::string why; plant_params::check(h->model_id, nullptr, 0, np, &why); return fail("slsqp_cl_set_plant_params: " + why); }
    const size_t rows = per_instance ? (size_t)h->B : 1, nP = rows * np, nE = (size_t)h->B * h->d.nx;
    std::vector<double> host(nP);
    if (opt_fetch(host, P, loc)) return -1;
    std::string why;
    if (!plant_params::check(h->model_id, host.data(), rows, np, &why)) return fail("slsqp_cl_set_plant_params: " + why);
    if (opt_install("slsqp_cl_set_plant_params", &h->pp_P, host, nE, &h->pp_host)) return -1;      // (model_err behind the rows, zeroed)
    h->pp_merr = h->pp_P + nP; h->pp_np = np; h->pp_stride = per_instance ? np : 0;
    return 0;
}
// An option's rows as slsqp_get serves them, (B, T, w): elements [off, off + w) of the T rows of width W of `host` (the option's host copy: one set per
// instance, or a shared one repeated), or `dflt` (w) for every row where the option is unset (host NULL)
static std::vector<double> opt_rows(size_t B, const std::vector<double> *host, bool per_instance, size_t T, size_t W, size_t off, size_t w, const double *dflt) {
    std::vector<double> v(B * T * w);
    for (size_t b = 0; b < B; b++)
        for (size_t t = 0; t < T; t++)
            for (size_t i = 0; i < w; i++) v[(b * T + t) * w + i] = host ? (*host)[(per_instance ? b * T * W : 0) + t * W + off + i] : dflt[i];
    return v;
}
// slsqp_get names that depend on the plant parameters: plant_params (B,np) (a shared row repeated; the defaults for a handle without parameters),
// model_err (B,nx) (zeros without parameters).  Returns 1 when `name` was one of them and has been served, 0 when not, -1 on error.
static int get_plant_named(slsqp_handle *h, const char *name, void *out, int loc) {
    const bool is_P = !strcmp(name, "plant_params"), is_e = !strcmp(name, "model_err");
    if (!is_P && !is_e) return 0;
    if (h->model_id < 0) return fail(std::string(name) + ": slsqp_set_model must be called first");
    const hipMemcpyKind kind = loc == SLSQP_HOST ? hipMemcpyHostToHost : hipMemcpyHostToDevice;
    HIPCHK(hipStreamSynchronize(h->st));
    if (is_e) {
        const size_t n = (size_t)h->B * h->d.nx;
        if (h->pp_P || h->adv_policy != cl_adversary::OFF) HIPCHK(hipMemcpy(out, h->pp_P ? h->pp_merr : h->adv_merr, sizeof(double) * n, loc == SLSQP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));      // (under an adversary without parameters: what the persistent kernels' PP variants wrote for the model's row -- zeros)
        else { std::vector<double> z(n, 0.0); HIPCHK(hipMemcpy(out, z.data(), sizeof(double) * n, kind)); }
        return 1;
    }
    const int np = plant_params::count(h->model_id);
    std::vector<double> dflt(np);
    for (int i = 0; i < np; i++) dflt[i] = plant_params::default_value(h->model_id, i);
    const std::vector<double> v = opt_rows(h->B, h->pp_P ? &h->pp_host : nullptr, h->pp_stride != 0, 1, np, 0, np, dflt.data());
    HIPCHK(hipMemcpy(out, v.data(), sizeof(double) * v.size(), kind));
    return 1;
}

// Box bounds over MPC time (include/slsqp.h): validated and packed on the host (cl_bounds.hpp) into rows [g(t); gf(t)], uploaded into a new buffer,
// and only then the previous buffer is dropped: a refused call leaves the previous bounds in force.
extern "C" int slsqp_cl_set_bounds(slsqp_handle *h, const double *g, const double *gf, int T, int per_instance, int loc) {
    hipSetDevice(h->dev);
    if (h->general_G) return fail("slsqp_cl_set_bounds: general G: the bounds are the right-hand sides of a box G = [I;-I]");
    if (h->model_id < 0) return fail("slsqp_cl_set_bounds: slsqp_set_model must be called first");
    if (loc != SLSQP_HOST && loc != SLSQP_DEVICE) return fail("slsqp_cl_set_bounds: loc must be SLSQP_HOST or SLSQP_DEVICE");
    std::string why;
    if (!cl_bounds::check_call(g, T, per_instance, &why)) return fail("slsqp_cl_set_bounds: " + why);
    HIPCHK(hipStreamSynchronize(h->st));      // no launch may still read the buffer that is replaced
    if (T == 0) {
        opt_clear(&h->bnd_rows, &h->bnd_host);
        h->bnd_T = 0; h->bnd_stride = 0;
        return 0;
    }
    if (!gf && !h->have_cons) return fail("slsqp_cl_set_bounds: gf = NULL repeats the model's gf: slsqp_set_constraints must be called first");
    const size_t ni = h->d.ni, nif = h->d.ni_f, sets = per_instance ? (size_t)h->B : 1, rows = sets * (size_t)T;
    std::vector<double> hg(rows * ni), hgf(gf ? rows * nif : 0), packed;
    if (opt_fetch(hg, g, loc) || (gf && opt_fetch(hgf, gf, loc))) return -1;
    if (!cl_bounds::pack(hg.data(), gf ? hgf.data() : nullptr, h->gf_raw_host.data(), sets, T, (int)ni, (int)nif, &packed, &why)) return fail("slsqp_cl_set_bounds: " + why);
    if (opt_install("slsqp_cl_set_bounds", &h->bnd_rows, packed, 0, &h->bnd_host)) return -1;
    h->bnd_T = T; h->bnd_stride = per_instance ? (size_t)T * (ni + nif) : 0;
    return 0;
}
// slsqp_get names of the bounds: bounds_g (B, T, ni), bounds_gf (B, T, ni_f) (a shared set repeated; without bounds the model's box with T = 1).
// Returns 1 when `name` was one of them and has been served, 0 when not, -1 on error.
static int get_bounds_named(slsqp_handle *h, const char *name, void *out, int loc) {
    const bool is_g = !strcmp(name, "bounds_g"), is_f = !strcmp(name, "bounds_gf");
    if (!is_g && !is_f) return 0;
    if (h->model_id < 0 || !h->have_cons) return fail(std::string(name) + ": slsqp_set_model and slsqp_set_constraints must be called first");
    const size_t ni = h->d.ni, nif = h->d.ni_f;
    const std::vector<double> v = opt_rows(h->B, h->bnd_rows ? &h->bnd_host : nullptr, h->bnd_stride != 0, h->bnd_rows ? (size_t)h->bnd_T : 1, ni + nif, is_g ? 0 : ni, is_g ? ni : nif,
                                           is_g ? h->g_raw_host.data() : h->gf_raw_host.data());
    HIPCHK(hipMemcpy(out, v.data(), sizeof(double) * v.size(), loc == SLSQP_HOST ? hipMemcpyHostToHost : hipMemcpyHostToDevice));
    return 1;
}

// slsqp_get names of the hold steps (slsqp_cl_hold_step): hold_index[int32] (1) hold steps since the last solve, hold_xi (N+1,nx) the column states
// (rows above the index zero), hold_policy[int32] (1) of the last hold step; zeros on a handle that never held.  Returns 1 when `name` was one of
// them and has been served, 0 when not, -1 on error.
static int get_hold_named(slsqp_handle *h, const char *name, void *out, int loc) {
    const bool is_k = !strcmp(name, "hold_index"), is_x = !strcmp(name, "hold_xi"), is_p = !strcmp(name, "hold_policy");
    if (!is_k && !is_x && !is_p) return 0;
    HIPCHK(hipStreamSynchronize(h->st));
    const size_t B = h->B, nxi = B * (h->d.N + 1) * h->d.nx;
    const hipMemcpyKind from_host = loc == SLSQP_HOST ? hipMemcpyHostToHost : hipMemcpyHostToDevice, from_dev = loc == SLSQP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (is_k && cl_hold::index_per_instance(h->hold, h->cl_steps) && h->hold_k) HIPCHK(hipMemcpy(out, h->hold_k, sizeof(int) * B, from_dev));      // (an event-triggered run: every instance at its own index)
    else if (is_k) { const std::vector<int> v(B, cl_hold::index(h->hold, h->cl_steps)); HIPCHK(hipMemcpy(out, v.data(), sizeof(int) * B, from_host)); }
    else if (!h->hold_xi) {
        if (is_x) { const std::vector<double> z(nxi, 0.0); HIPCHK(hipMemcpy(out, z.data(), sizeof(double) * nxi, from_host)); }
        else { const std::vector<int> z(B, 0); HIPCHK(hipMemcpy(out, z.data(), sizeof(int) * B, from_host)); }
    }
    else if (is_x) HIPCHK(hipMemcpy(out, h->hold_xi, sizeof(double) * nxi, from_dev));
    else HIPCHK(hipMemcpy(out, h->hold_policy, sizeof(int) * B, from_dev));
    return 1;
}

// slsqp_get names of plan fallback (slsqp_cl_set_plan_fallback): plan_age[int32] (1), plan_A (N,nx,nx), plan_Bm (N,nx,nu), plan_Kc (N,nu,nx),
// plan_backoff_x (N+1,nx): every instance's backup and its age; ages -1 and zeros on a handle that never ran with the option on.  Returns as above.
static int get_plan_named(slsqp_handle *h, const char *name, void *out, int loc) {
    const int part = plan_part_named(name);
    const bool is_age = !strcmp(name, "plan_age");
    if (!is_age && part < 0) return 0;
    HIPCHK(hipStreamSynchronize(h->st));
    const size_t B = h->B;
    const hipMemcpyKind from_host = loc == SLSQP_HOST ? hipMemcpyHostToHost : hipMemcpyHostToDevice, from_dev = loc == SLSQP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (is_age) {
        if (h->plan_age) HIPCHK(hipMemcpy(out, h->plan_age, sizeof(int) * B, from_dev));
        else { const std::vector<int> v(B, -1); HIPCHK(hipMemcpy(out, v.data(), sizeof(int) * B, from_host)); }
    } else {
        const size_t n = B * plan_doubles(h, part);
        if (h->plan_bk) HIPCHK(hipMemcpy(out, plan_part(h, part), sizeof(double) * n, from_dev));
        else { const std::vector<double> z(n, 0.0); HIPCHK(hipMemcpy(out, z.data(), sizeof(double) * n, from_host)); }
    }
    return 1;
}

static int get_adversary_named(slsqp_handle *h, const char *name, void *out, int loc);      // slsqp_cl_set_adversary, below
static int get_meas_named(slsqp_handle *h, const char *name, void *out, int loc);      // slsqp_cl_set_meas_noise, below
extern "C" int slsqp_get(slsqp_handle *h, const char *name, void *out, int loc) {
    hipSetDevice(h->dev);
    if (const int r = get_adversary_named(h, name, out, loc)) return r < 0 ? -1 : 0;
    if (const int r = get_meas_named(h, name, out, loc)) return r < 0 ? -1 : 0;
    if (const int r = get_plant_named(h, name, out, loc)) return r < 0 ? -1 : 0;
    if (const int r = get_bounds_named(h, name, out, loc)) return r < 0 ? -1 : 0;
    if (const int r = get_hold_named(h, name, out, loc)) return r < 0 ? -1 : 0;
    if (const int r = get_plan_named(h, name, out, loc)) return r < 0 ? -1 : 0;
    if (h->adv_policy == cl_adversary::OFF && h->lg_wadv && !strcmp(name, "log_w_applied")) HIPCHK(hipMemsetAsync(h->lg_wadv, 0, sizeof(double) * (size_t)h->B * h->log_steps * h->d.nx, h->st));      // (the option is off: all zeros, whatever an earlier run left)
    if (!h->pp_P && h->adv_policy == cl_adversary::OFF && h->lg_merr && !strcmp(name, "log_model_error")) HIPCHK(hipMemsetAsync(h->lg_merr, 0, sizeof(double) * (size_t)h->B * h->log_steps * h->d.nx, h->st));      // (a handle without parameters: all zeros, whatever an earlier run with parameters left)
    auto it = h->named.find(name);
    if (it == h->named.end()) return fail(std::string("unknown result name: ") + name);
    const size_t bytes = it->second.second * (size_t)h->B;
    {   // arrays that slsqp_reset only marked stale
        const slsqp_dims &d = h->d;
        if (!strcmp(name, "eta") || !strcmp(name, "eta_f")) {
            hipLaunchKernelGGL(k_zero_stale, dim3(h->B), dim3(256), 0, h->st, h->stale, 1, h->eta, (size_t)d.N * d.N * d.ni, h->eta_f, (size_t)(d.N + 1) * d.ni_f);
            hipLaunchKernelGGL(k_eta_broadcast, dim3(h->B), dim3(256), 0, h->st, d.N, d.ni, d.ni_f, h->stale, h->eta, h->eta_f);
        }
        else if (!strcmp(name, "K")) {
            hipLaunchKernelGGL(k_zero_stale, dim3(h->B), dim3(256), 0, h->st, h->stale, 2, h->K, (size_t)d.N * (d.N + 1) * d.nu * d.nx, (double *)nullptr, (size_t)0);
            hipLaunchKernelGGL(k_K_broadcast, dim3(h->B), dim3(256), 0, h->st, d.N, d.nu * d.nx, h->stale, h->Kc, h->K);
        }
        else if (!strcmp(name, "beta")) hipLaunchKernelGGL(k_beta_upper_zero, dim3(h->B), dim3(256), 0, h->st, d.N, d.ni, h->stale, h->beta);
    }
    HIPCHK(hipMemcpyAsync(out, it->second.first, bytes, loc == SLSQP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    return 0;
}

// Overwrite a named array (the reference's callers poke the QP's bounds between solves: QP.update_ubg, qp_jit.py:578-586, used by
// SCP_SLS_jit.py:86-99).  Writable: ubg, lbg, q, nominal_x, nominal_u, x_meas, x_plant.
extern "C" int slsqp_set(slsqp_handle *h, const char *name, const void *src, int loc) {
    hipSetDevice(h->dev);
    static const char *ok[] = {"ubg", "lbg", "q", "nominal_x", "nominal_u", "x_meas"};
    bool allowed = false;
    for (const char *k : ok) allowed |= (strcmp(k, name) == 0);
    if (!strcmp(name, "x_plant")) {      // the true state: an array of its own under slsqp_cl_set_meas_noise (x_meas then is the measurement alone), else x_meas itself
        HIPCHK(hipMemcpyAsync(h->mn.T > 0 ? h->x_plant : h->xmeas, src, sizeof(double) * (size_t)h->B * h->d.nx, loc == SLSQP_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, h->st));
        HIPCHK(hipStreamSynchronize(h->st));
        return 0;
    }
    auto it = h->named.find(name);
    if (!allowed || it == h->named.end()) return fail(std::string("slsqp_set: not a writable array: ") + name);
    const size_t bytes = it->second.second * (size_t)h->B;
    HIPCHK(hipMemcpyAsync(it->second.first, src, bytes, loc == SLSQP_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    return 0;
}

extern "C" int slsqp_reset(slsqp_handle *h) {
    hipSetDevice(h->dev);
    // reset_solver_to_zeros (fast_SLS_jit.py:424-442): eta/eta_f/iteration_number to zero, bounds and linear cost dropped.
    // `_prev_primal_vec` is NOT cleared by the reference (quirk q5) and is not cleared here.
    const size_t B = h->B;
    // eta, eta_f and K (1.5 GB at rocket B = 4096) are not cleared here: every entry the device reads is rewritten first (evaluate_dual_eta before the
    // sweep, the sweep before anything reads K), so they are only marked stale and zeroed on demand when slsqp_get asks for them
    hipLaunchKernelGGL(k_reset_stale, dim3((h->B + 255) / 256), dim3(256), 0, h->st, h->stale, h->B);
    HIPCHK(hipMemsetAsync(h->itnum, 0, sizeof(int) * B, h->st));
    HIPCHK(hipMemsetAsync(h->pending_reset, 0, sizeof(int) * B, h->st));
    HIPCHK(hipMemsetAsync(h->q, 0, sizeof(double) * B * h->n, h->st));
    h->have_dyn = false;
    return 0;
}

// ---- linearisation step in front of the path (SCP_SLS.update_jacobian) ----------------------------------------------
extern "C" int slsqp_set_model(slsqp_handle *h, int model_id, const double *g_raw) {
    hipSetDevice(h->dev);
    if (h->general_G) return fail("general G: the plants of slsqp_set_model have box constraints");
    const int want_nx = model_id == 0 ? 4 : (model_id == 1 ? 13 : (model_id == 2 ? 17 : -1));
    if (want_nx != h->d.nx || h->d.nw != h->d.nx) return fail("model id does not match the handle's dimensions (0 pendulum, 1 quadrotor, 2 rocket; nw = nx)");
    HIPCHK(hipMemcpy(h->g_raw, g_raw, sizeof(double) * h->d.ni, hipMemcpyHostToDevice));
    h->g_raw_host.assign(g_raw, g_raw + h->d.ni);
    h->model_id = model_id;
    return 0;
}

extern "C" int slsqp_set_E(slsqp_handle *h, const double *E, int loc) {
    hipSetDevice(h->dev);
    return put_E(h, E, loc);
}

// step / stepno: the MPC step whose window of the reference forms q and whose window of the bounds forms g, gN (a handle with a reference / with bounds only): `step` for every instance, or stepno[b]
static int linearize_impl(slsqp_handle *h, const double *X, const double *U, int loc, const int *run, int step, const int *stepno = nullptr) {
    hipSetDevice(h->dev);
    if (h->model_id < 0 || !h->have_costs || !h->have_cons) return fail("set_model, set_costs and set_constraints must be called first");
    const slsqp_dims &d = h->d;
    const size_t B = h->B;
    const double *dX = X, *dU = U;
    if (loc == SLSQP_HOST) {
        const size_t nX = B * (d.N + 1) * d.nx, nU = B * d.N * d.nu;
        double *tmp = stage_buf(h, sizeof(double) * (nX + nU));
        if (!tmp) return -1;
        HIPCHK(hipMemcpyAsync(tmp, X, sizeof(double) * nX, hipMemcpyHostToDevice, h->st));
        HIPCHK(hipMemcpyAsync(tmp + nX, U, sizeof(double) * nU, hipMemcpyHostToDevice, h->st));
        dX = tmp; dU = tmp + nX;
    }
    const LinArgs a = lin_args(h, dX, dU, run);
    const int grid = 2048, blk = 128;
    const int gval = (int)((B * d.N + blk - 1) / blk);
    const ClOptions op = cl_options(h);
    if (with_model(h, [&](auto M) {
            constexpr int NX = dyn::Dims<M()>::NX, NU = dyn::Dims<M()>::NU;
            hipLaunchKernelGGL((k_lin_val<M()>), dim3(gval), dim3(blk), 0, h->st, a); hipLaunchKernelGGL((k_lin_tan<M()>), dim3(grid), dim3(blk), 0, h->st, a);
            with_ref_bnd(op, [&](auto REF, auto BND) { hipLaunchKernelGGL((k_lin_vec<NX, NU, REF(), BND()>), dim3(grid), dim3(256), 0, h->st, a, op.own_rf, bnd_args(h, step, stepno)); });
        })) return -1;
    hipLaunchKernelGGL(k_set_bounds, dim3(1024), dim3(256), 0, h->st, bounds_args(h, run));
    HIPCHK(hipGetLastError());
    if (loc == SLSQP_HOST) HIPCHK(hipStreamSynchronize(h->st));   // the caller's buffers may be reused on return; device callers stay asynchronous on the handle's stream
    h->have_dyn = true;
    return 0;
}
extern "C" int slsqp_linearize(slsqp_handle *h, const double *X, const double *U, int loc) { return linearize_impl(h, X, U, loc, nullptr, h->cl_steps); }

// ---- closed-loop driver around the path (SCP_SLS.solve + reset_warm_start + plant) -------------------------
extern "C" int slsqp_cl_init(slsqp_handle *h, const double *x_meas, const double *X_nom, const double *U_nom, const double *u_init, int loc) {
    hipSetDevice(h->dev);
    if (h->model_id < 0) return fail("slsqp_set_model must be called first");
    const slsqp_dims &d = h->d;
    const size_t B = h->B;
    if (put(h, h->xmeas, x_meas, sizeof(double) * B * d.nx, loc)) return -1;
    // slsqp_cl_set_meas_noise: the table the setter last accepted is in force from here on; `x_meas` is the TRUE state, x_plant <- x, x_meas <- x + n_0
    // (the roll-out below and slsqp_nominal_solve then start from the measurement)
    if (h->mn.rows && h->mn.rows != h->mn_next.rows) { HIPCHK(hipStreamSynchronize(h->st)); hipFree(h->mn.rows); }
    h->mn.rows = h->mn_next.rows; h->mn.T = h->mn_next.T; h->mn.stride = h->mn_next.stride; h->mn.host = h->mn_next.host;
    if (h->mn.T > 0) hipLaunchKernelGGL(k_cl_meas, dim3((h->B + 63) / 64), dim3(64), 0, h->st, meas_args(h), h->B, d.nx, h->xmeas, 1, -1, nullptr, nullptr);
    if (X_nom && U_nom) {
        if (put(h, h->Xn, X_nom, sizeof(double) * B * (d.N + 1) * d.nx, loc)) return -1;
        if (put(h, h->Un, U_nom, sizeof(double) * B * d.N * d.nu, loc)) return -1;
    } else {
        std::vector<double> ui(d.nu, 0.0);
        if (u_init) for (int i = 0; i < d.nu; i++) ui[i] = u_init[i];
        HIPCHK(hipMemcpy(h->u_init, ui.data(), sizeof(double) * d.nu, hipMemcpyHostToDevice));
        ClArgs a = cl_args(h, nullptr);
        const int gb = (h->B + 63) / 64;
        if (with_model(h, [&](auto M) { hipLaunchKernelGGL((k_cl_rollout<M()>), dim3(gb), dim3(64), 0, h->st, a); })) return -1;
        HIPCHK(hipGetLastError());
    }
    h->cl_steps = 0;
    cl_hold::on_init(h->hold);      // no plan to hold yet
    if (h->plan_age) HIPCHK(hipMemsetAsync(h->plan_age, 0xFF, sizeof(int) * B, h->st));      // (plan fallback: no backup, every age -1)
    if (h->lg_age) HIPCHK(hipMemsetAsync(h->lg_age, 0, sizeof(int) * B * h->log_steps, h->st));      // (log_plan_age: written by the steps of a handle with the option on)
    if (h->lg_hold) HIPCHK(hipMemsetAsync(h->lg_hold, 0, sizeof(int) * B * h->log_steps * 2, h->st));      // (log_hold, log_hold_policy: solved steps never write them)
    if (h->adv_buf) {      // (slsqp_cl_set_adversary: no plant step yet; without parameters of its own the handle's model error and its log are the PP variants' to write, zeros until then)
        HIPCHK(hipMemsetAsync(h->adv_merr, 0, sizeof(double) * 2 * B * d.nx, h->st));
        if (!h->pp_P && h->lg_merr) HIPCHK(hipMemsetAsync(h->lg_merr, 0, sizeof(double) * B * h->log_steps * d.nx, h->st));
    }
    if (h->lg_ratio) { HIPCHK(hipMemsetAsync(h->lg_ratio, 0, sizeof(double) * B * h->log_steps, h->st)); HIPCHK(hipMemsetAsync(h->lg_trig, 0, sizeof(int) * B * h->log_steps, h->st)); }      // (written by event-triggered runs only)
    HIPCHK(hipMemsetAsync(h->has_prev, 0, sizeof(int) * B, h->st));   // a fresh SCP_SLS object has no convergence history
    HIPCHK(hipStreamSynchronize(h->st));
    return slsqp_reset(h);
}

// Nominal-trajectory initialiser: trust-region SCP on the path's QP kernel (see k_nom_eval).  Works on the nominal held by the
// handle (slsqp_cl_init: caller's guess or roll-out) and the measured state given there.
extern "C" int slsqp_nominal_solve(slsqp_handle *h, int max_qp, double tol, double rho, const slsqp_opts *opts) {
    hipSetDevice(h->dev);
    if (h->general_G) return fail("general G: only the sweep-level boundary (slsqp_sweep) is available; the QP solver needs box constraints G = [I;-I]");
    if (h->model_id < 0 || !h->have_costs || !h->have_cons) return fail("set_model, set_costs and set_constraints must be called first");
    slsqp_opts o;
    if (opts) o = *opts; else slsqp_default_opts(&o);
    if (mw_refuse(h, o)) return -1;
    const slsqp_dims &d = h->d;
    const int B = h->B, gbi = (B + 255) / 256;
    if (max_qp <= 0) max_qp = 120;
    if (!(tol > 0.0)) tol = 1e-7;
    if (!(rho > 0.0)) rho = 1e3;
    int *active = h->scp_active;
    hipLaunchKernelGGL(k_nom_init, dim3(gbi), dim3(256), 0, h->st, B, h->nom_st, active, h->nom_need_lin, h->nom_status, h->nom_iters, 1.0, 0.5);
    NomArgs na;
    na.B = B; na.N = d.N; na.Xn = h->Xn; na.Un = h->Un; na.xmeas = h->xmeas; na.primal = h->primal; na.qp_status = h->status; na.g_raw = h->g_raw; na.gf_raw = h->gf_raw;
    na.cst = costs_of(h); na.st = h->nom_st; na.active = active; na.need_lin = h->nom_need_lin; na.status = h->nom_status; na.iters = h->nom_iters;
    na.n_active = h->counter + 2; na.rho = rho; na.tol = tol; na.w_max = 1e8;
    const ClOptions op = cl_options(h);      // the tracked objective and the box, window of step 0
    auto eval = [&](int mode) {
        na.mode = mode;
        return with_model(h, [&](auto M) {
            with_ref_bnd(op, [&](auto REF, auto BND) { hipLaunchKernelGGL((k_nom_eval<M(), REF(), BND()>), dim3(B), dim3(128), 0, h->st, na, op.own_rf, bnd_args(h, 0, nullptr)); });
        });
    };
    if (eval(0)) return -1;
    double tq = 0;
    for (int it = 0; it < max_qp; it++) {
        if (linearize_impl(h, h->Xn, h->Un, SLSQP_DEVICE, h->nom_need_lin, 0)) return -1;     // accepted instances only; the others re-solve
        NomBoundsArgs ba{B, d.N, d.nx, d.ni, d.ni_f, h->g, h->gN, h->c, h->nom_st, active, h->ubg, h->lbg, 1e-10};
        hipLaunchKernelGGL(k_nom_bounds, dim3(1024), dim3(256), 0, h->st, ba);
        hipLaunchKernelGGL(k_nom_x0, dim3((B * d.nx + 255) / 256), dim3(256), 0, h->st, B, d.N, d.nx, h->Xn, h->xmeas, h->nom_st, h->x0val);
        HIPCHK(hipEventRecord(h->ev[6], h->st));
        QpCall qc;
        qc.warm = it > 0 ? 1 : 0; qc.prox = h->nom_st;      // (S[0] = w: stride 12)
        if (launch_qp(h, active, &o, qc)) return -1;
        HIPCHK(hipEventRecord(h->ev[7], h->st));
        HIPCHK(hipMemsetAsync(h->counter + 2, 0, sizeof(int), h->st));
        if (eval(1)) return -1;
        int nact = 0;
        HIPCHK(hipMemcpyAsync(&nact, h->counter + 2, sizeof(int), hipMemcpyDeviceToHost, h->st));
        HIPCHK(hipStreamSynchronize(h->st));
        harvest_kernel_events(h);
        tq += ev_ms(h->ev[6], h->ev[7]);
        if (nact == 0) break;
    }
    h->t_qp = tq; h->t_total = tq; h->t_sweep = 0;
    h->have_dyn = false;   // the bounds in the handle are the initialiser's, not the path's: linearise again before slsqp_solve
    return 0;
}

// Device-side log of the closed loop: after this call every slsqp_cl_step stores what the reference's scripts keep per MPC step
// (expe/main_rocket_robust_closed_loop.py:160-178) into entry cl_steps of (B, max_steps, ...) buffers; slsqp_get names: log_state (S,nx)
// log_u0 (S,nu) log_nominal_x (S,N+1,nx) log_nominal_u (S,N,nu) log_backoff_x (S,N+1,nx) log_backoff_u (S,N,nu) log_success[int32] (S)
// log_scp_iterations[int32] (S).  slsqp_cl_init restarts at entry 0.
extern "C" int slsqp_cl_log(slsqp_handle *h, int max_steps) {
    hipSetDevice(h->dev);
    if (max_steps < 1) return fail("slsqp_cl_log: max_steps must be >= 1");
    HIPCHK(hipStreamSynchronize(h->st));
    h->log_steps = 0;
    free_all(h->log_owned);
    static const char *names[] = {"log_nominal_x", "log_nominal_u", "log_backoff_x", "log_backoff_u", "log_state", "log_u0", "log_success", "log_scp_iterations", "log_primal_infeasibility", "log_x0_viol", "log_model_error", "log_hold", "log_hold_policy", "log_tube_ratio", "log_solve_trigger", "log_plan_age", "log_w_applied", "log_plant_state", "log_measured_state"};
    for (const char *nm : names) h->named.erase(nm);
    h->lg_x0v = nullptr; h->lg_merr = nullptr; h->lg_hold = h->lg_hpol = nullptr; h->lg_ratio = nullptr; h->lg_trig = nullptr; h->lg_age = nullptr; h->lg_wadv = nullptr; h->lg_plant = h->lg_meas = nullptr;
    h->lg_x = h->lg_u = h->lg_bx = h->lg_bu = h->lg_state = h->lg_u0 = h->lg_pinf = nullptr; h->lg_succ = h->lg_it = nullptr;
    const slsqp_dims &d = h->d;
    const size_t B = h->B, S = max_steps, nX = (size_t)(d.N + 1) * d.nx, nU = (size_t)d.N * d.nu;
    int rc = 0;
    auto &ow = h->log_owned;
    rc |= dalloc(ow, &h->lg_x, B * S * nX); rc |= dalloc(ow, &h->lg_u, B * S * nU); rc |= dalloc(ow, &h->lg_bx, B * S * nX); rc |= dalloc(ow, &h->lg_bu, B * S * nU);
    rc |= dalloc(ow, &h->lg_state, B * S * d.nx); rc |= dalloc(ow, &h->lg_u0, B * S * d.nu); rc |= dalloc(ow, &h->lg_succ, B * S); rc |= dalloc(ow, &h->lg_it, B * S);
    rc |= dalloc(ow, &h->lg_pinf, B * S); rc |= dalloc(ow, &h->lg_x0v, B * S * 2); rc |= dalloc(ow, &h->lg_merr, B * S * d.nx);
    rc |= dalloc(ow, &h->lg_hold, B * S * 2); h->lg_hpol = h->lg_hold ? h->lg_hold + B * S : nullptr;
    rc |= dalloc(ow, &h->lg_ratio, B * S); rc |= dalloc(ow, &h->lg_trig, B * S); rc |= dalloc(ow, &h->lg_age, B * S); rc |= dalloc(ow, &h->lg_wadv, B * S * d.nx);
    rc |= dalloc(ow, &h->lg_plant, B * S * d.nx); rc |= dalloc(ow, &h->lg_meas, B * S * d.nx);
    if (rc) { free_all(ow); h->lg_plant = h->lg_meas = nullptr; h->lg_wadv = nullptr; h->lg_age = nullptr; h->lg_ratio = nullptr; h->lg_trig = nullptr; h->lg_x0v = nullptr; h->lg_merr = nullptr; h->lg_hold = h->lg_hpol = nullptr; h->lg_x = h->lg_u = h->lg_bx = h->lg_bu = h->lg_state = h->lg_u0 = h->lg_pinf = nullptr; h->lg_succ = h->lg_it = nullptr; return -1; }
    h->log_steps = max_steps;
    auto reg = [&](const char *nm, void *p, size_t bytes) { h->named[nm] = {p, bytes}; };
    reg("log_nominal_x", h->lg_x, sizeof(double) * S * nX); reg("log_nominal_u", h->lg_u, sizeof(double) * S * nU);
    reg("log_backoff_x", h->lg_bx, sizeof(double) * S * nX); reg("log_backoff_u", h->lg_bu, sizeof(double) * S * nU);
    reg("log_state", h->lg_state, sizeof(double) * S * d.nx); reg("log_u0", h->lg_u0, sizeof(double) * S * d.nu);
    reg("log_success", h->lg_succ, sizeof(int) * S); reg("log_scp_iterations", h->lg_it, sizeof(int) * S);
    reg("log_primal_infeasibility", h->lg_pinf, sizeof(double) * S); reg("log_x0_viol", h->lg_x0v, sizeof(double) * S * 2);
    reg("log_hold", h->lg_hold, sizeof(int) * S); reg("log_hold_policy", h->lg_hpol, sizeof(int) * S);      // slsqp_cl_hold_step: 0 for a solved step, k for hold step k; whether the policy ran
    reg("log_tube_ratio", h->lg_ratio, sizeof(double) * S); reg("log_solve_trigger", h->lg_trig, sizeof(int) * S);      // an event-triggered slsqp_cl_run (slsqp_cl_set_hold_trigger): the ratio where it was evaluated, the reason code of cl_hold::decide; zeros from every other run
    reg("log_plan_age", h->lg_age, sizeof(int) * S);      // plan fallback (slsqp_cl_set_plan_fallback): the age every step left behind; zeros from a handle with the option off
    reg("log_w_applied", h->lg_wadv, sizeof(double) * S * d.nx);      // the sample every step's plant step used under slsqp_cl_set_adversary; zeros from a handle with the option off
    reg("log_plant_state", h->lg_plant, sizeof(double) * S * d.nx); reg("log_measured_state", h->lg_meas, sizeof(double) * S * d.nx);      // slsqp_cl_set_meas_noise: the true state and the measurement at the top of every step; copies of log_state from a handle with the option off (slsqp_get)
    reg("log_model_error", h->lg_merr, sizeof(double) * S * d.nx);      // ddyn_p - ddyn of every step's plant step (slsqp_cl_set_plant_params; zeros without parameters)
    return 0;
}

// entry `step` of the per-step copy of x0_viol (slsqp_cl_step with slsqp_cl_log; the closed-loop kernels write theirs themselves)
__global__ void k_cl_log_x0v(int B, int log_steps, int step, const double *x0viol, const int *qpstat, double *lg) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * B) lg[((size_t)(i / 2) * log_steps + step) * 2 + (i & 1)] = qpstat[(size_t)i * 8 + 6] == -1 ? 0.0 : x0viol[i];      // (a QP that took no part records 0)
}

static int ensure_plan(slsqp_handle *h);      // plan fallback, beside slsqp_cl_hold_step below
static PlanArgs plan_args(const slsqp_handle *h);
static void hold_args_on_backup(const slsqp_handle *h, HoldArgs &a);
static ClArgs plant_args_on_u(const slsqp_handle *h, ClArgs a);
extern const char *const FALLBACK_NEEDS;
// slsqp_cl_set_adversary on the stepped paths: k_cl_adversary directly in front of a plant launch, which then takes adv_w as its
// samples.  w (B,nx) or NULL: the caller's sample of this step; step, or mask / stepno / W_all as the plant launch of a round takes them.
static int launch_adversary(slsqp_handle *h, const ClOptions &op, const double *w, int step, const int *mask, const int *stepno, const double *W_all) {
    const int gb = (h->B + 63) / 64;
    return with_model(h, [&](auto M) { hipLaunchKernelGGL((k_cl_adversary<dyn::Dims<M()>::NX>), dim3(gb), dim3(64), 0, h->st, op.aa, h->B, h->xmeas, h->E, w, step, mask, stepno, W_all); });
}
// slsqp_cl_set_meas_noise on the stepped paths: k_cl_meas in front of (post = 0) and behind (post = 1) a plant launch, with the
// step, or the mask / stepno, that launch takes.  Nothing is launched for a handle with the option off.
static void launch_meas(slsqp_handle *h, const ClOptions &op, int post, int step, const int *mask, const int *stepno) {
    if (!op.mn) return;
    hipLaunchKernelGGL(k_cl_meas, dim3((h->B + 63) / 64), dim3(64), 0, h->st, op.ma, h->B, h->d.nx, h->xmeas, post, step, mask, stepno);
}
// One MPC step for the whole batch: [warm-start shift + solver reset] -> rti x (linearise, fast-SLS solve of x_nom0 - x_meas,
// nominal += delta) -> u0 = first nominal input -> plant step x_meas <- ddyn(x_meas,u0) + E w.   w (B,nx) or NULL (no noise).
extern "C" int slsqp_cl_step(slsqp_handle *h, int rti, const double *w, int loc, const slsqp_opts *opts) {
    hipSetDevice(h->dev);
    if (h->model_id < 0) return fail("slsqp_set_model must be called first");
    if (opts && mw_refuse(h, *opts)) return -1;
    const slsqp_dims &d = h->d;
    const int gb = (h->B + 63) / 64;
    const double *dw = nullptr;
    if (w) { if (put(h, h->wbuf, w, sizeof(double) * (size_t)h->B * d.nx, loc)) return -1; dw = h->wbuf; }
    ClArgs a = cl_args(h, dw);
    const ClOptions op = cl_options(h);
    slsqp_opts o;
    if (opts) o = *opts; else slsqp_default_opts(&o);
    if (op.fallback && !(rti == 1 && o.rti_steps == 1)) return fail(std::string("slsqp_cl_step: ") + FALLBACK_NEEDS + " (the backup keeps the compact gains of the shared Riccati recursion; the full K is not snapshotted)");
    if (op.fallback && ensure_plan(h)) return -1;
    if (h->cl_steps > 0) {
        if (with_model(h, [&](auto M) { hipLaunchKernelGGL((k_cl_shift_plant<M()>), dim3(gb), dim3(64), 0, h->st, a, 1, 0); })) return -1;
        if (slsqp_reset(h)) return -1;
        h->horizon_shifted = 1;
    }
    // SCP_SLS.solve (solver/SCP_SLS_jit.py:65-152): rti > 0 -> exactly rti iterations; rti <= 0 -> until |delta|inf < scp_eps
    // (epsilon_convergence :29) or MAX_ITER_SCP (:47).  Instances leave the loop one by one (failed step / converged); the
    // linearisation, the fast-SLS solve and the nominal update only touch the ones still iterating.
    const bool converge = rti <= 0;
    const int max_it = converge ? o.max_scp_iter : rti;
    const int B = h->B, gbi = (B + 255) / 256;
    hipLaunchKernelGGL(k_fill_int, dim3(gbi), dim3(256), 0, h->st, h->scp_active, 1, B);
    hipLaunchKernelGGL(k_fill_int, dim3(gbi), dim3(256), 0, h->st, h->scp_success, 0, B);
    hipLaunchKernelGGL(k_fill_int, dim3(gbi), dim3(256), 0, h->st, h->scp_iters, 0, B);
    {
        const int tl_j = tl_begin(h, 3);
        if (linearize_impl(h, h->Xn, h->Un, SLSQP_DEVICE, nullptr, h->cl_steps)) return -1;
        tl_end(h, tl_j);
    }
    for (int ii = 0; ii < max_it; ii++) {
        hipLaunchKernelGGL(k_cl_x0arg, dim3(64), dim3(256), 0, h->st, a);
        const BndArgs bd = bnd_args(h, h->cl_steps, nullptr);      // (the tightening's terminal row: the window of this step)
        if (solve_impl(h, h->x0arg, SLSQP_DEVICE, &o, h->scp_active, /* no_sync */ true, op.bnd ? &bd : nullptr)) return -1;
        HIPCHK(hipMemsetAsync(h->counter + 2, 0, sizeof(int), h->st));
        hipLaunchKernelGGL(k_cl_scp_update, dim3(B), dim3(64), 0, h->st, a, scp_args(h, o, ii, converge ? 1 : 0));
        if (with_model(h, [&](auto M) { hipLaunchKernelGGL((k_cl_infeas<M()>), dim3(B), dim3(64), 0, h->st, a, h->scp_upd, h->pinf); })) return -1;
        if (ii + 1 == max_it) break;
        if (converge) {     // the host decides whether anyone is still iterating; RTI mode runs its rti iterations without looking (the instances that
                            // failed are masked on the device), so a whole RTI step is one burst of launches on the stream
            int nact = 0;
            HIPCHK(hipMemcpyAsync(&nact, h->counter + 2, sizeof(int), hipMemcpyDeviceToHost, h->st));
            HIPCHK(hipStreamSynchronize(h->st));
            tl_flush(h);
            if (nact == 0) break;
        }
        const int tl_j = tl_begin(h, 3);
        if (linearize_impl(h, h->Xn, h->Un, SLSQP_DEVICE, h->scp_active, h->cl_steps)) return -1;   // update_jacobian for the next iteration (:138)
        tl_end(h, tl_j);
    }
    if (h->log_steps > 0 && h->cl_steps < h->log_steps) {
        hipLaunchKernelGGL(k_cl_log, dim3(1024), dim3(256), 0, h->st, cl_log_args(h, nullptr, nullptr, h->cl_steps));
        hipLaunchKernelGGL(k_cl_log_x0v, dim3((2 * h->B + 255) / 256), dim3(256), 0, h->st, h->B, h->log_steps, h->cl_steps, h->x0viol, h->qpstat, h->lg_x0v);
        h->named["log_x0_viol"] = {h->lg_x0v, sizeof(double) * 2 * (size_t)h->log_steps};      // (a slsqp_cl_run in between points the name at its own per-run buffer)
    }
    // plan fallback: one more launch, a wave per instance -- the plan of an instance that succeeded goes into its backup, one that
    // failed runs the backup's policy -- which writes the input to apply for every instance; the plant launch then takes that buffer as a one-stage plan
    // (the policy reads x_meas as the controller saw it, so its launch stands in front of everything that belongs to the plant: under
    // slsqp_cl_set_meas_noise k_cl_meas puts the truth there for the adversary and the plant step, and the next measurement behind them)
    ClArgs ap = op.fallback ? plant_args_on_u(h, a) : a;
    if (op.fallback && with_model(h, [&](auto M) {
            const bool log = h->log_steps > 0 && h->cl_steps < h->log_steps;
            HoldArgs ha{a, 0, h->A, h->Bm, h->K, h->Kc, h->stale, h->scp_success, h->hold_xi, h->hold_u, h->hold_policy, log ? h->log_steps : 0, h->cl_steps,
                        h->lg_state, h->lg_u0, h->lg_x0v, h->lg_it, h->lg_hold, h->lg_hpol};
            hold_args_on_backup(h, ha);
            hipLaunchKernelGGL((k_cl_plan_fallback<M()>), dim3(h->B), dim3(64), 0, h->st, ha, plan_args(h), 0);
        })) return -1;
    launch_meas(h, op, 0, h->cl_steps, nullptr, nullptr);
    if (op.adv) { if (launch_adversary(h, op, dw, h->cl_steps, nullptr, nullptr, nullptr)) return -1; ap.w = h->adv_w; }      // (x_meas stays as it is until the plant launch)
    if (with_model(h, [&](auto M) {
            if (op.pp) hipLaunchKernelGGL((k_cl_shift_plant_pp<M()>), dim3(gb), dim3(64), 0, h->st, ap, op.pa, h->cl_steps, nullptr, nullptr, nullptr);      // the plant has its own parameters
            else hipLaunchKernelGGL((k_cl_shift_plant<M()>), dim3(gb), dim3(64), 0, h->st, ap, 0, 1);
        })) return -1;
    launch_meas(h, op, 1, h->cl_steps, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    if (finish_enqueued(h, false)) return -1;
    h->cl_steps++;
    return 0;
}

// M of slsqp_cl_run (and of slsqp_cl_run_scp where it forwards to slsqp_cl_run's kernel): a property of the handle like x0_box_tol, default 1.
// 1 <= M <= N (K has N rows); anything else is refused and changes nothing.  slsqp_cl_step and slsqp_cl_hold_step do not read it.
extern "C" int slsqp_cl_set_solve_every(slsqp_handle *h, int M) {
    if (!cl_hold::valid_solve_every(M, h->d.N)) return fail("slsqp_cl_set_solve_every: M = " + std::to_string(M) + " outside 1 .. N = " + std::to_string(h->d.N) + " (K has N rows: at most N - 1 hold steps between two solves)");
    h->solve_every = M;
    return 0;
}
extern "C" int slsqp_cl_get_solve_every(slsqp_handle *h) { return h->solve_every; }
// theta of the event-triggered schedule of slsqp_cl_run with M > 1: a property of the handle, default +inf = off (the fixed
// period).  Anything outside [0, +inf], a NaN included, is refused and changes nothing.  slsqp_cl_step and slsqp_cl_hold_step do not read it.
extern "C" int slsqp_cl_set_hold_trigger(slsqp_handle *h, double theta) {
    if (!cl_hold::valid_trigger(theta)) return fail("slsqp_cl_set_hold_trigger: theta = " + std::to_string(theta) + " outside [0, +inf] (a fraction of the tube; +inf = off)");
    h->hold_trigger = theta;
    return 0;
}
extern "C" double slsqp_cl_get_hold_trigger(slsqp_handle *h) { return h->hold_trigger; }
// Plan fallback: a property of the handle, default 0 = off.  1: a step that applies no freshly certified plan (a solve that
// failed, a hold step) runs the tube policy of the instance's last plan that succeeded, read from a per-instance backup.  Read by slsqp_cl_step,
// slsqp_cl_hold_step and slsqp_cl_run (rti = 1 with one fast-SLS step: the compact gains).  Anything but 0 / 1 is refused and changes nothing.
extern "C" int slsqp_cl_set_plan_fallback(slsqp_handle *h, int on) {
    if (!cl_hold::valid_plan_fallback(on)) return fail("slsqp_cl_set_plan_fallback: " + std::to_string(on) + " is neither 0 (off) nor 1 (on)");
    h->plan_fallback = on;
    return 0;
}
extern "C" int slsqp_cl_get_plan_fallback(slsqp_handle *h) { return h->plan_fallback; }
// Fast-SLS converge mode inside the persistent launch: a property of the handle, default 0 = off.  1: slsqp_cl_run_scp takes
// opts.rti_steps <= 0 and runs it on the CONV variants of its kernel; with opts.rti_steps >= 1 it launches what it launches with the option off.
// Read by slsqp_cl_run_scp alone.  Anything but 0 / 1 is refused and changes nothing.
extern "C" int slsqp_cl_set_sls_converge(slsqp_handle *h, int on) {
    if (!cl_sls_conv::valid_option(on)) return fail("slsqp_cl_set_sls_converge: " + std::to_string(on) + " is neither 0 (off) nor 1 (on)");
    h->sls_converge = on;
    return 0;
}
extern "C" int slsqp_cl_get_sls_converge(slsqp_handle *h) { return h->sls_converge; }
// the allocation [the model's plant parameters (np) | model_err (B, nx) | adv_w (B, nx)] the persistent kernels' PP variants take for a handle that
// has an option of theirs on (adversary, measurement noise) and no plant parameters of its own; made by the first setter call that needs it
static int ensure_model_row(slsqp_handle *h, const char *who) {
    if (h->adv_buf) return 0;
    const int np = plant_params::count(h->model_id);
    const size_t nE = (size_t)h->B * h->d.nx;
    std::vector<double> dflt((size_t)np);
    for (int i = 0; i < np; i++) dflt[i] = plant_params::default_value(h->model_id, i);
    if (opt_install(who, &h->adv_buf, dflt, 2 * nE)) return -1;      // (model_err and adv_w behind the row, zeroed)
    h->adv_merr = h->adv_buf + np; h->adv_w = h->adv_merr + nE;
    return 0;
}
// State-feedback disturbance adversary (cl_adversary.hpp): a property of the handle, default off.  With a policy on, every plant
// step of slsqp_cl_step, slsqp_cl_hold_step, slsqp_cl_run and slsqp_cl_run_scp reads the sample the rule decides from the measured state, on the
// channels of `mask` (NULL: every channel); the caller's W stays the sample of every other channel.  policy = 0 clears it.  A refused call -- the
// message names the argument -- leaves the previous setting in force.
extern "C" int slsqp_cl_set_adversary(slsqp_handle *h, int policy, double amp, const unsigned char *mask) {
    std::string why;
    if (!cl_adversary::check(policy, amp, h->model_id >= 0, h->general_G, h->d.nx, &why)) return fail("slsqp_cl_set_adversary: " + why);
    hipSetDevice(h->dev);
    HIPCHK(hipStreamSynchronize(h->st));
    if (policy == cl_adversary::OFF) { h->adv_policy = cl_adversary::OFF; return 0; }
    if (ensure_model_row(h, "slsqp_cl_set_adversary")) return -1;
    h->adv_policy = policy; h->adv_amp = amp; h->adv_mask = cl_adversary::mask_bits(mask, h->d.nx);
    return 0;
}
extern "C" int slsqp_cl_get_adversary(slsqp_handle *h, int *policy, double *amp) {
    if (policy) *policy = h->adv_policy;
    if (amp) *amp = h->adv_amp;
    return 0;
}
// slsqp_get name of the adversary: w_applied (B,nx), the sample the last plant step under the option used (zeros on a handle that never had it on).
// Returns 1 when `name` was it and has been served, 0 when not, -1 on error.
static int get_adversary_named(slsqp_handle *h, const char *name, void *out, int loc) {
    if (strcmp(name, "w_applied")) return 0;
    HIPCHK(hipStreamSynchronize(h->st));
    const size_t n = (size_t)h->B * h->d.nx;
    if (h->adv_w) HIPCHK(hipMemcpy(out, h->adv_w, sizeof(double) * n, loc == SLSQP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
    else { const std::vector<double> z(n, 0.0); HIPCHK(hipMemcpy(out, z.data(), sizeof(double) * n, loc == SLSQP_HOST ? hipMemcpyHostToHost : hipMemcpyHostToDevice)); }
    return 1;
}

// Measurement noise (cl_meas.hpp): a property of the handle, default off.  Nm (T,nx) shared by the batch or (B,T,nx), the
// error of the measurement in state coordinates, row min(s, T - 1) for MPC step s counted from slsqp_cl_init; copied by the call.  T = 0 with
// Nm = NULL clears it.  The table is latched by slsqp_cl_init: a call between two of them changes nothing in the loop in progress.  A refused call --
// the message names the argument -- leaves the previous table in force.
extern "C" int slsqp_cl_set_meas_noise(slsqp_handle *h, const double *Nm, int T, int per_instance, int loc) {
    std::string why;
    if (!cl_meas::check(Nm, T, per_instance, loc, h->model_id >= 0, h->B, h->d.nx, &why)) return fail("slsqp_cl_set_meas_noise: " + why);
    hipSetDevice(h->dev);
    slsqp_handle::MeasTab &nx_ = h->mn_next;
    if (T == 0) {
        if (nx_.rows && nx_.rows != h->mn.rows) hipFree(nx_.rows);      // (a table no slsqp_cl_init has latched; the latched one is the loop's until the next slsqp_cl_init)
        nx_.rows = nullptr; nx_.T = 0; nx_.stride = 0; nx_.host.clear();
        return 0;
    }
    const size_t n = (size_t)(per_instance ? h->B : 1) * (size_t)T * h->d.nx;
    std::vector<double> host(n);
    if (opt_fetch(host, Nm, loc)) return -1;
    if (!cl_meas::check_entries(host.data(), T, per_instance, h->B, h->d.nx, &why)) return fail("slsqp_cl_set_meas_noise: " + why);
    if (ensure_model_row(h, "slsqp_cl_set_meas_noise")) return -1;
    if (!h->x_plant) {
        HIPCHK(hipMalloc((void **)&h->x_plant, sizeof(double) * (size_t)h->B * h->d.nx + 64));
        HIPCHK(hipMemset(h->x_plant, 0, sizeof(double) * (size_t)h->B * h->d.nx));
    }
    double *fresh = nullptr;      // (never the latched buffer: opt_install frees what the slot holds)
    if (opt_install("slsqp_cl_set_meas_noise", &fresh, host, 0, &nx_.host)) return -1;
    if (nx_.rows && nx_.rows != h->mn.rows) hipFree(nx_.rows);
    nx_.rows = fresh; nx_.T = T; nx_.stride = per_instance ? (size_t)T * h->d.nx : 0;
    return 0;
}
// slsqp_get names of the option: x_plant (B,nx), the true state (x_meas itself while the option is off); meas_noise (B,T,nx), the table in force (a
// shared one repeated; nothing while the option is off); log_plant_state / log_measured_state on a handle with the option off: copies of log_state,
// made here, then served like every log.  Returns 1 when `name` has been served, 0 when not (or not yet), -1 on error.
static int get_meas_named(slsqp_handle *h, const char *name, void *out, int loc) {
    const size_t n = (size_t)h->B * h->d.nx;
    if (!strcmp(name, "x_plant")) {
        HIPCHK(hipMemcpyAsync(out, h->mn.T > 0 ? h->x_plant : h->xmeas, sizeof(double) * n, loc == SLSQP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->st));
        HIPCHK(hipStreamSynchronize(h->st));
        return 1;
    }
    if (!strcmp(name, "meas_noise")) {
        if (h->mn.T == 0) return 1;
        const std::vector<double> v = opt_rows(h->B, &h->mn.host, h->mn.stride != 0, h->mn.T, h->d.nx, 0, h->d.nx, nullptr);
        HIPCHK(hipMemcpy(out, v.data(), sizeof(double) * v.size(), loc == SLSQP_HOST ? hipMemcpyHostToHost : hipMemcpyHostToDevice));
        return 1;
    }
    if (h->mn.T == 0 && h->lg_state && (!strcmp(name, "log_plant_state") || !strcmp(name, "log_measured_state")))
        HIPCHK(hipMemcpyAsync(!strcmp(name, "log_plant_state") ? h->lg_plant : h->lg_meas, h->lg_state, sizeof(double) * n * h->log_steps, hipMemcpyDeviceToDevice, h->st));
    return 0;
}

// One closed-loop step WITHOUT a solve: the one-stage shift slsqp_cl_step applies at its top, then k_cl_hold -- the tube policy
// of the last solve on the measured state, and the plant step.  No slsqp_reset (K stays valid); slsqp_cl_step is not involved and finds, at its next
// call, a nominal whose stage 0 is the plan's prediction of where the plant is.  The handle's solve_every is not read here: the caller decides which of
// its steps are solves.  (The persistent launch runs the same stages per instance: cl_step_begin / cl_step_end with HOLD.)
static int ensure_hold(slsqp_handle *h) {
    if (h->hold_xi) return 0;
    const size_t nxi = (size_t)h->B * (h->d.N + 1) * h->d.nx, nu = (size_t)h->B * h->d.nu;
    double *buf = nullptr; int *pol = nullptr;
    HIPCHK(hipMalloc((void **)&buf, sizeof(double) * (nxi + nu) + 64));
    if (hipMalloc((void **)&pol, sizeof(int) * 2 * h->B + 64) != hipSuccess || hipMemset(buf, 0, sizeof(double) * (nxi + nu)) != hipSuccess || hipMemset(pol, 0, sizeof(int) * 2 * h->B) != hipSuccess) {      // [hold_policy | hold_k]
        hipFree(buf); if (pol) hipFree(pol);
        return fail("slsqp_cl_hold_step: allocation failed");
    }
    h->hold_xi = buf; h->hold_u = buf + nxi; h->hold_policy = pol; h->hold_k = pol + h->B;
    return 0;
}
// Plan fallback: the backup store and the ages, allocated by the first step that runs with the option on, beside ensure_hold's
// buffers (the policy's column states and input are the hold steps').  No backup yet: every age -1.
static int ensure_plan(slsqp_handle *h) {
    if (ensure_hold(h)) return -1;
    if (h->plan_bk) return 0;
    size_t per = 0;
    for (int i = 0; i < 4; i++) per += plan_doubles(h, i);
    double *buf = nullptr; int *age = nullptr;
    HIPCHK(hipMalloc((void **)&buf, sizeof(double) * per * h->B + 64));
    if (hipMalloc((void **)&age, sizeof(int) * h->B + 64) != hipSuccess || hipMemset(buf, 0, sizeof(double) * per * h->B) != hipSuccess || hipMemset(age, 0xFF, sizeof(int) * h->B) != hipSuccess) {
        hipFree(buf); if (age) hipFree(age);
        return fail("slsqp_cl_set_plan_fallback: allocation of the backup plans failed");
    }
    h->plan_bk = buf; h->plan_age = age;
    return 0;
}
// the option's arguments (ensure_plan first) and the HoldArgs that go with them: the policy reads the backup
static PlanArgs plan_args(const slsqp_handle *h) {
    PlanArgs f;
    memset(&f, 0, sizeof f);
    f.on = 1;
    f.A = h->A; f.Bm = h->Bm; f.Kc = h->Kc; f.backoff_x = h->backoff_x;
    f.bA = plan_part(h, 0); f.bB = plan_part(h, 1); f.bKc = plan_part(h, 2); f.bbo = plan_part(h, 3);
    f.age = h->plan_age; f.lage = h->lg_age;
    return f;
}
static void hold_args_on_backup(const slsqp_handle *h, HoldArgs &a) { a.A = plan_part(h, 0); a.Bm = plan_part(h, 1); a.Kc = plan_part(h, 2); }
// the plant launch of a step under the option: "the first nominal input" of instance b is hold_u[b], the trick of k_cl_hold
static ClArgs plant_args_on_u(const slsqp_handle *h, ClArgs a) { a.N = 1; a.Un = h->hold_u; return a; }
const char *const FALLBACK_NEEDS = "plan fallback needs rti = 1 with one fast-SLS step";

extern "C" int slsqp_cl_hold_step(slsqp_handle *h, const double *w, int loc) {
    hipSetDevice(h->dev);
    std::string why;
    const int k = cl_hold::next_index(h->hold, h->model_id >= 0, h->cl_steps, h->d.N, loc, &why);
    if (!k) return fail("slsqp_cl_hold_step: " + why);
    const ClOptions op = cl_options(h);
    if (op.fallback ? ensure_plan(h) : ensure_hold(h)) return -1;
    const slsqp_dims &d = h->d;
    const int gb = (h->B + 63) / 64;
    const double *dw = nullptr;
    if (w) { if (put(h, h->wbuf, w, sizeof(double) * (size_t)h->B * d.nx, loc)) return -1; dw = h->wbuf; }
    // slsqp_cl_set_adversary: k_cl_adversary goes first (neither the shift nor the policy touches x_meas), and every plant step below reads adv_w
    // slsqp_cl_set_meas_noise: the policy reads the measurement and the adversary the truth, so the order is shift, policy (k_cl_hold_policy, or the
    // fallback's launch), k_cl_meas, adversary, the plant launch on u, k_cl_meas
    if (op.adv && !op.mn && launch_adversary(h, op, dw, h->cl_steps, nullptr, nullptr, nullptr)) return -1;
    const ClArgs a = cl_args(h, op.adv ? h->adv_w : dw);
    const bool log = h->log_steps > 0 && h->cl_steps < h->log_steps;
    HoldArgs ha{a, k, h->A, h->Bm, h->K, h->Kc, h->stale, h->scp_success, h->hold_xi, h->hold_u, h->hold_policy, log ? h->log_steps : 0, h->cl_steps,
                h->lg_state, h->lg_u0, h->lg_x0v, h->lg_it, h->lg_hold, h->lg_hpol};
    if (op.fallback) hold_args_on_backup(h, ha);      // (every instance at the index its backup's age gives; k is the batch's, for the log and for an instance without a plan)
    if (with_model(h, [&](auto M) {
            hipLaunchKernelGGL((k_cl_shift_plant<M()>), dim3(gb), dim3(64), 0, h->st, a, 1, 0);
            if (log) hipLaunchKernelGGL(k_cl_log, dim3(1024), dim3(256), 0, h->st, cl_log_args(h, nullptr, nullptr, h->cl_steps));      // nominal = the shifted plan, back-offs and success of the last solve; k_cl_hold writes the rest
            if (op.fallback || op.mn) {
                if (op.fallback) hipLaunchKernelGGL((k_cl_plan_fallback<M()>), dim3(h->B), dim3(64), 0, h->st, ha, plan_args(h), k);
                else hipLaunchKernelGGL((k_cl_hold_policy<M()>), dim3(h->B), dim3(64), 0, h->st, ha);
                launch_meas(h, op, 0, h->cl_steps, nullptr, nullptr);
                if (op.adv && op.mn) hipLaunchKernelGGL((k_cl_adversary<dyn::Dims<M()>::NX>), dim3(gb), dim3(64), 0, h->st, op.aa, h->B, h->xmeas, h->E, dw, h->cl_steps, (const int *)nullptr, (const int *)nullptr, (const double *)nullptr);
                const ClArgs au = plant_args_on_u(h, a);
                if (op.pp) hipLaunchKernelGGL((k_cl_shift_plant_pp<M()>), dim3(gb), dim3(64), 0, h->st, au, op.pa, h->cl_steps, nullptr, nullptr, nullptr);
                else hipLaunchKernelGGL((k_cl_shift_plant<M()>), dim3(gb), dim3(64), 0, h->st, au, 0, 1);
                launch_meas(h, op, 1, h->cl_steps, nullptr, nullptr);
            } else with_flag(op.pp, [&](auto PP) { hipLaunchKernelGGL((k_cl_hold<M(), PP()>), dim3(h->B), dim3(64), 0, h->st, ha, op.pa); });
        })) return -1;
    if (log) h->named["log_x0_viol"] = {h->lg_x0v, sizeof(double) * 2 * (size_t)h->log_steps};
    HIPCHK(hipGetLastError());
    if (finish_enqueued(h, false)) return -1;
    h->cl_steps++;
    cl_hold::on_hold(h->hold, k, h->cl_steps);
    return 0;
}

// The tube ratio of every instance for the hold step slsqp_cl_hold_step would run next (its refusals apply); +inf for an instance without a valid
// plan.  out (B).  Changes nothing in the handle.
extern "C" int slsqp_cl_tube_ratio(slsqp_handle *h, double *out, int loc) {
    hipSetDevice(h->dev);
    std::string why;
    const int k = cl_hold::next_index(h->hold, h->model_id >= 0, h->cl_steps, h->d.N, loc, &why);
    if (!k) return fail("slsqp_cl_tube_ratio: " + why);
    if (!out) return fail("slsqp_cl_tube_ratio: out is NULL");
    double *dout = loc == SLSQP_DEVICE ? out : stage_buf(h, sizeof(double) * (size_t)h->B);
    if (!dout) return -1;
    const ClArgs a = cl_args(h, nullptr);
    if (with_model(h, [&](auto M) { hipLaunchKernelGGL((k_cl_tube_ratio<M()>), dim3(h->B), dim3(64), 0, h->st, a, h->backoff_x, h->scp_success, k, dout); })) return -1;
    HIPCHK(hipGetLastError());
    if (loc != SLSQP_DEVICE) HIPCHK(hipMemcpyAsync(out, dout, sizeof(double) * (size_t)h->B, hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    return 0;
}

// ---- the whole closed loop with instances advancing independently ------------------------------------------------------------------
__global__ void k_cl_begin_flags(int B, const int *begin, int *scp_success, int *scp_iters) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && begin[b]) { scp_success[b] = 0; scp_iters[b] = 0; }
}
// the persistent closed-loop launch (k_cl_loop): as many waves as the GPU holds at the kernel's occupancy (or as there are instances)
// conv: the CONV variant of k_cl_loop_scp (fast-SLS converge mode; S only)
template <int MODEL>
static int launch_loop_t(slsqp_handle *h, bool S, bool conv = false) {
    constexpr int NX = dyn::Dims<MODEL>::NX, NU = dyn::Dims<MODEL>::NU;
    const ClOptions op = cl_options(h);      // (the bounds themselves are in the block: make_loop_block)
    // (HOLD: the hold function works in the same dynamic LDS -- the larger of the two sizes; which one binds per model: DESIGN.md section 20)
    const size_t lds = op.hold ? std::max(chain_lds_bytes<NX, NU>(h), sizeof(double) * (size_t)cl_hold_lds_doubles<MODEL>()) : chain_lds_bytes<NX, NU>(h);
    if (op.hold && S) return fail("no persistent closed-loop kernel for solve_every > 1 with several SCP iterations or fast-SLS steps per MPC step");
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, h->dev) != hipSuccess || cu <= 0) cu = 256;
    const int env_waves = getenv("SLSQP_LOOP_WAVES") ? atoi(getenv("SLSQP_LOOP_WAVES")) : 0;      // (tests / experiments: fewer waves than the GPU holds)
    const int slots = env_waves > 0 ? env_waves : cu * 4 * QP_PERSIST_WAVES_PER_SIMD;
    const int grid = std::max(1, std::min(h->B, slots));
    h->cl_loop_waves = grid;
    const ScpLoopArgs *blk = (const ScpLoopArgs *)h->loop_blk;
    bool found = false;
    timed_launch(h, [&] {
        hipEventRecord(h->ev[8], h->st);
        found = with_loop_var(op.var, [&](auto V) {
            if constexpr (var_hold(V())) hipLaunchKernelGGL((k_cl_loop<MODEL, V()>), dim3(grid), dim3(64), lds, h->st, blk, op.rf, op.pa);      // (k_cl_loop only: refused above for S)
            else if (S && conv) hipLaunchKernelGGL((k_cl_loop_scp<MODEL, V(), true>), dim3(grid), dim3(64), lds, h->st, blk, op.rf, op.pa);
            else if (S) hipLaunchKernelGGL((k_cl_loop_scp<MODEL, V()>), dim3(grid), dim3(64), lds, h->st, blk, op.rf, op.pa);      // (the general sweep's LDS, sweep_lds_doubles, is part of chain_lds_bytes)
            else hipLaunchKernelGGL((k_cl_loop<MODEL, V()>), dim3(grid), dim3(64), lds, h->st, blk, op.rf, op.pa);
        }, /* hold_sets */ !S);
        hipEventRecord(h->ev[9], h->st);
    });
    if (!found) return fail("no persistent closed-loop kernel for variant " + std::to_string(op.var));
    HIPCHK(hipGetLastError());
    return 0;
}
// the argument block of one persistent launch, composed of the builders' results (memset first: the block is copied and compared as bytes); no HIP call in
// here -- the x0 tolerance its QPs ask for is cl_run_persistent's to write
// sls_conv (the CONV variants of k_cl_loop_scp): rti_steps carries the cap opts.max_sls_iter of the fast-SLS loop
static ScpLoopArgs make_loop_block(slsqp_handle *h, int steps, const double *dW, const slsqp_opts &o, bool scp, int scp_rti, bool sls_conv = false) {
    const int max_it = !scp ? 1 : (scp_rti > 0 ? scp_rti : o.max_scp_iter);
    ScpLoopArgs S;
    memset(&S, 0, sizeof S);
    LoopArgs &L = S.L;
    const int *active = scp ? h->scp_active : nullptr;      // (k_cl_loop_scp masks an instance whose step failed for the rest of its MPC step, as slsqp_cl_step does)
    L.c = make_chain_args(h, o, active, 1);
    L.c.q.call_ids = h->call_ids;
    L.c.q.shift_stepno = h->cl_stepno;      // the horizon has moved for the instances past their first step
    L.c.qplog = h->qplog; L.c.x0vlog = h->x0vlog; L.c.stepno = h->cl_stepno; L.c.log_steps = h->qplog_steps;
    L.cl = cl_args(h, nullptr);
    L.lin = lin_args(h, h->Xn, h->Un, nullptr);
    L.ba = bounds_args(h, nullptr);
    L.sb = solve_begin_args(h, o, h->x0arg, active, nullptr);
    L.lg = cl_log_args(h, h->cl_stepno, nullptr, 0);
    L.sa = scp_args(h, o, 0, 0);
    L.steps = steps; L.n = h->n; L.have_log = h->log_steps > 0 ? 1 : 0;
    L.keep_laggards = getenv("SLSQP_LOOP_KEEP") ? atoi(getenv("SLSQP_LOOP_KEEP")) : 1;
    L.fence = getenv("SLSQP_LOOP_FENCE") ? atoi(getenv("SLSQP_LOOP_FENCE")) : 3;      // (experiments only: 0 drops the hand-over fences)
    L.stepno = h->cl_stepno; L.call_ids = h->call_ids; L.q = h->q; L.stale = h->stale; L.itnum = h->itnum; L.pending = h->pending_reset; L.scp_active = h->scp_active;
    L.W_all = dW; L.pinf = h->pinf;
    L.Q = ClQueue{h->clq_slots, h->clq_cap - 1u, (unsigned *)h->clq_ctl, (unsigned *)h->clq_ctl + 1, h->clq_ctl + 2, h->clq_ctl + 3};
    L.busy = h->cl_busy; L.t_begin = h->cl_tbegin;
    S.max_it = max_it; S.converge = scp_rti <= 0 ? 1 : 0; S.rti_steps = sls_conv ? o.max_sls_iter : o.rti_steps; S.nsolves = h->qplog_nsolves;
    if (cl_options(h).bnd) { S.bd.rows = h->bnd_rows; S.bd.T = h->bnd_T; S.bd.stride = h->bnd_stride; S.bd.stepno = h->cl_stepno; S.bd.step = 0; }      // (field by field: the padding stays zero; all zero bytes without bounds, and never read)
    return S;
}
// the block goes to the handle's device buffer on the handle's stream, ahead of the launch that reads it (and behind the previous launch, which may
// still be reading the previous contents: stream order).  loop_blk_host keeps the bytes in memory the handle owns; every persistent run ends with a
// synchronisation of the stream, so the previous copy out of it has been taken
static void stage_loop_block(slsqp_handle *h, const ScpLoopArgs &S) {
    static_assert(sizeof(ScpLoopArgs) <= 4096, "slsqp_handle::loop_blk is 4096 bytes");
    h->loop_blk_host.resize(sizeof S);
    memcpy(h->loop_blk_host.data(), &S, sizeof S);
}
static int write_loop_block(slsqp_handle *h, const ScpLoopArgs &S) {
    stage_loop_block(h, S);
    HIPCHK(hipMemcpyAsync(h->loop_blk, h->loop_blk_host.data(), sizeof S, hipMemcpyHostToDevice, h->st));
    return 0;
}
// what the HOLD variants read behind it (no HIP call in here; the buffers are ensure_hold's): the HoldArgs slsqp_cl_hold_step passes, with the log
// of a run -- every instance at its own entry -- and M
static HoldLoopArgs make_hold_block(slsqp_handle *h) {
    HoldLoopArgs H;
    memset(&H, 0, sizeof H);
    HoldArgs &a = H.a;
    a.cl = cl_args(h, nullptr);
    a.A = h->A; a.Bm = h->Bm; a.K = h->K; a.Kc = h->Kc; a.stale = h->stale; a.scp_success = h->scp_success;
    a.xi = h->hold_xi; a.u = h->hold_u; a.policy = h->hold_policy;
    a.S = h->log_steps;
    a.lstate = h->lg_state; a.lu0 = h->lg_u0; a.lx0v = h->lg_x0v; a.lit = h->lg_it; a.lhold = h->lg_hold; a.lpol = h->lg_hpol;      // (lx0v: the log's own buffer; the run's log_x0_viol is the block's x0vlog)
    H.M = h->solve_every;
    H.theta = h->hold_trigger; H.backoff_x = h->backoff_x; H.hold_k = h->hold_k; H.lratio = h->lg_ratio; H.ltrig = h->lg_trig;
    if (h->plan_fallback) { hold_args_on_backup(h, a); H.backoff_x = plan_part(h, 3); }      // (ensure_plan has run: the policy and the trigger's ratio read the backup)
    return H;
}
static int write_hold_block(slsqp_handle *h, const HoldLoopArgs &H) {
    h->hold_blk_host.resize(sizeof H);
    memcpy(h->hold_blk_host.data(), &H, sizeof H);
    HIPCHK(hipMemcpyAsync(h->loop_blk + HOLD_BLK_OFFSET, h->hold_blk_host.data(), sizeof H, hipMemcpyHostToDevice, h->st));
    return 0;
}
// the PlanArgs behind the hold block: written when the option is on, and once more, as zero bytes, by the first HOLD launch after it was switched off
// (the buffer starts as zeros: a handle that never had the option on writes nothing here)
static int write_plan_block(slsqp_handle *h, bool on) {
    if (!on && !h->plan_blk_dev) return 0;
    PlanArgs f;
    memset(&f, 0, sizeof f);
    if (on) f = plan_args(h);
    h->plan_blk_host.resize(sizeof f);
    memcpy(h->plan_blk_host.data(), &f, sizeof f);
    HIPCHK(hipMemcpyAsync(h->loop_blk + PLAN_BLK_OFFSET, h->plan_blk_host.data(), sizeof f, hipMemcpyHostToDevice, h->st));
    h->plan_blk_dev = on ? 1 : 0;
    return 0;
}
// what the CONV variants of k_cl_loop_scp read behind the plan block (no HIP call in make_conv_block; the buffer is cl_run_prepare's): the run's two
// per-step arrays, indexed with the run's own step count as log_qp_stats is
static SlsConvArgs make_conv_block(const slsqp_handle *h) {
    SlsConvArgs V;
    memset(&V, 0, sizeof V);
    V.itlog = h->sls_itlog; V.lastit = h->sls_itlog + (size_t)h->B * h->qplog_cap; V.log_steps = h->qplog_steps;
    return V;
}
static int write_conv_block(slsqp_handle *h, const SlsConvArgs &V) {
    h->conv_blk_host.resize(sizeof V);
    memcpy(h->conv_blk_host.data(), &V, sizeof V);
    HIPCHK(hipMemcpyAsync(h->loop_blk + CONV_BLK_OFFSET, h->conv_blk_host.data(), sizeof V, hipMemcpyHostToDevice, h->st));
    return 0;
}
// the AdvArgs behind the CONV block (slsqp_cl_set_adversary): written by the runs with the option on, and once more, as zero bytes, by the first
// persistent launch after it was switched off (the buffer starts as zeros: a handle that never had the option on writes nothing here)
static int write_adv_block(slsqp_handle *h, bool on) {
    if (!on && !h->adv_blk_dev) return 0;
    AdvArgs A;
    memset(&A, 0, sizeof A);
    if (on) A = adv_args(h);
    h->adv_blk_host.resize(sizeof A);
    memcpy(h->adv_blk_host.data(), &A, sizeof A);
    HIPCHK(hipMemcpyAsync(h->loop_blk + ADV_BLK_OFFSET, h->adv_blk_host.data(), sizeof A, hipMemcpyHostToDevice, h->st));
    h->adv_blk_dev = on ? 1 : 0;
    return 0;
}
// the cl_meas::Args behind the adversary's block (slsqp_cl_set_meas_noise), written as write_adv_block writes its own
static int write_meas_block(slsqp_handle *h, bool on) {
    if (!on && !h->mn_blk_dev) return 0;
    MeasArgs A;
    memset(&A, 0, sizeof A);
    if (on) A = meas_args(h);
    h->mn_blk_host.resize(sizeof A);
    memcpy(h->mn_blk_host.data(), &A, sizeof A);
    HIPCHK(hipMemcpyAsync(h->loop_blk + MEAS_BLK_OFFSET, h->mn_blk_host.data(), sizeof A, hipMemcpyHostToDevice, h->st));
    h->mn_blk_dev = on ? 1 : 0;
    return 0;
}
// scp = false: k_cl_loop (one SCP iteration, one fast-SLS step per MPC step); true: k_cl_loop_scp with scp_rti (slsqp_cl_run_scp), sls_conv: its CONV
// variant (fast-SLS converge mode, opts.max_sls_iter the cap; slsqp_cl_set_sls_converge)
static int cl_run_persistent(slsqp_handle *h, int steps, const double *dW, const slsqp_opts &o, int *rounds_out, bool scp = false, int scp_rti = 1, bool sls_conv = false) {
    const int max_it = !scp ? 1 : (scp_rti > 0 ? scp_rti : o.max_scp_iter);
    const slsqp_dims &d = h->d;
    const int B = h->B;
    if (!h->beta_inited) {      // what the handle's first solve does once: beta = eps everywhere (later solves only repair swept instances)
        hipLaunchKernelGGL(k_fill_doubles, dim3(1024), dim3(256), 0, h->st, h->beta, o.eps_backoff, (size_t)B * d.N * d.N * d.ni);
        hipLaunchKernelGGL(k_fill_doubles, dim3(1024), dim3(256), 0, h->st, h->beta_f, o.eps_backoff, (size_t)B * (d.N + 1) * d.ni_f);
        h->beta_inited = true;
    }
    h->time_kernels = o.time_kernels != 0;
    set_x0_tol(h, h->x0_box_tol);
    const ScpLoopArgs S = make_loop_block(h, steps, dW, o, scp, scp_rti, sls_conv);
    const LoopArgs &L = S.L;
    if (write_loop_block(h, S)) return -1;
    if (sls_conv && write_conv_block(h, make_conv_block(h))) return -1;
    if (write_adv_block(h, h->adv_policy != cl_adversary::OFF)) return -1;
    if (write_meas_block(h, h->mn.T > 0)) return -1;
    const int M = scp ? 1 : h->solve_every;      // (slsqp_cl_run_scp has refused M > 1 for its own kernel)
    const bool fallback = !scp && h->plan_fallback;      // (slsqp_cl_run_scp has refused the option for its own kernel)
    if ((M > 1 || fallback) && ((fallback ? ensure_plan(h) : ensure_hold(h)) || write_hold_block(h, make_hold_block(h)) || write_plan_block(h, fallback))) return -1;
    const bool triggered = cl_hold::trigger_on(h->hold_trigger, M);      // every instance on its own schedule: its first step is a solve
    if (triggered) HIPCHK(hipMemsetAsync(h->hold_k, 0, sizeof(int) * (size_t)B, h->st));
    hipLaunchKernelGGL(k_clq_init, dim3(64), dim3(256), 0, h->st, B, L.Q);
    HIPCHK(hipMemsetAsync(h->cl_busy, 0, 16 * sizeof(unsigned long long), h->st));
    HIPCHK(hipMemsetAsync(h->cl_busy + 14, 0xFF, sizeof(unsigned long long), h->st));      // (CL_LOOP_STAMP builds: earliest wave start)
    HIPCHK(hipMemsetAsync(h->counter + 2, 0, sizeof(int), h->st));
    const int tl_tot = tl_begin(h, 2), tl_c = tl_begin(h, 4);
    int rc = -1;
    if (with_model(h, [&](auto M) { rc = launch_loop_t<M()>(h, scp, sls_conv); }) || rc) return -1;
    if (scp && S.converge) hipLaunchKernelGGL(k_cl_qplog_masked, dim3(steps), dim3(256), 0, h->st, B, steps, h->qplog_steps, h->qplog_nsolves, h->qplog, h->x0vlog);
    if (sls_conv) hipLaunchKernelGGL(k_cl_qplog_sls_conv, dim3(steps), dim3(256), 0, h->st, B, steps, h->qplog_steps, S.rti_steps, h->qplog_nsolves, h->sls_itlog + (size_t)B * h->qplog_cap, h->qplog, h->x0vlog);
    tl_end(h, tl_c); tl_end(h, tl_tot);
    int ctl[4] = {0, 0, 0, 0};
    std::vector<int> sn((size_t)B);
    HIPCHK(hipMemcpyAsync(ctl, h->clq_ctl, sizeof(ctl), hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipMemcpyAsync(sn.data(), h->cl_stepno, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipMemcpyAsync(h->cl_busy_host, h->cl_busy, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->st));
    if (h->chain_times_host) {
        if (scp) memset(h->chain_times_host, 0, 4 * sizeof(unsigned long long));      // (no per-part clock in the general step: the launch counts as QP time)
        else HIPCHK(hipMemcpyAsync(h->chain_times_host, h->chain_times, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->st));
    }
    if (finish_enqueued(h, false)) return -1;
    h->cl_loop_ms = ev_ms(h->ev[8], h->ev[9]);
    h->have_dyn = true;
    int unfinished = 0;
    for (int b = 0; b < B; b++) unfinished += sn[b] < steps ? 1 : 0;
    if (ctl[3] != 0 || unfinished != 0)
        return fail("slsqp_cl_run (persistent): the instance queue did not drain (err " + std::to_string(ctl[3]) + ", " + std::to_string(unfinished) + " instances short of their steps)");
    h->cl_steps = steps;
    if (triggered) {      // the solves per instance are the run's to decide: the ids stay distinct and increasing under the upper bound; "hold_index": the device array
        cl_hold::on_triggered_run(h->hold, h->cl_steps);
        h->call_id += (double)steps * max_it;
    } else {
        cl_hold::on_run(h->hold, h->cl_steps, cl_hold::hold_index_at(steps - 1, M));      // (no per-batch plan: slsqp_cl_hold_step refuses until a slsqp_cl_step; "hold_index": the last step's)
        h->call_id += (double)cl_hold::solves_in(steps, M) * max_it;
    }
    if (rounds_out) *rounds_out = 1;
    return 0;
}
// wave statistics of the last persistent slsqp_cl_run: [0] waves launched, [1] sum over the MPC steps of the time a wave spent on them (ms),
// [2] MPC steps run, [3] duration of the launch (ms; HIP events, opts.time_kernels)
extern "C" int slsqp_cl_run_stats(slsqp_handle *h, double *out, int len) {
    if (!out || len < SLSQP_CL_RUN_STATS_LEN) return fail("slsqp_cl_run_stats: the buffer must hold SLSQP_CL_RUN_STATS_LEN (4) doubles");
    out[0] = (double)h->cl_loop_waves; out[1] = (double)h->cl_busy_host[0] * 1e-5; out[2] = (double)h->cl_busy_host[2]; out[3] = h->cl_loop_ms;
    for (int i = 4; i < 16 && i < len; i++) out[i] = (double)h->cl_busy_host[i] * 1e-5;
    if (len >= 16) { out[14] = (double)(h->cl_busy_host[15] - h->cl_busy_host[14]) * 1e-5; out[15] = (double)h->cl_busy_host[1]; }      // first wave start -> last wave exit; waves that ran      // -DCL_LOOP_STAMP builds: ms spent in the parts of the step around the chain
    return 0;
}

// what both closed-loop entry points do before their loop: disturbance samples on the device, the per-step qp_stats log of THIS run (registered and
// indexed with the run's own step count; the allocation only grows), step counters, call ids
static int cl_run_prepare(slsqp_handle *h, int steps, const double *W, int loc, const double **dW_out) {
    const slsqp_dims &d = h->d;
    const int B = h->B;
    const double *dW = nullptr;
    if (W) {
        const size_t nW = (size_t)steps * B * d.nx;
        if (loc == SLSQP_HOST) {
            if (nW > h->cl_W_doubles) { if (h->cl_W) hipFree(h->cl_W); h->cl_W = nullptr; h->cl_W_doubles = 0; HIPCHK(hipMalloc((void **)&h->cl_W, nW * sizeof(double) + 64)); h->cl_W_doubles = nW; }
            HIPCHK(hipMemcpyAsync(h->cl_W, W, nW * sizeof(double), hipMemcpyHostToDevice, h->st));
            dW = h->cl_W;
        } else dW = W;
    }
    if (h->qplog_cap < steps) {
        if (h->qplog) hipFree(h->qplog);
        if (h->x0vlog) hipFree(h->x0vlog);
        if (h->qplog_nsolves) hipFree(h->qplog_nsolves);
        if (h->sls_itlog) hipFree(h->sls_itlog);
        h->qplog = nullptr; h->x0vlog = nullptr; h->qplog_nsolves = nullptr; h->sls_itlog = nullptr; h->qplog_cap = 0; h->qplog_steps = 0;
        HIPCHK(hipMalloc((void **)&h->qplog, (size_t)B * steps * 16 * sizeof(int) + 64));
        HIPCHK(hipMalloc((void **)&h->x0vlog, (size_t)B * steps * 2 * sizeof(double) + 64));
        HIPCHK(hipMalloc((void **)&h->qplog_nsolves, (size_t)B * steps * sizeof(int) + 64));
        HIPCHK(hipMalloc((void **)&h->sls_itlog, (size_t)B * steps * 2 * sizeof(int) + 64));
        h->qplog_cap = steps;
    }
    h->qplog_steps = steps;
    HIPCHK(hipMemsetAsync(h->qplog, 0, (size_t)B * steps * 16 * sizeof(int), h->st));
    HIPCHK(hipMemsetAsync(h->qplog_nsolves, 0, (size_t)B * steps * sizeof(int), h->st));
    HIPCHK(hipMemsetAsync(h->sls_itlog, 0, (size_t)B * h->qplog_cap * 2 * sizeof(int), h->st));
    HIPCHK(hipMemsetAsync(h->x0vlog, 0, (size_t)B * steps * 2 * sizeof(double), h->st));
    h->named["log_qp_stats"] = {h->qplog, sizeof(int) * 16 * (size_t)steps};
    h->named["log_x0_viol"] = {h->x0vlog, sizeof(double) * 2 * (size_t)steps};
    h->named["log_sls_iterations"] = {h->sls_itlog, sizeof(int) * (size_t)steps};      // written by the CONV variants of k_cl_loop_scp alone (slsqp_cl_set_sls_converge): zeros from every other run
    HIPCHK(hipMemsetAsync(h->cl_stepno, 0, sizeof(int) * B, h->st));
    HIPCHK(hipMemsetAsync(h->cl_lag, 0, sizeof(int) * B, h->st));
    hipLaunchKernelGGL(k_fill_doubles, dim3(64), dim3(256), 0, h->st, h->call_ids, h->call_id, (size_t)B);
    *dW_out = dW;
    return 0;
}

// `steps` MPC steps of every instance (rti = 1 with one fast-SLS step: the rocket script's setting), W (steps, B, nx) or NULL.  Per instance the
// same sequence of operations as `steps` calls of slsqp_cl_step -- same bits -- but no instance waits for another: the loop runs in ROUNDS (one
// burst of launches each); in a round an instance either begins its next MPC step (shift, reset, linearise, chain, nominal update, plant) or
// resumes the QP solve a previous round's deadline suspended; a chain that is not done `budget_ms` after its launch started suspends itself
// between two block solves and the instance simply takes part in the next round where it stopped.  A batch-wide step lasts as long as its slowest
// instance (50-90 block solves against a mean of 20: two thirds of a step's time is spent waiting for a few per cent of the instances); a round
// lasts budget_ms at most, and ends earlier once cut_frac of its participants are done (0 < cut_frac < 1; the stragglers of a round then are cut as soon
// as the bulk has finished, whatever time that took).  budget_ms <= 0: no time limit.  Results: the device-side log (slsqp_cl_log with max_steps >= steps), the final state, and log_qp_stats (steps, 2, 8).
// slsqp_cl_set_solve_every with M > 1: the persistent launch runs k_cl_loop's HOLD variant -- steps 0, M, 2M, ... of an instance are solves, the others the
// hold step of slsqp_cl_hold_step inside the loop of the wave that holds the instance; the rounds refuse.  M = 1: exactly the launches above.
extern "C" int slsqp_cl_run(slsqp_handle *h, int steps, const double *W, int loc, const slsqp_opts *opts, double budget_ms, double cut_frac, int *rounds_out) {
    hipSetDevice(h->dev);
    if (h->model_id < 0) return fail("slsqp_set_model must be called first");
    if (h->cl_steps != 0) return fail("slsqp_cl_run starts a closed loop: call slsqp_cl_init first");
    if (steps < 1) return fail("slsqp_cl_run: steps must be >= 1");
    if (h->log_steps > 0 && h->log_steps < steps) return fail("slsqp_cl_run: the device-side log (slsqp_cl_log) is shorter than the run");
    slsqp_opts o;
    if (opts) o = *opts; else slsqp_default_opts(&o);
    if (h->solve_waves > 1) return fail("slsqp_cl_run: the persistent loop is one wave per instance: solve_waves must be 1 (use slsqp_cl_step with solve_waves > 1)");
    h->ne_waves = 0;      // (slsqp_ne_solve's factors do not survive a QP solve)
    if (!(o.rti_steps == 1 && o.precision == 0 && o.fuse_rti && chain_allowed() && sweep_shared_allowed()) || h->general_G)
        return fail("slsqp_cl_run needs the fused RTI chain: rti_steps = 1, fp64, fuse_rti = 1, box constraints (use slsqp_cl_step otherwise)");
    const int B = h->B, gbi = (B + 255) / 256, gb = (B + 63) / 64;
    const double *dW = nullptr;
    if (h->solve_every > 1 && !o.cl_persistent)
        return fail("slsqp_cl_run: solve_every = " + std::to_string(h->solve_every) + " runs in the persistent launch only (cl_persistent = 1): the round-based loop solves at every step (use slsqp_cl_step / slsqp_cl_hold_step)");
    if (h->plan_fallback && !o.cl_persistent)
        return fail("slsqp_cl_run: plan fallback runs in the persistent launch only (cl_persistent = 1): the round-based loop applies the nominal input of a failed step (use slsqp_cl_step / slsqp_cl_hold_step)");
    if (cl_run_prepare(h, steps, W, loc, &dW)) return -1;
    if (o.cl_persistent) return cl_run_persistent(h, steps, dW, o, rounds_out);
    h->cl_budget = budget_ms > 0.0 ? (unsigned long long)(std::max(0.05, budget_ms) * 1e5) : (1ULL << 62);
    h->cl_total_steps = steps;
    ClArgs a = cl_args(h, nullptr);
    const ClOptions op = cl_options(h);
    int rounds = 0;
    const int max_rounds = 40 * steps + 100;
    for (;; rounds++) {
        int unfinished = 0;
        HIPCHK(hipMemsetAsync(h->counter + 1, 0, sizeof(int), h->st));
        hipLaunchKernelGGL(k_cl_round_masks, dim3(gbi), dim3(256), 0, h->st, B, steps, h->cl_stepno, h->cl_lag, h->cl_begin, h->cl_runm, h->cl_skipb, h->cl_done, h->counter + 1);
        HIPCHK(hipMemcpyAsync(&unfinished, h->counter + 1, sizeof(int), hipMemcpyDeviceToHost, h->st));
        HIPCHK(hipStreamSynchronize(h->st));
        tl_flush(h);
        if (unfinished == 0) break;
        h->cl_cut_count = (cut_frac > 0.0 && cut_frac < 1.0) ? (unsigned)std::max(1.0, std::ceil(cut_frac * unfinished)) : 0xFFFFFFFFu;
        if (rounds >= max_rounds) { h->cl_round = false; h->cl_skip_begin = nullptr; return fail("slsqp_cl_run: round limit reached"); }
        // begin: reset_warm_start (shift + solver reset) for the instances past their first step
        if (with_model(h, [&](auto M) { hipLaunchKernelGGL((k_cl_shift_plant<M()>), dim3(gb), dim3(64), 0, h->st, a, 1, 0, h->cl_begin, h->cl_stepno, nullptr); })) return -1;
        hipLaunchKernelGGL(k_cl_reset_masked, dim3(B), dim3(256), 0, h->st, B, h->n, h->cl_begin, h->cl_stepno, h->stale, h->itnum, h->pending_reset, h->q);
        hipLaunchKernelGGL(k_cl_bump_call, dim3(gbi), dim3(256), 0, h->st, B, h->cl_begin, h->call_ids);
        hipLaunchKernelGGL(k_cl_begin_flags, dim3(gbi), dim3(256), 0, h->st, B, h->cl_begin, h->scp_success, h->scp_iters);
        h->have_dyn = false;
        {
            const int tl_j = tl_begin(h, 3);
            if (linearize_impl(h, h->Xn, h->Un, SLSQP_DEVICE, h->cl_begin, 0, h->cl_stepno)) return -1;
            tl_end(h, tl_j);
        }
        hipLaunchKernelGGL(k_cl_x0arg, dim3(64), dim3(256), 0, h->st, a, h->cl_begin);
        h->horizon_shifted = rounds > 0 ? 1 : 0;
        h->cl_round = true; h->cl_skip_begin = h->cl_skipb;
        const BndArgs bd = bnd_args(h, 0, h->cl_stepno);
        const int rc = solve_impl(h, h->x0arg, SLSQP_DEVICE, &o, h->cl_runm, /* no_sync */ true, op.bnd ? &bd : nullptr);
        h->cl_round = false; h->cl_skip_begin = nullptr;
        if (rc) return -1;
        // end of the step for the instances whose chain is done: nominal += delta, primal_infeasibility, log entry, plant + noise, step counter
        hipLaunchKernelGGL(k_copy_int, dim3(gbi), dim3(256), 0, h->st, h->cl_done, h->scp_active, B);
        HIPCHK(hipMemsetAsync(h->counter + 2, 0, sizeof(int), h->st));
        hipLaunchKernelGGL(k_cl_scp_update, dim3(B), dim3(64), 0, h->st, a, scp_args(h, o, 0, 0));
        if (with_model(h, [&](auto M) { hipLaunchKernelGGL((k_cl_infeas<M()>), dim3(B), dim3(64), 0, h->st, a, h->scp_upd, h->pinf); })) return -1;
        if (h->log_steps > 0) hipLaunchKernelGGL(k_cl_log, dim3(1024), dim3(256), 0, h->st, cl_log_args(h, h->cl_stepno, h->cl_done, 0));
        // slsqp_cl_set_adversary: every instance of the round's mask gets the sample of ITS step decided from its x_meas, and the plant launch reads adv_w
        ClArgs aw = a;
        launch_meas(h, op, 0, 0, h->cl_done, h->cl_stepno);      // slsqp_cl_set_meas_noise: around the plant launch, for the instances of its mask at THEIR step
        if (op.adv) { if (launch_adversary(h, op, nullptr, 0, h->cl_done, h->cl_stepno, dW)) return -1; aw.w = h->adv_w; }
        const double *pW = op.adv ? nullptr : dW;
        if (with_model(h, [&](auto M) {
                if (op.pp) hipLaunchKernelGGL((k_cl_shift_plant_pp<M()>), dim3(gb), dim3(64), 0, h->st, aw, op.pa, 0, h->cl_done, h->cl_stepno, pW);
                else hipLaunchKernelGGL((k_cl_shift_plant<M()>), dim3(gb), dim3(64), 0, h->st, aw, 0, 1, h->cl_done, h->cl_stepno, pW);
            })) return -1;
        launch_meas(h, op, 1, 0, h->cl_done, h->cl_stepno);
        hipLaunchKernelGGL(k_cl_advance, dim3(gbi), dim3(256), 0, h->st, B, h->cl_done, h->cl_stepno, h->call_ids, h->cl_begin);
        HIPCHK(hipGetLastError());
    }
    tl_take(h);
    h->cl_steps = steps;
    cl_hold::on_run(h->hold, h->cl_steps);
    h->call_id += steps;
    if (rounds_out) *rounds_out = rounds;
    return 0;
}

// `steps` MPC steps of every instance as ONE persistent launch for any SCP setting of slsqp_cl_step (SCP_SLS.solve, SCP_SLS_jit.py:103-135, around
// fast_SLS.solve in RTI mode, fast_SLS_jit.py:278-296): rti > 0 -> exactly rti SCP iterations per MPC step, rti <= 0 -> converge mode
// (opts.scp_eps, opts.max_scp_iter), opts.rti_steps >= 1 fast-SLS steps per solve.  Per instance the same operations in the same order as
// `steps` calls of slsqp_cl_step(h, rti, ...): same bits.  rti = 1 with rti_steps = 1 is slsqp_cl_run's own kernel.
extern "C" int slsqp_cl_run_scp(slsqp_handle *h, int steps, int rti, const double *W, int loc, const slsqp_opts *opts) {
    hipSetDevice(h->dev);
    if (h->model_id < 0) return fail("slsqp_set_model must be called first");
    if (h->cl_steps != 0) return fail("slsqp_cl_run_scp starts a closed loop: call slsqp_cl_init first");
    if (steps < 1) return fail("slsqp_cl_run_scp: steps must be >= 1");
    if (h->log_steps > 0 && h->log_steps < steps) return fail("slsqp_cl_run_scp: the device-side log (slsqp_cl_log) is shorter than the run");
    slsqp_opts o;
    if (opts) o = *opts; else slsqp_default_opts(&o);
    if (h->solve_waves > 1) return fail("slsqp_cl_run_scp: the persistent loop is one wave per instance: solve_waves must be 1 (use slsqp_cl_step with solve_waves > 1)");
    h->ne_waves = 0;      // (slsqp_ne_solve's factors do not survive a QP solve)
    const bool sls_conv = o.rti_steps <= 0 && h->sls_converge;      // (slsqp_cl_set_sls_converge: the CONV variants of k_cl_loop_scp)
    if (const char *why = cl_sls_conv::run_scp_refusal(o.rti_steps, h->sls_converge, o.max_sls_iter)) return fail(why);
    if (o.precision != 0) return fail("slsqp_cl_run_scp: mixed precision (precision = 1) does not run inside the persistent loop: fp64 only (use slsqp_cl_step)");
    if (h->general_G) return fail("slsqp_cl_run_scp: box constraints only (general G: use the sweep-level boundary)");
    if (!(o.fuse_rti && chain_allowed() && sweep_shared_allowed())) return fail("slsqp_cl_run_scp needs the fused chain: fuse_rti = 1, SLSQP_FUSE_RTI and SLSQP_SWEEP_SHARED not 0 (use slsqp_cl_step otherwise)");
    if (rti <= 0 && o.max_scp_iter < 1) return fail("slsqp_cl_run_scp: converge mode needs max_scp_iter >= 1");
    if (h->solve_every > 1 && !(rti == 1 && o.rti_steps == 1))
        return fail("slsqp_cl_run_scp: solve_every = " + std::to_string(h->solve_every) + " needs rti = 1 with one fast-SLS step (slsqp_cl_run's kernel): the general persistent loop keeps its gains per SCP iteration and solves at every step (use slsqp_cl_step / slsqp_cl_hold_step)");
    if (h->plan_fallback && !(rti == 1 && o.rti_steps == 1))
        return fail(std::string("slsqp_cl_run_scp: ") + FALLBACK_NEEDS + " (slsqp_cl_run's kernel): the backup keeps the compact gains, the general persistent loop keeps its gains per SCP iteration");
    const double *dW = nullptr;
    if (cl_run_prepare(h, steps, W, loc, &dW)) return -1;
    if (rti == 1 && o.rti_steps == 1) return cl_run_persistent(h, steps, dW, o, nullptr);
    return cl_run_persistent(h, steps, dW, o, nullptr, true, rti, sls_conv);
}

// ---- QP-level boundary (osqp_generated look-alike, batched) -------------------------------------------------
extern "C" int slsqp_qp_update_data_mat(slsqp_handle *h, const double *P_x, const double *A_x, int loc) {
    hipSetDevice(h->dev);
    const slsqp_dims &d = h->d;
    int n, m, nnzP, nnzA;
    slsqp_qp_nnz(&d, &n, &m, &nnzP, &nnzA);
    if (P_x) {   // diagonal of 2*blkdiag(Q,R,...,Qf): take instance 0 (weights are batch-constant)
        std::vector<double> p0(n);
        HIPCHK(hipMemcpy(p0.data(), P_x, sizeof(double) * n, loc == SLSQP_HOST ? hipMemcpyHostToHost : hipMemcpyDeviceToHost));
        std::vector<double> cur(2 * d.nx + d.nu);
        for (int i = 0; i < d.nx; i++) cur[i] = 0.5 * p0[i];
        for (int i = 0; i < d.nu; i++) cur[d.nx + i] = 0.5 * p0[d.nx + i];
        for (int i = 0; i < d.nx; i++) cur[d.nx + d.nu + i] = 0.5 * p0[(size_t)h->nz * d.N + i];
        HIPCHK(hipMemcpy(h->cst, cur.data(), sizeof(double) * cur.size(), hipMemcpyHostToDevice));
        h->have_costs = true;
    }
    if (A_x) {
        const double *src = A_x;
        if (loc == SLSQP_HOST) {
            double *tmp = stage_buf(h, sizeof(double) * (size_t)h->B * nnzA);
            if (!tmp) return -1;
            HIPCHK(hipMemcpyAsync(tmp, A_x, sizeof(double) * (size_t)h->B * nnzA, hipMemcpyHostToDevice, h->st));
            src = tmp;
        }
        hipLaunchKernelGGL(k_gather_csc, dim3(1024), dim3(256), 0, h->st, h->B, d.N * d.nx * d.nx, nnzA, h->mapA, src, h->A);
        hipLaunchKernelGGL(k_gather_csc, dim3(1024), dim3(256), 0, h->st, h->B, d.N * d.nx * d.nu, nnzA, h->mapB, src, h->Bm);
        HIPCHK(hipStreamSynchronize(h->st));
    }
    return 0;
}

extern "C" int slsqp_qp_update_data_vec(slsqp_handle *h, const double *q, const double *l, const double *u, int loc) {
    hipSetDevice(h->dev);
    const size_t B = h->B;
    if (q && put(h, h->q, q, sizeof(double) * B * h->n, loc)) return -1;
    if (l && u) {
        const double *dl = l, *du = u;
        if (loc == SLSQP_HOST) {
            double *tmp = stage_buf(h, sizeof(double) * 2 * B * h->m);
            if (!tmp) return -1;
            HIPCHK(hipMemcpyAsync(tmp, l, sizeof(double) * B * h->m, hipMemcpyHostToDevice, h->st));
            HIPCHK(hipMemcpyAsync(tmp + B * h->m, u, sizeof(double) * B * h->m, hipMemcpyHostToDevice, h->st));
            dl = tmp; du = tmp + B * h->m;
        }
        hipLaunchKernelGGL(k_split_lu, dim3(1024), dim3(256), 0, h->st, h->B, h->mb, h->d.nx, dl, du, h->lbg, h->ubg, h->x0val);
        HIPCHK(hipStreamSynchronize(h->st));
    }
    h->have_dyn = true;
    return 0;
}

extern "C" int slsqp_qp_solve(slsqp_handle *h, double *x, double *y, int *status, int *iters, int loc, const slsqp_opts *opts) {
    hipSetDevice(h->dev);
    if (h->general_G) return fail("general G: only the sweep-level boundary (slsqp_sweep) is available; the QP solver needs box constraints G = [I;-I]");
    if (!h->have_costs) return fail("costs not set");
    slsqp_opts o;
    if (opts) o = *opts; else slsqp_default_opts(&o);
    if (mw_refuse(h, o)) return -1;
    HIPCHK(hipEventRecord(h->ev[0], h->st));
    QpCall qc;
    qc.warm = o.warm_start ? 1 : 0;
    if (launch_qp(h, nullptr, &o, qc)) return -1;
    HIPCHK(hipEventRecord(h->ev[1], h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    harvest_kernel_events(h);
    h->t_total = h->t_qp = ev_ms(h->ev[0], h->ev[1]); h->t_sweep = 0;
    const hipMemcpyKind kd = loc == SLSQP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (x) HIPCHK(hipMemcpyAsync(x, h->primal, sizeof(double) * (size_t)h->B * h->n, kd, h->st));
    if (y) {
        double *tmp = stage_buf(h, sizeof(double) * (size_t)h->B * h->m);
        if (!tmp) return -1;
        hipLaunchKernelGGL(k_join_y, dim3(1024), dim3(256), 0, h->st, h->B, h->mb, h->d.nx, h->dual, h->pin_dual, tmp);
        HIPCHK(hipMemcpyAsync(y, tmp, sizeof(double) * (size_t)h->B * h->m, kd, h->st));
    }
    if (status) HIPCHK(hipMemcpyAsync(status, h->status, sizeof(int) * h->B, kd, h->st));
    if (iters) HIPCHK(hipMemcpyAsync(iters, h->iters, sizeof(int) * h->B, kd, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    return 0;
}

// ---- sweep-level boundary -----------------------------------------------------------------------------------
extern "C" int slsqp_sweep(slsqp_handle *h, const double *eta, const double *eta_f, double *K, double *beta, double *beta_f, double *backoff,
                           double *backoff_f, int loc) {
    hipSetDevice(h->dev);
    if (!h->have_costs) return fail("costs not set");
    const slsqp_dims &d = h->d;
    const size_t B = h->B;
    if (put(h, h->eta, eta, sizeof(double) * B * d.N * d.N * d.ni, loc)) return -1;
    if (put(h, h->eta_f, eta_f, sizeof(double) * B * (d.N + 1) * d.ni_f, loc)) return -1;
    hipLaunchKernelGGL(k_fill_int, dim3((h->B + 255) / 256), dim3(256), 0, h->st, h->stale, 8, h->B);   // eta given by the caller, K and beta written for every instance
    HIPCHK(hipEventRecord(h->ev[0], h->st));
    if (launch_sweep(h, nullptr, h->eta, h->eta_f, 1e-10)) return -1;
    HIPCHK(hipEventRecord(h->ev[1], h->st));
    launch_tighten(h, tighten_args(h, nullptr, 0), nullptr);
    HIPCHK(hipEventRecord(h->ev[2], h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    h->t_sweep = ev_ms(h->ev[0], h->ev[1]); h->t_total = ev_ms(h->ev[0], h->ev[2]); h->t_qp = 0;
    const hipMemcpyKind kd = loc == SLSQP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (K) HIPCHK(hipMemcpyAsync(K, h->K, sizeof(double) * B * d.N * (d.N + 1) * d.nu * d.nx, kd, h->st));
    if (beta) {
        hipLaunchKernelGGL(k_beta_upper_zero, dim3(h->B), dim3(256), 0, h->st, d.N, d.ni, h->stale, h->beta);      // (a handle that has solved before: eps above the diagonal)
        HIPCHK(hipMemcpyAsync(beta, h->beta, sizeof(double) * B * d.N * d.N * d.ni, kd, h->st));
    }
    if (beta_f) HIPCHK(hipMemcpyAsync(beta_f, h->beta_f, sizeof(double) * B * (d.N + 1) * d.ni_f, kd, h->st));
    if (backoff) HIPCHK(hipMemcpyAsync(backoff, h->backoff, sizeof(double) * B * d.N * d.ni, kd, h->st));
    if (backoff_f) HIPCHK(hipMemcpyAsync(backoff_f, h->backoff_f, sizeof(double) * B * d.ni_f, kd, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    return 0;
}

// ---- self-test of the wave-level building blocks (wave_la.hpp) ---------------------------------------------------
// One wave runs one primitive on operands the caller supplies; tests/test_gpu_parity.py compares with numpy.  `in` / `out` are packed
// row-major matrices in the order given per case below; device scratch is allocated per call (diagnostic entry point, not a hot path).
template <int NX, int NU>
__global__ __launch_bounds__(64) void k_selftest(int which, const double *in, double *out, int n_in, int n_out) {
    extern __shared__ double sm[];
    const int lane = threadIdx.x;
    constexpr int MM = NX * NX, NB = NX * NU;
    double *I0 = sm, *O0 = sm + n_in;
    for (int o = lane; o < n_in; o += 64) I0[o] = in[o];
    for (int o = lane; o < n_out; o += 64) O0[o] = 0.0;
    wla::wsync();
    if (which == 0) wla::gemm_mfma<NX, NX, NX, false, false>(I0, NX, I0 + MM, NX, O0, NX, lane);                                   // A B
    else if (which == 1) wla::gemm_mfma<NX, NX, NX, true, false>(I0, NX, I0 + MM, NX, O0, NX, lane);                                // A' B
    else if (which == 2) wla::gemm_mfma<NU, NX, NX, true, false>(I0, NU, I0 + NB, NX, O0, NX, lane);                                // Bm' S   (in: Bm NX x NU, S NX x NX)
    else if (which == 3) wla::gemm_mfma<NX, NX, NX, false, false, false, true>(I0, NX, I0 + MM, NX, O0, NX, lane, nullptr, 0, I0 + 2 * MM);   // A diag(s) B
    else if (which == 4) wla::gemm_mfma<NX, NX, NU, false, false, true>(I0, NU, I0 + NB, NX, O0, NX, lane, I0 + 2 * NB, NX);        // D + Bm K  (in: Bm, K NU x NX, D NX x NX)
    else if (which == 5) wla::gemm_mfma_pair<NU, NX, NX, NX>(I0, NX, I0 + NB, NX, I0 + NB + MM, NX, O0, NX, O0 + NB, NX, lane);     // K P | A P (in: K NU x NX, A, P)
    else if (which == 6) { const int f = wla::spd_inv_gj<NX>(I0, NX, O0, NX, (double *)nullptr, lane); if (lane == 0) O0[MM] = (double)f; }   // inverse of the SPD matrix whose lower triangle is given
    else if (which == 8) {   // the same inverse by the matrix-core sweep; its block-packed copy (4 x gj_blocks doubles) follows the flag in the output
        const int f = wla::spd_inv_gj_mfma<NX>(I0, NX, O0, NX, O0 + MM + 1, lane); if (lane == 0) O0[MM] = (double)f;
    }
    else if (which == 7) {   // lower(Y) = A diag(pix) A' + B diag(piu) B' - T (A diag(pix))' + diag(d) + delta    (in: A, B, T, pix, piu, d)
        const double *A = I0, *Bm = I0 + MM, *T = I0 + MM + NB, *pix = T + MM, *piu = pix + NX, *d = piu + NU;
        if constexpr (NX >= 5) wla::build_Y_mfma<NX, NU>(A, pix, Bm, piu, T, true, d, 1e-13, O0, lane);
    }
    wla::wsync();
    for (int o = lane; o < n_out; o += 64) out[o] = O0[o];
}

extern "C" int slsqp_selftest(int nx, int nu, int which, const double *in, int n_in, double *out, int n_out) {
    if (n_in <= 0 || n_out <= 0 || n_in + n_out > 4000) return fail("selftest: operand sizes");
    double *din = nullptr, *dout = nullptr;
    HIPCHK(hipMalloc(&din, sizeof(double) * n_in));
    if (hipMalloc(&dout, sizeof(double) * n_out) != hipSuccess) { hipFree(din); return fail("selftest: hipMalloc"); }
    int rc = 0;
    if (hipMemcpy(din, in, sizeof(double) * n_in, hipMemcpyHostToDevice) != hipSuccess) rc = -1;
    const size_t lds = sizeof(double) * (size_t)(n_in + n_out);
    if (!rc) {
        if (nx == 17 && nu == 4) hipLaunchKernelGGL((k_selftest<17, 4>), dim3(1), dim3(64), lds, 0, which, din, dout, n_in, n_out);
        else if (nx == 13 && nu == 4) hipLaunchKernelGGL((k_selftest<13, 4>), dim3(1), dim3(64), lds, 0, which, din, dout, n_in, n_out);
        else rc = -2;
    }
    if (!rc && (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, dout, sizeof(double) * n_out, hipMemcpyDeviceToHost) != hipSuccess)) rc = -1;
    hipFree(din); hipFree(dout);
    if (rc == -2) return fail("selftest: (nx, nu) must be (17, 4) or (13, 4)");
    return rc ? fail("selftest: HIP error") : 0;
}

// ---- one block solve of the normal equations on given weights (diagnostic, like slsqp_selftest) -----------------------
template <int NX, int NU>
static int launch_ne_solve_t(slsqp_handle *h, int W, int factor, double delta, double *dPI, double *dV, double *dW, double *dG, double *dUF, double *dout) {
    if (allow_lds(k_ne_solve<NX, NU>)) return -1;
    NeG<NX, NU> g;
    g.A = h->A; g.Bm = h->Bm; g.ub = h->ubg; g.lb = h->lbg; g.Linv = h->Linv; g.PI = dPI; g.V = dV; g.G = dG; g.W = dW; g.UF = dUF; g.N = h->d.N;
    const size_t lds = W == 1 ? sizeof(double) * (size_t)qp_lds_doubles<NX, NU>(h->d.N) : sizeof(double) * (size_t)MwLds<NX, NU>::total(h->d.N, W);
    if (lds > 160 * 1024) return fail("slsqp_ne_solve: the work areas of that many waves do not fit the LDS for this horizon");
    hipLaunchKernelGGL((k_ne_solve<NX, NU>), dim3(h->B), dim3(64 * W), lds, h->st, g, h->B, h->cr, W, factor, delta, dout);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int slsqp_ne_solve(slsqp_handle *h, int waves, int factor, const double *PI, const double *V, double delta, double *W, double *G, double *bmax, int *fail_out,
                              int loc) {
    hipSetDevice(h->dev);
    if (waves != 1 && waves != 2 && waves != 4 && waves != 8) return fail("slsqp_ne_solve: waves must be 1, 2, 4 or 8");
    if (!PI || !V || !W || !G) return fail("slsqp_ne_solve: PI, V, W and G are required");
    if (!h->have_dyn) return fail("slsqp_ne_solve: update_dynamics must be called first (A and B are the handle's)");
    if (!factor && h->ne_waves != waves) return fail("slsqp_ne_solve: factor = 0 needs a factorising call with the same `waves` before it, with no QP solve in between");
    if (waves > 1 && ensure_cr(h)) return -1;
    const size_t B = h->B, n = h->n, nw = (size_t)h->d.N * h->d.nx;
    // device operands: PI | V | G (n each), W | UF (N nx each), (max|b|, flag) per instance
    const size_t total = B * (3 * n + 2 * nw + 2);
    double *buf = nullptr;
    HIPCHK(hipMalloc(&buf, sizeof(double) * total));
    double *dPI = buf, *dV = dPI + B * n, *dG = dV + B * n, *dW = dG + B * n, *dUF = dW + B * nw, *dout = dUF + B * nw;
    const hipMemcpyKind kin = loc == SLSQP_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, kout = loc == SLSQP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    int rc = 0;
    std::vector<double> ho(2 * B);
    if (hipMemsetAsync(dG, 0, sizeof(double) * B * (n + 2 * nw + 2), h->st) != hipSuccess) rc = -1;
    if (!rc && hipMemcpyAsync(dPI, PI, sizeof(double) * B * n, kin, h->st) != hipSuccess) rc = -1;
    if (!rc && hipMemcpyAsync(dV, V, sizeof(double) * B * n, kin, h->st) != hipSuccess) rc = -1;
    if (!rc) {
        // the QP solves' own stored factors live in the same scratch: they are gone after this call
        forget_factors(h);
        if (with_dims(h, [&](auto NX, auto NU) { return launch_ne_solve_t<NX(), NU()>(h, waves, factor, delta, dPI, dV, dW, dG, dUF, dout); })) rc = -2;      // (-2: the message is already there)
    }
    if (!rc && hipMemcpyAsync(W, dW, sizeof(double) * B * nw, kout, h->st) != hipSuccess) rc = -1;
    if (!rc && hipMemcpyAsync(G, dG, sizeof(double) * B * n, kout, h->st) != hipSuccess) rc = -1;
    if (!rc && hipMemcpyAsync(ho.data(), dout, sizeof(double) * 2 * B, hipMemcpyDeviceToHost, h->st) != hipSuccess) rc = -1;
    if (hipStreamSynchronize(h->st) != hipSuccess && !rc) rc = -1;
    if (!rc) {
        std::vector<double> bm(B); std::vector<int> fl(B);
        for (size_t b = 0; b < B; b++) { bm[b] = ho[2 * b]; fl[b] = (int)ho[2 * b + 1]; }
        const hipMemcpyKind kh = loc == SLSQP_HOST ? hipMemcpyHostToHost : hipMemcpyHostToDevice;
        if (bmax && hipMemcpy(bmax, bm.data(), sizeof(double) * B, kh) != hipSuccess) rc = -1;
        if (fail_out && hipMemcpy(fail_out, fl.data(), sizeof(int) * B, kh) != hipSuccess) rc = -1;
        if (factor) h->ne_waves = waves;
    }
    hipFree(buf);
    if (rc == -1) return fail("slsqp_ne_solve: HIP error");
    return rc ? -1 : 0;
}
