// Stand-alone host program (own main) around the argument builders of the closed-loop kernels (csrc/slsqp_api.hip: make_qp_args, make_chain_args,
// make_loop_block, stage_loop_block -- no HIP call on the paths taken here), compiled for the host only so that it runs without a GPU and can be built
// with -fsanitize=address,undefined (tests/test_loop_args_cpu.py).  The handle is a value-initialised slsqp_handle whose device pointers are distinct
// made-up addresses: nothing dereferences them.
//   1. the two QpArgs of a chain the old way -- two independent make_qp_args calls with (warm, stat_slot, snap_use) = (w, 0, 0) and (1, 1, 1) --
//      against the new way, the common struct and qp_second_args, byte for byte, for w = 0 and w = 1 (and with ipm_restart off);
//   2. the block the host stages for a launch against the LoopArgs that went to the kernel by value before, field by field;
//   3. the description of the handle's options (cl_options) in each of the 8 states (reference, parameters, bounds on or off): the persistent
//      kernels' variant, reference and plant arguments, the batch-wide kernels' flags, and the bounds in the block against the struct they were before;
//   4. every argument builder against the struct "as it was", the positional initialiser of the launch sites before the builders,
//      field by field for every combination of the varying parameters a site uses; make_chain_args and make_loop_block against the same composition
//      written the way it was, memcmp, plain and SCP in the option states 000 and 111;
//   5. no launch is entered by make_qp_args, make_chain_args or make_loop_block with a non-zero x0 tolerance on the handle (the launch entry points of
//      the runtime are this program's own and count), and with_dims on a pair the build does not hold fails and says so.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../robust-nonlinear-mpc_amd/csrc/slsqp_api.hip"

// The kernels' host stubs register themselves with the HIP runtime when the program starts; this program holds no device code (host-only compilation
// with -fuse-cuid=none: the code object's symbol is plain __hip_fatbin) and launches nothing, so the registration entry points are its own empty ones
// and the runtime is never entered.
extern "C" {
extern const char __hip_fatbin[8] = {0};
void **__hipRegisterFatBinary(const void *) { static void *handle; return &handle; }
void __hipRegisterFunction(void **, const void *, char *, const char *, unsigned, void *, void *, void *, void *, int *) {}
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}
void __hipUnregisterFatBinary(void **) {}
}
// a kernel launch begins here (hipLaunchKernelGGL pushes the launch configuration first): counted and refused, so that the kernel's stub is not called
static int launches_entered = 0;
extern "C" hipError_t __hipPushCallConfiguration(dim3, dim3, size_t, hipStream_t) { launches_entered++; return hipErrorUnknown; }

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)
#define SAME(a, b) EXPECT(sizeof(a) == sizeof(b) && std::memcmp(&(a), &(b), sizeof(a)) == 0)

static uintptr_t next_addr = 0x10000;
#define FAKE(f) do { h->f = (decltype(h->f))(next_addr); next_addr += 0x1000; } while (0)

static slsqp_handle *fake_handle(int B, int N) {
    slsqp_handle *h = new slsqp_handle();
    h->B = B; h->d.N = N; h->d.nx = 4; h->d.nu = 1; h->d.nw = 4; h->d.ni = 10; h->d.ni_f = 8; h->n = 5 * N + 4;
    h->call_id = 7.0; h->log_steps = 6; h->qplog_steps = 6; h->clq_cap = 32;
    h->x0_box_tol = 1e-3;      // (the device word holds 0: a builder that wrote the tolerance would launch)
    FAKE(A); FAKE(Aclc); FAKE(Bm); FAKE(E); FAKE(K); FAKE(Kc); FAKE(Linv); FAKE(Un); FAKE(Xn); FAKE(alive); FAKE(backoff); FAKE(backoff_f); FAKE(backoff_u);
    FAKE(backoff_x); FAKE(beta); FAKE(beta_f); FAKE(c); FAKE(call_ids); FAKE(chain_times); FAKE(cl_busy); FAKE(cl_stepno); FAKE(cl_tbegin); FAKE(clq_ctl);
    FAKE(clq_slots); FAKE(conv); FAKE(cost); FAKE(cost_tube); FAKE(counter); FAKE(cst); FAKE(ct_part); FAKE(dual); FAKE(eta); FAKE(eta_f); FAKE(g); FAKE(gN);
    FAKE(g_raw); FAKE(gf_raw); FAKE(has_prev); FAKE(infeas); FAKE(inst_launches); FAKE(iters); FAKE(itnum); FAKE(kkt); FAKE(lbg); FAKE(lg_bu); FAKE(lg_bx);
    FAKE(lg_it); FAKE(lg_pinf); FAKE(lg_state); FAKE(lg_succ); FAKE(lg_u); FAKE(lg_u0); FAKE(lg_x); FAKE(lin_stage); FAKE(lin_tape); FAKE(mask);
    FAKE(pending_reset); FAKE(pin_dual); FAKE(pinf); FAKE(prev_primal); FAKE(primal); FAKE(q); FAKE(qp_diag); FAKE(qplog); FAKE(qplog_nsolves); FAKE(qpstat);
    FAKE(qpstate); FAKE(scp_active); FAKE(scp_dmax); FAKE(scp_iters); FAKE(scp_success); FAKE(scp_upd); FAKE(stale); FAKE(status); FAKE(success); FAKE(u0);
    FAKE(u_init); FAKE(ubg); FAKE(ws); FAKE(x0arg); FAKE(x0val); FAKE(x0vlog); FAKE(xmeas); FAKE(zero_ref);
    return h;
}

// a QP call from the six positional values make_qp_args took before QpCall, in their order then
static QpCall qp_call(int warm, const double *prox, int stat_slot, int snap_take, int snap_use, int warm_shift) {
    QpCall c;
    c.warm = warm; c.prox = prox; c.stat_slot = stat_slot; c.snap_take = snap_take; c.snap_use = snap_use; c.warm_shift = warm_shift;
    return c;
}

// what cl_run_persistent passed to k_cl_loop by value before the block: its statements, with the two QpArgs of the chain filled independently
struct OldArgs { QpArgs q1, q2; };
static OldArgs old_qp_pair(slsqp_handle *h, const slsqp_opts &o) {
    OldArgs r;
    r.q1 = make_qp_args(h, h->alive, &o, qp_call(o.warm_start ? 1 : 0, nullptr, 0, 1, 0, 1));
    r.q2 = make_qp_args(h, h->alive, &o, qp_call(1, nullptr, 1, 1, 1, 1));
    r.q1.call_ids = r.q2.call_ids = h->call_ids;
    r.q1.shift_stepno = r.q2.shift_stepno = h->cl_stepno;
    return r;
}

// the bounds' argument as it was declared before the table type: the block's bd keeps these bytes
struct OldBndArgs { const double *rows; int T; size_t stride; const int *stepno; int step; };
static_assert(sizeof(OldBndArgs) == sizeof(BndArgs) && sizeof(RefArgs) == 24, "the argument layouts stay");

// ---- 3: states (ref, pp, bnd); the variant each ran as before the bit set was 0, 1, 2, 2, 3, 3, 4, 4 in the order of `want` below
static void check_option_states() {
    static const int want[8] = {/* 000 */ 0, /* 001 */ 5, /* 010 */ 3, /* 011 */ 7, /* 100 */ 1, /* 101 */ 5, /* 110 */ 3, /* 111 */ 7};
    for (int st = 0; st < 8; st++) {
        const bool ref = st & 4, pp = st & 2, bnd = st & 1;
        slsqp_handle *h = fake_handle(5, 3);
        if (ref) { FAKE(ref_Y); h->ref_T = 2; h->ref_stride = 2 * 5; }
        if (pp) { FAKE(pp_P); FAKE(pp_merr); FAKE(lg_merr); h->pp_np = 3; h->pp_stride = 3; }
        if (bnd) { FAKE(bnd_rows); h->bnd_T = 2; h->bnd_stride = 2 * 18; }
        const ClOptions op = cl_options(h);
        EXPECT(op.ref == ref && op.pp == pp && op.bnd == bnd && op.var == want[st]);
        EXPECT(var_ref(op.var) == (st != 0) && var_pp(op.var) == pp && var_bnd(op.var) == bnd);
        int seen = -1, calls = 0;
        EXPECT(with_loop_var(op.var, [&](auto V) { seen = V(); calls++; }) && seen == want[st] && calls == 1);
        with_ref_bnd(op, [&](auto REF, auto BND) { EXPECT(REF() == ref && BND() == bnd); calls++; });      // k_lin_vec, k_nom_eval: the handle's own, no zero row
        EXPECT(calls == 2);
        if (ref) EXPECT(op.own_rf.rows == h->ref_Y && op.own_rf.T == 2 && op.own_rf.stride == 10);      // k_lin_vec, k_nom_eval: the handle's own or none
        else EXPECT(op.own_rf.rows == nullptr && op.own_rf.T == 0 && op.own_rf.stride == 0);
        if (ref) EXPECT(op.rf.rows == h->ref_Y && op.rf.T == 2 && op.rf.stride == 10);
        else if (st) EXPECT(op.rf.rows == h->zero_ref && op.rf.T == 1 && op.rf.stride == 0);
        else EXPECT(op.rf.rows == nullptr && op.rf.T == 0 && op.rf.stride == 0);
        if (pp) EXPECT(op.pa.P == h->pp_P && op.pa.stride == 3 && op.pa.model_err == h->pp_merr && op.pa.lg == h->lg_merr && op.pa.S == h->log_steps);
        else EXPECT(op.pa.P == nullptr && op.pa.stride == 0 && op.pa.model_err == nullptr && op.pa.lg == nullptr && op.pa.S == 0);
        const BndArgs bd = bnd_args(h, 4, h->cl_stepno);      // tighten / chain (BND = op.bnd) and the step of either table's window
        EXPECT(bd.rows == h->bnd_rows && bd.T == h->bnd_T && bd.stride == h->bnd_stride && bd.stepno == h->cl_stepno && bd.step == 4);
        // the block's bounds: the bytes of the struct as it was, filled field by field; all zero bytes without bounds
        slsqp_opts o;
        slsqp_default_opts(&o);
        const ScpLoopArgs S = make_loop_block(h, 3, nullptr, o, false, 1);
        OldBndArgs old;
        std::memset(&old, 0, sizeof old);
        if (bnd) { old.rows = h->bnd_rows; old.T = h->bnd_T; old.stride = h->bnd_stride; old.stepno = h->cl_stepno; old.step = 0; }
        EXPECT(std::memcmp(&S.bd, &old, sizeof old) == 0);
        EXPECT((const unsigned char *)&S.bd + sizeof S.bd == (const unsigned char *)&S + sizeof S);      // bd stays behind every other field
        delete h;
    }
    for (int v : {-1, 2, 4, 6, 8}) EXPECT(!with_loop_var(v, [&](auto) { fails++; }));      // no instantiation, no fall-back
}

// ---- 4: the argument structs as they were.  Each function is the initialiser of the launch sites before the builders, its varying parts as parameters.
static Costs old_costs(slsqp_handle *h) {
    const int nx = h->d.nx, nu = h->d.nu;
    Costs c;
    c.Qd = h->cst; c.Rd = c.Qd + nx; c.Qfd = c.Rd + nu; c.Qregd = c.Qfd + nx; c.Rregd = c.Qregd + nx; c.Qregfd = c.Rregd + nu; c.prox = 0.0;
    return c;
}
static TightenArgs old_tighten(slsqp_handle *h, const int *run, int flag) {
    const slsqp_dims &d = h->d;
    const int B = h->B;
    return TightenArgs{B, d.N, d.nx, d.nu, d.ni, d.ni_f, h->beta, h->beta_f, h->g, h->gf_raw, h->c, run, h->backoff, h->backoff_f, h->backoff_x, h->backoff_u, h->ubg, flag, h->ct_part, h->cost_tube};
}
static SweepArgs old_sweep(slsqp_handle *h, const int *run, const double *eta, const double *eta_f, double eps) {
    SweepArgs a;
    a.B = h->B; a.N = h->d.N; a.NW = h->d.nw; a.A = h->A; a.Bm = h->Bm; a.E = h->E; a.E_per_instance = 0; a.eta = eta; a.eta_f = eta_f;
    a.run = run; a.cst = old_costs(h); a.K = h->K; a.beta = h->beta; a.beta_f = h->beta_f; a.ct_part = h->ct_part; a.eps = eps;
    return a;
}
static AfterQpArgs old_after_qp(slsqp_handle *h, const slsqp_opts &o, const int *active, int rti, int first, int shared) {
    const slsqp_dims &d = h->d;
    const int B = h->B;
    EtaArgs ea{B, d.N, d.nx, d.ni, d.ni_f, h->dual, h->beta, h->beta_f, h->alive, h->eta, h->eta_f, o.eps_backoff, h->stale, shared};
    ConvArgs ca{B, h->n, h->primal, h->prev_primal, h->has_prev, h->alive, h->conv, o.conv_tol};
    return AfterQpArgs{B, rti, first, h->status, active, h->alive, h->infeas, h->mask, h->success, h->itnum, h->counter, h->stale, h->conv, ea, ca, h->beta, h->beta_f};
}
static InitBackoffArgs old_init_backoff(slsqp_handle *h, const slsqp_opts &o, const int *run, int fill_beta) {
    const slsqp_dims &d = h->d;
    const int B = h->B;
    return InitBackoffArgs{B, d.N, d.nx, d.nu, o.eps_backoff, run, h->beta, h->beta_f, h->backoff, h->backoff_f, h->backoff_x, h->backoff_u, fill_beta};
}
static SolveBeginArgs old_solve_begin(slsqp_handle *h, const slsqp_opts &o, const double *x0, const int *active, const int *skip) {
    const slsqp_dims &d = h->d;
    const int B = h->B;
    return SolveBeginArgs{B, d.nx, x0, h->x0val, active, h->alive, h->infeas, h->success, h->pending_reset, h->itnum, h->stale,
                          h->eta, h->eta_f, (size_t)d.N * d.N * d.ni, (size_t)(d.N + 1) * d.ni_f,
                          InitBackoffArgs{B, d.N, d.nx, d.nu, o.eps_backoff, active, h->beta, h->beta_f, h->backoff, h->backoff_f, h->backoff_x, h->backoff_u, 0}, skip};
}
static LinArgs old_lin(slsqp_handle *h, const double *dX, const double *dU, const int *run) {
    const slsqp_dims &d = h->d;
    return LinArgs{h->B, d.N, dX, dU, h->g_raw, h->gf_raw, old_costs(h), h->A, h->Bm, h->c, h->g, h->gN, h->q, run, h->lin_stage, h->lin_tape};
}
static BoundsArgs old_bounds(slsqp_handle *h, const int *run) {
    const slsqp_dims &d = h->d;
    return BoundsArgs{h->B, d.N, d.nx, d.ni, d.ni_f, h->g, h->gN, h->c, h->ubg, h->lbg, 1e-10, run};
}
static ClLogArgs old_cl_log(slsqp_handle *h, const int *stepno, const int *mask, int step) {
    const slsqp_dims &d = h->d;
    return ClLogArgs{stepno, mask, h->B, d.N, d.nx, d.nu, h->log_steps, step, h->Xn, h->Un, h->backoff_x, h->backoff_u, h->scp_success, h->scp_iters,
                     h->pinf, h->lg_x, h->lg_u, h->lg_bx, h->lg_bu, h->lg_state, h->lg_u0, h->lg_pinf, h->lg_succ, h->lg_it};
}
static ScpArgs old_scp(slsqp_handle *h, const slsqp_opts &o, int ii, int converge) {
    return ScpArgs{ii, converge, o.scp_eps, h->scp_active, h->scp_success, h->scp_iters, h->counter + 2, h->scp_dmax, h->scp_upd};
}
static ChainArgs old_chain_args(slsqp_handle *h, const slsqp_opts &o, const int *active, int wshift) {
    const slsqp_dims &d = h->d;
    const int B = h->B;
    ChainArgs c;
    memset(&c, 0, sizeof c);
    c.q = make_qp_args(h, h->alive, &o, qp_call(o.warm_start ? 1 : 0, nullptr, 0, 1, 0, wshift));
    c.q2 = Qp2Ints{1, 1, o.ipm_restart ? 1 : 0};
    EtaArgs ea{B, d.N, d.nx, d.ni, d.ni_f, h->dual, h->beta, h->beta_f, h->alive, h->eta, h->eta_f, o.eps_backoff, h->stale, 1};
    ConvArgs ca{B, h->n, h->primal, h->prev_primal, h->has_prev, h->alive, h->conv, o.conv_tol};
    c.aq = AfterQpArgs{B, 1, 1, h->status, active, h->alive, h->infeas, h->mask, h->success, h->itnum, h->counter, h->stale, h->conv, ea, ca, h->beta, h->beta_f};
    SweepArgs sa;
    sa.B = h->B; sa.N = d.N; sa.NW = d.nw; sa.A = h->A; sa.Bm = h->Bm; sa.E = h->E; sa.E_per_instance = 0; sa.eta = h->eta; sa.eta_f = h->eta_f;
    sa.run = h->mask; sa.cst = old_costs(h); sa.K = h->K; sa.beta = h->beta; sa.beta_f = h->beta_f; sa.ct_part = h->ct_part; sa.eps = o.eps_backoff;
    c.sw = SweepSharedArgs{sa, h->Kc, h->Aclc, h->stale};
    c.ta = TightenArgs{B, d.N, d.nx, d.nu, d.ni, d.ni_f, h->beta, h->beta_f, h->g, h->gf_raw, h->c, h->mask, h->backoff, h->backoff_f, h->backoff_x, h->backoff_u, h->ubg, 1, h->ct_part, h->cost_tube};
    c.active = active; c.success = h->success; c.infeas = h->infeas; c.times = h->chain_times;
    c.max_ticks = qp_max_ticks(c.q, o.qp_max_iter);
    c.lag = nullptr; c.runm = nullptr; c.done = nullptr; c.t0word = nullptr; c.budget = 0; c.qplog = nullptr; c.x0vlog = nullptr; c.stepno = nullptr; c.log_steps = 0; c.fin_count = nullptr; c.cut_count = 0xFFFFFFFFu;
    return c;
}
static ScpLoopArgs old_loop_block(slsqp_handle *h, int steps, const double *dW, const slsqp_opts &o, bool scp, int scp_rti) {
    const int max_it = !scp ? 1 : (scp_rti > 0 ? scp_rti : o.max_scp_iter);
    const slsqp_dims &d = h->d;
    const int B = h->B;
    ScpLoopArgs S;
    memset(&S, 0, sizeof S);
    LoopArgs &L = S.L;
    const int *active = scp ? h->scp_active : nullptr;
    L.c = old_chain_args(h, o, active, 1);
    L.c.q.call_ids = h->call_ids;
    L.c.q.shift_stepno = h->cl_stepno;
    L.c.qplog = h->qplog; L.c.x0vlog = h->x0vlog; L.c.stepno = h->cl_stepno; L.c.log_steps = h->qplog_steps;
    L.cl = cl_args(h, nullptr);
    L.lin = LinArgs{B, d.N, h->Xn, h->Un, h->g_raw, h->gf_raw, old_costs(h), h->A, h->Bm, h->c, h->g, h->gN, h->q, nullptr, h->lin_stage, h->lin_tape};
    L.ba = BoundsArgs{B, d.N, d.nx, d.ni, d.ni_f, h->g, h->gN, h->c, h->ubg, h->lbg, 1e-10, nullptr};
    L.sb = SolveBeginArgs{B, d.nx, h->x0arg, h->x0val, active, h->alive, h->infeas, h->success, h->pending_reset, h->itnum, h->stale,
                          h->eta, h->eta_f, (size_t)d.N * d.N * d.ni, (size_t)(d.N + 1) * d.ni_f,
                          InitBackoffArgs{B, d.N, d.nx, d.nu, o.eps_backoff, active, h->beta, h->beta_f, h->backoff, h->backoff_f, h->backoff_x, h->backoff_u, 0}, nullptr};
    L.lg = ClLogArgs{h->cl_stepno, nullptr, B, d.N, d.nx, d.nu, h->log_steps, 0, h->Xn, h->Un, h->backoff_x, h->backoff_u, h->scp_success, h->scp_iters,
                     h->pinf, h->lg_x, h->lg_u, h->lg_bx, h->lg_bu, h->lg_state, h->lg_u0, h->lg_pinf, h->lg_succ, h->lg_it};
    L.sa = ScpArgs{0, 0, o.scp_eps, h->scp_active, h->scp_success, h->scp_iters, h->counter + 2, h->scp_dmax, h->scp_upd};
    L.steps = steps; L.n = h->n; L.have_log = h->log_steps > 0 ? 1 : 0;
    L.keep_laggards = 1; L.fence = 3;      // (the defaults of SLSQP_LOOP_KEEP and SLSQP_LOOP_FENCE, which this program does not set)
    L.stepno = h->cl_stepno; L.call_ids = h->call_ids; L.q = h->q; L.stale = h->stale; L.itnum = h->itnum; L.pending = h->pending_reset; L.scp_active = h->scp_active;
    L.W_all = dW; L.pinf = h->pinf;
    L.Q = ClQueue{h->clq_slots, h->clq_cap - 1u, (unsigned *)h->clq_ctl, (unsigned *)h->clq_ctl + 1, h->clq_ctl + 2, h->clq_ctl + 3};
    L.busy = h->cl_busy; L.t_begin = h->cl_tbegin;
    S.max_it = max_it; S.converge = scp_rti <= 0 ? 1 : 0; S.rti_steps = o.rti_steps; S.nsolves = h->qplog_nsolves;
    if (h->bnd_rows != nullptr) { S.bd.rows = h->bnd_rows; S.bd.T = h->bnd_T; S.bd.stride = h->bnd_stride; S.bd.stepno = h->cl_stepno; S.bd.step = 0; }
    return S;
}
// field by field (the structs have padding, which an initialiser leaves undefined)
#define F(x) (a.x == b.x)
static bool eq(const Costs &a, const Costs &b) { return F(Qd) && F(Rd) && F(Qfd) && F(Qregd) && F(Rregd) && F(Qregfd) && F(prox); }
static bool eq(const TightenArgs &a, const TightenArgs &b) {
    return F(B) && F(N) && F(NX) && F(NU) && F(NI) && F(NIF) && F(beta) && F(beta_f) && F(g) && F(gf_raw) && F(c) && F(run) && F(backoff) && F(backoff_f) && F(backoff_x) &&
           F(backoff_u) && F(ubg) && F(write_ubg) && F(ct_part) && F(cost_tube);
}
static bool eq(const SweepArgs &a, const SweepArgs &b) {
    return F(B) && F(N) && F(NW) && F(A) && F(Bm) && F(E) && F(E_per_instance) && F(eta) && F(eta_f) && F(run) && eq(a.cst, b.cst) && F(K) && F(beta) && F(beta_f) && F(ct_part) && F(eps);
}
static bool eq(const EtaArgs &a, const EtaArgs &b) {
    return F(B) && F(N) && F(NX) && F(NI) && F(NIF) && F(dual) && F(beta) && F(beta_f) && F(run) && F(eta) && F(eta_f) && F(eps) && F(stale) && F(first_iter);
}
static bool eq(const ConvArgs &a, const ConvArgs &b) { return F(B) && F(n) && F(primal) && F(prev) && F(has_prev) && F(run) && F(conv) && F(tol); }
static bool eq(const AfterQpArgs &a, const AfterQpArgs &b) {
    return F(B) && F(rti) && F(first_iter) && F(status) && F(active) && F(alive) && F(infeas) && F(mask) && F(success) && F(itnum) && F(counter) && F(stale) && F(conv) && eq(a.ea, b.ea) &&
           eq(a.ca, b.ca) && F(beta_w) && F(beta_f_w);
}
static bool eq(const InitBackoffArgs &a, const InitBackoffArgs &b) {
    return F(B) && F(N) && F(NX) && F(NU) && F(eps) && F(run) && F(beta) && F(beta_f) && F(backoff) && F(backoff_f) && F(backoff_x) && F(backoff_u) && F(fill_beta);
}
static bool eq(const SolveBeginArgs &a, const SolveBeginArgs &b) {
    return F(B) && F(NX) && F(x0) && F(x0val) && F(active) && F(alive) && F(infeas) && F(success) && F(pending) && F(itnum) && F(stale) && F(eta) && F(eta_f) && F(neta) && F(netaf) &&
           eq(a.ib, b.ib) && F(skip);
}
static bool eq(const LinArgs &a, const LinArgs &b) {
    return F(B) && F(N) && F(X) && F(U) && F(g_raw) && F(gf_raw) && eq(a.cst, b.cst) && F(A) && F(Bm) && F(c) && F(g) && F(gN) && F(q) && F(run) && F(stage) && F(tape);
}
static bool eq(const BoundsArgs &a, const BoundsArgs &b) { return F(B) && F(N) && F(NX) && F(NI) && F(NIF) && F(g) && F(gN) && F(c) && F(ubg) && F(lbg) && F(eps) && F(run); }
static bool eq(const ClLogArgs &a, const ClLogArgs &b) {
    return F(stepno) && F(mask) && F(B) && F(N) && F(NX) && F(NU) && F(S) && F(step) && F(Xn) && F(Un) && F(bx) && F(bu) && F(success) && F(scp_iters) && F(pinf) && F(lx) && F(lu) &&
           F(lbx) && F(lbu) && F(lstate) && F(lu0) && F(lpinf) && F(lsucc) && F(lit);
}
static bool eq(const ScpArgs &a, const ScpArgs &b) {
    return F(ii) && F(converge) && F(eps) && F(active) && F(scp_success) && F(scp_iters) && F(n_active) && F(dmax) && F(updated);
}
#undef F

static void check_builders() {
    slsqp_handle *h = fake_handle(5, 3);
    slsqp_opts o;
    slsqp_default_opts(&o);
    o.eps_backoff = 3e-10; o.conv_tol = 2e-3; o.scp_eps = 4e-10;      // (not the defaults: a builder that ignored its options would show)
    const double *hostless = nullptr, *dX = (const double *)(uintptr_t)0x8000000, *dU = (const double *)(uintptr_t)0x8100000;
    // the combinations the launch sites use
    EXPECT(eq(tighten_args(h, h->mask, 1), old_tighten(h, h->mask, 1)) && eq(tighten_args(h, nullptr, 0), old_tighten(h, nullptr, 0)));      // a solve, the chain; slsqp_sweep
    EXPECT(!eq(tighten_args(h, h->mask, 1), old_tighten(h, nullptr, 0)));                                                                      // (the comparison sees both)
    EXPECT(eq(sweep_args(h, h->mask, h->eta, h->eta_f, o.eps_backoff), old_sweep(h, h->mask, h->eta, h->eta_f, o.eps_backoff)));             // a solve, the chain
    EXPECT(eq(sweep_args(h, nullptr, h->eta, h->eta_f, 1e-10), old_sweep(h, nullptr, h->eta, h->eta_f, 1e-10)));                             // slsqp_sweep
    for (int rti = 0; rti < 2; rti++) for (int first = 0; first < 2; first++) for (int shared = 0; shared < 2; shared++) for (const int *active : {(const int *)nullptr, (const int *)h->scp_active})
        EXPECT(eq(after_qp_args(h, o, active, rti, first, shared), old_after_qp(h, o, active, rti, first, shared)));
    for (const double *x0 : {hostless, (const double *)h->x0arg}) for (const int *active : {(const int *)nullptr, (const int *)h->scp_active}) for (const int *skip : {(const int *)nullptr, (const int *)h->cl_stepno})
        EXPECT(eq(solve_begin_args(h, o, x0, active, skip), old_solve_begin(h, o, x0, active, skip)));
    for (const int *run : {(const int *)nullptr, (const int *)h->scp_active}) for (int fill = 0; fill < 2; fill++)
        EXPECT(eq(init_backoff_args(h, o, run, fill), old_init_backoff(h, o, run, fill)));
    for (const int *run : {(const int *)nullptr, (const int *)h->scp_active}) {
        EXPECT(eq(lin_args(h, dX, dU, run), old_lin(h, dX, dU, run)) && eq(lin_args(h, h->Xn, h->Un, run), old_lin(h, h->Xn, h->Un, run)));
        EXPECT(eq(bounds_args(h, run), old_bounds(h, run)));
    }
    EXPECT(eq(cl_log_args(h, nullptr, nullptr, 4), old_cl_log(h, nullptr, nullptr, 4)));                           // slsqp_cl_step
    EXPECT(eq(cl_log_args(h, h->cl_stepno, h->cl_done, 0), old_cl_log(h, h->cl_stepno, h->cl_done, 0)));           // a round of slsqp_cl_run
    EXPECT(eq(cl_log_args(h, h->cl_stepno, nullptr, 0), old_cl_log(h, h->cl_stepno, nullptr, 0)));                 // the persistent loops
    for (int converge = 0; converge < 2; converge++) EXPECT(eq(scp_args(h, o, 2 * converge, converge), old_scp(h, o, 2 * converge, converge)));
    // the two named QP calls are the positional ones they replace, and qp_second_ints is the last one's three ints
    for (int restart = 0; restart < 2; restart++) for (int w = 0; w < 2; w++) for (int ws = 0; ws < 2; ws++) {
        o.ipm_restart = restart;
        const QpArgs f1 = make_qp_args(h, h->alive, &o, qp_first_call(w, ws)), f0 = make_qp_args(h, h->alive, &o, qp_call(w, nullptr, 0, 1, 0, ws));
        const QpArgs l1 = make_qp_args(h, h->alive, &o, qp_last_call(ws)), l0 = make_qp_args(h, h->alive, &o, qp_call(1, nullptr, 1, 1, 1, ws));
        SAME(f1, f0);
        SAME(l1, l0);
        const Qp2Ints s = qp_second_ints(o);
        EXPECT(s.warm == l0.warm && s.stat_slot == l0.stat_slot && s.snap_use == l0.snap_use && s.warm == 1 && s.stat_slot == 1 && s.snap_use == restart);
    }
    EXPECT(qp_x0_tol(h, QpCall{}) == 1e-3 && qp_x0_tol(h, qp_call(0, dX, 0, 0, 0, 0)) == 0.0);      // (prox: the nominal initialiser's QPs stay strict)
    delete h;
}
// the compositions against the way they were written, byte for byte (both are memset first), plain and SCP, in the option states 000 and 111
static void check_compositions() {
    for (int st : {0, 7}) for (int scp = 0; scp < 2; scp++) {
        slsqp_handle *h = fake_handle(6, 4);
        if (st) { FAKE(ref_Y); h->ref_T = 2; h->ref_stride = 2 * 5; FAKE(pp_P); FAKE(pp_merr); FAKE(lg_merr); h->pp_np = 3; h->pp_stride = 3; FAKE(bnd_rows); h->bnd_T = 2; h->bnd_stride = 2 * 18; }
        slsqp_opts o;
        slsqp_default_opts(&o);
        o.rti_steps = 1 + scp; o.warm_start = scp;
        const int *active = scp ? h->scp_active : nullptr;
        const ChainArgs c = make_chain_args(h, o, active, 1), c0 = old_chain_args(h, o, active, 1);
        SAME(c, c0);
        const ScpLoopArgs S = make_loop_block(h, 4, (const double *)(uintptr_t)0x7000000, o, scp != 0, 2), S0 = old_loop_block(h, 4, (const double *)(uintptr_t)0x7000000, o, scp != 0, 2);
        SAME(S, S0);
        EXPECT((S.bd.rows != nullptr) == (st != 0));
        delete h;
    }
}
// with_dims: the handle's pair as constants; a pair the build does not hold is an error that names the pair and the list, and f is not called
static void check_with_dims() {
    slsqp_handle *h = fake_handle(5, 3);
    int nx = -1, nu = -1, calls = 0;
    EXPECT(with_dims(h, [&](auto NX, auto NU) { nx = NX(); nu = NU(); return 7; }) == 7 && nx == 4 && nu == 1);
    h->d.nx = 5; h->d.nu = 2;
    EXPECT(with_dims(h, [&](auto, auto) { calls++; return 0; }) != 0 && calls == 0);
    const std::string e = slsqp_last_error();
    EXPECT(e.find("(nx, nu) = (5,2)") != std::string::npos && e.find(dims_list()) != std::string::npos && e.find("(4,1) (13,4) (17,4)") != std::string::npos);
    delete h;
}
// nothing above entered a launch, although every fake handle asks for a tolerance the device word does not hold; set_x0_tol, which the launching
// functions call, does (so the count would have shown it)
static void check_no_launch() {
    EXPECT(launches_entered == 0);
    slsqp_handle *h = fake_handle(5, 3);
    set_x0_tol(h, h->x0_box_tol);
    EXPECT(launches_entered == 1 && h->x0_tol_dev == 1e-3);
    set_x0_tol(h, h->x0_box_tol);
    EXPECT(launches_entered == 1);
    delete h;
}

int main() {
    check_option_states();
    check_builders();
    for (int w = 0; w < 2; w++) for (int restart = 0; restart < 2; restart++) for (int scp = 0; scp < 2; scp++) {
        slsqp_handle *h = fake_handle(5 + w, 3 + 2 * restart);
        slsqp_opts o;
        slsqp_default_opts(&o);
        o.warm_start = w; o.ipm_restart = restart; o.warm_rounds = 3 + w; o.as_first = restart; o.rti_steps = 1;
        const int steps = 4 + scp, rti = 2;
        const double *dW = (const double *)(uintptr_t)0x7000000;
        const int *active = scp ? h->scp_active : nullptr;
        // ---- 1: the chain's pair (as make_chain_args builds it, no call ids) and the loop's pair
        {
            QpArgs q1 = make_qp_args(h, h->alive, &o, qp_call(w, nullptr, 0, 1, 0, 1)), q2 = make_qp_args(h, h->alive, &o, qp_call(1, nullptr, 1, 1, 1, 1));
            EXPECT(q1.warm == w && q1.stat_slot == 0 && q1.snap_use == 0 && q2.warm == 1 && q2.stat_slot == 1 && q2.snap_use == restart);
            const ChainArgs c = make_chain_args(h, o, active, 1);
            const QpArgs n1 = c.q, n2 = qp_second_args(c.q, c.q2);
            SAME(n1, q1);
            SAME(n2, q2);
            EXPECT(std::memcmp(&q1, &q2, sizeof q1) != 0);
            const QpArgs again = qp_second_args(c.q, Qp2Ints{c.q.warm, c.q.stat_slot, c.q.snap_use});      // pass 0 of rti_chain_dev
            SAME(again, q1);
        }
        const ScpLoopArgs S = make_loop_block(h, steps, dW, o, scp != 0, rti);
        const OldArgs old = old_qp_pair(h, o);
        {
            const QpArgs n2 = qp_second_args(S.L.c.q, S.L.c.q2);
            SAME(S.L.c.q, old.q1);
            SAME(n2, old.q2);
        }
        // ---- 2: the staged block
        stage_loop_block(h, S);
        EXPECT(h->loop_blk_host.size() == sizeof(ScpLoopArgs));
        ScpLoopArgs G;
        std::memcpy(&G, h->loop_blk_host.data(), sizeof G);
        SAME(G, S);
        const LoopArgs &L = G.L;
        const slsqp_dims &d = h->d;
        const int B = h->B;
        // the chain behind its QpArgs
        const ChainArgs c = make_chain_args(h, o, active, 1);
        EXPECT(L.c.aq.status == c.aq.status && L.c.sw.s.K == c.sw.s.K && L.c.ta.backoff == c.ta.backoff && L.c.ta.backoff == h->backoff);
        EXPECT(L.c.aq.B == B && L.c.aq.active == active && L.c.aq.alive == h->alive && L.c.aq.beta_w == h->beta && L.c.sw.s.A == h->A && L.c.sw.s.N == d.N && L.c.ta.ubg == h->ubg);
        EXPECT(L.c.active == active && L.c.success == h->success && L.c.infeas == h->infeas && L.c.times == h->chain_times);
        EXPECT(L.c.max_ticks == qp_max_ticks(old.q1, o.qp_max_iter) && L.c.max_ticks > 0);
        EXPECT(L.c.lag == nullptr && L.c.runm == nullptr && L.c.done == nullptr && L.c.t0word == nullptr && L.c.budget == 0 && L.c.fin_count == nullptr && L.c.cut_count == 0xFFFFFFFFu);
        EXPECT(L.c.qplog == h->qplog && L.c.x0vlog == h->x0vlog && L.c.stepno == h->cl_stepno && L.c.log_steps == h->qplog_steps);
        // the parts around the chain
        const ClArgs cl = cl_args(h, nullptr);
        EXPECT(L.cl.B == B && L.cl.N == d.N && L.cl.NX == d.nx && L.cl.NU == d.nu && L.cl.Xn == h->Xn && L.cl.Un == h->Un && L.cl.xmeas == h->xmeas && L.cl.primal == h->primal &&
               L.cl.success == h->success && L.cl.x0arg == h->x0arg && L.cl.E == h->E && L.cl.w == nullptr && L.cl.u0 == h->u0 && L.cl.u_init == h->u_init && L.cl.B == cl.B);
        EXPECT(L.lin.B == B && L.lin.N == d.N && L.lin.A == h->A && L.lin.Bm == h->Bm && L.lin.c == h->c && L.lin.q == h->q && L.lin.cst.Qd == h->cst && L.lin.cst.Rd == h->cst + d.nx);
        EXPECT(L.ba.B == B && L.ba.N == d.N && L.ba.NX == d.nx && L.ba.NI == d.ni && L.ba.NIF == d.ni_f && L.ba.g == h->g && L.ba.gN == h->gN && L.ba.c == h->c && L.ba.ubg == h->ubg &&
               L.ba.lbg == h->lbg && L.ba.eps == 1e-10 && L.ba.run == nullptr);
        EXPECT(L.sb.B == B && L.sb.NX == d.nx && L.sb.x0 == h->x0arg && L.sb.x0val == h->x0val && L.sb.active == active && L.sb.alive == h->alive && L.sb.infeas == h->infeas &&
               L.sb.success == h->success && L.sb.pending == h->pending_reset && L.sb.itnum == h->itnum && L.sb.stale == h->stale && L.sb.eta == h->eta && L.sb.eta_f == h->eta_f &&
               L.sb.neta == (size_t)d.N * d.N * d.ni && L.sb.netaf == (size_t)(d.N + 1) * d.ni_f && L.sb.ib.B == B && L.sb.ib.N == d.N && L.sb.ib.eps == o.eps_backoff &&
               L.sb.ib.run == active && L.sb.ib.backoff == h->backoff && L.sb.ib.backoff_u == h->backoff_u);
        EXPECT(L.lg.B == B && L.lg.N == d.N && L.lg.NX == d.nx && L.lg.NU == d.nu);
        EXPECT(L.sa.ii == 0 && L.sa.converge == 0 && L.sa.eps == o.scp_eps && L.sa.active == h->scp_active && L.sa.scp_success == h->scp_success && L.sa.scp_iters == h->scp_iters &&
               L.sa.updated == h->scp_upd);
        EXPECT(L.steps == steps && L.n == h->n && L.have_log == 1 && L.fence == 3 && L.keep_laggards == 1);
        EXPECT(L.stepno == h->cl_stepno && L.call_ids == h->call_ids && L.q == h->q && L.stale == h->stale && L.itnum == h->itnum && L.pending == h->pending_reset && L.scp_active == h->scp_active);
        EXPECT(L.W_all == dW && L.pinf == h->pinf && L.busy == h->cl_busy && L.t_begin == h->cl_tbegin);
        EXPECT(L.Q.slots == h->clq_slots && L.Q.mask == h->clq_cap - 1u && L.Q.head == (unsigned *)h->clq_ctl && L.Q.tail == (unsigned *)h->clq_ctl + 1 && L.Q.avail == h->clq_ctl + 2 &&
               L.Q.err == h->clq_ctl + 3);
        EXPECT(G.max_it == (scp ? rti : 1) && G.converge == 0 && G.rti_steps == o.rti_steps && G.nsolves == h->qplog_nsolves);
        // a second launch of the same handle with other steps and options: the staged block follows
        o.warm_rounds += 2; o.as_first = 1 - o.as_first;
        h->qplog_steps = 2; h->log_steps = 0;
        const ScpLoopArgs S2 = make_loop_block(h, 2, nullptr, o, scp != 0, rti);
        stage_loop_block(h, S2);
        std::memcpy(&G, h->loop_blk_host.data(), sizeof G);
        EXPECT(G.L.steps == 2 && G.L.c.log_steps == 2 && G.L.have_log == 0 && G.L.W_all == nullptr && G.L.c.q.warm_rounds == o.warm_rounds && G.L.c.q.as_first == o.as_first);
        delete h;
    }
    check_compositions();
    check_with_dims();
    check_no_launch();
    if (fails) return 1;
    std::printf("loop_args_check ok\n");
    return 0;
}
