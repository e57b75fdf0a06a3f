// Stand-alone host program (own main) around the state-feedback disturbance adversary, built by tests/test_adversary_cpu.py
// with -fsanitize=address,undefined from csrc/slsqp_api.hip compiled for the host only, as tests/cl_sls_conv_check_main.cpp is.  The handle is a
// value-initialised slsqp_handle with made-up device addresses: nothing dereferences them, no launch is entered.
//   no argument:
//     1. the decision function of csrc/cl_adversary.hpp on a table of cases: the tie, absent sides, a NaN state, a dense E whose sum cancels, a padded
//        channel, the mask, amp, policy 2 with and without a reference, the row min(s, T - 1) of shared and per-instance tables, the log's last entry;
//     2. the setter's validation routine, message by message;
//     3. cl_options with the option on: the PP bit, the model's row as the plant's parameters, the handle's own flags untouched;
//     4. the argument block: ScpLoopArgs and the blocks behind it where they were, the new block aligned and inside the buffer, the staged
//        ScpLoopArgs independent of the option.
//   shim IN OUT: a host shim for tests/test_adversary_cpu.py -- IN holds cases as doubles [policy, nx, nz, amp, mask bits, has_W, x (nx), g (2 nz),
//     xref (nx), E (nx nx), W (nx)], OUT receives w_applied (nx) of every case.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../robust-nonlinear-mpc_amd/csrc/slsqp_api.hip"

extern "C" {
extern const char __hip_fatbin[8] = {0};
void **__hipRegisterFatBinary(const void *) { static void *handle; return &handle; }
void __hipRegisterFunction(void **, const void *, char *, const char *, unsigned, void *, void *, void *, void *, int *) {}
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}
void __hipUnregisterFatBinary(void **) {}
}
static int launches_entered = 0;
extern "C" hipError_t __hipPushCallConfiguration(dim3, dim3, size_t, hipStream_t) { launches_entered++; return hipErrorUnknown; }

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static const double INF = std::numeric_limits<double>::infinity(), NaN = std::numeric_limits<double>::quiet_NaN();
namespace adv = cl_adversary;

// one instance, one step, tables of one row: g (2 nz) = [hi; -lo], xref (nx) or NULL (zeros), W (nx) or NULL
static std::vector<double> one(int policy, double amp, unsigned mask, int nx, int nz, const double *x, const double *g, const double *xref, const double *E, const double *W) {
    std::vector<double> out(nx, -777.0), zero(nz, 0.0);
    adv::Args a;
    std::memset(&a, 0, sizeof a);
    a.policy = policy; a.nz = nz; a.mask = mask; a.amp = amp; a.adv_w = out.data(); a.lg = nullptr; a.S = 0;
    a.bd = adv::Tab{g, 1, 0}; a.bdW = 2 * nz; a.rf = adv::Tab{xref ? xref : zero.data(), 1, 0};
    adv::decide(a, nx, 0, 0, x, E, W);
    return out;
}

static void check_cases() {
    const unsigned ALL = 0xFFFFFFFFu;
    {   // nx = 2, nu = 1: g = [hi_x0 hi_x1 hi_u | -lo_x0 -lo_x1 -lo_u], diagonal E
        const double E[4] = {0.5, 0.0, 0.0, -0.25}, W[2] = {0.125, -0.375};
        double g[6] = {2.0, 4.0, 1.0, 2.0, 0.0, 1.0};      // x0 in [-2, 2], x1 in [0, 4]
        double x[2] = {0.0, 2.0};      // both exactly mid-box: the tie gives +1
        std::vector<double> w = one(adv::NEAREST_BOUND, 1.0, ALL, 2, 3, x, g, nullptr, E, W);
        EXPECT(w[0] == 1.0 && w[1] == -1.0);      // (E_11 < 0: pushing x1 up takes w_1 = -amp)
        x[0] = -0.5; x[1] = 2.5;
        w = one(adv::NEAREST_BOUND, 1.0, ALL, 2, 3, x, g, nullptr, E, W);
        EXPECT(w[0] == -1.0 && w[1] == -1.0);
        x[1] = 1.5;
        w = one(adv::NEAREST_BOUND, 0.5, ALL, 2, 3, x, g, nullptr, E, W);      // amp
        EXPECT(w[0] == -0.5 && w[1] == 0.5);
        // each side absent, through +inf and through 1e20
        for (double none : {INF, 1e20, 3e20}) {
            double gh[6] = {none, 4.0, 1.0, 2.0, 0.0, 1.0};      // no upper side of x0: only lo pulls
            x[0] = 1.9; x[1] = 2.0;
            w = one(adv::NEAREST_BOUND, 1.0, ALL, 2, 3, x, gh, nullptr, E, W);
            EXPECT(w[0] == -1.0 && w[1] == -1.0);
            double gl[6] = {2.0, 4.0, 1.0, none, 0.0, 1.0};      // no lower side of x0: only hi pulls
            x[0] = -1.9;
            w = one(adv::NEAREST_BOUND, 1.0, ALL, 2, 3, x, gl, nullptr, E, W);
            EXPECT(w[0] == 1.0);
            double gn[6] = {none, 4.0, 1.0, none, 0.0, 1.0};      // neither: the given sample
            w = one(adv::NEAREST_BOUND, 1.0, ALL, 2, 3, x, gn, nullptr, E, W);
            EXPECT(w[0] == 0.125 && w[1] == -1.0);
            w = one(adv::NEAREST_BOUND, 1.0, ALL, 2, 3, x, gn, nullptr, E, nullptr);      // ... which is 0 where the caller gave none
            EXPECT(w[0] == 0.0 && !std::signbit(w[0]));
        }
        double gj[6] = {2.0, 4.0, 1.0, 2.0, 0.0, 1.0};
        gj[0] = 0.99e20;      // just below the threshold: a side like any other
        x[0] = 0.0;
        w = one(adv::NEAREST_BOUND, 1.0, ALL, 2, 3, x, gj, nullptr, E, W);
        EXPECT(w[0] == -1.0);
        // a NaN state pushes nowhere, under both policies
        x[0] = NaN; x[1] = 3.0;
        w = one(adv::NEAREST_BOUND, 1.0, ALL, 2, 3, x, g, nullptr, E, W);
        EXPECT(w[0] == 0.125 && w[1] == -1.0);
        w = one(adv::AWAY_FROM_TARGET, 1.0, ALL, 2, 3, x, g, nullptr, E, W);
        EXPECT(w[0] == 0.125 && w[1] == -1.0);
        // the mask: a channel outside it keeps the given sample
        x[0] = 1.0; x[1] = 3.0;
        w = one(adv::NEAREST_BOUND, 1.5, 0x2u, 2, 3, x, g, nullptr, E, W);
        EXPECT(w[0] == 0.125 && w[1] == -1.5);
        w = one(adv::NEAREST_BOUND, 1.5, 0x0u, 2, 3, x, g, nullptr, E, W);
        EXPECT(w[0] == 0.125 && w[1] == -0.375);
        // policy 0 copies
        w = one(adv::OFF, 1.0, ALL, 2, 3, x, g, nullptr, E, W);
        EXPECT(w[0] == 0.125 && w[1] == -0.375);
        // policy 2: without a reference away from the origin (x = 0 counts as above), with one away from it
        x[0] = 0.0; x[1] = -0.1;
        w = one(adv::AWAY_FROM_TARGET, 1.0, ALL, 2, 3, x, g, nullptr, E, W);
        EXPECT(w[0] == 1.0 && w[1] == 1.0);
        const double xr[3] = {0.5, -0.2, 9.0};
        w = one(adv::AWAY_FROM_TARGET, 2.0, ALL, 2, 3, x, g, xr, E, W);
        EXPECT(w[0] == -2.0 && w[1] == -2.0);
    }
    {   // a dense E: two states pull channel 0 in opposite directions and cancel exactly -> the given sample; channel 1 adds up; channel 2 is padding (nw = 2 < nx = 3)
        const double E[9] = {0.75, 0.5, 0.0,
                             0.75, 0.25, 0.0,
                             0.0, -0.125, 0.0};
        const double g[8] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0}, W[3] = {0.3, 0.4, 0.6};
        const double x[3] = {0.5, -0.5, 0.25};      // d = (+1, -1, +1)
        std::vector<double> w = one(adv::NEAREST_BOUND, 1.0, 0xFFFFFFFFu, 3, 4, x, g, nullptr, E, W);
        EXPECT(w[0] == 0.3);      // 0.75 - 0.75 = 0
        EXPECT(w[1] == 1.0);      // 0.5 - 0.25 - 0.125 > 0
        EXPECT(w[2] == 0.6);      // a padded column of E
        unsigned pos = 0, neg = 0;
        adv::directions(adv::NEAREST_BOUND, 3, 4, x, g, nullptr, &pos, &neg);
        EXPECT(pos == 0x5u && neg == 0x2u);
    }
    {   // row selection min(s, T - 1): a shared table and a per-instance one, bounds and reference, and the log
        const int nx = 1, nz = 2, W_ = 2 * nz + 2 * nx, T = 3, B = 2;
        std::vector<double> bd((size_t)B * T * W_, 0.0), rf((size_t)B * T * nz, 0.0);
        for (int b = 0; b < B; b++)
            for (int t = 0; t < T; t++) {
                double *r = bd.data() + ((size_t)b * T + t) * W_;
                r[0] = 1.0 + t + 10.0 * b; r[1] = 1.0; r[2] = 1.0; r[3] = 1.0;      // hi of x0 moves with (b, t); lo = -1
                rf[((size_t)b * T + t) * nz] = 0.5 * t - 1.0 * b;
            }
        EXPECT(adv::row_at(adv::Tab{bd.data(), T, 0}, 1, 1, W_) == bd.data() + W_);      // shared: the instance does not matter
        EXPECT(adv::row_at(adv::Tab{bd.data(), T, 0}, 0, 7, W_) == bd.data() + 2 * W_);      // the last row is held
        EXPECT(adv::row_at(adv::Tab{bd.data(), T, (size_t)T * W_}, 1, 1, W_) == bd.data() + (size_t)(T + 1) * W_);
        EXPECT(adv::row_at(adv::Tab{bd.data(), T, (size_t)T * W_}, 1, 9, W_) == bd.data() + (size_t)(T + 2) * W_);
        EXPECT(adv::row_at(adv::Tab{bd.data(), 1, 0}, 3, 4, W_) == bd.data());
        const double E[1] = {2.0}, xb[2] = {0.4, 0.4}, x[2] = {0.6, 0.6};      // (B, nx): the states of the bounds' cases and of the reference's
        const int S = 2;
        std::vector<double> out((size_t)B * nx, -7.0), lg((size_t)B * S * nx, -7.0);
        adv::Args a;
        std::memset(&a, 0, sizeof a);
        a.policy = adv::NEAREST_BOUND; a.nz = nz; a.mask = 1u; a.amp = 1.0; a.adv_w = out.data(); a.lg = lg.data(); a.S = S;
        a.bd = adv::Tab{bd.data(), T, (size_t)T * W_}; a.bdW = W_; a.rf = adv::Tab{rf.data(), T, (size_t)T * nz};
        adv::decide(a, nx, 0, 0, xb, E, nullptr);      // b 0, s 0: box [-1, 1], x = 0.4 -> up
        EXPECT(out[0] == 1.0 && lg[0] == 1.0);
        adv::decide(a, nx, 0, 1, xb, E, nullptr);      // s 1: box [-1, 2] -> down
        EXPECT(out[0] == -1.0 && lg[1] == -1.0);
        adv::decide(a, nx, 0, 5, xb, E, nullptr);      // s 5: row 2, box [-1, 3]; past the log's last entry nothing is written
        EXPECT(out[0] == -1.0 && lg[0] == 1.0 && lg[1] == -1.0);
        adv::decide(a, nx, 1, 0, xb + 1, E, nullptr);      // b 1: box [-1, 11]
        EXPECT(out[1] == -1.0 && lg[2] == -1.0 && lg[3] == -7.0);
        a.bd.stride = 0;      // shared: instance 1 reads instance 0's rows
        adv::decide(a, nx, 1, 0, xb + 1, E, nullptr);
        EXPECT(out[1] == 1.0);
        a.policy = adv::AWAY_FROM_TARGET;      // xref rows: b 0: -, 0.5, 1.0; b 1: -1, -0.5, 0
        adv::decide(a, nx, 0, 1, x, E, nullptr);
        EXPECT(out[0] == 1.0);      // 0.6 >= 0.5
        adv::decide(a, nx, 0, 2, x, E, nullptr);
        EXPECT(out[0] == -1.0);      // 0.6 < 1.0
        adv::decide(a, nx, 0, 3, x, E, nullptr);
        EXPECT(out[0] == -1.0);      // held
        adv::decide(a, nx, 1, 2, x + 1, E, nullptr);
        EXPECT(out[1] == 1.0);
        a.rf.stride = 0;
        adv::decide(a, nx, 1, 2, x + 1, E, nullptr);
        EXPECT(out[1] == -1.0);
    }
}

// ---- 2: the setter's validation
static void check_validation() {
    std::string why;
    EXPECT(adv::check(0, NaN, false, true, 4, &why));      // clearing reads nothing else
    EXPECT(adv::check(1, 1.0, true, false, 4, &why) && adv::check(2, 1.5, true, false, 17, &why) && adv::check(1, 1e-300, true, false, 4, &why));
    EXPECT(!adv::check(3, 1.0, true, false, 4, &why) && why.find("policy = 3") != std::string::npos);
    EXPECT(!adv::check(-1, 1.0, true, false, 4, &why) && why.find("policy = -1") != std::string::npos);
    for (double bad : {NaN, INF, -INF, 0.0, -0.5}) { why.clear(); EXPECT(!adv::check(1, bad, true, false, 4, &why) && why.find("amp = ") == 0 && why.find("finite and > 0") != std::string::npos); }
    EXPECT(!adv::check(1, 1.0, false, false, 4, &why) && why.find("slsqp_set_model must be called first") != std::string::npos);
    EXPECT(!adv::check(2, 1.0, true, true, 4, &why) && why.find("general G") != std::string::npos);
    const unsigned char mk[4] = {1, 0, 7, 0};
    EXPECT(adv::mask_bits(nullptr, 4) == 0xFu && adv::mask_bits(mk, 4) == 0x5u && adv::mask_bits(nullptr, 17) == 0x1FFFFu);
    // the setter itself on a handle without a model: refused before anything is touched, the setting as it was
    slsqp_handle *h = new slsqp_handle();
    h->d.nx = 4; h->d.nu = 1; h->model_id = -1;
    EXPECT(slsqp_cl_set_adversary(h, 1, 1.0, nullptr) != 0 && std::strstr(slsqp_last_error(), "slsqp_cl_set_adversary: handle: slsqp_set_model"));
    h->model_id = 0;
    EXPECT(slsqp_cl_set_adversary(h, 5, 1.0, nullptr) != 0 && std::strstr(slsqp_last_error(), "policy = 5"));
    EXPECT(slsqp_cl_set_adversary(h, 2, -1.0, nullptr) != 0 && std::strstr(slsqp_last_error(), "amp = "));
    h->general_G = true;
    EXPECT(slsqp_cl_set_adversary(h, 2, 1.0, nullptr) != 0 && std::strstr(slsqp_last_error(), "general G"));
    int pol = -1; double amp = -1.0;
    EXPECT(slsqp_cl_get_adversary(h, &pol, &amp) == 0 && pol == 0 && amp == 1.0);
    delete h;
}

static uintptr_t next_addr = 0x10000;
#define FAKE(f) do { h->f = (decltype(h->f))(next_addr); next_addr += 0x1000; } while (0)
static slsqp_handle *fake_handle(int B, int N) {
    slsqp_handle *h = new slsqp_handle();
    h->B = B; h->d.N = N; h->d.nx = 4; h->d.nu = 1; h->d.nw = 4; h->d.ni = 10; h->d.ni_f = 8; h->n = 5 * N + 4; h->nz = 5;
    h->call_id = 7.0; h->log_steps = 6; h->qplog_steps = 6; h->qplog_cap = 8; h->clq_cap = 32; h->model_id = 0;
    FAKE(A); FAKE(Aclc); FAKE(Bm); FAKE(E); FAKE(K); FAKE(Kc); FAKE(Linv); FAKE(Un); FAKE(Xn); FAKE(alive); FAKE(backoff); FAKE(backoff_f); FAKE(backoff_u);
    FAKE(backoff_x); FAKE(beta); FAKE(beta_f); FAKE(c); FAKE(call_ids); FAKE(chain_times); FAKE(cl_busy); FAKE(cl_stepno); FAKE(cl_tbegin); FAKE(clq_ctl);
    FAKE(clq_slots); FAKE(conv); FAKE(cost); FAKE(cost_tube); FAKE(counter); FAKE(cst); FAKE(ct_part); FAKE(dual); FAKE(eta); FAKE(eta_f); FAKE(g); FAKE(gN);
    FAKE(g_raw); FAKE(gf_raw); FAKE(has_prev); FAKE(infeas); FAKE(inst_launches); FAKE(iters); FAKE(itnum); FAKE(kkt); FAKE(lbg); FAKE(lg_bu); FAKE(lg_bx);
    FAKE(lg_it); FAKE(lg_pinf); FAKE(lg_state); FAKE(lg_succ); FAKE(lg_u); FAKE(lg_u0); FAKE(lg_x); FAKE(lin_stage); FAKE(lin_tape); FAKE(mask);
    FAKE(pending_reset); FAKE(pin_dual); FAKE(pinf); FAKE(prev_primal); FAKE(primal); FAKE(q); FAKE(qp_diag); FAKE(qplog); FAKE(qplog_nsolves); FAKE(qpstat);
    FAKE(qpstate); FAKE(scp_active); FAKE(scp_dmax); FAKE(scp_iters); FAKE(scp_success); FAKE(scp_upd); FAKE(stale); FAKE(status); FAKE(success); FAKE(u0);
    FAKE(u_init); FAKE(ubg); FAKE(ws); FAKE(x0arg); FAKE(x0val); FAKE(x0vlog); FAKE(xmeas); FAKE(zero_ref);
    FAKE(hold_xi); FAKE(hold_u); FAKE(hold_policy); FAKE(lg_x0v); FAKE(lg_hold); FAKE(lg_hpol); FAKE(sls_itlog); FAKE(lg_merr); FAKE(lg_wadv);
    return h;
}

// ---- 3: the option states with the adversary on
static void check_option_states() {
    static const int base[8] = {/* 000 */ 0, /* 001 */ 5, /* 010 */ 3, /* 011 */ 7, /* 100 */ 1, /* 101 */ 5, /* 110 */ 3, /* 111 */ 7};
    for (int st = 0; st < 16; st++) {
        const bool hold = st & 8, ref = st & 4, pp = st & 2, bnd = st & 1;
        slsqp_handle *h = fake_handle(5, 3);
        if (ref) { FAKE(ref_Y); h->ref_T = 2; h->ref_stride = 2 * 5; }
        if (pp) { FAKE(pp_P); FAKE(pp_merr); h->pp_np = 3; h->pp_stride = 3; }
        if (bnd) { FAKE(bnd_rows); h->bnd_T = 2; h->bnd_stride = 2 * 18; }
        if (hold) EXPECT(slsqp_cl_set_solve_every(h, 2) == 0);
        const ClOptions off = cl_options(h);
        EXPECT(off.var == (base[st & 7] | (hold ? 9 : 0)) && !off.adv);
        FAKE(adv_buf); h->adv_merr = h->adv_buf + 3; h->adv_w = h->adv_merr + 20;      // what the setter's first call allocates
        h->adv_policy = 2; h->adv_amp = 0.5; h->adv_mask = 0x6u;
        const ClOptions on = cl_options(h);
        EXPECT(on.adv && on.var == (off.var | VAR_REF | VAR_PP));      // the PP variants (which come with REF), nothing else
        EXPECT(on.ref == off.ref && on.pp == off.pp && on.bnd == off.bnd && on.hold == off.hold && on.fallback == off.fallback);
        EXPECT(on.own_rf.rows == off.own_rf.rows);
        if (pp) EXPECT(on.pa.P == h->pp_P && on.pa.stride == 3 && on.pa.model_err == h->pp_merr && on.pa.lg == h->lg_merr);      // the handle's own parameters stay
        else EXPECT(on.pa.P == h->adv_buf && on.pa.stride == 0 && on.pa.model_err == h->adv_merr && on.pa.lg == h->lg_merr && on.pa.S == 6);      // the model's row, shared
        EXPECT(on.rf.rows == (ref ? h->ref_Y : h->zero_ref));
        const AdvArgs &A = on.aa;
        EXPECT(A.policy == 2 && A.amp == 0.5 && A.mask == 0x6u && A.nz == 5 && A.adv_w == h->adv_w && A.lg == h->lg_wadv && A.S == 6);
        if (bnd) EXPECT(A.bd.rows == h->bnd_rows && A.bd.T == 2 && A.bd.stride == 36 && A.bdW == 18);
        else EXPECT(A.bd.rows == h->g_raw && A.bd.T == 1 && A.bd.stride == 0 && A.bdW == 10);
        if (ref) EXPECT(A.rf.rows == h->ref_Y && A.rf.T == 2 && A.rf.stride == 10);
        else EXPECT(A.rf.rows == h->zero_ref && A.rf.T == 1 && A.rf.stride == 0);
        int seen = -1;
        EXPECT(with_loop_var(on.var, [&](auto V) { seen = V(); }, hold) && seen == on.var);      // an instantiated set: no new one
        h->log_steps = 0;
        EXPECT(cl_options(h).aa.lg == nullptr && cl_options(h).aa.S == 0);
        h->adv_policy = 0;      // cleared: as if it had never been set
        const ClOptions cleared = cl_options(h);
        EXPECT(cleared.var == off.var && !cleared.adv && cleared.pa.P == off.pa.P && cleared.aa.policy == 0 && cleared.aa.adv_w == nullptr);
        delete h;
    }
}

// ---- 4: the layouts and the staged block
static void check_layout() {
    static_assert(sizeof(ScpLoopArgs) == 2120 && sizeof(LoopArgs) == 2056, "the persistent kernels' argument block keeps its size");
    static_assert(HOLD_BLK_OFFSET == 2128, "the hold block stays where it was");
    static_assert(PLAN_BLK_OFFSET == ((HOLD_BLK_OFFSET + sizeof(HoldLoopArgs) + 15) & ~(size_t)15), "the plan block stays where it was");
    static_assert(CONV_BLK_OFFSET >= PLAN_BLK_OFFSET + sizeof(PlanArgs) && CONV_BLK_OFFSET % 16 == 0 && CONV_BLK_OFFSET + sizeof(SlsConvArgs) <= LOOP_BLK_BYTES,
                  "the CONV block stays where it was");
    static_assert(CONV_BLK_OFFSET == ((PLAN_BLK_OFFSET + sizeof(PlanArgs) + 15) & ~(size_t)15), "the CONV block stays where it was");
    static_assert(ADV_BLK_OFFSET >= CONV_BLK_OFFSET + sizeof(SlsConvArgs) && ADV_BLK_OFFSET % 16 == 0 && ADV_BLK_OFFSET + sizeof(AdvArgs) <= LOOP_BLK_BYTES,
                  "the new block lies behind the CONV block, 16-byte aligned, inside the handle's buffer");
    static_assert(sizeof(AdvArgs) == 96 && offsetof(AdvArgs, policy) == 0 && offsetof(AdvArgs, amp) == 16, "the block's layout (DESIGN.md section 24)");
    slsqp_opts o;
    slsqp_default_opts(&o);
    slsqp_handle *h = fake_handle(5, 4);
    const ScpLoopArgs off = make_loop_block(h, 6, nullptr, o, false, 1);
    FAKE(adv_buf); h->adv_merr = h->adv_buf + 3; h->adv_w = h->adv_merr + 20;
    h->adv_policy = 1; h->adv_amp = 1.0; h->adv_mask = 0xFu;
    const ScpLoopArgs on = make_loop_block(h, 6, nullptr, o, false, 1);
    EXPECT(std::memcmp(&off, &on, sizeof off) == 0);      // the option is not in the ScpLoopArgs: its own block carries it
    const AdvArgs a1 = adv_args(h), a2 = adv_args(h);
    EXPECT(std::memcmp(&a1, &a2, sizeof a1) == 0);      // (padding included: built from zero bytes)
    EXPECT(h->adv_blk_host.empty() && h->adv_blk_dev == 0);
    EXPECT(launches_entered == 0);
    delete h;
}

static int shim(const char *in, const char *outp) {
    std::FILE *f = std::fopen(in, "rb");
    if (!f) return 2;
    std::vector<double> buf;
    double tmp[256];
    size_t n;
    while ((n = std::fread(tmp, sizeof(double), 256, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
    std::fclose(f);
    std::vector<double> res;
    size_t p = 0;
    while (p + 6 <= buf.size()) {
        const int policy = (int)buf[p], nx = (int)buf[p + 1], nz = (int)buf[p + 2];
        const double amp = buf[p + 3];
        const unsigned mask = (unsigned)buf[p + 4];
        const bool has_W = buf[p + 5] != 0.0;
        p += 6;
        const size_t need = (size_t)nx + 2 * nz + nx + (size_t)nx * nx + nx;
        if (nx < 1 || nx > adv::MAX_NX || nz < nx || p + need > buf.size()) return 3;
        const double *x = &buf[p], *g = x + nx, *xref = g + 2 * nz, *E = xref + nx, *W = E + (size_t)nx * nx;
        p += need;
        const std::vector<double> w = one(policy, amp, mask, nx, nz, x, g, xref, E, has_W ? W : nullptr);
        res.insert(res.end(), w.begin(), w.end());
    }
    f = std::fopen(outp, "wb");
    if (!f) return 2;
    std::fwrite(res.data(), sizeof(double), res.size(), f);
    std::fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !std::strcmp(argv[1], "shim")) return shim(argv[2], argv[3]);
    check_cases();
    check_validation();
    check_option_states();
    check_layout();
    if (fails) { std::printf("cl_adversary_check: %d failures\n", fails); return 1; }
    std::printf("cl_adversary_check ok\n");
    return 0;
}
