// Stand-alone host program (own main) around what the event-triggered hold schedule needs on the host, built by
// tests/test_hold_trigger_cpu.py with -fsanitize=address,undefined from csrc/slsqp_api.hip compiled for the host only, as
// tests/cl_hold_loop_check_main.cpp is.  The handle is a value-initialised slsqp_handle with made-up device addresses: nothing dereferences them, no
// launch is entered.
//   1. cl_hold::tube_term and cl_hold::decide: every precedence case, theta in {0, 0.5, inf}, a NaN ratio, M in 1..N, and whole schedules driven by
//      made-up ratios (a run begins with a solve, hold indices count up from their solve and stay below M, a failed plan solves at once);
//   2. slsqp_cl_set_hold_trigger: the range, refusals that change nothing, the default;
//   3. HoldLoopArgs: the fields it had keep their offsets, the new ones lie behind M, the block fits the handle's buffer, make_hold_block names the
//      buffers and is byte-identical for two calls.
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

static uintptr_t next_addr = 0x10000;
#define FAKE(f) do { h->f = (decltype(h->f))(next_addr); next_addr += 0x1000; } while (0)

static const double INF = std::numeric_limits<double>::infinity(), NaN = std::numeric_limits<double>::quiet_NaN();

static slsqp_handle *fake_handle(int B, int N) {
    slsqp_handle *h = new slsqp_handle();
    h->B = B; h->d.N = N; h->d.nx = 4; h->d.nu = 1; h->d.nw = 4; h->d.ni = 10; h->d.ni_f = 8; h->n = 5 * N + 4;
    h->log_steps = 6;
    FAKE(A); FAKE(Bm); FAKE(E); FAKE(K); FAKE(Kc); FAKE(Un); FAKE(Xn); FAKE(backoff_x); FAKE(scp_success); FAKE(stale); FAKE(u0); FAKE(xmeas); FAKE(x0arg);
    FAKE(hold_xi); FAKE(hold_u); FAKE(hold_policy); FAKE(hold_k); FAKE(lg_state); FAKE(lg_u0); FAKE(lg_x0v); FAKE(lg_it); FAKE(lg_hold); FAKE(lg_hpol);
    FAKE(lg_ratio); FAKE(lg_trig);
    // what make_loop_block offsets or names besides
    FAKE(cst); FAKE(Aclc); FAKE(Linv); FAKE(alive); FAKE(backoff); FAKE(backoff_f); FAKE(backoff_u); FAKE(beta); FAKE(beta_f); FAKE(c); FAKE(call_ids); FAKE(chain_times);
    FAKE(cl_busy); FAKE(cl_stepno); FAKE(cl_tbegin); FAKE(clq_ctl); FAKE(clq_slots); FAKE(conv); FAKE(cost); FAKE(cost_tube); FAKE(counter); FAKE(ct_part); FAKE(dual);
    FAKE(eta); FAKE(eta_f); FAKE(g); FAKE(gN); FAKE(g_raw); FAKE(gf_raw); FAKE(has_prev); FAKE(infeas); FAKE(inst_launches); FAKE(iters); FAKE(itnum); FAKE(kkt); FAKE(lbg);
    FAKE(lg_bu); FAKE(lg_bx); FAKE(lg_pinf); FAKE(lg_succ); FAKE(lg_u); FAKE(lg_x); FAKE(lin_stage); FAKE(lin_tape); FAKE(mask); FAKE(pending_reset); FAKE(pin_dual);
    FAKE(pinf); FAKE(prev_primal); FAKE(primal); FAKE(q); FAKE(qp_diag); FAKE(qplog); FAKE(qplog_nsolves); FAKE(qpstat); FAKE(qpstate); FAKE(scp_active); FAKE(scp_dmax);
    FAKE(scp_iters); FAKE(scp_upd); FAKE(status); FAKE(success); FAKE(u_init); FAKE(ubg); FAKE(ws); FAKE(x0val); FAKE(x0vlog); FAKE(zero_ref);
    h->call_id = 7.0; h->qplog_steps = 6; h->clq_cap = 32;
    return h;
}

// ---- 1: the ratio's terms and the decision
static void check_decide() {
    using namespace cl_hold;
    EXPECT(tube_term(1.0, 0.75, 0.5) == 0.5 && tube_term(0.75, 1.0, 0.5) == 0.5 && tube_term(2.0, 2.0, 0.5) == 0.0);
    EXPECT(tube_term(1.0, 1.0, 0.0) == 0.0 && tube_term(1.0, 1.0 + 1e-15, 0.0) == INF && tube_term(-0.0, 0.0, 0.0) == 0.0);      // a tube of zero width
    EXPECT(tube_term(NaN, 1.0, 0.5) == INF && tube_term(1.0, NaN, 0.0) == INF && tube_term(1.0, 2.0, NaN) == INF && tube_term(INF, INF, 1.0) == INF);
    EXPECT(tube_term(1.0, 2.0, INF) == 0.0 && tube_term(0.3, 0.1, 0.1) == std::fabs(0.3 - 0.1) / 0.1);      // plain fp64: one subtraction, one division
    EXPECT(TRIG_HOLD == 0 && TRIG_SCHEDULED == 1 && TRIG_TUBE == 2 && TRIG_FAILED == 3);
    for (int N = 1; N <= 6; N++)
        for (int M = 1; M <= N; M++) {
            EXPECT(valid_solve_every(M, N));
            for (double theta : {0.0, 0.5, INF}) {
                EXPECT(valid_trigger(theta) && trigger_on(theta, M) == (M > 1 && theta < INF));
                for (int ok = 0; ok < 2; ok++)
                    for (double r : {0.0, 0.25, 0.5, 0.75, 1e300, INF, NaN}) {
                        EXPECT(decide(0, 0, M, ok, r, theta) == TRIG_SCHEDULED);      // a run begins with a solve, whatever else holds
                        for (int kp = 0; kp < M; kp++) {
                            const int s = 7 + kp, code = decide(s, kp, M, ok, r, theta);
                            if (kp + 1 >= M) EXPECT(code == TRIG_SCHEDULED);      // the cap comes first: even for a failed plan and a ratio outside
                            else if (!ok) EXPECT(code == TRIG_FAILED);            // then the failed plan: the ratio is not read
                            else if (std::isnan(r) || r > theta) EXPECT(code == TRIG_TUBE);
                            else EXPECT(code == TRIG_HOLD);
                        }
                    }
                // a whole schedule from made-up ratios and outcomes
                int kp = 0, solves = 0;
                unsigned rng = 12345u + 97u * N + 13u * M;
                for (int s = 0; s < 40; s++) {
                    rng = rng * 1664525u + 1013904223u;
                    const double r = (rng >> 8) % 1000 / 800.0;
                    const bool ok = ((rng >> 20) % 7) != 0;
                    const int code = decide(s, kp, M, ok, r, theta);
                    if (s == 0) EXPECT(code == TRIG_SCHEDULED);
                    if (code == TRIG_HOLD) { kp++; EXPECT(ok && r <= theta && kp <= M - 1 && kp <= N - 1); } else { kp = 0; solves++; }
                    if (theta == INF && ok) EXPECT((code == TRIG_HOLD) == (kp != 0));
                    if (theta == 0.0 && r > 0.0) EXPECT(code != TRIG_HOLD);
                }
                if (M == 1) EXPECT(solves == 40);      // every step is a solve, theta is not read
                EXPECT(solves >= solves_in(40, M));    // the fixed period is the fewest solves a cap of M allows
            }
        }
    EXPECT(decide(3, 0, 4, true, 0.5, 0.5) == TRIG_HOLD && decide(3, 0, 4, true, std::nextafter(0.5, 1.0), 0.5) == TRIG_TUBE);      // r <= theta holds
    EXPECT(decide(3, 0, 4, true, 0.0, 0.0) == TRIG_HOLD && decide(3, 0, 4, true, INF, INF) == TRIG_HOLD && decide(3, 0, 4, true, NaN, INF) == TRIG_TUBE);
    EXPECT(decide(3, 2, 4, true, 0.0, 0.5) == TRIG_HOLD && decide(3, 3, 4, true, 0.0, 0.5) == TRIG_SCHEDULED && decide(4, 2, 3, false, NaN, 0.5) == TRIG_SCHEDULED);
    EXPECT(!valid_trigger(-1e-300) && !valid_trigger(-INF) && !valid_trigger(NaN) && valid_trigger(0.0) && valid_trigger(INF));
    // the hold state an event-triggered run leaves: "hold_index" per instance, and still no per-batch plan
    State st;
    on_init(st);
    EXPECT(!index_per_instance(st, 0) && !index_per_instance(st, 5));
    on_triggered_run(st, 5);
    std::string why;
    EXPECT(index_per_instance(st, 5) && next_index(st, true, 5, 4, 0, &why) == 0 && why.find("slsqp_cl_run") != std::string::npos);
    EXPECT(!index_per_instance(st, 6) && index(st, 6) == 0 && next_index(st, true, 6, 4, 0, &why) == 1);      // after a slsqp_cl_step
    on_init(st);
    EXPECT(!index_per_instance(st, 5));
}

// ---- 2: the setter
static void check_setter() {
    slsqp_handle *h = fake_handle(5, 4);
    EXPECT(slsqp_cl_get_hold_trigger(h) == INF);      // off by default
    for (double theta : {0.0, 0.5, 1.0, 1e300, INF}) EXPECT(slsqp_cl_set_hold_trigger(h, theta) == 0 && slsqp_cl_get_hold_trigger(h) == theta);
    EXPECT(slsqp_cl_set_hold_trigger(h, 0.5) == 0 && slsqp_cl_set_solve_every(h, 3) == 0);
    const ClOptions before = cl_options(h);
    for (double bad : {-1.0, -1e-300, -INF, NaN}) {
        EXPECT(slsqp_cl_set_hold_trigger(h, bad) != 0 && std::strstr(slsqp_last_error(), "outside [0, +inf]"));
        EXPECT(slsqp_cl_get_hold_trigger(h) == 0.5 && slsqp_cl_get_solve_every(h) == 3);
    }
    // theta is no option bit: the variant is the one of solve_every alone
    EXPECT(before.var == (VAR_HOLD | VAR_REF) && cl_options(h).var == before.var);
    EXPECT(slsqp_cl_set_hold_trigger(h, INF) == 0 && cl_options(h).var == before.var);
    EXPECT(slsqp_cl_set_solve_every(h, 1) == 0 && slsqp_cl_set_hold_trigger(h, 0.25) == 0 && cl_options(h).var == 0 && !cl_options(h).hold);
    delete h;
}

// ---- 3: the hold block
#define OFF(T, f, at) static_assert(offsetof(T, f) == at, "a field of the hold block has moved: " #T "::" #f)
static void check_layout() {
    static_assert(sizeof(HoldArgs) == 232 && sizeof(ClArgs) == 96, "the arguments of the hold function keep their size");
    OFF(HoldLoopArgs, a, 0); OFF(HoldLoopArgs, M, 232);      // what the block held before the trigger
    OFF(HoldArgs, cl, 0); OFF(HoldArgs, k, 96); OFF(HoldArgs, A, 104); OFF(HoldArgs, Bm, 112); OFF(HoldArgs, K, 120); OFF(HoldArgs, Kc, 128); OFF(HoldArgs, stale, 136);
    OFF(HoldArgs, scp_success, 144); OFF(HoldArgs, xi, 152); OFF(HoldArgs, u, 160); OFF(HoldArgs, policy, 168); OFF(HoldArgs, S, 176); OFF(HoldArgs, step, 180);
    OFF(HoldArgs, lstate, 184); OFF(HoldArgs, lu0, 192); OFF(HoldArgs, lx0v, 200); OFF(HoldArgs, lit, 208); OFF(HoldArgs, lhold, 216); OFF(HoldArgs, lpol, 224);
    OFF(HoldLoopArgs, theta, 240); OFF(HoldLoopArgs, backoff_x, 248); OFF(HoldLoopArgs, hold_k, 256); OFF(HoldLoopArgs, lratio, 264); OFF(HoldLoopArgs, ltrig, 272);      // appended behind M
    static_assert(sizeof(HoldLoopArgs) == 280, "the hold block");
    static_assert(sizeof(ScpLoopArgs) == 2120 && HOLD_BLK_OFFSET == 2128 && HOLD_BLK_OFFSET + sizeof(HoldLoopArgs) <= LOOP_BLK_BYTES && LOOP_BLK_BYTES == 4096,
                  "the hold block lies where it lay, behind ScpLoopArgs, inside the handle's buffer");
    slsqp_handle *h = fake_handle(5, 4);
    EXPECT(slsqp_cl_set_solve_every(h, 3) == 0);
    const HoldLoopArgs H0 = make_hold_block(h);
    EXPECT(H0.M == 3 && H0.theta == INF && H0.a.k == 0 && H0.a.step == 0 && H0.a.S == h->log_steps);
    EXPECT(slsqp_cl_set_hold_trigger(h, 0.5) == 0);
    const HoldLoopArgs H = make_hold_block(h);
    EXPECT(H.M == 3 && H.theta == 0.5 && H.backoff_x == h->backoff_x && H.hold_k == h->hold_k && H.lratio == h->lg_ratio && H.ltrig == h->lg_trig);
    EXPECT(H.a.cl.Xn == h->Xn && H.a.cl.xmeas == h->xmeas && H.a.cl.N == 4 && H.a.cl.B == 5 && H.a.scp_success == h->scp_success);
    EXPECT(H.a.xi == h->hold_xi && H.a.u == h->hold_u && H.a.policy == h->hold_policy && H.a.lhold == h->lg_hold && H.a.lpol == h->lg_hpol);
    // theta is the only byte that differs between the two; everything before it is what a run without the trigger writes
    EXPECT(std::memcmp(&H0, &H, offsetof(HoldLoopArgs, theta)) == 0 && std::memcmp(&H0.backoff_x, &H.backoff_x, sizeof(HoldLoopArgs) - offsetof(HoldLoopArgs, backoff_x)) == 0);
    const HoldLoopArgs H2 = make_hold_block(h);
    EXPECT(std::memcmp(&H, &H2, sizeof H) == 0);      // (padding included: the block is built from zero bytes)
    // the ScpLoopArgs a launch stages does not depend on theta
    slsqp_opts o;
    slsqp_default_opts(&o);
    const ScpLoopArgs S5 = make_loop_block(h, 6, nullptr, o, false, 1);
    EXPECT(slsqp_cl_set_hold_trigger(h, INF) == 0);
    const ScpLoopArgs Sinf = make_loop_block(h, 6, nullptr, o, false, 1);
    EXPECT(std::memcmp(&S5, &Sinf, sizeof S5) == 0);
    EXPECT(launches_entered == 0);
    delete h;
}

int main() {
    check_decide();
    check_setter();
    check_layout();
    if (fails) { std::printf("cl_hold_trigger_check: %d failures\n", fails); return 1; }
    std::printf("cl_hold_trigger_check ok\n");
    return 0;
}
