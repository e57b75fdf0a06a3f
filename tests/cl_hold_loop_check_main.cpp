// Stand-alone host program (own main) around what the persistent closed loop needs on the host for solve_every > 1, built by
// tests/test_hold_loop_cpu.py with -fsanitize=address,undefined from csrc/slsqp_api.hip compiled for the host only, as tests/loop_args_check_main.cpp
// is.  The handle is a value-initialised slsqp_handle with made-up device addresses: nothing dereferences them, no launch is entered.
//   1. the solve / hold schedule (cl_hold.hpp) for every M in 1..N and run lengths that end on a solve, on a first hold and on a last hold;
//   2. cl_options in the 16 states of (reference, parameters, bounds, hold): var in {0, 1, 3, 5, 7} without hold, {9, 11, 13, 15} with it, never
//      another value; with_loop_var finds the hold sets only when asked for them; slsqp_cl_set_solve_every's range, a refusal changing nothing;
//   3. ScpLoopArgs: the size and the offset of every field as they were before the hold block, which lies behind it inside the 4096 bytes; the
//      block a launch stages does not depend on M; the hold block names the buffers slsqp_cl_hold_step passes.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

static slsqp_handle *fake_handle(int B, int N) {
    slsqp_handle *h = new slsqp_handle();
    h->B = B; h->d.N = N; h->d.nx = 4; h->d.nu = 1; h->d.nw = 4; h->d.ni = 10; h->d.ni_f = 8; h->n = 5 * N + 4;
    h->call_id = 7.0; h->log_steps = 6; h->qplog_steps = 6; h->clq_cap = 32;
    FAKE(A); FAKE(Aclc); FAKE(Bm); FAKE(E); FAKE(K); FAKE(Kc); FAKE(Linv); FAKE(Un); FAKE(Xn); FAKE(alive); FAKE(backoff); FAKE(backoff_f); FAKE(backoff_u);
    FAKE(backoff_x); FAKE(beta); FAKE(beta_f); FAKE(c); FAKE(call_ids); FAKE(chain_times); FAKE(cl_busy); FAKE(cl_stepno); FAKE(cl_tbegin); FAKE(clq_ctl);
    FAKE(clq_slots); FAKE(conv); FAKE(cost); FAKE(cost_tube); FAKE(counter); FAKE(cst); FAKE(ct_part); FAKE(dual); FAKE(eta); FAKE(eta_f); FAKE(g); FAKE(gN);
    FAKE(g_raw); FAKE(gf_raw); FAKE(has_prev); FAKE(infeas); FAKE(inst_launches); FAKE(iters); FAKE(itnum); FAKE(kkt); FAKE(lbg); FAKE(lg_bu); FAKE(lg_bx);
    FAKE(lg_it); FAKE(lg_pinf); FAKE(lg_state); FAKE(lg_succ); FAKE(lg_u); FAKE(lg_u0); FAKE(lg_x); FAKE(lin_stage); FAKE(lin_tape); FAKE(mask);
    FAKE(pending_reset); FAKE(pin_dual); FAKE(pinf); FAKE(prev_primal); FAKE(primal); FAKE(q); FAKE(qp_diag); FAKE(qplog); FAKE(qplog_nsolves); FAKE(qpstat);
    FAKE(qpstate); FAKE(scp_active); FAKE(scp_dmax); FAKE(scp_iters); FAKE(scp_success); FAKE(scp_upd); FAKE(stale); FAKE(status); FAKE(success); FAKE(u0);
    FAKE(u_init); FAKE(ubg); FAKE(ws); FAKE(x0arg); FAKE(x0val); FAKE(x0vlog); FAKE(xmeas); FAKE(zero_ref);
    FAKE(hold_xi); FAKE(hold_u); FAKE(hold_policy); FAKE(lg_x0v); FAKE(lg_hold); FAKE(lg_hpol);
    return h;
}

// ---- 1: the schedule
static void check_schedule() {
    for (int N = 1; N <= 6; N++)
        for (int M = 1; M <= N; M++) {
            EXPECT(cl_hold::valid_solve_every(M, N));
            // run lengths: one that ends on a solve (last step qM), on a first hold (qM + 1) and on a last hold (qM + M - 1), and every one up to 3 M
            std::vector<int> lens = {1, M + 1, 2 * M + 1, M + 2, 2 * M, 3 * M};
            for (int s = 1; s <= 3 * M; s++) lens.push_back(s);
            for (int steps : lens) {
                int solves = 0, since = 0;
                for (int s = 0; s < steps; s++) {
                    const int k = cl_hold::hold_index_at(s, M);
                    EXPECT(cl_hold::is_solve(s, M) == (k == 0));
                    if (s == 0) EXPECT(k == 0);      // a run begins with a solve
                    if (k == 0) { solves++; since = 0; } else { since++; EXPECT(k == since); }      // hold steps count up from their solve
                    EXPECT(k >= 0 && k <= M - 1 && k <= N - 1);      // K has N rows
                }
                EXPECT(solves == cl_hold::solves_in(steps, M));
                EXPECT(cl_hold::hold_index_at(steps - 1, M) == since);      // what "hold_index" serves after the run
            }
            if (M > 1) {
                EXPECT(cl_hold::hold_index_at(2 * M, M) == 0 && cl_hold::hold_index_at(2 * M + 1, M) == 1 && cl_hold::hold_index_at(3 * M - 1, M) == M - 1);
                EXPECT(cl_hold::solves_in(2 * M + 1, M) == 3 && cl_hold::solves_in(2 * M, M) == 2 && cl_hold::solves_in(M + 1, M) == 2);
            } else EXPECT(cl_hold::solves_in(5, 1) == 5 && cl_hold::hold_index_at(4, 1) == 0);
        }
    EXPECT(!cl_hold::valid_solve_every(0, 4) && !cl_hold::valid_solve_every(5, 4) && !cl_hold::valid_solve_every(-1, 4));
    EXPECT(cl_hold::solves_in(0, 3) == 0);
    // the hold state a run leaves: the index of its last step, and still no per-batch plan
    cl_hold::State s;
    cl_hold::on_init(s);
    cl_hold::on_run(s, 5, cl_hold::hold_index_at(4, 3));
    std::string why;
    EXPECT(cl_hold::index(s, 5) == 1 && cl_hold::next_index(s, true, 5, 4, 0, &why) == 0 && why.find("slsqp_cl_run") != std::string::npos);
    EXPECT(cl_hold::index(s, 6) == 0 && cl_hold::next_index(s, true, 6, 4, 0, &why) == 1);      // after a slsqp_cl_step
    cl_hold::on_init(s);
    cl_hold::on_run(s, 4, cl_hold::hold_index_at(3, 2));
    EXPECT(cl_hold::index(s, 4) == 1);
    cl_hold::on_init(s);
    cl_hold::on_run(s, 4);      // M = 1
    EXPECT(cl_hold::index(s, 4) == 0 && s.at_steps == -1);
}

// ---- 2: the option states
static void check_option_states() {
    static const int base[8] = {/* 000 */ 0, /* 001 */ 5, /* 010 */ 3, /* 011 */ 7, /* 100 */ 1, /* 101 */ 5, /* 110 */ 3, /* 111 */ 7};
    static const int held[8] = {9, 13, 11, 15, 9, 13, 11, 15};
    for (int st = 0; st < 16; st++) {
        const bool hold = st & 8, ref = st & 4, pp = st & 2, bnd = st & 1;
        slsqp_handle *h = fake_handle(5, 3);
        if (ref) { FAKE(ref_Y); h->ref_T = 2; h->ref_stride = 2 * 5; }
        if (pp) { FAKE(pp_P); FAKE(pp_merr); FAKE(lg_merr); h->pp_np = 3; h->pp_stride = 3; }
        if (bnd) { FAKE(bnd_rows); h->bnd_T = 2; h->bnd_stride = 2 * 18; }
        EXPECT(slsqp_cl_get_solve_every(h) == 1);
        if (hold) EXPECT(slsqp_cl_set_solve_every(h, 2 + (st & 1)) == 0 && slsqp_cl_get_solve_every(h) == 2 + (st & 1));
        const ClOptions op = cl_options(h);
        const int want = hold ? held[st & 7] : base[st & 7];
        EXPECT(op.ref == ref && op.pp == pp && op.bnd == bnd && op.hold == hold && op.var == want);
        EXPECT(var_hold(op.var) == hold && var_pp(op.var) == pp && var_bnd(op.var) == bnd && var_ref(op.var) == (st != 0));
        bool listed = false;
        for (int v : {0, 1, 3, 5, 7}) listed = listed || (!hold && op.var == v);
        for (int v : {9, 11, 13, 15}) listed = listed || (hold && op.var == v);
        EXPECT(listed);
        if (ref) EXPECT(op.rf.rows == h->ref_Y && op.rf.T == 2 && op.rf.stride == 10);
        else if (st) EXPECT(op.rf.rows == h->zero_ref && op.rf.T == 1 && op.rf.stride == 0);      // HOLD comes with REF: the zero row
        else EXPECT(op.rf.rows == nullptr && op.rf.T == 0 && op.rf.stride == 0);
        if (pp) EXPECT(op.pa.P == h->pp_P); else EXPECT(op.pa.P == nullptr && op.pa.model_err == nullptr);
        // k_cl_loop's dispatch finds every state; k_cl_loop_scp's only the ones without hold
        int seen = -1, calls = 0;
        EXPECT(with_loop_var(op.var, [&](auto V) { seen = V(); calls++; }, true) && seen == want && calls == 1);
        seen = -1; calls = 0;
        EXPECT(with_loop_var(op.var, [&](auto V) { seen = V(); calls++; }) == !hold && calls == (hold ? 0 : 1) && (hold || seen == want));
        // the range of M: a refusal says so and changes nothing
        const int before = slsqp_cl_get_solve_every(h);
        EXPECT(slsqp_cl_set_solve_every(h, 0) != 0 && std::strstr(slsqp_last_error(), "outside 1 .. N") && slsqp_cl_get_solve_every(h) == before);
        EXPECT(slsqp_cl_set_solve_every(h, h->d.N + 1) != 0 && slsqp_cl_set_solve_every(h, -3) != 0 && slsqp_cl_get_solve_every(h) == before);
        EXPECT(slsqp_cl_set_solve_every(h, h->d.N) == 0 && slsqp_cl_get_solve_every(h) == h->d.N);
        EXPECT(slsqp_cl_set_solve_every(h, 1) == 0 && cl_options(h).var == base[st & 7] && !cl_options(h).hold);
        delete h;
    }
    for (int v : {-1, 2, 4, 6, 8, 10, 12, 14, 16, 17}) EXPECT(!with_loop_var(v, [&](auto) { fails++; }, true) && !with_loop_var(v, [&](auto) { fails++; }));
}

// ---- 3: the layouts
#define OFF(T, f, at) static_assert(offsetof(T, f) == at, "a field of the persistent kernels' argument block has moved: " #T "::" #f)
static void check_layout() {
    static_assert(sizeof(ScpLoopArgs) == 2120 && sizeof(LoopArgs) == 2056, "the persistent kernels' argument block keeps its size");
    OFF(ScpLoopArgs, L, 0); OFF(ScpLoopArgs, max_it, 2056); OFF(ScpLoopArgs, converge, 2060); OFF(ScpLoopArgs, rti_steps, 2064); OFF(ScpLoopArgs, nsolves, 2072);
    OFF(ScpLoopArgs, bd, 2080);
    OFF(LoopArgs, c, 0); OFF(LoopArgs, cl, 1112); OFF(LoopArgs, lin, 1208); OFF(LoopArgs, ba, 1376); OFF(LoopArgs, sb, 1456); OFF(LoopArgs, lg, 1664);
    OFF(LoopArgs, sa, 1832); OFF(LoopArgs, steps, 1896); OFF(LoopArgs, n, 1900); OFF(LoopArgs, have_log, 1904); OFF(LoopArgs, fence, 1908);
    OFF(LoopArgs, keep_laggards, 1912); OFF(LoopArgs, stepno, 1920); OFF(LoopArgs, call_ids, 1928); OFF(LoopArgs, q, 1936); OFF(LoopArgs, stale, 1944);
    OFF(LoopArgs, itnum, 1952); OFF(LoopArgs, pending, 1960); OFF(LoopArgs, scp_active, 1968); OFF(LoopArgs, W_all, 1976); OFF(LoopArgs, pinf, 1984);
    OFF(LoopArgs, Q, 1992); OFF(LoopArgs, busy, 2040); OFF(LoopArgs, t_begin, 2048);
    static_assert(sizeof(ChainArgs) == 1112 && sizeof(ClArgs) == 96 && sizeof(LinArgs) == 168 && sizeof(BoundsArgs) == 80 && sizeof(SolveBeginArgs) == 208 &&
                  sizeof(ClLogArgs) == 168 && sizeof(ScpArgs) == 64 && sizeof(ClQueue) == 48 && sizeof(BndArgs) == 40, "the parts of the block keep their sizes");
    static_assert(HOLD_BLK_OFFSET >= sizeof(ScpLoopArgs) && HOLD_BLK_OFFSET % 16 == 0 && HOLD_BLK_OFFSET + sizeof(HoldLoopArgs) <= LOOP_BLK_BYTES, "the hold block lies behind bd, inside the handle's buffer");
    slsqp_opts o;
    slsqp_default_opts(&o);
    slsqp_handle *h = fake_handle(5, 4);
    const ScpLoopArgs S1 = make_loop_block(h, 6, nullptr, o, false, 1);
    EXPECT(slsqp_cl_set_solve_every(h, 3) == 0);
    const ScpLoopArgs S3 = make_loop_block(h, 6, nullptr, o, false, 1);
    EXPECT(std::memcmp(&S1, &S3, sizeof S1) == 0);      // M is not in it: a run with M = 1 writes the bytes it always did
    stage_loop_block(h, S3);
    EXPECT(h->loop_blk_host.size() == sizeof(ScpLoopArgs) && h->hold_blk_host.empty());
    const HoldLoopArgs H = make_hold_block(h);
    EXPECT(H.M == 3 && H.a.k == 0 && H.a.step == 0 && H.a.S == h->log_steps);
    EXPECT(H.a.cl.Xn == h->Xn && H.a.cl.Un == h->Un && H.a.cl.xmeas == h->xmeas && H.a.cl.N == 4 && H.a.cl.B == 5 && H.a.cl.w == nullptr);
    EXPECT(H.a.A == h->A && H.a.Bm == h->Bm && H.a.K == h->K && H.a.Kc == h->Kc && H.a.stale == h->stale && H.a.scp_success == h->scp_success);
    EXPECT(H.a.xi == h->hold_xi && H.a.u == h->hold_u && H.a.policy == h->hold_policy);
    EXPECT(H.a.lstate == h->lg_state && H.a.lu0 == h->lg_u0 && H.a.lx0v == h->lg_x0v && H.a.lit == h->lg_it && H.a.lhold == h->lg_hold && H.a.lpol == h->lg_hpol);
    const HoldLoopArgs H2 = make_hold_block(h);
    EXPECT(std::memcmp(&H, &H2, sizeof H) == 0);      // (padding included: the block is built from zero bytes)
    EXPECT(launches_entered == 0);
    delete h;
}

int main() {
    check_schedule();
    check_option_states();
    check_layout();
    if (fails) { std::printf("cl_hold_loop_check: %d failures\n", fails); return 1; }
    std::printf("cl_hold_loop_check ok\n");
    return 0;
}
