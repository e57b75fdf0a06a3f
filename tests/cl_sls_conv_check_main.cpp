// Stand-alone host program (own main) around what fast-SLS converge mode inside the persistent closed loop needs on the host,
// built by tests/test_sls_converge_cpu.py with -fsanitize=address,undefined from csrc/slsqp_api.hip compiled for the host only, as
// tests/cl_hold_loop_check_main.cpp is.  The handle is a value-initialised slsqp_handle with made-up device addresses: nothing dereferences them, no
// launch is entered.
//   1. the "took no part" rule of csrc/cl_sls_conv.hpp against a brute-force model of the batch-wide launches of solve_impl's converge mode, on every
//      table of iteration counts for caps 1..4 and batches of 1..4 instances, with instances that take no part in the solve at all;
//   2. slsqp_cl_set_sls_converge's range, a refusal changing nothing; what slsqp_cl_run_scp answers to rti_steps with the option off and on;
//   3. cl_options in the 16 states of (reference, parameters, bounds, hold) with the option on: the var values of the option off;
//   4. ScpLoopArgs with its size, the hold and plan blocks where they were, the new block behind them inside the 4096 bytes; the block a launch stages
//      with the option on and a fixed number of fast-SLS steps is byte for byte the one with the option off.
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
    h->call_id = 7.0; h->log_steps = 6; h->qplog_steps = 6; h->qplog_cap = 8; h->clq_cap = 32;
    FAKE(A); FAKE(Aclc); FAKE(Bm); FAKE(E); FAKE(K); FAKE(Kc); FAKE(Linv); FAKE(Un); FAKE(Xn); FAKE(alive); FAKE(backoff); FAKE(backoff_f); FAKE(backoff_u);
    FAKE(backoff_x); FAKE(beta); FAKE(beta_f); FAKE(c); FAKE(call_ids); FAKE(chain_times); FAKE(cl_busy); FAKE(cl_stepno); FAKE(cl_tbegin); FAKE(clq_ctl);
    FAKE(clq_slots); FAKE(conv); FAKE(cost); FAKE(cost_tube); FAKE(counter); FAKE(cst); FAKE(ct_part); FAKE(dual); FAKE(eta); FAKE(eta_f); FAKE(g); FAKE(gN);
    FAKE(g_raw); FAKE(gf_raw); FAKE(has_prev); FAKE(infeas); FAKE(inst_launches); FAKE(iters); FAKE(itnum); FAKE(kkt); FAKE(lbg); FAKE(lg_bu); FAKE(lg_bx);
    FAKE(lg_it); FAKE(lg_pinf); FAKE(lg_state); FAKE(lg_succ); FAKE(lg_u); FAKE(lg_u0); FAKE(lg_x); FAKE(lin_stage); FAKE(lin_tape); FAKE(mask);
    FAKE(pending_reset); FAKE(pin_dual); FAKE(pinf); FAKE(prev_primal); FAKE(primal); FAKE(q); FAKE(qp_diag); FAKE(qplog); FAKE(qplog_nsolves); FAKE(qpstat);
    FAKE(qpstate); FAKE(scp_active); FAKE(scp_dmax); FAKE(scp_iters); FAKE(scp_success); FAKE(scp_upd); FAKE(stale); FAKE(status); FAKE(success); FAKE(u0);
    FAKE(u_init); FAKE(ubg); FAKE(ws); FAKE(x0arg); FAKE(x0val); FAKE(x0vlog); FAKE(xmeas); FAKE(zero_ref);
    FAKE(hold_xi); FAKE(hold_u); FAKE(hold_policy); FAKE(lg_x0v); FAKE(lg_hold); FAKE(lg_hpol); FAKE(sls_itlog);
    return h;
}

// ---- 1: the rule against the launches
// What solve_impl's converge-mode loop leaves in slot 0 of every instance.  n[b]: the sweeps instance b runs (it goes on to a sweep after the loop QPs
// 0 .. n[b] - 1 and leaves at QP n[b], or hits the cap with n[b] = cap); in[b] = false: it takes no part in the solve (not `active`).  Returns per
// instance the index of the loop QP whose statistics its slot 0 holds, or -1: "took no part".
static std::vector<int> launches(const std::vector<int> &n, const std::vector<bool> &in, int cap) {
    const int B = (int)n.size();
    std::vector<int> slot0(B, -2), alive(B);
    for (int b = 0; b < B; b++) alive[b] = in[b] ? 1 : 0;
    for (int i = 0; i < cap; i++) {
        for (int b = 0; b < B; b++) slot0[b] = alive[b] ? i : -1;      // launch_qp(h, h->alive, ...): slot 0 of everybody
        int nmask = 0;
        for (int b = 0; b < B; b++) {      // k_after_qp: converged or failed -> alive = 0, else mask = 1
            if (!alive[b]) continue;
            if (i < n[b]) nmask++; else alive[b] = 0;
        }
        if (nmask == 0) break;      // every instance converged or failed
    }
    return slot0;
}
static void check_rule() {
    long tables = 0;
    for (int cap = 1; cap <= 4; cap++)
        for (int B = 1; B <= 4; B++) {
            std::vector<int> n(B, 0);
            for (;;) {
                for (int out = 0; out < (1 << B); out++) {      // the instances that take no part in the solve
                    std::vector<bool> in(B);
                    std::vector<int> nn = n;
                    for (int b = 0; b < B; b++) { in[b] = !((out >> b) & 1); if (!in[b]) nn[b] = 0; }      // (inside the launch such an instance counts 0 sweeps)
                    const std::vector<int> slot0 = launches(nn, in, cap);
                    int nmax = 0;
                    for (int b = 0; b < B; b++) nmax = nn[b] > nmax ? nn[b] : nmax;
                    for (int b = 0; b < B; b++) {
                        const bool rule = cl_sls_conv::slot0_took_no_part(nn[b], nmax, cap);
                        // inside the launch the instance's own last loop QP wrote the slot: QP n (n - 1 at the cap), or "took no part" where it is not in the solve
                        const int own = !in[b] ? -1 : (nn[b] < cap ? nn[b] : cap - 1);
                        const int after = rule ? -1 : own;
                        if (after != slot0[b]) { std::printf("cap %d B %d instance %d: n %d nmax %d in %d -> launches %d, rule %d\n", cap, B, b, nn[b], nmax, (int)in[b], slot0[b], after); fails++; }
                    }
                    tables++;
                }
                int b = 0;
                while (b < B && n[b] == cap) n[b++] = 0;
                if (b == B) break;
                n[b]++;
            }
        }
    EXPECT(tables > 5000);
    EXPECT(cl_sls_conv::last_loop_qp(0, 30) == 0 && cl_sls_conv::last_loop_qp(4, 30) == 4 && cl_sls_conv::last_loop_qp(30, 30) == 29 && cl_sls_conv::last_loop_qp(29, 30) == 29);
    EXPECT(!cl_sls_conv::slot0_took_no_part(3, 3, 30) && cl_sls_conv::slot0_took_no_part(1, 3, 30) && !cl_sls_conv::slot0_took_no_part(30, 30, 30) && !cl_sls_conv::slot0_took_no_part(29, 30, 30));
    EXPECT(cl_sls_conv::slot0_took_no_part(28, 30, 30) && !cl_sls_conv::slot0_took_no_part(0, 0, 1) && !cl_sls_conv::slot0_took_no_part(0, 1, 1));
}

// ---- 2: the option and the refusals that depend on it
static void check_option() {
    slsqp_handle *h = fake_handle(5, 3);
    EXPECT(slsqp_cl_get_sls_converge(h) == 0);      // off by default
    EXPECT(slsqp_cl_set_sls_converge(h, 2) != 0 && std::strstr(slsqp_last_error(), "neither 0 (off) nor 1 (on)") && slsqp_cl_get_sls_converge(h) == 0);
    EXPECT(slsqp_cl_set_sls_converge(h, -1) != 0 && slsqp_cl_get_sls_converge(h) == 0);
    EXPECT(slsqp_cl_set_sls_converge(h, 1) == 0 && slsqp_cl_get_sls_converge(h) == 1);
    EXPECT(slsqp_cl_set_sls_converge(h, 2) != 0 && slsqp_cl_set_sls_converge(h, -1) != 0 && slsqp_cl_get_sls_converge(h) == 1);      // a refusal changes nothing
    EXPECT(slsqp_cl_set_sls_converge(h, 0) == 0 && slsqp_cl_get_sls_converge(h) == 0);
    EXPECT(cl_sls_conv::valid_option(0) && cl_sls_conv::valid_option(1) && !cl_sls_conv::valid_option(2) && !cl_sls_conv::valid_option(-1));
    delete h;
    // off: today's words for rti_steps <= 0; on: it runs with a cap >= 1; a fixed number of steps is nobody's business here
    const char *off = cl_sls_conv::run_scp_refusal(0, 0, 30);
    EXPECT(off && std::strstr(off, "fast-SLS converge mode (rti_steps <= 0) does not run inside the persistent loop (use slsqp_cl_step)"));
    EXPECT(cl_sls_conv::run_scp_refusal(-3, 0, 30) == off);
    EXPECT(cl_sls_conv::run_scp_refusal(0, 1, 30) == nullptr && cl_sls_conv::run_scp_refusal(-1, 1, 1) == nullptr);
    const char *cap = cl_sls_conv::run_scp_refusal(0, 1, 0);
    EXPECT(cap && std::strstr(cap, "max_sls_iter >= 1") && cl_sls_conv::run_scp_refusal(0, 1, -2) == cap);
    for (int on = 0; on <= 1; on++) for (int k : {1, 2, 7}) for (int mi : {-1, 0, 30}) EXPECT(cl_sls_conv::run_scp_refusal(k, on, mi) == nullptr);
}

// ---- 3: the option states with the option on
static void check_option_states() {
    static const int base[8] = {/* 000 */ 0, /* 001 */ 5, /* 010 */ 3, /* 011 */ 7, /* 100 */ 1, /* 101 */ 5, /* 110 */ 3, /* 111 */ 7};
    static const int held[8] = {9, 13, 11, 15, 9, 13, 11, 15};
    for (int st = 0; st < 16; st++) {
        const bool hold = st & 8, ref = st & 4, pp = st & 2, bnd = st & 1;
        slsqp_handle *h = fake_handle(5, 3);
        if (ref) { FAKE(ref_Y); h->ref_T = 2; h->ref_stride = 2 * 5; }
        if (pp) { FAKE(pp_P); FAKE(pp_merr); FAKE(lg_merr); h->pp_np = 3; h->pp_stride = 3; }
        if (bnd) { FAKE(bnd_rows); h->bnd_T = 2; h->bnd_stride = 2 * 18; }
        if (hold) EXPECT(slsqp_cl_set_solve_every(h, 2) == 0);
        const ClOptions off = cl_options(h);
        EXPECT(slsqp_cl_set_sls_converge(h, 1) == 0);
        const ClOptions on = cl_options(h);
        const int want = hold ? held[st & 7] : base[st & 7];
        EXPECT(on.var == want && off.var == want);
        EXPECT(on.ref == off.ref && on.pp == off.pp && on.bnd == off.bnd && on.hold == off.hold && on.fallback == off.fallback);
        EXPECT(on.rf.rows == off.rf.rows && on.rf.T == off.rf.T && on.rf.stride == off.rf.stride && on.pa.P == off.pa.P);
        bool listed = false;
        for (int v : {0, 1, 3, 5, 7}) listed = listed || (!hold && on.var == v);
        for (int v : {9, 11, 13, 15}) listed = listed || (hold && on.var == v);
        EXPECT(listed);
        int seen = -1, calls = 0;      // k_cl_loop_scp's dispatch, the one the CONV variants go through: the five sets without hold
        EXPECT(with_loop_var(on.var, [&](auto V) { seen = V(); calls++; }) == !hold && calls == (hold ? 0 : 1) && (hold || seen == want));
        delete h;
    }
}

// ---- 4: the layouts and the staged blocks
static void check_layout() {
    static_assert(sizeof(ScpLoopArgs) == 2120 && sizeof(LoopArgs) == 2056, "the persistent kernels' argument block keeps its size");
    static_assert(offsetof(ScpLoopArgs, max_it) == 2056 && offsetof(ScpLoopArgs, converge) == 2060 && offsetof(ScpLoopArgs, rti_steps) == 2064 &&
                  offsetof(ScpLoopArgs, nsolves) == 2072 && offsetof(ScpLoopArgs, bd) == 2080, "a field of the persistent kernels' argument block has moved");
    static_assert(HOLD_BLK_OFFSET == 2128, "the hold block stays where it was");
    static_assert(PLAN_BLK_OFFSET == ((HOLD_BLK_OFFSET + sizeof(HoldLoopArgs) + 15) & ~(size_t)15), "the plan block stays where it was");
    static_assert(CONV_BLK_OFFSET >= PLAN_BLK_OFFSET + sizeof(PlanArgs) && CONV_BLK_OFFSET % 16 == 0 && CONV_BLK_OFFSET + sizeof(SlsConvArgs) <= LOOP_BLK_BYTES,
                  "the new block lies behind the plan block, inside the handle's buffer");
    slsqp_opts o;
    slsqp_default_opts(&o);
    o.rti_steps = 2;
    slsqp_handle *h = fake_handle(5, 4);
    const ScpLoopArgs off = make_loop_block(h, 6, nullptr, o, true, 3);
    EXPECT(slsqp_cl_set_sls_converge(h, 1) == 0);
    const ScpLoopArgs on = make_loop_block(h, 6, nullptr, o, true, 3);
    EXPECT(std::memcmp(&off, &on, sizeof off) == 0);      // the option is not in it: a run with rti_steps >= 1 writes the bytes it always did
    EXPECT(off.rti_steps == 2 && off.max_it == 3 && off.converge == 0);
    stage_loop_block(h, on);
    EXPECT(h->loop_blk_host.size() == sizeof(ScpLoopArgs) && h->conv_blk_host.empty() && h->hold_blk_host.empty());
    // converge mode: the cap travels in rti_steps, and nothing else differs
    o.rti_steps = 0; o.max_sls_iter = 9;
    const ScpLoopArgs cv = make_loop_block(h, 6, nullptr, o, true, 3, true);
    EXPECT(cv.rti_steps == 9 && cv.max_it == 3 && cv.converge == 0);
    ScpLoopArgs same = cv;
    same.rti_steps = 2;
    EXPECT(std::memcmp(&same, &off, sizeof off) == 0);
    const ScpLoopArgs cs = make_loop_block(h, 6, nullptr, o, true, -1, true);      // both loops data-dependent
    EXPECT(cs.rti_steps == 9 && cs.converge == 1 && cs.max_it == o.max_scp_iter);
    const SlsConvArgs V = make_conv_block(h);
    EXPECT(V.itlog == h->sls_itlog && V.lastit == h->sls_itlog + (size_t)h->B * h->qplog_cap && V.log_steps == h->qplog_steps);
    const SlsConvArgs V2 = make_conv_block(h);
    EXPECT(std::memcmp(&V, &V2, sizeof V) == 0);      // (padding included: the block is built from zero bytes)
    EXPECT(launches_entered == 0);
    delete h;
}

int main() {
    check_rule();
    check_option();
    check_option_states();
    check_layout();
    if (fails) { std::printf("cl_sls_conv_check: %d failures\n", fails); return 1; }
    std::printf("cl_sls_conv_check ok\n");
    return 0;
}
