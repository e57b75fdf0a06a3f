// Stand-alone host program (own main) around what plan fallback needs on the host, built by tests/test_plan_fallback_cpu.py
// with -fsanitize=address,undefined from csrc/slsqp_api.hip compiled for the host only, as tests/cl_hold_trigger_check_main.cpp is.  The handle is a
// value-initialised slsqp_handle with made-up device addresses: nothing dereferences them, no launch is entered.
//   1. cl_hold::fallback_index, plan_age_after and policy_code over hand-written sequences, valid_plan_fallback;
//   2. slsqp_cl_set_plan_fallback: 0 / 1, refusals that change nothing, the default, the option's path through cl_options;
//   3. the argument block: every field it had keeps its offset (ScpLoopArgs, HoldLoopArgs and HoldArgs keep their sizes), the PlanArgs lie behind the
//      hold block inside the handle's buffer; make_hold_block is byte-identical with the option off and points the policy at the backup with it on.
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
#define FAKE(f) do { h->f = (decltype(h->f))(next_addr); next_addr += 0x100000; } while (0)

static slsqp_handle *fake_handle(int B, int N) {
    slsqp_handle *h = new slsqp_handle();
    h->B = B; h->d.N = N; h->d.nx = 4; h->d.nu = 1; h->d.nw = 4; h->d.ni = 10; h->d.ni_f = 8; h->n = 5 * N + 4;
    h->log_steps = 6;
    FAKE(A); FAKE(Bm); FAKE(E); FAKE(K); FAKE(Kc); FAKE(Un); FAKE(Xn); FAKE(backoff_x); FAKE(scp_success); FAKE(stale); FAKE(u0); FAKE(xmeas); FAKE(x0arg);
    FAKE(hold_xi); FAKE(hold_u); FAKE(hold_policy); FAKE(hold_k); FAKE(lg_state); FAKE(lg_u0); FAKE(lg_x0v); FAKE(lg_it); FAKE(lg_hold); FAKE(lg_hpol);
    FAKE(lg_ratio); FAKE(lg_trig); FAKE(plan_bk); FAKE(plan_age); FAKE(lg_age);
    return h;
}

// ---- 1: the age rule
static void check_rule() {
    using namespace cl_hold;
    EXPECT(valid_plan_fallback(0) && valid_plan_fallback(1) && !valid_plan_fallback(2) && !valid_plan_fallback(-1) && !valid_plan_fallback(256));
    // no backup; a backup of age 0 .. N - 2 has a row left; age N - 1 has none (K has N rows)
    EXPECT(fallback_index(-1, 4) == 0 && fallback_index(0, 4) == 1 && fallback_index(1, 4) == 2 && fallback_index(2, 4) == 3 && fallback_index(3, 4) == 0 && fallback_index(9, 4) == 0);
    EXPECT(fallback_index(0, 1) == 0 && fallback_index(0, 2) == 1 && fallback_index(1, 2) == 0);
    EXPECT(plan_age_after(true, -1, 4) == 0 && plan_age_after(true, 3, 4) == 0 && plan_age_after(false, -1, 4) == -1 && plan_age_after(false, 0, 4) == 1);
    EXPECT(plan_age_after(false, 2, 4) == 3 && plan_age_after(false, 3, 4) == -1);
    EXPECT(policy_code(false, 0) == POLICY_NOMINAL && policy_code(true, 0) == POLICY_NOMINAL && policy_code(true, 2) == POLICY_HOLD && policy_code(false, 2) == POLICY_FALLBACK);
    EXPECT(POLICY_NOMINAL == 0 && POLICY_HOLD == 1 && POLICY_FALLBACK == 2);
    // N = 3, M = 1: a failure at step 0 (no backup), a success, three failures in a row (k = 1, 2, then no row left), a success, a failure
    {
        const bool ok[] = {false, true, false, false, false, true, false};
        const int want_age[] = {-1, 0, 1, 2, -1, 0, 1}, want_code[] = {0, 0, 2, 2, 0, 0, 2};
        int age = -1;
        for (int s = 0; s < 7; s++) {
            const int k = ok[s] ? 0 : fallback_index(age, 3);
            EXPECT((ok[s] ? 0 : policy_code(false, k)) == want_code[s]);
            age = plan_age_after(ok[s], age, 3);
            EXPECT(age == want_age[s]);
        }
    }
    // N = 6, M = 3: hold steps after a success count with the schedule; the solve at step 3 fails and the hold steps 4, 5 go on at k = 4, 5
    {
        const int N = 6, M = 3;
        const bool ok[] = {true, false, false, false, false, false, true, false, false};      // (read at the solves 0, 3, 6 only)
        const int want_age[] = {0, 1, 2, 3, 4, 5, 0, 1, 2}, want_code[] = {0, 1, 1, 2, 1, 1, 0, 1, 1};
        int age = -1;
        for (int s = 0; s < 9; s++) {
            const int sched = hold_index_at(s, M);
            const bool fresh = sched == 0 && ok[s];
            const int k = fresh ? 0 : fallback_index(age, N);
            EXPECT((fresh ? 0 : policy_code(sched != 0, k)) == want_code[s]);
            if (sched && age == sched - 1 && age >= 0) EXPECT(k == sched);      // after a success the age is the hold index
            age = plan_age_after(fresh, age, N);
            EXPECT(age == want_age[s]);
        }
    }
}

// ---- 2: the setter
static void check_setter() {
    slsqp_handle *h = fake_handle(5, 4);
    EXPECT(slsqp_cl_get_plan_fallback(h) == 0 && !cl_options(h).fallback && !cl_options(h).hold && cl_options(h).var == 0);      // off by default
    EXPECT(slsqp_cl_set_plan_fallback(h, 1) == 0 && slsqp_cl_get_plan_fallback(h) == 1);
    for (int bad : {2, -1, 3, 1 << 20}) {
        EXPECT(slsqp_cl_set_plan_fallback(h, bad) != 0 && std::strstr(slsqp_last_error(), "neither 0"));
        EXPECT(slsqp_cl_get_plan_fallback(h) == 1);
    }
    // no VAR bit of its own: M = 1 with the option on launches the HOLD variant, as solve_every > 1 does
    EXPECT(cl_options(h).fallback && cl_options(h).hold && cl_options(h).var == (VAR_HOLD | VAR_REF));
    EXPECT(slsqp_cl_set_solve_every(h, 3) == 0 && cl_options(h).var == (VAR_HOLD | VAR_REF));
    EXPECT(slsqp_cl_set_plan_fallback(h, 0) == 0 && slsqp_cl_get_plan_fallback(h) == 0 && cl_options(h).hold && !cl_options(h).fallback);
    EXPECT(slsqp_cl_set_solve_every(h, 1) == 0 && cl_options(h).var == 0 && !cl_options(h).hold);
    for (int bad : {2, -1}) { EXPECT(slsqp_cl_set_plan_fallback(h, bad) != 0); EXPECT(slsqp_cl_get_plan_fallback(h) == 0); }
    delete h;
}

// ---- 3: the argument block
#define OFF(T, f, at) static_assert(offsetof(T, f) == at, "a field of the argument block has moved: " #T "::" #f)
static void check_layout() {
    static_assert(sizeof(HoldArgs) == 232 && sizeof(ClArgs) == 96, "the arguments of the hold function keep their size");
    OFF(HoldArgs, cl, 0); OFF(HoldArgs, k, 96); OFF(HoldArgs, A, 104); OFF(HoldArgs, Bm, 112); OFF(HoldArgs, K, 120); OFF(HoldArgs, Kc, 128); OFF(HoldArgs, stale, 136);
    OFF(HoldArgs, scp_success, 144); OFF(HoldArgs, xi, 152); OFF(HoldArgs, u, 160); OFF(HoldArgs, policy, 168); OFF(HoldArgs, S, 176); OFF(HoldArgs, step, 180);
    OFF(HoldArgs, lstate, 184); OFF(HoldArgs, lu0, 192); OFF(HoldArgs, lx0v, 200); OFF(HoldArgs, lit, 208); OFF(HoldArgs, lhold, 216); OFF(HoldArgs, lpol, 224);
    OFF(HoldLoopArgs, a, 0); OFF(HoldLoopArgs, M, 232); OFF(HoldLoopArgs, theta, 240); OFF(HoldLoopArgs, backoff_x, 248); OFF(HoldLoopArgs, hold_k, 256);
    OFF(HoldLoopArgs, lratio, 264); OFF(HoldLoopArgs, ltrig, 272);
    static_assert(sizeof(HoldLoopArgs) == 280 && sizeof(ScpLoopArgs) == 2120 && HOLD_BLK_OFFSET == 2128 && LOOP_BLK_BYTES == 4096, "the blocks before the option keep their place and size");
    OFF(ScpLoopArgs, L, 0);
    static_assert(offsetof(ScpLoopArgs, bd) + sizeof(BndArgs) == sizeof(ScpLoopArgs), "bd stays the last field of ScpLoopArgs");
    // the new fields lie behind the last field of the hold block, inside the handle's buffer
    static_assert(PLAN_BLK_OFFSET >= HOLD_BLK_OFFSET + sizeof(HoldLoopArgs) && PLAN_BLK_OFFSET % 16 == 0 && PLAN_BLK_OFFSET + sizeof(PlanArgs) <= LOOP_BLK_BYTES, "the plan block");
    OFF(PlanArgs, on, 0);
    slsqp_handle *h = fake_handle(5, 4);
    EXPECT(slsqp_cl_set_solve_every(h, 3) == 0);
    const HoldLoopArgs H0 = make_hold_block(h);
    EXPECT(H0.a.A == h->A && H0.a.Bm == h->Bm && H0.a.Kc == h->Kc && H0.backoff_x == h->backoff_x);
    EXPECT(slsqp_cl_set_plan_fallback(h, 1) == 0 && slsqp_cl_set_plan_fallback(h, 0) == 0);
    const HoldLoopArgs H1 = make_hold_block(h);
    EXPECT(std::memcmp(&H0, &H1, sizeof H0) == 0);      // off: the bytes a run without the option writes
    EXPECT(slsqp_cl_set_plan_fallback(h, 1) == 0);
    const HoldLoopArgs H = make_hold_block(h);
    const PlanArgs f = plan_args(h);
    // the backup store: four parts with the shapes of the live arrays, in one buffer, none overlapping
    const size_t B = 5, N = 4, nx = 4, nu = 1;
    EXPECT(f.on == 1 && f.A == h->A && f.Bm == h->Bm && f.Kc == h->Kc && f.backoff_x == h->backoff_x && f.age == h->plan_age && f.lage == h->lg_age);
    EXPECT(f.bA == h->plan_bk && f.bB == f.bA + B * N * nx * nx && f.bKc == f.bB + B * N * nx * nu && f.bbo == f.bKc + B * N * nu * nx);
    EXPECT(plan_doubles(h, 0) == N * nx * nx && plan_doubles(h, 1) == N * nx * nu && plan_doubles(h, 2) == N * nu * nx && plan_doubles(h, 3) == (N + 1) * nx);
    // on: the policy and the trigger's ratio read the backup; everything else in the hold block is what it was
    EXPECT(H.a.A == f.bA && H.a.Bm == f.bB && H.a.Kc == f.bKc && H.backoff_x == f.bbo && H.a.K == h->K);
    HoldLoopArgs Hc = H;
    Hc.a.A = h->A; Hc.a.Bm = h->Bm; Hc.a.Kc = h->Kc; Hc.backoff_x = h->backoff_x;
    EXPECT(std::memcmp(&Hc, &H0, sizeof H0) == 0);
    EXPECT(plan_part_named("plan_A") == 0 && plan_part_named("plan_Bm") == 1 && plan_part_named("plan_Kc") == 2 && plan_part_named("plan_backoff_x") == 3 && plan_part_named("A") == -1);
    const ClArgs au = plant_args_on_u(h, cl_args(h, nullptr));
    EXPECT(au.N == 1 && au.Un == h->hold_u && au.xmeas == h->xmeas && au.B == 5);
    EXPECT(launches_entered == 0);
    delete h;
}

int main() {
    check_rule();
    check_setter();
    check_layout();
    if (fails) { std::printf("cl_plan_fallback_check: %d failures\n", fails); return 1; }
    std::printf("cl_plan_fallback_check ok\n");
    return 0;
}
