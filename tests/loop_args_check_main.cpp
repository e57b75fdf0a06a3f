// Stand-alone host program (own main) around the argument builders of the closed-loop kernels (csrc/slsqp_api.hip: make_qp_args, make_chain_args,
// make_loop_block, stage_loop_block -- no HIP call on the paths taken here), compiled for the host only so that it runs without a GPU and can be built
// with -fsanitize=address,undefined (tests/test_loop_args_cpu.py).  The handle is a value-initialised slsqp_handle whose device pointers are distinct
// made-up addresses: nothing dereferences them.
//   1. the two QpArgs of a chain the old way -- two independent make_qp_args calls with (warm, stat_slot, snap_use) = (w, 0, 0) and (1, 1, 1) --
//      against the new way, the common struct and qp_second_args, byte for byte, for w = 0 and w = 1 (and with ipm_restart off);
//   2. the block the host stages for a launch against the LoopArgs that went to the kernel by value before, field by field;
//   3. the description of the handle's options (cl_options) in each of the 8 states (reference, parameters, bounds on or off): the persistent
//      kernels' variant, reference and plant arguments, the batch-wide kernels' flags, and the bounds in the block against the struct they were before.
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

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)
#define SAME(a, b) EXPECT(sizeof(a) == sizeof(b) && std::memcmp(&(a), &(b), sizeof(a)) == 0)

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
    return h;
}

// what cl_run_persistent passed to k_cl_loop by value before the block: its statements, with the two QpArgs of the chain filled independently
struct OldArgs { QpArgs q1, q2; };
static OldArgs old_qp_pair(slsqp_handle *h, const slsqp_opts &o) {
    OldArgs r;
    r.q1 = make_qp_args(h, h->alive, &o, o.warm_start ? 1 : 0, nullptr, 0, 1, 0, 1);
    r.q2 = make_qp_args(h, h->alive, &o, 1, nullptr, 1, 1, 1, 1);
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

int main() {
    check_option_states();
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
            QpArgs q1 = make_qp_args(h, h->alive, &o, w, nullptr, 0, 1, 0, 1), q2 = make_qp_args(h, h->alive, &o, 1, nullptr, 1, 1, 1, 1);
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
    if (fails) return 1;
    std::printf("loop_args_check ok\n");
    return 0;
}
