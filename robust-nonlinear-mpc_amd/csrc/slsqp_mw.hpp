// slsqp_mw.hpp -- the multi-wave QP path for small batches: ONE workgroup of W = 2, 4 or 8 waves per MPC instance.
//
// The single-wave kernels solve the block-tridiagonal normal equations  Y nu = b  by a block LDL' recursion whose N stages depend on each other
// (ne_forward / ne_backward); with one instance on the device that is one wave on one SIMD.  ne_solve_cr below solves the same system by block
// cyclic reduction: the blocks at the odd positions of the remaining list are eliminated at once, each by one wave, so the dependent chain is
// ceil(log2 N) levels deep.  k_qp_solve_mw runs the tick loop of qp_solve_dev around it; the phase logic (phase_update) is the single-wave
// code, unchanged, on wave 0.
//
// Hand-over between the waves -- through the LDS and through the global scratch alike -- is by __syncthreads() only: every wave reaches every
// barrier (a wave without a block at some level just arrives), all loop bounds are workgroup-uniform.  No flags, no spinning, no atomics.
// For the global scratch that rests on two things: __syncthreads() carries a workgroup-scope release / acquire fence around s_barrier, and the waves of a
// workgroup sit on one CU and share its vector L1, so a block stored by one wave before the barrier is what another loads behind it.  It would not
// hold with the workgroup split over CUs (threadgroup-split mode, tgsplit): the library is never built or run that way.
#pragma once
#include "slsqp_kernels.hpp"

namespace slsqp {

constexpr int MW_MAX_WAVES = 8;

// LDS of the workgroup: a shared head (cross-wave reductions; the vector b -> y -> nu of the whole horizon) and one work area per wave: five
// NX x NX buffers, B_k and the stage vectors of the QpLds layout.
template <int NX, int NU>
struct MwLds {
    static constexpr int NZ = NX + NU, MM = NX * NX;
    static constexpr int oM0 = 0, oM1 = MM, oM2 = 2 * MM, oM3 = 3 * MM, oM4 = 4 * MM, oB = 5 * MM, oPiS = oB + NX * NU, oVS = oPiS + NZ + NX, oT1 = oVS + NZ + NX,
                         WAVE = (oT1 + NX + 2) & ~1;
    static constexpr int oRed = 0, oNu = 2 * MW_MAX_WAVES;
    __host__ __device__ static constexpr int head(int N) { return (oNu + N * NX + 1) & ~1; }
    __host__ __device__ static constexpr int total(int N, int W) { return head(N) + W * WAVE; }
};
// per instance: N x 3 blocks of NX x NX doubles.  Block i before its elimination: [0] D_i (lower triangle), [1] its coupling Y_{i,l} to the left
// neighbour l in the current list; afterwards [0] D_i^-1 (full), [1] F_l = D_i^-1 Y_{i,l}, [2] F_r = D_i^-1 Y_{i,r}.
template <int NX>
__host__ __device__ constexpr size_t mw_scratch_doubles(int N) { return (size_t)N * 3 * NX * NX; }

namespace mw {
template <int MM>
__device__ __forceinline__ void ld_blk(double *s, const double *g, int lane) {
#pragma unroll
    for (int o = lane; o < MM; o += 64) s[o] = g[o];
}
template <int MM>
__device__ __forceinline__ void st_blk(double *g, const double *s, int lane) {
#pragma unroll
    for (int o = lane; o < MM; o += 64) g[o] = s[o];
}
// C (NX x NX) = op(A) op(B)
template <int NX, bool TA, bool TB>
__device__ __forceinline__ void mm(const double *A, const double *B, double *C, int lane) {
    if constexpr (QpLds<NX, 1>::MFMA) wla::gemm_mfma<NX, NX, NX, TA, TB>(A, NX, B, NX, C, NX, lane);
    else wla::gemm_blk<NX, NX, NX, TA, TB, 2, 2, false>(A, NX, B, NX, C, NX, 1.0, lane);
    wla::wsync();
}
// lower triangle of the global block g -= T (LDS)
template <int NX>
__device__ __forceinline__ void sub_lower(double *g, const double *T, int lane) {
#pragma unroll
    for (int o = lane; o < NX * NX; o += 64)
        if (o % NX <= o / NX) g[o] -= T[o];
}
}  // namespace mw

// Block cyclic reduction of  Y nu = b  by the W waves of the workgroup (same operands as ne_forward + ne_backward; UF and Linv are not touched).
//   Y_kk = A_k diag(pi_x,k) A_k' [k > 0] + B_k diag(pi_u,k) B_k' + diag(pi_x,k+1) + delta,   Y_{k,k-1} = -A_k diag(pi_x,k),
//   b_k = A_k v_x,k + B_k v_u,k - v_x,k+1 - eflag e_k.
// Level s = 1, 2, 4, ..: the list holds the blocks 0, s, 2s, ..; those at its odd positions, i = (2m+1) s, are eliminated (neighbours l = i - s and,
// if it exists, r = i + s):
//   D_i^-1;  F_l = D_i^-1 Y_{i,l};  F_r = D_i^-1 Y_{i,r};  y_i = D_i^-1 b_i;
//   D_l -= Y_{i,l}' F_l,  b_l -= F_l' b_i;       D_r -= Y_{r,i} F_r,  b_r -= F_r' b_i,  Y_{r,l} = -Y_{r,i} F_l.
// Block 0 is the root.  Back-substitution down the levels: nu_i = y_i - F_l nu_l - F_r nu_r.  Then W = nu and G = E' nu, stage by stage.
// factor = false: substitution only, from the D_i^-1, F_l, F_r a factorising call left in the scratch.
// res_tol >= 0 (residual-only ticks): the routine stops after the right-hand side when max|b| < res_tol and returns 2; W and G keep their values.
// Returns (workgroup-uniform) bit 0: a block was not positive definite, bit 1: stopped after the right-hand side.  *bmax_out = max|b|.
template <int NX, int NU>
__device__ __forceinline__ int ne_solve_cr(double *sm, const NeG<NX, NU> g, double *cr, bool factor, double eflag, double delta, int lane, int wave, int W,
                                           double *bmax_out, double res_tol = -1.0) {
    using Ld = MwLds<NX, NU>;
    constexpr int NZ = NX + NU, SR = NX + 2 * NZ, MM = NX * NX;
    constexpr bool MFMA = QpLds<NX, NU>::MFMA;
    const int N = g.N;
    double *sRed = sm + Ld::oRed, *sNu = sm + Ld::oNu;
    double *sw = sm + Ld::head(N) + wave * Ld::WAVE;
    double *m0 = sw + Ld::oM0, *m1 = sw + Ld::oM1, *m2 = sw + Ld::oM2, *m3 = sw + Ld::oM3, *m4 = sw + Ld::oM4;
    double *sB = sw + Ld::oB, *sPiS = sw + Ld::oPiS, *sVS = sw + Ld::oVS, *sT1 = sw + Ld::oT1;
    auto blk = [&](int i, int slot) -> double * { return cr + ((size_t)i * 3 + slot) * MM; };
    int fail = 0;
    double bmax = 0.0;

    // ---- right-hand side, diagonal blocks and couplings: stage k on wave k mod W
    if (factor && MFMA) {       // (the matrix-core build of Y_kk always subtracts a T M1' term: T = 0 here)
        for (int o = lane; o < MM; o += 64) m3[o] = 0.0;
    }
    for (int k = wave; k < N; k += W) {
        mw::ld_blk<MM>(m1, g.A + (size_t)k * MM, lane);
        mw::ld_blk<NX * NU>(sB, g.Bm + (size_t)k * NX * NU, lane);
        if (lane < NZ + NX) { sPiS[lane] = g.PI[k * NZ + lane]; sVS[lane] = g.V[k * NZ + lane]; }
        const int lx = min(lane, NX - 1);
        const double ek = (eflag != 0.0) ? 0.5 * (g.ub[k * SR + lx] + g.lb[k * SR + lx]) : 0.0;
        wla::wsync();
        double b = wla::matvec_split3<NX, NX, false>(m1, NX, sVS, lane) + wla::matvec_split3<NX, NU, false>(sB, NU, sVS + NX, lane);
        if (lane < NX) { b += -sVS[NZ + lane] - eflag * ek; sNu[k * NX + lane] = b; } else b = 0.0;
        bmax = fmax(bmax, fabs(b));
        if (factor) {
            // M1 = A diag(pi_x,k) (0 at stage 0: x_0 is pinned); the coupling is -M1
#pragma unroll
            for (int o = lane; o < MM; o += 64) m2[o] = (k > 0) ? m1[o] * sPiS[o % NX] : 0.0;
            wla::wsync();
            if constexpr (MFMA) wla::build_Y_mfma<NX, NU>(m1, sPiS, sB, sPiS + NX, m3, k > 0, sPiS + NZ, delta, m0, lane);
            else wla::build_Y_lower<NX, NU>(m2, m1, sB, sPiS + NX, m3, false, sPiS + NZ, delta, m0, lane);
            wla::wsync();
            double *gD = blk(k, 0), *gC = blk(k, 1);
#pragma unroll
            for (int o = lane; o < MM; o += 64) {
                if (o % NX <= o / NX) gD[o] = m0[o];
                gC[o] = -m2[o];
            }
        }
        wla::wsync();
    }
    bmax = wla::wave_max(bmax);
    if (lane == 0) sRed[wave] = bmax;
    __syncthreads();
    bmax = 0.0;
    for (int w = 0; w < W; w++) bmax = fmax(bmax, sRed[w]);
    if (bmax_out) *bmax_out = bmax;
    if (res_tol >= 0.0 && bmax < res_tol) return 2;

    // ---- reduction
    int s = 1;
    for (; s < N; s *= 2) {
        const int cnt = (N + s - 1) / s, ne = cnt / 2;      // blocks in the list, eliminations of this level
        for (int m_ = 0; m_ < ne; m_ += W) {
            const int m = m_ + wave;
            const bool mine = m < ne;
            const int i = (2 * m + 1) * s, l = i - s, r = i + s;
            const bool has_r = mine && r < N;
            if (mine) {
                if (factor) {
                    mw::ld_blk<MM>(m0, blk(i, 0), lane);                 // D_i (lower)
                    mw::ld_blk<MM>(m1, blk(i, 1), lane);                 // Y_{i,l}
                    if (has_r) mw::ld_blk<MM>(m2, blk(r, 1), lane);      // Y_{r,i}
                    wla::wsync();
                    if constexpr (MFMA && NE_GJ_MFMA != 0) fail |= wla::spd_inv_gj_mfma<NX>(m0, NX, m4, NX, nullptr, lane);
                    else fail |= wla::spd_inv_gj<NX, double>(m0, NX, m4, NX, nullptr, lane);
                    wla::wsync();
                    mw::mm<NX, false, false>(m4, m1, m3, lane);           // F_l = D^-1 Y_{i,l}
                    if (has_r) mw::mm<NX, false, true>(m4, m2, m0, lane);    // F_r = D^-1 Y_{r,i}'
                    mw::st_blk<MM>(blk(i, 0), m4, lane);
                    mw::st_blk<MM>(blk(i, 1), m3, lane);
                    if (has_r) mw::st_blk<MM>(blk(i, 2), m0, lane);
                } else {
                    mw::ld_blk<MM>(m4, blk(i, 0), lane);                 // D_i^-1
                    mw::ld_blk<MM>(m3, blk(i, 1), lane);                 // F_l
                    if (has_r) mw::ld_blk<MM>(m0, blk(i, 2), lane);      // F_r
                }
                if (lane < NX) sT1[lane] = sNu[i * NX + lane];            // b_i
                wla::wsync();
                const double y = wla::matvec_split3<NX, NX, false>(m4, NX, sT1, lane);
                const double dl = wla::matvec_split3<NX, NX, true>(m3, NX, sT1, lane);
                if (lane < NX) { sNu[i * NX + lane] = y; sNu[l * NX + lane] -= dl; }
                wla::wsync();
                if (factor) {
                    mw::mm<NX, true, false>(m1, m3, m4, lane);            // Y_{i,l}' F_l
                    mw::sub_lower<NX>(blk(l, 0), m4, lane);
                }
            }
            __syncthreads();      // the left neighbours are done: they are the right neighbours of other eliminations
            if (has_r) {
                const double dr = wla::matvec_split3<NX, NX, true>(m0, NX, sT1, lane);
                if (lane < NX) sNu[r * NX + lane] -= dr;
                if (factor) {
                    wla::wsync();
                    mw::mm<NX, false, false>(m2, m0, m4, lane);           // Y_{r,i} F_r
                    mw::sub_lower<NX>(blk(r, 0), m4, lane);
                    mw::mm<NX, false, false>(m2, m3, m1, lane);           // Y_{r,l} = -Y_{r,i} F_l
                    double *gC = blk(r, 1);
#pragma unroll
                    for (int o = lane; o < MM; o += 64) gC[o] = -m1[o];
                }
            }
            __syncthreads();
        }
    }
    // ---- root
    if (wave == 0) {
        if (factor) {
            mw::ld_blk<MM>(m0, blk(0, 0), lane);
            wla::wsync();
            if constexpr (MFMA && NE_GJ_MFMA != 0) fail |= wla::spd_inv_gj_mfma<NX>(m0, NX, m4, NX, nullptr, lane);
            else fail |= wla::spd_inv_gj<NX, double>(m0, NX, m4, NX, nullptr, lane);
            wla::wsync();
            mw::st_blk<MM>(blk(0, 0), m4, lane);
        } else mw::ld_blk<MM>(m4, blk(0, 0), lane);
        if (lane < NX) sT1[lane] = sNu[lane];
        wla::wsync();
        const double y = wla::matvec_split3<NX, NX, false>(m4, NX, sT1, lane);
        if (lane < NX) sNu[lane] = y;
    }
    __syncthreads();
    // ---- back-substitution, down the levels
    for (s /= 2; s >= 1; s /= 2) {
        const int cnt = (N + s - 1) / s, ne = cnt / 2;
        for (int m = wave; m < ne; m += W) {
            const int i = (2 * m + 1) * s, l = i - s, r = i + s;
            mw::ld_blk<MM>(m3, blk(i, 1), lane);
            if (r < N) mw::ld_blk<MM>(m0, blk(i, 2), lane);
            wla::wsync();
            double v = wla::matvec_split3<NX, NX, false>(m3, NX, sNu + l * NX, lane);
            if (r < N) v += wla::matvec_split3<NX, NX, false>(m0, NX, sNu + r * NX, lane);
            if (lane < NX) sNu[i * NX + lane] -= v;
            wla::wsync();
        }
        __syncthreads();
    }
    // ---- W = nu, G = E' nu: stage k on wave k mod W
    for (int k = wave; k < N; k += W) {
        mw::ld_blk<MM>(m1, g.A + (size_t)k * MM, lane);
        mw::ld_blk<NX * NU>(sB, g.Bm + (size_t)k * NX * NU, lane);
        wla::wsync();
        const double *nu = sNu + k * NX;
        const double ga = wla::matvec_split3<NX, NX, true>(m1, NX, nu, lane);
        const double gb = wla::matvec_split3<NU, NX, true>(sB, NU, nu, lane);
        if (lane < NX) {
            g.W[k * NX + lane] = nu[lane];
            g.G[k * NZ + lane] = (k > 0) ? ga - sNu[(k - 1) * NX + lane] : ga;
            if (k == N - 1) g.G[N * NZ + lane] = 0.0 - nu[lane];
        }
        if (lane < NU) g.G[k * NZ + NX + lane] = gb;
        wla::wsync();
    }
    if (lane == 0) sRed[MW_MAX_WAVES + wave] = (double)fail;
    __syncthreads();
    int f = 0;
    for (int w = 0; w < W; w++) f |= (sRed[MW_MAX_WAVES + w] != 0.0) ? 1 : 0;
    __syncthreads();      // (sRed is written again by the next call)
    return f;
}

// The QP solve of one instance by one workgroup of W waves: the tick loop of qp_solve_dev with the cooperative block solve in place of the two
// sweeps.  The phase logic runs on wave 0 while the others wait at the barrier behind it (phase_update<.., false>: no workgroup barrier inside, see
// phase_sync); every wave reads the phase from QpState after that barrier.
// cr: (B, N, 3, NX, NX) scratch of the reduction.  (cr and W are kernel parameters of their own: QpArgs keeps its size)
template <int NX, int NU>
__global__ __launch_bounds__(64 * MW_MAX_WAVES) void k_qp_solve_mw(QpArgs a, int max_ticks, double *cr, int W) {
    int b = blockIdx.x;
    if (b >= a.B) return;
    extern __shared__ double sm[];
    int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (a.run && !a.run[b]) {       // not part of this solve (workgroup-uniform)
        if (wave == 0 && a.qpstat && lane < 8) a.qpstat[((size_t)b * 2 + a.stat_slot) * 8 + lane] = (lane == 6) ? -1 : 0;
        return;
    }
    if (wave == 0) phase_update<NX, NU, false>(a, 1, b, lane);
    __syncthreads();
    unsigned long long n_sweeps = 0, n_factor = 0, n_fstages = 0, n_bwd_skipped = 0;
#ifdef QP_STAMP
    // cycle stamps of wave 0 (scripts/stamp_qp.py): cooperative solves that factorise / that only substitute (each up to the barrier behind it, so the
    // slowest wave counts), phase logic (up to the barrier behind it); kkt slots 2..7 as in qp_solve_dev, slot 5 (backward sweeps) stays 0
    long long c_crf = 0, c_cr = 0, c_ph = 0, c_t0 = __builtin_readcyclecounter(), c_last = c_t0;
#define MW_STAMP(acc) do { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); const long long t_ = __builtin_readcyclecounter(); acc += t_ - c_last; c_last = t_; } while (0)
#else
#define MW_STAMP(acc) do {} while (0)
#endif
    for (int t = 0; t < max_ticks; t++) {
        // (the instance index and the lane id are laundered at the head of every part, as in qp_solve_dev: nothing derived from them is hoisted out of
        // the tick loop and kept in registers across the block solve)
        LAUNDER_B(b);
        asm volatile("" : "+v"(lane));
        QpState *st = (QpState *)a.state + b;
        double *crb = cr + (size_t)b * mw_scratch_doubles<NX>(a.N);
        const int phase = (int)st->phase;
        if (phase == P_DONE) break;
        const FwdPlan fp = fwd_plan(st, phase, a.N);
        // no partial re-factorisation here; a QP that inherits its predecessor's factorisation (k0 = N) substitutes only
        const bool factor = fp.factor && !(phase == P_POL0 && fp.k0 >= a.N);
        const double res_tol = (phase == P_POL2 && st->res_only != 0.0) ? RES_ONLY_TOL * st->qscale : -1.0;
        double bmax = 0.0;
        const int f = ne_solve_cr<NX, NU>(sm, make_neg<NX, NU>(a, b), crb, factor, fp.eflag, fp.delta, lane, wave, W, &bmax, res_tol);
        if (wave == 0 && lane == 0) {
            if (phase == P_POL1 || phase == P_POL2) st->pbox = bmax;
            st->ticks += 1.0;
            if (fp.factor) { st->fticks += 1.0; if (phase == P_POL0) st->pol_fail = f & 1; }
        }
        n_sweeps++; n_factor += fp.factor ? 1 : 0; n_fstages += factor ? (unsigned long long)a.N : 0ULL; n_bwd_skipped += (f & 2) ? 1 : 0;
        __threadfence_block();
        __syncthreads();
#ifdef QP_STAMP
        if (factor) MW_STAMP(c_crf); else MW_STAMP(c_cr);
#endif
        LAUNDER_B(b);
        asm volatile("" : "+v"(lane));
        if (wave == 0) phase_update<NX, NU, false>(a, 0, b, lane, sm);
        __threadfence_block();
        __syncthreads();
        MW_STAMP(c_ph);
    }
#ifdef QP_STAMP
    if (wave == 0 && lane == 0) { double *kk = a.kkt + (size_t)b * 8; kk[2] = (double)c_crf; kk[3] = (double)n_fstages; kk[4] = (double)c_cr; kk[5] = 0.0; kk[6] = (double)c_ph; kk[7] = (double)(__builtin_readcyclecounter() - c_t0); }
#endif
    if (wave == 0 && lane == 0) {
        atomicAdd(a.inst_launches, n_sweeps); atomicAdd(a.inst_launches + 1, n_factor); atomicAdd(a.inst_launches + 2, n_fstages);
        atomicAdd(a.inst_launches + 3, (((QpState *)a.state + b)->ticks > 0.0) ? 1ULL : 0ULL);
        if (n_bwd_skipped) atomicAdd(a.inst_launches + 4, n_bwd_skipped);
    }
}

// One block solve of every instance on given Pi and v (slsqp_ne_solve): W = 1 runs the two sweeps of the single-wave kernels (full factorisation or
// none), W > 1 the cyclic reduction.  out: (B,2) max|b| and the "not positive definite" flag.
template <int NX, int NU>
__global__ __launch_bounds__(64 * MW_MAX_WAVES) void k_ne_solve(NeG<NX, NU> g0, int B, double *cr, int W, int factor, double delta, double *out) {
    const int b = blockIdx.x;
    if (b >= B) return;
    extern __shared__ double sm[];
    using L = Lay<NX, NU>;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int N = g0.N, n = L::n(N);
    NeG<NX, NU> g = g0;
    g.A += (size_t)b * N * NX * NX; g.Bm += (size_t)b * N * NX * NU; g.Linv += (size_t)b * N * NX * NX;
    g.PI += (size_t)b * n; g.V += (size_t)b * n; g.G += (size_t)b * n; g.W += (size_t)b * N * NX; g.UF += (size_t)b * N * NX;
    double bmax = 0.0;
    int f;
    if (W == 1) {
        f = ne_forward<NX, NU>(sm, g, factor != 0, 0.0, delta, lane, &bmax, 0, 0);
        wla::wsync_mem();
        ne_backward<NX, NU>(sm, g, lane);
    } else {
        f = ne_solve_cr<NX, NU>(sm, g, cr + (size_t)b * mw_scratch_doubles<NX>(N), factor != 0, 0.0, delta, lane, wave, W, &bmax);
    }
    if (threadIdx.x == 0) { out[2 * b] = bmax; out[2 * b + 1] = (double)(f & 1); }
}

}  // namespace slsqp
