// cl_hold_kernel.hpp -- one closed-loop step WITHOUT a solve: the tube's disturbance-feedback policy acts on the plan of the last solve
// (slsqp_cl_hold_step, include/slsqp.h).
//
// Hold step k = 1, 2, ... <= N - 1 after a solve, stage 0 of the plan pinned to the state measured then.  Per instance, column states xi_j (NX),
// j = 1..k (column 0 is zero: x_0 was pinned), the state-space realisation of Phi_u = K Phi_x (fast_SLS_jit.py:87-117):
//     e    = x_meas - z_k
//     xi_j <- (A_{k-1} + B_{k-1} K[k-1,j]) xi_j      1 <= j < k      what the plan predicts of the old columns
//     xi_k  = e - sum_{j<k} xi_j                                     what it did not predict: disturbance + model defect
//     u     = v_k + sum_{1<=j<=k} K[k,j] xi_j
//     x_meas <- plant(x_meas, u) + E w
// The caller has shifted the nominal by one stage, so z_k, v_k are stage 0 of Xn / Un; A, B, K are indexed from the solve.
#ifndef SLSQP_CL_HOLD_KERNEL_HPP
#define SLSQP_CL_HOLD_KERNEL_HPP
#include "cl_hold.hpp"
#include "slsqp_kernels.hpp"

namespace slsqp {

struct HoldArgs {
    ClArgs cl;                  // the shifted nominal, x_meas, E, w, u0
    int k;                      // hold index, 1 .. N - 1
    const double *A, *Bm;       // (B,N,NX,NX), (B,N,NX,NU): the linearisation of the last solve
    const double *K, *Kc;       // (B,N,N+1,NU,NX) and the compact gains (B,N,NU,NX) of the shared Riccati recursion
    const int *stale;           // (B) bit 32: the gains are Kc (K[k,j] = Kc[k], j <= k); else bit 2: K is from before the last reset (reads as zero)
    const int *scp_success;     // (B) outcome of the last slsqp_cl_step: 0 = no valid plan, the instance applies v_k
    double *xi;                 // (B,N+1,NX) column states, row j = xi_j
    double *u;                  // (B,NU) the input the plant step applies
    int *policy;                // (B) 1: the policy ran, 0: the nominal input was applied
    int S, step;                // the closed-loop log (S = 0: off) and the entry of this step
    double *lstate, *lu0, *lx0v;
    int *lit, *lhold, *lpol;
};

// One 64-lane wave per instance.  Old columns: groups of NX lanes take 64 / NX columns side by side, lane (g, i) forms row i of its column --
// y = K[k-1,j] xi_j on the group's first NU lanes, then A xi_j + B y; A_{k-1}, B_{k-1} and the columns are read from global memory once, coalesced,
// into LDS.  New column and the sum over the columns: lane i = row i.  Policy sum: lane j forms K[k,j] xi_j (k <= 63 columns), the NU sums go
// through the crossbar.  Plant step: lane 0, the function the solved steps use, with u in the place of the first nominal input.
//
// The work is written once, for one wave and one instance, and has two callers: k_cl_hold below (one block per instance, slsqp_cl_hold_step) and the
// hold path of the persistent closed-loop kernel (k_cl_loop's HOLD variants), which passes its dynamic LDS.
template <int MODEL>
constexpr int cl_hold_lds_doubles() {      // sA | sB | sXi | sY
    constexpr int NX = dyn::Dims<MODEL>::NX, NU = dyn::Dims<MODEL>::NU;
    return NX * NX + NX * NU + 64 * NX + (64 / NX) * NU;
}
// xi, u and policy of hold step k of instance b (a.k is not read); ends with u in global memory for every lane of the wave
template <int MODEL>
__device__ __forceinline__ void cl_hold_wave(const HoldArgs &a, int b, int lane, int k, double *sm) {
    constexpr int NX = dyn::Dims<MODEL>::NX, NU = dyn::Dims<MODEL>::NU, G = 64 / NX;
    static_assert(NU <= NX && G >= 1, "row i of y lives on lane i of a column's group");
    double *sA = sm, *sB = sA + NX * NX, *sXi = sB + NX * NU, *sY = sXi + 64 * NX;
    const int N = a.cl.N;
    double *xi = a.xi + (size_t)b * (N + 1) * NX;
    const double *Un0 = a.cl.Un + (size_t)b * N * NU;
    const bool ok = a.scp_success[b] != 0;
    if (!ok) {      // no valid plan: the shifted nominal input, as a failed solved step applies it; xi stays (all zero from the first hold step on)
        if (k == 1) for (int o = lane; o < (N + 1) * NX; o += 64) xi[o] = 0.0;
        if (lane < NU) a.u[(size_t)b * NU + lane] = Un0[lane];
    } else {
        const int st = a.stale[b];
        const bool compact = st & 32, zeroK = !compact && (st & 2);
        const double *Kb = a.K + (size_t)b * N * (N + 1) * NU * NX, *Kcb = a.Kc + (size_t)b * N * NU * NX;
        auto gain = [&](int kk, int j) { return compact ? Kcb + (size_t)kk * NU * NX : Kb + ((size_t)kk * (N + 1) + j) * NU * NX; };
        const double *Ak = a.A + ((size_t)b * N + (k - 1)) * NX * NX, *Bk = a.Bm + ((size_t)b * N + (k - 1)) * NX * NU;
        for (int o = lane; o < NX * NX; o += 64) sA[o] = Ak[o];
        for (int o = lane; o < NX * NU; o += 64) sB[o] = Bk[o];
        for (int o = lane; o < (k - 1) * NX; o += 64) sXi[o] = xi[NX + o];      // column j at sXi[(j - 1) NX ...]
        wla::wsync();
        const int g = lane / NX, i = lane - g * NX;
        for (int j0 = 0; j0 < k - 1; j0 += G) {
            const int jj = j0 + g;
            const bool act = g < G && jj < k - 1;
            if (act && i < NU) {
                double y = 0.0;
                if (!zeroK) {
                    const double *Kr = gain(k - 1, jj + 1) + i * NX;
#pragma unroll
                    for (int l = 0; l < NX; l++) y = fma(Kr[l], sXi[jj * NX + l], y);
                }
                sY[g * NU + i] = y;
            }
            wla::wsync();
            double v = 0.0;
            if (act) {
#pragma unroll
                for (int l = 0; l < NX; l++) v = fma(sA[i * NX + l], sXi[jj * NX + l], v);
#pragma unroll
                for (int c = 0; c < NU; c++) v = fma(sB[i * NU + c], sY[g * NU + c], v);
            }
            wla::wsync();      // every lane of the group has read the old column
            if (act) sXi[jj * NX + i] = v;
        }
        wla::wsync();
        if (lane < NX) {
            double s = 0.0;
            for (int jj = 0; jj < k - 1; jj++) s += sXi[jj * NX + lane];
            const double e = a.cl.xmeas[(size_t)b * NX + lane] - a.cl.Xn[(size_t)b * (N + 1) * NX + lane];
            sXi[(k - 1) * NX + lane] = e - s;
        }
        wla::wsync();
        for (int o = lane; o < k * NX; o += 64) xi[NX + o] = sXi[o];
        if (k == 1) for (int o = lane; o < (N + 1) * NX; o += 64) if (o < NX || o >= 2 * NX) xi[o] = 0.0;      // a new plan: no other column yet
        double p[NU];
#pragma unroll
        for (int c = 0; c < NU; c++) p[c] = 0.0;
        if (lane < k && !zeroK) {
            const double *Kr = gain(k, lane + 1);
#pragma unroll
            for (int c = 0; c < NU; c++)
#pragma unroll
                for (int l = 0; l < NX; l++) p[c] = fma(Kr[c * NX + l], sXi[lane * NX + l], p[c]);
        }
#pragma unroll
        for (int c = 0; c < NU; c++) {
            const double s = wla::wave_sum(p[c]);
            if (lane == c) a.u[(size_t)b * NU + c] = Un0[c] + s;
        }
    }
    if (lane == 0) a.policy[b] = ok ? 1 : 0;
    wla::wsync_mem();      // u is in global memory for lane 0's plant step and for the log
}
// entry `step` of the closed-loop log as a hold step leaves it (a.S = 0: no log; a.step is not read): state and applied input of this step; no
// solve: 0 iterations, nothing on record for the stage-0 gate
template <int MODEL>
__device__ __forceinline__ void cl_hold_log(const HoldArgs &a, int b, int lane, int k, int step) {
    constexpr int NX = dyn::Dims<MODEL>::NX, NU = dyn::Dims<MODEL>::NU;
    if (a.S > 0 && step < a.S) {
        const bool ok = a.scp_success[b] != 0;
        const size_t e = (size_t)b * a.S + step;
        if (lane < NX) a.lstate[e * NX + lane] = a.cl.xmeas[(size_t)b * NX + lane];
        if (lane < NU) a.lu0[e * NU + lane] = a.u[(size_t)b * NU + lane];
        if (lane == 0) { a.lit[e] = 0; a.lhold[e] = k; a.lpol[e] = ok ? 1 : 0; a.lx0v[e * 2] = 0.0; a.lx0v[e * 2 + 1] = 0.0; }
        wla::wsync_mem();      // the state is logged before lane 0 replaces it
    }
}
// The tube ratio of instance b for the hold step k that would come next (cl_hold.hpp): max_i |x_meas_i - z_i| / backoff_x[k, i],
// z stage 1 of the nominal as it stands (the plan's stage k: a hold step shifts before it acts).  Lane i takes component i; the lanes above NX hold 0,
// no term is negative or a NaN (cl_hold::tube_term), so the crossbar's max is the max in ascending i.  Every lane returns it.  Reads only.
// Two callers: k_cl_tube_ratio below (slsqp_cl_tube_ratio) and the event-triggered HOLD variants of the persistent closed-loop kernel.
template <int MODEL>
__device__ __forceinline__ double cl_tube_ratio_wave(const ClArgs &cl, const double *backoff_x, int b, int lane, int k) {
    constexpr int NX = dyn::Dims<MODEL>::NX;
    static_assert(NX <= 64, "lane i takes component i");
    const size_t row = (size_t)b * (cl.N + 1) * NX;
    double t = 0.0;
    if (lane < NX) t = cl_hold::tube_term(cl.xmeas[(size_t)b * NX + lane], cl.Xn[row + NX + lane], backoff_x[row + (size_t)k * NX + lane]);
    return wla::wave_max(t);
}
// one wave per instance: out[b] = the ratio for hold step k, +inf for an instance without a valid plan
template <int MODEL>
__global__ __launch_bounds__(64) void k_cl_tube_ratio(ClArgs cl, const double *backoff_x, const int *scp_success, int k, double *out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= cl.B) return;
    const double r = scp_success[b] != 0 ? cl_tube_ratio_wave<MODEL>(cl, backoff_x, b, lane, k) : INFINITY;
    if (lane == 0) out[b] = r;
}
template <int MODEL, bool PP>
__global__ __launch_bounds__(64) void k_cl_hold(HoldArgs a, PlantArgs pa) {
    __shared__ double sm[cl_hold_lds_doubles<MODEL>()];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= a.cl.B) return;
    cl_hold_wave<MODEL>(a, b, lane, a.k, sm);
    cl_hold_log<MODEL>(a, b, lane, a.k, a.step);
    if (lane == 0) {
        ClArgs c = a.cl;
        c.N = 1; c.Un = a.u;      // "the first nominal input" of instance b is u[b]: the nominal itself stays the plan
        cl_plant_one<MODEL, PP>(c, b, a.cl.w, PP ? &pa : nullptr, a.step);
    }
}

}  // namespace slsqp
#endif
