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
    int *policy;                // (B) 1: the policy ran, 0: the nominal input was applied (plan fallback: 2 = a failed solve ran the backup's policy)
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
// plan (wave-uniform; plan fallback): 0 -- the plan is the live one, valid when the last solve succeeded, gains where stale says;
// > 0 -- a.A / a.Bm / a.Kc are the backup, valid, its gains compact, and `plan` is the policy code to record; < 0 -- no plan (k: the schedule's index)
template <int MODEL>
__device__ __forceinline__ void cl_hold_wave(const HoldArgs &a, int b, int lane, int k, double *sm, int plan = 0) {
    constexpr int NX = dyn::Dims<MODEL>::NX, NU = dyn::Dims<MODEL>::NU, G = 64 / NX;
    static_assert(NU <= NX && G >= 1, "row i of y lives on lane i of a column's group");
    double *sA = sm, *sB = sA + NX * NX, *sXi = sB + NX * NU, *sY = sXi + 64 * NX;
    const int N = a.cl.N;
    double *xi = a.xi + (size_t)b * (N + 1) * NX;
    const double *Un0 = a.cl.Un + (size_t)b * N * NU;
    const bool ok = plan ? plan > 0 : a.scp_success[b] != 0;
    if (!ok) {      // no valid plan: the shifted nominal input, as a failed solved step applies it; xi stays (all zero from the first hold step on)
        if (k == 1) for (int o = lane; o < (N + 1) * NX; o += 64) xi[o] = 0.0;
        if (lane < NU) a.u[(size_t)b * NU + lane] = Un0[lane];
    } else {
        const int st = plan ? 32 : a.stale[b];
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
    if (lane == 0) a.policy[b] = ok ? (plan > 0 ? plan : 1) : 0;
    wla::wsync_mem();      // u is in global memory for lane 0's plant step and for the log
}
// entry `step` of the closed-loop log as a hold step leaves it (a.S = 0: no log; a.step is not read): state and applied input of this step; no
// solve: 0 iterations, nothing on record for the stage-0 gate
template <int MODEL>
__device__ __forceinline__ void cl_hold_log(const HoldArgs &a, int b, int lane, int k, int step) {
    constexpr int NX = dyn::Dims<MODEL>::NX, NU = dyn::Dims<MODEL>::NU;
    if (a.S > 0 && step < a.S) {
        const int pol = a.policy[b];      // (cl_hold_wave's, behind its barrier)
        const size_t e = (size_t)b * a.S + step;
        if (lane < NX) a.lstate[e * NX + lane] = a.cl.xmeas[(size_t)b * NX + lane];
        if (lane < NU) a.lu0[e * NU + lane] = a.u[(size_t)b * NU + lane];
        if (lane == 0) { a.lit[e] = 0; a.lhold[e] = k; a.lpol[e] = pol; a.lx0v[e * 2] = 0.0; a.lx0v[e * 2 + 1] = 0.0; }
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
// PP: the waves per SIMD the instantiation had before the plant step took a third inlined model step (the model's row, cl_plant_one) are asked for, so
// that step costs registers of the allocation, not occupancy; 0 without parameters: no request, the code object as it was
template <int MODEL, bool PP>
constexpr int cl_hold_waves() { return !PP ? 0 : MODEL == 0 ? 5 : MODEL == 1 ? 3 : 2; }
template <int MODEL, bool PP>
__global__ __launch_bounds__(64, (cl_hold_waves<MODEL, PP>())) void k_cl_hold(HoldArgs a, PlantArgs pa) {
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
// The hold step of a handle with measurement noise (slsqp_cl_set_meas_noise): the policy and the log of k_cl_hold WITHOUT its
// plant step -- the policy reads the measurement in x_meas, the plant launch that follows (behind k_cl_meas, which puts the truth there) takes u as
// "the first nominal input" of a one-stage plan, as under plan fallback.
template <int MODEL>
__global__ __launch_bounds__(64) void k_cl_hold_policy(HoldArgs a) {
    __shared__ double sm[cl_hold_lds_doubles<MODEL>()];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= a.cl.B) return;
    cl_hold_wave<MODEL>(a, b, lane, a.k, sm);
    cl_hold_log<MODEL>(a, b, lane, a.k, a.step);
}

// ---- plan fallback (slsqp_cl_set_plan_fallback) ---------------------------------------------------------------------------
// The live plan of the instances, the backup of each one's last plan that succeeded (same shapes), the age of that backup (cl_hold.hpp) and its
// per-step log.  With the option on, the HoldArgs beside this struct carry the BACKUP in A / Bm / Kc: every policy step reads the backup store.
struct PlanArgs {
    int on;
    const double *A, *Bm, *Kc, *backoff_x;      // (B,N,NX,NX) (B,N,NX,NU) (B,N,NU,NX) (B,N+1,NX)
    double *bA, *bB, *bKc, *bbo;
    int *age;                                   // (B)
    int *lage;                                  // (B,S) or NULL
};
// n doubles, coalesced; 16-byte accesses where both addresses allow them (a per-instance block is only 8-byte aligned for an odd count)
__device__ __forceinline__ void cl_copy_wave(const double *s, double *d, int n, int lane) {
    if (((((size_t)s) | ((size_t)d)) & 15) == 0) {
        const double2 *s2 = (const double2 *)s;
        double2 *d2 = (double2 *)d;
        const int n2 = n >> 1;
#pragma unroll 4
        for (int o = lane; o < n2; o += 64) d2[o] = s2[o];
        if ((n & 1) && lane == 0) d[n - 1] = s[n - 1];
    } else {
#pragma unroll 4
        for (int o = lane; o < n; o += 64) d[o] = s[o];
    }
}
// one wave copies the plan its instance's solve has just certified into the backup; pure streaming, no LDS
template <int MODEL>
__device__ __forceinline__ void cl_plan_save_wave(const PlanArgs &f, int b, int lane, int N) {
    constexpr int NX = dyn::Dims<MODEL>::NX, NU = dyn::Dims<MODEL>::NU;
    const size_t oA = (size_t)b * N * NX * NX, oB = (size_t)b * N * NX * NU, oX = (size_t)b * (N + 1) * NX;
    cl_copy_wave(f.A + oA, f.bA + oA, N * NX * NX, lane);
    cl_copy_wave(f.Bm + oB, f.bB + oB, N * NX * NU, lane);
    cl_copy_wave(f.Kc + oB, f.bKc + oB, N * NU * NX, lane);
    cl_copy_wave(f.backoff_x + oX, f.bbo + oX, (N + 1) * NX, lane);
}
// What the step of instance b does under the option, sched_k its index in the schedule (0: a solve, whose outcome is a.scp_success).  A solve that
// succeeded: the plan goes into the backup, age 0, the first nominal input goes into u verbatim.  Every other step: k = cl_hold::fallback_index of the
// age -- the caller runs cl_hold_wave(a, b, lane, *kk, sm, *plan) when this returns true (hold step k of the backup, or today's hold step without a
// plan), a failed solve without a plan applies the nominal input.  The age is written here; *age_out: the value, *code: the policy code of the step.
template <int MODEL>
__device__ __forceinline__ bool cl_fallback_begin(const HoldArgs &a, const PlanArgs &f, int b, int lane, int sched_k, int *kk, int *plan, int *age_out, int *code) {
    constexpr int NU = dyn::Dims<MODEL>::NU;
    const int N = a.cl.N;
    const bool fresh = sched_k == 0 && a.scp_success[b] != 0;
    const int age = f.age[b];
    const int kf = fresh ? 0 : cl_hold::fallback_index(age, N);
    *age_out = cl_hold::plan_age_after(fresh, age, N);
    *code = cl_hold::policy_code(sched_k != 0, kf);
    if (fresh) cl_plan_save_wave<MODEL>(f, b, lane, N);
    if (lane == 0) f.age[b] = *age_out;
    if (kf) { *kk = kf; *plan = *code; return true; }
    if (sched_k) { *kk = sched_k; *plan = -1; return true; }
    if (lane < NU) a.u[(size_t)b * NU + lane] = a.cl.Un[(size_t)b * N * NU + lane];
    if (lane == 0 && !fresh) a.policy[b] = 0;
    wla::wsync_mem();      // u is in global memory for the plant step and for the log
    return false;
}
// entry `step` of the log under the option: the age the step left; on a solved step also the input that was applied and the policy code (a hold
// step's are cl_hold_log's)
template <int MODEL>
__device__ __forceinline__ void cl_fallback_log(const HoldArgs &a, const PlanArgs &f, int b, int lane, int step, bool held, int age, int code) {
    constexpr int NU = dyn::Dims<MODEL>::NU;
    if (a.S > 0 && step < a.S) {
        const size_t e = (size_t)b * a.S + step;
        if (!held && lane < NU) a.lu0[e * NU + lane] = a.u[(size_t)b * NU + lane];
        if (lane == 0) { if (!held) a.lpol[e] = code; f.lage[e] = age; }
    }
}
// slsqp_cl_step and slsqp_cl_hold_step under the option, one wave per instance, behind the step's other launches (k_cl_scp_update / k_cl_infeas /
// k_cl_log; the shift and k_cl_log of a hold step): u (B,NU) receives the input to apply for EVERY instance, and the plant launch that follows takes it
// as "the first nominal input" of a one-stage plan.  sched_k: 0 for a solved step, the batch's hold index for a hold step.
template <int MODEL>
__global__ __launch_bounds__(64) void k_cl_plan_fallback(HoldArgs a, PlanArgs f, int sched_k) {
    __shared__ double sm[cl_hold_lds_doubles<MODEL>()];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= a.cl.B) return;
    int kk = 0, plan = 0, age = -1, code = 0;
    if (cl_fallback_begin<MODEL>(a, f, b, lane, sched_k, &kk, &plan, &age, &code)) cl_hold_wave<MODEL>(a, b, lane, kk, sm, plan);
    if (sched_k) cl_hold_log<MODEL>(a, b, lane, sched_k, a.step);
    cl_fallback_log<MODEL>(a, f, b, lane, a.step, sched_k != 0, age, code);
}

}  // namespace slsqp
#endif
