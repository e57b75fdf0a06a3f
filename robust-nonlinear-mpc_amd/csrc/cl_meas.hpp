// cl_meas.hpp -- measurement noise of the closed loops (slsqp_cl_set_meas_noise): the controller of instance b sees
// x_meas = x_plant + n_s at its MPC step s while the plant steps from x_plant.  One definition for the batch-wide kernel k_cl_meas, for the lane that
// runs the plant step inside the persistent closed-loop kernels, and for the host (the setter's validation; tests/cl_meas_noise_check_main.cpp).  No
// HIP call in here.
//
// The plant step itself is not touched: it reads and writes the array x_meas, as ever.  The two halves of the rule stand around its one call site:
//   pre   (before the adversary and the plant step of step s)   log entries s of the measurement and of the truth; x_meas <- x_plant
//   post  (after the plant step of step s)                      x_plant <- x_meas; x_meas <- x_meas + n_{s+1}
// so the adversary and the plant step find the truth in x_meas, and everything on the controller's side finds the measurement there.  n_s is row
// min(s, T - 1) of the table (the last row is held; T = 1: a constant bias).  The measurement is ONE fp64 addition per component and no product: no
// instantiation can contract it into a multiply-add, and numpy gives the same bits.  post with s = -1 is what slsqp_cl_init does: x_plant <- x,
// x_meas <- x + n_0.
#ifndef SLSQP_CL_MEAS_HPP
#define SLSQP_CL_MEAS_HPP

#include <cmath>
#include <cstddef>
#include <string>

#ifdef __HIPCC__
#define CL_MEAS_HD __host__ __device__ inline
#else
#define CL_MEAS_HD inline
#endif

namespace cl_meas {

// rows: the table, (T, nx) shared by the batch (stride 0) or one block of T rows per instance (stride T nx); T = 0: the option is off and no other
// field is read.  x_plant (B, nx): the true state.  lg_plant / lg_meas (B, S, nx) or NULL: the per-step logs of the truth and of the measurement
// (nothing is written past the log's last entry).
struct Args {
    const double *rows;
    int T, S;
    size_t stride;
    double *x_plant, *lg_plant, *lg_meas;
};

CL_MEAS_HD bool on(const Args &a) { return a.T > 0; }
// the table's row for MPC step s, the last one held (s < 0 counts as 0)
CL_MEAS_HD int row_index(int s, int T) { return s < 0 ? 0 : (s < T - 1 ? s : T - 1); }
CL_MEAS_HD const double *row_at(const Args &a, int nx, int b, int s) { return a.rows + (size_t)b * a.stride + (size_t)row_index(s, a.T) * (size_t)nx; }
// the measurement of one component: one addition
CL_MEAS_HD double measure(double x_plant, double n) { return x_plant + n; }

// before the adversary and the plant step of instance b at its step s: xm is row b of x_meas, which holds the measurement the step's controller used
CL_MEAS_HD void pre(const Args &a, int nx, int b, int s, double *xm) {
    const bool log = s >= 0 && s < a.S;
    double *xp = a.x_plant + (size_t)b * nx;
    for (int i = 0; i < nx; i++) {
        const double t = xp[i];
        if (log) {
            const size_t e = ((size_t)b * a.S + s) * nx + i;
            if (a.lg_meas) a.lg_meas[e] = xm[i];
            if (a.lg_plant) a.lg_plant[e] = t;
        }
        xm[i] = t;
    }
}
// after the plant step of instance b at its step s (s = -1: slsqp_cl_init): xm holds the new true state
CL_MEAS_HD void post(const Args &a, int nx, int b, int s, double *xm) {
    const double *n = row_at(a, nx, b, s + 1);
    double *xp = a.x_plant + (size_t)b * nx;
    for (int i = 0; i < nx; i++) {
        const double t = xm[i];
        xp[i] = t;
        xm[i] = measure(t, n[i]);
    }
}

// ---- host only: what slsqp_cl_set_meas_noise refuses (the message names the argument) -------------------------------------------------------------
// Nm: the caller's table on the host, rows x T x nx doubles (rows = B with per_instance, else 1), or NULL.  T = 0 with Nm = NULL clears the option.
inline bool check(const double *Nm, int T, int per_instance, int loc, bool have_model, int B, int nx, std::string *why) {
    auto no = [&](const std::string &m) { if (why) *why = m; return false; };
    if (!have_model) return no("handle: slsqp_set_model must be called first");
    if (per_instance != 0 && per_instance != 1) return no("per_instance = " + std::to_string(per_instance) + " must be 0 (one table (T,nx) for the batch) or 1 (Nm (B,T,nx))");
    if (loc != 0 && loc != 1) return no("loc = " + std::to_string(loc) + " must be SLSQP_HOST or SLSQP_DEVICE");
    if (T < 0) return no("T = " + std::to_string(T) + " must be >= 0 (0 with Nm = NULL clears the option)");
    if (T == 0 && Nm) return no("T = 0 clears the option and takes Nm = NULL");
    if (T > 0 && !Nm) return no("Nm is NULL with T = " + std::to_string(T) + " (T = 0 clears the option)");
    return true;
}
// the entries, once they are on the host
inline bool check_entries(const double *Nm, int T, int per_instance, int B, int nx, std::string *why) {
    const size_t n = (size_t)(per_instance ? B : 1) * (size_t)T * (size_t)nx;
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(Nm[i])) { if (why) *why = "Nm holds a NaN or infinite entry (at flat index " + std::to_string(i) + ")"; return false; }
    return true;
}

}  // namespace cl_meas
#endif
