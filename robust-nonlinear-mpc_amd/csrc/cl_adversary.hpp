// cl_adversary.hpp -- the state-feedback disturbance adversary of the closed loops (slsqp_cl_set_adversary): which sample the
// plant step x+ = ddyn(x, u0) + E w of instance b at MPC step s reads, decided from the measured state at that step.  One definition for the batch-wide
// kernel k_cl_adversary, for the lane that runs the plant step inside the persistent closed-loop kernels, and for the host (the setter's validation;
// tests/cl_adversary_check_main.cpp).  No HIP call in here.
//
//   OFF (0)               the caller's sample, as without the option
//   NEAREST_BOUND (1)     d_i = +1 towards the upper side of the box of state i where that side is the nearer one (a tie counts as nearer), -1 towards
//                         the lower; a side that is +inf or >= 1e20 in the [hi; -lo] row is absent: only the other one pulls, none gives d_i = 0
//   AWAY_FROM_TARGET (2)  d_i = +1 if x_i >= xref_i, else -1
// A NaN x_i gives d_i = 0 under both.  Channel j then gets s_j = sum_i d_i E_ij, i ascending, as additions and subtractions of E_ij (no product: no
// instantiation can contract it into a multiply-add and round differently), and
//   w_applied_j = amp sign(s_j)   where mask bit j is set and s_j != 0,      the caller's W_j (0 without a sample) otherwise.
#ifndef SLSQP_CL_ADVERSARY_HPP
#define SLSQP_CL_ADVERSARY_HPP

#include <cmath>
#include <cstddef>
#include <string>

#ifdef __HIPCC__
#define CL_ADV_HD __host__ __device__ inline
#else
#define CL_ADV_HD inline
#endif

namespace cl_adversary {

constexpr int OFF = 0, NEAREST_BOUND = 1, AWAY_FROM_TARGET = 2;
constexpr int MAX_NX = 32;      // the directions and the mask travel as bit sets

// A table over MPC time as the closed-loop options keep them (RowTab, slsqp_kernels.hpp): rows of width W, shared by the batch (stride 0) or one block
// of T rows per instance (stride T W).  The adversary reads the row of the instance's own step, the last row held: min(s, T - 1).
struct Tab { const double *rows; int T; size_t stride; };
CL_ADV_HD const double *row_at(const Tab &t, int b, int s, int W) { return t.rows + (size_t)b * t.stride + (size_t)(s < t.T - 1 ? s : t.T - 1) * (size_t)W; }

// What the option needs at the plant step, beside the measured state, E and the caller's sample.  bd: the bounds in force, rows [g; gf] of width bdW
// whose first 2 nz entries are g = [hi; -lo] over [x; u] (slsqp_cl_set_bounds' table, or the model's g as one shared row); rf: the reference, rows
// [x_ref; u_ref] of width nz (slsqp_cl_set_reference's table, or one shared row of zeros).  mask: bit j = channel j is the adversary's.  adv_w (B, nx)
// receives the sample of every instance's last plant step, lg (B, S, nx) or NULL its per-step log (nothing is written past the log's last entry).
struct Args {
    int policy, nz;
    unsigned mask;
    int bdW;
    double amp;
    double *adv_w, *lg;
    int S, pad_;
    Tab bd, rf;
};

CL_ADV_HD bool side_absent(double v) { return !(v < 1e20); }      // (+inf or >= 1e20; the setters refuse a NaN)
CL_ADV_HD int dir_nearest(double x, double hi, double neg_lo) {
    if (x != x) return 0;
    const bool no_hi = side_absent(hi), no_lo = side_absent(neg_lo);
    if (no_hi && no_lo) return 0;
    if (no_lo) return 1;
    if (no_hi) return -1;
    return (hi - x <= x - (-neg_lo)) ? 1 : -1;
}
CL_ADV_HD int dir_away(double x, double xref) {
    if (x != x) return 0;
    return x >= xref ? 1 : -1;
}
// the directions of the nx states as two bit sets (bit i of *pos: d_i = +1, of *neg: d_i = -1).  g: the stage row [hi; -lo] over nz = nx + nu
// components; xref (nx).  An unknown policy pushes nowhere.
CL_ADV_HD void directions(int policy, int nx, int nz, const double *x, const double *g, const double *xref, unsigned *pos, unsigned *neg) {
    unsigned p = 0u, n = 0u;
    for (int i = 0; i < nx; i++) {
        const int d = policy == NEAREST_BOUND ? dir_nearest(x[i], g[i], g[nz + i]) : policy == AWAY_FROM_TARGET ? dir_away(x[i], xref[i]) : 0;
        if (d > 0) p |= 1u << i; else if (d < 0) n |= 1u << i;
    }
    *pos = p; *neg = n;
}
// channel j: E (nx, nx) row-major with its padded columns zero, Wj the caller's sample of the channel
CL_ADV_HD double channel(int j, int nx, unsigned pos, unsigned neg, const double *E, double amp, unsigned mask, double Wj) {
    double s = 0.0;
    for (int i = 0; i < nx; i++) {
        if ((pos >> i) & 1u) s += E[i * nx + j];
        else if ((neg >> i) & 1u) s -= E[i * nx + j];
    }
    if (!((mask >> j) & 1u)) return Wj;
    return s > 0.0 ? amp : s < 0.0 ? -amp : Wj;
}
// The decision for instance b at MPC step s: x (nx) its measured state, W (nx) the caller's sample of the step or NULL.  Writes row b of adv_w and,
// where there is a log with an entry s, that entry.  policy OFF copies the sample.
CL_ADV_HD void decide(const Args &a, int nx, int b, int s, const double *x, const double *E, const double *W) {
    unsigned pos = 0u, neg = 0u;
    if (a.policy != OFF) directions(a.policy, nx, a.nz, x, row_at(a.bd, b, s, a.bdW), row_at(a.rf, b, s, a.nz), &pos, &neg);
    const bool log = a.lg && s < a.S;
    for (int j = 0; j < nx; j++) {
        const double Wj = W ? W[j] : 0.0;
        const double w = a.policy != OFF ? channel(j, nx, pos, neg, E, a.amp, a.mask, Wj) : Wj;
        a.adv_w[(size_t)b * nx + j] = w;
        if (log) a.lg[((size_t)b * a.S + s) * nx + j] = w;
    }
}

// ---- host only: what slsqp_cl_set_adversary refuses (the message names the argument) ------------------------------------------------------------
inline bool valid_policy(int policy) { return policy == OFF || policy == NEAREST_BOUND || policy == AWAY_FROM_TARGET; }
inline bool check(int policy, double amp, bool have_model, bool general_G, int nx, std::string *why) {
    if (!valid_policy(policy)) { if (why) *why = "policy = " + std::to_string(policy) + " is none of 0 (off), 1 (nearest bound), 2 (away from target)"; return false; }
    if (policy == OFF) return true;      // (clears the option: amp and the mask are not read)
    if (!std::isfinite(amp) || !(amp > 0.0)) { if (why) *why = "amp = " + std::to_string(amp) + " must be finite and > 0 (1 = the vertices of the unit box; above 1: outside the box the tubes were designed for)"; return false; }
    if (general_G) { if (why) *why = "handle: general G: the adversary reads the box of G = [I;-I]"; return false; }      // (asked first: such a handle never gets a model)
    if (!have_model) { if (why) *why = "handle: slsqp_set_model must be called first"; return false; }
    if (nx > MAX_NX) { if (why) *why = "handle: nx above " + std::to_string(MAX_NX); return false; }
    return true;
}
// mask (nx) bytes or NULL (every channel) as the bit set the kernels read
inline unsigned mask_bits(const unsigned char *mask, int nx) {
    unsigned m = 0u;
    for (int j = 0; j < nx && j < MAX_NX; j++) if (!mask || mask[j]) m |= 1u << j;
    return m;
}
inline const char *policy_name(int policy) { return policy == NEAREST_BOUND ? "nearest_bound" : policy == AWAY_FROM_TARGET ? "away_from_target" : "off"; }

}  // namespace cl_adversary
#endif
