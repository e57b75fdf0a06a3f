// cl_bounds.hpp -- host side of the time-varying box bounds (slsqp_cl_set_bounds): the validation of a caller's rows and their packing into the
// layout the kernels read.  Plain C++ without a HIP call, so that a stand-alone host program can exercise it (tests/cl_bounds_check_main.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <string>
#include <vector>

namespace cl_bounds {

// One block of rows, g (rows, ni) or gf (rows, nif), of a box G = [I; -I]: entry i is the upper side hi_i, entry half + i the negated lower side
// -lo_i (half = ni / 2).  Refused: NaN, -inf (a side at -inf leaves nothing), hi < lo.  +inf is "no bound" on that side, as 1e20 is.
inline bool check_rows(const char *what, const double *g, size_t rows, int ni, std::string *why) {
    const int half = ni / 2;
    for (size_t r = 0; r < rows; r++) {
        const double *row = g + r * (size_t)ni;
        for (int i = 0; i < ni; i++) {
            const double v = row[i];
            if (std::isnan(v) || (std::isinf(v) && v < 0.0)) {
                if (why) *why = std::string(what) + " row " + std::to_string(r) + ", entry " + std::to_string(i) + " is NaN or -inf";
                return false;
            }
        }
        for (int i = 0; i < half; i++)
            if (row[i] + row[half + i] < 0.0) {      // hi - lo < 0
                if (why) *why = std::string(what) + " row " + std::to_string(r) + ", component " + std::to_string(i) + ": upper bound " + std::to_string(row[i]) +
                                " below lower bound " + std::to_string(-row[half + i]);
                return false;
            }
    }
    return true;
}

// The arguments of the call that do not need the data: T, the pointers, per_instance.
inline bool check_call(const double *g, int T, int per_instance, std::string *why) {
    if (per_instance != 0 && per_instance != 1) { if (why) *why = "per_instance must be 0 (one set of rows for the batch: g (T,ni), gf (T,ni_f)) or 1 (g (B,T,ni), gf (B,T,ni_f))"; return false; }
    if (T < 0) { if (why) *why = "T must be >= 1 (or 0 with g = NULL to clear the bounds)"; return false; }
    if (T == 0 && g) { if (why) *why = "T = 0 clears the bounds and takes g = NULL; bounds have T >= 1 rows"; return false; }
    if (T > 0 && !g) { if (why) *why = "g is NULL with T > 0 (T = 0 clears the bounds)"; return false; }
    return true;
}

// g (sets, T, ni) and gf (sets, T, nif) or NULL (every terminal row is gf_model (nif)) -> out (sets, T, ni + nif), row = [g(t); gf(t)]: what the
// kernels index (BndArgs, slsqp_kernels.hpp).  sets = 1 (shared) or the batch.  Returns false with the reason in *why and `out` untouched when a row
// is refused.
inline bool pack(const double *g, const double *gf, const double *gf_model, size_t sets, int T, int ni, int nif, std::vector<double> *out, std::string *why) {
    const size_t rows = sets * (size_t)T;
    if (!check_rows("g", g, rows, ni, why)) return false;
    if (gf ? !check_rows("gf", gf, rows, nif, why) : !check_rows("the model's gf", gf_model, 1, nif, why)) return false;
    std::vector<double> p(rows * (size_t)(ni + nif));
    for (size_t r = 0; r < rows; r++) {
        double *row = p.data() + r * (size_t)(ni + nif);
        for (int i = 0; i < ni; i++) row[i] = g[r * (size_t)ni + i];
        for (int i = 0; i < nif; i++) row[ni + i] = gf ? gf[r * (size_t)nif + i] : gf_model[i];
    }
    out->swap(p);
    return true;
}

}  // namespace cl_bounds
