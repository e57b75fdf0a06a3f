// plant_params.hpp -- host side of the plant parameters (slsqp_cl_set_plant_params): names, defaults and the validation of a caller's values.
// Plain C++ without a HIP call, so that a stand-alone host program can exercise it (tests/plant_params_check_main.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <string>

#include "dynamics.hpp"

namespace plant_params {

inline int count(int model_id) {
    return model_id == 0 ? dyn::Dims<0>::NP : model_id == 1 ? dyn::Dims<1>::NP : model_id == 2 ? dyn::Dims<2>::NP : -1;
}
// the order of dyn::ParamDefault; quadrotor and rocket: the keys of the reference's `params` dicts (dyn/quadrotor.py:32-40, dyn/rocket.py:25-39)
inline const char *name(int model_id, int i) {
    static const char *pend[] = {"m1", "m2", "l", "g"};
    static const char *quad[] = {"m", "g", "l", "Jx", "Jy", "Jz", "kM"};
    static const char *rock[] = {"mass", "gravity_constant", "inertia_xx", "inertia_yy", "inertia_zz", "thrust_cog_offset", "thrust_magnitude_time_constant",
                                 "servo_angle_time_constant", "gimbal_a", "gimbal_b", "gimbal_c", "gimbal_d", "gimbal_e"};
    if (i < 0 || i >= count(model_id)) return nullptr;
    return model_id == 0 ? pend[i] : model_id == 1 ? quad[i] : rock[i];
}
inline double default_value(int model_id, int i) {
    return model_id == 0 ? dyn::param_default<0>(i) : model_id == 1 ? dyn::param_default<1>(i) : dyn::param_default<2>(i);
}
// Every entry must be > 0 that the ODE divides by or that is a mass, an inertia, a length, a time constant or g: all but the quadrotor's yaw moment
// coefficient kM, which only has to be finite.
inline bool must_be_positive(int model_id, int i) { return !(model_id == 1 && i == 6); }

// P (rows, np) row-major.  Returns true when every entry passes; otherwise false with the reason in *why.
inline bool check(int model_id, const double *P, size_t rows, int np, std::string *why) {
    const int want = count(model_id);
    if (want < 0) { if (why) *why = "no model set"; return false; }
    if (np != want) {
        if (why) *why = "np = " + std::to_string(np) + ", but the handle's model has " + std::to_string(want) + " plant parameters";
        return false;
    }
    for (size_t r = 0; r < rows; r++)
        for (int i = 0; i < np; i++) {
            const double v = P[r * (size_t)np + i];
            if (!std::isfinite(v)) {
                if (why) *why = std::string("row ") + std::to_string(r) + ": " + name(model_id, i) + " is NaN or infinite";
                return false;
            }
            if (must_be_positive(model_id, i) && !(v > 0.0)) {
                if (why) *why = std::string("row ") + std::to_string(r) + ": " + name(model_id, i) + " = " + std::to_string(v) + " must be > 0";
                return false;
            }
        }
    return true;
}

}  // namespace plant_params
