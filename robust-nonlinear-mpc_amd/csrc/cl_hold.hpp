// cl_hold.hpp -- host-side bookkeeping of slsqp_cl_hold_step (include/slsqp.h): which hold step comes next and when the call
// is refused.  Free of HIP calls, so that tests/cl_hold_check_main.cpp can run it in a stand-alone program under the sanitizers.
//
// The handle counts closed-loop steps (cl_steps: 0 after slsqp_cl_init, + 1 per slsqp_cl_step and per hold step, = steps after a slsqp_cl_run /
// slsqp_cl_run_scp).  A hold step records the count it leaves behind; when the next hold step finds another count, a slsqp_cl_step has run in
// between (nothing else moves the count by a call that leaves a plan) and the index starts again at 1: slsqp_cl_step itself knows nothing of this.
#ifndef SLSQP_CL_HOLD_HPP
#define SLSQP_CL_HOLD_HPP
#include <string>

namespace cl_hold {

struct State {
    int k = 0;              // index of the last hold step (1 = the first plant step after a solve)
    int at_steps = -1;      // the handle's step count right after that hold step (-1: none since slsqp_cl_init)
    int run_steps = -1;     // the step count a persistent / round-based run left behind (-1: none since slsqp_cl_init)
};

inline void on_init(State &s) { s = State{}; }
inline void on_run(State &s, int cl_steps_after) { s.run_steps = cl_steps_after; }
inline void on_hold(State &s, int k, int cl_steps_after) { s.k = k; s.at_steps = cl_steps_after; }
// "hold_index": hold steps since the last solve
inline int index(const State &s, int cl_steps) { return cl_steps == s.at_steps ? s.k : 0; }

// The index k >= 1 of the hold step a call would run, or 0 with *why set: the call is refused and changes nothing.
inline int next_index(const State &s, bool have_model, int cl_steps, int N, int loc, std::string *why) {
    if (!have_model) { *why = "slsqp_set_model must be called first"; return 0; }
    if (loc != 0 && loc != 1) { *why = "loc must be SLSQP_HOST or SLSQP_DEVICE"; return 0; }
    if (cl_steps <= 0) { *why = "no slsqp_cl_step since slsqp_cl_init: there is no plan to hold"; return 0; }
    if (cl_steps == s.run_steps) { *why = "slsqp_cl_run / slsqp_cl_run_scp leave no per-batch plan: run slsqp_cl_step first"; return 0; }
    const int k = index(s, cl_steps) + 1;
    if (k > N - 1) { *why = "hold step " + std::to_string(k) + " of a horizon N = " + std::to_string(N) + ": K has N rows, at most N - 1 hold steps between two solves"; return 0; }
    return k;
}

}  // namespace cl_hold
#endif
