// cl_hold.hpp -- host-side bookkeeping of slsqp_cl_hold_step (include/slsqp.h): which hold step comes next and when the call
// is refused.  Free of HIP calls, so that tests/cl_hold_check_main.cpp can run it in a stand-alone program under the sanitizers.
//
// The handle counts closed-loop steps (cl_steps: 0 after slsqp_cl_init, + 1 per slsqp_cl_step and per hold step, = steps after a slsqp_cl_run /
// slsqp_cl_run_scp).  A hold step records the count it leaves behind; when the next hold step finds another count, a slsqp_cl_step has run in
// between (nothing else moves the count by a call that leaves a plan) and the index starts again at 1: slsqp_cl_step itself knows nothing of this.
#ifndef SLSQP_CL_HOLD_HPP
#define SLSQP_CL_HOLD_HPP
#include <string>

#ifdef __HIPCC__
#define CL_HOLD_HD __host__ __device__
#else
#define CL_HOLD_HD
#endif

namespace cl_hold {

// The schedule of a run that solves every M-th step (slsqp_cl_set_solve_every): step s = 0, 1, ... of a run is a solve when
// hold_index_at is 0 and else the hold step of that index since the last solve.  One definition for the host and for the persistent kernel.
CL_HOLD_HD inline bool valid_solve_every(int M, int N) { return M >= 1 && M <= N; }      // K has N rows: at most N - 1 hold steps between two solves
CL_HOLD_HD inline int hold_index_at(int step, int M) { return M > 1 ? step % M : 0; }
CL_HOLD_HD inline bool is_solve(int step, int M) { return hold_index_at(step, M) == 0; }
inline int solves_in(int steps, int M) { return steps <= 0 ? 0 : (steps + M - 1) / M; }      // solves among the steps 0 .. steps - 1

struct State {
    int k = 0;              // index of the last hold step (1 = the first plant step after a solve)
    int at_steps = -1;      // the handle's step count right after that hold step (-1: none since slsqp_cl_init)
    int run_steps = -1;     // the step count a persistent / round-based run left behind (-1: none since slsqp_cl_init)
};

inline void on_init(State &s) { s = State{}; }
// k_last > 0: the run's last step was the hold step of that index (a persistent run with solve_every > 1): "hold_index" serves it
inline void on_run(State &s, int cl_steps_after, int k_last = 0) { s.run_steps = cl_steps_after; if (k_last > 0) { s.k = k_last; s.at_steps = cl_steps_after; } }
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
