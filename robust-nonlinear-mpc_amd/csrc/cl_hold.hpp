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

// The event-triggered schedule (slsqp_cl_set_hold_trigger): an instance holds while its measured state stays inside the
// fraction theta of the tube its plan computed, and solves when it does not, or after M steps at the latest.  theta = +inf (the default): off, the
// schedule above.  One definition for the host, the persistent kernel, slsqp_cl_tube_ratio and tests/hold_trigger_ref.py.
CL_HOLD_HD inline bool valid_trigger(double theta) { return theta >= 0.0; }      // [0, +inf]; a NaN is refused
CL_HOLD_HD inline bool trigger_on(double theta, int M) { return M > 1 && theta <= 1.7976931348623157e308; }
// component i of the tube ratio: |x - z| / bo in plain fp64; a tube of zero width holds exactly its centre; a NaN counts as outside every tube
CL_HOLD_HD inline double tube_term(double x, double z, double bo) {
    if (bo == 0.0) return x == z ? 0.0 : __builtin_huge_val();
    const double t = __builtin_fabs(x - z) / bo;
    return t == t ? t : __builtin_huge_val();
}
enum Trigger { TRIG_HOLD = 0, TRIG_SCHEDULED = 1, TRIG_TUBE = 2, TRIG_FAILED = 3 };
// What an instance does at its step s: k_prev is the hold index of step s - 1 (0: a solve), k = k_prev + 1 the hold step that would come next,
// plan_ok the success of its last solve, r the tube ratio of the measured state at stage k of that plan (read only where s >= 1 and plan_ok).
// TRIG_HOLD: hold step k; every other code: solve.
CL_HOLD_HD inline int decide(int s, int k_prev, int M, bool plan_ok, double r, double theta) {
    if (s == 0 || k_prev + 1 >= M) return TRIG_SCHEDULED;
    if (!plan_ok) return TRIG_FAILED;
    if (!(r <= theta)) return TRIG_TUBE;      // (a NaN ratio triggers)
    return TRIG_HOLD;
}

// Plan fallback (slsqp_cl_set_plan_fallback): a step that applies no freshly certified plan -- a solve that failed, or a hold
// step -- runs the tube policy of the instance's last plan that succeeded, kept in a backup beside the live arrays.  age: plant steps since that plan
// pinned its stage 0 (0 right after the successful solve, -1: no backup).  One definition for the host, both kernels and tests/plan_fallback_ref.py.
CL_HOLD_HD inline bool valid_plan_fallback(int on) { return on == 0 || on == 1; }
// the hold step of the backup such a step runs, or 0: no backup, or the backup has no row left (K has N rows: k <= N - 1)
CL_HOLD_HD inline int fallback_index(int age, int N) { return (age >= 0 && age + 1 <= N - 1) ? age + 1 : 0; }
// the age a step leaves behind; fresh: a solve that succeeded.  A step that found no plan marks the backup gone
CL_HOLD_HD inline int plan_age_after(bool fresh, int age, int N) {
    if (fresh) return 0;
    const int k = fallback_index(age, N);
    return k ? k : -1;
}
enum Policy { POLICY_NOMINAL = 0, POLICY_HOLD = 1, POLICY_FALLBACK = 2 };
// hold_policy / log_hold_policy of a step that applied no fresh plan: k = fallback_index of the age it found; hold_step: the schedule made it a hold step
CL_HOLD_HD inline int policy_code(bool hold_step, int k) { return k ? (hold_step ? POLICY_HOLD : POLICY_FALLBACK) : POLICY_NOMINAL; }

struct State {
    int k = 0;              // index of the last hold step (1 = the first plant step after a solve)
    int at_steps = -1;      // the handle's step count right after that hold step (-1: none since slsqp_cl_init)
    int run_steps = -1;     // the step count a persistent / round-based run left behind (-1: none since slsqp_cl_init)
    int dev_steps = -1;     // the step count an event-triggered run left behind: "hold_index" is the per-instance device array (-1: none since slsqp_cl_init)
};

inline void on_init(State &s) { s = State{}; }
// k_last > 0: the run's last step was the hold step of that index (a persistent run with solve_every > 1): "hold_index" serves it
inline void on_run(State &s, int cl_steps_after, int k_last = 0) { s.run_steps = cl_steps_after; if (k_last > 0) { s.k = k_last; s.at_steps = cl_steps_after; } }
// an event-triggered run: every instance ends at its own index
inline void on_triggered_run(State &s, int cl_steps_after) { s.run_steps = cl_steps_after; s.dev_steps = cl_steps_after; }
inline bool index_per_instance(const State &s, int cl_steps) { return cl_steps == s.dev_steps; }
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
