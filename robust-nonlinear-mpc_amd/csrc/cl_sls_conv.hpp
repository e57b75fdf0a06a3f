// cl_sls_conv.hpp -- fast-SLS converge mode inside the persistent closed-loop launch (slsqp_cl_set_sls_converge): the option's
// range, and which statistics slots the batch-wide launches of the step-by-step loop leave as "took no part".  Free of HIP calls: one definition for
// the host, the post-pass kernel behind the launch and tests/cl_sls_conv_check_main.cpp.
//
// The step-by-step loop (solve_impl, converge mode) launches QP i = 0, 1, ... of a solve for the whole batch with the instances still `alive` as its
// mask; an instance that is no longer alive gets "took no part" (status -1, zeros elsewhere) written into the slot of every such launch.  After QP i it
// counts the instances that go on to a sweep and stops when there are none, or when i + 1 = max_sls_iter.  Inside the persistent launch an instance
// walks its own iterations and knows nothing of the others; what it keeps is n, the sweeps it ran in the step's last solve -- it took part in the loop
// QPs 0 .. n (0 .. n - 1 when n = max_sls_iter: it hit the cap) -- and the rule below says from the n of all instances whether a later launch rewrote its slot 0.
#ifndef SLSQP_CL_SLS_CONV_HPP
#define SLSQP_CL_SLS_CONV_HPP

#ifdef __HIPCC__
#define CL_SLS_CONV_HD __host__ __device__
#else
#define CL_SLS_CONV_HD
#endif

namespace cl_sls_conv {

CL_SLS_CONV_HD inline bool valid_option(int on) { return on == 0 || on == 1; }
CL_SLS_CONV_HD inline bool valid_cap(int max_sls_iter) { return max_sls_iter >= 1; }
// what slsqp_cl_run_scp says to opts.rti_steps with the option off / on: NULL = the setting runs (rti_steps <= 0: on the CONV variants), else the refusal
inline const char *run_scp_refusal(int rti_steps, int option_on, int max_sls_iter) {
    if (rti_steps >= 1) return nullptr;
    if (!option_on) return "slsqp_cl_run_scp: fast-SLS converge mode (rti_steps <= 0) does not run inside the persistent loop (use slsqp_cl_step)";
    if (!valid_cap(max_sls_iter)) return "slsqp_cl_run_scp: fast-SLS converge mode needs max_sls_iter >= 1";
    return nullptr;
}
// the index of the last loop QP the batch launches in a solve whose busiest instance ran nmax sweeps (cap = max_sls_iter >= 1)
CL_SLS_CONV_HD inline int last_loop_qp(int nmax, int cap) { return nmax < cap - 1 ? nmax : cap - 1; }
// slot 0 of an instance that ran n sweeps in that solve holds "took no part" afterwards: a loop QP was launched after the last one it took part in
CL_SLS_CONV_HD inline bool slot0_took_no_part(int n, int nmax, int cap) { return n < last_loop_qp(nmax, cap); }

}  // namespace cl_sls_conv
#endif
