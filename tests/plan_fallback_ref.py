"""Plain numpy restatement of plan fallback's bookkeeping (test helper, CPU only): which policy step a closed-loop step runs and
the age it leaves, the rule of csrc/cl_hold.hpp (fallback_index, plan_age_after, policy_code).

Per instance: `age` = plant steps since the last plan that succeeded pinned its stage 0 (-1: no backup).  A solve that succeeds applies its own plan
and sets age = 0.  Every other step -- a solve that failed, a hold step -- runs hold step k = age + 1 of the backup while the backup exists and
k <= N - 1 (K has N rows), and then age = k; else it applies the nominal input and the backup is gone (age = -1).
Policy codes: 0 the nominal input (or a fresh plan), 1 a hold step that ran the policy, 2 a failed solve that ran the backup's policy."""
import numpy as np

NOMINAL, HOLD, FALLBACK = 0, 1, 2


def fallback_index(age, N):
    return age + 1 if age >= 0 and age + 1 <= N - 1 else 0


def step(age, N, solve, success):
    """One step of one instance.  solve: the schedule makes it a solve; success: that solve's outcome (not read on a hold step).
    Returns (k, code, age_after): k the hold step of the backup that ran (0: none)."""
    if solve and success:
        return 0, NOMINAL, 0
    k = fallback_index(age, N)
    return k, (FALLBACK if solve else HOLD) if k else NOMINAL, k if k else -1


def run(N, hold_index, success):
    """A whole run from the log: hold_index (B, steps) of the schedule (0: a solve), success (B, steps).  Returns (k, code, age), each (B, steps)."""
    hold_index, success = np.asarray(hold_index), np.asarray(success, dtype=bool)
    k, code, age = (np.zeros(hold_index.shape, dtype=np.int32) for _ in range(3))
    for b in range(hold_index.shape[0]):
        a = -1
        for s in range(hold_index.shape[1]):
            k[b, s], code[b, s], a = step(a, N, hold_index[b, s] == 0, success[b, s])
            age[b, s] = a
    return k, code, age
