"""Input sets of the sweep-route tests (tests/test_sweep_ref_cpu.py on the CPU, tests/test_gpu_sweep_routes.py on the GPU): the smallest shapes that
reach every branch of the shared sweep (k_sweep_ric1 + k_sweep_prop, two disturbance columns per wave), each with three disturbance matrices.

  shapes    pendulum (4,1), vector-ALU products:   N = 1 (N + 1 = 2: one pair whose second column is terminal-only), 2 (a pair plus a single), 5 (even)
            quadrotor (13,4), matrix-core pair:     N = 2, 5
            rocket (17,4), matrix-core pair:        N = 3, 6
  E         "model"  the model's diagonal E at every stage (what every other test uses)
            "dense"  nw = nx, E_0 = the model's E (the plant step of a closed loop reads only that block), later stages the model's E plus
                     0.5 |E_ii| N(0,1) on about half the entries of row i: dense and different at every stage
            "nw"     nw < nx (2 for the pendulum, 5 for the others): full nx x nw blocks (every entry perturbed), different at every stage, stage 0 included
Instances are problems.make_instance data (seed = batch index) at amplitude 0.3, with a linear cost that drives about half the inputs 1.5 times
past one of their bounds (push_inputs_to_bounds): at amplitude 0.3 alone no constraint of any instance is active, every dual and with it every
eta is zero, and the sweep would only ever see the unconstrained regulator.
"""
from types import SimpleNamespace

import numpy as np

from problems import make_instance

SHAPES = [("pendulum", 1), ("pendulum", 2), ("pendulum", 5), ("quadrotor", 2), ("quadrotor", 5), ("rocket", 3), ("rocket", 6)]
VARIANTS = ("model", "dense", "nw")
NW_SMALL = {"pendulum": 2, "quadrotor": 5, "rocket": 5}
AMP = 0.3
B_MAX = 11          # the separate launches run 11 instances (k_sweep_prop's XCD mapping: 8 in its first branch, 3 in its remainder branch)

_MODEL_KEYS = ("nx", "nu", "nz", "ni", "ni_f", "G", "Gf", "g", "gf", "Q", "R", "Qf", "Q_reg", "R_reg", "Q_reg_f", "x_ref", "u_ref", "x_lb", "x_ub")


def dense_E(m, N, nw=None, first_is_model=True, seed=0, density=0.5):
    """(N+1, nx, nw) blocks: the model's E (its first nw columns) plus 0.5 |E_ii| N(0,1) on about `density` of the entries of row i, at every stage.
    (Per row, not 0.5 max|E| everywhere: the rocket's E spans 8.7e-5 .. 4e-2, and noise of 2e-2 on its attitude rows makes every tightened QP of
    the N = 6 instances infeasible, so no second fast-SLS iteration could be tested on them.)"""
    nw = m.nw if nw is None else nw
    rng = np.random.default_rng(7000 + 31 * seed + N)
    base = np.asarray(m.E, dtype=float)[:, :nw]
    amp = 0.5 * np.abs(np.diag(np.asarray(m.E, dtype=float)))[:, None]
    E = np.stack([base + amp * rng.normal(size=base.shape) * (rng.uniform(size=base.shape) < density) for _ in range(N + 1)])
    if first_is_model:
        E[0] = base
    return E


def make_E(m, N, variant):
    if variant == "model":
        return np.stack([np.asarray(m.E, dtype=float)] * (N + 1))
    if variant == "dense":
        return dense_E(m, N)
    assert variant == "nw"
    return dense_E(m, N, nw=NW_SMALL[m.name], first_is_model=False, seed=1, density=1.0)


def push_inputs_to_bounds(inst, seed):
    """q of input i at stage k (every other (k, i), the pattern moves with the seed) := -2 R_ii 1.5 (distance to its upper bound), or the same
    towards its lower bound: the unconstrained minimiser lies 1.5 times past the bound, the QP puts the input on it and its multiplier is
    positive.  The tightened QPs stay feasible (tests/test_sweep_ref_cpu.py asserts it)."""
    m, N = inst.m, inst.N
    nx, nu, nz = m.nx, m.nu, m.nz
    Rd = np.diag(m.R)
    for k in range(N):
        for i in range(nu):
            if (k + i + seed) % 2:
                continue
            up = (k + seed) % 3 != 0
            margin = inst.g_list[k][nx + i] if up else inst.g_list[k][nz + nx + i]
            inst.q[k * nz + nx + i] = (-1.0 if up else 1.0) * 2.0 * Rd[i] * 1.5 * margin


def make_case(model, N, variant, B):
    """B instances that share one E (N+1, nx, nw).  With nw < nx the instances carry a copy of the model that says so."""
    insts = [make_instance(model, seed=s, x0_amp=AMP, N=N) for s in range(B)]
    m = insts[0].m
    for s, i in enumerate(insts):
        push_inputs_to_bounds(i, s)
    E = make_E(m, N, variant)
    if variant == "nw":
        m = SimpleNamespace(name=m.name, nw=E.shape[2], E=E[0], **{k: getattr(m, k) for k in _MODEL_KEYS})
    for i in insts:
        i.m, i.E = m, E
    return insts


def shifted_E(E):
    """The mistake a wrong stage offset would make: column j starts from E_{j+1} (the last column from E_0)."""
    return np.roll(E, -1, axis=0)


def case_id(model, N, variant):
    return f"{model}-N{N}-{variant}"


ALL_CASES = [(model, N, v) for model, N in SHAPES for v in VARIANTS]
