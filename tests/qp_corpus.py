"""Seeded corpus of hard QPs of the path, plus independent host checks (test helper, CPU only).

Every QP is in the reference row layout that `qp_update_data_vec` takes (qp_jit.py:101-123): per stage nx dynamics rows
(l = -c - eps, u = -c + eps), nz upper-bound rows z <= hi and nz lower-bound rows -z <= -lo (l = -1e20), the terminal rows, then the
nx rows that pin x_0.  The QP is strictly convex (diagonal Q, R, Qf > 0), so its optimum is unique when it is feasible.

Classes (all three plants):
  easy         today's regime (x0 amplitude 0.2-1)
  stress       scripts/stress.py's two regimes (x0 amplitude 2 / 8, Jacobian noise 1e-2 / 3e-2, defects 1e-2 / 5e-2)
  bigset       boxes shrunk towards the nominal until the optimum has many active bounds (>= 29 where the plant has room for them)
  degenerate   bounds exactly at the optimum of the QP without them (weakly active), zero-width input boxes, all boxes infinite
               (one copy +-1e20, one copy +-inf)
  x0edge       x0 exactly on its stage-0 box, 5e-10 outside (under the kernel's 1e-9 threshold), 1e-6 and 1 outside
  infeasible   x0 inside its box; an empty box at a middle stage, or a state bound no input sequence reaches
  scaled       q scaled by 1e4 and by 1e-4

The checks share no code with the library: `feasibility_margin` is a phase-1 LP (scipy's HiGHS), `reference` the dense interior point and
active-set polish of tests/ref_ipm.py with its own KKT residual, `host_certificate` the oracle's KKT measure plus explicit finiteness and
box / dynamics residuals computed here.
"""
import numpy as np

from problems import make_instance, qp1_bounds

PLANTS = ("pendulum", "quadrotor", "rocket")
BIG = 1e19          # |bound| >= BIG: no bound (the reference writes 1e20)


class QP:
    """One QP instance: plant data (A, B, weights), q, l, u in the reference row layout, its class and what it is meant to be."""

    def __init__(self, m, N, A, B, q, l, u, cls, name, intent="feasible"):
        self.m, self.N = m, N
        self.A, self.B = np.array(A, dtype=float), np.array(B, dtype=float)
        self.q, self.l, self.u = np.array(q, dtype=float), np.array(l, dtype=float), np.array(u, dtype=float)
        self.cls, self.name, self.intent = cls, name, intent
        self.twin = None     # name of a QP that must give the same answer (the +-1e20 / +-inf pair)

    # ---- layout -------------------------------------------------------------------------------------------
    @property
    def nx(self):
        return self.m.nx

    @property
    def nz(self):
        return self.m.nz

    @property
    def SR(self):
        return self.m.nx + self.m.ni

    @property
    def n(self):
        return self.nz * self.N + self.nx

    @property
    def mb(self):
        return self.N * self.SR + self.m.ni_f

    def hi_row(self, e):
        """row of u that holds the upper bound of primal element e (stage-ordered z = [x_0 u_0 x_1 u_1 ... x_N])"""
        k, i = divmod(e, self.nz)
        return k * self.SR + self.nx + i if k < self.N else self.N * self.SR + i

    def lo_row(self, e):
        k, i = divmod(e, self.nz)
        return k * self.SR + self.nx + self.nz + i if k < self.N else self.N * self.SR + self.nx + i

    def boxes(self):
        """hi, lo per primal element (the stage-0 state box included)"""
        idx = np.arange(self.n)
        hi = self.u[[self.hi_row(e) for e in idx]]
        lo = -self.u[[self.lo_row(e) for e in idx]]
        return hi, lo

    def set_box(self, e, hi=None, lo=None):
        if hi is not None:
            self.u[self.hi_row(e)] = hi
        if lo is not None:
            self.u[self.lo_row(e)] = -lo

    def x0val(self):
        return 0.5 * (self.l[self.mb:] + self.u[self.mb:])     # the value the pin rows fix (the kernel's own arithmetic)

    def x0_violation(self):
        hi, lo = self.boxes()
        x0 = self.x0val()
        return float(np.max(np.maximum(x0 - hi[:self.nx], lo[:self.nx] - x0)))

    def Pd(self):
        m = self.m
        return 2.0 * np.concatenate([np.concatenate([np.diag(m.Q), np.diag(m.R)])] * self.N + [np.diag(m.Qf)])

    def equalities(self):
        """E z = e: x_0 pin, then A_k x_k + B_k u_k - x_{k+1} = -c_k with c_k = -(l + u)/2 of the dynamics rows"""
        from ref_ipm import build_equalities
        c = np.stack([-0.5 * (self.u[k * self.SR:k * self.SR + self.nx] + self.l[k * self.SR:k * self.SR + self.nx]) for k in range(self.N)])
        return build_equalities(self.A, self.B, c, self.x0val())

    def qscale(self):
        return max(1.0, float(np.abs(self.q).max()))

    def copy(self, cls=None, name=None, intent=None):
        c = QP(self.m, self.N, self.A, self.B, self.q, self.l, self.u, cls or self.cls, name or self.name, intent or self.intent)
        return c


def _base(model, seed, x0_amp, jac_amp=0.0, c_amp=1e-3, cls="easy", name=None, intent="feasible"):
    inst = make_instance(model, seed, x0_amp, c_amp=c_amp)
    if jac_amp > 0.0:
        rng = np.random.default_rng(5000 + seed)
        inst.A = inst.A + jac_amp * rng.normal(size=inst.A.shape)
        inst.B = inst.B + jac_amp * rng.normal(size=inst.B.shape)
    l, u = qp1_bounds(inst)
    return QP(inst.m, inst.N, inst.A, inst.B, inst.q, l, u, cls, name or f"{cls}-{seed}", intent)


# ---- independent checks -----------------------------------------------------------------------------------------
def feasibility_margin(qp):
    """Phase-1 LP: t* = min t  s.t.  E z = e (x_0 pinned),  z - t <= hi,  lo - z <= t on the finite bounds,  t >= -1.
    Returns (t*, verdict): 'feasible' for t* <= -delta, 'infeasible' for t* >= delta, else 'borderline'; delta = 1e-6 max(1, |bounds|inf)."""
    import scipy.sparse as sp
    from scipy.optimize import linprog
    E, e = qp.equalities()
    hi, lo = qp.boxes()
    fu, fl = np.abs(hi) < BIG, np.abs(lo) < BIG
    n = qp.n
    iu, il = np.flatnonzero(fu), np.flatnonzero(fl)
    rows = len(iu) + len(il)
    Aub = sp.lil_matrix((rows, n + 1))
    for r, i in enumerate(iu):
        Aub[r, i] = 1.0; Aub[r, n] = -1.0
    for r, i in enumerate(il):
        Aub[len(iu) + r, i] = -1.0; Aub[len(iu) + r, n] = -1.0
    bub = np.concatenate([hi[iu], -lo[il]])
    Aeq = sp.hstack([sp.csr_matrix(E), sp.csr_matrix((E.shape[0], 1))])
    cost = np.zeros(n + 1); cost[n] = 1.0
    res = linprog(cost, A_ub=Aub.tocsr(), b_ub=bub, A_eq=Aeq.tocsr(), b_eq=e, bounds=[(None, None)] * n + [(-1.0, None)], method="highs")
    assert res.status == 0, res.message
    t = float(res.x[n])
    scale = max(1.0, float(np.abs(bub).max(initial=0.0)), float(np.abs(e).max()))
    delta = 1e-6 * scale
    return t, ("feasible" if t <= -delta else ("infeasible" if t >= delta else "borderline"))


def reference(qp):
    """Optimum of the QP the kernel solves (the pinned x_0 has no box of its own: the stage-0 state box only gates the x0 check), by
    tests/ref_ipm.py's dense interior point + active-set polish.  Returns dict(x, y) in the reference layout (OSQP signs), or None when the
    pinned x_0 lies outside its box or the interior point does not converge."""
    from ref_ipm import polish, qp_box
    if qp.x0_violation() > 1e-9:
        return None
    E, e = qp.equalities()
    hi, lo = qp.boxes()
    hi, lo = np.where(np.abs(hi) < BIG, hi, 1e20), np.where(np.abs(lo) < BIG, lo, -1e20)
    hi[:qp.nx], lo[:qp.nx] = 1e20, -1e20
    Pd, q = qp.Pd(), qp.q
    z, nu, lu, ll, ok, its = qp_box(Pd, q, E, e, lo, hi)
    if not ok:
        return None
    zp, nup, lup, llp, polished = polish(Pd, q, E, e, lo, hi, z, lu, ll)
    if polished:
        z, nu, lu, ll = zp, nup, lup, llp
    # own KKT residual of the reference optimum
    sc = qp.qscale()
    fu, fl = hi < BIG, lo > -BIG
    kkt = max(np.abs(Pd * z + q + E.T @ nu + lu - ll).max() / sc, np.abs(E @ z - e).max() / sc,
              np.max(np.where(fu, z - hi, 0.0)), np.max(np.where(fl, lo - z, 0.0)), -min(lu.min(), ll.min()))
    nx, nz, SR, N = qp.nx, qp.nz, qp.SR, qp.N
    y = np.zeros(qp.mb + nx)
    for k in range(N):
        y[k * SR:k * SR + nx] = nu[nx * (k + 1):nx * (k + 2)]
        y[k * SR + nx:k * SR + nx + nz] = lu[k * nz:(k + 1) * nz]
        y[k * SR + nx + nz:k * SR + nx + 2 * nz] = ll[k * nz:(k + 1) * nz]
    y[N * SR:N * SR + nx] = lu[N * nz:]; y[N * SR + nx:N * SR + 2 * nx] = ll[N * nz:]
    y[-nx:] = nu[:nx]
    act = (lu > 1e-6 * sc) | (ll > 1e-6 * sc)
    slack = np.minimum(np.where(fu, hi - z, np.inf), np.where(fl, z - lo, np.inf))
    free = np.arange(qp.n) >= nx
    strict = bool(np.all(act[free] | (slack[free] > 1e-6)))          # strictly complementary: every bound either clearly active or clearly slack
    return dict(x=z, y=y, kkt=float(kkt), polished=bool(polished), strict=strict, n_active=int(act[free].sum()))


def host_certificate(qp, x, y, status, qp_eps=1e-6):
    """The documented certificate checked on the host, with 10x slack: status 0 needs stationarity, box violation and
    multiplier sign <= 1e-8 qscale and dynamics residual <= 1e-6 qscale; status 4 (interior point accurate, polish rejected) the
    interior-point accuracy, max(qp_eps, 1e-9) qscale, on the first three.  Returns (ok, report)."""
    from oracle import oracle as O
    m = qp.m
    rep = dict(finite=bool(np.isfinite(x).all() and np.isfinite(y).all()))
    if not rep["finite"]:
        return False, rep
    d = O.dims_of(m.nx, m.nu, m.nw, qp.N, m.ni, m.ni_f)
    l = np.where(np.isneginf(qp.l), -1e20, np.where(np.isposinf(qp.l), 1e20, qp.l))
    u = np.where(np.isposinf(qp.u), 1e20, np.where(np.isneginf(qp.u), -1e20, qp.u))
    k = O.qp_kkt(d, qp.A, qp.B, m.G, m.Gf, m.Q, m.R, m.Qf, qp.q, l, u, x, y)
    hi, lo = qp.boxes()
    fu, fl = np.abs(hi) < BIG, np.abs(lo) < BIG
    box = max(0.0, float(np.max(np.where(fu, x - hi, 0.0))), float(np.max(np.where(fl, lo - x, 0.0))))
    E, e = qp.equalities()
    dyn = float(np.abs(E @ x - e).max())
    # multiplier signs of the box rows (upper rows: y >= 0; lower rows written as -z <= -lo: y >= 0 as well)
    ybox = np.concatenate([y[[qp.hi_row(i) for i in range(qp.n)]], y[[qp.lo_row(i) for i in range(qp.n)]]])
    sign = max(0.0, float(-ybox.min()), k["dual_sign"])
    rep.update(stationarity=k["stationarity"], box=box, sign=sign, dynamics=dyn)
    sc = qp.qscale()
    tol = 1e-8 if status == 0 else 10.0 * max(qp_eps, 1e-9)
    ok = rep["stationarity"] <= tol * sc and box <= tol * sc and sign <= tol * sc and dyn <= 1e-6 * sc
    return bool(ok), rep


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1.0, float(np.max(np.abs(b)))))


# ---- classes ----------------------------------------------------------------------------------------------------
def _bigset(model, seed, want=29):
    """Boxes of the stages after x_0 shrunk towards the nominal (z = 0) until the optimum has >= want active bounds (or the LP margin runs
    out): all boxes first, the input boxes alone when that runs out of margin first (the rocket's state boxes do)."""
    base = _base(model, seed, 0.6, cls="bigset")
    n_free = base.n - base.nx
    want = min(want, int(0.45 * n_free))
    hi, lo = base.boxes()
    best, best_act = None, -1
    for inputs_only in (False, True):
        for s in (0.5, 0.3, 0.2, 0.12, 0.08, 0.05, 0.03, 0.02):
            qp = base.copy(name=f"bigset-{seed}-{'u' if inputs_only else 'z'}{s}")
            for e in range(base.nx, base.n):
                if inputs_only and (e % base.nz < base.nx):
                    continue
                if abs(hi[e]) < BIG and hi[e] > 0:
                    qp.set_box(e, hi=s * hi[e])
                if abs(lo[e]) < BIG and lo[e] < 0:
                    qp.set_box(e, lo=s * lo[e])
            t, verdict = feasibility_margin(qp)
            if verdict != "feasible" or t > -1e-3:
                break
            ref = reference(qp)
            if ref is None:
                break
            if ref["n_active"] > best_act:
                best, best_act = qp, ref["n_active"]
            if best_act >= want:
                return best
    return best


def _weakly_active(model, seed):
    """Bounds placed exactly at the optimum of the QP without them: active with multiplier 0."""
    qp = _base(model, seed, 0.5, cls="degenerate", name=f"weak-{seed}")
    ref = reference(qp)
    hi, lo = qp.boxes()
    z = ref["x"]
    slack = np.minimum(hi - z, z - lo)
    cand = [e for e in range(qp.nx, qp.n) if slack[e] > 1e-3]
    rng = np.random.default_rng(77 + seed)
    for e in rng.choice(cand, size=min(6, len(cand)), replace=False):
        if rng.uniform() < 0.5:
            qp.set_box(int(e), hi=z[e])
        else:
            qp.set_box(int(e), lo=z[e])
    return qp


def _zero_width(model, seed):
    """lo == hi on every input of a few stages (inside the original box)."""
    qp = _base(model, seed, 0.5, cls="degenerate", name=f"zerowidth-{seed}")
    hi, lo = qp.boxes()
    for k in (1, qp.N // 2, qp.N - 1):
        for i in range(qp.m.nu):
            e = k * qp.nz + qp.nx + i
            v = lo[e] + 0.3 * (hi[e] - lo[e])
            qp.set_box(e, hi=v, lo=v)
    return qp


def _unbounded(model, seed, val):
    qp = _base(model, seed, 0.5, cls="degenerate", name=f"nobox-{'inf' if np.isinf(val) else '1e20'}-{seed}")
    for e in range(qp.n):
        qp.set_box(e, hi=val, lo=-val)
    return qp


def _x0edge(model, seed, off):
    qp = _base(model, seed, 0.5, cls="x0edge", name=f"x0edge-{off:g}-{seed}", intent="feasible" if off <= 0 else "x0out")
    x0 = qp.x0val()
    i = seed % qp.nx
    qp.set_box(i, hi=x0[i] - off)          # the stage-0 upper bound of component i at (or off below) x0
    return qp


def _empty_box(model, seed):
    qp = _base(model, seed, 0.5, cls="infeasible", name=f"emptybox-{seed}", intent="infeasible")
    hi, lo = qp.boxes()
    e = (qp.N // 2) * qp.nz + qp.nx + (seed % qp.m.nu)
    qp.set_box(e, lo=hi[e] + 0.5)
    return qp


def _unreachable(model, seed):
    """x0 inside its box, but a state bound at a middle stage beyond what any admissible input sequence reaches (found by an LP)."""
    import scipy.sparse as sp
    from scipy.optimize import linprog
    qp = _base(model, seed, 0.5, cls="infeasible", name=f"unreachable-{seed}", intent="infeasible")
    E, e = qp.equalities()
    hi, lo = qp.boxes()
    b = np.where(np.abs(hi) < BIG, hi, None), np.where(np.abs(lo) < BIG, lo, None)
    bounds = [(b[1][i], b[0][i]) for i in range(qp.n)]
    for i in range(qp.nx):
        bounds[i] = (None, None)
    j = (qp.N // 2) * qp.nz + (seed % qp.nx)
    cost = np.zeros(qp.n); cost[j] = -1.0
    res = linprog(cost, A_eq=sp.csr_matrix(E), b_eq=e, bounds=bounds, method="highs")
    zmax = -res.fun if res.status == 0 else hi[j]
    qp.set_box(j, hi=1e20, lo=zmax + 0.05 * max(1.0, abs(zmax)))
    return qp


def corpus(model):
    """The seeded corpus of one plant (~25 QPs)."""
    out = [_base(model, s, a, name=f"easy-{a}-{s}") for s, a in ((0, 0.2), (1, 0.6), (2, 1.0))]
    for r, (amp, jac, c) in enumerate(((2.0, 1e-2, 1e-2), (8.0, 3e-2, 5e-2))):
        out += [_base(model, 10 + 2 * r + s, amp, jac, c, cls="stress", name=f"stress{r}-{s}", intent="any") for s in range(2)]
    for s in range(4):
        bq = _bigset(model, 20 + s)
        if bq is not None:
            out.append(bq)
    out += [_weakly_active(model, 30), _weakly_active(model, 31), _zero_width(model, 32)]
    a, b = _unbounded(model, 33, 1e20), _unbounded(model, 33, np.inf)
    a.twin, b.twin = b.name, a.name
    out += [a, b]
    out += [_x0edge(model, 40 + s, off) for s, off in enumerate((0.0, 5e-10, 1e-6, 1.0))]
    out += [_empty_box(model, 50), _unreachable(model, 51)]
    for s, f in ((60, 1e4), (61, 1e-4)):
        qp = _base(model, s, 0.5, cls="scaled", name=f"scaled-{f:g}")
        qp.q = qp.q * f
        out.append(qp)
    return out
