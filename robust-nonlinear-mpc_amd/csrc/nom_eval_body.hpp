// nom_eval_body.hpp -- the statements of k_nom_eval and k_nom_eval_bnd (slsqp_kernels.hpp), included INTO both __global__ functions: the two kernels
// differ in their parameter lists (the second one also takes the bounds), and a function around the statements that both kernels called would change
// the register allocation of the first (DESIGN.md sections 13 and 15).  In scope at the point of inclusion: MODEL, REF, BND, NomArgs a, RefArgs rf,
// const BndArgs *bd (NULL and unread without BND).
    constexpr int NX = dyn::Dims<MODEL>::NX, NU = dyn::Dims<MODEL>::NU, NZ = NX + NU;
    const int b = blockIdx.x, t = threadIdx.x;
    if (!a.active[b]) return;
    __shared__ double red[128];
    __shared__ int dec_s;
    const int N = a.N, n = NZ * N + NX;
    double *X = a.Xn + (size_t)b * (N + 1) * NX, *U = a.Un + (size_t)b * N * NU;
    const double *d = a.primal + (size_t)b * n;
    double *S = a.st + (size_t)b * 12;
    const bool trial = a.mode == 1;
    double f = 0.0, v = 0.0, dm = 0.0, c = 0.0;
    for (int e = t; e < n; e += 128) {
        const int k = e / NZ, i = e % NZ;
        const double z0 = (i < NX) ? X[k * NX + i] : U[k * NU + (i - NX)];
        const double dv = trial ? d[e] : 0.0, z = z0 + dv;
        const double hw = (k < N) ? (i < NX ? a.cst.Qd[i] : a.cst.Rd[i - NX]) : a.cst.Qfd[i];
        double hi, lo;
        if constexpr (BND) {      // the box of stage k in the window of MPC step 0
            const double *r = bnd_row(*bd, b, 0, k, 2 * NZ + 2 * NX);
            hi = (k < N) ? r[i] : r[2 * NZ + i]; lo = (k < N) ? -r[NZ + i] : -r[2 * NZ + NX + i];
        } else { hi = (k < N) ? a.g_raw[i] : a.gf_raw[i]; lo = (k < N) ? -a.g_raw[NZ + i] : -a.gf_raw[NX + i]; }
        const double zt = REF ? z - ref_entry<NZ>(rf, b, 0, k, i) : z;
        f += hw * zt * zt;
        if (e >= NX) v += fmax(z - hi, 0.0) + fmax(lo - z, 0.0);   // x_0 is data (pinned to x_meas), its box is not the solver's to fix
        dm = fmax(dm, fabs(dv));
    }
    for (int k = t; k < N; k += 128) {
        double x[NX], u[NU], xp[NX];
        for (int i = 0; i < NX; i++) x[i] = X[k * NX + i] + (trial ? d[k * NZ + i] : 0.0);
        for (int i = 0; i < NU; i++) u[i] = U[k * NU + i] + (trial ? d[k * NZ + NX + i] : 0.0);
        dyn::ddyn<MODEL, double>(x, u, xp);
        for (int i = 0; i < NX; i++) c += fabs(xp[i] - (X[(k + 1) * NX + i] + (trial ? d[(k + 1) * NZ + i] : 0.0)));
    }
    if (t < NX) c += fabs(X[t] + (trial ? d[t] : 0.0) - a.xmeas[(size_t)b * NX + t]);
    f = block_sum128(f, red); v = block_sum128(v, red); c = block_sum128(c, red); dm = block_max128(dm, red);
    if (t == 0) {
        int dec = 0;   // 0 retry the QP (same linearisation), 1 step accepted, 2 converged, 3 failed
        double w = S[0], kap = S[1], kap0 = S[2];
        const double f0 = S[3], c0 = S[4], v0 = S[5];
        if (!trial) {
            S[3] = f; S[4] = c; S[5] = v; S[1] = (v > 1e-7 || c > 1e-6) ? kap0 : 0.0;
            dec = -1;
        } else {
            const int qs = a.qp_status[b];
            const double phi0 = f0 + a.rho * (c0 + v0);
            double r = 0.0;
            if (!(qs == 0 || qs == 4)) {       // QP infeasible at this tau: ask for less
                if (kap < 0.995) { kap = 1.0 - 0.3 * (1.0 - kap); dec = 0; } else dec = 3;
            } else {
                const double pred = phi0 - (f + a.rho * kap * (v0 + c0));     // linearised model: violation shrinks to kappa * (v0 + c0)
                const double act = phi0 - (f + a.rho * (c + v));
                r = pred > 0.0 ? act / pred : -1.0;
                if (pred <= 1e-12 * fmax(1.0, fabs(phi0)) || dm < a.tol) dec = (v0 < 1e-7 && c0 < 1e-7)   /* l1 sums; the QP's own 1e-10 pads on every bound add up to ~1e-9 */ ? 2 : 1;
                else if (r < 0.1) { w *= 4.0; kap = 1.0 - (1.0 - kap) / 3.0; dec = (w > a.w_max) ? 3 : 0; }
                else { dec = 1; kap0 = kap; if (r > 0.7) { w = fmax(w / 3.0, 1e-6); kap0 = kap > 0.01 ? kap / 3.0 : 0.0; } }
            }
            S[6] = r; S[7] = dm;
            if (dec == 1 || dec == 2) {
                S[3] = f; S[4] = c; S[5] = v;
                kap = (v > 1e-7 || c > 1e-6) ? kap0 : 0.0;
                a.iters[b] += 1;
            }
            S[0] = w; S[1] = kap; S[2] = kap0;
            a.need_lin[b] = (dec == 1) ? 1 : 0;
            if (dec == 2) { a.status[b] = 0; a.active[b] = 0; }
            else if (dec == 3) { a.status[b] = 2; a.active[b] = 0; }
            else atomicAdd(a.n_active, 1);
        }
        dec_s = dec;
    }
    __syncthreads();
    if (dec_s == 1 || dec_s == 2) {
        for (int e = t; e < n; e += 128) {
            const int k = e / NZ, i = e % NZ;
            if (i < NX) X[k * NX + i] += d[e]; else U[k * NU + (i - NX)] += d[e];
        }
    }
