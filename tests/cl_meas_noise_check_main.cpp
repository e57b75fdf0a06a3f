// Stand-alone host program (own main) around the measurement-noise rule of the closed loops (csrc/cl_meas.hpp), built by
// tests/test_meas_noise_cpu.py with -fsanitize=address,undefined.  No GPU, no HIP call: the header has none.
//   no argument:
//     1. the setter's validation, refusal by refusal, each message naming its argument;
//     2. the row selection with the held last row, shared and per-instance strides, on heap buffers of exactly (T,nx) and (B,T,nx) doubles (a read past
//        either end is the sanitizer's to report);
//     3. the two halves of the rule around a stand-in plant step, with a log of fewer entries than steps (heap buffers of exactly (B,S,nx)).
//   shim IN OUT: for tests/test_meas_noise_cpu.py -- IN holds doubles [B, nx, T, per_instance, S, steps, table, x0 (B,nx), deltas (steps,B,nx)]; OUT
//     receives x_plant (B,nx), x_meas (B,nx), the log of the truth (B,S,nx) and of the measurement (B,S,nx) after `steps` steps x <- x + delta.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../robust-nonlinear-mpc_amd/csrc/cl_meas.hpp"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static const double INF = std::numeric_limits<double>::infinity(), NaN = std::numeric_limits<double>::quiet_NaN();
namespace mn = cl_meas;

static bool refused(const double *Nm, int T, int per, int loc, bool model, int B, int nx, const char *word) {
    std::string why;
    if (mn::check(Nm, T, per, loc, model, B, nx, &why) && (T == 0 || mn::check_entries(Nm, T, per, B, nx, &why))) return false;
    if (why.find(word) == std::string::npos) { std::printf("message \"%s\" does not name \"%s\"\n", why.c_str(), word); return false; }
    return true;
}

static void check_validation() {
    const int B = 3, nx = 2, T = 2;
    std::unique_ptr<double[]> sh(new double[T * nx]), pi(new double[B * T * nx]);      // exactly (T,nx) and (B,T,nx)
    for (int i = 0; i < T * nx; i++) sh[i] = 1e-3 * i;
    for (int i = 0; i < B * T * nx; i++) pi[i] = -1e-3 * i;
    std::string why;
    EXPECT(mn::check(sh.get(), T, 0, 0, true, B, nx, &why) && mn::check_entries(sh.get(), T, 0, B, nx, &why));
    EXPECT(mn::check(pi.get(), T, 1, 1, true, B, nx, &why) && mn::check_entries(pi.get(), T, 1, B, nx, &why));
    EXPECT(mn::check(nullptr, 0, 0, 0, true, B, nx, &why));      // clears
    EXPECT(mn::check(nullptr, 0, 1, 1, true, B, nx, nullptr));      // (no message asked for)
    EXPECT(refused(sh.get(), -1, 0, 0, true, B, nx, "T = -1"));
    EXPECT(refused(sh.get(), 0, 0, 0, true, B, nx, "T = 0"));
    EXPECT(refused(nullptr, 2, 0, 0, true, B, nx, "Nm is NULL"));
    EXPECT(refused(sh.get(), T, 2, 0, true, B, nx, "per_instance = 2"));
    EXPECT(refused(sh.get(), T, -1, 0, true, B, nx, "per_instance = -1"));
    EXPECT(refused(sh.get(), T, 0, 2, true, B, nx, "loc = 2"));
    EXPECT(refused(sh.get(), T, 0, -1, true, B, nx, "loc = -1"));
    EXPECT(refused(sh.get(), T, 0, 0, false, B, nx, "slsqp_set_model"));
    EXPECT(refused(nullptr, 0, 0, 0, false, B, nx, "slsqp_set_model"));
    for (double bad : {NaN, INF, -INF}) {
        pi[B * T * nx - 1] = bad;      // the very last entry of the per-instance table
        EXPECT(refused(pi.get(), T, 1, 0, true, B, nx, "NaN or infinite"));
        pi[B * T * nx - 1] = 0.0;
        sh[0] = bad;
        EXPECT(refused(sh.get(), T, 0, 0, true, B, nx, "NaN or infinite"));
        sh[0] = 0.0;
    }
    EXPECT(mn::check_entries(sh.get(), T, 0, B, nx, nullptr));
}

static void check_rows() {
    EXPECT(mn::row_index(-1, 3) == 0 && mn::row_index(0, 3) == 0 && mn::row_index(1, 3) == 1 && mn::row_index(2, 3) == 2 && mn::row_index(3, 3) == 2 && mn::row_index(1000, 3) == 2);
    EXPECT(mn::row_index(0, 1) == 0 && mn::row_index(7, 1) == 0);
    const int B = 3, nx = 2, T = 2;
    std::unique_ptr<double[]> sh(new double[T * nx]), pi(new double[B * T * nx]);
    for (int i = 0; i < T * nx; i++) sh[i] = i;
    for (int i = 0; i < B * T * nx; i++) pi[i] = 100 + i;
    mn::Args a;
    std::memset(&a, 0, sizeof a);
    EXPECT(!mn::on(a));
    a.rows = sh.get(); a.T = T; a.stride = 0;
    EXPECT(mn::on(a));
    for (int b = 0; b < B; b++) {
        EXPECT(mn::row_at(a, nx, b, 0) == sh.get() && mn::row_at(a, nx, b, 1) == sh.get() + nx && mn::row_at(a, nx, b, 5) == sh.get() + nx);
        EXPECT(mn::row_at(a, nx, b, 9)[nx - 1] == T * nx - 1);      // the last double of the buffer
    }
    a.rows = pi.get(); a.stride = (size_t)T * nx;
    for (int b = 0; b < B; b++)
        for (int s = 0; s < 4; s++) EXPECT(mn::row_at(a, nx, b, s)[1] == 100 + (b * T + (s < T ? s : T - 1)) * nx + 1);
    EXPECT(mn::measure(0.1, 0.2) == 0.1 + 0.2 && mn::measure(1.0, -0.0) == 1.0);
}

// `steps` steps of x <- x + delta between the two halves of the rule, as the closed loops call them; every buffer on the heap at its exact size
struct Sim { std::vector<double> xp, xm, lp, lm; };
static Sim simulate(int B, int nx, int T, int per, int S, int steps, const double *table, const double *x0, const double *deltas) {
    const size_t nt = (size_t)(per ? B : 1) * T * nx, nl = (size_t)B * S * nx;
    std::unique_ptr<double[]> tab(new double[nt]), xp(new double[B * nx]), xm(new double[B * nx]), lp(new double[nl ? nl : 1]), lm(new double[nl ? nl : 1]);      // (exactly (B,S,nx) where there is a log)
    std::memcpy(tab.get(), table, sizeof(double) * nt);
    for (size_t i = 0; i < (size_t)B * S * nx; i++) lp[i] = lm[i] = -777.0;
    for (int i = 0; i < B * nx; i++) { xp[i] = -1.0; xm[i] = x0[i]; }
    mn::Args a;
    std::memset(&a, 0, sizeof a);
    a.rows = tab.get(); a.T = T; a.S = S; a.stride = per ? (size_t)T * nx : 0; a.x_plant = xp.get();
    a.lg_plant = S ? lp.get() : nullptr; a.lg_meas = S ? lm.get() : nullptr;
    for (int b = 0; b < B; b++) mn::post(a, nx, b, -1, xm.get() + (size_t)b * nx);      // slsqp_cl_init
    for (int s = 0; s < steps; s++)
        for (int b = 0; b < B; b++) {
            double *x = xm.get() + (size_t)b * nx;
            mn::pre(a, nx, b, s, x);
            for (int i = 0; i < nx; i++) x[i] = x[i] + deltas[((size_t)s * B + b) * nx + i];      // the plant step reads and writes x_meas
            mn::post(a, nx, b, s, x);
        }
    Sim r;
    r.xp.assign(xp.get(), xp.get() + B * nx); r.xm.assign(xm.get(), xm.get() + B * nx);
    r.lp.assign(lp.get(), lp.get() + (size_t)B * S * nx); r.lm.assign(lm.get(), lm.get() + (size_t)B * S * nx);
    return r;
}

static void check_rule() {
    const int B = 2, nx = 2, T = 2, S = 2, steps = 4;      // the log is shorter than the run
    const double tab[B * T * nx] = {0.25, -0.5, 0.125, 1.0, /* instance 1 */ -0.25, 0.5, 2.0, -1.0};
    const double x0[B * nx] = {1.0, 2.0, 3.0, 4.0};
    std::vector<double> d((size_t)steps * B * nx);
    for (size_t i = 0; i < d.size(); i++) d[i] = 0.5 * (double)(i % 5) - 1.0;
    const Sim r = simulate(B, nx, T, 1, S, steps, tab, x0, d.data());
    for (int b = 0; b < B; b++)
        for (int i = 0; i < nx; i++) {
            double x = x0[b * nx + i];
            for (int s = 0; s < steps; s++) {
                if (s < S) {
                    EXPECT(r.lp[((size_t)b * S + s) * nx + i] == x);
                    EXPECT(r.lm[((size_t)b * S + s) * nx + i] == x + tab[(b * T + (s < T ? s : T - 1)) * nx + i]);
                }
                x += d[((size_t)s * B + b) * nx + i];
            }
            EXPECT(r.xp[b * nx + i] == x && r.xm[b * nx + i] == x + tab[(b * T + T - 1) * nx + i]);
        }
    const Sim q = simulate(B, nx, 1, 0, 0, steps, tab, x0, d.data());      // a shared constant bias, no log
    for (int b = 0; b < B; b++)
        for (int i = 0; i < nx; i++) EXPECT(q.xm[b * nx + i] == q.xp[b * nx + i] + tab[i]);
    EXPECT(q.lp.empty() && q.lm.empty());
}

static int shim(const char *fin, const char *fout) {
    std::FILE *f = std::fopen(fin, "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<double> in((size_t)bytes / sizeof(double));
    if (std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) { std::fclose(f); return 2; }
    std::fclose(f);
    if (in.size() < 6) return 2;
    const int B = (int)in[0], nx = (int)in[1], T = (int)in[2], per = (int)in[3], S = (int)in[4], steps = (int)in[5];
    const size_t nt = (size_t)(per ? B : 1) * T * nx;
    if (in.size() != 6 + nt + (size_t)B * nx + (size_t)steps * B * nx) return 3;
    const Sim r = simulate(B, nx, T, per, S, steps, in.data() + 6, in.data() + 6 + nt, in.data() + 6 + nt + (size_t)B * nx);
    std::FILE *g = std::fopen(fout, "wb");
    if (!g) return 2;
    for (const std::vector<double> *v : {&r.xp, &r.xm, &r.lp, &r.lm}) std::fwrite(v->data(), sizeof(double), v->size(), g);
    std::fclose(g);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !std::strcmp(argv[1], "shim")) return shim(argv[2], argv[3]);
    check_validation();
    check_rows();
    check_rule();
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("cl_meas_noise_check ok\n");
    return 0;
}
