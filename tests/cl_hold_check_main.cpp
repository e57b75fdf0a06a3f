// Stand-alone check of csrc/cl_hold.hpp (the bookkeeping of slsqp_cl_hold_step: which hold step comes next, when the call is refused), built by
// tests/test_hold_cpu.py with -fsanitize=address,undefined.  The handle's step count is played by an int that moves as the entry points move it.
#include <cstdio>
#include <string>

#include "../robust-nonlinear-mpc_amd/csrc/cl_hold.hpp"

static int fails = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); fails++; } \
    } while (0)

struct Handle {
    cl_hold::State s;
    int cl_steps = 0, N;
    bool model = true;
    explicit Handle(int N_) : N(N_) {}
    void init() { cl_steps = 0; cl_hold::on_init(s); }
    void step() { cl_steps++; }                                              // slsqp_cl_step knows nothing of the hold state
    void run(int steps) { cl_steps = steps; cl_hold::on_run(s, cl_steps); }   // slsqp_cl_run / slsqp_cl_run_scp (they need cl_steps == 0)
    int hold(int loc = 0, std::string *why_out = nullptr) {                   // slsqp_cl_hold_step: the index it ran with, 0 = refused
        std::string why;
        const int before = cl_steps;
        const int k = cl_hold::next_index(s, model, cl_steps, N, loc, &why);
        if (why_out) *why_out = why;
        if (!k) { EXPECT(!why.empty()); EXPECT(cl_steps == before); return 0; }
        EXPECT(why.empty());
        cl_steps++;
        cl_hold::on_hold(s, k, cl_steps);
        return k;
    }
    int index() const { return cl_hold::index(s, cl_steps); }
};

int main() {
    std::string why;
    {   // before any solve; M = 3 in a loop; the index returns to 0 after every solve
        Handle h(4);
        h.init();
        EXPECT(h.hold(0, &why) == 0 && why.find("no slsqp_cl_step") != std::string::npos);
        EXPECT(h.index() == 0);
        for (int cycle = 0; cycle < 3; cycle++) {
            h.step();
            EXPECT(h.index() == 0);
            EXPECT(h.hold() == 1 && h.index() == 1);
            EXPECT(h.hold() == 2 && h.index() == 2);
        }
        EXPECT(h.cl_steps == 9);
    }
    {   // the N-th hold in a row: k = N - 1 is the last one
        Handle h(4);
        h.init(); h.step();
        EXPECT(h.hold() == 1 && h.hold() == 2 && h.hold() == 3);
        const cl_hold::State keep = h.s;
        EXPECT(h.hold(0, &why) == 0 && why.find("at most N - 1") != std::string::npos);
        EXPECT(h.s.k == keep.k && h.s.at_steps == keep.at_steps && h.index() == 3);
        h.step();
        EXPECT(h.index() == 0 && h.hold() == 1);
    }
    {   // N = 1 has no hold step at all; N = 2 exactly one
        Handle a(1), b(2);
        a.init(); a.step();
        EXPECT(a.hold() == 0);
        b.init(); b.step();
        EXPECT(b.hold() == 1 && b.hold() == 0);
    }
    {   // after a persistent run: refused until a slsqp_cl_step; slsqp_cl_init forgets the run
        Handle h(5);
        h.init(); h.run(7);
        EXPECT(h.hold(0, &why) == 0 && why.find("slsqp_cl_run") != std::string::npos);
        h.step();
        EXPECT(h.hold() == 1 && h.hold() == 2);
        h.init();
        EXPECT(h.hold() == 0);
        for (int i = 0; i < 7; i++) h.step();      // the same count as the run left, reached by solved steps
        EXPECT(h.hold() == 1);
    }
    {   // a run of one step (the count a single slsqp_cl_step would leave)
        Handle h(5);
        h.init(); h.run(1);
        EXPECT(h.hold() == 0);
    }
    {   // slsqp_cl_init in the middle of a hold sequence
        Handle h(6);
        h.init(); h.step(); h.step();
        EXPECT(h.hold() == 1 && h.hold() == 2);
        h.init();
        EXPECT(h.index() == 0 && h.hold() == 0);
        h.step(); h.step(); h.step(); h.step();      // back at the count the last hold left: still a fresh plan
        EXPECT(h.index() == 0 && h.hold() == 1);
    }
    {   // no model, loc outside {host, device}
        Handle h(4);
        h.init(); h.step();
        h.model = false;
        EXPECT(h.hold(0, &why) == 0 && why.find("slsqp_set_model") != std::string::npos);
        h.model = true;
        EXPECT(h.hold(2, &why) == 0 && why.find("loc") != std::string::npos);
        EXPECT(h.hold(-1) == 0);
        EXPECT(h.hold(1) == 1);
    }
    if (fails) { std::printf("cl_hold_check: %d failures\n", fails); return 1; }
    std::printf("cl_hold_check ok\n");
    return 0;
}
