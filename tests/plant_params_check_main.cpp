// Stand-alone host program (own main) around the validation routine of slsqp_cl_set_plant_params (csrc/plant_params.hpp: no HIP call in it), so
// that it can be built with -fsanitize=address,undefined and run without a GPU (tests/test_plant_params_cpu.py).  Heap buffers of exactly the
// documented sizes: P (np) and (B, np).
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../robust-nonlinear-mpc_amd/csrc/plant_params.hpp"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

int main() {
    namespace pp = plant_params;
    EXPECT(pp::count(0) == 4 && pp::count(1) == 7 && pp::count(2) == 13 && pp::count(3) == -1 && pp::count(-1) == -1);
    EXPECT(dyn::NP_MAX == 13);
    for (int m = 0; m < 3; m++) {
        const int np = pp::count(m);
        EXPECT(pp::name(m, -1) == nullptr && pp::name(m, np) == nullptr);
        std::string why;
        for (int B : {1, 5}) {
            std::vector<double> P((size_t)B * np);
            for (int b = 0; b < B; b++) for (int i = 0; i < np; i++) P[(size_t)b * np + i] = pp::default_value(m, i) * (1.0 + 0.01 * b);
            EXPECT(pp::check(m, P.data(), B, np, &why));
            EXPECT(pp::check(m, P.data(), B, np, nullptr));
            EXPECT(!pp::check(m, P.data(), B, np + 1, &why) && why.find("np") != std::string::npos);
            EXPECT(!pp::check(m, P.data(), B, np - 1, &why));
            for (int i = 0; i < np; i++) {      // the last row's entry i: NaN, infinite, zero, negative
                double &v = P[(size_t)(B - 1) * np + i];
                const double keep = v;
                v = NAN; EXPECT(!pp::check(m, P.data(), B, np, &why) && why.find("NaN") != std::string::npos && why.find(pp::name(m, i)) != std::string::npos);
                v = INFINITY; EXPECT(!pp::check(m, P.data(), B, np, &why));
                v = -INFINITY; EXPECT(!pp::check(m, P.data(), B, np, &why));
                const bool pos = pp::must_be_positive(m, i);
                v = 0.0; EXPECT(pp::check(m, P.data(), B, np, &why) == !pos);
                v = -keep; EXPECT(pp::check(m, P.data(), B, np, &why) == !pos);
                if (pos) EXPECT(why.find("> 0") != std::string::npos && why.find(pp::name(m, i)) != std::string::npos);
                v = keep;
            }
            EXPECT(pp::check(m, P.data(), B, np, &why));
        }
    }
    EXPECT(!pp::must_be_positive(1, 6) && std::string(pp::name(1, 6)) == "kM");
    std::string why;
    EXPECT(!pp::check(-1, nullptr, 0, 4, &why) && why.find("model") != std::string::npos);
    if (fails) return 1;
    std::printf("plant_params_check ok\n");
    return 0;
}
