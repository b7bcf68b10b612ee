// user_bs_gpu<nparts, 2, 2>::getModelExpectations() (include/ssme_gpu/bsfilter_gpu.hpp): the functionals that the model's header
// declares (tests/models/svol_two_factor_h.h: n_h = 7), summed on the device, against the same object's filter(y, fs) with the same
// seven functions as host std::functions.  Linked against the library built with that header.  Prints "name value" lines that
// tests/test_user_functionals_gpu.py compares; scale_k = E|h_k|, what an error of a sign-changing functional is measured against.
#include <array>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/ssme_gpu/bsfilter_gpu.hpp"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::vector<double> spy;
    {
        std::ifstream f(argv[1]);
        std::string line;
        while (std::getline(f, line)) if (!line.empty()) spy.push_back(std::stod(line));
    }
    constexpr std::size_t N = 3000;
    using model = ssme_gpu::user_bs_gpu<N, 2, 2>;
    using sv = model::state_vector;
    ssme_gpu::gpu_options o;
    o.seed = 21;
    model mod({1.1, 0.95, 0.9, 0.2, 0.15, -0.4}, o, /*filter_id=*/1);
    std::vector<model::func> fs = {
        [](const sv& x) { return x[0]; },
        [](const sv& x) { return x[1]; },
        [](const sv& x) { return x[0] * x[0]; },
        [](const sv& x) { return x[0] * x[1]; },
        [](const sv& x) { return x[1] * x[1]; },
        [](const sv& x) { return std::exp(0.5 * (x[0] + x[1])); },
        [](const sv&) { return 0.0 + 1.0; }};                      // filter(y) has no covariate: z = 0
    const std::size_t nf = fs.size();
    for (std::size_t k = 0; k < nf; ++k) fs.push_back([f = fs[k]](const sv& x) { return std::fabs(f(x)); });
    const int T = 6;
    for (int t = 0; t < T; ++t) {
        const std::array<double, 2> y = {spy[t], spy[100 + t]};
        if (t == T - 1) mod.filter(y, fs); else mod.filter(y);
    }
    std::printf("n_h %d\n", ssme_pf_user_model_n_h());
    const std::vector<double> dev = mod.getModelExpectations(), again = mod.getModelExpectations();
    if (dev.size() != nf) return 3;
    for (std::size_t k = 0; k < nf; ++k) {
        std::printf("dev_%zu %.17g\n", k, dev[k]);
        std::printf("host_%zu %.17g\n", k, mod.getExpectations()[k]);
        std::printf("scale_%zu %.17g\n", k, mod.getExpectations()[nf + k]);
    }
    std::printf("repeat %s\n", dev == again ? "same" : "different");
    return 0;
}
