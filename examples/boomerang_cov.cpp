// boomerang_cov -- the covariance of a Boomerang path kept on the device, through the C++ mirror (include/pdmp_mi355.hpp):
//   pdmp(∇ϕ!, 0.0, x0, θ0, T, c, Boomerang(I, μ, 0.5); adapt=true) on the Gaussian target Γt = 1.2 I about μ (test/maintest.jl:139-154 in small),
// with Options::consume and the pair list of the lower triangle: every slice of the trace adds its arcs to S_ij = ∫ (x_i − c_i)(x_j − c_j) dt
// and J_i = ∫ (x_i − c_i) dt before the buffer of 48 events is recycled.  Usage: boomerang_cov d T seed
// Prints: d, events, num, an FNV-1a of the trace (t, x, θ), an FNV-1a of (S, J, T_last), and the largest |cov_ij − (Γt⁻¹)_ij| of the pairs.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "pdmp_mi355.hpp"

static uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t k = 0; k < n; ++k) h = (h ^ b[k]) * 1099511628211ull;
    return h;
}

int main(int argc, char** argv) {
    const int64_t d = argc > 1 ? std::atoll(argv[1]) : 8;
    const double T = argc > 2 ? std::atof(argv[2]) : 200.0;
    const uint64_t seed = argc > 3 ? std::strtoull(argv[3], nullptr, 0) : 7;
    try {
        pdmp::GaussianTarget target;  // Γt = 1.2 I, μt = μ
        target.Gamma.n = d;
        pdmp::Boomerang B;
        B.lambda_ref = 0.5;
        std::vector<double> x0((size_t)d), th0((size_t)d);
        pdmp::Options o;
        for (int64_t k = 0; k < d; ++k) {
            target.Gamma.colptr.push_back(k);
            target.Gamma.rowval.push_back(k);
            target.Gamma.nzval.push_back(1.2);
            B.mu.push_back(0.125 + 0.0625 * (double)k);
            x0[(size_t)k] = B.mu[(size_t)k] + 0.25 * (double)(k % 3 - 1);
            th0[(size_t)k] = (k % 2) ? -0.75 : 1.25;
            o.cov_center.push_back(0.03125 * (double)k - 0.0625);
            for (int64_t j = 0; j <= k; ++j) {  // the lower triangle, row by row
                o.cov_pi.push_back(k);
                o.cov_pj.push_back(j);
            }
        }
        target.Gamma.colptr.push_back(d);
        target.mu = B.mu;
        o.adapt = true;
        o.seed = seed;
        o.trace_capacity = 48;  // (drained and continued several times)
        o.consume = true;
        const auto R = pdmp::pdmp(target, 0.0, x0, th0, T, 3.0, B, o);
        uint64_t h = 14695981039346656037ull, g = h;
        h = fnv1a(h, R.trace.t.data(), R.trace.t.size() * sizeof(double));
        h = fnv1a(h, R.trace.x.data(), R.trace.x.size() * sizeof(double));
        h = fnv1a(h, R.trace.theta.data(), R.trace.theta.size() * sizeof(double));
        g = fnv1a(g, R.pairs.S.data(), R.pairs.S.size() * sizeof(double));
        g = fnv1a(g, R.pairs.J.data(), R.pairs.J.size() * sizeof(double));
        g = fnv1a(g, &R.pairs.T, sizeof(double));
        const double L = R.pairs.T;  // t0 = 0
        double worst = 0.0;
        for (size_t k = 0; k < o.cov_pi.size(); ++k) {
            const int64_t i = o.cov_pi[k], j = o.cov_pj[k];
            const double cov = R.pairs.S[k] / L - (R.pairs.J[(size_t)i] / L) * (R.pairs.J[(size_t)j] / L);
            worst = std::fmax(worst, std::fabs(cov - (i == j ? 1.0 / 1.2 : 0.0)));
        }
        std::printf("%lld %zu %lld %016llx %016llx %.17g\n", (long long)d, R.trace.t.size(), (long long)R.num, (unsigned long long)h,
                    (unsigned long long)g, worst);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "boomerang_cov: %s\n", ex.what());
        return 1;
    }
    return 0;
}
