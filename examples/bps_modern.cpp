// bps_modern -- the speed-recorded Bouncy Particle through the C++ mirror (include/pdmp_mi355.hpp):
//   pdmp(dϕ, ∇ϕ!, t0, x0, θ0, n, LocalBound(c), BouncyParticle(missing, missing, λref, ρ, U, L); oscn)   src/not_fact_samplers.jl:336-384
// on a tridiagonal Gaussian target.  Usage: bps_modern d n seed [u|oscn]
// Prints: d, records, num, acc, an FNV-1a of every record (t, x, θ) and of the final (t, x, θ, c), the last record's time.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "pdmp_mi355.hpp"

static uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t k = 0; k < n; ++k) h = (h ^ b[k]) * 1099511628211ull;
    return h;
}

int main(int argc, char** argv) {
    const int64_t d = argc > 1 ? std::atoll(argv[1]) : 100;
    const int64_t n = argc > 2 ? std::atoll(argv[2]) : 40;
    const uint64_t seed = argc > 3 ? std::strtoull(argv[3], nullptr, 0) : 7;
    const std::string mode = argc > 4 ? argv[4] : "";
    try {
        pdmp::GaussianTarget target;
        target.Gamma.n = d;
        target.Gamma.colptr.push_back(0);
        for (int64_t j = 0; j < d; ++j) {
            for (int64_t r = std::max<int64_t>(j - 1, 0); r <= std::min<int64_t>(j + 1, d - 1); ++r) {
                target.Gamma.rowval.push_back(r);
                target.Gamma.nzval.push_back(r == j ? 2.0 + 0.125 * (double)(j % 5) : -0.5);
            }
            target.Gamma.colptr.push_back((int64_t)target.Gamma.rowval.size());
        }
        std::vector<double> x0((size_t)d), th0((size_t)d);
        for (int64_t k = 0; k < d; ++k) {
            x0[(size_t)k] = (double)((k * 37) % 101) / 50.0 - 1.0;
            th0[(size_t)k] = (k % 3 == 0) ? -1.0 : 0.75;
        }
        pdmp::BouncyParticle B;
        B.lambda_ref = 1.0;
        B.rho = 0.9;
        if (mode == "u")
            for (int64_t k = 0; k < d; ++k) B.U.push_back(0.5 + 0.25 * (double)(k % 7));
        pdmp::Options o;
        o.seed = seed;
        o.oscn = mode == "oscn";
        o.trace_capacity = 16;  // (drained and continued several times)
        const auto R = pdmp::pdmp(target, 0.0, x0, th0, n, pdmp::LocalBound{5.0}, B, o);
        uint64_t h = 14695981039346656037ull;
        h = fnv1a(h, R.trace.t.data(), R.trace.t.size() * sizeof(double));
        h = fnv1a(h, R.trace.x.data(), R.trace.x.size() * sizeof(double));
        h = fnv1a(h, R.trace.theta.data(), R.trace.theta.size() * sizeof(double));
        h = fnv1a(h, R.t.data(), sizeof(double));
        h = fnv1a(h, R.x.data(), R.x.size() * sizeof(double));
        h = fnv1a(h, R.theta.data(), R.theta.size() * sizeof(double));
        h = fnv1a(h, R.c.data(), sizeof(double));
        std::printf("%lld %zu %lld %lld %016llx %.17g\n", (long long)d, R.trace.t.size(), (long long)R.num, (long long)R.acc[0],
                    (unsigned long long)h, R.trace.t.empty() ? 0.0 : R.trace.t.back());
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "bps_modern: %s\n", ex.what());
        return 1;
    }
    return 0;
}
