// stickyzz_box -- the ZigZag with sticky and reflecting barriers through the C++ mirror (include/pdmp_mi355.hpp):
//   stickyzz(u0, target, StickyFlow(ZigZag(0.9Γ, 0)), StickyUpperBounds(G, G1, 0.9Γ, c), barriers, EndTime(T))   src/stickyzz.jl:176-218
// on a tridiagonal Gaussian target inside the box [-1, 0.5]^d: reflecting walls (κ = Inf) on the even coordinates, a sticky floor (κ = 0.8)
// under a reflecting ceiling (κ = 5) on the odd ones.  Usage: stickyzz_box d T seed
// Prints: d, events, num, acc, frozen coordinates at the end, an FNV-1a of every event (t, i, x, θ) and of the final (t, x, θ, saved speeds), t′.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "pdmp_mi355.hpp"

static uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t k = 0; k < n; ++k) h = (h ^ b[k]) * 1099511628211ull;
    return h;
}

int main(int argc, char** argv) {
    const int64_t d = argc > 1 ? std::atoll(argv[1]) : 16;
    const double T = argc > 2 ? std::atof(argv[2]) : 50.0;
    const uint64_t seed = argc > 3 ? std::strtoull(argv[3], nullptr, 0) : 7;
    try {
        pdmp::GaussianTarget target;
        pdmp::ZigZag F;
        target.Gamma.n = F.Gamma.n = d;
        target.Gamma.colptr.push_back(0);
        for (int64_t j = 0; j < d; ++j) {
            for (int64_t r = std::max<int64_t>(j - 1, 0); r <= std::min<int64_t>(j + 1, d - 1); ++r) {
                target.Gamma.rowval.push_back(r);
                target.Gamma.nzval.push_back(r == j ? 2.0 + 0.125 * (double)(j % 5) : -0.5);
            }
            target.Gamma.colptr.push_back((int64_t)target.Gamma.rowval.size());
        }
        F.Gamma = target.Gamma;
        for (double& v : F.Gamma.nzval) v *= 0.9;
        F.mu.assign((size_t)d, 0.0);
        F.sigma.assign((size_t)d, 1.0);
        std::vector<double> x0((size_t)d), th0((size_t)d), c((size_t)d);
        std::vector<pdmp::Barrier> barriers((size_t)d);
        for (int64_t k = 0; k < d; ++k) {
            x0[(size_t)k] = (double)((k * 37) % 101) / 100.0 - 0.75;  // inside (-1, 0.5)
            th0[(size_t)k] = (k % 3 == 0) ? -1.0 : 0.75;
            c[(size_t)k] = 2.0;
            pdmp::Barrier& b = barriers[(size_t)k];
            b.lo = -1.0;
            b.hi = 0.5;
            if (k % 2 == 1) {
                b.rule_lo = PDMP_BARRIER_STICKY;
                b.kappa_lo = 0.8;
                b.kappa_hi = 5.0;
            }
        }
        pdmp::Options o;
        o.seed = seed;
        o.trace_capacity = 64;  // (drained and continued several times)
        const auto R = pdmp::stickyzz(target, 0.0, x0, th0, T, c, F, barriers, o);
        uint64_t h = 14695981039346656037ull;
        h = fnv1a(h, R.trace.events.data(), R.trace.events.size() * sizeof(pdmp::Event));
        h = fnv1a(h, R.t.data(), R.t.size() * sizeof(double));
        h = fnv1a(h, R.x.data(), R.x.size() * sizeof(double));
        h = fnv1a(h, R.theta.data(), R.theta.size() * sizeof(double));
        h = fnv1a(h, R.theta_saved.data(), R.theta_saved.size() * sizeof(double));
        int64_t nfrozen = 0;
        for (uint8_t f : R.frozen) nfrozen += f;
        std::printf("%lld %zu %lld %lld %lld %016llx %.17g\n", (long long)d, R.trace.events.size(), (long long)R.num, (long long)R.acc[0],
                    (long long)nfrozen, (unsigned long long)h, R.t_prime);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "stickyzz_box: %s\n", ex.what());
        return 1;
    }
    return 0;
}
