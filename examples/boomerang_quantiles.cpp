// boomerang_quantiles -- medians and a 90 % interval of a Boomerang path from marginal histograms kept on the device, through the C++ mirror
// (include/pdmp_mi355.hpp):
//   pdmp(∇ϕ!, 0.0, x0, θ0, T, c, Boomerang(I, μ, 0.5); adapt=true) on the Gaussian target Γt = 1.2 I about μ (test/maintest.jl:139-154 in small),
// with Options::consume and hist_bins = 64 on [μ_i − 5, μ_i + 5): every slice of the trace adds the exact time its arcs spend in each bin before
// the buffer of 48 events is recycled.  flow = 1 runs a BouncyParticle(I, μ, 0.5) on the same target instead (c = 1e-3): lines, the same rows.
// Usage: boomerang_quantiles d T seed flow
// Prints: d, events, num, an FNV-1a of the trace (t, x, θ), an FNV-1a of (H, Z, T_last), then per coordinate the 5 %, 50 % and 95 % quantiles.
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
    const int flow = argc > 4 ? std::atoi(argv[4]) : 0;
    try {
        pdmp::GaussianTarget target;  // Γt = 1.2 I, μt = μ
        target.Gamma.n = d;
        std::vector<double> mu, x0((size_t)d), th0((size_t)d);
        pdmp::Options o;
        for (int64_t k = 0; k < d; ++k) {
            target.Gamma.colptr.push_back(k);
            target.Gamma.rowval.push_back(k);
            target.Gamma.nzval.push_back(1.2);
            mu.push_back(0.125 + 0.0625 * (double)k);
            x0[(size_t)k] = mu[(size_t)k] + 0.25 * (double)(k % 3 - 1);
            th0[(size_t)k] = (k % 2) ? -0.75 : 1.25;
            o.hist_lo.push_back(mu[(size_t)k] - 5.0);
            o.hist_hi.push_back(mu[(size_t)k] + 5.0);
        }
        target.Gamma.colptr.push_back(d);
        target.mu = mu;
        o.hist_bins = 64;  // (hist_coords empty: every coordinate)
        o.adapt = true;
        o.seed = seed;
        o.trace_capacity = 48;  // (drained and continued several times)
        o.consume = true;
        pdmp::Result<pdmp::PDMPTrace> R;
        if (flow == 0) {
            pdmp::Boomerang B;
            B.lambda_ref = 0.5;
            B.mu = mu;
            R = pdmp::pdmp(target, 0.0, x0, th0, T, 3.0, B, o);
        } else {
            pdmp::BouncyParticle B;
            B.Gamma = target.Gamma;  // (the flow's Γ = I: the identity mass)
            for (double& v : B.Gamma.nzval) v = 1.0;
            B.mu = mu;
            B.lambda_ref = 0.5;
            R = pdmp::pdmp(target, 0.0, x0, th0, T, 1e-3, B, o);
        }
        uint64_t h = 14695981039346656037ull, g = h;
        h = fnv1a(h, R.trace.t.data(), R.trace.t.size() * sizeof(double));
        h = fnv1a(h, R.trace.x.data(), R.trace.x.size() * sizeof(double));
        h = fnv1a(h, R.trace.theta.data(), R.trace.theta.size() * sizeof(double));
        g = fnv1a(g, R.hist.H.data(), R.hist.H.size() * sizeof(double));
        g = fnv1a(g, R.hist.Z.data(), R.hist.Z.size() * sizeof(double));
        g = fnv1a(g, &R.hist.T, sizeof(double));
        std::printf("%lld %zu %lld %016llx %016llx\n", (long long)d, R.trace.t.size(), (long long)R.num, (unsigned long long)h, (unsigned long long)g);
        for (size_t s = 0; s < R.hist.coords.size(); ++s)
            std::printf("%lld %.17g %.17g %.17g\n", (long long)R.hist.coords[s], R.hist.quantile(s, 0.05), R.hist.quantile(s, 0.5), R.hist.quantile(s, 0.95));
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "boomerang_quantiles: %s\n", ex.what());
        return 1;
    }
    return 0;
}
