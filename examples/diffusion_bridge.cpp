// diffusion_bridge -- the reference's diffusion-bridge example through the C++ mirror (include/pdmp_mi355.hpp):
//   spdmp(∇ϕmoving, 0.0, ξ0, θ0, T′, c, ZigZag(sparse(I), 0), SelfMoving(), L, T; adapt=true)   research/diffusion_bridge/diffbridge.jl:32-33
// the bridge of dX = (−0.1 X + 1.5 sin(2πX)) ds + dW from u = 1.5 at time 0 to v = −0.5 at time T = 2 in the Faber-Schauder basis up to level L
// (d = (2 << L) + 1 coefficients; the end points are fixed: θ0 = 0 and c = 0 there).  Usage: diffusion_bridge L T′ seed
// Prints: d, events, num, the accepted reflections, an FNV-1a of every event (t, i, x, θ) and of the final (t, ξ, θ, c), and the bridge at
// T/2 of the final coefficients (dotψ, faberschauder.jl:16-24).
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
    const int L = argc > 1 ? std::atoi(argv[1]) : 7;
    const double Tp = argc > 2 ? std::atof(argv[2]) : 20.0;
    const uint64_t seed = argc > 3 ? std::strtoull(argv[3], nullptr, 0) : 7;
    try {
        pdmp::DiffusionBridge target;
        target.L = L;
        const int64_t d = target.d();
        const double u = 1.5, v = -0.5;
        pdmp::ZigZag F;  // ZigZag(sparse(I), 0)
        F.Gamma.n = d;
        for (int64_t j = 0; j < d; ++j) {
            F.Gamma.colptr.push_back(j);
            F.Gamma.rowval.push_back(j);
            F.Gamma.nzval.push_back(1.0);
        }
        F.Gamma.colptr.push_back(d);
        F.mu.assign((size_t)d, 0.0);
        F.sigma.assign((size_t)d, 1.0);
        std::vector<double> xi0((size_t)d, 0.0), th0((size_t)d), c((size_t)d, 1.0);
        for (int64_t k = 0; k < d; ++k) th0[(size_t)k] = (k % 3 == 0) ? -1.0 : 1.0;
        xi0.front() = u / std::sqrt(target.T);
        xi0.back() = v / std::sqrt(target.T);
        th0.front() = th0.back() = 0.0;  // fix the end points, diffbridge.jl:23-26
        c.front() = c.back() = 0.0;
        pdmp::Options o;
        o.adapt = true;
        o.seed = seed;
        o.trace_capacity = 256;  // (drained and continued several times)
        const auto R = pdmp::spdmp(target, 0.0, xi0, th0, Tp, c, F, o);
        uint64_t h = 14695981039346656037ull;
        h = fnv1a(h, R.trace.events.data(), R.trace.events.size() * sizeof(pdmp::Event));
        h = fnv1a(h, R.t.data(), R.t.size() * sizeof(double));
        h = fnv1a(h, R.x.data(), R.x.size() * sizeof(double));
        h = fnv1a(h, R.theta.data(), R.theta.size() * sizeof(double));
        h = fnv1a(h, R.c.data(), R.c.size() * sizeof(double));
        int64_t acc = 0;
        for (int64_t a : R.acc) acc += a;
        std::printf("%lld %zu %lld %lld %016llx %.17g\n", (long long)d, R.trace.events.size(), (long long)R.num, (long long)acc,
                    (unsigned long long)h, target.path(R.x, target.T / 2));
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "diffusion_bridge: %s\n", ex.what());
        return 1;
    }
    return 0;
}
