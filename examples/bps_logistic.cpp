// bps_logistic -- the speed-recorded Bouncy Particle on a Bayesian logistic regression through the C++ mirror (include/pdmp_mi355.hpp):
//   pdmp(dϕ, ∇ϕ!, t0, x0, θ0, nrec, LocalBound(c), BouncyParticle(missing, missing, λref, ρ, U, L); oscn, adapt)   src/not_fact_samplers.jl:336-384
// with dϕ, ∇ϕ! of ϕ(x) = Σ_i [m_i log(1 + e^{η_i}) − y_i η_i] + (γ0/2)‖x‖², η = A x (pdmp::LogisticRegression).
// The data set is a function of the arguments: observation i has entries in the columns i % d, (3i + 1) % d and (7i + 2) % d (those that
// differ), A[i, j] = ((13 i + 7 j) % 11 − 5) / 8, m_i = 1 + i % 3, y_i = 5 i % (m_i + 1), γ0 = 0.5.
// Usage: bps_logistic d n nrec seed [u|oscn]
// Prints: d, n, records, num, acc, an FNV-1a of every record (t, x, θ) and of the final (t, x, θ, c), the last record's time.
#include <algorithm>
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
    const int64_t n = argc > 2 ? std::atoll(argv[2]) : 130;
    const int64_t nrec = argc > 3 ? std::atoll(argv[3]) : 40;
    const uint64_t seed = argc > 4 ? std::strtoull(argv[4], nullptr, 0) : 7;
    const std::string mode = argc > 5 ? argv[5] : "";
    try {
        pdmp::LogisticRegression target;
        target.n = n;
        target.gamma0 = 0.5;
        // At first (column = observation, coordinates ascending), then A by a counting pass over it
        target.At.n = n;
        target.At.colptr.push_back(0);
        for (int64_t i = 0; i < n; ++i) {
            int64_t cols[3] = {i % d, (3 * i + 1) % d, (7 * i + 2) % d};
            std::sort(cols, cols + 3);
            const int64_t k = std::unique(cols, cols + 3) - cols;
            for (int64_t q = 0; q < k; ++q) {
                target.At.rowval.push_back(cols[q]);
                target.At.nzval.push_back((double)((13 * i + 7 * cols[q]) % 11 - 5) / 8.0);
            }
            target.At.colptr.push_back((int64_t)target.At.rowval.size());
            const int64_t m = 1 + i % 3;
            target.m.push_back((double)m);
            target.y.push_back((double)((5 * i) % (m + 1)));
        }
        const int64_t nnz = (int64_t)target.At.rowval.size();
        target.A.n = d;
        target.A.colptr.assign((size_t)d + 1, 0);
        target.A.rowval.resize((size_t)nnz);
        target.A.nzval.resize((size_t)nnz);
        for (int64_t q = 0; q < nnz; ++q) target.A.colptr[(size_t)target.At.rowval[(size_t)q] + 1]++;
        for (int64_t j = 0; j < d; ++j) target.A.colptr[(size_t)j + 1] += target.A.colptr[(size_t)j];
        std::vector<int64_t> fill(target.A.colptr.begin(), target.A.colptr.end() - 1);
        for (int64_t i = 0; i < n; ++i)
            for (int64_t q = target.At.colptr[(size_t)i]; q < target.At.colptr[(size_t)i + 1]; ++q) {
                const int64_t s = fill[(size_t)target.At.rowval[(size_t)q]]++;
                target.A.rowval[(size_t)s] = i;
                target.A.nzval[(size_t)s] = target.At.nzval[(size_t)q];
            }
        std::vector<double> x0((size_t)d), th0((size_t)d);
        for (int64_t k = 0; k < d; ++k) {
            x0[(size_t)k] = ((double)((k * 37) % 101) / 50.0 - 1.0) / 4.0;
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
        o.adapt = true;
        o.trace_capacity = 16;  // (drained and continued several times)
        const auto R = pdmp::pdmp(target, 0.0, x0, th0, nrec, pdmp::LocalBound{30.0}, B, o);
        uint64_t h = 14695981039346656037ull;
        h = fnv1a(h, R.trace.t.data(), R.trace.t.size() * sizeof(double));
        h = fnv1a(h, R.trace.x.data(), R.trace.x.size() * sizeof(double));
        h = fnv1a(h, R.trace.theta.data(), R.trace.theta.size() * sizeof(double));
        h = fnv1a(h, R.t.data(), sizeof(double));
        h = fnv1a(h, R.x.data(), R.x.size() * sizeof(double));
        h = fnv1a(h, R.theta.data(), R.theta.size() * sizeof(double));
        h = fnv1a(h, R.c.data(), sizeof(double));
        std::printf("%lld %lld %zu %lld %lld %016llx %.17g\n", (long long)d, (long long)n, R.trace.t.size(), (long long)R.num, (long long)R.acc[0],
                    (unsigned long long)h, R.trace.t.empty() ? 0.0 : R.trace.t.back());
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "bps_logistic: %s\n", ex.what());
        return 1;
    }
    return 0;
}
