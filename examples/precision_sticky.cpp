// precision_sticky -- the reference's precision case study through the C++ mirror (include/pdmp_mi355.hpp):
//   sspdmp(∇ϕ, t0, x0, θ0, T, c, G, ZigZag(Γ̂, μ̂), κ, YY, (𝕀, 𝕁), N; adapt=true)                     casestudies/precision/precision.jl:82
// learning a sparse precision matrix through its Cholesky factor: Γtrue = SymTridiagonal(1, −0.3), N observations Y_k ~ N(0, Γtrue⁻¹),
// YY = Y Yᵀ; the coordinates are the lower triangle of L packed column by column (d = n(n+1)/2).  The flow is centred at the per-column mode μ̂
// of the flat-prior posterior with the curvature γ̂ there on its diagonal; x0 = pack(Ltrue) + 0.01 z, θ0 = ±1, c = 10, κ = 0.01 (:59,64,70,79).
// Usage: precision_sticky n N T seed [dump-file]
// Prints: d, events, num, acc, an FNV-1a of every event (t, i, x, θ) and of the final (t, x, θ, c), ‖L̂L̂ᵀ − Γtrue‖_F of the posterior mean L̂, and
// the mean inclusion probability of the first, second and third sub-diagonal (the first carries the signal).  With a dump-file the inputs are
// written there as raw doubles -- n, N, then YY, γ̂, μ̂, x0, θ0 -- for another front end to run the same problem.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "pdmp_detmath.h"
#include "pdmp_mi355.hpp"

static uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t k = 0; k < n; ++k) h = (h ^ b[k]) * 1099511628211ull;
    return h;
}

// w = A⁻¹ e1 for the trailing block A = YY[c:, c:] (m = n − c), by a Cholesky factorisation of the block
static std::vector<double> first_column_of_inverse(const std::vector<double>& YY, int n, int c) {
    const int m = n - c;
    std::vector<double> L((size_t)m * m, 0.0), w((size_t)m, 0.0);
    for (int j = 0; j < m; ++j)
        for (int i = j; i < m; ++i) {
            double s = YY[(size_t)(c + i) * n + c + j];
            for (int k = 0; k < j; ++k) s -= L[(size_t)i * m + k] * L[(size_t)j * m + k];
            L[(size_t)i * m + j] = (i == j) ? std::sqrt(s) : s / L[(size_t)j * m + j];
        }
    for (int i = 0; i < m; ++i) {  // L z = e1
        double s = (i == 0) ? 1.0 : 0.0;
        for (int k = 0; k < i; ++k) s -= L[(size_t)i * m + k] * w[(size_t)k];
        w[(size_t)i] = s / L[(size_t)i * m + i];
    }
    for (int i = m - 1; i >= 0; --i) {  // Lᵀ w = z
        double s = w[(size_t)i];
        for (int k = i + 1; k < m; ++k) s -= L[(size_t)k * m + i] * w[(size_t)k];
        w[(size_t)i] = s / L[(size_t)i * m + i];
    }
    return w;
}

int main(int argc, char** argv) {
    const int n = argc > 1 ? std::atoi(argv[1]) : 60;
    const int N = argc > 2 ? std::atoi(argv[2]) : 1000;
    const double T = argc > 3 ? std::atof(argv[3]) : 20.0;
    const uint64_t seed = argc > 4 ? std::strtoull(argv[4], nullptr, 0) : 5;
    const char* dump = argc > 5 ? argv[5] : nullptr;
    try {
        if (n < 1 || n > 64 || N < 1) throw std::invalid_argument("1 <= n <= 64, N >= 1");
        pdmp::PrecisionCholesky target;
        target.n = n;
        target.N = (double)N;
        const int64_t d = target.d();
        // Ltrue: the bidiagonal Cholesky factor of SymTridiagonal(1, −0.3), :22-25
        std::vector<double> ld((size_t)n), ls((size_t)n, 0.0);
        for (int i = 0; i < n; ++i) {
            ld[(size_t)i] = std::sqrt(1.0 - (i ? ls[(size_t)i - 1] * ls[(size_t)i - 1] : 0.0));
            if (i + 1 < n) ls[(size_t)i] = -0.3 / ld[(size_t)i];
        }
        // Y = Ltrue⁻ᵀ Z (:26), YY = Y Yᵀ (:27), the lower triangle mirrored: symmetric bit for bit
        std::vector<double> YY((size_t)n * n, 0.0), y((size_t)n);
        for (int k = 0; k < N; ++k) {
            for (int i = n - 1; i >= 0; --i) {
                const double z = pdmp_randn(seed, PDMP_STREAM_INIT, (uint64_t)k * (uint64_t)n + (uint64_t)i);
                y[(size_t)i] = (z - (i + 1 < n ? ls[(size_t)i] * y[(size_t)i + 1] : 0.0)) / ld[(size_t)i];
            }
            for (int r = 0; r < n; ++r)
                for (int c = 0; c <= r; ++c) YY[(size_t)r * n + c] += y[(size_t)r] * y[(size_t)c];
        }
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < r; ++c) YY[(size_t)c * n + r] = YY[(size_t)r * n + c];
        target.YY = YY;
        // μ̂: per column the mode of exp(−½ vᵀ A v + N log v₁), v = A⁻¹e1 √(N / (A⁻¹)₁₁); γ̂: the curvature of ϕ there
        std::vector<double> mu((size_t)d), gam((size_t)d), x0((size_t)d), th0((size_t)d), c((size_t)d, 10.0), kappa((size_t)d, 0.01);
        for (int col = 0; col < n; ++col) {
            const std::vector<double> w = first_column_of_inverse(YY, n, col);
            const double scale = std::sqrt((double)N / w[0]);
            for (int r = col; r < n; ++r) {
                const int64_t i = target.index(r, col);
                mu[(size_t)i] = w[(size_t)(r - col)] * scale;
                gam[(size_t)i] = YY[(size_t)r * n + r] + (r == col ? (double)N / (mu[(size_t)i] * mu[(size_t)i]) : 0.0);
                const double truth = (r == col) ? ld[(size_t)col] : (r == col + 1 ? ls[(size_t)col] : 0.0);
                x0[(size_t)i] = truth + 0.01 * pdmp_randn(seed, PDMP_STREAM_INIT, ((uint64_t)N * (uint64_t)n) + (uint64_t)i);  // :59
                if (r == col) x0[(size_t)i] = std::fabs(x0[(size_t)i]);
                th0[(size_t)i] = (pdmp_u01(seed, PDMP_STREAM_INIT, ((uint64_t)N * (uint64_t)n) + (uint64_t)d + (uint64_t)i) < 0.5) ? -1.0 : 1.0;  // :64
            }
        }
        if (dump) {
            std::FILE* f = std::fopen(dump, "wb");
            if (!f) throw std::runtime_error("cannot open the dump file");
            const double head[2] = {(double)n, (double)N};
            std::fwrite(head, sizeof(double), 2, f);
            for (const std::vector<double>* v : {&YY, &gam, &mu, &x0, &th0}) std::fwrite(v->data(), sizeof(double), v->size(), f);
            std::fclose(f);
        }
        pdmp::ZigZag F;  // ZigZag(Γ̂, μ̂), Γ̂ diagonal
        F.Gamma.n = d;
        for (int64_t j = 0; j < d; ++j) {
            F.Gamma.colptr.push_back(j);
            F.Gamma.rowval.push_back(j);
            F.Gamma.nzval.push_back(gam[(size_t)j]);
        }
        F.Gamma.colptr.push_back(d);
        F.mu = mu;
        F.sigma.assign((size_t)d, 1.0);
        pdmp::Options o;
        o.adapt = true;
        o.seed = seed;
        o.trace_capacity = 4096;  // (drained and continued several times)
        const auto R = pdmp::sspdmp(target, 0.0, x0, th0, T, c, F, kappa, o);
        uint64_t h = 14695981039346656037ull;
        h = fnv1a(h, R.trace.events.data(), R.trace.events.size() * sizeof(pdmp::Event));
        h = fnv1a(h, R.t.data(), R.t.size() * sizeof(double));
        h = fnv1a(h, R.x.data(), R.x.size() * sizeof(double));
        h = fnv1a(h, R.theta.data(), R.theta.size() * sizeof(double));
        h = fnv1a(h, R.c.data(), R.c.size() * sizeof(double));
        // mean(Ξ) and inclusion_prob(Ξ) of the returned trace as the reference defines them (src/trace.jl:161-200): per coordinate the trapezoids
        // between its own events, over T = the time of the last event
        const double Tl = R.trace.events.empty() ? 1.0 : R.trace.events.back().t;
        std::vector<double> tc((size_t)d, 0.0), xc(x0), mean((size_t)d, 0.0), away((size_t)d, 0.0);
        for (const pdmp::Event& e : R.trace.events) {
            const size_t i = (size_t)e.i;
            const double dt = e.t - tc[i];
            mean[i] += (xc[i] + e.x) * dt;
            if (xc[i] != 0 || e.x != 0) away[i] += dt;
            tc[i] = e.t;
            xc[i] = e.x;
        }
        for (int64_t i = 0; i < d; ++i) {
            mean[(size_t)i] /= 2 * Tl;
            away[(size_t)i] /= Tl;
        }
        const std::vector<double> Lh = target.unpack(mean);
        double err = 0.0;
        for (int r = 0; r < n; ++r)
            for (int q = 0; q < n; ++q) {
                double s = 0.0;
                for (int k = 0; k < n; ++k) s += Lh[(size_t)r * n + k] * Lh[(size_t)q * n + k];
                const double g = (r == q) ? 1.0 : (std::abs(r - q) == 1 ? -0.3 : 0.0);
                err += (s - g) * (s - g);
            }
        double inc[3] = {0.0, 0.0, 0.0};
        for (int k = 1; k <= 3; ++k) {
            for (int col = 0; col + k < n; ++col) inc[k - 1] += away[(size_t)target.index(col + k, col)];
            if (n > k) inc[k - 1] /= (double)(n - k);
        }
        std::printf("%lld %zu %lld %lld %016llx %.17g %.17g %.17g %.17g\n", (long long)d, R.trace.events.size(), (long long)R.num, (long long)R.acc[0],
                    (unsigned long long)h, std::sqrt(err), inc[0], inc[1], inc[2]);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "precision_sticky: %s\n", ex.what());
        return 1;
    }
    return 0;
}
