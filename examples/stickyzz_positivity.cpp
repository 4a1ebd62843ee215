// stickyzz_positivity -- a constrained target consumed on the device, through the C++ mirror (include/pdmp_mi355.hpp): the shape of the
// reference's examples/positivityconstraint.jl -- two coordinates, none constrained but the second, which lives above a wall at 2.5
// (StickyBarriers((2.5, Inf), (:reflect, :reflect), (Inf, Inf))), start (2, 5), c = 20 adapted with multiplier 1.5, the trace discretised with
// dt = 0.5 for the mean -- with a correlated Gaussian N((−3, 3), Γ⁻¹) as the target.  Options::consume runs the device consumers over every
// slice of the trace (mean, the grid, the barrier occupation) while Options::trace_capacity bounds the buffer; with consume_only the events
// never leave the device.
// Usage: stickyzz_positivity T seed [consume_only]
// Prints: T_last, events copied to the host, the mean of the grid rows per coordinate, mean(Ξ) per coordinate, hits of the wall, time frozen on it (0: a wall).
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "pdmp_mi355.hpp"

int main(int argc, char** argv) {
    const double T = argc > 1 ? std::atof(argv[1]) : 2000.0;
    const uint64_t seed = argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 7;
    const int64_t d = 2;
    const double dt = 0.5;
    try {
        pdmp::GaussianTarget target;
        target.Gamma.n = d;
        target.Gamma.colptr = {0, 2, 4};
        target.Gamma.rowval = {0, 1, 0, 1};
        target.Gamma.nzval = {1.0, 0.25, 0.25, 0.5};
        target.mu = {-3.0, 3.0};
        pdmp::ZigZag F;  // the bounds see the target's own Γ
        F.Gamma = target.Gamma;
        F.mu.assign((size_t)d, 0.0);
        F.sigma.assign((size_t)d, 1.0);
        std::vector<pdmp::Barrier> barriers((size_t)d);  // coordinate 0: no barrier
        barriers[1].lo = 2.5;                              // coordinate 1: reflected at once at 2.5, nothing above
        pdmp::Options o;
        o.seed = seed;
        o.adapt = true;
        o.factor = 1.5;
        o.trace_capacity = 4096;
        o.consume = true;
        o.consume_dt = dt;
        o.consume_points = (int64_t)(T / dt) + 64;
        o.consume_only = argc > 3 && std::atoi(argv[3]) != 0;  // (the events are then never copied to the host)
        const auto R = pdmp::stickyzz(target, 0.0, {2.0, 5.0}, {-1.0, 1.0}, T, {20.0, 20.0}, F, barriers, o);
        const pdmp::BarrierConsumed& C = R.consumed;
        double gm[2] = {0.0, 0.0};
        for (int64_t k = 0; k < C.npoints; ++k)
            for (int64_t i = 0; i < d; ++i) gm[i] += C.grid_x[(size_t)(k * d + i)];
        for (double& v : gm) v /= (double)C.npoints;
        std::printf("%.17g %zu %.17g %.17g %.17g %.17g %llu %.17g\n", C.T, R.trace.events.size(), gm[0], gm[1], C.mean[0], C.mean[1],
                    (unsigned long long)C.hits_lo[1], C.frozen_lo[1]);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "stickyzz_positivity: %s\n", ex.what());
        return 1;
    }
    return 0;
}
