// pdmp_capi_tune.hip -- placement tuning: where set_state puts the two arrays its event loop scatters over.
//
// WHERE the records and the pairs of a full-width tracked ensemble lie decides whether its slices take 38 or 45 ms (DESIGN.md 5 "The timing modes are a
// property of the allocation": the same binary, the same process, by the hipMalloc that backs either array).  No API shows the property, a few
// milliseconds of the event loop do: after the state is set, a short launch is timed, one of the two arrays -- then the other -- is given a new
// allocation (the old ones stay reserved, so the new ones are other memory), the state is set again and the launch repeated; the fastest combination is
// kept, the rest freed, and the state set one last time.  Every probe does identical work, so the times compare directly; the ensemble the caller gets
// is bit for bit the one set_state alone would have made.  pdmp_debug_set_placement(ens, 0, ...) turns it off.
#include <algorithm>
#include <chrono>
#include <cstdio>

#include "pdmp_ensemble.hpp"

namespace {

// The allocations a tuning pass has tried for its two arrays (index 0 of each list: what set_state allocated) and its spacers.  Whatever way the pass
// ends, all but the kept pair are freed.
struct Candidates {
    std::vector<void*> list[2], spacers;
    size_t keep[2] = {0, 0};
    void release() {
        for (int w = 0; w < 2; ++w) {
            for (size_t k = 0; k < list[w].size(); ++k)
                if (k != keep[w]) (void)hipFree(list[w][k]);
            list[w].clear();
        }
        for (void* sp : spacers) (void)hipFree(sp);
        spacers.clear();
    }
    ~Candidates() { release(); }
};

struct TunePlan {
    const char* tag[2];      // the two arrays' letters in tune_log
    std::vector<int> steps;  // which of the two arrays gets a new allocation on each step
    float settle;            // done once the slowest probe exceeds the fastest by this ratio: both levels seen, the fast one in hand
    size_t spacer_bytes;     // an allocation held to the end before every candidate, so that it lands somewhere else (0: none)
    size_t min_free;         // a step needs its allocation, its spacer and this much free memory (0: hipMalloc's failure alone ends the steps)
    const char* headline;    // opens tune_log
};

// reinit() sets the state again (after either array moved), probe(&ms) times the launch.  On return the two buffers hold the fastest pair seen, the
// state is as set_state makes it, and tune_log lists the probes.
template <class A, class B, class Reinit, class Probe>
pdmp_status tune_placement(pdmp_ensemble* e, DevBuf<A>& a, DevBuf<B>& b, const TunePlan& plan, Reinit reinit, Probe probe) {
    const auto t_begin = std::chrono::steady_clock::now();
    const size_t bytes[2] = {a.n * sizeof(A), b.n * sizeof(B)};
    Candidates cand;
    cand.list[0].push_back(a.p);
    cand.list[1].push_back(b.p);
    struct Trial { size_t k[2]; float ms; };
    std::vector<Trial> trials;
    auto use = [&](size_t ka, size_t kb) {
        a.p = static_cast<A*>(cand.list[0][ka]);
        b.p = static_cast<B*>(cand.list[1][kb]);
        cand.keep[0] = ka;
        cand.keep[1] = kb;
    };
    auto measure = [&](size_t ka, size_t kb) -> pdmp_status {
        use(ka, kb);
        if (!trials.empty()) PDMP_TRY(reinit());
        float ms = 0;
        PDMP_TRY(probe(&ms));
        trials.push_back({{ka, kb}, ms});
        return PDMP_OK;
    };
    auto slower = [](const Trial& p, const Trial& q) { return p.ms < q.ms; };
    auto best = [&]() { return *std::min_element(trials.begin(), trials.end(), slower); };
    auto settled = [&]() { return trials.size() >= 2 && std::max_element(trials.begin(), trials.end(), slower)->ms > plan.settle * best().ms; };
    pdmp_status st = measure(0, 0);
    for (size_t step = 0; st == PDMP_OK && step < plan.steps.size() && !settled(); ++step) {
        const int w = plan.steps[step];
        size_t freeb = 0, totb = 0;
        if (plan.min_free && (hipMemGetInfo(&freeb, &totb) != hipSuccess || freeb < bytes[w] + plan.spacer_bytes + plan.min_free)) {
            (void)hipGetLastError();
            break;
        }
        // what matters is which REGIONS of the memory the two arrays lie in, and consecutive hipMallocs are neighbours: hence the spacer
        void *sp = nullptr, *np = nullptr;
        if (plan.spacer_bytes && hipMalloc(&sp, plan.spacer_bytes) == hipSuccess) cand.spacers.push_back(sp);
        else if (plan.spacer_bytes) (void)hipGetLastError();
        if (hipMalloc(&np, bytes[w]) != hipSuccess) {
            (void)hipGetLastError();
            break;
        }
        cand.list[w].push_back(np);
        st = w == 0 ? measure(cand.list[0].size() - 1, best().k[1]) : measure(best().k[0], cand.list[1].size() - 1);
    }
    // keep the best pair, free the rest (on every way out: cand's destructor), and leave the state as set_state makes it
    const Trial kept = trials.empty() ? Trial{{0, 0}, 0.f} : best();
    use(kept.k[0], kept.k[1]);
    HIP_TRY(hipDeviceSynchronize());
    cand.release();
    const pdmp_status st2 = reinit();
    e->last_kernel = "";  // (pdmp_debug_last_kernel: '' before the caller's first run)
    char t[96];
    e->tune_log = plan.headline;
    for (const Trial& q : trials) {
        snprintf(t, sizeof t, " %.2f[%s%zu %s%zu]", q.ms, plan.tag[0], q.k[0], plan.tag[1], q.k[1]);
        e->tune_log += t;
    }
    snprintf(t, sizeof t, "; kept %s%zu %s%zu; %.2f s", plan.tag[0], kept.k[0], plan.tag[1], kept.k[1],
             std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count());
    e->tune_log += t;
    return st != PDMP_OK ? st : st2;
}

}  // namespace

// The factorised samplers: the records, and level 0 of the queue -- (key, time) pairs under tracking, plain keys otherwise.  The probe is a launch in
// which every chain pauses after PLACE_PROBE_DRAWS draws; new pairs and new records in turn, at most four of each, a spacer before each.
#define PLACE_PROBE_DRAWS 12000u
#define PLACE_TUNE_MIN_CHAINS 1024  // (the two modes were seen on launches that fill the device: 4096 chains; narrower ones are probed as well, it costs milliseconds)
pdmp_status init_state_tuned(pdmp_ensemble* e, double t0, const double* x0, const double* th0, const double* c, const uint64_t* seeds,
                             uint64_t seed0) {
    e->tune_log.clear();
    PDMP_TRY(init_state(e, t0, x0, th0, c, seeds, seed0));
    // The families of pdmp_kernels.hip / pdmp_trackp.hip / pdmp_exactp.hip only, under spdmp (they pause on the draw count; the general-degree, logistic
    // and sticky ones are not probed).  A family the run would refuse is reported too: the probe's run then raises the refusal and set_state returns it.
    DevBuf<double>& keybuf = e->track_pairs ? e->d_kp : e->d_keys;
    const size_t rec_bytes = e->d_rec.n * sizeof(*e->d_rec.p), kp_bytes = keybuf.n * sizeof(double);
    KernelFamily fam;
    (void)select_family(e, run_params(e, t0, PDMP_RUN_STOP_BEFORE), general_params(e), logistic_tables(e), &fam);
    const bool probed_kernel = e->cfg.sampler == PDMP_SAMPLER_ZIGZAG_LOCAL &&
                               (fam == FAM_SPEC || fam == FAM_TRACKP || fam == FAM_EXACTP || fam == FAM_ONE_EVENT);  // (FAM_ONE_EVENT never pauses)
    if (e->place_tune == 0 || !probed_kernel || e->dbg_dump != 0 || e->cfg.nchains < PLACE_TUNE_MIN_CHAINS || rec_bytes < ((size_t)2 << 30) ||
        e->d_rec.placed.va || keybuf.placed.va || e->dbg_count_limit != 0)
        return PDMP_OK;
    size_t freeb = 0, totb = 0;
    if (hipMemGetInfo(&freeb, &totb) != hipSuccess || freeb < 3 * (rec_bytes + kp_bytes) + ((size_t)8 << 30)) {
        (void)hipGetLastError();
        return PDMP_OK;
    }
    char headline[96];
    snprintf(headline, sizeof headline, "placement probes (ms, %u draws per chain):", PLACE_PROBE_DRAWS);
    // (the modes are 17 % apart; probes repeat to 1-2 %)
    const TunePlan plan{{"r", "p"}, {1, 0, 1, 0, 1, 0, 1, 0}, 1.08f, (size_t)6 << 30, rec_bytes + kp_bytes + ((size_t)8 << 30), headline};
    return tune_placement(
        e, e->d_rec, keybuf, plan, [&]() { return init_state(e, t0, x0, th0, c, seeds, seed0); },
        [&](float* ms) -> pdmp_status {
            e->dbg_count_limit = PLACE_PROBE_DRAWS;
            const pdmp_status r = ensemble_run_impl(e, t0 + 1.0e3, PDMP_RUN_STOP_BEFORE, nullptr);
            e->dbg_count_limit = 0;
            return r != PDMP_OK ? r : elapsed_ms(e->ev0, e->ev1, ms);
        });
}

// The Bouncy Particle streams every event's (x, θ) into two large arrays; whether those two allocations get along decides 4.5 or 5.3 ms per step of config
// C2 (tools/mode_move_bps.py: moving either flips it; x, θ and the event times do not matter) -- the same property of the memory as init_state_tuned's.
// With a trace of at least 2 GB per array: fill it once (every chain pauses when its segment is full), time that, give the θ array three times (then the
// x array twice) new hipMallocs, keep the fastest pair, set the state again.
pdmp_status init_state_bps_tuned(pdmp_ensemble* e, double t0, const double* x0, const double* theta0, double c, const uint64_t* seeds) {
    if (e) e->tune_log.clear();
    PDMP_TRY(init_state_bps(e, t0, x0, theta0, c, seeds));
    const size_t ev_bytes = e->b_ev_th.n * sizeof(double);
    size_t freeb = 0, totb = 0;
    if (e->bps.modern) return PDMP_OK;  // (a record per 1/λref of speed-time: the trace writes do not bound this loop, nothing to place)
    if (e->place_tune == 0 || e->cfg.trace_capacity <= 0 || ev_bytes < ((size_t)2 << 30) || e->b_ev_th.placed.va) return PDMP_OK;
    if (hipMemGetInfo(&freeb, &totb) != hipSuccess || freeb < 6 * ev_bytes + ((size_t)8 << 30)) {
        (void)hipGetLastError();
        return PDMP_OK;
    }
    // (three levels here: the trace filled in 5.9-6.1, 6.3 or 6.9-7.3 ms -- steps of 4.6, 4.9, 5.4 ms; done once the whole spread has been seen)
    const TunePlan plan{{"x", "th"}, {1, 1, 1, 0, 0}, 1.15f, 0, 0, "placement probes (ms, the trace filled once):"};
    return tune_placement(
        e, e->b_ev_x, e->b_ev_th, plan, [&]() { return init_state_bps(e, t0, x0, theta0, c, seeds); },
        [&](float* ms) -> pdmp_status {
            const pdmp_status r = ensemble_run_impl(e, t0 + 1.0e30, PDMP_RUN_STOP_BEFORE, nullptr);
            return r != PDMP_OK ? r : elapsed_ms(e->ev0, e->ev1, ms);
        });
}
