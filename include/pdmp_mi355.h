/*
 * pdmp_mi355.h -- C ABI of libpdmp_mi355.so, the MI355X (gfx950) ensemble engine for the PDMP event loop.
 *
 * The reference (ZigZagBoomerang.jl @ v0.13.2) has no FFI: its boundary is the Julia method signatures
 *     spdmp(∇ϕ, t0, x0, θ0, T, c, [G,] F::ZigZag, args...; factor, adapt, seed) -> Ξ,(t,x,θ),(acc,num),c
 *                                                               (src/sfact.jl:162-163,211,214)
 *     pdmp (∇ϕ, ...same...)                = spdmp(..., All(), ...)   (src/sfact.jl:236)
 *     pdmp (∇ϕ!, t0,x0,θ0,T,c, B::BouncyParticle; ...)               (src/not_fact_samplers.jl:117,395)
 *     sspdmp(∇ϕ, t0,x0,θ0,T,c, [G,] F::ZigZag, κ, args...; ...)       (src/ss_fact.jl:159-160,217)
 * Each entry point below names the reference lines it replaces.  A Julia `ccall` shim that keeps those
 * signatures is shown in INTEGRATION.md; the Python mirror lives in zigzagboomerang.jl_amd/samplers.py.
 *
 * Conventions
 *   - plain C, caller-owned HOST pointers unless a name ends in `_dev`; the library never frees caller
 *     memory and never keeps a caller pointer after the call returns;
 *   - coordinates are 0-based (the Julia shim adds 1); matrices are CSC with int64 colptr/rowval,
 *     rows ascending inside a column (SparseArrays layout, src/common.jl:17-20);
 *   - return codes, never exceptions; per-chain status words replace the reference's `error(...)`
 *     (src/sfact.jl:124): one diverged chain never aborts the ensemble;
 *   - one ensemble is bound to one HIP device; calls on one ensemble must be serialised by the caller,
 *     different ensembles are independent (no globals except the thread-local error string; the library reads no
 *     environment variables -- diagnostics are per-ensemble calls declared in pdmp_debug.h);
 *   - a user gradient closure cannot cross a C ABI: targets are an enumerated set (Gaussian CSC now).
 *   - randomness: chain k draws from Philox4x32-10 keyed by seeds[k]; draw order is the reference's
 *     `rand(rng)` call order (include/pdmp_detmath.h, oracle/pdmp_oracle.h).
 */
#ifndef PDMP_MI355_H
#define PDMP_MI355_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: pdmp_ensemble_run_partitioned takes the mask's length; pdmp_ensemble_path_integrals, the trace consumers, the G argument
 *    (pdmp_ensemble_set_neighbourhood), pdmp_ensemble_set_target_bps and the pdmp_comm_* (RCCL) entry points; Boomerang ensembles
 *    need an explicit mass factor like BouncyParticle ones.
 * 3: pdmp_ensemble_consume_discretized no longer clamps *npoints (it reports the grid points the trace reaches; row 0 is always x0),
 *    pdmp_ensemble_gather_bps_traces / pdmp_comm_gathered_bps_copy / pdmp_ensemble_bps_trace_dev exist, and ensembles of at most seven chains per compute unit (1792 on an MI355X)
 *    run the tracked local ZigZag with a helper wavefront per chain (same results; include/pdmp_debug.h: pdmp_debug_set_helper_wave).
 *    A host binding must check pdmp_abi_version() at load time.
 *    (still 3: pdmp_ensemble_set_bps_sticky, pdmp_ensemble_bps_trace_free_copy and pdmp_ensemble_bps_final_sticky were ADDED later -- the sticky
 *    Bouncy Particle / Boomerang; nothing that existed changed, so a binding that wants them looks the symbols up.  The same holds for
 *    pdmp_ensemble_set_flow_bps_modern and pdmp_ensemble_set_bps_record_limit, the speed-recorded Bouncy Particle.) */
#define PDMP_ABI_VERSION 3

typedef enum {
    PDMP_OK = 0,
    PDMP_ERR_INVALID = 1,     /* bad argument / call order */
    PDMP_ERR_NO_DEVICE = 2,   /* no gfx950 HIP device: the engine has NO CPU fallback */
    PDMP_ERR_HIP = 3,         /* a HIP runtime call failed; see pdmp_last_error() */
    PDMP_ERR_UNSUPPORTED = 4, /* configuration outside what the kernels implement */
    PDMP_ERR_NOMEM = 5
} pdmp_status;

/* sampler = which reference driver the ensemble reproduces */
#define PDMP_SAMPLER_ZIGZAG_LOCAL 0 /* spdmp, G = Matched()      src/sfact.jl:73-145,214 */
#define PDMP_SAMPLER_ZIGZAG_ALL 1   /* pdmp,  G = All()          src/sfact.jl:236        */
#define PDMP_SAMPLER_BPS 2          /* pdmp,  BouncyParticle     src/not_fact_samplers.jl:52-147 */
#define PDMP_SAMPLER_STICKY_ZIGZAG 3 /* sspdmp                   src/ss_fact.jl:78-215   */
#define PDMP_SAMPLER_BARRIER_ZIGZAG 4 /* stickyzz                src/stickyzz.jl:176-319 */

/* per-chain status words */
#define PDMP_CHAIN_OK 0
#define PDMP_CHAIN_BOUND_VIOLATED 1 /* l >= lb with adapt = false (reference: error, src/sfact.jl:124) */
#define PDMP_CHAIN_STALLED 2        /* queue minimum is +Inf */
#define PDMP_CHAIN_TRACE_FULL 3     /* trace buffer full: drain with pdmp_ensemble_trace_* and run again */
#define PDMP_CHAIN_PAUSED 4         /* a launch counts its draws and proposals in 32 bits: a chain that has used 3 * 2^30 of them inside ONE call of
                                     * pdmp_ensemble_run (~10^9 proposals: only without a trace buffer) stops there, nothing to drain -- run again,
                                     * the run continues exactly (ABI 3) */

/* run flags */
#define PDMP_RUN_REFERENCE_TAIL 0 /* `while t′ < T` (src/sfact.jl:199): the last event has t′ >= T        */
#define PDMP_RUN_STOP_BEFORE 1    /* pause BEFORE popping a key >= T (slice boundary; resumable, exact)  */

typedef struct pdmp_ensemble pdmp_ensemble;

typedef struct {
    uint32_t struct_size; /* sizeof(pdmp_config), for ABI growth */
    int32_t device;       /* HIP device ordinal */
    int32_t sampler;      /* PDMP_SAMPLER_* */
    int32_t adapt;        /* kwarg adapt  (src/sfact.jl:163) */
    double factor;        /* kwarg factor (src/sfact.jl:163: 1.8; BPS 2.0; sticky 1.5) */
    int64_t nchains;      /* ensemble width on THIS device */
    int64_t d;            /* dimension */
    int64_t trace_capacity; /* events kept per chain (0: count only, no trace) */
} pdmp_config;

/* One FactTrace event (t[i], i, x[i], θ[i]) after the flip: src/sfact.jl:50-52, src/trace.jl:38. 32 bytes. */
typedef struct {
    double t;
    int64_t i; /* 0-based */
    double x;
    double theta;
} pdmp_event;

/* Per-chain counters (the reference returns (acc, num); src/sfact.jl:211). */
typedef struct {
    double t_last;      /* t′ of the last processed event/proposal */
    uint64_t num;       /* proposals                (num, src/sfact.jl:120) */
    uint64_t nacc;      /* accepted reflections     (sum(acc), :122)        */
    uint64_t nrefresh;  /* refresh events           (:78-114)               */
    uint64_t ntrace;    /* events currently in the trace buffer             */
    uint64_t nevents;   /* events emitted since set_state (never reset)     */
    uint64_t ndraw_main;
    uint64_t ndraw_global;
    uint32_t status;    /* PDMP_CHAIN_* */
    uint32_t reserved;
} pdmp_chain_counters;

const char* pdmp_last_error(void);
int pdmp_abi_version(void);
/* number of usable gfx950 devices (0 if none / HIP not initialisable) */
int pdmp_device_count(void);

pdmp_status pdmp_ensemble_create(const pdmp_config* cfg, pdmp_ensemble** out);
void pdmp_ensemble_destroy(pdmp_ensemble* ens);

/*
 * Flow Z = ZigZag(Γ, μ, σ; λref, ρ) (src/types.jl:19-27).  Γ is the BOUNDING precision used by ab()
 * (src/fact_samplers.jl:50-54); its column pattern defines G1 (src/sfact.jl:170) and G2 (:178).
 * sigma may be NULL (ones).  lambda_ref > 0 enables the refresh clock (src/sfact.jl:78-114,188-190).
 */
pdmp_status pdmp_ensemble_set_flow_zigzag(pdmp_ensemble* ens, const int64_t* colptr, const int64_t* rowval,
                                          const double* nzval, const double* mu, const double* sigma,
                                          double lambda_ref, double rho);

/*
 * Flow F = FactBoomerang(Γ, μ, λref, σ; ρ) (src/types.jl:71-79) for spdmp: Hamiltonian rotation about μ between events
 * (src/sfact.jl:29-36), rate ((∇ϕ_i − (x_i−μ_i)Γ_ii)θ_i)⁺ (src/fact_samplers.jl:37-39), bound a = c_i√(x_i²+θ_i²)·z + (x_i²+θ_i²)Γ_ii,
 * b = 0 (:58-65), mandatory refresh θ_i = ρθ_i + ρ̄σ_i·randn at rate λref > 0 (src/sfact.jl:103, src/fact_samplers.jl:18).
 * Same arguments as set_flow_zigzag; sampler must be PDMP_SAMPLER_ZIGZAG_LOCAL (the factorised driver spdmp).
 */
pdmp_status pdmp_ensemble_set_flow_factboomerang(pdmp_ensemble* ens, const int64_t* colptr, const int64_t* rowval,
                                                 const double* nzval, const double* mu, const double* sigma,
                                                 double lambda_ref, double rho);

/*
 * The neighbourhood argument of spdmp(∇ϕ, t0, x0, θ0, T, c, G, F, ...) / sspdmp(∇ϕ, t0, x0, θ0, T, c, G, F, κ, ...) (src/sfact.jl:162,171-179;
 * src/ss_fact.jl:159,167-172): G[i] = g_rowval[g_colptr[i] .. g_colptr[i+1]) (ascending) is what a proposal of i moves before the gradient is
 * taken (:82) and what the gradient may read (:116); G1[i] = the pattern of column i of the flow's Γ stays what is re-bounded (:131-135), and
 * G2[i] = ∪_{j ∈ G1[i]} G1[j] \ G[i] what an accepted event moves on top (:178).  G[i] ⊇ G1[i] is required (the reference's @assert, :177):
 * PDMP_ERR_INVALID otherwise.  Without this call G = Matched() = G1.  Call after set_flow_* and BEFORE set_target_* (the target's pattern
 * may then use all of G); such ensembles run on the general-neighbourhood kernel.  Not for PDMP_SAMPLER_ZIGZAG_ALL (G = All()).
 */
pdmp_status pdmp_ensemble_set_neighbourhood(pdmp_ensemble* ens, const int64_t* g_colptr, const int64_t* g_rowval);

/*
 * Target ∇ϕ(x, i) = Γt[:,i]·x  [ − Γt[:,i]·μt ]  (idot, src/common.jl:16-24; closure of
 * scripts/gaussianrandomfield.jl:25, test/maintest.jl:9).  The pattern of Γt must be contained in the
 * flow's Γ pattern (the reference reads only x[j], j in G[i]: src/sfact.jl:116).  mu may be NULL.
 * Must be called after set_flow_zigzag.
 */
pdmp_status pdmp_ensemble_set_target_gaussian_csc(pdmp_ensemble* ens, const int64_t* colptr,
                                                  const int64_t* rowval, const double* nzval,
                                                  const double* mu);

/*
 * Target of config C4: subsampled logistic regression with a control variate at μ, evaluated with SelfMoving():
 *   ∇ϕmoving(t,x,θ,i,t′,F,A,At,μ,y,ny,k) = γ0*x[i] − fdot_moving(A,At,i,t,x,θ,t′,F,μ,y,ny,k)   (scripts/logistic.jl:78-95,107,167)
 * A is the n x p design in CSC (column = coordinate), At = A' in CSC (column = observation), y / ny the per-observation
 * success / failure counts, k_sub the subsample size; the k_sub row indices of every proposal are draws of the chain's
 * PDMP_STREAM_GLOBAL stream (the reference takes them from Julia's global rng).  Must follow set_flow_zigzag.
 */
pdmp_status pdmp_ensemble_set_target_logistic(pdmp_ensemble* ens, int64_t n, const int64_t* A_colptr,
                                              const int64_t* A_rowval, const double* A_nzval, const int64_t* At_colptr,
                                              const int64_t* At_rowval, const double* At_nzval, const double* y,
                                              const double* ny, const double* mu, double gamma0, int64_t k_sub);

/*
 * Target of the reference's diffusion-bridge example (research/diffusion_bridge/diffbridge.jl, faberschauder.jl): the bridge of
 *   dX = b(X) ds + dW on [0, T],  b(x) = −beta x + alpha sin(omega x),
 * expanded in the Faber-Schauder basis up to level L: d = (2 << L) + 1 coefficients ξ, ξ[0] = u/√T and ξ[d−1] = v/√T being the fixed end
 * points.  The gradient is ∇ϕmoving (faberschauder.jl:137-144), evaluated with SelfMoving() / ExtendedForm (src/sfact.jl:57-68): it draws a time
 * s in the support of basis function i -- draw ndraw_global of PDMP_STREAM_GLOBAL, taken before the thinning coin --, moves the L + 1
 * coefficients whose basis functions cover s to the proposal time, and returns an unbiased estimate of ∂ϕ/∂ξ_i.  b′ and b″ are the true
 * derivatives of b (the script's carry a stray factor 2).  Runs on zz_bridge_run_kernel, bit for bit tests/ref/bridge_ref.c.
 * Valid on PDMP_SAMPLER_ZIGZAG_LOCAL after set_flow_zigzag, in place of another target (the later target call wins).
 * PDMP_ERR_INVALID: d != (2 << L) + 1, L < 0, T <= 0, a parameter that is not finite, another sampler, a state that already exists.
 * PDMP_ERR_UNSUPPORTED: L > 10 (d > 2049).  pdmp_ensemble_set_state then answers PDMP_ERR_UNSUPPORTED, naming the cause, to a flow Γ that is
 * not the identity, μ != 0, a refresh clock, a FactBoomerang, pdmp_ensemble_set_neighbourhood, gradient tracking, LocalBound, adaptscale, a
 * synthetic state, and θ0 != 0 at either end point of any chain (free end points are not implemented; give the end points c = 0 as the script does).
 * A chain whose |omega X_s| exceeds 2^30, or whose sampled s rounds up to T, ends as PDMP_CHAIN_STALLED.  The trace consumers
 * (pdmp_ensemble_consume_*) serve these traces; pdmp_ensemble_batch_means, _ess_* and _path_integrals answer PDMP_ERR_UNSUPPORTED (this loop
 * keeps no ∫ξ dt).  (Added under ABI version 3: nothing that existed changed, a binding that wants it looks the symbol up.)
 */
pdmp_status pdmp_ensemble_set_target_diffusion_bridge(pdmp_ensemble* ens, int32_t L, double T, double alpha, double beta, double omega);

/*
 * Target of the reference's precision case study (casestudies/precision/precision.jl; research/newsticky/precision/precision4.jl with
 * gamma0 > 0): learning a sparse precision matrix through its Cholesky factor.  N observations Y_k ~ N(0, (L L')^-1) enter through
 * YY = sum_k Y_k Y_k' ([n x n] row-major, symmetric) and N.  The d = n(n+1)/2 coordinates are the lower triangle of L packed column by column
 * (0-based): u[i] = L[r, c], i = k0 + (r - c) with k0 = c n - c(c-1)/2; column c occupies [k0, k0 + n - c).
 *   phi(u)     = 1/2 sum_c L[:,c]' YY L[:,c] - N sum_c log L[c,c] + gamma0/2 (sum_{r>c} L[r,c]^2 + sum_c (L[c,c] - 1)^2)
 *   dphi/du_i  = sum_{q < n-c} YY[r, c+q] u[k0+q] + (r == c ? -N/u_i + gamma0 (u_i - 1) : gamma0 u_i)
 * the sum being the 64-lane sum of the products in wave order (lane q holds product q, 0.0 past the column; xor butterfly 1, 2, .., 32) with
 * the diagonal or prior term added to it.  Runs on zz_precision_run_kernel, bit for bit tests/ref/precision_ref.c: sspdmp (src/ss_fact.jl)
 * with G1[i] = {i}, G[i] = the column of i, G2[i] empty.
 * Valid on PDMP_SAMPLER_STICKY_ZIGZAG after set_flow_zigzag, in place of another target (the later target call wins); pdmp_ensemble_set_sticky
 * (kappa, reversible, strong_upperbounds) as for every sticky ZigZag.
 * PDMP_ERR_INVALID: d != n(n+1)/2, n < 1, N not finite or <= 0, gamma0 < 0 or not finite, a YY entry that is not finite, YY not symmetric bit
 * for bit, another sampler, a state that already exists.  PDMP_ERR_UNSUPPORTED: n > 64 (d > 2080).  pdmp_ensemble_set_state then answers
 * PDMP_ERR_UNSUPPORTED, naming the cause, to a flow matrix that is not diagonal with positive entries, pdmp_ensemble_set_neighbourhood, gradient
 * tracking, LocalBound, a synthetic state, an x0 whose diagonal coordinates L[c, c] are not all > 0, and a refresh clock (one that arrives with
 * a flow set again after pdmp_ensemble_set_sticky: that call itself refuses a flow with one).  adaptscale never gets as far:
 * pdmp_ensemble_set_adaptscale answers PDMP_ERR_UNSUPPORTED on every sticky ensemble.
 * A freeze popped for a diagonal coordinate ends its chain as PDMP_CHAIN_STALLED before any state changes (the next gradient would be N/0); so
 * does a thaw that finds no saved speed (a coordinate started at x = 0 with theta = 0).  The trace consumers (pdmp_ensemble_consume_*) serve
 * these traces; pdmp_ensemble_batch_means, _ess_* and _path_integrals answer PDMP_ERR_UNSUPPORTED (this loop keeps no integral of x dt).
 * (Added under ABI version 3: nothing that existed changed, a binding that wants it looks the symbol up.)
 */
pdmp_status pdmp_ensemble_set_target_precision_cholesky(pdmp_ensemble* ens, int32_t n, const double* YY /* [n x n] */, double N, double gamma0);

/*
 * Initial state (src/sfact.jl:164-190): x0, theta0 are [nchains x d] row-major; c is [d] (copied; with
 * adapt each chain gets its own copy, returned by final_state -- no hidden mutation of caller memory,
 * unlike src/fact_samplers.jl:68); seeds is [nchains].  Computes b[i] = ab(...) and the initial queue
 * Q[i] = poisson_time(b[i], rand(rng)) ON THE DEVICE, drawing the first d uniforms of each chain in
 * order i = 0..d-1 (:184-187; like the reference, t0 is not added to the initial keys).
 * For a ZigZag ensemble that fills the device (>= 1024 chains, >= 2 GB of records) the call also chooses WHERE the records and the queue's level 0
 * lie: it times a short launch, re-allocates the two arrays a few times and keeps the fastest placement (0.03-0.1 s; the state handed back is
 * the one described above, bit for bit: DESIGN.md 5 "The timing modes are a property of the allocation"; pdmp_debug_set_placement turns it off).
 */
pdmp_status pdmp_ensemble_set_state(pdmp_ensemble* ens, double t0, const double* x0, const double* theta0,
                                    const double* c, const uint64_t* seeds);

/*
 * Synthetic initial state generated on the device (benchmarks): seeds[k] = seed0 + k,
 * x0[k][i] = randn (Philox stream PDMP_STREAM_INIT, draw i), theta0[k][i] = ±1 (draw d+i)
 * -- the shape of scripts/gaussianrandomfield.jl:29-30.
 */
pdmp_status pdmp_ensemble_set_state_synthetic(pdmp_ensemble* ens, double t0, const double* c, uint64_t seed0);

/*
 * Advance every chain to time T (the `while t′ < T` driver loop, src/sfact.jl:199-208, around
 * spdmp_inner!, :73-145).  Asynchronous on `stream` (a hipStream_t, NULL = the ensemble's own stream);
 * re-entrant: calling run again with a larger T continues the same event sequence.
 */
pdmp_status pdmp_ensemble_run(pdmp_ensemble* ens, double T, int flags, void* stream);
pdmp_status pdmp_ensemble_sync(pdmp_ensemble* ens);
/*
 * parallel_spdmp (src/parallel.jl:104-253): every chain advanced by K wavefronts -- the coordinates cut into K chunks of d / K
 * (Partition(nt, n), :26), one worker per chunk (parallel_spdmp_inner!, :63-102, horizon Δ = `delta`) and a coordinator for the
 * coordinates whose neighbourhood leaves their chunk (parallel_spdmp_outer!, :176-253).  PDMP_SAMPLER_ZIGZAG_LOCAL on a Gaussian target,
 * lambda_ref = 0; `adapt` as configured.  G = the pattern of the flow tables; G1 = the slots with g1_mask[p] != 0 (NULL: all of them;
 * mask_len must equal the number of stored entries of the Γ given to set_flow_zigzag, else PDMP_ERR_INVALID), the
 * structural pattern of the bounding Γ -- pass the bounding Γ on the union pattern with zeros and mask them out when, as in
 * test/testparallel.jl:40-49, it is the target's Γ without the cross-chunk entries.  "Upper bounds may not depend across chunks." (:124-127)
 * returns PDMP_ERR_INVALID.  Starts from a fresh state only (set_state, then ONE call); blocks until done.  The trace holds the events in
 * the order the waves emitted them: sort by time as the reference does (:167); a buffer that is too small sets PDMP_CHAIN_TRACE_FULL and the
 * trace is incomplete.  Counters: num / nacc as the reference returns them, nrefresh = coordinator rounds.  Bit-identical to the oracle's
 * threaded restatement (tests/test_gpu_partitioned.py); 1 <= K <= 16, K | d, columns of at most 64 entries.
 */
pdmp_status pdmp_ensemble_run_partitioned(pdmp_ensemble* ens, double T, int K, double delta, const uint8_t* g1_mask, int64_t mask_len,
                                          void* stream);
/* duration of the most recent run's event-loop kernel, from HIP events recorded on its stream (syncs) */
pdmp_status pdmp_ensemble_last_run_ms(pdmp_ensemble* ens, float* ms);

pdmp_status pdmp_ensemble_counters(pdmp_ensemble* ens, pdmp_chain_counters* out /* [nchains] */);
/* sum over chains of num / nacc / nevents, reduced on the host from the counters */
pdmp_status pdmp_ensemble_totals(pdmp_ensemble* ens, uint64_t* num, uint64_t* nacc, uint64_t* nevents);

/* trace access (FactTrace.events, src/trace.jl:7-13): copy events [first, first+count) of one chain */
pdmp_status pdmp_ensemble_trace_copy(pdmp_ensemble* ens, int64_t chain, int64_t first, int64_t count,
                                     pdmp_event* out);
/* forget buffered events (after draining them); clears PDMP_CHAIN_TRACE_FULL */
pdmp_status pdmp_ensemble_trace_reset(pdmp_ensemble* ens);

/*
 * Final state of chains [chain_first, chain_first+n): per-coordinate clocks t, positions x, velocities θ
 * (NOT advanced to T, src/sfact.jl:210-211), accept counts acc (int64, :182) and bounds c.  Any output
 * pointer may be NULL.  All arrays are [n x d] row-major.
 */
pdmp_status pdmp_ensemble_final_state(pdmp_ensemble* ens, int64_t chain_first, int64_t n, double* t, double* x,
                                      double* theta, int64_t* acc, double* c);

/*
 * Path integrals for ESS / moments (no counterpart in the reference; the integrand is the one of
 * mean(trace), src/trace.jl:182-200).  Requires all chains paused with PDMP_RUN_STOP_BEFORE at time T.
 * Adds, for this batch [T_prev, T], Y = (1/ΔT) ∫ x_i dt per chain and accumulates over chains:
 *   sum_y[i] += Y, sum_y2[i] += Y*Y   (device reduction; outputs are host [d] arrays, may be NULL)
 *
 * Which T may be read (this call, pdmp_ensemble_ess_begin / _batch and pdmp_ensemble_path_integrals; checked on the host from one copy
 * of the chain headers per read, else PDMP_ERR_INVALID with the chain and the times in pdmp_last_error(), and neither the previous
 * batch's J nor any accumulator is touched): J_i(T) continues every coordinate linearly from its own clock to T, which is the path's
 * integral only while no event of the chain lies in between.  So every chain must be PDMP_CHAIN_OK (not TRACE_FULL, PAUSED,
 * BOUND_VIOLATED or STALLED short of the horizon: drain / run again first) and  t_last <= T <= horizon of the last run  (t0 before the
 * first run; t_last of pdmp_chain_counters).  A PDMP_RUN_REFERENCE_TAIL run processes one proposal at or past its horizon and is
 * refused at it.  With a refresh clock (λref > 0) proposals are not processed in time order and t_last is not the latest of them: T must
 * then EQUAL the horizon of the last run (a PDMP_RUN_STOP_BEFORE run, by the rule above).
 */
pdmp_status pdmp_ensemble_batch_means(pdmp_ensemble* ens, double T_prev, double T, double* sum_y, double* sum_y2);

/*
 * Effective sample size by batch means INSIDE each chain (no counterpart in the reference; integrand as above).  All chains
 * paused with PDMP_RUN_STOP_BEFORE at the times named:
 *   ess_begin(T0)   after burn-in: snapshots the path integrals J_i(T0) of every chain;
 *   ess_batch(T)    closes the batch (T_last, T]: Y = (J(T) − J(T_last))/(T − T_last) per chain and coordinate, device sums
 *                   ΣY and ΣY² over chains and batches (call it B times with equally long batches);
 *   ess_end(...)    the chain means over the whole run, M = (J(T_B) − J(T0))/(T_B − T0): ΣM and ΣM² over chains; returns all
 *                   four [d] sums, the number of batches and the run's end points.
 * With N chains, B batches of length b:  within-chain  S_w = ΣY² − B·ΣM²,  σ²_asym = b·S_w/(N(B−1))  (pooled over chains),
 * between-chain  σ²_asym ≈ B·b·(ΣM² − (ΣM)²/N)/(N−1)  (valid at stationarity),  ESS_i = N·B·b·Var_π,i/σ²_asym,i
 * (zigzagboomerang.jl_amd/ess.py).  ZigZag flows only (a FactBoomerang path rotates between events: PDMP_ERR_UNSUPPORTED, as for
 * pdmp_ensemble_batch_means).
 */
pdmp_status pdmp_ensemble_ess_begin(pdmp_ensemble* ens, double T0);
pdmp_status pdmp_ensemble_ess_batch(pdmp_ensemble* ens, double T);
pdmp_status pdmp_ensemble_ess_end(pdmp_ensemble* ens, double* sum_y, double* sum_y2, double* sum_m, double* sum_m2,
                                  int64_t* nbatches, double* T0, double* T1);

/*
 * The engine keeps ∫ x_i dt per chain and coordinate next to the state (what batch_means / ess_* / path_integrals read; the reference has no
 * such thing).  enable = 0 drops it: those calls then return PDMP_ERR_INVALID, and the kernels that hold a chain's state on chip (small d:
 * the subsampled logistic target, pdmp_logistic.hip) fit 13 chains per CU instead of 8 (config C4, d = 442: 11.9 against 18.7 KB of LDS per chain; measured 105 against 133 ms per step).  Default: kept.  Call before set_state.
 */
pdmp_status pdmp_ensemble_set_path_integrals(pdmp_ensemble* ens, int enable);

/*
 * J_i(T) = ∫_{t0}^{T} x_i(s) ds of EVERY chain at `nprobe` probe coordinates (0-based): out is [nchains x nprobe] row-major.  All chains
 * paused with PDMP_RUN_STOP_BEFORE at T.  Differences of successive calls are per-chain batch integrals, from which the host forms any
 * ESS estimator (batch means at several batch lengths, between-chain variances: zigzagboomerang.jl_amd/ess.py: multiscale_ess) while the
 * N x d records stay on the device.  ZigZag flows only, like pdmp_ensemble_batch_means.
 */
pdmp_status pdmp_ensemble_path_integrals(pdmp_ensemble* ens, double T, int64_t nprobe, const int64_t* probes, double* out);

/* ------------------------------------------------------------------ sticky ZigZag (PDMP_SAMPLER_STICKY_ZIGZAG)
 *
 * sspdmp(∇ϕ, t0, x0, θ0, T, c, F::ZigZag, κ, args...; reversible=false, strong_upperbounds=false, factor=1.5, adapt)
 * (src/ss_fact.jl:159-160,217).  Call after set_flow_zigzag / set_target_gaussian_csc and before set_state: kappa is the
 * [d] vector of thaw rates.  Events are FactTrace events (freeze, thaw and reflection alike, :154); the counters' nacc/num
 * are the reference's scalar (acc, num) (:175,214).  The refresh clock is not implemented by the reference (:86).
 */
pdmp_status pdmp_ensemble_set_sticky(pdmp_ensemble* ens, const double* kappa, int reversible, int strong_upperbounds);

/* ------------------------------------------------------------------ ZigZag with sticky and reflecting barriers (PDMP_SAMPLER_BARRIER_ZIGZAG)
 *
 * stickyzz(u0, target::StructuredTarget, flow::StickyFlow, upper_bounds::StickyUpperBounds, barriers::Vector{<:StickyBarriers}, end_condition)
 * (src/stickyzz.jl:176-319): every coordinate has a lower and an upper barrier at arbitrary levels (StickyBarriers, :19-25), each with a rule
 * acting when the coordinate thaws -- PDMP_BARRIER_STICKY keeps the saved speed, _REFLECT negates it, _REVERSIBLE flips its sign by a coin -- and a
 * thaw rate kappa > 0; kappa = +Inf is an instantaneous wall.  All arrays are [d], shared by the chains; lo = -Inf or hi = +Inf means no barrier on
 * that side.  Box constraints, truncated Gaussians, positivity constraints, sticking at levels other than 0.
 *
 * Call after set_flow_zigzag and set_target_gaussian_csc, before set_state.  Refusals, never a silent fall-back:
 *   set_barriers  PDMP_ERR_INVALID for lo > hi, kappa <= 0 or NaN, a rule outside 0..2.
 *   set_flow_zigzag on such an ensemble: PDMP_ERR_INVALID for a Γ without a diagonal entry.
 *   set_state     PDMP_ERR_INVALID for theta0[i] == 0 (the reference's dir() would index out of bounds) and for x0[i] outside a box [lo, hi]
 *                 with lo < hi.  lo == hi is one level met from either side, as sspdmp2's (0, 0): any start is allowed.
 *   set_state     PDMP_ERR_UNSUPPORTED for anything but: a ZigZag flow without refresh, the Gaussian target, G = G1 (no set_neighbourhood),
 *                 no gradient tracking / LocalBound, neighbourhoods of at most 64 members (what the one-event sticky kernel takes) with
 *                 |G1[i]| <= 63, an explicit state.  pdmp_ensemble_set_adaptscale itself returns PDMP_ERR_UNSUPPORTED on such an ensemble.
 * pdmp_ensemble_consume_begin returns PDMP_ERR_UNSUPPORTED (the device consumers' "time away from 0" has no meaning here):
 * pdmp_ensemble_barrier_consume_begin, below with the trace consumers, is the entry for such an ensemble; the host consumers work on the
 * returned trace as before.  One event after every hit, thaw and accepted reflection; the counters' nacc / num are the reference's scalar acc.
 * The path integrals (pdmp_ensemble_path_integrals, batch_means, ess_*) are kept: a frozen coordinate contributes its barrier level.
 * pdmp_ensemble_final_state's acc then holds action[i] (0 hit, 1 reflect, 2 unfreeze, :170-175).
 *
 * pdmp_ensemble_final_barrier: frozen [n x d] (1 where v[i] == 0 && v_old[i] != 0, :266) and theta_saved [n x d] = v_old (the ensemble's own
 * array of saved speeds, which no other getter returns); either may be NULL.
 */
#define PDMP_BARRIER_STICKY 0
#define PDMP_BARRIER_REFLECT 1
#define PDMP_BARRIER_REVERSIBLE 2
pdmp_status pdmp_ensemble_set_barriers(pdmp_ensemble* ens, const double* lo, const double* hi, const int32_t* rule_lo, const int32_t* rule_hi,
                                       const double* kappa_lo, const double* kappa_hi, int strong_upperbounds);
pdmp_status pdmp_ensemble_final_barrier(pdmp_ensemble* ens, int64_t chain_first, int64_t n, uint8_t* frozen, double* theta_saved);
/* The same for a sticky ZigZag (PDMP_SAMPLER_STICKY_ZIGZAG, src/ss_fact.jl): frozen [n x d] (1 where x[i] == 0 && theta[i] == 0, :108) and
 * theta_saved [n x d], the ensemble's array of saved speeds: for a frozen coordinate the speed its thaw gives back (never 0).  What the array
 * holds for a coordinate that is not frozen is the kernel's own business (zz_precision_run_kernel: 0).  Either may be NULL.  LocalBound, whose
 * renewal flags share the array, is refused on a sticky ensemble.  (Added under ABI version 3.) */
pdmp_status pdmp_ensemble_final_sticky(pdmp_ensemble* ens, int64_t chain_first, int64_t n, uint8_t* frozen, double* theta_saved);

/* ------------------------------------------------------------------ adaptscale (σ tuning in the refresh branch)
 *
 * spdmp(...; adaptscale=true) (src/sfact.jl:74,86-99,163): each refresh of coordinate i first retunes F.σ[i] -- ZigZag:
 * log σ[i] is pulled towards 0.3 accepted reflections per unit time and θ[i] = σ[i]·sign(θ[i]) is set WITHOUT a random draw
 * (:87-91); FactBoomerang: σ[i] *= exp(±0.03·min(1, √(τ/λref))) once τ = (1+2ρ/(1−ρ))/(t[i]·λref) < 0.2 (:93-98).  The
 * reference mutates F.σ in place; here σ becomes per-chain device state, initialised from the flow's sigma at set_state
 * and read back with pdmp_ensemble_final_sigma ([n x d]).  Needs a refresh clock (lambda_ref > 0), PDMP_SAMPLER_ZIGZAG_LOCAL
 * and the Gaussian target.  Call after set_flow_* and before set_state.  x^y is evaluated as pdmp_exp(y·pdmp_log x).
 */
pdmp_status pdmp_ensemble_set_adaptscale(pdmp_ensemble* ens, int enable);
pdmp_status pdmp_ensemble_final_sigma(pdmp_ensemble* ens, int64_t chain_first, int64_t n, double* sigma);

/* ------------------------------------------------------------------ tracked gradients (an evaluation strategy, not a sampler)
 *
 * enable = 1: the local ZigZag loop keeps, per coordinate, g_i = Γ[:,i]·x and gd_i = Γ[:,i]·θ instead of moving G[i] and gathering them at
 * every proposal (src/sfact.jl:82,116): a proposal then touches its own record only and an accepted reflection its G1 neighbours
 * -- about half the HBM traffic of the moving evaluation.  Same process, same draws, same thinning decisions: the event INDEX sequence,
 * accept / reject outcomes, (acc, num) and adapted bounds equal the reference's exactly; event times, positions and the final
 * (t, x, θ) agree to ~1e-13 relative instead of bit for bit, because sums that are advanced are not rounded like sums that are
 * recomputed (tests/test_gpu_track_parity.py: 1e-9; the default, enable = 0, stays bit-identical).  "Exactly" holds until a float
 * difference of that size flips an accept test or the order of two nearly simultaneous events -- measured on the north-star workload: one chain
 * in 4096 after 1.7e9 proposals, about 6e-10 per proposal (tools/track_soak.py); from there on that chain is another realisation of the same
 * process (the draws land on different events), not a wrong one.  pdmp_ensemble_final_state rebuilds
 * the reference's lazy clocks t[j] (src/sfact.jl:211) from the times of the last proposal / accept around j.
 * Requirements (else set_state returns PDMP_ERR_UNSUPPORTED -- never a silent fall-back): PDMP_SAMPLER_ZIGZAG_LOCAL, ZigZag flow
 * without refresh, Gaussian target, symmetric Γ, lattice-like neighbourhoods (|G1| <= 5, |S| <= 13) and 2048 <= d <= 16384.
 * With the LOGISTIC target (config C4; the same requirements on the flow, G = Matched(), a state that fits the LDS-resident kernel) the
 * BOUNDS are tracked and the subsampled gradient stays the moving evaluation: a proposal moves coordinate i and what its sampled rows read,
 * a rejection re-derives its bound from (g_i, gd_i, tg_i), an accepted event updates the k members of G1[i] instead of moving its two-hop
 * set and summing every member's column afresh.  The oracle's spdmp_zigzag_tracked_lg states it sequentially; the device equals it bit for
 * bit; the final clocks t[j] are the tracked process's own (a coordinate is as old as its last own event or visit by a sampled row).
 * Call before set_state.
 */
pdmp_status pdmp_ensemble_set_gradient_tracking(pdmp_ensemble* ens, int enable);

/* ------------------------------------------------------------------ c::LocalBound (src/local.jl)
 *
 * spdmp(∇ϕ, t0, x0, θ0, T, C::LocalBound, F::ZigZag, args...) (src/local.jl:95-149): the bound of coordinate j is built from the
 * target's own directional derivatives, b[j] = (c_j + ∇ϕj·θ_j, c_j/100 + vj, 2/c_j/|θ_j|) (:2-6) with (∇ϕj, vj) =
 * (Γt[:,j]·x − Γt[:,j]·μt, θ_j·Γt[:,j]·θ) for the Gaussian target (the `(∇ϕi, vi)` callback of performance/smartbound.jl:45-59),
 * and expires after its horizon: next_time (src/not_fact_samplers.jl:43-50) queues min(proposal, horizon) and a `renew` flag;
 * a renew event re-bounds j without a thinning step (:36-43).  The queue is initialised with t0 + τ (:122).  ZigZag flow without
 * refresh clock, Gaussian target whose pattern equals the flow's, PDMP_SAMPLER_ZIGZAG_LOCAL.  Call after set_flow / set_target,
 * before set_state; `c` of set_state is then LocalBound(c).c.
 * Ties: coordinates with equal c_i/|θ_i| re-bounded at the same instant get EXACTLY equal horizon keys; the reference pops tied
 * keys in heap order (src/priorityqueue.jl:46-77), this engine by lowest index.  Both are valid orders of simultaneous events of
 * independent clocks, but the random streams then pair differently: bit parity with the reference needs distinct c_i/|θ_i|.
 * With pdmp_ensemble_set_neighbourhood: PDMP_ERR_UNSUPPORTED from set_state.  src/local.jl:95-149 knows ONE graph -- its argument G is moved,
 * re-bounded member by member and gives G2 -- while the neighbourhood tables re-bound G1 = the pattern of F.Γ only: pass a flow matrix that
 * carries G's pattern (explicit zeros) instead.
 */
pdmp_status pdmp_ensemble_set_local_bound(pdmp_ensemble* ens, int enable);

/* ------------------------------------------------------------------ Bouncy particle sampler (PDMP_SAMPLER_BPS)
 *
 * pdmp(∇ϕ!, t0, x0, θ0, T, c, B::BouncyParticle; adapt, factor=2.0) -> Ξ::PDMPTrace, (t, x, θ), (acc, num), c
 * (src/not_fact_samplers.jl:117-147,395-396) with GlobalBound(c) and the Gaussian target ∇ϕ!(y, x) = Γ(x − μ)
 * (test/maintest.jl:163).  Γ is B.Γ: it enters ab() (:26-28) and -- unless pdmp_ensemble_set_target_gaussian_csc is called AFTER this
 * (accepted on this family: ∇ϕ!(y, x) = Γt(x − μt) of its own; ab(…GlobalBound…) keeps B.Γ, B.μ, LocalBound takes θ'∇ϕx and θ'Γtθ) -- the target.  The mass factor B.L =
 * cholesky(Symmetric(Γ)).L (src/types.jl:43) is identity for Γ = I (config C2); for any other Γ the caller must hand it over
 * with pdmp_ensemble_set_mass_cholesky before set_state_bps, which otherwise returns PDMP_ERR_UNSUPPORTED.
 * Events are (t, copy(x), copy(θ)) (:39-41); dot products use the fixed summation order stated in oracle/pdmp_oracle.c.
 */
pdmp_status pdmp_ensemble_set_flow_bps(pdmp_ensemble* ens, const int64_t* colptr, const int64_t* rowval,
                                       const double* nzval, const double* mu, double lambda_ref, double rho);

/* Flow = Boomerang(Γ, μ_flow, λref; ρ) (src/types.jl:59-66): Hamiltonian rotation about μ_flow between events
 * (src/dynamics.jl:29-36), grad_correct! ∇ϕx −= L'\(L\(x − μ_flow)) (src/not_fact_samplers.jl:9-12), constant bound
 * (√(‖θ‖² + ‖x − μ_flow‖²)·c, 0, Inf) (:34-36); same pdmp_inner! loop, events, counters and entry points as the bouncy
 * particle (create the ensemble with PDMP_SAMPLER_BPS).  The CSC matrix and mu_target describe the TARGET
 * ∇ϕ!(y, x) = Γt(x − μt) (test/maintest.jl:146).  The flow's own Γ enters only through its factor L = cholesky(Symmetric(Γ)).L
 * (src/types.jl:66), which the caller MUST hand over with pdmp_ensemble_set_mass_cholesky before set_state_bps (an identity factor for
 * Γ = I): without one set_state_bps returns PDMP_ERR_UNSUPPORTED -- never a silent L = I. */
pdmp_status pdmp_ensemble_set_flow_boomerang(pdmp_ensemble* ens, const int64_t* colptr, const int64_t* rowval,
                                             const double* nzval, const double* mu_target, const double* mu_flow,
                                             double lambda_ref, double rho);
/*
 * Mass factor F.L of BouncyParticle / Boomerang (src/types.jl:43,66): a LOWER-triangular d x d matrix in CSC form (rows
 * ascending, hence the diagonal entry first in its column; non-zero diagonal).  Used by reflect!
 * θ .-= (2⟨∇ϕx,θ⟩/‖L\∇ϕx‖²)·L'\(L\∇ϕx) (src/dynamics.jl:90-97), refresh! θ = ρθ + ρ̄·L'\randn(d) (:112-126) and Boomerang's
 * grad_correct! (src/not_fact_samplers.jl:9-12).  The reference factorises inside the constructor (dense LAPACK, or CHOLMOD with
 * its fill-reducing permutation for a sparse Γ, whose `.L` is the factor of the PERMUTED matrix); the caller -- the Julia shim
 * passes `sparse(B.L)` -- owns that choice, the engine only solves with what it is given, by column-oriented substitution in
 * the order oracle/pdmp_oracle.c states.  Call after set_flow_bps / set_flow_boomerang and before set_state_bps.
 */
pdmp_status pdmp_ensemble_set_mass_cholesky(pdmp_ensemble* ens, const int64_t* colptr, const int64_t* rowval,
                                            const double* nzval);
/*
 * local_bound: `c` of set_state_bps is LocalBound(c).c -- ab = (c + ⟨θ,∇ϕx⟩, v, 2√d/c/‖θ‖₂) with v = θ'Γθ (the second
 * directional derivative a `(∇ϕx, v)` gradient callback returns for the Gaussian target), next_time's horizon and the renew
 * branch of pdmp_inner! (src/not_fact_samplers.jl:29-31,43-50,65-71); BouncyParticle only.
 * subsample: kwarg `subsample` (:53,90): an accepted reflection does not end pdmp_inner!, only refreshments are recorded.
 * Call after set_flow_* and before set_state_bps.
 */
pdmp_status pdmp_ensemble_set_bps_options(pdmp_ensemble* ens, int local_bound, int subsample);
/* x0, theta0: [nchains x d]; c: the scalar bound constant (GlobalBound(c) or LocalBound(c)); seeds: [nchains] */
pdmp_status pdmp_ensemble_set_state_bps(pdmp_ensemble* ens, double t0, const double* x0, const double* theta0, double c,
                                        const uint64_t* seeds);
/* events [first, first+count) of one chain: t [count], x and theta [count x d] (any may be NULL) */
pdmp_status pdmp_ensemble_bps_trace_copy(pdmp_ensemble* ens, int64_t chain, int64_t first, int64_t count, double* t,
                                         double* x, double* theta);
/* final (t, x, θ) and adapted c of chains [chain_first, chain_first+n): t, c are [n]; x, theta are [n x d] */
pdmp_status pdmp_ensemble_bps_final_state(pdmp_ensemble* ens, int64_t chain_first, int64_t n, double* t, double* x,
                                          double* theta, double* c);
/*
 * Path moments of BouncyParticle / Boomerang (no counterpart in the reference; the exact time averages its trace's mean would approximate).
 * order 1 keeps J1 = ∫_{t0}^{t} x dt, order 2 also J2 = ∫_{t0}^{t} x² dt, per chain and coordinate, in the event loop's registers: every
 * segment adds its closed form -- linear, or the Boomerang's rotation about μ_flow.  Opt-in (default 0): order 0 runs the kernels of a
 * plain ensemble, and with order >= 1 the events, counters and state are bit for bit those of order 0 -- only the moments are added, so a
 * run with trace_capacity 0 gives posterior means and variances without writing a single event.  PDMP_SAMPLER_BPS only; call after
 * set_flow_bps / set_flow_boomerang and before set_state_bps (which starts the moments at t0); PDMP_ERR_INVALID otherwise, for an order
 * outside 0..2, or once a state exists.  set_flow_* resets the order to 0.
 */
pdmp_status pdmp_ensemble_set_bps_moments(pdmp_ensemble* ens, int order);
/*
 * j1 = ∫_{t0}^{T} x dt and j2 = ∫_{t0}^{T} x² dt of chains [chain_first, chain_first + n): host [n x d] row-major arrays; j2 may be NULL
 * (non-NULL needs order 2).  Every chain in the range must satisfy t <= T <= its next scheduled event (refreshment or proposal) with
 * status OK or TRACE_FULL -- what a run with PDMP_RUN_STOP_BEFORE at T leaves; otherwise PDMP_ERR_INVALID naming the chain (a
 * reference-tail run leaves the clock past T; a TRACE_FULL pause may leave the next event before T).
 * On a BPS ensemble with order >= 1, pdmp_ensemble_batch_means, pdmp_ensemble_ess_begin / _batch / _end, pdmp_ensemble_path_integrals and
 * pdmp_ensemble_reduce_moments read J1 at their T under the same rule and mean what they mean for the ZigZag (with order 0 they refuse as
 * for any BPS ensemble).
 */
pdmp_status pdmp_ensemble_bps_moments(pdmp_ensemble* ens, double T, int64_t chain_first, int64_t n, double* j1, double* j2);

/*
 * sspdmp(∇ϕ!, t0, x0, θ0, T, c, Flow::Union{BouncyParticle,Boomerang}, κ, ...; strong_upperbounds) (src/ss_not_fact.jl:104-201): the sticky
 * Bouncy Particle / Boomerang.  Every coordinate freezes when it hits 0 and thaws after an Exp(κ_i |θf_i|) time; reflections and refreshments
 * act on the free coordinates; every event carries the free mask f.  The trace begins with the event (t0, x0, θ0, all free) (:189).
 * kappa: [d] thaw-rate factors (> 0).  PDMP_SAMPLER_BPS; after set_flow_bps / set_flow_boomerang, before set_state_bps.  d <= 1024.
 * The loop never reads the mass factor of a BouncyParticle (set_state_bps does not ask for one and ignores one that was given); a Boomerang
 * needs the identity factor handed over explicitly (grad_correct!), a general one is refused.  Not combined with c::LocalBound, subsample or
 * pdmp_ensemble_set_bps_moments(order >= 1): set_state_bps returns PDMP_ERR_UNSUPPORTED naming the option.  A freeze that finds
 * |x_i| > 1e-8 (the reference's error(...), :129-132) and a violated bound without adapt end the chain as PDMP_CHAIN_BOUND_VIOLATED.
 * PDMP_ERR_INVALID: a kappa entry <= 0 or not finite, NULL, a state exists, another sampler.  set_flow_* clears the setting.
 * pdmp_ensemble_bps_trace_copy / _bps_final_state, the counters and trace_reset work as on a plain ensemble.
 */
pdmp_status pdmp_ensemble_set_bps_sticky(pdmp_ensemble* ens, const double* kappa, int strong_upperbounds);
/* f of events [first, first+count) of one chain: [count x d] bytes, 1 = free (sevent, :100-102) */
pdmp_status pdmp_ensemble_bps_trace_free_copy(pdmp_ensemble* ens, int64_t chain, int64_t first, int64_t count, uint8_t* f);
/* final free mask and saved speeds θf of chains [chain_first, chain_first+n): [n x d] each, either may be NULL */
pdmp_status pdmp_ensemble_bps_final_sticky(pdmp_ensemble* ens, int64_t chain_first, int64_t n, uint8_t* f, double* theta_f);

/*
 * pdmp(dϕ, ∇ϕ!, t0, x0, θ0, T, c::LocalBound, flow::BouncyParticle; oscn, adapt, factor) (src/not_fact_samplers.jl:151-384, "ModernBPS"): the
 * speed-recorded Bouncy Particle.  It bounds with both directional derivatives dϕ = (θ'Γt(x−μt), θ'Γtθ) and an expiry horizon, redraws the
 * refreshment time with every bound, refreshes and RECORDS in proportion to the speed V = record_rate(θ): a record (t, x, θ) every 1/λref of
 * speed-time ∫V dt, and nothing else -- the trace is the sample, no discretize pass is needed.  The trace does not begin with (t0, x0, θ0).
 *   u_diag  NULL: the L form, V ≡ 1, the mass factor L is the identity or what pdmp_ensemble_set_mass_cholesky hands over (reflect!
 *           :161-164, refresh! :173-180);  [d] > 0: the diagonal-U form, U = PDiagMat(u): reflect! with z = u .* ∇ϕx, refresh! with
 *           unwhiten = √u .* z, V = ‖θ ./ √u‖ (:156-172, :197).
 *   oscn    the orthogonal-subspace Crank-Nicolson bounce of src/oscn.jl (normalize = false) instead of reflect!; L = I only.
 * Call order, on a PDMP_SAMPLER_BPS ensemble: set_flow_bps_modern; pdmp_ensemble_set_target_gaussian_csc or
 * pdmp_ensemble_set_target_bps_logistic (a target is REQUIRED: this flow has no Γ of its own); optionally pdmp_ensemble_set_mass_cholesky (L form only); pdmp_ensemble_set_state_bps(t0, x0, θ0, c, seeds) with c = LocalBound(c).c.
 * adapt / factor are the ensemble configuration's.  d <= 1024.
 * set_state_bps returns PDMP_ERR_UNSUPPORTED naming the option for: d > 1024; set_bps_moments(order >= 1); set_bps_sticky; set_bps_options
 * (subsample or local_bound: they belong to the other driver, this one always bounds locally and always subsamples); oscn with u_diag or with
 * a mass factor that is not the identity; u_diag together with a mass factor.  PDMP_ERR_INVALID: lambda_ref <= 0, |rho| > 1, a u_diag entry
 * <= 0 or not finite, a missing target or a c that is not finite and > 0 (at set_state_bps), another sampler, a state exists.  Any set_flow_* clears the setting.
 * Records go to the BPS trace buffer: pdmp_ensemble_bps_trace_copy / _bps_final_state, trace_reset, the counters and the gather of BPS traces
 * serve them unchanged.  nevents counts records, num / nacc are the reference's, nrefresh counts refreshments.  l > lb without adapt (at a
 * record or at an accepted proposal) ends the chain as PDMP_CHAIN_BOUND_VIOLATED; the reference's `@assert Δrec > 0` failing ends it as
 * PDMP_CHAIN_STALLED.  PDMP_RUN_REFERENCE_TAIL stops at the first record with t >= T; PDMP_RUN_STOP_BEFORE pauses before any event, record
 * or expiry at a time >= T; sliced, drained (PDMP_CHAIN_TRACE_FULL) and paused (PDMP_CHAIN_PAUSED) runs continue bit for bit.
 */
pdmp_status pdmp_ensemble_set_flow_bps_modern(pdmp_ensemble* ens, double lambda_ref, double rho, const double* u_diag, int oscn);
/*
 * `T::Int` of the reference: a chain stops once nevents == n (0: no limit).  May be raised between runs to continue; a run takes whichever of
 * T and n comes first (pass T = +Inf for the count alone).  After set_flow_bps_modern (which resets it to 0); PDMP_ERR_INVALID otherwise or for n < 0.
 */
pdmp_status pdmp_ensemble_set_bps_record_limit(pdmp_ensemble* ens, int64_t n);
/*
 * A Bayesian logistic regression as the target of the speed-recorded driver: the reference's own application of it (turing/lr.jl:105-139,
 * tilde/lr.jl:55-98, the docstring at src/not_fact_samplers.jl:285-334).  A is the n x d design in CSC (column = coordinate, rows ascending,
 * explicit zeros allowed), At its transpose in CSC (column = observation), y[n] successes and m[n] trials with 0 <= y_i <= m_i, gamma0 >= 0 a
 * scalar prior precision.  With η = A x, ζ = A θ and p_i = 1 / (1 + pdmp_exp(−η_i)):
 *   ϕ(x)    = Σ_i [ m_i log(1 + e^{η_i}) − y_i η_i ] + (γ0/2)‖x‖²
 *   ∇ϕ!(x)  = Aᵀ r + γ0 x,                   r_i = m_i p_i − y_i
 *   dϕ(x,θ) = ( Σ_i r_i ζ_i + γ0 θ·x ,  Σ_i m_i p_i (1 − p_i) ζ_i² + γ0 θ·θ )
 * Call order, on a PDMP_SAMPLER_BPS ensemble: set_flow_bps_modern; this call IN PLACE OF pdmp_ensemble_set_target_gaussian_csc (the later of
 * the two wins); optionally set_mass_cholesky; set_bps_record_limit; set_state_bps.  u_diag, oscn, adapt / factor, the counters, bps_trace_copy,
 * bps_final_state, trace_reset, the BPS trace gather and pdmp_ensemble_bps_consume_* serve it unchanged; sliced, drained and paused runs
 * continue bit for bit (every chain carries η from launch to launch).
 * PDMP_ERR_INVALID: NULL; n <= 0; A / At inconsistent (nnz differ, colptr[0] != 0, rows out of range or not ascending, At not the transpose
 * pattern of A); y / m out of range or not finite; gamma0 < 0 or not finite; another sampler; a state exists.
 * set_state_bps returns PDMP_ERR_UNSUPPORTED naming the cause for a flow other than set_flow_bps_modern (plain set_flow_bps, Boomerang,
 * sticky) and where 8 d + 16 n bytes (the [d] staging buffer, η and ζ in LDS) exceed 160 KiB.
 */
pdmp_status pdmp_ensemble_set_target_bps_logistic(pdmp_ensemble* ens, int64_t n, const int64_t* A_colptr, const int64_t* A_rowval,
                                                  const double* A_nzval, const int64_t* At_colptr, const int64_t* At_rowval,
                                                  const double* At_nzval, const double* y, const double* m, double gamma0);

/* ------------------------------------------------------------------ trace consumers on the device (what callers do next with Ξ)
 *
 * mean(Ξ) (src/trace.jl:182-200) and collect(discretize(Ξ, dt)) (:94-125) of every chain's FactTrace, computed from the engine's trace
 * buffer slice by slice, so that a trace set far larger than the buffer (config C3: 8 MB per chain x 4096) is consumed without ever leaving
 * the device:
 *   consume_begin(grid_dt, grid_points)  after set_state, before the first run: snapshots (t0, x0, θ0) as every coordinate's cursor;
 *                                        grid_points > 0 reserves [nchains x grid_points x d] doubles for the grid t0 + k·grid_dt;
 *   consume()                            after EVERY run slice and before trace_reset: applies the buffered events (each coordinate's in
 *                                        order) -- the trapezoid sums of mean, the grid points a finished segment covers;
 *   consume_mean(chain_first, n, ...)    mean [n x d] and the last event time T of each chain (the reference's scale 1/(2T));
 *   consume_inclusion(chain_first, n, ...)  inclusion_prob [n x d] (:161-178: time with x_i ≠ 0 before or after an event of i, over T);
 *   consume_discretized(chain, k_first, k_count, out, npoints, grid_dev)
 *                                        rows k_first .. of chain's grid positions [k_count x d] (row k belongs to time t0 + k grid_dt; row 0 is
 *                                        x0); *npoints = number of grid times the reference would emit so far (those before the chain's last
 *                                        event; at least t0) -- NOT clamped: a value above grid_points means the grid of consume_begin was too
 *                                        short and the later rows were dropped; *grid_dev = the whole device array, for consumers that stay on the
 *                                        device.  Any of the three may be NULL.
 * Time-ordered traces of piecewise-linear paths only: ZigZag flow without refresh clock (spdmp, pdmp, sspdmp).  Values are those of
 * zigzagboomerang.jl_amd/trace.py (discretize: bitwise; mean: the same sums scaled once instead of term by term).
 */
pdmp_status pdmp_ensemble_consume_begin(pdmp_ensemble* ens, double grid_dt, int64_t grid_points);
pdmp_status pdmp_ensemble_consume(pdmp_ensemble* ens);
/* The same beside the sampler (ABI 3): what the last pdmp_ensemble_run (on `stream`, 0 = the ensemble's own) wrote is consumed on a second stream of
 * the ensemble and the trace segments are handed back EMPTY at once -- no pdmp_ensemble_trace_reset; the next run writes the other of two trace
 * buffers while this slice is consumed, and waits only for the consumer of the slice before it.  The reference returns Ξ (src/sfact.jl:211) and
 * callers then run discretize / mean over it (src/trace.jl:106-125,182-200): at the sampler's rate (32 B per event) a C3 trace exceeds what PCIe
 * drains, so this is how a full-rate run is USED.  Returns without waiting; consume_mean / _inclusion / _discretized and every entry point that
 * reads state wait for the consumers.  pdmp_ensemble_last_consume_ms: kernel time of the last asynchronous consumer (waits for it). */
pdmp_status pdmp_ensemble_consume_async(pdmp_ensemble* ens, void* stream);
pdmp_status pdmp_ensemble_last_consume_ms(pdmp_ensemble* ens, float* ms);
pdmp_status pdmp_ensemble_consume_mean(pdmp_ensemble* ens, int64_t chain_first, int64_t n, double* mean, double* T_last);
/* inclusion_prob(Ξ) (src/trace.jl:161-178) per chain: the fraction of [t0, T] each coordinate spent away from 0 -- what a sticky run is made for */
pdmp_status pdmp_ensemble_consume_inclusion(pdmp_ensemble* ens, int64_t chain_first, int64_t n, double* prob, double* T_last);
pdmp_status pdmp_ensemble_consume_discretized(pdmp_ensemble* ens, int64_t chain, int64_t k_first, int64_t k_count, double* out,
                                              int64_t* npoints, void** grid_dev);
/* cummean(Ξ) (src/trace.jl:203-226) on the device (round 6): once enabled (after consume_begin; the synchronous consumer), pdmp_ensemble_consume also leaves,
 * for every event of the segment it consumes, the running pair (t_i, Σ (x_prev + x_k)(t_k − t_prev) / (2 t_i)) of the event's coordinate -- the sums are
 * carried from segment to segment, so the pairs are those of the whole run's trace (bit for bit the reference's order of operations per coordinate).
 * _copy: the pairs of slots [first, first + count) of a chain's segment, the slots pdmp_ensemble_trace_copy returns the events of. */
pdmp_status pdmp_ensemble_consume_cummean(pdmp_ensemble* ens, int enable);
pdmp_status pdmp_ensemble_consume_cummean_copy(pdmp_ensemble* ens, int64_t chain, int64_t first, int64_t count, double* t, double* y);
/* subtrace(Ξ, J) (src/trace.jl:275-290) on the device (round 6): the events of a chain's current trace segment whose coordinate lies in the ascending
 * 0-based index set J, renumbered by their position in J, compacted on the device; n_out = how many there are (at most out_cap are written to `out`). */
pdmp_status pdmp_ensemble_subtrace_copy(pdmp_ensemble* ens, int64_t chain, const int64_t* J, int64_t nJ, pdmp_event* out, int64_t out_cap,
                                        int64_t* n_out);
/* The same consumers for a PDMP_SAMPLER_BARRIER_ZIGZAG ensemble (stickyzz, sspdmp2), with the barrier OCCUPATION in place of inclusion_prob.
 *   barrier_consume_begin(grid_dt, grid_points)  call order, argument checks and allocation of consume_begin; PDMP_ERR_INVALID on any other
 *       sampler.  Afterwards consume, consume_mean, consume_discretized, consume_cummean(_copy), subtrace_copy, consume_condition(ed),
 *       consume_pairs / consume_pair_integrals and pdmp_debug_trace_append serve the ensemble unchanged.  consume_async and consume_inclusion
 *       return PDMP_ERR_UNSUPPORTED.  The cursors start from the path the chain travels: θ = 0 for a coordinate that starts frozen on the
 *       barrier of its θ0 (src/stickyzz.jl:198-208), not the θ0 a returned trace records.
 *   barrier_consume_occupation(chain_first, n, z_lo, z_hi, n_lo, n_hi, T_last)  per chain and coordinate, [n x d] each: the time spent frozen
 *       (θ = 0) at the lower / upper barrier and the number of hits of each, as raw sums over [t0, T_last] (they pool exactly over chains);
 *       T_last [n] is the time of the chain's last consumed event, to which a coordinate still frozen is extended.  A coordinate is frozen
 *       from an event with θ = 0 to its next event; the side is that of its speed before the hit (upper iff > 0), at t0 that of θ0.  A wall
 *       (kappa = +Inf) counts one hit and no time.  1 − (z_lo + z_hi) / (T_last − t0) is sspdmp2's posterior inclusion probability.  Any
 *       output may be NULL; the stored sums are not modified.  PDMP_ERR_INVALID before barrier_consume_begin or for a chain range outside the
 *       ensemble.  zigzagboomerang.jl_amd/trace.py: barrier_occupation is the host mirror, bit for bit. */
pdmp_status pdmp_ensemble_barrier_consume_begin(pdmp_ensemble* ens, double grid_dt, int64_t grid_points);
pdmp_status pdmp_ensemble_barrier_consume_occupation(pdmp_ensemble* ens, int64_t chain_first, int64_t n, double* z_lo, double* z_hi,
                                                     uint64_t* n_lo, uint64_t* n_hi, double* T_last);
/* The same consumers for the flows with a refresh clock: a ZigZag with λref > 0 and a FactBoomerang (whose refresh clock is mandatory), whatever
 * kernel samples them.  A refresh records the refreshed coordinate at its own, stale clock (src/sfact.jl:84-85,143), so these traces are sorted
 * within a coordinate only; the reference's consumers take them in trace order (src/trace.jl:106-125,182-226), and so does this form:
 *   refresh_consume_begin(grid_dt, grid_points)  call order, argument checks and allocation of consume_begin.  PDMP_ERR_INVALID for a ZigZag
 *       without refresh clock (pdmp_ensemble_consume_begin serves it), a BPS, sticky or barrier ensemble, trace_capacity = 0, a call before
 *       set_state or after the first run, grid_points < 0 or grid_points > 0 with grid_dt <= 0.  Afterwards consume, consume_mean,
 *       consume_discretized, consume_cummean(_copy), subtrace_copy and pdmp_debug_trace_append serve the ensemble unchanged; consume_async,
 *       consume_condition, consume_pairs, consume_hist and consume_inclusion return PDMP_ERR_UNSUPPORTED (their cursors walk a sorted trace).
 *   Row k (time g = t0 + k·grid_dt) shows the LEADING events of the trace applied, up to but not including the first one whose time exceeds g:
 *       a stale event behind that one is not applied to row k although its time is <= g; it is applied to the next row.  Per coordinate the row
 *       is x + θ·τ, τ = g − (the coordinate's cursor time); a FactBoomerang: (x − μ)·c + θ·s + μ, (s, c) = pdmp_sincos(τ) of pdmp_detmath.h.  A row
 *       exists while g is below the running maximum of the event times: *npoints counts those (at least 1, NOT clamped to grid_points).
 *   T_last of consume_mean -- the reference's scale 1/(2T) -- is the time of the last consumed event in trace order, which need not be the maximum.
 * tests/ref/refresh_trace_ref.c states this sequentially and the device agrees with it bit for bit. */
pdmp_status pdmp_ensemble_refresh_consume_begin(pdmp_ensemble* ens, double grid_dt, int64_t grid_points);

/* ------------------------------------------------------------------ trace consumers of the Bouncy Particle family (PDMPTrace)
 *
 * mean(Ξ), cummean(Ξ) and collect(discretize(Ξ, dt)) of a PDMPTrace (src/trace.jl:129-150, 229-266) -- event-recorded BouncyParticle and
 * Boomerang, their sticky forms, the speed-recorded BouncyParticle -- computed from the BPS trace buffers slice by slice, in the manner of the
 * calls above: one event of this family is 8(2d + 1) bytes, and these three are what callers copy the trace to the host for.
 *   bps_consume_begin(grid_dt, grid_points)  after set_state_bps, before the first run: (t0, x0, θ0) become every coordinate's cursor, a sticky
 *                                        ensemble starts all free; grid_points > 0 reserves [nchains x grid_points x d] doubles, row 0 = x0;
 *   bps_consume()                        after EVERY run slice and before trace_reset; per event (t2, x2, θ2[, f2]): the grid rows t0 + k·grid_dt < t2
 *                                        from the cursor (x + θ·τ; a Boomerang (x − μ)·cos τ + θ·sin τ + μ with pdmp_sincos of pdmp_detmath.h; a
 *                                        coordinate that is not free keeps x), then y += (x + x2)(t2 − t), then the cursor moves to the event;
 *                                        its kernel time is what pdmp_ensemble_last_consume_ms returns afterwards;
 *   bps_consume_mean(chain_first, n, ...)  y / T_last [n x d] as the reference writes it (:229-246: no ½) and T_last [n] (t0 before any event);
 *   bps_consume_inclusion(...)           sticky ensembles only (PDMP_ERR_INVALID otherwise): the fraction of [t0, T_last] each coordinate was free
 *                                        (1, the initial mask, where T_last <= t0);
 *   bps_consume_discretized(...)         the contract of pdmp_ensemble_consume_discretized: rows [k_first, k_first + k_count) of a chain;
 *                                        *npoints = the number of k with t0 + k·grid_dt < T_last, at least 1, NOT clamped to grid_points;
 *   bps_consume_cummean(enable)          bps_consume also leaves y / (2·t2) [d] at every consumed event's slot (:263; 0/0 = NaN at t2 = 0);
 *   bps_consume_cummean_copy(chain, first, count, y)   those rows [count x d], the slots pdmp_ensemble_bps_trace_copy returns the events of.
 * Values are those of zigzagboomerang.jl_amd/trace.py up to the order of summation and, for a Boomerang, pdmp_sincos against libm's sin / cos;
 * tests/ref/pdmp_trace_ref.c states the arithmetic sequentially and the device agrees with it bit for bit.  PDMP_ERR_INVALID on an ensemble that
 * is not PDMP_SAMPLER_BPS, for begin after a run / with trace_capacity = 0 / with grid_points > 0 and grid_dt <= 0, for the others before begin.
 */
pdmp_status pdmp_ensemble_bps_consume_begin(pdmp_ensemble* ens, double grid_dt, int64_t grid_points);
pdmp_status pdmp_ensemble_bps_consume(pdmp_ensemble* ens);
pdmp_status pdmp_ensemble_bps_consume_mean(pdmp_ensemble* ens, int64_t chain_first, int64_t n, double* mean, double* T_last);
pdmp_status pdmp_ensemble_bps_consume_inclusion(pdmp_ensemble* ens, int64_t chain_first, int64_t n, double* prob, double* T_last);
pdmp_status pdmp_ensemble_bps_consume_discretized(pdmp_ensemble* ens, int64_t chain, int64_t k_first, int64_t k_count, double* out,
                                                  int64_t* npoints, void** grid_dev);
pdmp_status pdmp_ensemble_bps_consume_cummean(pdmp_ensemble* ens, int enable);
pdmp_status pdmp_ensemble_bps_consume_cummean_copy(pdmp_ensemble* ens, int64_t chain, int64_t first, int64_t count, double* y);

/* ------------------------------------------------------------------ conditional trace on the device (src/condition.jl)
 *
 * collect(conditional_trace(Ξ, (p, n))): the points where the sampled path crosses the hyperplane H = {x : <x − p, n> = 0}; the crossing times
 * weighted by |<θ, n>| sample the target restricted to H (x_i = a, x_i = x_j, a contrast over a block, a diffusion bridge through a point:
 * problems.bridge_point_condition).  Collected by the synchronous consumers above, slice by slice, without the trace leaving the device.
 * The contract is the closed form from the cursors, at most ONE hit per linear piece (the reference recomputes the hitting time from the point it
 * just put on the plane and may emit a crossing twice; DESIGN.md "Conditional trace"); every dot product in the 64-lane order of the
 * device's wave sum; tests/ref/condition_ref.c states it sequentially and the device agrees with it bit for bit.
 *   FactTrace (whatever consume_begin accepts).  S = the indices with n_j != 0, 1 <= |S| <= 1024.  A piece opens at t_b: t0, afterwards the time
 *     of the latest event of a coordinate of S.  With the cursors of S as of t_b: xs_k = x_c + θ_c (t_b − t_c), g = Σ n_k (p_k − xs_k),
 *     h = Σ n_k θ_c,k, τ = g / h, s = t_b + τ.  A candidate iff τ > 0; a hit, once, when the next event of S arrives at t_e >= s or the chain's
 *     last consumed event time T_last >= s.  Row: x_c + θ_c (s − t_c) for every j from j's last event with t < s, else from (t0, x0_j, θ0_j).
 *   PDMPTrace (event-recorded BouncyParticle and its sticky form).  Per event (t_k, ...) with the cursor (t_c, x_c, θ_c, f_c) before it:
 *     τ = <p − x_c, n> / <θ_c, n>; a hit iff τ > 0 and t_c + τ < t_k, at t_c + τ, row_j = f_c,j ? x_c,j + θ_c,j τ : x_c,j.
 *   [bps_]consume_condition(p, n, max_hits)   after [bps_]consume_begin and before the first [bps_]consume: reserves [nchains x max_hits] times
 *     and [nchains x max_hits x d] rows (the factorised family also 24 bytes of cursor per chain and coordinate).  Without this call nothing
 *     changes: no allocation, no kernel.  pdmp_ensemble_consume_async on such an ensemble: PDMP_ERR_UNSUPPORTED.
 *   [bps_]consume_conditioned(chain, first, count, t, x, nhits, rows_dev)   rows [first, first + count) of a chain, first + count <= max_hits;
 *     *nhits is NOT clamped to max_hits (a value above it: later rows were dropped); *rows_dev = the whole device array; any output may be NULL.
 * PDMP_ERR_INVALID: NULL / non-finite p or n, n = 0, max_hits < 1 or rows beyond 256 GiB, before begin, after the first consume (a
 * consume_async that handed a slice over counts), the other family's ensemble.
 * PDMP_ERR_UNSUPPORTED: |S| > 1024 on a FactTrace (a PDMPTrace has no such limit); a Boomerang flow (hittingtime has no method, src/condition.jl:18); the speed-recorded flow or subsample
 * (their records are not the corners of the path).
 */
pdmp_status pdmp_ensemble_consume_condition(pdmp_ensemble* ens, const double* p, const double* n, int64_t max_hits);
pdmp_status pdmp_ensemble_consume_conditioned(pdmp_ensemble* ens, int64_t chain, int64_t first, int64_t count, double* t, double* x,
                                              int64_t* nhits, void** rows_dev);
pdmp_status pdmp_ensemble_bps_consume_condition(pdmp_ensemble* ens, const double* p, const double* n, int64_t max_hits);
pdmp_status pdmp_ensemble_bps_consume_conditioned(pdmp_ensemble* ens, int64_t chain, int64_t first, int64_t count, double* t, double* x,
                                                  int64_t* nhits, void** rows_dev);

/* ------------------------------------------------------------------ pair integrals on the device: covariance of a sampled path
 *
 * S_ij = ∫ (x_i − c_i)(x_j − c_j) dt and J_i = ∫ (x_i − c_i) dt, exactly, over a caller-given sparse set of pairs (the diagonal, the pattern of
 * Γ, a dense block): cov_ij = S_ij / L − (J_i / L)(J_j / L) with L = T_last − t0, the quantity the reference's own acceptance test reads
 * (test/maintest.jl: mean|cov(xs) − Γ⁻¹| < 2.5/√T).  Kept by the synchronous consumers above, slice by slice; raw integrals pool exactly over
 * chains and ranks.  Plain double arithmetic, no fused multiply-add; tests/ref/pairs_ref.c states the contract sequentially and the device
 * agrees with it bit for bit (DESIGN.md "Pair integrals").
 *   A piece of the pair (i, j) over [s0, s1] with the states a = x_i(s0) − c_i, b = x_j(s0) − c_j, the velocities vi, vj and τ = s1 − s0 adds
 *     τ·(a·b + τ·(0.5·(a·vj + b·vi) + τ·((vi·vj)/3.0))) to S_ij; a coordinate's own piece adds τ·(a + 0.5·(vi·τ)) to J_i.  τ is taken signed.
 *   FactTrace (whatever consume_begin accepts).  Cursors of its own (t, x, θ, J per chain and coordinate, from (t0, x0, θ0, 0)).  An event
 *     (t, i, x, θ), in trace order: for every listed pair (i, j), s0 = max(t_i, t_j), a = (x_i − c_i) + θ_i·(s0 − t_i), b likewise from j's
 *     cursor, the piece [s0, t]; then J_i gets [t_i, t] and i's cursor becomes (t, x, θ).  A read closes every pair from max(t_i, t_j) and
 *     every J_i from t_i to the chain's last consumed event time T_last, without touching the accumulators: a run can be read midway.
 *   PDMPTrace (event-recorded BouncyParticle and its sticky form).  Per event (t_k, ...) with the cursor (t_c, x_c, θ_c, f_c) before it every
 *     pair's piece is [t_c, t_k] with a = x_c,i − c_i, vi = f_c,i ? θ_c,i : 0.  Nothing is added behind the last event.
 *   [bps_]consume_pairs(npairs, pi, pj, center)   after [bps_]consume_begin and before the first [bps_]consume: pairs 0-based, in any
 *     orientation, stored in the given order; center [d] or NULL = 0.  Reserves [nchains x npairs] doubles (the factorised family also 32 bytes
 *     of cursor per chain and coordinate, the Bouncy Particle family [nchains x d] for J).  Without this call nothing changes: no allocation,
 *     no kernel.  Coexists with consume_condition and consume_cummean.  pdmp_ensemble_consume_async on such an ensemble: PDMP_ERR_UNSUPPORTED.
 *   [bps_]consume_pair_integrals(chain_first, n, S, J, T_last, S_dev)   S [n x npairs], J [n x d] (every coordinate, listed or not), T_last [n]
 *     of chains [chain_first, chain_first + n); *S_dev = the device array the S just read lie in ([n x npairs]); any output may be NULL.
 * PDMP_ERR_INVALID: npairs < 1 or >= 2^30, a NULL list, an index outside [0, d), a pair listed twice (either orientation), a non-finite
 * centre, accumulators beyond 256 GiB, before begin, after the first consume (a consume_async that handed a slice over counts), the other
 * family's ensemble.
 * PDMP_ERR_UNSUPPORTED: the Bouncy Particle family on a Boomerang flow (the product of two rotations is another integral), on the
 * speed-recorded flow or with subsample (their records are not the corners of the path).
 */
pdmp_status pdmp_ensemble_consume_pairs(pdmp_ensemble* ens, int64_t npairs, const int64_t* pi, const int64_t* pj, const double* center);
pdmp_status pdmp_ensemble_consume_pair_integrals(pdmp_ensemble* ens, int64_t chain_first, int64_t n, double* S, double* J, double* T_last,
                                                 void** S_dev);
pdmp_status pdmp_ensemble_bps_consume_pairs(pdmp_ensemble* ens, int64_t npairs, const int64_t* pi, const int64_t* pj, const double* center);
pdmp_status pdmp_ensemble_bps_consume_pair_integrals(pdmp_ensemble* ens, int64_t chain_first, int64_t n, double* S, double* J, double* T_last,
                                                     void** S_dev);

/* ------------------------------------------------------------------ pair integrals of arcs: covariance of a Boomerang path
 *
 * The same S_ij = ∫ (x_i − z_i)(x_j − z_j) dt and J_i = ∫ (x_i − z_i) dt over [t0, T_last] for the event-recorded Boomerang and the sticky
 * Boomerang, whose pieces are arcs about the flow's μ (DESIGN.md "Pair integrals of arcs"; tests/ref/arc_pairs_ref.c states the contract
 * sequentially and the device agrees with it bit for bit).  Plain double arithmetic, no fused multiply-add, pdmp_sincos of pdmp_detmath.h.
 *   Per event (t_k, ...) with the cursor (t_c, x_c, θ_c, f_c) before it, τ = t_k − t_c signed; per coordinate  u = x_c − μ, p = θ_c, m = μ − z
 *   (free) or u = 0, p = 0, m = x_c − z (not free), so that x(s) − z = u·cos s + p·sin s + m.  Once per piece:
 *     (s, c) = pdmp_sincos(τ);  h = s·c
 *     Icc = 0.5·(τ + h)   Iss = 0.5·(τ − h)   Isc = 0.5·(s·s)   Ic = s   Is = c > 0 ? (s·s)/(1.0 + c) : 1.0 − c
 *     S_ij += (((ui·uj)·Icc + (pi·pj)·Iss) + (ui·pj + uj·pi)·Isc) + ((mi·(uj·Ic + pj·Is) + mj·(ui·Ic + pi·Is)) + (mi·mj)·τ)
 *     J_i  += (u·Ic + p·Is) + m·τ
 *   Symmetric in (i, j) bit for bit.  A τ outside pdmp_sincos's domain (|τ| > 2^30) yields NaN, as the grid rows of discretize do.  Nothing is
 *   added behind the last event.
 *   bps_consume_arc_pairs(npairs, pi, pj, center)   position, arguments, memory and PDMP_ERR_INVALID cases of bps_consume_pairs; center = z.
 *     Without this call nothing changes: no allocation, no kernel.  Coexists with the mean, cummean, the grid and the sticky free-time fractions.
 *   pdmp_ensemble_bps_consume_pair_integrals reads the result (a copy: nothing of it depends on the flow).
 * PDMP_ERR_UNSUPPORTED: a flow that is not a Boomerang (pdmp_ensemble_bps_consume_pairs is the call for lines), the speed-recorded flow,
 * subsample, a second pair list on one ensemble.
 */
pdmp_status pdmp_ensemble_bps_consume_arc_pairs(pdmp_ensemble* ens, int64_t npairs, const int64_t* pi, const int64_t* pj, const double* center);

/* ------------------------------------------------------------------ marginal histograms on the device: occupation times of a sampled path
 *
 * The time each of m listed coordinates spends in each of `bins` bins of its own range [lo_s, hi_s), below the range and at or above it: the
 * exact histogram of the path (between two events a coordinate is a line, so the time in a bin is a closed form; no grid, no discretisation
 * error).  Medians, credible intervals and densities of a marginal follow on the host; the raw times pool exactly over chains and ranks.  Kept
 * by the synchronous consumers above, slice by slice.  Plain double arithmetic, no fused multiply-add; tests/ref/hist_ref.c states the contract
 * sequentially and the device agrees with it bit for bit (DESIGN.md "Marginal histograms").
 *   Bins: w = (hi − lo) / bins, edges e_0 = lo, e_k = lo + w·k, e_bins = hi.  A row has bins + 2 numbers: slot 0 the time below lo, slots 1..bins
 *     the bins [e_k, e_k+1), slot bins + 1 the time at or above hi.
 *   A piece (a, v, τ) -- position at its start, velocity, duration; τ <= 0 adds nothing.  With b = a + v·τ: at rest (v == 0 or b == a) it adds τ
 *     to the slot of a (and, if v == 0, to the coordinate's rest time Z); otherwise with xl = min(a, b), xh = max(a, b), r = τ / (xh − xl) every
 *     bin between those of xl and xh gets (min(xh, e_k+1) − max(xl, e_k))·r where that is positive.
 *   FactTrace (whatever consume_begin or barrier_consume_begin accepts).  Cursors of its own (t, x, θ per chain and listed coordinate, from
 *     (t0, x0, θ0); θ = 0 where a barrier ensemble starts frozen).  An event (t, i, x, θ) of a listed coordinate adds the piece (x_c, θ_c, t − t_c),
 *     then the cursor becomes the event.  A read closes every open piece at the chain's last consumed event time T_last, without touching the
 *     rows: a run can be read midway, and reading twice returns the same bytes.
 *   PDMPTrace (event-recorded BouncyParticle and its sticky form).  Per event (t_k, ...) with the cursor (t_c, x_c, θ_c, f_c) before it every
 *     listed coordinate adds (x_c,i, f_c,i ? θ_c,i : 0, t_k − t_c).  Nothing is added behind the last event.
 *   Σ_k H[k] = T_last − t0 to rounding for every listed coordinate; Z <= Σ_k H[k].
 *   [bps_]consume_hist(m, coords, lo, hi, bins)   after [bps_]consume_begin (or barrier_consume_begin) and before the first [bps_]consume: m
 *     distinct coordinates, 0-based, stored in the given order; lo, hi [m]; 1 <= bins <= 4096.  Reserves [nchains x m x (bins + 2)] doubles (the
 *     factorised family also 32 bytes of cursor per chain and listed coordinate).  Without this call nothing changes: no allocation, no kernel.
 *     Coexists with consume_condition, consume_pairs and consume_cummean.  pdmp_ensemble_consume_async on such an ensemble: PDMP_ERR_UNSUPPORTED.
 *   [bps_]consume_histogram(chain_first, n, pooled, H, Z, T_last, H_dev)   of chains [chain_first, chain_first + n): pooled == 0: H [n x m x
 *     (bins + 2)], Z [n x m]; pooled != 0: H [m x (bins + 2)], Z [m], the chains added in chain order, sequentially per entry.  T_last [n] is
 *     always per chain.  *H_dev = the device array the H just read lie in; any output may be NULL.
 * PDMP_ERR_INVALID: m < 1, a NULL list, an index outside [0, d), a coordinate listed twice, lo >= hi or a non-finite bound, bins outside
 * 1..4096, rows beyond 256 GiB (refused before the lists are read), before begin, after the first consume, the other family's ensemble, a chain
 * range outside the ensemble.
 * PDMP_ERR_UNSUPPORTED: the Bouncy Particle family on a Boomerang flow (an arc is not a line: pdmp_ensemble_bps_consume_arc_hist), on the speed-recorded flow or with subsample
 * (their records are not the corners of the path).
 */
pdmp_status pdmp_ensemble_consume_hist(pdmp_ensemble* ens, int64_t m, const int64_t* coords, const double* lo, const double* hi, int64_t bins);
pdmp_status pdmp_ensemble_consume_histogram(pdmp_ensemble* ens, int64_t chain_first, int64_t n, int pooled, double* H, double* Z, double* T_last,
                                            void** H_dev);
pdmp_status pdmp_ensemble_bps_consume_hist(pdmp_ensemble* ens, int64_t m, const int64_t* coords, const double* lo, const double* hi, int64_t bins);
pdmp_status pdmp_ensemble_bps_consume_histogram(pdmp_ensemble* ens, int64_t chain_first, int64_t n, int pooled, double* H, double* Z,
                                                double* T_last, void** H_dev);

/* ------------------------------------------------------------------ marginal histograms of arcs: occupation times of a Boomerang path
 *
 * The same rows H and rest times Z for the event-recorded Boomerang and the sticky Boomerang, whose pieces are arcs about the flow's μ
 * (DESIGN.md "Marginal histograms of arcs"; tests/ref/arc_hist_ref.c states the contract sequentially and the device agrees with it bit for
 * bit).  Exact, as for lines: no grid.  Plain double arithmetic, no fused multiply-add, pdmp_acos / pdmp_atan2 of pdmp_detmath.h.  Bins, edges,
 * slots and the pooled read are those above.
 *   Per event (t_k, ...) with the cursor (t_c, x_c, θ_c, f_c) before it, τ = t_k − t_c; τ <= 0 adds nothing.  Per listed coordinate:
 *     at rest -- not free, or u = x_c − μ, p = θ_c, R = sqrt(u·u + p·p) == 0: τ to the slot of x_c and to Z;
 *     an arc otherwise: ψ0 = −pdmp_atan2(p, u), ψ1 = ψ0 + τ, and for a level y
 *       z = (y − μ)/R;  z >= 1: below = τ;  z <= −1: below = 0.0;  else α = pdmp_acos(z), L = 2π − 2α,
 *       W(ψ) = n·L + clamp(r − α, 0, L) with n = floor(ψ/2π), r = ψ − 2π·n (2π one double),  below(y) = W(ψ1) − W(ψ0);
 *     the bin [e_k, e_k+1) gets max(0.0, below(e_k+1) − below(e_k)), with e_−1 = −∞ and e_bins+1 = +∞.
 *   Nothing is added behind the last event.  Σ_k H[k] = T_last − t0 to rounding; Z <= Σ_k H[k].
 *   bps_consume_arc_hist(m, coords, lo, hi, bins)   position, arguments, memory and PDMP_ERR_INVALID cases of bps_consume_hist, and
 *     PDMP_ERR_INVALID where nchains x ceil(m / 4) reaches 2^24 (one wavefront per chain and listed coordinate in one launch).  Without this
 *     call nothing changes: no allocation, no kernel.  Coexists with the mean, cummean, the grid, the free-time fractions and
 *     bps_consume_arc_pairs.  pdmp_ensemble_bps_consume_histogram reads the result, per chain or pooled.
 * PDMP_ERR_UNSUPPORTED: a flow that is not a Boomerang (pdmp_ensemble_bps_consume_hist is the call for lines), the speed-recorded flow,
 * subsample, a second list on one ensemble.
 */
pdmp_status pdmp_ensemble_bps_consume_arc_hist(pdmp_ensemble* ens, int64_t m, const int64_t* coords, const double* lo, const double* hi, int64_t bins);

/* what the ensemble was created with (any pointer may be NULL) */
pdmp_status pdmp_ensemble_info(pdmp_ensemble* ens, int64_t* nchains, int64_t* d, int64_t* trace_capacity, int* device);

/* ------------------------------------------------------------------ the post-run exchange of a sharded ensemble (RCCL over xGMI)
 *
 * Chains are independent: rank r of R runs its own block of them with NO collective (one process, one ensemble, one communicator per GPU).
 * What follows a run (nothing in the reference -- it is single-process):
 *   pdmp_comm_unique_id     on ONE rank: an opaque PDMP_COMM_ID_BYTES token (ncclGetUniqueId) the host hands to the other ranks by its own means
 *                           (MPI.jl, a file, a socket: zigzagboomerang.jl_amd/parallel.py uses a TCP rendezvous on MASTER_ADDR);
 *   pdmp_comm_init          on every rank, collectively (ncclCommInitRank on `device`);
 *   pdmp_comm_barrier / pdmp_comm_allreduce (host doubles, PDMP_COMM_SUM | PDMP_COMM_MAX): timing and counter reductions of a benchmark;
 *   pdmp_ensemble_gather_traces   collective.  Every rank learns nchains_by_rank [world] and counts (events in the trace buffer of every
 *                           chain of the whole ensemble, rank-major; counts_cap entries available).  The trace segments travel to `root`:
 *                           ncclAllGather of the counts -> each rank compacts its segments on the device -> ONE grouped ncclSend / ncclRecv
 *                           (a gatherv: every peer streams over its own direct xGMI link).  On root the events of all chains lie back to back in
 *                           rank-major, chain-major order in a device buffer the communicator owns (*events_dev, valid until the next gather on
 *                           it or pdmp_comm_destroy) and, if events_host != NULL, are copied there (events_cap events available);
 *   pdmp_ensemble_reduce_moments  collective: pdmp_ensemble_batch_means on every rank, ncclReduce(sum) of the 2 d sums onto root's sum_y, sum_y2.
 * Calls on one communicator are serialised by the caller.  world = 1 is valid (the same code path on one GPU).
 */
#define PDMP_COMM_ID_BYTES 128
#define PDMP_COMM_SUM 0
#define PDMP_COMM_MAX 1
typedef struct pdmp_comm pdmp_comm;
pdmp_status pdmp_comm_unique_id(void* id, int64_t id_bytes);
pdmp_status pdmp_comm_init(const void* id, int rank, int world, int device, pdmp_comm** out);
void pdmp_comm_destroy(pdmp_comm* comm);
pdmp_status pdmp_comm_info(const pdmp_comm* comm, int* rank, int* world);
pdmp_status pdmp_comm_barrier(pdmp_comm* comm);
pdmp_status pdmp_comm_allreduce(pdmp_comm* comm, double* inout, int64_t n, int op);
pdmp_status pdmp_ensemble_gather_traces(pdmp_ensemble* ens, pdmp_comm* comm, int root, int64_t* nchains_by_rank, uint64_t* counts,
                                        int64_t counts_cap, pdmp_event* events_host, int64_t events_cap, void** events_dev,
                                        int64_t* nevents_total);
/* events [first, first + count) of what the last pdmp_ensemble_gather_traces left on this rank (root), device -> host */
pdmp_status pdmp_comm_gathered_copy(pdmp_comm* comm, pdmp_event* out, int64_t first, int64_t count);
pdmp_status pdmp_ensemble_reduce_moments(pdmp_ensemble* ens, pdmp_comm* comm, int root, double T_prev, double T, double* sum_y,
                                         double* sum_y2);
/* The same exchange for the PDMPTrace of the non-factorised samplers (pdmp on BouncyParticle / Boomerang: events (t, copy(x), copy(θ)),
 * src/not_fact_samplers.jl:39-41, 8 (2 d + 1) bytes each).  On root the events of all chains lie rank-major, chain-major in three device arrays the
 * communicator owns -- t [total], x [total x d], θ [total x d] -- valid until the next gather on it; pdmp_comm_gathered_bps_copy fetches a range
 * (any of t / x / theta may be NULL).  Collective; argument errors of ONE rank (a counts buffer that is too small, a failed allocation) are agreed
 * on before anything is sent, so every rank returns the error and the communicator stays usable -- the same holds for
 * pdmp_ensemble_gather_traces. */
pdmp_status pdmp_ensemble_gather_bps_traces(pdmp_ensemble* ens, pdmp_comm* comm, int root, int64_t* nchains_by_rank, uint64_t* counts,
                                            int64_t counts_cap, void** t_dev, void** x_dev, void** theta_dev, int64_t* nevents_total);
pdmp_status pdmp_comm_gathered_bps_copy(pdmp_comm* comm, double* t, double* x, double* theta, int64_t first, int64_t count);

/* ------------------------------------------------------------------ the one-dimensional samplers
 *
 * pdmp(∇ϕ, x, θ, T, c, Flow::Union{ZigZag1d, Boomerang1d}; adapt = false, factor = 2.0) -> Ξ::Vector{(t, x, θ)}, acc/num
 * (src/zigzagboom1d.jl:34-67; ab :15-16, λ :5-6, move_forward src/dynamics.jl:66-68,79-82) for an ensemble of independent chains, one
 * chain per LANE.  The gradient is the device-resident form of the reference's own test closure (test/test1d.jl:9-10):
 * ∇ϕ(x) = (x − mu)/sigma2 + noise·(rand() − 0.5).  Draw order: the reference's calls on its global generator, in program order, are the
 * draws of the chain's main stream.  One call runs every chain until t >= T, a bound violation (adapt = 0: PDMP_CHAIN_BOUND_VIOLATED, the
 * reference's error(...)) or a full event buffer (PDMP_CHAIN_TRACE_FULL: call again with the returned state -- the run continues exactly
 * where it stopped).  state[k] on the first call: {x, theta, c} = the start, started = 0, everything else 0.  events: host buffer
 * [nchains x trace_capacity], nevents[k] of chain k's row are valid (the first one of a fresh run is (0, x0, θ0), :36).  Host pointers only.
 */
#define PDMP_1D_ZIGZAG 0
#define PDMP_1D_BOOMERANG 1
typedef struct {
    uint32_t struct_size; /* sizeof(pdmp_1d_config) */
    int32_t device;
    int32_t flow;  /* PDMP_1D_ZIGZAG: ZigZag1d(); PDMP_1D_BOOMERANG: Boomerang1d(b_sigma, b_mu, b_lambda) (src/types.jl:82-100) */
    int32_t adapt; /* c *= factor on a violated bound instead of stopping (:54-56) */
    double factor;
    int64_t nchains;
    int64_t trace_capacity;
    double mu, sigma2, noise;        /* the target's gradient (test/test1d.jl:5-10) */
    double b_sigma, b_mu, b_lambda; /* Boomerang1d's Σ, μ, λref */
} pdmp_1d_config;
typedef struct {
    double t, x, theta;
} pdmp_event1d;
typedef struct {
    double t, x, theta, c; /* time, position, velocity, tuning parameter (grows under adapt) */
    double a, b, t_next, t_ref; /* the bound in force, the next proposal and refresh times */
    uint64_t ndraw;             /* draws of the main stream consumed */
    int64_t num, acc;           /* proposals, accepted proposals (:38,51,53) */
    int32_t started, status;    /* status: PDMP_CHAIN_* */
} pdmp_1d_state;
pdmp_status pdmp_1d_run(const pdmp_1d_config* cfg, pdmp_1d_state* state /* [nchains], in/out */, const uint64_t* seeds /* [nchains] */,
                        double T, pdmp_event1d* events /* [nchains x trace_capacity] */, int64_t* nevents /* [nchains] */);

/* raw device pointers for zero-copy consumers (e.g. an RCCL gather of trace segments) */
pdmp_status pdmp_ensemble_trace_dev(pdmp_ensemble* ens, void** events_dev, int64_t* capacity);
pdmp_status pdmp_ensemble_counters_dev(pdmp_ensemble* ens, void** counters_dev);
/* ... of a BouncyParticle / Boomerang ensemble: event times [nchains x capacity], positions and velocities [nchains x capacity x d] */
pdmp_status pdmp_ensemble_bps_trace_dev(pdmp_ensemble* ens, void** t_dev, void** x_dev, void** theta_dev);

#ifdef __cplusplus
}
#endif
#endif /* PDMP_MI355_H */
