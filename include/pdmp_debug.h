/*
 * pdmp_debug.h -- diagnostics and measurement hooks of libpdmp_mi355.so.  NOT part of the drop-in boundary (pdmp_mi355.h): nothing a
 * caller of spdmp / pdmp / sspdmp needs lives here.  Used by tests/ (kernel selection for parity runs, the numerical-contract probe)
 * and tools/ (phase profiles, memory-system probes).  All state is per ensemble; the library keeps no globals and reads no
 * environment variables.
 */
#ifndef PDMP_DEBUG_H
#define PDMP_DEBUG_H

#include <stddef.h>

#include "pdmp_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Which event-loop kernel a local-ZigZag / sticky ensemble uses.  AUTO: the widest speculative kernel the neighbourhood geometry
 * admits (8 events per iteration on lattice-like graphs, else 4, else 1); SEQ: one event per iteration; SPEC4: the 4-event kernel
 * where the 8-event one would run.  All of them produce the same event sequence bit for bit (tests/test_gpu_spec8_parity.py).
 * Must be called before set_flow_*. */
#define PDMP_DEBUG_KERNEL_AUTO 0
#define PDMP_DEBUG_KERNEL_SEQ 1
#define PDMP_DEBUG_KERNEL_SPEC4 2
#define PDMP_DEBUG_KERNEL_SPEC8 3 /* the 8-event kernel (8-lane groups): what AUTO runs for the moving evaluation on a lattice */
#define PDMP_DEBUG_KERNEL_EXACTP 4 /* the one-proposal-per-lane kernel of the moving evaluation (bit-identical; slower) */
pdmp_status pdmp_debug_set_kernel(pdmp_ensemble* ens, int kernel);
/* 4-event kernel: fetch the G2 records of every proposal speculatively instead of on accept only */
pdmp_status pdmp_debug_set_spec_g2(pdmp_ensemble* ens, int on);
/* Record the per-phase cycle counts of chain 0 during the following runs (a profiling instantiation of the same loop);
 * pdmp_debug_phase_profile returns the last run's 16 numbers: kind 1 (speculative kernels) [0..8] cycles per phase, [10] iterations;
 * kind 2 (general kernel) [0..6] select, move G1, gradient, coin + G2, re-bound, re-queue, tail, [10] proposals. */
pdmp_status pdmp_debug_set_phase_profile(pdmp_ensemble* ens, int on);
pdmp_status pdmp_debug_phase_profile(pdmp_ensemble* ens, double* out16, int* kind);
/* gradient tracking: which kernel runs where the one-proposal-per-lane kernel applies (plain lattice graph, no adaptation, 2048 <= d <= 16384).
 * 0 = default (zz_local_trackp_kernel: (key, t_old) pairs in blocks of 8, one dirty line per rejected proposal), 1 = the 8-lane-group kernel
 * (zz_local_track_kernel, which also serves adaptation, a target mean, a looser bounding Γ and lattice-like graphs) -- both compute the same
 * floats and commit the same sequence.  The choice fixes the queue's layout: call it BEFORE set_state.  (Rounds 1-2 carried two more
 * variants, key blocks of 32 and of 16 in the record layout; they were superseded and removed.) */
pdmp_status pdmp_debug_set_track_groups(pdmp_ensemble* ens, int which);
/* zz_local_trackp_kernel / zz_local_trackp2_kernel: the two-wave form gives every chain a helper wavefront (the chain's uniforms and their
 * logarithms produced ahead into a ring in LDS, the next windows' lines requested early); same committed sequence and floats.  -1 = chosen by
 * the ensemble's width (at most seven chains per compute unit, 1792 on an MI355X), 0 = never, 1 = always.  Before the next run. */
pdmp_status pdmp_debug_set_helper_wave(pdmp_ensemble* ens, int mode);
/* zz_local_trackp_kernel: how the chains that share a SIMD for a whole launch set their wave priority.  0 = in turns of 256 iterations (every
 * event loop's rule), 1 = by rank of progress: the waves of a SIMD post how far they are through the launch on a board in device memory and the
 * one furthest behind issues first (the one-wave forms up to d = 16384; the two-wave form and the form beyond d = 16384 take turns whatever is
 * set), -1 = the default, which is 1.  No result depends on it.  Before the next run. */
pdmp_status pdmp_debug_set_prio_policy(pdmp_ensemble* ens, int mode);
/* zz_local_trackl_kernel (round 6): the same event loop on the LINE layout -- a coordinate pair's (key, t_old) pairs, sums and constants in one
 * 128-byte line, nine-bit wheel images of the pair minima in LDS -- which is what ensembles of more than 12 chains per compute unit run on the
 * plain lattice with an even side (d <= 16384); same committed sequence and floats.  -1 = by the ensemble's width, 0 = never, 1 = wherever the
 * layout serves.  The choice fixes the state's layout: call it BEFORE set_state.  With this kernel pdmp_debug_set_helper_steering's first two
 * arguments are the block minima per quantum of the wheel and the events a window aims at (0: the defaults). */
pdmp_status pdmp_debug_set_track_lines(pdmp_ensemble* ens, int mode);
/* Device addresses of the ensemble's large arrays (tracked records, (key, t_old) pairs, trace slots, chain headers, canonical records, keys,
 * per-coordinate constants, tables): tools/mode_alloc.py relates the full-width slice's timing mode to where they landed. */
pdmp_status pdmp_debug_buffer_addresses(pdmp_ensemble* ens, uint64_t* out8);
/* How the arrays of several GB were laid over the device's three memory classes (csrc/pdmp_place.hip), as text: per array the class of every 1 GB
 * chunk in address order, the chunks created while looking for the classes and the seconds that took -- or "hipMalloc" where the array was not placed. */
pdmp_status pdmp_debug_placement(pdmp_ensemble* ens, char* buf, size_t nbuf);
/* Where the arrays lie.  tune: 1 (the default) = set_state times a short launch of a device-filling ZigZag ensemble, re-allocates the pairs / keys and the
 * records with hipMalloc and keeps the fastest combination (the "timing mode" of a full-width launch belongs to those allocations: DESIGN.md 5); 0 = take
 * what hipMalloc gives; -1 = leave as is.  place: 1 = EXPERIMENTAL chunk-wise placement over the device's three memory classes (csrc/pdmp_place.hip -- its
 * header says why it is off), with optional class patterns ("012", "0", ...) for the records, the pairs and the trace; 0 = off.  Before set_state. */
pdmp_status pdmp_debug_set_placement(pdmp_ensemble* ens, int tune, int place, const char* rec, const char* kp, const char* ev);
/* Copies one array (0 records, 1 pairs, 2 trace, 3 headers, 4 constants, 5 keys) into newly allocated memory and continues on the copy; the old
 * allocation stays reserved until the process ends (so that the copy lands on other pages).  For tools/mode_alloc.py only. */
pdmp_status pdmp_debug_move_buffer(pdmp_ensemble* ens, int which);
/* ... its tuning (none of it changes a result): the selection threshold moves by `gain` of the way towards `target` raw candidates per iteration;
 * the helper requests the lines of the blocks within `ahead` window lengths beyond the current window */
pdmp_status pdmp_debug_set_helper_steering(pdmp_ensemble* ens, double gain, int target, double ahead);
/* PDMP_CHAIN_PAUSED under test: a chain pauses once ONE launch has used n draws of its main stream (the subsampled-logistic kernel: n proposals)
 * instead of 3 * 2^30; 0 restores the default */
pdmp_status pdmp_debug_set_launch_count_limit(pdmp_ensemble* ens, uint32_t n);
/* pdmp_ensemble_consume_async: -1 = the consumer runs beside the next slice where the ensemble leaves SIMDs idle (at most 2048 chains) and between
 * the slices where it fills the device (measured: beside a full-width C3 launch it costs the launch more than its own time), 0 / 1 = always between / beside */
pdmp_status pdmp_debug_set_consumer_overlap(pdmp_ensemble* ens, int mode);
/* what the host could drain instead of consuming on the device: `bytes` of the ensemble's trace buffer copied to pinned host memory, GB/s */
pdmp_status pdmp_debug_host_drain_probe(pdmp_ensemble* ens, int64_t bytes, double* gbps);
/* name of the event-loop kernel the last pdmp_ensemble_run launched (bench.py prints it with every line: no figure without its kernel) */
pdmp_status pdmp_debug_last_kernel(pdmp_ensemble* ens, char* out, int64_t cap);
/* chains per wavefront of the LDS-resident logistic kernel (config C4): -1 the library's default, 0 one chain (pdmp_logistic.hip), 16 or 32 =
 * rows of that many lanes, 4 or 2 chains per wavefront (pdmp_logrows.hip); an ensemble that does not fit the rows asked for is refused at run */
pdmp_status pdmp_debug_set_logistic_rows(pdmp_ensemble* ens, int row_width);
/* one-event kernel: print the first n proposals of chain 0 to stderr during the next run */
pdmp_status pdmp_debug_set_proposal_dump(pdmp_ensemble* ens, int64_t n);

/*
 * Test hook: evaluate the shared numerical contract (include/pdmp_detmath.h) on the device for draws
 * k = 0..n-1 of `seed`; out is [8 x n] row-major: u01, pdmp_log(u), a/b, sqrt, poisson_time, pdmp_randn, pdmp_exp, sin+2cos of pdmp_sincos.
 * A host evaluation of the same expressions must agree bit-for-bit (tests/test_gpu_detmath.py).
 */
pdmp_status pdmp_debug_math_probe(int device, uint64_t seed, int64_t n, double* out);

/*
 * Test hook: evaluate ONE small scalar function of the device at the points (a[k], b[k], c[k]), k = 0..n-1; out is [2 x n] row-major,
 * row 1 holds the second output of the two-output functions and 0 otherwise.  There is one id per function of the shared contract and,
 * for poisson_time, sigmoid and pos (defined once, csrc/pdmp_device.hpp), one per unit that uses it: the function is probed by a kernel of
 * that translation unit, i.e. as compiled there under the library's flags (the _L forms receive L = pdmp_log(c)).  The host evaluates the
 * same ids with the oracle: the results must agree bit for bit (tests/test_gpu_detmath.py).  The probe kernels exist only in the parity
 * library (-DPDMP_EXTRA_KERNELS); the default library answers PDMP_ERR_UNSUPPORTED.  The comment of each such id names the unit and the
 * shared function it calls (tests/test_abi.py checks that against the sources).
 */
/* include/pdmp_detmath.h */
#define PDMP_MATH_U01 0        /* pdmp_bits_to_u01 of the 64 bits of a */
#define PDMP_MATH_LOG 1        /* pdmp_log(a) */
#define PDMP_MATH_EXP 2        /* pdmp_exp(a) */
#define PDMP_MATH_SINCOS 3     /* pdmp_sincos(a): sin, cos */
#define PDMP_MATH_SINCOS2PI 4  /* pdmp_sincos2pi(a): sin, cos */
#define PDMP_MATH_RANDN 5      /* pdmp_randn_from_u(a, b) */
#define PDMP_MATH_RANDN2 6     /* pdmp_randn2_from_u(a, b): z0, z1 */
#define PDMP_MATH_RANDINT 7    /* pdmp_randint(seed = 64 bits of a, PDMP_STREAM_GLOBAL, draw (uint64_t)b, n (uint32_t)c) */
#define PDMP_MATH_DIV 8        /* a / b */
#define PDMP_MATH_SQRT 9       /* sqrt(a) */
/* poisson_time(a, b, u = c), one id per unit that uses it */
#define PDMP_MATH_PT_DEV 16      /* pdmp_kernels.hip poisson_time */
#define PDMP_MATH_PT_DEV_L 17    /* pdmp_kernels.hip poisson_time_L */
#define PDMP_MATH_PT_BPS 18      /* pdmp_bps.hip poisson_time */
#define PDMP_MATH_PT_BPS_L 19    /* pdmp_bps.hip poisson_time_L_ref */
#define PDMP_MATH_PT_D1 20       /* pdmp_1d.hip poisson_time */
#define PDMP_MATH_PT_G 21        /* pdmp_general.hip poisson_time */
#define PDMP_MATH_PT_G_L 22      /* pdmp_general.hip poisson_time_L */
#define PDMP_MATH_PT_Q 23        /* pdmp_partition.hip poisson_time */
#define PDMP_MATH_PT_W_L 24      /* pdmp_trackp.hip poisson_time_L */
#define PDMP_MATH_PT_LOGISTIC_L 25 /* pdmp_logistic.hip poisson_time_L */
#define PDMP_MATH_PT_TRACKL_L 26 /* pdmp_trackl.hip poisson_time_L */
#define PDMP_MATH_PT_X_L 27      /* pdmp_exactp.hip poisson_time_L */
#define PDMP_MATH_PT_R_L 28      /* pdmp_logrows.hip poisson_time_L */
/* sigmoid(a) */
#define PDMP_MATH_SIGMOID_G 32        /* pdmp_general.hip sigmoid */
#define PDMP_MATH_SIGMOID_LOGISTIC 33 /* pdmp_logistic.hip sigmoid */
#define PDMP_MATH_SIGMOID_R 34        /* pdmp_logrows.hip sigmoid */
/* pos(a) */
#define PDMP_MATH_POS_DEV 40      /* pdmp_kernels.hip pos_part */
#define PDMP_MATH_POS_BPS 41      /* pdmp_bps.hip pos_part */
#define PDMP_MATH_POS_D1 42       /* pdmp_1d.hip pos_part */
#define PDMP_MATH_POS_G 43        /* pdmp_general.hip pos_part */
#define PDMP_MATH_POS_Q 44        /* pdmp_partition.hip pos_part */
#define PDMP_MATH_POS_W 45        /* pdmp_trackp.hip pos_part */
#define PDMP_MATH_POS_LOGISTIC 46 /* pdmp_logistic.hip pos_part */
#define PDMP_MATH_POS_TRACKL 47   /* pdmp_trackl.hip pos_part */
#define PDMP_MATH_POS_X 48        /* pdmp_exactp.hip pos_part */
#define PDMP_MATH_POS_R 49        /* pdmp_logrows.hip pos_part */
pdmp_status pdmp_debug_math_eval(int device, int fn, int64_t n, const double* a, const double* b, const double* c, double* out);
/*
 * Test hook: the scalars of the sticky Bouncy Particle / Boomerang loop as compiled inside pdmp_bps.hip, at (a[k], b[k], c[k]); out is [n].
 * fn 0: pdmp_atan(a); 1: the linear freezing_time(x = a, θ = b) (src/ss_fact.jl:10-16); 2: the Boomerang's freezing_time(x = a, θ = b, μ = c)
 * (src/ss_not_fact.jl:5-20).  The host restatement (tests/ref/sticky_notfact_ref.c) must agree bit for bit wherever the value is a number or
 * an infinity.  Where it is a NaN -- a NaN argument, or x = 0 with θ = 0 (0/0) -- both sides return a NaN; its sign and payload are outside the
 * contract (the default NaN of a 0/0 differs between x86-64 and gfx950), and the loop never lets a NaN clock win.  In every build of the library.
 */
pdmp_status pdmp_debug_sticky_eval(int device, int fn, int64_t n, const double* a, const double* b, const double* c, double* out);

/*
 * Test hook (parity build only, like pdmp_debug_math_eval; PDMP_ERR_UNSUPPORTED elsewhere): the scalars of the barrier ZigZag as compiled inside
 * pdmp_barrier.hip, at (a[k], b[k], c[k]); out is [2 x n] (second row: a second output, else 0).  The host restatements (orc_poisson_time3 of
 * the oracle, tests/ref/stickyzz_ref.c) must agree bit for bit.
 */
#define PDMP_BARRIER_FN_PT3_L 0 /* poisson_time3_L(a, b, 0.01, pdmp_log(c)): poisson_time((a, b, 0.01), u = c), src/poissontime.jl:39-65 */
#define PDMP_BARRIER_FN_HIT 1   /* barrier_hitting_time(x = a, v = b, barrier = c), src/stickyzz.jl:119-127 */
#define PDMP_BARRIER_FN_RATES 2 /* barrier_rates(a, b, c, 1.0): pos(a), pos(b + c), src/stickyzz.jl:129-135 */
pdmp_status pdmp_debug_barrier_eval(int device, int fn, int64_t n, const double* a, const double* b, const double* c, double* out);

/*
 * Test hooks one layer above the scalars (parity build only, like pdmp_debug_math_eval; PDMP_ERR_UNSUPPORTED elsewhere): the 64-lane primitives
 * and the first-level codes of the queues, each CALLED by a probe kernel of the unit that owns it (an anonymous-namespace helper can be reached
 * from nowhere else).  tests/wave_tables.py and tests/queue_tables.py hold the edge tables and a plain reference of every id;
 * tests/test_gpu_wave_primitives.py and tests/test_gpu_queue_codes.py hold the device to them.
 *
 * pdmp_debug_wave_eval: in0, in1 and out are [nrows x 64] 64-bit words -- the bit image of a double, or a u32 in the low half (the high half of
 * such an output is 0).  One 64-lane workgroup per row; out[row][lane] is what that lane holds after the call.
 */
/* csrc/pdmp_device.hpp, probed in pdmp_kernels.hip */
#define PDMP_WAVE_MIN_F64 0     /* wave_min_f64: every lane (wave-uniform) */
#define PDMP_WAVE_GRP8_MIN_F64 1 /* grp8_min_f64: every lane of each group of 8 */
#define PDMP_WAVE_ROW_MIN_F64 2 /* row_min_f64: every lane of each row of 16 */
#define PDMP_WAVE_MIN_U32 3     /* wave_min_u32: every lane */
#define PDMP_WAVE_MIN_U32_DPP 4 /* wave_min_u32_dpp: every lane */
#define PDMP_WAVE_SCAN_ADD_U32 5 /* scan_add_u32: inclusive prefix sum mod 2^32, every lane */
#define PDMP_WAVE_SCAN_MIN_F64 6 /* scan_min_f64: inclusive prefix minimum, every lane */
#define PDMP_WAVE_BPERM_F64 7   /* bperm_f64(v = in0, src = the low half of in1, 0..63) */
#define PDMP_WAVE_SUM_F64 8     /* pdmp_bps_common.hpp wave_sum_f64, probed in pdmp_bps.hip: every lane */
#define PDMP_WAVE_GRP8_MIN_U32 9 /* pdmp_trackp.hip w_grp8_min_u32: every lane of each group of 8 */
pdmp_status pdmp_debug_wave_eval(int device, int fn, int64_t nrows, const uint64_t* in0, const uint64_t* in1, uint64_t* out);

/* pdmp_debug_queue_eval: one helper at the points (a[k], b[k], c[k]); out is [2 x n] as in pdmp_debug_math_eval.  Integer arguments are given and
 * integer results returned as exactly representable doubles. */
#define PDMP_QUEUE_P_ENC 0  /* pdmp_trackp.hip p_enc(key = a, tb = b, pos = c) */
#define PDMP_QUEUE_P_THR 1  /* pdmp_trackp.hip p_thr(tau = a, tb = b) */
#define PDMP_QUEUE_P_DEC 2  /* pdmp_trackp.hip p_dec(bits = a, tb = b) */
#define PDMP_QUEUE_Q_ENC 3  /* pdmp_exactp.hip q_enc(key = a, tb = b, pos = c) */
#define PDMP_QUEUE_Q_THR 4  /* pdmp_exactp.hip q_thr(tau = a, tb = b) */
#define PDMP_QUEUE_Q_DEC 5  /* pdmp_exactp.hip q_dec(bits = a, tb = b) */
#define PDMP_QUEUE_TL_Q 6   /* pdmp_trackl.hip tl_q(t = a, tref = b, s = c) */
#define PDMP_QUEUE_BELOW 7  /* pdmp_device.hpp pdmp_below(a), probed in pdmp_kernels.hip */
#define PDMP_QUEUE_HB 8     /* pdmp_trackl.hip hb_word(b = a) in row 0, hb_bit(b = a) in row 1 */
#define PDMP_QUEUE_NB_HAS 9 /* pdmp_trackp.hip nb_has(nb = the bit images of a (x, y) and b (z, w), v = c given twice): 1 or 0 */
#define PDMP_QUEUE_NB_COUNT 10 /* pdmp_trackp.hip nb_count(nb = the bit images of a and b) */
/* (the selection's mask pass, same entry point, numbered on with the ids above: a whole-pass helper, not a code of the queue's tables) */
#define PDMP_SELECT_P_MASK32 11 /* pdmp_trackp.hip p_mask32(kk, thr = a): entry j = c is b, the others 0 (odd j) and 0x7f7fffff (even j); the 32-bit mask */
pdmp_status pdmp_debug_queue_eval(int device, int fn, int64_t n, const double* a, const double* b, const double* c, double* out);

/* pdmp_debug_state_eval: the helpers that keep a state in LDS, run by ONE wavefront on a given list of nchg changes (idx[k], val[k]) applied in order.
 *   WHEEL     img_set / img_get: the planes are cleared, write k is img_set(b = idx[k] < 8192, w9 = val[k] < 512), out [8192] is img_get of every
 *             block (keys, nkeys, d, has_refresh unused).
 *   LEVEL1    level1_build over keys [nkeys = nblk x 64, nblk <= 512], then per change keys[idx[k]] = val[k] and level1_update;
 *             out is [4 x nblk]: bk and bi after the build, bk and bi after the changes; then [nchg x 2]: the entry (bk, bi) of the changed key's
 *             block right after each update.
 *   S8_LEVEL1 s8_build_level1<true>(d, has_refresh) over keys [nkeys = nblk x 32], the refresh slot keys[d] (d < nkeys) parked at +Inf after the
 *             build as the kernels do, then s8_level1_update per change; out is [4 x 512] (the entries past nblk are part of the contract), then [nchg x 2] as above.
 * PDMP_ERR_INVALID for an index outside its array. */
#define PDMP_STATE_WHEEL 0     /* pdmp_trackl.hip img_set, img_get */
#define PDMP_STATE_LEVEL1 1    /* pdmp_device.hpp level1_build, level1_update, probed in pdmp_kernels.hip */
#define PDMP_STATE_S8_LEVEL1 2 /* pdmp_spec8_common.hpp s8_build_level1, s8_level1_update, probed in pdmp_kernels.hip */
pdmp_status pdmp_debug_state_eval(int device, int fn, int64_t nkeys, const double* keys, int64_t d, int has_refresh, int64_t nchg, const uint32_t* idx,
                                  const double* val, double* out);

/*
 * Test hook: puts a given trace segment in front of the device consumers (csrc/pdmp_consume.hip; tests/test_gpu_consumers_synthetic.py).  Waits for
 * the device (pending asynchronous consumers included), copies the n events into slots [ntrace, ntrace + n) of `chain`'s CURRENT trace buffer and
 * adds n to the chain's ntrace and nevents -- no event-loop kernel runs, no record changes.  PDMP_ERR_INVALID for a bad chain, n < 0,
 * ntrace + n > trace_capacity, a call before pdmp_ensemble_consume_begin (a barrier ensemble: pdmp_ensemble_barrier_consume_begin,
 * tests/test_gpu_barrier_consumers.py) and a non-factorised ensemble.  trace_copy, trace_reset, consume,
 * consume_async, subtrace_copy and the consume_* readers work as after a run.  From the first append on the records no longer match the trace:
 * pdmp_ensemble_run on that ensemble is refused with PDMP_ERR_INVALID (until the next set_state).
 */
pdmp_status pdmp_debug_trace_append(pdmp_ensemble* ens, int64_t chain, const pdmp_event* ev, int64_t n);
/* Its twin for a PDMP_SAMPLER_BPS ensemble (csrc/pdmp_consume_bps.hip; tests/test_gpu_bps_consumers.py): n events -- t [n], x and theta [n x d], and
 * for a sticky ensemble f [n x d] bytes (non-zero = free; NULL otherwise) -- into slots [ntrace, ntrace + n) of the BPS trace buffers, ntrace and
 * nevents bumped by n.  PDMP_ERR_INVALID for a call before pdmp_ensemble_bps_consume_begin, a bad chain, n < 0, ntrace + n > trace_capacity, f given
 * on an ensemble that is not sticky or missing on one that is, and a factorised ensemble.  pdmp_ensemble_run is then refused until the next
 * set_state_bps. */
pdmp_status pdmp_debug_bps_trace_append(pdmp_ensemble* ens, int64_t chain, const double* t, const double* x, const double* theta, const uint8_t* f,
                                        int64_t n);

/*
 * Measurement hook: time (ms per launch, HIP events) of a write-only kernel with the event-record store pattern of the bouncy
 * particle kernel -- one wavefront per chain writing `nrec` records of x[d] and θ[d] -- i.e. the HBM write ceiling that the C2
 * roofline fraction is read against (tools/bench_c2.py).
 */
pdmp_status pdmp_debug_write_probe(int device, int64_t nchains, int64_t d, int64_t nrec, int iters, double* ms_out);

/* Test/measurement hook: time per launch (ms) of a kernel that does nothing but the scattered record traffic of the local ZigZag
 * event loop -- one wavefront per chain, every lane reads the 32-byte first half of 4 pseudo-random 64-byte records of its chain
 * per round, `rounds` times, and with write != 0 stores them back changed.  nchains * d * 64 bytes are allocated for it.  The
 * sector rate it reaches is the practical ceiling quoted beside the event loop's own. */
pdmp_status pdmp_debug_sector_probe(int device, int64_t nchains, int64_t d, int rounds, int write, int iters,
                                             double* ms_out);

#ifdef __cplusplus
}
#endif
#endif /* PDMP_DEBUG_H */
