// pdmp_spec8_common.hpp -- the machinery of the 8-event ZigZag loop, written ONCE for its three kernels: zz_local_spec8_kernel and
// zz_local_track_kernel (pdmp_kernels.hip) and zz_local_spec8g_kernel (pdmp_spec8g.inc).
//
// The scheme: zz_local_spec_kernel's (speculate on the next events of one chain, validate exactly, commit the valid prefix) with EIGHT event
// slots per iteration, one per 8-lane group (spec8g<GW = 16>: four, one per 16-lane row).  The instruction stream of an iteration --
// selection, loads, accept chain, validation, commit -- is issued once for eight events instead of four.  The kernels sit at the memory
// system's random-sector rate and at the instruction issue rate of 4 waves per SIMD at the same time, so both the sectors and the
// instructions per event count.  What the scheme consists of:
//   queue     the first level has 512 entries over key blocks of 32: a popped block is four 64-byte sectors, not eight
//   select    one wave minimum m, then every first-level entry <= m + sel_dt is a candidate (compares + population counts);
//             the candidates (<= 16, else sel_dt is halved) are compacted into LDS by ballot prefix counts and rank
//             themselves against each other; ranks 0..7 become the slots.  The slots hold exactly the smallest entries in
//             time order whatever sel_dt is, so there is no hidden second-best to carry into the validation bound
//   accept    every lane evaluates the thinning test of every event for the draw offset equal to its lane number; the ballots
//             are walked on the scalar unit (offset of event r+1 = offset of r + 2 or 1 + k_r), no dependent LDS round trips
//   validate  event g commits iff all earlier ones do, its zone is disjoint from theirs, and nothing they produce or expose comes
//             before it; the patched copies of the popped key blocks give what each event exposes
//   commit    the valid prefix; the first level follows through a claim table (one LDS round trip) or, rarely, one update at a time
// Validation and commit rules are those of the other kernels, so the committed sequence is bit-identical to them and to the oracle.
//
// The split: everything here is the same for the three kernels and takes the LDS sub-array POINTERS each kernel computes at its top (the
// S8_* / G8_* layouts stay with the kernels).  A kernel keeps its prologue, how it evaluates and re-bounds the rate of an event (moved
// neighbourhood + gather, or tracked sums), where its neighbourhood comes from (blob templates in LDS, or per-coordinate line tables)
// and, for spec8g, its zone bitmap and its refresh of the draw window.  Template parameters: E event slots, GW lanes per slot
// (E * GW = 64), KPL = 32 / GW keys of a popped block per lane, REFRESH = the kernel serves the flow's refresh clock.
#pragma once

#include "pdmp_device.hpp"
#include "pdmp_engine.hpp"

namespace pdmp {

constexpr uint32_t S8_NBLK = 512;  // first-level entries: key blocks of 32 (four 64-byte sectors per popped block)
constexpr uint32_t SEL_CAP = 16;   // candidates ranked per iteration (power of two)

// Cycle counts per phase of an iteration (PROF instantiations only; what slot k means is the kernel's own, tests/test_gpu_run_diagnostics.py)
template <bool PROF>
struct PhaseClock {
    uint64_t ph[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t t0 = PROF ? (uint64_t)__builtin_readcyclecounter() : 0;
    uint64_t iters = 0;
    __device__ __forceinline__ void mark(int k) {
        if (PROF) {
            const uint64_t now_ = (uint64_t)__builtin_readcyclecounter();
            ph[k] += now_ - t0;
            t0 = now_;
        }
    }
    __device__ __forceinline__ void store(double* dbg) const {
        for (int q = 0; q < 10; ++q) dbg[q] = (double)ph[q];
        dbg[10] = (double)iters;
    }
};

// ---------------- first level: (min, argmin) of every key block of 32; entries past nblk stay +Inf
// (REFRESH: the refresh clock's slot, key d, sits inside the last block when d is no multiple of 32: it is no coordinate -- its time lives in
// t_ref, and the slot holds +Inf in memory for as long as the launch runs, so that the rescans of its block do not see it either)
template <bool REFRESH>
__device__ __forceinline__ void s8_build_level1(const double* keys, double* bk, uint16_t* bi, uint32_t nblk, int64_t d, bool has_refresh, int lane) {
    const bool hr = REFRESH && has_refresh;
    for (uint32_t b = lane; b < nblk; b += 64) {
        const double* kp = keys + (size_t)b * 32;
        double mk = (hr && b * 32 == (uint32_t)d) ? PDMP_INF : kp[0];
        uint32_t mi = 0;
#pragma unroll 8
        for (int q = 1; q < 32; ++q) {
            const double v = (hr && b * 32 + (uint32_t)q == (uint32_t)d) ? PDMP_INF : kp[q];
            if (v < mk) {
                mk = v;
                mi = q;
            }
        }
        bk[b] = mk;
        bi[b] = (uint16_t)(b * 32 + mi);
    }
    for (uint32_t b = nblk + lane; b < S8_NBLK; b += 64) {
        bk[b] = PDMP_INF;
        bi[b] = 0;
    }
}

// ---------------- select the (up to) E smallest block minima, in time order, WITHOUT a tournament per candidate: one wave minimum m, then
// every first-level entry below the threshold m + sel_dt is a candidate -- compares and population counts tell how many there are.  The
// candidates (at most SEL_CAP, else the threshold is halved) are compacted into LDS by ballot prefix counts, each ranks itself against the
// others with broadcast reads, and ranks 0..E-1 become the event slots (SLT: keys, SLB: blocks).  Whatever sel_dt is, the slots hold exactly
// the smallest entries of the queue, so the committed sequence does not depend on it; it is steered towards ~12 candidates per iteration.
// Esel = 0 with first_inf: no coordinate has a finite key.  do_ref: the refresh clock (t_ref; unused without REFRESH) comes first.
// TB_FENCE: the candidate's block is read before the slots are written over the partial ranks (spec8g's order of the two).
template <int E, bool REFRESH, bool TB_FENCE>
__device__ __forceinline__ void s8_select(const double* bk, double* TK, uint32_t* TB, uint32_t* PR, double* SLT, uint32_t* SLB, double* SELDT,
                                          int lane, bool stop_before, double T, bool has_refresh, double t_ref, int& Esel, bool& first_inf,
                                          bool& do_ref) {
    Esel = 0;
    first_inf = false;
    do_ref = false;
    double kk[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) kk[j] = bk[lane + 64 * j];
    const double mloc = min_f64(min_f64(min_f64(kk[0], kk[1]), min_f64(kk[2], kk[3])), min_f64(min_f64(kk[4], kk[5]), min_f64(kk[6], kk[7])));
    const double mq = wave_min_f64(mloc);
    if constexpr (REFRESH) do_ref = has_refresh && t_ref < mq && !(stop_before && !(t_ref < T));  // (a coordinate's event at the clock's very time goes first)
    if (do_ref) {
    } else if (!(mq < PDMP_INF)) {
        first_inf = true;
    } else if (!(stop_before && !(mq < T))) {
        if (lane < (int)SEL_CAP) TK[lane] = PDMP_INF;
        double dt_sel = uniform_f64(SELDT[0]);
        // (the candidate masks are recomputed where they are needed instead of being kept: eight 64-bit masks would crowd the scalar registers)
        // Compaction: entry (lane, j) gets index (candidates of slots < j) + (candidates of slot j in lower lanes).  There is no separate
        // counting pass: the scratch arrays take up to 64 candidates, and a pass that ends with more than SEL_CAP is repeated with half the
        // threshold.
        auto below = [](uint64_t m_) -> uint32_t {
            return __builtin_amdgcn_mbcnt_hi((uint32_t)(m_ >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m_, 0u));
        };
        double tau;
        uint32_t C;
        for (int tries = 0;; ++tries) {
            tau = mq + dt_sel;  // (>= mq: the minimum itself always qualifies)
            if (stop_before && !(tau < T)) tau = pdmp_below(T);
            if constexpr (REFRESH) {
                if (!(tau < t_ref)) tau = (t_ref > mq) ? pdmp_below(t_ref) : mq;  // nothing at or beyond the refresh clock's time (but the minimum itself)
            }
            const bool pile = tries > 64;  // more than SEL_CAP entries EQUAL to the minimum: one (lowest block) per iteration
            if (tries >= 64) tau = mq;     // a pile of exactly equal keys: the entries equal to the minimum only
            uint32_t base = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool cj_ = kk[j] <= tau;
                uint64_t Mj = __ballot(cj_);
                if (pile) Mj = (base == 0 && Mj) ? (Mj & (~Mj + 1)) : 0ull;
                if (cj_ && ((Mj >> lane) & 1ull)) {
                    const uint32_t ix = base + below(Mj);
                    if (ix < 64u) {
                        TK[ix] = kk[j];
                        TB[ix] = (uint32_t)lane + 64u * j;
                    }
                }
                base += (uint32_t)__popcll(Mj);
            }
            C = base;
            if (C <= SEL_CAP) break;
            dt_sel *= 0.5;
            PDMP_LDS_ORDER();
            if (lane < (int)SEL_CAP) TK[lane] = PDMP_INF;  // (entries past the new count must read +Inf in the ranking)
        }
        PDMP_LDS_ORDER();
        // rank of candidate n among all (ties by index), on a 16 x 4 grid: lane = 16 * part + n counts the candidates
        // 4 * part .. 4 * part + 3 that precede n; the four partial counts meet in LDS.  Unused entries hold +Inf.
        {
            const uint32_t n = (uint32_t)lane & 15u, part = (uint32_t)lane >> 4;
            const double own = TK[n];
            const double2* T2 = reinterpret_cast<const double2*>(TK + 4 * part);
            const double2 o01 = T2[0], o23 = T2[1];
            const uint32_t q = 4 * part;
            uint32_t pr = 0;
            pr += (o01.x < own || (o01.x == own && q + 0 < n)) ? 1u : 0u;
            pr += (o01.y < own || (o01.y == own && q + 1 < n)) ? 1u : 0u;
            pr += (o23.x < own || (o23.x == own && q + 2 < n)) ? 1u : 0u;
            pr += (o23.y < own || (o23.y == own && q + 3 < n)) ? 1u : 0u;
            PR[n * 4 + part] = pr;
            PDMP_LDS_ORDER();
            if ((uint32_t)lane < C) {
                const uint4 p4 = reinterpret_cast<const uint4*>(PR)[lane];
                const uint32_t rank = p4.x + p4.y + p4.z + p4.w;
                if constexpr (TB_FENCE) {
                    const uint32_t tbl = TB[lane];
                    PDMP_LDS_ORDER();
                    if (rank < (uint32_t)E) {
                        SLT[rank] = own;
                        SLB[rank] = tbl;
                    }
                } else if (rank < (uint32_t)E) {
                    SLT[rank] = own;
                    SLB[rank] = TB[lane];
                }
            }
        }
        Esel = (C < (uint32_t)E) ? (int)C : E;
        // steer the threshold: ~10 candidates next time
        const double f = (C > 14u) ? 0.8 : (C < 11u) ? ((C < 6u) ? 2.0 : 1.2) : 1.0;
        if (lane == 0) SELDT[0] = dt_sel * f;
    }
}

// ---------------- one first-level update, by the whole wave: coordinate j (wave-uniform) has the new key kj.  A lower key replaces the entry
// of j's 32-key block; if j WAS the entry and grew, the block is rescanned
__device__ __forceinline__ void s8_level1_update(double* bk, uint16_t* bi, const double* keys, int lane, uint32_t j, double kj) {
    const uint32_t bj = j >> 5;
    PDMP_LDS_ORDER();
    const double cur = bk[bj];
    const uint32_t ci = bi[bj];
    if (kj < cur || (kj == cur && j < ci)) {
        if (lane == 0) {
            bk[bj] = kj;
            bi[bj] = (uint16_t)j;
        }
    } else if (ci == j) {
        const double kv = __hip_atomic_load(keys + (size_t)bj * 32 + (lane & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double mn = wave_min_f64(kv);
        const uint64_t bl = __ballot(kv == mn);
        const int arg = bl ? (__ffsll((unsigned long long)bl) - 1) : 0;
        if (lane == 0) {
            bk[bj] = mn;
            bi[bj] = (uint16_t)(bj * 32 + (uint32_t)arg);
        }
    }
}
// ... as the level-1 form zz_refresh_event (pdmp_zz_refresh.hpp) takes its new keys through: the clock is no key here, its time is the
// kernel's t_ref
struct S8Level1 {
    static constexpr bool clock_is_key = false;
    double* bk;
    uint16_t* bi;
    __device__ __forceinline__ void operator()(const double* keys, int lane, uint32_t j, double kj) const {
        s8_level1_update(bk, bi, keys, lane, j, kj);
        PDMP_LDS_ORDER();
    }
};

// ---------------- candidate draws: a window of 64 draws (one per lane, in ureg) and their logs (LU), refilled when an iteration's `need`
// draws could leave it.  Returns the offset of draw dnm inside the window.
__device__ __forceinline__ uint32_t s8_draw_window(uint32_t need, uint32_t dnm, uint64_t seed, uint64_t nm0, int lane, double* LU, uint32_t& rng_base,
                                                   double& ureg) {
    if (dnm < rng_base || dnm + need > rng_base + 64u) {
        rng_base = dnm;
        ureg = pdmp_u01(seed, PDMP_STREAM_MAIN, nm0 + (uint64_t)dnm + (uint64_t)lane);
        LU[lane] = pdmp_log(ureg);
    }
    return dnm - rng_base;
}

// ---------------- blob slots of the lattice kernels: 0 holds the common template for the whole launch, 1 and 2 take the first two events of
// an iteration that need another one (tixi != common); the third such event and everything after it wait for the next iteration
template <uint32_t WPAD>
__device__ __forceinline__ uint32_t s8_blob_slot(const uint64_t* blob, uint64_t* LB, uint32_t tixi, uint32_t common, int g, int gl, int& Esel,
                                                 bool& gvalid) {
    uint32_t slot = 0;
    const bool nc = gvalid && tixi != common;
    const uint64_t ncball = __ballot(nc && gl == 0);
    if (ncball != 0) {
        const uint32_t rank = (uint32_t)__popcll(ncball & ((1ull << (8 * g)) - 1ull));
        if (__popcll(ncball) > 2) {
            uint64_t m_ = ncball;
            m_ &= m_ - 1;
            m_ &= m_ - 1;
            const int cut = (__ffsll((unsigned long long)m_) - 1) >> 3;
            Esel = cut;
            gvalid = g < Esel;
        }
        if (nc && gvalid) {
            slot = 1 + rank;
            const ulonglong2* bsrc = reinterpret_cast<const ulonglong2*>(blob + (size_t)tixi * WPAD);
            ulonglong2* bdst = reinterpret_cast<ulonglong2*>(LB + slot * WPAD);
            for (uint32_t w = gl; w < WPAD / 2; w += 8) bdst[w] = bsrc[w];
        }
    }
    return slot;
}

// ---------------- zone conflicts with earlier groups by id spans (lattice kernels; Z = [8][16] zone ids, a lane's own are sA and sB): the
// exact id comparison is made only for pairs of groups whose spans overlap.  Returns one bit per group that meets an earlier one.
__device__ __forceinline__ uint32_t s8_zone_conflicts(const uint32_t* Z, bool memberA, uint32_t sA, bool memberB, uint32_t sB, bool gvalid, int lane,
                                                      int g, int gl) {
    uint32_t lo = memberA ? sA : 0xffffffffu, hi = memberA ? sA : 0u;
    lo = (memberB && sB < lo) ? sB : lo;
    hi = (memberB && sB > hi) ? sB : hi;
    uint32_t o;
    o = dpp_u32<0xB1>(lo);   lo = (o < lo) ? o : lo;
    o = dpp_u32<0x4E>(lo);   lo = (o < lo) ? o : lo;
    o = dpp_u32<0x141>(lo);  lo = (o < lo) ? o : lo;
    o = dpp_u32<0xB1>(hi);   hi = (o > hi) ? o : hi;
    o = dpp_u32<0x4E>(hi);   hi = (o > hi) ? o : hi;
    o = dpp_u32<0x141>(hi);  hi = (o > hi) ? o : hi;
    // A pair of groups (q < g) whose spans overlap is compared exactly by the WHOLE wave: lane L holds id L & 15 of g
    // against ids 4 (L >> 4) .. + 3 of q -- the 256 id pairs in four xor / two min instructions per lane.  Empty
    // positions hold sentinels that equal nothing.
    uint32_t confmask = 0;
    const uint4* Z4 = reinterpret_cast<const uint4*>(Z);
    // lane gl of group g looks at the pair (g, q = gl): one ballot finds all pairs of groups whose spans overlap
    const uint32_t lq = (uint32_t)__builtin_amdgcn_ds_bpermute(32 * gl, (int)lo);  // span of group gl (its lane 0)
    const uint32_t hq = (uint32_t)__builtin_amdgcn_ds_bpermute(32 * gl, (int)hi);
    uint64_t ovb = __ballot(gvalid && gl < g && lo <= hq && lq <= hi);
    while (ovb != 0) {
        const int bit = __ffsll((unsigned long long)ovb) - 1;
        const int gsel = bit >> 3, q = bit & 7;
        ovb &= ovb - 1;
        const uint32_t idg = Z[gsel * 16 + (lane & 15)];
        const uint4 zq = Z4[q * 4 + (lane >> 4)];
        const uint32_t mn = umin3(idg ^ zq.x, idg ^ zq.y, umin3(idg ^ zq.z, idg ^ zq.w, 0xffffffffu));
        if (__ballot(mn == 0u) != 0) confmask |= 1u << gsel;
    }
    return confmask;
}

// ---------------- accept chain in time order.  Lane o holds the draw at offset o of the iteration (coin) and evaluates every event's test
// for it (:121); the ballots are then walked on the scalar unit: event r reads its bit at the offset the earlier outcomes imply (k = |G1| of
// the lane's event).  The offsets travel packed six bits apiece in one 64-bit scalar: offset after r events = bits 6r .. 6r+5 of offpack.
// Slots >= Esel hold stale rates: their bits are masked off, their offsets unused.  FIT: an event whose draws would leave the window -- or
// its end offset the six bits it travels in -- ends the candidate list (Esel is lowered).
template <int E, int GW, bool FIT>
__device__ __forceinline__ void s8_accept_walk(double coin, const double* LBr, const double* Lr, int k, int& Esel, uint32_t& accbits,
                                               uint64_t& offpack) {
    accbits = 0;
    offpack = 0;
    uint32_t off = 0;
    int fit = Esel;
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const uint64_t am_r = __ballot(coin * LBr[r] < Lr[r]);
        const uint32_t k_r = readlane_u32((uint32_t)k, GW * r);
        if constexpr (FIT) {
            if (r < fit && off + 1u + k_r > 63u) fit = r;
        }
        const uint32_t a_r = (uint32_t)(am_r >> (off & 63u)) & 1u;
        off += a_r ? (1u + k_r) : 2u;
        off = (off < 63u) ? off : 63u;  // (only stale slots can run past the window; keeps the shifts defined)
        accbits |= a_r << r;
        offpack |= (uint64_t)off << (6 * (r + 1));
    }
    if constexpr (FIT) {
        if (fit < Esel) Esel = fit;
    }
    accbits &= (1u << Esel) - 1u;
}

// ---------------- the patched copy of the popped key block (kq: the lane's KPL keys of it) goes into pk, the group's [32] f64 of the shared
// scratch area: all readers of what was there are done.  With KPL = 4 the two 16-byte pieces of a lane's chunk are stored in the order
// piece ^ pk_t (odd groups swapped): b128 accesses without bank conflicts.  A lane that re-bounded a coordinate of the block (patch)
// stores its new key over the old one.
template <int KPL>
__device__ __forceinline__ void s8_patch_block(double* pk, uint32_t pk_t, int gl, const double (&kq)[4], bool patch, uint32_t sA, double key) {
    if constexpr (KPL == 4) {
        double2* pk2 = reinterpret_cast<double2*>(pk + gl * 4);
        pk2[0 ^ pk_t] = make_double2(kq[0], kq[1]);
        pk2[1 ^ pk_t] = make_double2(kq[2], kq[3]);
    } else {
        reinterpret_cast<double2*>(pk + gl * 2)[0] = make_double2(kq[0], kq[1]);
    }
    PDMP_LDS_ORDER();
    if (patch) {
        const uint32_t e_ = sA & 31u;
        if constexpr (KPL == 4) pk[(e_ & ~3u) + ((((e_ & 3u) >> 1) ^ pk_t) << 1) + (e_ & 1u)] = key;
        else pk[e_] = key;
    }
    PDMP_LDS_ORDER();
}

__device__ __forceinline__ void s8_take_lower(double v, uint32_t idx, double& lm, uint32_t& li) {
    if (v < lm) {
        lm = v;
        li = idx;
    }
}

// ---------------- patched minimum of the popped block (rowmin, at coordinate cand, held by lane wl2 of the group), and everything this
// event could expose: that minimum or one of the new keys.  Mr[g] takes it.
template <int GW>
__device__ __forceinline__ void s8_patched_min(const double* pk, uint32_t pk_t, uint32_t blk, bool gvalid, double key, int g, int gl, double* Mr,
                                               double& rowmin, uint32_t& cand, int& wl2) {
    constexpr int KPL = 32 / GW;
    constexpr uint64_t GM = (GW == 8) ? 0xffull : 0xffffull;
    double lm;
    uint32_t li = 0;
    if constexpr (KPL == 4) {
        const double2* pk2 = reinterpret_cast<const double2*>(pk + gl * 4);
        const double2 p01 = pk2[0 ^ pk_t], p23 = pk2[1 ^ pk_t];
        lm = p01.x;
        s8_take_lower(p01.y, 1, lm, li);
        s8_take_lower(p23.x, 2, lm, li);
        s8_take_lower(p23.y, 3, lm, li);
    } else {
        const double2 p01 = reinterpret_cast<const double2*>(pk + gl * 2)[0];
        lm = p01.x;
        s8_take_lower(p01.y, 1, lm, li);
    }
    cand = blk * 32u + (uint32_t)gl * (uint32_t)KPL + li;
    rowmin = (GW == 8) ? grp8_min_f64(lm) : row_min_f64(lm);
    const uint64_t winball = __ballot(gvalid && lm == rowmin);
    wl2 = __ffs((unsigned)((winball >> (GW * g)) & GM)) - 1;
    const double keymin = (GW == 8) ? grp8_min_f64(key) : row_min_f64(key);
    const double expose = min_f64(rowmin, keymin);
    if (gl == 0) Mr[g] = expose;
    PDMP_LDS_ORDER();
}

// ---------------- validate: event g commits iff all earlier ones do, its zone is disjoint from theirs (confball: one bit per group), and
// nothing they produce or expose (Mr) comes before it.  Rc = the committable prefix, nacc_c = the accepted events in it, vsel = the event
// that violates its bound if it is the chain's next one (else -1).  `used` = trace entries of the launch so far.
template <int E, int GW>
__device__ __forceinline__ void s8_validate(const double* Mr, const double* SLT, uint64_t confball, bool gvalid, bool accept, bool violated, bool adapt,
                                            double tp, int g, int gl, bool stop_before, double T, bool traced, uint32_t used, uint32_t trace_room,
                                            uint32_t& Rc, uint32_t& nacc_c, int& vsel, uint32_t& status, bool& running) {
    constexpr int LG = (GW == 8) ? 3 : 4;
    constexpr uint64_t G0 = (GW == 8) ? 0x0101010101010101ull : 0x0001000100010001ull;  // lane 0 of every group
    vsel = -1;
    double pref = PDMP_INF;
#pragma unroll
    for (int q = 0; q < E - 1; ++q) {
        const double mq = Mr[q];
        pref = (q < g) ? min_f64(pref, mq) : pref;
    }
    const bool confg = ((confball >> g) & 1ull) != 0;
    const bool okg = gvalid && ((g == 0) || (!confg && pref > tp));
    const bool vstop = violated && !adapt;  // reference: error(...), :124 -> the event is not committed
    const uint64_t okball = __ballot(okg && !vstop && gl == 0);
    const uint64_t vball = __ballot(okg && vstop && gl == 0);
    const uint64_t accball = __ballot(accept && gl == 0);
    // length of the run of committable slots from slot 0 (one bit per slot at bit GW r): first zero among those bits
    const uint64_t gap = ~okball & G0;
    const uint32_t r_ok = gap ? (uint32_t)((__ffsll((unsigned long long)gap) - 1) >> LG) : (uint32_t)E;
    Rc = 0;
    nacc_c = 0;
    bool stopped = false;
    // the usual case needs no walk: the slice mode stops on time alone, and the trace has room for every accepted slot
    const uint32_t nacc_all = (uint32_t)__popcll(accball & ((r_ok < (uint32_t)E) ? ((1ull << (GW * r_ok)) - 1ull) : ~0ull));
    const bool plainrun = stop_before && !(traced && used + nacc_all >= trace_room);
    if (plainrun) {
        Rc = r_ok;
        nacc_c = nacc_all;
    }
    for (uint32_t r = 0; !plainrun && r < r_ok && !stopped; ++r) {
        Rc = r + 1;
        if ((accball >> (GW * r)) & 1ull) {
            nacc_c += 1;
            if (used + nacc_c >= trace_room && traced) {
                status = PDMP_CHAIN_TRACE_FULL;
                stopped = true;
            }
            if (!stop_before && !(uniform_f64(SLT[r]) < T)) {
                running = false;
                stopped = true;
            }
        }
    }
    if (!stopped && r_ok < (uint32_t)E && ((vball >> (GW * r_ok)) & 1ull)) {
        status = PDMP_CHAIN_BOUND_VIOLATED;
        vsel = (int)r_ok;
    }
}

// ---------------- level-1 updates for re-bounded neighbours living in other blocks (upd: this lane has one, coordinate sA, new key).  The
// final entry of a block is the smallest (key, coordinate) among its old entry and the new keys, whatever the order -- so when no two of
// these lanes aim at one block (checked through the small claim table CL) and none has to rescan, every lane updates its block by itself,
// in one LDS round trip for all of them; otherwise the updates are made one by one in event order.
template <int GW>
__device__ __forceinline__ void s8_level1_commit(double* bk, uint16_t* bi, uint8_t* CL, const double* keys, const uint32_t* SLB, bool upd, uint32_t sA,
                                                 double key, int k, uint32_t Rc, uint64_t accball2, int lane) {
    if (__ballot(upd) == 0) return;
    PDMP_LDS_ORDER();
    const uint32_t bjv = upd ? (sA >> 5) : 0u;
    const double curv = bk[bjv];
    const uint32_t civ = bi[bjv];
    const bool lower = upd && (key < curv || (key == curv && sA < civ));
    const bool resc = upd && !lower && civ == sA;
    if (lower) CL[bjv & 63u] = (uint8_t)lane;
    PDMP_LDS_ORDER();
    const bool lost = lower && CL[bjv & 63u] != (uint8_t)lane;
    if (__ballot(lost || resc) == 0) {
        if (lower) {
            bk[bjv] = key;
            bi[bjv] = (uint16_t)sA;
        }
        return;
    }
    for (uint32_t r = 0; r < Rc; ++r) {
        if (!((accball2 >> (GW * r)) & 1ull)) continue;
        const uint32_t own = uniform_u32(SLB[r]);
        const int kr = (int)readlane_u32((uint32_t)k, GW * (int)r);
        for (int jj = 0; jj < kr; ++jj) {
            const uint32_t j = readlane_u32(sA, GW * (int)r + jj);
            if ((j >> 5) == own) continue;
            s8_level1_update(bk, bi, keys, lane, j, readlane_f64(key, GW * (int)r + jj));
        }
    }
}

// ---------------- counters of an iteration.  The violating proposal itself (vsel >= 0) is counted and its draws consumed, acc is bumped
// (vnacc) -- then the reference stops with error(...), :120-124: what zz_local_run_kernel and the oracle leave behind.
template <int GW>
__device__ __forceinline__ void s8_count(int vsel, uint32_t Rc, uint32_t nacc_c, uint64_t offpack, uint64_t accball2, const double* SLT, uint32_t& dnum,
                                         uint32_t& dnacc, uint32_t& dnm, uint32_t& vnacc, double& t_last, double& t_event) {
    constexpr int LG = (GW == 8) ? 3 : 4;
    if (vsel >= 0) {
        dnum += 1;
        vnacc = 1;
        dnm += ((uint32_t)(offpack >> (6 * vsel)) & 63u) + 1u - ((uint32_t)(offpack >> (6 * Rc)) & 63u);
    }
    if (Rc > 0) {
        dnum += Rc;
        dnacc += nacc_c;
        dnm += (uint32_t)(offpack >> (6 * Rc)) & 63u;
        t_last = uniform_f64(SLT[Rc - 1]);
        if (accball2) t_event = uniform_f64(SLT[(63 - __builtin_clzll(accball2)) >> LG]);
    }
    if (vsel >= 0) t_last = uniform_f64(SLT[vsel]);  // the violating event's time is the chain's current time
}

// ---------------- the chain's header when the launch ends (lane 0).  REFRESH: the clock's time goes back into its queue slot, key d.
template <bool REFRESH>
__device__ __forceinline__ void s8_store_header(DevChain* hdr, double* keys, int64_t d, double t_last, double t_event, uint32_t dnum, uint32_t dnacc,
                                                uint32_t vnacc, uint64_t ntrace0, uint64_t nm0, uint32_t dnm, uint32_t status, bool has_refresh,
                                                double t_ref, uint32_t dnref, uint64_t ng) {
    hdr->c.t_last = t_last;
    hdr->t_event = t_event;
    hdr->c.num += dnum;
    hdr->c.nacc += dnacc + vnacc;
    hdr->c.ntrace = ntrace0 + dnacc + dnref;
    hdr->c.nevents += dnacc + dnref;
    if constexpr (REFRESH) {
        hdr->c.nrefresh += dnref;
        hdr->c.ndraw_global = ng;
        if (has_refresh) keys[d] = t_ref;
    }
    hdr->c.ndraw_main = nm0 + dnm;
    hdr->c.status = status;
}

}  // namespace pdmp
