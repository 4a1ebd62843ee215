// pdmp_spec4_common.hpp -- the machinery of the 4-event speculative loop, written ONCE for its kernels: zz_local_spec_kernel and
// zz_local_spec_wide_kernel (one body, zz_local_spec_body) and zz_sticky_spec_kernel (pdmp_kernels.hip).
//
// The scheme (stated in full above zz_local_spec_body): up to four events of one chain per iteration, one per 16-lane DPP row -- select the
// four smallest block minima, execute every event on the state as it is without storing anything, resolve the draw offsets in time order,
// validate (an event commits iff all earlier ones do, its two-hop zone is disjoint from theirs and nothing they produce or expose comes
// before it) and commit the valid prefix.
//
// The split is the 8-event header's (pdmp_spec8_common.hpp): what is here is the same whatever an event is -- the LDS layout, selection, the
// blob fetch and the draw window, zone conflicts, what an event exposes, validation, the first level's commit.  A kernel keeps its
// prologue's sampler-specific loads, how it types an event, its moves, gradient, accept or chain walk, re-bound, commit stores and counters.
//
// Who uses what: zz_sticky_spec_kernel all of it.  zz_local_spec_body takes the layout, spec_select, the zone conflicts and
// spec_patched_min, as it always did, and keeps the rest WRITTEN OUT -- with the shared pieces its WIDE form spilled more or its lattice
// form ran 0.6 % slower (DESIGN.md §4 has the figures).  A change to spec_blob_fetch, spec_draw_window, spec_expose, spec_validate or
// spec_level1_commit is a change to that body too.
#pragma once

#include "pdmp_device.hpp"
#include "pdmp_engine.hpp"

namespace pdmp {

// LDS layout of the speculative kernel: every fixed-size array sits at a compile-time offset (folds into the DS
// instruction's immediate, no SGPR per array); the three size-dependent arrays come last.
constexpr uint32_t SP_U = 0;        // [64] f64 draws rng_base + lane
constexpr uint32_t SP_LU = 512;     // [64] f64 their logs
constexpr uint32_t SP_SX = 1024;    // [4][16] f64
constexpr uint32_t SP_STH = 1536;   // [4][16] f64
constexpr uint32_t SP_PK = 2048;    // [4][64] f64 patched key blocks
constexpr uint32_t SP_SLT = 4096;   // [4] f64 candidate keys
constexpr uint32_t SP_SLH = 4128;   // [4] f64 second-best entry of the offering lanes
constexpr uint32_t SP_LR = 4160;    // [4] f64 true rates
constexpr uint32_t SP_LBR = 4192;   // [4] f64 bounds
constexpr uint32_t SP_MR = 4224;    // [4] f64 what each event exposes (validation)
constexpr uint32_t SP_Z = 4256;     // [64] u32 zone ids
constexpr uint32_t SP_KR = 4512;    // [4] u32 k per event
constexpr uint32_t SP_SLB = 4528;   // [4] u32 candidate blocks
constexpr uint32_t SP_OFR = 4544;   // [8] u32 draw offsets after 0..4 events
constexpr uint32_t SP_LB = 4576;    // [4][Wpad] u64 blobs, then bk[nblk_pad] f64, bi[nblk_pad] u32

// WIDE (17 <= |S[i]| <= 32: two zone members per lane of a 16-lane row; the second one is always G2-only because |G1| <= 15): the same
// arrays with 32 slots per group where a slot is a zone member
// arrays with 32 slots per group where a slot is a zone member.  The patched key blocks take the place of sx / sth once the re-bound has read
// them (as in the 8-event kernel), so that a chain stays inside 10 KB: 16 chains per CU, all 4096 chains of the ensemble resident at once.
constexpr uint32_t SPW_SX = 1024;    // [4][32] f64
constexpr uint32_t SPW_STH = 2048;   // [4][32] f64
constexpr uint32_t SPW_PK = 1024;    // [4][64] f64 (over sx / sth)
constexpr uint32_t SPW_SLT = 3072, SPW_SLH = 3104, SPW_LR = 3136, SPW_LBR = 3168, SPW_MR = 3200;
constexpr uint32_t SPW_Z = 3232;     // [4][32] u32 zone ids
constexpr uint32_t SPW_KR = 3744, SPW_SLB = 3760, SPW_OFR = 3776;
constexpr uint32_t SPW_LB = 3808;

// Select up to E candidate events: lane l owns the level-1 entries l, l+64, ...; it offers its best entry and remembers its
// second best.  A lane offers only ONE entry per iteration, so the candidates are the E smallest entries only if no lane holds
// two of them -- the lane's second best therefore enters the validation bound of every later event, which keeps the commit rule
// exact.  Winners publish (key, second best, block) straight into the LDS slots.  Returns the number selected.
// FULLQ: the first level has exactly 4 * 64 entries (the launcher's promise for the 128 x 128 lattice): no bounds predicate, and
// (best, second best, argmin) of the lane's four entries come out of a 5-comparator network instead of a compare-select chain.
template <int NE, int E, bool FULLQ = false>
__device__ __forceinline__ int spec_select(const double* bk, uint32_t nblk, int lane, bool stop_before, double T, double* SLT,
                                           double* SLH, uint32_t* SLB, bool& first_inf) {
    double best = PDMP_INF, second = PDMP_INF;
    uint32_t bestb = 0;
    if constexpr (FULLQ && NE == 4) {
        const double k0 = bk[lane], k1 = bk[lane + 64], k2 = bk[lane + 128], k3 = bk[lane + 192];
        const double m01 = min_f64(k0, k1), x01 = max_f64(k0, k1), m23 = min_f64(k2, k3), x23 = max_f64(k2, k3);
        best = min_f64(m01, m23);
        second = min_f64(max_f64(m01, m23), min_f64(x01, x23));
        bestb = (uint32_t)lane + ((k0 == best) ? 0u : (k1 == best) ? 64u : (k2 == best) ? 128u : 192u);  // lowest block on ties
    } else {
#pragma unroll
        for (int q = 0; q < NE; ++q) {
            const uint32_t b = (uint32_t)lane + 64u * q;
            const double v = (b < nblk) ? bk[b] : PDMP_INF;
            const bool lt = v < best;
            second = min_f64(second, lt ? best : v);
            bestb = lt ? b : bestb;
            best = lt ? v : best;
        }
    }
    int Esel = 0;
    first_inf = false;
#pragma unroll
    for (int r = 0; r < E; ++r) {
        if (Esel == r) {
            const double tpr = wave_min_f64(best);
            if (!(tpr < PDMP_INF)) {
                if (r == 0) first_inf = true;
            } else if (!(stop_before && !(tpr < T))) {
                const uint64_t ball = __ballot(best == tpr);
                const int wl = __ffsll((unsigned long long)ball) - 1;
                if (lane == wl) {
                    SLT[r] = best;
                    SLH[r] = second;
                    SLB[r] = bestb;
                    best = PDMP_INF;
                }
                Esel = r + 1;
            }
        }
    }
    return Esel;
}

// Zone conflicts with earlier groups (exact: compare member ids through LDS): does this lane's member id occur in the zone of
// a group q < g?  A cheap necessary condition runs first -- the id must lie inside the [min, max] id span of an earlier group's
// zone (two u32 row reductions, six scalar reads) -- and only if some lane of the wave passes it (about one iteration in three
// on the 128 x 128 lattice) are the 48 id comparisons made.
template <int E>
__device__ __forceinline__ bool spec_zone_conflict(const uint32_t* Z, uint32_t s, int g, bool member) {
    uint32_t lo = member ? s : 0xffffffffu, hi = member ? s : 0u;
    {
        uint32_t o;
        o = dpp_u32<0xB1>(lo);   lo = (o < lo) ? o : lo;
        o = dpp_u32<0x4E>(lo);   lo = (o < lo) ? o : lo;
        o = dpp_u32<0x141>(lo);  lo = (o < lo) ? o : lo;
        o = dpp_u32<0x140>(lo);  lo = (o < lo) ? o : lo;
        o = dpp_u32<0xB1>(hi);   hi = (o > hi) ? o : hi;
        o = dpp_u32<0x4E>(hi);   hi = (o > hi) ? o : hi;
        o = dpp_u32<0x141>(hi);  hi = (o > hi) ? o : hi;
        o = dpp_u32<0x140>(hi);  hi = (o > hi) ? o : hi;
    }
    bool maybe = false;
#pragma unroll
    for (int q = 0; q < E - 1; ++q) {
        const uint32_t lq = readlane_u32(lo, 16 * q), hq = readlane_u32(hi, 16 * q);
        maybe = maybe || ((q < g) && s >= lq && s <= hq);
    }
    maybe = maybe && member;
    if (__ballot(maybe) == 0) return false;
    const uint2* Z2 = reinterpret_cast<const uint2*>(Z);
    bool myconf = false;
#pragma unroll
    for (int q = 0; q < E - 1; ++q) {
        bool hit = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint2 zz = Z2[q * 8 + j];
            hit = hit || (zz.x == s) || (zz.y == s);
        }
        myconf = myconf || (hit && (q < g));
    }
    return myconf && member;
}

// WIDE: two ids per lane (s, s2), 32 per group: Z[q][32]
template <int E>
__device__ __forceinline__ bool spec_zone_conflict_wide(const uint32_t* Z, uint32_t s, uint32_t s2, int g, bool member, bool member2) {
    uint32_t lo = member ? s : 0xffffffffu, hi = member ? s : 0u;
    lo = (member2 && s2 < lo) ? s2 : lo;
    hi = (member2 && s2 > hi) ? s2 : hi;
    {
        uint32_t o;
        o = dpp_u32<0xB1>(lo);   lo = (o < lo) ? o : lo;
        o = dpp_u32<0x4E>(lo);   lo = (o < lo) ? o : lo;
        o = dpp_u32<0x141>(lo);  lo = (o < lo) ? o : lo;
        o = dpp_u32<0x140>(lo);  lo = (o < lo) ? o : lo;
        o = dpp_u32<0xB1>(hi);   hi = (o > hi) ? o : hi;
        o = dpp_u32<0x4E>(hi);   hi = (o > hi) ? o : hi;
        o = dpp_u32<0x141>(hi);  hi = (o > hi) ? o : hi;
        o = dpp_u32<0x140>(hi);  hi = (o > hi) ? o : hi;
    }
    bool maybe = false;
#pragma unroll
    for (int q = 0; q < E - 1; ++q) {
        const uint32_t lq = readlane_u32(lo, 16 * q), hq = readlane_u32(hi, 16 * q);
        maybe = maybe || ((q < g) && ((member && s >= lq && s <= hq) || (member2 && s2 >= lq && s2 <= hq)));
    }
    if (__ballot(maybe) == 0) return false;
    const uint4* Z4 = reinterpret_cast<const uint4*>(Z);
    bool myconf = false;
#pragma unroll
    for (int q = 0; q < E - 1; ++q) {
        bool hit = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint4 zz = Z4[q * 8 + j];
            hit = hit || (member && (zz.x == s || zz.y == s || zz.z == s || zz.w == s)) ||
                  (member2 && (zz.x == s2 || zz.y == s2 || zz.z == s2 || zz.w == s2));
        }
        myconf = myconf || (hit && (q < g));
    }
    return myconf;
}

// Minimum of the group's patched copy of the popped key block (4 keys per lane): row minimum, this lane's candidate.
__device__ __forceinline__ void spec_patched_min(const double* pk, int gl, uint32_t blk, double& rowmin, double& candmin,
                                                 uint32_t& cand) {
    const double2* pk2 = reinterpret_cast<const double2*>(pk + gl * 4);
    const double2 p01 = pk2[0], p23 = pk2[1];
    double lm = p01.x;
    uint32_t li = 0;
    if (p01.y < lm) {
        lm = p01.y;
        li = 1;
    }
    if (p23.x < lm) {
        lm = p23.x;
        li = 2;
    }
    if (p23.y < lm) {
        lm = p23.y;
        li = 3;
    }
    candmin = lm;
    cand = blk * 64u + (uint32_t)gl * 4u + li;
    rowmin = row_min_f64(lm);
}

// ---------------- level-1 loads (functions of i alone), per group: the blob of the group's coordinate into the group's LDS slot lb, 16 bytes
// per lane and step
__device__ __forceinline__ void spec_blob_fetch(const uint64_t* blob, const uint32_t* tix, uint32_t w_pad, uint64_t* lb, bool gvalid, uint32_t i,
                                                int gl) {
    const uint32_t tixi = gvalid ? tix[i] : 0u;
    const ulonglong2* bsrc = reinterpret_cast<const ulonglong2*>(blob + (size_t)tixi * w_pad);
    ulonglong2* bdst = reinterpret_cast<ulonglong2*>(lb);
    if (gvalid) {
        for (uint32_t w = gl; w < (w_pad >> 1); w += 16) bdst[w] = bsrc[w];
    }
}

// ---------------- candidate draws: LDS holds draws rng_base .. rng_base + 63 of the chain's stream (U) and their logs (LU).  An iteration
// consumes at most `need` = E (1 + KMAX) <= 64 of them (about 10 on the lattice), so one wave-wide Philox + log call serves several
// iterations; the window is refilled only when the worst case would run past its end.  Returns the offset of draw dnm inside the window.
__device__ __forceinline__ uint32_t spec_draw_window(uint32_t need, uint32_t dnm, uint64_t seed, uint64_t nm0, int lane, double* U, double* LU,
                                                     uint32_t& rng_base) {
    if (dnm < rng_base || dnm + need > rng_base + 64u) {
        rng_base = dnm;
        const double u = pdmp_u01(seed, PDMP_STREAM_MAIN, nm0 + (uint64_t)dnm + (uint64_t)lane);
        U[lane] = u;
        LU[lane] = pdmp_log(u);
    }
    return dnm - rng_base;
}

// ---------------- what event g exposes (Mr[g]): the patched minimum of its popped block (rowmin, at coordinate cand, held by lane wl2 of the
// group), its new keys (key; +Inf in a lane that has none) and the second-best entry of the lane that offered it (hidg)
__device__ __forceinline__ void spec_expose(const double* pk, int g, int gl, uint32_t blk, bool gvalid, double key, double hidg, double* Mr,
                                            double& rowmin, uint32_t& cand, int& wl2) {
    double candmin;
    spec_patched_min(pk, gl, blk, rowmin, candmin, cand);
    const uint64_t winball = __ballot(gvalid && candmin == rowmin);
    wl2 = __ffs((unsigned)((winball >> (16 * g)) & 0xffffu)) - 1;
    const double keymin = row_min_f64(key);
    const double expose = min_f64(min_f64(rowmin, keymin), hidg);
    if (gl == 0) Mr[g] = expose;
}

// one bit per group out of a ballot of the groups' first lanes
__device__ __forceinline__ uint32_t spec_bits4(uint64_t m_) {
    return (uint32_t)((m_ & 1ull) | ((m_ >> 15) & 2ull) | ((m_ >> 30) & 4ull) | ((m_ >> 45) & 8ull));
}

// ---------------- validate: event g commits iff all earlier ones do, its zone is disjoint from theirs (confball), and nothing they produce or
// expose (Mr) comes before it: okg.  Per-lane evaluation + ballots; the prefix is resolved on the scalar unit.
//   vstop    the event would end the chain with the reference's error(...): it is not committed
//   is_event the event is a trace event (an accepted reflection; the sticky kernel's freeze and thaw)
//   used     trace entries of the launch so far; traced: the chain has a trace at all
// Yields Rc = the committed prefix, evb_c = its trace events (bit r: event r), vsel = the event that stops the chain if it is the chain's
// next one (else -1; status then says so); the chain also stops AFTER a trace event that fills the trace or passes T (`while t′ < T`).
__device__ __forceinline__ void spec_validate(const double* Mr, const double* SLT, uint64_t confball, bool gvalid, bool vstop, bool is_event, double tp,
                                              int g, int gl, bool stop_before, double T, bool traced, uint32_t used, uint32_t trace_room, bool& okg,
                                              uint32_t& Rc, uint32_t& evb_c, int& vsel, uint32_t& status, bool& running) {
    constexpr uint32_t E = 4;
    const double m0 = Mr[0], m1 = Mr[1], m2 = Mr[2];
    const double pref = (g == 0) ? PDMP_INF : (g == 1) ? m0 : (g == 2) ? min_f64(m0, m1) : min_f64(min_f64(m0, m1), m2);
    const bool confg = ((confball >> (16 * g)) & 0xffffull) != 0;
    okg = gvalid && ((g == 0) || (!confg && pref > tp));
    const uint32_t okb = spec_bits4(__ballot(okg && !vstop && gl == 0)), vb = spec_bits4(__ballot(okg && vstop && gl == 0));
    const uint32_t evb = spec_bits4(__ballot(gvalid && is_event && gl == 0));
    const uint32_t gap = ~okb & 0xfu;  // the run of committable slots from slot 0 ends at the first zero bit
    const uint32_t r_ok = gap ? (uint32_t)(__ffs((int)gap) - 1) : E;
    Rc = 0;
    evb_c = 0;
    vsel = -1;
    uint32_t nev_c = 0;
    bool stopped = false;
    // the usual case needs no walk: the slice mode stops on time alone, and the trace has room for every trace event of the run
    const uint32_t ev_run = evb & ((1u << r_ok) - 1u);
    const bool plainrun = stop_before && !(traced && used + (uint32_t)__popc(ev_run) >= trace_room);
    if (plainrun) {
        Rc = r_ok;
        evb_c = ev_run;
    }
    for (uint32_t r = 0; !plainrun && r < r_ok && !stopped; ++r) {
        Rc = r + 1;
        if ((evb >> r) & 1u) {
            evb_c |= 1u << r;
            nev_c += 1;
            if (used + nev_c >= trace_room && traced) {
                status = PDMP_CHAIN_TRACE_FULL;
                stopped = true;
            }
            if (!stop_before && !(uniform_f64(SLT[r]) < T)) {
                running = false;
                stopped = true;
            }
        }
    }
    // the first event that does not commit stops the chain (and nothing stopped it before that event)
    if (!stopped && r_ok < E && ((vb >> r_ok) & 1u)) {
        status = PDMP_CHAIN_BOUND_VIOLATED;
        vsel = (int)r_ok;
    }
}

// ---------------- level-1 updates for new keys living in other blocks than the event's popped one (upd: this lane has one, coordinate s, new
// key).  A block's final entry is the smallest (key, coordinate) among its old entry and the new keys, whatever the order: when no two of
// these lanes aim at one block (claims through the now idle zone-id array Z) and none has to rescan, every lane updates its block by itself
// in one LDS round trip; otherwise one by one in event order, then lane order.
__device__ __forceinline__ void spec_level1_commit(double* bk, uint32_t* bi, uint32_t* Z, const double* keys, bool upd, uint32_t s, double key,
                                                   int lane) {
    uint64_t todo = __ballot(upd);
    if (todo == 0) return;
    PDMP_LDS_ORDER();
    const uint32_t bjv = upd ? (s >> 6) : 0u;
    const double curv = bk[bjv];
    const uint32_t civ = bi[bjv];
    const bool lower = upd && (key < curv || (key == curv && s < civ));
    const bool resc = upd && !lower && civ == s;
    if (lower) Z[bjv & 63u] = (uint32_t)lane;
    PDMP_LDS_ORDER();
    const bool lost = lower && Z[bjv & 63u] != (uint32_t)lane;
    if (__ballot(lost || resc) == 0) {
        if (lower) {
            bk[bjv] = key;
            bi[bjv] = s;
        }
        return;
    }
    while (todo) {
        const int l = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1ull;
        level1_update(bk, bi, keys, lane, readlane_u32(s, l), readlane_f64(key, l));
    }
}

}  // namespace pdmp
