// pdmp_spec8g.inc -- zz_local_spec8g_kernel: the 8-event scheme (pdmp_spec8_common.hpp; included by pdmp_kernels.hip after zz_local_spec8_kernel) for ANY sparse Γ
// with |G1[i]| <= 8 and |S[i]| <= 32 (GW = 8: eight events per iteration) or <= 64 (GW = 16: four) -- `spdmp` builds G1 / G2 from whatever CSC pattern it is given (src/sfact.jl:170-179).  What the lattice
// kernel takes from a blob template in LDS (one template serves 94 % of a lattice's coordinates; on a graph without that regularity every
// coordinate has its own, and eight of them do not fit beside the queue) each lane here reads straight from two per-coordinate tables of ONE 128-byte
// line per coordinate (the tables compete with the chains' records for the L2: what counts is how many lines an event touches -- 9 here, 25 when the
// same data sat in seven arrays, which cost a quarter of the kernel's memory traffic):
//   line [d] x 128 B     bytes 0-63: S[i] = G1[i] ++ G2[i] transposed, 4 x u16 per lane -- lane gl owns zone positions gl, gl + 8, gl + 16, gl + 24
//                        (0x7FFF past |S[i]|; bit 15 of the first id: the position belongs to G1[i]); positions >= 8 are G2-only (|G1| <= 8), touched by
//                        accepted events only.  bytes 64-127: for member j = G1[i][gl] the positions inside S[i] of the members of G1[j], one byte each
//   member [d] x 128 B   bytes 0-63: Γ[G1[j], j] (bounding), 0.0 past |G1[j]|; then c_j, Γ[:,j]·μ: requested together with j's record.  When the
//                        target's Γ equals the bounding one (SAME) the gradient's coefficient Γt[G1[i][gl], i] is word gl of member[i];
//   gamt [d][8] f64      ... otherwise it comes from this table.  The gradient's terms are formed by the lanes that hold the members and summed in
//                        idot's order (src/common.jl:16-24) from lane to lane
// Zones of two events are compared through a bitmap of the d coordinates in LDS (set by the groups in event order, tested by the next one: the
// DS queue of a wave is in order, so the eight set / test pairs are issued back to back), which costs the same whatever the graph looks like --
// the lattice kernel's id spans separate nothing on a graph without locality.  2048 <= d <= 16384; a refresh clock is served since round 6 (its events by themselves) (everything else keeps
// zz_local_spec_kernel, 4 events per iteration); FULL adds `adapt` (per-chain bounds c, multiplied by `factor` when a proposal violates its bound,
// src/fact_samplers.jl:67-70) and a target with a mean.  The committed sequence is bit-identical
// to the other kernels and the oracle (tests/test_gpu_spec_wide.py).
constexpr uint32_t G8_LU = 0;                      // [64] f64 logs of the draw window
constexpr uint32_t G8_R = 512;                     // 4224 bytes in turn: selection scratch, zone bitmap, sx / sth, patched key blocks
constexpr uint32_t G8_SX = G8_R;                   // [E][4 GW + 1] f64: 8 groups of 8 lanes (|S| <= 32) or 4 groups of 16 lanes (|S| <= 64)
constexpr uint32_t G8_STH = G8_R + 2112;           // the same for θ
constexpr uint32_t G8_BM = G8_R;                   // [512 + 1] u32: one bit per coordinate; word 512 takes the absent zone positions
constexpr uint32_t G8_PK = G8_R;                   // [8][32] f64
constexpr uint32_t G8_TK = G8_R;                   // [64] f64
constexpr uint32_t G8_TB = G8_R + 64 * 8;          // [64] u32
constexpr uint32_t G8_SLT = G8_R + 4224;           // [8] f64 candidate keys
constexpr uint32_t G8_LR = G8_SLT + 64;            // [8] f64 true rates
constexpr uint32_t G8_LBR = G8_LR + 64;            // [8] f64 bounds
constexpr uint32_t G8_MR = G8_LBR + 64;            // [8] f64 what each event exposes
constexpr uint32_t G8_SLB = G8_MR + 64;            // [8] u32 candidate blocks
constexpr uint32_t G8_BK = G8_SLB + 32;            // [512] f64 block minima (key blocks of 32)
constexpr uint32_t G8_BI = G8_BK + S8_NBLK * 8;    // [512] u16 their coordinates
constexpr uint32_t G8_SELDT = G8_BI + S8_NBLK * 2;
constexpr uint32_t G8_CL = G8_SELDT + 8;           // [64] u8 claims of the parallel first-level update
constexpr uint32_t G8_BYTES = G8_CL + 64;          // 10216
constexpr uint32_t G8_PR = G8_SLT;                 // [16][4] u32 partial ranks (over SLT .. MR, written after the ranking)
static_assert(G8_BYTES <= 10240, "16 chains per CU: 160 KB / 16");
static_assert(8 * 33 * 8 <= 2112 && 4 * 65 * 8 <= 2112 && 513 * 4 <= 4224 && 8 * 32 * 8 <= 4224 && (G8_BK % 16) == 0 && (G8_STH % 8) == 0, "scratch area");
size_t zz_spec8g_lds_bytes() { return G8_BYTES; }

// GW = lanes per event group: 8 (eight events per iteration, |S| <= 32) or 16 (four events per iteration, |S| <= 64: a lane still owns four zone
// positions, gl, gl + GW, gl + 2 GW, gl + 3 GW; |G1| <= 8 either way, so G1 sits in the first 8 lanes of a group)
template <bool PROF, bool SAME, bool FULL = false, int GW = 8>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void zz_local_spec8g_kernel(ZzRunParams P) {
    static_assert(GW == 8 || GW == 16, "8 or 16 lanes per event");
    constexpr int E = 64 / GW;
    constexpr int LG = (GW == 8) ? 3 : 4;
    constexpr uint64_t GM = (GW == 8) ? 0xffull : 0xffffull;                                // the lanes of one group in a ballot
    constexpr uint32_t G8_SXP = 4 * GW + 1;
    constexpr uint32_t LSTR = (GW == 8) ? 16u : 24u;  // u64 words per coordinate in the line table: GW id words + 8 position words
    constexpr int KPL = 32 / GW;                      // keys of the popped block per lane
    constexpr uint32_t KMAX = 8;
    const uint32_t nblk = P.nblk;  // 32-key blocks that hold coordinates (<= S8_NBLK)
    const int lane0 = threadIdx.x;
    const int64_t chain = blockIdx.x;
    const int64_t d = P.d;

    extern __shared__ __align__(16) unsigned char smem[];
    double* const LU = reinterpret_cast<double*>(smem + G8_LU);
    double* const SLT = reinterpret_cast<double*>(smem + G8_SLT);
    double* const Lr = reinterpret_cast<double*>(smem + G8_LR);
    double* const LBr = reinterpret_cast<double*>(smem + G8_LBR);
    double* const Mr = reinterpret_cast<double*>(smem + G8_MR);
    uint32_t* const SLB = reinterpret_cast<uint32_t*>(smem + G8_SLB);
    uint32_t* const BM = reinterpret_cast<uint32_t*>(smem + G8_BM);
    double* const bk = reinterpret_cast<double*>(smem + G8_BK);
    uint16_t* const bi = reinterpret_cast<uint16_t*>(smem + G8_BI);
    double* const TK = reinterpret_cast<double*>(smem + G8_TK);
    uint32_t* const TB = reinterpret_cast<uint32_t*>(smem + G8_TB);
    double* const SELDT = reinterpret_cast<double*>(smem + G8_SELDT);
    uint32_t* const PR = reinterpret_cast<uint32_t*>(smem + G8_PR);

    ZzRec* rec = P.rec + chain * d;
    double* keys = P.keys + chain * P.dk;
    DevChain* hdr = P.hdr + chain;
    pdmp_event* ev = P.ev ? P.ev + chain * P.trace_cap : nullptr;
    double* const cmut = (FULL && P.c_chain) ? (P.c_chain + chain * d) : nullptr;
    const bool adapt = FULL && P.adapt != 0;
    const uint64_t* const lineI = P.g8_line;                                          // [d][16] u64
    const double2* const member2 = reinterpret_cast<const double2*>(P.g8_member);     // [d][8] double2

    uint32_t status = hdr->c.status;
    if (chain_ended(status)) return;
    const uint64_t seed = hdr->seed;
    const uint64_t nm0 = hdr->c.ndraw_main, ntrace0 = hdr->c.ntrace;
    uint32_t dnm = 0, dnum = 0, dnacc = 0;
    uint32_t vnacc = 0;  // 1 if the launch ends on a bound violation (acc is bumped before the check)
    // the flow's refresh clock (src/sfact.jl:78-114; round 6, as in zz_local_spec8_kernel): its time is a wave-uniform scalar, its events are processed by
    // themselves between the speculative iterations -- from the neighbourhood blobs zz_local_run_kernel uses (the host builds them for every graph)
    const bool has_refresh = P.has_refresh != 0;
    double t_ref = has_refresh ? keys[d] : PDMP_INF;
    uint32_t dnref = 0;
    uint64_t ng = hdr->c.ndraw_global;
    double t_last = hdr->c.t_last;
    double t_event = hdr->t_event;
    status = PDMP_CHAIN_OK;

    const double T = P.T;
    const bool stop_before = (P.flags & PDMP_RUN_STOP_BEFORE) != 0;
    const uint32_t trace_room = launch_trace_room(P.trace_cap, ntrace0);

    if (lane0 == 0) SELDT[0] = 1e-3;
    s8_build_level1<true>(keys, bk, bi, nblk, d, has_refresh, lane0);
    PDMP_LDS_ORDER();
    if (has_refresh && lane0 == 0) __hip_atomic_store(keys + d, PDMP_INF, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    uint32_t rng_base = 0xffffffffu;
    double ureg = 0.0;  // draw rng_base + lane of the chain's stream
    PhaseClock<PROF> phc;

    bool running = stop_before || (t_event < T);
    PrioTurn prio;
    while (running) {
        // (the lane index is made opaque once per iteration: LLVM otherwise hoists lane-only arithmetic -- masks, LDS addresses -- out of this
        // loop, runs out of registers and SPILLS it; the reload inside the loop waits with vmcnt(0) for every store in flight)
        int lane = lane0;
        asm volatile("" : "+v"(lane));
        const int g = lane >> LG;        // group = event slot
        const int gl = lane & (GW - 1);  // lane inside the group
        double* const sx = reinterpret_cast<double*>(smem + G8_SX) + g * G8_SXP;
        double* const sth = reinterpret_cast<double*>(smem + G8_STH) + g * G8_SXP;
        double* const pk = reinterpret_cast<double*>(smem + G8_PK) + g * 32;
        const uint32_t pk_t = (GW == 8) ? ((uint32_t)g & 1u) : 0u;  // odd groups store the two 16-byte pieces of a lane's chunk swapped: no bank conflicts
        prio.step();
        if (dnacc + dnref >= trace_room) {
            status = PDMP_CHAIN_TRACE_FULL;
            break;
        }
        if (dnm >= P.count_limit) {  // (32-bit counters of the launch: pause, the host runs again)
            status = PDMP_CHAIN_PAUSED;
            break;
        }
        // ---------------- select the (up to) E smallest block minima in time order
        int Esel;
        bool first_inf, do_ref;
        s8_select<E, true, true>(bk, TK, TB, PR, SLT, SLB, SELDT, lane, stop_before, T, has_refresh, t_ref, Esel, first_inf, do_ref);
        if (do_ref) {
            // ---------------- the refresh clock is the chain's next event: src/sfact.jl:78-114 (zz_refresh_event), from the neighbourhood blobs
            // zz_local_run_kernel uses (the host builds them for every graph).  Scratch inside the shared area: the blob (<= 137 words: |S| <= 64,
            // |G1| <= 8), then sx and sth as [64]
            const double tp = t_ref;
#ifdef PDMP_G8_DEBUG
            if (chain == 0 && lane == 0) printf("g8 refresh: it %u tp %.17g dnum %u dnref %u blob_w %u sw %u pw %u kmax %u\n", (unsigned)prio.it, tp, dnum, dnref, P.blob_w, P.blob_sw, P.blob_pw, P.blob_kmax);
#endif
            t_last = tp;
            const ZzRefreshed rf = zz_refresh_event<false, 0>(P, BlobGeom{P.blob_w, P.blob_w_pad, P.blob_sw, P.blob_pw, 4 + P.blob_pw + P.blob_kmax}, rec, keys,
                                                           cmut, d, seed, nm0 + (uint64_t)dnm, ng, tp, lane, reinterpret_cast<uint64_t*>(smem + G8_R),
                                                           reinterpret_cast<double*>(smem + G8_R + 1152),
                                                           reinterpret_cast<double*>(smem + G8_R + 1152 + 512), false, S8Level1{bk, bi});
            dnm += rf.ndraw;
            ng = rf.ng;
            t_ref = rf.t_ref;  // (stored into keys[d] when the launch ends)
            if (ev && lane == 0) {  // event(i, t, x, θ, F) = (t[i], i, x[i], θ[i]), :143
                pdmp_event e;
                e.t = rf.t;
                e.i = (int64_t)rf.i2;
                e.x = rf.x;
                e.theta = rf.th;
                ev[ntrace0 + dnacc + dnref] = e;
            }
            dnref += 1;
            t_event = tp;
            if (!stop_before && !(tp < T)) running = false;
            PDMP_LDS_ORDER();
            continue;
        }
        if (Esel == 0) {
            if (first_inf && !(t_ref < PDMP_INF)) status = PDMP_CHAIN_STALLED;
            break;
        }
#ifdef PDMP_G8_DEBUG
        if (chain == 0 && lane == 0 && (prio.it % 64u) == 0u) printf("g8 iter %u Esel %d t_ref %.17g t_last %.17g dnum %u\n", (unsigned)prio.it, Esel, t_ref, t_last, dnum);
#endif
        PDMP_LDS_ORDER();
        phc.mark(0);
        if (PROF) phc.iters += 1;
        bool gvalid = g < Esel;
        const double tp = gvalid ? SLT[g] : PDMP_INF;
        const uint32_t blk = gvalid ? SLB[g] : 0u;
        const uint32_t i = gvalid ? (uint32_t)bi[blk] : 0u;

        // ---------------- level-1 loads: functions of i alone, each lane its own words (L2-resident tables)
        const uint64_t idw64 = lineI[(size_t)i * LSTR + (size_t)gl];
        const uint64_t posw = lineI[(size_t)i * LSTR + GW + (size_t)(gl & 7)];
        double gv = SAME ? reinterpret_cast<const double*>(P.g8_member)[(size_t)i * 16 + (size_t)(gl & 7)] : P.g8_gamt[(size_t)i * 8 + (size_t)(gl & 7)];
        if (GW == 16 && gl >= 8) gv = 0.0;  // (G1 sits in the first 8 lanes)
        const ZzRec* ri = rec + i;
        const double told_i = ri->t_old, a_i = ri->a, b_i = ri->b;
        const uint64_t acc_i = ri->acc;
        double kq[4] = {0.0, 0.0, 0.0, 0.0};
        {
            const double2* kp = reinterpret_cast<const double2*>(keys + (size_t)blk * 32 + gl * KPL);
            const double2 k01 = kp[0];
            kq[0] = k01.x;
            kq[1] = k01.y;
            if (KPL == 4) {
                const double2 k23 = kp[1];
                kq[2] = k23.x;
                kq[3] = k23.y;
            }
        }
        // ---------------- the window of draws: refreshed at every iteration (an iteration uses ~20 of its 64; up to 8 (1 + KMAX) = 72 could be
        // asked for -- an event whose draws would leave the window ends the candidate list, below)
        if (dnm != rng_base) {
            rng_base = dnm;
            ureg = pdmp_u01(seed, PDMP_STREAM_MAIN, nm0 + (uint64_t)dnm + (uint64_t)lane);
            LU[lane] = pdmp_log(ureg);
        }
        phc.mark(1);
        const uint32_t idlo = (uint32_t)idw64, idhi = (uint32_t)(idw64 >> 32);
        const bool memberA = gvalid && (idlo & 0x7fffu) != 0x7fffu, memberB = gvalid && ((idlo >> 16) & 0x7fffu) != 0x7fffu,
                   memberC = gvalid && (idhi & 0x7fffu) != 0x7fffu, memberD = gvalid && ((idhi >> 16) & 0x7fffu) != 0x7fffu;
        const bool isG1 = memberA && ((idlo >> 15) & 1u) != 0u;  // zone position gl belongs to G1[i] (the positions 0 .. k − 1)
        const uint32_t sA = memberA ? (idlo & 0x7fffu) : 0xffffffffu;
        const uint32_t sB = memberB ? ((idlo >> 16) & 0x7fffu) : 0xffffffffu;
        const uint32_t sC = memberC ? (idhi & 0x7fffu) : 0xffffffffu;
        const uint32_t sD = memberD ? ((idhi >> 16) & 0x7fffu) : 0xffffffffu;
        const int k = __popc((unsigned)((__ballot(isG1) >> (GW * g)) & GM));                              // |G1[i]|
        const int self = __ffs((unsigned)((__ballot(memberA && sA == i) >> (GW * g)) & GM)) - 1;          // position of i in G1[i]
        phc.mark(2);
        // ---------------- level-2 loads (functions of the member ids), one straight-line batch: the record of G1 member gl (lanes without one
        // read i's) and the tables of member j = G1[i][gl] (lanes without one read i's: L2 hits)
        const uint32_t jA = isG1 ? sA : i;
        ZzRec* rsA = rec + jA;
        double x = rsA->x, th = rsA->th, t = rsA->t, I = rsA->I;
        // the member line of the proposal's own coordinate is needed whatever the outcome (the rejected proposal's re-bound): requested now; the
        // other members' lines only by an accepted event (one proposal in seven), there
        double2 v01 = make_double2(0.0, 0.0), v23 = v01, v45 = v01, v67 = v01, cg = v01;
        if (gl == self) {
            v01 = member2[(size_t)i * 8 + 0];
            v23 = member2[(size_t)i * 8 + 1];
            v45 = member2[(size_t)i * 8 + 2];
            v67 = member2[(size_t)i * 8 + 3];
            cg = member2[(size_t)i * 8 + 4];
            if (FULL && cmut) cg.x = cmut[i];
        }
        rsA = rec + (memberA ? sA : i);
        ZzRec* const rsB = rec + (memberB ? sB : i);
        ZzRec* const rsC = rec + (memberC ? sC : i);
        ZzRec* const rsD = rec + (memberD ? sD : i);

        // ---------------- zone conflicts with earlier groups: a bitmap of the coordinates, set by the groups in event order and tested by the
        // next one.  The DS operations of a wave execute in order, so the E set / test pairs are issued back to back and waited for once.
        PDMP_LDS_ORDER();
        uint64_t confball;
        {
            // (the selection scratch is dead: its readers finished before the PDMP_LDS_ORDER above)
#pragma unroll
            for (int q = 0; q < 2; ++q) reinterpret_cast<uint4*>(BM)[lane + 64 * q] = make_uint4(0u, 0u, 0u, 0u);
            if (lane == 0) BM[512] = 0u;
            PDMP_LDS_ORDER();
            const uint32_t wA = memberA ? (sA >> 5) : 512u, wB = memberB ? (sB >> 5) : 512u, wC = memberC ? (sC >> 5) : 512u,
                           wD = memberD ? (sD >> 5) : 512u;
            const uint32_t bA = memberA ? (1u << (sA & 31u)) : 0u, bB = memberB ? (1u << (sB & 31u)) : 0u, bC = memberC ? (1u << (sC & 31u)) : 0u,
                           bD = memberD ? (1u << (sD & 31u)) : 0u;
            uint32_t rA = 0, rB = 0, rC = 0, rD = 0;
#pragma unroll
            for (int s_ = 0; s_ < E; ++s_) {
                if (g == s_ && gvalid) {  // (group 0 tests nothing: the bitmap is empty)
                    if (s_ > 0) {
                        rA = BM[wA];
                        rB = BM[wB];
                        rC = BM[wC];
                        rD = BM[wD];
                    }
                    atomicOr(&BM[wA], bA);
                    atomicOr(&BM[wB], bB);
                    atomicOr(&BM[wC], bC);
                    atomicOr(&BM[wD], bD);
                }
                PDMP_LDS_ORDER();  // (keeps the groups' blocks in event order: to a single lane they are mutually exclusive branches)
            }
            PDMP_LDS_ORDER();
            const bool hit = ((rA & bA) | (rB & bB) | (rC & bC) | (rD & bD)) != 0u;
            const uint64_t hb = __ballot(hit);
            uint32_t confmask = 0;
#pragma unroll
            for (int s_ = 1; s_ < E; ++s_) confmask |= (((hb >> (GW * s_)) & GM) != 0ull) ? (1u << s_) : 0u;
            confball = confmask;
        }
        PDMP_LDS_ORDER();
        phc.mark(3);

        // ---------------- smove_forward!(G, i, ...), gradient, rates
        {
            const double dt = tp - t;
            const double xn = x + th * dt;
            I = I + dt * ((x + xn) * 0.5);
            x = xn;
            t = tp;
            sx[gl] = x;
            sth[gl] = th;
        }
        PDMP_LDS_ORDER();
        double l, lbound;
        {
            // Γt[:, i] . x in ascending row order (idot): lane p forms its own term, the sum runs over the group's lanes in order; the terms past k
            // are ±0.0 (gamt is zero there, x finite) and change nothing
            const double prod = gv * x;
            double gr = 0.0;
#pragma unroll
            for (uint32_t p = 0; p < KMAX; ++p) gr += bperm_f64(prod, (uint32_t)(GW * g) + p);
            if (FULL && P.tb.gmu_t) gr = gr - P.tb.gmu_t[i];
            const double th_i = sth[self];
            l = pos_part(gr * th_i);
            lbound = pos_part(a_i + b_i * (tp - told_i));
            if (gl == 0) {
                Lr[g] = l;
                LBr[g] = lbound;
            }
        }
        PDMP_LDS_ORDER();
        // ---------------- accept chain in time order (the window starts at the front: the draw at offset o is lane o's); an event whose draws
        // would leave the window ends the candidate list
        uint32_t accbits;
        uint64_t offpack;
        s8_accept_walk<E, GW, true>(ureg, LBr, Lr, k, Esel, accbits, offpack);
        gvalid = g < Esel;
        const uint32_t myoff = (uint32_t)(offpack >> (6 * g)) & 63u;
        const bool accept = gvalid && ((accbits >> g) & 1u) != 0;
        const bool violated = accept && (l >= lbound);  // :123
        phc.mark(4);

        // (a G2 member's velocity does not change: it is not kept, and not stored again)
        double x2 = 0.0, I2 = 0.0, x3 = 0.0, I3 = 0.0, x4 = 0.0, I4 = 0.0;
        if (accept) {
            if (memberA && !isG1) {  // smove_forward!(G2, i, ...), :129
                x = rsA->x;
                th = rsA->th;
                t = rsA->t;
                I = rsA->I;
                const double dt = tp - t;
                const double xn = x + th * dt;
                I = I + dt * ((x + xn) * 0.5);
                x = xn;
                t = tp;
            }
            double tb2 = 0.0, tb3 = 0.0, tb4 = 0.0, th2 = 0.0, th3 = 0.0, th4 = 0.0;
            if (memberB) {
                x2 = rsB->x;
                th2 = rsB->th;
                tb2 = rsB->t;
                I2 = rsB->I;
            }
            if (memberC) {
                x3 = rsC->x;
                th3 = rsC->th;
                tb3 = rsC->t;
                I3 = rsC->I;
            }
            if (memberD) {
                x4 = rsD->x;
                th4 = rsD->th;
                tb4 = rsD->t;
                I4 = rsD->I;
            }
            if (memberB) {
                const double dt = tp - tb2;
                const double xn = x2 + th2 * dt;
                I2 = I2 + dt * ((x2 + xn) * 0.5);
                x2 = xn;
                sx[GW + gl] = x2;
                sth[GW + gl] = th2;
            }
            if (memberC) {
                const double dt = tp - tb3;
                const double xn = x3 + th3 * dt;
                I3 = I3 + dt * ((x3 + xn) * 0.5);
                x3 = xn;
                sx[2 * GW + gl] = x3;
                sth[2 * GW + gl] = th3;
            }
            if (memberD) {
                const double dt = tp - tb4;
                const double xn = x4 + th4 * dt;
                I4 = I4 + dt * ((x4 + xn) * 0.5);
                x4 = xn;
                sx[3 * GW + gl] = x4;
                sth[3 * GW + gl] = th4;
            }
            if (gl == self) th = -th;  // reflect!, :130
            if (memberA) {
                sx[gl] = x;
                sth[gl] = th;
            }
        }
        PDMP_LDS_ORDER();
        // ---------------- re-bound (ab + poisson_time) -- results stay in registers until the commit
        const bool active = gvalid && (accept ? isG1 : (gl == self));
        double key = PDMP_INF, a = 0.0, b = 0.0;
        if (active) {
            if (gl != self) {  // (an accepted event's other members: their lines are requested here, one proposal in seven)
                v01 = member2[(size_t)sA * 8 + 0];
                v23 = member2[(size_t)sA * 8 + 1];
                v45 = member2[(size_t)sA * 8 + 2];
                v67 = member2[(size_t)sA * 8 + 3];
                cg = member2[(size_t)sA * 8 + 4];
                if (FULL && cmut) cg.x = cmut[sA];
            }
            double cj = cg.x;
            const double gmu = cg.y;
            if (FULL && violated && gl == self) cj *= P.factor;  // adapt!(c, i, factor), :127 (stored at commit)
            // Γ[:, j] . x and Γ[:, j] . θ over G1[j] in idot's order; entries past |G1[j]| are 0.0 at position 0
            const double vv[8] = {v01.x, v01.y, v23.x, v23.y, v45.x, v45.y, v67.x, v67.y};
            double gx = 0.0, gt = 0.0;
#pragma unroll
            for (int q = 0; q < (int)KMAX; ++q) {
                const int ps = (int)((posw >> (8 * q)) & 0xff);
                gx += vv[q] * sx[ps];
                gt += vv[q] * sth[ps];
            }
            a = cj + (gx - gmu) * th;
            b = cj / 100 + th * gt;
            const double L = LU[(myoff + 1u + (accept ? (uint32_t)gl : 0u)) & 63u];
            key = t + poisson_time_L(a, b, L);
        }
        PDMP_LDS_ORDER();
        // the patched copy of the popped key block goes where sx / sth were: all their readers are done
        s8_patch_block<KPL>(pk, pk_t, gl, kq, active && (sA >> 5) == blk, sA, key);
        phc.mark(5);
        // ---------------- patched minimum of the popped block, and everything this event could expose
        double rowmin;
        uint32_t cand;
        int wl2;
        s8_patched_min<GW>(pk, pk_t, blk, gvalid, key, g, gl, Mr, rowmin, cand, wl2);
        // ---------------- validate: the committable prefix Rc, its accepted events, the event that violates its bound if it is the next one
        uint32_t Rc, nacc_c;
        int vsel;
        s8_validate<E, GW>(Mr, SLT, confball, gvalid, accept, violated, adapt, tp, g, gl, stop_before, T, P.trace_cap > 0, dnacc + dnref, trace_room, Rc,
                           nacc_c, vsel, status, running);
        phc.mark(6);

        // ---------------- commit the valid prefix
        const bool commit = gvalid && (uint32_t)g < Rc;
        const uint64_t accball2 = __ballot(commit && accept && gl == 0);
        if (commit) {
            if (accept ? memberA : isG1) {
                rsA->x = x;
                rsA->th = th;
                rsA->t = t;
                rsA->I = I;
            }
            if (accept && memberB) {
                rsB->x = x2;
                rsB->t = tp;
                rsB->I = I2;
            }
            if (accept && memberC) {
                rsC->x = x3;
                rsC->t = tp;
                rsC->I = I3;
            }
            if (accept && memberD) {
                rsD->x = x4;
                rsD->t = tp;
                rsD->I = I4;
            }
            if (active) {
                rsA->t_old = t;
                rsA->a = a;
                rsA->b = b;
                keys[sA] = key;
                if (FULL && violated && gl == self) cmut[sA] = cg.x * P.factor;
            }
            if (accept && gl == self) rsA->acc = acc_i + 1;
            if (gl == wl2) {
                bk[blk] = rowmin;
                bi[blk] = (uint16_t)cand;
            }
            if (accept && gl == self && ev) {
                const uint32_t rank = (uint32_t)__popcll(accball2 & ((1ull << (GW * g)) - 1ull));
                pdmp_event e;
                e.t = tp;
                e.i = (int64_t)i;
                e.x = x;
                e.theta = th;
                ev[ntrace0 + dnacc + dnref + rank] = e;
            }
        }
        PDMP_LDS_ORDER();
        phc.mark(7);
        // ---------------- level-1 updates for re-bounded neighbours living in other blocks
        s8_level1_commit<GW>(bk, bi, reinterpret_cast<uint8_t*>(smem + G8_CL), keys, SLB, commit && accept && isG1 && (sA >> 5) != blk, sA, key, k, Rc,
                             accball2, lane);
        phc.mark(8);
        // ---------------- the violating proposal itself (counted, G[i] moved, acc bumped -- then error(...), :120-124), counters
        if (vsel >= 0 && g == vsel && isG1) {
            rsA->x = x;
            rsA->t = t;
            rsA->I = I;
        }
        s8_count<GW>(vsel, Rc, nacc_c, offpack, accball2, SLT, dnum, dnacc, dnm, vnacc, t_last, t_event);
        if (status != PDMP_CHAIN_OK) break;
        PDMP_LDS_ORDER();
    }

    if (PROF && P.dbg && chain == 0 && lane0 == 0) phc.store(P.dbg);
    if (lane0 == 0) s8_store_header<true>(hdr, keys, d, t_last, t_event, dnum, dnacc, vnacc, ntrace0, nm0, dnm, status, has_refresh, t_ref, dnref, ng);
}
