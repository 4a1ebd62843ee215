// pdmp_capi_zigzag.hip -- the factorised samplers: flow, neighbourhood, targets, the neighbourhood programs, the state and its options.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>

#include "pdmp_ensemble.hpp"

#include "../../include/pdmp_detmath.h"

// g1mask (optional, one flag per stored entry): the structural entries of the bounding Γ, i.e. G1 (src/sfact.jl:170), when the pattern handed
// over is the larger neighbourhood G ⊇ G1 of spdmp(∇ϕ, t0, x0, θ0, T, c, G, F, ...) (:162,171-179) with explicit zeros outside G1
static pdmp_status set_flow_common(pdmp_ensemble* e, const int64_t* colptr, const int64_t* rowval, const double* nzval,
                                   const double* mu, const double* sigma, double lambda_ref, double rho, int kind,
                                   const uint8_t* g1mask = nullptr) {
    if (!e || !colptr || !rowval || !nzval) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int64_t d = e->cfg.d;
    PDMP_TRY(check_csc("flow matrix", colptr, rowval, d, d));
    const int64_t nnz = colptr[d];
    if (nnz <= 0 || nnz >= (int64_t)1 << 31) return fail(PDMP_ERR_INVALID, "bad nnz %lld", (long long)nnz);
    if (lambda_ref < 0) return fail(PDMP_ERR_INVALID, "lambda_ref < 0");
    e->colptr.assign(colptr, colptr + d + 1);
    e->rowval.assign(nnz, 0);
    e->bval.assign(nzval, nzval + nnz);
    std::vector<uint8_t> selfpos(d, 0);
    std::vector<uint16_t> selfpos16(d, 0);
    bool general = false;
    uint32_t mmax_all = 0;
    for (int64_t i = 0; i < d; ++i) {
        const int64_t k = colptr[i + 1] - colptr[i];
        if (k > 4096) return fail(PDMP_ERR_UNSUPPORTED, "column %lld has %lld > 4096 non-zeros", (long long)i, (long long)k);
        bool has_diag = false;
        for (int64_t p = colptr[i]; p < colptr[i + 1]; ++p) {
            const int64_t r = rowval[p];
            if (r == i && (!g1mask || g1mask[p])) {
                has_diag = true;
                selfpos[i] = (uint8_t)(p - colptr[i]);
                selfpos16[i] = (uint16_t)(p - colptr[i]);
            }
            e->rowval[p] = (uint32_t)r;
        }
        if (!has_diag)  // (stickyzz re-bounds i itself at its thaw, src/stickyzz.jl:277-283: a call error there)
            return fail(e->cfg.sampler == PDMP_SAMPLER_BARRIER_ZIGZAG ? PDMP_ERR_INVALID : PDMP_ERR_UNSUPPORTED,
                        "Γ[%lld,%lld] is structurally zero: i must belong to G1[i]", (long long)i, (long long)i);
    }
    e->nnz = nnz;
    e->mu.assign(d, 0.0);
    if (mu) e->mu.assign(mu, mu + d);
    e->sigma.assign(d, 1.0);
    if (sigma) e->sigma.assign(sigma, sigma + d);
    e->lambda_ref = lambda_ref;
    e->rho = rho;

    // gmu_b[i] = idot(Γ, i, μ) (src/fact_samplers.jl:51), summed in CSC order like idot (src/common.jl:16-24)
    std::vector<double> gmu(d, 0.0);
    for (int64_t i = 0; i < d; ++i) {
        double s = 0.0;
        for (uint32_t p = e->colptr[i]; p < e->colptr[i + 1]; ++p) s += e->bval[p] * e->mu[e->rowval[p]];
        gmu[i] = s;
    }

    // S[i] = G1[i] ++ G2[i], G2[i] = (∪_{j∈G1[i]} G1[j]) \ G1[i]  (src/sfact.jl:178), both ascending
    std::vector<uint32_t> sptr(d + 1, 0), sidx;
    sidx.reserve((size_t)nnz * 3);
    std::vector<uint32_t> qptr(nnz + 1, 0);
    std::vector<uint8_t> pos;
    pos.reserve((size_t)nnz * 5);
    std::vector<uint16_t> pos16, qrow16;
    std::vector<double> qbval;     // Γ value of every (member j of G1[i], entry of column j) pair, same order as pos16
    std::vector<uint32_t> member;  // per entry p of column i: {j, k_j, qptr[p], 0} -- one 16-byte load per member
    pos16.reserve((size_t)nnz * 5);
    std::vector<uint32_t> tmp;
    for (int64_t i = 0; i < d; ++i) {
        const uint32_t c0 = e->colptr[i], c1 = e->colptr[i + 1];
        tmp.clear();
        for (uint32_t p = c0; p < c1; ++p) {
            if (g1mask && !g1mask[p]) continue;  // G2[i] = ∪_{j ∈ G1[i]} G1[j] \ G[i], src/sfact.jl:178
            const uint32_t j = e->rowval[p];
            for (uint32_t q = e->colptr[j]; q < e->colptr[j + 1]; ++q)
                if (!g1mask || g1mask[q]) tmp.push_back(e->rowval[q]);
        }
        std::sort(tmp.begin(), tmp.end());
        tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
        const size_t s0 = sidx.size();
        for (uint32_t p = c0; p < c1; ++p) sidx.push_back(e->rowval[p]);
        for (uint32_t v : tmp) {
            if (!std::binary_search(e->rowval.begin() + c0, e->rowval.begin() + c1, v)) sidx.push_back(v);
        }
        const size_t m = sidx.size() - s0;
        if (m > 4096)
            return fail(PDMP_ERR_UNSUPPORTED, "two-hop neighbourhood of coordinate %lld has %zu > 4096 members",
                        (long long)i, m);
        if (m > 64 || (c1 - c0) > 64) general = true;  // beyond one lane per member: pdmp_general.hip
        mmax_all = std::max<uint32_t>(mmax_all, (uint32_t)m);
        sptr[i + 1] = (uint32_t)sidx.size();
        // positions inside S[i] of the members of G1[j], j = G1[i][jj]
        for (uint32_t p = c0; p < c1; ++p) {
            const uint32_t j = e->rowval[p];
            qptr[p] = (uint32_t)pos.size();
            if (g1mask && !g1mask[p]) continue;  // (a member of G[i] \ G1[i]: moved, never re-bounded)
            for (uint32_t q = e->colptr[j]; q < e->colptr[j + 1]; ++q) {
                if (g1mask && !g1mask[q]) continue;
                const uint32_t r = e->rowval[q];
                size_t where = m;
                for (size_t w = 0; w < m; ++w) {
                    if (sidx[s0 + w] == r) {
                        where = w;
                        break;
                    }
                }
                if (where == m)
                    return fail(PDMP_ERR_UNSUPPORTED,
                                "pattern of Γ is not symmetric: row %u of column %u is not reachable from %lld", r, j,
                                (long long)i);
                pos.push_back((uint8_t)where);
                pos16.push_back((uint16_t)where);
                qrow16.push_back((uint16_t)r);  // (used by the small-d kernel only: d < 65536 is checked there)
                qbval.push_back(e->bval[q]);
            }
        }
    }
    qptr[nnz] = (uint32_t)pos.size();
    if (pos.empty()) pos.push_back(0);
    if (pos16.empty()) pos16.push_back(0);
    if (qbval.empty()) qbval.push_back(0.0);
    if (qrow16.empty()) qrow16.push_back(0);
    member.resize((size_t)nnz * 4 + 4, 0u);
    for (int64_t p = 0; p < nnz; ++p) {
        const uint32_t j = e->rowval[p];
        member[(size_t)p * 4 + 0] = j;
        uint32_t kj = 0;
        for (uint32_t q = e->colptr[j]; q < e->colptr[j + 1]; ++q) kj += (!g1mask || g1mask[q]) ? 1u : 0u;
        member[(size_t)p * 4 + 1] = (g1mask && !g1mask[p]) ? 0u : kj;
        member[(size_t)p * 4 + 2] = qptr[p];
        member[(size_t)p * 4 + 3] = (!g1mask || g1mask[p]) ? 1u : 0u;
    }
    {
        uint32_t hist[16] = {0}, best = 0;
        for (int64_t k = 0; k < d; ++k) hist[std::min<uint32_t>(e->colptr[(size_t)k + 1] - e->colptr[(size_t)k], 15u)] += 1;
        for (uint32_t k = 1; k < 16; ++k)
            if (hist[k] > hist[best]) best = k;
        e->typ_extra = best > 0 ? best - 1u : 0u;
    }
    e->flow_kind = kind;
    e->has_g1mask = g1mask != nullptr;
    e->needs_general = general || kind == 1 || e->has_g1mask;  // FactBoomerang and G ⊋ G1 run on the general kernel
    e->mmax_all = mmax_all;
    {
        std::vector<double> diag((size_t)d, 0.0);
        for (int64_t i = 0; i < d; ++i) diag[i] = e->bval[e->colptr[i] + selfpos16[i]];
        PDMP_TRY(e->d_diag.upload(diag));
        PDMP_TRY(e->d_mu.upload(e->mu));
    }

    e->h_gmu_b = gmu;
    e->h_sptr = sptr;
    e->h_sidx = sidx;
    e->h_qptr = qptr;
    e->h_pos = pos;
    e->h_selfpos = selfpos;

    PDMP_TRY(e->d_colptr.upload(e->colptr));
    PDMP_TRY(e->d_rowval.upload(e->rowval));
    PDMP_TRY(e->d_bval.upload(e->bval));
    PDMP_TRY(e->d_gmu_b.upload(gmu));
    PDMP_TRY(e->d_sptr.upload(sptr));
    PDMP_TRY(e->d_sidx.upload(sidx));
    PDMP_TRY(e->d_qptr.upload(qptr));
    PDMP_TRY(e->d_pos.upload(pos));
    PDMP_TRY(e->d_selfpos.upload(selfpos));
    PDMP_TRY(e->d_sigma.upload(e->sigma));
    PDMP_TRY(e->d_pos16.upload(pos16));
    PDMP_TRY(e->d_qbval.upload(qbval));
    PDMP_TRY(e->d_qrow16.upload(qrow16));
    PDMP_TRY(e->d_member.upload(member));
    PDMP_TRY(e->d_selfpos16.upload(selfpos16));
    e->target_kind = 0;

    const int64_t nkeys = d + 1;  // slot d is the refresh clock (+Inf when λref = 0)
    e->nblk = (uint32_t)((nkeys + 63) / 64);
    e->nblk_pad = (e->nblk + 1u) & ~1u;
    e->dk = (int64_t)e->nblk * 64;
    e->local_bound = false;
    e->adaptscale = false;
    e->has_flow = true;
    e->has_target = false;
    e->has_state = false;
    return PDMP_OK;
}

// Per-coordinate "neighbourhood program": everything a proposal at coordinate i needs that depends on i alone,
// packed in 64-bit words so that ONE coalesced wave load brings it on chip (kernel: zz_local_run_kernel).
//   [0]                 k | m<<8 | selfpos<<16 | kjmax<<24          (kjmax = max_j |G1[j]|, j in G1[i])
//   [1 .. 1+SW)         S[i] = G1[i] ++ G2[i], two u32 ids per word                (SW = ceil(MMAX/2))
//   then k sub-records of R = 4 + PW + KMAX words, one per j = G1[i][jj]:
//     [0] Γt[j,i] (target)   [1] Γ[:,j]·μ   [2] c[j]   [3] |G1[j]|
//     [4 .. 4+PW)        positions inside S[i] of the members of G1[j], 8 bytes per word (PW = ceil(KMAX/8))
//     [4+PW .. +KMAX)    Γ[G1[j], j] (bounding precision values, CSC order)
static pdmp_status build_blob(pdmp_ensemble* e, const double* c) {
    const int64_t d = e->cfg.d;
    uint32_t kmax = 0, mmax = 0;
    for (int64_t i = 0; i < d; ++i) {
        kmax = std::max(kmax, e->colptr[i + 1] - e->colptr[i]);
        mmax = std::max(mmax, e->h_sptr[i + 1] - e->h_sptr[i]);
    }
    const uint32_t SW = (mmax + 1) / 2, PW = (kmax + 7) / 8, R = 4 + PW + kmax;
    const uint32_t W = 1 + SW + kmax * R;
    const uint32_t Wpad = (W + 1u) & ~1u;
    if ((double)W * 8.0 * (double)d > 4.0e9)
        return fail(PDMP_ERR_UNSUPPORTED, "neighbourhood programs would take %.1f GB (d=%lld, max column nnz %u)",
                    (double)W * 8.0 * (double)d / 1e9, (long long)d, kmax);
    if (pdmp::zz_local_lds_bytes(e->nblk_pad, Wpad) > 160 * 1024)
        return fail(PDMP_ERR_UNSUPPORTED, "d = %lld / max column nnz %u need %zu bytes of LDS per chain (> 160 KiB)",
                    (long long)d, kmax, pdmp::zz_local_lds_bytes(e->nblk_pad, Wpad));
    std::vector<uint64_t> blob((size_t)Wpad * (size_t)d, 0);
    auto bits = [](double v) {
        uint64_t u;
        memcpy(&u, &v, sizeof u);
        return u;
    };
    for (int64_t i = 0; i < d; ++i) {
        uint64_t* B = blob.data() + (size_t)i * Wpad;
        const uint32_t c0 = e->colptr[i], k = e->colptr[i + 1] - c0;
        const uint32_t s0 = e->h_sptr[i], m = e->h_sptr[i + 1] - s0;
        uint32_t kjmax = 0;
        for (uint32_t w = 0; w < m; ++w) {
            // member ids RELATIVE to i (two's complement u32): coordinates with the same local structure -- every interior
            // point of a lattice -- then share one program, and the table shrinks from d programs to a few dozen
            const uint64_t id = (uint32_t)(e->h_sidx[s0 + w] - (uint32_t)i);
            B[1 + (w >> 1)] |= (w & 1) ? (id << 32) : id;
        }
        for (uint32_t jj = 0; jj < k; ++jj) {
            const uint32_t j = e->rowval[c0 + jj];
            const uint32_t cj0 = e->colptr[j], kj = e->colptr[j + 1] - cj0;
            kjmax = std::max(kjmax, kj);
            uint64_t* S = B + 1 + SW + (size_t)jj * R;
            S[0] = bits(e->h_tval[c0 + jj]);
            S[1] = bits(e->h_gmu_b[j]);
            S[2] = bits(c[j]);
            S[3] = kj;
            const uint32_t q0 = e->h_qptr[c0 + jj];
            for (uint32_t pp = 0; pp < kj; ++pp) {
                S[4 + (pp >> 3)] |= (uint64_t)e->h_pos[q0 + pp] << (8 * (pp & 7));
                S[4 + PW + pp] = bits(e->bval[cj0 + pp]);
            }
        }
        B[0] = (uint64_t)k | ((uint64_t)m << 8) | ((uint64_t)e->h_selfpos[i] << 16) | ((uint64_t)kjmax << 24);
    }
    // de-duplicate identical programs
    std::vector<uint32_t> tix((size_t)d, 0);
    std::vector<uint64_t> templates;
    {
        std::unordered_map<std::string, uint32_t> seen;
        seen.reserve(1024);
        for (int64_t i = 0; i < d; ++i) {
            const uint64_t* B = blob.data() + (size_t)i * Wpad;
            std::string key(reinterpret_cast<const char*>(B), (size_t)Wpad * 8);
            auto it = seen.find(key);
            if (it == seen.end()) {
                const uint32_t id = (uint32_t)seen.size();
                seen.emplace(std::move(key), id);
                templates.insert(templates.end(), B, B + Wpad);
                tix[i] = id;
            } else {
                tix[i] = it->second;
            }
        }
        e->n_templates = seen.size();
        std::vector<int64_t> cnt(seen.size(), 0);
        for (int64_t i = 0; i < d; ++i) cnt[tix[i]] += 1;
        e->common_tix = (uint32_t)(std::max_element(cnt.begin(), cnt.end()) - cnt.begin());
    }
    blob.swap(templates);
    PDMP_TRY(e->d_tix.upload(tix));
    e->blob_w = W;
    e->blob_w_pad = Wpad;
    e->blob_sw = SW;
    e->blob_pw = PW;
    e->blob_kmax = kmax;
    e->blob_mmax = mmax;
    // (pdmp_debug_set_kernel(PDMP_DEBUG_KERNEL_SEQ) forces the one-event-per-iteration kernel: A/B runs, parity tests)
    // eight events per iteration off the lattice: per-coordinate tables instead of blob templates (pdmp_spec8g.inc)
    e->has_g8 = false;
    e->g8_same = false;
    // (every graph of that size whose blob geometry is not EXACTLY the 2-d lattice's, which zz_local_spec8_kernel serves from LDS templates)
    e->g8_gw = 8;
    if (kmax <= 8 && mmax <= 64 && d >= 2048 && d <= 16384 && !(SW == 7 && PW == 1 && kmax == 5 && Wpad == 58)) {
        // 8 lanes per event (eight events per iteration) up to |S| = 32, 16 lanes (four events) up to 64: a lane owns zone positions gl + q GW
        const uint32_t GW = (mmax <= 32) ? 8u : 16u, LSTR = GW + 8u;
        e->g8_gw = (int)GW;
        std::vector<uint64_t> line((size_t)d * LSTR, 0ull);
        std::vector<double> member((size_t)d * 16, 0.0), gamt((size_t)d * 8, 0.0);
        bool same = true;
        for (int64_t i = 0; i < d; ++i) {
            const uint32_t c0 = e->colptr[i], k = e->colptr[i + 1] - c0;
            const uint32_t s0 = e->h_sptr[i], m = e->h_sptr[i + 1] - s0;
            uint16_t ids[64];
            for (uint32_t w = 0; w < 4 * GW; ++w) ids[w] = (w < m) ? (uint16_t)(e->h_sidx[s0 + w] | (w < k ? 0x8000u : 0u)) : (uint16_t)0x7FFF;
            for (uint32_t gl = 0; gl < GW; ++gl)
                line[(size_t)i * LSTR + gl] = (uint64_t)ids[gl] | ((uint64_t)ids[gl + GW] << 16) | ((uint64_t)ids[gl + 2 * GW] << 32) | ((uint64_t)ids[gl + 3 * GW] << 48);
            for (uint32_t jj = 0; jj < k; ++jj) {
                gamt[(size_t)i * 8 + jj] = e->h_tval[c0 + jj];
                member[(size_t)i * 16 + jj] = e->bval[c0 + jj];
                same = same && e->h_tval[c0 + jj] == e->bval[c0 + jj];
                const uint32_t j = e->rowval[c0 + jj];
                const uint32_t kj = e->colptr[j + 1] - e->colptr[j];
                const uint32_t q0 = e->h_qptr[c0 + jj];
                uint64_t pw = 0;
                for (uint32_t pp = 0; pp < kj; ++pp) pw |= (uint64_t)e->h_pos[q0 + pp] << (8 * pp);
                line[(size_t)i * LSTR + GW + jj] = pw;
            }
            member[(size_t)i * 16 + 8] = c[i];
            member[(size_t)i * 16 + 9] = e->h_gmu_b[i];
        }
        PDMP_TRY(e->d_g8_line.upload(line));
        PDMP_TRY(e->d_g8_member.upload(member));
        if (!same) PDMP_TRY(e->d_g8_gamt.upload(gamt));
        e->g8_same = same;
        e->has_g8 = true;
    }
    e->use_spec = pdmp::zz_spec_supported(e->nblk, mmax, kmax) && e->dbg_kernel != PDMP_DEBUG_KERNEL_SEQ &&
                  (mmax > 16 ? pdmp::zz_spec_wide_lds_bytes(e->nblk_pad, Wpad) : pdmp::zz_spec_lds_bytes(e->nblk_pad, Wpad)) <= 64 * 1024;
    return e->d_blob.upload(blob);
}

// the n x n 5-point lattice in column-major numbering (scripts/gridlaplace.jl): G1[i] = {i-n, i-1, i, i+1, i+n} inside the grid
static void detect_lattice(pdmp_ensemble* e) {
    const int64_t d = e->cfg.d;
    e->lattice_n = 0;
    int64_t nl = (int64_t)std::llround(std::sqrt((double)d));
    bool lat = nl * nl == d && nl >= 16 && nl <= 256 && !e->colptr.empty();  // (256: pdmp_trackp.hip's 8192 block bounds; other users check their own limit)
    for (int64_t col = 0; lat && col < nl; ++col)
        for (int64_t row = 0; lat && row < nl; ++row) {
            const int64_t ii = row + nl * col;
            uint32_t want[5];
            int nw = 0;
            if (col > 0) want[nw++] = (uint32_t)(ii - nl);
            if (row > 0) want[nw++] = (uint32_t)(ii - 1);
            want[nw++] = (uint32_t)ii;
            if (row < nl - 1) want[nw++] = (uint32_t)(ii + 1);
            if (col < nl - 1) want[nw++] = (uint32_t)(ii + nl);
            if ((int64_t)(e->colptr[ii + 1] - e->colptr[ii]) != nw) {
                lat = false;
                break;
            }
            for (int q = 0; q < nw; ++q)
                if (e->rowval[e->colptr[ii] + q] != want[q]) lat = false;
        }
    if (lat) e->lattice_n = (int32_t)nl;
}

static pdmp_status alloc_state(pdmp_ensemble* e) {
    const int64_t d = e->cfg.d, n = e->cfg.nchains;
    const size_t nrec = (size_t)(n * d) * (e->track ? 2 : 1);  // TrRec is two ZzRec long
    if (e->d_rec.n != nrec) PDMP_TRY(e->d_rec.alloc(nrec, &e->place_cfg, &e->place_cfg.rec));
    if (e->d_keys.n != (size_t)(n * e->dk)) PDMP_TRY(e->d_keys.alloc((size_t)(n * e->dk)));
    if (e->d_hdr.n != (size_t)n) PDMP_TRY(e->d_hdr.alloc((size_t)n));
    if (e->cfg.adapt && e->d_c_chain.n != (size_t)(n * d)) PDMP_TRY(e->d_c_chain.alloc((size_t)(n * d)));
    if (e->cfg.trace_capacity > 0 && e->d_ev.n != (size_t)(n * e->cfg.trace_capacity))
        PDMP_TRY(e->d_ev.alloc((size_t)(n * e->cfg.trace_capacity), &e->place_cfg, &e->place_cfg.ev));
    e->d_jprev.release();
    return PDMP_OK;
}

// Γ[i,j] is read where the reference reads Γ[j,i] (the stored column of the reflecting coordinate): is the bounding matrix symmetric, in pattern and
// values?  With two_sums also the target's, and *two_sums tells whether the two matrices differ anywhere.
static bool symmetric_matrices(const pdmp_ensemble* e, bool* two_sums) {
    bool two = false;
    for (int64_t col = 0; col < e->cfg.d; ++col)
        for (uint32_t pp = e->colptr[col]; pp < e->colptr[col + 1]; ++pp) {
            const uint32_t row = e->rowval[pp];
            const uint32_t* lo = e->rowval.data() + e->colptr[row];
            const uint32_t* hi = e->rowval.data() + e->colptr[row + 1];
            const uint32_t* it = std::lower_bound(lo, hi, (uint32_t)col);
            if (it == hi || *it != (uint32_t)col) return false;
            const size_t q = (size_t)(it - e->rowval.data());
            if (e->bval[q] != e->bval[pp] || (two_sums && e->h_tval[q] != e->h_tval[pp])) return false;
            if (two_sums && e->bval[pp] != e->h_tval[pp]) two = true;
        }
    if (two_sums) *two_sums = two;
    return true;
}

// what zz_trackp_supported / zz_trackl_supported ask about an ensemble whose state is being set (track_mean decided)
static pdmp::ZzRunParams track_query_params(const pdmp_ensemble* e) {
    pdmp::ZzRunParams G{};
    G.tb = e->tables();
    if (e->track_mean == 2) G.tb.gmu_t = nullptr;  // (the target's mean is served: the support tests need not refuse it)
    G.lattice_n = e->lattice_n;
    G.adapt = e->cfg.adapt;
    G.c_chain = e->cfg.adapt ? e->d_c_chain.p : nullptr;
    G.track_two_sums = e->track_two_sums ? 1 : 0;
    G.has_refresh = e->lambda_ref > 0;
    G.d = e->cfg.d;
    return G;
}

pdmp_status init_state(pdmp_ensemble* e, double t0, const double* x0, const double* th0, const double* c,
                              const uint64_t* seeds, uint64_t seed0) {
    if (!e->has_flow || !e->has_target) return fail(PDMP_ERR_INVALID, "flow and target must be set before the state");
    const bool sticky = e->cfg.sampler == PDMP_SAMPLER_STICKY_ZIGZAG;
    if (sticky && !e->has_kappa) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_set_sticky must be called before the state");
    if (!c) return fail(PDMP_ERR_INVALID, "c is required");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int64_t d = e->cfg.d, n = e->cfg.nchains;
    const bool barrier = e->cfg.sampler == PDMP_SAMPLER_BARRIER_ZIGZAG;
    if (barrier) {
        // stickyzz (src/stickyzz.jl) runs on zz_barrier_run_kernel alone: everything that kernel does not take is refused here, never served by another
        if (!e->has_barriers) return fail(PDMP_ERR_INVALID, "pdmp_ensemble_set_barriers must be called before the state");
        if (e->flow_kind != 0 || e->lambda_ref > 0)
            return fail(PDMP_ERR_UNSUPPORTED, "stickyzz: a ZigZag flow without refreshment (src/stickyzz.jl has no refresh clock)");
        if (e->target_kind != 0) return fail(PDMP_ERR_UNSUPPORTED, "stickyzz: the Gaussian target only");
        if (e->has_g1mask) return fail(PDMP_ERR_UNSUPPORTED, "stickyzz: G = G1 only (no pdmp_ensemble_set_neighbourhood)");
        if (e->track_requested || e->local_bound)  // (adaptscale: pdmp_ensemble_set_adaptscale itself refuses every sampler but spdmp, PDMP_ERR_UNSUPPORTED)
            return fail(PDMP_ERR_UNSUPPORTED, "stickyzz: no gradient tracking or LocalBound");
        if (e->needs_general)
            return fail(PDMP_ERR_UNSUPPORTED, "stickyzz: neighbourhoods of at most 64 members (|G1[i]| and |G1[i] ∪ G2[i]|), as zz_sticky_run_kernel takes");
        for (int64_t i = 0; i < d; ++i)  // (the head draw and one draw per re-bounded member come from the 64 candidates of an iteration)
            if (e->colptr[(size_t)i + 1] - e->colptr[(size_t)i] > 63u)
                return fail(PDMP_ERR_UNSUPPORTED, "stickyzz: |G1[%lld]| = %u > 63", (long long)i, e->colptr[(size_t)i + 1] - e->colptr[(size_t)i]);
        if (!x0 || !th0) return fail(PDMP_ERR_UNSUPPORTED, "stickyzz: an explicit state (x0 must lie inside the barriers)");
        for (int64_t q = 0; q < n * d; ++q) {
            const pdmp::BarrierEntry& be = e->h_barriers[(size_t)(q % d)];
            if (!(th0[q] != 0.0) || th0[q] != th0[q])  // dir(ui) = 0 indexes barrier.x[0], src/stickyzz.jl:115,121
                return fail(PDMP_ERR_INVALID, "stickyzz: θ0[%lld] of chain %lld is %g: every coordinate needs a direction", (long long)(q % d), (long long)(q / d), th0[q]);
            // a box (lo < hi) holds its coordinate: a start outside it is the reference's own "fix me" (src/stickyzz.jl:121).  lo == hi is one
            // level met from either side (sspdmp2's (0, 0), :330): any start is inside
            if (be.lo < be.hi && !(x0[q] >= be.lo && x0[q] <= be.hi))
                return fail(PDMP_ERR_INVALID, "stickyzz: x0[%lld] = %g of chain %lld lies outside its barriers [%g, %g]", (long long)(q % d), x0[q], (long long)(q / d), be.lo, be.hi);
        }
    }
    if (e->target_kind == TARGET_BRIDGE) {
        // the diffusion bridge runs on zz_bridge_run_kernel alone (pdmp_bridge.inc): the script's configuration (research/diffusion_bridge/diffbridge.jl:
        // ZigZag(sparse(I), 0), fixed end points), everything else is refused here, never served by another kernel
        if (e->cfg.sampler != PDMP_SAMPLER_ZIGZAG_LOCAL) return fail(PDMP_ERR_UNSUPPORTED, "diffusion bridge: spdmp only (PDMP_SAMPLER_ZIGZAG_LOCAL)");
        if (e->flow_kind != 0) return fail(PDMP_ERR_UNSUPPORTED, "diffusion bridge: a ZigZag flow, not a FactBoomerang");
        if (e->has_g1mask) return fail(PDMP_ERR_UNSUPPORTED, "diffusion bridge: no pdmp_ensemble_set_neighbourhood (the gradient moves what it reads; G = G1 = {i})");
        if (e->adaptscale) return fail(PDMP_ERR_UNSUPPORTED, "diffusion bridge: no adaptscale");  // (it comes with a refresh clock: named first)
        if (e->lambda_ref > 0) return fail(PDMP_ERR_UNSUPPORTED, "diffusion bridge: no refresh clock (lambda_ref = %g)", e->lambda_ref);
        bool ident = e->nnz == d;
        for (int64_t i = 0; ident && i < d; ++i) ident = e->rowval[(size_t)i] == (uint32_t)i && e->bval[(size_t)i] == 1.0;
        if (!ident) return fail(PDMP_ERR_UNSUPPORTED, "diffusion bridge: the flow's Γ must be the identity (ZigZag(sparse(I), 0))");
        for (int64_t i = 0; i < d; ++i)
            if (e->mu[(size_t)i] != 0.0) return fail(PDMP_ERR_UNSUPPORTED, "diffusion bridge: the flow's μ must be 0 (μ[%lld] = %g)", (long long)i, e->mu[(size_t)i]);
        if (e->track_requested) return fail(PDMP_ERR_UNSUPPORTED, "diffusion bridge: no gradient tracking (the gradient is a fresh Monte Carlo estimate at every proposal)");
        if (e->local_bound) return fail(PDMP_ERR_UNSUPPORTED, "diffusion bridge: no LocalBound (pdmp_ensemble_set_local_bound)");
        if (!x0 || !th0) return fail(PDMP_ERR_UNSUPPORTED, "diffusion bridge: an explicit state (the end points ξ[0], ξ[d-1] are data)");
        // the reference's end-point gradients (faberschauder.jl:129-136) read coefficients they did not move: fixed end points are what is served
        for (int64_t k = 0; k < n; ++k)
            for (int64_t i : {(int64_t)0, d - 1})
                if (th0[k * d + i] != 0.0)
                    return fail(PDMP_ERR_UNSUPPORTED, "diffusion bridge: θ0[%lld] = %g of chain %lld: the end points are fixed (θ0 = 0 at both; free end points are not implemented)",
                                (long long)i, th0[k * d + i], (long long)k);
    }
    if (e->target_kind == TARGET_PRECISION) {
        // the Cholesky-factor precision target runs on zz_precision_run_kernel alone (pdmp_precision.inc): the case study's configuration
        // (casestudies/precision/precision.jl: sspdmp with a diagonal Γ̂), everything else is refused here, never served by another kernel
        if (!sticky) return fail(PDMP_ERR_UNSUPPORTED, "precision cholesky: sspdmp only (PDMP_SAMPLER_STICKY_ZIGZAG)");
        if (e->flow_kind != 0) return fail(PDMP_ERR_UNSUPPORTED, "precision cholesky: a ZigZag flow, not a FactBoomerang");
        if (e->has_g1mask)
            return fail(PDMP_ERR_UNSUPPORTED, "precision cholesky: no pdmp_ensemble_set_neighbourhood (G[i] is the column of i, the target's own; G1[i] = {i})");
        // (adaptscale: pdmp_ensemble_set_adaptscale itself refuses every sampler but spdmp, PDMP_ERR_UNSUPPORTED; a refresh clock gets here only
        // where the flow was set again after pdmp_ensemble_set_sticky, which refuses one)
        if (e->lambda_ref > 0) return fail(PDMP_ERR_UNSUPPORTED, "precision cholesky: no refresh clock (lambda_ref = %g)", e->lambda_ref);
        bool diagonal = e->nnz == d;
        for (int64_t i = 0; diagonal && i < d; ++i) diagonal = e->rowval[(size_t)i] == (uint32_t)i && e->bval[(size_t)i] > 0 && std::isfinite(e->bval[(size_t)i]);
        if (!diagonal) return fail(PDMP_ERR_UNSUPPORTED, "precision cholesky: the flow's Γ must be diagonal with positive entries (ZigZag(diag Γ̂, μ̂))");
        if (e->track_requested) return fail(PDMP_ERR_UNSUPPORTED, "precision cholesky: no gradient tracking (the diagonal's −N/u term is not linear in time)");
        if (e->local_bound) return fail(PDMP_ERR_UNSUPPORTED, "precision cholesky: no LocalBound (pdmp_ensemble_set_local_bound)");
        if (!x0 || !th0) return fail(PDMP_ERR_UNSUPPORTED, "precision cholesky: an explicit state (the diagonal of L must start positive)");
        const int64_t pn = e->precision.n;
        for (int64_t k = 0; k < n; ++k)
            for (int64_t cc = 0; cc < pn; ++cc) {
                const int64_t i = cc * pn - cc * (cc - 1) / 2;
                if (!(x0[k * d + i] > 0))
                    return fail(PDMP_ERR_UNSUPPORTED, "precision cholesky: x0[%lld] = %g of chain %lld: the diagonal coordinates L[c, c] must start > 0 (the potential has −N log L[c, c])",
                                (long long)i, x0[k * d + i], (long long)k);
            }
    }
    e->track = false;
    e->track_lg = false;
    if (e->track_requested && e->target_kind == 1) {
        // tracked BOUNDS under the subsampled logistic target (pdmp_logistic.hip, TRK): the plain spdmp configuration of config C4 only
        if (e->cfg.sampler != PDMP_SAMPLER_ZIGZAG_LOCAL || e->flow_kind != 0 || e->adaptscale || e->local_bound || e->lambda_ref > 0 ||
            e->dbg_kernel != PDMP_DEBUG_KERNEL_AUTO || e->dbg_dump > 0 || e->has_g1mask)
            return fail(PDMP_ERR_UNSUPPORTED, "gradient tracking with the logistic target: spdmp, ZigZag flow without refresh, G = Matched()");
        if (!symmetric_matrices(e, nullptr)) return fail(PDMP_ERR_UNSUPPORTED, "gradient tracking needs a symmetric bounding matrix");
        e->track_lg = true;
    } else
    if (e->track_requested) {
        // opt-in, so never a silent fall-back: everything the tracked-gradient kernel needs is checked here
        if (e->cfg.sampler != PDMP_SAMPLER_ZIGZAG_LOCAL || e->needs_general || e->target_kind != 0 || e->flow_kind != 0 || e->adaptscale ||
            e->local_bound || e->lambda_ref > 0 || e->dbg_kernel != PDMP_DEBUG_KERNEL_AUTO || e->dbg_dump > 0)
            return fail(PDMP_ERR_UNSUPPORTED, "gradient tracking: spdmp with a ZigZag flow without refresh and the Gaussian target only");
        bool two = false;
        if (!symmetric_matrices(e, &two)) return fail(PDMP_ERR_UNSUPPORTED, "gradient tracking needs symmetric precision matrices (flow and target)");
        e->track_two_sums = two;
        e->track = true;
        detect_lattice(e);
    }
    // the bit-identical one-proposal-per-lane kernel (pdmp_exactp.hip; opt-in with PDMP_DEBUG_KERNEL_EXACTP: measured at 2x the 8-event
    // kernel's time) wants the plain lattice with the bounding Γ equal to the target's
    e->exactp = false;
    if (!e->track_requested && e->cfg.sampler == PDMP_SAMPLER_ZIGZAG_LOCAL && !e->needs_general && e->target_kind == 0 && e->flow_kind == 0 &&
        !e->adaptscale && !e->local_bound && !(e->lambda_ref > 0) && !e->cfg.adapt && !e->has_tmu && e->dbg_kernel == PDMP_DEBUG_KERNEL_EXACTP &&
        e->dbg_dump == 0 && e->h_tval.size() == e->bval.size()) {
        bool same = true, mu0 = true;
        for (size_t q = 0; q < e->bval.size() && same; ++q) same = e->bval[q] == e->h_tval[q];
        for (size_t q = 0; q < e->h_gmu_b.size() && mu0; ++q) mu0 = e->h_gmu_b[q] == 0.0;
        if (same && mu0) {
            detect_lattice(e);
            e->exactp = e->lattice_n != 0;
        }
    }
    PDMP_TRY(alloc_state(e));
    std::vector<double> cv(c, c + d);
    PDMP_TRY(e->d_c.upload(cv));
    {
        std::vector<double> c2v((size_t)d * 2);
        for (int64_t k = 0; k < d; ++k) {
            c2v[2 * (size_t)k] = c[k];
            c2v[2 * (size_t)k + 1] = c[k] / 100;
        }
        PDMP_TRY(e->d_c2.upload(c2v));
        std::vector<pdmp::CoordConst> ccv((size_t)d);
        for (int64_t k = 0; k < d; ++k) {
            ccv[(size_t)k].c = c[k];
            ccv[(size_t)k].c100 = c[k] / 100;
            ccv[(size_t)k].cp = e->colptr.empty() ? 0u : (uint32_t)e->colptr[(size_t)k];
            ccv[(size_t)k].k = e->colptr.empty() ? 0u : (uint32_t)(e->colptr[(size_t)k + 1] - e->colptr[(size_t)k]);
            for (int q = 0; q < 5; ++q)
                ccv[(size_t)k].gam[q] = ((uint32_t)q < ccv[(size_t)k].k && ccv[(size_t)k].k <= 5u && !e->h_tval.empty()) ? e->h_tval[ccv[(size_t)k].cp + (size_t)q] : 0.0;
        }
        PDMP_TRY(e->d_cc.upload(ccv));
    }
    if (general_path(e)) {
        if (e->cfg.sampler != PDMP_SAMPLER_ZIGZAG_LOCAL && e->cfg.sampler != PDMP_SAMPLER_ZIGZAG_ALL &&
            e->cfg.sampler != PDMP_SAMPLER_STICKY_ZIGZAG)
            return fail(PDMP_ERR_UNSUPPORTED,
                        "neighbourhoods beyond 64 members / the logistic target / FactBoomerang / adaptscale run on the general "
                        "kernel: spdmp, pdmp and sspdmp only");
        if (sticky && (e->flow_kind == 1 || e->adaptscale || e->local_bound))
            return fail(PDMP_ERR_UNSUPPORTED, "sspdmp on the general kernel: ZigZag flow, Gaussian or logistic target");
        if (e->cfg.sampler == PDMP_SAMPLER_ZIGZAG_ALL && e->target_kind == 1)
            return fail(PDMP_ERR_UNSUPPORTED, "the logistic target moves what it reads (SelfMoving): use PDMP_SAMPLER_ZIGZAG_LOCAL");
        if (e->target_kind == 1 && (e->flow_kind == 1 || e->lambda_ref > 0))
            return fail(PDMP_ERR_UNSUPPORTED, "the logistic target is implemented for ZigZag without refresh");
        if (pdmp::zz_general_lds_bytes(e->nblk_pad, (e->mmax_all + 63u) & ~63u, e->flow_kind == 1) > 160 * 1024)
            return fail(PDMP_ERR_UNSUPPORTED, "LDS budget exceeded by the general kernel");
        if (e->local_bound) {
            if (e->cfg.sampler != PDMP_SAMPLER_ZIGZAG_LOCAL || e->flow_kind != 0 || e->lambda_ref > 0 || e->target_kind != 0)
                return fail(PDMP_ERR_UNSUPPORTED,
                            "LocalBound (src/local.jl) is implemented for spdmp with a ZigZag flow without refresh and the Gaussian target");
            // src/local.jl:95,107-108 knows one graph: with an argument G it re-bounds ALL of G[i] and takes G2 from G's two-hop sets, while the
            // tables of pdmp_ensemble_set_neighbourhood re-bound G1[i] = the pattern of F.Γ only.  Give the flow's Γ the pattern of G instead.
            if (e->has_g1mask)
                return fail(PDMP_ERR_UNSUPPORTED,
                            "LocalBound with pdmp_ensemble_set_neighbourhood: src/local.jl re-bounds all of G[i]; pass a flow matrix with G's pattern");
            // the target's Γ values in the (member j of G1[i], entry of column j) layout of the re-bound tables
            std::vector<double> qtval;
            qtval.reserve(e->h_qptr.empty() ? 0 : e->h_qptr.back());
            for (int64_t pp = 0; pp < e->nnz; ++pp) {
                const uint32_t j = e->rowval[pp];
                for (uint32_t q = e->colptr[j]; q < e->colptr[j + 1]; ++q) qtval.push_back(e->h_tval[q]);
            }
            if (qtval.empty()) qtval.push_back(0.0);
            PDMP_TRY(e->d_qtval.upload(qtval));
        }
        if (e->adaptscale) {
            if (e->target_kind == 1) return fail(PDMP_ERR_UNSUPPORTED, "adaptscale needs the refresh clock; the logistic target has none");
            std::vector<double> sg((size_t)(n * d));
            for (int64_t k = 0; k < n; ++k) std::copy(e->sigma.begin(), e->sigma.end(), sg.begin() + (size_t)(k * d));
            PDMP_TRY(e->d_sig_chain.upload(sg));
        }
        e->use_spec = false;
    } else if (e->target_kind == TARGET_BRIDGE || e->target_kind == TARGET_PRECISION) {
        e->use_spec = false;  // (no neighbourhood program: zz_bridge_run_kernel / zz_precision_run_kernel compute what they read from i)
    } else {
        PDMP_TRY(build_blob(e, c));
    }
    DevBuf<double> sx, sth;
    DevBuf<uint64_t> sseed;
    if (x0) {
        PDMP_TRY(sx.alloc((size_t)(n * d)));
        PDMP_TRY(sth.alloc((size_t)(n * d)));
        HIP_TRY(hipMemcpy(sx.p, x0, (size_t)(n * d) * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(sth.p, th0, (size_t)(n * d) * sizeof(double), hipMemcpyHostToDevice));
    }
    if (seeds) {
        PDMP_TRY(sseed.alloc((size_t)n));
        HIP_TRY(hipMemcpy(sseed.p, seeds, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    pdmp::ZzInitParams P{};
    P.tb = e->tables();
    P.rec = e->d_rec.p;
    P.keys = e->d_keys.p;
    P.hdr = e->d_hdr.p;
    P.c_chain = e->cfg.adapt ? e->d_c_chain.p : nullptr;
    P.x0 = x0 ? sx.p : nullptr;
    P.th0 = x0 ? sth.p : nullptr;
    P.seeds = seeds ? sseed.p : nullptr;
    P.seed0 = seed0;
    P.d = d;
    P.dk = e->dk;
    P.nchains = n;
    P.t0 = t0;
    P.lambda_ref = e->lambda_ref;
    P.has_refresh = e->lambda_ref > 0;
    P.flow_kind = e->flow_kind;
    P.mu = e->d_mu.p;
    P.diag = e->d_diag.p;
    P.sticky = sticky ? 1 : 0;
    P.local_bound = e->local_bound ? 1 : 0;
    P.g1_member = e->has_g1mask ? reinterpret_cast<const uint4*>(e->d_member.p) : nullptr;
    e->track_generic = false;
    bool trackp_ok = false;
    if (e->track) {
        // which tracked kernel will run is decided HERE (the pair layout belongs to one of them): pdmp_debug_set_track_groups before set_state.
        // One proposal per lane (pdmp_trackp.hip) on the plain lattice, or on any other symmetric graph with |G1| <= 8 (ids and values tabulated).
        uint32_t kmax_g1 = 0;
        for (int64_t k = 0; k < d; ++k) kmax_g1 = std::max(kmax_g1, e->colptr[(size_t)k + 1] - e->colptr[(size_t)k]);
        if (e->lattice_n == 0 && kmax_g1 <= (uint32_t)pdmp::TRACKP_KMAX && d <= 16384 && e->dbg_track_groups == 0) {
            std::vector<uint16_t> nb((size_t)d * 8, (uint16_t)0xFFFF);
            std::vector<double> g8((size_t)d * 8, 0.0);
            for (int64_t k = 0; k < d; ++k)
                for (uint32_t q = e->colptr[(size_t)k]; q < e->colptr[(size_t)k + 1]; ++q) {
                    nb[(size_t)k * 8 + (q - e->colptr[(size_t)k])] = (uint16_t)e->rowval[q];
                    g8[(size_t)k * 8 + (q - e->colptr[(size_t)k])] = e->h_tval[q];
                }
            PDMP_TRY(e->d_nb16.upload(nb));
            PDMP_TRY(e->d_gam8.upload(g8));
            e->track_generic = true;
        }
        // the means (round 6): the one-proposal-per-lane kernel keeps ONE constant Γ[:,i]·μ per coordinate -- the flow's, which enters every bound
        // (src/fact_samplers.jl:51); a target mean is served where its Γμ is the same numbers (the usual Z = ZigZag(Γ, μ) on ∇ϕ = Γ(x − μ))
        {
            bool flow_mean = false;
            for (double v : e->h_gmu_b) flow_mean = flow_mean || v != 0.0;
            e->track_mean = flow_mean ? 1 : 0;
            if (e->has_tmu) {
                const bool same = e->h_gmu_t.size() == e->h_gmu_b.size() && std::equal(e->h_gmu_t.begin(), e->h_gmu_t.end(), e->h_gmu_b.begin());
                if (same && !e->track_two_sums) e->track_mean = 2;
            }
        }
        pdmp::ZzRunParams G = track_query_params(e);
        trackp_ok = pdmp::zz_trackp_supported(G) && e->dbg_track_groups == 0;
        if (!trackp_ok) e->track_generic = false;
        G.blob_sw = e->blob_sw;
        G.blob_pw = e->blob_pw;
        G.blob_kmax = e->blob_kmax;
        G.blob_w_pad = e->blob_w_pad;
        G.has_refresh = 0;
        if (!trackp_ok && (!e->use_spec || !pdmp::zz_spec8_geometry(G))) {
            e->track = false;
            return fail(PDMP_ERR_UNSUPPORTED,
                        "gradient tracking: without adaptation, target mean or a bounding matrix of its own (one proposal per lane) the n x n lattice "
                        "with 2048 <= d <= 65536 or a symmetric graph with |G1| <= 8 and 2048 <= d <= 16384; else the 8-event kernel's geometry "
                        "(|G1| <= 5, |S| <= 13, 2048 <= d <= 16384)");
        }
    }
    P.track = e->track ? 1 : 0;
    e->t0_state = t0;
    e->run_T = t0;
    if (sticky || e->local_bound || barrier) {
        if (e->d_thf.n != (size_t)(n * d)) PDMP_TRY(e->d_thf.alloc((size_t)(n * d)));
        P.thf = e->d_thf.p;
    }
    P.barriers = barrier ? e->d_barriers.p : nullptr;
    LAUNCH_TRY("zz_init", pdmp::launch_zz_init(P, e->stream));
    if (e->track_lg) {
        if (e->d_trk.n != (size_t)(n * d * 4)) PDMP_TRY(e->d_trk.alloc((size_t)(n * d * 4)));
        LAUNCH_TRY("zz_logistic_track_init", pdmp::launch_zz_logistic_track_init(e->d_rec.p, e->tables(), d, n, t0, e->d_trk.p, e->stream));
    }
    e->track_pairs = false;
    e->track_lines = false;
    e->canon_stale = false;
    discard_async_consumer(e);  // (a consumer deferred behind "the next run" belongs to the state that is being replaced)
    if (e->track) {
        if (trackp_ok) {
            if (e->d_kp.n != (size_t)(2 * n * e->dk)) PDMP_TRY(e->d_kp.alloc((size_t)(2 * n * e->dk), &e->place_cfg, &e->place_cfg.kp));
            LAUNCH_TRY("keys_to_pairs", pdmp::launch_zz_keys_to_pairs(e->d_keys.p, e->d_kp.p, n * e->dk, t0, e->stream));
            LAUNCH_TRY("trackp_consts", pdmp::launch_zz_trackp_consts(e->d_rec.p, e->d_cc.p, e->track_generic ? e->d_nb16.p : nullptr, e->track_mean ? e->d_gmu_b.p : nullptr, d, n, e->stream));
            e->track_pairs = true;
            // the line layout where the ensemble fills the device (decided here: the layout belongs to the kernel)
            // (measured, round 6: 2.7 instead of 3.2 lines read per proposal, but 72 instead of 54 vector instructions -- 47.9 ms against 45.4 / 38.8 ms
            // for pdmp_trackp.hip's form on boxes in the slow / fast timing mode: the layout is kept as an opt-in form, never chosen by width)
            if (pdmp::zz_trackl_supported(track_query_params(e)) && !e->track_generic && e->track_mean == 0 && e->dbg_track_lines == 1) {
                if (e->d_tl_lines.n != (size_t)(n * e->dk / 2)) PDMP_TRY(e->d_tl_lines.alloc((size_t)(n * e->dk / 2)));
                if (e->d_tl_cold.n != (size_t)(n * e->dk)) PDMP_TRY(e->d_tl_cold.alloc((size_t)(n * e->dk)));
                LAUNCH_TRY("trackl_pack", pdmp::launch_zz_trackl_pack(e->d_rec.p, e->d_kp.p, e->d_tl_lines.p, e->d_tl_cold.p, d, e->dk, n, e->stream));
                e->track_lines = true;
            }
        }
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->has_state = true;
    e->ran = false;
    e->timed = false;
    e->consuming = false;
    e->cn_on = false;
    e->pr_on = false;
    e->hs_on = false;
    e->trace_appended = false;
    return PDMP_OK;
}

extern "C" {

pdmp_status pdmp_ensemble_set_flow_zigzag(pdmp_ensemble* e, const int64_t* colptr, const int64_t* rowval,
                                          const double* nzval, const double* mu, const double* sigma,
                                          double lambda_ref, double rho) {
    return set_flow_common(e, colptr, rowval, nzval, mu, sigma, lambda_ref, rho, 0);
}

pdmp_status pdmp_ensemble_set_flow_factboomerang(pdmp_ensemble* e, const int64_t* colptr, const int64_t* rowval,
                                                 const double* nzval, const double* mu, const double* sigma,
                                                 double lambda_ref, double rho) {
    if (e && e->cfg.sampler != PDMP_SAMPLER_ZIGZAG_LOCAL && e->cfg.sampler != PDMP_SAMPLER_ZIGZAG_ALL)
        return fail(PDMP_ERR_UNSUPPORTED, "FactBoomerang is available for the factorised drivers spdmp / pdmp (PDMP_SAMPLER_ZIGZAG_LOCAL / _ALL)");
    if (!(lambda_ref > 0)) return fail(PDMP_ERR_INVALID, "FactBoomerang needs a strictly positive refreshment rate");
    return set_flow_common(e, colptr, rowval, nzval, mu, sigma, lambda_ref, rho, 1);
}

pdmp_status pdmp_ensemble_set_neighbourhood(pdmp_ensemble* e, const int64_t* g_colptr, const int64_t* g_rowval) {
    if (!e || !g_colptr || !g_rowval) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    if (!e->has_flow) return fail(PDMP_ERR_INVALID, "set_flow_zigzag / set_flow_factboomerang first");
    if (e->has_g1mask) return fail(PDMP_ERR_INVALID, "the neighbourhood was set already: call set_flow_* again first");
    if (e->cfg.sampler == PDMP_SAMPLER_ZIGZAG_ALL) return fail(PDMP_ERR_INVALID, "pdmp is spdmp with G = All(): it takes no G");
    const int64_t d = e->cfg.d;
    PDMP_TRY(check_csc("neighbourhood G", g_colptr, g_rowval, d, d));
    const int64_t gn = g_colptr[d];
    if (gn < e->nnz || gn >= (int64_t)1 << 31) return fail(PDMP_ERR_INVALID, "G must contain G1 (src/sfact.jl:177)");
    std::vector<double> nz((size_t)gn, 0.0);
    std::vector<uint8_t> mask((size_t)gn, 0);
    for (int64_t i = 0; i < d; ++i) {
        uint32_t q = e->colptr[i];
        const uint32_t q1 = e->colptr[i + 1];
        for (int64_t p = g_colptr[i]; p < g_colptr[i + 1]; ++p) {
            const int64_t r = g_rowval[p];
            if (q < q1 && (int64_t)e->rowval[q] == r) {
                nz[(size_t)p] = e->bval[q];
                mask[(size_t)p] = 1;
                ++q;
            }
        }
        if (q != q1)  // @assert all(a.second ⊇ b.second for (a, b) in zip(G, G1)), src/sfact.jl:177
            return fail(PDMP_ERR_INVALID, "G[%lld] does not contain G1[%lld] = rowvals(F.Γ)[nzrange(F.Γ, %lld)] (src/sfact.jl:177)", (long long)i,
                        (long long)i, (long long)i);
    }
    if (gn == e->nnz) return PDMP_OK;  // G == G1: Matched()
    const std::vector<double> mu = e->mu, sigma = e->sigma;
    return set_flow_common(e, g_colptr, g_rowval, nz.data(), mu.data(), sigma.data(), e->lambda_ref, e->rho, e->flow_kind, mask.data());
}

pdmp_status pdmp_ensemble_set_target_gaussian_csc(pdmp_ensemble* e, const int64_t* colptr, const int64_t* rowval,
                                                  const double* nzval, const double* mu) {
    if (!e || !colptr || !rowval || !nzval) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler == PDMP_SAMPLER_BPS) {
        // pdmp(∇ϕ!, t0, x0, θ0, T, c, B::BouncyParticle): ∇ϕ! is the caller's (src/not_fact_samplers.jl:122), ab(…GlobalBound…) uses B.Γ, B.μ
        // (:26-28).  A Gaussian target of its own: ∇ϕ!(y, x) = Γt(x − μt).
        if (!e->has_flow || e->bps.flow_kind != 0)
            return fail(PDMP_ERR_INVALID, "a target of its own follows set_flow_bps (set_flow_boomerang takes the target directly)");
        HIP_TRY(hipSetDevice(e->cfg.device));
        const int64_t dd = e->cfg.d;
        PDMP_TRY(check_csc("target matrix", colptr, rowval, dd, dd));
        const int64_t tn = colptr[dd];
        if (tn <= 0 || tn >= (int64_t)1 << 31) return fail(PDMP_ERR_INVALID, "bad nnz %lld", (long long)tn);
        PDMP_TRY(e->bt_colptr.upload(std::vector<int64_t>(colptr, colptr + dd + 1)));
        PDMP_TRY(e->bt_rowval.upload(std::vector<int64_t>(rowval, rowval + tn)));
        PDMP_TRY(e->bt_nzval.upload(std::vector<double>(nzval, nzval + tn)));
        std::vector<double> tm((size_t)dd, 0.0);
        if (mu) tm.assign(mu, mu + dd);
        PDMP_TRY(e->bt_mu.upload(tm));
        e->bps.own_target = true;
        e->bps.logit = false;  // (the later of the two target calls wins)
        e->has_state = false;
        return PDMP_OK;
    }
    NEED_FACTORISED(e);
    if (!e->has_flow) return fail(PDMP_ERR_INVALID, "set_flow_zigzag must be called first");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int64_t d = e->cfg.d;
    PDMP_TRY(check_csc("target matrix", colptr, rowval, d, d));
    // align Γt to the flow's pattern: slots absent from Γt carry 0.0 (s + 0.0*x == s bit-for-bit)
    std::vector<double> tval(e->nnz, 0.0), gmu_t(d, 0.0);
    for (int64_t i = 0; i < d; ++i) {
        uint32_t q = e->colptr[i];
        const uint32_t q1 = e->colptr[i + 1];
        double s = 0.0;
        for (int64_t p = colptr[i]; p < colptr[i + 1]; ++p) {
            const int64_t r = rowval[p];
            while (q < q1 && (int64_t)e->rowval[q] < r) ++q;
            if (q == q1 || (int64_t)e->rowval[q] != r)
                return fail(PDMP_ERR_UNSUPPORTED,
                            "target Γt[%lld,%lld] lies outside the flow's pattern G[%lld] (src/sfact.jl:116)",
                            (long long)r, (long long)i, (long long)i);
            tval[q] = nzval[p];
            if (mu) s += nzval[p] * mu[r];
        }
        gmu_t[i] = s;
    }
    e->has_tmu = (mu != nullptr);
    e->h_gmu_t = gmu_t;
    e->target_kind = 0;
    e->h_tval = tval;
    PDMP_TRY(e->d_tval.upload(tval));
    PDMP_TRY(e->d_gmu_t.upload(gmu_t));
    e->has_target = true;
    e->has_state = false;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_target_logistic(pdmp_ensemble* e, int64_t n, const int64_t* A_colptr,
                                                         const int64_t* A_rowval, const double* A_nzval,
                                                         const int64_t* At_colptr, const int64_t* At_rowval,
                                                         const double* At_nzval, const double* y, const double* ny,
                                                         const double* mu, double gamma0, int64_t k_sub) {
    if (!e || !A_colptr || !A_rowval || !A_nzval || !At_colptr || !At_rowval || !At_nzval || !y || !ny || !mu)
        return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    if (!e->has_flow) return fail(PDMP_ERR_INVALID, "set_flow_zigzag must be called first");
    if (n <= 0 || k_sub <= 0) return fail(PDMP_ERR_INVALID, "n and k_sub must be positive");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int64_t p = e->cfg.d;
    const int64_t nnzA = A_colptr[p], nnzAt = At_colptr[n];
    if (A_colptr[0] != 0 || At_colptr[0] != 0 || nnzA != nnzAt) return fail(PDMP_ERR_INVALID, "A / At are inconsistent");
    for (int64_t j = 0; j < p; ++j)
        if (A_colptr[j + 1] <= A_colptr[j])
            return fail(PDMP_ERR_UNSUPPORTED, "coordinate %lld has no observation (rand over an empty range)", (long long)j);
    // control-variate terms sigmoidn(u0), nsigmoid(u0) with u0 = idot(At, row, μ) (src/common.jl:16-24 order): constants of
    // the observation, evaluated here with the SAME deterministic exp the kernels use (bit-identical on x86-64 and gfx950)
    std::vector<double> sn0((size_t)n, 0.0), ns0((size_t)n, 0.0);
    for (int64_t r = 0; r < n; ++r) {
        double s = 0.0;
        for (int64_t q = At_colptr[r]; q < At_colptr[r + 1]; ++q) {
            if (At_rowval[q] < 0 || At_rowval[q] >= p) return fail(PDMP_ERR_INVALID, "At row index out of range");
            s += At_nzval[q] * mu[At_rowval[q]];
        }
        sn0[r] = 1.0 / (1.0 + pdmp_exp(s));     // sigmoidn(u0) = sigmoid(-u0) = inv(1 + exp(u0))
        ns0[r] = -(1.0 / (1.0 + pdmp_exp(-s)));  // nsigmoid(u0) = -sigmoid(u0)
    }
    PDMP_TRY(e->lg_Acp.upload(std::vector<int64_t>(A_colptr, A_colptr + p + 1)));
    PDMP_TRY(e->lg_Arv.upload(std::vector<int64_t>(A_rowval, A_rowval + nnzA)));
    PDMP_TRY(e->lg_Anz.upload(std::vector<double>(A_nzval, A_nzval + nnzA)));
    PDMP_TRY(e->lg_Atcp.upload(std::vector<int64_t>(At_colptr, At_colptr + n + 1)));
    PDMP_TRY(e->lg_Atrv.upload(std::vector<int64_t>(At_rowval, At_rowval + nnzAt)));
    {
        std::vector<uint32_t> r32((size_t)nnzAt);
        for (int64_t q = 0; q < nnzAt; ++q) r32[(size_t)q] = (uint32_t)At_rowval[q];
        PDMP_TRY(e->lg_Atrv32.upload(r32));
    }
    PDMP_TRY(e->lg_Atnz.upload(std::vector<double>(At_nzval, At_nzval + nnzAt)));
    PDMP_TRY(e->lg_y.upload(std::vector<double>(y, y + n)));
    PDMP_TRY(e->lg_ny.upload(std::vector<double>(ny, ny + n)));
    PDMP_TRY(e->lg_u0.upload(sn0));
    PDMP_TRY(e->lg_ns0.upload(ns0));
    // the kernels' table struct wants tval / gmu_t allocated even if unused
    PDMP_TRY(e->d_tval.upload(std::vector<double>((size_t)e->nnz, 0.0)));
    PDMP_TRY(e->d_gmu_t.upload(std::vector<double>((size_t)p, 0.0)));
    e->has_tmu = false;
    e->lg_gamma0 = gamma0;
    e->lg_k = k_sub;
    e->lg_nemax = 0;
    for (int64_t r = 0; r < n; ++r) e->lg_nemax = std::max<int64_t>(e->lg_nemax, At_colptr[r + 1] - At_colptr[r]);
    // packed tables of the LDS-resident kernel (pdmp_logistic.hip): observations with at most 6 regressors, d and nnz(A) within 16 / 32 bits
    e->lg_coord.release();
    e->lg_obs.release();
    e->lg_arow.release();
    if (e->lg_nemax <= 6 && p < 65536 && nnzA < ((int64_t)1 << 32) && n < ((int64_t)1 << 32)) {
        std::vector<pdmp::LgCoord> hc((size_t)p);
        for (int64_t j = 0; j < p; ++j) {
            pdmp::LgCoord& c = hc[(size_t)j];
            c.cp0 = e->colptr[(size_t)j];
            c.k = e->colptr[(size_t)j + 1] - c.cp0;
            c.sp0 = e->h_sptr[(size_t)j];
            c.m = e->h_sptr[(size_t)j + 1] - c.sp0;
            c.l = (uint32_t)(A_colptr[j + 1] - A_colptr[j]);
            c.r0 = (uint32_t)A_colptr[j];
            c.lk = (double)c.l / (double)(uint32_t)k_sub;
        }
        std::vector<pdmp::LgObs> ho((size_t)n);
        memset(ho.data(), 0, ho.size() * sizeof(pdmp::LgObs));
        for (int64_t r = 0; r < n; ++r) {
            pdmp::LgObs& o = ho[(size_t)r];
            o.y = y[r];
            o.ny = ny[r];
            o.sn0 = sn0[(size_t)r];
            o.ns0 = ns0[(size_t)r];
            o.ne = (uint16_t)(At_colptr[r + 1] - At_colptr[r]);
            for (int64_t q = At_colptr[r]; q < At_colptr[r + 1]; ++q) {
                o.val[q - At_colptr[r]] = At_nzval[q];
                o.idx[q - At_colptr[r]] = (uint16_t)At_rowval[q];
            }
        }
        std::vector<uint32_t> ar((size_t)nnzA);
        for (int64_t q = 0; q < nnzA; ++q) {
            if (A_rowval[q] < 0 || A_rowval[q] >= n) return fail(PDMP_ERR_INVALID, "A row index out of range");
            ar[(size_t)q] = (uint32_t)A_rowval[q];
        }
        PDMP_TRY(e->lg_coord.upload(hc));
        PDMP_TRY(e->lg_obs.upload(ho));
        PDMP_TRY(e->lg_arow.upload(ar));
    }
    e->target_kind = 1;
    e->has_target = true;
    e->has_state = false;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_target_diffusion_bridge(pdmp_ensemble* e, int32_t L, double T, double alpha, double beta, double omega) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_ZIGZAG_LOCAL)
        return fail(PDMP_ERR_INVALID, "%s: the diffusion-bridge target belongs to spdmp (PDMP_SAMPLER_ZIGZAG_LOCAL)", __func__);
    if (!e->has_flow) return fail(PDMP_ERR_INVALID, "set_flow_zigzag must be called first");
    if (e->has_state) return fail(PDMP_ERR_INVALID, "a state exists already: the target is set before pdmp_ensemble_set_state (set the flow again to start over)");
    if (L < 0) return fail(PDMP_ERR_INVALID, "diffusion bridge: L = %d < 0", (int)L);
    if (!(T > 0) || !std::isfinite(T)) return fail(PDMP_ERR_INVALID, "diffusion bridge: T = %g must be positive and finite", T);
    if (!std::isfinite(alpha) || !std::isfinite(beta) || !std::isfinite(omega))
        return fail(PDMP_ERR_INVALID, "diffusion bridge: alpha = %g, beta = %g, omega = %g must be finite", alpha, beta, omega);
    if (L > 40 || e->cfg.d != ((int64_t)2 << L) + 1)
        return fail(PDMP_ERR_INVALID, "diffusion bridge: d = %lld is not (2 << L) + 1 for L = %d", (long long)e->cfg.d, (int)L);
    if (L > pdmp::PDMP_BRIDGE_LMAX)
        return fail(PDMP_ERR_UNSUPPORTED, "diffusion bridge: L = %d > %d (one level per lane and one block of 64 keys per lane: d <= 2049)", (int)L,
                    pdmp::PDMP_BRIDGE_LMAX);
    HIP_TRY(hipSetDevice(e->cfg.device));
    // the kernels' table struct wants tval / gmu_t allocated even if unused
    e->h_tval.assign((size_t)e->nnz, 0.0);
    PDMP_TRY(e->d_tval.upload(e->h_tval));
    PDMP_TRY(e->d_gmu_t.upload(std::vector<double>((size_t)e->cfg.d, 0.0)));
    e->has_tmu = false;
    e->bridge.L = L;
    e->bridge.pad_ = 0;
    e->bridge.T = T;
    e->bridge.alpha = alpha;
    e->bridge.beta = beta;
    e->bridge.omega = omega;
    e->target_kind = TARGET_BRIDGE;  // (the later of two target calls wins: the Gaussian and the logistic setters put their own kind back)
    e->has_target = true;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_target_precision_cholesky(pdmp_ensemble* e, int32_t n, const double* YY, double N, double gamma0) {
    if (!e || !YY) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_STICKY_ZIGZAG)
        return fail(PDMP_ERR_INVALID, "%s: the precision-cholesky target belongs to sspdmp (PDMP_SAMPLER_STICKY_ZIGZAG)", __func__);
    if (!e->has_flow) return fail(PDMP_ERR_INVALID, "set_flow_zigzag must be called first");
    if (e->has_state) return fail(PDMP_ERR_INVALID, "a state exists already: the target is set before pdmp_ensemble_set_state (set the flow again to start over)");
    if (n < 1) return fail(PDMP_ERR_INVALID, "precision cholesky: n = %d < 1", (int)n);
    if (e->cfg.d != (int64_t)n * ((int64_t)n + 1) / 2)
        return fail(PDMP_ERR_INVALID, "precision cholesky: d = %lld is not n (n + 1)/2 for n = %d", (long long)e->cfg.d, (int)n);
    if (!(N > 0) || !std::isfinite(N)) return fail(PDMP_ERR_INVALID, "precision cholesky: N = %g must be positive and finite", N);
    if (!(gamma0 >= 0) || !std::isfinite(gamma0)) return fail(PDMP_ERR_INVALID, "precision cholesky: gamma0 = %g must be finite and not negative", gamma0);
    if (n > pdmp::PDMP_PRECISION_NMAX)
        return fail(PDMP_ERR_UNSUPPORTED, "precision cholesky: n = %d > %d (one column member per lane and one block of 64 keys per lane: d <= 2080)", (int)n,
                    pdmp::PDMP_PRECISION_NMAX);
    for (int64_t r = 0; r < n; ++r)
        for (int64_t q = 0; q <= r; ++q) {
            const double v = YY[r * n + q], w = YY[q * n + r];
            if (!std::isfinite(v) || !std::isfinite(w)) return fail(PDMP_ERR_INVALID, "precision cholesky: YY[%lld, %lld] is not finite", (long long)r, (long long)q);
            if (std::memcmp(&v, &w, sizeof v) != 0)
                return fail(PDMP_ERR_INVALID, "precision cholesky: YY is not symmetric bit for bit (YY[%lld, %lld] = %.17g, YY[%lld, %lld] = %.17g)", (long long)r,
                            (long long)q, v, (long long)q, (long long)r, w);
        }
    HIP_TRY(hipSetDevice(e->cfg.device));
    // the kernels' table struct wants tval / gmu_t allocated even if unused
    e->h_tval.assign((size_t)e->nnz, 0.0);
    PDMP_TRY(e->d_tval.upload(e->h_tval));
    PDMP_TRY(e->d_gmu_t.upload(std::vector<double>((size_t)e->cfg.d, 0.0)));
    e->has_tmu = false;
    PDMP_TRY(e->d_prec_yy.upload(std::vector<double>(YY, YY + (size_t)n * (size_t)n)));
    e->precision.n = n;
    e->precision.pad_ = 0;
    e->precision.N = N;
    e->precision.gamma0 = gamma0;
    e->precision.YY = e->d_prec_yy.p;
    e->target_kind = TARGET_PRECISION;  // (the later of two target calls wins: the Gaussian and the logistic setters put their own kind back)
    e->has_target = true;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_state(pdmp_ensemble* e, double t0, const double* x0, const double* theta0,
                                    const double* c, const uint64_t* seeds) {
    if (!e || !x0 || !theta0 || !seeds) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    return init_state_tuned(e, t0, x0, theta0, c, seeds, 0);
}

pdmp_status pdmp_ensemble_set_state_synthetic(pdmp_ensemble* e, double t0, const double* c, uint64_t seed0) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    return init_state_tuned(e, t0, nullptr, nullptr, c, nullptr, seed0);
}

pdmp_status pdmp_ensemble_set_sticky(pdmp_ensemble* e, const double* kappa, int reversible, int strong_upperbounds) {
    if (!e || !kappa) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_STICKY_ZIGZAG) return fail(PDMP_ERR_INVALID, "ensemble is not a sticky ZigZag");
    if (!e->has_flow) return fail(PDMP_ERR_INVALID, "set_flow_zigzag must be called first");
    if (e->lambda_ref > 0) return fail(PDMP_ERR_UNSUPPORTED, "refreshment not implemented (src/ss_fact.jl:86)");
    HIP_TRY(hipSetDevice(e->cfg.device));
    PDMP_TRY(e->d_kappa.upload(std::vector<double>(kappa, kappa + e->cfg.d)));
    e->reversible = reversible;
    e->strong_upperbounds = strong_upperbounds;
    e->has_kappa = true;
    e->has_state = false;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_barriers(pdmp_ensemble* e, const double* lo, const double* hi, const int32_t* rule_lo, const int32_t* rule_hi,
                                       const double* kappa_lo, const double* kappa_hi, int strong_upperbounds) {
    if (!e || !lo || !hi || !rule_lo || !rule_hi || !kappa_lo || !kappa_hi) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BARRIER_ZIGZAG) return fail(PDMP_ERR_INVALID, "ensemble is not a barrier ZigZag (PDMP_SAMPLER_BARRIER_ZIGZAG)");
    if (!e->has_flow) return fail(PDMP_ERR_INVALID, "set_flow_zigzag must be called first");
    const int64_t d = e->cfg.d;
    std::vector<pdmp::BarrierEntry> tab((size_t)d);
    for (int64_t i = 0; i < d; ++i) {
        if (!(lo[i] <= hi[i])) return fail(PDMP_ERR_INVALID, "barriers of coordinate %lld: lo = %g > hi = %g (or NaN)", (long long)i, lo[i], hi[i]);
        if (!(kappa_lo[i] > 0) || !(kappa_hi[i] > 0))
            return fail(PDMP_ERR_INVALID, "barriers of coordinate %lld: κ = (%g, %g) must be positive (+Inf: a wall)", (long long)i, kappa_lo[i], kappa_hi[i]);
        if (rule_lo[i] < 0 || rule_lo[i] > 2 || rule_hi[i] < 0 || rule_hi[i] > 2)
            return fail(PDMP_ERR_INVALID, "barriers of coordinate %lld: rules (%d, %d) must be PDMP_BARRIER_STICKY / _REFLECT / _REVERSIBLE", (long long)i, rule_lo[i], rule_hi[i]);
        pdmp::BarrierEntry& be = tab[(size_t)i];
        be.lo = lo[i];
        be.hi = hi[i];
        be.klo = kappa_lo[i];
        be.khi = kappa_hi[i];
        be.rules = (uint32_t)rule_lo[i] | ((uint32_t)rule_hi[i] << 8);
        be.pad = 0;
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    PDMP_TRY(e->d_barriers.upload(tab));
    e->h_barriers.swap(tab);
    e->strong_upperbounds = strong_upperbounds;
    e->has_barriers = true;
    e->has_state = false;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_final_barrier(pdmp_ensemble* e, int64_t chain_first, int64_t n, uint8_t* frozen, double* theta_saved) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_BARRIER_ZIGZAG) return fail(PDMP_ERR_INVALID, "ensemble is not a barrier ZigZag (PDMP_SAMPLER_BARRIER_ZIGZAG)");
    if (!e->has_state) return fail(PDMP_ERR_INVALID, "no state");
    PDMP_TRY(check_chain_range(e, chain_first, n));
    if (n == 0) return PDMP_OK;
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t d = e->cfg.d;
    std::vector<double> vold((size_t)(n * d));
    HIP_TRY(hipMemcpy(vold.data(), e->d_thf.p + chain_first * d, vold.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (frozen) {  // v[i] == 0 && v_old[i] != 0, src/stickyzz.jl:266
        std::vector<double> th((size_t)(n * d));
        PDMP_TRY(pdmp_ensemble_final_state(e, chain_first, n, nullptr, nullptr, th.data(), nullptr, nullptr));
        for (size_t q = 0; q < th.size(); ++q) frozen[q] = (th[q] == 0.0 && vold[q] != 0.0) ? 1 : 0;
    }
    if (theta_saved) std::copy(vold.begin(), vold.end(), theta_saved);
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_final_sticky(pdmp_ensemble* e, int64_t chain_first, int64_t n, uint8_t* frozen, double* theta_saved) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (e->cfg.sampler != PDMP_SAMPLER_STICKY_ZIGZAG) return fail(PDMP_ERR_INVALID, "ensemble is not a sticky ZigZag (PDMP_SAMPLER_STICKY_ZIGZAG)");
    if (!e->has_state) return fail(PDMP_ERR_INVALID, "no state");
    PDMP_TRY(check_chain_range(e, chain_first, n));
    if (n == 0) return PDMP_OK;
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(device_sync(e));
    const int64_t d = e->cfg.d;
    if (frozen) {  // x[i] == 0 && θ[i] == 0, src/ss_fact.jl:108
        std::vector<double> x((size_t)(n * d)), th((size_t)(n * d));
        PDMP_TRY(pdmp_ensemble_final_state(e, chain_first, n, nullptr, x.data(), th.data(), nullptr, nullptr));
        for (size_t q = 0; q < th.size(); ++q) frozen[q] = (x[q] == 0.0 && th[q] == 0.0) ? 1 : 0;
    }
    if (theta_saved) HIP_TRY(hipMemcpy(theta_saved, e->d_thf.p + chain_first * d, (size_t)(n * d) * sizeof(double), hipMemcpyDeviceToHost));
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_gradient_tracking(pdmp_ensemble* e, int enable) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    e->track_requested = enable != 0;
    e->has_state = false;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_local_bound(pdmp_ensemble* e, int enable) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    if (!e->has_flow) return fail(PDMP_ERR_INVALID, "set_flow_* must be called first");
    e->local_bound = enable != 0;
    e->has_state = false;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_set_adaptscale(pdmp_ensemble* e, int enable) {
    if (!e) return fail(PDMP_ERR_INVALID, "null argument");
    if (!e->has_flow) return fail(PDMP_ERR_INVALID, "set_flow_* must be called first");
    if (enable && e->cfg.sampler != PDMP_SAMPLER_ZIGZAG_LOCAL)
        return fail(PDMP_ERR_UNSUPPORTED, "adaptscale is a keyword of spdmp (src/sfact.jl:163): PDMP_SAMPLER_ZIGZAG_LOCAL only");
    if (enable && !(e->lambda_ref > 0))
        return fail(PDMP_ERR_INVALID, "adaptscale acts in the refresh branch (src/sfact.jl:86): lambda_ref must be positive");
    e->adaptscale = enable != 0;
    e->has_state = false;
    return PDMP_OK;
}

pdmp_status pdmp_ensemble_final_sigma(pdmp_ensemble* e, int64_t chain_first, int64_t n, double* sigma) {
    if (!e || !sigma) return fail(PDMP_ERR_INVALID, "null argument");
    NEED_FACTORISED(e);
    if (!e->has_state) return fail(PDMP_ERR_INVALID, "no state");
    const int64_t d = e->cfg.d;
    if (chain_first < 0 || n < 0 || chain_first + n > e->cfg.nchains) return fail(PDMP_ERR_INVALID, "chain range out of bounds");
    HIP_TRY(hipSetDevice(e->cfg.device));
    if (e->adaptscale) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipMemcpy(sigma, e->d_sig_chain.p + chain_first * d, (size_t)(n * d) * sizeof(double), hipMemcpyDeviceToHost));
    } else {
        for (int64_t k = 0; k < n; ++k) std::copy(e->sigma.begin(), e->sigma.end(), sigma + k * d);
    }
    return PDMP_OK;
}

}  // extern "C"
