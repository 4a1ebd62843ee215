/*
 * stickyzz_ref.c -- sequential restatement of the reference's ZigZag with sticky and reflecting barriers,
 *   stickyzz(u0, target::StructuredTarget, flow::StickyFlow, upper_bounds::StickyUpperBounds, barriers, end_condition)
 * (src/stickyzz.jl:119-319) with the proposal times of src/poissontime.jl:39-65,86-92, line by line, for the tests to hold the device loop
 * (csrc/pdmp_barrier.hip) to.  Test infrastructure only: the product never loads it.  It shares include/pdmp_detmath.h with the kernels
 * (Philox draws, log) and restates everything else itself.  Written from reading the Julia; every block cites its lines.
 *
 * What the reference leaves open is fixed the way the engine fixes it everywhere:
 *   draws   the reference's rng calls are, in program order, draws nm = 0, 1, 2, ... of PDMP_STREAM_MAIN; rand((-1,1)) of the :reversible rule
 *           (the GLOBAL generator in the reference, :271) is one more draw of that stream, u < 0.5 -> -1.
 *   queue   an exact minimum over all coordinates, lowest index on ties (the reference's heap pops tied keys in heap-shape order).
 *   target  the Gaussian ∇ϕ(x, i) = idot(Γt, i, x) - idot(Γt, i, μt), the constant subtracted only when a mean is given (the engine's target).
 *   G = G1 = the column patterns of the flow's Γ (StructuredTarget(Γ, ∇ϕ), :68), G2[i] = ∪_{j ∈ G1[i]} G1[j] \ G[i] (:43).
 * Quirks of the reference that are kept: the 0.01 floor is in the proposal time (:91 of poissontime.jl) but NOT in the thinning bound
 * (λ, :129-135); hitting_time is Inf when v (x - barrier) >= 0 ("sic", :122), so a coordinate on its barrier passes through it;
 * accept! counts before the bound check (:293-294); v_old starts as a copy of v0 (:182); the setup loop stops coordinates as it goes, so
 * b[i] sees θ = 0 at the earlier coordinates that started frozen (:198-208); t0 IS added to the first keys (:152,159).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/pdmp_detmath.h"

#define REF_OK 0
#define REF_BOUND_VIOLATED 1 /* error("Tuning parameter `c` too small. ..."), :295 */

#define ACT_HIT 0 /* @enum Action, :170-175 */
#define ACT_REFLECT 1
#define ACT_UNFREEZE 2

#define RULE_STICKY 0
#define RULE_REFLECT 1
#define RULE_REVERSIBLE 2

#define EV_HIT 0
#define EV_THAW 1
#define EV_REFLECTION 2

typedef struct {
    int64_t d;
    int32_t adapt, strong;
    /* the flow's Γ, μ: ab (src/fact_samplers.jl:50-54), G = G1 */
    const int64_t* colptr;
    const int64_t* rowval;
    const double* nzval;
    const double* mu;
    /* the Gaussian target Γt, μt (μt may be NULL) */
    const int64_t* t_colptr;
    const int64_t* t_rowval;
    const double* t_nzval;
    const double* t_mu;
    /* StickyBarriers, :19-25: index 1 = lower, 2 = upper */
    const double* lo;
    const double* hi;
    const double* klo;
    const double* khi;
    const int32_t* rlo;
    const int32_t* rhi;
    double factor;
    uint64_t seed;
} ref_params;

typedef struct {
    int64_t num, nacc, nevents, nhit, nthaw, nrefl, nadapt;
    uint64_t ndraw_main;
    int32_t status, pad_;
    double t;
} ref_result;

/* pos(x) = max(zero(x), x), src/common.jl:8 */
static double pos(double x) { return x > 0 ? x : (x != x ? x : 0.0); }

/* poisson_time((a,b,c)::NTuple{3}, u), src/poissontime.jl:39-65 */
double ref_poisson_time3(double a, double b, double c, double u) {
    const double lu = pdmp_log(u);
    if (b > 0) {
        if (a < 0) {
            if (-c * a / b + lu < 0.0) return sqrt(-2 * b * lu + c * c + 2 * a * c) / b - (a + c) / b; /* :43 */
            return -lu / c;                                                                             /* :45 */
        }
        return sqrt(-lu * 2.0 * b + (a + c) * (a + c)) / b - (a + c) / b; /* :48 */
    } else if (b == 0) {
        if (a > 0) return -lu / (a + c); /* :52 */
        return -lu / c;                  /* :54 */
    }
    if (a <= 0.0) return -lu / c;                                                                                    /* :58 */
    if (-c * a / b - (a * a) / (2 * b) + lu > 0.0) return +sqrt((a + c) * (a + c) - 2.0 * lu * b) / b - (a + c) / b; /* :60 */
    return (-lu + (a * a) / (2 * b)) / c;                                                                            /* :62 */
}

/* poisson_time(t, b::Tuple, r), src/poissontime.jl:86-92, b = (t_bound, a, b, Inf) */
static double poisson_time4(double t, double tb, double a, double b, double u) {
    const double dt = t - tb;     /* :88 */
    const double a2 = a + dt * b; /* :89 */
    return t + ref_poisson_time3(a2, b, 0.01, u); /* :91: guarantee minimum rate */
}

/* hitting_time(barrier, ui, flow), :119-127, with barrier.x[dir(ui)] */
double ref_hitting_time(double x, double v, double bar) {
    if (v * (x - bar) >= 0) return INFINITY; /* sic!, :122 */
    return -(x - bar) / v;                   /* :125 */
}

typedef struct {
    const ref_params* p;
    double *t, *x, *v, *t_old, *v_old, *c;
    double *ba, *bb; /* b[i] = (t[i], a, b, Inf), :138-142: the time is t_old[i] */
    int64_t* action;
    double* Q;
    double* gmu; /* idot(Γ, i, μ) */
    double* gmu_t;
    uint64_t nm;
} ref_state;

/* idot(A, j, x), src/common.jl:16-24 */
static double idot(const int64_t* cp, const int64_t* rv, const double* nz, int64_t j, const double* x) {
    double s = 0.0;
    for (int64_t q = cp[j]; q < cp[j + 1]; ++q) s += nz[q] * x[rv[q]];
    return s;
}

static double draw(ref_state* S) { return pdmp_u01(S->p->seed, PDMP_STREAM_MAIN, S->nm++); }

/* dir(ui), :115 (v != 0 wherever it is called) */
static double barrier_of(const ref_params* p, int64_t i, double v) { return v > 0 ? p->hi[i] : p->lo[i]; }
static double kappa_of(const ref_params* p, int64_t i, double v) { return v > 0 ? p->khi[i] : p->klo[i]; }
static int32_t rule_of(const ref_params* p, int64_t i, double v) { return v > 0 ? p->rhi[i] : p->rlo[i]; }

/* ab(rng, su, flow, target, t′, u, j), :138-142 -> ab(G1, j, x, v, c, Z::ZigZag), src/fact_samplers.jl:50-54 */
static void ab(ref_state* S, int64_t j) {
    const ref_params* p = S->p;
    S->ba[j] = S->c[j] + (idot(p->colptr, p->rowval, p->nzval, j, S->x) - S->gmu[j]) * S->v[j];
    S->bb[j] = S->c[j] / 100 + S->v[j] * idot(p->colptr, p->rowval, p->nzval, j, S->v);
}

/* queue_time!(rng, Q, u, i, b, action, barriers, flow), :144-165 (b[i][1] = t[i]: the bound was just made) */
static void queue_time(ref_state* S, int64_t i) {
    const double trefl = poisson_time4(S->t[i], S->t[i], S->ba[i], S->bb[i], draw(S)) - S->t[i]; /* :147 */
    const double thit = ref_hitting_time(S->x[i], S->v[i], barrier_of(S->p, i, S->v[i]));        /* :148 */
    if (thit <= trefl) { /* :149 */
        S->action[i] = ACT_HIT;
        S->Q[i] = S->t[i] + thit;
    } else {
        S->action[i] = ACT_REFLECT;
        S->Q[i] = S->t[i] + trefl;
    }
}

/* ssmove_forward!(G, i, t, x, θ, t′, Z), src/ss_fact.jl:38-45, over an index list */
static void ssmove(ref_state* S, const int64_t* idx, int64_t n, double tp) {
    for (int64_t q = 0; q < n; ++q) {
        const int64_t j = idx[q];
        if (S->v[j] != 0.0) {
            S->x[j] = S->x[j] + S->v[j] * (tp - S->t[j]);
            S->t[j] = tp;
        }
    }
}

/* b[j] = ab(...); t_old[j] = t[j]; queue_time! for j in neighbours(G1, i) with v[j] != 0, :257-263 = :277-283 = :301-307 */
static void rebound_neighbours(ref_state* S, int64_t i) {
    const ref_params* p = S->p;
    for (int64_t q = p->colptr[i]; q < p->colptr[i + 1]; ++q) {
        const int64_t j = p->rowval[q];
        if (S->v[j] != 0) {
            ab(S, j);
            S->t_old[j] = S->t[j];
            queue_time(S, j);
        }
    }
}

int ref_stickyzz(const ref_params* p, double t0, double T, double* x, double* v, double* t, double* c, double* v_old, int64_t* action,
                 double* ev_t, int64_t* ev_i, double* ev_x, double* ev_th, int8_t* ev_kind, int64_t ev_cap, ref_result* out) {
    const int64_t d = p->d;
    ref_state S;
    memset(&S, 0, sizeof S);
    S.p = p;
    S.t = t;
    S.x = x;
    S.v = v;
    S.c = c;
    S.v_old = v_old;
    S.action = action;
    S.t_old = (double*)malloc((size_t)d * sizeof(double));
    S.ba = (double*)malloc((size_t)d * sizeof(double));
    S.bb = (double*)malloc((size_t)d * sizeof(double));
    S.Q = (double*)malloc((size_t)d * sizeof(double));
    S.gmu = (double*)malloc((size_t)d * sizeof(double));
    S.gmu_t = (double*)malloc((size_t)d * sizeof(double));
    /* G2[i] = setdiff(union(G1[j] for j in G1[i]), G[i]), :43, ascending */
    int64_t* g2ptr = (int64_t*)malloc((size_t)(d + 1) * sizeof(int64_t));
    int64_t* g2idx = NULL;
    uint8_t* mark = (uint8_t*)calloc((size_t)d, 1);
    if (!S.t_old || !S.ba || !S.bb || !S.Q || !S.gmu || !S.gmu_t || !g2ptr || !mark) return 1;
    {
        int64_t cap = 16, n = 0;
        g2idx = (int64_t*)malloc((size_t)cap * sizeof(int64_t));
        if (!g2idx) return 1;
        for (int64_t i = 0; i < d; ++i) {
            g2ptr[i] = n;
            memset(mark, 0, (size_t)d);
            for (int64_t q = p->colptr[i]; q < p->colptr[i + 1]; ++q) {
                const int64_t j = p->rowval[q];
                for (int64_t r = p->colptr[j]; r < p->colptr[j + 1]; ++r) mark[p->rowval[r]] = 1;
            }
            for (int64_t q = p->colptr[i]; q < p->colptr[i + 1]; ++q) mark[p->rowval[q]] = 0;
            for (int64_t j = 0; j < d; ++j)
                if (mark[j]) {
                    if (n == cap) {
                        cap *= 2;
                        g2idx = (int64_t*)realloc(g2idx, (size_t)cap * sizeof(int64_t));
                        if (!g2idx) return 1;
                    }
                    g2idx[n++] = j;
                }
        }
        g2ptr[d] = n;
    }
    for (int64_t i = 0; i < d; ++i) {
        S.gmu[i] = idot(p->colptr, p->rowval, p->nzval, i, p->mu);
        S.gmu_t[i] = p->t_mu ? idot(p->t_colptr, p->t_rowval, p->t_nzval, i, p->t_mu) : 0.0;
    }
    memset(out, 0, sizeof *out);

    /* stickyzz, :176-208 */
    double tp = t0; /* t′ = maximum(t0), :181 */
    for (int64_t i = 0; i < d; ++i) {
        t[i] = t0;
        S.t_old[i] = t0; /* u_old = (copy(t0), x0, v0_old), :184 */
        v_old[i] = v[i]; /* v0_old = copy(v0), :182 */
        action[i] = ACT_HIT; /* fill(Action(0), d), :195 */
    }
    for (int64_t i = 0; i < d; ++i) { /* fill priorityqueue, :198-208 */
        ab(&S, i);                    /* push!(b, ab(...)), :199 */
        if (x[i] != barrier_of(p, i, v[i])) { /* :201 */
            queue_time(&S, i);                /* enqueue_time!, :202 */
        } else {
            const double kap = kappa_of(p, i, v[i]);
            v_old[i] = v[i]; /* v0_old[i], v0[i] = v0[i], 0.0: stop and save speed, :204 */
            v[i] = 0.0;
            action[i] = ACT_UNFREEZE;                 /* :205 */
            S.Q[i] = tp - pdmp_log(draw(&S)) / kap; /* :206 */
        }
    }

    int status = REF_OK;
    /* sticky_main, :220-238: while finished(end_condition, t′), i.e. t′ < T */
    while (status == REF_OK && tp < T) {
        int64_t i;
        int kind;
        for (;;) { /* stickyzz_inner!, :239-319 */
            /* i, t′ = peek(Q), :243 */
            i = 0;
            for (int64_t j = 1; j < d; ++j)
                if (S.Q[j] < S.Q[i]) i = j;
            tp = S.Q[i];
            const int64_t* G = p->rowval + p->colptr[i];
            const int64_t nG = p->colptr[i + 1] - p->colptr[i];
            const int64_t* G2 = g2idx + g2ptr[i];
            const int64_t nG2 = g2ptr[i + 1] - g2ptr[i];
            if (action[i] == ACT_HIT) { /* case 1) to be frozen or to reflect from boundary, :247-265 */
                const double vi = v[i];   /* di = dir(geti(u, i)), :248 */
                x[i] = barrier_of(p, i, vi); /* :249 */
                S.t_old[i] = t[i] = tp;      /* :250 */
                v_old[i] = vi;               /* stop and save speed, :251 */
                v[i] = 0.0;
                action[i] = ACT_UNFREEZE;                              /* :252 */
                S.Q[i] = tp - pdmp_log(draw(&S)) / kappa_of(p, i, vi); /* :253 */
                if (!p->strong) {                                      /* :254 */
                    ssmove(&S, G, nG, tp);                             /* :255 */
                    ssmove(&S, G2, nG2, tp);                           /* :256 */
                    rebound_neighbours(&S, i);                         /* :257-263 */
                }
                kind = EV_HIT;
                break; /* return i, t′, :265 */
            } else if (v[i] == 0 && v_old[i] != 0) { /* case 2) was frozen, :266-284 */
                S.t_old[i] = t[i] = tp;              /* :267 */
                v[i] = v_old[i];                     /* unfreeze, restore speed, :268 */
                v_old[i] = 0.0;
                const int32_t rule = rule_of(p, i, v[i]); /* di = dir(geti(u, i)), :269 */
                if (rule == RULE_REVERSIBLE) {            /* :270-271 */
                    v[i] *= (draw(&S) < 0.5) ? -1.0 : 1.0;
                } else if (rule == RULE_REFLECT) { /* :272-273 */
                    v[i] = -v[i];
                }
                ssmove(&S, G, nG, tp);     /* :275 */
                ssmove(&S, G2, nG2, tp);   /* :276 */
                rebound_neighbours(&S, i); /* :277-283 */
                kind = EV_THAW;
                break; /* :284 */
            } else {   /* a reflection time or an event time from the upper bound, :285-316 */
                ssmove(&S, G, nG, tp); /* :287 */
                double g = idot(p->t_colptr, p->t_rowval, p->t_nzval, i, x); /* ∇ϕi = target(t′, u, i, flow), :288 */
                if (p->t_mu) g = g - S.gmu_t[i];
                const double l = pos(g * v[i]);                                  /* λ, :129-135 */
                const double lb = pos(S.ba[i] + S.bb[i] * (t[i] - S.t_old[i])); /* (without the 0.01) */
                out->num += 1;
                if (draw(&S) * lb < l) { /* :292 */
                    out->nacc += 1;      /* accept!, :293 */
                    if (l > lb) {        /* :294 */
                        if (!p->adapt) { /* :295 */
                            status = REF_BOUND_VIOLATED;
                            kind = -1;
                            break;
                        }
                        out->nacc = out->num = 0; /* reset!(acc), :296 */
                        c[i] *= p->factor;        /* adapt!, :297, src/fact_samplers.jl:67-70 */
                        out->nadapt += 1;
                    }
                    v[i] = -v[i];              /* reflect!, :299, src/dynamics.jl:46-49 */
                    ssmove(&S, G2, nG2, tp);   /* :300 */
                    rebound_neighbours(&S, i); /* :301-307 */
                    kind = EV_REFLECTION;
                    break; /* :308 */
                } else {   /* :309-315 */
                    ab(&S, i);            /* :311 */
                    S.t_old[i] = t[i];    /* :312 */
                    queue_time(&S, i);    /* :313 */
                    continue;             /* don't save */
                }
            }
        }
        if (kind < 0) break;
        /* push!(Ξ, event(i, t, x, v, flow.old)), :230, src/fact_samplers.jl:73-75 */
        if (out->nevents < ev_cap) {
            ev_t[out->nevents] = t[i];
            ev_i[out->nevents] = i;
            ev_x[out->nevents] = x[i];
            ev_th[out->nevents] = v[i];
            ev_kind[out->nevents] = (int8_t)kind;
        }
        out->nevents += 1;
        if (kind == EV_HIT) out->nhit += 1;
        else if (kind == EV_THAW) out->nthaw += 1;
        else out->nrefl += 1;
    }
    out->status = status;
    out->ndraw_main = S.nm;
    out->t = tp;
    free(S.t_old);
    free(S.ba);
    free(S.bb);
    free(S.Q);
    free(S.gmu);
    free(S.gmu_t);
    free(g2ptr);
    free(g2idx);
    free(mark);
    return 0;
}
