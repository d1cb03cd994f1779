// qpn_lp.hip -- batched LP solver for the polyhedral primitives (qpn_solve_lps).
//
// Jobs over shared polyhedra: job t minimises c_t'x over {x : l <= A x <= u} of polyhedron poly_of[t], with c_t given or a signed
// row of A read in place.  Bounded-variable primal simplex on the row-activity form (x free, s = A x in [l, u]); the method is
// stated in include/qpn_hip.h and, operation by operation, by its numpy twin polyhedra.solve_lps_host, to which every output is
// bit-equal: sums run over the ascending index as acc = acc + a * b (no contraction), maxima / minima / lowest ids are exact in
// any order.  A team (one wavefront, or one workgroup of 256) works on one job:
//   a lane per row     for the basic values, the ratio test and the row sums of the post-check,
//   a lane per column  for the reduced costs, the pricing and the column sums of the post-check,
//   the pivot update   column by column (a wavefront per column), lanes along the rows: the dictionary is column-major with an
//                      odd leading dimension, so both access patterns are free of LDS bank conflicts.
// Classes by the size of a job's slice (lp_slice_bytes): up to 16 KiB one wavefront per job, LP_WAVES jobs per workgroup, in
// LDS; up to 156 KiB one workgroup per job in LDS; beyond, one workgroup per job over a slice of the context workspace, launched
// in chunks.  Every loop is bounded: the crash by d, the simplex loop by max_iters.
//
// qpn_issubset_pairs runs the same set-up, loop and check (lp_setup, lp_loop, lp_point, lp_check) with one
// team per pair P1 within P2: the crash and phase 1 over P1 once (lp_feasible), then the finite bounds of P2 one after the other
// as objectives from the basis the previous one left (lp_resolve), until one refutes (subset_core; polyhedra.issubset_pairs_host
// is its twin).  The slice is that of an LP over P1; the row of P2 is read in place into its cost vector.
//
// qpn_implicit_bounds runs them with one team per polyhedron: lp_feasible once, then the rows that are no
// explicit equalities from the last to the first, the minimum and the maximum of each by lp_resolve from the basis the previous
// solve left; a row whose values at two points the solves ended at differ by more than tol needs no LP (ib_core;
// polyhedra.implicit_bounds_host is its twin).  The slice is that of an LP; the witnesses stay in the registers of the lane that
// owns the row, the answers go straight to the job's output rows.
//
// qpn_exemplar_polys runs them with one team per polyhedron whose bounds may be open: the team writes the rows
// of the polyhedron's slack LP (min eps, A x + eps >= l, -A x + eps >= -u, eps >= -cap) into its region of the workspace, solves
// it as a job of qpn_solve_lps is solved (lp_setup, lp_finish cold) and applies the reference's rule to eps and the multipliers of
// the open bounds (ex_job; polyhedra.exemplar_polys_host is its twin).  The slice is that of an LP of 2 n + 1 rows in d + 1 variables.
//
// qpn_exemplar_products asks the same question of products of pieces, one team per product: the team gathers
// the rows of the product's factors from a pool of rows by index, tests the closure at the product's point, and solves the slack LP of
// the gathered rows as ex_job does (prod_job; polyhedra.exemplar_products_host is its twin).  Nothing of the pool is copied per product
// but the rows of the LP the job solves.
//
// qpn_irredundant_bounds runs them with one team per polyhedron: lp_feasible once, then the finite bounds of
// the rows from the last to the first, each relaxed in the job's working bounds and its row minimised (maximised) by lp_resolve
// from the basis the previous solve left; a bound the optimum does not pass is implied by the others and stays out, any other
// comes back (red_core; polyhedra.irredundant_bounds_host is its twin).  The working bounds are the job's own output rows.
//
// The six entries share the kernels and the launcher: lp_wave_kernel<Job> and lp_group_kernel<Job, LDS>
// run the job function of the kind Job (LpJob, SubsetJob, IbJob, ExJob, ProdJob, RedJob), lp_launch<Job> picks the class and launches.
#include <climits>

#include "qpn_internal.h"

namespace {

constexpr int LP_WAVES = 4;                     // jobs per workgroup in the wave class
constexpr int LP_GROUP = 256;
constexpr size_t LP_WAVE_SLICE_MAX = size_t(16) << 10;
constexpr size_t LP_GROUP_SLICE_MAX = size_t(156) << 10;
constexpr size_t LP_WS_CHUNK_BYTES = size_t(256) << 20;
constexpr double LP_BAND = 1.0 - 0x1p-30;       // candidates within this factor of the best count as equal (PIV_BAND)
constexpr double LP_TIE = 1e-12;
constexpr int LP_BLAND_AFTER = 20;

__host__ __device__ inline int lp_ld(int r) { return (r + 1) | 1; }
// doubles: T [ld x d] (cost row = row r), colb [r + 1], xn dj xf ray c [d each], xb g ls us sc lam amax tgt [r each], red [8]
__host__ __device__ inline size_t lp_slice_doubles(int r, int d)
{
    return (size_t)lp_ld(r) * d + (size_t)(r + 1) + 5 * (size_t)d + 8 * (size_t)r + 8;
}
size_t lp_slice_bytes(int r, int d) { return (lp_slice_doubles(r, d) * 8 + (size_t)(r + d) * 4 + 15) & ~(size_t)15; }

template <int T> __device__ inline void team_sync()
{
    if (T == 64) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

// exact reductions over the team; every thread gets the result.  red: 4 doubles of the slice
template <int T> __device__ inline double team_max(double v, double *red, int tid)
{
    for (int o = 32; o; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    if (T == 64) return v;
    team_sync<T>();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    team_sync<T>();
    v = red[0];
    for (int w = 1; w < T / 64; ++w) v = fmax(v, red[w]);
    return v;
}
template <int T> __device__ inline double team_min(double v, double *red, int tid)
{
    for (int o = 32; o; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    if (T == 64) return v;
    team_sync<T>();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    team_sync<T>();
    v = red[0];
    for (int w = 1; w < T / 64; ++w) v = fmin(v, red[w]);
    return v;
}
template <int T> __device__ inline int team_min_int(int v, double *red, int tid)
{
    for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o));
    if (T == 64) return v;
    team_sync<T>();
    if ((tid & 63) == 0) red[tid >> 6] = (double)v;
    team_sync<T>();
    v = (int)red[0];
    for (int w = 1; w < T / 64; ++w) v = min(v, (int)red[w]);
    return v;
}

// exchange the basic variable of row pi and the nonbasic one of column pj (the twin's _lp_pivot)
template <int T> __device__ inline void lp_pivot(double *Tm, double *colb, int r, int d, int ld, int pi, int pj, int tid)
{
    const double p = Tm[(size_t)pj * ld + pi];
    for (int k = tid; k <= r; k += T) colb[k] = Tm[(size_t)pj * ld + k];
    team_sync<T>();
    for (int c = tid; c < d; c += T) Tm[(size_t)c * ld + pi] = c == pj ? 1.0 / p : -Tm[(size_t)c * ld + pi] / p;
    team_sync<T>();
    const int lane = tid & 63;
    for (int c = tid >> 6; c < d; c += T / 64) {
        double *col = Tm + (size_t)c * ld;
        const double ni = col[pi];
        if (c == pj) {
            for (int k = lane; k <= r; k += 64) if (k != pi) col[k] = colb[k] / p;
        } else {
            for (int k = lane; k <= r; k += 64) if (k != pi) col[k] = col[k] + colb[k] * ni;
        }
    }
    team_sync<T>();
}

struct LpSlice {
    double *Tm, *colb, *xn, *dj, *xf, *ray, *cv, *xb, *g, *ls, *us, *sc, *lam, *amx, *tgt, *red;
    int *rb, *cn;
    __device__ LpSlice(double *base, int r, int d)
    {
        Tm = base; colb = Tm + (size_t)lp_ld(r) * d; xn = colb + (r + 1); dj = xn + d; xf = dj + d; ray = xf + d; cv = ray + d;
        xb = cv + d; g = xb + r; ls = g + r; us = ls + r; sc = us + r; lam = sc + r; amx = lam + r; tgt = amx + r; red = tgt + r;
        rb = reinterpret_cast<int *>(red + 8); cn = rb + r;
    }
};

// One polyhedron {x : lb <= Ab x <= ub} and the tolerances of its solves
struct LpProb {
    int r, d;
    const double *Ab, *lb, *ub;
    double piv_tol, feas_tol, opt_tol, ct;
    int max_iters;
};
__device__ inline LpProb lp_prob(int r, int d, const double *Ab, const double *lb, const double *ub, const LpTol &t)
{
    return LpProb{r, d, Ab, lb, ub, t.piv_tol, t.feas_tol, t.opt_tol, t.check_tol, t.max_iters};
}

// Steps 0-4 with the objective in S.cv: the data screen, scaling, the dictionary, the crash, the nonbasic values.
// -> QPN_LP_FAILURE when the screen fails the job (an entry of A or c that is not finite, a bound that is not a number, l = +inf
// or u = -inf; nothing is claimed, S.lam stays zero), QPN_LP_INFEASIBLE when an all-zero row outside its bounds settles it (its
// unit Farkas vector in S.lam), 0 otherwise.
template <int T> __device__ int lp_setup(const LpProb &P, const LpSlice &S, int tid)
{
    const int r = P.r, d = P.d, ld = lp_ld(r);
    const double *Ab = P.Ab, *lb = P.lb, *ub = P.ub;
    const double piv_tol = P.piv_tol;
    double *Tm = S.Tm, *red = S.red;
    int *rb = S.rb, *cn = S.cn;

    // 1. row scaling, 2. the dictionary
    int zbad = INT_MAX;                                   // -1: the data screen (0.) fails the job
    for (int j = tid; j < d; j += T) {
        if (!(fabs(S.cv[j]) < QINF)) zbad = -1;
        Tm[(size_t)j * ld + r] = S.cv[j]; cn[j] = j; S.xn[j] = 0.0;
    }
    for (int i = tid; i < r; i += T) {
        double m = 0.0;
        for (int j = 0; j < d; ++j) {
            const double v = fabs(Ab[(size_t)j * r + i]);
            if (!(v < QINF)) zbad = -1;
            m = fmax(m, v);
        }
        if (!(lb[i] < QINF) || !(ub[i] > -QINF)) zbad = -1;
        if (m == 0.0 && (ub[i] < 0.0 || lb[i] > 0.0)) zbad = min(zbad, i);
        const double s = m > 0.0 ? 1.0 / m : 1.0;
        S.amx[i] = m; S.sc[i] = s; S.ls[i] = lb[i] * s; S.us[i] = ub[i] * s; rb[i] = d + i;
        for (int j = 0; j < d; ++j) Tm[(size_t)j * ld + i] = Ab[(size_t)j * r + i] * s;
    }
    team_sync<T>();
    zbad = team_min_int<T>(zbad, red, tid);
    if (zbad < 0) return QPN_LP_FAILURE;
    if (zbad < r) {                                       // an all-zero row outside its bounds: the unit Farkas vector
        if (tid == 0) S.lam[zbad] = ub[zbad] < 0.0 ? 1.0 : -1.0;
        team_sync<T>();
        return QPN_LP_INFEASIBLE;
    }

    // 3. crash
    for (int j = 0; j < d; ++j) {
        const double *col = Tm + (size_t)j * ld;
        double m = 0.0;
        for (int i = tid; i < r; i += T) if (rb[i] >= d) m = fmax(m, fabs(col[i]));
        const double best = team_max<T>(m, red, tid);
        if (!(best > piv_tol)) continue;
        const double thr = best * LP_BAND;
        int mi = INT_MAX;
        for (int i = tid; i < r; i += T) if (rb[i] >= d && fabs(col[i]) >= thr) mi = min(mi, i);
        const int pi = team_min_int<T>(mi, red, tid);
        lp_pivot<T>(Tm, S.colb, r, d, ld, pi, j, tid);
        if (tid == 0) { const int v = rb[pi]; rb[pi] = cn[j]; cn[j] = v; }
        team_sync<T>();
    }
    // 4. nonbasic values
    for (int j = tid; j < d; j += T) {
        const int id = cn[j];
        double v = 0.0;
        if (id >= d) {
            const double lo = S.ls[id - d], hi = S.us[id - d];
            const bool fl = !isinf(lo) && lo == lo, fh = !isinf(hi) && hi == hi;
            if (fl && fh) v = fabs(lo) <= fabs(hi) ? lo : hi;
            else if (fl) v = lo;
            else if (fh) v = hi;
        }
        S.xn[j] = v;
    }
    team_sync<T>();
    return 0;
}

// Steps 5-8: the simplex loop from the slice's dictionary, with a fresh degeneracy counter and the step counter at iters0 (the
// steps before a rebuild count against the same max_iters).  -> status; the steps, and the last entering column and its direction
// (the ray of an UNBOUNDED end).
template <int T>
__device__ int lp_loop(const LpProb &P, const LpSlice &S, int tid, int iters0, int *iters_out, int *e_out, double *dirn_out)
{
    const int r = P.r, d = P.d, ld = lp_ld(r);
    const double piv_tol = P.piv_tol, feas_tol = P.feas_tol, opt_tol = P.opt_tol;
    double *Tm = S.Tm, *red = S.red;
    int *rb = S.rb, *cn = S.cn;
    int status = QPN_LP_FAILURE, iters = iters0, degen = 0, e = -1;
    double dirn = 0.0;
    for (;;) {
        // basic values, violations
        int viol = 1;
        for (int i = tid; i < r; i += T) {
            double acc = 0.0;
            for (int j = 0; j < d; ++j) {
                const double v = S.xn[j];
                if (v != 0.0) acc = acc + Tm[(size_t)j * ld + i] * v;
            }
            const int id = rb[i];
            const double lo = id >= d ? S.ls[id - d] : -QINF, up = id >= d ? S.us[id - d] : QINF;
            const bool below = acc < lo - feas_tol * fmax(1.0, fabs(lo)), above = acc > up + feas_tol * fmax(1.0, fabs(up));
            S.xb[i] = acc; S.g[i] = below ? -1.0 : above ? 1.0 : 0.0;
            if (below || above) viol = 0;
        }
        team_sync<T>();
        const bool phase1 = team_min_int<T>(viol, red, tid) == 0;
        // 5. reduced costs
        for (int j = tid; j < d; j += T) {
            const double *col = Tm + (size_t)j * ld;
            double acc = col[r];
            if (phase1) {
                acc = 0.0;
                for (int i = 0; i < r; ++i) {
                    const double gi = S.g[i];
                    if (gi != 0.0) acc = acc + gi * col[i];
                }
            }
            S.dj[j] = acc;
        }
        team_sync<T>();
        // 6. the entering variable
        const bool bland = degen >= LP_BLAND_AFTER;
        double m = 0.0;
        int low = INT_MAX;
        for (int j = tid; j < d; j += T) {
            const int id = cn[j];
            const double lo = id >= d ? S.ls[id - d] : -QINF, up = id >= d ? S.us[id - d] : QINF, v = S.xn[j], dv = S.dj[j];
            if (lo != up && ((dv < -opt_tol && v < up) || (dv > opt_tol && v > lo))) { m = fmax(m, fabs(dv)); low = min(low, id); }
        }
        int eid;
        if (bland) {
            eid = team_min_int<T>(low, red, tid);
        } else {
            const double thr = team_max<T>(m, red, tid) * LP_BAND;
            low = INT_MAX;
            for (int j = tid; j < d; j += T) {
                const int id = cn[j];
                const double lo = id >= d ? S.ls[id - d] : -QINF, up = id >= d ? S.us[id - d] : QINF, v = S.xn[j], dv = S.dj[j];
                if (lo != up && ((dv < -opt_tol && v < up) || (dv > opt_tol && v > lo)) && fabs(dv) >= thr) low = min(low, id);
            }
            eid = team_min_int<T>(low, red, tid);
        }
        if (eid == INT_MAX) { status = phase1 ? QPN_LP_INFEASIBLE : QPN_LP_OPTIMAL; break; }
        for (int j = tid; j < d; j += T)
            if (cn[j] == eid) {
                const double up = eid >= d ? S.us[eid - d] : QINF;
                red[4] = (double)j; red[5] = (S.dj[j] < -opt_tol && S.xn[j] < up) ? 1.0 : -1.0;
            }
        team_sync<T>();
        e = (int)red[4]; dirn = red[5];
        // 7. the ratio test
        const double *ecol = Tm + (size_t)e * ld;
        double tm = QINF;
        for (int i = tid; i < r; i += T) {
            const double av = ecol[i] * dirn, gi = S.g[i];
            const int id = rb[i];
            const double lo = id >= d ? S.ls[id - d] : -QINF, up = id >= d ? S.us[id - d] : QINF;
            const double tg = av > 0.0 ? (gi < 0.0 ? lo : gi > 0.0 ? QINF : up) : (gi > 0.0 ? up : gi < 0.0 ? -QINF : lo);
            const double ra = fabs(av) > piv_tol ? fmax((tg - S.xb[i]) / av, 0.0) : QINF;
            S.colb[i] = ra; S.tgt[i] = tg;
            tm = fmin(tm, ra);
        }
        const double elo = eid >= d ? S.ls[eid - d] : -QINF, eup = eid >= d ? S.us[eid - d] : QINF, exn = S.xn[e];
        const double tflip = dirn > 0.0 ? eup - exn : exn - elo;
        const double tmin = fmin(tflip, team_min<T>(tm, red, tid));
        if (!(tmin < QINF)) { status = phase1 ? QPN_LP_FAILURE : QPN_LP_UNBOUNDED; break; }
        const double thr = tmin + LP_TIE * fmax(1.0, tmin);
        int w = INT_MAX;
        for (int i = tid; i < r; i += T) if (S.colb[i] <= thr) w = min(w, rb[i]);
        int win = team_min_int<T>(w, red, tid);
        if (tflip <= thr && eid < win) win = eid;
        if (win == INT_MAX) { status = QPN_LP_FAILURE; break; }   // (not-a-number data: no candidate compares)
        if (iters >= P.max_iters) { status = QPN_LP_ITER_LIMIT; break; }   // a step is due and none is left
        ++iters;
        degen = tmin == 0.0 ? degen + 1 : 0;
        if (win == eid) {                                 // a flip to the opposite bound: no pivot
            team_sync<T>();
            if (tid == 0) S.xn[e] = dirn > 0.0 ? eup : elo;
            team_sync<T>();
        } else {
            for (int i = tid; i < r; i += T) if (rb[i] == win) { red[6] = (double)i; red[7] = S.tgt[i]; }
            team_sync<T>();
            const int pi = (int)red[6];
            const double tv = red[7];
            lp_pivot<T>(Tm, S.colb, r, d, ld, pi, e, tid);  // 8.
            if (tid == 0) { rb[pi] = eid; cn[e] = win; S.xn[e] = tv; }
            team_sync<T>();
        }
    }
    *iters_out = iters; *e_out = e; *dirn_out = dirn;
    return status;
}

// 9. the answer on the unscaled data: x into S.xf.  -> c'x
template <int T> __device__ double lp_point(const LpProb &P, const LpSlice &S, int tid)
{
    const int r = P.r, d = P.d;
    for (int j = tid; j < d; j += T) if (S.cn[j] < d) S.xf[S.cn[j]] = S.xn[j];
    for (int i = tid; i < r; i += T) if (S.rb[i] < d) S.xf[S.rb[i]] = S.xb[i];
    team_sync<T>();
    double obj = 0.0;
    for (int k = 0; k < d; ++k) obj = obj + S.cv[k] * S.xf[k];
    return obj;
}

// ... and the check of what an OPTIMAL / UNBOUNDED / INFEASIBLE end claims: the multipliers / Farkas vector into S.lam, the ray
// into S.ray (both zeroed by the caller).  -> status, or QPN_LP_FAILURE when the certificate does not hold.
template <int T> __device__ int lp_check(const LpProb &P, const LpSlice &S, int status, int e, double dirn, int tid)
{
    const int r = P.r, d = P.d, ld = lp_ld(r);
    const double *Ab = P.Ab, *lb = P.lb, *ub = P.ub;
    const double ct = P.ct;
    double *Tm = S.Tm, *red = S.red;
    int *rb = S.rb, *cn = S.cn;
    int ok = 1;
    double *s = S.xb;                                      // (the basic values are not needed any more)
    for (int i = tid; i < r; i += T) {
        double acc = 0.0;
        for (int j = 0; j < d; ++j) acc = acc + Ab[(size_t)j * r + i] * S.xf[j];
        s[i] = acc;
        const double tl = ct * fmax(1.0, fabs(lb[i])), tu = ct * fmax(1.0, fabs(ub[i]));
        if (status != QPN_LP_INFEASIBLE && !(acc >= lb[i] - tl && acc <= ub[i] + tu)) ok = 0;
    }
    if (status == QPN_LP_OPTIMAL) {
        for (int j = tid; j < d; j += T) if (cn[j] >= d) S.lam[cn[j] - d] = S.dj[j] * S.sc[cn[j] - d];
        team_sync<T>();
        for (int k = tid; k < d; k += T) {
            double acc = 0.0;
            for (int i = 0; i < r; ++i) acc = acc + Ab[(size_t)k * r + i] * S.lam[i];
            if (!(fabs(S.cv[k] - acc) <= ct * fmax(1.0, fabs(S.cv[k])))) ok = 0;
        }
        for (int i = tid; i < r; i += T) {
            const double lm = S.lam[i];
            if (lm > ct && !(fabs(s[i] - lb[i]) <= ct * fmax(1.0, fabs(lb[i])))) ok = 0;
            if (lm < -ct && !(fabs(s[i] - ub[i]) <= ct * fmax(1.0, fabs(ub[i])))) ok = 0;
        }
    } else if (status == QPN_LP_UNBOUNDED) {
        const double *ecol = Tm + (size_t)e * ld;
        if (tid == 0 && cn[e] < d) S.ray[cn[e]] = dirn;
        for (int i = tid; i < r; i += T) if (rb[i] < d) S.ray[rb[i]] = ecol[i] * dirn;
        team_sync<T>();
        double cr = 0.0, rmax = 0.0;
        for (int k = 0; k < d; ++k) { cr = cr + S.cv[k] * S.ray[k]; rmax = fmax(rmax, fabs(S.ray[k])); }
        if (!(cr < 0.0)) ok = 0;
        for (int i = tid; i < r; i += T) {
            double acc = 0.0;
            for (int j = 0; j < d; ++j) acc = acc + Ab[(size_t)j * r + i] * S.ray[j];
            const double tr = ct * fmax(1.0, rmax) * S.amx[i];
            if (!isinf(lb[i]) && lb[i] == lb[i] && !(acc >= -tr)) ok = 0;
            if (!isinf(ub[i]) && ub[i] == ub[i] && !(acc <= tr)) ok = 0;
        }
    } else {
        for (int i = tid; i < r; i += T) if (rb[i] >= d) S.lam[rb[i] - d] = S.g[i] * S.sc[rb[i] - d];
        for (int j = tid; j < d; j += T)
            if (cn[j] >= d) {
                const int k = cn[j] - d;
                double y = -S.dj[j];
                if ((y > 0.0 && !(fabs(ub[k]) < QINF)) || (y < 0.0 && !(fabs(lb[k]) < QINF))) y = 0.0;
                S.lam[k] = y * S.sc[k];
            }
        team_sync<T>();
        // the Farkas sum is negative by more than every bound relaxed by the tolerance primal feasibility is judged at accounts for
        double ymax = 0.0, bound = 0.0, slack = 0.0;
        for (int i = 0; i < r; ++i) {
            const double y = S.lam[i];
            ymax = fmax(ymax, fabs(y));
            if (y > 0.0) { bound = bound + y * ub[i]; slack = slack + y * (ct * fmax(1.0, fabs(ub[i]))); }
            else if (y < 0.0) { bound = bound + y * lb[i]; slack = slack - y * (ct * fmax(1.0, fabs(lb[i]))); }
        }
        ymax = fmax(1.0, ymax);
        for (int k = tid; k < d; k += T) {
            double acc = 0.0;
            for (int i = 0; i < r; ++i) acc = acc + Ab[(size_t)k * r + i] * S.lam[i];
            if (!(fabs(acc) <= ct * ymax)) ok = 0;
        }
        if (!(bound < -slack)) ok = 0;
    }
    team_sync<T>();
    return team_min_int<T>(ok, red, tid) ? status : QPN_LP_FAILURE;
}

// Step 10, the dictionary of the current basis once more from the scaled rows (the twin's _lp_rebuild): T = A * sc with the cost
// row S.cv, every x nonbasic; then, for the columns j ascending whose x is basic in the current basis (a row's id stands in column
// j: a nonbasic x never left its own column), the crash's pivot restricted to the rows whose id is nonbasic in the current basis
// and still basic here.  At most d pivots; the nonbasic rows keep their values.  S.g, S.tgt and S.dj hold the basis meanwhile (the
// loop writes them before it reads them).  -> false when a pivot is not above piv_tol.
template <int T> __device__ bool lp_rebuild(const LpProb &P, const LpSlice &S, int tid)
{
    const int r = P.r, d = P.d, ld = lp_ld(r);
    double *Tm = S.Tm, *red = S.red;
    int *rb = S.rb, *cn = S.cn;
    team_sync<T>();
    for (int i = tid; i < r; i += T) { S.g[i] = 0.0; S.tgt[i] = 0.0; }
    team_sync<T>();
    for (int j = tid; j < d; j += T) {
        const int id = cn[j];
        S.dj[j] = id >= d ? 1.0 : 0.0;
        if (id >= d) { S.g[id - d] = 1.0; S.tgt[id - d] = S.xn[j]; }
        Tm[(size_t)j * ld + r] = S.cv[j]; cn[j] = j;
    }
    for (int i = tid; i < r; i += T) {
        const double s = S.sc[i];
        rb[i] = d + i;
        for (int j = 0; j < d; ++j) Tm[(size_t)j * ld + i] = P.Ab[(size_t)j * r + i] * s;
    }
    team_sync<T>();
    for (int j = 0; j < d; ++j) {
        if (S.dj[j] == 0.0) continue;                     // (the same in every thread)
        const double *col = Tm + (size_t)j * ld;
        double m = 0.0;
        for (int i = tid; i < r; i += T) if (S.g[i] != 0.0 && rb[i] >= d) m = fmax(m, fabs(col[i]));
        const double best = team_max<T>(m, red, tid);
        if (!(best > P.piv_tol)) return false;
        const double thr = best * LP_BAND;
        int mi = INT_MAX;
        for (int i = tid; i < r; i += T) if (S.g[i] != 0.0 && rb[i] >= d && fabs(col[i]) >= thr) mi = min(mi, i);
        const int pi = team_min_int<T>(mi, red, tid);
        lp_pivot<T>(Tm, S.colb, r, d, ld, pi, j, tid);
        if (tid == 0) { const int v = rb[pi]; rb[pi] = cn[j]; cn[j] = v; }
        team_sync<T>();
    }
    for (int j = tid; j < d; j += T) if (cn[j] >= d) S.xn[j] = S.tgt[cn[j] - d];
    team_sync<T>();
    return true;
}

// Steps 5-10 from the slice's dictionary with the objective in S.cv and S.lam, S.ray zero (the twin's _lp_finish): the loop, the
// point and step 9's check; an end that is not certified -- a FAILURE of the loop, an INFEASIBLE end of a warm solve (the
// polyhedron has a point), a certificate that fails -- rebuilds the dictionary and runs the loop once more, the step counter going
// on; what that ends with stands.  LP_COLD: an INFEASIBLE end is an outcome, checked like the others; LP_FEASIBLE: that, and an
// OPTIMAL end is taken unchecked (c = 0); LP_WARM: an INFEASIBLE end is a FAILURE.  -> status; every status but a certified one
// leaves S.lam = S.ray = 0.  x in S.xf, c'x in *obj_out and, after a check, A x in S.xb.
enum { LP_WARM = 0, LP_COLD = 1, LP_FEASIBLE = 2 };
template <int T> __device__ int lp_finish(const LpProb &P, const LpSlice &S, int tid, int mode, int *iters_out, double *obj_out)
{
    int iters = 0, status;
    for (int attempt = 0;; ++attempt) {
        int e;
        double dirn;
        status = lp_loop<T>(P, S, tid, iters, &iters, &e, &dirn);
        *obj_out = lp_point<T>(P, S, tid);
        if (status == QPN_LP_ITER_LIMIT || (status == QPN_LP_OPTIMAL && mode == LP_FEASIBLE)) break;
        if (status == QPN_LP_OPTIMAL || status == QPN_LP_UNBOUNDED || (status == QPN_LP_INFEASIBLE && mode != LP_WARM))
            if (lp_check<T>(P, S, status, e, dirn, tid) == status) break;
        status = QPN_LP_FAILURE;
        team_sync<T>();
        for (int j = tid; j < P.d; j += T) S.ray[j] = 0.0;
        for (int i = tid; i < P.r; i += T) S.lam[i] = 0.0;
        team_sync<T>();
        if (attempt == 1 || !lp_rebuild<T>(P, S, tid)) break;
    }
    *iters_out = iters;
    return status;
}

// The feasibility solve of the subset tests and the implicit bounds (sections 5g (a), 5h (a); the twin's _lp_feasible): the set-up and
// lp_finish with c = 0 from zeroed slice vectors.  -> QPN_LP_OPTIMAL (a point of the polyhedron in S.xf, its basis in the dictionary),
// QPN_LP_INFEASIBLE (an all-zero row outside its bounds, *iters_out = 0, or an INFEASIBLE end whose Farkas certificate holds),
// QPN_LP_ITER_LIMIT, or QPN_LP_FAILURE (the data screen, *iters_out = 0, and an end the rebuild does not certify included).
template <int T> __device__ int lp_feasible(const LpProb &P, const LpSlice &S, int tid, int *iters_out)
{
    const int r = P.r, d = P.d;
    *iters_out = 0;
    for (int j = tid; j < d; j += T) { S.cv[j] = 0.0; S.xf[j] = 0.0; S.ray[j] = 0.0; }
    for (int i = tid; i < r; i += T) S.lam[i] = 0.0;
    team_sync<T>();
    if (const int settled = lp_setup<T>(P, S, tid)) return settled;
    double obj;
    return lp_finish<T>(P, S, tid, LP_FEASIBLE, iters_out, &obj);
}

// The solve of the objective in S.cv (all threads past a barrier) from the basis the previous solve over the polyhedron left
// (the twin's _lp_resolve): the cost row of c in the current dictionary (section 5g (e)), then lp_finish with fresh
// counters.  -> QPN_LP_OPTIMAL or QPN_LP_UNBOUNDED, certified; QPN_LP_ITER_LIMIT; QPN_LP_FAILURE (of the loop, an INFEASIBLE end, a
// certificate that fails, each after the rebuild and the second loop).  x in S.xf, c'x in *obj_out and, after a check, A x in S.xb.
template <int T> __device__ int lp_resolve(const LpProb &P, const LpSlice &S, int tid, int *iters_out, double *obj_out)
{
    const int r = P.r, d = P.d, ld = lp_ld(r);
    for (int j = tid; j < d; j += T) {
        const double *col = S.Tm + (size_t)j * ld;
        double acc = 0.0;
        for (int k = 0; k < r; ++k) {
            const int id = S.rb[k];
            if (id < d) acc = acc + S.cv[id] * col[k];
        }
        if (S.cn[j] < d) acc = acc + S.cv[S.cn[j]];
        S.Tm[(size_t)j * ld + r] = acc;
    }
    for (int j = tid; j < d; j += T) S.ray[j] = 0.0;
    for (int k = tid; k < r; k += T) S.lam[k] = 0.0;
    team_sync<T>();
    return lp_finish<T>(P, S, tid, LP_WARM, iters_out, obj_out);
}

// The solve of job t over polyhedron b.  Leaves x in S.xf, the multipliers / Farkas vector in S.lam, the ray in S.ray (zeroed by
// the caller).  -> status; *iters, *objv.
template <int T>
__device__ int lp_core(const LpArgs &a, const LpSlice &S, int t, int b, int orow, int tid, int *iters_out, double *obj_out)
{
    const int r = a.r, d = a.d;
    const LpProb P = lp_prob(r, d, a.A + (size_t)b * r * d, a.l + (size_t)b * r, a.u + (size_t)b * r, a.lp);
    *iters_out = 0; *obj_out = 0.0;
    for (int j = tid; j < d; j += T)
        S.cv[j] = a.cost ? a.cost[(size_t)t * d + j] : (double)a.obj_sign[t] * P.Ab[(size_t)j * r + orow];
    if (const int settled = lp_setup<T>(P, S, tid)) return settled;
    return lp_finish<T>(P, S, tid, LP_COLD, iters_out, obj_out);
}

template <int T> __device__ void lp_job(const LpArgs &a, int t, double *base, int tid)
{
    const int r = a.r, d = a.d;
    const LpSlice S(base, r, d);
    for (int j = tid; j < d; j += T) { S.xf[j] = 0.0; S.ray[j] = 0.0; }
    for (int i = tid; i < r; i += T) S.lam[i] = 0.0;
    if (tid < 8) S.red[tid] = 0.0;
    team_sync<T>();
    // an index out of range (device arrays are not read by the host): the job fails and reads nothing
    const int b = a.poly_of[t], orow = a.cost ? 0 : a.obj_row[t];
    int status = QPN_LP_FAILURE, iters = 0;
    double obj = 0.0;
    if (b >= 0 && b < a.polys && orow >= 0 && orow < r) status = lp_core<T>(a, S, t, b, orow, tid, &iters, &obj);
    team_sync<T>();
    if (a.x) for (int j = tid; j < d; j += T) a.x[(size_t)t * d + j] = S.xf[j];
    if (a.ray) for (int j = tid; j < d; j += T) a.ray[(size_t)t * d + j] = S.ray[j];
    if (a.lam) for (int i = tid; i < r; i += T) a.lam[(size_t)t * r + i] = S.lam[i];
    if (tid == 0) {
        a.status[t] = status;
        if (a.obj) a.obj[t] = obj;
        if (a.iters) a.iters[t] = iters;
    }
}

// ---- subset tests: one team per pair ------------------------------------------------------------------------------------------
struct SubsetOut { int how, bound, lps, iters; double val; };

// P1 = first piece b1, P2 = second piece b2 (both in range).  Every value a branch depends on is the same in all threads of
// the team (team reductions, or sums every thread runs over the slice), so a whole team leaves together.
template <int T> __device__ void subset_core(const SubsetArgs &a, const LpSlice &S, int b1, int b2, int tid, SubsetOut &o)
{
    const int r = a.r1, d = a.d, r2 = a.r2;
    const LpProb P = lp_prob(r, d, a.A1 + (size_t)b1 * r * d, a.l1 + (size_t)b1 * r, a.u1 + (size_t)b1 * r, a.lp);
    const double *A2 = a.A2 + (size_t)b2 * r2 * d, *l2 = a.l2 + (size_t)b2 * r2, *u2 = a.u2 + (size_t)b2 * r2;
    const double tol = a.tol;
    // (a) the feasibility solve
    int it;
    o.lps = 1;
    int status = lp_feasible<T>(P, S, tid, &it);
    o.iters = it;
    if (status != QPN_LP_OPTIMAL) {
        o.how = status == QPN_LP_INFEASIBLE ? QPN_SUBSET_EMPTY : status == QPN_LP_ITER_LIMIT ? QPN_SUBSET_ITER_LIMIT : QPN_SUBSET_FAILURE;
        return;
    }
    // (b) the bounds of P2 in order
    for (int i = 0; i < r2; ++i) {
        const double l2i = l2[i], u2i = u2[i];
        const bool fl = fabs(l2i) < QINF, fu = fabs(u2i) < QINF;
        if (!fl && !fu) continue;
        team_sync<T>();
        for (int j = tid; j < d; j += T) S.cv[j] = A2[(size_t)j * r2 + i];
        team_sync<T>();
        // (c) rows of P1 equal to this one: the tightest of their bounds
        double lo = -QINF, hi = QINF;
        for (int k = tid; k < r; k += T) {
            bool same = true;
            for (int c = 0; c < d && same; ++c) same = P.Ab[(size_t)c * r + k] == S.cv[c];
            if (same) { lo = fmax(lo, P.lb[k]); hi = fmin(hi, P.ub[k]); }
        }
        const double lo1 = team_max<T>(lo, S.red, tid);
        const double hi1 = team_min<T>(hi, S.red, tid);
        for (int side = 0; side < 2; ++side) {
            double beta;
            if (side == 0) {
                if (!fl || lo1 >= l2i - tol) continue;
                beta = l2i;
            } else {
                if (!fu || hi1 <= u2i + tol) continue;
                beta = -u2i;
                team_sync<T>();
                for (int j = tid; j < d; j += T) S.cv[j] = -A2[(size_t)j * r2 + i];
                team_sync<T>();
            }
            o.bound = 2 * i + side;
            // (d) the point the previous solve ended at
            double v = 0.0;
            for (int k = 0; k < d; ++k) v = v + S.cv[k] * S.xf[k];
            if (v < beta - tol) { o.how = QPN_SUBSET_BY_POINT; o.val = v; return; }
            // (e) the cost row of c in the current dictionary, (f) solve and decide
            double obj;
            ++o.lps;
            status = lp_resolve<T>(P, S, tid, &it, &obj);
            o.iters += it;
            if (status == QPN_LP_ITER_LIMIT) { o.how = QPN_SUBSET_ITER_LIMIT; return; }
            if (status == QPN_LP_FAILURE) { o.how = QPN_SUBSET_FAILURE; return; }
            if (status == QPN_LP_UNBOUNDED) { o.how = QPN_SUBSET_UNBOUNDED; return; }
            if (obj < beta - tol) { o.how = QPN_SUBSET_BY_OPTIMUM; o.val = obj; return; }
            o.bound = -1;
        }
    }
    o.how = QPN_SUBSET_HOLDS;                             // (g)
}

template <int T> __device__ void subset_job(const SubsetArgs &a, int q, double *base, int tid)
{
    const LpSlice S(base, a.r1, a.d);
    if (tid < 8) S.red[tid] = 0.0;
    team_sync<T>();
    // an index out of range (device arrays are not read by the host): the pair fails and reads nothing
    const int b1 = a.pi[q], b2 = a.pj[q];
    SubsetOut o{QPN_SUBSET_FAILURE, -1, 0, 0, 0.0};
    if (b1 >= 0 && b1 < a.B1 && b2 >= 0 && b2 < a.B2) subset_core<T>(a, S, b1, b2, tid, o);
    if (tid == 0) {
        a.sub[q] = o.how == QPN_SUBSET_HOLDS || o.how == QPN_SUBSET_EMPTY ? 1 : 0;
        if (a.how) a.how[q] = o.how;
        if (a.bound) a.bound[q] = o.bound;
        if (a.val) a.val[q] = o.val;
        if (a.lps) a.lps[q] = o.lps;
        if (a.iters) a.iters[q] = o.iters;
    }
}

// ---- implicit bounds: one team per polyhedron -----------------------------------------------------------------------------------
// Rows a lane owns at the most: row i belongs to lane i % T.  ceil(QPN_LP_MAX_R / LP_GROUP) in the workgroup classes; in the
// wavefront class a slice of at most 16 KiB holds r <= 195 rows (lp_slice_bytes >= 84 r), that is 4 per lane as well.
constexpr int IB_NK = 4;
static_assert(IB_NK * LP_GROUP >= QPN_LP_MAX_R && IB_NK * 64 >= LP_WAVE_SLICE_MAX / 84, "a lane's rows must fit its registers");

struct IbOut { int status, fail_row, lps, iters; };

// Polyhedron b (in range).  Every value a branch depends on is the same in all threads of the team (team reductions, values
// read from the slice after a barrier, the polyhedron's own bounds), so a whole team leaves together.  The witnesses wlo / whi of
// a lane's rows are registers: the arrays are indexed by unrolled constants only.
template <int T> __device__ void ib_core(const IbArgs &a, const LpSlice &S, int b, int tid, IbOut &o)
{
    const int r = a.r, d = a.d;
    const LpProb P = lp_prob(r, d, a.A + (size_t)b * r * d, a.l + (size_t)b * r, a.u + (size_t)b * r, a.lp);
    const double tol = a.tol;
    const bool every = (a.flags & QPN_IB_ALL_EXTREMES) != 0;
    uint8_t *eq = a.eq + (size_t)b * r;
    double *vals = a.vals + (size_t)b * r;
    int32_t *how = a.how ? a.how + (size_t)b * r : nullptr;
    double *lo = a.lo ? a.lo + (size_t)b * r : nullptr, *hi = a.hi ? a.hi + (size_t)b * r : nullptr;
    // (0) explicit rows; the other rows' answers until an LP or two points decide them
    int uncrossed = 1;
#pragma unroll
    for (int k = 0; k < IB_NK; ++k) {
        const int i = tid + k * T;
        if (i < r) {
            const double li = P.lb[i], ui = P.ub[i];
            const bool ex = fabs(li - ui) <= tol || li == ui;
            if (!ex && li > ui) uncrossed = 0;
            eq[i] = ex ? 1 : 0; vals[i] = ex ? 0.5 * (li + ui) : QINF;
            if (how) how[i] = ex ? QPN_IB_HOW_EXPLICIT : QPN_IB_HOW_UNDECIDED;
            if (lo) lo[i] = __builtin_nan("");
            if (hi) hi[i] = __builtin_nan("");
        }
    }
    if (!team_min_int<T>(uncrossed, S.red, tid)) { o.status = QPN_IB_EMPTY; return; }   // crossed bounds: no LP is started
    // (a) the feasibility solve
    int it;
    o.lps = 1;
    int status = lp_feasible<T>(P, S, tid, &it);
    o.iters = it;
    if (status != QPN_LP_OPTIMAL) {
        o.status = status == QPN_LP_INFEASIBLE ? QPN_IB_EMPTY : status == QPN_LP_ITER_LIMIT ? QPN_IB_ITER_LIMIT : QPN_IB_FAILURE;
        return;
    }
    // (b) the witnesses: a lane per row, A read in place
    double wlo[IB_NK], whi[IB_NK];
#pragma unroll
    for (int k = 0; k < IB_NK; ++k) {
        const int i = tid + k * T;
        double acc = 0.0;
        if (i < r)
            for (int j = 0; j < d; ++j) acc = acc + P.Ab[(size_t)j * r + i] * S.xf[j];
        wlo[k] = acc; whi[k] = acc;
    }
    // (c) the rows from the last
    for (int i = r - 1; i >= 0; --i) {
        const double li = P.lb[i], ui = P.ub[i];
        if (fabs(li - ui) <= tol || li == ui) continue;
        const bool mine = i % T == tid;                   // this lane owns the row
        // the witnesses of row i, from the lane that holds them
        team_sync<T>();
#pragma unroll
        for (int k = 0; k < IB_NK; ++k)
            if (tid + k * T == i) { S.red[5] = wlo[k]; S.red[6] = whi[k]; }
        team_sync<T>();
        double wl = S.red[5], wh = S.red[6];
        if (!every && wh - wl > tol) {
            if (mine && how) how[i] = QPN_IB_HOW_BY_POINTS;
            continue;
        }
        double lov = 0.0, hiv = 0.0;
        bool decided = false;
        for (int side = 0; side < 2 && !decided; ++side) {
            team_sync<T>();
            for (int j = tid; j < d; j += T) { const double v = P.Ab[(size_t)j * r + i]; S.cv[j] = side ? -v : v; }
            team_sync<T>();
            double obj;
            ++o.lps;
            status = lp_resolve<T>(P, S, tid, &it, &obj);
            o.iters += it;
            if (status == QPN_LP_ITER_LIMIT) { o.status = QPN_IB_ITER_LIMIT; o.fail_row = i; return; }
            if (status == QPN_LP_FAILURE) { o.status = QPN_IB_FAILURE; o.fail_row = i; return; }
            // (b) the rows at the new point: the check left A x in S.xb
#pragma unroll
            for (int k = 0; k < IB_NK; ++k) {
                const int ii = tid + k * T;
                if (ii < r) {
                    const double s = S.xb[ii];
                    wlo[k] = s < wlo[k] ? s : wlo[k]; whi[k] = s > whi[k] ? s : whi[k];
                }
            }
            const double si = S.xb[i];
            wl = si < wl ? si : wl; wh = si > wh ? si : wh;
            if (side == 0) {
                lov = status == QPN_LP_UNBOUNDED ? -QINF : obj;
                if (mine && lo) lo[i] = lov;
                if (!every) {
                    if (status == QPN_LP_UNBOUNDED) {
                        if (mine && how) how[i] = QPN_IB_HOW_UNBOUNDED;
                        decided = true;
                    } else if (wh - lov > tol) {
                        if (mine && how) how[i] = QPN_IB_HOW_BY_POINTS;
                        decided = true;
                    }
                }
            } else {
                hiv = status == QPN_LP_UNBOUNDED ? QINF : -obj;
                if (mine && hi) hi[i] = hiv;
            }
        }
        if (decided) continue;
        const bool finite = fabs(lov) < QINF && fabs(hiv) < QINF;
        const bool same = finite && fabs(lov - hiv) <= tol;
        if (mine) {
            if (same) { eq[i] = 1; vals[i] = 0.5 * (hiv + lov); }
            if (how) how[i] = same ? QPN_IB_HOW_IMPLICIT : finite ? QPN_IB_HOW_BY_EXTREMES : QPN_IB_HOW_UNBOUNDED;
        }
    }
    o.status = QPN_IB_OK;
}

template <int T> __device__ void ib_job(const IbArgs &a, int b, double *base, int tid)
{
    const LpSlice S(base, a.r, a.d);
    if (tid < 8) S.red[tid] = 0.0;
    team_sync<T>();
    IbOut o{QPN_IB_FAILURE, -1, 0, 0};
    ib_core<T>(a, S, b, tid, o);
    if (tid == 0) {
        a.status[b] = o.status;
        if (a.fail_row) a.fail_row[b] = o.fail_row;
        if (a.lps) a.lps[b] = o.lps;
        if (a.iters) a.iters[b] = o.iters;
    }
}

// ---- emptiness of polyhedra with open bounds: one team per polyhedron -----------------------------------------------------------
// A job's region of the workspace: the rows of its slack LP, A [(d + 1) x (2 n + 1)] column-major, then l and u [2 n + 1 each]
__host__ __device__ inline size_t ex_rows_bytes(int n, int d)
{
    const size_t R = 2 * (size_t)n + 1;
    return ((R * (size_t)(d + 1) + 2 * R) * 8 + 15) & ~(size_t)15;
}

// Job t of a launch: polyhedron a.first + t, the rows in region t.  Every value a branch depends on is the same in all threads
// of the team (the status of the solve, values read from the slice after a barrier, a team reduction).
template <int T> __device__ void ex_job(const ExArgs &a, int t, double *base, int tid)
{
    const int n = a.n, d = a.d, R = 2 * n + 1, D = d + 1;
    const size_t b = (size_t)a.first + (size_t)t;
    const double *A = a.A + b * n * d, *l = a.l + b * n, *u = a.u + b * n;
    double *Ae = reinterpret_cast<double *>(a.rows + (size_t)t * ex_rows_bytes(n, d)), *le = Ae + (size_t)R * D, *ue = le + R;
    const LpSlice S(base, R, D);
    // (a) the rows of the slack LP: [a_i, 1] >= l_i, [-a_i, 1] >= -u_i, eps >= -slack_cap; the objective is the last row
    for (int i = tid; i < R; i += T) {
        const int k = i < n ? i : i - n;
        for (int j = 0; j < d; ++j) Ae[(size_t)j * R + i] = i < n ? A[(size_t)j * n + k] : i < 2 * n ? -A[(size_t)j * n + k] : 0.0;
        Ae[(size_t)d * R + i] = 1.0;
        le[i] = i < n ? l[k] : i < 2 * n ? -u[k] : -a.slack_cap;
        ue[i] = QINF;
        S.lam[i] = 0.0;
    }
    for (int j = tid; j < D; j += T) { S.cv[j] = j == d ? 1.0 : 0.0; S.xf[j] = 0.0; S.ray[j] = 0.0; }
    if (tid < 8) S.red[tid] = 0.0;
    team_sync<T>();
    const LpProb P = lp_prob(R, D, Ae, le, ue, a.lp);
    int iters = 0;
    double obj = 0.0;
    int status = lp_setup<T>(P, S, tid);
    if (!status) status = lp_finish<T>(P, S, tid, LP_COLD, &iters, &obj);
    team_sync<T>();
    // (b) the rule on the certified optimum
    const double tol = a.tol;
    int how = status == QPN_LP_ITER_LIMIT ? QPN_EX_ITER_LIMIT : QPN_EX_FAILURE, row = -1;
    double eps = __builtin_nan("");
    if (status == QPN_LP_OPTIMAL) {
        eps = S.xf[d];
        if (eps > tol) {
            how = QPN_EX_EMPTY_SLACK;
        } else if (eps > -tol) {
            int low = INT_MAX;
            for (int i = tid; i < n; i += T) {
                if (a.open_hi && a.open_hi[b * n + i] && fabs(u[i]) < QINF && fabs(S.lam[n + i]) > tol) low = min(low, 2 * i + 1);
                if (a.open_lo && a.open_lo[b * n + i] && fabs(l[i]) < QINF && fabs(S.lam[i]) > tol) low = min(low, 2 * i);
            }
            low = team_min_int<T>(low, S.red, tid);
            how = low == INT_MAX ? QPN_EX_MEMBER_BAND : QPN_EX_EMPTY_OPEN;
            if (low != INT_MAX) row = low;
        } else {
            how = QPN_EX_MEMBER;
        }
    }
    const bool member = how == QPN_EX_MEMBER || how == QPN_EX_MEMBER_BAND, solved = status == QPN_LP_OPTIMAL;
    if (a.x) for (int j = tid; j < d; j += T) a.x[b * d + j] = member ? S.xf[j] : 0.0;
    if (a.lam) for (int i = tid; i < R; i += T) a.lam[b * R + i] = solved ? S.lam[i] : 0.0;
    if (tid == 0) {
        a.empty[b] = how == QPN_EX_EMPTY_SLACK || how == QPN_EX_EMPTY_OPEN ? 1 : 0;
        if (a.how) a.how[b] = how;
        if (a.eps) a.eps[b] = eps;
        if (a.row) a.row[b] = row;
        if (a.iters) a.iters[b] = iters;
    }
}

// ---- emptiness of products of pieces: one team per product ------------------------------------------------------------------------
// A job's region of the workspace: the rows of its slack LP as in ex_rows_bytes, then the map product row -> pool row [n] int32
__host__ __device__ inline size_t prod_region_bytes(int n, int d) { return (ex_rows_bytes(n, d) + (size_t)n * 4 + 15) & ~(size_t)15; }

// Job t of a launch: product a.first + t, region t.  Every value a branch depends on is the same in all threads of the team: the
// factor slots every thread walks, team reductions, the status of the solve, values read from the slice after a barrier.  The rule
// (c) is ex_job's own (b), stated again here: ex_job is not edited, so that its kernels stay what they were.
template <int T> __device__ void prod_job(const ProdArgs &a, int t, double *base, int tid)
{
    const int n = a.n, d = a.d, R = 2 * n + 1, D = d + 1;
    const size_t b = (size_t)a.first + (size_t)t;
    const int32_t *fac = a.factors + b * a.k;
    double *Ae = reinterpret_cast<double *>(a.regions + (size_t)t * prod_region_bytes(n, d)), *le = Ae + (size_t)R * D, *ue = le + R;
    int32_t *map = reinterpret_cast<int32_t *>(reinterpret_cast<unsigned char *>(Ae) + ex_rows_bytes(n, d));
    const LpSlice S(base, R, D);
    if (tid < 8) S.red[tid] = 0.0;
    team_sync<T>();
    // (d) a bad product (device arrays are not read by the host) fails and reads nothing through the bad index
    bool ok = true;
    long long total = 0;
    for (int s = 0; s < a.k && ok; ++s) {
        const int f = fac[s];
        if (f == -1) continue;
        if (f < -1 || f >= a.pieces) { ok = false; break; }
        const int lo = a.piece_row[f], hi = a.piece_row[f + 1];
        if (lo < 0 || hi < lo || hi > a.rows) ok = false;
        total += hi - lo;
    }
    if (total != n) ok = false;
    const int po = a.point ? a.point_of[b] : 0;
    if (a.point && (po < 0 || po >= a.points)) ok = false;
    int how = QPN_EX_FAILURE, row = -1, iters = 0, status = QPN_LP_FAILURE, near = 0;
    double eps = __builtin_nan("");
    if (ok) {
        // (a) the map, (b) the closure test at the product's point: a lane per product row
        const double *p = a.point ? a.point + (size_t)po * d : nullptr;
        int low = INT_MAX;
        for (int i = tid; i < n; i += T) {
            int at = 0, pr = 0;
            for (int s = 0; s < a.k; ++s) {
                const int f = fac[s];
                if (f < 0) continue;
                const int lo = a.piece_row[f], cnt = a.piece_row[f + 1] - lo;
                if (i < at + cnt) { pr = lo + (i - at); break; }
                at += cnt;
            }
            map[i] = pr;
            if (p) {
                const double *ar = a.A + (size_t)pr * d;
                double acc = 0.0;
                for (int j = 0; j < d; ++j) acc = acc + ar[j] * p[j];
                if (!(a.l[pr] - a.point_tol <= acc)) low = min(low, 2 * i);
                else if (!(acc - a.point_tol <= a.u[pr])) low = min(low, 2 * i + 1);
            }
        }
        low = team_min_int<T>(low, S.red, tid);
        if (low != INT_MAX) {
            how = QPN_EX_NOT_NEAR; row = low;
        } else {
            near = 1;
            // (c) the rows of the slack LP from the pool, as ex_job (a) writes them from its polyhedron
            for (int i = tid; i < n; i += T) {
                const int pr = map[i];
                const double *ar = a.A + (size_t)pr * d;
                for (int j = 0; j < d; ++j) { const double v = ar[j]; Ae[(size_t)j * R + i] = v; Ae[(size_t)j * R + n + i] = -v; }
                Ae[(size_t)d * R + i] = 1.0; Ae[(size_t)d * R + n + i] = 1.0;
                le[i] = a.l[pr]; le[n + i] = -a.u[pr];
                ue[i] = QINF; ue[n + i] = QINF;
                S.lam[i] = 0.0; S.lam[n + i] = 0.0;
            }
            for (int j = tid; j < D; j += T) {
                Ae[(size_t)j * R + 2 * n] = j == d ? 1.0 : 0.0;
                S.cv[j] = j == d ? 1.0 : 0.0; S.xf[j] = 0.0; S.ray[j] = 0.0;
            }
            if (tid == 0) { le[2 * n] = -a.slack_cap; ue[2 * n] = QINF; S.lam[2 * n] = 0.0; }
            team_sync<T>();
            const LpProb P = lp_prob(R, D, Ae, le, ue, a.lp);
            double obj = 0.0;
            status = lp_setup<T>(P, S, tid);
            if (!status) status = lp_finish<T>(P, S, tid, LP_COLD, &iters, &obj);
            team_sync<T>();
            const double tol = a.tol;
            how = status == QPN_LP_ITER_LIMIT ? QPN_EX_ITER_LIMIT : QPN_EX_FAILURE;
            if (status == QPN_LP_OPTIMAL) {
                eps = S.xf[d];
                if (eps > tol) {
                    how = QPN_EX_EMPTY_SLACK;
                } else if (eps > -tol) {
                    int act = INT_MAX;
                    for (int i = tid; i < n; i += T) {
                        const int pr = map[i];
                        if (a.open_hi && a.open_hi[pr] && fabs(a.u[pr]) < QINF && fabs(S.lam[n + i]) > tol) act = min(act, 2 * i + 1);
                        if (a.open_lo && a.open_lo[pr] && fabs(a.l[pr]) < QINF && fabs(S.lam[i]) > tol) act = min(act, 2 * i);
                    }
                    act = team_min_int<T>(act, S.red, tid);
                    how = act == INT_MAX ? QPN_EX_MEMBER_BAND : QPN_EX_EMPTY_OPEN;
                    if (act != INT_MAX) row = act;
                } else {
                    how = QPN_EX_MEMBER;
                }
            }
        }
    }
    const bool member = how == QPN_EX_MEMBER || how == QPN_EX_MEMBER_BAND, solved = status == QPN_LP_OPTIMAL;
    if (a.x) for (int j = tid; j < d; j += T) a.x[b * d + j] = member ? S.xf[j] : 0.0;
    if (a.lam) for (int i = tid; i < R; i += T) a.lam[b * R + i] = solved ? S.lam[i] : 0.0;
    if (tid == 0) {
        a.near[b] = (uint8_t)near;
        a.empty[b] = how == QPN_EX_EMPTY_SLACK || how == QPN_EX_EMPTY_OPEN ? 1 : 0;
        if (a.how) a.how[b] = how;
        if (a.eps) a.eps[b] = eps;
        if (a.row) a.row[b] = row;
        if (a.iters) a.iters[b] = iters;
    }
}

// ---- irredundant bounds: one team per polyhedron -----------------------------------------------------------------------------------
struct RedOut { int status, fail_row, lps, iters; };

// Polyhedron b.  The working copy of the unscaled bounds is the job's own output rows lr, ur: P.lb, P.ub point at them, so lp_check
// reads a relaxed bound as relaxed; the scaled copy is S.ls, S.us.  Row i belongs to lane i % T, which alone writes its bounds, its
// verdicts and its extremes; a barrier stands between such a write and the solve that reads it.  Every value a branch depends on is
// the same in all threads of the team (the polyhedron's own bounds, S.amx after the set-up's barriers, the status and the
// objective of a solve), so a whole team leaves together.  At most 2 r solves of max_iters steps each.
template <int T> __device__ void red_core(const RedArgs &a, const LpSlice &S, int b, int tid, RedOut &o)
{
    const int r = a.r, d = a.d;
    const double *l = a.l + (size_t)b * r, *u = a.u + (size_t)b * r;
    double *lr = a.lr + (size_t)b * r, *ur = a.ur + (size_t)b * r;
    int32_t *how = a.how ? a.how + (size_t)b * r * 2 : nullptr;
    double *ext = a.ext ? a.ext + (size_t)b * r * 2 : nullptr;
    const LpProb P = lp_prob(r, d, a.A + (size_t)b * r * d, lr, ur, a.lp);
    const double tol = a.tol;
    // (0) the working bounds; crossed bounds: no LP is started
    int uncrossed = 1;
    for (int i = tid; i < r; i += T) {
        const double li = l[i], ui = u[i];
        if (li > ui) uncrossed = 0;
        lr[i] = li; ur[i] = ui;
        if (how) { how[2 * i] = QPN_RED_UNDECIDED; how[2 * i + 1] = QPN_RED_UNDECIDED; }
        if (ext) { ext[2 * i] = __builtin_nan(""); ext[2 * i + 1] = __builtin_nan(""); }
    }
    if (!team_min_int<T>(uncrossed, S.red, tid)) { o.status = QPN_IB_EMPTY; return; }
    // (a) the feasibility solve
    int it;
    o.lps = 1;
    int status = lp_feasible<T>(P, S, tid, &it);
    o.iters = it;
    if (status != QPN_LP_OPTIMAL) {
        o.status = status == QPN_LP_INFEASIBLE ? QPN_IB_EMPTY : status == QPN_LP_ITER_LIMIT ? QPN_IB_ITER_LIMIT : QPN_IB_FAILURE;
        return;
    }
    // (b) the rows from the last, the lower bound before the upper
    for (int i = r - 1; i >= 0; --i) {
        const double li = l[i], ui = u[i];
        const bool mine = i % T == tid;                   // this lane owns the row
        if (li == ui) {
            if (mine && how) { how[2 * i] = QPN_RED_KEPT_EQUALITY; how[2 * i + 1] = QPN_RED_KEPT_EQUALITY; }
            continue;
        }
        if (S.amx[i] == 0.0) {                            // (a) has shown 0 within its bounds
            team_sync<T>();
            if (mine) {
                lr[i] = -QINF; ur[i] = QINF; S.ls[i] = -QINF; S.us[i] = QINF;
                if (how) { how[2 * i] = QPN_RED_REMOVED_ZERO_ROW; how[2 * i + 1] = QPN_RED_REMOVED_ZERO_ROW; }
            }
            continue;
        }
        for (int side = 0; side < 2; ++side) {
            const double bound = side ? ui : li;
            if (!(fabs(bound) < QINF)) {
                if (mine && how) how[2 * i + side] = QPN_RED_NONE;
                continue;
            }
            // the bound leaves the working bounds, its row is the objective
            team_sync<T>();
            if (mine) {
                if (side) { ur[i] = QINF; S.us[i] = QINF; } else { lr[i] = -QINF; S.ls[i] = -QINF; }
            }
            for (int j = tid; j < d; j += T) { const double v = P.Ab[(size_t)j * r + i]; S.cv[j] = side ? -v : v; }
            team_sync<T>();
            double obj;
            ++o.lps;
            status = lp_resolve<T>(P, S, tid, &it, &obj);
            o.iters += it;
            if (status == QPN_LP_ITER_LIMIT) { o.status = QPN_IB_ITER_LIMIT; o.fail_row = i; return; }
            if (status == QPN_LP_FAILURE) { o.status = QPN_IB_FAILURE; o.fail_row = i; return; }
            // (c) the verdict
            const double margin = tol * fmax(1.0, fabs(bound));
            double e;
            int verdict;
            if (status == QPN_LP_UNBOUNDED) {
                e = side ? QINF : -QINF;
                verdict = QPN_RED_KEPT_UNBOUNDED;
            } else {
                e = side ? -obj : obj;
                const bool beyond = side ? e > bound + margin : e < bound - margin;
                verdict = beyond ? QPN_RED_KEPT_BY_OPTIMUM : QPN_RED_REMOVED;
            }
            if (mine) {
                if (ext) ext[2 * i + side] = e;
                if (how) how[2 * i + side] = verdict;
            }
            if (verdict == QPN_RED_REMOVED) continue;
            // (d) a kept bound comes back; a nonbasic s_i outside it takes its value
            const double v = bound * S.sc[i];
            team_sync<T>();
            if (mine) {
                if (side) { ur[i] = bound; S.us[i] = v; } else { lr[i] = bound; S.ls[i] = v; }
            }
            for (int j = tid; j < d; j += T)
                if (S.cn[j] == d + i && (side ? S.xn[j] > v : S.xn[j] < v)) S.xn[j] = v;
        }
    }
    o.status = QPN_IB_OK;
}

template <int T> __device__ void red_job(const RedArgs &a, int b, double *base, int tid)
{
    const int r = a.r;
    const LpSlice S(base, r, a.d);
    if (tid < 8) S.red[tid] = 0.0;
    team_sync<T>();
    RedOut o{QPN_IB_FAILURE, -1, 0, 0};
    red_core<T>(a, S, b, tid, o);
    if (o.status != QPN_IB_OK) {                          // (e) the input back; a removal is no verdict any more (a lane's own rows)
        for (int i = tid; i < r; i += T) {
            a.lr[(size_t)b * r + i] = a.l[(size_t)b * r + i]; a.ur[(size_t)b * r + i] = a.u[(size_t)b * r + i];
            if (a.how)
                for (int side = 0; side < 2; ++side) {
                    int32_t *h = a.how + ((size_t)b * r + i) * 2 + side;
                    if (*h == QPN_RED_REMOVED || *h == QPN_RED_REMOVED_ZERO_ROW) *h = QPN_RED_UNDECIDED;
                }
        }
    }
    if (tid == 0) {
        a.status[b] = o.status;
        if (a.fail_row) a.fail_row[b] = o.fail_row;
        if (a.lps) a.lps[b] = o.lps;
        if (a.iters) a.iters[b] = o.iters;
    }
}

// ---- the kernels and the launcher of every job kind ------------------------------------------------------------------------------
// A job kind names its argument struct and runs job t of it with a team of T threads on the slice at base.
struct LpJob {
    using Args = LpArgs;
    template <int T> static __device__ void run(const Args &a, int t, double *base, int tid) { lp_job<T>(a, t, base, tid); }
};
struct SubsetJob {
    using Args = SubsetArgs;
    template <int T> static __device__ void run(const Args &a, int t, double *base, int tid) { subset_job<T>(a, t, base, tid); }
};
struct IbJob {
    using Args = IbArgs;
    template <int T> static __device__ void run(const Args &a, int t, double *base, int tid) { ib_job<T>(a, t, base, tid); }
};
struct ExJob {
    using Args = ExArgs;
    template <int T> static __device__ void run(const Args &a, int t, double *base, int tid) { ex_job<T>(a, t, base, tid); }
};
struct ProdJob {
    using Args = ProdArgs;
    template <int T> static __device__ void run(const Args &a, int t, double *base, int tid) { prod_job<T>(a, t, base, tid); }
};
struct RedJob {
    using Args = RedArgs;
    template <int T> static __device__ void run(const Args &a, int t, double *base, int tid) { red_job<T>(a, t, base, tid); }
};

template <class Job> __global__ __launch_bounds__(64 * LP_WAVES) void lp_wave_kernel(typename Job::Args a, int32_t count, size_t slice)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lp_lds[];
    const int w = threadIdx.x / 64;
    const long long t = (long long)blockIdx.x * LP_WAVES + w;
    if (t >= count) return;                               // a whole wavefront leaves: the others never wait for it
    Job::template run<64>(a, (int)t, reinterpret_cast<double *>(lp_lds + (size_t)w * slice), threadIdx.x % 64);
}

template <class Job, bool LDS>
__global__ __launch_bounds__(LP_GROUP) void lp_group_kernel(typename Job::Args a, int32_t first, unsigned char *gws, size_t slice)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lp_lds[];
    unsigned char *base = LDS ? lp_lds : gws + (size_t)blockIdx.x * slice;
    Job::template run<LP_GROUP>(a, first + (int)blockIdx.x, reinterpret_cast<double *>(base), threadIdx.x);
}

int32_t lp_chunk(int32_t jobs, int32_t r, int32_t d)
{
    size_t c = LP_WS_CHUNK_BYTES / lp_slice_bytes(r, d);
    if (c < 1) c = 1;
    return (int32_t)(c < (size_t)jobs ? c : (size_t)jobs);
}

// `count` jobs of one kind over LPs of r rows in d variables, by the class of their slice; gws: qpn_lp_workspace_bytes(count, r, d)
template <class Job> hipError_t lp_launch(const typename Job::Args &a, int32_t count, int32_t r, int32_t d, void *gws, hipStream_t s)
{
    if (count <= 0) return hipSuccess;
    const int cls = qpn_lp_class(r, d);
    const size_t slice = lp_slice_bytes(r, d);
    if (cls < 2) {                                        // (4 slices of 16 KiB: at the 64 KiB default, raised for clarity)
        static QpnLdsLimits lds_limits;
        if (const hipError_t e = lds_limits.raise({{lp_wave_kernel<Job>, (int)(LP_WAVE_SLICE_MAX * LP_WAVES)},
                                                   {lp_group_kernel<Job, true>, (int)LP_GROUP_SLICE_MAX}});
            e != hipSuccess)
            return e;
    }
    if (cls == 0) {
        const unsigned grid = (unsigned)((count + LP_WAVES - 1) / LP_WAVES);
        hipLaunchKernelGGL(lp_wave_kernel<Job>, dim3(grid), dim3(64 * LP_WAVES), slice * LP_WAVES, s, a, count, slice);
        return hipGetLastError();
    }
    if (cls == 1) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(lp_group_kernel<Job, true>), dim3((unsigned)count), dim3(LP_GROUP), slice, s, a, 0,
                           static_cast<unsigned char *>(nullptr), slice);
        return hipGetLastError();
    }
    const int32_t chunk = lp_chunk(count, r, d);
    for (int32_t first = 0; first < count; first += chunk) {
        const int32_t n = count - first < chunk ? count - first : chunk;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(lp_group_kernel<Job, false>), dim3((unsigned)n), dim3(LP_GROUP), 0, s, a, first,
                           static_cast<unsigned char *>(gws), slice);
        if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

// What a job that writes the rows of its own LP (R rows in D variables) takes of the workspace: its region of `region` bytes and, in
// the workspace class, its slice; and the jobs of a launch
size_t region_job_bytes(size_t region, int32_t R, int32_t D) { return region + (qpn_lp_class(R, D) == 2 ? lp_slice_bytes(R, D) : 0); }
int32_t region_chunk(int32_t jobs, size_t job_bytes)
{
    size_t c = LP_WS_CHUNK_BYTES / job_bytes;
    if (c < 1) c = 1;
    return (int32_t)(c < (size_t)jobs ? c : (size_t)jobs);
}

// The workspace holds the slices of a chunk's jobs (workspace class), then their regions; a chunk is one launch of lp_launch (at most
// lp_chunk jobs, as a job takes more than its slice), and the chunks of a call follow one another on the stream.  first, regions: the
// members of the argument struct that tell a launch its first job and where the regions start.
template <class Job>
hipError_t lp_launch_regions(typename Job::Args a, int32_t Job::Args::*first, unsigned char *Job::Args::*regions, int32_t jobs, int32_t R,
                             int32_t D, size_t region, void *gws, hipStream_t s)
{
    if (jobs <= 0) return hipSuccess;
    const int32_t chunk = region_chunk(jobs, region_job_bytes(region, R, D));
    a.*regions = static_cast<unsigned char *>(gws) + (qpn_lp_class(R, D) == 2 ? (size_t)chunk * lp_slice_bytes(R, D) : 0);
    for (int32_t f = 0; f < jobs; f += chunk) {
        a.*first = f;
        const int32_t count = jobs - f < chunk ? jobs - f : chunk;
        if (const hipError_t e = lp_launch<Job>(a, count, R, D, gws, s); e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace

int qpn_lp_class(int32_t r, int32_t d)
{
    if (r <= 0 || d <= 0 || r > QPN_LP_MAX_R || d > QPN_LP_MAX_D) return -1;
    const size_t b = lp_slice_bytes(r, d);
    return b <= LP_WAVE_SLICE_MAX ? 0 : b <= LP_GROUP_SLICE_MAX ? 1 : 2;
}

size_t qpn_lp_workspace_bytes(int32_t jobs, int32_t r, int32_t d)
{
    if (jobs <= 0 || qpn_lp_class(r, d) != 2) return 0;
    return (size_t)lp_chunk(jobs, r, d) * lp_slice_bytes(r, d);
}

hipError_t qpn_launch_solve_lps(const LpArgs &a, void *gws, hipStream_t s) { return lp_launch<LpJob>(a, a.jobs, a.r, a.d, gws, s); }
hipError_t qpn_launch_issubset_pairs(const SubsetArgs &a, void *gws, hipStream_t s) { return lp_launch<SubsetJob>(a, a.pairs, a.r1, a.d, gws, s); }
hipError_t qpn_launch_implicit_bounds(const IbArgs &a, void *gws, hipStream_t s) { return lp_launch<IbJob>(a, a.polys, a.r, a.d, gws, s); }
hipError_t qpn_launch_irredundant_bounds(const RedArgs &a, void *gws, hipStream_t s) { return lp_launch<RedJob>(a, a.polys, a.r, a.d, gws, s); }

size_t qpn_exemplar_workspace_bytes(int32_t polys, int32_t n, int32_t d)
{
    if (polys <= 0 || qpn_lp_class(2 * n + 1, d + 1) < 0) return 0;
    const size_t job = region_job_bytes(ex_rows_bytes(n, d), 2 * n + 1, d + 1);
    return (size_t)region_chunk(polys, job) * job;
}

hipError_t qpn_launch_exemplar_polys(const ExArgs &a, void *gws, hipStream_t s)
{
    return lp_launch_regions<ExJob>(a, &ExArgs::first, &ExArgs::rows, a.polys, 2 * a.n + 1, a.d + 1, ex_rows_bytes(a.n, a.d), gws, s);
}

size_t qpn_products_workspace_bytes(int32_t products, int32_t n, int32_t d)
{
    if (products <= 0 || qpn_lp_class(2 * n + 1, d + 1) < 0) return 0;
    const size_t job = region_job_bytes(prod_region_bytes(n, d), 2 * n + 1, d + 1);
    return (size_t)region_chunk(products, job) * job;
}

hipError_t qpn_launch_exemplar_products(const ProdArgs &a, void *gws, hipStream_t s)
{
    return lp_launch_regions<ProdJob>(a, &ProdArgs::first, &ProdArgs::regions, a.products, 2 * a.n + 1, a.d + 1,
                                      prod_region_bytes(a.n, a.d), gws, s);
}
