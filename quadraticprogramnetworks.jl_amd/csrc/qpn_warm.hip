// qpn_warm.hip -- warm start of the n, m <= 32 node solve from a hinted active set (QPN_AVI_FLAG_WARM_DUALS, gfx950).
//
// The outer loop sweeps the same nodes again and again; between two sweeps only w moves and a node's active set usually
// does not.  The multiplier part of the incoming z names a set: side_i = +1 where lambda_i > 0 (row i at l_i), -1 where
// lambda_i < 0 (at u_i), 0 otherwise.  One wavefront per node solves the LINEAR KKT system of the k hinted rows,
//     [[Qd, -A_act'], [A_act, 0]] [x; lam_act] = [-(qd + R w); bound_act - B_act w],      every other multiplier 0,
// in fp64 by block elimination:
//   1. T = [Qd | A_act' | -(qd + R w)]  (n x (n + k + 1), LDS, row stride 65) is reduced by Gaussian elimination with partial
//      pivoting on its first n columns (Qd may be non-symmetric), a lane per column; back-substitution, a lane per right-hand
//      column, leaves W = Qd^-1 A_act' and h = -Qd^-1 (qd + R w) in place;
//   2. S = A_act W (k x k) and c = bound_act - B_act w - A_act h go where Qd's factors were (they are dead) and are solved by
//      the same elimination: S lam_act = c;   x = h + W lam_act.
// The point then takes the post-check, the residual and the active-set classification every solver kernel applies
// (QPN_ROW_POSTCHECK, qpn_internal.h: check_tol, comp_tol) on the ORIGINAL blocks.  A node is ACCEPTED only if every hinted row has a finite
// bound on its side, k <= n, no pivot of the two eliminations is below piv_tol, every lam_act carries its side's sign and the
// post-check passes; it then writes z, status = QPN_SUCCESS, resid, pivots = 0, active and the x scatter.  Every other node
// (a NaN or an infinity among the hinted multipliers included) DECLINES: it writes none of its outputs and appends its index
// to the decliners' list, which the cold route then takes as its order array (qpn_capi.hip).
//
// The workgroup IS one wavefront: wave_sync (qpn_internal.h) orders its LDS accesses, no s_barrier needed.  26 KB of LDS: six
// wavefronts per CU.
#include "qpn_internal.h"

namespace {

constexpr int TS = 65;      // row stride of T: 32 + 32 + 1 columns (odd: a column's rows fall into distinct banks)
constexpr int AS = 33;      // column stride of the staged Ad

__global__ __launch_bounds__(WAVE) void warm_nodes(AviBatchArgs a, int32_t *dec_list, int32_t *dec_count)
{
    typedef const AviBatchArgs __attribute__((address_space(4))) *kargs;
    const kargs kp = (kargs)__builtin_amdgcn_kernarg_segment_ptr();    // (the mirrors are indexed there, not in a private copy)
    const int l = threadIdx.x;
    int b = blockIdx.x;
    // the schedule of the cold launch this one precedes: a bad entry leaves the slot unsolved there, and here
    if (a.order) { b = a.order[blockIdx.x]; if ((unsigned)b >= (unsigned)a.batch) return; }
    const int n = a.nd.n, m = a.nd.m, np_ = a.nd.p, N = n + m;

    __shared__ double T[32 * TS];       // [Qd | A_act' | rhs], later [S | W | h]
    __shared__ double sA[32 * AS];      // Ad: row i, column j at j * AS + i
    __shared__ double sq[64];           // q = [qd + R w; B w] in item order
    __shared__ double sv[64];           // right-hand side / solution of the Schur system; then z in item order
    __shared__ int srow[32];            // the hinted rows, ascending

    auto decline = [&]() { if (l == 0) qpn_decline_warm(dec_list, dec_count, b); };

    const size_t vo = (size_t)b * (size_t)N;
    const double *Q_ = a.nd.Qd + (size_t)b * n * n;
    const double *A_ = a.nd.Ad + (size_t)b * m * n;
    const double *R_ = a.nd.R + (size_t)b * n * np_;
    const double *B_ = a.nd.B + (size_t)b * m * np_;
    const double *w_ = a.nd.w + (size_t)b * (size_t)a.nd.stride_w;
    const bool act = l < N, isx = l < n;
    const int row = isx ? 0 : (act ? l - n : 0);       // constraint row of lanes n .. N-1

    // ---- the hint ---------------------------------------------------------------------------------------------------
    double lk = -QINF, uk = QINF, lam0 = 0.0;
    if (act && !isx) { lk = a.nd.l[(size_t)b * m + row]; uk = a.nd.u[(size_t)b * m + row]; lam0 = a.z[vo + l]; }
    const int side = lam0 > 0.0 ? 1 : (lam0 < 0.0 ? -1 : 0);
    const bool hinted = side != 0;
    const double bnd = side > 0 ? lk : uk;
    // a NaN or an infinity among the multipliers; a hinted side without a finite bound
    if (qpn_ballot(!(fabs(lam0) < QINF) || (hinted && !(fabs(bnd) < QINF))) != 0ull) { decline(); return; }
    const unsigned long long hmask = qpn_ballot(hinted) >> n;                       // bit i: row i is hinted
    const int k = __popcll(hmask);
    if (k > n) { decline(); return; }
    const int rank = __popcll(hmask & ((1ull << row) - 1ull));
    if (hinted) srow[rank] = row;

    // ---- q, Ad and Qd -------------------------------------------------------------------------------------------------
    if (act) {
        const double *col = isx ? R_ + l : B_ + row;
        const size_t cs = isx ? (size_t)n : (size_t)m;
        double s = isx ? a.nd.qd[(size_t)b * n + l] : 0.0;
        for (int t = 0; t < np_; ++t) s = fma(col[(size_t)t * cs], w_[t], s);
        sq[l] = s;
    }
    for (int e = l; e < m * n; e += WAVE) { const int j = e / m, i = e - j * m; sA[j * AS + i] = A_[e]; }
    for (int e = l; e < n * n; e += WAVE) { const int j = e / n, i = e - j * n; T[i * TS + j] = Q_[e]; }
    wave_sync();
    const int Wd = n + k + 1;
    for (int e = l; e < n * k; e += WAVE) { const int i = e / k, c = e - i * k; T[i * TS + n + c] = sA[i * AS + srow[c]]; }
    if (isx) T[l * TS + n + k] = -sq[l];
    wave_sync();

    const double ptol = a.piv_tol;
    // ---- 1. elimination on the first n columns (partial pivoting), a lane per column ---------------------------------
    for (int j = 0; j < n; ++j) {
        const double v = (l >= j && l < n) ? fabs(T[l * TS + j]) : -1.0;
        const double best = wave_max_f64(v);
        if (!(best >= ptol)) { decline(); return; }
        const int pr = wave_first(v == best);
        if (pr != j) {
            for (int c = j + l; c < Wd; c += WAVE) { const double t0 = T[j * TS + c]; T[j * TS + c] = T[pr * TS + c]; T[pr * TS + c] = t0; }
            wave_sync();
        }
        const double rp = 1.0 / T[j * TS + j];
        const int c = j + 1 + l;                        // (at most 64 columns lie right of column j)
        if (c < Wd) {
            const double tj = T[j * TS + c];
            for (int i = j + 1; i < n; ++i) T[i * TS + c] = fma(-(T[i * TS + j] * rp), tj, T[i * TS + c]);
        }
        wave_sync();
    }
    // back-substitution: lane c takes the right-hand column n + c (the k columns of A_act' and the rhs)
    if (l <= k) {
        const int c = n + l;
        for (int i = n - 1; i >= 0; --i) {
            double s = T[i * TS + c];
            for (int j = i + 1; j < n; ++j) s = fma(-T[i * TS + j], T[j * TS + c], s);
            T[i * TS + c] = s / T[i * TS + i];
        }
    }
    wave_sync();

    // ---- 2. S = A_act W, c = bound_act - B_act w - A_act h; S lam_act = c --------------------------------------------
    if (!isx && hinted) sv[32 + rank] = bnd - sq[l];
    wave_sync();
    for (int e = l; e < k * (k + 1); e += WAVE) {
        const int r = e / (k + 1), c = e - r * (k + 1);
        const int ar = srow[r];
        double s = 0.0;
        for (int i = 0; i < n; ++i) s = fma(sA[i * AS + ar], T[i * TS + n + c], s);
        if (c < k) T[r * TS + c] = s;                   // (columns < k <= n: the dead factors of Qd)
        else sv[r] = sv[32 + r] - s;
    }
    wave_sync();
    for (int j = 0; j < k; ++j) {
        const double v = (l >= j && l < k) ? fabs(T[l * TS + j]) : -1.0;
        const double best = wave_max_f64(v);
        if (!(best >= ptol)) { decline(); return; }
        const int pr = wave_first(v == best);
        if (pr != j) {
            const int c = j + l;
            if (c < k) { const double t0 = T[j * TS + c]; T[j * TS + c] = T[pr * TS + c]; T[pr * TS + c] = t0; }
            else if (c == k) { const double t0 = sv[j]; sv[j] = sv[pr]; sv[pr] = t0; }
            wave_sync();
        }
        const double rp = 1.0 / T[j * TS + j];
        const int c = j + 1 + l;
        if (c < k) {
            const double tj = T[j * TS + c];
            for (int i = j + 1; i < k; ++i) T[i * TS + c] = fma(-(T[i * TS + j] * rp), tj, T[i * TS + c]);
        } else if (c == k) {
            const double tj = sv[j];
            for (int i = j + 1; i < k; ++i) sv[i] = fma(-(T[i * TS + j] * rp), tj, sv[i]);
        }
        wave_sync();
    }
    for (int i = k - 1; i >= 0; --i) {
        const double li = sv[i] / T[i * TS + i];
        wave_sync();
        if (l < i) sv[l] = fma(-T[l * TS + i], li, sv[l]);
        else if (l == i) sv[l] = li;
        wave_sync();
    }

    // ---- the point: x = h + W lam_act, the hinted multipliers, zeros elsewhere ---------------------------------------
    double zk = 0.0;
    if (isx) {
        zk = T[l * TS + n + k];
        for (int c = 0; c < k; ++c) zk = fma(T[l * TS + n + c], sv[c], zk);
    } else if (hinted) zk = sv[rank];
    // every multiplier of the hint carries its side's sign (a NaN does not)
    if (qpn_ballot(hinted && !(zk * (double)side > 0.0)) != 0ull) { decline(); return; }
    wave_sync();
    if (act) sv[l] = zk;
    wave_sync();

    // ---- post-check against the ORIGINAL blocks: QPN_ROW_POSTCHECK (src/avi.jl:71-76 / :148-156) ------------------------
    double rk = 0.0;
    if (act) {
        rk = sq[l];
        if (isx) {
            for (int j = 0; j < n; ++j) rk = fma(Q_[(size_t)j * n + l], sv[j], rk);        // lane <-> row: coalesced
            for (int i = 0; i < m; ++i) rk = fma(-sA[l * AS + i], sv[n + i], rk);          // -Ad'
        } else {
            for (int j = 0; j < n; ++j) rk = fma(sA[j * AS + row], sv[j], rk);
        }
    }
    const int gk = isx ? 0 : 1;
    const double pp = gk ? rk : zk, dv = gk ? zk : rk;
    int bad = 0;
    double nres = 0.0;
    unsigned mask = 0;
    if (act) QPN_ROW_POSTCHECK(bad, nres, mask, pp, dv, lk, uk, gk, a.check_tol, a.comp_tol);
    if (qpn_ballot(bad != 0) != 0ull) { decline(); return; }
    nres = wave_max_f64_nc(nres);

    // ---- accepted ----------------------------------------------------------------------------------------------------
    if (act) {
        a.z[vo + l] = zk;
        if (a.x && isx) qpn_store_primal(kp, a.x, (size_t)b * (size_t)a.stride_x + l, zk);     // primal block -> the caller's iterate and its replicas
        if (a.active) a.active[vo + l] = (uint8_t)mask;
    }
    if (l == 0) {
        a.status[b] = QPN_SUCCESS;
        if (a.resid) a.resid[b] = nres;
        if (a.pivots) a.pivots[b] = 0;
    }
}

} // namespace

// a.nd set, n, m <= 32, m >= 1, a.z holds the hint; a.order (may be null) as the cold launch behind it will see it.
// dec_list: a.batch + 1 words, every one -1 (the last is the counter); on return of the launch the decliners' indices stand in
// its first words, in no particular order, the rest is still -1.
hipError_t qpn_launch_warm_nodes(const AviBatchArgs &a, int32_t *dec_list, hipStream_t stream)
{
    if (a.batch <= 0) return hipSuccess;
    hipLaunchKernelGGL(warm_nodes, dim3((unsigned)a.batch), dim3(WAVE), 0, stream, a, dec_list, dec_list + a.batch);
    return hipGetLastError();
}
