// qpn_warm_mid.hip -- warm start of the mid-size node solves (n, m <= 128, one of them > 32) from a hinted active set, for resident
// handles that opted in (qpn_nodes_set_warm; QPN_AVI_FLAG_WARM_DUALS, gfx950).
//
// Mathematics and accept rule are those of qpn_warm.hip (the 32-class): the multiplier signs of the incoming z name k rows and
// their sides, and the LINEAR KKT system of those rows,
//     [[Qd, -A_act'], [A_act, 0]] [x; lam_act] = [-(qd + R w); bound_act - B_act w],      every other multiplier 0,
// is solved in fp64 by block elimination: W | h = Qd^-1 [A_act' | -(qd + R w)], S = A_act W, c = bound_act - B_act w - A_act h,
// S lam_act = c, x = h + W lam_act.  The point takes the post-check, the residual and the masks of QPN_ROW_POSTCHECK (qpn_internal.h) on the ORIGINAL
// blocks.  ACCEPTED: every hinted multiplier finite with a finite bound on its side, k <= n, warm_mid_fits(n, k), no pivot below
// piv_tol, every lam_act of its side's sign, post-check passed -- the node writes z, status = QPN_SUCCESS, resid, pivots = 0,
// active and the x scatter.  Every other node writes nothing but its index, appended to the decliners' list.
//
// One workgroup of 256 threads per node.  Both eliminations are Gauss-Jordan with partial pivoting (Qd may be non-symmetric;
// the pivot row is chosen among the rows not yet used and stays where it is, so no rows are exchanged) on a matrix that lives in
// REGISTERS: thread (ty, tx) = (t & 15, t >> 4) holds the entries (ty + 16 r, tx + 16 s), r < RT, s < CT.  A step sends only the
// pivot column and the pivot row through LDS (double-buffered: two barriers a step), every thread then updates its own slice;
// column tiles that are dead (left of the pivot) or beyond the matrix are skipped by wave-uniform branches.  LDS holds A_act (k x n),
// W | h (n x (k + 1)) and kWarmMidFixed bytes of vectors: warm_mid_fits (qpn_internal.h) is exactly that budget.  Every exit
// before or between barriers is decided from LDS words or ballots that all four waves read: it is uniform over the workgroup.
#include "qpn_internal.h"

namespace {

constexpr int WM_THREADS = 256;
// the fixed part of the LDS layout, in doubles from the base; the ints follow, then A_act, then W | h
constexpr int oPC = 0, oPROW = 256, oPINV = 800, oSQ = 928, oSZ = 1184, oBND = 1440, oSV = 1568, oINTS = 1696;
constexpr int iCOLOF = 0, iSROW = 128, iSRANK = 256, iSIDE = 384, iFLAG = 512, iMASK = 516, nINTS = 520;
static_assert(oINTS * 8 + nINTS * 4 == kWarmMidFixed, "warm_mid_fits counts the fixed part of this layout");

// Gauss-Jordan elimination with partial pivoting of the nr x nc matrix in `a` (pivots in its first nr columns).  On return row
// i holds, in the columns c >= nr, pivot x (component colof[i] of the solutions), and pinv[j] = 1 / pivot of column j.
// false: a pivot below ptol (every thread of the workgroup returns the same).
template <int RT, int CT>
__device__ __forceinline__ bool gauss_jordan(double (&a)[RT][CT], int nr, int nc, double ptol, double *pc, double *prow, double *pinv,
                                             int *colof, int t)
{
    const int lane = t & 63, ty = t & 15, tx = t >> 4;
    unsigned long long used0 = 0ull, used1 = 0ull;
    for (int j = 0; j < nr; ++j) {
        double *pcj = pc + (j & 1) * 128, *prj = prow + (j & 1) * 272;
        const int sj = j >> 4;
        // the pivot column, from the threads that hold it
        if (tx == (j & 15)) {
#pragma unroll
            for (int s = 0; s < CT; ++s)
                if (s == sj) {
#pragma unroll
                    for (int r = 0; r < RT; ++r) pcj[ty + 16 * r] = a[r][s];
                }
        }
        __syncthreads();
        // every wave finds the pivot among the unused rows on its own: the same numbers, the same answer
        double v0 = -1.0, v1 = -1.0;
        if (lane < nr && !((used0 >> lane) & 1ull)) v0 = fabs(pcj[lane]);
        if (lane + 64 < nr && !((used1 >> lane) & 1ull)) v1 = fabs(pcj[lane + 64]);
        const double best = wave_max_f64(fmax(v0, v1));
        const unsigned long long b0 = qpn_ballot(v0 == best), b1 = qpn_ballot(v1 == best);
        if (!(best >= ptol) || (b0 | b1) == 0ull) return false;
        const int pr = b0 ? __ffsll((long long)b0) - 1 : 64 + __ffsll((long long)b1) - 1;
        if (pr < 64) used0 |= 1ull << pr; else used1 |= 1ull << (pr - 64);
        // the pivot row, from the threads that hold it
        const int rj = pr >> 4;
        if (ty == (pr & 15)) {
#pragma unroll
            for (int r = 0; r < RT; ++r)
                if (r == rj) {
#pragma unroll
                    for (int s = 0; s < CT; ++s) prj[tx + 16 * s] = a[r][s];
                }
        }
        const double ri = 1.0 / pcj[pr];
        if (t == 0) { colof[pr] = j; pinv[j] = ri; }
        __syncthreads();
        // (one branch per column tile; a row tile beyond the matrix costs its FMAs, which is less than a branch per tile)
        double f[RT];
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int i = ty + 16 * r;
            f[r] = (i == pr || i >= nr) ? 0.0 : -(pcj[i] * ri);
        }
#pragma unroll
        for (int s = 0; s < CT; ++s)
            if (16 * s + 15 > j && 16 * s < nc) {
                const double pv = prj[tx + 16 * s];
#pragma unroll
                for (int r = 0; r < RT; ++r) a[r][s] = fma(f[r], pv, a[r][s]);
            }
    }
    return true;
}

template <int RT, int CT>
__global__ __launch_bounds__(WM_THREADS) void warm_mid_nodes(AviBatchArgs a, int32_t *dec_list, int32_t *dec_count)
{
    typedef const AviBatchArgs __attribute__((address_space(4))) *kargs;
    const kargs kp = (kargs)__builtin_amdgcn_kernarg_segment_ptr();    // (the mirrors are indexed there, not in a private copy)
    extern __shared__ double lds[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, ty = t & 15, tx = t >> 4;
    int b = blockIdx.x;
    // the schedule of the cold launch this one precedes: a bad entry leaves the slot unsolved there, and here (uniform exit)
    if (a.order) { b = a.order[blockIdx.x]; if ((unsigned)b >= (unsigned)a.batch) return; }
    const int n = a.nd.n, m = a.nd.m, np_ = a.nd.p, N = n + m;

    double *pc = lds + oPC, *prow = lds + oPROW, *pinv = lds + oPINV, *sq = lds + oSQ, *sz = lds + oSZ, *sbnd = lds + oBND;
    double *sv = lds + oSV;
    int *ints = reinterpret_cast<int *>(lds + oINTS);
    int *colof = ints + iCOLOF, *srow = ints + iSROW, *srank = ints + iSRANK, *sside = ints + iSIDE, *flag = ints + iFLAG;
    unsigned long long *smask = reinterpret_cast<unsigned long long *>(ints + iMASK);

    auto decline = [&]() { if (t == 0) qpn_decline_warm(dec_list, dec_count, b); };

    const size_t vo = (size_t)b * (size_t)N;
    const double *Q_ = a.nd.Qd + (size_t)b * n * n;
    const double *A_ = a.nd.Ad + (size_t)b * m * n;
    const double *R_ = a.nd.R + (size_t)b * n * np_;
    const double *B_ = a.nd.B + (size_t)b * m * np_;
    const double *w_ = a.nd.w + (size_t)b * (size_t)a.nd.stride_w;

    // ---- the hint: thread t < m has row t ------------------------------------------------------------------------------
    if (t < 4) flag[t] = 0;
    __syncthreads();
    int side = 0;
    double bnd = 0.0;
    {
        double lam0 = 0.0, lk = -QINF, uk = QINF;
        if (t < m) { lk = a.nd.l[(size_t)b * m + t]; uk = a.nd.u[(size_t)b * m + t]; lam0 = a.z[vo + n + t]; }
        side = lam0 > 0.0 ? 1 : (lam0 < 0.0 ? -1 : 0);
        bnd = side > 0 ? lk : uk;
        // a NaN or an infinity among the multipliers; a hinted side without a finite bound
        if (!(fabs(lam0) < QINF) || (side != 0 && !(fabs(bnd) < QINF))) flag[0] = 1;
    }
    const bool hinted = side != 0;
    {
        const unsigned long long hb = qpn_ballot(hinted);                 // rows 64 wave .. 64 wave + 63 (m <= 128: waves 0, 1)
        if (lane == 0 && wave < 2) smask[wave] = hb;
    }
    __syncthreads();
    if (flag[0] != 0) { decline(); return; }
    const unsigned long long hm0 = smask[0], hm1 = smask[1];
    const int k = uni(__popcll(hm0) + __popcll(hm1));                       // (every thread read the same words: scalar from here on)
    if (k > n || !warm_mid_fits(n, k)) { decline(); return; }
    const int SA = n | 1, WS = (k + 1) | 1;
    double *sAct = lds + oINTS + nINTS / 2;                                // A_act: row r, column i at r * SA + i
    double *sW = sAct + k * SA;                                            // W | h: row i, column c at i * WS + c
    if (t < m) {
        const int rank = t < 64 ? __popcll(hm0 & ((1ull << t) - 1ull)) : __popcll(hm0) + __popcll(hm1 & ((1ull << (t - 64)) - 1ull));
        srank[t] = hinted ? rank : -1;
        if (hinted) { srow[rank] = t; sside[rank] = side; sbnd[rank] = bnd; }
    }
    // ---- q = [qd + R w; B w] in item order -------------------------------------------------------------------------------
    if (t < N) {
        const bool isx = t < n;
        const double *col = isx ? R_ + t : B_ + (t - n);
        const size_t cs = isx ? (size_t)n : (size_t)m;
        double s = isx ? a.nd.qd[(size_t)b * n + t] : 0.0;
        for (int e = 0; e < np_; ++e) s = fma(col[(size_t)e * cs], w_[e], s);
        sq[t] = s;
    }
    __syncthreads();
    // ---- A_act: the hinted rows of Ad (column-major, m rows: a column's rows are neighbours) ------------------------------
    if (k > 0) {
        const int mw = m > 64 ? 128 : 64, row = t & (mw - 1), step = WM_THREADS / mw;
        const int rk = row < m ? srank[row] : -1;
        if (rk >= 0)
            for (int i = t / mw; i < n; i += step) sAct[rk * SA + i] = A_[(size_t)i * m + row];
    }
    __syncthreads();

    // ---- 1. [Qd | A_act' | -(qd + R w)] in registers; Gauss-Jordan on its first n columns ---------------------------------
    double reg[RT][CT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        const int i = ty + 16 * r;
#pragma unroll
        for (int s = 0; s < CT; ++s) {
            const int c = tx + 16 * s;
            double v = 0.0;
            if (i < n) {
                if (c < n) v = Q_[(size_t)c * n + i];
                else if (c < n + k) v = sAct[(c - n) * SA + i];
                else if (c == n + k) v = -sq[i];
            }
            reg[r][s] = v;
        }
    }
    const double ptol = a.piv_tol;
    if (!gauss_jordan<RT, CT>(reg, n, n + k + 1, ptol, pc, prow, pinv, colof, t)) { decline(); return; }
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        const int i = ty + 16 * r;
        if (i < n) {
            const int j = colof[i];
            const double sc = pinv[j];
#pragma unroll
            for (int s = 0; s < CT; ++s) {
                const int c = tx + 16 * s - n;
                if (c >= 0 && c <= k) sW[j * WS + c] = reg[r][s] * sc;
            }
        }
    }
    __syncthreads();

    // ---- 2. [S | c] = [A_act W | bound_act - B_act w - A_act h] in registers; S lam_act = c --------------------------------
    if (k > 0) {
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int s = 0; s < CT; ++s) reg[r][s] = 0.0;
        for (int i = 0; i < n; ++i) {
            double ar[RT];
#pragma unroll
            for (int r = 0; r < RT; ++r) ar[r] = ty + 16 * r < k ? sAct[(ty + 16 * r) * SA + i] : 0.0;
#pragma unroll
            for (int s = 0; s < CT; ++s)
                if (16 * s <= k) {
                    const double wv = tx + 16 * s <= k ? sW[i * WS + tx + 16 * s] : 0.0;
#pragma unroll
                    for (int r = 0; r < RT; ++r) reg[r][s] = fma(ar[r], wv, reg[r][s]);
                }
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int rr = ty + 16 * r;
#pragma unroll
            for (int s = 0; s < CT; ++s)
                if (tx + 16 * s == k && rr < k) reg[r][s] = (sbnd[rr] - sq[n + srow[rr]]) - reg[r][s];
        }
        if (!gauss_jordan<RT, CT>(reg, k, k + 1, ptol, pc, prow, pinv, colof, t)) { decline(); return; }
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int rr = ty + 16 * r;
#pragma unroll
            for (int s = 0; s < CT; ++s)
                if (tx + 16 * s == k && rr < k) { const int j = colof[rr]; sv[j] = reg[r][s] * pinv[j]; }
        }
        __syncthreads();
    }

    // ---- the point in item order: x = h + W lam_act, the hinted multipliers, zeros elsewhere -----------------------------
    const bool act = t < N, isx = t < n;
    const int row = isx ? 0 : (act ? t - n : 0);
    double zk = 0.0;
    if (isx) {
        zk = sW[t * WS + k];
        for (int c = 0; c < k; ++c) zk = fma(sW[t * WS + c], sv[c], zk);
    } else if (act) {
        const int rk = srank[row];
        if (rk >= 0) {
            zk = sv[rk];
            // every multiplier of the hint carries its side's sign (a NaN does not)
            if (!(zk * (double)sside[rk] > 0.0)) flag[1] = 1;
        }
    }
    if (act) sz[t] = zk;
    __syncthreads();
    if (flag[1] != 0) { decline(); return; }

    // ---- post-check against the ORIGINAL blocks: QPN_ROW_POSTCHECK ------------------------------------------------------
    double rk_ = 0.0, lk = -QINF, uk = QINF;
    if (act) {
        rk_ = sq[t];
        if (isx) {
            for (int j = 0; j < n; ++j) rk_ = fma(Q_[(size_t)j * n + t], sz[j], rk_);      // thread <-> row: coalesced
            for (int r = 0; r < k; ++r) rk_ = fma(-sAct[r * SA + t], sv[r], rk_);          // -Ad' lam: the other multipliers are 0
        } else {
            lk = a.nd.l[(size_t)b * m + row]; uk = a.nd.u[(size_t)b * m + row];
            for (int j = 0; j < n; ++j) rk_ = fma(A_[(size_t)j * m + row], sz[j], rk_);
        }
    }
    const int gk = isx ? 0 : 1;
    const double pp = gk ? rk_ : zk, dv = gk ? zk : rk_;
    int bad = 0;
    double nres = 0.0;
    unsigned mask = 0;
    if (act) QPN_ROW_POSTCHECK(bad, nres, mask, pp, dv, lk, uk, gk, a.check_tol, a.comp_tol);
    if (bad != 0) flag[2] = 1;
    nres = wave_max_f64_nc(nres);
    if (lane == 0) pc[wave] = nres;                                        // (the pivot columns are dead)
    __syncthreads();
    if (flag[2] != 0) { decline(); return; }

    // ---- accepted --------------------------------------------------------------------------------------------------------
    if (act) {
        a.z[vo + t] = zk;
        if (a.x && isx) qpn_store_primal(kp, a.x, (size_t)b * (size_t)a.stride_x + t, zk);     // primal block -> the caller's iterate and its replicas
        if (a.active) a.active[vo + t] = (uint8_t)mask;
    }
    if (t == 0) {
        a.status[b] = QPN_SUCCESS;
        if (a.resid) a.resid[b] = fmax(fmax(pc[0], pc[1]), fmax(pc[2], pc[3]));
        if (a.pivots) a.pivots[b] = 0;
    }
}

// LDS of a launch: the fixed part and the largest hint of the shape that the rule admits
size_t warm_mid_lds_bytes(int n, int m)
{
    int k = n < m ? n : m;
    while (k > 0 && !warm_mid_fits(n, k)) --k;
    return (size_t)kWarmMidFixed + 8 * ((size_t)k * (size_t)(n | 1) + (size_t)n * (size_t)((k + 1) | 1));
}

} // namespace

// a.nd set, 1 <= n, m <= 128, a.z holds the hint; a.order (may be null) as the cold launch behind it will see it.
// dec_list: a.batch + 1 words, every one -1 (the last is the counter); on return of the launch the decliners' indices stand in
// its first words, in no particular order, the rest is still -1.
hipError_t qpn_launch_warm_mid_nodes(const AviBatchArgs &a, int32_t *dec_list, hipStream_t stream)
{
    if (a.batch <= 0) return hipSuccess;
    const int n = a.nd.n, m = a.nd.m;
    if (n < 1 || m < 1 || n > 128 || m > 128) return hipErrorInvalidValue;
    const size_t lds = warm_mid_lds_bytes(n, m);
    // (dynamic LDS beyond 64 KB needs the attribute, once per device and kernel)
    static QpnLdsLimits lds_limits;
    if (const hipError_t e = lds_limits.raise({{warm_mid_nodes<3, 7>, kWarmMidLds}, {warm_mid_nodes<4, 9>, kWarmMidLds},
                                               {warm_mid_nodes<6, 13>, kWarmMidLds}, {warm_mid_nodes<8, 17>, kWarmMidLds}});
        e != hipSuccess)
        return e;
    // RT row tiles hold n rows, CT column tiles the n + k + 1 <= 2 n + 1 columns
    const dim3 grid((unsigned)a.batch), block(WM_THREADS);
    if (n <= 48) hipLaunchKernelGGL((warm_mid_nodes<3, 7>), grid, block, lds, stream, a, dec_list, dec_list + a.batch);
    else if (n <= 64) hipLaunchKernelGGL((warm_mid_nodes<4, 9>), grid, block, lds, stream, a, dec_list, dec_list + a.batch);
    else if (n <= 96) hipLaunchKernelGGL((warm_mid_nodes<6, 13>), grid, block, lds, stream, a, dec_list, dec_list + a.batch);
    else hipLaunchKernelGGL((warm_mid_nodes<8, 17>), grid, block, lds, stream, a, dec_list, dec_list + a.batch);
    return hipGetLastError();
}
