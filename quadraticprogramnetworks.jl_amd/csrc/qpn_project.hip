// qpn_project.hip -- the projection of DEGENERATE solution-graph pieces onto [x_d; x_p] (qpn_project_pieces): what
// qpn_reduced_pieces flags and leaves to its caller.  One workgroup of 256 threads per piece, three stages.
//
//   1  equality elimination: reduce_pieces_kernel's column loop (qpn_pieces.hip), the same operations in the same order -- a
//      SECOND COPY of that loop, kept apart on purpose: qpn_reduced_pieces' code generation stays what its tests pin bit for
//      bit.  Where reduce_pieces_kernel raises flag bit 0 (no equality row pins the column while an alive row holds it above
//      tol), the column goes into the ascending list `left` instead.
//   2  the alive rows are compacted in their order into a scratch buffer of `cap` rows, and every column j of `left`, ascending,
//      takes one Fourier-Motzkin step from one scratch buffer into the other:
//        rows with |a_kj| <= tol come first, in order, unchanged;
//        every other row k gives up to two one-sided inequalities, in this order: (a_k, u_k) if u_k is finite, (-a_k, -l_k) if
//        l_k is finite; each is divided, entry by entry and in its bound, by |a_kj| and joins the list `ub` if its entry j is
//        > 0, the list `lb` otherwise;
//        the new rows are au + al with bounds (-inf, bu + bl), for every entry of ub (outer) against every entry of lb (inner).
//      Divisions and additions only (fp contraction off): bit-equal to the numpy restatement (avi_solutions.project_rows).
//      COUNT BEFORE WRITE: a step first counts nz + |ub| |lb| in 64 bits; beyond cap the piece gets flag bit 2, its outputs are
//      all fill, and the workgroup does nothing more for it -- no index beyond cap is ever formed.  (The lists hold at most two
//      entries per row of a buffer of at most cap rows: zl [cap], ul, ll [2 cap].)
//   3  the columns [x_d (n); x_p (p)] of the last buffer go out as Ar (cap x (n+p) column-major), lr, ur, rows, flags, with
//      qpn_reduced_pieces' fill beyond rows[t] (0, -inf, +inf).  Flag bit 0 is never set; bit 1: more than cap alive rows after
//      stage 1 (the first cap go out, no Fourier-Motzkin step is taken).
//
// Only the columns that are read again travel through stage 2: x_d, x_p and the columns of `left` still to come.  Rows are
// contiguous in the column-major buffers, so threads run along the rows of a column.
#include "qpn_internal.h"

namespace {

// exclusive prefix sums of (a, b, c) over the 256 threads, and the totals; s: 3 x 256 ints
__device__ __forceinline__ void block_scan3(int *s, int tid, int a, int b, int c, int &ea, int &eb, int &ec, int &ta, int &tb, int &tc)
{
    s[tid] = a; s[256 + tid] = b; s[512 + tid] = c;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        int va = 0, vb = 0, vc = 0;
        if (tid >= off) { va = s[tid - off]; vb = s[256 + tid - off]; vc = s[512 + tid - off]; }
        __syncthreads();
        s[tid] += va; s[256 + tid] += vb; s[512 + tid] += vc;
        __syncthreads();
    }
    ea = s[tid] - a; eb = s[256 + tid] - b; ec = s[512 + tid] - c;
    ta = s[255]; tb = s[511]; tc = s[767];
    __syncthreads();
}

// A [rows x cols] column-major in the workspace (rows = 2N, cols = N + p), lp / up / keep [rows] as local_pieces_kernel left
// them.  buf: two buffers of cap x cols doubles per piece, bnd: their bounds (l, u, l, u: 4 cap), lists: zl, ul, ll (5 cap ints).
// Dynamic LDS: l, u, the current column (rows doubles each), the pivot row (cols doubles), the output map (rows ints), `left`
// (m ints), alive flags (rows bytes), membership in `left` (m bytes).
__global__ __launch_bounds__(256) void project_pieces_kernel(int32_t n, int32_t m, int32_t p, double tol, int32_t cap, double *Ap,
                                                             const double *lp, const double *up, const uint8_t *keep, double *buf,
                                                             double *bnd, int32_t *lists, double *Ar, double *lr, double *ur,
                                                             int32_t *rows_out, int32_t *flags_out)
{
    extern __shared__ double lds[];
    const int t = blockIdx.x, tid = threadIdx.x;
    const int N = n + m, rows = 2 * N, cols = N + p;
    const size_t capz = (size_t)cap;
    double *s_l = lds, *s_u = lds + rows, *s_col = lds + 2 * rows, *s_row = lds + 3 * rows;
    int *s_map = reinterpret_cast<int *>(s_row + cols);
    int *s_left = s_map + rows;
    uint8_t *s_alive = reinterpret_cast<uint8_t *>(s_left + m);
    uint8_t *s_isleft = s_alive + rows;
    __shared__ double r_val[256];
    __shared__ int r_row[256];
    __shared__ int s_scan[3 * 256];
    __shared__ int s_any, s_cnt, s_nleft;
    double *A = Ap + (size_t)t * (size_t)rows * cols;
    for (int r = tid; r < rows; r += 256) {
        s_l[r] = lp[(size_t)t * rows + r]; s_u[r] = up[(size_t)t * rows + r]; s_alive[r] = keep[(size_t)t * rows + r];
    }
    for (int i = tid; i < m; i += 256) s_isleft[i] = 0;
    if (tid == 0) s_nleft = 0;
    __syncthreads();
    // ---- stage 1: reduce_pieces_kernel's column loop
    for (int j = n; j < N; ++j) {
        // the alive equality row with the largest |A[., j]| (the first of equal ones)
        double best = 0.0; int brow = rows; int any = 0;
        for (int r = tid; r < rows; r += 256) {
            const double v = A[(size_t)j * rows + r];
            s_col[r] = v;
            const double a = fabs(v);
            if (s_alive[r]) {
                if (a > tol) any = 1;
                const double lo = s_l[r];
                if (lo == s_u[r] && !isinf(lo) && a > best) { best = a; brow = r; }   // (rows ascend per thread: the first maximum stays)
            }
        }
        r_val[tid] = best; r_row[tid] = brow;
        if (tid == 0) s_any = 0;
        __syncthreads();
        if (any) s_any = 1;                                          // (benign race: every writer stores 1)
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) {
                const double v2 = r_val[tid + s]; const int w2 = r_row[tid + s];
                if (v2 > r_val[tid] || (v2 == r_val[tid] && w2 < r_row[tid])) { r_val[tid] = v2; r_row[tid] = w2; }
            }
            __syncthreads();
        }
        const double bestv = r_val[0];
        const int i = r_row[0];
        if (!(bestv > tol)) {                                        // no equality pins lambda_j: Fourier-Motzkin's, if a row holds it
            if (tid == 0 && s_any) { s_left[s_nleft++] = j; s_isleft[j - n] = 1; }
            __syncthreads();
            continue;
        }
        for (int c = tid; c < cols; c += 256) s_row[c] = A[(size_t)c * rows + i];
        __syncthreads();
        const double piv = s_col[i], li = s_l[i], ui = s_u[i];
        for (int k = tid; k < rows; k += 256) {
            if (k == i || !s_alive[k]) continue;
            const double akj = s_col[k];
            if (akj == 0.0) continue;
            const double f = akj / piv;
            for (int c = 0; c < cols; ++c) {
                const double prod = f * s_row[c];
                A[(size_t)c * rows + k] = A[(size_t)c * rows + k] - prod;
            }
            A[(size_t)j * rows + k] = 0.0;
            const double pl = f * li, pu = f * ui;
            s_l[k] = s_l[k] - pl; s_u[k] = s_u[k] - pu;
        }
        __syncthreads();
        if (tid == 0) s_alive[i] = 0;
        __syncthreads();
    }
    // ---- stage 2: the alive rows, in order, into the first scratch buffer
    if (tid == 0) {
        int cnt = 0;
        for (int r = 0; r < rows; ++r) s_map[r] = s_alive[r] ? cnt++ : -1;
        s_cnt = cnt;
    }
    __syncthreads();
    const int nleft = s_nleft;
    int flag = 0, R = s_cnt;
    if (R > cap) { flag = 2; R = cap; }
    double *src = buf + (size_t)t * 2 * capz * cols, *dst = src + capz * cols;
    double *sl = bnd + (size_t)t * 4 * capz, *su = sl + capz, *dl = su + capz, *du = dl + capz;
    int32_t *zl = lists + (size_t)t * 5 * capz, *ul = zl + capz, *ll = ul + 2 * capz;
    for (int c = 0; c < cols; ++c) {
        if (c >= n && c < N && !s_isleft[c - n]) continue;
        for (int r = tid; r < rows; r += 256) {
            const int o = s_map[r];
            if (o >= 0 && o < cap) src[(size_t)c * capz + o] = A[(size_t)c * rows + r];
        }
    }
    for (int r = tid; r < rows; r += 256) {
        const int o = s_map[r];
        if (o >= 0 && o < cap) { sl[o] = s_l[r]; su[o] = s_u[r]; }
    }
    __syncthreads();
    // ---- one Fourier-Motzkin step per column of `left`
    for (int q = 0; q < nleft && flag == 0; ++q) {
        const int j = s_left[q];
        const double *colj = src + (size_t)j * capz;
        int nz = 0, nu = 0, nl = 0;
        for (int r0 = 0; r0 < R; r0 += 256) {                        // (R <= cap: every list index below stays inside its list)
            const int r = r0 + tid;
            int fz = 0, s0 = 0, s1 = 0;                              // s0, s1: where (a, u) and (-a, -l) go -- 0 nowhere, 1 ub, 2 lb
            if (r < R) {
                const double a = colj[r];
                if (fabs(a) <= tol) fz = 1;
                else {
                    if (isfinite(su[r])) s0 = a > 0.0 ? 1 : 2;
                    if (isfinite(sl[r])) s1 = -a > 0.0 ? 1 : 2;
                }
            }
            const int fu = (s0 == 1) + (s1 == 1), fl = (s0 == 2) + (s1 == 2);
            int ez, eu, el, tz, tu, tl;
            block_scan3(s_scan, tid, fz, fu, fl, ez, eu, el, tz, tu, tl);
            if (fz) zl[nz + ez] = r;
            if (s0 == 1) ul[nu + eu] = 2 * r;
            if (s1 == 1) ul[nu + eu + (s0 == 1)] = 2 * r + 1;
            if (s0 == 2) ll[nl + el] = 2 * r;
            if (s1 == 2) ll[nl + el + (s0 == 2)] = 2 * r + 1;
            nz += tz; nu += tu; nl += tl;
        }
        __syncthreads();
        // count before write
        const long long tot = (long long)nz + (long long)nu * (long long)nl;
        if (tot > (long long)cap) { flag = 4; break; }
        const int P = (int)(tot - nz);
        for (int c = 0; c < cols; ++c) {
            if (c >= n && c < N && !(s_isleft[c - n] && c > j)) continue;     // (column j itself is 0 from here on, and never read again)
            const double *sc = src + (size_t)c * capz;
            double *dc = dst + (size_t)c * capz;
            for (int o = tid; o < nz; o += 256) dc[o] = sc[zl[o]];
            for (int o = tid; o < P; o += 256) {
                const int ia = o / nl, ib = o - ia * nl;
                const int eu = ul[ia], el = ll[ib], ku = eu >> 1, kl = el >> 1;
                double xu = sc[ku], xl = sc[kl];
                if (eu & 1) xu = -xu;
                if (el & 1) xl = -xl;
                const double au = xu / fabs(colj[ku]), al = xl / fabs(colj[kl]);
                dc[nz + o] = au + al;
            }
        }
        for (int o = tid; o < nz; o += 256) { dl[o] = sl[zl[o]]; du[o] = su[zl[o]]; }
        for (int o = tid; o < P; o += 256) {
            const int ia = o / nl, ib = o - ia * nl;
            const int eu = ul[ia], el = ll[ib], ku = eu >> 1, kl = el >> 1;
            const double xu = (eu & 1) ? -sl[ku] : su[ku], xl = (el & 1) ? -sl[kl] : su[kl];
            const double bu = xu / fabs(colj[ku]), bl = xl / fabs(colj[kl]);
            dl[nz + o] = -QINF; du[nz + o] = bu + bl;
        }
        R = (int)tot;
        { double *x = src; src = dst; dst = x; x = sl; sl = dl; dl = x; x = su; su = du; du = x; }
        __syncthreads();
    }
    // ---- stage 3: the columns [x_d (n); x_p (p)]
    const int cnt = (flag & 4) ? 0 : R;
    double *Ao = Ar + (size_t)t * (size_t)(n + p) * capz;
    for (int c = 0; c < n + p; ++c) {
        const int cs = c < n ? c : c + m;
        for (int o = tid; o < cnt; o += 256) Ao[(size_t)c * capz + o] = src[(size_t)cs * capz + o];
        for (int o = cnt + tid; o < cap; o += 256) Ao[(size_t)c * capz + o] = 0.0;
    }
    for (int o = tid; o < cnt; o += 256) { lr[(size_t)t * capz + o] = sl[o]; ur[(size_t)t * capz + o] = su[o]; }
    for (int o = cnt + tid; o < cap; o += 256) { lr[(size_t)t * capz + o] = -QINF; ur[(size_t)t * capz + o] = QINF; }
    if (tid == 0) { rows_out[t] = cnt; flags_out[t] = flag; }
}

} // namespace

size_t qpn_project_pieces_lds(int32_t n, int32_t m, int32_t p)
{
    const size_t N = (size_t)n + m, rows = 2 * N, cols = N + p;
    return (3 * rows + cols) * sizeof(double) + (rows + (size_t)m) * sizeof(int) + ((rows + (size_t)m + 7) & ~(size_t)7);
}

// scratch of one piece besides its local piece, in bytes: the two row buffers, their bounds, the lists (each a multiple of 8)
size_t qpn_project_pieces_scratch(int32_t n, int32_t m, int32_t p, int32_t cap)
{
    const size_t cols = (size_t)n + m + p, c = (size_t)cap;
    return 2 * c * cols * sizeof(double) + 4 * c * sizeof(double) + ((5 * c * sizeof(int32_t) + 7) & ~(size_t)7);
}

hipError_t qpn_launch_project_pieces(int32_t pieces, int32_t n, int32_t m, int32_t p, double tol, int32_t cap, double *Ap, const double *lp,
                                     const double *up, const uint8_t *keep, double *buf, double *bnd, int32_t *lists, double *Ar,
                                     double *lr, double *ur, int32_t *rows_out, int32_t *flags_out, hipStream_t stream)
{
    if (pieces <= 0) return hipSuccess;
    const size_t lds = qpn_project_pieces_lds(n, m, p);
    if (lds > (size_t)kProjectLdsMax) return hipErrorInvalidValue;
    static QpnLdsLimits lds_limits;
    if (const hipError_t e = lds_limits.raise({{project_pieces_kernel, kProjectLdsMax}}); e != hipSuccess) return e;
    hipLaunchKernelGGL(project_pieces_kernel, dim3((unsigned)pieces), dim3(256), lds, stream, n, m, p, tol, cap, Ap, lp, up, keep, buf, bnd,
                       lists, Ar, lr, ur, rows_out, flags_out);
    return hipGetLastError();
}
