// qpn_finish.hip -- the finishing step of a level's solution-graph pieces on the device (the uncapped route of
// level_batch.solution_pieces, max_pieces = None): what the host did per piece to qpn_reduced_pieces' output, data-parallel
// over the pieces, so that only the pieces the host has to build cross to it.
//
//   finish_norm_kernel    per piece: the rows over the item's columns in ascending global order (take[]), each row brought to a
//                         largest coefficient of 1 (the bounds with it), entries |a| < 1e-8 dropped, the row divided by the
//                         absolute value of its leading nonzero (negated, bounds swapped, when that is negative) -- Poly's
//                         normalisation, src/sets.jl:76-89 --; the point's worst violation over the live rows; the merge test of
//                         avi_solutions._dedupe (a close adjacent pair of row projections on the probe vector, or a valid all-zero
//                         row); the 64-bit hash of the 6-digit rounded key.  One wavefront per piece up to 96 rows, one workgroup
//                         of 256 above.  The normalised rows are not stored: the per-row scale and divisor are, and the two later
//                         kernels recompute an entry from them with the same operations, so every copy is bit-equal.
//   finish_dup_kernel     one wavefront per candidate piece, the candidates sorted by (item, hash, piece): the earliest earlier
//                         piece of the run with an equal key (same row count, rounded rows and rounded bounds bit for bit)
//   finish_store_kernel   the compacted store: the pieces the host builds, normalised, column-major like qpn_reduced_pieces' Ar
//
// Arithmetic contract (level_batch._finish_host, the numpy twin, does the same operations in the same order; fp contraction
// off): sc = big > 0 ? 1 / big : 1;  v = a * sc;  v = |v| < 1e-8 ? 0 : v;  v = v / (neg ? -|lead| : |lead|);
// L = l * sc / |lead|, U = u * sc / |lead| (swapped and negated when neg);  key entries rint(v * 1e6) / 1e6 + 0.0 (rows),
// rint(L * 1e6) / 1e6 (bounds).  worst and the projections are sums whose order numpy does not fix: they agree to rounding.
#include "qpn_internal.h"

namespace {

constexpr int FIN_MAX_CAP = 1024;                 // n + 2m with n + m <= 512
constexpr unsigned long long HGOLD = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ unsigned long long fin64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// one key word at position idx of the key (rows row-major, then the r lower bounds, then the r upper bounds)
__device__ __forceinline__ unsigned long long hword(double v, long long idx)
{
    return fin64((unsigned long long)__double_as_longlong(v) + (unsigned long long)(idx + 1) * HGOLD);
}
__device__ __forceinline__ double round6(double v) { return rint(v * 1e6) / 1e6; }
__device__ __forceinline__ double norm_entry(double a, double sc, double div)
{
    double v = a * sc;
    if (fabs(v) < 1e-8) v = 0.0;
    return v / div;
}

struct FinArgs {
    int32_t oc, cap;
    const double *Ar, *lr, *ur;
    const int32_t *rows, *flags, *rec_of, *ncols, *take;
    const double *xk, *probe;
    double member_tol;
    double *rsc, *rdiv, *Ln, *Un;
    int32_t *status; double *worst; unsigned long long *hash; int32_t *dup_of;
};

template <int BS>
__global__ __launch_bounds__(BS) void finish_norm_kernel(FinArgs a)
{
    __shared__ double s_h[FIN_MAX_CAP];
    __shared__ double r_w[BS];
    __shared__ unsigned long long r_h[BS];
    __shared__ int s_merge;
    const int t = blockIdx.x, tid = threadIdx.x;
    const int cap = a.cap, oc = a.oc;
    if (a.flags[t] != 0) {                                           // left to the host (_reduce_on_host)
        if (tid == 0) { a.status[t] = QPN_FIN_FLAGGED; a.worst[t] = 0.0; a.hash[t] = 0ull; a.dup_of[t] = -1; }
        return;
    }
    const int rec = a.rec_of[t], nc = a.ncols[rec], rt = a.rows[t];
    const int32_t *tk = a.take + (size_t)rec * oc;
    const double *xr = a.xk + (size_t)rec * oc, *pr = a.probe + (size_t)rec * oc;
    const double *A = a.Ar + (size_t)t * oc * cap;
    if (tid == 0) s_merge = 0;
    double wmax = 0.0;
    unsigned long long hs = 0ull;
    int zero_row = 0;
    for (int r = tid; r < cap; r += BS) {
        double big = 0.0;
        for (int c = 0; c < nc; ++c) big = fmax(big, fabs(A[(size_t)tk[c] * cap + r]));
        const double sc = big > 0.0 ? 1.0 / big : 1.0;
        double lead = 1.0; bool has = false;
        for (int c = 0; c < nc; ++c) {
            double v = A[(size_t)tk[c] * cap + r] * sc;
            if (fabs(v) < 1e-8) v = 0.0;
            if (v != 0.0) { lead = v; has = true; break; }
        }
        const double nrm = fabs(lead);
        const bool neg = has && lead < 0.0;
        const double div = neg ? -nrm : nrm;
        const double L2 = a.lr[(size_t)t * cap + r] * sc, U2 = a.ur[(size_t)t * cap + r] * sc;
        const double ln = L2 / nrm, un = U2 / nrm;
        const double L = neg ? -un : ln, U = neg ? -ln : un;
        const bool valid = r < rt;
        double ax = 0.0, h = 0.0;
        for (int c = 0; c < nc; ++c) {
            const double v = norm_entry(A[(size_t)tk[c] * cap + r], sc, div);
            const double px = v * xr[c], ph = v * pr[c];
            ax = ax + px; h = h + ph;
            if (valid) hs += hword(round6(v) + 0.0, (long long)r * nc + c);
        }
        if (valid) {
            hs += hword(round6(L), (long long)rt * nc + r);
            hs += hword(round6(U), (long long)rt * nc + rt + r);
            if (has) wmax = fmax(wmax, fmax(L - ax, ax - U));
            else zero_row = 1;
        }
        if (r < FIN_MAX_CAP) s_h[r] = valid ? h : QINF;
        a.rsc[(size_t)t * cap + r] = sc; a.rdiv[(size_t)t * cap + r] = div;
        a.Ln[(size_t)t * cap + r] = L; a.Un[(size_t)t * cap + r] = U;
    }
    __syncthreads();
    // a close adjacent pair after sorting: each valid row against its successor in sorted order (the smallest larger value,
    // or an equal value of a later row), without sorting
    int close = zero_row;
    for (int i = tid; i < rt; i += BS) {
        const double hi = s_h[i];
        double succ = QINF; bool found = false;
        for (int j = 0; j < rt; ++j) {
            const double hj = s_h[j];
            if ((hj > hi || (hj == hi && j > i)) && (!found || hj < succ)) { succ = hj; found = true; }
        }
        if (found && isfinite(succ) && succ - hi <= 1e-7 * (1.0 + fabs(succ))) close = 1;
    }
    if (close) s_merge = 1;                                          // (benign race: every writer stores 1)
    r_w[tid] = wmax; r_h[tid] = hs;
    __syncthreads();
    for (int s = BS / 2; s > 0; s >>= 1) {
        if (tid < s) { r_w[tid] = fmax(r_w[tid], r_w[tid + s]); r_h[tid] += r_h[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) {
        const double w = r_w[0];
        a.worst[t] = w;
        a.hash[t] = fin64(r_h[0] ^ (unsigned long long)rt);
        a.status[t] = (w <= a.member_tol ? QPN_FIN_MEMBER : 0) | (s_merge ? QPN_FIN_MERGE : 0);
        a.dup_of[t] = -1;
    }
}

// the key word w of piece t (rows row-major over nc columns, then r lower, then r upper bounds), as bits
__device__ __forceinline__ unsigned long long key_word(const FinArgs &a, int t, int r, int nc, const int32_t *tk, int w)
{
    const int cap = a.cap;
    double v;
    if (w < r * nc) {
        const int i = w / nc, c = w - i * nc;
        v = round6(norm_entry(a.Ar[(size_t)t * a.oc * cap + (size_t)tk[c] * cap + i], a.rsc[(size_t)t * cap + i],
                              a.rdiv[(size_t)t * cap + i])) + 0.0;
    } else if (w < r * nc + r) {
        v = round6(a.Ln[(size_t)t * cap + (w - r * nc)]);
    } else {
        v = round6(a.Un[(size_t)t * cap + (w - r * nc - r)]);
    }
    return (unsigned long long)__double_as_longlong(v);
}

// ord: the candidates sorted; pos[i]: a position of ord with an earlier one of the same (item, hash), run0[i] that run's start
__global__ __launch_bounds__(256) void finish_dup_kernel(FinArgs a, int32_t cnt, const int32_t *ord, const int32_t *pos, const int32_t *run0)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= cnt) return;                                            // (whole wavefronts)
    const int s = pos[i];
    const int t = ord[s], r = a.rows[t], rec = a.rec_of[t], nc = a.ncols[rec];
    const int32_t *tk = a.take + (size_t)rec * a.oc;
    const int words = r * nc + 2 * r;
    for (int q = run0[i]; q < s; ++q) {
        const int t2 = ord[q];
        if (a.rows[t2] != r) continue;
        bool diff = false;
        for (int w = lane; w < words && !diff; w += 64) diff = key_word(a, t, r, nc, tk, w) != key_word(a, t2, r, nc, tk, w);
        if (qpn_ballot(diff) == 0ull) {
            if (lane == 0) { a.dup_of[t] = t2; a.status[t] |= QPN_FIN_DUP; }
            return;
        }
    }
}

__global__ __launch_bounds__(256) void finish_store_kernel(FinArgs a, const int32_t *src, double *As, double *ls, double *us, int32_t *rows_s)
{
    const int s = blockIdx.x, tid = threadIdx.x, t = src[s], cap = a.cap, oc = a.oc;
    const int rec = a.rec_of[t], nc = a.ncols[rec];
    const int32_t *tk = a.take + (size_t)rec * oc;
    const double *A = a.Ar + (size_t)t * oc * cap;
    double *Ao = As + (size_t)s * oc * cap;
    for (int c = 0; c < oc; ++c)
        for (int r = tid; r < cap; r += 256)
            Ao[(size_t)c * cap + r] = c < nc ? norm_entry(A[(size_t)tk[c] * cap + r], a.rsc[(size_t)t * cap + r], a.rdiv[(size_t)t * cap + r]) : 0.0;
    for (int r = tid; r < cap; r += 256) { ls[(size_t)s * cap + r] = a.Ln[(size_t)t * cap + r]; us[(size_t)s * cap + r] = a.Un[(size_t)t * cap + r]; }
    if (tid == 0) rows_s[s] = a.rows[t];
}

} // namespace

hipError_t qpn_launch_finish_norm(int32_t pieces, int32_t oc, int32_t cap, const double *Ar, const double *lr, const double *ur,
                                  const int32_t *rows, const int32_t *flags, const int32_t *rec_of, const int32_t *ncols, const int32_t *take,
                                  const double *xk, const double *probe, double member_tol, double *rsc, double *rdiv, double *Ln, double *Un,
                                  int32_t *status, double *worst, unsigned long long *hash, int32_t *dup_of, hipStream_t stream)
{
    if (pieces <= 0) return hipSuccess;
    const FinArgs a{oc, cap, Ar, lr, ur, rows, flags, rec_of, ncols, take, xk, probe, member_tol, rsc, rdiv, Ln, Un, status, worst, hash, dup_of};
    if (cap <= 96) hipLaunchKernelGGL(finish_norm_kernel<64>, dim3((unsigned)pieces), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL(finish_norm_kernel<256>, dim3((unsigned)pieces), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t qpn_launch_finish_dup(int32_t cnt, const int32_t *ord, const int32_t *pos, const int32_t *run0, int32_t oc, int32_t cap, const double *Ar,
                                 const int32_t *rows, const int32_t *rec_of, const int32_t *ncols, const int32_t *take, const double *rsc,
                                 const double *rdiv, const double *Ln, const double *Un, int32_t *status, int32_t *dup_of, hipStream_t stream)
{
    if (cnt <= 0) return hipSuccess;
    const FinArgs a{oc, cap, Ar, nullptr, nullptr, rows, nullptr, rec_of, ncols, take, nullptr, nullptr, 0.0, const_cast<double *>(rsc),
                    const_cast<double *>(rdiv), const_cast<double *>(Ln), const_cast<double *>(Un), status, nullptr, nullptr, dup_of};
    hipLaunchKernelGGL(finish_dup_kernel, dim3((unsigned)((cnt + 3) / 4)), dim3(256), 0, stream, a, cnt, ord, pos, run0);
    return hipGetLastError();
}

hipError_t qpn_launch_finish_store(int32_t stored, const int32_t *src, int32_t oc, int32_t cap, const double *Ar, const int32_t *rows,
                                   const int32_t *rec_of, const int32_t *ncols, const int32_t *take, const double *rsc, const double *rdiv,
                                   const double *Ln, const double *Un, double *As, double *ls, double *us, int32_t *rows_s, hipStream_t stream)
{
    if (stored <= 0) return hipSuccess;
    const FinArgs a{oc, cap, Ar, nullptr, nullptr, rows, nullptr, rec_of, ncols, take, nullptr, nullptr, 0.0, const_cast<double *>(rsc),
                    const_cast<double *>(rdiv), const_cast<double *>(Ln), const_cast<double *>(Un), nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(finish_store_kernel, dim3((unsigned)stored), dim3(256), 0, stream, a, src, As, ls, us, rows_s);
    return hipGetLastError();
}
