// qpn_convexity.hip -- check_qp_convexity (src/qp_processing.jl:39-55) for a batch of nodes: is the node's Hessian positive
// semidefinite on the null space of its implicit equality rows?
//
// Per node (Qd n x n and Ad m x n column-major, eq a uint8[m] mask of the implicit equality rows):
//   1. S = Qd + Qd'                                   (the reference's QQ + QQ'; a skew part of Qd cancels, nothing is halved)
//   2. V = Ae' (n x k): the selected rows of Ad that are not all zero, as columns.  A Householder QR with column pivoting of
//      V gives the rank r: pivot columns are taken while the largest remaining column norm |R_jj| exceeds
//      min(k, n) * eps * sigma_max(V) -- Julia's rank(Diagonal(svdvals)) rule with |R_jj| in the place of the singular values;
//      sigma_max comes from a power iteration and is never taken below the largest column norm.  A remaining column whose
//      norm has fallen to CVX_DEP * sqrt(n) * eps of its OWN original norm counts as zero: that is the rounding a Householder
//      sweep leaves of a column that depends exactly on the pivots taken (an implicit equality arrives as two opposing
//      rows), and min(k, n) * eps * sigma_max underestimates it when k is small and n large.
//   3. The r reflectors H_0 .. H_{r-1} (Q = H_0 ... H_{r-1}, Z = Q[:, r:n]) are applied on both sides of S; the trailing
//      (n-r) x (n-r) block is then Z' S Z.
//   4. That block is brought to tridiagonal form by Householder similarity transforms and its smallest eigenvalue found by
//      multisection on the Sturm count: every thread of the team counts at its own point, so one round narrows the bracket
//      by a factor T + 1; rounds go on until the bracket is a few ulps of its ends wide.
// Outputs: convex = (min_eig > -tol), min_eig (+inf when r = n), null_dim = n - r.  A non-finite entry of Qd or of a selected
// row gives convex = 0, min_eig = NaN, null_dim = -1, and nothing else is computed.
//
// Size classes (a "team" serves one node; everything the node needs lives in one workspace slice, see slice_bytes):
//   wave class     n <= 32 and the slice fits 40 KiB: a team is one wavefront, CVX_WAVES nodes per workgroup, the slices in
//                  LDS, wavefront barriers only (the nodes of a workgroup never wait for each other)
//   group class    n <= 128 and the slice fits 128 KiB: a team is a 256-thread workgroup, the slice in LDS
//   global class   anything else the entry accepts (n <= 256, m <= 1024): a 256-thread workgroup per node, the slice in a
//                  global workspace, launched in chunks of nodes so the workspace stays bounded
// Every index a thread forms stays inside its node's own slice and its own input record.
#include "qpn_internal.h"

#include <cfloat>

namespace {

constexpr int CVX_WAVES = 4;                 // nodes per workgroup in the wave class
constexpr int CVX_GROUP = 256;               // threads per node in the group and global classes
constexpr int CVX_POWER_ITERS = 30;
constexpr int CVX_MAX_ROUNDS = 64;
// A dependent column's residue was measured at up to 0.63 sqrt(n) eps of its original norm (k = 2 .. 1000, n = 2 .. 256, rank up
// to n - 2; profiles/convexity_accuracy.txt), the smallest genuine pivot of square Gaussian rows at 3.5e-3 of it: 8 leaves a
// factor 12 to the one side and eleven orders of magnitude to the other.
constexpr double CVX_DEP = 8.0;
constexpr size_t CVX_WAVE_SLICE_MAX = size_t(40) << 10;
constexpr size_t CVX_GROUP_SLICE_MAX = size_t(128) << 10;
constexpr size_t CVX_GLOBAL_CHUNK_BYTES = size_t(512) << 20;

// slice layout: doubles S[n*n] V[n*m] tau[n] vb[n] p[n] a[n] b2[n] cn[max(m,1)] c0[max(m,1)] red[T], then ints sel[max(m,1)] misc[4]
__host__ __device__ inline size_t slice_bytes(int n, int m, int T)
{
    const size_t mm = m > 0 ? m : 1;
    const size_t dbl = (size_t)n * n + (size_t)n * m + 5 * (size_t)n + 2 * mm + T;
    return (dbl * 8 + (mm + 4) * 4 + 15) & ~size_t(15);
}

template <int T, bool WAVE>
__device__ inline void team_sync()
{
    if constexpr (WAVE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

// tree reduction through red[T]; every thread of the team gets the result.  op 0 = sum, 1 = max, 2 = min.
template <int T, bool WAVE, int OP>
__device__ inline double team_reduce(double v, double *red, int t)
{
    red[t] = v;
    team_sync<T, WAVE>();
    for (int s = T / 2; s > 0; s >>= 1) {
        if (t < s) {
            const double o = red[t + s];
            red[t] = OP == 0 ? red[t] + o : (OP == 1 ? fmax(red[t], o) : fmin(red[t], o));
        }
        team_sync<T, WAVE>();
    }
    const double r = red[0];
    team_sync<T, WAVE>();
    return r;
}

// Householder reflector of x = (X[0], X[inc], ..., X[(len-1)*inc]) as dlarfg makes it: (I - tau v v') x = beta e_1, v_0 = 1,
// v[1:] written to vout[1 : len].  x[1:] = 0 gives tau = 0, beta = x_0.  Every thread returns the same tau and beta.
template <int T, bool WAVE>
__device__ inline void house(const double *X, int inc, int len, double *vout, double *red, int t, double &tau, double &beta)
{
    double part = 0.0;
    for (int i = 1 + t; i < len; i += T) {
        const double xi = X[(size_t)i * inc];
        part += xi * xi;
    }
    const double sig = team_reduce<T, WAVE, 0>(part, red, t);
    const double x0 = X[0];
    if (sig == 0.0) {
        tau = 0.0; beta = x0;
        for (int i = 1 + t; i < len; i += T) vout[i] = 0.0;
    } else {
        const double nrm = sqrt(x0 * x0 + sig);
        beta = x0 >= 0.0 ? -nrm : nrm;
        tau = (beta - x0) / beta;
        const double sc = 1.0 / (x0 - beta);
        for (int i = 1 + t; i < len; i += T) vout[i] = X[(size_t)i * inc] * sc;
    }
    if (t == 0) vout[0] = 1.0;
    team_sync<T, WAVE>();
}

// S[j0:n, j0:n] <- H S[j0:n, j0:n] H with H = I - tau v v', v = vb[j0 : n] (vb[j0] = 1), S symmetric, leading dimension n:
// p = tau S v, w = p - (tau/2)(p'v) v, S -= v w' + w v'.  The result stays exactly symmetric.
template <int T, bool WAVE>
__device__ inline void two_sided(double *S, int n, int j0, const double *vb, double tau, double *p, double *red, int t)
{
    if (tau == 0.0) return;
    const int len = n - j0;
    for (int i = t; i < len; i += T) {
        double acc = 0.0;
        for (int l = 0; l < len; ++l) acc += S[(size_t)(j0 + l) * n + (j0 + i)] * vb[j0 + l];
        p[j0 + i] = tau * acc;
    }
    team_sync<T, WAVE>();
    double part = 0.0;
    for (int i = t; i < len; i += T) part += p[j0 + i] * vb[j0 + i];
    const double K = 0.5 * tau * team_reduce<T, WAVE, 0>(part, red, t);
    for (int i = t; i < len; i += T) p[j0 + i] = p[j0 + i] - K * vb[j0 + i];
    team_sync<T, WAVE>();
    for (int e = t; e < len * len; e += T) {
        const int i = e % len, l = e / len;
        double &s = S[(size_t)(j0 + l) * n + (j0 + i)];
        s = s - (vb[j0 + i] * p[j0 + l] + p[j0 + i] * vb[j0 + l]);     // one commutative sum: (i, l) and (l, i) agree bitwise
    }
    team_sync<T, WAVE>();
}

// number of eigenvalues of the symmetric tridiagonal (a, b) below x (Sturm sequence of the LDL' pivots; a pivot that vanishes is
// replaced by -pmin, as LAPACK's dlaebz does)
__device__ inline int sturm_count(const double *a, const double *b2, int d, double x, double pmin)
{
    int c = 0;
    double q = a[0] - x;
    if (fabs(q) < pmin) q = -pmin;
    c += q < 0.0;
    for (int i = 1; i < d; ++i) {
        q = (a[i] - x) - b2[i - 1] / q;
        if (fabs(q) < pmin) q = -pmin;
        c += q < 0.0;
    }
    return c;
}

template <int T, bool WAVE>
__device__ void convexity_node(void *slice, int n, int m, const double *__restrict__ Qd, const double *__restrict__ Ad,
                               const uint8_t *__restrict__ eq, double tol, int32_t *convex, double *min_eig, int32_t *null_dim,
                               int t)
{
    const int mm = m > 0 ? m : 1;
    double *S = static_cast<double *>(slice);
    double *V = S + (size_t)n * n;
    double *tau = V + (size_t)n * m;
    double *vb = tau + n, *p = vb + n, *a = p + n, *b2 = a + n, *cn = b2 + n, *c0 = cn + mm, *red = c0 + mm;
    int *sel = reinterpret_cast<int *>(red + T);
    int *misc = sel + mm;                         // misc[0] = non-finite flag, misc[1] = k, misc[2] = pivot column

    // -- 1. S = Qd + Qd', the row flags of Ad, the non-finite check ------------------------------------------------------
    if (t == 0) misc[0] = 0;
    team_sync<T, WAVE>();
    bool bad = false;
    for (int e = t; e < n * n; e += T) {
        const int i = e % n, j = e / n;
        const double q = Qd[e];
        bad |= !isfinite(q);
        S[e] = q + Qd[(size_t)i * n + j];
    }
    for (int i = t; i < m; i += T) {
        int f = 0;
        if (eq[i]) {
            bool nz = false, nf = false;
            for (int j = 0; j < n; ++j) {
                const double v = Ad[(size_t)j * m + i];
                nz |= v != 0.0;
                nf |= !isfinite(v);
            }
            bad |= nf;
            f = nz ? 1 : 0;
        }
        sel[i] = f;
    }
    if (bad) misc[0] = 1;
    team_sync<T, WAVE>();
    if (misc[0]) {
        if (t == 0) { *convex = 0; *min_eig = __builtin_nan(""); *null_dim = -1; }
        return;
    }
    if (t == 0) {                                 // compact the selected, non-zero rows
        int k = 0;
        for (int i = 0; i < m; ++i)
            if (sel[i]) sel[k++] = i;
        misc[1] = k;
    }
    team_sync<T, WAVE>();
    const int k = misc[1];
    for (int e = t; e < n * k; e += T) {
        const int j = e % n, c = e / n;
        V[e] = Ad[(size_t)j * m + sel[c]];
    }
    team_sync<T, WAVE>();

    // -- 2. rank of V = Ae' by pivoted Householder QR --------------------------------------------------------------------
    int r = 0;
    if (k > 0) {
        // the columns' own squared norms: c0 travels with its column through the pivoting
        for (int c = t; c < k; c += T) {
            double acc = 0.0;
            for (int i = 0; i < n; ++i) {
                const double v = V[(size_t)c * n + i];
                acc += v * v;
            }
            c0[c] = acc;
        }
        team_sync<T, WAVE>();
        const double dep2 = CVX_DEP * CVX_DEP * DBL_EPSILON * DBL_EPSILON * (double)n;
        // sigma_max(V) by power iteration on V V' (a lower bound that converges to it)
        for (int j = t; j < n; j += T) vb[j] = 1.0 + 0.5 * sin(0.7 * (double)(j + 1));
        team_sync<T, WAVE>();
        double sig2 = 0.0;
        for (int it = 0; it < CVX_POWER_ITERS; ++it) {
            for (int c = t; c < k; c += T) {
                double acc = 0.0;
                for (int j = 0; j < n; ++j) acc += V[(size_t)c * n + j] * vb[j];
                cn[c] = acc;
            }
            team_sync<T, WAVE>();
            double part = 0.0;
            for (int j = t; j < n; j += T) {
                double acc = 0.0;
                for (int c = 0; c < k; ++c) acc += V[(size_t)c * n + j] * cn[c];
                p[j] = acc;
                part += acc * acc;
            }
            const double nx = sqrt(team_reduce<T, WAVE, 0>(part, red, t));
            double part2 = 0.0;
            for (int j = t; j < n; j += T) part2 += vb[j] * vb[j];
            const double n0 = sqrt(team_reduce<T, WAVE, 0>(part2, red, t));
            if (!(nx > 0.0) || !(n0 > 0.0)) break;
            sig2 = nx / n0;
            for (int j = t; j < n; j += T) vb[j] = p[j] / nx;
            team_sync<T, WAVE>();
        }
        double thr = -1.0;
        const int steps = k < n ? k : n;
        for (int j = 0; j < steps; ++j) {
            double best = -1.0;
            for (int c = j + t; c < k; c += T) {
                double acc = 0.0;
                for (int i = j; i < n; ++i) {
                    const double v = V[(size_t)c * n + i];
                    acc += v * v;
                }
                if (!(acc > dep2 * c0[c])) acc = 0.0;   // rounding residue of a column that depends on the pivots taken
                cn[c] = acc;
                best = fmax(best, acc);
            }
            best = team_reduce<T, WAVE, 1>(best, red, t);
            if (t == 0) {                         // the first column of largest remaining norm
                int pc = j;
                for (int c = j; c < k; ++c)
                    if (cn[c] == best) { pc = c; break; }
                misc[2] = pc;
            }
            team_sync<T, WAVE>();
            if (thr < 0.0) thr = (double)steps * DBL_EPSILON * fmax(sqrt(sig2), sqrt(best));
            if (!(sqrt(best) > thr)) break;
            const int pc = misc[2];
            if (pc != j) {
                for (int i = t; i < n; i += T) {
                    const double x = V[(size_t)j * n + i];
                    V[(size_t)j * n + i] = V[(size_t)pc * n + i];
                    V[(size_t)pc * n + i] = x;
                }
                if (t == 0) {
                    const double x = c0[j];
                    c0[j] = c0[pc];
                    c0[pc] = x;
                }
            }
            team_sync<T, WAVE>();
            double tj, bj;
            house<T, WAVE>(V + (size_t)j * n + j, 1, n - j, vb + j, red, t, tj, bj);
            // the reflector stays in V's column j below the diagonal (R_jj = beta on it)
            for (int i = j + 1 + t; i < n; i += T) V[(size_t)j * n + i] = vb[i];
            if (t == 0) { V[(size_t)j * n + j] = bj; tau[j] = tj; }
            if (tj != 0.0)
                for (int c = j + 1 + t; c < k; c += T) {
                    double dot = 0.0;
                    for (int i = j; i < n; ++i) dot += vb[i] * V[(size_t)c * n + i];
                    dot *= tj;
                    for (int i = j; i < n; ++i) V[(size_t)c * n + i] -= dot * vb[i];
                }
            team_sync<T, WAVE>();
            r = j + 1;
        }
    }

    // -- 3. Z' S Z: the reflectors on both sides of S ---------------------------------------------------------------------
    for (int j = 0; j < r; ++j) {
        for (int i = j + t; i < n; i += T) vb[i] = i == j ? 1.0 : V[(size_t)j * n + i];
        team_sync<T, WAVE>();
        two_sided<T, WAVE>(S, n, j, vb, tau[j], p, red, t);
    }
    const int d = n - r;
    if (d == 0) {
        if (t == 0) { *convex = 1; *min_eig = __builtin_huge_val(); *null_dim = 0; }
        return;
    }

    // -- 4. tridiagonal form of the trailing block, then its smallest eigenvalue ------------------------------------------
    for (int j = r; j + 2 < n; ++j) {
        double tj, bj;
        house<T, WAVE>(S + (size_t)j * n + (j + 1), 1, n - j - 1, vb + (j + 1), red, t, tj, bj);
        if (t == 0) b2[j - r] = bj * bj;
        two_sided<T, WAVE>(S, n, j + 1, vb, tj, p, red, t);
    }
    for (int i = t; i < d; i += T) a[i] = S[(size_t)(r + i) * n + (r + i)];
    if (t == 0 && d >= 2) {
        const double bl = S[(size_t)(n - 2) * n + (n - 1)];
        b2[d - 2] = bl * bl;
    }
    team_sync<T, WAVE>();
    // Gershgorin bracket [lo, hi] of the smallest eigenvalue: count(lo) = 0, count(hi) >= 1
    double glo = __builtin_huge_val(), amin = __builtin_huge_val(), bmax = 0.0, scale = 0.0;
    for (int i = t; i < d; i += T) {
        const double bl = i > 0 ? sqrt(b2[i - 1]) : 0.0, br = i + 1 < d ? sqrt(b2[i]) : 0.0;
        glo = fmin(glo, a[i] - bl - br);
        amin = fmin(amin, a[i]);
        bmax = fmax(bmax, i + 1 < d ? b2[i] : 0.0);
        scale = fmax(scale, fabs(a[i]) + bl + br);
    }
    glo = team_reduce<T, WAVE, 2>(glo, red, t);
    amin = team_reduce<T, WAVE, 2>(amin, red, t);
    bmax = team_reduce<T, WAVE, 1>(bmax, red, t);
    scale = team_reduce<T, WAVE, 1>(scale, red, t);
    const double pad = 4.0 * DBL_EPSILON * scale + DBL_MIN;
    const double pmin = DBL_MIN * fmax(1.0, bmax);
    double lo = glo - pad, hi = amin + pad;
    for (int round = 0; round < CVX_MAX_ROUNDS; ++round) {
        if (!(hi - lo > 2.0 * DBL_EPSILON * fmax(fabs(lo), fabs(hi)) + DBL_MIN)) break;
        const double x = lo + (hi - lo) * ((double)(t + 1) / (double)(T + 1));
        const int c = (x > lo && x < hi) ? sturm_count(a, b2, d, x, pmin) : -1;
        const double nhi = team_reduce<T, WAVE, 2>(c >= 1 ? x : hi, red, t);
        const double nlo = team_reduce<T, WAVE, 1>(c == 0 ? x : lo, red, t);
        if (nhi == hi && nlo == lo) break;        // no point strictly inside the bracket any more
        hi = nhi; lo = nlo;
    }
    if (t == 0) {
        const double lam = 0.5 * (lo + hi);
        *min_eig = lam;
        *convex = lam > -tol ? 1 : 0;
        *null_dim = d;
    }
}

__global__ __launch_bounds__(64 * CVX_WAVES) void convexity_wave_kernel(int32_t batch, int32_t n, int32_t m, const double *Qd,
                                                                        const double *Ad, const uint8_t *eq, double tol,
                                                                        int32_t *convex, double *min_eig, int32_t *null_dim,
                                                                        size_t slice)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char cvx_lds[];
    const int w = threadIdx.x / 64, t = threadIdx.x % 64;
    const long long b = (long long)blockIdx.x * CVX_WAVES + w;
    if (b >= batch) return;                       // a whole wavefront leaves: the others never wait for it
    convexity_node<64, true>(cvx_lds + (size_t)w * slice, n, m, Qd + (size_t)b * n * n, Ad + (size_t)b * m * n,
                             eq + (size_t)b * m, tol, convex + b, min_eig + b, null_dim + b, t);
}

template <bool LDS>
__global__ __launch_bounds__(CVX_GROUP) void convexity_group_kernel(int32_t first, int32_t count, int32_t n, int32_t m,
                                                                    const double *Qd, const double *Ad, const uint8_t *eq,
                                                                    double tol, int32_t *convex, double *min_eig,
                                                                    int32_t *null_dim, unsigned char *gws, size_t slice)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char cvx_lds[];
    const int local = blockIdx.x;
    if (local >= count) return;
    const long long b = (long long)first + local;
    void *base = LDS ? static_cast<void *>(cvx_lds) : static_cast<void *>(gws + (size_t)local * slice);
    convexity_node<CVX_GROUP, false>(base, n, m, Qd + (size_t)b * n * n, Ad + (size_t)b * m * n, eq + (size_t)b * m, tol,
                                     convex + b, min_eig + b, null_dim + b, threadIdx.x);
}

enum CvxClass { CVX_WAVE, CVX_GROUP_LDS, CVX_GLOBAL };

CvxClass cvx_class(int32_t n, int32_t m)
{
    if (n <= 32 && slice_bytes(n, m, 64) <= CVX_WAVE_SLICE_MAX) return CVX_WAVE;
    if (n <= 128 && slice_bytes(n, m, CVX_GROUP) <= CVX_GROUP_SLICE_MAX) return CVX_GROUP_LDS;
    return CVX_GLOBAL;
}

int32_t cvx_chunk(int32_t batch, int32_t n, int32_t m)
{
    const size_t per = slice_bytes(n, m, CVX_GROUP);
    size_t c = CVX_GLOBAL_CHUNK_BYTES / per;
    if (c < 1) c = 1;
    return (int32_t)(c < (size_t)batch ? c : (size_t)batch);
}

} // namespace

size_t qpn_convexity_workspace_bytes(int32_t batch, int32_t n, int32_t m)
{
    if (batch <= 0 || cvx_class(n, m) != CVX_GLOBAL) return 0;
    return (size_t)cvx_chunk(batch, n, m) * slice_bytes(n, m, CVX_GROUP);
}

hipError_t qpn_launch_convexity(int32_t batch, int32_t n, int32_t m, const double *Qd, const double *Ad, const uint8_t *eq,
                                double tol, int32_t *convex, double *min_eig, int32_t *null_dim, void *gws, hipStream_t s)
{
    if (batch <= 0) return hipSuccess;
    const CvxClass cls = cvx_class(n, m);
    if (cls == CVX_WAVE) {
        const size_t slice = slice_bytes(n, m, 64);
        const size_t lds = slice * CVX_WAVES;
        static QpnLdsLimits lds_limits;        // the largest wave-class request is 160 KiB: above the 64 KiB default
        if (const hipError_t e = lds_limits.raise({{convexity_wave_kernel, (int)(CVX_WAVE_SLICE_MAX * CVX_WAVES)}}); e != hipSuccess)
            return e;
        const unsigned grid = (unsigned)((batch + CVX_WAVES - 1) / CVX_WAVES);
        hipLaunchKernelGGL(convexity_wave_kernel, dim3(grid), dim3(64 * CVX_WAVES), lds, s, batch, n, m, Qd, Ad, eq, tol, convex,
                           min_eig, null_dim, slice);
        return hipGetLastError();
    }
    if (cls == CVX_GROUP_LDS) {
        const size_t slice = slice_bytes(n, m, CVX_GROUP);
        static QpnLdsLimits lds_limits;
        if (const hipError_t e = lds_limits.raise({{convexity_group_kernel<true>, (int)CVX_GROUP_SLICE_MAX}}); e != hipSuccess) return e;
        hipLaunchKernelGGL(convexity_group_kernel<true>, dim3((unsigned)batch), dim3(CVX_GROUP), slice, s, 0, batch, n, m, Qd, Ad,
                           eq, tol, convex, min_eig, null_dim, static_cast<unsigned char *>(nullptr), slice);
        return hipGetLastError();
    }
    const size_t slice = slice_bytes(n, m, CVX_GROUP);
    const int32_t chunk = cvx_chunk(batch, n, m);
    for (int32_t first = 0; first < batch; first += chunk) {
        const int32_t count = batch - first < chunk ? batch - first : chunk;
        hipLaunchKernelGGL(convexity_group_kernel<false>, dim3((unsigned)count), dim3(CVX_GROUP), 0, s, first, count, n, m, Qd, Ad,
                           eq, tol, convex, min_eig, null_dim, static_cast<unsigned char *>(gws), slice);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
