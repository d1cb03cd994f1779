// qpn_explore.hip -- multiplier-vertex exploration (QPNetOptions.exploration_vertices; src/avi_solutions.jl:92-129, :241-382).
//
// qpn_multiplier_vertices: per item, vertices of the multiplier set at a point,
//     Lambda = { lambda : E lambda = g,  lambda_j >= 0 (class GE), <= 0 (LE), free (FREE), = 0 (ZERO) },   E = Ad' (n x m),
// found from the verified multiplier lambda0 by a fixed, documented walk.  The numpy twin is
// level_batch.multiplier_vertices_host; both do the same operations in the same order (fp contraction off), so they agree to
// the last bits on every decision that is not within rounding of a tolerance.
//   setup     ZERO columns are dropped, LE columns negated (mu = sign * lambda >= 0), every row of [E | g] divided by its
//             largest |entry| (a row without one must have |g_i| <= feas * max(1, |g|): otherwise EMPTY).
//   factor    Gauss-Jordan over a list of columns in order: the pivot row is the largest |entry| among the rows not yet
//             pivoted, entries within 2^-30 of it count as equal and the lowest row wins; a column whose candidates are all
//             <= tol depends on the pivoted ones.
//   start     FREE columns first: one that depends on the others means Lambda has a lineality space (NO_VERTEX).  Then
//             purification of mu0 = sign * lambda0 (negative GE/LE entries taken as 0): the support is factored in ascending
//             order; at the first dependent column c the null direction d (d_c = 1, d_q = -T[row_q, c]) moves mu until a
//             sign-constrained entry reaches 0 -- forward if some entry of d is < -tol, backward otherwise; the lowest index
//             among ratios within 2^-30 of the least leaves -- and the factorisation starts again.  The independent support is
//             then completed in ascending order; a row left without a pivot must have |rhs| <= feas * max(1, |rhs|): else EMPTY.
//   walk      breadth first over bases, from that one.  A basis is factored afresh (its columns ascending) and its basic solution
//             read off; sign-constrained entries below -feas * scale make it infeasible (skipped), entries below tol * scale
//             are taken as 0.  A vertex new after rounding to 5 digits (the reference's QuantizedVector) is stored; the V+1-st
//             ends the walk (VERTEX_BUDGET).  Neighbours: every nonbasic GE/LE column j ascending enters; the ratio test runs
//             over the basic GE/LE rows with T[row, j] > tol; EVERY row whose ratio lies within 2^-30 of the least leaves in
//             turn (ascending basic column), so the degenerate bases of one vertex are all reached.  A basis seen before is
//             skipped; one beyond max_bases is dropped and the walk ends as BASIS_BUDGET unless a vertex budget ended it first.
// Size classes (a team serves one item):
//   wave class     n, m <= 32: a team is one wavefront, MV_WAVES items per workgroup, the tableau in LDS
//   group class    n, m <= 128: a team is a 256-thread workgroup, the tableau in LDS
//   global class   n, m <= 512: a 256-thread workgroup per item, the tableau in a global workspace, launched in chunks
// The visited bases (max_bases bitsets of m bits) live in the global workspace in every class.
//
// qpn_recipe_filter: one thread per recipe; recipe t of product row v = vrow_of[t] is dropped when an earlier row s of the same
// item (first_of[v] <= s < v) holds every one of its codes.
#include "qpn_internal.h"

namespace {

constexpr int MV_WAVES = 4;
constexpr int MV_GROUP = 256;
constexpr int MV_MAXW = 8;                    // bitset words of a basis: m <= 512
constexpr double MV_BAND = 1.0 - 0x1p-30;
constexpr double MV_TIE = 0x1p-30;
constexpr size_t MV_CHUNK_BYTES = size_t(256) << 20;

enum { MV_GE = 0, MV_LE = 1, MV_FREE = 2, MV_ZERO = 3 };

// slice: doubles T[n*(m+1)] mu[m] d[m] s[n] fcol[n] red[TT], then ints rowof[m] colof[n]
__host__ __device__ inline size_t mv_slice_bytes(int n, int m, int TT)
{
    const size_t dbl = (size_t)n * (m + 1) + 2 * (size_t)m + 2 * (size_t)n + TT;
    return (dbl * 8 + ((size_t)m + n) * 4 + 15) & ~size_t(15);
}

__host__ __device__ inline int mv_words(int m) { return (m + 63) / 64; }

template <int TT, bool WAVE>
struct MvTeam {
    double *red;
    int t;
    // the visited bitsets are global memory written by one thread and read by all: the fences are workgroup-scoped in both
    // classes (a wave-scoped fence does not order global memory)
    __device__ void sync() const
    {
        if constexpr (WAVE) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        } else {
            __syncthreads();
        }
    }
    template <int OP> __device__ double reduce(double v) const   // OP 1 = max, 2 = min; every thread gets the result
    {
        red[t] = v;
        sync();
        for (int s = TT / 2; s > 0; s >>= 1) {
            if (t < s) red[t] = OP == 1 ? fmax(red[t], red[t + s]) : fmin(red[t], red[t + s]);
            sync();
        }
        const double r = red[0];
        sync();
        return r;
    }
};

struct MvItem {
    int n, m, ld;
    const double *E, *g;
    const uint8_t *cls;
    double *T, *mu, *d, *s, *fcol;
    int *rowof, *colof;
    double tol;
};

// [E | g] of the item, columns of class ZERO dropped, LE negated, rows divided by s; pivot maps cleared
template <int TT, bool WAVE>
__device__ void mv_load(const MvItem &it, const MvTeam<TT, WAVE> &tm)
{
    const int n = it.n, m = it.m, ld = it.ld;
    for (int idx = tm.t; idx < n * ld; idx += TT) {
        const int i = idx / ld, k = idx - i * ld;
        const double si = it.s[i];
        double v;
        if (k < m) {
            const int c = it.cls[k];
            v = c == MV_ZERO ? 0.0 : (c == MV_LE ? -it.E[(size_t)i * m + k] : it.E[(size_t)i * m + k]);
            if (si > 0.0) v = v / si;
        } else {
            v = si > 0.0 ? it.g[i] / si : 0.0;
        }
        it.T[idx] = v;
    }
    for (int j = tm.t; j < m; j += TT) it.rowof[j] = -1;
    for (int i = tm.t; i < n; i += TT) it.colof[i] = -1;
    tm.sync();
}

// one Gauss-Jordan step on column c; returns the pivot row or -1
template <int TT, bool WAVE>
__device__ int mv_pivot(const MvItem &it, const MvTeam<TT, WAVE> &tm, int c)
{
    const int n = it.n, ld = it.ld;
    double a = -1.0;
    for (int i = tm.t; i < n; i += TT)
        if (it.colof[i] < 0) a = fmax(a, fabs(it.T[(size_t)i * ld + c]));
    const double amax = tm.template reduce<1>(a);
    if (!(amax > it.tol)) return -1;
    const double thr = amax * MV_BAND;
    double ri = 1e30;
    for (int i = tm.t; i < n; i += TT)
        if (it.colof[i] < 0 && fabs(it.T[(size_t)i * ld + c]) >= thr) ri = fmin(ri, (double)i);
    const int r = (int)tm.template reduce<2>(ri);
    const double p = it.T[(size_t)r * ld + c];
    for (int i = tm.t; i < n; i += TT) it.fcol[i] = i == r ? 0.0 : it.T[(size_t)i * ld + c];
    tm.sync();
    for (int k = tm.t; k < ld; k += TT) it.T[(size_t)r * ld + k] = it.T[(size_t)r * ld + k] / p;
    tm.sync();
    for (int idx = tm.t; idx < n * ld; idx += TT) {
        const int i = idx / ld, k = idx - i * ld;
        if (i != r) it.T[idx] = it.T[idx] - it.fcol[i] * it.T[(size_t)r * ld + k];
    }
    if (tm.t == 0) { it.colof[r] = c; it.rowof[c] = r; }
    tm.sync();
    return r;
}

__device__ inline double mv_key(double v) { return rint(v * 1e5) / 1e5 + 0.0; }

__device__ inline bool mv_sgn(int c) { return c == MV_GE || c == MV_LE; }

template <int TT, bool WAVE>
__device__ void mv_item(unsigned char *slice, uint64_t *vis, int n, int m, const double *E, const double *g, const uint8_t *cls,
                        const double *lam0, int V, int max_bases, double tol, double feas, double *verts, int32_t *count,
                        int32_t *status, int t)
{
    const int ld = m + 1, W = mv_words(m);
    double *T = reinterpret_cast<double *>(slice);
    double *mu = T + (size_t)n * ld, *d = mu + m, *s = d + m, *fcol = s + n, *red = fcol + n;
    int *rowof = reinterpret_cast<int *>(red + TT), *colof = rowof + m;
    const MvTeam<TT, WAVE> tm{red, t};
    const MvItem it{n, m, ld, E, g, cls, T, mu, d, s, fcol, rowof, colof, tol};
    auto finish = [&](int cnt, int st) {
        if (t == 0) { *count = cnt; *status = st; }
    };
    // row scales and the right-hand side's scale
    double gm = 0.0;
    for (int i = t; i < n; i += TT) {
        double a = 0.0;
        for (int k = 0; k < m; ++k)
            if (cls[k] != MV_ZERO) a = fmax(a, fabs(E[(size_t)i * m + k]));
        s[i] = a;
        gm = fmax(gm, fabs(g[i]));
    }
    double gs = fmax(1.0, tm.template reduce<1>(gm));
    double bad = 0.0;
    for (int i = t; i < n; i += TT)
        if (s[i] == 0.0 && fabs(g[i]) > feas * gs) bad = 1.0;
    if (tm.template reduce<1>(bad) > 0.0) { finish(0, 3); return; }
    double gm2 = 0.0;
    for (int i = t; i < n; i += TT) gm2 = fmax(gm2, s[i] > 0.0 ? fabs(g[i] / s[i]) : 0.0);
    gs = fmax(1.0, tm.template reduce<1>(gm2));
    for (int j = t; j < m; j += TT) {
        const int c = cls[j];
        double v = c == MV_ZERO ? 0.0 : (c == MV_LE ? -lam0[j] : lam0[j]);
        if (mv_sgn(c) && v < 0.0) v = 0.0;
        mu[j] = v;
    }
    tm.sync();
    // 1. purification
    for (;;) {
        mv_load(it, tm);
        for (int c = 0; c < m; ++c)
            if (cls[c] == MV_FREE && mv_pivot(it, tm, c) < 0) { finish(0, 4); return; }
        int dep = -1;
        for (int c = 0; c < m; ++c) {
            if (!mv_sgn(cls[c]) || !(mu[c] > tol)) continue;
            if (mv_pivot(it, tm, c) < 0) { dep = c; break; }
        }
        if (dep < 0) break;
        double neg = 0.0;
        for (int j = t; j < m; j += TT) {
            const double dj = j == dep ? 1.0 : (rowof[j] >= 0 ? -T[(size_t)rowof[j] * ld + dep] : 0.0);
            d[j] = dj;
            if (mv_sgn(cls[j]) && (rowof[j] >= 0 || j == dep) && dj < -tol) neg = 1.0;
        }
        const bool fwd = tm.template reduce<1>(neg) > 0.0;
        double rmin = __builtin_huge_val();
        for (int j = t; j < m; j += TT) {
            const bool cand = mv_sgn(cls[j]) && (rowof[j] >= 0 || j == dep);
            if (cand && (fwd ? d[j] < -tol : d[j] > tol)) rmin = fmin(rmin, mu[j] / (fwd ? -d[j] : d[j]));
        }
        const double th = tm.template reduce<2>(rmin);
        double bi = 1e30;
        for (int j = t; j < m; j += TT) {
            const bool cand = mv_sgn(cls[j]) && (rowof[j] >= 0 || j == dep);
            if (cand && (fwd ? d[j] < -tol : d[j] > tol) && mu[j] / (fwd ? -d[j] : d[j]) <= th + th * MV_TIE) bi = fmin(bi, (double)j);
        }
        const int blk = (int)tm.template reduce<2>(bi);
        const double stp = (fwd ? 1.0 : -1.0) * th;
        for (int j = t; j < m; j += TT) {
            double v = mu[j] + stp * d[j];
            if (j == blk) v = 0.0;
            if (mv_sgn(cls[j]) && v < 0.0) v = 0.0;
            mu[j] = v;
        }
        tm.sync();
    }
    // 2. the rest of the first basis
    for (int c = 0; c < m; ++c)
        if (mv_sgn(cls[c]) && !(mu[c] > tol)) mv_pivot(it, tm, c);
    bad = 0.0;
    for (int i = t; i < n; i += TT)
        if (colof[i] < 0 && fabs(T[(size_t)i * ld + m]) > feas * gs) bad = 1.0;
    if (tm.template reduce<1>(bad) > 0.0) { finish(0, 3); return; }
    if (t == 0) {
        for (int w = 0; w < W; ++w) {
            uint64_t b = 0;
            for (int k = 0; k < 64 && w * 64 + k < m; ++k)
                if (rowof[w * 64 + k] >= 0) b |= uint64_t(1) << k;
            vis[w] = b;
        }
    }
    tm.sync();
    // 3. the walk
    int nvis = 1, head = 0, cnt = 0, st = 0;
    bool overflow = false;
    while (head < nvis) {
        uint64_t Bw[MV_MAXW];
        for (int w = 0; w < W; ++w) Bw[w] = vis[(size_t)head * W + w];
        ++head;
        mv_load(it, tm);
        bool ok = true;
        for (int c = 0; c < m && ok; ++c)
            if ((Bw[c >> 6] >> (c & 63)) & 1) ok = mv_pivot(it, tm, c) >= 0;
        if (!ok) continue;
        double inf = 0.0;
        for (int j = t; j < m; j += TT) {
            double v = rowof[j] >= 0 ? T[(size_t)rowof[j] * ld + m] : 0.0;
            if (mv_sgn(cls[j]) && v < -feas * gs) inf = 1.0;
            if (mv_sgn(cls[j]) && v < tol * gs) v = 0.0;
            mu[j] = v;
        }
        if (tm.template reduce<1>(inf) > 0.0) continue;
        // the vertex, and whether it is new (each thread compares the columns it writes itself)
        bool fresh = true;
        for (int q = 0; q < cnt && fresh; ++q) {
            double diff = 0.0;
            for (int j = t; j < m; j += TT) {
                const double lj = cls[j] == MV_LE ? -mu[j] : mu[j];
                if (mv_key(lj) != mv_key(verts[(size_t)q * m + j])) diff = 1.0;
            }
            fresh = tm.template reduce<1>(diff) > 0.0;
        }
        if (fresh) {
            if (cnt == V) { st = 1; break; }
            for (int j = t; j < m; j += TT) verts[(size_t)cnt * m + j] = cls[j] == MV_LE ? -mu[j] : mu[j];
            ++cnt;
        }
        // the neighbours (every thread runs the ratio tests itself: uniform control)
        for (int j = 0; j < m; ++j) {
            if (!mv_sgn(cls[j]) || rowof[j] >= 0) continue;
            double th = __builtin_huge_val();
            for (int c = 0; c < m; ++c) {
                if (rowof[c] < 0 || !mv_sgn(cls[c])) continue;
                const double a = T[(size_t)rowof[c] * ld + j];
                if (a > tol) th = fmin(th, mu[c] / a);
            }
            if (th == __builtin_huge_val()) continue;
            const double lim = th + th * MV_TIE;
            for (int c = 0; c < m; ++c) {
                if (rowof[c] < 0 || !mv_sgn(cls[c])) continue;
                const double a = T[(size_t)rowof[c] * ld + j];
                if (!(a > tol) || !(mu[c] / a <= lim)) continue;
                uint64_t nb[MV_MAXW];
                for (int w = 0; w < W; ++w) nb[w] = Bw[w];
                nb[c >> 6] &= ~(uint64_t(1) << (c & 63));
                nb[j >> 6] |= uint64_t(1) << (j & 63);
                double found = 0.0;
                for (int e = t; e < nvis; e += TT) {
                    bool eq = true;
                    for (int w = 0; w < W; ++w) eq = eq && vis[(size_t)e * W + w] == nb[w];
                    if (eq) found = 1.0;
                }
                if (tm.template reduce<1>(found) > 0.0) continue;
                if (nvis >= max_bases) { overflow = true; continue; }
                if (t == 0)
                    for (int w = 0; w < W; ++w) vis[(size_t)nvis * W + w] = nb[w];
                ++nvis;
                tm.sync();
            }
        }
    }
    if (st == 0 && overflow) st = 2;
    finish(cnt, st);
}

struct MvArgs {
    int32_t n, m, V, max_bases;
    const double *E, *g, *lam0;
    const uint8_t *cls;
    double tol, feas;
    double *verts;
    int32_t *count, *status;
};

__global__ __launch_bounds__(64 * MV_WAVES) void mv_wave_kernel(MvArgs a, int32_t first, int32_t cnt, uint64_t *vis, size_t slice)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char mv_lds[];
    const int w = threadIdx.x / 64, t = threadIdx.x % 64;
    const int local = blockIdx.x * MV_WAVES + w;
    if (local >= cnt) return;                      // a whole wavefront leaves: the others never wait for it
    const size_t b = (size_t)first + local;
    const size_t n = a.n, m = a.m;
    mv_item<64, true>(mv_lds + (size_t)w * slice, vis + (size_t)local * a.max_bases * mv_words(a.m), a.n, a.m, a.E + b * n * m,
                      a.g + b * n, a.cls + b * m, a.lam0 + b * m, a.V, a.max_bases, a.tol, a.feas, a.verts + b * a.V * m,
                      a.count + b, a.status + b, t);
}

template <bool LDS>
__global__ __launch_bounds__(MV_GROUP) void mv_group_kernel(MvArgs a, int32_t first, int32_t cnt, uint64_t *vis,
                                                           unsigned char *gws, size_t slice)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char mv_lds[];
    const int local = blockIdx.x;
    if (local >= cnt) return;
    const size_t b = (size_t)first + local;
    const size_t n = a.n, m = a.m;
    unsigned char *base = LDS ? mv_lds : gws + (size_t)local * slice;
    mv_item<MV_GROUP, false>(base, vis + (size_t)local * a.max_bases * mv_words(a.m), a.n, a.m, a.E + b * n * m, a.g + b * n,
                             a.cls + b * m, a.lam0 + b * m, a.V, a.max_bases, a.tol, a.feas, a.verts + b * a.V * m, a.count + b,
                             a.status + b, threadIdx.x);
}

enum MvClass { MVC_WAVE, MVC_GROUP, MVC_GLOBAL };

MvClass mv_class(int n, int m)
{
    if (n <= 32 && m <= 32) return MVC_WAVE;
    if (n <= 128 && m <= 128) return MVC_GROUP;
    return MVC_GLOBAL;
}

size_t mv_item_ws(int n, int m, int max_bases)
{
    size_t b = (size_t)max_bases * mv_words(m) * 8;
    if (mv_class(n, m) == MVC_GLOBAL) b += mv_slice_bytes(n, m, MV_GROUP);
    return (b + 255) & ~size_t(255);
}

int32_t mv_chunk(int32_t batch, int n, int m, int max_bases)
{
    size_t c = MV_CHUNK_BYTES / mv_item_ws(n, m, max_bases);
    if (c < 1) c = 1;
    if (mv_class(n, m) == MVC_WAVE) c = c < MV_WAVES ? MV_WAVES : c / MV_WAVES * MV_WAVES;
    return (int32_t)(c < (size_t)batch ? c : (size_t)batch);
}

__global__ void recipe_filter_kernel(int32_t pieces, int32_t N, const uint8_t *masks, const uint8_t *K, const int32_t *vrow_of,
                                     const int32_t *first_of, int32_t rows, uint8_t *keep)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= pieces) return;
    const int v = vrow_of[t];
    if (v < 0 || v >= rows) { keep[t] = 1; return; }
    int s0 = first_of[v];
    if (s0 < 0) s0 = 0;
    uint8_t kp = 1;
    for (int s = s0; s < v && kp; ++s) {
        bool in = true;
        for (int i = 0; i < N && in; ++i) {
            const int code = K[(size_t)t * N + i];
            in = code >= 1 && code <= 8 && ((masks[(size_t)s * N + i] >> (code - 1)) & 1);
        }
        if (in) kp = 0;
    }
    keep[t] = kp;
}

} // namespace

size_t qpn_multiplier_vertices_workspace_bytes(int32_t batch, int32_t n, int32_t m, int32_t max_bases)
{
    if (batch <= 0) return 0;
    return (size_t)mv_chunk(batch, n, m, max_bases) * mv_item_ws(n, m, max_bases) + 256;   // (+256: the tableaux' alignment)
}

hipError_t qpn_launch_multiplier_vertices(int32_t batch, int32_t n, int32_t m, const double *E, const double *g, const uint8_t *cls,
                                          const double *lam0, int32_t V, int32_t max_bases, double tol, double feas, double *verts,
                                          int32_t *count, int32_t *status, void *ws, hipStream_t s)
{
    if (batch <= 0) return hipSuccess;
    const MvArgs a{n, m, V, max_bases, E, g, lam0, cls, tol, feas, verts, count, status};
    const MvClass cls_ = mv_class(n, m);
    const int32_t chunk = mv_chunk(batch, n, m, max_bases);
    const size_t visb = (size_t)max_bases * mv_words(m) * 8;
    static QpnLdsLimits lds_limits;
    if (const hipError_t e = lds_limits.raise({{mv_wave_kernel, (int)(mv_slice_bytes(32, 32, 64) * MV_WAVES)},
                                               {mv_group_kernel<true>, (int)mv_slice_bytes(128, 128, MV_GROUP)}});
        e != hipSuccess)
        return e;
    for (int32_t first = 0; first < batch; first += chunk) {
        const int32_t cnt = batch - first < chunk ? batch - first : chunk;
        unsigned char *base = static_cast<unsigned char *>(ws);
        uint64_t *vis = reinterpret_cast<uint64_t *>(base);
        if (cls_ == MVC_WAVE) {
            const size_t slice = mv_slice_bytes(n, m, 64);
            hipLaunchKernelGGL(mv_wave_kernel, dim3((unsigned)((cnt + MV_WAVES - 1) / MV_WAVES)), dim3(64 * MV_WAVES), slice * MV_WAVES,
                               s, a, first, cnt, vis, slice);
        } else if (cls_ == MVC_GROUP) {
            const size_t slice = mv_slice_bytes(n, m, MV_GROUP);
            hipLaunchKernelGGL(mv_group_kernel<true>, dim3((unsigned)cnt), dim3(MV_GROUP), slice, s, a, first, cnt, vis,
                               static_cast<unsigned char *>(nullptr), slice);
        } else {
            // the tableaux follow the chunk's bitsets in the workspace
            const size_t slice = mv_slice_bytes(n, m, MV_GROUP);
            unsigned char *gws = base + (((size_t)chunk * visb + 255) & ~size_t(255));
            hipLaunchKernelGGL(mv_group_kernel<false>, dim3((unsigned)cnt), dim3(MV_GROUP), 0, s, a, first, cnt, vis, gws, slice);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t qpn_launch_recipe_filter(int32_t pieces, int32_t N, const uint8_t *masks, const uint8_t *K, const int32_t *vrow_of,
                                    const int32_t *first_of, int32_t rows, uint8_t *keep, hipStream_t s)
{
    if (pieces <= 0) return hipSuccess;
    hipLaunchKernelGGL(recipe_filter_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, s, pieces, N, masks, K, vrow_of,
                       first_of, rows, keep);
    return hipGetLastError();
}
