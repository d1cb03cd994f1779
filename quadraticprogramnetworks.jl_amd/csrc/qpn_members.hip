// qpn_members.hip -- interior members of polyhedra (polyhedra.interior_members_batch / remove_subsets_many) with the node
// records made on the device.
//
//   interior_records_kernel   the node record of the slack program  min eps + delta/2 (|x|^2 + eps^2)  over one polyhedron
//                             (A [r x d], l, u), every word of it, structural zeros included:
//                               free block [x (d); eps; mu_E (ne)]:  Qd = [[delta I, -A_E'], [A_E, D]],  qd = [0; 1; -l_E],
//                               rows: nlo slots [a_i, +1, 0] in (l_i, inf), nhi slots [a_i, -1, 0] in (-inf, u_i), padding to mp.
//                             It copies, negates and writes constants: the numpy twin (polyhedra.interior_member_records) gives
//                             the same values.  The rows of a class are its first rows in ascending order (ballot + popcount
//                             rank inside a wavefront, a running base in LDS across the chunks of 256 rows).
//   members_extract_kernel    ok = status == SUCCESS and z[d] <= 1e-6 and not flagged;  x = z[0 .. d).
//   members_outside_kernel    pair q: does member X[pi[q]] violate a row of piece pj[q] by more than t?  One wavefront per 16
//                             consecutive pairs (one read of the piece serves them when they share it), lanes over the rows
//                             (chunks of 64), a.x summed over ascending columns: acc = acc + a * x[c].
#include "qpn_internal.h"

namespace {

constexpr int kMemThreads = 256;

// One workgroup per item.  Dynamic LDS: the row lists of the three classes (r ints each).
__global__ __launch_bounds__(kMemThreads) void interior_records_kernel(int32_t r, int32_t d, const double *A, const double *l, const double *u,
                                                                      double delta, int32_t ne, int32_t nlo, int32_t nhi, double *Qd,
                                                                      double *qd, double *Ad, double *lo, double *uo, uint8_t *flag)
{
    extern __shared__ int s_rows[];
    __shared__ int s_cnt[3][kMemThreads / WAVE];
    __shared__ int s_base[3];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    int *s_E = s_rows, *s_LO = s_rows + r, *s_HI = s_rows + 2 * r;
    const double *Ab = A + (size_t)b * d * r, *lb = l + (size_t)b * r, *ub = u + (size_t)b * r;
    if (tid < 3) s_base[tid] = 0;
    __syncthreads();
    for (int r0 = 0; r0 < r; r0 += kMemThreads) {
        const int row = r0 + tid;
        const bool in = row < r;
        const double lv = in ? lb[row] : -QINF, uv = in ? ub[row] : QINF;
        const bool eq = in && !isinf(lv) && lv == uv;              // (a NaN bound is in no class, as in the twin)
        const bool cl[3] = {eq, in && !eq && lv == lv && !isinf(lv), in && !eq && uv == uv && !isinf(uv)};
        int rank[3];
        for (int c = 0; c < 3; ++c) {
            const unsigned long long bal = __ballot(cl[c]);
            rank[c] = __popcll(bal & ((1ull << lane) - 1ull));
            if (lane == 0) s_cnt[c][wave] = __popcll(bal);
        }
        __syncthreads();
        for (int c = 0; c < 3; ++c) {
            int base = s_base[c];
            for (int w = 0; w < wave; ++w) base += s_cnt[c][w];
            if (cl[c]) s_rows[c * r + base + rank[c]] = row;       // (a class has at most r rows: the lists cannot overflow)
        }
        __syncthreads();
        if (tid < 3) {
            int tot = 0;
            for (int w = 0; w < kMemThreads / WAVE; ++w) tot += s_cnt[tid][w];
            s_base[tid] += tot;
        }
        __syncthreads();
    }
    int cE = s_base[0], cLO = s_base[1], cHI = s_base[2];
    // more rows of a class than the record has slots: nothing is cut off -- the item is flagged and gets the record of a
    // polyhedron without rows (inert, solvable); members_extract_kernel reports "no answer" for it
    const bool over = cE > ne || cLO > nlo || cHI > nhi;
    if (over) cE = cLO = cHI = 0;
    if (tid == 0) flag[b] = over ? 1 : 0;

    const int nf = d + 1 + ne, mi = nlo + nhi;
    const int mp = mi <= 16 ? 16 : (mi + 15) & ~15;
    // Qd, column-major: word (j, i) at j * nf + i, lanes along i
    double *Qb = Qd + (size_t)b * nf * nf;
    {
        int j = tid / nf, i = tid - j * nf;
        for (; j < nf; ) {
            double v = 0.0;
            if (j <= d) {
                if (i == j) v = delta;
                else if (j < d && i > d && i - d - 1 < cE) v = Ab[(size_t)j * r + s_E[i - d - 1]];        // A_E[k][j]
            } else {
                const int k = j - d - 1;
                if (i < d) { if (k < cE) v = -Ab[(size_t)i * r + s_E[k]]; }                                // -A_E[k][i]
                else if (i == j) v = k < cE ? 0.0 : 1.0;                                                   // idle multiplier: 1 * mu = 0
            }
            Qb[(size_t)j * nf + i] = v;
            i += kMemThreads;
            while (i >= nf) { i -= nf; ++j; }
        }
    }
    for (int i = tid; i < nf; i += kMemThreads) {
        double v = 0.0;
        if (i == d) v = 1.0;
        else if (i > d && i - d - 1 < cE) v = -lb[s_E[i - d - 1]];
        qd[(size_t)b * nf + i] = v;
    }
    // Ad, column-major: word (c, slot) at c * mp + slot, lanes along the slots
    double *Adb = Ad + (size_t)b * nf * mp;
    {
        int c = tid / mp, s = tid - c * mp;
        for (; c < nf; ) {
            double v = 0.0;
            if (c <= d) {
                int row = -1; double one = 0.0;
                if (s < nlo) { if (s < cLO) { row = s_LO[s]; one = 1.0; } }
                else if (s < mi) { if (s - nlo < cHI) { row = s_HI[s - nlo]; one = -1.0; } }
                if (row >= 0) v = c < d ? Ab[(size_t)c * r + row] : one;
            }
            Adb[(size_t)c * mp + s] = v;
            s += kMemThreads;
            while (s >= mp) { s -= mp; ++c; }
        }
    }
    for (int s = tid; s < mp; s += kMemThreads) {
        double lv = -QINF, uv = QINF;
        if (s < nlo) { if (s < cLO) lv = lb[s_LO[s]]; }
        else if (s < mi) { if (s - nlo < cHI) uv = ub[s_HI[s - nlo]]; }
        lo[(size_t)b * mp + s] = lv; uo[(size_t)b * mp + s] = uv;
    }
}

__global__ __launch_bounds__(kMemThreads) void members_extract_kernel(int32_t batch, int32_t d, int32_t N, const double *z,
                                                                     const int32_t *status, const uint8_t *flag, double *x, uint8_t *ok)
{
    const long long t = (long long)blockIdx.x * kMemThreads + threadIdx.x;
    if (t >= (long long)batch * d) return;
    const int b = (int)(t / d), c = (int)(t - (long long)b * d);
    x[t] = z[(size_t)b * N + c];
    if (c == 0) ok[b] = (status[b] == QPN_SUCCESS && !flag[b] && z[(size_t)b * N + d] <= 1e-6) ? 1 : 0;
}

// One wavefront per kMemTile consecutive pairs, lanes over the rows of the piece (chunks of 64).  Column c of the piece is
// contiguous over its rows: lanes read it coalesced; x[c] is the same word for the whole wavefront.  A level asks every member
// of a list against every piece of it, so callers order the pairs by piece: when the pairs of a tile share their piece (the
// common case), each word of the piece is read once for the whole tile and feeds kMemTile accumulators -- a list of thousands of
// pieces would otherwise stream every piece from HBM once per member.  Each pair's sum is the same ascending-column sum either way.
constexpr int kMemTile = 16;

__device__ __forceinline__ bool member_outside_one(const double *Ab, const double *lb, const double *ub, const double *x, int d, int rj,
                                                   double t, int lane)
{
    bool viol = false;
    for (int r0 = 0; r0 < rj; r0 += WAVE) {
        const int row = r0 + lane;
        if (row < rj) {
            double acc = 0.0;
            for (int c = 0; c < d; ++c) acc = acc + Ab[(size_t)c * rj + row] * x[c];
            viol = viol || acc < lb[row] - t || acc > ub[row] + t;
        }
    }
    return viol;
}

__global__ __launch_bounds__(kMemThreads) void members_outside_kernel(int32_t pairs, int32_t d, int32_t rj, const double *Aj, const double *lj,
                                                                     const double *uj, int32_t Bj, const double *X, int32_t Bi,
                                                                     const int32_t *pi, const int32_t *pj, double t, uint8_t *out)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const long long wv = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kMemThreads / WAVE) + threadIdx.x / WAVE));
    const long long q0 = wv * kMemTile;
    if (q0 >= pairs) return;
    const int cnt = pairs - q0 < kMemTile ? (int)(pairs - q0) : kMemTile;
    // a full tile of in-range pairs over one piece?
    bool tiled = cnt == kMemTile && (long long)Bi * d < (1ll << 31);
    const int j0 = pj[q0];
    for (int k = 0; k < cnt && tiled; ++k) {
        const int i = pi[q0 + k];
        tiled = pj[q0 + k] == j0 && i >= 0 && i < Bi && j0 >= 0 && j0 < Bj;
    }
    if (tiled) {
        const double *Ab = Aj + (size_t)j0 * d * rj, *lb = lj + (size_t)j0 * rj, *ub = uj + (size_t)j0 * rj;
        unsigned xo[kMemTile];                               // the members' offsets in X (Bi * d < 2^31: checked at launch)
#pragma unroll
        for (int k = 0; k < kMemTile; ++k) xo[k] = (unsigned)pi[q0 + k] * (unsigned)d;
        unsigned viol = 0;
        for (int r0 = 0; r0 < rj; r0 += WAVE) {
            const int row = r0 + lane;
            if (row < rj) {
                double acc[kMemTile];
#pragma unroll
                for (int k = 0; k < kMemTile; ++k) acc[k] = 0.0;
                for (int c = 0; c < d; ++c) {
                    const double a = Ab[(size_t)c * rj + row];
#pragma unroll
                    for (int k = 0; k < kMemTile; ++k) acc[k] = acc[k] + a * X[xo[k] + c];
                }
                const double lo = lb[row] - t, hi = ub[row] + t;
#pragma unroll
                for (int k = 0; k < kMemTile; ++k) viol |= (acc[k] < lo || acc[k] > hi) ? (1u << k) : 0u;
            }
        }
#pragma unroll
        for (int k = 0; k < kMemTile; ++k) {
            const unsigned long long any = __ballot((viol >> k) & 1u);
            if (lane == 0) out[q0 + k] = any ? 1 : 0;
        }
        return;
    }
    for (int k = 0; k < cnt; ++k) {
        const long long q = q0 + k;
        const int i = pi[q], j = pj[q];
        if (i < 0 || i >= Bi || j < 0 || j >= Bj) {          // an index out of range: "not settled here"
            if (lane == 0) out[q] = 1;
            continue;
        }
        const bool v = member_outside_one(Aj + (size_t)j * d * rj, lj + (size_t)j * rj, uj + (size_t)j * rj, X + (size_t)i * d, d, rj, t, lane);
        const unsigned long long any = __ballot(v);
        if (lane == 0) out[q] = any ? 1 : 0;
    }
}

} // namespace

size_t qpn_interior_records_lds(int32_t r) { return 3 * (size_t)r * sizeof(int); }

hipError_t qpn_launch_interior_records(int32_t batch, int32_t r, int32_t d, const double *A, const double *l, const double *u, double delta,
                                       int32_t ne, int32_t nlo, int32_t nhi, double *Qd, double *qd, double *Ad, double *lo, double *uo,
                                       uint8_t *flag, hipStream_t s)
{
    if (batch <= 0) return hipSuccess;
    hipLaunchKernelGGL(interior_records_kernel, dim3((unsigned)batch), dim3(kMemThreads), qpn_interior_records_lds(r), s, r, d, A, l, u, delta,
                       ne, nlo, nhi, Qd, qd, Ad, lo, uo, flag);
    return hipGetLastError();
}

hipError_t qpn_launch_members_extract(int32_t batch, int32_t d, int32_t N, const double *z, const int32_t *status, const uint8_t *flag,
                                      double *x, uint8_t *ok, hipStream_t s)
{
    if (batch <= 0) return hipSuccess;
    const long long total = (long long)batch * d;
    hipLaunchKernelGGL(members_extract_kernel, dim3((unsigned)((total + kMemThreads - 1) / kMemThreads)), dim3(kMemThreads), 0, s, batch, d, N,
                       z, status, flag, x, ok);
    return hipGetLastError();
}

hipError_t qpn_launch_members_outside(int32_t pairs, int32_t d, int32_t rj, const double *Aj, const double *lj, const double *uj, int32_t Bj,
                                      const double *X, int32_t Bi, const int32_t *pi, const int32_t *pj, double t, uint8_t *out, hipStream_t s)
{
    if (pairs <= 0) return hipSuccess;
    const int per = (kMemThreads / WAVE) * kMemTile;
    hipLaunchKernelGGL(members_outside_kernel, dim3((unsigned)((pairs + per - 1) / per)), dim3(kMemThreads), 0, s, pairs, d, rj, Aj, lj, uj, Bj, X,
                       Bi, pi, pj, t, out);
    return hipGetLastError();
}
