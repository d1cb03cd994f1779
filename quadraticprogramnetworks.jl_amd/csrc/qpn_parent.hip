// qpn_parent.hip -- the records of inner nodes made on the device (qpn_assemble_parent_nodes).
//
// A node's constraint stack is [base; child pieces] (src/qp_processing.jl:62-66, :183-187).  The base blocks of every distinct
// parent (static store), every distinct child piece over its own columns (piece pool) and the column map of every distinct
// (parent shape, piece column list) pair go up once; an item names a parent and up to QPN_PARENT_SLOTS (piece, map) pairs.
//
//   parent_maps_kernel      one workgroup per map: entries in [-1, n0 + p), no column named twice -> map_bad.
//   parent_records_kernel   one workgroup per item.  The ROW PLAN is the only per-item computation: the row count of every
//                           slot, and in form 1 the position of every stack row among the equality rows E (finite l == u) or the
//                           others I (ballot + popcount rank inside a wavefront, a running base in LDS across chunks of 256
//                           rows).  Then every word of the record is written once from the static store (lanes along the
//                           column-major outputs' fast index), and after a barrier the pieces' coefficients are put over it,
//                           lanes along the rows of one piece column.  Copies and negations only: the numpy twin
//                           (level_batch.assemble_parent_records_host) gives the same bits.
#include "qpn_internal.h"

namespace {

constexpr int kParThreads = 256;
constexpr int kParSlots = QPN_PARENT_SLOTS;
constexpr int kParRows = QPN_PARENT_MAX_ROWS;

__global__ __launch_bounds__(kParThreads) void parent_maps_kernel(int32_t map_words, const int32_t *map_off, const int32_t *map_data,
                                                                 long long ncol, uint8_t *map_bad)
{
    __shared__ int s_bad;
    const int k = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    const int a = map_off[k], b = map_off[k + 1];
    bool bad = a < 0 || b < a || b > map_words;
    if (!bad)
        for (int i = a + tid; i < b; i += kParThreads) {
            const int v = map_data[i];
            if (v < -1 || v >= ncol) bad = true;
            else if (v >= 0)
                for (int j = a; j < i; ++j) bad = bad || map_data[j] == v;
        }
    if (bad) s_bad = 1;
    __syncthreads();
    if (tid == 0) map_bad[k] = s_bad ? 1 : 0;
}

__global__ __launch_bounds__(kParThreads) void parent_records_kernel(ParentArgs a)
{
    __shared__ int s_E[kParRows], s_I[kParRows], s_dst[kParRows];
    __shared__ int s_seg[kParSlots + 2];                   // stack rows: base [seg[0], seg[1]), slot k [seg[k+1], seg[k+2])
    __shared__ int s_row0[kParSlots], s_c[kParSlots], s_off[kParSlots], s_mapo[kParSlots];
    __shared__ int s_cnt[2][kParThreads / WAVE];
    __shared__ int s_base[2];
    __shared__ int s_err, s_flag;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int n0 = a.n0, m = a.m, p = a.p, mb = a.mb, ps = a.ps;
    const int pa = a.parent_of[b];
    const bool pa_ok = pa >= 0 && pa < a.parents;

    // ---- 1. indices, ranges and maps (codes 1, 2) and the stack's size (code 4): one lane, a few words per slot
    if (tid == 0) {
        bool any1 = !pa_ok, any2 = false;
        int mbt = 0;
        if (pa_ok) {
            mbt = a.mb_true[pa];
            if (mbt < 0 || mbt > mb) { any1 = true; mbt = 0; }
        }
        bool over = mbt > kParRows;                        // more stack rows than the plan holds
        if (over) mbt = 0;
        s_seg[0] = 0; s_seg[1] = mbt;
        int T = mbt;
        for (int k = 0; k < kParSlots; ++k) {
            int rows = 0;
            const int q = a.piece_of[(size_t)b * kParSlots + k];
            s_row0[k] = s_c[k] = s_off[k] = s_mapo[k] = 0;
            if (q != -1) {
                const int mp = a.map_of[(size_t)b * kParSlots + k];
                if (q < 0 || q >= a.pieces || mp < 0 || mp >= a.maps) any1 = true;
                else {
                    const int row0 = a.piece_desc[4 * (size_t)q], r = a.piece_desc[4 * (size_t)q + 1], c = a.piece_desc[4 * (size_t)q + 2],
                              off = a.piece_desc[4 * (size_t)q + 3];
                    if (row0 < 0 || r < 0 || c < 0 || off < 0 || (long long)row0 + r > a.pool_rows ||
                        (long long)off + (long long)r * c > a.pool_words) any1 = true;
                    else if (a.map_bad[mp] || a.map_off[mp + 1] - a.map_off[mp] != c) any2 = true;
                    else { rows = r; s_row0[k] = row0; s_c[k] = c; s_off[k] = off; s_mapo[k] = a.map_off[mp]; }
                }
            }
            over = over || rows > kParRows - T;
            if (!over) T += rows;
            s_seg[k + 2] = T;
        }
        s_err = any1 ? 1 : any2 ? 2 : over ? 4 : 0;
        s_flag = 0;
        s_base[0] = s_base[1] = 0;
    }
    __syncthreads();
    int err = s_err;

    // ---- 2. a -1 map entry under a non-zero coefficient (code 3)
    if (err == 0) {
        for (int k = 0; k < kParSlots; ++k) {
            const int r = s_seg[k + 2] - s_seg[k + 1], c = s_c[k];
            const double *pk = a.pA + s_off[k];
            const int32_t *mk = a.map_data + s_mapo[k];
            for (int cc = 0; cc < c; ++cc) {
                if (mk[cc] != -1) continue;
                for (int rr = tid; rr < r; rr += kParThreads)
                    if (pk[(size_t)rr * c + cc] != 0.0) s_flag = 1;
            }
        }
        __syncthreads();
        if (s_flag) err = 3;
    }

    // ---- 3. the row plan: every stack row's place among E or I
    const int T = err == 0 ? s_seg[kParSlots + 1] : 0;
    const int mbt = s_seg[1];
    auto stack_row = [&](int t, const double *base, const double *pool) -> double {     // l or u of stack row t < T
        if (t < mbt) return base[(size_t)pa * mb + t];
        int k = 0;
        while (t >= s_seg[k + 2]) ++k;
        return pool[s_row0[k] + (t - s_seg[k + 1])];
    };
    for (int t0 = 0; t0 < T; t0 += kParThreads) {
        const int t = t0 + tid;
        const bool in = t < T;
        bool eq = false;
        if (in && a.form) {
            const double lv = stack_row(t, a.sl, a.pl), uv = stack_row(t, a.su, a.pu);
            eq = !isinf(lv) && lv == uv;                              // (a NaN bound is no equality, as in the twin)
        }
        const bool cl[2] = {eq, in && !eq};
        int rank[2];
        for (int c = 0; c < 2; ++c) {
            const unsigned long long bal = __ballot(cl[c]);
            rank[c] = __popcll(bal & ((1ull << lane) - 1ull));
            if (lane == 0) s_cnt[c][wave] = __popcll(bal);
        }
        __syncthreads();
        for (int c = 0; c < 2; ++c) {
            int base = s_base[c];
            for (int w = 0; w < wave; ++w) base += s_cnt[c][w];
            if (cl[c]) {
                const int at = base + rank[c];                        // (at most T <= kParRows rows in a class)
                (c == 0 ? s_E : s_I)[at] = t;
                s_dst[t] = c == 0 ? -1 - at : at;
            }
        }
        __syncthreads();
        if (tid < 2) {
            int tot = 0;
            for (int w = 0; w < kParThreads / WAVE; ++w) tot += s_cnt[tid][w];
            s_base[tid] += tot;
        }
        __syncthreads();
    }
    int cE = s_base[0], cI = s_base[1];
    if (err == 0) {
        if (cI > m) err = 4;
        else if (a.form && cE != a.ne) err = 5;
    }
    if (err) cE = cI = 0;
    if (tid == 0) a.err[b] = err;
    const int nb = err ? 0 : mbt;                                     // base rows in use

    // ---- 4. every word of the record, from the static store; the pieces' columns as zeros
    const int n = n0 + (a.form ? a.ne : 0);
    const double *sQ = a.sQd + (size_t)(pa_ok ? pa : 0) * n0 * n0, *sR = a.sR + (size_t)(pa_ok ? pa : 0) * ps * n0;
    const double *sA = a.sAd + (size_t)(pa_ok ? pa : 0) * n0 * mb, *sB = a.sB + (size_t)(pa_ok ? pa : 0) * ps * mb;
    double *Qb = a.Qd + (size_t)b * n * n, *Rb = a.R + (size_t)b * p * n, *qb = a.qd + (size_t)b * n;
    double *Ab = a.Ad + (size_t)b * n * m, *Bb = a.B + (size_t)b * p * m, *lb = a.l + (size_t)b * m, *ub = a.u + (size_t)b * m;
    {   // Qd, column-major: word (j, i) at j * n + i, lanes along i
        int j = tid / n, i = tid - j * n;
        for (; j < n; ) {
            double v = 0.0;
            if (j < n0) {
                if (i < n0) { if (pa_ok) v = sQ[(size_t)j * n0 + i]; }
                else if (i - n0 < cE) { const int t = s_E[i - n0]; if (t < nb) v = sA[(size_t)j * mb + t]; }           //  A_E[e][j]
            } else if (i < n0 && j - n0 < cE) {
                const int t = s_E[j - n0];
                v = t < nb ? -sA[(size_t)i * mb + t] : -0.0;                                                          // -A_E[e][i]
            }
            Qb[(size_t)j * n + i] = v;
            i += kParThreads;
            while (i >= n) { i -= n; ++j; }
        }
    }
    {   // R [p][n]: word (k, i) at k * n + i
        int k = tid / n, i = tid - k * n;
        for (; k < p; ) {
            double v = 0.0;
            if (k < ps) {
                if (i < n0) { if (pa_ok) v = sR[(size_t)k * n0 + i]; }
                else if (i - n0 < cE) { const int t = s_E[i - n0]; if (t < nb) v = sB[(size_t)k * mb + t]; }
            }
            Rb[(size_t)k * n + i] = v;
            i += kParThreads;
            while (i >= n) { i -= n; ++k; }
        }
    }
    for (int i = tid; i < n; i += kParThreads) {
        double v = 0.0;
        if (i < n0) { if (pa_ok) v = a.sqd[(size_t)pa * n0 + i]; }
        else if (i - n0 < cE) v = -stack_row(s_E[i - n0], a.sl, a.pl);
        qb[i] = v;
    }
    if (m > 0) {
        {   // Ad [n][m]: word (j, r) at j * m + r, lanes along the rows
            int j = tid / m, r = tid - j * m;
            for (; j < n; ) {
                double v = 0.0;
                if (j < n0 && r < cI) { const int t = s_I[r]; if (t < nb) v = sA[(size_t)j * mb + t]; }
                Ab[(size_t)j * m + r] = v;
                r += kParThreads;
                while (r >= m) { r -= m; ++j; }
            }
        }
        {   // B [p][m]
            int k = tid / m, r = tid - k * m;
            for (; k < p; ) {
                double v = 0.0;
                if (k < ps && r < cI) { const int t = s_I[r]; if (t < nb) v = sB[(size_t)k * mb + t]; }
                Bb[(size_t)k * m + r] = v;
                r += kParThreads;
                while (r >= m) { r -= m; ++k; }
            }
        }
        for (int r = tid; r < m; r += kParThreads) {
            double lv = -QINF, uv = QINF;
            if (r < cI) { const int t = s_I[r]; lv = stack_row(t, a.sl, a.pl); uv = stack_row(t, a.su, a.pu); }
            lb[r] = lv; ub[r] = uv;
        }
    }
    if (err) return;
    __syncthreads();                                                  // (the zeros are in place before a coefficient lands on one)

    // ---- 5. the pieces' coefficients: piece column cc of slot k goes to the record's column map[cc], lanes along its rows
    for (int k = 0; k < kParSlots; ++k) {
        const int r = s_seg[k + 2] - s_seg[k + 1], c = s_c[k], t1 = s_seg[k + 1];
        if (r == 0 || c == 0) continue;
        const double *pk = a.pA + s_off[k];
        const int32_t *mk = a.map_data + s_mapo[k];
        int cc = tid / r, rr = tid - cc * r;
        for (; cc < c; ) {
            const int j = mk[cc];
            if (j >= 0) {
                const double v = pk[(size_t)rr * c + cc];
                const int d = s_dst[t1 + rr];
                if (j < n0) {
                    if (d < 0) { const int e = n0 + (-1 - d); Qb[(size_t)j * n + e] = v; Qb[(size_t)e * n + j] = -v; }
                    else Ab[(size_t)j * m + d] = v;
                } else {
                    if (d < 0) Rb[(size_t)(j - n0) * n + n0 + (-1 - d)] = v;
                    else Bb[(size_t)(j - n0) * m + d] = v;
                }
            }
            rr += kParThreads;
            while (rr >= r) { rr -= r; ++cc; }
        }
    }
}

} // namespace

hipError_t qpn_launch_parent_records(const ParentArgs &a, hipStream_t s)
{
    if (a.items <= 0) return hipSuccess;
    if (a.maps > 0)
        hipLaunchKernelGGL(parent_maps_kernel, dim3((unsigned)a.maps), dim3(kParThreads), 0, s, a.map_words, a.map_off, a.map_data,
                           (long long)a.n0 + a.p, a.map_bad);
    hipLaunchKernelGGL(parent_records_kernel, dim3((unsigned)a.items), dim3(kParThreads), 0, s, a);
    return hipGetLastError();
}
