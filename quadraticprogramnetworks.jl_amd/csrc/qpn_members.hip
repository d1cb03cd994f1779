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
//   members_outside_lists_kernel  the same question for every member of a list against every piece of it, the pairs enumerated
//                             here from a CSR of the lists: one workgroup per piece (and chunk of positions), the piece in LDS,
//                             one bit per pair and one count of unsettled pairs per piece.
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

// ---- the same question asked list by list -------------------------------------------------------------
// "Every member of a list against every piece of the same list" is said by the lists, not by pairs: a workgroup owns one second
// piece j (blockIdx.x) and the words blockIdx.y * kListChunkWords + [0, kListChunkWords), then the same gridDim.y chunks further on,
// of its list's positions.  The piece is fetched ONCE per workgroup -- into LDS when 8 rj (d + 2) bytes fit kListsLdsBudget (kLds),
// else read through L2 by the same loop -- and every member of the chunk passes by it.  A wavefront takes the 32 positions of one
// word of `bits` as eight passes of the accumulator body of members_outside_kernel, 4 members a pass, lanes over the rows; the
// verdicts are combined by ballot and the word is stored by lane 0: one writer per word, no atomics on `bits`.  `undecided` is
// summed in LDS and added, one integer atomicAdd a workgroup, to the 0 members_lists_items_kernel left there (integer adds: any
// order).  The members' coordinates are the same for the whole wavefront and read-only in the launch (const __restrict__):
// scalar loads; list_mem and ok are read by the lanes, one position each.
constexpr int kListWaves = kMemThreads / WAVE;
constexpr int kListTile = 4;                                 // members per pass: 4 accumulators a lane, 8 passes a word
typedef double x4 __attribute__((ext_vector_type(4), aligned(8)));     // four consecutive coordinates of a member (a row of X is 8-byte aligned)
constexpr int kListChunkWords = 32;                          // 1024 positions per visit of a workgroup, 8 words per wavefront
// the piece (A, l, u) of a workgroup in LDS: 78 KiB at the most, so that with the kernel's static LDS (16 bytes) two
// workgroups fit a CU's 160 KiB -- 2 wavefronts per SIMD at the budget, 4 at (64, 64) (33 KiB), the registers' 7 from 22 KiB down
constexpr int kListsLdsBudget = 78 * 1024;

// What a piece's own indices say: nothing is read or written through one that is out of range.  k: the length of its list, -1
// when the list itself is bad (list_of out of range, its list_ptr entries decreasing or outside list_mem); nw: the words of
// its segment, -1 when the segment does not lie inside bits; good: list, own position and segment are all in order.
struct ListItem {
    long long p0, w0, nw;
    int k, sp;
    bool good;
};

__device__ __forceinline__ ListItem list_item(int j, int32_t Bj, int32_t lists, const int32_t *__restrict__ list_ptr,
                                              const int32_t *__restrict__ list_of, const int32_t *__restrict__ self_pos,
                                              const int64_t *__restrict__ word_ptr)
{
    ListItem it;
    const long long W = word_ptr[Bj], w1 = word_ptr[j + 1];
    it.w0 = word_ptr[j];
    it.nw = it.w0 >= 0 && w1 >= it.w0 && w1 <= W ? w1 - it.w0 : -1;
    it.p0 = 0; it.k = -1;
    const int a = list_of[j];
    if (a >= 0 && a < lists) {
        const long long M = list_ptr[lists], p0 = list_ptr[a], p1 = list_ptr[a + 1];
        if (p0 >= 0 && p1 >= p0 && p1 <= M && p1 - p0 < (1ll << 31) - 64) { it.p0 = p0; it.k = (int)(p1 - p0); }
    }
    it.sp = self_pos[j];
    it.good = it.k >= 0 && it.sp >= 0 && it.sp < it.k && it.nw >= ((it.k + 31) >> 5);
    return it;
}

// One wavefront per piece, before the kernel below: undecided starts at 0 for a good piece, whose words beyond its list's
// ceil(k / 32) are written 0; a bad piece gets its answer here -- its whole segment 0 and undecided = max(k - 1, 0), or 0 when the
// list itself is bad -- and the kernel below leaves it alone.
__global__ __launch_bounds__(WAVE) void members_lists_items_kernel(int32_t Bj, int32_t lists, const int32_t *__restrict__ list_ptr,
                                                                  const int32_t *__restrict__ list_of, const int32_t *__restrict__ self_pos,
                                                                  const int64_t *__restrict__ word_ptr, uint32_t *__restrict__ bits,
                                                                  int32_t *__restrict__ undecided)
{
    const int j = blockIdx.x, lane = threadIdx.x;
    const ListItem it = list_item(j, Bj, lists, list_ptr, list_of, self_pos, word_ptr);
    for (long long w = (it.good ? (it.k + 31) >> 5 : 0) + lane; w < it.nw; w += WAVE) bits[it.w0 + w] = 0u;
    if (lane == 0) undecided[j] = it.good || it.k < 1 ? 0 : it.k - 1;
}

template <bool kLds>
__global__ __launch_bounds__(kMemThreads) void members_outside_lists_kernel(
    int32_t d, int32_t rj, const double *__restrict__ Aj, const double *__restrict__ lj, const double *__restrict__ uj, int32_t Bj,
    const double *__restrict__ X, const uint8_t *__restrict__ ok, int32_t Bi, int32_t lists, const int32_t *__restrict__ list_ptr,
    const int32_t *__restrict__ list_mem, const int32_t *__restrict__ list_of, const int32_t *__restrict__ self_pos,
    const int64_t *__restrict__ word_ptr, double t, uint32_t *__restrict__ bits, int32_t *__restrict__ undecided)
{
    extern __shared__ double s_piece[];
    __shared__ int s_und[kListWaves];
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const ListItem it = list_item(j, Bj, lists, list_ptr, list_of, self_pos, word_ptr);
    const int k = it.k, sp = it.sp, nwk = (k + 31) >> 5;
    if (!it.good || (int)blockIdx.y * kListChunkWords >= nwk) return;          // (a bad piece has its answer from the kernel above)
    const int32_t *lm = list_mem + it.p0;
    uint32_t *seg = bits + it.w0;
    int32_t *und_j = undecided + j;
    asm volatile("" : "+v"(und_j), "+v"(seg));               // (kept in vector registers across the loops: the scalar ones are the members')

    const double *Ab = Aj + (size_t)j * d * rj, *lb = lj + (size_t)j * rj, *ub = uj + (size_t)j * rj;
    if (kLds) {
        const int na = d * rj;                               // (8 (na + 2 rj) <= kListsLdsBudget)
        for (int i = tid; i < na; i += kMemThreads) s_piece[i] = Ab[i];
        for (int i = tid; i < rj; i += kMemThreads) { s_piece[na + i] = lb[i]; s_piece[na + rj + i] = ub[i]; }
        __syncthreads();
        Ab = s_piece; lb = s_piece + na; ub = s_piece + na + rj;
    }

    const double *a_lane = Ab + lane, *l_lane = lb + lane, *u_lane = ub + lane;      // this lane's row of the chunk at r0 = 0
    int und = 0;
    for (int wc = (int)blockIdx.y * kListChunkWords; wc < nwk; wc += (int)gridDim.y * kListChunkWords) {
        const int wend = wc + kListChunkWords < nwk ? wc + kListChunkWords : nwk;
        for (int w = wc + wave; w < wend; w += kListWaves) {
            // the word's 32 positions, one per lane (the upper half of the wavefront repeats the lower): which are put to the
            // piece, which are answered 1 unseen, and where their members start in X (Bi * d < 2^31: checked at launch)
            const int s = 32 * w + (lane & 31);
            int m = -1;
            if (s < k) m = lm[s];
            bool use = m >= 0 && m < Bi && s != sp;
            if (use) use = ok[m] != 0;                        // (no member, or none that is ok: refutes nothing)
            const bool keep = s < k && s != sp && (m < -1 || m >= Bi);             // as qpn_members_outside: "not settled here"
            const unsigned live32 = (unsigned)__ballot(use), kept32 = (unsigned)__ballot(keep);
            const unsigned off = use ? (unsigned)m * (unsigned)d : 0u;
            unsigned word = kept32;
#pragma unroll 1
            for (int pass = 0; pass < 32 / kListTile; ++pass) {
                const unsigned live = (live32 >> (kListTile * pass)) & ((1u << kListTile) - 1u);
                if (!live) continue;
                const double *xp[kListTile];                 // (pointers, not offsets: no address arithmetic per column)
#pragma unroll
                for (int q = 0; q < kListTile; ++q) xp[q] = X + __builtin_amdgcn_readlane(off, kListTile * pass + q);
                unsigned viol = 0u;
                for (int r0 = 0; r0 < rj; r0 += WAVE) {
                    const int row = r0 + lane;
                    if (row < rj) {
                        double acc[kListTile];
#pragma unroll
                        for (int q = 0; q < kListTile; ++q) acc[q] = 0.0;
                        const double *ap = a_lane + r0;
                        int c = 0;
                        // four columns a turn: a member's four words are ONE scalar load; every sum still runs over ascending columns
#pragma unroll 1
                        for (; c + 4 <= d; c += 4) {
                            const double a0 = ap[0], a1 = ap[rj], a2 = ap[2 * (size_t)rj], a3 = ap[3 * (size_t)rj];
                            ap += 4 * (size_t)rj;
#pragma unroll
                            for (int q = 0; q < kListTile; ++q) {
                                const x4 xv = *reinterpret_cast<const x4 *>(xp[q] + c);
                                acc[q] = acc[q] + a0 * xv.x;
                                acc[q] = acc[q] + a1 * xv.y;
                                acc[q] = acc[q] + a2 * xv.z;
                                acc[q] = acc[q] + a3 * xv.w;
                            }
                        }
#pragma unroll 1
                        for (; c < d; ++c) {
                            const double av = *ap;
                            ap += rj;
#pragma unroll
                            for (int q = 0; q < kListTile; ++q) acc[q] = acc[q] + av * xp[q][c];
                        }
                        const double lo = l_lane[r0] - t, hi = u_lane[r0] + t;
#pragma unroll
                        for (int q = 0; q < kListTile; ++q) viol |= (acc[q] < lo || acc[q] > hi) ? (1u << q) : 0u;
                    }
                }
                unsigned hit = 0u;
#pragma unroll
                for (int q = 0; q < kListTile; ++q) hit |= __ballot((viol >> q) & 1u) ? 1u << q : 0u;
                word |= (hit & live) << (kListTile * pass);
            }
            // the positions of this word that are asked: s < k, s != sp
            unsigned asked = 32 * w + 32 <= k ? 0xffffffffu : (1u << (k - 32 * w)) - 1u;
            if ((sp >> 5) == w) asked &= ~(1u << (sp & 31));
            und += __popc(asked & ~word);
            if (lane == 0) seg[w] = word;
        }
    }
    if (lane == 0) s_und[wave] = und;
    __syncthreads();
    if (tid == 0) {
        int tot = 0;
        for (int v = 0; v < kListWaves; ++v) tot += s_und[v];
        if (tot) atomicAdd(und_j, tot);
    }
}

} // namespace

size_t qpn_interior_records_lds(int32_t r) { return 3 * (size_t)r * sizeof(int); }

// dynamic LDS of members_outside_lists_kernel for pieces of rj rows in d columns; 0: beyond the budget, the piece stays in global memory
size_t qpn_members_lists_lds(int32_t rj, int32_t d)
{
    const size_t bytes = 8 * (size_t)rj * ((size_t)d + 2);
    return bytes <= (size_t)kListsLdsBudget ? bytes : 0;
}

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

hipError_t qpn_launch_members_outside_lists(int32_t d, int32_t rj, const double *Aj, const double *lj, const double *uj, int32_t Bj,
                                            const double *X, const uint8_t *ok, int32_t Bi, int32_t lists, const int32_t *list_ptr,
                                            const int32_t *list_mem, const int32_t *list_of, const int32_t *self_pos,
                                            const int64_t *word_ptr, double t, uint32_t *bits, int32_t *undecided, hipStream_t s)
{
    if (Bj <= 0) return hipSuccess;
    hipLaunchKernelGGL(members_lists_items_kernel, dim3((unsigned)Bj), dim3(WAVE), 0, s, Bj, lists, list_ptr, list_of, self_pos, word_ptr, bits,
                       undecided);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // few pieces (a long list split over packs, or one list alone): more workgroups per piece, about 2048 in all, 64 at the most
    const unsigned gy = Bj >= 2048 ? 1u : (unsigned)((2048 + Bj - 1) / Bj < 64 ? (2048 + Bj - 1) / Bj : 64);
    const dim3 grid((unsigned)Bj, gy);
    const size_t lds = qpn_members_lists_lds(rj, d);
    if (lds) {
        static QpnLdsLimits lds_limits;                      // the budget is above the 64 KiB default
        e = lds_limits.raise({{members_outside_lists_kernel<true>, kListsLdsBudget}});
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(members_outside_lists_kernel<true>, grid, dim3(kMemThreads), lds, s, d, rj, Aj, lj, uj, Bj, X, ok, Bi, lists,
                           list_ptr, list_mem, list_of, self_pos, word_ptr, t, bits, undecided);
    } else {
        hipLaunchKernelGGL(members_outside_lists_kernel<false>, grid, dim3(kMemThreads), 0, s, d, rj, Aj, lj, uj, Bj, X, ok, Bi, lists,
                           list_ptr, list_mem, list_of, self_pos, word_ptr, t, bits, undecided);
    }
    return hipGetLastError();
}
