// qpn_crash_big.hip -- reuse sweeps of the large class's crash cache (QPN_OPT_CRASH_CACHE_BIG; 64 < n <= 256, m <= 256), gfx950.
//
// Stage A of qpn_avi_schur_big2.hip eliminates the top half [H | C | g] with rank-64 block pivots and forms S = -Ad W,
// c = B w - Ad h.  Of all that only ONE column moves with w: g = qd + R w -> h, and with it c and the scale of the pivot
// threshold.  H, C, the pivot blocks, their inverses, the multipliers U' of every pass, W and S are made of Qd and Ad alone.  A
// filling sweep (the FILL instantiations of that file) leaves per node: U' of every pass in the H column tiles that die with
// the pass, W in the C tiles, S, the smallest accepted pivot and max |M| over H and C (layout: BigCrash, qpn_internal.h).
//
// crash_big_replay redoes the g column alone, with the instructions and operands the elimination itself applies to the g tile:
//   * g as the records route forms it (qd, then fma over the columns of R ascending);
//   * max |M| = max(cached max over H and C, max |g|) -- the maximum the cold route takes over the same entries -- the threshold
//     1e-4 max(1, max |M|), and the node is declined (status -1) when the cached smallest pivot lies below it: the cold route
//     stops at the first pivot below the threshold, i.e. exactly when the smallest one is;
//   * per pass kb: the raw g tiles of the block's row tiles are the B operands, the cached U' of row tile I the A operands of the
//     same sixteen MFMA_NEGA (s ascending; s < 4 bw in a narrow last block) on the g tile of row tile I.  v_mfma_f64_16x16x4_f64
//     forms output element (i, j) from row i of A and column j of B: a tile is updated from its own columns alone, so the g tile
//     comes out as in the full elimination whatever the other tiles held;
//   * c: schur_big2_sprod's accumulation for its last column tile (B w in column 0 at the start, sixteen MFMAs per block of 64
//     rows, blocks ascending);
//   * the reduced problem's bounds, cold start, nsplit, nred, status -2; S is COPIED from the cache into the node's Lemke
//     dictionary: schur_big_lemke folds its pending pairs into that dictionary in place and writes its covering column there,
//     so Stage B never sees the cached S itself.
// One workgroup of 16 wavefronts per node, wavefront I on row tile I as in the elimination: the chain is 16 MFMAs per pass and
// wave, the work is the 0.5 MB of U' and the one pass over Ad, and sixteen waves keep sixteen 2 KB loads in flight per pass.
#include "qpn_internal.h"

namespace {

constexpr int TPBR = 1024;              // 16 wavefronts
typedef double d2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(TPBR, 1) void crash_big_replay(AviBatchArgs a, SchurBigWs w, double *dict, BigCrash bc)
{
    const int tid = threadIdx.x, b = blockIdx.x;
    if (!bc.flag[b]) return;            // no entry: the filling kernels behind this one take the node
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, lc = lane & 15, lq = lane >> 4;
    const int n = a.nd.n, m = a.nd.m, np_ = a.nd.p, N = n + m;
    const int nrt = pad16(n) >> 4, mct = pad16(m) >> 4, nct = nrt + mct + 1;
    __shared__ double sG[256];          // g = qd + R w
    __shared__ double sBv[256];         // B w
    __shared__ double sRed[16];
    __shared__ __attribute__((aligned(32))) double sV[16 * 256];     // g tiles: the raw pivot rows of a pass, then all of h
    double *const Tt = w.Tt + (size_t)b * (size_t)w.tt_stride;
    auto tile = [&](int I_, int J_) -> double * { return Tt + ((size_t)(I_ * nct + J_) << 8); };
    const double *w_ = a.nd.w + (size_t)b * (size_t)a.nd.stride_w;
    const size_t vo = (size_t)b * (size_t)N;

    // equality rows are not stage A's (the test is on updatable fields: every sweep repeats it)
    int bad_row = 0;
    if (tid < m && a.nd.l[(size_t)b * m + tid] == a.nd.u[(size_t)b * m + tid]) bad_row = 1;
    double mg = 0.0;
    if (tid < n) {
        const double *R_ = a.nd.R + (size_t)b * n * np_;
        double s_ = a.nd.qd[(size_t)b * n + tid];
        for (int k = 0; k < np_; ++k) s_ = fma(R_[(size_t)k * n + tid], w_[k], s_);
        sG[tid] = s_;
        mg = fabs(s_);
    }
    if (tid < m) {
        const double *B_ = a.nd.B + (size_t)b * m * np_;
        double s = 0.0;
        for (int k = 0; k < np_; ++k) s = fma(B_[(size_t)k * m + tid], w_[k], s);
        sBv[tid] = s;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(mg, off, 64); mg = o > mg ? o : mg; }
    if (lane == 0) sRed[wave] = mg;
    if (__syncthreads_count(bad_row) > 0) { if (tid == 0) a.status[b] = -1; return; }
    // this sweep's threshold against the smallest pivot of the fill
    double ms = bc.fig[2 * (size_t)b + 1];
#pragma unroll
    for (int k = 0; k < 16; ++k) ms = sRed[k] > ms ? sRed[k] : ms;
    const double thr = 1e-4 * (ms > 1.0 ? ms : 1.0);
    if (bc.fig[2 * (size_t)b] < thr) { if (tid == 0) a.status[b] = -1; return; }

    // ---- the g column through the passes: wave I holds the g tile of row tile I
    const bool owner = wave < nrt;
    const int I = wave;
    d4 ct;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int r = 16 * I + 4 * g + lq;
        const double q = sG[r < n ? r : 0];
        ct[g] = (owner && lc == 0 && r < n) ? q : 0.0;
    }
    const int npass = (nrt + 3) / 4;
    for (int kb = 0; kb < npass; ++kb) {
        const int bw = (nrt - 4 * kb) < 4 ? (nrt - 4 * kb) : 4;
        double ua[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) ua[s] = (owner && s < 4 * bw) ? tile(I, 4 * kb + (s >> 2))[(s & 3) * 64 + lane] : 0.0;
        if (I >= 4 * kb && I < 4 * kb + bw) {
#pragma unroll
            for (int g = 0; g < 4; ++g) sV[((I - 4 * kb) << 8) + g * 64 + lane] = ct[g];
        }
        __syncthreads();
        if (owner) {
            const double *const vb = sV + lane;
            if (bw == 4) {
#pragma unroll
                for (int s = 0; s < 16; ++s) ct = MFMA_NEGA(ua[s], vb[((s >> 2) << 8) + (s & 3) * 64], ct);
            } else {
#pragma unroll
                for (int s = 0; s < 12; ++s)
                    if (s < 4 * bw) ct = MFMA_NEGA(ua[s], vb[((s >> 2) << 8) + (s & 3) * 64], ct);
            }
        }
        __syncthreads();
    }
    // h: into the node's top half (the finish kernel reads W | h there) and into LDS for the product below
    if (owner) {
        double *const dst = tile(I, nct - 1);
#pragma unroll
        for (int g = 0; g < 4; ++g) dst[g * 64 + lane] = ct[g];
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) sV[(I << 8) + g * 64 + lane] = owner ? ct[g] : 0.0;
    __syncthreads();

    // ---- c = B w - Ad h: wave Is holds row tile Is of the h column tile of [S | c]
    const int Is = wave;
    if (Is < mct) {
        const double *A_ = a.nd.Ad + (size_t)b * m * n;
        d4 acc;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ri = 16 * Is + 4 * g + lq;
            const double bv = sBv[ri < m ? ri : 0];
            acc[g] = (lc == 0 && ri < m) ? bv : 0.0;
        }
        for (int kc = 0; kc < npass; ++kc) {
            double aop[16];
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int ri = 16 * Is + lc, k = 64 * kc + 4 * s + lq;
                const bool ok = ri < m && k < n;
                const double v = A_[ok ? k * m + ri : 0];
                aop[s] = ok ? -v : 0.0;
            }
#pragma unroll
            for (int s = 0; s < 16; ++s) acc = MFMA(aop[s], sV[((4 * kc + (s >> 2)) << 8) + (s & 3) * 64 + lane], acc);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ri = 16 * Is + 4 * g + lq;
            if (lc == 0 && ri < m) w.c[vo + ri] = acc[g];
        }
    }
    // ---- S: a private copy in the node's dictionary (row stride pad16(m + 1): m rows of it, an even count of doubles; a
    // dictionary slot starts N (N + 1) doubles after the last, an even count too)
    {
        const d2 *src = reinterpret_cast<const d2 *>(bc.S + (size_t)b * (size_t)bc.s_stride);
        d2 *dst = reinterpret_cast<d2 *>(dict + (size_t)b * (size_t)N * (size_t)(N + 1));
        const int cnt = (m * pad16(m + 1)) >> 1;
        for (int k = tid; k < cnt; k += TPBR) dst[k] = src[k];
    }
    // reduced problem data: bounds of the constraint rows, cold start
    for (int k = tid; k < m; k += TPBR) {
        w.l2[vo + k] = a.nd.l[(size_t)b * m + k]; w.u2[vo + k] = a.nd.u[(size_t)b * m + k]; w.lam[vo + k] = 0.0;
    }
    if (tid == 0) { w.nsplit[b] = n; w.nred[b] = m; a.status[b] = -2; }
}

__global__ __launch_bounds__(256) void crash_big_count(int batch, const uint8_t *flag, int32_t *count)
{
    int c = 0;
    for (int k = threadIdx.x; k < batch; k += 256) c += flag[k] ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    __shared__ int red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) *count = red[0] + red[1] + red[2] + red[3];
}

} // namespace

hipError_t qpn_launch_crash_big_replay(const AviBatchArgs &a, const SchurBigWs &w, double *dict, const BigCrash &bc, hipStream_t stream)
{
    if (!qpn_schur_big2_shape(a.nd.n, a.nd.m) || a.nd.n + a.nd.m != a.N) return hipErrorInvalidValue;
    hipLaunchKernelGGL(crash_big_replay, dim3((unsigned)a.batch), dim3(TPBR), 0, stream, a, w, dict, bc);
    return hipGetLastError();
}

hipError_t qpn_launch_crash_big_count(int batch, const uint8_t *flag, int32_t *count, hipStream_t stream)
{
    hipLaunchKernelGGL(crash_big_count, dim3(1), dim3(256), 0, stream, batch, flag, count);
    return hipGetLastError();
}
