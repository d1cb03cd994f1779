// qpn_subset.hip -- the row traffic of qpn_solve_nodes_subset_h (gfx950): a caller's compact arrays, slot s belonging to node
// idx[s], against the full-size staging buffers that the node kernels sweep under a launch list.  Three kernels, none of them
// a solver: the list kernel checks idx and writes the launch list, scatter moves rows of w and of the hint z to their nodes'
// places, gather brings the listed nodes' outputs back.  Plain vector loads and stores only.
#include "qpn_internal.h"

namespace {

constexpr int kBlock = 256;

// One array of rows on its way between the two layouts: row r of the compact side, row list[r] of the full-size side.  Strides
// and len in elements; elem = 8 (doubles) or 1 (bytes).  vec: bases and strides admit 16-byte accesses (elem = 8 only).
struct RowJob {
    const void *src;
    void *dst;
    int64_t src_stride, dst_stride;
    int32_t len, elem, vec;
};
struct RowJobs {
    RowJob job[3];
    int32_t jobs;
};

// Lanes that share a row: a whole wavefront once a row has 64 elements, the next power of two over its accesses below that
// (several rows per wavefront).  Host and device agree on it: the grid is sized from it.
__host__ __device__ inline int row_lanes(const RowJob &j)
{
    if (j.len >= WAVE) return WAVE;
    const int acc = j.vec ? (j.len + 1) / 2 : j.len;
    int l = 1;
    while (l < acc) l <<= 1;
    return l;
}

template <class T> __device__ __forceinline__ void copy_row(T *dst, const T *src, int len, int lane, int lanes)
{
    for (int i = lane; i < len; i += lanes) dst[i] = src[i];
}
template <class T> __device__ __forceinline__ void zero_row(T *dst, int len, int lane, int lanes)
{
    for (int i = lane; i < len; i += lanes) dst[i] = T{};
}

// GATHER: dst row r <- src row list[r], zeros where list[r] < 0 (a bad slot).  Scatter: dst row list[r] <- src row r, bad slots
// move nothing.  blockIdx.y = the job; consecutive lanes take consecutive 16-byte (or 8-byte, or 1-byte) pieces of one row.
template <bool GATHER> __device__ __forceinline__ void move_rows(const RowJob &j, int32_t count, const int32_t *list)
{
    const int lanes = row_lanes(j);
    const int64_t r = (int64_t)blockIdx.x * (kBlock / lanes) + threadIdx.x / lanes;
    const int lane = threadIdx.x % lanes;
    if (r >= count || !j.dst) return;
    const int32_t node = list[r];
    if (!GATHER && node < 0) return;
    const int64_t srow = GATHER ? node : r, drow = GATHER ? r : node;
    if (j.elem == 1) {
        uint8_t *d = (uint8_t *)j.dst + drow * j.dst_stride;
        if (node < 0) zero_row(d, j.len, lane, lanes);
        else copy_row(d, (const uint8_t *)j.src + srow * j.src_stride, j.len, lane, lanes);
        return;
    }
    double *d = (double *)j.dst + drow * j.dst_stride;
    const double *s = (const double *)j.src + (node < 0 ? 0 : srow * j.src_stride);
    if (j.vec) {
        const int pairs = j.len >> 1;
        if (node < 0) zero_row((double2 *)d, pairs, lane, lanes);
        else copy_row((double2 *)d, (const double2 *)s, pairs, lane, lanes);
        if ((j.len & 1) && lane == 0) d[j.len - 1] = node < 0 ? 0.0 : s[j.len - 1];
    } else if (node < 0) zero_row(d, j.len, lane, lanes);
    else copy_row(d, s, j.len, lane, lanes);
}

// One thread per slot: in range, and the first to claim its node?  The winner's node goes to the launch list; a loser -- an
// entry out of range, or one that another slot has claimed -- leaves -1 there, which the node kernels skip and gather reports.
// slot_of and list arrive filled with -1.
__global__ __launch_bounds__(kBlock) void subset_list(int32_t count, int32_t batch, const int32_t *__restrict__ idx,
                                                      int32_t *__restrict__ slot_of, int32_t *__restrict__ list)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= count) return;
    const int32_t v = idx[s];
    const bool ok = (uint32_t)v < (uint32_t)batch && atomicCAS(&slot_of[v], -1, (int32_t)s) == -1;
    list[s] = ok ? v : -1;
}

__global__ __launch_bounds__(kBlock) void subset_scatter(RowJobs js, int32_t count, const int32_t *__restrict__ list)
{
    move_rows<false>(js.job[blockIdx.y], count, list);
}

// blockIdx.y < js.jobs: a row job; the last y: status, resid, pivots, one thread per slot
__global__ __launch_bounds__(kBlock) void subset_gather(RowJobs js, int32_t count, const int32_t *__restrict__ list,
                                                        const int32_t *__restrict__ st_full, const double *__restrict__ res_full,
                                                        const int32_t *__restrict__ pv_full, int32_t *__restrict__ status,
                                                        double *__restrict__ resid, int32_t *__restrict__ pivots)
{
    if ((int)blockIdx.y < js.jobs) { move_rows<true>(js.job[blockIdx.y], count, list); return; }
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= count) return;
    const int32_t node = list[s];
    status[s] = node < 0 ? (int32_t)QPN_FAILURE : st_full[node];
    if (resid) resid[s] = node < 0 ? 0.0 : res_full[node];
    if (pivots) pivots[s] = node < 0 ? 0 : pv_full[node];
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

RowJob rows_f64(const double *src, int64_t src_stride, double *dst, int64_t dst_stride, int32_t len)
{
    const bool vec = aligned16(src) && aligned16(dst) && !(src_stride & 1) && !(dst_stride & 1);
    return RowJob{src, dst, src_stride, dst_stride, len, 8, vec ? 1 : 0};
}

unsigned row_blocks(const RowJob &j, int32_t count)
{
    const int per = kBlock / row_lanes(j);
    return (unsigned)(((int64_t)count + per - 1) / per);
}

} // namespace

hipError_t qpn_launch_subset_list(int32_t count, int32_t batch, const int32_t *idx, int32_t *slot_of, int32_t *list,
                                  hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(subset_list, dim3((unsigned)((count + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, count, batch, idx,
                       slot_of, list);
    return hipGetLastError();
}

hipError_t qpn_launch_subset_scatter(int32_t count, const int32_t *list, int32_t p, int32_t N, const double *w, int64_t stride_w,
                                     double *w_full, const double *z, double *z_full, hipStream_t stream)
{
    RowJobs js{};
    if (w && p > 0) js.job[js.jobs++] = rows_f64(w, stride_w, w_full, p, p);
    if (z) js.job[js.jobs++] = rows_f64(z, N, z_full, N, N);
    if (count <= 0 || !js.jobs) return hipSuccess;
    unsigned blocks = 0;
    for (int k = 0; k < js.jobs; ++k) { const unsigned b = row_blocks(js.job[k], count); if (b > blocks) blocks = b; }
    hipLaunchKernelGGL(subset_scatter, dim3(blocks, (unsigned)js.jobs), dim3(kBlock), 0, stream, js, count, list);
    return hipGetLastError();
}

hipError_t qpn_launch_subset_gather(int32_t count, const int32_t *list, int32_t n, int32_t N, const SubsetRows &full,
                                    const SubsetRows &out, double *x, int64_t stride_x, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    RowJobs js{};
    if (out.z) js.job[js.jobs++] = rows_f64(full.z, N, out.z, N, N);
    if (x) js.job[js.jobs++] = rows_f64(full.z, N, x, stride_x, n);
    if (out.active) {
        // rows of N bytes move as doubles where N and the addresses allow it
        if (N % 8 == 0 && !((uintptr_t)full.active & 7) && !((uintptr_t)out.active & 7))
            js.job[js.jobs++] = rows_f64((const double *)full.active, N / 8, (double *)out.active, N / 8, N / 8);
        else js.job[js.jobs++] = RowJob{full.active, out.active, N, N, N, 1, 0};
    }
    unsigned blocks = (unsigned)((count + kBlock - 1) / kBlock);
    for (int k = 0; k < js.jobs; ++k) { const unsigned b = row_blocks(js.job[k], count); if (b > blocks) blocks = b; }
    hipLaunchKernelGGL(subset_gather, dim3(blocks, (unsigned)js.jobs + 1), dim3(kBlock), 0, stream, js, count, list, full.status,
                       full.resid, full.pivots, out.status, out.resid, out.pivots);
    return hipGetLastError();
}
