// qpn_tree.hip -- the intersection tree of combine walked breadth first on the device (qpn_intersection_trees).
//
// IntersectionRoot (src/intersection.jl:55-138) walks, per node, the tree whose depth-t nodes are the intersections of one piece
// from each of the first t unions, and never visits the subtree under a prefix that is empty (:74, :83).  Here all trees of a call
// advance one depth at a time.  The arithmetic of a candidate is the existing job of qpn_launch_exemplar_products (qpn_lp.hip,
// untouched); this unit is the frontier machinery around it:
//
//   tree_csr_kernel      list_ptr as a whole ascends within list_mem, or no tree of the call is walked (lists must not overlap).
//   tree_check_kernel    one wavefront per tree, a lane per list: every index the walk will read through is checked once, a bad
//                        tree answers tree_leaves = -1 and forms no candidate; F_0 (one empty tuple per tree) is written.
//   tree_near_kernel     one wavefront per list: a lane per pool row of the named piece, AND over the piece, the near members
//                        compacted in order next to their complement flags.
//   tree_scan_kernel     ONE workgroup: exclusive scan of the parents' list widths in chunks of kTreeScan, a running sum carried
//                        from chunk to chunk -- no workgroup ever waits for another.  Writes the depth's candidate count.
//   tree_expand_kernel   a thread per candidate: its parent by bisection of the scan, its tuple, its rows n, a histogram of n.
//   tree_bucket_kernel   one workgroup per n that occurs: a stable selection of the candidates of that n (the same chunked scan)
//                        into the bucket's run of the factors array -- ProdArgs has one n per launch -- and the canonical
//                        candidate's place there.
//   tree_keep_kernel     ONE workgroup: the verdicts read back at the canonical positions, a stable scan of the kept ones.
//   tree_move_kernel     a thread per candidate: the kept tuples to the next frontier, or at depth L to the leaves.
//
// The host reads one small header back per depth (the histogram and the counts): it needs them to size the LP launches.  Plain
// C++ throughout; every value is written with vector stores.
#include <type_traits>

#include "qpn_internal.h"

namespace {

constexpr int kTreeScan = 1024;                  // threads of the single-workgroup scans
constexpr int kTreeThreads = 256;
constexpr int kTreeBuckets = QPN_EX_MAX_N + 1;   // hist[n], n = 1 .. 511
constexpr size_t kTreeLpBudget = size_t(64) << 20;

struct TreeHdr {                                 // what the host reads back per depth
    int32_t hist[kTreeBuckets];
    long long C, nF;                             // the depth's candidates; the tuples of the frontier
    int32_t overflow, csr_bad;                   // csr_bad: list_ptr is not ascending within list_mem (tree_csr_kernel)
};

struct TreeWs {
    TreeHdr *hdr;
    int32_t *nmem, *ncnt, *nsol;                 // near members per list (in the list's own run of list_mem's index space), counts
    uint8_t *ncomp;
    long long *off;                              // [capF] the scan
    int32_t *ftup, *ftree, *fn;                  // the frontier: [capF][L], [capF], [capF]
    uint8_t *fallc;
    int32_t *ctup, *ctree, *cn, *pos, *dst;      // the candidates, canonical order: [cap][L], [cap] ...
    uint8_t *callc;
    int32_t *bfac, *bhow;                        // by bucket: factors [cap][L], how
    uint8_t *bnear, *bempty;
    void *gws;
    size_t gws_bytes;
};

// exclusive prefix of v over the workgroup's kTreeScan threads; total: the sum.  wsum: kTreeScan / 64 + 1 words of LDS.
template <class T> __device__ T tree_block_scan(T v, T *wsum, T &total)
{
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    constexpr int nw = kTreeScan / WAVE;
    T inc = v;
    for (int o = 1; o < WAVE; o <<= 1) {
        const T y = __shfl_up(inc, o, WAVE);
        if (lane >= o) inc += y;
    }
    if (lane == WAVE - 1) wsum[w] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        T s = 0;
        for (int i = 0; i < nw; ++i) { const T x = wsum[i]; wsum[i] = s; s += x; }
        wsum[nw] = s;
    }
    __syncthreads();
    total = wsum[nw];
    const T r = wsum[w] + inc - v;
    __syncthreads();                             // (wsum is written again by the next chunk)
    return r;
}

// list_ptr as a whole: 0 <= list_ptr[i] <= list_ptr[i + 1] <= members for every i.  Lists that overlap in list_mem would share their
// slots of nmem / ncomp, and they can overlap only where the offsets decrease: then no tree of the call is walked.  (hdr was zeroed
// before; every thread that finds a fault stores the same 1.)
__global__ __launch_bounds__(kTreeThreads) void tree_csr_kernel(TreeArgs a, TreeWs w)
{
    const long long TL = (long long)a.trees * a.L;
    for (long long i = (long long)blockIdx.x * kTreeThreads + threadIdx.x; i < TL; i += (long long)gridDim.x * kTreeThreads) {
        const int p0 = a.list_ptr[i], p1 = a.list_ptr[i + 1];
        if (p0 < 0 || p1 < p0 || p1 > a.members) w.hdr->csr_bad = 1;
    }
}

__global__ __launch_bounds__(WAVE) void tree_check_kernel(TreeArgs a, TreeWs w)
{
    __shared__ int s_bad, s_sum;
    const int g = blockIdx.x, t = threadIdx.x;
    if (t == 0) { s_bad = 0; s_sum = 0; }
    __syncthreads();
    if (t < a.L) {
        const size_t li = (size_t)g * a.L + t;
        const int p0 = a.list_ptr[li], p1 = a.list_ptr[li + 1], red = a.list_red[li];
        bool bad = p0 < 0 || p1 < p0 || p1 > a.members || red < 0 || red > p1 - p0;
        int longest = 0;
        for (int j = p0; !bad && j < p1; ++j) {
            const int f = a.list_mem[j];
            if (f < 0 || f >= a.pieces) { bad = true; break; }
            const int lo = a.piece_row[f], hi = a.piece_row[f + 1];
            if (lo < 0 || hi <= lo || hi > a.rows) { bad = true; break; }
            longest = max(longest, hi - lo);
        }
        if (bad) atomicOr(&s_bad, 1);
        else atomicAdd(&s_sum, min(longest, QPN_EX_MAX_N + 1));
    }
    __syncthreads();
    if (t == 0) {
        bool bad = s_bad || s_sum > QPN_EX_MAX_N || w.hdr->csr_bad;
        if (a.point) { const int po = a.point_of[g]; bad = bad || po < 0 || po >= a.points; }
        a.tree_leaves[g] = bad ? -1 : 0;
        w.ftree[g] = g; w.fn[g] = 0; w.fallc[g] = 1;                         // F_0
        if (g == 0) {
            w.hdr->C = 0; w.hdr->nF = a.trees; w.hdr->overflow = 0;
            *a.n_leaves = 0; *a.overflow = 0;
        }
    }
    if (g == 0 && t < a.L) { a.tested[t] = 0; a.alive[t] = 0; a.unanswered[t] = 0; }
}

__global__ __launch_bounds__(WAVE) void tree_near_kernel(TreeArgs a, TreeWs w)
{
    const size_t li = blockIdx.x;
    const int g = (int)(li / a.L), lane = threadIdx.x;
    int cnt = 0, sol = 0;
    if (a.tree_leaves[g] >= 0) {                                             // (a bad tree: nothing is read through its indices)
        const int p0 = a.list_ptr[li], p1 = a.list_ptr[li + 1], red = a.list_red[li];
        const double *p = a.point ? a.point + (size_t)a.point_of[g] * a.d : nullptr;
        for (int j = p0; j < p1; ++j) {
            const int f = a.list_mem[j];
            bool ok = true;
            if (p) {
                const int lo = a.piece_row[f], hi = a.piece_row[f + 1];
                for (int r = lo + lane; r < hi; r += WAVE) {
                    const double *ar = a.A + (size_t)r * a.d;
                    double acc = 0.0;
                    for (int c = 0; c < a.d; ++c) acc = acc + ar[c] * p[c];
                    ok = ok && (a.l[r] - a.point_tol <= acc) && (acc - a.point_tol <= a.u[r]);
                }
            }
            if (__all(ok)) {
                const bool comp = j >= p1 - red;
                if (lane == 0) { w.nmem[p0 + cnt] = f; w.ncomp[p0 + cnt] = comp ? 1 : 0; }
                ++cnt;
                if (!comp) ++sol;
            }
        }
    }
    if (lane == 0) { w.ncnt[li] = cnt; w.nsol[li] = sol; }
}

// depth t (1-based): off[p] = the first candidate of parent p; at t = L a parent made of complement pieces alone takes the solution
// pieces of its list only (they come first: the redzone is the tail of a list)
__global__ __launch_bounds__(kTreeScan) void tree_scan_kernel(TreeArgs a, TreeWs w, int t)
{
    __shared__ long long wsum[kTreeScan / WAVE + 1];
    const int tid = threadIdx.x;
    const long long nF = w.hdr->nF;
    const bool last = t == a.L;
    long long run = 0;
    for (long long base = 0; base < nF; base += kTreeScan) {
        const long long p = base + tid;
        long long width = 0;
        if (p < nF) {
            const size_t li = (size_t)w.ftree[p] * a.L + (t - 1);
            width = last && w.fallc[p] ? w.nsol[li] : w.ncnt[li];
        }
        long long total;
        const long long excl = tree_block_scan<long long>(width, wsum, total);
        if (p < nF) w.off[p] = run + excl;
        run += total;
    }
    for (int i = tid; i < kTreeBuckets; i += kTreeScan) w.hdr->hist[i] = 0;
    if (tid == 0) {
        w.hdr->C = run;
        a.tested[t - 1] = run;
        if (run > a.cap) { w.hdr->overflow = t; *a.overflow = t; }
    }
}

__global__ __launch_bounds__(kTreeThreads) void tree_expand_kernel(TreeArgs a, TreeWs w, int t)
{
    const long long C = w.hdr->C, nF = w.hdr->nF;
    if (C > a.cap) return;
    const int L = a.L;
    for (long long c = (long long)blockIdx.x * kTreeThreads + threadIdx.x; c < C; c += (long long)gridDim.x * kTreeThreads) {
        long long lo = 0, hi = nF;                                           // the last parent whose first candidate is <= c
        while (hi - lo > 1) {
            const long long mid = (lo + hi) >> 1;
            if (w.off[mid] <= c) lo = mid; else hi = mid;
        }
        const long long p = lo;
        const int j = (int)(c - w.off[p]), g = w.ftree[p];
        const size_t li = (size_t)g * L + (t - 1);
        const int p0 = a.list_ptr[li], f = w.nmem[p0 + j];
        const int n = w.fn[p] + (a.piece_row[f + 1] - a.piece_row[f]);
        int32_t *tup = w.ctup + (size_t)c * L;
        const int32_t *par = w.ftup + (size_t)p * L;
        for (int s = 0; s < L; ++s) tup[s] = s < t - 1 ? par[s] : s == t - 1 ? f : -1;
        w.ctree[c] = g; w.cn[c] = n; w.callc[c] = w.fallc[p] && w.ncomp[p0 + j] ? 1 : 0;
        if (n >= 1 && n < kTreeBuckets) atomicAdd(&w.hdr->hist[n], 1);
    }
}

// workgroup b: the candidates of n = n0 + b, in canonical order, to the run of the factors array that starts after the smaller n's
__global__ __launch_bounds__(kTreeScan) void tree_bucket_kernel(TreeArgs a, TreeWs w, int n0, int C)
{
    __shared__ int wsum[kTreeScan / WAVE + 1];
    __shared__ int s_base;
    const int n = n0 + blockIdx.x, tid = threadIdx.x, L = a.L;
    if (w.hdr->hist[n] == 0) return;                                         // (the whole workgroup)
    if (tid == 0) {
        int b = 0;
        for (int m = 1; m < n; ++m) b += w.hdr->hist[m];
        s_base = b;
    }
    __syncthreads();
    int run = s_base;
    for (int base = 0; base < C; base += kTreeScan) {
        const int c = base + tid;
        const int flag = c < C && w.cn[c] == n ? 1 : 0;
        int total;
        const int excl = tree_block_scan<int>(flag, wsum, total);
        if (flag) {
            const int i = run + excl;
            w.pos[c] = i;
            const int32_t *tup = w.ctup + (size_t)c * L;
            int32_t *fac = w.bfac + (size_t)i * L;
            for (int s = 0; s < L; ++s) fac[s] = tup[s];
        }
        run += total;
    }
}

__global__ __launch_bounds__(kTreeScan) void tree_keep_kernel(TreeArgs a, TreeWs w, int t, int C)
{
    __shared__ int wsum[kTreeScan / WAVE + 1];
    __shared__ int s_un;
    const int tid = threadIdx.x;
    if (tid == 0) s_un = 0;
    __syncthreads();
    int run = 0, un = 0;
    for (int base = 0; base < C; base += kTreeScan) {
        const int c = base + tid;
        int keep = 0;
        if (c < C) {
            const int i = w.pos[c];
            keep = w.bempty[i] == 0 ? 1 : 0;
            const int how = w.bhow[i];
            if (keep && (how == QPN_EX_ITER_LIMIT || how == QPN_EX_FAILURE)) ++un;
        }
        int total;
        const int excl = tree_block_scan<int>(keep, wsum, total);
        if (c < C) w.dst[c] = keep ? run + excl : -1;
        run += total;
    }
    if (un) atomicAdd(&s_un, un);
    __syncthreads();
    if (tid == 0) {
        a.alive[t - 1] = run; a.unanswered[t - 1] = s_un;
        w.hdr->nF = run;
        if (t == a.L) *a.n_leaves = run;
    }
}

__global__ __launch_bounds__(kTreeThreads) void tree_move_kernel(TreeArgs a, TreeWs w, int t, int C)
{
    const int L = a.L;
    const bool last = t == L;
    for (int c = blockIdx.x * kTreeThreads + threadIdx.x; c < C; c += gridDim.x * kTreeThreads) {
        const int i = w.dst[c];
        if (i < 0) continue;
        const int32_t *tup = w.ctup + (size_t)c * L;
        int32_t *to = (last ? a.leaves : w.ftup) + (size_t)i * L;
        for (int s = 0; s < L; ++s) to[s] = tup[s];
        const int g = w.ctree[c];
        if (last) {
            a.leaf_tree[i] = g; a.leaf_how[i] = w.bhow[w.pos[c]];
            atomicAdd(&a.tree_leaves[g], 1);
        } else {
            w.ftree[i] = g; w.fn[i] = w.cn[c]; w.fallc[i] = w.callc[c];
        }
    }
}

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// the LP workspace: the largest single job, or kTreeLpBudget's worth of jobs when `cap` of them need more
size_t tree_lp_bytes(int32_t cap, int32_t d)
{
    const size_t one = qpn_products_workspace_bytes(1, QPN_EX_MAX_N, d);
    size_t all = (size_t)cap * one;
    if (all > kTreeLpBudget) all = kTreeLpBudget;
    return all > one ? all : one;
}

// carves the workspace (base == nullptr: counts the bytes only)
size_t tree_carve(TreeWs &w, unsigned char *base, int32_t trees, int32_t L, int32_t members, int32_t cap, int32_t d)
{
    size_t at = 0;
    auto take = [&](auto *&ptr, size_t bytes) {
        ptr = reinterpret_cast<std::remove_reference_t<decltype(ptr)>>(base ? base + at : nullptr);
        at += up256(bytes);
    };
    const size_t capF = (size_t)(cap > trees ? cap : trees), cp = (size_t)cap, TL = (size_t)trees * L, M = (size_t)(members > 0 ? members : 1);
    take(w.hdr, sizeof(TreeHdr));
    take(w.nmem, M * 4); take(w.ncomp, M); take(w.ncnt, TL * 4); take(w.nsol, TL * 4);
    take(w.off, capF * 8);
    take(w.ftup, capF * L * 4); take(w.ftree, capF * 4); take(w.fn, capF * 4); take(w.fallc, capF);
    take(w.ctup, cp * L * 4); take(w.ctree, cp * 4); take(w.cn, cp * 4); take(w.pos, cp * 4); take(w.dst, cp * 4); take(w.callc, cp);
    take(w.bfac, cp * L * 4); take(w.bhow, cp * 4); take(w.bnear, cp); take(w.bempty, cp);
    w.gws_bytes = tree_lp_bytes(cap, d);
    take(w.gws, w.gws_bytes);
    return at;
}

unsigned tree_grid(long long items)
{
    const long long g = (items + kTreeThreads - 1) / kTreeThreads;
    return (unsigned)(g < 1 ? 1 : g > 2048 ? 2048 : g);
}

} // namespace

size_t qpn_tree_workspace_bytes(int32_t trees, int32_t L, int32_t members, int32_t cap, int32_t d)
{
    TreeWs w;
    return tree_carve(w, nullptr, trees, L, members, cap, d);
}

#define TREE_LAUNCHED()                                                \
    do {                                                               \
        if (const hipError_t e__ = hipGetLastError(); e__ != hipSuccess) return e__; \
    } while (0)

hipError_t qpn_run_intersection_trees(const TreeArgs &a, void *ws, hipStream_t s)
{
    if (a.trees <= 0) return hipSuccess;
    TreeWs w;
    tree_carve(w, static_cast<unsigned char *>(ws), a.trees, a.L, a.members, a.cap, a.d);
    if (const hipError_t e = hipMemsetAsync(w.hdr, 0, sizeof(TreeHdr), s); e != hipSuccess) return e;
    hipLaunchKernelGGL(tree_csr_kernel, dim3(tree_grid((long long)a.trees * a.L)), dim3(kTreeThreads), 0, s, a, w);
    TREE_LAUNCHED();
    hipLaunchKernelGGL(tree_check_kernel, dim3((unsigned)a.trees), dim3(WAVE), 0, s, a, w);
    TREE_LAUNCHED();
    hipLaunchKernelGGL(tree_near_kernel, dim3((unsigned)((size_t)a.trees * a.L)), dim3(WAVE), 0, s, a, w);
    TREE_LAUNCHED();
    TreeHdr h;
    for (int t = 1; t <= a.L; ++t) {
        hipLaunchKernelGGL(tree_scan_kernel, dim3(1), dim3(kTreeScan), 0, s, a, w, t);
        TREE_LAUNCHED();
        hipLaunchKernelGGL(tree_expand_kernel, dim3(tree_grid(a.cap)), dim3(kTreeThreads), 0, s, a, w, t);
        TREE_LAUNCHED();
        // the depth's one read-back: the LP launches below are sized by it
        if (const hipError_t e = hipMemcpyAsync(&h, w.hdr, sizeof(TreeHdr), hipMemcpyDeviceToHost, s); e != hipSuccess) return e;
        if (const hipError_t e = hipStreamSynchronize(s); e != hipSuccess) return e;
        if (h.overflow || h.C == 0) break;                                  // (3), or every tree is dead: the counts stay 0
        const int C = (int)h.C;
        int n0 = 0, n1 = 0;
        for (int n = 1; n < kTreeBuckets; ++n)
            if (h.hist[n]) { if (!n0) n0 = n; n1 = n; }
        if (!n0) return hipErrorUnknown;                                    // (cannot be: every candidate has 1 .. 511 rows)
        hipLaunchKernelGGL(tree_bucket_kernel, dim3((unsigned)(n1 - n0 + 1)), dim3(kTreeScan), 0, s, a, w, n0, C);
        TREE_LAUNCHED();
        size_t base = 0;
        for (int n = n0; n <= n1; ++n) {
            const size_t count = (size_t)h.hist[n];
            if (!count) continue;
            ProdArgs pa{};
            pa.d = a.d; pa.rows = a.rows; pa.pieces = a.pieces; pa.n = n; pa.k = a.L; pa.points = 0;
            pa.A = a.A; pa.l = a.l; pa.u = a.u; pa.open_lo = a.open_lo; pa.open_hi = a.open_hi; pa.piece_row = a.piece_row;
            pa.point_tol = a.point_tol; pa.tol = a.tol; pa.slack_cap = a.slack_cap;
            pa.lp = a.lp;
            if (pa.lp.max_iters <= 0) pa.lp.max_iters = 50 * (2 * n + 1 + a.d + 1) + 100;
            // qpn_launch_exemplar_products chunks a call over a workspace it takes to be qpn_products_workspace_bytes(products, n, d)
            // large, up to 256 MiB.  Ours is capped at kTreeLpBudget so that a walk does not grow the context workspace by that
            // much: hence this loop, over parts of at most `per` jobs, each of which fits whole (per * bytes of one job <= gws_bytes).
            size_t per = w.gws_bytes / qpn_products_workspace_bytes(1, n, a.d);
            if (per < 1) per = 1;
            for (size_t f = 0; f < count; f += per) {
                const size_t at = base + f;
                pa.products = (int32_t)(count - f < per ? count - f : per);
                pa.factors = w.bfac + at * a.L;
                pa.near = w.bnear + at; pa.empty = w.bempty + at; pa.how = w.bhow + at;
                if (const hipError_t e = qpn_launch_exemplar_products(pa, w.gws, s); e != hipSuccess) return e;
            }
            base += count;
        }
        hipLaunchKernelGGL(tree_keep_kernel, dim3(1), dim3(kTreeScan), 0, s, a, w, t, C);
        TREE_LAUNCHED();
        hipLaunchKernelGGL(tree_move_kernel, dim3(tree_grid(C)), dim3(kTreeThreads), 0, s, a, w, t, C);
        TREE_LAUNCHED();
    }
    return hipSuccess;
}
