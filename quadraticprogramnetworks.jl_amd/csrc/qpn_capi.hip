// qpn_capi.hip -- the extern "C" boundary of libqpn_hip.so (include/qpn_hip.h).
// Host-side staging, argument checking and error mapping only; all arithmetic is in the
// HIP kernels (qpn_avi_*.hip, qpn_kkt.hip, qpn_verify.hip, ...).  No exceptions cross the ABI.
// The node sweep and the resident node handle are qpn_capi_nodes.hip; qpn_capi.h is what the two units share.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "qpn_capi.h"

#ifdef QPN_STAMPS
unsigned long long *g_stamps = nullptr;
#endif

namespace {

// The tolerances of the LP entries' solves over polyhedra of r rows in d variables: the caller's options or, without, the defaults;
// max_iters <= 0 is 50 (r + d) + 100.
LpTol lp_tol(const qpn_lp_opts *opts, int32_t r, int32_t d)
{
    qpn_lp_opts o;
    if (opts) o = *opts; else qpn_lp_default_opts(&o);
    return LpTol{o.piv_tol, o.feas_tol, o.opt_tol, o.check_tol, o.max_iters > 0 ? o.max_iters : 50 * (r + d) + 100};
}

// the number of recipes of one row of masks: the product of its codes' popcounts, saturating
int64_t recipe_count(const uint8_t *row, int N)
{
    int64_t tot = 1;
    for (int i = 0; i < N; ++i) {
        const int r = __builtin_popcount(row[i]);
        if (r > 1) tot = (tot > INT64_MAX / r) ? INT64_MAX : tot * r;
    }
    return tot;
}

// qpn_recipes_batch (first == nullptr: every node's recipes start at number 0 of its product) and qpn_recipes_batch_range
int recipes_batch_any(qpn_ctx *ctx, const char *who, int32_t nodes, int32_t N, const uint8_t *masks, const int64_t *first,
                      const int64_t *offsets, uint8_t *K, int32_t *node_of, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (nodes <= 0 || N <= 0 || !masks || !offsets) return fail_arg(ctx, who, "bad argument");
    Stage st(ctx, mem, who);
    if (int rc = st.check()) return rc;
    if (offsets[0] != 0) return fail_arg(ctx, who, "offsets[0] must be 0");
    for (int b = 0; b < nodes; ++b) {
        if (offsets[b + 1] < offsets[b]) return fail_arg(ctx, who, "offsets must not decrease");
        if (first && first[b] < 0) return fail_arg(ctx, who, "first must not be negative");
    }
    const int64_t total = offsets[nodes];
    if (total == 0) return QPN_OK;
    if (!K || !node_of) return fail_arg(ctx, who, "null output");
    if (total > INT32_MAX) { ctx->last_error = std::string(who) + ": more than 2^31 - 1 recipes in one call"; return QPN_ERR_SIZE; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // every node's range must lie inside its product.  Host masks are checked as they are; device masks are read back for the
    // check (nodes x N bytes) when `first` is given, and are the caller's without it: a count beyond the product wraps around
    // inside the product, it cannot leave the arrays
    std::vector<uint8_t> hm;
    const uint8_t *mk = masks;
    if (!st.host && first) {
        hm.resize((size_t)nodes * N);
        HIPCHK(ctx, hipMemcpyAsync(hm.data(), masks, hm.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        mk = hm.data();
    }
    for (int b = 0; (st.host || first) && b < nodes; ++b) {
        const int64_t tot = recipe_count(mk + (size_t)b * N, N), cnt = offsets[b + 1] - offsets[b], f = first ? first[b] : 0;
        if (cnt > 0 && (f >= tot || cnt > tot - f)) return fail_arg(ctx, who, "a node asks for recipes beyond its product");
    }
    const long long *doff, *dfirst = nullptr; const uint8_t *dm; uint8_t *dK; int32_t *dno;
    st.lib_in(doff, offsets, (size_t)(nodes + 1) * 8);
    if (first) st.lib_in(dfirst, first, (size_t)nodes * 8);
    st.in(dm, masks, (size_t)nodes * N); st.out(dK, K, (size_t)total * N); st.out(dno, node_of, (size_t)total * 4);
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    // (offsets and first are the caller's host arrays, which may be pageable: the copies must be done before the call returns)
    HIPCHK(ctx, hipStreamSynchronize(s));
    HIPCHK(ctx, qpn_launch_recipes_batch(nodes, N, dm, doff, total, dK, dno, s, dfirst));
    return st.finish();
}

// what qpn_local_pieces and qpn_reduced_pieces ask of the arguments they share (`outputs`: none of the entry's own is null)
int pieces_check(qpn_ctx *ctx, const char *who, bool host, int32_t pieces, int32_t nodes, int32_t n, int32_t m, int32_t p,
                 const double *Qd, const double *R, const double *qd, const double *Ad, const double *B, const double *l,
                 const double *u, const int32_t *node_of, const uint8_t *K, bool outputs)
{
    if (pieces < 0 || nodes <= 0 || n <= 0 || m < 0 || p < 0) return fail_arg(ctx, who, "bad sizes");
    if (pieces == 0) return QPN_OK;
    if (n + m > 512) { ctx->last_error = std::string(who) + ": n + m <= 512 in ABI v1"; return QPN_ERR_SIZE; }
    if (!Qd || !qd || (m > 0 && (!Ad || !l || !u)) || (p > 0 && (!R || (m > 0 && !B))) || !K || !outputs)
        return fail_arg(ctx, who, "null pointer");
    if (!node_of && nodes < pieces) return fail_arg(ctx, who, "fewer record sets than pieces and no node_of");
    for (int t = 0; t < pieces && host && node_of; ++t)
        if (node_of[t] < 0 || node_of[t] >= nodes) return fail_arg(ctx, who, "node_of outside 0..nodes-1");
    return QPN_OK;
}

} // namespace

extern "C" {

int qpn_abi_version(void) { return QPN_ABI_VERSION; }

const char *qpn_strerror(int code)
{
    switch (code) {
    case QPN_OK: return "ok";
    case QPN_ERR_ARG: return "bad argument";
    case QPN_ERR_HIP: return "HIP runtime error";
    case QPN_ERR_NODEVICE: return "no gfx950 device visible";
    case QPN_ERR_SIZE: return "problem size not supported";
    default: return "unknown error";
    }
}

void qpn_avi_default_opts(qpn_avi_opts *o)
{
    if (!o) return;
    o->check_tol = 1e-6;   // src/avi.jl:148
    o->piv_tol = 1e-11;
    o->feas_tol = 1e-12;
    o->comp_tol = 1e-2;    // src/avi_solutions.jl:511
    o->max_pivots = 0;
    o->flags = 0;
}

int qpn_ctx_create(int device_id, qpn_ctx **out)
{
    if (!out) return QPN_ERR_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return QPN_ERR_NODEVICE;
    if (device_id < 0 || device_id >= count) return QPN_ERR_ARG;
    qpn_ctx *ctx = new (std::nothrow) qpn_ctx();
    if (!ctx) return QPN_ERR_ARG;
    ctx->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess) { delete ctx; return QPN_ERR_HIP; }
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx; return QPN_ERR_HIP;
    }
    ctx->stream = ctx->own_stream;
    *out = ctx;
    return QPN_OK;
}

int qpn_ctx_set_option(qpn_ctx *ctx, int32_t option, int32_t value)
{
    if (!ctx) return QPN_ERR_ARG;
    switch (option) {
    case QPN_OPT_MID_ROUTE:
        if (value < 0 || value > 1) return fail_arg(ctx, "qpn_ctx_set_option: QPN_OPT_MID_ROUTE takes 0 or 1");
        if (ctx->mid_route != value) ctx->route_epoch++;
        ctx->mid_route = value;
        return QPN_OK;
    case QPN_OPT_BIG_ROUTE:
        if (value != 1) return fail_arg(ctx, "qpn_ctx_set_option: QPN_OPT_BIG_ROUTE takes 1 (round 2's route over an assembled M is gone)");
        return QPN_OK;
    case QPN_OPT_SYM_ROUTE:
        if (value < 0 || value > 1) return fail_arg(ctx, "qpn_ctx_set_option: QPN_OPT_SYM_ROUTE takes 0 or 1");
        if (ctx->sym_route != value) ctx->route_epoch++;
        ctx->sym_route = value;
        return QPN_OK;
    case QPN_OPT_CRASH_CACHE:
        // (no new route epoch: cached sweeps return the same bits, so what a handle knows about its declines stays true)
        if (value < 0 || value > 1) return fail_arg(ctx, "qpn_ctx_set_option: QPN_OPT_CRASH_CACHE takes 0 or 1");
        ctx->crash_cache = value;
        return QPN_OK;
    case QPN_OPT_CRASH_CACHE_BIG:
        // (no new route epoch either: the same bits, the same declines)
        if (value < 0 || value > 1) return fail_arg(ctx, "qpn_ctx_set_option: QPN_OPT_CRASH_CACHE_BIG takes 0 or 1");
        ctx->crash_cache_big = value;
        return QPN_OK;
    case QPN_OPT_WARM_BIG:
        // (no new route epoch: the same nodes decline, stage A does not see the hint)
        if (value < 0 || value > 1) return fail_arg(ctx, "qpn_ctx_set_option: QPN_OPT_WARM_BIG takes 0 or 1");
        ctx->warm_big = value;
        return QPN_OK;
    case QPN_OPT_LLC_BUDGET_MB:
        // (a cache policy of the loads: the same bits either way, no new route epoch)
        if (value < -1) return fail_arg(ctx, "qpn_ctx_set_option: QPN_OPT_LLC_BUDGET_MB takes a size in MiB, 0 (never stream) or -1 (always)");
        ctx->llc_budget_mb = value;
        return QPN_OK;
    default:
        return fail_arg(ctx, "qpn_ctx_set_option: unknown option");
    }
}

int qpn_ctx_destroy(qpn_ctx *ctx)
{
    if (!ctx) return QPN_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->ws) (void)hipFree(ctx->ws);
    if (ctx->order) (void)hipFree(ctx->order);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return QPN_OK;
}

int qpn_ctx_set_stream(qpn_ctx *ctx, void *hip_stream)
{
    if (!ctx) return QPN_ERR_ARG;
    hipStream_t ns = static_cast<hipStream_t>(hip_stream);   // NULL = HIP's legacy default stream
    // the workspace is shared by all entry points and carved from offset 0 by each: launches still running on the
    // stream that is being left may be using it
    if (ns != ctx->stream) { HIPCHK(ctx, hipSetDevice(ctx->device)); HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); }
    ctx->stream = ns;
    return QPN_OK;
}

int qpn_ctx_use_own_stream(qpn_ctx *ctx)
{
    if (!ctx) return QPN_ERR_ARG;
    if (ctx->stream != ctx->own_stream) { HIPCHK(ctx, hipSetDevice(ctx->device)); HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); }
    ctx->stream = ctx->own_stream;
    return QPN_OK;
}

int qpn_ctx_synchronize(qpn_ctx *ctx)
{
    if (!ctx) return QPN_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return QPN_OK;
}

const char *qpn_ctx_last_error(qpn_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }

#ifdef QPN_DIAG
// diagnostic builds only: run Stage A of the MFMA Schur kernel and dump S, c, W, h (device pointers)
int qpn_debug_schur_stage_a(qpn_ctx *ctx, int32_t batch, int32_t N, const double *M, const double *q,
                            const double *l, const double *u, const uint8_t *kind, int32_t *status,
                            double *S, double *c, double *W, double *h)
{
    AviBatchArgs a{};
    a.batch = batch; a.N = N; a.M = M; a.strideM = (int64_t)N * N; a.q = q; a.l = l; a.u = u; a.kind = kind;
    a.stride_kind = N; a.status = status;
    if (qpn_launch_avi_solve_schur(a, S, c, W, h, ctx->stream) != hipSuccess) return QPN_ERR_HIP;
    return hipStreamSynchronize(ctx->stream) == hipSuccess ? QPN_OK : QPN_ERR_HIP;
}
#endif

#ifdef QPN_STAMPS
// diagnostic builds only: where the next device-path solve writes its [batch][8] cycle sums
int qpn_debug_set_stamps(void *p) { g_stamps = static_cast<unsigned long long *>(p); return 0; }
#endif

// -------------------------------------------------------------------------------------------
int qpn_solve_avi_batch(qpn_ctx *ctx, int32_t batch, int32_t N, const double *M, int64_t strideM,
                        const double *q, const double *l, const double *u, const uint8_t *kind,
                        int64_t stride_kind, double *z, int32_t *status, double *resid,
                        int32_t *pivots, uint8_t *active, const qpn_avi_opts *opts, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (batch < 0 || N <= 0) return fail_arg(ctx, "qpn_solve_avi_batch: batch < 0 or N <= 0");
    if (batch == 0) return QPN_OK;
    if (!M || !q || !l || !u || !z || !status) return fail_arg(ctx, "qpn_solve_avi_batch: null pointer");
    if (strideM != 0 && strideM < (int64_t)N * N) return fail_arg(ctx, "qpn_solve_avi_batch: strideM < N*N");
    if (kind && stride_kind != 0 && stride_kind < N) return fail_arg(ctx, "qpn_solve_avi_batch: stride_kind < N");
    if (N > qpn_avi_max_n()) { ctx->last_error = "qpn_solve_avi_batch: N > 1024 not supported by ABI v1"; return QPN_ERR_SIZE; }
    const bool big = N > 64;   // one workgroup per item, dictionary in a workspace (qpn_avi_big.hip)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    qpn_avi_opts o;
    if (opts) o = *opts; else qpn_avi_default_opts(&o);

    AviBatchArgs a{};
    a.batch = batch; a.N = N; a.strideM = strideM; a.stride_kind = kind ? stride_kind : 0;
    a.check_tol = o.check_tol; a.piv_tol = o.piv_tol; a.feas_tol = o.feas_tol; a.comp_tol = o.comp_tol;
    a.max_pivots = o.max_pivots;
    a.flags = o.flags & 0xFFFF;           // (the upper bits are internal: QPN_AVI_IFLAG_*)
#ifdef QPN_STAMPS
    if (mem == QPN_MEM_DEVICE) a.stamps = g_stamps;
#endif

    const size_t bN = (size_t)batch * N;
    const size_t mBytes = sizeof(double) * (strideM ? (size_t)(batch - 1) * strideM + (size_t)N * N : (size_t)N * N);
    const size_t kBytes = kind ? (stride_kind ? (size_t)(batch - 1) * stride_kind + N : (size_t)N) : 0;
    Stage st(ctx, mem, "qpn_solve_avi_batch");
    st.in(a.M, M, mBytes); st.in(a.q, q, bN * 8); st.in(a.l, l, bN * 8); st.in(a.u, u, bN * 8);
    st.inout(a.z, z, bN * 8, true); st.in(a.kind, kind, kBytes);
    st.out(a.status, status, (size_t)batch * 4); st.out(a.resid, resid, (size_t)batch * 8);
    st.out(a.pivots, pivots, (size_t)batch * 4); st.out(a.active, active, bN);
    double *wsb = nullptr;
    if (big) st.scratch(wsb, qpn_avi_big_workspace_bytes(batch, N));
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    if (big) HIPCHK(ctx, qpn_launch_avi_solve_big(a, wsb, ctx->stream));
    else HIPCHK(ctx, qpn_launch_avi_solve(a, ctx->stream));
    return st.finish();
}

int qpn_solve_mcp_csc(qpn_ctx *ctx, int32_t N, const int32_t *colptr, const int32_t *rowval,
                      const double *nzval, const double *q, const double *l, const double *u,
                      double *z, int32_t *status, double *resid, int32_t *pivots,
                      const qpn_avi_opts *opts)
{
    if (!ctx) return QPN_ERR_ARG;
    if (N <= 0 || !colptr || !q || !l || !u || !z || !status) return fail_arg(ctx, "qpn_solve_mcp_csc: bad argument");
    const int32_t nnz = colptr[N] - 1;
    if (nnz < 0 || (nnz > 0 && (!rowval || !nzval))) return fail_arg(ctx, "qpn_solve_mcp_csc: bad CSC arrays");
    std::vector<double> dense((size_t)N * N, 0.0);
    for (int32_t j = 0; j < N; ++j) {
        for (int32_t t = colptr[j] - 1; t < colptr[j + 1] - 1; ++t) {
            int32_t i = rowval[t] - 1;
            if (i < 0 || i >= N) return fail_arg(ctx, "qpn_solve_mcp_csc: row index out of range");
            dense[(size_t)j * N + i] += nzval[t];
        }
    }
    return qpn_solve_avi_batch(ctx, 1, N, dense.data(), 0, q, l, u, nullptr, 0, z, status, resid,
                               pivots, nullptr, opts, QPN_MEM_HOST);
}

// -------------------------------------------------------------------------------------------
int qpn_check_avi_batch(qpn_ctx *ctx, int32_t batch, int32_t N, const double *M, int64_t strideM,
                        const double *q, const double *l, const double *u, const uint8_t *kind,
                        int64_t stride_kind, const double *z, double tol, int32_t *degree,
                        double *r, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (batch < 0 || N <= 0) return fail_arg(ctx, "qpn_check_avi_batch: bad sizes");
    if (batch == 0) return QPN_OK;
    if (!M || !q || !l || !u || !z || !degree) return fail_arg(ctx, "qpn_check_avi_batch: null pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t bN = (size_t)batch * N;
    const size_t mBytes = sizeof(double) * (strideM ? (size_t)(batch - 1) * strideM + (size_t)N * N : (size_t)N * N);
    const size_t kBytes = kind ? (stride_kind ? (size_t)(batch - 1) * stride_kind + N : (size_t)N) : 0;
    const double *dM, *dq, *dl, *du, *dz; const uint8_t *dk; int32_t *dd; double *dr;
    Stage st(ctx, mem, "qpn_check_avi_batch");
    st.in(dM, M, mBytes); st.in(dq, q, bN * 8); st.in(dl, l, bN * 8); st.in(du, u, bN * 8); st.in(dz, z, bN * 8);
    st.in(dk, kind, kBytes);
    st.out(dd, degree, (size_t)batch * 4); st.out(dr, r, bN * 8);
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_check_avi(batch, N, dM, strideM, dq, dl, du, dk, kind ? stride_kind : 0, dz, tol, dd, dr, ctx->stream));
    return st.finish();
}

int qpn_comp_indices(qpn_ctx *ctx, int64_t count, const double *zv, const double *rv,
                     const double *l, const double *u, double tol, int32_t shift, uint8_t *mask,
                     int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (count < 0 || (shift != 0 && shift != 4)) return fail_arg(ctx, "qpn_comp_indices: bad count/shift");
    if (count == 0) return QPN_OK;
    if (!zv || !rv || !l || !u || !mask) return fail_arg(ctx, "qpn_comp_indices: null pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nb = (size_t)count * 8;
    const double *dz, *dr, *dl, *du; uint8_t *dm;
    Stage st(ctx, mem, "qpn_comp_indices");
    st.in(dz, zv, nb); st.in(dr, rv, nb); st.in(dl, l, nb); st.in(du, u, nb); st.out(dm, mask, (size_t)count);
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_comp_indices(count, dz, dr, dl, du, tol, shift, dm, ctx->stream));
    return st.finish();
}

int qpn_assemble_nodes(qpn_ctx *ctx, int32_t batch, int32_t n, int32_t m, int32_t p,
                       const double *Qd, const double *R, const double *qd, const double *Ad,
                       const double *B, const double *l, const double *u, const double *w,
                       int64_t stride_w, double *Mout, double *qout, double *lout, double *uout,
                       uint8_t *kind_out, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (batch < 0 || n <= 0 || m < 0 || p < 0) return fail_arg(ctx, "qpn_assemble_nodes: bad sizes");
    if (batch == 0) return QPN_OK;
    if (!Qd || !qd || (m > 0 && (!Ad || !l || !u)) || (p > 0 && (!R || !w || (m > 0 && !B))) || !Mout || !qout ||
        !lout || !uout || !kind_out)
        return fail_arg(ctx, "qpn_assemble_nodes: null pointer");
    if (stride_w != 0 && stride_w < p) return fail_arg(ctx, "qpn_assemble_nodes: stride_w < p");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const NodeSizes sz = node_sizes(batch, n, m, p, stride_w);
    const int N = n + m;
    const size_t bN = (size_t)batch * N;
    NodeDev d{};
    double *dM, *dqo, *dlo, *duo; uint8_t *dk;
    Stage st(ctx, mem, "qpn_assemble_nodes");
    stage_records(st, d, sz, Qd, R, qd, Ad, B, l, u);
    st.in(d.w, w, sz.w, 8);
    st.out(dM, Mout, bN * N * 8); st.out(dqo, qout, bN * 8); st.out(dlo, lout, bN * 8); st.out(duo, uout, bN * 8);
    st.out(dk, kind_out, bN);
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_assemble_nodes(batch, n, m, p, d.Q, d.R, d.q, d.A, d.B, d.l, d.u, d.w, stride_w, dM, dqo, dlo, duo, dk,
                                          ctx->stream));
    return st.finish();
}

// ---- (F1) local pieces ------------------------------------------------------------------------------------------
int qpn_recipes_from_masks(qpn_ctx *ctx, int32_t N, const uint8_t *mask, int64_t first, int32_t count, uint8_t *K,
                           int64_t *total, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (N <= 0 || !mask || first < 0 || count < 0 || (count > 0 && !K)) return fail_arg(ctx, "qpn_recipes_from_masks: bad argument");
    Stage st(ctx, mem, "qpn_recipes_from_masks");
    if (int rc = st.check()) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    std::vector<uint8_t> hm((size_t)N);
    if (st.host) memcpy(hm.data(), mask, (size_t)N);
    else { HIPCHK(ctx, hipMemcpyAsync(hm.data(), mask, (size_t)N, hipMemcpyDeviceToHost, s)); HIPCHK(ctx, hipStreamSynchronize(s)); }
    const int64_t tot = recipe_count(hm.data(), N);
    if (total) *total = tot;
    if (count == 0) return QPN_OK;
    if (first >= tot || (int64_t)count > tot - first) return fail_arg(ctx, "qpn_recipes_from_masks: first + count beyond the number of recipes");
    const uint8_t *dm; uint8_t *dK;
    st.in(dm, mask, (size_t)N); st.out(dK, K, (size_t)count * N);
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_recipes(N, dm, first, count, dK, s));
    return st.finish();
}

int qpn_recipes_batch(qpn_ctx *ctx, int32_t nodes, int32_t N, const uint8_t *masks, const int64_t *offsets, uint8_t *K,
                      int32_t *node_of, int mem)
{
    return recipes_batch_any(ctx, "qpn_recipes_batch", nodes, N, masks, nullptr, offsets, K, node_of, mem);
}

int qpn_reduced_pieces(qpn_ctx *ctx, int32_t pieces, int32_t nodes, int32_t n, int32_t m, int32_t p, const double *Qd,
                       const double *R, const double *qd, const double *Ad, const double *B, const double *l,
                       const double *u, const int32_t *node_of, const uint8_t *K, double tol, double *Ar, double *lr, double *ur,
                       int32_t *rows, int32_t *flags, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    Stage st(ctx, mem, "qpn_reduced_pieces");
    if (int rc = pieces_check(ctx, st.who, st.host, pieces, nodes, n, m, p, Qd, R, qd, Ad, B, l, u, node_of, K, Ar && lr && ur && rows && flags))
        return rc;
    if (pieces == 0) return QPN_OK;
    if (int rc = st.check()) return rc;
    if (!(tol >= 0.0)) return fail_arg(ctx, "qpn_reduced_pieces: bad tolerance");
    if (qpn_reduce_pieces_lds(n, m, p) > 60 * 1024) { ctx->last_error = "qpn_reduced_pieces: too many parameters for one workgroup's LDS"; return QPN_ERR_SIZE; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int N = n + m;
    const size_t rws = 2 * (size_t)N, cols = (size_t)N + p, cap = (size_t)n + 2 * (size_t)m, oc = (size_t)n + p;
    NodeDev d{};
    const int32_t *dno; const uint8_t *dK;
    double *dAp, *dlp, *dup, *dAr, *dlr, *dur; uint8_t *dkeep; int32_t *drows, *dflags;
    st.scratch(dAp, (size_t)pieces * rws * cols * 8); st.scratch(dlp, (size_t)pieces * rws * 8);
    st.scratch(dup, (size_t)pieces * rws * 8); st.scratch(dkeep, (size_t)pieces * rws);
    stage_records(st, d, node_sizes(nodes, n, m, p, 0), Qd, R, qd, Ad, B, l, u);
    st.in(dno, node_of, (size_t)pieces * 4); st.in(dK, K, (size_t)pieces * N);
    st.out(dAr, Ar, (size_t)pieces * oc * cap * 8); st.out(dlr, lr, (size_t)pieces * cap * 8, 8);
    st.out(dur, ur, (size_t)pieces * cap * 8, 8); st.out(drows, rows, (size_t)pieces * 4); st.out(dflags, flags, (size_t)pieces * 4);
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_local_pieces(pieces, nodes, n, m, p, d.Q, d.R, d.q, d.A, d.B, d.l, d.u, dno, dK, dAp, dlp, dup, dkeep, s));
    HIPCHK(ctx, qpn_launch_reduce_pieces(pieces, n, m, p, tol, dAp, dlp, dup, dkeep, dAr, dlr, dur, drows, dflags, s));
    return st.finish();
}

int qpn_project_pieces(qpn_ctx *ctx, int32_t pieces, int32_t nodes, int32_t n, int32_t m, int32_t p, const double *Qd,
                       const double *R, const double *qd, const double *Ad, const double *B, const double *l,
                       const double *u, const int32_t *node_of, const uint8_t *K, double tol, int32_t cap, double *Ar, double *lr,
                       double *ur, int32_t *rows, int32_t *flags, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    Stage st(ctx, mem, "qpn_project_pieces");
    if (int rc = pieces_check(ctx, st.who, st.host, pieces, nodes, n, m, p, Qd, R, qd, Ad, B, l, u, node_of, K, Ar && lr && ur && rows && flags))
        return rc;
    if ((int64_t)cap < (int64_t)n + 2 * (int64_t)m) return fail_arg(ctx, "qpn_project_pieces: cap < n + 2m");
    if (pieces == 0) return QPN_OK;
    if (int rc = st.check()) return rc;
    if (!(tol >= 0.0)) return fail_arg(ctx, "qpn_project_pieces: bad tolerance");
    if (qpn_project_pieces_lds(n, m, p) > (size_t)kProjectLdsMax) { ctx->last_error = "qpn_project_pieces: too many parameters for one workgroup's LDS"; return QPN_ERR_SIZE; }
    const int N = n + m;
    const size_t rws = 2 * (size_t)N, cols = (size_t)N + p, capz = (size_t)cap, oc = (size_t)n + p;
    // one piece's share of the workspace: its local piece and the scratch of the Fourier-Motzkin steps (the first test keeps the
    // products below inside size_t)
    const size_t slack = 16 * 256;                                   // the slots' alignment
    size_t per = 0;
    if (capz <= kProjectWsBytes / (16 * cols)) per = rws * cols * 8 + 2 * rws * 8 + rws + qpn_project_pieces_scratch(n, m, p, cap);
    if (per == 0 || per > kProjectWsBytes - slack) {
        ctx->last_error = "qpn_project_pieces: cap rows of one piece do not fit the workspace";
        return QPN_ERR_SIZE;
    }
    const size_t chunk = std::min((size_t)pieces, (kProjectWsBytes - slack) / per);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    NodeDev d{};
    const int32_t *dno; const uint8_t *dK;
    double *dAp, *dlp, *dup, *dbuf, *dbnd, *dAr, *dlr, *dur; uint8_t *dkeep; int32_t *dlists, *drows, *dflags;
    st.scratch(dAp, chunk * rws * cols * 8); st.scratch(dlp, chunk * rws * 8); st.scratch(dup, chunk * rws * 8); st.scratch(dkeep, chunk * rws);
    st.scratch(dbuf, chunk * 2 * capz * cols * 8); st.scratch(dbnd, chunk * 4 * capz * 8); st.scratch(dlists, chunk * 5 * capz * 4);
    stage_records(st, d, node_sizes(nodes, n, m, p, 0), Qd, R, qd, Ad, B, l, u);
    st.in(dno, node_of, (size_t)pieces * 4); st.in(dK, K, (size_t)pieces * N);
    st.out(dAr, Ar, (size_t)pieces * oc * capz * 8); st.out(dlr, lr, (size_t)pieces * capz * 8); st.out(dur, ur, (size_t)pieces * capz * 8);
    st.out(drows, rows, (size_t)pieces * 4); st.out(dflags, flags, (size_t)pieces * 4);
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    for (size_t t0 = 0; t0 < (size_t)pieces; t0 += chunk) {
        const int32_t cnt = (int32_t)std::min(chunk, (size_t)pieces - t0);
        // without node_of piece t reads record t: a chunk's records start at its first piece
        const size_t b0 = dno ? 0 : t0;
        HIPCHK(ctx, qpn_launch_local_pieces(cnt, nodes - (int32_t)b0, n, m, p, d.Q + b0 * n * n, d.R + b0 * n * p, d.q + b0 * n, d.A + b0 * m * n,
                                            d.B + b0 * m * p, d.l + b0 * m, d.u + b0 * m, dno ? dno + t0 : nullptr, dK + t0 * N, dAp, dlp, dup,
                                            dkeep, s));
        HIPCHK(ctx, qpn_launch_project_pieces(cnt, n, m, p, tol, cap, dAp, dlp, dup, dkeep, dbuf, dbnd, dlists, dAr + t0 * oc * capz,
                                              dlr + t0 * capz, dur + t0 * capz, drows + t0, dflags + t0, s));
    }
    return st.finish();
}

int qpn_recipes_batch_range(qpn_ctx *ctx, int32_t nodes, int32_t N, const uint8_t *masks, const int64_t *first, const int64_t *offsets,
                            uint8_t *K, int32_t *node_of, int mem)
{
    return recipes_batch_any(ctx, first ? "qpn_recipes_batch_range" : "qpn_recipes_batch", nodes, N, masks, first, offsets, K, node_of, mem);
}

int qpn_finish_pieces(qpn_ctx *ctx, int32_t pieces, int32_t records, int32_t n, int32_t m, int32_t p, const double *Ar, const double *lr,
                      const double *ur, const int32_t *rows, const int32_t *flags, const int32_t *rec_of, const int32_t *ncols,
                      const int32_t *take, const double *xk, const double *probe, double member_tol, int32_t *status, double *worst,
                      uint64_t *hash, int32_t *dup_of, int32_t *store_of, int32_t store_cap, double *As, double *ls, double *us,
                      int32_t *rows_s, int32_t *stored, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (pieces < 0 || records <= 0 || n <= 0 || m < 0 || p < 0 || store_cap < 0) return fail_arg(ctx, "qpn_finish_pieces: bad sizes");
    if (!stored) return fail_arg(ctx, "qpn_finish_pieces: null pointer");
    *stored = 0;
    if (pieces == 0) return QPN_OK;
    if (n + m > 512) { ctx->last_error = "qpn_finish_pieces: n + m <= 512 in ABI v1"; return QPN_ERR_SIZE; }
    if (!Ar || !lr || !ur || !rows || !flags || !rec_of || !ncols || !take || !xk || !probe || !status || !worst || !hash || !dup_of ||
        !store_of || (store_cap > 0 && (!As || !ls || !us || !rows_s)))
        return fail_arg(ctx, "qpn_finish_pieces: null pointer");
    if (!(member_tol >= 0.0)) return fail_arg(ctx, "qpn_finish_pieces: bad tolerance");
    Stage st(ctx, mem, "qpn_finish_pieces");
    if (int rc = st.check()) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int oc = n + p, cap = n + 2 * m;
    // the index arrays are checked on the host in both modes (device ones are read back: they are small)
    std::vector<int32_t> h_rows, h_rec, h_nc, h_take;
    const int32_t *cr = rows, *crec = rec_of, *cnc = ncols, *ctk = take;
    if (!st.host) {
        h_rows.resize(pieces); h_rec.resize(pieces); h_nc.resize(records); h_take.resize((size_t)records * oc);
        HIPCHK(ctx, hipMemcpyAsync(h_rows.data(), rows, (size_t)pieces * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(h_rec.data(), rec_of, (size_t)pieces * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(h_nc.data(), ncols, (size_t)records * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(h_take.data(), take, (size_t)records * oc * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        cr = h_rows.data(); crec = h_rec.data(); cnc = h_nc.data(); ctk = h_take.data();
    }
    for (int k = 0; k < records; ++k) {
        if (cnc[k] < 0 || cnc[k] > oc) return fail_arg(ctx, "qpn_finish_pieces: ncols outside 0..n+p");
        for (int c = 0; c < cnc[k]; ++c)
            if (ctk[(size_t)k * oc + c] < 0 || ctk[(size_t)k * oc + c] >= oc) return fail_arg(ctx, "qpn_finish_pieces: take outside 0..n+p-1");
    }
    for (int t = 0; t < pieces; ++t) {
        if (crec[t] < 0 || crec[t] >= records) return fail_arg(ctx, "qpn_finish_pieces: rec_of outside 0..records-1");
        if (cr[t] < 0 || cr[t] > cap) return fail_arg(ctx, "qpn_finish_pieces: rows outside 0..n+2m");
    }
    const size_t P = (size_t)pieces;
    const double *dAr, *dlr, *dur, *dxk, *dpr; const int32_t *drows, *dflags, *drec, *dnc, *dtk;
    double *drsc, *drdiv, *dLn, *dUn, *dworst, *dAs, *dls, *dus;
    int32_t *dstatus, *ddup, *dstore, *drows_s, *dord, *drun0, *dsrc; unsigned long long *dhash;
    st.in(dAr, Ar, P * oc * cap * 8); st.in(dlr, lr, P * cap * 8); st.in(dur, ur, P * cap * 8);
    st.in(drows, rows, P * 4); st.in(dflags, flags, P * 4); st.in(drec, rec_of, P * 4);
    st.in(dnc, ncols, (size_t)records * 4); st.in(dtk, take, (size_t)records * oc * 4);
    st.in(dxk, xk, (size_t)records * oc * 8); st.in(dpr, probe, (size_t)records * oc * 8);
    st.scratch(drsc, P * cap * 8); st.scratch(drdiv, P * cap * 8); st.scratch(dLn, P * cap * 8); st.scratch(dUn, P * cap * 8);
    st.scratch(dord, P * 4); st.scratch(drun0, P * 4); st.scratch(dsrc, P * 4);
    st.out(dstatus, status, P * 4); st.out(dworst, worst, P * 8); st.out(dhash, hash, P * 8); st.out(ddup, dup_of, P * 4);
    st.out(dstore, store_of, P * 4);
    // the store: host mode copies back only the slots that are filled (below), not the whole capacity
    const size_t scap = (size_t)store_cap;
    if (st.host) { st.scratch(dAs, scap * oc * cap * 8); st.scratch(dls, scap * cap * 8); st.scratch(dus, scap * cap * 8); st.scratch(drows_s, scap * 4); }
    else { dAs = As; dls = ls; dus = us; drows_s = rows_s; }
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_finish_norm(pieces, oc, cap, dAr, dlr, dur, drows, dflags, drec, dnc, dtk, dxk, dpr, member_tol, drsc, drdiv, dLn,
                                       dUn, dstatus, dworst, dhash, ddup, s));
    // the duplicate candidates (members, neither merge candidates nor flagged) sorted by (item, hash, piece): equal keys are neighbours
    std::vector<int32_t> h_st(P);
    std::vector<unsigned long long> h_hash(P);
    HIPCHK(ctx, hipMemcpyAsync(h_st.data(), dstatus, P * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(h_hash.data(), dhash, P * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    std::vector<int32_t> ord, run0;
    ord.reserve(P);
    for (int t = 0; t < pieces; ++t)
        if (h_st[t] == QPN_FIN_MEMBER) ord.push_back(t);
    std::sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) {
        if (crec[a] != crec[b]) return crec[a] < crec[b];
        if (h_hash[a] != h_hash[b]) return h_hash[a] < h_hash[b];
        return a < b;
    });
    run0.resize(ord.size());
    bool any_run = false;
    for (size_t q = 0; q < ord.size(); ++q) {
        const bool same = q > 0 && crec[ord[q]] == crec[ord[q - 1]] && h_hash[ord[q]] == h_hash[ord[q - 1]];
        run0[q] = same ? run0[q - 1] : (int32_t)q;
        any_run |= same;
    }
    if (any_run) {
        // (only the pieces that have an earlier one of the same hash need a comparison)
        std::vector<int32_t> ord2, run2;
        for (size_t q = 0; q < ord.size(); ++q)
            if (run0[q] < (int32_t)q) { ord2.push_back((int32_t)q); }
        // positions refer to the full sorted list: upload it, and the positions to check with their run starts
        std::vector<int32_t> pos(ord2.size()), r0(ord2.size());
        for (size_t i = 0; i < ord2.size(); ++i) { pos[i] = ord2[i]; r0[i] = run0[ord2[i]]; }
        HIPCHK(ctx, hipMemcpyAsync(dord, ord.data(), ord.size() * 4, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemcpyAsync(drun0, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemcpyAsync(dsrc, r0.data(), r0.size() * 4, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, qpn_launch_finish_dup((int32_t)pos.size(), dord, drun0, dsrc, oc, cap, dAr, drows, drec, dnc, dtk, drsc, drdiv, dLn, dUn,
                                          dstatus, ddup, s));
        HIPCHK(ctx, hipMemcpyAsync(h_st.data(), dstatus, P * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    // the store: members that are neither duplicates nor flagged, in piece order
    std::vector<int32_t> h_store(P, -1), src;
    for (int t = 0; t < pieces; ++t)
        if ((h_st[t] & QPN_FIN_MEMBER) && !(h_st[t] & (QPN_FIN_DUP | QPN_FIN_FLAGGED))) { h_store[t] = (int32_t)src.size(); src.push_back(t); }
    if (src.size() > scap) { ctx->last_error = "qpn_finish_pieces: more pieces to store than store_cap"; return QPN_ERR_SIZE; }
    *stored = (int32_t)src.size();
    HIPCHK(ctx, hipMemcpyAsync(dstore, h_store.data(), P * 4, hipMemcpyHostToDevice, s));
    if (!src.empty()) {
        HIPCHK(ctx, hipMemcpyAsync(dsrc, src.data(), src.size() * 4, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, qpn_launch_finish_store((int32_t)src.size(), dsrc, oc, cap, dAr, drows, drec, dnc, dtk, drsc, drdiv, dLn, dUn, dAs, dls, dus,
                                            drows_s, s));
    }
    if (st.host && !src.empty()) {
        const size_t S = src.size();
        HIPCHK(ctx, hipMemcpyAsync(As, dAs, S * oc * cap * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(ls, dls, S * cap * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(us, dus, S * cap * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(rows_s, drows_s, S * 4, hipMemcpyDeviceToHost, s));
    }
    rc = st.finish();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));                            // (the host vectors above are read by the copies)
    return QPN_OK;
}

int qpn_local_pieces(qpn_ctx *ctx, int32_t pieces, int32_t nodes, int32_t n, int32_t m, int32_t p, const double *Qd,
                     const double *R, const double *qd, const double *Ad, const double *B, const double *l,
                     const double *u, const int32_t *node_of, const uint8_t *K, double *Ap, double *lp, double *up,
                     uint8_t *keep, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    Stage st(ctx, mem, "qpn_local_pieces");
    if (int rc = pieces_check(ctx, st.who, st.host, pieces, nodes, n, m, p, Qd, R, qd, Ad, B, l, u, node_of, K, Ap && lp && up && keep))
        return rc;
    if (pieces == 0) return QPN_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int N = n + m;
    const size_t rows = 2 * (size_t)N, cols = (size_t)N + p;
    NodeDev d{};
    const int32_t *dno; const uint8_t *dK;
    double *dAp, *dlp, *dup; uint8_t *dkeep;
    stage_records(st, d, node_sizes(nodes, n, m, p, 0), Qd, R, qd, Ad, B, l, u);
    st.in(dno, node_of, (size_t)pieces * 4); st.in(dK, K, (size_t)pieces * N);
    st.out(dAp, Ap, (size_t)pieces * rows * cols * 8); st.out(dlp, lp, (size_t)pieces * rows * 8);
    st.out(dup, up, (size_t)pieces * rows * 8); st.out(dkeep, keep, (size_t)pieces * rows);
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_local_pieces(pieces, nodes, n, m, p, d.Q, d.R, d.q, d.A, d.B, d.l, d.u, dno, dK, dAp, dlp, dup, dkeep,
                                        ctx->stream));
    return st.finish();
}

// ---- (A6) pool assembly -------------------------------------------------------------------------------------
int qpn_pool_size(const qpn_pool_shape *sh, int form, int32_t *N)
{
    if (!sh || !N || sh->players <= 0 || sh->nd <= 0 || sh->p < 0 || !sh->n_i || !sh->m_i) return QPN_ERR_ARG;
    if (form != QPN_POOL_REDUCED && form != QPN_POOL_REFERENCE) return QPN_ERR_ARG;
    int64_t sn = 0, sm = 0;
    for (int i = 0; i < sh->players; ++i) {
        if (sh->n_i[i] <= 0 || sh->m_i[i] < 0) return QPN_ERR_ARG;
        sn += sh->n_i[i]; sm += sh->m_i[i];
    }
    const int64_t n = form == QPN_POOL_REFERENCE ? sh->nd + sn + 2 * sm : sh->nd + sm;
    if (n > 1 << 20) return QPN_ERR_SIZE;
    *N = (int32_t)n;
    return QPN_OK;
}

int qpn_assemble_pools(qpn_ctx *ctx, const qpn_pool_shape *sh, int form, int32_t batch, const double *Qd,
                       int64_t stride_Qd, const double *Qp, int64_t stride_Qp, const double *qd, int64_t stride_qd,
                       const double *Ad, int64_t stride_Ad, const double *Bp, int64_t stride_Bp, const double *l,
                       const double *u, int64_t stride_lu, const double *w, int64_t stride_w, double *Mout,
                       int64_t strideM, double *qout, double *lout, double *uout, uint8_t *kind_out, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    int32_t N = 0;
    int rc = qpn_pool_size(sh, form, &N);
    if (rc != QPN_OK) return rc == QPN_ERR_ARG ? fail_arg(ctx, "qpn_assemble_pools: bad pool shape or form") : rc;
    if (batch < 0) return fail_arg(ctx, "qpn_assemble_pools: batch < 0");
    if (batch == 0) return QPN_OK;
    if (!sh->dpos) return fail_arg(ctx, "qpn_assemble_pools: null dpos");
    const int nd = sh->nd, p = sh->p;
    int sn = 0, sm = 0;
    for (int i = 0; i < sh->players; ++i) { sn += sh->n_i[i]; sm += sh->m_i[i]; }
    if (!Qd || !qd || (sm > 0 && (!Ad || !l || !u)) || (p > 0 && (!Qp || !w || (sm > 0 && !Bp))) || !Mout || !qout || !lout ||
        !uout || !kind_out)
        return fail_arg(ctx, "qpn_assemble_pools: null pointer");
    // the index maps of the shape
    std::vector<int32_t> maps((size_t)2 * sn + sm + nd, -1);
    int32_t *xi_owner = maps.data(), *xi_dpos = xi_owner + sn, *con_owner = xi_dpos + sn, *dec_src = con_owner + sm;
    {
        int t = 0, k = 0;
        for (int i = 0; i < sh->players; ++i) {
            for (int e = 0; e < sh->n_i[i]; ++e, ++t) {
                const int d = sh->dpos[t];
                if (d < 0 || d >= nd) return fail_arg(ctx, "qpn_assemble_pools: dpos outside 0..nd-1");
                xi_owner[t] = i; xi_dpos[t] = d;
                if (form == QPN_POOL_REDUCED) {
                    if (dec_src[d] >= 0) return fail_arg(ctx, "qpn_assemble_pools: reduced form needs disjoint decision sets");
                    dec_src[d] = t;
                }
            }
            for (int r = 0; r < sh->m_i[i]; ++r, ++k) con_owner[k] = i;
        }
        if (form == QPN_POOL_REDUCED)
            for (int d = 0; d < nd; ++d)
                if (dec_src[d] < 0) return fail_arg(ctx, "qpn_assemble_pools: a decision position belongs to no player");
    }
    const size_t szQd = (size_t)sn * nd, szQp = (size_t)sn * p, szAd = (size_t)sm * nd, szBp = (size_t)sm * p;
    auto bad_stride = [&](int64_t st, size_t need) { return st != 0 && (st < 0 || (size_t)st < need); };
    if (bad_stride(stride_Qd, szQd) || bad_stride(stride_Qp, szQp) || bad_stride(stride_qd, (size_t)sn) || bad_stride(stride_Ad, szAd) ||
        bad_stride(stride_Bp, szBp) || bad_stride(stride_lu, (size_t)sm) || bad_stride(stride_w, (size_t)p) ||
        bad_stride(strideM, (size_t)N * N))
        return fail_arg(ctx, "qpn_assemble_pools: item stride smaller than the item");
    if (strideM == 0 && batch > 1 && (stride_Qd != 0 || stride_Ad != 0))
        return fail_arg(ctx, "qpn_assemble_pools: a shared M needs shared Qd and Ad");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    auto span = [&](int64_t st, size_t item) { return (st ? (size_t)(batch - 1) * (size_t)st + item : item) * 8; };
    const size_t bQd = span(stride_Qd, szQd), bQp = span(stride_Qp, szQp), bqd = span(stride_qd, sn), bAd = span(stride_Ad, szAd),
                 bBp = span(stride_Bp, szBp), blu = span(stride_lu, sm), bw = span(stride_w, p);
    const size_t bM = span(strideM, (size_t)N * N), bN = (size_t)batch * N;
    QpnPoolLaunch L{};
    L.batch = batch; L.form = form; L.nd = nd; L.sn = sn; L.sm = sm; L.p = p;
    L.s_Qd = stride_Qd; L.s_Qp = stride_Qp; L.s_qd = stride_qd; L.s_Ad = stride_Ad; L.s_Bp = stride_Bp; L.s_lu = stride_lu;
    L.s_w = stride_w; L.s_M = strideM;
    const int32_t *dmaps;
    Stage st(ctx, mem, "qpn_assemble_pools");
    st.lib_in(dmaps, maps.data(), maps.size() * 4);
    // (an empty item uploads nothing, whatever its stride)
    st.in(L.Qd, Qd, bQd, 8); st.in(L.Qp, Qp, szQp ? bQp : 0, 8); st.in(L.qd, qd, bqd, 8); st.in(L.Ad, Ad, szAd ? bAd : 0, 8);
    st.in(L.Bp, Bp, szBp ? bBp : 0, 8); st.in(L.l, l, sm ? blu : 0, 8); st.in(L.u, u, sm ? blu : 0, 8); st.in(L.w, w, p ? bw : 0, 8);
    st.out(L.M, Mout, bM); st.out(L.q, qout, bN * 8); st.out(L.lo, lout, bN * 8); st.out(L.hi, uout, bN * 8); st.out(L.kind, kind_out, bN);
    rc = st.begin();
    if (rc != QPN_OK) return rc;
    L.xi_owner = dmaps; L.xi_dpos = dmaps + sn; L.con_owner = dmaps + 2 * sn; L.dec_src = dmaps + 2 * sn + sm;
    HIPCHK(ctx, qpn_launch_assemble_pools(L, s));
    if ((rc = st.finish()) != QPN_OK) return rc;
    // (device mode: the maps were copied from a host vector that dies with this call: the copy must have left it)
    if (!st.host) HIPCHK(ctx, hipStreamSynchronize(s));
    return QPN_OK;
}

// ---- multi-GPU: shared iterate buffers and their replicas ------------------------------------------------
static_assert(sizeof(hipIpcMemHandle_t) == QPN_IPC_HANDLE_BYTES, "IPC handle size");

int qpn_shared_alloc(qpn_ctx *ctx, size_t bytes, int flags, void **dev_ptr, uint8_t *handle)
{
    if (!ctx) return QPN_ERR_ARG;
    if (!dev_ptr || !handle || bytes == 0) return fail_arg(ctx, "qpn_shared_alloc: null pointer or zero size");
    if (flags & ~QPN_SHARED_FINE_GRAINED) return fail_arg(ctx, "qpn_shared_alloc: unknown flag");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    void *p = nullptr;
    if (flags & QPN_SHARED_FINE_GRAINED) HIPCHK(ctx, hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained));
    else HIPCHK(ctx, hipMalloc(&p, bytes));
    hipIpcMemHandle_t h;
    hipError_t e = hipIpcGetMemHandle(&h, p);
    if (e != hipSuccess) { (void)hipFree(p); return fail_hip(ctx, e, "hipIpcGetMemHandle"); }
    e = hipMemsetAsync(p, 0, bytes, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { (void)hipFree(p); return fail_hip(ctx, e, "qpn_shared_alloc: clear"); }
    memcpy(handle, &h, sizeof h);
    *dev_ptr = p;
    return QPN_OK;
}

int qpn_shared_open(qpn_ctx *ctx, const uint8_t *handle, void **dev_ptr)
{
    if (!ctx) return QPN_ERR_ARG;
    if (!dev_ptr || !handle) return fail_arg(ctx, "qpn_shared_open: null pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipIpcMemHandle_t h;
    memcpy(&h, handle, sizeof h);
    void *p = nullptr;
    HIPCHK(ctx, hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
    *dev_ptr = p;
    return QPN_OK;
}

int qpn_shared_close(qpn_ctx *ctx, void *dev_ptr)
{
    if (!ctx) return QPN_ERR_ARG;
    if (!dev_ptr) return QPN_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < ctx->mirror_count; ++k)
        if ((void *)ctx->mirror_peer[k] == dev_ptr) { ctx->mirror_count = 0; break; }   // never leave a dangling replica
    HIPCHK(ctx, hipIpcCloseMemHandle(dev_ptr));
    return QPN_OK;
}

int qpn_shared_free(qpn_ctx *ctx, void *dev_ptr)
{
    if (!ctx) return QPN_ERR_ARG;
    if (!dev_ptr) return QPN_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if ((const void *)ctx->mirror_own == dev_ptr) { ctx->mirror_count = 0; ctx->mirror_own = nullptr; ctx->mirror_bytes = 0; }
    HIPCHK(ctx, hipFree(dev_ptr));
    return QPN_OK;
}

int qpn_set_primal_mirrors(qpn_ctx *ctx, const double *own, size_t bytes, int32_t count, double *const *peers)
{
    if (!ctx) return QPN_ERR_ARG;
    if (count < 0 || count > QPN_MAX_MIRRORS) return fail_arg(ctx, "qpn_set_primal_mirrors: count outside 0..QPN_MAX_MIRRORS");
    if (count > 0 && (!own || !peers || bytes == 0)) return fail_arg(ctx, "qpn_set_primal_mirrors: null pointer");
    for (int k = 0; k < count; ++k)
        if (!peers[k] || peers[k] == own) return fail_arg(ctx, "qpn_set_primal_mirrors: null or self peer");
    ctx->mirror_count = 0;
    ctx->mirror_own = count ? own : nullptr;
    ctx->mirror_bytes = count ? bytes : 0;
    for (int k = 0; k < count; ++k) ctx->mirror_peer[k] = peers[k];
    ctx->mirror_count = count;
    return QPN_OK;
}

static_assert(QPN_SWEEP_BOX_BYTES == 2 * QPN_MAX_RANKS * 32, "mailbox = 2 parities x QPN_MAX_RANKS slots of 32 B");

int qpn_sweep_status(qpn_ctx *ctx, const int32_t *status, const double *resid, int32_t count, double *out,
                     int32_t rank, int32_t world, void *const *boxes, uint64_t epoch, int32_t timeout_ms)
{
    if (!ctx) return QPN_ERR_ARG;
    if (!status || !out || count < 0) return fail_arg(ctx, "qpn_sweep_status: bad arguments");
    if (world > QPN_MAX_RANKS) return fail_arg(ctx, "qpn_sweep_status: world > QPN_MAX_MIRRORS + 1");
    SweepBoxes bx{};
    if (world > 1) {
        if (rank < 0 || rank >= world || !boxes || epoch == 0 || timeout_ms <= 0)
            return fail_arg(ctx, "qpn_sweep_status: bad rank / boxes / epoch / timeout");
        for (int r = 0; r < world; ++r) {
            if (!boxes[r]) return fail_arg(ctx, "qpn_sweep_status: null mailbox");
            bx.box[r] = boxes[r];
        }
    } else { world = 1; rank = 0; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, qpn_launch_sweep_status(status, resid, count, out, rank, world, bx, epoch,
                                        (unsigned long long)timeout_ms * 100000ull, ctx->stream));   // 100 MHz wall clock
    return QPN_OK;
}

int qpn_convexity_nodes(qpn_ctx *ctx, int32_t batch, int32_t n, int32_t m, const double *Qd, const double *Ad,
                        const uint8_t *eq, double tol, int32_t *convex, double *min_eig, int32_t *null_dim, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (batch < 0 || n <= 0 || m < 0) return fail_arg(ctx, "qpn_convexity_nodes: bad sizes");
    if (n > QPN_CONVEXITY_MAX_N || m > QPN_CONVEXITY_MAX_M) {
        ctx->last_error = "qpn_convexity_nodes: n <= 256, m <= 1024 in ABI v1";
        return QPN_ERR_SIZE;
    }
    if (!Qd || (m > 0 && (!Ad || !eq)) || !convex || !min_eig || !null_dim) return fail_arg(ctx, "qpn_convexity_nodes: null pointer");
    Stage st(ctx, mem, "qpn_convexity_nodes");
    if (int rc = st.check()) return rc;
    if (batch == 0) return QPN_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const double *dQ, *dA; const uint8_t *de; int32_t *dcvx, *dnull; double *dmin; void *gws;
    st.in(dQ, Qd, (size_t)batch * n * n * 8); st.in(dA, Ad, (size_t)batch * m * n * 8); st.in(de, eq, (size_t)batch * m);
    st.out(dcvx, convex, (size_t)batch * 4); st.out(dmin, min_eig, (size_t)batch * 8); st.out(dnull, null_dim, (size_t)batch * 4);
    st.scratch(gws, qpn_convexity_workspace_bytes(batch, n, m));
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_convexity(batch, n, m, dQ, dA, de, tol, dcvx, dmin, dnull, gws, ctx->stream));
    return st.finish();
}

int qpn_multiplier_vertices(qpn_ctx *ctx, int32_t batch, int32_t n, int32_t m, const double *Ad, const double *g, const uint8_t *cls,
                            const double *lam0, int32_t V, int32_t max_bases, double tol, double feas, double *verts, int32_t *count,
                            int32_t *status, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (batch < 0 || n <= 0 || m <= 0 || V <= 0 || max_bases <= 0) return fail_arg(ctx, "qpn_multiplier_vertices: bad sizes");
    if (n > qpn_verify_max_dim() || m > qpn_verify_max_dim()) {
        ctx->last_error = "qpn_multiplier_vertices: n, m <= 512 in ABI v1";
        return QPN_ERR_SIZE;
    }
    if (!Ad || !g || !cls || !lam0 || !verts || !count || !status) return fail_arg(ctx, "qpn_multiplier_vertices: null pointer");
    Stage st(ctx, mem, "qpn_multiplier_vertices");
    if (int rc = st.check()) return rc;
    if (batch == 0) return QPN_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const double *dA, *dg, *dl; const uint8_t *dc; double *dv; int32_t *dcnt, *dst; void *ws;
    st.in(dA, Ad, (size_t)batch * n * m * 8); st.in(dg, g, (size_t)batch * n * 8); st.in(dc, cls, (size_t)batch * m);
    st.in(dl, lam0, (size_t)batch * m * 8);
    st.out(dv, verts, (size_t)batch * V * m * 8); st.out(dcnt, count, (size_t)batch * 4); st.out(dst, status, (size_t)batch * 4);
    st.scratch(ws, qpn_multiplier_vertices_workspace_bytes(batch, n, m, max_bases));
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, hipMemsetAsync(dv, 0, (size_t)batch * V * m * 8, ctx->stream));
    HIPCHK(ctx, qpn_launch_multiplier_vertices(batch, n, m, dA, dg, dc, dl, V, max_bases, tol, feas, dv, dcnt, dst, ws, ctx->stream));
    return st.finish();
}

int qpn_recipe_filter(qpn_ctx *ctx, int32_t pieces, int32_t rows, int32_t N, const uint8_t *masks, const uint8_t *K,
                      const int32_t *vrow_of, const int32_t *first_of, uint8_t *keep, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (pieces < 0 || rows < 0 || N <= 0) return fail_arg(ctx, "qpn_recipe_filter: bad sizes");
    if (pieces > 0 && (!masks || !K || !vrow_of || !first_of || !keep || rows == 0)) return fail_arg(ctx, "qpn_recipe_filter: null pointer");
    Stage st(ctx, mem, "qpn_recipe_filter");
    if (int rc = st.check()) return rc;
    if (pieces == 0) return QPN_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint8_t *dm, *dK; const int32_t *dvr, *dfo; uint8_t *dk;
    st.in(dm, masks, (size_t)rows * N); st.in(dK, K, (size_t)pieces * N); st.in(dvr, vrow_of, (size_t)pieces * 4);
    st.in(dfo, first_of, (size_t)rows * 4); st.out(dk, keep, (size_t)pieces);
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_recipe_filter(pieces, N, dm, dK, dvr, dfo, rows, dk, ctx->stream));
    return st.finish();
}

} // extern "C"

namespace {

// the record shape of a batch of interior-member queries (polyhedra.interior_member_records)
struct MemberShape { int32_t nf, mp; };

// what qpn_assemble_interior_nodes and qpn_interior_members ask of the arguments they share; *sh: the record shape
int members_check(qpn_ctx *ctx, const char *who, int32_t batch, int32_t r, int32_t d, const double *A, const double *l, const double *u,
                  int32_t ne, int32_t nlo, int32_t nhi, bool outputs, MemberShape *sh)
{
    if (batch < 0 || r <= 0 || d <= 0 || ne < 0 || nlo < 0 || nhi < 0) return fail_arg(ctx, who, "bad sizes");
    const int64_t nf = (int64_t)d + 1 + ne, mi = (int64_t)nlo + nhi, mp = mi <= 16 ? 16 : (mi + 15) / 16 * 16;
    if (nf + mp > qpn_avi_max_n() || r > QPN_MEMBERS_MAX_ROWS) {
        ctx->last_error = std::string(who) + ": d + 1 + ne + mp <= 1024 and r <= 4096 in ABI v1";
        return QPN_ERR_SIZE;
    }
    if (batch > 0 && (!A || !l || !u || !outputs)) return fail_arg(ctx, who, "null pointer");
    sh->nf = (int32_t)nf; sh->mp = (int32_t)mp;
    return QPN_OK;
}

} // namespace

extern "C" {

// ---- interior members of polyhedra: records made on the device (qpn_members.hip) ------------------------------------------
int qpn_assemble_interior_nodes(qpn_ctx *ctx, int32_t batch, int32_t r, int32_t d, const double *A, const double *l, const double *u,
                                double delta, int32_t ne, int32_t nlo, int32_t nhi, double *Qd, double *qd, double *Ad, double *lo,
                                double *uo, uint8_t *flag, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    MemberShape sh;
    Stage st(ctx, mem, "qpn_assemble_interior_nodes");
    if (int rc = members_check(ctx, st.who, batch, r, d, A, l, u, ne, nlo, nhi, Qd && qd && Ad && lo && uo && flag, &sh)) return rc;
    if (int rc = st.check()) return rc;
    if (batch == 0) return QPN_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t B = (size_t)batch, nf = sh.nf, mp = sh.mp;
    const double *dA, *dl, *du; double *dQ, *dq, *dAd, *dlo, *duo; uint8_t *dflag;
    st.in(dA, A, B * r * d * 8); st.in(dl, l, B * r * 8); st.in(du, u, B * r * 8);
    st.out(dQ, Qd, B * nf * nf * 8); st.out(dq, qd, B * nf * 8); st.out(dAd, Ad, B * nf * mp * 8);
    st.out(dlo, lo, B * mp * 8); st.out(duo, uo, B * mp * 8); st.out(dflag, flag, B);
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_interior_records(batch, r, d, dA, dl, du, delta, ne, nlo, nhi, dQ, dq, dAd, dlo, duo, dflag, ctx->stream));
    return st.finish();
}

int qpn_interior_members(qpn_ctx *ctx, int32_t batch, int32_t r, int32_t d, const double *A, const double *l, const double *u,
                         double delta, int32_t ne, int32_t nlo, int32_t nhi, double *x_out, uint8_t *ok, int32_t *status, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    MemberShape sh;
    Stage st(ctx, mem, "qpn_interior_members");
    if (int rc = members_check(ctx, st.who, batch, r, d, A, l, u, ne, nlo, nhi, x_out && ok && status, &sh)) return rc;
    if (int rc = st.check()) return rc;
    if (batch == 0) return QPN_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // the solve of qpn_solve_nodes over these records with p = 1, R = 0, B = 0, w = 0, default options and a cold start
    const int32_t n = sh.nf, m = sh.mp, N = n + m;
    qpn_avi_opts o;
    qpn_avi_default_opts(&o);
    o.flags |= QPN_AVI_FLAG_COLD_START;
    const NodeRoute route = node_route(ctx, n, m, o);
    const size_t B = (size_t)batch, bN = B * N;
    NodeWs ws{};
    st.scratch(ws.M, bN * N * 8); st.scratch(ws.q, bN * 8); st.scratch(ws.l, bN * 8); st.scratch(ws.u, bN * 8); st.scratch(ws.kind, bN);
    if (N > 64) st.scratch(ws.big, qpn_avi_big_workspace_bytes(batch, N));
    const double *dA, *dl, *du;
    st.in(dA, A, B * r * d * 8); st.in(dl, l, B * r * 8); st.in(du, u, B * r * 8);
    double *rQ, *rq, *rA, *rl, *ru, *zeros, *dx; uint8_t *dflag, *dok;
    st.scratch(rQ, B * n * n * 8); st.scratch(rq, B * n * 8); st.scratch(rA, B * n * m * 8); st.scratch(rl, B * m * 8);
    st.scratch(ru, B * m * 8);
    const size_t nz = B * n + B * m + 1;                       // R [batch][n][1], B [batch][m][1], w [1]
    st.scratch(zeros, nz * 8); st.scratch(dflag, B);
    NodeDev nd{};
    st.scratch(nd.z, bN * 8); st.out(nd.st, status, B * 4); st.scratch(nd.res, B * 8); st.scratch(nd.pv, B * 4); st.scratch(nd.act, bN);
    st.out(dx, x_out, B * d * 8); st.out(dok, ok, B);
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, hipMemsetAsync(zeros, 0, nz * 8, s));
    HIPCHK(ctx, qpn_launch_interior_records(batch, r, d, dA, dl, du, delta, ne, nlo, nhi, rQ, rq, rA, rl, ru, dflag, s));
    nd.Q = rQ; nd.R = zeros; nd.q = rq; nd.A = rA; nd.B = zeros + B * n; nd.l = rl; nd.u = ru; nd.w = zeros + B * n + B * m;
    if ((rc = solve_nodes_launch(ctx, nullptr, batch, n, m, 1, nd, 0, o, nullptr, 0, ws, route)) != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_members_extract(batch, d, N, nd.z, nd.st, dflag, dx, dok, s));
    return st.finish();
}

int qpn_members_outside(qpn_ctx *ctx, int32_t pairs, int32_t d, int32_t rj, const double *Aj, const double *lj, const double *uj,
                        int32_t Bj, const double *X, int32_t Bi, const int32_t *pi, const int32_t *pj, double t, uint8_t *out, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (pairs < 0 || d <= 0 || rj <= 0 || Bj < 0 || Bi < 0) return fail_arg(ctx, "qpn_members_outside: bad sizes");
    Stage st(ctx, mem, "qpn_members_outside");
    if (int rc = st.check()) return rc;
    if (pairs == 0) return QPN_OK;
    if (!Aj || !lj || !uj || !X || !pi || !pj || !out || Bj == 0 || Bi == 0) return fail_arg(ctx, "qpn_members_outside: null pointer");
    // host index arrays are checked here; device ones by the kernel (such a pair answers 1: not settled)
    for (int q = 0; st.host && q < pairs; ++q)
        if (pi[q] < 0 || pi[q] >= Bi || pj[q] < 0 || pj[q] >= Bj) return fail_arg(ctx, "qpn_members_outside: pair index out of range");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const double *dA, *dl, *du, *dX; const int32_t *dpi, *dpj; uint8_t *dout;
    st.in(dA, Aj, (size_t)Bj * d * rj * 8); st.in(dl, lj, (size_t)Bj * rj * 8); st.in(du, uj, (size_t)Bj * rj * 8);
    st.in(dX, X, (size_t)Bi * d * 8); st.in(dpi, pi, (size_t)pairs * 4); st.in(dpj, pj, (size_t)pairs * 4);
    st.out(dout, out, (size_t)pairs);
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_members_outside(pairs, d, rj, dA, dl, du, Bj, dX, Bi, dpi, dpj, t, dout, ctx->stream));
    return st.finish();
}

int qpn_members_outside_lists(qpn_ctx *ctx, int32_t d, int32_t rj, const double *Aj, const double *lj, const double *uj, int32_t Bj,
                              const double *X, const uint8_t *ok, int32_t Bi, int32_t lists, const int32_t *list_ptr,
                              const int32_t *list_mem, const int32_t *list_of, const int32_t *self_pos, const int64_t *word_ptr,
                              double t, uint32_t *bits, int32_t *undecided, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    Stage st(ctx, mem, "qpn_members_outside_lists");
    if (Bj < 0 || Bi < 0 || lists < 0) return fail_arg(ctx, st.who, "bad sizes");
    if (d < 1 || rj < 1 || rj > QPN_MEMBERS_MAX_ROWS || (int64_t)Bi * d >= ((int64_t)1 << 31)) {
        ctx->last_error = std::string(st.who) + ": 1 <= d, 1 <= rj <= 4096 and Bi * d < 2^31 in ABI v1";
        return QPN_ERR_SIZE;
    }
    if (int rc = st.check()) return rc;
    if (Bj == 0) return QPN_OK;
    if (!Aj || !lj || !uj || !list_ptr || !list_of || !self_pos || !word_ptr || !undecided || (Bi > 0 && (!X || !ok)))
        return fail_arg(ctx, st.who, "null pointer");
    // host index arrays are checked here, all of them; device ones by the kernel, item by item
    int64_t M = 0, Wn = 0;
    if (st.host) {
        if (list_ptr[0] != 0 || word_ptr[0] != 0) return fail_arg(ctx, st.who, "list_ptr and word_ptr start at 0");
        for (int32_t a = 0; a < lists; ++a)
            if (list_ptr[a + 1] < list_ptr[a]) return fail_arg(ctx, st.who, "list_ptr is not monotone");
        M = list_ptr[lists];
        if (M > 0 && !list_mem) return fail_arg(ctx, st.who, "null pointer");
        for (int64_t e = 0; e < M; ++e)
            if (list_mem[e] < -1 || list_mem[e] >= Bi) return fail_arg(ctx, st.who, "list_mem entry out of range");
        for (int32_t j = 0; j < Bj; ++j) {
            if (word_ptr[j + 1] < word_ptr[j]) return fail_arg(ctx, st.who, "word_ptr is not monotone");
            if (lists == 0) continue;                          // (no lists: every segment is written 0)
            if (list_of[j] < 0 || list_of[j] >= lists) return fail_arg(ctx, st.who, "list_of out of range");
            const int64_t k = (int64_t)list_ptr[list_of[j] + 1] - list_ptr[list_of[j]];
            if (self_pos[j] < 0 || self_pos[j] >= k) return fail_arg(ctx, st.who, "self_pos out of range");
            if (word_ptr[j + 1] - word_ptr[j] < (k + 31) / 32) return fail_arg(ctx, st.who, "segment of bits shorter than its list");
        }
        Wn = word_ptr[Bj];
        if (Wn > 0 && !bits) return fail_arg(ctx, st.who, "null pointer");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const double *dA, *dl, *du, *dX; const uint8_t *dok; const int32_t *dlp, *dlm, *dlo, *dsp; const int64_t *dwp;
    uint32_t *dbits; int32_t *dund;
    st.in(dA, Aj, (size_t)Bj * d * rj * 8); st.in(dl, lj, (size_t)Bj * rj * 8); st.in(du, uj, (size_t)Bj * rj * 8);
    st.in(dX, X, (size_t)Bi * d * 8); st.in(dok, ok, (size_t)Bi);
    st.in(dlp, list_ptr, ((size_t)lists + 1) * 4); st.in(dlm, list_mem, (size_t)M * 4);
    st.in(dlo, list_of, (size_t)Bj * 4); st.in(dsp, self_pos, (size_t)Bj * 4); st.in(dwp, word_ptr, ((size_t)Bj + 1) * 8);
    st.out(dbits, bits, (size_t)Wn * 4); st.out(dund, undecided, (size_t)Bj * 4);
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_members_outside_lists(d, rj, dA, dl, du, Bj, dX, dok, Bi, lists, dlp, dlm, dlo, dsp, dwp, t, dbits, dund,
                                                 ctx->stream));
    return st.finish();
}

// ---- inner-node records from a static store, a piece pool and column maps (qpn_parent.hip) ----------------------------------
int qpn_assemble_parent_nodes(qpn_ctx *ctx, int32_t items, int32_t form, int32_t n0, int32_t ne, int32_t m, int32_t p,
                              int32_t parents, int32_t mb, int32_t ps, const double *sQd, const double *sR, const double *sqd,
                              const double *sAd, const double *sB, const double *sl, const double *su, const int32_t *mb_true,
                              int32_t pieces, const int32_t *piece_desc, int32_t pool_rows, int32_t pool_words, const double *pA,
                              const double *pl, const double *pu, int32_t maps, const int32_t *map_off, int32_t map_words,
                              const int32_t *map_data, const int32_t *parent_of, const int32_t *piece_of, const int32_t *map_of,
                              double *Qd, double *R, double *qd, double *Ad, double *B, double *l, double *u, int32_t *err, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    Stage st(ctx, mem, "qpn_assemble_parent_nodes");
    if (items < 0 || (form != 0 && form != 1) || n0 <= 0 || ne < 0 || m < 0 || p < 1 || parents < 0 || mb < 0 || ps < 0 || pieces < 0 ||
        pool_rows < 0 || pool_words < 0 || maps < 0 || map_words < 0)
        return fail_arg(ctx, st.who, "bad sizes");
    if (form == 0) ne = 0;
    const int64_t n64 = (int64_t)n0 + ne;
    if (n64 + m > qpn_avi_max_n()) {
        ctx->last_error = std::string(st.who) + ": n0 + ne + m <= 1024 in ABI v1";
        return QPN_ERR_SIZE;
    }
    if (int rc = st.check()) return rc;
    if (items == 0) return QPN_OK;
    const size_t I = (size_t)items, n = (size_t)n64, P = (size_t)parents;
    if (!parent_of || !piece_of || !map_of || !Qd || !R || !qd || !err || (m && (!Ad || !B || !l || !u)) ||
        (parents && (!sQd || !sqd || !mb_true || (ps && !sR) || (mb && (!sAd || !sl || !su || (ps && !sB))))) ||
        (pieces && !piece_desc) || (pool_rows && (!pl || !pu)) || (pool_words && !pA) || (maps && !map_off) || (map_words && !map_data))
        return fail_arg(ctx, st.who, "null pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ParentArgs a{};
    a.items = items; a.form = form; a.n0 = n0; a.ne = ne; a.m = m; a.p = p; a.parents = parents; a.mb = mb; a.ps = ps;
    a.pieces = pieces; a.pool_rows = pool_rows; a.pool_words = pool_words; a.maps = maps; a.map_words = map_words;
    st.in(a.sQd, sQd, P * n0 * n0 * 8); st.in(a.sR, sR, P * ps * n0 * 8); st.in(a.sqd, sqd, P * n0 * 8);
    st.in(a.sAd, sAd, P * n0 * mb * 8); st.in(a.sB, sB, P * ps * mb * 8); st.in(a.sl, sl, P * mb * 8); st.in(a.su, su, P * mb * 8);
    st.in(a.mb_true, mb_true, P * 4);
    st.in(a.piece_desc, piece_desc, (size_t)pieces * 16); st.in(a.pA, pA, (size_t)pool_words * 8);
    st.in(a.pl, pl, (size_t)pool_rows * 8); st.in(a.pu, pu, (size_t)pool_rows * 8);
    st.in(a.map_off, map_off, maps ? ((size_t)maps + 1) * 4 : 0); st.in(a.map_data, map_data, (size_t)map_words * 4);
    st.in(a.parent_of, parent_of, I * 4); st.in(a.piece_of, piece_of, I * QPN_PARENT_SLOTS * 4);
    st.in(a.map_of, map_of, I * QPN_PARENT_SLOTS * 4);
    st.scratch(a.map_bad, (size_t)maps);
    st.out(a.Qd, Qd, I * n * n * 8); st.out(a.R, R, I * p * n * 8); st.out(a.qd, qd, I * n * 8);
    st.out(a.Ad, Ad, I * n * m * 8); st.out(a.B, B, I * p * m * 8); st.out(a.l, l, I * m * 8); st.out(a.u, u, I * m * 8);
    st.out(a.err, err, I * 4);
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_parent_records(a, ctx->stream));
    if ((rc = st.finish()) != QPN_OK) return rc;
    // host arrays: the kernel's own verdicts are the check (nothing was read through a bad index)
    for (size_t i = 0; st.host && i < I; ++i)
        if (err[i]) return fail_arg(ctx, st.who, "bad item (see err)");
    return QPN_OK;
}

// ---- batched LP solver (qpn_lp.hip) ----------------------------------------------------------------------------------------
void qpn_lp_default_opts(qpn_lp_opts *o)
{
    if (!o) return;
    o->piv_tol = 1e-9; o->feas_tol = 1e-9; o->opt_tol = 1e-9; o->check_tol = 1e-6; o->max_iters = 0; o->reserved = 0;
}

int qpn_lp_kernel_class(int32_t r, int32_t d) { return qpn_lp_class(r, d); }

int qpn_solve_lps(qpn_ctx *ctx, int32_t polys, int32_t r, int32_t d, const double *A, const double *l, const double *u, int32_t jobs,
                  const int32_t *poly_of, const double *cost, const int32_t *obj_row, const int32_t *obj_sign, const qpn_lp_opts *opts,
                  int32_t *status, double *x, double *obj, double *lambda, double *ray, int32_t *iters, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (polys < 0 || jobs < 0 || r <= 0 || d <= 0) return fail_arg(ctx, "qpn_solve_lps: bad sizes");
    if (r > QPN_LP_MAX_R || d > QPN_LP_MAX_D) { ctx->last_error = "qpn_solve_lps: d <= 256, r <= 1024 in ABI v1"; return QPN_ERR_SIZE; }
    Stage st(ctx, mem, "qpn_solve_lps");
    if (int rc = st.check()) return rc;
    if (jobs == 0) return QPN_OK;
    if (polys == 0 || !A || !l || !u || !poly_of || !status || (!cost && (!obj_row || !obj_sign))) return fail_arg(ctx, "qpn_solve_lps: null pointer");
    // host index arrays are checked here; device ones by the kernel (such a job answers QPN_LP_FAILURE)
    for (int t = 0; st.host && t < jobs; ++t)
        if (poly_of[t] < 0 || poly_of[t] >= polys || (!cost && (obj_row[t] < 0 || obj_row[t] >= r)))
            return fail_arg(ctx, "qpn_solve_lps: poly_of / obj_row out of range");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)polys, J = (size_t)jobs;
    LpArgs a{};
    a.polys = polys; a.r = r; a.d = d; a.jobs = jobs;
    a.lp = lp_tol(opts, r, d);
    void *gws;
    st.in(a.A, A, P * r * d * 8); st.in(a.l, l, P * r * 8); st.in(a.u, u, P * r * 8); st.in(a.poly_of, poly_of, J * 4);
    st.in(a.cost, cost, J * d * 8);
    st.in(a.obj_row, cost ? nullptr : obj_row, J * 4); st.in(a.obj_sign, cost ? nullptr : obj_sign, J * 4);
    st.out(a.status, status, J * 4);
    st.out_opt(a.x, x, J * d * 8);
    st.out_opt(a.obj, obj, J * 8);
    st.out_opt(a.lam, lambda, J * r * 8);
    st.out_opt(a.ray, ray, J * d * 8);
    st.out_opt(a.iters, iters, J * 4);
    st.scratch(gws, qpn_lp_workspace_bytes(jobs, r, d));
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_solve_lps(a, gws, ctx->stream));
    return st.finish();
}

int qpn_issubset_pairs(qpn_ctx *ctx, int32_t d, int32_t B1, int32_t r1, const double *A1, const double *l1, const double *u1,
                       int32_t B2, int32_t r2, const double *A2, const double *l2, const double *u2, int32_t pairs, const int32_t *pi,
                       const int32_t *pj, double tol, const qpn_lp_opts *opts, uint8_t *sub, int32_t *how, int32_t *bound, double *val,
                       int32_t *lps, int32_t *iters, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (B1 < 0 || B2 < 0 || pairs < 0 || r1 <= 0 || r2 <= 0 || d <= 0) return fail_arg(ctx, "qpn_issubset_pairs: bad sizes");
    if (r1 > QPN_LP_MAX_R || r2 > QPN_LP_MAX_R || d > QPN_LP_MAX_D) {
        ctx->last_error = "qpn_issubset_pairs: d <= 256, r1, r2 <= 1024 in ABI v1";
        return QPN_ERR_SIZE;
    }
    Stage st(ctx, mem, "qpn_issubset_pairs");
    if (int rc = st.check()) return rc;
    if (pairs == 0) return QPN_OK;
    if (B1 == 0 || B2 == 0 || !A1 || !l1 || !u1 || !A2 || !l2 || !u2 || !pi || !pj || !sub) return fail_arg(ctx, "qpn_issubset_pairs: null pointer");
    // host index arrays are checked here; device ones by the kernel (such a pair answers QPN_SUBSET_FAILURE)
    for (int q = 0; st.host && q < pairs; ++q)
        if (pi[q] < 0 || pi[q] >= B1 || pj[q] < 0 || pj[q] >= B2) return fail_arg(ctx, "qpn_issubset_pairs: pi / pj out of range");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)pairs;
    SubsetArgs a{};
    a.d = d; a.B1 = B1; a.r1 = r1; a.B2 = B2; a.r2 = r2; a.pairs = pairs; a.tol = tol;
    a.lp = lp_tol(opts, r1, d);
    void *gws;
    st.in(a.A1, A1, (size_t)B1 * r1 * d * 8); st.in(a.l1, l1, (size_t)B1 * r1 * 8); st.in(a.u1, u1, (size_t)B1 * r1 * 8);
    st.in(a.A2, A2, (size_t)B2 * r2 * d * 8); st.in(a.l2, l2, (size_t)B2 * r2 * 8); st.in(a.u2, u2, (size_t)B2 * r2 * 8);
    st.in(a.pi, pi, N * 4); st.in(a.pj, pj, N * 4);
    st.out(a.sub, sub, N);
    st.out_opt(a.how, how, N * 4);
    st.out_opt(a.bound, bound, N * 4);
    st.out_opt(a.val, val, N * 8);
    st.out_opt(a.lps, lps, N * 4);
    st.out_opt(a.iters, iters, N * 4);
    st.scratch(gws, qpn_lp_workspace_bytes(pairs, r1, d));
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_issubset_pairs(a, gws, ctx->stream));
    return st.finish();
}

int qpn_implicit_bounds(qpn_ctx *ctx, int32_t polys, int32_t r, int32_t d, const double *A, const double *l, const double *u, double tol,
                        int32_t flags, const qpn_lp_opts *opts, int32_t *status, int32_t *fail_row, uint8_t *eq, double *vals, int32_t *how,
                        double *lo, double *hi, int32_t *lps, int32_t *iters, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (polys < 0 || r <= 0 || d <= 0 || (flags & ~QPN_IB_ALL_EXTREMES)) return fail_arg(ctx, "qpn_implicit_bounds: bad sizes or flags");
    if (r > QPN_LP_MAX_R || d > QPN_LP_MAX_D) { ctx->last_error = "qpn_implicit_bounds: d <= 256, r <= 1024 in ABI v1"; return QPN_ERR_SIZE; }
    Stage st(ctx, mem, "qpn_implicit_bounds");
    if (int rc = st.check()) return rc;
    if (polys == 0) return QPN_OK;
    if (!A || !l || !u || !status || !eq || !vals) return fail_arg(ctx, "qpn_implicit_bounds: null pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)polys;
    IbArgs a{};
    a.polys = polys; a.r = r; a.d = d; a.flags = flags; a.tol = tol;
    a.lp = lp_tol(opts, r, d);
    void *gws;
    st.in(a.A, A, P * r * d * 8); st.in(a.l, l, P * r * 8); st.in(a.u, u, P * r * 8);
    st.out(a.status, status, P * 4); st.out(a.eq, eq, P * r); st.out(a.vals, vals, P * r * 8);
    st.out_opt(a.fail_row, fail_row, P * 4);
    st.out_opt(a.how, how, P * r * 4);
    st.out_opt(a.lo, lo, P * r * 8);
    st.out_opt(a.hi, hi, P * r * 8);
    st.out_opt(a.lps, lps, P * 4);
    st.out_opt(a.iters, iters, P * 4);
    st.scratch(gws, qpn_lp_workspace_bytes(polys, r, d));
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_implicit_bounds(a, gws, ctx->stream));
    return st.finish();
}

int qpn_irredundant_bounds(qpn_ctx *ctx, int32_t polys, int32_t r, int32_t d, const double *A, const double *l, const double *u, double tol,
                           const qpn_lp_opts *opts, int32_t *status, int32_t *fail_row, double *lr, double *ur, int32_t *how, double *ext,
                           int32_t *lps, int32_t *iters, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (polys < 0 || r <= 0 || d <= 0) return fail_arg(ctx, "qpn_irredundant_bounds: bad sizes");
    if (r > QPN_LP_MAX_R || d > QPN_LP_MAX_D) { ctx->last_error = "qpn_irredundant_bounds: d <= 256, r <= 1024 in ABI v1"; return QPN_ERR_SIZE; }
    Stage st(ctx, mem, "qpn_irredundant_bounds");
    if (int rc = st.check()) return rc;
    if (polys == 0) return QPN_OK;
    if (!A || !l || !u || !status || !lr || !ur) return fail_arg(ctx, "qpn_irredundant_bounds: null pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)polys;
    RedArgs a{};
    a.polys = polys; a.r = r; a.d = d; a.tol = tol;
    a.lp = lp_tol(opts, r, d);
    void *gws;
    st.in(a.A, A, P * r * d * 8); st.in(a.l, l, P * r * 8); st.in(a.u, u, P * r * 8);
    st.out(a.status, status, P * 4); st.out(a.lr, lr, P * r * 8); st.out(a.ur, ur, P * r * 8);
    st.out_opt(a.fail_row, fail_row, P * 4);
    st.out_opt(a.how, how, P * r * 2 * 4);
    st.out_opt(a.ext, ext, P * r * 2 * 8);
    st.out_opt(a.lps, lps, P * 4);
    st.out_opt(a.iters, iters, P * 4);
    st.scratch(gws, qpn_lp_workspace_bytes(polys, r, d));
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_irredundant_bounds(a, gws, ctx->stream));
    return st.finish();
}

int qpn_exemplar_polys(qpn_ctx *ctx, int32_t polys, int32_t n, int32_t d, const double *A, const double *l, const double *u,
                       const uint8_t *open_lo, const uint8_t *open_hi, double tol, double slack_cap, const qpn_lp_opts *opts,
                       uint8_t *empty, int32_t *how, double *eps, double *x, int32_t *row, double *lambda, int32_t *iters, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (polys < 0 || n <= 0 || d <= 0) return fail_arg(ctx, "qpn_exemplar_polys: bad sizes");
    if (n > QPN_EX_MAX_N || d > QPN_EX_MAX_D) { ctx->last_error = "qpn_exemplar_polys: n <= 511, d <= 255 in ABI v1"; return QPN_ERR_SIZE; }
    Stage st(ctx, mem, "qpn_exemplar_polys");
    if (int rc = st.check()) return rc;
    if (polys == 0) return QPN_OK;
    if (!A || !l || !u || !empty) return fail_arg(ctx, "qpn_exemplar_polys: null pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)polys, R = 2 * (size_t)n + 1;
    ExArgs a{};
    a.polys = polys; a.n = n; a.d = d; a.tol = tol; a.slack_cap = slack_cap;
    a.lp = lp_tol(opts, 2 * n + 1, d + 1);
    void *gws;
    st.in(a.A, A, P * n * d * 8); st.in(a.l, l, P * n * 8); st.in(a.u, u, P * n * 8);
    st.in(a.open_lo, open_lo, P * n); st.in(a.open_hi, open_hi, P * n);
    st.out(a.empty, empty, P);
    st.out_opt(a.how, how, P * 4);
    st.out_opt(a.eps, eps, P * 8);
    st.out_opt(a.x, x, P * d * 8);
    st.out_opt(a.row, row, P * 4);
    st.out_opt(a.lam, lambda, P * R * 8);
    st.out_opt(a.iters, iters, P * 4);
    st.scratch(gws, qpn_exemplar_workspace_bytes(polys, n, d));
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_exemplar_polys(a, gws, ctx->stream));
    return st.finish();
}

int qpn_exemplar_products(qpn_ctx *ctx, int32_t d, int32_t rows, const double *A, const double *l, const double *u,
                          const uint8_t *open_lo, const uint8_t *open_hi, int32_t pieces, const int32_t *piece_row, int32_t products,
                          int32_t n, int32_t k, const int32_t *factors, int32_t points, const double *point, const int32_t *point_of,
                          double point_tol, double tol, double slack_cap, const qpn_lp_opts *opts, uint8_t *near, uint8_t *empty,
                          int32_t *how, double *eps, double *x, int32_t *row, double *lambda, int32_t *iters, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (products < 0 || rows < 0 || pieces < 0 || points < 0 || n <= 0 || d <= 0 || k <= 0) return fail_arg(ctx, "qpn_exemplar_products: bad sizes");
    if (n > QPN_EX_MAX_N || d > QPN_EX_MAX_D || k > QPN_PROD_MAX_K) {
        ctx->last_error = "qpn_exemplar_products: n <= 511, d <= 255, k <= 32 in ABI v1";
        return QPN_ERR_SIZE;
    }
    Stage st(ctx, mem, "qpn_exemplar_products");
    if (int rc = st.check()) return rc;
    if (products == 0) return QPN_OK;
    if (!A || !l || !u || !piece_row || !factors || !near || !empty || rows == 0 || pieces == 0)
        return fail_arg(ctx, "qpn_exemplar_products: null pointer");
    if ((point == nullptr) != (point_of == nullptr) || (point && points == 0))
        return fail_arg(ctx, "qpn_exemplar_products: point and point_of go together");
    // host index arrays are checked here; device ones by the kernel (such a product answers QPN_EX_FAILURE)
    if (st.host) {
        for (int p = 0; p <= pieces; ++p)
            if (piece_row[p] < (p ? piece_row[p - 1] : 0) || piece_row[p] > rows) return fail_arg(ctx, "qpn_exemplar_products: piece_row not ascending within the pool");
        for (int t = 0; t < products; ++t) {
            int64_t total = 0;
            for (int s = 0; s < k; ++s) {
                const int32_t f = factors[(size_t)t * k + s];
                if (f < -1 || f >= pieces) return fail_arg(ctx, "qpn_exemplar_products: factor out of range");
                if (f >= 0) total += piece_row[f + 1] - piece_row[f];
            }
            if (total != n) return fail_arg(ctx, "qpn_exemplar_products: a product's rows do not add up to n");
            if (point_of && (point_of[t] < 0 || point_of[t] >= points)) return fail_arg(ctx, "qpn_exemplar_products: point_of out of range");
        }
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)products, R = 2 * (size_t)n + 1;
    ProdArgs a{};
    a.d = d; a.rows = rows; a.pieces = pieces; a.products = products; a.n = n; a.k = k; a.points = points;
    a.point_tol = point_tol; a.tol = tol; a.slack_cap = slack_cap;
    a.lp = lp_tol(opts, 2 * n + 1, d + 1);
    void *gws;
    st.in(a.A, A, (size_t)rows * d * 8); st.in(a.l, l, (size_t)rows * 8); st.in(a.u, u, (size_t)rows * 8);
    st.in(a.open_lo, open_lo, (size_t)rows); st.in(a.open_hi, open_hi, (size_t)rows);
    st.in(a.piece_row, piece_row, ((size_t)pieces + 1) * 4); st.in(a.factors, factors, P * k * 4);
    st.in(a.point, point, (size_t)points * d * 8); st.in(a.point_of, point_of, P * 4);
    st.out(a.near, near, P);
    st.out(a.empty, empty, P);
    st.out_opt(a.how, how, P * 4);
    st.out_opt(a.eps, eps, P * 8);
    st.out_opt(a.x, x, P * d * 8);
    st.out_opt(a.row, row, P * 4);
    st.out_opt(a.lam, lambda, P * R * 8);
    st.out_opt(a.iters, iters, P * 4);
    st.scratch(gws, qpn_products_workspace_bytes(products, n, d));
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_exemplar_products(a, gws, ctx->stream));
    return st.finish();
}

int qpn_intersection_trees(qpn_ctx *ctx, int32_t d, int32_t rows, const double *A, const double *l, const double *u,
                           const uint8_t *open_lo, const uint8_t *open_hi, int32_t pieces, const int32_t *piece_row, int32_t trees,
                           int32_t L, int32_t members, const int32_t *list_ptr, const int32_t *list_mem, const int32_t *list_red,
                           int32_t points, const double *point, const int32_t *point_of, double point_tol, double tol, double slack_cap,
                           const qpn_lp_opts *opts, int32_t cap, int32_t *leaves, int32_t *leaf_tree, int32_t *leaf_how,
                           int64_t *n_leaves, int32_t *tree_leaves, int64_t *tested, int64_t *alive, int64_t *unanswered,
                           int32_t *overflow, int mem)
{
    const char *who = "qpn_intersection_trees";
    if (!ctx) return QPN_ERR_ARG;
    if (trees < 0 || rows < 0 || pieces < 0 || points < 0 || members < 0 || d <= 0 || L <= 0 || cap <= 0) return fail_arg(ctx, who, "bad sizes");
    if (d > QPN_EX_MAX_D || L < 2 || L > QPN_TREE_MAX_L || cap > QPN_TREE_MAX_CAP) {
        ctx->last_error = std::string(who) + ": d <= 255, 2 <= L <= 32, cap <= 2^22 in ABI v1";
        return QPN_ERR_SIZE;
    }
    Stage st(ctx, mem, who);
    if (int rc = st.check()) return rc;
    if (!n_leaves || !overflow || !tested || !alive || !unanswered) return fail_arg(ctx, who, "null pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (trees == 0) {
        if (st.host) {
            *n_leaves = 0; *overflow = 0;
            for (int t = 0; t < L; ++t) tested[t] = alive[t] = unanswered[t] = 0;
            return QPN_OK;
        }
        HIPCHK(ctx, hipMemsetAsync(n_leaves, 0, 8, ctx->stream)); HIPCHK(ctx, hipMemsetAsync(overflow, 0, 4, ctx->stream));
        for (int64_t *p : {tested, alive, unanswered}) HIPCHK(ctx, hipMemsetAsync(p, 0, (size_t)L * 8, ctx->stream));
        return QPN_OK;
    }
    if (!A || !l || !u || !piece_row || !list_ptr || !list_red || (members && !list_mem) || !leaves || !leaf_tree || !leaf_how || !tree_leaves ||
        rows == 0 || pieces == 0)
        return fail_arg(ctx, who, "null pointer");
    if ((point == nullptr) != (point_of == nullptr) || (point && points == 0)) return fail_arg(ctx, who, "point and point_of go together");
    const size_t TL = (size_t)trees * L;
    // host index arrays are checked here and nothing is launched on a bad one; device ones by the kernel (such a tree answers -1)
    if (st.host) {
        for (int p = 0; p <= pieces; ++p)
            if (piece_row[p] < (p ? piece_row[p - 1] : 0) || piece_row[p] > rows) return fail_arg(ctx, who, "piece_row not ascending within the pool");
        if (list_ptr[0] < 0 || list_ptr[TL] > members) return fail_arg(ctx, who, "list_ptr not ascending within list_mem");
        for (size_t i = 0; i < TL; ++i)
            if (list_ptr[i + 1] < list_ptr[i]) return fail_arg(ctx, who, "list_ptr not ascending within list_mem");
        for (int g = 0; g < trees; ++g) {
            int64_t longest = 0;
            for (int t = 0; t < L; ++t) {
                const size_t li = (size_t)g * L + t;
                if (list_red[li] < 0 || list_red[li] > list_ptr[li + 1] - list_ptr[li]) return fail_arg(ctx, who, "list_red outside its list");
                int32_t most = 0;
                for (int32_t j = list_ptr[li]; j < list_ptr[li + 1]; ++j) {
                    const int32_t f = list_mem[j];
                    if (f < 0 || f >= pieces) return fail_arg(ctx, who, "member out of range");
                    if (piece_row[f + 1] == piece_row[f]) return fail_arg(ctx, who, "a member piece has no rows");
                    most = std::max(most, piece_row[f + 1] - piece_row[f]);
                }
                longest += most;
            }
            if (longest > QPN_EX_MAX_N) {
                ctx->last_error = std::string(who) + ": the longest pieces of a tree's lists add up to more than 511 rows";
                return QPN_ERR_SIZE;
            }
            if (point_of && (point_of[g] < 0 || point_of[g] >= points)) return fail_arg(ctx, who, "point_of out of range");
        }
    }
    qpn_lp_opts o;
    if (opts) o = *opts; else qpn_lp_default_opts(&o);
    TreeArgs a{};
    a.d = d; a.rows = rows; a.pieces = pieces; a.trees = trees; a.L = L; a.members = members; a.points = points; a.cap = cap;
    a.point_tol = point_tol; a.tol = tol; a.slack_cap = slack_cap;
    a.lp = LpTol{o.piv_tol, o.feas_tol, o.opt_tol, o.check_tol, o.max_iters};      // (max_iters <= 0: the default, by the size of each job)
    const size_t cp = (size_t)cap;
    void *ws;
    st.in(a.A, A, (size_t)rows * d * 8); st.in(a.l, l, (size_t)rows * 8); st.in(a.u, u, (size_t)rows * 8);
    st.in(a.open_lo, open_lo, (size_t)rows); st.in(a.open_hi, open_hi, (size_t)rows);
    st.in(a.piece_row, piece_row, ((size_t)pieces + 1) * 4);
    st.in(a.list_ptr, list_ptr, (TL + 1) * 4); st.in(a.list_mem, list_mem, (size_t)members * 4, 4); st.in(a.list_red, list_red, TL * 4);
    st.in(a.point, point, (size_t)points * d * 8); st.in(a.point_of, point_of, (size_t)trees * 4);
    st.out(a.leaves, leaves, cp * L * 4); st.out(a.leaf_tree, leaf_tree, cp * 4); st.out(a.leaf_how, leaf_how, cp * 4);
    st.out(a.n_leaves, n_leaves, 8); st.out(a.tree_leaves, tree_leaves, (size_t)trees * 4);
    st.out(a.tested, tested, (size_t)L * 8); st.out(a.alive, alive, (size_t)L * 8); st.out(a.unanswered, unanswered, (size_t)L * 8);
    st.out(a.overflow, overflow, 4);
    st.scratch(ws, qpn_tree_workspace_bytes(trees, L, members, cap, d));
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, qpn_run_intersection_trees(a, ws, ctx->stream));
    return st.finish();
}

} // extern "C"
