// qpn_capi.h -- what the translation units of the extern "C" boundary share (qpn_capi.hip, qpn_capi_nodes.hip): the context, the
// error mapping, the staging of one call's buffers and the views of node records.  Private to csrc/: not installed.
#pragma once

#include <string>
#include <vector>

#include "qpn_internal.h"

struct qpn_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string last_error;
    // grow-only device workspace used by the host-pointer paths and multi-kernel entry points
    void *ws = nullptr;
    size_t ws_bytes = 0;
    // schedule hint of qpn_solve_nodes (qpn_order_nodes_by_pivots / qpn_set_node_order): context-owned
    int32_t *order = nullptr;
    int32_t order_count = 0;      // 0 = no hint installed
    int32_t order_cap = 0;
    // automatic schedule hint (qpn_ctx_set_auto_schedule): refreshed from a call's own pivot counts every `period`
    // calls of the same batch size, unless the caller has installed a hint of their own
    int32_t auto_period = 16;
    int32_t auto_calls = 0;
    int32_t auto_batch = 0;
    bool order_user = false;
    // replicas of the iterate on peer GPUs (qpn_set_primal_mirrors)
    const double *mirror_own = nullptr;
    size_t mirror_bytes = 0;
    int32_t mirror_count = 0;
    double *mirror_peer[QPN_MAX_MIRRORS] = {};
    // route of mid-size node records (qpn_ctx_set_option QPN_OPT_MID_ROUTE): 1 the fused kernels (one wavefront per node up to 48,
    // one workgroup per node beyond), 0 the route of the large nodes / the general kernels (the tests' cross-check)
    int32_t mid_route = 1;
    // every route option change bumps this; a resident handle that learned its declines under another epoch asks again
    int32_t route_epoch = 0;
    // QPN_OPT_SYM_ROUTE: 1 = resident records whose Qd blocks are all bitwise symmetric take the kernel variants that use it
    int32_t sym_route = 1;
    // QPN_OPT_CRASH_CACHE: 1 = resident symmetric n = m = 32 records keep the parameter-free part of the crash across sweeps
    int32_t crash_cache = 1;
    // QPN_OPT_CRASH_CACHE_BIG: 1 = resident records on the blocked crash of large nodes keep what Qd and Ad alone decide
    int32_t crash_cache_big = 0;
    // QPN_OPT_WARM_BIG: 1 = sweeps over large resident nodes on the symmetric route that carry QPN_AVI_FLAG_WARM_DUALS start block
    // principal pivoting from the set the incoming multipliers name
    int32_t warm_big = 0;
    // QPN_OPT_LLC_BUDGET_MB: the share of the last-level cache, in MiB, that sweeps over the crash cache count on (llc_streams_crash,
    // qpn_internal.h); 0 = never stream the crash cache, -1 = always
    int32_t llc_budget_mb = kLlcBudgetMB;
};

// (nothing below is part of the library's interface: its symbols stay out of the dynamic table)
#pragma GCC visibility push(hidden)

inline int fail_hip(qpn_ctx *ctx, hipError_t e, const char *where)
{
    if (ctx) {
        ctx->last_error = std::string(where) + ": " + hipGetErrorString(e);
    }
    return QPN_ERR_HIP;
}
inline int fail_arg(qpn_ctx *ctx, const char *msg)
{
    if (ctx) ctx->last_error = msg;
    return QPN_ERR_ARG;
}
inline int fail_arg(qpn_ctx *ctx, const char *who, const char *what) { return fail_arg(ctx, (std::string(who) + ": " + what).c_str()); }

#define HIPCHK(ctx, call)                                        \
    do {                                                         \
        hipError_t e__ = (call);                                 \
        if (e__ != hipSuccess) return fail_hip(ctx, e__, #call); \
    } while (0)

// The buffers of one entry point call.  Device mode (QPN_MEM_DEVICE): the caller's pointers go to the kernels as they are.
// Host mode (QPN_MEM_HOST): each buffer gets a slot (256-B aligned) of the ctx workspace, begin() uploads the inputs in the
// order they were registered, finish() downloads the outputs in that order and waits for them.  Scratch and library-owned
// host data get a slot in both modes.  A slot of 0 bytes is a null pointer.  begin() writes the registered pointer variables
// and finish() reads them: they have to live until the call returns.
struct Stage {
    qpn_ctx *ctx;
    const char *who;
    bool host, bad_mem;
    size_t need = 0;
    struct Slot { void **dev; size_t off; };
    struct Copy { void **dev; void *host; size_t bytes, hpitch = 0, dpitch = 0, rows = 0; };   // rows > 0: 2-D, rows x bytes
    std::vector<Slot> slots;
    std::vector<Copy> up, down;

    Stage(qpn_ctx *c, int mem, const char *w)
        : ctx(c), who(w), host(mem == QPN_MEM_HOST), bad_mem(mem != QPN_MEM_HOST && mem != QPN_MEM_DEVICE) {}
    int check() const { return bad_mem ? fail_arg(ctx, who, "bad mem kind") : QPN_OK; }

    template <class T> void carve(T *&dev, size_t bytes)
    {
        dev = nullptr;
        if (!bytes) return;
        slots.push_back({(void **)&dev, need});
        need += (bytes + 255) & ~(size_t)255;
    }
    // an input; `pad` extra bytes keep the pointer valid when the array is empty or absent
    template <class T> void in(T *&dev, const void *src, size_t bytes, size_t pad = 0)
    {
        if (!host) { dev = (T *)src; return; }
        carve(dev, src || pad ? bytes + pad : 0);
        if (src && bytes) up.push_back({(void **)&dev, (void *)src, bytes});
    }
    // an output (host mode carves it even when the caller does not want it)
    template <class T> void out(T *&dev, void *dst, size_t bytes, size_t pad = 0)
    {
        if (!host) { dev = (T *)dst; return; }
        carve(dev, bytes + pad);
        if (dst && bytes) down.push_back({(void **)&dev, dst, bytes});
    }
    // an optional output: host mode carves it only when the caller wants it (the kernel skips a null one)
    template <class T> void out_opt(T *&dev, void *dst, size_t bytes)
    {
        dev = nullptr;
        if (dst || !host) out(dev, dst, bytes);
    }
    template <class T> void inout(T *&dev, T *p, size_t bytes, bool upload)
    {
        if (!host) { dev = p; return; }
        carve(dev, bytes);
        if (p && upload) up.push_back({(void **)&dev, p, bytes});
        if (p) down.push_back({(void **)&dev, p, bytes});
    }
    // host mode: `rows` blocks of `bytes` from a staged buffer (pitch dpitch) to the caller's (pitch hpitch)
    template <class T> void out2d(T *const &dev, size_t dpitch, void *dst, size_t hpitch, size_t bytes, size_t rows)
    {
        if (host) down.push_back({(void **)&dev, dst, bytes, hpitch, dpitch, rows});
    }
    template <class T> void scratch(T *&dev, size_t bytes) { carve(dev, bytes); }
    // host data the kernels read in either mode (index maps, offsets)
    template <class T> void lib_in(T *&dev, const void *src, size_t bytes)
    {
        carve(dev, bytes);
        if (bytes) up.push_back({(void **)&dev, (void *)src, bytes});
    }

    int begin()
    {
        if (int rc = check()) return rc;
        if (need > ctx->ws_bytes) {
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            if (ctx->ws) HIPCHK(ctx, hipFree(ctx->ws));
            ctx->ws = nullptr; ctx->ws_bytes = 0;
            size_t want = need + need / 4;
            HIPCHK(ctx, hipMalloc(&ctx->ws, want));
            ctx->ws_bytes = want;
        }
        for (auto &s : slots) *s.dev = static_cast<char *>(ctx->ws) + s.off;
        for (auto &c : up) HIPCHK(ctx, hipMemcpyAsync(*c.dev, c.host, c.bytes, hipMemcpyHostToDevice, ctx->stream));
        return QPN_OK;
    }
    int finish()
    {
        if (!host) return QPN_OK;
        for (auto &c : down) {
            if (c.rows) HIPCHK(ctx, hipMemcpy2DAsync(c.host, c.hpitch, *c.dev, c.dpitch, c.bytes, c.rows, hipMemcpyDeviceToHost, ctx->stream));
            else HIPCHK(ctx, hipMemcpyAsync(c.host, *c.dev, c.bytes, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return QPN_OK;
    }
};

struct NodeSizes { size_t Q, R, q, A, B, lu, w; };
inline NodeSizes node_sizes(int32_t batch, int32_t n, int32_t m, int32_t p, int64_t stride_w)
{
    NodeSizes s;
    s.Q = (size_t)batch * n * n * 8; s.R = (size_t)batch * n * p * 8; s.q = (size_t)batch * n * 8;
    s.A = (size_t)batch * m * n * 8; s.B = (size_t)batch * m * p * 8; s.lu = (size_t)batch * m * 8;
    // (w goes up only when p > 0: a stride alone names no data)
    s.w = p ? (stride_w ? (size_t)(batch - 1) * stride_w + p : (size_t)p) * 8 : 0;
    return s;
}

struct NodeDev {                // device views of one call's node records, parameters and outputs
    const double *Q, *R, *q, *A, *B, *l, *u, *w;
    double *z; int32_t *st; double *res; int32_t *pv; uint8_t *act;
};

// the seven record arrays (the padded ones stay valid when empty)
inline void stage_records(Stage &st, NodeDev &d, const NodeSizes &sz, const double *Qd, const double *R, const double *qd,
                          const double *Ad, const double *B, const double *l, const double *u)
{
    st.in(d.Q, Qd, sz.Q); st.in(d.R, R, sz.R, 8); st.in(d.q, qd, sz.q); st.in(d.A, Ad, sz.A, 8);
    st.in(d.B, B, sz.B, 8); st.in(d.l, l, sz.lu, 8); st.in(d.u, u, sz.lu, 8);
}

// ---- the node sweep (qpn_capi_nodes.hip), as far as qpn_interior_members needs it ---------------------------------------------
// Which kernels take the nodes of one qpn_solve_nodes call: decided once per call, from the shape, the pivot budget and the
// context's route options.
enum class NodeRoute {
    fused32,    // n, m <= 32: the fused MFMA kernel (qpn_avi_schur.hip)
    mid,        // 33 .. 128: the fused mid-size kernels (qpn_avi_schur48.hip, qpn_avi_schur_wg.hip, qpn_avi_schur_wg2.hip)
    big2,       // n 65 .. 256, m <= 256: the blocked crash straight from the records (qpn_avi_schur_big2.hip)
    general,    // assembled blocks on qpn_launch_avi_solve / qpn_launch_avi_solve_big
};
NodeRoute node_route(const qpn_ctx *ctx, int32_t n, int32_t m, const qpn_avi_opts &o);

struct NodeWs {                 // workspace of the general kernels: assembled blocks, large-item dictionaries (null when not carved)
    double *M, *q, *l, *u; uint8_t *kind; double *big;
};

// The lists a sweep of the fused routes may run under (batch + 1 words each, device).  Either makes it a sweep over a part of
// the nodes: no census of declines, no filling of a crash cache (sweep_partial, qpn_capi_nodes.hip).
struct SweepList {
    // qpn_solve_nodes_subset_h: the nodes to solve, the rest -1; takes the place of every installed order.  Such a sweep leaves
    // the handle's schedule and its pivot statistics alone as well.
    const int32_t *subset = nullptr;
    // QPN_AVI_FLAG_WARM_DUALS: receives the nodes the warm kernel declines (the order of the cold launches)
    int32_t *warm = nullptr;
    bool partial() const { return subset || warm; }
};

int solve_nodes_launch(qpn_ctx *ctx, qpn_nodes *h, int32_t batch, int32_t n, int32_t m, int32_t p, const NodeDev &d,
                       int64_t stride_w, const qpn_avi_opts &o, double *x_dev, int64_t stride_x, const NodeWs &ws,
                       NodeRoute route, const SweepList &sl = SweepList{});

int order_reserve(qpn_ctx *ctx, int32_t count);

#ifdef QPN_STAMPS
// diagnostic builds only: where the next device-path solve writes its [batch][8] cycle sums (qpn_debug_set_stamps, qpn_capi.hip)
extern unsigned long long *g_stamps;
#endif

#pragma GCC visibility pop
