// qpn_capi_nodes.hip -- the node sweep behind the extern "C" boundary (include/qpn_hip.h): qpn_solve_nodes and its kin, the
// resident node handle (qpn_nodes_*), the schedule hints and qpn_verify_nodes.  Host-side routing, staging and bookkeeping only;
// the rest of the boundary is qpn_capi.hip.
#include <cstdint>
#include <new>

#include "qpn_capi.h"

namespace {

// A count on its way to the host.  A kernel leaves the count in the device word; send() copies it to the pinned host word behind
// an event; poll(), at the start of later sweeps, settles the state once the event has passed.  No sweep waits for the answer.
struct HostCount {
    int32_t *dev = nullptr;
    int32_t *host = nullptr;
    hipEvent_t ev = nullptr;
    int state = 0;              // 0 unknown, 1 the count is on its way to the host, 2 all clear, 3 some

    hipError_t create()
    {
        hipError_t e = hipMalloc((void **)&dev, 4);
        if (e == hipSuccess) e = hipHostMalloc((void **)&host, 4, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e == hipSuccess) *host = 0;
        return e;
    }
    void destroy()              // (waits for an answer in flight: it is written to the host word)
    {
        (void)forget();
        if (ev) (void)hipEventDestroy(ev);
        if (dev) (void)hipFree(dev);
        if (host) (void)hipHostFree(host);
        *this = HostCount{};
    }
    void poll(int32_t all_clear)
    {
        if (state == 1 && hipEventQuery(ev) == hipSuccess) state = (*host == all_clear) ? 2 : 3;
    }
    hipError_t arm(hipStream_t s) { return hipMemsetAsync(dev, 0, 4, s); }
    hipError_t send(hipStream_t s)
    {
        hipError_t e = hipMemcpyAsync(host, dev, 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipEventRecord(ev, s);
        if (e == hipSuccess) state = 1;
        return e;
    }
    // what was counted is void: an answer still in flight must not be read as the next one's
    hipError_t forget()
    {
        const hipError_t e = state == 1 ? hipEventSynchronize(ev) : hipSuccess;
        state = 0;
        return e;
    }
};

// A cache of what Qd and Ad alone decide, kept by a resident handle across sweeps: the lifecycle that the crash caches of the
// 32-class and of the large class share.  Each cache has its own layout of buf, its own allocation step and its own predicate
// for `applies` (below).
struct CrashCache {
    double *buf = nullptr;          // allocated by the first sweep that would use it, kept until the handle goes
    uint8_t *flag = nullptr;        // a flag per node
    int state = 0;                  // 0 none, 1 valid (filled by one whole-batch sweep on `stream`), -1 its memory could not be had
    hipStream_t stream = nullptr;

    // Mode of the next sweep over the handle's records: 2 reuse, 1 fill, 0 run uncached.  applies: the context's options and the
    // records admit the cache; own_batch: the sweep is over the handle's batch; s: its stream; own_order: it runs under the
    // handle's own order; reuse_foreign: a valid cache may be reused under a foreign order.  alloc() is the cache's allocation
    // step: it runs once, and a failure is remembered (the handle runs uncached from then on), not reported.
    template <class Alloc>
    int mode(bool applies, bool own_batch, hipStream_t s, bool own_order, bool reuse_foreign, Alloc alloc)
    {
        if (!applies || !own_batch || state < 0) return 0;
        if (state == 1) {
            // a cache filled on another stream is not reused (there is no ordering with that stream), and stays valid
            if (stream != s) return 0;
            return (own_order || reuse_foreign) ? 2 : 0;
        }
        // a foreign order may leave nodes out (entries outside 0 .. count - 1): such a sweep fills nothing
        if (!own_order) return 0;
        if (!buf && alloc() != hipSuccess) {
            (void)hipGetLastError();            // (the failed allocation is not this sweep's error)
            free();
            state = -1;
            return 0;
        }
        return 1;
    }
    // valid only after the filling launch has been issued without error
    void filled(hipStream_t s) { state = 1; stream = s; }
    // the entries are void; the memory stays for the next fill
    void drop() { if (state == 1) state = 0; }
    void free()
    {
        if (buf) (void)hipFree(buf);
        if (flag) (void)hipFree(flag);
        buf = nullptr; flag = nullptr;
    }
    // for qpn_nodes_info: 1 = cached (valid, and the options admit it), 2 = refused (they do not, or its memory could not be had)
    int info(bool applies) const { return (state == 1 && applies ? 1 : 0) | (!applies || state < 0 ? 2 : 0); }
};

// Full-size staging of qpn_solve_nodes_subset_h, owned by the handle: the arrays the node kernels sweep, a node at its own
// index, and the two index arrays of the list kernel.  ONE allocation, made by the first subset call and kept until the handle
// goes.  w and z start as zeros (rows that no subset call has written stay finite) and keep what later calls leave in them.
struct SubsetStage {
    char *buf = nullptr;
    double *w = nullptr, *z = nullptr, *resid = nullptr;
    int32_t *status = nullptr, *pivots = nullptr;
    int32_t *slot_of = nullptr, *list = nullptr;        // [batch] | [batch + 1], contiguous: one fill sets both
    uint8_t *active = nullptr;

    hipError_t reserve(int32_t batch, int32_t N, int32_t p, hipStream_t s)
    {
        if (buf) return hipSuccess;
        const size_t b = (size_t)batch;
        const size_t bytes[7] = {b * (size_t)(p > 0 ? p : 1) * 8, b * N * 8, b * 8, b * 4, b * 4, (2 * b + 1) * 4, b * N};
        size_t off[7], total = 0;
        for (int i = 0; i < 7; ++i) { off[i] = total; total += (bytes[i] + 255) & ~(size_t)255; }
        hipError_t e = hipMalloc((void **)&buf, total);
        if (e == hipSuccess) e = hipMemsetAsync(buf, 0, off[2], s);
        if (e != hipSuccess) { free(); return e; }
        w = (double *)(buf + off[0]); z = (double *)(buf + off[1]); resid = (double *)(buf + off[2]);
        status = (int32_t *)(buf + off[3]); pivots = (int32_t *)(buf + off[4]);
        slot_of = (int32_t *)(buf + off[5]); list = slot_of + b;
        active = (uint8_t *)(buf + off[6]);
        return hipSuccess;
    }
    void free()
    {
        if (buf) (void)hipFree(buf);
        *this = SubsetStage{};
    }
};

} // namespace

// resident node records (qpn_nodes_upload): library-owned copies in HBM + what depends on them alone
struct qpn_nodes {
    int device = 0;
    int32_t batch = 0, n = 0, m = 0, p = 0;
    double *buf = nullptr;                      // one allocation, the seven arrays carved from it
    double *f[7] = {};                          // QPN_NODE_QD .. QPN_NODE_U
    size_t fbytes[7] = {};
    // does any node of these records need the general kernel?  The fused kernel adds its declines to the device word; all clear
    // is 0 (state 2: sweeps are ONE launch).  Allocated at upload.
    HostCount declines;
    // longest-first schedule of these nodes
    int32_t *order = nullptr;
    int32_t *key = nullptr;                     // smoothed pivot counts the order is made from
    bool order_valid = false;
    int32_t period = 16, calls = 0;
    // every Qd block bitwise symmetric?  Settled when the records arrive (one pass, nodes_check_symmetry)
    bool sym = false;
    // the context's route epoch the decline knowledge was learned under (qpn_ctx_set_option bumps it: another kernel variant
    // applies its pivot test to slightly different numbers, so "no node declines" has to be asked again)
    int32_t route_epoch = 0;
    // crash cache (symmetric n = m = 32 records): what Stage A of the fused kernel makes of Qd and Ad alone -- the panels U',
    // the tiles W~ and S in buf, a pass / fail flag per node (layout: qpn_internal.h) -- 22 528 bytes per node
    CrashCache crash;
    // did the last sweep fetch the crash cache with non-temporal loads?  (qpn_nodes_info bit 4)
    bool crash_streamed = false;
    // crash cache of the large class (QPN_OPT_CRASH_CACHE_BIG; layout: BigCrash, qpn_internal.h): buf holds top halves | S |
    // figures.  A node whose elimination stopped in a filling sweep has no entry and runs the filling kernels again in every
    // sweep; big_entries counts the nodes that have one, all clear is batch (state 2: reuse sweeps launch the replay kernel
    // alone).  Allocated with the cache.
    CrashCache big;
    HostCount big_entries;
    // qpn_nodes_set_warm: sweeps on the mid route that carry QPN_AVI_FLAG_WARM_DUALS run the warm kernel (qpn_warm_mid.hip) first
    bool warm_mid = false;
    // qpn_solve_nodes_subset_h: its full-size staging buffers
    SubsetStage subset;
};

NodeRoute node_route(const qpn_ctx *ctx, int32_t n, int32_t m, const qpn_avi_opts &o)
{
    if (n <= 32 && m <= 32 && m >= 1) return NodeRoute::fused32;
    // the crash of the larger fused routes makes n pivots: a caller-set budget has to leave Lemke at least one
    const bool budget = o.max_pivots <= 0 || o.max_pivots - n >= 1;
    // QPN_OPT_MID_ROUTE = 0 sends the mid-size nodes down the general route
    if (budget && ctx->mid_route == 1 && (qpn_schur_wg_shape(n, m) || qpn_schur_wg2_shape(n, m))) return NodeRoute::mid;
    if (budget && qpn_schur_big2_shape(n, m)) return NodeRoute::big2;
    return NodeRoute::general;
}

namespace {

// ---- the crash cache of the 32-class ------------------------------------------------------------------------------------
// Does the context's option set, and do the records, admit the crash cache?  (Symmetric n = m = 32 records on the symmetric
// route; the other size classes and the general variants run uncached.)
bool crash_cache_applies(const qpn_ctx *ctx, const qpn_nodes *h)
{
    return ctx->crash_cache == 1 && h->n == 32 && h->m == 32 && h->sym && ctx->sym_route == 1;
}

// Mixed reuse sweeps (qpn_avi_schur.hip, CRASH = 3): the share of the wavefronts that compute Stage A although the cache is
// valid, in 1/256ths (0: plain reuse sweeps), and the tail rule -- how many launch positions BEFORE the last partial round of
// the resident set already reuse, in 1/256ths of that set.  Both are tuning constants (-D for variant builds); no result
// depends on them.
#ifndef QPN_CRASH_MIX_SHARE
#define QPN_CRASH_MIX_SHARE 96
#endif
#ifndef QPN_CRASH_MIX_TAIL
#define QPN_CRASH_MIX_TAIL 0
#endif
constexpr int kCrashMixShare = QPN_CRASH_MIX_SHARE;
constexpr int kCrashMixTail = QPN_CRASH_MIX_TAIL;
static_assert(kCrashMixShare >= 0 && kCrashMixShare <= 256 && kCrashMixTail >= 0, "share in 1/256ths; tail >= 0");

// First launch position of the all-reuse tail: the last partial round of the resident set (it is bound by latency, not by HBM:
// the shorter chain wins there) and kCrashMixTail / 256 of a round before it.
int32_t crash_mix_reuse_from(int32_t batch)
{
    const int64_t full = (int64_t)(batch / kResidentMI355X) * kResidentMI355X;
    const int64_t from = full - (int64_t)kResidentMI355X * kCrashMixTail / 256;
    return (int32_t)(from > 0 ? from : 0);
}

// Crash-cache mode of the next fused sweep over the handle's records (CrashCache::mode).  A valid cache is reused under any
// order: the kernel looks a node's entry up by the node's index.
int crash_cache_mode(qpn_ctx *ctx, qpn_nodes *h, int32_t batch, bool own_order)
{
    if (!h) return 0;
    CrashCache &c = h->crash;
    return c.mode(crash_cache_applies(ctx, h), batch == h->batch, ctx->stream, own_order, true, [&] {
        hipError_t e = hipMalloc((void **)&c.buf, (size_t)batch * kCrashDoubles * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void **)&c.flag, (size_t)batch);
        return e;
    });
}

// ---- the crash cache of the large class ---------------------------------------------------------------------------------
// Does the context's option set, and do the records, admit it?  (Records that the default options send down the blocked crash.)
bool big_cache_applies(const qpn_ctx *ctx, const qpn_nodes *h)
{
    qpn_avi_opts o;
    qpn_avi_default_opts(&o);
    return ctx->crash_cache_big == 1 && node_route(ctx, h->n, h->m, o) == NodeRoute::big2;
}

BigCrash big_cache_views(const qpn_nodes *h)
{
    BigCrash bc{};
    bc.tt_stride = (int64_t)qpn_big_crash_tt_doubles(h->n, h->m);
    bc.s_stride = (int64_t)qpn_big_crash_s_doubles(h->m);
    bc.tt = h->big.buf;
    bc.S = bc.tt + (size_t)h->batch * (size_t)bc.tt_stride;
    bc.fig = bc.S + (size_t)h->batch * (size_t)bc.s_stride;
    bc.flag = h->big.flag;
    return bc;
}

// the entries are void (Qd or Ad replaced, the records moved off the route), and so is their census: only a valid cache has one
void big_cache_drop(qpn_nodes *h)
{
    (void)h->big_entries.forget();
    h->big.drop();
}

// Mode of the next sweep of the blocked crash over the handle's records (CrashCache::mode).  A valid cache is reused under a
// foreign order only when its census says that every node has an entry: the others would need the filling kernels, and a
// sweep under a foreign order fills nothing.
int big_cache_mode(qpn_ctx *ctx, qpn_nodes *h, int32_t batch, bool own_order)
{
    if (!h) return 0;
    const bool own_batch = batch == h->batch, applies = own_batch && big_cache_applies(ctx, h);
    if (applies && h->big.state >= 0) h->big_entries.poll(h->batch);        // (asked only while the cache is in use)
    return h->big.mode(applies, own_batch, ctx->stream, own_order, h->big_entries.state == 2, [&] {
        const BigCrash v = big_cache_views(h);
        const size_t doubles = (size_t)batch * ((size_t)v.tt_stride + (size_t)v.s_stride + 2);
        hipError_t e = hipMalloc((void **)&h->big.buf, doubles * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void **)&h->big.flag, (size_t)batch);
        if (e == hipSuccess) e = h->big_entries.create();
        if (e != hipSuccess) h->big_entries.destroy();
        return e;
    });
}

// ---- what a handle knows about its records ------------------------------------------------------------------------------
// one pass over the resident Qd blocks (behind the copies on the context's stream); waits for the answer
hipError_t nodes_check_symmetry(qpn_ctx *ctx, qpn_nodes *h)
{
    h->sym = false;
    int32_t *cnt = h->declines.dev;                    // (the decline counter is idle: no solve is in flight)
    hipError_t e = h->declines.arm(ctx->stream);
    if (e == hipSuccess) e = qpn_launch_qd_asymmetry(h->batch, h->n, h->f[QPN_NODE_QD], cnt, ctx->stream);
    int32_t asym = 1;
    if (e == hipSuccess) e = hipMemcpyAsync(&asym, cnt, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) h->sym = asym == 0;
    return e;
}

void nodes_poll_declines(qpn_nodes *h)
{
    if (h) h->declines.poll(0);
}
// a route option changed since the handle last learned its declines: forget the answer
void nodes_sync_route(qpn_ctx *ctx, qpn_nodes *h)
{
    if (!h || h->route_epoch == ctx->route_epoch) return;
    (void)h->declines.forget();
    h->route_epoch = ctx->route_epoch;
    // a new route epoch drops the 32-class cache always (the variants keep different tile sets), the large cache only when the
    // records have moved off the blocked crash
    h->crash.drop();
    if (!big_cache_applies(ctx, h)) big_cache_drop(h);
}

// Decline protocol of the fused routes.  Which nodes a fused kernel declines (status = -1) depends on Qd, Ad, l, u alone (block
// pivots of H, equality rows), never on w: a handle asks once -- the kernel counts its declines into the census' device word,
// declines_end sends the count to the host -- and leaves the general launches out once it knows that none does.
// *need_general: whether the general launches behind the fused kernel are needed.
int declines_begin(qpn_ctx *ctx, qpn_nodes *h, AviBatchArgs &a, bool *need_general)
{
    *need_general = true;
    if (!h) return QPN_OK;
    nodes_poll_declines(h);
    *need_general = h->declines.state != 2;
    if (h->declines.state == 0) {
        HIPCHK(ctx, h->declines.arm(ctx->stream));
        a.decl_count = h->declines.dev;
    }
    return QPN_OK;
}

int declines_end(qpn_ctx *ctx, qpn_nodes *h)
{
    if (!h || h->declines.state != 0) return QPN_OK;
    HIPCHK(ctx, h->declines.send(ctx->stream));
    return QPN_OK;
}

// Does the handle keep a longest-first schedule for launches of this size?  Only for launches beyond the fused kernel's resident
// set (`from` nodes): a smaller one has no tail to shorten.
bool schedules(const qpn_nodes *h, int32_t batch, int32_t from) { return h && h->period > 0 && batch > from; }

// The handle's longest-first schedule for the NEXT sweeps: the fused kernel keeps the smoothed pivot counts h->key up to date,
// the order is re-sorted from them every `period` sweeps while they settle (eight refreshes), every 4 x period afterwards: the
// sort is a one-workgroup launch (14 us) that the next sweep waits for.
int schedule_refresh(qpn_ctx *ctx, qpn_nodes *h, int32_t batch)
{
    const int32_t per = h->calls < 8 * h->period ? h->period : 4 * h->period;
    if (h->calls % per == 0) {
        HIPCHK(ctx, qpn_launch_order_by_pivots(nullptr, batch, h->order, ctx->stream, h->key));
        h->order_valid = true;
    }
    h->calls++;
    return QPN_OK;
}

// Where a sweep's primal blocks go besides z: the caller's iterate and, when the whole written range lies inside the registered
// buffer, its replicas on peer GPUs (qpn_set_primal_mirrors) at the same offset
struct PrimalOut {
    double *x; int64_t stride; bool mirrored; ptrdiff_t off;
};

// every primal block the kernel stores to x goes to the replicas too
void set_mirrors(const qpn_ctx *ctx, AviBatchArgs &a, ptrdiff_t x_off)
{
    a.n_mirror = ctx->mirror_count;
    for (int k = 0; k < ctx->mirror_count; ++k) a.mirror[k] = ctx->mirror_peer[k] + x_off;
}

// The general kernels, over the nodes a fused route declined (gated: status = -1) or over all of them.  The 32-class's is ONE
// small scan-mode register launch (assemble_in_scan: its waves pick the flagged nodes, assemble their blocks into the workspace
// and solve them); every other route assembles the blocks first and solves them on qpn_launch_avi_solve / _big.
int solve_general(qpn_ctx *ctx, const AviBatchArgs &a, const NodeWs &ws, bool gated, bool assemble_in_scan)
{
    if (!ws.M) return fail_arg(ctx, "qpn_solve_nodes: internal error (no workspace for the general path)");
    hipStream_t s = ctx->stream;
    const int N = a.N;
    AviBatchArgs g = a;
    g.decl_count = nullptr;
    g.M = ws.M; g.strideM = (int64_t)N * N; g.q = ws.q; g.l = ws.l; g.u = ws.u; g.kind = ws.kind; g.stride_kind = N;
    if (gated) { g.only_if = a.status; g.only_if_value = -1; }
    if (assemble_in_scan) {
        g.scan = 1; g.assemble_first = 1;
        HIPCHK(ctx, qpn_launch_avi_solve_reg(g, s));
        return QPN_OK;
    }
    const NodeSrc &r = a.nd;
    HIPCHK(ctx, qpn_launch_assemble_nodes(a.batch, r.n, r.m, r.p, r.Qd, r.R, r.qd, r.Ad, r.B, r.l, r.u, r.w, r.stride_w, ws.M,
                                          ws.q, ws.l, ws.u, ws.kind, s, g.only_if, g.only_if_value));
    if (N > 64) HIPCHK(ctx, qpn_launch_avi_solve_big(g, ws.big, s));
    else HIPCHK(ctx, qpn_launch_avi_solve(g, s));
    return QPN_OK;
}

// ---- a sweep under a list (SweepList): what the fused routes share -------------------------------------------------------
// The launch arguments under the lists of this sweep.  A subset list takes the place of whatever order `a` carries.
// QPN_AVI_FLAG_WARM_DUALS: the warm kernel goes first, over the nodes of that order.  What it accepts is done; the indices of
// the others come back compacted in sl.warm, padded with -1, and that list is the order of the cold launches -- out-of-range
// entries leave a slot unsolved, so nothing waits for the count on the host.
int sweep_lists(qpn_ctx *ctx, AviBatchArgs &a, const SweepList &sl,
                hipError_t (*launch_warm)(const AviBatchArgs &, int32_t *, hipStream_t))
{
    if (sl.subset) a.order = sl.subset;
    if (sl.warm) {
        HIPCHK(ctx, hipMemsetAsync(sl.warm, 0xFF, ((size_t)a.batch + 1) * 4, ctx->stream));
        HIPCHK(ctx, launch_warm(a, sl.warm, ctx->stream));
        a.order = sl.warm;
    }
    return QPN_OK;
}

// Decline protocol of a sweep that may run under a list.  A sweep over a part of the nodes is no census of the fused kernel's
// declines: the handle uses what it knows and learns nothing from this one.
int sweep_declines_begin(qpn_ctx *ctx, qpn_nodes *h, AviBatchArgs &a, const SweepList &sl, bool *need_general)
{
    if (!sl.partial()) return declines_begin(ctx, h, a, need_general);
    nodes_poll_declines(h);
    *need_general = !(h && h->declines.state == 2);
    return QPN_OK;
}

int sweep_declines_end(qpn_ctx *ctx, qpn_nodes *h, const SweepList &sl) { return sl.partial() ? QPN_OK : declines_end(ctx, h); }

// ---- the four routes of a sweep (solve_nodes_launch).  *x_in_kernel: the kernels wrote the primal blocks to `out` themselves ----

// n, m <= 32: the fused kernel, and the general kernel behind it, write the primal blocks themselves
int sweep_fused32(qpn_ctx *ctx, qpn_nodes *h, AviBatchArgs &a, const NodeWs &ws, const PrimalOut &out, const SweepList &sl,
                  bool *x_in_kernel)
{
    hipStream_t s = ctx->stream;
    const int32_t batch = a.batch;
    int rc = QPN_OK;
    if (out.x) { a.x = out.x; a.stride_x = out.stride; *x_in_kernel = true; }
    if (out.mirrored) set_mirrors(ctx, a, out.off);
    // schedule hint (longest first): the handle's own, else the context's
    // the smoothed counts are fed by every sweep while the schedule settles (128 sweeps), by every fourth one afterwards:
    // a sample of the sweeps tells the order as well, and the solve kernel's read-modify-write of its node's key is
    // 0.5 % of the sweep
    // (a subset call leaves the schedule and its statistics alone)
    const bool sched = schedules(h, batch, 4096) && !sl.subset;
    if (sched && (h->calls < 128 || (h->calls & 3) == 0)) a.sched_key = h->key;
    if (h && h->order_valid) a.order = h->order;
    else if (ctx->order_count == batch && (!h || ctx->order_user)) a.order = ctx->order;     // a caller-installed order also serves handles
    // The lists of this sweep (sweep_lists).  A list is not the handle's own order, so such a sweep does not FILL the crash
    // cache (it reuses a valid one -- the same bits either way), a mixed launch deals its two Stage A bodies by launch position
    // as ever, and of a warm sweep only the decliners feed the smoothed pivot counts of the schedule.
    if ((rc = sweep_lists(ctx, a, sl, qpn_launch_warm_nodes)) != QPN_OK) return rc;
    // resident symmetric n = m = 32 records: the first whole-batch sweep keeps the parameter-free part of the crash, the
    // later ones reuse it (same stream: no host synchronisation).  The handle's own order: none, or h->order -- asked after
    // the warm list has taken the order's place
    const int crash = crash_cache_mode(ctx, h, batch, a.order == nullptr || (h && a.order == h->order));
    if (crash) { a.crash = h->crash.buf; a.crash_flag = h->crash.flag; a.crash_mode = crash; }
    // a reuse sweep beyond the resident set is a mixed launch: kCrashMixShare / 256 of its wavefronts compute Stage A, which
    // trades HBM bytes for fp64-pipe cycles (the two variants saturate one each); the tail reuses (the shorter chain)
    if (crash == 2 && kCrashMixShare > 0 && batch > kResidentMI355X) {
        a.crash_share = kCrashMixShare;
        a.crash_reuse_from = crash_mix_reuse_from(batch);
    }
    // ... and it streams the crash cache past the last-level cache when that lets the node records stay there until the next sweep
    if (crash == 2 && llc_streams_crash(batch, a.nd.n, a.nd.m, a.nd.p, ctx->llc_budget_mb)) a.crash_stream = 1;
    if (h && !sl.subset) h->crash_streamed = a.crash_stream != 0;
    bool need_general;
    if ((rc = sweep_declines_begin(ctx, h, a, sl, &need_general)) != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_avi_solve_schur_nodes(a, s));
    if (crash == 1) h->crash.filled(s);
    if (need_general && (rc = solve_general(ctx, a, ws, true, true)) != QPN_OK) return rc;
    if ((rc = sweep_declines_end(ctx, h, sl)) != QPN_OK) return rc;
    if (h) {
        if (sched && (rc = schedule_refresh(ctx, h, batch)) != QPN_OK) return rc;
    } else if (sl.warm) {
        // (the pivot counts of this call are not those of a cold sweep: no schedule is made from them)
    } else if (ctx->auto_period > 0 && !ctx->order_user && a.pivots && batch > 4096) {
        // automatic longest-first schedule for the NEXT calls over this batch (launches that fill the GPU only)
        if (ctx->auto_batch != batch) { ctx->auto_batch = batch; ctx->auto_calls = 0; }
        if (ctx->auto_calls % ctx->auto_period == 0) {
            if ((rc = order_reserve(ctx, batch)) != QPN_OK) return rc;
            HIPCHK(ctx, qpn_launch_order_by_pivots(a.pivots, batch, ctx->order, s));
            ctx->order_count = batch;
        }
        ctx->auto_calls++;
    }
    return QPN_OK;
}

// mid-size nodes (n, m <= 128): one wavefront (max(n, m) <= 48) or one workgroup per node straight from the records, ONE
// launch; what they decline (status = -1) is assembled and solved by the general kernels in gated launches
// sl.warm (a handle that opted in, qpn_nodes_set_warm; the caller decides): the warm kernel goes first, as in the 32-class
int sweep_mid(qpn_ctx *ctx, qpn_nodes *h, AviBatchArgs &a, const NodeWs &ws, const PrimalOut &out, const SweepList &sl,
              bool *x_in_kernel)
{
    hipStream_t s = ctx->stream;
    const int32_t batch = a.batch, n = a.nd.n, m = a.nd.m;
    int rc = QPN_OK;
    bool need_general;
    if ((rc = sweep_declines_begin(ctx, h, a, sl, &need_general)) != QPN_OK) return rc;
    AviBatchArgs f = a;
    // the kernel writes the primal blocks into the iterate itself once it is known that nothing declines (the general
    // kernels behind it do not); until then the strided copy of solve_nodes_launch does
    if (out.x && !need_general) {
        f.x = out.x; f.stride_x = out.stride; *x_in_kernel = true;
        if (out.mirrored) set_mirrors(ctx, f, out.off);
    }
    // the handle's longest-first schedule as in the 32-class (launches beyond the resident set only: 2 048 wavefronts of the
    // one-wavefront kernel, 1 024 workgroups of the 49-64 class, 256 of the 65-128 class)
    const bool one_wave = qpn_schur48_shape(n, m), two_role = qpn_schur_wg2_shape(n, m);
    // (a subset call leaves the schedule and its statistics alone)
    const bool sched = schedules(h, batch, one_wave ? 2048 : (two_role ? 256 : 1024)) && !sl.subset;
    if (sched) { f.sched_key = h->key; if (h->order_valid) f.order = h->order; }
    // The lists of this sweep (sweep_lists).  QPN_AVI_FLAG_WARM_DUALS on a handle that opted in: the warm kernel writes the
    // primal blocks under the same rule, and only its decliners feed the smoothed pivot counts of the schedule.
    if ((rc = sweep_lists(ctx, f, sl, qpn_launch_warm_mid_nodes)) != QPN_OK) return rc;
    if (two_role) HIPCHK(ctx, qpn_launch_schur_wg2_nodes(f, s));
    else if (one_wave) HIPCHK(ctx, qpn_launch_avi_solve_schur48_nodes(f, s));
    else HIPCHK(ctx, qpn_launch_schur_wg_nodes(f, s));
    if (sched && (rc = schedule_refresh(ctx, h, batch)) != QPN_OK) return rc;
    if (need_general && (rc = solve_general(ctx, a, ws, true, false)) != QPN_OK) return rc;
    return sweep_declines_end(ctx, h, sl);
}

// large nodes (BASELINE config 5): the blocked crash straight from the records, the delayed-update Lemke kernel on the
// Schur problems, read-back and post-check on the records; no M is assembled unless a node declines -- those
// (status = -1) are assembled and solved by the general kernel in gated launches
// warm_big: Stage B starts from the set the multipliers of the incoming a.z name (QPN_OPT_WARM_BIG; solve_nodes_launch decides)
int sweep_big2(qpn_ctx *ctx, qpn_nodes *h, AviBatchArgs &a, const NodeWs &ws, bool warm_big)
{
    hipStream_t s = ctx->stream;
    const int32_t batch = a.batch;
    SchurBigWs sw{};
    double *dict = ws.big;
    void *sb = ws.big + (size_t)batch * (size_t)a.N * (size_t)(a.N + 1);
    // QPN_OPT_CRASH_CACHE_BIG, resident records: the first whole-batch sweep runs stage A in the handle's cache and keeps what
    // Qd and Ad alone decide; later sweeps replay the g column of the nodes that have an entry and run the filling kernels
    // for the others, as long as there are any (same stream: no host synchronisation).  The handle's own order: any but one
    // that the caller installed for this batch
    const int crash = big_cache_mode(ctx, h, batch, !(ctx->order_user && ctx->order_count == batch));
    if (crash) {
        const BigCrash bc = big_cache_views(h);
        // the filling sweep zeroes the flags: a node gets its entry from the kernels of this sweep or not at all
        if (crash == 1) HIPCHK(ctx, hipMemsetAsync(h->big.flag, 0, (size_t)batch, s));
        const bool fill = crash == 1 || h->big_entries.state != 2;
        HIPCHK(ctx, qpn_launch_schur_big2_stage_a_cached(a, sb, dict, &sw, bc, crash == 2, fill, s));
        if (crash == 1) h->big.filled(s);
        // the census of the entries is sent again only while none is in flight
        if (fill && h->big_entries.state != 1) {
            HIPCHK(ctx, qpn_launch_crash_big_count(batch, h->big.flag, h->big_entries.dev, s));
            HIPCHK(ctx, h->big_entries.send(s));
        }
    } else {
        HIPCHK(ctx, qpn_launch_schur_big2_stage_a(a, sb, dict, &sw, s));
    }
    // Stage B: resident records with symmetric Qd blocks (a.nd.sym) go through block principal pivoting first; whatever it
    // leaves (and every node otherwise) is the delayed-update Lemke kernel's
    // (a caller-set pivot budget is Lemke's to count: its pivots are the unit of max_pivots)
    const bool bpp = a.nd.sym && a.max_pivots <= 0;
    // (the hint is for the sweeps that launch it: with a pivot budget, or on the general variants, the flag changes nothing)
    if (bpp) HIPCHK(ctx, qpn_launch_schur_big_bpp(a, sw, dict, warm_big, s));
    HIPCHK(ctx, qpn_launch_schur_big_lemke(a, sw, dict, s, bpp ? 1 : 0));
    HIPCHK(ctx, qpn_launch_schur_big2_finish(a, sw, s));
    return solve_general(ctx, a, ws, true, false);
}

// every other shape, and the shapes above under options that close their route: the general kernels over all the nodes
int sweep_general(qpn_ctx *ctx, const AviBatchArgs &a, const NodeWs &ws) { return solve_general(ctx, a, ws, false, false); }

} // namespace

// The launches of one sweep over device-resident records and outputs.  `h` (may be null) owns the records:
// its decline knowledge and its schedule are used and refreshed.  ws = workspace of the general kernels (not carved
// only when h knows that no node declines).
int solve_nodes_launch(qpn_ctx *ctx, qpn_nodes *h, int32_t batch, int32_t n, int32_t m, int32_t p, const NodeDev &d,
                       int64_t stride_w, const qpn_avi_opts &o, double *x_dev, int64_t stride_x, const NodeWs &ws,
                       NodeRoute route, const SweepList &sl)
{
    hipStream_t s = ctx->stream;
    const int N = n + m;
    AviBatchArgs a{};
    a.batch = batch; a.N = N; a.z = d.z; a.status = d.st; a.resid = d.res; a.pivots = d.pv; a.active = d.act;
    a.check_tol = o.check_tol; a.piv_tol = o.piv_tol; a.feas_tol = o.feas_tol; a.comp_tol = o.comp_tol;
    // (the warm-start bit is this function's: the solve kernels see the flags of a call without it)
    a.max_pivots = o.max_pivots; a.flags = o.flags & 0xFFFF & ~QPN_AVI_FLAG_WARM_DUALS;
    a.nd = NodeSrc{n, m, p, d.Q, d.R, d.q, d.A, d.B, d.l, d.u, d.w, stride_w, (h && h->sym && ctx->sym_route == 1) ? 1 : 0};
    // QPN_OPT_WARM_BIG: large resident nodes on the symmetric route seed block principal pivoting from the caller's multipliers
    // (d.z carries them when the call is no cold start: solve_nodes_any makes a call without z one)
    const bool warm_big = ctx->warm_big == 1 && route == NodeRoute::big2 && a.nd.sym && o.max_pivots <= 0 && d.z &&
                          (o.flags & QPN_AVI_FLAG_WARM_DUALS) && !(o.flags & QPN_AVI_FLAG_COLD_START);
#ifdef QPN_STAMPS
    a.stamps = g_stamps;
#endif
    // replicas on peer GPUs: only when the whole written range lies inside the registered buffer
    const size_t x_span = x_dev ? ((size_t)(batch - 1) * (size_t)stride_x + (size_t)n) * 8 : 0;
    const bool mirrored = x_dev && ctx->mirror_count > 0 && (const char *)x_dev >= (const char *)ctx->mirror_own &&
                          (const char *)x_dev + x_span <= (const char *)ctx->mirror_own + ctx->mirror_bytes;
    const PrimalOut out{x_dev, stride_x, mirrored, mirrored ? x_dev - ctx->mirror_own : 0};
    bool x_in_kernel = false;
    int rc = QPN_OK;
    switch (route) {
    case NodeRoute::fused32: rc = sweep_fused32(ctx, h, a, ws, out, sl, &x_in_kernel); break;
    case NodeRoute::mid: rc = sweep_mid(ctx, h, a, ws, out, sl, &x_in_kernel); break;
    case NodeRoute::big2: rc = sweep_big2(ctx, h, a, ws, warm_big); break;
    case NodeRoute::general: rc = sweep_general(ctx, a, ws); break;
    }
    if (rc != QPN_OK) return rc;
    if (x_dev && !x_in_kernel) {     // strided device copy of the primal blocks (and to the replicas)
        HIPCHK(ctx, hipMemcpy2DAsync(x_dev, (size_t)stride_x * 8, d.z, (size_t)N * 8, (size_t)n * 8, (size_t)batch,
                                     hipMemcpyDeviceToDevice, s));
        for (int k = 0; mirrored && k < ctx->mirror_count; ++k)
            HIPCHK(ctx, hipMemcpy2DAsync(ctx->mirror_peer[k] + out.off, (size_t)stride_x * 8, d.z, (size_t)N * 8,
                                         (size_t)n * 8, (size_t)batch, hipMemcpyDefault, s));
    }
    return QPN_OK;
}

int order_reserve(qpn_ctx *ctx, int32_t count)
{
    if (count <= ctx->order_cap) return QPN_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));          // earlier launches may still read the old buffer
    if (ctx->order) { HIPCHK(ctx, hipFree(ctx->order)); ctx->order = nullptr; ctx->order_cap = 0; ctx->order_count = 0; }
    HIPCHK(ctx, hipMalloc((void **)&ctx->order, (size_t)count * 4));
    ctx->order_cap = count;
    return QPN_OK;
}

namespace {

// One sweep: stages host buffers (the records only when h == null), carves the workspace, launches, reads back.
int solve_nodes_any(qpn_ctx *ctx, qpn_nodes *h, int32_t batch, int32_t n, int32_t m, int32_t p, const double *Qd,
                    const double *R, const double *qd, const double *Ad, const double *B, const double *l, const double *u,
                    const double *w, int64_t stride_w, double *z, int32_t *status, double *resid, int32_t *pivots,
                    uint8_t *active, const qpn_avi_opts *opts, int mem, double *x, int64_t stride_x)
{
    Stage st(ctx, mem, "qpn_solve_nodes");
    if (int rc = st.check()) return rc;
    const int N = n + m;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    qpn_avi_opts o;
    if (opts) o = *opts; else qpn_avi_default_opts(&o);
    const size_t bN = (size_t)batch * N;
    const NodeRoute route = node_route(ctx, n, m, o);
    // the handle may already know that the general path behind a fused route has nothing to do: no workspace for it then
    nodes_poll_declines(h);
    nodes_sync_route(ctx, h);
    const bool fused = route == NodeRoute::fused32 || route == NodeRoute::mid;
    const bool need_ws = !(h && fused && h->declines.state == 2);

    NodeWs ws{};
    if (need_ws) {
        st.scratch(ws.M, bN * N * 8); st.scratch(ws.q, bN * 8); st.scratch(ws.l, bN * 8); st.scratch(ws.u, bN * 8);
        st.scratch(ws.kind, bN);
        if (N > 64) st.scratch(ws.big, qpn_avi_big_workspace_bytes(batch, N));
    }
    const NodeSizes sz = node_sizes(batch, n, m, p, stride_w);
    NodeDev d{Qd, R, qd, Ad, B, l, u};     // (a handle's records are resident)
    if (!h) stage_records(st, d, sz, Qd, R, qd, Ad, B, l, u);
    st.in(d.w, w, sz.w, 8);
    if (z) st.inout(d.z, z, bN * 8, !(o.flags & QPN_AVI_FLAG_COLD_START));
    else { st.scratch(d.z, bN * 8); o.flags |= QPN_AVI_FLAG_COLD_START; }   // no z wanted (handle calls): the kernels still need one
    st.out(d.st, status, (size_t)batch * 4); st.out(d.res, resid, (size_t)batch * 8); st.out(d.pv, pivots, (size_t)batch * 4);
    st.out(d.act, active, bN);
    // host mode: the primal blocks come down on their own (2.5 MB at 10 000 nodes; z is twice that), from a buffer of their own
    // when the fused kernel writes them
    const bool x_ws = st.host && x && route == NodeRoute::fused32;
    double *hx = nullptr;
    if (x_ws) st.scratch(hx, (size_t)batch * n * 8);
    if (x) st.out2d(x_ws ? hx : d.z, (size_t)(x_ws ? n : N) * 8, x, (size_t)stride_x * 8, (size_t)n * 8, (size_t)batch);
    // QPN_AVI_FLAG_WARM_DUALS: honoured by the 32-class, and by the mid route on a handle that opted in (qpn_nodes_set_warm), when
    // the caller's z carries a hint (z given, no cold start); the list of the nodes the warm kernel declines and its counter
    const bool warm_route = route == NodeRoute::fused32 || (route == NodeRoute::mid && h && h->warm_mid);
    const bool warm = warm_route && (o.flags & QPN_AVI_FLAG_WARM_DUALS) && !(o.flags & QPN_AVI_FLAG_COLD_START);
    int32_t *warm_list = nullptr;
    if (warm) st.scratch(warm_list, ((size_t)batch + 1) * 4);
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    rc = solve_nodes_launch(ctx, h, batch, n, m, p, d, stride_w, o, st.host ? hx : x, st.host ? (int64_t)n : stride_x, ws, route,
                            SweepList{nullptr, warm_list});
    if (rc != QPN_OK) return rc;
    return st.finish();
}

// A host index list: every entry in 0 .. batch - 1, no entry twice
bool subset_list_ok(const int32_t *idx, int32_t count, int32_t batch)
{
    std::vector<bool> seen((size_t)batch, false);
    for (int32_t s = 0; s < count; ++s) {
        if ((uint32_t)idx[s] >= (uint32_t)batch || seen[(size_t)idx[s]]) return false;
        seen[(size_t)idx[s]] = true;
    }
    return true;
}

// One sweep over the listed nodes of a handle (qpn_solve_nodes_subset_h): the caller's compact arrays are staged like those of
// any call, their rows go to the handle's full-size buffers and back (qpn_subset.hip), and the sweep in between is
// solve_nodes_launch over those buffers -- under the list on the fused routes, whose kernels take one, and an ordinary full
// sweep on the others.
int solve_nodes_subset(qpn_ctx *ctx, qpn_nodes *h, int32_t count, const int32_t *idx, const double *w, int64_t stride_w,
                       double *z, int32_t *status, double *resid, int32_t *pivots, uint8_t *active, const qpn_avi_opts *opts,
                       int mem, double *x, int64_t stride_x)
{
    Stage st(ctx, mem, "qpn_solve_nodes_subset_h");
    if (int rc = st.check()) return rc;
    const int32_t batch = h->batch, n = h->n, m = h->m, p = h->p;
    const int N = n + m;
    // a host list is checked before anything is launched; a device list is the list kernel's to check
    if (st.host && !subset_list_ok(idx, count, batch))
        return fail_arg(ctx, "qpn_solve_nodes_subset_h: idx entries must lie in [0, batch) and be pairwise distinct");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    qpn_avi_opts o;
    if (opts) o = *opts; else qpn_avi_default_opts(&o);
    const size_t bN = (size_t)batch * N, cN = (size_t)count * N;
    const NodeRoute route = node_route(ctx, n, m, o);
    nodes_poll_declines(h);
    nodes_sync_route(ctx, h);
    // the fused routes' kernels take a launch list; the others run a full sweep
    const bool fused = route == NodeRoute::fused32 || route == NodeRoute::mid;
    const bool need_ws = !(fused && h->declines.state == 2);
    SubsetStage &S = h->subset;
    // (a failed allocation is this call's error: the handle stays as it was)
    HIPCHK(ctx, S.reserve(batch, N, p, ctx->stream));

    NodeWs ws{};
    if (need_ws) {
        st.scratch(ws.M, bN * N * 8); st.scratch(ws.q, bN * 8); st.scratch(ws.l, bN * 8); st.scratch(ws.u, bN * 8);
        st.scratch(ws.kind, bN);
        if (N > 64) st.scratch(ws.big, qpn_avi_big_workspace_bytes(batch, N));
    }
    const int32_t *didx;
    const double *dw;
    st.in(didx, idx, (size_t)count * 4);
    st.in(dw, w, node_sizes(count, n, m, p, stride_w).w, 8);
    // the compact z: the hint on its way in (no cold start), the solution on its way out
    SubsetRows out{};
    if (z) st.inout(out.z, z, cN * 8, !(o.flags & QPN_AVI_FLAG_COLD_START));
    else o.flags |= QPN_AVI_FLAG_COLD_START;
    const bool hinted = !(o.flags & QPN_AVI_FLAG_COLD_START);
    st.out(out.status, status, (size_t)count * 4); st.out_opt(out.resid, resid, (size_t)count * 8);
    st.out_opt(out.pivots, pivots, (size_t)count * 4); st.out_opt(out.active, active, cN);
    // host mode: the primal blocks come down from a compact buffer of their own
    double *dx = x;
    if (st.host && x) {
        st.scratch(dx, (size_t)count * n * 8);
        st.out2d(dx, (size_t)n * 8, x, (size_t)stride_x * 8, (size_t)n * 8, (size_t)count);
    }
    const bool warm_route = route == NodeRoute::fused32 || (route == NodeRoute::mid && h->warm_mid);
    int32_t *warm_list = nullptr;
    if (warm_route && hinted && (o.flags & QPN_AVI_FLAG_WARM_DUALS)) st.scratch(warm_list, ((size_t)batch + 1) * 4);
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    hipStream_t s = ctx->stream;
    HIPCHK(ctx, hipMemsetAsync(S.slot_of, 0xFF, (2 * (size_t)batch + 1) * 4, s));
    // the gated general launch (status = -1) must see this call's decliners only
    HIPCHK(ctx, hipMemsetAsync(S.status, 0, (size_t)batch * 4, s));
    HIPCHK(ctx, qpn_launch_subset_list(count, batch, didx, S.slot_of, S.list, s));
    // a shared w (stride 0) is read where it is
    const bool own_w = p > 0 && stride_w != 0;
    HIPCHK(ctx, qpn_launch_subset_scatter(count, S.list, p, N, own_w ? dw : nullptr, stride_w, S.w, hinted ? out.z : nullptr, S.z, s));
    const NodeDev d{h->f[0], h->f[1], h->f[2], h->f[3], h->f[4], h->f[5], h->f[6], own_w ? S.w : dw,
                    S.z, S.status, S.resid, S.pivots, S.active};
    rc = solve_nodes_launch(ctx, h, batch, n, m, p, d, own_w ? (int64_t)p : 0, o, nullptr, 0, ws, route,
                            SweepList{fused ? S.list : nullptr, warm_list});
    if (rc != QPN_OK) return rc;
    const SubsetRows full{S.z, S.status, S.resid, S.pivots, S.active};
    HIPCHK(ctx, qpn_launch_subset_gather(count, S.list, n, N, full, out, dx, st.host ? (int64_t)n : stride_x, s));
    return st.finish();
}

// A host index list of the verify form: every entry in 0 .. batch - 1 (an entry may come more than once)
bool verify_list_ok(const int32_t *idx, int32_t count, int32_t batch)
{
    for (int32_t s = 0; s < count; ++s)
        if ((uint32_t)idx[s] >= (uint32_t)batch) return false;
    return true;
}

// qpn_verify_nodes, qpn_verify_nodes_h and, with a list (idx != nullptr: `count` slots over the `batch` resident records, slot s
// verifying record idx[s]), qpn_verify_nodes_subset_h.  `items` -- the nodes of the full call, the slots of the list form -- sizes
// every per-item array and all scratch, and is the grid.
int verify_nodes_any(qpn_ctx *ctx, bool records_on_device, int32_t batch, int32_t n, int32_t m, int32_t p,
                     const double *Qd, const double *R, const double *qd, const double *Ad, const double *B,
                     const double *l, const double *u, const double *xd, const double *w, int64_t stride_w, double tol,
                     int32_t *solution, double *lambda, int32_t *path, int mem, const char *who = "qpn_verify_nodes",
                     int32_t count = 0, const int32_t *idx = nullptr)
{
    if (!ctx) return QPN_ERR_ARG;
    if (batch < 0 || n <= 0 || m < 0 || p < 0) return fail_arg(ctx, who, "bad sizes");
    const int32_t items = idx ? count : batch;
    if (items == 0) return QPN_OK;
    if (n > qpn_verify_max_dim() || m > qpn_verify_max_dim()) { ctx->last_error = std::string(who) + ": n, m <= 512 in ABI v1"; return QPN_ERR_SIZE; }
    const bool wide_avi = m > 64;         // the bounded-LSQ fallback of wide nodes runs on the large-item AVI kernel
    if (!Qd || !qd || !xd || (m > 0 && (!Ad || !l || !u || !lambda)) || (p > 0 && (!R || !w || (m > 0 && !B))) ||
        !solution || !path)
        return fail_arg(ctx, who, "null pointer");
    if (stride_w != 0 && stride_w < p) return fail_arg(ctx, who, "stride_w < p");
    Stage st(ctx, mem, who);
    // a host list is checked before anything is staged or launched; a device list is the kernels' to check
    if (idx) {
        if (int rc = st.check()) return rc;
        if (st.host && !verify_list_ok(idx, count, batch)) return fail_arg(ctx, who, "idx entries must lie in [0, batch)");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t mm = (size_t)(m > 0 ? m : 1);
    const bool wide = n > QPN_VERIFY_WIDE_FROM || m > QPN_VERIFY_WIDE_FROM;
    const bool mid = !wide && (n > 32 || m > 32);      // verify_node64's class: a small slot workspace for the nodes it hands on
    const size_t mp16 = (size_t)((m + 15) & ~15);
    const NodeSizes sz_ = node_sizes(items, n, m, p, stride_w);
    NodeDev d{Qd, R, qd, Ad, B, l, u};
    if (!records_on_device) stage_records(st, d, sz_, Qd, R, qd, Ad, B, l, u);
    const double *dx; double *dlam; int32_t *dsol, *dpath; const int32_t *didx = nullptr;
    if (idx) st.in(didx, idx, (size_t)items * 4);
    st.in(dx, xd, sz_.q); st.in(d.w, w, sz_.w, 8);
    st.out(dsol, solution, (size_t)items * 4); st.out(dpath, path, (size_t)items * 4); st.out(dlam, lambda, sz_.lu, 8);
    // scratch of the bounded-LSQ fallback (src/qp_processing.jl:129-137): Gram block + vectors
    double *sG, *sq, *slb, *sub, *sz, *sres, *wbig = nullptr, *gws = nullptr; int32_t *sst;
    st.scratch(sG, (size_t)items * mm * mm * 8); st.scratch(sq, (size_t)items * mm * 8);
    st.scratch(slb, (size_t)items * mm * 8); st.scratch(sub, (size_t)items * mm * 8);
    st.scratch(sz, (size_t)items * mm * 8); st.scratch(sres, (size_t)items * 8); st.scratch(sst, (size_t)items * 4);
    if (wide_avi) st.scratch(wbig, qpn_avi_big_workspace_bytes(items, m));
    if (wide && m > 0) st.scratch(gws, (size_t)items * 2 * mp16 * mp16 * 8);
    else if (mid && m > 0) st.scratch(gws, (size_t)QPN_VERIFY_MID_SLOTS * 2 * mp16 * mp16 * 8 + 64);
    int rc = st.begin();
    if (rc != QPN_OK) return rc;
    if (idx)
        HIPCHK(ctx, qpn_launch_verify_nodes_list(items, didx, batch, n, m, p, d.Q, d.R, d.q, d.A, d.B, d.l, d.u, dx, d.w, stride_w,
                                                 tol, dsol, dlam, dpath, sG, sq, slb, sub, sz, sres, sst, ctx->stream, wbig, gws));
    else
        HIPCHK(ctx, qpn_launch_verify_nodes(batch, n, m, p, d.Q, d.R, d.q, d.A, d.B, d.l, d.u, dx, d.w, stride_w, tol,
                                            dsol, dlam, dpath, sG, sq, slb, sub, sz, sres, sst, ctx->stream, wbig, gws));
    return st.finish();
}

} // namespace

extern "C" {

int qpn_solve_nodes_into(qpn_ctx *ctx, int32_t batch, int32_t n, int32_t m, int32_t p, const double *Qd,
                         const double *R, const double *qd, const double *Ad, const double *B,
                         const double *l, const double *u, const double *w, int64_t stride_w, double *z,
                         int32_t *status, double *resid, int32_t *pivots, uint8_t *active,
                         const qpn_avi_opts *opts, int mem, double *x, int64_t stride_x)
{
    if (!ctx) return QPN_ERR_ARG;
    if (x && stride_x < n) return fail_arg(ctx, "qpn_solve_nodes_into: stride_x < n");
    if (batch < 0 || n <= 0 || m < 0 || p < 0) return fail_arg(ctx, "qpn_solve_nodes: bad sizes");
    if (batch == 0) return QPN_OK;
    if (!Qd || !qd || (m > 0 && (!Ad || !l || !u)) || (p > 0 && (!R || !w || (m > 0 && !B))) || !z || !status)
        return fail_arg(ctx, "qpn_solve_nodes: null pointer");
    if (stride_w != 0 && stride_w < p) return fail_arg(ctx, "qpn_solve_nodes: stride_w < p");
    if (n + m > qpn_avi_max_n()) { ctx->last_error = "qpn_solve_nodes: n+m > 1024 not supported by ABI v1"; return QPN_ERR_SIZE; }
    return solve_nodes_any(ctx, nullptr, batch, n, m, p, Qd, R, qd, Ad, B, l, u, w, stride_w, z, status, resid, pivots,
                           active, opts, mem, x, stride_x);
}

int qpn_solve_nodes(qpn_ctx *ctx, int32_t batch, int32_t n, int32_t m, int32_t p, const double *Qd,
                    const double *R, const double *qd, const double *Ad, const double *B,
                    const double *l, const double *u, const double *w, int64_t stride_w, double *z,
                    int32_t *status, double *resid, int32_t *pivots, uint8_t *active,
                    const qpn_avi_opts *opts, int mem)
{
    return qpn_solve_nodes_into(ctx, batch, n, m, p, Qd, R, qd, Ad, B, l, u, w, stride_w, z, status, resid,
                                pivots, active, opts, mem, nullptr, 0);
}

// ---- resident node records ------------------------------------------------------------------------------------
int qpn_nodes_free(qpn_ctx *ctx, qpn_nodes *h)
{
    if (!ctx) return QPN_ERR_ARG;
    if (!h) return QPN_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(ctx->stream);
    h->declines.destroy();
    h->big_entries.destroy();
    h->crash.free();
    h->big.free();
    h->subset.free();
    if (h->buf) (void)hipFree(h->buf);
    if (h->order) (void)hipFree(h->order);
    if (h->key) (void)hipFree(h->key);
    delete h;
    return QPN_OK;
}

int qpn_nodes_upload(qpn_ctx *ctx, int32_t batch, int32_t n, int32_t m, int32_t p, const double *Qd,
                     const double *R, const double *qd, const double *Ad, const double *B, const double *l,
                     const double *u, int mem, qpn_nodes **out)
{
    if (!ctx) return QPN_ERR_ARG;
    if (!out) return fail_arg(ctx, "qpn_nodes_upload: null out");
    *out = nullptr;
    if (batch <= 0 || n <= 0 || m < 0 || p < 0) return fail_arg(ctx, "qpn_nodes_upload: bad sizes");
    if (!Qd || !qd || (m > 0 && (!Ad || !l || !u)) || (p > 0 && (!R || (m > 0 && !B))))
        return fail_arg(ctx, "qpn_nodes_upload: null pointer");
    if (mem != QPN_MEM_HOST && mem != QPN_MEM_DEVICE) return fail_arg(ctx, "qpn_nodes_upload: bad mem kind");
    if (n + m > qpn_avi_max_n()) { ctx->last_error = "qpn_nodes_upload: n+m > 1024 not supported by ABI v1"; return QPN_ERR_SIZE; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    qpn_nodes *h = new (std::nothrow) qpn_nodes();
    if (!h) return fail_arg(ctx, "qpn_nodes_upload: out of host memory");
    h->device = ctx->device; h->batch = batch; h->n = n; h->m = m; h->p = p;
    const NodeSizes sz = node_sizes(batch, n, m, p, 0);
    const size_t fb[7] = {sz.Q, sz.R, sz.q, sz.A, sz.B, sz.lu, sz.lu};
    const double *src[7] = {Qd, R, qd, Ad, B, l, u};
    size_t total = 0, off[7];
    for (int i = 0; i < 7; ++i) { off[i] = total; total += (fb[i] + 8 + 255) & ~(size_t)255; h->fbytes[i] = fb[i]; }
    hipError_t e = hipMalloc((void **)&h->buf, total);
    if (e == hipSuccess) e = h->declines.create();
    if (e == hipSuccess) e = hipMalloc((void **)&h->order, (size_t)batch * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&h->key, (size_t)batch * 4);
    if (e == hipSuccess) e = hipMemsetAsync(h->key, 0, (size_t)batch * 4, ctx->stream);
    const hipMemcpyKind kind = mem == QPN_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    for (int i = 0; i < 7 && e == hipSuccess; ++i) {
        h->f[i] = reinterpret_cast<double *>(reinterpret_cast<char *>(h->buf) + off[i]);
        if (fb[i]) e = hipMemcpyAsync(h->f[i], src[i], fb[i], kind, ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);     // the caller's arrays are free again on return
    if (e == hipSuccess) e = nodes_check_symmetry(ctx, h);
    if (e != hipSuccess) { int rc = fail_hip(ctx, e, "qpn_nodes_upload"); qpn_nodes_free(ctx, h); return rc; }
    *out = h;
    return QPN_OK;
}

int qpn_nodes_update(qpn_ctx *ctx, qpn_nodes *h, int32_t field, const double *data, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (!h || field < 0 || field > 6 || !data) return fail_arg(ctx, "qpn_nodes_update: bad argument");
    if (mem != QPN_MEM_HOST && mem != QPN_MEM_DEVICE) return fail_arg(ctx, "qpn_nodes_update: bad mem kind");
    if (h->device != ctx->device) return fail_arg(ctx, "qpn_nodes_update: handle belongs to another device");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (h->fbytes[field])
        HIPCHK(ctx, hipMemcpyAsync(h->f[field], data, h->fbytes[field],
                                   mem == QPN_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ctx->stream));
    if (mem == QPN_MEM_HOST) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // what was known about the old records is void
    HIPCHK(ctx, h->declines.forget());
    // both crash caches are made of Qd and Ad alone: replacing either drops them, R, qd, B, l, u keep them
    if (field == QPN_NODE_QD || field == QPN_NODE_AD) { h->crash.drop(); big_cache_drop(h); }
    if (field == QPN_NODE_QD) HIPCHK(ctx, nodes_check_symmetry(ctx, h));
    return QPN_OK;
}

int qpn_nodes_set_schedule(qpn_ctx *ctx, qpn_nodes *h, int32_t period)
{
    if (!ctx) return QPN_ERR_ARG;
    if (!h || period < 0) return fail_arg(ctx, "qpn_nodes_set_schedule: bad argument");
    h->period = period; h->calls = 0;
    if (period == 0) h->order_valid = false;
    return QPN_OK;
}

int qpn_nodes_set_warm(qpn_ctx *ctx, qpn_nodes *h, int32_t on)
{
    if (!ctx) return QPN_ERR_ARG;
    if (!h || (on != 0 && on != 1)) return fail_arg(ctx, "qpn_nodes_set_warm: bad argument");
    // only the shapes of the mid route have this switch: n, m <= 32 honour the flag anyway, larger nodes have QPN_OPT_WARM_BIG
    if (qpn_schur_wg_shape(h->n, h->m) || qpn_schur_wg2_shape(h->n, h->m)) h->warm_mid = on == 1;
    return QPN_OK;
}

int qpn_nodes_info(qpn_ctx *ctx, qpn_nodes *h, int32_t info[4])
{
    if (!ctx) return QPN_ERR_ARG;
    if (!h || !info) return fail_arg(ctx, "qpn_nodes_info: null argument");
    nodes_poll_declines(h);
    info[0] = h->declines.state; info[1] = h->declines.state >= 2 ? *h->declines.host : 0;
    // bits 2, 3: the 32-class cache is valid / refused; 5, 6: the large class's
    info[2] = (h->order_valid ? 1 : 0) | (h->sym ? 2 : 0) | (h->crash_streamed ? 16 : 0) |
              (h->crash.info(crash_cache_applies(ctx, h)) << 2) | (h->big.info(big_cache_applies(ctx, h)) << 5);
    info[3] = h->calls;
    return QPN_OK;
}

int qpn_solve_nodes_h(qpn_ctx *ctx, qpn_nodes *h, const double *w, int64_t stride_w, double *z,
                      int32_t *status, double *resid, int32_t *pivots, uint8_t *active,
                      const qpn_avi_opts *opts, int mem, double *x, int64_t stride_x)
{
    if (!ctx) return QPN_ERR_ARG;
    if (!h) return fail_arg(ctx, "qpn_solve_nodes_h: null handle");
    if (h->device != ctx->device) return fail_arg(ctx, "qpn_solve_nodes_h: handle belongs to another device");
    if (x && stride_x < h->n) return fail_arg(ctx, "qpn_solve_nodes_h: stride_x < n");
    if (!status || (h->p > 0 && !w)) return fail_arg(ctx, "qpn_solve_nodes_h: null pointer");
    if (stride_w != 0 && stride_w < h->p) return fail_arg(ctx, "qpn_solve_nodes_h: stride_w < p");
    return solve_nodes_any(ctx, h, h->batch, h->n, h->m, h->p, h->f[0], h->f[1], h->f[2], h->f[3], h->f[4], h->f[5], h->f[6],
                           w, stride_w, z, status, resid, pivots, active, opts, mem, x, stride_x);
}

int qpn_solve_nodes_subset_h(qpn_ctx *ctx, qpn_nodes *h, int32_t count, const int32_t *idx, const double *w,
                             int64_t stride_w, double *z, int32_t *status, double *resid, int32_t *pivots, uint8_t *active,
                             const qpn_avi_opts *opts, int mem, double *x, int64_t stride_x)
{
    if (!ctx) return QPN_ERR_ARG;
    if (!h) return fail_arg(ctx, "qpn_solve_nodes_subset_h: null handle");
    if (h->device != ctx->device) return fail_arg(ctx, "qpn_solve_nodes_subset_h: handle belongs to another device");
    if (count < 0 || count > h->batch) return fail_arg(ctx, "qpn_solve_nodes_subset_h: count outside [0, batch]");
    if (count == 0) return QPN_OK;
    if (x && stride_x < h->n) return fail_arg(ctx, "qpn_solve_nodes_subset_h: stride_x < n");
    if (!idx || !status || (h->p > 0 && !w)) return fail_arg(ctx, "qpn_solve_nodes_subset_h: null pointer");
    if (stride_w != 0 && stride_w < h->p) return fail_arg(ctx, "qpn_solve_nodes_subset_h: stride_w < p");
    return solve_nodes_subset(ctx, h, count, idx, w, stride_w, z, status, resid, pivots, active, opts, mem, x, stride_x);
}

int qpn_verify_nodes(qpn_ctx *ctx, int32_t batch, int32_t n, int32_t m, int32_t p,
                     const double *Qd, const double *R, const double *qd, const double *Ad,
                     const double *B, const double *l, const double *u, const double *xd,
                     const double *w, int64_t stride_w, double tol, int32_t *solution,
                     double *lambda, int32_t *path, int mem)
{
    return verify_nodes_any(ctx, mem == QPN_MEM_DEVICE, batch, n, m, p, Qd, R, qd, Ad, B, l, u, xd, w, stride_w, tol, solution,
                            lambda, path, mem);
}

int qpn_verify_nodes_h(qpn_ctx *ctx, qpn_nodes *h, const double *xd, const double *w, int64_t stride_w,
                       double tol, int32_t *solution, double *lambda, int32_t *path, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (!h) return fail_arg(ctx, "qpn_verify_nodes_h: null handle");
    if (h->device != ctx->device) return fail_arg(ctx, "qpn_verify_nodes_h: handle belongs to another device");
    return verify_nodes_any(ctx, true, h->batch, h->n, h->m, h->p, h->f[0], h->f[1], h->f[2], h->f[3], h->f[4], h->f[5],
                            h->f[6], xd, w, stride_w, tol, solution, lambda, path, mem);
}

int qpn_verify_nodes_subset_h(qpn_ctx *ctx, qpn_nodes *h, int32_t count, const int32_t *idx, const double *xd, const double *w,
                              int64_t stride_w, double tol, int32_t *solution, double *lambda, int32_t *path, int mem)
{
    const char *who = "qpn_verify_nodes_subset_h";
    if (!ctx) return QPN_ERR_ARG;
    if (!h) return fail_arg(ctx, who, "null handle");
    if (h->device != ctx->device) return fail_arg(ctx, who, "handle belongs to another device");
    if (count < 0) return fail_arg(ctx, who, "count < 0");
    if (count == 0) return QPN_OK;
    if (!idx) return fail_arg(ctx, who, "null pointer");
    return verify_nodes_any(ctx, true, h->batch, h->n, h->m, h->p, h->f[0], h->f[1], h->f[2], h->f[3], h->f[4], h->f[5],
                            h->f[6], xd, w, stride_w, tol, solution, lambda, path, mem, who, count, idx);
}

// ---- schedule hints of the context ----------------------------------------------------------------------------
int qpn_order_nodes_by_pivots(qpn_ctx *ctx, const int32_t *pivots, int32_t count, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (!pivots || count <= 0) return fail_arg(ctx, "qpn_order_nodes_by_pivots: bad arguments");
    Stage st(ctx, mem, "qpn_order_nodes_by_pivots");
    if (int rc = st.check()) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = order_reserve(ctx, count);
    if (rc != QPN_OK) return rc;
    const int32_t *dp;
    st.in(dp, pivots, (size_t)count * 4);
    if ((rc = st.begin()) != QPN_OK) return rc;
    HIPCHK(ctx, qpn_launch_order_by_pivots(dp, count, ctx->order, ctx->stream));
    if ((rc = st.finish()) != QPN_OK) return rc;
    ctx->order_count = count;
    ctx->order_user = true;
    return QPN_OK;
}

int qpn_set_node_order(qpn_ctx *ctx, const int32_t *order, int32_t count, int mem)
{
    if (!ctx) return QPN_ERR_ARG;
    if (!order) { ctx->order_count = 0; ctx->order_user = false; ctx->auto_calls = 0; return QPN_OK; }
    if (count <= 0) return fail_arg(ctx, "qpn_set_node_order: bad count");
    if (mem != QPN_MEM_HOST && mem != QPN_MEM_DEVICE) return fail_arg(ctx, "qpn_set_node_order: bad mem kind");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = order_reserve(ctx, count);
    if (rc != QPN_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->order, order, (size_t)count * 4,
                               mem == QPN_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ctx->stream));
    if (mem == QPN_MEM_HOST) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->order_count = count;
    ctx->order_user = true;
    return QPN_OK;
}

int qpn_ctx_set_auto_schedule(qpn_ctx *ctx, int32_t period)
{
    if (!ctx) return QPN_ERR_ARG;
    if (period < 0) return fail_arg(ctx, "qpn_ctx_set_auto_schedule: negative period");
    ctx->auto_period = period;
    ctx->auto_calls = 0;
    if (period == 0 && !ctx->order_user) ctx->order_count = 0;      // drop a hint this mechanism installed
    return QPN_OK;
}

} // extern "C"
