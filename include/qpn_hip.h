/*
 * qpn_hip.h -- C-ABI of the MI355X-native QPNet node-AVI engine (libqpn_hip.so).
 *
 * Drop-in boundary for the hot path of forrestlaine/QuadraticProgramNetworks.jl v0.4.0
 * (paths below are relative to the reference tree).  Every entry point is `extern "C"`,
 * takes plain pointers and sizes, returns an int error code (0 = ok, <0 = API misuse or HIP
 * error; per-item solver outcomes are ONLY reported in status[]), never throws, never
 * keeps a caller pointer past return, and keeps no global state (one qpn_ctx per
 * thread/stream is safe).  All matrices are dense COLUMN-MAJOR fp64 (Julia's layout);
 * +-Inf bounds are literal IEEE infinities (src/avi.jl:125-126).
 *
 * `mem` says where the caller's buffers live: QPN_MEM_HOST (the library stages them
 * through HBM itself -- what the Julia `ccall` shim uses) or QPN_MEM_DEVICE (pointers are
 * already in HBM on the ctx's device; the call is asynchronous on the ctx stream).
 */
#ifndef QPN_HIP_H
#define QPN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QPN_ABI_VERSION 1

/* per-item status: the reference enum StatusCode, src/avi.jl:1-6 */
enum { QPN_SUCCESS = 1, QPN_RAY_TERM = 2, QPN_MAX_ITERS = 3, QPN_FAILURE = 4 };

/* API error codes (function return values) */
enum {
    QPN_OK = 0,
    QPN_ERR_ARG = -1,      /* bad argument (null pointer, size out of range)  */
    QPN_ERR_HIP = -2,      /* a HIP runtime call failed; see qpn_ctx_last_error */
    QPN_ERR_NODEVICE = -3, /* no gfx950 device visible                        */
    QPN_ERR_SIZE = -4      /* problem size not supported by any kernel        */
};

enum { QPN_MEM_HOST = 0, QPN_MEM_DEVICE = 1 };

/* row kinds of the mixed complementarity problem solved per item
 *   QPN_ROW_STD : (Mz+q)_i  _|_  l_i <= z_i <= u_i       AVI row,  src/avi.jl:56-61
 *   QPN_ROW_GAVI:  z_i      _|_  l_i <= (Mz+q)_i <= u_i  second GAVI condition, src/avi.jl:22-24
 * A batch with kind == NULL is a plain box-MCP: exactly PATHSolver.solve_mcp's problem. */
enum { QPN_ROW_STD = 0, QPN_ROW_GAVI = 1 };

typedef struct qpn_ctx qpn_ctx;

/* qpn_avi_opts.flags */
#define QPN_AVI_FLAG_COLD_START 1 /* ignore the z input: every item starts from z0 = 0 (no reset pass) */
/* Warm start of a node solve from the active set of an earlier sweep.  Honoured by qpn_solve_nodes, qpn_solve_nodes_into and
 * qpn_solve_nodes_h when n, m <= 32, z != NULL and QPN_AVI_FLAG_COLD_START is not set; in every other size class and on every
 * other entry point the bit is ignored and the solve is cold.  The multiplier part of the incoming z names the hint: row i is
 * taken to sit at l_i where lambda_i > 0, at u_i where lambda_i < 0, and to be inactive otherwise (z of the previous sweep
 * over the same nodes is such a hint; its primal part is not read).  Per node, the linear KKT system of the hinted rows is
 * solved in fp64 and the point takes the post-check, residual and active-set classification of the cold solve.  The node is
 * ACCEPTED only if every hinted row has a finite bound on its side, there are at most n hinted rows, no pivot of the
 * factorisations falls under piv_tol, every hinted multiplier comes out with its side's sign and the post-check passes: it
 * then returns status = QPN_SUCCESS, pivots = 0, and z, resid, active and the x scatter of that point (equal to the cold
 * solve's up to rounding).  Every other node -- a NaN or an infinity in its hint, an empty hint on a node with active rows, a
 * wrong row or side -- is solved by the cold route in the same call, with results bit-identical to a call without the bit.
 * Accepted nodes do not feed a handle's pivot statistics, its schedule or its count of declined nodes, and a sweep with the
 * bit set does not fill the crash cache (it reuses a valid one).
 * One more class takes the hint once its context opts in: resident records of large nodes (64 < n <= 256, m <= 256) on the
 * symmetric route, through qpn_solve_nodes_h with QPN_OPT_WARM_BIG = 1 (see there: the hint seeds block principal pivoting,
 * pivots = n when it held).  Without that option the bit is ignored there as everywhere else.
 * The mid-size classes (n, m <= 128, one of them > 32) take the hint per resident handle: after qpn_nodes_set_warm(ctx, nodes, 1)
 * a qpn_solve_nodes_h sweep with the bit (z != NULL, QPN_AVI_FLAG_COLD_START clear) that the fused mid-size kernels serve
 * (QPN_OPT_MID_ROUTE = 1, no pivot budget that closes them) runs the same warm solve, one workgroup per node, with the same accept
 * rule and outputs (pivots = 0) and one more condition: the k hinted rows have to fit the kernel's LDS,
 * 8 (k (n | 1) + n ((k + 1) | 1)) + 15 648 <= 163 840 bytes -- every k <= min(n, 64) in every shape, every k <= 71 at n = 128.
 * A node outside it is solved cold like every other decliner.  Handles that have not opted in, and the per-call entry points,
 * ignore the bit in these classes. */
#define QPN_AVI_FLAG_WARM_DUALS 2

typedef struct {
    double check_tol;  /* post-check tolerance, 1e-6       (src/avi.jl:148)                 */
    double piv_tol;    /* smallest admissible pivot, 1e-11                                   */
    double feas_tol;   /* basic infeasibility treated as zero, 1e-12                         */
    double comp_tol;   /* active-set classification tolerance, 1e-2 (src/avi_solutions.jl:511); finite */
    int32_t max_pivots; /* <= 0: 50*N + 100 (cf. PATH limits at src/avi.jl:67-70)             */
    int32_t flags;      /* QPN_AVI_FLAG_* (0 by default)                                        */
} qpn_avi_opts;

/* ---- context ------------------------------------------------------------------- */
int qpn_abi_version(void);
int qpn_ctx_create(int device_id, qpn_ctx **out);
int qpn_ctx_destroy(qpn_ctx *ctx);
/* Launch on an existing hipStream_t (e.g. torch's current stream).  NULL is HIP's legacy default
 * (null) stream, NOT "no stream".  A new ctx launches on a private non-blocking stream;
 * qpn_ctx_use_own_stream returns to it. */
int qpn_ctx_set_stream(qpn_ctx *ctx, void *hip_stream);
int qpn_ctx_use_own_stream(qpn_ctx *ctx);
int qpn_ctx_synchronize(qpn_ctx *ctx);
const char *qpn_ctx_last_error(qpn_ctx *ctx);
const char *qpn_strerror(int code);
void qpn_avi_default_opts(qpn_avi_opts *opts);

/* ---- (A2+A3+A9) batched AVI solve ------------------------------------------------
 * Replaces PATHSolver.solve_mcp as called at src/avi.jl:64-70 and src/qp_processing.jl:22-27,
 * including the post-check of src/avi.jl:71-76 (check_avi_solution, :148-156) and the
 * active-set classification of src/avi_solutions.jl:511-562 / :587-612.
 *   M       [batch][N*N] column-major, item stride strideM doubles (0: one M shared by all items)
 *   q,l,u   [batch][N]
 *   kind    [batch][N] uint8 row kinds, item stride stride_kind (0: shared), or NULL (all STD)
 *   z       [batch][N] in: z0 (warm start of the bounded STD variables; duals start cold as
 *                       src/avi.jl:404)   out: solution
 *   status  [batch] int32 (QPN_SUCCESS..QPN_FAILURE), resid [batch] natural-map residual,
 *   pivots  [batch] int32, active [batch][N] uint8: bit (c-1) set for code c of
 *           src/avi_solutions.jl:511-562 on STD rows, bit (c+3) on GAVI rows (codes 5..8).
 *   Any of resid/pivots/active may be NULL.  N <= 1024 in ABI version 1 (N <= 64: one wavefront per item; larger: one workgroup). */
int qpn_solve_avi_batch(qpn_ctx *ctx, int32_t batch, int32_t N, const double *M, int64_t strideM,
                        const double *q, const double *l, const double *u, const uint8_t *kind,
                        int64_t stride_kind, double *z, int32_t *status, double *resid,
                        int32_t *pivots, uint8_t *active, const qpn_avi_opts *opts, int mem);

/* One problem in Julia's own SparseMatrixCSC{Float64,Int32} layout (1-based colptr/rowval):
 * the exact argument list of PATHSolver.solve_mcp(M, q, l, u, z0) at src/avi.jl:64.
 * Host pointers only.  z: in z0, out solution. */
int qpn_solve_mcp_csc(qpn_ctx *ctx, int32_t N, const int32_t *colptr, const int32_t *rowval,
                      const double *nzval, const double *q, const double *l, const double *u,
                      double *z, int32_t *status, double *resid, int32_t *pivots,
                      const qpn_avi_opts *opts);

/* ---- (A3) batched check_avi_solution, src/avi.jl:148-156 --------------------------
 *   degree [batch] int32 violation count (sol_bad = degree > 0), r [batch][N] = Mz+q (may be NULL) */
int qpn_check_avi_batch(qpn_ctx *ctx, int32_t batch, int32_t N, const double *M, int64_t strideM,
                        const double *q, const double *l, const double *u, const uint8_t *kind,
                        int64_t stride_kind, const double *z, double tol, int32_t *degree,
                        double *r, int mem);

/* ---- (A9) comp_indices core, src/avi_solutions.jl:511-562 --------------------------
 * Flat arrays of `count` rows; mask bit (c-1+shift) for code c in 1..4 (shift = 4 for the
 * s2 block of the GAVI wrapper, :587-612). */
int qpn_comp_indices(qpn_ctx *ctx, int64_t count, const double *zv, const double *rv,
                     const double *l, const double *u, double tol, int32_t shift, uint8_t *mask,
                     int mem);

/* ---- (A5+A6) per-node KKT assembly, single-node pools, reduced form -----------------
 * src/avi.jl:205-251 + :305-377 restated densely without the dead xi block and the slack
 * block: per node i with n decision variables, m constraint rows,
 * p parameters,
 *     M_i = [[Qd_i, -Ad_i'],[Ad_i, 0]]   (N = n+m),   q_i = [qd_i + R_i w ; B_i w],
 *     l/u = [-Inf/+Inf x n ; l_i ; u_i],  kind = [STD x n ; GAVI x m].
 *   Qd [batch][n*n], R [batch][n*p], qd [batch][n], Ad [batch][m*n], B [batch][m*p],
 *   l,u [batch][m], w [batch][p] with item stride stride_w (0: one shared parameter vector). */
int qpn_assemble_nodes(qpn_ctx *ctx, int32_t batch, int32_t n, int32_t m, int32_t p,
                       const double *Qd, const double *R, const double *qd, const double *Ad,
                       const double *B, const double *l, const double *u, const double *w,
                       int64_t stride_w, double *Mout, double *qout, double *lout, double *uout,
                       uint8_t *kind_out, int mem);

/* ---- (A6) pool assembly: combine_gavis, src/avi.jl:305-377 (and convert, :113-128) -------------------------------
 * One AVI per Nash pool (all nodes of a level jointly, src/avi.jl:399-400), `batch` instances of ONE pool shape
 * (config 3: 1 000 payoff draws of the four-player game; a level of a net: batch = 1).  The shape (host arrays, read
 * during the call only): `players` nodes in pool order (sorted ids, :319), player i with n_i decision variables and m_i
 * constraint rows; the pool's decision variables are the union (nd positions = dec_inds, sorted), the other variables
 * of the net are the p parameters; dpos (concatenated over the players, sum n_i entries) = position in dec_inds of each
 * of a player's decision variables.
 * Numeric inputs, the players' blocks stacked in pool order, column-major, sn = sum n_i, sm = sum m_i:
 *   Qd [sn x nd] = Q_i[dvars_i, dec_inds]     Qp [sn x p] = Q_i[dvars_i, param_inds]     qd [sn] = q_i[dvars_i]
 *   Ad [sm x nd] = M2_i[:, dec_inds]          Bp [sm x p] = M2_i[:, param_inds]          l, u [sm]
 *   w [p] parameters.  Every input has an item stride in doubles; 0 shares it across the batch.
 * Output: M [N x N] column-major (item stride strideM; 0 = ONE shared M, allowed when Qd and Ad are shared), q, l, u,
 * kind [batch][N], ready for qpn_solve_avi_batch.
 *   QPN_POOL_REFERENCE  z = [dec | xi_i per player | lambda-psi_i per player | slack], N = nd + sn + 2 sm: the AVI the
 *                       reference hands to PATH, rows [sum_i xi^i_d = 0 (:356-367) | player KKT rows (:335-340) |
 *                       [A -I] | [0 I 0] (:113-128)], all STD
 *   QPN_POOL_REDUCED    z = [dec | lambda-psi], N = nd + sm, kinds [STD x nd | GAVI x sm]: without the xi block (it is
 *                       multiplied by 0, :244) and the slack block; needs disjoint decision sets (sn = nd)
 * qpn_pool_size returns N for a shape and form. */
typedef struct {
    int32_t players, nd, p;
    const int32_t *n_i, *m_i; /* [players] */
    const int32_t *dpos;      /* [sum n_i] */
} qpn_pool_shape;
enum { QPN_POOL_REDUCED = 0, QPN_POOL_REFERENCE = 1 };
int qpn_pool_size(const qpn_pool_shape *shape, int form, int32_t *N);
int qpn_assemble_pools(qpn_ctx *ctx, const qpn_pool_shape *shape, int form, int32_t batch, const double *Qd,
                       int64_t stride_Qd, const double *Qp, int64_t stride_Qp, const double *qd, int64_t stride_qd,
                       const double *Ad, int64_t stride_Ad, const double *Bp, int64_t stride_Bp, const double *l,
                       const double *u, int64_t stride_lu, const double *w, int64_t stride_w, double *Mout,
                       int64_t strideM, double *qout, double *lout, double *uout, uint8_t *kind_out, int mem);

/* ---- (A5+A6+A2+A3+A9) fused: assemble each node's KKT blocks on the fly and solve ----------
 * Same inputs as qpn_assemble_nodes, same outputs as qpn_solve_avi_batch (N = n+m, z = [x_d; lambda]);
 * identical results to calling the two in sequence, without materialising M in HBM: one pass of the
 * hot path per outer sweep (src/algorithm.jl:95 -> solve_qep -> src/avi.jl:399-409 for single-node
 * pools).  z: in z0 (ignored with QPN_AVI_FLAG_COLD_START; with QPN_AVI_FLAG_WARM_DUALS its multipliers are the hint of the
 * warm start, see there), out solution.  n, m <= 32 run on the fused
 * matrix-core kernel (one wavefront per node); n, m <= 64 on the four-wavefronts-per-node path (crash on the
 * matrix cores straight from the records, cold duals); larger nodes (n+m <= 1024) are assembled and take the
 * blocked matrix-core path for large node-shaped items (n, m <= 512) or the general kernels. */
int qpn_solve_nodes(qpn_ctx *ctx, int32_t batch, int32_t n, int32_t m, int32_t p, const double *Qd,
                    const double *R, const double *qd, const double *Ad, const double *B,
                    const double *l, const double *u, const double *w, int64_t stride_w, double *z,
                    int32_t *status, double *resid, int32_t *pivots, uint8_t *active,
                    const qpn_avi_opts *opts, int mem);

/* Same, and additionally scatters every node's primal block x_d = z[0..n) into the caller's iterate:
 *   x[b * stride_x + i] = z[b][i], i < n   (stride_x >= n, in doubles; x in the same memory space as z).
 * This is the write-back the outer sweep does after each solve (src/algorithm.jl:97-101,
 * x[decision_inds] = x_opt[decision_inds]); doing it from the solve kernel spares two copy kernels per
 * sweep.  x == NULL behaves exactly like qpn_solve_nodes. */
int qpn_solve_nodes_into(qpn_ctx *ctx, int32_t batch, int32_t n, int32_t m, int32_t p, const double *Qd,
                         const double *R, const double *qd, const double *Ad, const double *B,
                         const double *l, const double *u, const double *w, int64_t stride_w, double *z,
                         int32_t *status, double *resid, int32_t *pivots, uint8_t *active,
                         const qpn_avi_opts *opts, int mem, double *x, int64_t stride_x);

/* ---- resident node records: upload once, sweep many times ----------------------------------------------
 * The outer loop (src/algorithm.jl:13-117) sweeps the SAME nodes again and again: between two sweeps only the
 * parameters w (the other players' decision variables) change, while Qd, R, qd, Ad, B, l, u -- 22 KB per
 * n = m = 32 node -- stay what they were.  A caller with host arrays (the Julia shim) that went through
 * qpn_solve_nodes every sweep would move those records over PCIe every time (2.3 M solves/s against 85 M/s
 * from resident records).  qpn_nodes_upload copies the records into HBM owned by the
 * library ONCE and returns a handle; qpn_solve_nodes_h / qpn_verify_nodes_h then take the handle, w and the
 * output buffers, exactly as qpn_solve_nodes_into / qpn_verify_nodes would with the records in place.
 *   mem (upload)    where Qd..u live (QPN_MEM_HOST / QPN_MEM_DEVICE); the handle holds its own copy either way,
 *                   so the records cannot change under it
 *   mem (solve)     where w, z0/z, status, resid, pivots, active, x live.  With QPN_MEM_HOST only w goes up and
 *                   only the requested outputs come down; z may be NULL when only the primal blocks (x) or only
 *                   the statuses are wanted.
 * The handle also keeps what depends on the records alone: whether any of its nodes needs the general
 * (pivoting) kernel -- decided by Qd, Ad, l, u, never by w -- so that sweeps over well-conditioned nodes are ONE
 * launch, and the longest-first schedule of its nodes (from exponentially smoothed pivot counts, which every sweep's
 * solve kernel updates; the order is re-sorted from them every `period` sweeps at first and every 4 x `period` once
 * settled; qpn_nodes_set_schedule, period 0 = natural order).
 * qpn_nodes_update replaces one array of the records (e.g. the bounds after a new child piece was chosen).
 * qpn_nodes_set_warm(on = 1) lets the sweeps over a handle of the mid-size classes (n, m <= 128, one of them > 32) honour
 * QPN_AVI_FLAG_WARM_DUALS (see there); on = 0, the default, makes them cold again.  Any other value of `on` is QPN_ERR_ARG.  On a
 * handle of another shape the call succeeds and changes nothing: n, m <= 32 honour the flag anyway, and beyond 128
 * QPN_OPT_WARM_BIG is the switch.
 * Symmetric n = m = 32 records also keep the part of the solve that Qd and Ad alone decide (QPN_OPT_CRASH_CACHE): the first
 * sweep stores it, the later ones reuse it, with bit-identical results.  Cost in HBM: the records are 22 KB per n = m = 32
 * node, the crash cache adds 22 KB per node (symmetric records; the general variants -- 24 KB -- are not cached).  It is allocated
 * by the first sweep that would use it; when that memory cannot be had the handle runs uncached.  qpn_nodes_update of
 * QPN_NODE_QD or QPN_NODE_AD (and a change of QPN_OPT_SYM_ROUTE) drops it, the next sweep fills it again; updates of R, qd, B,
 * l, u keep it.
 * Large records (64 < n <= 256, m <= 256: the blocked crash) have a cache of their own, off by default
 * (QPN_OPT_CRASH_CACHE_BIG): the eliminated top half at the node's own size with the multipliers of every pass in its dead
 * tiles, and S -- 8 (pad16(n) (pad16(n) + pad16(m) + 16) + m pad16(m + 1) + 2) + 1 bytes per node, 1 638 417 at n = m = 256
 * (the records are 1.06 MB), 839 MB for 512 such nodes.  Same life cycle: allocated by the first sweep that would use it, the
 * handle runs uncached when it cannot be had; an update of QPN_NODE_QD or QPN_NODE_AD drops it, R, qd, B, l, u keep it. */
typedef struct qpn_nodes qpn_nodes;
enum { QPN_NODE_QD = 0, QPN_NODE_R = 1, QPN_NODE_Q = 2, QPN_NODE_AD = 3, QPN_NODE_B = 4, QPN_NODE_L = 5, QPN_NODE_U = 6 };
int qpn_nodes_upload(qpn_ctx *ctx, int32_t batch, int32_t n, int32_t m, int32_t p, const double *Qd,
                     const double *R, const double *qd, const double *Ad, const double *B, const double *l,
                     const double *u, int mem, qpn_nodes **out);
int qpn_nodes_update(qpn_ctx *ctx, qpn_nodes *nodes, int32_t field, const double *data, int mem);
int qpn_nodes_set_schedule(qpn_ctx *ctx, qpn_nodes *nodes, int32_t period);
int qpn_nodes_set_warm(qpn_ctx *ctx, qpn_nodes *nodes, int32_t on);
int qpn_nodes_free(qpn_ctx *ctx, qpn_nodes *nodes);
/* info[0] = what is known about the general kernel's share of these records: 0 nothing yet, 1 the count of the first
 * sweep is on its way to the host, 2 no node needs it (sweeps are one launch), 3 some do; info[1] = that count (valid
 * in states 2, 3); info[2] = bit 0: a longest-first schedule is installed, bit 1: every Qd block of the records is bitwise
 * symmetric (settled by one pass when the records arrive or Qd is replaced; QPN_OPT_SYM_ROUTE), bit 2: a valid crash cache is
 * installed, bit 3: the crash cache is refused (QPN_OPT_CRASH_CACHE = 0, records of a shape or route that is not cached, or its
 * memory could not be had), bit 4: the last sweep streamed the crash cache past the last-level cache (QPN_OPT_LLC_BUDGET_MB),
 * bit 5: a valid crash cache of the large class is installed (QPN_OPT_CRASH_CACHE_BIG), bit 6: that cache is refused (the option
 * is 0, records of a shape or route that is not the blocked crash of large nodes, or its memory could not be had);
 * info[3] = sweeps since the last schedule reset. */
int qpn_nodes_info(qpn_ctx *ctx, qpn_nodes *nodes, int32_t info[4]);
int qpn_solve_nodes_h(qpn_ctx *ctx, qpn_nodes *nodes, const double *w, int64_t stride_w, double *z,
                      int32_t *status, double *resid, int32_t *pivots, uint8_t *active,
                      const qpn_avi_opts *opts, int mem, double *x, int64_t stride_x);
/* A sweep over a chosen part of a handle's nodes.  The arguments are those of qpn_solve_nodes_h with every per-item array
 * compact: slot s (0 <= s < count) belongs to node idx[s].  w is [count][p] with item stride stride_w (0 = one shared vector),
 * z and active are [count][n + m], status, resid and pivots [count], x[s * stride_x + i] receives the primal block of node
 * idx[s]; idx lives where mem says; z, resid, pivots, active and x may be NULL as in qpn_solve_nodes_h.
 * Contract: let w_full[idx[s]] = w[s], the other rows arbitrary but finite (and z_full likewise when the call carries a hint).
 * Slot s of every output -- z, status, resid, pivots, active, x -- then equals the output of node idx[s] in
 * qpn_solve_nodes_h(nodes, w_full, ...) under the same options and context options, bit for bit; where that sweep is specified
 * up to rounding (the seeded block principal pivoting of QPN_OPT_WARM_BIG), so is this call.  QPN_AVI_FLAG_WARM_DUALS (the
 * warm kernel runs over the list, its decliners go cold in the same call), QPN_AVI_FLAG_COLD_START, max_pivots and nodes
 * that the fused kernel hands to the general one are all covered.
 * The list: count == 0 succeeds and touches nothing; count < 0 or count > batch is QPN_ERR_ARG.  Entries lie in [0, batch) and
 * are pairwise distinct, in any order.  A host list is checked before anything is launched (QPN_ERR_ARG, no output written).
 * A device list is checked on the device, and nothing waits for the answer on the host: a slot whose entry is out of range
 * answers status = QPN_FAILURE and zeros elsewhere; of the slots that name one node, the first to claim it is solved and
 * every other one answers the same way.  The other slots are unaffected.
 * On the fused routes (n, m <= 128 under the default options) only the listed nodes are solved.  The call uses what the handle
 * knows -- its count of declined nodes (state 2: no general launch, no workspace), a valid crash cache, mixed launches and the
 * LLC streaming policy -- and changes none of it: it fills no crash cache, takes no census, feeds no pivot statistics, does
 * not advance info[3] and installs or refreshes no schedule; the handle's order and a caller-installed context order are
 * ignored and stay in place; qpn_nodes_info reads the same before and after.  The launch still covers `batch` positions,
 * those without a node ending at once; the primal mirrors of qpn_set_primal_mirrors are not written.
 * On the other routes (large records on the blocked crash, the general route) there is NO saving: the call runs one ordinary
 * full sweep -- rows of w_full that no subset call has written are zero, later calls keep the last values -- and returns the
 * listed rows; the handle's state moves exactly as that sweep moves it.
 * The handle owns the full-size device buffers this takes (w, z, status, resid, pivots, active and 2 batch + 1 int32),
 * allocated by the first subset call and freed with the handle; when they cannot be had the call fails with QPN_ERR_HIP and
 * the handle stays usable. */
int qpn_solve_nodes_subset_h(qpn_ctx *ctx, qpn_nodes *nodes, int32_t count, const int32_t *idx, const double *w,
                             int64_t stride_w, double *z, int32_t *status, double *resid, int32_t *pivots,
                             uint8_t *active, const qpn_avi_opts *opts, int mem, double *x, int64_t stride_x);
int qpn_verify_nodes_h(qpn_ctx *ctx, qpn_nodes *nodes, const double *xd, const double *w, int64_t stride_w,
                       double tol, int32_t *solution, double *lambda, int32_t *path, int mem);
/* The accept gate over a chosen part of a handle's nodes.  The arguments are those of qpn_verify_nodes_h with every per-item
 * array compact: slot s (0 <= s < count) belongs to node idx[s].  xd is [count][n], w [count][p] with item stride stride_w
 * (0 = one shared vector), solution and path [count], lambda [count][m]; idx lives where mem says.
 * Contract: slot s of solution, path and every word of the lambda row equals, bit for bit, what qpn_verify_nodes_h returns for
 * node idx[s] when that node is given the same xd and w rows and the same tol.  One exception, which the full call has already:
 * in the 33 .. 64 class, when more nodes of a call than its workspace has slots (256) have more than 32 active rows, which of
 * them the workgroup kernel takes depends on the order in which workgroups start; flags and paths are equal then, the
 * multipliers equal up to the kernel that took the node.
 * The list: entries lie in [0, batch), in any order, and need NOT be distinct -- every slot owns its outputs and scratch and the
 * records are only read, so one node may be put to several points in one call; count may exceed batch.  count == 0 succeeds and
 * touches nothing; count < 0 is QPN_ERR_ARG.  A host list is checked before anything is staged or launched (a bad entry:
 * QPN_ERR_ARG, no output written).  A device list is checked in the kernels, and nothing waits for the answer on the host: a
 * slot whose entry is out of range reads no record and answers solution = 0, path = 6 ("no such node") and a zero lambda row;
 * the other slots are unaffected.
 * The launches cover `count` blocks and all scratch is sized by count: the cost follows the list, not the handle.  The handle's
 * state does not move. */
int qpn_verify_nodes_subset_h(qpn_ctx *ctx, qpn_nodes *nodes, int32_t count, const int32_t *idx,
                              const double *xd, const double *w, int64_t stride_w, double tol,
                              int32_t *solution, double *lambda, int32_t *path, int mem);

/* ---- schedule hint for qpn_solve_nodes[_into]: longest solves first ---------------------------------
 * The outer loop (src/algorithm.jl:13-117) sweeps the SAME nodes again and again, and a node's pivot
 * count changes little between sweeps, while a launch ends with a tail in which the last, longest
 * solves run on a nearly empty GPU.  qpn_order_nodes_by_pivots builds, on the device, a permutation of
 * 0..count-1 by DESCENDING pivot count (`pivots` = the output of an earlier sweep over the same nodes)
 * and installs it in the context; later qpn_solve_nodes[_into] calls with batch == count hand node
 * order[i] to the i-th wavefront.  Inputs, outputs and their layout do not change -- only which
 * wavefront solves which node (results are independent of it, bit for bit).  qpn_set_node_order installs
 * a caller-made permutation (entries outside 0..count-1 leave their slot unsolved) or, with order ==
 * NULL, clears the hint.  The hint is ignored whenever batch != count. */
int qpn_order_nodes_by_pivots(qpn_ctx *ctx, const int32_t *pivots, int32_t count, int mem);
int qpn_set_node_order(qpn_ctx *ctx, const int32_t *order, int32_t count, int mem);
/* By default the context does this by itself: a qpn_solve_nodes[_into] call that fills the GPU (batch > 4096, n, m <= 32)
 * and returns pivot counts refreshes the hint from them every `period`-th call of the same batch size (default 16; the
 * first call of a batch size installs it), one 8 us launch behind the solve.  A hint installed through the two
 * functions above takes precedence until qpn_set_node_order(ctx, NULL, ...) clears it; period = 0 switches the
 * mechanism off.  Results never depend on any of this. */
int qpn_ctx_set_auto_schedule(qpn_ctx *ctx, int32_t period);

/* Per-context options that select between kernel routes with IDENTICAL contracts (A/B measurements, tests of a route
 * against the one it replaced).  Results never depend on them beyond rounding.
 *   QPN_OPT_MID_ROUTE  node records with n, m <= 128 and one of them > 32 (qpn_solve_nodes*): 1 = one fused kernel per node
 *                      (default: ONE wavefront per node for max(n, m) <= 48, one workgroup per node beyond), 0 = the general
 *                      route (assembled blocks -> the route of large nodes / the general kernels): the cross-check of the tests.
 *                      (Round 3's values 2 and 3 -- round 2's three-kernel route, the workgroup kernel for 33 .. 48 -- are gone;
 *                      the library reads no environment variable.)
 *   QPN_OPT_BIG_ROUTE  kept for callers that set the default: takes 1 only (the blocked matrix-core crash straight from the
 *                      records, BASELINE config 5); round 2's route over an assembled M is gone as a node-record switch -- the
 *                      same kernels serve large node-shaped items passed as M through qpn_solve_avi_batch.
 *   QPN_OPT_SYM_ROUTE  resident records (qpn_nodes_upload) whose Qd blocks are ALL bitwise symmetric: 1 = kernel variants that
 *                      use the symmetry of H and of S = A H^-1 A' (default; n = m = 32: 8 of 88 fp64 MFMAs per solve less; large
 *                      nodes, 64 < n <= 256 and m <= 256: the complementarity phase runs as block principal pivoting on the
 *                      symmetric Schur problem, the Lemke kernel behind it for what it leaves -- `pivots` then reports n + the
 *                      number of complementarity pairs switched; with a caller-set max_pivots the Lemke kernel, whose pivots
 *                      that budget counts, runs alone), 0 = the general variants.  Records with any asymmetric Qd, and records
 *                      passed per call, always take the general variants.
 *   QPN_OPT_CRASH_CACHE resident symmetric n = m = 32 records on the symmetric route: 1 = the first sweep over a handle stores
 *                      what the crash makes of Qd and Ad alone (panels, W~ = -H^-1 C, S = A H^-1 A', pivot-test verdicts; 22 KB
 *                      per node) and later sweeps reuse it instead of recomputing it (default), 0 = never.  The cached sweeps
 *                      perform the parameter-dependent operations in the same order on the same numbers: results are
 *                      bit-identical either way, and the same nodes decline.
 *   QPN_OPT_LLC_BUDGET_MB sweeps that reuse the crash cache: the share of the GPU's last-level cache, in MiB, that a sweep counts on
 *                      (default: a tuning constant of the build).  A sweep whose node records and outputs fit
 *                      that budget while records + crash cache do not fetches the crash cache with non-temporal loads, so that the
 *                      records stay in the cache from sweep to sweep; smaller and larger sweeps use the default policy throughout.
 *                      0 = never, -1 = every sweep that reuses the crash cache (tests, A/B runs).  A policy of the loads only:
 *                      results are bit-identical.
 *   QPN_OPT_CRASH_CACHE_BIG resident records on the blocked crash of large nodes (64 < n <= 256, m <= 256, any Qd): 1 = the first
 *                      sweep over a handle keeps what the elimination makes of Qd and Ad alone (the multipliers of every rank-64
 *                      pass, W = -H^-1 C, S = -Ad W, the smallest pivot, max |M| over H and C; 1.6 MB per node at n = m = 256) and
 *                      later sweeps replay only the column that moves with w; 0 = never (default).  The pivot threshold
 *                      1e-4 max(1, max |M|) takes in g = qd + R w: a cached sweep forms the same maximum from this sweep's g and
 *                      declines exactly the nodes whose smallest cached pivot lies below it.  A node whose elimination stops in a
 *                      filling sweep has no entry and is recomputed by every sweep until it gets through.  Results are
 *                      bit-identical either way, and the same nodes decline.  Records passed per call are never cached.
 *   QPN_OPT_WARM_BIG   resident records of large nodes (64 < n <= 256, m <= 256) on the symmetric route: 1 = a sweep that carries
 *                      QPN_AVI_FLAG_WARM_DUALS (z given, QPN_AVI_FLAG_COLD_START clear, no caller-set max_pivots) starts block
 *                      principal pivoting from the set the multipliers of the incoming z name -- row i at l_i when lambda_i > 0
 *                      and l_i is finite, at u_i when lambda_i < 0 and u_i is finite, free otherwise (NaN and zeros name nothing;
 *                      the primal part is not read); 0 = the flag is ignored in this class as in every other but n, m <= 32
 *                      (default).  A node whose hint names no row or more than 112 rows starts cold, bit for bit; a seeded
 *                      start that fails is repeated from the cold start in the same launch, so a wrong hint costs rounds, never
 *                      the result.  `pivots` = n + the pairs switched after the seed: pivots == n says that the hint held.
 *                      Results equal the un-hinted ones up to rounding (the same post-check certifies them), not bit for bit.
 *                      The same nodes decline and the crash caches are filled and reused as without it: no new route epoch.
 * A resident handle remembers under which option values it learned that none of its nodes declines; after a change it asks again
 * on its next sweep (another kernel variant applies its pivot test to slightly different numbers). */
#define QPN_OPT_MID_ROUTE 1
#define QPN_OPT_BIG_ROUTE 2
#define QPN_OPT_SYM_ROUTE 3
#define QPN_OPT_CRASH_CACHE 4
#define QPN_OPT_LLC_BUDGET_MB 5
#define QPN_OPT_CRASH_CACHE_BIG 6
#define QPN_OPT_WARM_BIG 7
int qpn_ctx_set_option(qpn_ctx *ctx, int32_t option, int32_t value);

/* ---- multi-GPU: replicas of the iterate on peer GPUs, written by the solve itself -----------------------
 * One process per GPU; rank g solves its own node range and every rank needs the whole iterate x for the
 * next sweep (src/algorithm.jl:95-101 reads x_opt of all children).  Instead of a collective after the solve,
 * the solve kernel stores each primal block to the local iterate AND to the same offset of the peers'
 * iterates: xGMI is point-to-point, the blocks are 8n bytes, and the stores ride along with the launch.
 *   qpn_shared_alloc   zeroed device buffer on ctx's GPU + its 64-byte IPC handle, to be sent to the peers by any
 *                      host channel (torch.distributed all_gather_object, MPI, a pipe, ...)
 *   qpn_shared_open    map a peer's buffer into this process (hipIpcOpenMemHandle); qpn_shared_close unmaps
 *   qpn_shared_free    release a buffer from qpn_shared_alloc (peers must have closed it)
 *   qpn_set_primal_mirrors  own = this rank's iterate buffer ([bytes], from qpn_shared_alloc), peers[k] = the
 *                      k-th peer's buffer as opened here (count <= QPN_MAX_MIRRORS; count = 0 clears).  Later
 *                      qpn_solve_nodes_into calls (device memory) whose x lies inside own[] also write
 *                      peers[k] + (x - own).  The stores are complete when the launch is; the CALLER orders
 *                      them against the peers' next reads (one barrier / tiny all-reduce per sweep). */
#define QPN_MAX_MIRRORS 7
#define QPN_IPC_HANDLE_BYTES 64
#define QPN_SHARED_FINE_GRAINED 1 /* qpn_shared_alloc flag: fine-grained (in-kernel cross-GPU visibility), for mailboxes */
int qpn_shared_alloc(qpn_ctx *ctx, size_t bytes, int flags, void **dev_ptr, uint8_t *handle);
int qpn_shared_open(qpn_ctx *ctx, const uint8_t *handle, void **dev_ptr);
int qpn_shared_close(qpn_ctx *ctx, void *dev_ptr);
int qpn_shared_free(qpn_ctx *ctx, void *dev_ptr);
int qpn_set_primal_mirrors(qpn_ctx *ctx, const double *own, size_t bytes, int32_t count, double *const *peers);

/* Per-sweep stop / raise decision (the reference ends a sweep with solved = false when any solve of the level
 * failed, src/algorithm.jl:95-109, src/avi.jl:426): out[0] = number of items with status != QPN_SUCCESS,
 * out[1] = max resid (NaN if any), out[2] = 1; out has 4 doubles.  status/resid/out in device memory, one small
 * launch, no host sync.
 * With world > 1 the pair is combined over all ranks (sum, max) WITHOUT a collective: boxes[r] is rank r's
 * mailbox (QPN_SWEEP_BOX_BYTES, from qpn_shared_alloc(QPN_SHARED_FINE_GRAINED), opened here; boxes[rank] the own
 * one); each rank posts its pair into every mailbox and waits until its own holds all `world` posts of this
 * `epoch` (the caller counts sweeps: 1, 2, 3, ... -- identical on all ranks).  Because it is enqueued after the
 * solve on the same stream, it is also the barrier that orders the solve's replica stores
 * (qpn_set_primal_mirrors) against the peers' next reads.  A peer that does not arrive within timeout_ms gives
 * out[2] = 0 (out[0..1] then cover the ranks that did) and out[3] += 1 -- a sticky count of missed barriers that the
 * caller zeroes and reads whenever it likes. */
#define QPN_SWEEP_BOX_BYTES 512
int qpn_sweep_status(qpn_ctx *ctx, const int32_t *status, const double *resid, int32_t count, double *out,
                     int32_t rank, int32_t world, void *const *boxes, uint64_t epoch, int32_t timeout_ms);

/* ---- (F1) local pieces of a node's solution map: local_piece, src/avi_solutions.jl:400-496 -----------------------
 * For the per-node GAVI of process_solution_graph (src/avi.jl:447-477) -- z = [x_d (n); lambda (m)], w = x_p (p), built from
 * the same node records as qpn_solve_nodes -- and a recipe K (one code per row of z: 1..4 on the x_d rows, 5..8 on the
 * constraint rows, src/avi_solutions.jl:390-399; code 0 = no condition), the polyhedral piece on which that recipe holds:
 *     rows [M N ; I2 0 ; I1 0 ; A B] over [z; w]  (:405-408),  bounds per code (:413-432),  noisy l > u -> l = u (:437-438),
 *     entries <= 1e-8 dropped (:439),  keep[] = find_non_trivial (:384-388).
 * Output per piece: Ap [(2N) x (N+p)] column-major (N = n+m), lp, up [2N], keep [2N]; simplify / projection stay with the
 * caller (polyhedral algebra).  `pieces` items; item t uses the records of node node_of[t] (node_of == NULL: node t), so
 * the many recipes of one solution share its records (nodes = number of record sets behind the pointers).  node_of entries
 * outside 0 .. nodes-1: QPN_ERR_ARG for host arrays; for device arrays (not read by the host) the piece comes back EMPTY --
 * keep = 0 on every row, bounds (-inf, +inf), zero coefficients -- and no record is read.  Codes outside a row's range
 * (x_d rows: 1..3, constraint rows: 5..8) mean "no condition" like code 0 (what qpn_recipes_from_masks emits for an empty mask).
 * qpn_recipes_from_masks enumerates recipes from the active-set masks of a solve (`active` of qpn_solve_nodes, one uint8
 * per row: the code sets J of src/avi_solutions.jl:511-562): recipe number first + t of the Cartesian product of the rows'
 * code sets (all_Ks, :200-215; row 0 is the fastest digit) for t < count; *total (may be NULL) = number of recipes
 * (saturating at INT64_MAX). */
int qpn_local_pieces(qpn_ctx *ctx, int32_t pieces, int32_t nodes, int32_t n, int32_t m, int32_t p, const double *Qd,
                     const double *R, const double *qd, const double *Ad, const double *B, const double *l,
                     const double *u, const int32_t *node_of, const uint8_t *K, double *Ap, double *lp, double *up,
                     uint8_t *keep, int mem);
int qpn_recipes_from_masks(qpn_ctx *ctx, int32_t N, const uint8_t *mask, int64_t first, int32_t count, uint8_t *K,
                           int64_t *total, int mem);

/* ---- (F1, batched over a level) the solution-graph pieces of MANY nodes with O(1) calls -------------------------------------
 * The outer loop maps process_qp over the nodes of a level (src/algorithm.jl:44-52) and every optimal node below level 1
 * makes its solution graph (src/qp_processing.jl:158, :193-198, :231 -> process_solution_graph, src/avi.jl:447-477).
 * qpn_recipes_batch: all_Ks (src/avi_solutions.jl:200-215) for `nodes` solutions in one launch.  masks [nodes][N]; offsets
 *   [nodes + 1] (ALWAYS a host array, like a pool shape: offsets[0] = 0, node b gets the recipes 0 .. offsets[b+1]-offsets[b]-1 of
 *   its Cartesian product, at most as many as the product has); outputs K [offsets[nodes]][N] and node_of [offsets[nodes]] --
 *   exactly what qpn_local_pieces / qpn_reduced_pieces take.
 * qpn_reduced_pieces: local_piece (src/avi_solutions.jl:400-496, as qpn_local_pieces) followed by the elimination of the m
 *   multiplier columns through the piece's own equality rows (eliminate_variables, src/sets.jl:731-800: one column at a time,
 *   the alive equality row with the largest entry |a| > tol, the first of equal ones; that row then leaves) -- what
 *   project_and_permute (src/avi_solutions.jl:79-91) comes to when the active rows pin the multipliers.  Output per piece, over
 *   the columns [x_d (n); x_p (p)] and with room for cap = n + 2m rows: Ar = the cap x (n+p) matrix, column-major,
 *   lr, ur [cap], rows = the number of rows that remain (in their original order), flags: bit 0 = a multiplier column was pinned
 *   by no equality row while an alive row still holds it (degenerate active set: the projection needs Fourier-Motzkin / vertex
 *   enumeration: qpn_project_pieces below takes such pieces -- the piece's output here is then incomplete), bit 1 = more than cap
 *   rows remained.
 *   Beyond rows[t] every output is filled: Ar with zeros, lr with -inf, ur with +inf (a piece whose device-side node_of entry
 *   is out of range is all fill: rows = 0, flags = 0).
 *   The local pieces themselves live in the context's workspace only.  n + m <= 512. */
int qpn_recipes_batch(qpn_ctx *ctx, int32_t nodes, int32_t N, const uint8_t *masks, const int64_t *offsets, uint8_t *K,
                      int32_t *node_of, int mem);
int qpn_reduced_pieces(qpn_ctx *ctx, int32_t pieces, int32_t nodes, int32_t n, int32_t m, int32_t p, const double *Qd,
                       const double *R, const double *qd, const double *Ad, const double *B, const double *l,
                       const double *u, const int32_t *node_of, const uint8_t *K, double tol, double *Ar, double *lr, double *ur,
                       int32_t *rows, int32_t *flags, int mem);

/* ---- degenerate pieces: the projection onto [x_d; x_p] by Fourier-Motzkin steps ------------------------------------------------
 * qpn_project_pieces: qpn_reduced_pieces for the pieces it flags with bit 0.  Arguments as there, plus cap: the rows of room per
 *   piece, cap >= n + 2m (else QPN_ERR_ARG).  Per piece:
 *   1. local_piece and the elimination through the piece's own equality rows, operation by operation as qpn_reduced_pieces does
 *      them; a multiplier column that no equality row pins while an alive row holds it (|a| > tol) is not flagged but joins the
 *      list `left`, ascending.  The alive rows are then taken in their order.
 *   2. One Fourier-Motzkin step per column j of `left`, ascending, on the rows the step before it left:
 *        the rows with |a_kj| <= tol come first, in order, unchanged;
 *        every other row k, in order, gives up to two one-sided inequalities, in this order: (a_k, u_k) if u_k is finite, then
 *        (-a_k, -l_k) if l_k is finite; each is divided, entry by entry and in its bound, by |a_kj|, and goes to the list ub if
 *        its entry j is > 0, else to the list lb;
 *        the new rows are au + al with the bounds (-inf, bu + bl), for every entry of ub (outer loop) against every entry of lb
 *        (inner loop); column j is then 0 in all rows.
 *      Divisions and additions only, no contraction: bit-equal to the same steps in IEEE double arithmetic on the host.
 *      A step first counts its rows, nz + |ub| |lb|, in 64 bits: more than cap gives the piece flag bit 2, its outputs are all
 *      fill with rows = 0, and nothing more is computed for it.  Redundant rows are not removed.
 *   3. Output over the columns [x_d (n); x_p (p)]: Ar = the cap x (n+p) matrix, column-major, lr, ur [cap], rows, flags; beyond
 *      rows[t] the fill of qpn_reduced_pieces (0, -inf, +inf).  For a piece without a left column the first n + 2m rows equal
 *      qpn_reduced_pieces' output.
 *   flags: bit 0 is never set;  bit 1 = more than cap rows were alive after step 1 (the first cap go out, step 2 is skipped: not
 *   possible for cap >= n + 2m unless the x_d rows carry codes other than 2);  bit 2 (value 4) = a step needed more than cap rows.
 *   The local pieces and the steps' rows live in the context's workspace: a call is split into chunks of pieces that fit 512 MiB
 *   of it; a cap of which not even one piece fits is QPN_ERR_SIZE.  n + m <= 512. */
int qpn_project_pieces(qpn_ctx *ctx, int32_t pieces, int32_t nodes, int32_t n, int32_t m, int32_t p, const double *Qd,
                       const double *R, const double *qd, const double *Ad, const double *B, const double *l,
                       const double *u, const int32_t *node_of, const uint8_t *K, double tol, int32_t cap, double *Ar, double *lr,
                       double *ur, int32_t *rows, int32_t *flags, int mem);

/* ---- every recipe of a solution graph, chunk by chunk, finished on the device (QPNetOptions.max_pieces = None) --------------
 * qpn_recipes_batch_range: qpn_recipes_batch from a starting recipe per node: node b gets the recipes
 *   first[b] .. first[b] + offsets[b+1] - offsets[b] - 1 of its Cartesian product (row 0 the fastest digit).  first [nodes] int64
 *   and offsets are ALWAYS host arrays; first[b] < 0 or a range beyond the product (device masks are read back to check it) is
 *   QPN_ERR_ARG.  first == NULL is qpn_recipes_batch.
 * qpn_finish_pieces: the finishing step of qpn_reduced_pieces' output (Ar [pieces][n+p][cap] column-major, lr, ur [pieces][cap],
 *   rows, flags [pieces], cap = n + 2m, n + m <= 512).  Piece t belongs to item rec_of[t] (0 .. records-1); item k reads the
 *   ncols[k] <= n + p columns take[k][0 .. ncols[k]-1] of Ar (in ascending global order: the item's column map), the point xk[k][.]
 *   and the probe vector probe[k][.] on them (take, xk, probe: [records][n+p]).  Per piece, over those columns, with the host's
 *   operations in the host's order (fp contraction off): every row scaled to a largest |coefficient| of 1 (bounds with it),
 *   entries < 1e-8 dropped, the row divided by |its leading nonzero| (negated, bounds swapped, when that is negative).  Outputs:
 *     status [pieces]  QPN_FIN_MEMBER: worst <= member_tol;  QPN_FIN_MERGE: two row projections on the probe vector are close
 *                      after sorting (<= 1e-7 (1 + |h|)) or a valid row is all zero;  QPN_FIN_DUP: an equal earlier piece exists;
 *                      QPN_FIN_FLAGGED: flags[t] != 0, nothing else is computed for the piece (worst 0, hash 0)
 *     worst [pieces]   the largest violation of the point over the live rows (index < rows[t], some nonzero coefficient), >= 0
 *     hash [pieces]    64 bits of the key: the rows rounded to 6 digits (rint(v 1e6) / 1e6 + 0.0), then the bounds rounded
 *     dup_of [pieces]  for a member that is neither a merge candidate nor flagged: the earliest earlier such piece of the same item
 *                      whose rows, rounded rows and rounded bounds are bit-equal (-1: none); -1 for every other piece
 *     store_of [pieces] the piece's slot in the store, or -1.  Stored: the members that are neither duplicates nor flagged.
 *     As [store_cap][n+p][cap] (column-major; columns >= ncols are 0), ls, us [store_cap][cap], rows_s [store_cap]: the
 *                      normalised pieces, in piece order; *stored (host) = their number.  More than store_cap: QPN_ERR_SIZE.
 *   Host mode copies back only the first *stored slots of the store. */
#define QPN_FIN_MEMBER 1
#define QPN_FIN_MERGE 2
#define QPN_FIN_DUP 4
#define QPN_FIN_FLAGGED 8
int qpn_recipes_batch_range(qpn_ctx *ctx, int32_t nodes, int32_t N, const uint8_t *masks, const int64_t *first, const int64_t *offsets,
                            uint8_t *K, int32_t *node_of, int mem);
int qpn_finish_pieces(qpn_ctx *ctx, int32_t pieces, int32_t records, int32_t n, int32_t m, int32_t p, const double *Ar, const double *lr,
                      const double *ur, const int32_t *rows, const int32_t *flags, const int32_t *rec_of, const int32_t *ncols,
                      const int32_t *take, const double *xk, const double *probe, double member_tol, int32_t *status, double *worst,
                      uint64_t *hash, int32_t *dup_of, int32_t *store_of, int32_t store_cap, double *As, double *ls, double *us,
                      int32_t *rows_s, int32_t *stored, int mem);

/* ---- (A8) batched per-node KKT verification, src/qp_processing.jl:57-149 ------------
 *   xd [batch][n] current decision values, w as above.
 *   solution [batch] int32 (1 = optimal for the node), lambda [batch][m] (sign: + at the lower
 *   bound, - at the upper, :120-123), path [batch] int32: 0 infeasible (:86-89), 1 m==0
 *   shortcut (:91-96), 2 least-squares duals accepted (:114-124), 3 bounded-LSQ fallback
 *   accepted (:129-139), 4 fallback rejected (:141), 5 fallback solver failed (:144),
 *   6 no such node (qpn_verify_nodes_subset_h only: the slot's entry of a device list is out of range).
 *   tol = 1e-4 (:57).  n, m <= 64: one wavefront per node; up to 512: one workgroup per node.
 *   QPN_MEM_DEVICE with m == 0: Ad must still point at 8 readable bytes.  The n <= 32 kernel (verify_node32) loads the first
 *   element of the node's Ad block with a clamped index whatever m is, so a null Ad is a load from address 0 there.  Host memory
 *   and resident handles are safe: the library pads their empty arrays. */
int qpn_verify_nodes(qpn_ctx *ctx, int32_t batch, int32_t n, int32_t m, int32_t p,
                     const double *Qd, const double *R, const double *qd, const double *Ad,
                     const double *B, const double *l, const double *u, const double *xd,
                     const double *w, int64_t stride_w, double tol, int32_t *solution,
                     double *lambda, int32_t *path, int mem);

/* ---- batched reduced-Hessian convexity check, check_qp_convexity (src/qp_processing.jl:39-55) ----------
 *   Qd [batch][n][n] and Ad [batch][m][n] column-major per node as above, eq [batch][m] uint8: 1 marks an
 *   implicit equality row (polyhedra.implicit_bounds).  Z = an orthonormal basis of null(Ad[eq, :]) (the rank
 *   by Julia's rule, count sigma_i > min(k, n) * eps * sigma_max, with all-zero rows left out of k);
 *   H = Z' (Qd + Qd') Z.  convex [batch] int32 = all eigenvalues of H > -tol; min_eig [batch] = the smallest
 *   one (+inf when H is empty); null_dim [batch] int32 = n - rank.  A non-finite entry of Qd or of a selected
 *   row gives convex = 0, min_eig = NaN, null_dim = -1.  tol = 1e-6 (:39).  1 <= n <= 256, 0 <= m <= 1024
 *   (QPN_ERR_SIZE beyond).  n <= 32: one wavefront per node; up to 128: one workgroup per node in LDS;
 *   beyond: one workgroup per node over a global workspace. */
int qpn_convexity_nodes(qpn_ctx *ctx, int32_t batch, int32_t n, int32_t m, const double *Qd, const double *Ad,
                        const uint8_t *eq, double tol, int32_t *convex, double *min_eig, int32_t *null_dim, int mem);

/* ---- multiplier-vertex exploration, QPNetOptions.exploration_vertices (src/avi_solutions.jl:92-129, :241-382) ----------
 * qpn_multiplier_vertices: per item, vertices of Lambda = { lambda : Ad' lambda = g, per-row class } -- the multiplier set of a
 *   node at a point.  Ad [batch][m][n] column-major as above (so Ad' is [n][m] row-major), g [batch][n], cls [batch][m] uint8
 *   (QPN_MV_GE: lambda_j >= 0, QPN_MV_LE: <= 0, QPN_MV_FREE, QPN_MV_ZERO: lambda_j = 0), lam0 [batch][m] the multiplier the
 *   walk starts from (purified to a vertex).  Up to V vertices, distinct after rounding to 5 digits, in the breadth-first order
 *   of a walk over adjacent bases (every tied leaving row, 2^-30 relative tie band; each basis factored afresh), at most
 *   max_bases bases per item.  tol: pivot and zero tolerance on the row-equilibrated system (1e-9); feas: a sign-constrained
 *   basic value down to -feas (times max(1, |rhs|)) counts as feasible (1e-6).  Outputs verts [batch][V][m] (unused slots 0),
 *   count [batch], status [batch] (QPN_MV_*).  1 <= n, m <= 512 (QPN_ERR_SIZE beyond).  n, m <= 32: one wavefront per item;
 *   up to 128: one workgroup per item in LDS; beyond: one workgroup per item over a global workspace.
 * qpn_recipe_filter: recipes K [pieces][N] (codes 1..8) of product rows vrow_of [pieces] (int32) of masks [rows][N]; first_of
 *   [rows] (int32) = the first row of the same item.  keep [pieces] uint8 = 0 when an earlier row s (first_of[v] <= s < v) of
 *   the recipe's item holds every one of its codes (the reference's setdiff with the explored recipes), 1 otherwise. */
enum { QPN_MV_GE = 0, QPN_MV_LE = 1, QPN_MV_FREE = 2, QPN_MV_ZERO = 3 };
enum { QPN_MV_COMPLETE = 0, QPN_MV_VERTEX_BUDGET = 1, QPN_MV_BASIS_BUDGET = 2, QPN_MV_EMPTY = 3, QPN_MV_NO_VERTEX = 4 };
int qpn_multiplier_vertices(qpn_ctx *ctx, int32_t batch, int32_t n, int32_t m, const double *Ad, const double *g, const uint8_t *cls,
                            const double *lam0, int32_t V, int32_t max_bases, double tol, double feas, double *verts, int32_t *count,
                            int32_t *status, int mem);
int qpn_recipe_filter(qpn_ctx *ctx, int32_t pieces, int32_t rows, int32_t N, const uint8_t *masks, const uint8_t *K,
                      const int32_t *vrow_of, const int32_t *first_of, uint8_t *keep, int mem);

/* ---- interior members of polyhedra: the prefilter of remove_subsets (src/sets.jl:889-902, the slack program of `exemplar`,
 *      :591-642), node records made on the device ----------
 * A batch of polyhedra {x : l <= A x <= u} of one size: A [batch][r][d] column-major per item (row i, column c at c * r + i),
 * l, u [batch][r].  Row classes per item: eq = finite l and l == u;  lo = not eq and finite l;  hi = not eq and finite u.
 * The caller passes capacities ne, nlo, nhi (at least the batch's largest class counts).  The record of an item is the node
 *     min eps + delta/2 (|x|^2 + eps^2)   s.t.  a_i'x = l_i (eq),  a_i'x + eps >= l_i (lo),  a_i'x - eps <= u_i (hi)
 * with the equality multipliers in the free block: nf = d + 1 + ne free variables [x; eps; mu_E], mp = max(16, nlo + nhi
 * rounded up to 16) rows, in the layout of qpn_solve_nodes (p = 1, R = 0, B = 0, w = 0):
 *     Qd [batch][nf][nf] = [[delta I_(d+1), -A_E'], [A_E, D]]  (D: 1 on idle multiplier slots, 0 on used ones),
 *     qd [batch][nf] = [0_d; 1; -l_E],  Ad [batch][mp][nf]: slots 0 .. nlo-1 the lo rows [a_i, +1, 0] in (l_i, +inf), slots
 *     nlo .. nlo+nhi-1 the hi rows [a_i, -1, 0] in (-inf, u_i), every other slot a zero row in (-inf, +inf).
 * The rows of a class are taken in ascending row order.  An item with more rows of a class than its capacity is not cut
 * short: flag [batch] uint8 = 1 for it, its record is that of a polyhedron without rows, and it has no member (ok = 0).
 * Limits: nf + mp <= 1024 (as qpn_solve_nodes), r <= 4096; QPN_ERR_SIZE beyond.
 *
 * qpn_assemble_interior_nodes: the records alone (every word written, zeros included).
 * qpn_interior_members: records (workspace of the context) -> the solve of qpn_solve_nodes with default options and a cold
 *   start -> x_out [batch][d] = the member, ok [batch] uint8 = status == QPN_SUCCESS and eps <= 1e-6 and not flagged (x_out is
 *   meaningful only where ok), status [batch] the solver's.  Host mode moves A, l, u up and x_out, ok, status down.
 * qpn_members_outside: pair q asks whether member X[pi[q]] (X [Bi][d]) lies outside piece pj[q] of a group of Bj pieces of one
 *   size (Aj [Bj][rj][d] column-major, lj, uj [Bj][rj]): out[q] = 1 when a row has a.x < l - t or a.x > u + t, a.x summed over
 *   ascending columns (acc = acc + a * x[c], no contraction).  Order the pairs by piece where many members meet one piece: 16
 *   consecutive pairs over one piece share one read of it.  Host index arrays out of range: QPN_ERR_ARG; device ones: that
 *   pair answers 1 ("not settled here").
 * qpn_members_outside_lists: the same question list by list, the pairs enumerated on the device.  One call covers one pack of
 *   Bj second pieces of one size and the members of dimension d, with ok [Bi] as qpn_interior_members wrote it (a member with
 *   ok == 0 refutes nothing).  list_ptr [lists + 1] and list_mem [list_ptr[lists]] are a CSR: position s of list a is row
 *   list_mem[list_ptr[a] + s] of X, -1 = that piece has no member; a list names ALL its pieces in list order, those whose own
 *   matrices sit in another pack included.  list_of [Bj]: the list of piece j; self_pos [Bj]: its own position there;
 *   word_ptr [Bj + 1] (int64): piece j owns the words bits [word_ptr[j], word_ptr[j + 1]), at least ceil(k / 32) of them for a
 *   list of k.  Every word of every segment is written: bit (s & 31) of word (s >> 5) of the segment is 1 when s != self_pos[j],
 *   the member at position s exists and is ok, and it violates a row of piece j by more than t (the arithmetic of
 *   qpn_members_outside); every other bit is 0.  undecided [Bj] = the number of positions s != self_pos[j] of the list with bit 0:
 *   the pairs still to be put to an LP.  Host mode: list_ptr and word_ptr start at 0 and are monotone, every index is in range
 *   (list_of, self_pos, list_mem in [-1, Bi)) and every segment long enough, else QPN_ERR_ARG and nothing is launched.  Device
 *   mode: list_ptr and word_ptr lie inside their buffers (the caller's duty: list_mem has list_ptr[lists] entries, bits
 *   word_ptr[Bj] words); a piece with a bad list_of, self_pos or too short a segment gets its whole segment 0 and undecided =
 *   max(k - 1, 0), or 0 when the list itself is bad, and nothing is read through the bad index; a list_mem entry outside
 *   [-1, Bi) answers 1 for that position (other than self_pos), the convention of qpn_members_outside.  1 <= d, 1 <= rj <= 4096,
 *   Bi * d < 2^31 (QPN_ERR_SIZE beyond); Bj == 0 or lists == 0 succeeds (lists == 0: every segment 0, undecided 0). */
int qpn_assemble_interior_nodes(qpn_ctx *ctx, int32_t batch, int32_t r, int32_t d, const double *A, const double *l, const double *u,
                                double delta, int32_t ne, int32_t nlo, int32_t nhi, double *Qd, double *qd, double *Ad, double *lo,
                                double *uo, uint8_t *flag, int mem);
int qpn_interior_members(qpn_ctx *ctx, int32_t batch, int32_t r, int32_t d, const double *A, const double *l, const double *u,
                         double delta, int32_t ne, int32_t nlo, int32_t nhi, double *x_out, uint8_t *ok, int32_t *status, int mem);
int qpn_members_outside(qpn_ctx *ctx, int32_t pairs, int32_t d, int32_t rj, const double *Aj, const double *lj, const double *uj,
                        int32_t Bj, const double *X, int32_t Bi, const int32_t *pi, const int32_t *pj, double t, uint8_t *out, int mem);
int qpn_members_outside_lists(qpn_ctx *ctx, int32_t d, int32_t rj, const double *Aj, const double *lj, const double *uj, int32_t Bj,
                              const double *X, const uint8_t *ok, int32_t Bi, int32_t lists, const int32_t *list_ptr,
                              const int32_t *list_mem, const int32_t *list_of, const int32_t *self_pos, const int64_t *word_ptr,
                              double t, uint32_t *bits, int32_t *undecided, int mem);

/* ---- inner-node records made on the device from a pool of child pieces (src/qp_processing.jl:62-66, :183-187: a node's
 *      constraint stack is [base; child pieces]) ----------
 * An ITEM is one parent under one choice of its children's pieces.  Its record is made from inputs that go up once:
 *   static store, `parents` parents of one shape, in the layout of qpn_solve_nodes: sQd [parents][n0][n0], sR [parents][ps][n0],
 *     sqd [parents][n0], sAd [parents][n0][mb] (row t, column j at j * mb + t), sB [parents][ps][mb], sl, su [parents][mb],
 *     mb_true [parents] int32: the parent's own base row count (<= mb, the common padded count);
 *   piece pool: piece_desc [pieces][4] int32 = (row0, rows, c, off): the piece's rows are pl, pu [row0 .. row0 + rows) (of
 *     pool_rows) and its coefficients pA [off .. off + rows * c) (of pool_words), row-major over its own c columns;
 *   column maps: map k is map_data [map_off[k] .. map_off[k + 1]) (map_off [maps + 1], map_data [map_words], int32), one entry
 *     per piece column: j in [0, n0) = decision column j (Ad), n0 + k with k < p = parameter column k (B), -1 = the parent does
 *     not read that variable (legal only under coefficients that are all zero).  No column may be named twice by one map;
 *   items: parent_of [items], piece_of, map_of [items][QPN_PARENT_SLOTS] int32 (piece_of -1 = empty slot).
 * The stack of an item is its parent's mb_true base rows, then the rows of its slots in slot order; parameter columns
 * k >= ps of a base row are zero.
 *   form 0 (the verify form): n = n0;  Qd = sQd, R = [sR, 0], qd = sqd, rows 0 .. T-1 the stack, rows T .. m-1 inert
 *     (0'x in (-inf, +inf)).  `ne` is ignored.
 *   form 1 (the solve form, equality rows in the free block): E = the stack rows with finite l == u, in order, I = the others,
 *     in order; n = n0 + ne with ne = |E| for EVERY item of the call;  Qd = [[sQd, -A_E'], [A_E, 0]], R = [R; B_E],
 *     qd = [sqd; -l_E], rows [A_I 0], B_I, l_I, u_I, then inert rows up to m.  The negation is applied to every entry of A_E'
 *     and l_E (a zero becomes -0.0); every other structural zero is +0.0.  No other arithmetic is done.
 * Outputs, every word written: Qd [items][n][n], R [items][p][n], qd [items][n], Ad [items][n][m], B [items][p][m], l, u
 * [items][m] (the layout of qpn_solve_nodes / qpn_verify_nodes, which take them in place in device mode), err [items] int32:
 *   0 good;  1 a parent, piece or map index (or a piece's range in the pool, or mb_true) out of range;  2 a map that is not as
 *   long as its piece has columns, has an entry outside [-1, n0 + p) or names a column twice;  3 a -1 map entry under a
 *   non-zero coefficient;  4 more rows than m (or than 1024 in the stack);  5 form 1: |E| != ne.  The lowest code that applies.
 * A bad item's record is its parent's static blocks (zeros when the parent index itself is bad) over all-inert rows, the ne
 * extra free variables zero.  Nothing is read through a bad index.  Host mode: a bad item gives QPN_ERR_ARG (err is still
 * written); device mode: QPN_OK, err tells.  Limits: n + m <= 1024 (QPN_ERR_SIZE), p >= 1.  items == 0 succeeds.
 * level_batch.assemble_parent_records_host is the numpy twin and the normative statement: every output is bit-equal to it. */
#define QPN_PARENT_SLOTS 8
int qpn_assemble_parent_nodes(qpn_ctx *ctx, int32_t items, int32_t form, int32_t n0, int32_t ne, int32_t m, int32_t p,
                              int32_t parents, int32_t mb, int32_t ps, const double *sQd, const double *sR, const double *sqd,
                              const double *sAd, const double *sB, const double *sl, const double *su, const int32_t *mb_true,
                              int32_t pieces, const int32_t *piece_desc, int32_t pool_rows, int32_t pool_words, const double *pA,
                              const double *pl, const double *pu, int32_t maps, const int32_t *map_off, int32_t map_words,
                              const int32_t *map_data, const int32_t *parent_of, const int32_t *piece_of, const int32_t *map_of,
                              double *Qd, double *R, double *qd, double *Ad, double *B, double *l, double *u, int32_t *err, int mem);

/* ---- batched LP solver for the polyhedral primitives: `exemplar`, `isempty`, `issubset`, `implicit_bounds` (src/sets.jl:591-713,
 *      :376-407; one OSQP LP per question there) ----------
 * qpn_solve_lps: `jobs` LPs over `polys` shared polyhedra {x : l <= A x <= u} of one size.  A [polys][r][d] column-major per item
 * (row i, column c at c * r + i), l, u [polys][r] (+-inf allowed), poly_of [jobs] int32.  Job t minimises c_t'x with c_t =
 * cost[t] (cost [jobs][d]) or, when cost == NULL, obj_sign[t] * row obj_row[t] of A[poly_of[t]] (int32 arrays; the device reads
 * the row in place).  Outputs per job (x, obj, lambda, ray, iters may be NULL):
 *   status [jobs] int32 (QPN_LP_*), x [jobs][d] (the optimum; for UNBOUNDED the feasible point the ray starts from; otherwise
 *   the point reached), obj [jobs] = c'x on the unscaled data, iters [jobs] int32 (flips and pivots after the crash),
 *   lambda [jobs][r]: OPTIMAL: c = A'lambda, + at the lower bound, - at the upper (the convention of qpn_verify_nodes);
 *     INFEASIBLE: a Farkas vector y, A'y = 0 and sum(y_i > 0 ? y_i u_i : y_i l_i) < 0 by the margin of step 9;  zeros otherwise
 *     (ITER_LIMIT and every FAILURE, whatever produced it),
 *   ray [jobs][d]: UNBOUNDED: c'ray < 0, (A ray)_i >= 0 where l_i is finite, <= 0 where u_i is finite;  zeros otherwise.
 * Method (polyhedra.solve_lps_host is its numpy twin and the normative statement; every output is bit-equal to it: each sum runs
 * over the ascending index as acc = acc + a * b, no contraction): bounded-variable primal simplex on the row-activity form, x
 * free, s = A x in [l, u].  (0) data screen: an entry of A or c that is not finite, a bound that is not a number, l_i = +inf or
 * u_i = -inf makes the job QPN_LP_FAILURE at 0 steps with zeros (the comparisons of the method are not defined on such data).
 * The screen reads the polyhedron and qpn_solve_lps' own c.  The objective of a warm solve (qpn_issubset_pairs (f): a row of P2)
 * passes no screen: a non-finite entry there makes every comparison of the pricing false, the loop ends at once, the check of step
 * 9 fails before and after step 10's rebuild, and that solve is QPN_LP_FAILURE.
 * (1) rows and their bounds scaled by 1 / max|a_i|; an all-zero row with l_i > 0 or u_i < 0 makes the
 * job INFEASIBLE (Farkas vector -+e_i), otherwise it is inert.  (2) dictionary basic = T nonbasic, r x d, plus a cost row; ids
 * x_j = j, s_i = d + i; start basic = s, T = A, cost row = c.  (3) crash, columns ascending: pivot on the largest |T_ij| among rows
 * still holding an s (2^-30 relative band, lowest row); a column whose best entry is <= piv_tol stays nonbasic, free, at 0; a
 * basic x never leaves.  (4) a nonbasic s starts at its finite bound nearest zero (the lower on a tie), at 0 without one.
 * (5) phase 1 minimises the sum of the basic violations beyond feas_tol * max(1, |bound|), phase 2 minimises c; the phase is
 * decided before every step.  (6) entering: reduced cost beyond opt_tol in a direction the value allows, never a fixed variable;
 * the largest |reduced cost| (2^-30 band, lowest id); after 20 consecutive zero-length steps the lowest eligible id until a step
 * is positive.  (7) ratio test: the entering variable's opposite bound (a flip, no pivot) and basic variables with |entry| >
 * piv_tol; a violated basic blocks at the bound it violates when moving towards it, not when moving away; the smallest ratio,
 * negative ones clamped to 0, ties within 1e-12 * max(1, ratio) to the lowest id.  (8) pivot p = T[i][j]: new row i = -T[i][k] / p,
 * 1 / p at j; every other row and the cost row, f = their entry at j: T[k][c] += f * new_i[c], T[k][j] = f / p.  (9) phase 1
 * without entering variable: INFEASIBLE; phase 2 without blocking candidate: UNBOUNDED; phase 2 without entering variable:
 * OPTIMAL; a further step due after max_iters: ITER_LIMIT.  A claimed outcome is checked on the unscaled rows at check_tol --
 * primal feasibility within check_tol * max(1, |bound|); |c - A'lambda| <= check_tol * max(1, |c_k|), a multiplier beyond +-check_tol only at its
 * bound; |A'y| <= check_tol * max(1, |y|_inf) and the Farkas sum < -sum_i |y_i| check_tol max(1, |bound_i|), bound_i the bound the
 * sum takes of row i (infeasible even with every bound relaxed by the tolerance primal feasibility is judged at: a residual of A'y
 * tolerated at check_tol |y|_inf makes a sum nearer to zero prove nothing); c'ray < 0 and the row conditions within check_tol *
 * max(1, |ray|_inf) * max|a_i|.  (10) an end that is not certified -- a claimed outcome that fails its check, phase 1 without a
 * blocking candidate, and in a warm solve (qpn_issubset_pairs (f), qpn_implicit_bounds (c)) an INFEASIBLE end -- has met the drift of
 * a dictionary updated in place: the dictionary of the current basis is rebuilt from the scaled rows, T = A, cost row = c, then for
 * the columns j ascending whose x is basic the pivot of step 3 among the rows whose s is nonbasic in that basis and still basic here
 * (at most d pivots; the nonbasic s keep their values), and the loop runs once more, the step count going on towards max_iters.
 * What that second loop ends with stands; not certified again, or a rebuild pivot <= piv_tol, is QPN_LP_FAILURE.  A loop that ends
 * certified never rebuilds.
 * opts == NULL: the defaults.  max_iters <= 0: 50 (r + d) + 100.  Host poly_of / obj_row out of range: QPN_ERR_ARG; device ones:
 * that job answers QPN_LP_FAILURE with zeros and reads nothing.  1 <= d <= 256, 1 <= r <= 1024 (QPN_ERR_SIZE beyond).
 * qpn_lp_kernel_class(r, d): 0 = one wavefront per job, dictionary in LDS, four jobs per workgroup; 1 = one workgroup of 256 per
 * job in LDS; 2 = one workgroup per job over a slice of the context workspace, launched in chunks; -1 beyond the limits. */
enum { QPN_LP_OPTIMAL = 1, QPN_LP_INFEASIBLE = 2, QPN_LP_UNBOUNDED = 3, QPN_LP_ITER_LIMIT = 4, QPN_LP_FAILURE = 5 };
typedef struct {
    double piv_tol;    /* 1e-9, on the row-scaled data */
    double feas_tol;   /* 1e-9 */
    double opt_tol;    /* 1e-9 */
    double check_tol;  /* 1e-6, the post-check on the unscaled data */
    int32_t max_iters; /* <= 0: 50 (r + d) + 100 */
    int32_t reserved;
} qpn_lp_opts;
void qpn_lp_default_opts(qpn_lp_opts *opts);
int qpn_lp_kernel_class(int32_t r, int32_t d);
int qpn_solve_lps(qpn_ctx *ctx, int32_t polys, int32_t r, int32_t d, const double *A, const double *l, const double *u, int32_t jobs,
                  const int32_t *poly_of, const double *cost, const int32_t *obj_row, const int32_t *obj_sign, const qpn_lp_opts *opts,
                  int32_t *status, double *x, double *obj, double *lambda, double *ray, int32_t *iters, int mem);

/* qpn_issubset_pairs: `pairs` subset questions P1 within P2 (`issubset`, src/sets.jl:376-407) over B1 first pieces and B2 second
 * pieces, one job per pair: first piece pi[q] against second piece pj[q].  A1 [B1][r1][d], A2 [B2][r2][d] column-major per item,
 * l1, u1 [B1][r1], l2, u2 [B2][r2] (+-inf allowed), pi, pj [pairs] int32.  Outputs per pair (how, bound, val, lps, iters may be NULL):
 *   sub [pairs] uint8: 1 for HOLDS and EMPTY, 0 otherwise;  how [pairs] int32 (QPN_SUBSET_*);
 *   bound [pairs] int32: 2 i + side of the bound of P2 that decided (side 0 = l2[i], 1 = u2[i]), -1 where none did;
 *   val [pairs]: the objective value that decided (BY_POINT, BY_OPTIMUM), 0 otherwise;
 *   lps [pairs] int32: simplex solves started, the feasibility solve counted;  iters [pairs] int32: all their steps.
 * Method (polyhedra.issubset_pairs_host is its numpy twin and the normative statement; every output is bit-equal to it, by the
 * discipline of qpn_solve_lps, whose set-up, loop and check it runs):  (a) steps 1-8 of qpn_solve_lps on P1 with c = 0: the crash
 * and phase 1 once per pair; an INFEASIBLE end whose Farkas certificate holds is EMPTY, otherwise (after step 10's rebuild and
 * second loop) FAILURE; ITER_LIMIT and FAILURE pass through.  (b) the rows i of P2 ascending, the lower bound (c = +a2_i, beta = l2[i]) before the upper (c = -a2_i, beta =
 * -u2[i]); a non-finite bound is skipped.  (c) own-row skip: when rows k of P1 equal row i of P2 entry by entry (IEEE ==, unscaled)
 * and max l1[k] >= l2[i] - tol (min u1[k] <= u2[i] + tol) over them, the bound holds on all of P1 and needs no work.  (d) point
 * test: v = c'x at the point the previous solve ended at; v < beta - tol is BY_POINT.  (e) no second crash: the cost row of c in the
 * current dictionary, column j: acc = 0; rows i ascending that hold an x: acc = acc + c[id] * T[i][j]; then + c[id] when column j
 * holds an x.  (f) the loop with fresh step and degeneracy counters (max_iters per objective), then the check of step 9 on P1 and,
 * where the end is not certified, step 10: OPTIMAL with obj < beta - tol is BY_OPTIMUM, otherwise the next bound; a certified ray is
 * UNBOUNDED; a certificate that fails, or an INFEASIBLE end, after the rebuild too, is FAILURE.  (g) no bound left: HOLDS.
 * Kernel classes are those of qpn_lp_kernel_class(r1, d); nothing of P2 is copied.  Host pi / pj out of range: QPN_ERR_ARG; device
 * ones: that pair answers sub = 0, QPN_SUBSET_FAILURE, bound = -1, zeros elsewhere and reads nothing.  1 <= d <= 256, 1 <= r1, r2
 * <= 1024 (QPN_ERR_SIZE beyond).  pairs == 0 succeeds. */
enum {
    QPN_SUBSET_HOLDS = 0,      /* every finite bound of P2 passed                                  sub = 1 */
    QPN_SUBSET_BY_POINT = 1,   /* the current vertex of P1 lies below a bound by more than tol     sub = 0 */
    QPN_SUBSET_BY_OPTIMUM = 2, /* a certified optimum lies below the bound by more than tol        sub = 0 */
    QPN_SUBSET_UNBOUNDED = 3,  /* a bound's objective is unbounded below on P1, certified by a ray sub = 0 */
    QPN_SUBSET_ITER_LIMIT = 4, /* the iteration limit was reached                                  sub = 0 */
    QPN_SUBSET_FAILURE = 5,    /* failure, or a certificate that does not hold: the piece is kept  sub = 0 */
    QPN_SUBSET_EMPTY = 6       /* P1 is empty, certified by the Farkas vector                      sub = 1 */
};
int qpn_issubset_pairs(qpn_ctx *ctx, int32_t d, int32_t B1, int32_t r1, const double *A1, const double *l1, const double *u1,
                       int32_t B2, int32_t r2, const double *A2, const double *l2, const double *u2, int32_t pairs, const int32_t *pi,
                       const int32_t *pj, double tol, const qpn_lp_opts *opts, uint8_t *sub, int32_t *how, int32_t *bound, double *val,
                       int32_t *lps, int32_t *iters, int mem);

/* qpn_implicit_bounds: `implicit_bounds` (src/sets.jl:660-713) of `polys` polyhedra {x : l <= A x <= u} of one shape, one job per
 * polyhedron: which rows have implicitly equal lower and upper bounds on the polyhedron, and their values.  A [polys][r][d]
 * column-major per item, l, u [polys][r] (+-inf allowed), as for qpn_solve_lps.  Outputs (how, lo, hi, lps, iters, fail_row may be NULL):
 *   status [polys] int32 (QPN_IB_*);  fail_row [polys] int32: the row whose solve ended the polyhedron, -1 without one;
 *   eq [polys][r] uint8: 1 where the row is an (explicit or implicit) equality;  vals [polys][r]: its value there, +inf elsewhere;
 *   how [polys][r] int32 (QPN_IB_HOW_*);  lo, hi [polys][r]: the extremes of a_i'x, -+inf when unbounded, NaN where no LP computed them;
 *   lps [polys] int32: simplex solves started, the feasibility solve counted;  iters [polys] int32: all their steps.
 * Method (polyhedra.implicit_bounds_host is its numpy twin and the normative statement; every output is bit-equal to it, by the
 * discipline of qpn_solve_lps, whose set-up, loop and check it runs):  (0) a row with |l - u| <= tol or l == u is EXPLICIT: eq = 1,
 * val = 0.5 (l + u); no LP takes it as objective.  Another row with l > u makes the polyhedron EMPTY before any LP (lps = 0).
 * (a) steps 1-8 of qpn_solve_lps with c = 0: the crash and phase 1 once per
 * polyhedron; an infeasible all-zero row, or an INFEASIBLE end whose Farkas certificate holds, is EMPTY, a certificate that fails
 * (after step 10's rebuild and second loop) FAILURE, ITER_LIMIT itself; the polyhedron stops there and its other rows keep eq = 0, val = +inf, UNDECIDED.  (b) witnesses: s =
 * A x at the end point on the unscaled rows, columns ascending (acc = acc + a * x); wlo = whi = s, and after every later solve
 * whose certificate holds wlo = s where s < wlo, whi = s where s > whi.  (c) the rows r - 1 ... 0 that are not explicit: whi - wlo
 * > tol is BY_POINTS without an LP; otherwise the minimum, c = +a_i from the current basis (the cost row as in qpn_issubset_pairs
 * (e), fresh step and degeneracy counters, max_iters per objective, the loop, the point, the check of step 9): a certified ray
 * gives lo = -inf, UNBOUNDED; an optimum lo = obj, and whi - lo > tol is BY_POINTS; then the maximum with c = -a_i: hi = -obj or
 * +inf.  eq = lo, hi finite and |lo - hi| <= tol: val = 0.5 (hi + lo), IMPLICIT; else BY_EXTREMES, or UNBOUNDED when one of the two
 * is infinite.  ITER_LIMIT, or an INFEASIBLE end or a failed certificate that step 10's rebuild and second loop do not mend, in
 * one of these solves ends the polyhedron with that status and fail_row = the row.  flags & QPN_IB_ALL_EXTREMES: no BY_POINTS and no early exit after an unbounded minimum; every row that
 * is not explicit gets both extremes and is decided by them alone.
 * Kernel classes are those of qpn_lp_kernel_class(r, d).  1 <= d <= 256, 1 <= r <= 1024 (QPN_ERR_SIZE beyond).  polys == 0 succeeds. */
enum {
    QPN_IB_OK = 0,         /* every row decided */
    QPN_IB_EMPTY = 1,      /* the polyhedron is empty, certified by the Farkas vector */
    QPN_IB_ITER_LIMIT = 2, /* the iteration limit was reached (fail_row: the objective, -1: the feasibility solve) */
    QPN_IB_FAILURE = 3     /* failure, or a certificate that does not hold */
};
enum {
    QPN_IB_HOW_UNDECIDED = 0,   /* the polyhedron ended before the row's turn                       eq = 0 */
    QPN_IB_HOW_EXPLICIT = 1,    /* |l - u| <= tol or l == u                                          eq = 1 */
    QPN_IB_HOW_IMPLICIT = 2,    /* minimum and maximum are finite and within tol                    eq = 1 */
    QPN_IB_HOW_BY_POINTS = 3,   /* two points the solves ended at differ by more than tol           eq = 0 */
    QPN_IB_HOW_BY_EXTREMES = 4, /* minimum and maximum are finite and more than tol apart           eq = 0 */
    QPN_IB_HOW_UNBOUNDED = 5    /* the minimum or the maximum is infinite, certified by a ray       eq = 0 */
};
#define QPN_IB_ALL_EXTREMES 1
int qpn_implicit_bounds(qpn_ctx *ctx, int32_t polys, int32_t r, int32_t d, const double *A, const double *l, const double *u, double tol,
                        int32_t flags, const qpn_lp_opts *opts, int32_t *status, int32_t *fail_row, uint8_t *eq, double *vals, int32_t *how,
                        double *lo, double *hi, int32_t *lps, int32_t *iters, int mem);

/* qpn_irredundant_bounds: which bounds of `polys` polyhedra {x : l <= A x <= u} of one shape their other bounds imply, one job per
 * polyhedron (the reference's `project`, src/sets.jl:501-523, returns the facets of a projected piece; this engine projects by
 * elimination, qpn_reduced_pieces and qpn_project_pieces, and prunes here).  A [polys][r][d] column-major per item, l, u [polys][r]
 * (+-inf allowed), as for qpn_solve_lps.  Outputs (how, ext, lps, iters, fail_row may be NULL):
 *   status [polys] int32 (QPN_IB_OK, _EMPTY, _ITER_LIMIT, _FAILURE);  fail_row [polys] int32: the row whose solve ended the polyhedron,
 *   -1 without one;  lr, ur [polys][r]: l and u with every removed bound at -inf / +inf; where status is not QPN_IB_OK, l and u as given;
 *   how [polys][r][2] int32 (QPN_RED_*), [..][0] the lower bound;  ext [polys][r][2]: the extreme of a_i'x an LP found with the bound
 *   relaxed, -+inf when unbounded, NaN where no LP ran;
 *   lps [polys] int32: simplex solves started, the feasibility solve counted;  iters [polys] int32: all their steps.
 * Method (polyhedra.irredundant_bounds_host is its numpy twin and the normative statement; every output is bit-equal to it, by the
 * discipline of qpn_solve_lps, whose set-up, loop and check it runs).  A bound the others imply shows only with that bound out of
 * the way -- a sum of two facet rows is tight exactly where both are, so its extreme over the whole set equals its bound -- hence
 * the test relaxes the bound it tests, and a removed bound stays removed for every later test, which keeps one of two equal rows.
 * A row with l > u makes the polyhedron EMPTY before any LP (lps = 0).  (a) steps 1-8 of qpn_solve_lps with c = 0 over the working
 * bounds (the job's lr, ur, filled from l, u): EMPTY, FAILURE, ITER_LIMIT as in qpn_implicit_bounds (a).  (b) the rows r - 1 ... 0,
 * on each the lower bound before the upper: l == u is KEPT_EQUALITY on both sides, no LP; an all-zero row has both bounds
 * REMOVED_ZERO_ROW, no LP; an infinite bound is NONE; any other bound is set to -+inf in the working bounds, unscaled (the check of
 * step 9 reads those) and scaled (the loop reads those), nothing else of the state changing, and c = +a_i (lower) or c = -a_i
 * (upper) is solved from the current basis as in qpn_implicit_bounds (c).  (c) a certified ray: KEPT_UNBOUNDED, ext = -+inf; an
 * optimum, ext = obj (lower) or -obj (upper): ext < l - tol max(1, |l|) (ext > u + tol max(1, |u|)) is KEPT_BY_OPTIMUM, anything
 * else REMOVED and the bound stays infinite.  ITER_LIMIT, or a FAILURE that step 10 does not mend, ends the polyhedron with
 * fail_row = the row.  (d) a kept bound is restored, unscaled and as bound * scale_i; a basic s_i outside it is a phase-1 violation
 * the next solve repairs, a nonbasic s_i whose value lies outside it takes the bound's value.  (e) a polyhedron that does not end
 * OK returns lr = l, ur = u, and its REMOVED / REMOVED_ZERO_ROW verdicts read UNDECIDED again: a finished pruning, or the input.
 * lr, ur must not overlap l, u.  Kernel classes are those of qpn_lp_kernel_class(r, d).  1 <= d <= 256, 1 <= r <= 1024
 * (QPN_ERR_SIZE beyond).  max_iters is per solve.  polys == 0 succeeds. */
enum {
    QPN_RED_UNDECIDED = 0,        /* the polyhedron ended before the bound's turn, or did not end OK    bound as given */
    QPN_RED_NONE = 1,             /* the bound is infinite                                               bound as given */
    QPN_RED_KEPT_EQUALITY = 2,    /* l == u                                                              bound as given */
    QPN_RED_REMOVED_ZERO_ROW = 3, /* an all-zero row of a polyhedron that has a point                    removed        */
    QPN_RED_KEPT_UNBOUNDED = 4,   /* without the bound the row is unbounded on that side, by a ray       bound as given */
    QPN_RED_KEPT_BY_OPTIMUM = 5,  /* without the bound the row passes it by more than tol max(1, |b|)    bound as given */
    QPN_RED_REMOVED = 6           /* without the bound the row stays within tol max(1, |b|) of it        removed        */
};
int qpn_irredundant_bounds(qpn_ctx *ctx, int32_t polys, int32_t r, int32_t d, const double *A, const double *l, const double *u, double tol,
                           const qpn_lp_opts *opts, int32_t *status, int32_t *fail_row, double *lr, double *ur, int32_t *how, double *ext,
                           int32_t *lps, int32_t *iters, int mem);

/* qpn_exemplar_polys: `exemplar` / `isempty` (src/sets.jl:591-655) of `polys` polyhedra {x : l <= A x <= u} of one shape whose
 * bounds may be open, one job per polyhedron.  A [polys][n][d] column-major per item, l, u [polys][n] (+-inf allowed), open_lo,
 * open_hi [polys][n] uint8 (nonzero: that bound is open; NULL: every such bound is closed).  Outputs (how, eps, x, row, lambda,
 * iters may be NULL):
 *   empty [polys] uint8;  how [polys] int32 (QPN_EX_*);  eps [polys]: the optimal slack, NaN for ITER_LIMIT and FAILURE;
 *   x [polys][d]: a member, zeros when the polyhedron is empty or the job ended in ITER_LIMIT or FAILURE;
 *   row [polys] int32: 2 i + side (side 0 = l[i], 1 = u[i]) of the lowest open bound that decided EMPTY_OPEN, -1 otherwise;
 *   lambda [polys][2 n + 1]: the multipliers of the slack LP's rows (below), zeros for ITER_LIMIT and FAILURE;
 *   iters [polys] int32: the steps of the solve.
 * Method (polyhedra.exemplar_polys_host is its numpy twin and the normative statement; every output is bit-equal to it, by the
 * discipline of qpn_solve_lps, whose steps 0-10 it runs):  (a) the slack LP in the variables (x, eps): rows i < n: [a_i, 1] >= l_i;
 * rows n + i: [-a_i, 1] >= -u_i; row 2 n: eps >= -slack_cap; every upper bound +inf; the objective is the last row, eps.  The job
 * writes these rows into its own region of the context workspace -- the host expands nothing -- and solves the LP as qpn_solve_lps
 * solves a job, the data screen of step 0 included: l_i = +inf, u_i = -inf or an entry of A that is not finite is FAILURE.
 * (b) the rule on the certified optimum, eps = its last coordinate:  eps > tol: EMPTY_SLACK.  eps > -tol (the band): a bound
 * is active when it is open, finite (an open flag on an infinite bound is ignored, src/sets.jl:354-356) and its multiplier has
 * |lambda_i| > tol (lower bound of row i) or |lambda_{n+i}| > tol (upper bound); any active bound: EMPTY_OPEN, row = the lowest 2 i +
 * side; none: MEMBER_BAND.  eps <= -tol: MEMBER.  (c) an iteration limit is ITER_LIMIT; every other end that is no certified
 * optimum is FAILURE (the slack LP is feasible and bounded below, so INFEASIBLE and UNBOUNDED cannot be true answers).
 * Kernel classes are those of qpn_lp_kernel_class(2 n + 1, d + 1); a call whose regions exceed the workspace chunk is launched in
 * chunks.  1 <= n <= 511, 1 <= d <= 255 (QPN_ERR_SIZE beyond).  max_iters <= 0: 50 (2 n + d + 2) + 100.  polys == 0 succeeds. */
enum {
    QPN_EX_MEMBER = 0,       /* eps <= -tol: x is a member with slack                                   empty = 0 */
    QPN_EX_MEMBER_BAND = 1,  /* -tol < eps <= tol and no open bound is active: x is a member             empty = 0 */
    QPN_EX_EMPTY_SLACK = 2,  /* eps > tol                                                                empty = 1 */
    QPN_EX_EMPTY_OPEN = 3,   /* -tol < eps <= tol and an open, finite bound is active (row names it)     empty = 1 */
    QPN_EX_ITER_LIMIT = 4,   /* the iteration limit was reached: no answer                               empty = 0 */
    QPN_EX_FAILURE = 5,      /* the data screen, or an end that is no certified optimum: no answer       empty = 0 */
    QPN_EX_NOT_NEAR = 6      /* qpn_exemplar_products: the point is outside the product's closure         empty = 0 */
};
int qpn_exemplar_polys(qpn_ctx *ctx, int32_t polys, int32_t n, int32_t d, const double *A, const double *l, const double *u,
                       const uint8_t *open_lo, const uint8_t *open_hi, double tol, double slack_cap, const qpn_lp_opts *opts,
                       uint8_t *empty, int32_t *how, double *eps, double *x, int32_t *row, double *lambda, int32_t *iters, int mem);

/* qpn_exemplar_products: the emptiness test of the intersection tree (`combine`, src/qp_processing.jl:260-291; src/intersection.jl:66-105:
 * a product of pieces is kept when the current point lies in its closure, :74, and it is not empty, :83) for `products` products of
 * pieces, one job per product.  The pieces are runs of rows of one pool that goes up once: A [rows][d], l, u [rows] (+-inf allowed),
 * open_lo, open_hi [rows] uint8 (NULL: closed), piece_row [pieces + 1] int32 ascending, piece p = the pool rows piece_row[p] ..
 * piece_row[p + 1] - 1 (an empty piece is allowed).  The unit of the pool is the ROW, not the polyhedron, so A is ROW-major: entry c of
 * row i is at i * d + c -- unlike the per-item column-major A of the entries above.  factors [products][k] int32: product t is the
 * intersection of the pieces factors[t][0 .. k - 1] in slot order, -1 = no factor in that slot; its rows are the factors' rows one
 * after the other, `n` in all, the same n for every product of a call (the caller groups by n).  point [points][d], point_of [products]
 * int32: the point whose closure test product t takes; both NULL: no closure test, every product is near.
 * Outputs (how, eps, x, row, lambda, iters may be NULL): near [products] uint8, and empty, how, eps, x [products][d], row, lambda
 * [products][2 n + 1], iters as qpn_exemplar_polys gives them for the polyhedron of the product's n rows; row counts product rows.
 * Method (polyhedra.exemplar_products_host is its numpy twin and the normative statement; every output is bit-equal to it):
 * (a) gather: the job writes the map product row i -> pool row into its own region of the context workspace.  (b) closure test, when
 * point is given: per product row s_i = a_i'p over the ascending columns, acc = acc + a * p, no contraction; the product is near when
 * l_i - point_tol <= s_i and s_i - point_tol <= u_i on every row -- closed relations whatever the open flags.  A product that is not
 * near answers near = 0, how = QPN_EX_NOT_NEAR, empty = 0, eps = NaN, x = 0, lambda = 0, iters = 0 and row = the lowest 2 i + side
 * violated (a comparison with a NaN counts as violated); no LP is started.  (c) otherwise near = 1 and the job runs the method of
 * qpn_exemplar_polys on the n gathered rows and their flags: it writes the slack LP of 2 n + 1 rows in d + 1 variables into its region
 * and solves it; the rule, the outputs and the codes are those of QPN_EX_*.  (d) a product is bad when a factor is outside [-1, pieces),
 * when a factor's piece_row entries are not 0 <= first <= last <= rows, when its factors' rows do not add up to n, or when its point_of
 * is outside [0, points).  Host arrays: QPN_ERR_ARG.  Device arrays: that product answers near = 0, empty = 0, QPN_EX_FAILURE, eps =
 * NaN, row = -1, zeros elsewhere, and nothing is read through the bad index.
 * Kernel classes are those of qpn_lp_kernel_class(2 n + 1, d + 1); a call whose regions exceed the workspace chunk is launched in
 * chunks.  1 <= n <= 511, 1 <= d <= 255, 1 <= k <= 32 (QPN_ERR_SIZE beyond).  max_iters <= 0: 50 (2 n + d + 2) + 100.  products == 0
 * succeeds. */
int qpn_exemplar_products(qpn_ctx *ctx, int32_t d, int32_t rows, const double *A, const double *l, const double *u,
                          const uint8_t *open_lo, const uint8_t *open_hi, int32_t pieces, const int32_t *piece_row, int32_t products,
                          int32_t n, int32_t k, const int32_t *factors, int32_t points, const double *point, const int32_t *point_of,
                          double point_tol, double tol, double slack_cap, const qpn_lp_opts *opts, uint8_t *near, uint8_t *empty,
                          int32_t *how, double *eps, double *x, int32_t *row, double *lambda, int32_t *iters, int mem);

/* qpn_intersection_trees: the lazy enumeration of `combine` (src/qp_processing.jl:260-291): IntersectionRoot's tree walk
 * (src/intersection.jl:66-105, :116-138), in which a node of depth t is the intersection of one piece from each of the first t unions
 * and the subtree under an empty prefix is never visited -- for `trees` trees of one depth L over ONE pool of rows, breadth first.
 * The pool is that of qpn_exemplar_products, unchanged: d, rows, A [rows][d] ROW-major, l, u, open_lo, open_hi [rows] (NULL: closed),
 * pieces, piece_row [pieces + 1].  list_ptr [trees L + 1] and list_mem [members] int32 form a CSR: list g L + t holds the pieces of
 * union t of tree g, in the reference's order; its last list_red[g L + t] members are complement pieces (the redzone, :123).  point
 * [points][d], point_of [trees]: the tree's point; both NULL: no closure test.  cap: the most tuples any frontier or any depth's
 * candidates may hold (the caller groups trees by (d, L), as it groups products by (d, n)).
 * Outputs: leaves [cap][L] int32 (pool pieces), leaf_tree, leaf_how [cap] int32 (QPN_EX_*), of which the first n_leaves [1] int64 are
 * written;  tree_leaves [trees] int32;  tested, alive, unanswered [L] int64, one count per depth;  overflow [1] int32.
 * Method (polyhedra.intersection_trees_host is its numpy twin and the normative statement; every output is equal to it):
 * (0) near: a member of a list stays when every row of its piece passes the closure test of qpn_exemplar_products (b) at the tree's
 * point -- ascending columns, acc = acc + a * p, no contraction, closed relations whatever the flags; the order of the rest is kept.
 * near(product) is the AND over its rows, so this is the per-product test bit for bit, and no job takes a point afterwards.
 * (1) expand: F_0 is one empty tuple per tree; for t = 1 .. L the candidates are, for every tuple of F_(t-1) in order and every near
 * member of list t in order, the tuple with that member appended; at t = L a candidate whose members are all complement pieces is not
 * formed (prefixes of complement pieces alone are: a later slot may hold a solution piece).  A candidate is one job of
 * qpn_exemplar_products (c): its tuple as factors, -1 from slot t on, n = its rows.  It is kept when empty == 0; ITER_LIMIT and
 * FAILURE are no answer: the candidate stays alive and is counted in unanswered[t - 1].  F_t is the kept candidates in candidate
 * order; tested[t - 1] and alive[t - 1] are the two counts.  (2) the leaves are F_L in order: by tree, then lexicographic in list
 * positions -- the order `iterate` yields them in.  (3) a depth that forms more than cap candidates ends the call: overflow = that
 * depth (1-based), tested of that depth = the count it formed, later counts 0, n_leaves = 0; the call still returns QPN_OK and the
 * caller falls back.  (4) 1 <= d <= 255, 2 <= L <= 32, 1 <= cap <= 2^22 (QPN_ERR_SIZE beyond); every member piece has at least one
 * row, and per tree the longest pieces of its lists add up to at most 511 rows.  Host arrays: an index out of range, a CSR that is
 * not ascending within list_mem, a member piece of no rows: QPN_ERR_ARG; a sum beyond 511: QPN_ERR_SIZE; nothing is launched.
 * Device arrays: a tree with such a list, a list_red outside its list or a point_of outside [0, points) forms no candidate and
 * answers tree_leaves = -1, the other trees are not affected, and nothing is read through the bad index.  The lists must not overlap
 * in list_mem: list_ptr ascends as a whole within [0, members], and where a device list_ptr does not, EVERY tree of the call answers
 * tree_leaves = -1.
 * The jobs run on the kernels of qpn_exemplar_products, one launch per row count n that a depth's candidates have; the host reads one
 * small header back per depth (the histogram of n and the counts), nothing per launch or per tree.  max_iters <= 0: as there, by
 * the n of each job.  trees == 0 succeeds with every count 0. */
int qpn_intersection_trees(qpn_ctx *ctx, int32_t d, int32_t rows, const double *A, const double *l, const double *u,
                           const uint8_t *open_lo, const uint8_t *open_hi, int32_t pieces, const int32_t *piece_row, int32_t trees,
                           int32_t L, int32_t members, const int32_t *list_ptr, const int32_t *list_mem, const int32_t *list_red,
                           int32_t points, const double *point, const int32_t *point_of, double point_tol, double tol, double slack_cap,
                           const qpn_lp_opts *opts, int32_t cap, int32_t *leaves, int32_t *leaf_tree, int32_t *leaf_how,
                           int64_t *n_leaves, int32_t *tree_leaves, int64_t *tested, int64_t *alive, int64_t *unanswered,
                           int32_t *overflow, int mem);

#ifdef __cplusplus
}
#endif
#endif /* QPN_HIP_H */
