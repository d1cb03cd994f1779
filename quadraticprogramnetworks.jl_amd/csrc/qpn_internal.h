// Internal declarations shared by the HIP translation units of libqpn_hip.so.
#pragma once

#include <hip/hip_runtime.h>
#include <initializer_list>
#include <stddef.h>
#include <stdint.h>

#include "../../include/qpn_hip.h"

// per-node records (qpn_solve_nodes): the solve kernel assembles the KKT blocks on the fly
struct NodeSrc {
    int32_t n, m, p;
    const double *Qd, *R, *qd, *Ad, *B, *l, *u, *w;
    int64_t stride_w;
    int32_t sym;     // 1 = every Qd of these records is bitwise symmetric (known for resident records only)
};

// internal flag bits of AviBatchArgs::flags (above the ABI's QPN_AVI_FLAG_*)
// register kernel only: M is given in the register-block layout of avi_solve_reg<BS> -- lane fastest, [l][k][lane] with BS x BS
// entries per lane, item stride strideM --, every row is a GAVI row, cold start; the kernel then loads its dictionary with
// plain coalesced loads (no LDS staging), and returns z / status / pivots without the post-check (the caller checks on its
// own original blocks)
#define QPN_AVI_IFLAG_BLOCKED_M (1 << 16)
int qpn_avi_reg_block_size(int N);      // BS of the instantiation qpn_launch_avi_solve_reg picks for size N

struct AviBatchArgs {
    int32_t batch;
    int32_t N;
    const double *M;
    int64_t strideM;
    const double *q;
    const double *l;
    const double *u;
    const uint8_t *kind;
    int64_t stride_kind;
    double *z;
    int32_t *status;
    double *resid;
    int32_t *pivots;
    uint8_t *active;
    double check_tol, piv_tol, feas_tol, comp_tol;
    int32_t max_pivots;
    int32_t flags;   // QPN_AVI_FLAG_*
    // optional gate: item b runs only when only_if[b] == only_if_value (others are left untouched)
    const int32_t *only_if;
    int32_t only_if_value;
    // compact form of the gate (register kernel only): scan != 0 launches a SMALL grid whose waves scan
    // only_if[] and solve just the matching items, one after the other; with assemble_first != 0 the
    // item's blocks are first assembled from `nd` into M/q/l/u/kind (the fallback of qpn_solve_nodes).
    int32_t scan;
    int32_t assemble_first;
    // diagnostic builds only (-DQPN_STAMPS): per-item cycle sums per phase, [batch][8] uint64
    unsigned long long *stamps;
    NodeSrc nd;      // used by the fused node path only
    // optional scatter of the primal block z[b][0..nd.n) into x[b * stride_x + i] (qpn_solve_nodes_into)
    double *x;
    int64_t stride_x;
    // replicas of the iterate on peer GPUs (qpn_set_primal_mirrors): every primal block stored to x[off] is
    // also stored to mirror[k][off], k < n_mirror -- plain stores over xGMI, no collective
    int32_t n_mirror;
    double *mirror[QPN_MAX_MIRRORS];
    // optional schedule of the fused node kernel: wavefront i solves node order[i] (a permutation)
    const int32_t *order;
    // optional stride of the per-item vectors (0: N); reduced problems keep their parent's
    int64_t vec_stride;
    // fused node kernel only: counts the items it declines (status = -1), for callers that own the records and
    // want to know whether the general-kernel launch behind it has anything to do (qpn_nodes handles); may be null
    int32_t *decl_count;
    // fused node kernel only: exponentially smoothed pivot count per node (units of 1/32 pivot), updated by every sweep
    // (key <- key - key/32 + pivots); the longest-first order of a resident-records handle is made from it.  May be null.
    int32_t *sched_key;
    // fused node kernel, symmetric n = m = 32 resident records only: the handle's crash cache (kCrashDoubles per node) and its
    // per-node flags (1 = crash passed, 2 = Stage A failed: pivot test, or W~ not finite); crash_mode 0 = not used, 1 = this sweep fills it, 2 = reuses it
    double *crash;
    uint8_t *crash_flag;
    int32_t crash_mode;
    // crash_mode 2 only: a mixed launch.  crash_share = the share of the wavefronts, in 1/256ths, that compute Stage A although the
    // cache is valid (0: every wavefront reuses); crash_reuse_from = the launch position from which every wavefront reuses
    // (the tail of the launch, which no longer saturates HBM).  The results do not depend on either (crash_mix_recomputes).
    int32_t crash_share;
    int32_t crash_reuse_from;
    // crash_mode 2 only: 1 = this sweep fetches the crash cache with non-temporal loads (llc_streams_crash below; read by the
    // launcher alone -- the policy is a template parameter of the kernel)
    int32_t crash_stream;
};

// Wavefronts of the fused 32-class kernel resident at once on an MI355X: 16 per CU (LDS- and VGPR-bound), 256 CUs.
constexpr int kResidentMI355X = 16 * 256;

// Mixed launches of the fused symmetric n = m = 32 kernel: does the wavefront at launch position `pos` (blockIdx.x) compute
// Stage A instead of reusing the cache?  Consecutive workgroup ids go round-robin over the 8 XCDs, so the share is spread over
// the position WITHIN an XCD, k = pos >> 3, by an error-diffusion (Bresenham) rule: position k computes when the running sum
// k * share + phase crosses a multiple of 256.  Any run of L consecutive k of one XCD then holds L * share / 256 computing
// wavefronts to within one.  The phases of the 8 XCDs are the 8 multiples of 32, in bit-reversed order: a row of 8 consecutive
// positions (one k) then holds 8 * share / 256 to within one as well (Hermite's identity), and neighbouring dies do not lead
// each other.  Wave-uniform scalar arithmetic; positions from reuse_from on always reuse.
__host__ __device__ inline bool crash_mix_recomputes(int pos, int share, int reuse_from)
{
    if (pos >= reuse_from) return false;
    const int x = pos & 7, k = pos >> 3;
    const int phase = 32 * (((x & 1) << 2) | (x & 2) | (x >> 2));
    return ((k * share + phase) & 255) + share >= 256;
}

// Crash cache of one symmetric n = m = 32 node, in doubles from the node's base.  U' and S sit in the layout the registers
// have: U' step-major, [8 steps][32 rows] of 4 doubles (what lane < 32 writes to sU in step KB); the three S tiles with register
// g of tile t at ((4 t + g) * 64 + lane), so that every load and store moves 512 contiguous bytes.  W~ sits column by column
// (crash_w_index below).  The node stride is 176 cache lines and kCrashW 64 of them: with the allocation's alignment (hipMalloc:
// at least 256 bytes) every block of a node starts on a 128-byte line.
constexpr int kCrashU = 0, kCrashW = 1024, kCrashS = 2048, kCrashDoubles = 2816;      // 22 528 bytes per node
static_assert(kCrashW % 16 == 0 && kCrashDoubles % 16 == 0, "W~ of every node starts on a 128-byte line");

// W~ (32 x 32) in the crash cache: the offset, in doubles from kCrashW, of entry (row, col).  A column owns its cache lines:
// column j is the 32 doubles from 32 j on, two 128-byte lines, one per row half Ib = row >> 4 -- so a reuse sweep's read-back
// fetches only the columns whose multiplier is not zero.  Inside a line the four tile registers g of one lane group lq (row =
// 16 Ib + 4 g + lq) are neighbours, position 4 lq + g: a lane moves them as one 32-byte piece, at crash_w_index(16 Ib + lq, col).
__host__ __device__ inline int crash_w_index(int row, int col)
{
    const int ib = row >> 4, g = (row >> 2) & 3, lq = row & 3;
    return 32 * col + 16 * ib + 4 * lq + g;
}

// Cache policy of a sweep that reads the crash cache (reuse and mixed launches).  The last-level cache (256 MiB on an MI355X) keeps
// a line from one sweep to the next only while everything loaded or stored in between fits it.  R = what a sweep touches of the
// node records and the outputs, C = the crash cache.  While R + C fits, default loads keep all of it resident; when R alone does
// not fit, nothing can be kept; in between, the crash cache is streamed (non-temporal loads: read once per sweep, not retained) and
// the records stay.  budget_mb: the share of the cache counted on, in MiB (QPN_OPT_LLC_BUDGET_MB; 0 = never stream, negative =
// always).  The default is a tuning constant taken from node-count runs, not the datasheet's 256: a mixed
// sweep reads about half of C (3/8 of its wavefronts compute, and the read-back fetches a third of W~), so with C counted in
// full the lower edge of the window sits where the streamed sweeps start to win only for a budget above the cache's size.  No
// result depends on it.
#ifndef QPN_LLC_BUDGET_MB
#define QPN_LLC_BUDGET_MB 320
#endif
constexpr int kLlcBudgetMB = QPN_LLC_BUDGET_MB;
__host__ inline bool llc_streams_crash(int64_t batch, int64_t n, int64_t m, int64_t p, int64_t budget_mb)
{
    if (budget_mb < 0) return true;
    if (budget_mb == 0) return false;
    const int64_t record = 8 * (n * n + n * p + n + m * n + m * p + 2 * m);      // Qd, R, qd, Ad, B, l, u
    const int64_t outputs = 8 * (n + m) + (n + m) + 4 + 8 + 4 + 8 * n;            // z, active, status, resid, pivots, x
    const int64_t R = batch * (record + outputs), C = batch * (int64_t)kCrashDoubles * 8, budget = budget_mb << 20;
    return R <= budget && budget < R + C;
}

// Function attributes (dynamic LDS limits) are per device: a launcher raises its kernels' limits once per device it is used on,
// through a static QpnLdsLimits:  static QpnLdsLimits lds_limits;  ... lds_limits.raise({{kernel_a, bytes_a}, {kernel_b, bytes_b}})
// sets the attribute kernel by kernel in that order and returns the first error; the device counts as done only once every
// call has succeeded.  (Two host threads racing here both set the same value.)
struct QpnLdsLimit {
    const void *kernel;
    int bytes;
    template <typename K> QpnLdsLimit(K *k, int b) : kernel(reinterpret_cast<const void *>(k)), bytes(b) {}
};
struct QpnLdsLimits {
    bool done[64] = {};
    hipError_t raise(std::initializer_list<QpnLdsLimit> limits)
    {
        int d = 0;
        (void)hipGetDevice(&d);
        d &= 63;
        if (done[d]) return hipSuccess;
        for (const QpnLdsLimit &k : limits) {
            const hipError_t e = hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k.bytes);
            if (e != hipSuccess) return e;
        }
        done[d] = true;
        return hipSuccess;
    }
};


// qpn_avi_big.hip: 64 < N <= 1024, one workgroup per item, dictionary in an HBM workspace
int qpn_avi_big_max_n();
size_t qpn_avi_big_workspace_bytes(int batch, int N);
hipError_t qpn_launch_avi_solve_big(const AviBatchArgs &a, double *workspace, hipStream_t stream);

// A8: nodes with n or m above this take the workgroup kernel verify_wide_node (qpn_verify.hip), the others one wavefront per node
constexpr int QPN_VERIFY_WIDE_FROM = 64;
// ... and the few nodes of the 33 .. 64 class with more than 32 active rows (verify_node64 flags them) take the same kernel out
// of a workspace of this many slots (a device counter hands them out; nodes beyond it go to round 1's kernels)
constexpr int QPN_VERIFY_MID_SLOTS = 256;

// qpn_avi_schur_big.hip: blocked MFMA crash for large node-shaped items (workspace views filled by stage A)
struct SchurBigWs {
    double *Tt, *S, *c, *l2, *u2, *lam;
    int32_t *st2, *piv2, *nsplit, *nred;
    int64_t tt_stride, s_stride;
    int32_t s_rowmajor;      // layout of S (2: already in the Lemke kernel's dictionary, row stride m + 1): row-major for the workgroup Lemke kernel (its dictionary is row-major: no
                             // transposition anywhere), column-major for the kernels that take S as an ABI-layout M
};
size_t qpn_schur_big_workspace_bytes(int batch, int N);
hipError_t qpn_launch_schur_big_stage_a(const AviBatchArgs &a, void *ws, SchurBigWs *out, int s_rowmajor, hipStream_t stream);
hipError_t qpn_launch_schur_big_finish(const AviBatchArgs &a, const SchurBigWs &w, hipStream_t stream);
hipError_t qpn_launch_schur_big_lemke(const AviBatchArgs &a, const SchurBigWs &w, double *dict, hipStream_t stream, int after_bpp = 0);
// symmetric S only; warm = start from the set the multipliers of a.z name (QPN_OPT_WARM_BIG)
hipError_t qpn_launch_schur_big_bpp(const AviBatchArgs &a, const SchurBigWs &w, double *dict, bool warm, hipStream_t stream);

// qpn_avi_schur_big2.hip: the same stage A straight from node records (64 < n <= 256, m <= 256), rank-64 block pivots, one
// workgroup of 16 wavefronts per node; its finish reads the records too.  Same workspace views: the Lemke kernel above runs
// between the two.
bool qpn_schur_big2_shape(int n, int m);
hipError_t qpn_launch_schur_big2_stage_a(const AviBatchArgs &a, void *ws, double *dict, SchurBigWs *out, hipStream_t stream);   // a.nd set
hipError_t qpn_launch_schur_big2_finish(const AviBatchArgs &a, const SchurBigWs &w, hipStream_t stream);

// Crash cache of the large class (QPN_OPT_CRASH_CACHE_BIG; qpn_crash_big.hip): what stage A above makes of Qd and Ad alone, per
// node of a resident handle --
//   tt    the node's top half at its own size, pad16(n) x (pad16(n) + pad16(m) + 16) doubles, tile by tile as stage A lays it
//         out: the C tiles hold W, the H column tiles of pass kb (dead once that pass has formed its multipliers) hold the
//         rank-64 multipliers U' of that pass (register s of row tile I: tile (I, 4 kb + s / 4), doubles (s % 4) 64 + lane), the
//         g tiles are rewritten by every sweep (h of that sweep: the finish kernel reads W | h from here);
//   S     m rows of pad16(m + 1) doubles, the layout stage A writes into the Lemke dictionary;
//   fig   [0] the smallest pivot accepted over all passes, [1] max |M| over the H and C entries (g left out);
//   flag  1 = the node has an entry (its elimination got through in a filling sweep).
struct BigCrash {
    double *tt, *S, *fig;
    uint8_t *flag;
    int64_t tt_stride, s_stride;
};
inline size_t qpn_big_crash_tt_doubles(int n, int m) { return (size_t)((n + 15) & ~15) * (size_t)(((n + 15) & ~15) + ((m + 15) & ~15) + 16); }
inline size_t qpn_big_crash_s_doubles(int m) { return (size_t)m * (size_t)((m + 1 + 15) & ~15); }
// Stage A on a handle with a crash cache: nodes with an entry are replayed (g, h, c, bounds; S copied into the dictionary), and
// when `fill` is set the others run the elimination and the S product in their slot of the cache and leave an entry behind if
// they get through.  Same outputs, bit for bit, as qpn_launch_schur_big2_stage_a.
hipError_t qpn_launch_schur_big2_stage_a_cached(const AviBatchArgs &a, void *ws, double *dict, SchurBigWs *out, const BigCrash &bc,
                                                bool replay, bool fill, hipStream_t stream);
hipError_t qpn_launch_crash_big_replay(const AviBatchArgs &a, const SchurBigWs &w, double *dict, const BigCrash &bc, hipStream_t stream);
// number of nodes with an entry -> *count (device)
hipError_t qpn_launch_crash_big_count(int batch, const uint8_t *flag, int32_t *count, hipStream_t stream);

// qpn_avi_schur_wg.hip: node records with 49 <= max(n, m) <= 64 in ONE fused workgroup kernel (crash, Lemke, read-back, post-check; no workspace)
bool qpn_schur_wg_shape(int n, int m);
hipError_t qpn_launch_schur_wg_nodes(const AviBatchArgs &a, hipStream_t stream);
// one wavefront per node, 33 <= max(n, m) <= 48 (qpn_avi_schur48.hip)
bool qpn_schur48_shape(int n, int m);
hipError_t qpn_launch_avi_solve_schur48_nodes(const AviBatchArgs &a, hipStream_t stream);              // a.nd set; declined nodes keep status -1

// qpn_avi_schur_wg2.hip: the fused workgroup kernel for n, m <= 128 (one of them > 64): two wavefronts per row tile
bool qpn_schur_wg2_shape(int n, int m);
hipError_t qpn_launch_schur_wg2_nodes(const AviBatchArgs &a, hipStream_t stream);             // a.nd set; declined nodes keep status -1

// qpn_avi_schur.hip: MFMA Schur-complement variant for items of shape [free STD x n | GAVI x m]
hipError_t qpn_launch_avi_solve_schur(const AviBatchArgs &a, double *dbgS, double *dbgc, double *dbgW,
                                      double *dbgh, hipStream_t stream);
hipError_t qpn_launch_avi_solve_schur_nodes(const AviBatchArgs &a, hipStream_t stream);   // a.nd set, a.M unused

// qpn_warm.hip: the n, m <= 32 node solve from the active set the multipliers of a.z name (QPN_AVI_FLAG_WARM_DUALS), one wavefront
// per node, ahead of the cold launch.  Accepted nodes write their outputs (pivots = 0); the others write nothing and append their
// index to dec_list -- a.batch + 1 words that the caller has set to -1 (the last one counts) --, which then serves as the cold
// launch's order array: its -1 entries leave their slots unsolved.
hipError_t qpn_launch_warm_nodes(const AviBatchArgs &a, int32_t *dec_list, hipStream_t stream);

// qpn_warm_mid.hip: the same warm start for the mid-size classes (n, m <= 128, one of them > 32; qpn_nodes_set_warm), one
// workgroup per node; accept rule, outputs and decliners' list as above.  The kernel keeps A_act (k x n) and W | h (n x (k + 1))
// in LDS beside kWarmMidFixed bytes of vectors; a hint of k rows that this does not hold declines.  ONE rule, a pure function
// of (n, k) and monotone in k: every k <= min(n, 64) in every shape, every k <= 71 at n = 128.
constexpr int kWarmMidLds = 160 * 1024, kWarmMidFixed = 15648;
__host__ __device__ constexpr bool warm_mid_fits(int n, int k)
{
    return k >= 0 && k <= n && 8 * (k * (n | 1) + n * ((k + 1) | 1)) + kWarmMidFixed <= kWarmMidLds;
}
hipError_t qpn_launch_warm_mid_nodes(const AviBatchArgs &a, int32_t *dec_list, hipStream_t stream);

// qpn_subset.hip: rows between the compact arrays of qpn_solve_nodes_subset_h (slot s = node idx[s], `count` slots) and the
// full-size staging buffers of the handle.
// list: slot_of (batch words) and list (batch + 1 words) arrive filled with -1.  A slot whose entry lies in 0 .. batch - 1 and
// is the first to claim slot_of[entry] (one compare-and-swap) gets list[s] = entry; every other slot is bad and keeps -1.  The
// list is then the order array of the node kernels (its -1 entries leave their launch positions idle) and the row map below.
hipError_t qpn_launch_subset_list(int32_t count, int32_t batch, const int32_t *idx, int32_t *slot_of, int32_t *list,
                                  hipStream_t stream);
// scatter: w row s ([p], item stride stride_w) -> w_full[list[s]], z row s ([N]) -> z_full[list[s]]; a null w or z moves nothing
hipError_t qpn_launch_subset_scatter(int32_t count, const int32_t *list, int32_t p, int32_t N, const double *w, int64_t stride_w,
                                     double *w_full, const double *z, double *z_full, hipStream_t stream);
// gather: the outputs of node list[s] -> slot s, x[s * stride_x + i] = z_full[list[s]][i] (i < n); null outputs (all but status)
// are skipped; a bad slot reads status = QPN_FAILURE and zeros
struct SubsetRows { double *z; int32_t *status; double *resid; int32_t *pivots; uint8_t *active; };
hipError_t qpn_launch_subset_gather(int32_t count, const int32_t *list, int32_t n, int32_t N, const SubsetRows &full,
                                    const SubsetRows &out, double *x, int64_t stride_x, hipStream_t stream);

// qpn_avi_reg.hip
hipError_t qpn_launch_avi_solve(const AviBatchArgs &a, hipStream_t stream);      // dispatcher: Schur kernel, then the register kernel
hipError_t qpn_launch_avi_solve_reg(const AviBatchArgs &a, hipStream_t stream);  // register-tableau kernel
int qpn_avi_max_n();

// qpn_kkt.hip
hipError_t qpn_launch_order_by_pivots(const int32_t *pivots, int32_t count, int32_t *order, hipStream_t stream,
                                      int32_t *key = nullptr);     // key: smoothed counts, see the kernel
// per-sweep status pair, optionally exchanged through the ranks' mailboxes (box[r] = rank r's mailbox as mapped here)
#define QPN_MAX_RANKS (QPN_MAX_MIRRORS + 1)
struct SweepBoxes { void *box[QPN_MAX_RANKS]; };
hipError_t qpn_launch_sweep_status(const int32_t *status, const double *resid, int32_t count, double *out,
                                   int32_t rank, int32_t world, const SweepBoxes &boxes, unsigned long long epoch,
                                   unsigned long long timeout_ticks, hipStream_t stream);
// local pieces (local_piece) and recipe enumeration (all_Ks): all pointers device
// flag[0] = 1 if any Qd block (n x n, column-major, `batch` of them) is not bitwise symmetric; flag[0] is left alone otherwise
hipError_t qpn_launch_qd_asymmetry(int32_t batch, int32_t n, const double *Qd, int32_t *flag, hipStream_t stream);
hipError_t qpn_launch_local_pieces(int32_t batch, int32_t nodes, int32_t n, int32_t m, int32_t p, const double *Qd, const double *R,
                                   const double *qd, const double *Ad, const double *B, const double *l, const double *u,
                                   const int32_t *node_of, const uint8_t *K, double *Ap, double *lp, double *up, uint8_t *keep,
                                   hipStream_t stream);
hipError_t qpn_launch_recipes(int32_t N, const uint8_t *mask, long long first, int32_t count, uint8_t *K, hipStream_t stream);
// qpn_pieces.hip: a level's recipes / pieces with the multipliers eliminated, one call each
hipError_t qpn_launch_recipes_batch(int32_t nodes, int32_t N, const uint8_t *masks, const long long *offsets, long long total, uint8_t *K,
                                    int32_t *node_of, hipStream_t stream, const long long *first = nullptr);
size_t qpn_reduce_pieces_lds(int32_t n, int32_t m, int32_t p);
// qpn_finish.hip: the finishing step of the pieces (normalise + member / merge / key, duplicates, compacted store)
hipError_t qpn_launch_finish_norm(int32_t pieces, int32_t oc, int32_t cap, const double *Ar, const double *lr, const double *ur,
                                  const int32_t *rows, const int32_t *flags, const int32_t *rec_of, const int32_t *ncols, const int32_t *take,
                                  const double *xk, const double *probe, double member_tol, double *rsc, double *rdiv, double *Ln, double *Un,
                                  int32_t *status, double *worst, unsigned long long *hash, int32_t *dup_of, hipStream_t stream);
hipError_t qpn_launch_finish_dup(int32_t cnt, const int32_t *ord, const int32_t *pos, const int32_t *run0, int32_t oc, int32_t cap, const double *Ar,
                                 const int32_t *rows, const int32_t *rec_of, const int32_t *ncols, const int32_t *take, const double *rsc,
                                 const double *rdiv, const double *Ln, const double *Un, int32_t *status, int32_t *dup_of, hipStream_t stream);
hipError_t qpn_launch_finish_store(int32_t stored, const int32_t *src, int32_t oc, int32_t cap, const double *Ar, const int32_t *rows,
                                   const int32_t *rec_of, const int32_t *ncols, const int32_t *take, const double *rsc, const double *rdiv,
                                   const double *Ln, const double *Un, double *As, double *ls, double *us, int32_t *rows_s, hipStream_t stream);
hipError_t qpn_launch_reduce_pieces(int32_t pieces, int32_t n, int32_t m, int32_t p, double tol, double *Ap, const double *lp,
                                    const double *up, const uint8_t *keep, double *Ar, double *lr, double *ur, int32_t *rows_out,
                                    int32_t *flags_out, hipStream_t stream);
// qpn_project.hip: the pieces reduce_pieces_kernel would flag, projected by Fourier-Motzkin steps (qpn_project_pieces).  buf, bnd, lists:
// qpn_project_pieces_scratch bytes per piece (2 cap cols doubles, 4 cap doubles, 5 cap ints).  A call is split into chunks of
// pieces whose local pieces and scratch fit kProjectWsBytes of the context's workspace.
constexpr int kProjectLdsMax = 64 * 1024;
constexpr size_t kProjectWsBytes = (size_t)512 << 20;
size_t qpn_project_pieces_lds(int32_t n, int32_t m, int32_t p);
size_t qpn_project_pieces_scratch(int32_t n, int32_t m, int32_t p, int32_t cap);
hipError_t qpn_launch_project_pieces(int32_t pieces, int32_t n, int32_t m, int32_t p, double tol, int32_t cap, double *Ap, const double *lp,
                                     const double *up, const uint8_t *keep, double *buf, double *bnd, int32_t *lists, double *Ar,
                                     double *lr, double *ur, int32_t *rows_out, int32_t *flags_out, hipStream_t stream);
// pool assembly (combine_gavis): all pointers device
struct QpnPoolLaunch {
    int32_t batch, form, nd, sn, sm, p;
    const int32_t *xi_owner, *xi_dpos, *con_owner, *dec_src;
    const double *Qd, *Qp, *qd, *Ad, *Bp, *l, *u, *w;
    int64_t s_Qd, s_Qp, s_qd, s_Ad, s_Bp, s_lu, s_w;
    double *M, *q, *lo, *hi; uint8_t *kind;
    int64_t s_M;
};
hipError_t qpn_launch_assemble_pools(const QpnPoolLaunch &L, hipStream_t stream);
hipError_t qpn_launch_check_avi(int32_t batch, int32_t N, const double *M, int64_t strideM,
                                const double *q, const double *l, const double *u,
                                const uint8_t *kind, int64_t stride_kind, const double *z,
                                double tol, int32_t *degree, double *r, hipStream_t stream);
hipError_t qpn_launch_comp_indices(int64_t count, const double *zv, const double *rv,
                                   const double *l, const double *u, double tol, int32_t shift,
                                   uint8_t *mask, hipStream_t stream);
hipError_t qpn_launch_assemble_nodes(int32_t batch, int32_t n, int32_t m, int32_t p,
                                     const double *Qd, const double *R, const double *qd,
                                     const double *Ad, const double *B, const double *l,
                                     const double *u, const double *w, int64_t stride_w,
                                     double *Mout, double *qout, double *lout, double *uout,
                                     uint8_t *kind_out, hipStream_t stream,
                                     const int32_t *only_if = nullptr, int32_t only_if_value = 0);
hipError_t qpn_launch_verify_nodes(int32_t batch, int32_t n, int32_t m, int32_t p,
                                   const double *Qd, const double *R, const double *qd,
                                   const double *Ad, const double *B, const double *l,
                                   const double *u, const double *xd, const double *w,
                                   int64_t stride_w, double tol, int32_t *solution, double *lambda,
                                   int32_t *path, double *sG, double *sq, double *slb, double *sub,
                                   double *sz, double *sres, int32_t *sst, hipStream_t stream,
                                   double *wbig = nullptr,       // wbig: large-item AVI workspace (m > 64 only)
                                   double *gws = nullptr);       // gws: [batch][2][pad16(m)^2] Gram block / factor of verify_wide_node (n or m > 64)
// The list form (qpn_verify_nodes_subset_h): `count` slots, slot s verifies record list[s] of the nrec records (device list;
// entries outside [0, nrec) answer path 6).  xd, w, the outputs and every scratch array are compact: sized by count.
hipError_t qpn_launch_verify_nodes_list(int32_t count, const int32_t *list, int32_t nrec, int32_t n, int32_t m, int32_t p,
                                        const double *Qd, const double *R, const double *qd,
                                        const double *Ad, const double *B, const double *l,
                                        const double *u, const double *xd, const double *w,
                                        int64_t stride_w, double tol, int32_t *solution, double *lambda,
                                        int32_t *path, double *sG, double *sq, double *slb, double *sub,
                                        double *sz, double *sres, int32_t *sst, hipStream_t stream,
                                        double *wbig = nullptr, double *gws = nullptr);
int qpn_verify_max_dim();

// qpn_convexity.hip: check_qp_convexity for a batch of nodes (n <= 256, m <= 1024); gws: qpn_convexity_workspace_bytes
hipError_t qpn_launch_convexity(int32_t batch, int32_t n, int32_t m, const double *Qd, const double *Ad, const uint8_t *eq,
                                double tol, int32_t *convex, double *min_eig, int32_t *null_dim, void *gws, hipStream_t stream);
size_t qpn_convexity_workspace_bytes(int32_t batch, int32_t n, int32_t m);
hipError_t qpn_launch_multiplier_vertices(int32_t batch, int32_t n, int32_t m, const double *E, const double *g, const uint8_t *cls,
                                          const double *lam0, int32_t V, int32_t max_bases, double tol, double feas, double *verts,
                                          int32_t *count, int32_t *status, void *ws, hipStream_t s);
size_t qpn_multiplier_vertices_workspace_bytes(int32_t batch, int32_t n, int32_t m, int32_t max_bases);
hipError_t qpn_launch_recipe_filter(int32_t pieces, int32_t N, const uint8_t *masks, const uint8_t *K, const int32_t *vrow_of,
                                    const int32_t *first_of, int32_t rows, uint8_t *keep, hipStream_t s);
// qpn_members.hip: interior-member node records made on the device, the members taken from the solve, members against pieces
hipError_t qpn_launch_interior_records(int32_t batch, int32_t r, int32_t d, const double *A, const double *l, const double *u, double delta,
                                       int32_t ne, int32_t nlo, int32_t nhi, double *Qd, double *qd, double *Ad, double *lo, double *uo,
                                       uint8_t *flag, hipStream_t s);
size_t qpn_interior_records_lds(int32_t r);
hipError_t qpn_launch_members_extract(int32_t batch, int32_t d, int32_t N, const double *z, const int32_t *status, const uint8_t *flag,
                                      double *x, uint8_t *ok, hipStream_t s);
hipError_t qpn_launch_members_outside(int32_t pairs, int32_t d, int32_t rj, const double *Aj, const double *lj, const double *uj, int32_t Bj,
                                      const double *X, int32_t Bi, const int32_t *pi, const int32_t *pj, double t, uint8_t *out, hipStream_t s);
size_t qpn_members_lists_lds(int32_t rj, int32_t d);
hipError_t qpn_launch_members_outside_lists(int32_t d, int32_t rj, const double *Aj, const double *lj, const double *uj, int32_t Bj,
                                            const double *X, const uint8_t *ok, int32_t Bi, int32_t lists, const int32_t *list_ptr,
                                            const int32_t *list_mem, const int32_t *list_of, const int32_t *self_pos,
                                            const int64_t *word_ptr, double t, uint32_t *bits, int32_t *undecided, hipStream_t s);
#define QPN_MEMBERS_MAX_ROWS 4096
// qpn_parent.hip: inner-node records from a static store, a pool of child pieces and column maps (qpn_assemble_parent_nodes).
// Pointers are device pointers; map_bad [maps] uint8 is scratch the launch fills first.
struct ParentArgs {
    int32_t items, form, n0, ne, m, p;
    int32_t parents, mb, ps;
    const double *sQd, *sR, *sqd, *sAd, *sB, *sl, *su;
    const int32_t *mb_true;
    int32_t pieces, pool_rows, pool_words;
    const int32_t *piece_desc;
    const double *pA, *pl, *pu;
    int32_t maps, map_words;
    const int32_t *map_off, *map_data;
    const int32_t *parent_of, *piece_of, *map_of;
    uint8_t *map_bad;
    double *Qd, *R, *qd, *Ad, *B, *l, *u;
    int32_t *err;
};
#define QPN_PARENT_MAX_ROWS 1024
hipError_t qpn_launch_parent_records(const ParentArgs &a, hipStream_t s);

// qpn_lp.hip: the batched LP solver (qpn_solve_lps).  Pointers are device pointers; x, obj, lam, ray, iters may be null.
struct LpTol {                                 // the resolved tolerances of an entry's solves
    double piv_tol, feas_tol, opt_tol, check_tol;
    int32_t max_iters;                         // > 0, per objective
};
struct LpArgs {
    int32_t polys, r, d, jobs;
    const double *A, *l, *u;
    const int32_t *poly_of;
    const double *cost;                        // [jobs][d], or null: obj_sign[t] * row obj_row[t] of the job's polyhedron
    const int32_t *obj_row, *obj_sign;
    int32_t *status;
    double *x, *obj, *lam, *ray;
    int32_t *iters;
    LpTol lp;
};
#define QPN_LP_MAX_D 256
#define QPN_LP_MAX_R 1024
int qpn_lp_class(int32_t r, int32_t d);        // 0 wavefront, 1 workgroup in LDS, 2 workgroup over the workspace, -1 beyond the limits
size_t qpn_lp_workspace_bytes(int32_t jobs, int32_t r, int32_t d);
hipError_t qpn_launch_solve_lps(const LpArgs &a, void *gws, hipStream_t s);
// ... and the subset tests over it (qpn_issubset_pairs).  how, bound, val, lps, iters may be null.
struct SubsetArgs {
    int32_t d, B1, r1, B2, r2, pairs;
    const double *A1, *l1, *u1, *A2, *l2, *u2;
    const int32_t *pi, *pj;
    double tol;
    uint8_t *sub;
    int32_t *how, *bound;
    double *val;
    int32_t *lps, *iters;
    LpTol lp;
};
hipError_t qpn_launch_issubset_pairs(const SubsetArgs &a, void *gws, hipStream_t s);   // gws: qpn_lp_workspace_bytes(pairs, r1, d)
// ... and the implicit bounds of polyhedra (qpn_implicit_bounds), one job per polyhedron.  how, lo, hi, lps, iters, fail_row may be null.
struct IbArgs {
    int32_t polys, r, d, flags;
    const double *A, *l, *u;
    double tol;
    int32_t *status, *fail_row;
    uint8_t *eq;
    double *vals;
    int32_t *how;
    double *lo, *hi;
    int32_t *lps, *iters;
    LpTol lp;
};
hipError_t qpn_launch_implicit_bounds(const IbArgs &a, void *gws, hipStream_t s);     // gws: qpn_lp_workspace_bytes(polys, r, d)
// ... and the bounds of polyhedra that their other bounds imply (qpn_irredundant_bounds), one job per polyhedron.  lr, ur are the
// job's working bounds while it runs.  how, ext, lps, iters, fail_row may be null.
struct RedArgs {
    int32_t polys, r, d;
    const double *A, *l, *u;
    double tol;
    int32_t *status, *fail_row;
    double *lr, *ur;
    int32_t *how;                              // [polys][r][2]
    double *ext;                               // [polys][r][2]
    int32_t *lps, *iters;
    LpTol lp;
};
hipError_t qpn_launch_irredundant_bounds(const RedArgs &a, void *gws, hipStream_t s); // gws: qpn_lp_workspace_bytes(polys, r, d)
// ... and the emptiness of polyhedra with open bounds (qpn_exemplar_polys), one job per polyhedron over its slack LP of 2 n + 1 rows
// in d + 1 variables.  open_lo, open_hi null: closed;  how, eps, x, row, lam, iters may be null.
struct ExArgs {
    int32_t polys, n, d;
    const double *A, *l, *u;
    const uint8_t *open_lo, *open_hi;
    double tol, slack_cap;
    uint8_t *empty;
    int32_t *how;
    double *eps, *x;
    int32_t *row;
    double *lam;
    int32_t *iters;
    LpTol lp;
    int32_t first;                             // set by the launcher: the polyhedron of a launch's job 0, and where the jobs'
    unsigned char *rows;                       // regions of expanded rows start
};
#define QPN_EX_MAX_N 511
#define QPN_EX_MAX_D 255
size_t qpn_exemplar_workspace_bytes(int32_t polys, int32_t n, int32_t d);
hipError_t qpn_launch_exemplar_polys(const ExArgs &a, void *gws, hipStream_t s);      // gws: qpn_exemplar_workspace_bytes(polys, n, d)
// ... and of products of pieces (qpn_exemplar_products), one job per product: the factors' rows, n in all, gathered from a pool of
// rows (A [rows][d] ROW-major) into the job's slack LP.  open_lo, open_hi null: closed;  point, point_of null: no closure test;
// how, eps, x, row, lam, iters may be null.
struct ProdArgs {
    int32_t d, rows, pieces, products, n, k, points;
    const double *A, *l, *u;
    const uint8_t *open_lo, *open_hi;
    const int32_t *piece_row, *factors;
    const double *point;
    const int32_t *point_of;
    double point_tol, tol, slack_cap;
    uint8_t *near, *empty;
    int32_t *how;
    double *eps, *x;
    int32_t *row;
    double *lam;
    int32_t *iters;
    LpTol lp;
    int32_t first;                             // set by the launcher, as in ExArgs
    unsigned char *regions;
};
#define QPN_PROD_MAX_K 32
size_t qpn_products_workspace_bytes(int32_t products, int32_t n, int32_t d);
hipError_t qpn_launch_exemplar_products(const ProdArgs &a, void *gws, hipStream_t s); // gws: qpn_products_workspace_bytes(products, n, d)
// qpn_tree.hip: the intersection tree of combine, breadth first (qpn_intersection_trees): the frontier machinery around the jobs of
// qpn_launch_exemplar_products.  Pointers are device pointers; open_lo, open_hi, point and point_of may be null.  lp.max_iters <= 0:
// the default of the LP entries, per job size.
struct TreeArgs {
    int32_t d, rows, pieces, trees, L, members, points, cap;
    const double *A, *l, *u;
    const uint8_t *open_lo, *open_hi;
    const int32_t *piece_row, *list_ptr, *list_mem, *list_red;
    const double *point;
    const int32_t *point_of;
    double point_tol, tol, slack_cap;
    LpTol lp;
    int32_t *leaves, *leaf_tree, *leaf_how;    // [cap][L], [cap], [cap]
    long long *n_leaves;                       // [1]
    int32_t *tree_leaves;                      // [trees]
    long long *tested, *alive, *unanswered;    // [L] each
    int32_t *overflow;                         // [1]
};
#define QPN_TREE_MAX_L 32
#define QPN_TREE_MAX_CAP (1 << 22)
size_t qpn_tree_workspace_bytes(int32_t trees, int32_t L, int32_t members, int32_t cap, int32_t d);
// The whole walk on stream s: one read-back of a depth's histogram and counts per depth, and the stream's work is done when it returns
// only as far as those read-backs need (the outputs are ordered on s like any kernel's).  ws: qpn_tree_workspace_bytes(...).
hipError_t qpn_run_intersection_trees(const TreeArgs &a, void *ws, hipStream_t s);
#define QPN_CONVEXITY_MAX_N 256
#define QPN_CONVEXITY_MAX_M 1024

// ---- wave64 helpers (CDNA4: one wavefront = 64 lanes) --------------------------------
#ifdef __HIPCC__
constexpr int WAVE = 64;
#define QINF __builtin_huge_val()

typedef double d4 __attribute__((ext_vector_type(4)));
#define MFMA(a_, b_, c_) __builtin_amdgcn_mfma_f64_16x16x4f64((a_), (b_), (c_), 0, 0, 0)
// D = C - A B: on gfx950 the BLGP field of the fp64 MFMAs holds NEG modifiers (bit 0: A, bit 1: B, bit 2: C;
// tools/mfma_neg_probe.hip), so an operand's sign costs no VALU instruction
#define MFMA_NEGA(a_, b_, c_) __builtin_amdgcn_mfma_f64_16x16x4f64((a_), (b_), (c_), 0, 0, 1)

// diagnostic builds (-DQPN_STAMPS): a kernel declares its clocks with STAMP_DECL; STAMP(slot) adds the clocks since the previous
// stamp to stamp_acc[slot]; where the sums go is each kernel's own business
#ifdef QPN_STAMPS
#define STAMP_DECL                                                      \
    unsigned long long stamp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};         \
    unsigned long long stamp_last = __builtin_amdgcn_s_memtime()
#define STAMP(slot)                                                     \
    do {                                                                \
        unsigned long long now__ = __builtin_amdgcn_s_memtime();        \
        __builtin_amdgcn_s_waitcnt(0xC07F);                             \
        stamp_acc[slot] += now__ - stamp_last;                          \
        stamp_last = now__;                                             \
    } while (0)
#else
#define STAMP_DECL (void)0      // (not an empty do-while: even that changes the code generated around it)
#define STAMP(slot) do { } while (0)
#endif

// (A5+A6) reduced single-node KKT assembly of item b by ONE wavefront (src/avi.jl:205-251 + :305-377):
// M = [[Qd, -Ad'],[Ad, 0]] column-major, q = [qd + R w; B w], bounds [free; l..u], kinds [STD; GAVI].
// Column j of M (length N = n+m) is written by lanes striding the rows: coalesced.
__device__ __forceinline__ void qpn_assemble_item(const NodeSrc &nd, int b, int lane, double *Mout,
                                                  double *qout, double *lout, double *uout,
                                                  uint8_t *kind_out)
{
    const int n = nd.n, m = nd.m, p = nd.p, N = n + m;
    const double *Q_ = nd.Qd + (size_t)b * n * n;
    const double *A_ = nd.Ad + (size_t)b * m * n;
    const double *R_ = nd.R + (size_t)b * n * p;
    const double *B_ = nd.B + (size_t)b * m * p;
    const double *w_ = nd.w + (size_t)b * (size_t)nd.stride_w;
    double *Mo = Mout + (size_t)b * N * N;
    const size_t vo = (size_t)b * (size_t)N;
    // columns 0..n-1: [Qd(:,j) ; Ad(:,j)]
    for (int j = 0; j < n; ++j)
        for (int i = lane; i < N; i += 64)
            Mo[(size_t)j * N + i] = i < n ? Q_[(size_t)j * n + i] : A_[(size_t)j * m + (i - n)];
    // columns n..N-1: [-Ad(c,:)' ; 0]
    for (int c = 0; c < m; ++c)
        for (int i = lane; i < N; i += 64)
            Mo[(size_t)(n + c) * N + i] = i < n ? -A_[(size_t)i * m + c] : 0.0;
    for (int i = lane; i < N; i += 64) {
        double s;
        if (i < n) {
            s = nd.qd[(size_t)b * n + i];
            for (int k = 0; k < p; ++k) s = fma(R_[(size_t)k * n + i], w_[k], s);
            lout[vo + i] = -__builtin_huge_val(); uout[vo + i] = __builtin_huge_val(); kind_out[vo + i] = QPN_ROW_STD;
        } else {
            const int r = i - n;
            s = 0.0;
            for (int k = 0; k < p; ++k) s = fma(B_[(size_t)k * m + r], w_[k], s);
            lout[vo + i] = nd.l[(size_t)b * m + r]; uout[vo + i] = nd.u[(size_t)b * m + r];
            kind_out[vo + i] = QPN_ROW_GAVI;
        }
        qout[vo + i] = s;
    }
}

__device__ __forceinline__ double udbl(double v);
// ---- DPP / readlane based wave64 primitives (no LDS round trips) -------------------------
// dpp_ctrl encodings (GFX9): quad_perm = 0x00..0xFF, row_half_mirror = 0x141, row_mirror = 0x140
template <int CTRL> __device__ __forceinline__ double dpp_f64(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    // every source lane of the row patterns used here is valid, so `old` is irrelevant: mov_dpp
    // (old = undef) saves the two register copies update_dpp(old = v) costs
    lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xF, 0xF, true);
    hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
// value of `v` in lane `l`; l must be wave-uniform (it is turned into an SGPR)
__device__ __forceinline__ double readlane_f64(double v, int l)
{
    l = __builtin_amdgcn_readfirstlane(l);
    int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ int readlane_i32(int v, int l)
{
    return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(l));
}
// Keeps a wave-uniform value in scalar registers across a join: an empty asm with a scalar in/out operand.  The compiler
// selects the phi of a uniform value into SGPRs and then moves it into VGPRs -- with every phi that feeds it, a copy at each
// join and a v_readfirstlane in front of each scalar use -- when one of its inputs is a vector register or more than one of its
// uses wants a vector operand (the VGPR copy in front of a v_readfirstlane counts).  Behind keep_scalar the phi has ONE use, the
// asm, and what follows reads the asm's result, which is no phi.  No instruction is issued.  (An input that is a vector register
// after all -- the undefined value the structurizer puts into the join phis of a double is one -- is no silent fallback: the
// build stops with "illegal VGPR to SGPR copy".)
__device__ __forceinline__ void keep_scalar(int &x) { asm volatile("" : "+s"(x)); }
__device__ __forceinline__ void keep_scalar(unsigned long long &x) { asm volatile("" : "+s"(x)); }
// v with lane `lane` (wave-uniform) replaced by the wave-uniform value `x`: v_writelane_b32, no
// compare/select.  (No clang builtin on this toolchain, hence asm; gfx9 allows one SGPR per VALU instruction, so the lane
// select goes through M0 (saved and restored: the compiler owns M0); the s_nop covers the wait states between the SALU write of M0 / a VALU-written
// data SGPR and their use, which the hazard recognizer cannot see through inline asm.)
__device__ __forceinline__ int writelane_i32(int v, int lane, int x)
{
    const int xs = __builtin_amdgcn_readfirstlane(x), ls = __builtin_amdgcn_readfirstlane(lane);
    int m0save;
    asm("s_mov_b32 %1, m0\n\ts_mov_b32 m0, %3\n\ts_nop 3\n\tv_writelane_b32 %0, %2, m0\n\ts_mov_b32 m0, %1"
        : "+v"(v), "=&s"(m0save) : "s"(xs), "s"(ls));
    return v;
}
__device__ __forceinline__ double writelane_f64(double v, int lane, double x)
{
    const int ls = __builtin_amdgcn_readfirstlane(lane);
    const int xl = __builtin_amdgcn_readfirstlane(__double2loint(x)), xh = __builtin_amdgcn_readfirstlane(__double2hiint(x));
    int lo = __double2loint(v), hi = __double2hiint(v);
    int m0save;
    asm("s_mov_b32 %2, m0\n\ts_mov_b32 m0, %5\n\ts_nop 3\n\tv_writelane_b32 %0, %3, m0\n\tv_writelane_b32 %1, %4, m0\n\t"
        "s_mov_b32 m0, %2"
        : "+v"(lo), "+v"(hi), "=&s"(m0save) : "s"(xl), "s"(xh), "s"(ls));
    return __hiloint2double(hi, lo);
}
#define QPN_ROW_REDUCE(v, OP)                                  \
    do {                                                       \
        double o__;                                            \
        o__ = dpp_f64<0xB1>(v); v = OP(v, o__); /* quad_perm [1,0,3,2] */ \
        o__ = dpp_f64<0x4E>(v); v = OP(v, o__); /* quad_perm [2,3,0,1] */ \
        o__ = dpp_f64<0x141>(v); v = OP(v, o__); /* row_half_mirror */    \
        o__ = dpp_f64<0x140>(v); v = OP(v, o__); /* row_mirror      */    \
    } while (0)
__device__ __forceinline__ double qpn_max2(double a, double b) { return fmax(a, b); }  // v_max_f64
__device__ __forceinline__ double qpn_min2(double a, double b) { return fmin(a, b); }  // v_min_f64
// NaN-free inputs assumed by callers (they feed -1 / +inf sentinels for inactive lanes)
__device__ __forceinline__ double wave_max_f64(double v)
{
    QPN_ROW_REDUCE(v, qpn_max2);
    double r0 = readlane_f64(v, 0), r1 = readlane_f64(v, 16), r2 = readlane_f64(v, 32), r3 = readlane_f64(v, 48);
    return udbl(qpn_max2(qpn_max2(r0, r1), qpn_max2(r2, r3)));
}
__device__ __forceinline__ double wave_min_f64(double v)
{
    QPN_ROW_REDUCE(v, qpn_min2);
    double r0 = readlane_f64(v, 0), r1 = readlane_f64(v, 16), r2 = readlane_f64(v, 32), r3 = readlane_f64(v, 48);
    return udbl(qpn_min2(qpn_min2(r0, r1), qpn_min2(r2, r3)));
}
// min over lanes 0..31 only (two DPP rows); lanes 32..63 are ignored
__device__ __forceinline__ double wave_min32_f64(double v)
{
    QPN_ROW_REDUCE(v, qpn_min2);
    double r0 = readlane_f64(v, 0), r1 = readlane_f64(v, 16);
    return qpn_min2(r0, r1);
}
// v_min_f64 without the canonicalising v_max the compiler puts in front of fmin() (callers feed no NaNs).
// The asm carries no wait states of its own: the compiler's hazard recogniser treats the VGPR an asm block defines like
// any VALU result and puts the wait states in front of the DPP move or v_readlane that reads it (2 and 1 on gfx950).  An
// s_nop inside the asm only doubled them.  This is a property of the toolchain, not a guarantee of the ISA: with another
// compiler, dump every unit that uses these helpers (tools/isa.sh on qpn_avi_schur, _wg, _wg2) and see in the listing that
// an s_nop 1 stands between each of these v_min_f64 and a v_mov_b32_dpp of its result, an s_nop 0 in front of a v_readlane;
// if one is missing, the s_nop 1 goes back into the asm.
__device__ __forceinline__ double min_f64_nc(double a, double b)
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// the same with a wave-uniform second operand (an SGPR pair)
__device__ __forceinline__ double min_f64_nc_s(double a, double bs)
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "s"(bs));
    return r;
}
// v_max_f64 without the canonicalising v_max x, x the compiler puts in front of each operand of fmax() (the same toolchain
// property as min_f64_nc above, and the same listing check).  For operands that are COMPUTED values and never NaNs: the
// result of an fp64 add, subtract or |.| of one, a constant, or a NaN already replaced by a select.  On such operands the
// canonicalisation is the identity (it only quiets signalling NaNs; fp64 denormals are kept), so both forms give the same bits.
__device__ __forceinline__ double max_f64_nc(double a, double b)
{
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// wave_max_f64 for such operands, wave-uniform result: the four row stages, then the rows cross as in
// wave_min64_with_limit_f64 (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3) and lane 63 is read out --
// 6 v_max_f64 and 2 v_readlane where fmax() and four row read-outs cost 7 + 14 v_max_f64, 8 v_readlane and their copies.
// A maximum does not depend on the order of its operands, so the other crossing gives the same bits.
__device__ __forceinline__ double wave_max_f64_nc(double v)
{
    v = max_f64_nc(v, dpp_f64<0xB1>(v));
    v = max_f64_nc(v, dpp_f64<0x4E>(v));
    v = max_f64_nc(v, dpp_f64<0x141>(v));
    v = max_f64_nc(v, dpp_f64<0x140>(v));
    {
        int lo = __double2loint(v), hi = __double2hiint(v);
        lo = __builtin_amdgcn_update_dpp(lo, lo, 0x142, 0xA, 0xF, false);      // rows 1, 3 <- lane 15 of rows 0, 2
        hi = __builtin_amdgcn_update_dpp(hi, hi, 0x142, 0xA, 0xF, false);
        v = max_f64_nc(v, __hiloint2double(hi, lo));
    }
    {
        int lo = __double2loint(v), hi = __double2hiint(v);
        lo = __builtin_amdgcn_update_dpp(lo, lo, 0x143, 0xC, 0xF, false);      // rows 2, 3 <- lane 31
        hi = __builtin_amdgcn_update_dpp(hi, hi, 0x143, 0xC, 0xF, false);
        v = max_f64_nc(v, __hiloint2double(hi, lo));
    }
    return readlane_f64(v, 63);
}
// min over lanes 0..31, returned in EVERY lane 0..31 (lanes 32..63 get the min of their own half):
// four DPP row stages + one ds_swizzle (lane ^ 16, on the LDS crossbar) -- no v_readlane, no SGPR detour
__device__ __forceinline__ double wave_min32_all_f64(double v)
{
    v = min_f64_nc(v, dpp_f64<0xB1>(v));
    v = min_f64_nc(v, dpp_f64<0x4E>(v));
    v = min_f64_nc(v, dpp_f64<0x141>(v));
    v = min_f64_nc(v, dpp_f64<0x140>(v));
    const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(v), 0x401F);
    const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(v), 0x401F);
    return min_f64_nc(v, __hiloint2double(hi, lo));
}
// the same minimum with the row crossing through v_readlane (two SGPR pairs) instead of the LDS crossbar: a few
// more instructions, but ~100 cycles less latency -- for loops whose waves wait on dependent chains, not on issue
__device__ __forceinline__ double wave_min32_all_lowlat_f64(double v)
{
    v = min_f64_nc(v, dpp_f64<0xB1>(v));
    v = min_f64_nc(v, dpp_f64<0x4E>(v));
    v = min_f64_nc(v, dpp_f64<0x141>(v));
    v = min_f64_nc(v, dpp_f64<0x140>(v));
    return min_f64_nc(readlane_f64(v, 0), readlane_f64(v, 16));
}
// min over lanes 0..31 of v and the wave-uniform `lim`, returned wave-uniform (it lands in an SGPR pair): four DPP row
// stages, then row 0's minimum crosses into row 1 with row_bcast:15 (gfx9 DPP: lane 15 of a row to every lane of the next
// one) and lane 31 is read out -- 2 DPP moves + 2 v_readlane for the crossing instead of 4 v_readlane + 4 v_mov; `lim`
// rides in as one v_min with a scalar operand before the stages instead of a v_mov + v_min after them
// (_s: `lim` is an SGPR pair already and goes in as it is)
__device__ __forceinline__ double wave_min32_with_limit_s_f64(double v, double lim)
{
    v = min_f64_nc_s(v, lim);
    v = min_f64_nc(v, dpp_f64<0xB1>(v));
    v = min_f64_nc(v, dpp_f64<0x4E>(v));
    v = min_f64_nc(v, dpp_f64<0x141>(v));
    v = min_f64_nc(v, dpp_f64<0x140>(v));
    {
        // rows 1 and 3 receive lane 15 of rows 0 and 2 (row_mask 0xa)
        int lo = __double2loint(v), hi = __double2hiint(v);
        lo = __builtin_amdgcn_mov_dpp(lo, 0x142, 0xA, 0xF, false);      // (rows 0, 2 of the result are undefined: only lane 31 is read)
        hi = __builtin_amdgcn_mov_dpp(hi, 0x142, 0xA, 0xF, false);
        v = min_f64_nc(v, __hiloint2double(hi, lo));
    }
    return readlane_f64(v, 31);
}
__device__ __forceinline__ double wave_min32_with_limit_f64(double v, double lim) { return wave_min32_with_limit_s_f64(v, udbl(lim)); }
// min over all 64 lanes of v and the wave-uniform `lim`, returned wave-uniform: four DPP row stages, row_bcast:15 into rows
// 1 and 3, row_bcast:31 into rows 2 and 3, lane 63 read out (callers feed no NaNs; non-candidates carry +inf)
__device__ __forceinline__ double wave_min64_with_limit_f64(double v, double lim)
{
    v = min_f64_nc_s(v, udbl(lim));
    v = min_f64_nc(v, dpp_f64<0xB1>(v));
    v = min_f64_nc(v, dpp_f64<0x4E>(v));
    v = min_f64_nc(v, dpp_f64<0x141>(v));
    v = min_f64_nc(v, dpp_f64<0x140>(v));
    {
        int lo = __double2loint(v), hi = __double2hiint(v);
        lo = __builtin_amdgcn_update_dpp(lo, lo, 0x142, 0xA, 0xF, false);      // rows 1, 3 <- lane 15 of rows 0, 2
        hi = __builtin_amdgcn_update_dpp(hi, hi, 0x142, 0xA, 0xF, false);
        v = min_f64_nc(v, __hiloint2double(hi, lo));
    }
    {
        int lo = __double2loint(v), hi = __double2hiint(v);
        lo = __builtin_amdgcn_update_dpp(lo, lo, 0x143, 0xC, 0xF, false);      // rows 2, 3 <- lane 31
        hi = __builtin_amdgcn_update_dpp(hi, hi, 0x143, 0xC, 0xF, false);
        v = min_f64_nc(v, __hiloint2double(hi, lo));
    }
    return readlane_f64(v, 63);
}
__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// lane mask of a predicate.  HIP's __ballot(p) compares int(p) with 0: the compiler materialises the flag in a VGPR and
// compares it again (v_cndmask + v_cmp_ne per ballot); the builtin takes the i1 as it is -- the compare that produced
// the predicate IS the mask
__device__ __forceinline__ unsigned long long qpn_ballot(bool pred) { return __builtin_amdgcn_ballot_w64(pred); }
// lowest lane whose predicate holds, or -1 (wave-uniform result)
__device__ __forceinline__ int wave_first(bool pred)
{
    unsigned long long b = qpn_ballot(pred);
    return b ? (__ffsll((long long)b) - 1) : -1;
}
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
// Tell the compiler a value is wave-uniform (moves it to SGPRs): branches on it become scalar.
__device__ __forceinline__ bool ubool(bool v) { return __builtin_amdgcn_readfirstlane((int)v) != 0; }
__device__ __forceinline__ double udbl(double v)
{
    int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
    int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
// Ordering among the lanes of ONE wavefront: LDS operations of a wave execute in issue order, so ordering between a lane's
// store and another lane's load needs no s_barrier and no drain of the memory counters -- only that the compiler keeps the
// program order of the LDS accesses (it must: they may alias) and does not move them across this point.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// 1/x (callers guarantee |x| is well away from 0 on every lane whose result is used).  v_rcp_f64 is good to
// 4.6e-8; one Newton step brings it to <= 2.3e-15 relative (10 ulp), two give the correctly rounded quotient
// (tools/rcp_probe.hip).  The pivoting arithmetic uses one step: its results are certified by the post-check
// on the original blocks, and 1e-15 is far inside the 1e-9 parity bar.
__device__ __forceinline__ double rcp64(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    const double e = fma(-x, r, 1.0);
    return fma(r, e, r);
}
// max(a, |b|) in ONE instruction (fmax(a, fabs(b)) costs three: the compiler canonicalises both operands first; the
// callers feed no NaNs that matter: a NaN entry fails the pivot test and the item goes to the general kernel)
__device__ __forceinline__ double max_abs_nc(double a, double b)
{
    double r;
    asm("v_max_f64 %0, %1, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double min_abs_nc(double a, double b)      // min(a, |b|)
{
    double r;
    asm("v_min_f64 %0, %1, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// v[l] + v[l ^ 32] in every lane (gfx950: v_permlane32_swap exchanges the upper half of one register with the lower half of another)
__device__ __forceinline__ double sum_halves(double v)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const auto c = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto d = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return __hiloint2double(d[0], c[0]) + __hiloint2double(d[1], c[1]);
}
// v + (v of lane ^ 16) + (v of lane ^ 32) + (v of lane ^ 48): gfx950's row / half swaps (VALU, no LDS trip, no address registers)
__device__ __forceinline__ double xsum_rows(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    const double s = __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
    lo = __double2loint(s); hi = __double2hiint(s);
    const auto c = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto d = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return __hiloint2double(d[0], c[0]) + __hiloint2double(d[1], c[1]);
}
// lane id recomputed on the spot (v_mbcnt on the full EXEC mask; opaque, so the compiler does not keep the copy from the
// start of the kernel alive -- and spill it -- across the phases): every phase derives its own lane coordinates
__device__ __forceinline__ int lane_id_fresh()
{
    int x = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    asm volatile("" : "+v"(x));
    return x;
}
__device__ __forceinline__ int pad16(int v) { return (v + 15) & ~15; }

// ---- the epilogue every solver kernel shares ---------------------------------------------------------------------------------
// THE row post-check: one row with primal part p, dual part d (STD row: p = z_k, d = (M z + q)_k; GAVI row: the other way
// round) and bounds l <= u.  What a solve reports as status, resid and active[] is made of these and of nothing else; each kernel
// only maps rows to lanes and reduces the count and the residual over its wavefront or workgroup.
//   QPN_ROW_VIOLATIONS   adds the violated conditions of check_avi_solution (src/avi.jl:148-156) to `bad`: a count, check_avi
//                        returns its sum as the degree
//   QPN_ROW_RESIDUAL     e = the natural-map residual |p - clamp(p - d, l, u)|, a NaN replaced by +inf
//   QPN_ROW_MASK         mask = the comp_indices mask (src/avi_solutions.jl:511-562), bit c - 1 for code c, before any shift
//   QPN_ROW_POSTCHECK    the three of a solver row, in that order; the mask of a GAVI row is shifted by 4 (:587-612)
// Function-like macros for the reason STAMP and QPN_ROW_REDUCE are: the 32-class kernel (qpn_avi_schur.hip) is generated around
// these statements, and behind a __forceinline__ function -- returning a struct or writing through references alike -- its
// code is scheduled otherwise and the sweep of the benchmark loses 0.3 % (profiles/postcheck_ab.txt); pasted, the unit's code is
// the one it was (profiles/postcheck_kernel_resources.md).  The arguments are plain variables or constants: they are evaluated
// more than once.  level_batch.node_postcheck restates the macros in numpy; tests/test_postcheck_host.py wraps them in a host
// program and compares them with that twin and with the oracle.
//
// qpn_approx: x == y, or both finite and within ct (isapprox with atol = ct).  An infinite operand makes |x - y| infinite (or
// NaN for inf - inf, which the first clause has already taken), so the finiteness tests of the scalar statement are implied.
// PRECONDITION: ct (comp_tol) is finite -- with ct = +inf an infinite |x - y| would pass.
__host__ __device__ __forceinline__ bool qpn_approx(double x, double y, double ct) { return (x == y) | (fabs(x - y) <= ct); }
#define QPN_ROW_VIOLATIONS(bad, p, d, l, u, tol)                                              \
    do {                                                                                      \
        if ((d) > (tol) && fabs((p) - (l)) > (tol)) (bad)++;    /* :152 */                    \
        if ((d) < -(tol) && fabs((p) - (u)) > (tol)) (bad)++;   /* :153 */                    \
        if ((p) - (l) < -(tol)) (bad)++;                        /* :154 */                    \
        if ((p) - (u) > (tol)) (bad)++;                                                       \
        if (isnan(p) || isnan(d)) (bad)++;                                                    \
    } while (0)
#define QPN_ROW_RESIDUAL(e, p, d, l, u)                                                       \
    do {                                                                                      \
        double tt__ = (p) - (d);                                                              \
        if (tt__ < (l)) tt__ = (l);                                                           \
        if (tt__ > (u)) tt__ = (u);                                                           \
        (e) = fabs((p) - tt__);                                                               \
        if (isnan(e)) (e) = QINF;                                                             \
    } while (0)
#define QPN_ROW_MASK(mask, p, d, l, u, ct)                                                    \
    do {                                                                                      \
        (mask) = 0;                                                                           \
        if (!qpn_approx(l, u, ct)) {                                               /* :512 */ \
            if (qpn_approx(p, l, ct) && (d) >= -(ct)) (mask) |= 1u;                /* :543 */ \
            if ((l) - (ct) <= (p) && (p) <= (u) + (ct) && fabs(d) <= (ct)) (mask) |= 2u;      \
            if (qpn_approx(p, u, ct) && (d) <= (ct)) (mask) |= 4u;                 /* :549 */ \
        } else (mask) = 8u;                                                    /* :552-558 */ \
    } while (0)
#define QPN_ROW_POSTCHECK(bad, e, mask, p, d, l, u, gavi, check_tol, comp_tol)                \
    do {                                                                                      \
        const double tol__ = (check_tol);                                                     \
        QPN_ROW_VIOLATIONS(bad, p, d, l, u, tol__);                                           \
        QPN_ROW_RESIDUAL(e, p, d, l, u);                                                      \
        const double ct__ = (comp_tol);                                                       \
        QPN_ROW_MASK(mask, p, d, l, u, ct__);                                                 \
        if (gavi) (mask) <<= 4;                                                               \
    } while (0)

// Primal store: entry xo of the caller's iterate and of its replicas on the peer GPUs (AviBatchArgs::mirror).  `args` points at
// the kernel's AviBatchArgs wherever the kernel reads the mirror table from: the kernarg segment, or its by-value argument.
template <typename ArgsPtr> __device__ __forceinline__ void qpn_store_primal(ArgsPtr args, double *x, size_t xo, double v)
{
    x[xo] = v;
    const int nmir = args->n_mirror;
    for (int k = 0; k < nmir; ++k) args->mirror[k][xo] = v;
}

// Smoothed pivot count of a node (AviBatchArgs::sched_key, units of 1/32 pivot): key <- key - key / 32 + pivots, a first
// sweep starts it at 32 * pivots.
__host__ __device__ __forceinline__ int qpn_smooth_pivots(int key, int pivots) { return key > 0 ? key - (key >> 5) + pivots : 32 * pivots; }
__device__ __forceinline__ void qpn_update_sched_key(int32_t *sched_key, int b, int pivots)
{
    if (sched_key) sched_key[b] = qpn_smooth_pivots(sched_key[b], pivots);
}

// THE decline rules; the host protocol of qpn_capi_nodes.hip rests on every kernel doing exactly this, in ONE thread of the
// wavefront or workgroup that owns node b.
// Cold: a fused kernel hands node b to the general kernels -- status -1, counted for the owner of the records (decl_count may be null).
__device__ __forceinline__ void qpn_decline_cold(int32_t *status, int b, int32_t *decl_count)
{
    status[b] = -1;
    if (decl_count) atomicAdd(decl_count, 1);
}
// Warm: a warm kernel writes nothing but b, appended to the decliners' list.  The list starts at -1 in every word, its counter
// (the word behind it) included: slot = old count + 1.
__device__ __forceinline__ void qpn_decline_warm(int32_t *dec_list, int32_t *dec_count, int b)
{
    dec_list[atomicAdd(dec_count, 1) + 1] = b;
}

// sixteen-way scalar dispatch on a wave-uniform index %[cs] (0..15; anything else: nothing) inside an asm statement: leaf k
// names register k statically
#define DISPATCH16(P, L0, L1, L2, L3, L4, L5, L6, L7, L8, L9, L10, L11, L12, L13, L14, L15)                                        \
    /* (numeric local labels, all referenced forwards: the compiler may duplicate an asm statement -- loop peeling --, and named  \
        labels would then be defined twice; P only documents the call site) */                                                     \
    "s_cmp_gt_u32 %[cs], 7\n\ts_cbranch_scc1 20f\n\t"                                                                             \
    "s_cmp_gt_u32 %[cs], 3\n\ts_cbranch_scc1 4f\n\t"                                                                              \
    "s_cmp_gt_u32 %[cs], 1\n\ts_cbranch_scc1 2f\n\t"                                                                              \
    "s_cmp_eq_u32 %[cs], 0\n\ts_cbranch_scc0 1f\n\t"                                                                              \
    L0 "\n\ts_branch 30f\n"                                                                                                        \
    "1:\n\t" L1 "\n\ts_branch 30f\n"                                                                                              \
    "2:\n\ts_cmp_eq_u32 %[cs], 2\n\ts_cbranch_scc0 3f\n\t" L2 "\n\ts_branch 30f\n"                                              \
    "3:\n\t" L3 "\n\ts_branch 30f\n"                                                                                              \
    "4:\n\ts_cmp_gt_u32 %[cs], 5\n\ts_cbranch_scc1 6f\n\t"                                                                       \
    "s_cmp_eq_u32 %[cs], 4\n\ts_cbranch_scc0 5f\n\t" L4 "\n\ts_branch 30f\n"                                                    \
    "5:\n\t" L5 "\n\ts_branch 30f\n"                                                                                              \
    "6:\n\ts_cmp_eq_u32 %[cs], 6\n\ts_cbranch_scc0 7f\n\t" L6 "\n\ts_branch 30f\n"                                              \
    "7:\n\t" L7 "\n\ts_branch 30f\n"                                                                                              \
    "20:\n\ts_cmp_gt_u32 %[cs], 15\n\ts_cbranch_scc1 30f\n\t"                                                                    \
    "s_cmp_gt_u32 %[cs], 11\n\ts_cbranch_scc1 12f\n\t"                                                                            \
    "s_cmp_gt_u32 %[cs], 9\n\ts_cbranch_scc1 10f\n\t"                                                                             \
    "s_cmp_eq_u32 %[cs], 8\n\ts_cbranch_scc0 9f\n\t" L8 "\n\ts_branch 30f\n"                                                    \
    "9:\n\t" L9 "\n\ts_branch 30f\n"                                                                                              \
    "10:\n\ts_cmp_eq_u32 %[cs], 10\n\ts_cbranch_scc0 11f\n\t" L10 "\n\ts_branch 30f\n"                                         \
    "11:\n\t" L11 "\n\ts_branch 30f\n"                                                                                            \
    "12:\n\ts_cmp_gt_u32 %[cs], 13\n\ts_cbranch_scc1 14f\n\t"                                                                    \
    "s_cmp_eq_u32 %[cs], 12\n\ts_cbranch_scc0 13f\n\t" L12 "\n\ts_branch 30f\n"                                                 \
    "13:\n\t" L13 "\n\ts_branch 30f\n"                                                                                            \
    "14:\n\ts_cmp_eq_u32 %[cs], 14\n\ts_cbranch_scc0 15f\n\t" L14 "\n\ts_branch 30f\n"                                         \
    "15:\n\t" L15 "\n"                                                                                                            \
    "30:\n\t"
#endif
