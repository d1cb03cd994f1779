"""Host wrapper over the C-ABI (include/qpn_hip.h): one ``Engine`` = one ``qpn_ctx`` on one GPU.

Buffers may be numpy arrays (host; the library stages them through HBM) or torch CUDA tensors
(device; zero-copy, asynchronous on torch's current stream: a tensor has to be of the ABI's element type for its argument,
contiguous and on the engine's device, see ``Engine._stage``).  All matrix buffers are in the
ABI layout: per item COLUMN-MAJOR (Julia), i.e. a ``(batch, N, N)`` array ``Mc`` holds
``Mc[b, j, i] = M_b[i, j]``.  ``colmajor()`` converts from the usual math layout.

There is no CPU path here: every method ends in a HIP kernel launch or raises.
"""
from __future__ import annotations

import collections
import ctypes as C
import time

import numpy as np

from . import _lib
from ._lib import MEM_DEVICE, MEM_HOST, AviOpts, LpOpts

try:  # torch is plumbing (device memory, streams, torch.distributed), not a requirement to import
    import torch
except Exception:  # pragma: no cover
    torch = None


class QpnError(RuntimeError):
    pass


def colmajor(M):
    """(..., rows, cols) math-layout array -> same data in the ABI's column-major layout."""
    if torch is not None and isinstance(M, torch.Tensor):
        return M.transpose(-1, -2).contiguous()
    return np.ascontiguousarray(np.swapaxes(np.asarray(M, dtype=np.float64), -1, -2))


def _torch_dt(dt):
    return {np.dtype(np.int32): torch.int32, np.dtype(np.float64): torch.float64, np.dtype(np.uint8): torch.uint8}[np.dtype(dt)]


_DTYPES = dict(f64="float64", u8="uint8", i32="int32", i64="int64")      # Engine._stage's groups: the ABI's element types, by numpy / torch name


def _is_dev(x):
    return torch is not None and isinstance(x, torch.Tensor) and x.is_cuda


def _ptr(x):
    if x is None:
        return None
    if torch is not None and isinstance(x, torch.Tensor):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(x.ctypes.data)


class Engine:
    """One context on one GPU.  ``device`` is a HIP device ordinal."""

    def __init__(self, device: int = 0, use_torch_stream: bool = True):
        self.lib = _lib.load_library()
        self.device = int(device)
        h = C.c_void_p()
        rc = self.lib.qpn_ctx_create(self.device, C.byref(h))
        if rc != 0:
            raise QpnError(f"qpn_ctx_create({device}) failed: {self.lib.qpn_strerror(rc).decode()}")
        self.ctx = h
        self.use_torch_stream = use_torch_stream
        self.calls = collections.Counter()       # C-ABI calls per entry point (the tests assert O(1) calls per level with it)
        self.seconds = collections.Counter()     # wall time per entry point, method entry to the library's return (host-pointer
        self._t0 = None                          # calls are synchronous, so this is staging + kernels + read-back)
        self._bound = "own"                      # which stream the context launches on (a new context: its own)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.qpn_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # -- helpers ---------------------------------------------------------------------------
    def _chk(self, rc, what):
        self.calls[what] += 1
        if self._t0 is not None:
            self.seconds[what] += time.perf_counter() - self._t0
            self._t0 = None
        if rc != 0:
            msg = self.lib.qpn_ctx_last_error(self.ctx).decode()
            raise QpnError(f"{what}: {self.lib.qpn_strerror(rc).decode()} ({msg})")

    def _bind_stream(self, dev):
        # device buffers: launch on torch's current stream so torch ops before/after the call are
        # ordered with the kernels (cuda_stream == 0 is the legacy default stream, a real stream)
        if dev and self.use_torch_stream:
            s = torch.cuda.current_stream(self.device).cuda_stream
            if s != self._bound:                 # (the binding call is skipped while the stream stays what it was)
                # the binding is cached only once the library has accepted it (the call synchronises the old stream and can fail)
                self._bound = None
                self._call("qpn_ctx_set_stream", C.c_void_p(s))
                self._bound = s
        elif not dev:
            if self._bound != "own":
                self._bound = None
                self._call("qpn_ctx_use_own_stream")
                self._bound = "own"
        self._t0 = time.perf_counter()

    def _call(self, name, *args):
        """Entry point `name` of the library on this context; counted, and a failure raised, under that one name."""
        self._chk(getattr(self.lib, name)(self.ctx, *args), name)

    @staticmethod
    def _mem(dev):
        return MEM_DEVICE if dev else MEM_HOST

    def synchronize(self):
        self._call("qpn_ctx_synchronize")

    def default_opts(self) -> AviOpts:
        o = AviOpts()
        self.lib.qpn_avi_default_opts(C.byref(o))
        return o

    def _stage(self, who, names, raw=(), **typed):
        """The buffers of one call of method `who`, grouped by the element type the ABI declares for them (f64=, u8=, i32=;
        None allowed anywhere; `names` names them, in the same order, for the error message).  Host or device is decided over
        all of them and `raw` (buffers with a rule of their own, left to the caller), never a mix; the stream is bound; host
        buffers become contiguous arrays of their type.  Device tensors go to the kernels as raw addresses, so they have to be
        what the ABI says they are already: that dtype, contiguous, on the engine's device.  Returns [dev, *buffers]."""
        devs = [_is_dev(a) for g in (raw, *typed.values()) for a in g if a is not None]
        if any(devs) and not all(devs):
            raise QpnError("mixing host and device buffers in one call")
        dev = bool(devs and devs[0])
        self._bind_stream(dev)
        staged = [dev]
        for kind, group in typed.items():
            dt = getattr(torch if dev else np, _DTYPES[kind])
            for a in group:
                if a is not None:
                    if not dev:
                        a = np.ascontiguousarray(a, dtype=dt)
                    elif a.dtype != dt or not a.is_contiguous() or a.device.index != self.device:
                        raise QpnError(f"{who}: {names.split()[len(staged) - 1]} must be a contiguous {_DTYPES[kind]} tensor on "
                                       f"cuda:{self.device}")
                staged.append(a)
        return staged

    @staticmethod
    def _x_stride(x_out, dev, batch, n):
        if x_out is None:
            return 0
        if dev:
            if x_out.dtype != torch.float64 or x_out.dim() != 2 or x_out.shape[0] != batch or x_out.shape[1] < n \
                    or x_out.stride(1) != 1:
                raise ValueError("x_out must be a [batch, >= n] fp64 tensor with unit inner stride")
            return x_out.stride(0)
        if x_out.dtype != np.float64 or x_out.ndim != 2 or x_out.shape[0] != batch or x_out.shape[1] < n \
                or x_out.strides[1] != 8:
            raise ValueError("x_out must be a [batch, >= n] float64 array with unit inner stride")
        return x_out.strides[0] // 8

    def upload_nodes(self, Qc, Rc, qd, Ac, Bc, l, u) -> "Nodes":
        """Make a level's node records resident (qpn_nodes_upload); see ``Nodes``."""
        return Nodes(self, Qc, Rc, qd, Ac, Bc, l, u)

    def _alloc(self, dev, shape, dtype):
        if dev:
            tdt = {np.float64: torch.float64, np.int32: torch.int32, np.uint8: torch.uint8, np.int64: torch.int64,
                   np.uint32: torch.uint32}[dtype]
            return torch.empty(shape, dtype=tdt, device=f"cuda:{self.device}")
        return np.empty(shape, dtype=dtype)

    # -- (A2+A3+A9) ------------------------------------------------------------------------
    def solve_avi_batch(self, Mc, q, l, u, z0=None, kind=None, opts=None, want_active=True, out=None):
        """Batched AVI solve; replaces PATHSolver.solve_mcp (src/avi.jl:64-70) per item.

        Mc: (batch, N, N) column-major per item, or (N, N) shared.  q, l, u: (batch, N).
        kind: None | (N,) shared | (batch, N) uint8.  z0 = None is a cold start (z0 = 0, handled in
        the kernel: no reset pass).  `out` may carry the dict of a previous call to reuse its
        buffers.  Returns dict(z, status, resid, pivots, active).
        """
        dev, Mc, q, l, u, z0, kind = self._stage("solve_avi_batch", "Mc q l u z0 kind", f64=(Mc, q, l, u, z0), u8=(kind,))
        batch, N = q.shape
        strideM = 0 if Mc.ndim == 2 else N * N
        sk = 0 if (kind is None or kind.ndim == 1) else N
        res, o = self._solve_outputs(dev, batch, N, z0, opts, want_active, out)
        self._call("qpn_solve_avi_batch", batch, N, _ptr(Mc), strideM, _ptr(q), _ptr(l), _ptr(u), _ptr(kind), sk, _ptr(res["z"]),
                   _ptr(res["status"]), _ptr(res["resid"]), _ptr(res["pivots"]), _ptr(res["active"]), C.byref(o), self._mem(dev))
        return res

    def _solve_outputs(self, dev, batch, N, z0, opts, want_active, out):
        """The result dict of a solve (`out`'s buffers when its z has the right shape, else new ones) and its options: z starts
        from z0, or cold -- the kernel's own cold start under the default options, zeros under the caller's."""
        o = opts if opts is not None else self.default_opts()
        if out is not None and out["z"].shape == (batch, N):
            res = {k: out[k] for k in ("z", "status", "resid", "pivots", "active")}
        else:
            res = dict(z=self._alloc(dev, (batch, N), np.float64), status=self._alloc(dev, (batch,), np.int32),
                       resid=self._alloc(dev, (batch,), np.float64), pivots=self._alloc(dev, (batch,), np.int32),
                       active=self._alloc(dev, (batch, N), np.uint8) if want_active else None)
        if z0 is None:
            if opts is None:
                o.flags |= _lib.AVI_FLAG_COLD_START
            elif dev:
                res["z"].zero_()
            else:
                res["z"][...] = 0.0
        elif dev:
            res["z"].copy_(z0)
        else:
            res["z"][...] = z0
        return res, o

    def solve_mcp_csc(self, N, colptr, rowval, nzval, q, l, u, z0, opts=None):
        """One box-MCP in Julia's SparseMatrixCSC{Float64,Int32} layout (1-based): the argument
        list of PATHSolver.solve_mcp at src/avi.jl:64.  Returns (status, z, info)."""
        colptr = np.ascontiguousarray(colptr, dtype=np.int32)
        rowval = np.ascontiguousarray(rowval, dtype=np.int32)
        nzval = np.ascontiguousarray(nzval, dtype=np.float64)
        q, l, u = (np.ascontiguousarray(a, dtype=np.float64) for a in (q, l, u))
        z = np.array(z0, dtype=np.float64, copy=True)
        st, res, piv = C.c_int32(0), C.c_double(0), C.c_int32(0)
        o = opts if opts is not None else self.default_opts()
        self._call("qpn_solve_mcp_csc", int(N), _ptr(colptr), _ptr(rowval), _ptr(nzval), _ptr(q), _ptr(l), _ptr(u), _ptr(z),
                   C.byref(st), C.byref(res), C.byref(piv), C.byref(o))
        return int(st.value), z, dict(resid=res.value, pivots=piv.value)

    # -- (A3) ------------------------------------------------------------------------------
    def check_avi_batch(self, Mc, q, l, u, z, kind=None, tol=1e-6, want_r=True):
        dev, Mc, q, l, u, z, kind = self._stage("check_avi_batch", "Mc q l u z kind", f64=(Mc, q, l, u, z), u8=(kind,))
        batch, N = q.shape
        strideM = 0 if Mc.ndim == 2 else N * N
        sk = 0 if (kind is None or kind.ndim == 1) else N
        degree = self._alloc(dev, (batch,), np.int32)
        r = self._alloc(dev, (batch, N), np.float64) if want_r else None
        self._call("qpn_check_avi_batch", batch, N, _ptr(Mc), strideM, _ptr(q), _ptr(l), _ptr(u), _ptr(kind), sk, _ptr(z),
                   float(tol), _ptr(degree), _ptr(r), self._mem(dev))
        return degree, r

    # -- (A9) ------------------------------------------------------------------------------
    def comp_indices(self, zv, rv, l, u, tol=1e-2, shift=0):
        dev, zv, rv, l, u = self._stage("comp_indices", "zv rv l u", f64=(zv, rv, l, u))
        count = int(np.prod(zv.shape))
        mask = self._alloc(dev, tuple(zv.shape), np.uint8)
        self._call("qpn_comp_indices", count, _ptr(zv), _ptr(rv), _ptr(l), _ptr(u), float(tol), int(shift), _ptr(mask),
                   self._mem(dev))
        return mask

    # -- (A5+A6) ---------------------------------------------------------------------------
    def assemble_nodes(self, Qc, Rc, qd, Ac, Bc, l, u, w, out=None):
        """Per-node reduced KKT blocks.  Qc (batch,n,n), Rc (batch,p,n), Ac (batch,n,m),
        Bc (batch,p,m): all column-major per item (see ``colmajor``); w (p,) shared or (batch,p).
        `out` may carry the tuple of a previous call to reuse its buffers."""
        dev, Qc, Rc, qd, Ac, Bc, l, u, w = self._stage("assemble_nodes", "Qc Rc qd Ac Bc l u w", f64=(Qc, Rc, qd, Ac, Bc, l, u, w))
        batch, n = qd.shape
        m = l.shape[1]
        p = w.shape[-1]
        sw = 0 if w.ndim == 1 else p
        N = n + m
        if out is not None and out[1].shape == (batch, N):
            Mout, qout, lout, uout, kind = out
        else:
            Mout = self._alloc(dev, (batch, N, N), np.float64)
            qout = self._alloc(dev, (batch, N), np.float64)
            lout = self._alloc(dev, (batch, N), np.float64)
            uout = self._alloc(dev, (batch, N), np.float64)
            kind = self._alloc(dev, (batch, N), np.uint8)
        self._call("qpn_assemble_nodes", batch, n, m, p, _ptr(Qc), _ptr(Rc), _ptr(qd), _ptr(Ac), _ptr(Bc), _ptr(l), _ptr(u), _ptr(w),
                   sw, _ptr(Mout), _ptr(qout), _ptr(lout), _ptr(uout), _ptr(kind), self._mem(dev))
        return Mout, qout, lout, uout, kind

    # -- (F1) local pieces ------------------------------------------------------------------------
    def recipes_from_masks(self, mask, first=0, count=None):
        """all_Ks (src/avi_solutions.jl:200-215) from one solution's active-set masks (uint8 per row of z): recipes number
        first .. first+count-1 of the Cartesian product of the rows' code sets.  Returns (K [count, N] uint8, total)."""
        dev, mask = self._stage("recipes_from_masks", "mask", u8=(mask,))
        N = int(mask.shape[0])
        total = C.c_int64(0)
        self._call("qpn_recipes_from_masks", N, _ptr(mask), 0, 0, None, C.byref(total), self._mem(dev))
        tot = int(total.value)
        if count is None:
            count = tot - first
        K = self._alloc(dev, (count, N), np.uint8)
        self._call("qpn_recipes_from_masks", N, _ptr(mask), int(first), int(count), _ptr(K), None, self._mem(dev))
        return K, tot

    def local_pieces(self, Qc, Rc, qd, Ac, Bc, l, u, K, node_of=None):
        """local_piece (src/avi_solutions.jl:400-496, before simplify) for recipes K [pieces, n+m] over node records in the
        ABI layout (as solve_nodes); node_of [pieces] int32 names each recipe's node (default: recipe t <-> node t).
        Returns (Ap [pieces, N+p, 2N] column-major per piece, lp, up [pieces, 2N], keep [pieces, 2N] uint8)."""
        dev, Qc, Rc, qd, Ac, Bc, l, u, K, node_of = self._stage("local_pieces", "Qc Rc qd Ac Bc l u K node_of",
                                                                f64=(Qc, Rc, qd, Ac, Bc, l, u), u8=(K,), i32=(node_of,))
        nodes, n = qd.shape
        m = l.shape[1]
        p = Rc.shape[1]
        N = n + m
        pieces = int(K.shape[0])
        Ap = self._alloc(dev, (pieces, N + p, 2 * N), np.float64)
        lp = self._alloc(dev, (pieces, 2 * N), np.float64)
        up = self._alloc(dev, (pieces, 2 * N), np.float64)
        keep = self._alloc(dev, (pieces, 2 * N), np.uint8)
        self._call("qpn_local_pieces", pieces, nodes, n, m, p, _ptr(Qc), _ptr(Rc), _ptr(qd), _ptr(Ac), _ptr(Bc), _ptr(l), _ptr(u),
                   _ptr(node_of), _ptr(K), _ptr(Ap), _ptr(lp), _ptr(up), _ptr(keep), self._mem(dev))
        return Ap, lp, up, keep

    # -- (F1, a level at a time) --------------------------------------------------------------------
    def recipes_batch(self, masks, offsets, first=None):
        """all_Ks (src/avi_solutions.jl:200-215) for MANY solutions in one launch (qpn_recipes_batch): masks [nodes, N] uint8,
        offsets [nodes + 1] int64 (host; node b gets the first offsets[b+1] - offsets[b] recipes of its product).
        first [nodes] int64 (host; qpn_recipes_batch_range): node b's recipes start at number first[b] of its product instead.
        Returns (K [total, N] uint8, node_of [total] int32)."""
        dev, masks = self._stage("recipes_batch", "masks", u8=(masks,))
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        nodes, N = int(masks.shape[0]), int(masks.shape[1])
        if offsets.shape != (nodes + 1,):
            raise ValueError("recipes_batch: offsets must have nodes + 1 entries")
        total = int(offsets[-1])
        K = self._alloc(dev, (total, N), np.uint8)
        node_of = self._alloc(dev, (total,), np.int32)
        if first is None:
            self._call("qpn_recipes_batch", nodes, N, _ptr(masks), _ptr(offsets), _ptr(K), _ptr(node_of), self._mem(dev))
            return K, node_of
        first = np.ascontiguousarray(first, dtype=np.int64)
        if first.shape != (nodes,):
            raise ValueError("recipes_batch: first must have one entry per node")
        self._call("qpn_recipes_batch_range", nodes, N, _ptr(masks), _ptr(first), _ptr(offsets), _ptr(K), _ptr(node_of), self._mem(dev))
        return K, node_of

    def finish_pieces(self, Ar, lr, ur, rows, flags, rec_of, ncols, take, xk, probe, n, m, member_tol=1e-5, store_cap=None):
        """The finishing step of reduced_pieces' output (qpn_finish_pieces; level_batch.finish_pieces_host is its numpy twin):
        piece t of item rec_of[t] over the item's columns take[k, :ncols[k]] (ascending global order), the point xk and the probe
        vector on them ([records, n+p] each); Ar [pieces, n+p, n+2m].  Returns dict(status, worst, hash, dup_of, store_of [pieces], As [S, n+p, cap]
        column-major, ls, us [S, cap], rows_s [S], stored = S): the store holds the members that are neither duplicates nor flagged.
        Device inputs give device outputs (hash as int64 bits); the store then has room for store_cap (default: pieces) slots,
        of which the first `stored` are filled."""
        dev, Ar, lr, ur, xk, probe, rows, flags, rec_of, ncols, take = self._stage(
            "finish_pieces", "Ar lr ur xk probe rows flags rec_of ncols take", f64=(Ar, lr, ur, xk, probe),
            i32=(rows, flags, rec_of, ncols, take))
        pieces, oc, cap = (int(v) for v in Ar.shape)
        records = int(ncols.shape[0])
        if tuple(take.shape) != (records, oc) or tuple(xk.shape) != (records, oc) or tuple(probe.shape) != (records, oc) \
                or tuple(lr.shape) != (pieces, cap) or tuple(ur.shape) != (pieces, cap) or tuple(rows.shape) != (pieces,) \
                or tuple(flags.shape) != (pieces,) or tuple(rec_of.shape) != (pieces,):
            raise QpnError("finish_pieces: inconsistent shapes")
        n, m = int(n), int(m)
        p = oc - n
        if cap != n + 2 * m or p < 0:
            raise QpnError("finish_pieces: Ar must be [pieces, n + p, n + 2m]")
        sc = pieces if store_cap is None else int(store_cap)
        status = self._alloc(dev, (pieces,), np.int32)
        worst = self._alloc(dev, (pieces,), np.float64)
        hsh = self._alloc(dev, (pieces,), np.int64) if dev else np.empty(pieces, np.uint64)
        dup_of = self._alloc(dev, (pieces,), np.int32)
        store_of = self._alloc(dev, (pieces,), np.int32)
        As = self._alloc(dev, (sc, oc, cap), np.float64)
        ls = self._alloc(dev, (sc, cap), np.float64)
        us = self._alloc(dev, (sc, cap), np.float64)
        rows_s = self._alloc(dev, (sc,), np.int32)
        stored = C.c_int32(0)
        self._call("qpn_finish_pieces", pieces, records, n, m, p, _ptr(Ar), _ptr(lr), _ptr(ur), _ptr(rows), _ptr(flags), _ptr(rec_of),
                   _ptr(ncols), _ptr(take), _ptr(xk), _ptr(probe), float(member_tol), _ptr(status), _ptr(worst), _ptr(hsh),
                   _ptr(dup_of), _ptr(store_of), sc, _ptr(As), _ptr(ls), _ptr(us), _ptr(rows_s), C.byref(stored), self._mem(dev))
        S = int(stored.value)
        return dict(status=status, worst=worst, hash=hsh, dup_of=dup_of, store_of=store_of, As=As[:S], ls=ls[:S], us=us[:S],
                    rows_s=rows_s[:S], stored=S)

    def reduced_pieces(self, Qc, Rc, qd, Ac, Bc, l, u, K, node_of=None, tol=1e-9):
        """local_piece (src/avi_solutions.jl:400-496) for recipes K over node records, with the m multiplier columns eliminated
        through each piece's own equality rows (qpn_reduced_pieces).  Returns (Ar [pieces, n+p, cap] column-major per piece --
        Ar[t].T is the cap x (n+p) row matrix over [x_d; x_p] --, lr, ur [pieces, cap], rows [pieces], flags [pieces]),
        cap = n + 2m."""
        dev, Qc, Rc, qd, Ac, Bc, l, u, K, node_of = self._stage("reduced_pieces", "Qc Rc qd Ac Bc l u K node_of",
                                                                f64=(Qc, Rc, qd, Ac, Bc, l, u), u8=(K,), i32=(node_of,))
        nodes, n = qd.shape
        m = l.shape[1]
        p = Rc.shape[1]
        pieces = int(K.shape[0])
        cap = n + 2 * m
        Ar = self._alloc(dev, (pieces, n + p, cap), np.float64)
        lr = self._alloc(dev, (pieces, cap), np.float64)
        ur = self._alloc(dev, (pieces, cap), np.float64)
        rows = self._alloc(dev, (pieces,), np.int32)
        flags = self._alloc(dev, (pieces,), np.int32)
        self._call("qpn_reduced_pieces", pieces, nodes, n, m, p, _ptr(Qc), _ptr(Rc), _ptr(qd), _ptr(Ac), _ptr(Bc), _ptr(l), _ptr(u),
                   _ptr(node_of), _ptr(K), float(tol), _ptr(Ar), _ptr(lr), _ptr(ur), _ptr(rows), _ptr(flags), self._mem(dev))
        return Ar, lr, ur, rows, flags

    def project_pieces(self, Qc, Rc, qd, Ac, Bc, l, u, K, node_of=None, tol=1e-9, cap=None):
        """reduced_pieces for the pieces it flags with bit 0 (qpn_project_pieces; level_batch.project_pieces_host is its numpy
        twin): the multipliers eliminated through each piece's own equality rows, then one Fourier-Motzkin step per column that
        no equality pins, all of them in this one call.  cap >= n + 2m: the rows of room per piece (default
        level_batch.project_cap(n, m)).  Returns (Ar [pieces, n+p, cap] column-major per piece, lr, ur [pieces, cap], rows, flags
        [pieces]); flags: 2 = more than cap rows alive before the first step, 4 = a step needed more than cap rows (the piece is
        all fill, rows 0)."""
        dev, Qc, Rc, qd, Ac, Bc, l, u, K, node_of = self._stage("project_pieces", "Qc Rc qd Ac Bc l u K node_of",
                                                                f64=(Qc, Rc, qd, Ac, Bc, l, u), u8=(K,), i32=(node_of,))
        nodes, n = qd.shape
        m = l.shape[1]
        p = Rc.shape[1]
        pieces = int(K.shape[0])
        if cap is None:
            from .level_batch import project_cap
            cap = project_cap(n, m)
        cap = int(cap)
        if cap < n + 2 * m:
            raise QpnError("project_pieces: cap < n + 2m")
        Ar = self._alloc(dev, (pieces, n + p, cap), np.float64)
        lr = self._alloc(dev, (pieces, cap), np.float64)
        ur = self._alloc(dev, (pieces, cap), np.float64)
        rows = self._alloc(dev, (pieces,), np.int32)
        flags = self._alloc(dev, (pieces,), np.int32)
        self._call("qpn_project_pieces", pieces, nodes, n, m, p, _ptr(Qc), _ptr(Rc), _ptr(qd), _ptr(Ac), _ptr(Bc), _ptr(l), _ptr(u),
                   _ptr(node_of), _ptr(K), float(tol), cap, _ptr(Ar), _ptr(lr), _ptr(ur), _ptr(rows), _ptr(flags), self._mem(dev))
        return Ar, lr, ur, rows, flags

    # -- (A6) pool assembly ----------------------------------------------------------------------
    def assemble_pools(self, n_i, m_i, dpos, nd, Qd, Qp, qd, Ad, Bp, l, u, w, form="reduced", share_M=None):
        """combine_gavis (src/avi.jl:305-377) for `batch` instances of one pool shape, on the device.

        Shape: n_i, m_i (per player, pool order), dpos (decision position of every stacked player row), nd.
        Blocks in the ABI layout (column-major), each either shared ((cols, rows)) or per item ((batch, cols, rows)):
        Qd (nd, sn), Qp (p, sn), qd (sn,), Ad (nd, sm), Bp (p, sm), l, u (sm,), w (p,).  form: "reduced" | "reference".
        share_M (default: automatically when Qd and Ad are shared): write ONE M for the whole batch.
        Returns (Mc, q, lo, hi, kind) ready for solve_avi_batch (Mc (N, N) when shared)."""
        from ._lib import POOL_REDUCED, POOL_REFERENCE, PoolShape
        dev, Qd, Qp, qd, Ad, Bp, l, u, w = self._stage("assemble_pools", "Qd Qp qd Ad Bp l u w", f64=(Qd, Qp, qd, Ad, Bp, l, u, w))
        n_i = np.ascontiguousarray(n_i, dtype=np.int32); m_i = np.ascontiguousarray(m_i, dtype=np.int32)
        dpos = np.ascontiguousarray(dpos, dtype=np.int32)
        sn, sm = int(n_i.sum()), int(m_i.sum())
        p = int(w.shape[-1])
        item_dims = dict(Qd=2, Qp=2, qd=1, Ad=2, Bp=2, l=1, u=1, w=1)
        arrs = dict(Qd=Qd, Qp=Qp, qd=qd, Ad=Ad, Bp=Bp, l=l, u=u, w=w)
        sizes = dict(Qd=sn * nd, Qp=sn * p, qd=sn, Ad=sm * nd, Bp=sm * p, l=sm, u=sm, w=p)
        batch = 1
        strides = {}
        for k, a_ in arrs.items():
            if a_.ndim == item_dims[k] + 1:
                batch = max(batch, int(a_.shape[0])); strides[k] = sizes[k]
            elif a_.ndim == item_dims[k]:
                strides[k] = 0
            else:
                raise ValueError(f"assemble_pools: {k} has {a_.ndim} dimensions")
            n_el = int(np.prod(a_.shape[-item_dims[k]:])) if item_dims[k] else 1
            if n_el != sizes[k]:
                raise ValueError(f"assemble_pools: {k} has {n_el} entries per item, the shape says {sizes[k]}")
        if strides["l"] != strides["u"]:
            raise ValueError("assemble_pools: l and u must both be shared or both per item")
        for k, a_ in arrs.items():
            if strides[k] and a_.shape[0] != batch:
                raise ValueError(f"assemble_pools: {k} has batch {a_.shape[0]}, others {batch}")
        fcode = {"reduced": POOL_REDUCED, "reference": POOL_REFERENCE}[form]
        shape = PoolShape(len(n_i), int(nd), p, n_i.ctypes.data, m_i.ctypes.data, dpos.ctypes.data)
        Nn = C.c_int32(0)
        if self.lib.qpn_pool_size(C.byref(shape), fcode, C.byref(Nn)) != 0:
            raise QpnError("qpn_pool_size: bad pool shape")
        N = int(Nn.value)
        if share_M is None:
            share_M = strides["Qd"] == 0 and strides["Ad"] == 0
        Mout = self._alloc(dev, (N, N) if share_M else (batch, N, N), np.float64)
        qout = self._alloc(dev, (batch, N), np.float64)
        lout = self._alloc(dev, (batch, N), np.float64)
        uout = self._alloc(dev, (batch, N), np.float64)
        kind = self._alloc(dev, (batch, N), np.uint8)
        self._call("qpn_assemble_pools", C.byref(shape), fcode, batch, _ptr(Qd), strides["Qd"], _ptr(Qp), strides["Qp"], _ptr(qd),
                   strides["qd"], _ptr(Ad), strides["Ad"], _ptr(Bp), strides["Bp"], _ptr(l), _ptr(u), strides["l"], _ptr(w),
                   strides["w"], _ptr(Mout), 0 if share_M else N * N, _ptr(qout), _ptr(lout), _ptr(uout), _ptr(kind), self._mem(dev))
        return Mout, qout, lout, uout, kind

    # -- (A5+A6+A2+A3+A9 fused) --------------------------------------------------------------
    def solve_nodes(self, Qc, Rc, qd, Ac, Bc, l, u, w, z0=None, opts=None, want_active=True, out=None,
                    x_out=None):
        """Assemble every node's KKT blocks on the fly and solve (one kernel for n, m <= 32); same
        results as assemble_nodes + solve_avi_batch without materialising M.  z = [x_d; lambda].
        x_out (optional, [batch, >= n] fp64, rows may be strided): the primal blocks are also written
        there by the solve itself -- the outer sweep's x[decision_inds] = x_opt[decision_inds]
        (src/algorithm.jl:97-101).
        With AVI_FLAG_WARM_DUALS in opts.flags (n, m <= 32) the multipliers of z0 name the active set every node starts from:
        a node whose hint holds comes back with pivots = 0, the others are solved cold in the same call (include/qpn_hip.h)."""
        dev, Qc, Rc, qd, Ac, Bc, l, u, w, z0 = self._stage("solve_nodes", "Qc Rc qd Ac Bc l u w z0", f64=(Qc, Rc, qd, Ac, Bc, l, u, w, z0))
        batch, n = qd.shape
        m = l.shape[1]
        p = w.shape[-1]
        sw = 0 if w.ndim == 1 else p
        res, o = self._solve_outputs(dev, batch, n + m, z0, opts, want_active, out)
        sx = self._x_stride(x_out, dev, batch, n)
        self._call("qpn_solve_nodes_into", batch, n, m, p, _ptr(Qc), _ptr(Rc), _ptr(qd), _ptr(Ac), _ptr(Bc), _ptr(l), _ptr(u), _ptr(w),
                   sw, _ptr(res["z"]), _ptr(res["status"]), _ptr(res["resid"]), _ptr(res["pivots"]), _ptr(res["active"]), C.byref(o),
                   self._mem(dev), _ptr(x_out), sx)
        return res

    def order_nodes_by_pivots(self, pivots):
        """Schedule hint for later solve_nodes calls over the SAME nodes: longest solves first, from the
        pivot counts of an earlier sweep (device or host int32 array).  Results do not depend on it."""
        dev, pivots = self._stage("order_nodes_by_pivots", "pivots", i32=(pivots,))
        self._call("qpn_order_nodes_by_pivots", _ptr(pivots), int(pivots.shape[0]), self._mem(dev))

    def set_auto_schedule(self, period=16):
        """Period (in calls) of the context's own longest-first schedule refresh for solve_nodes batches that fill the
        GPU; 0 switches it off.  An explicit hint (order_nodes_by_pivots / set_node_order) takes precedence."""
        self._call("qpn_ctx_set_auto_schedule", int(period))

    def set_option(self, option, value):
        """Per-context route option (include/qpn_hip.h: QPN_OPT_*), e.g. set_option(OPT_MID_ROUTE, 2)."""
        self._call("qpn_ctx_set_option", int(option), int(value))

    def set_node_order(self, order=None):
        """Install a caller-made permutation of the nodes as the schedule (None clears the hint)."""
        if order is None:
            self._call("qpn_set_node_order", None, 0, self._mem(False))
            return
        dev, order = self._stage("set_node_order", "order", i32=(order,))
        self._call("qpn_set_node_order", _ptr(order), int(order.shape[0]), self._mem(dev))

    # -- (A8) ------------------------------------------------------------------------------
    # -- multi-GPU: shared iterate buffers, replicas, per-sweep status (include/qpn_hip.h) ----------
    def shared_alloc(self, nbytes, fine_grained=False):
        """Zeroed device buffer + its IPC handle: (address, handle bytes)."""
        from ._lib import IPC_HANDLE_BYTES, SHARED_FINE_GRAINED
        ptr = C.c_void_p()
        h = (C.c_uint8 * IPC_HANDLE_BYTES)()
        self._call("qpn_shared_alloc", int(nbytes), SHARED_FINE_GRAINED if fine_grained else 0, C.byref(ptr), h)
        return int(ptr.value), bytes(h)

    def shared_open(self, handle: bytes) -> int:
        """Map a peer's shared buffer into this process; returns its address here."""
        ptr = C.c_void_p()
        h = (C.c_uint8 * len(handle)).from_buffer_copy(handle)
        self._call("qpn_shared_open", h, C.byref(ptr))
        return int(ptr.value)

    def shared_close(self, addr: int):
        self._call("qpn_shared_close", C.c_void_p(addr))

    def shared_free(self, addr: int):
        self._call("qpn_shared_free", C.c_void_p(addr))

    def set_primal_mirrors(self, own_addr=0, nbytes=0, peer_addrs=()):
        """Later solve_nodes(x_out=...) calls whose x_out lies inside [own_addr, own_addr + nbytes) also store
        every primal block at the same offset of each peer buffer.  No arguments: clear."""
        arr = (C.c_void_p * max(len(peer_addrs), 1))(*[C.c_void_p(a) for a in peer_addrs])
        self._call("qpn_set_primal_mirrors", C.c_void_p(own_addr), int(nbytes), len(peer_addrs), arr)

    def sweep_status(self, status, resid, out, rank=0, world=1, boxes=None, epoch=0, timeout_ms=1000):
        """out[0:3] (device fp64, 4 entries) <- (items not solved, max resid, 1), combined over `world` ranks
        through their mailboxes when world > 1 (also the barrier after the replica stores); a missed barrier gives
        out[2] = 0 and out[3] += 1.  Asynchronous on the stream."""
        dev, status, resid, out = self._stage("sweep_status", "status resid out", i32=(status,), f64=(resid, out))
        if not dev:
            raise QpnError("sweep_status: device tensors only")
        arr = None
        if world > 1:
            arr = (C.c_void_p * world)(*[C.c_void_p(a) for a in boxes])
        self._call("qpn_sweep_status", _ptr(status), _ptr(resid), int(status.shape[0]), _ptr(out), int(rank), int(world), arr,
                   int(epoch), int(timeout_ms))
        return out

    def verify_nodes(self, Qc, Rc, qd, Ac, Bc, l, u, xd, w, tol=1e-4):
        """Batched verify_solution (src/qp_processing.jl:57-149) -> (solution, lambda, path)."""
        dev, Qc, Rc, qd, Ac, Bc, l, u, xd, w = self._stage("verify_nodes", "Qc Rc qd Ac Bc l u xd w", f64=(Qc, Rc, qd, Ac, Bc, l, u, xd, w))
        batch, n = qd.shape
        m = l.shape[1]
        p = w.shape[-1]
        records = (batch, n, m, p, _ptr(Qc), _ptr(Rc), _ptr(qd), _ptr(Ac), _ptr(Bc), _ptr(l), _ptr(u))
        return self._verify("qpn_verify_nodes", dev, records, batch, m, p, xd, w, tol)

    def _verify(self, name, dev, records, batch, m, p, xd, w, tol):
        """The common end of verify_nodes and Nodes.verify, which differ in where the records are (`records`: the arguments
        that name them)."""
        sol = self._alloc(dev, (batch,), np.int32)
        path = self._alloc(dev, (batch,), np.int32)
        lam = self._alloc(dev, (batch, max(m, 1)), np.float64)
        self._call(name, *records, _ptr(xd), _ptr(w), 0 if w.ndim == 1 else p, float(tol), _ptr(sol), _ptr(lam), _ptr(path),
                   self._mem(dev))
        return sol, lam[:, :m], path

    def convexity_nodes(self, Qc, Ac, eq, tol=1e-6):
        """Batched check_qp_convexity (src/qp_processing.jl:39-55) on node blocks: Qc [batch, n, n] and Ac [batch, n, m] in
        the ABI layout, eq [batch, m] uint8 (the implicit equality rows) -> (convex [batch] int32, min_eig [batch],
        null_dim [batch] int32)."""
        dev, Qc, Ac, eq = self._stage("convexity_nodes", "Qc Ac eq", f64=(Qc, Ac), u8=(eq,))
        batch, n = Qc.shape[0], Qc.shape[-1]
        m = eq.shape[1]
        convex = self._alloc(dev, (batch,), np.int32)
        min_eig = self._alloc(dev, (batch,), np.float64)
        null_dim = self._alloc(dev, (batch,), np.int32)
        self._call("qpn_convexity_nodes", batch, n, m, _ptr(Qc), _ptr(Ac) if m else None, _ptr(eq) if m else None, float(tol),
                   _ptr(convex), _ptr(min_eig), _ptr(null_dim), self._mem(dev))
        return convex, min_eig, null_dim

    def multiplier_vertices(self, Ac, g, cls, lam0, V, max_bases=None, tol=1e-9, feas=1e-6):
        """Vertices of the multiplier sets Lambda = {lambda : Ad' lambda = g, classes} of many items (qpn_multiplier_vertices;
        level_batch.multiplier_vertices_host is its numpy twin): Ac [batch, n, m] (Ad in the ABI layout), g [batch, n], cls
        [batch, m] uint8 (level_batch.MV_GE / LE / FREE / ZERO), lam0 [batch, m] the start, V the vertex budget, max_bases the
        basis budget (default 64 V).  Returns (verts [batch, V, m], count [batch] int32, status [batch] int32)."""
        dev, Ac, g, lam0, cls = self._stage("multiplier_vertices", "Ac g lam0 cls", f64=(Ac, g, lam0), u8=(cls,))
        batch, n, m = (int(v) for v in Ac.shape)
        V = int(V)
        mb = 64 * max(V, 1) if max_bases is None else int(max_bases)
        if tuple(g.shape) != (batch, n) or tuple(cls.shape) != (batch, m) or tuple(lam0.shape) != (batch, m):
            raise QpnError("multiplier_vertices: inconsistent shapes")
        verts = self._alloc(dev, (batch, V, m), np.float64)
        count = self._alloc(dev, (batch,), np.int32)
        status = self._alloc(dev, (batch,), np.int32)
        self._call("qpn_multiplier_vertices", batch, n, m, _ptr(Ac), _ptr(g), _ptr(cls), _ptr(lam0), V, mb, float(tol), float(feas),
                   _ptr(verts), _ptr(count), _ptr(status), self._mem(dev))
        return verts, count, status

    def recipe_filter(self, masks, K, vrow_of, first_of):
        """qpn_recipe_filter (level_batch.recipe_filter_host is its numpy twin): keep [pieces] uint8, 0 for a recipe K[t] of
        product row vrow_of[t] that an earlier product row of the same item (first_of[row] <= s < row) holds."""
        dev, masks, K, vrow_of, first_of = self._stage("recipe_filter", "masks K vrow_of first_of", u8=(masks, K), i32=(vrow_of, first_of))
        rows, N = int(masks.shape[0]), int(masks.shape[1])
        pieces = int(K.shape[0])
        keep = self._alloc(dev, (pieces,), np.uint8)
        self._call("qpn_recipe_filter", pieces, rows, N, _ptr(masks), _ptr(K), _ptr(vrow_of), _ptr(first_of), _ptr(keep), self._mem(dev))
        return keep

    # -- interior members of polyhedra: records made on the device ---------------------------------------------
    def _member_args(self, who, Ac, l, u, ne, nlo, nhi):
        batch, d, r = (int(v) for v in Ac.shape)
        if tuple(l.shape) != (batch, r) or tuple(u.shape) != (batch, r):
            raise QpnError(f"{who}: inconsistent shapes")
        ne, nlo, nhi = int(ne), int(nlo), int(nhi)
        mi = nlo + nhi
        return batch, r, d, ne, nlo, nhi, d + 1 + ne, max(16, -(-mi // 16) * 16)

    def assemble_interior_nodes(self, Ac, l, u, delta, ne, nlo, nhi):
        """The node records of the interior-member queries of a batch of polyhedra (qpn_assemble_interior_nodes;
        polyhedra.interior_member_records is its numpy twin): Ac [batch, d, r] (A in the ABI layout, ``colmajor(A)``), l, u
        [batch, r]; ne, nlo, nhi the slot counts of the three row classes.  Returns (Qc [batch, nf, nf], qd [batch, nf],
        Ac [batch, nf, mp], l, u [batch, mp], flag [batch] uint8: 1 = more rows of a class than slots, inert record)."""
        dev, Ac, l, u = self._stage("assemble_interior_nodes", "Ac l u", f64=(Ac, l, u))
        batch, r, d, ne, nlo, nhi, nf, mp = self._member_args("assemble_interior_nodes", Ac, l, u, ne, nlo, nhi)
        Qo = self._alloc(dev, (batch, nf, nf), np.float64)
        qo = self._alloc(dev, (batch, nf), np.float64)
        Ao = self._alloc(dev, (batch, nf, mp), np.float64)
        lo = self._alloc(dev, (batch, mp), np.float64)
        uo = self._alloc(dev, (batch, mp), np.float64)
        flag = self._alloc(dev, (batch,), np.uint8)
        self._call("qpn_assemble_interior_nodes", batch, r, d, _ptr(Ac), _ptr(l), _ptr(u), float(delta), ne, nlo, nhi, _ptr(Qo), _ptr(qo),
                   _ptr(Ao), _ptr(lo), _ptr(uo), _ptr(flag), self._mem(dev))
        return Qo, qo, Ao, lo, uo, flag

    def interior_members(self, Ac, l, u, delta, ne, nlo, nhi):
        """One interior member per polyhedron (qpn_interior_members): the records of assemble_interior_nodes are made in the
        library's workspace, solved as solve_nodes(..., z0=None) solves them, and the members taken out.
        Returns (x [batch, d], ok [batch] uint8, status [batch] int32); x is meaningful where ok."""
        dev, Ac, l, u = self._stage("interior_members", "Ac l u", f64=(Ac, l, u))
        batch, r, d, ne, nlo, nhi, _, _ = self._member_args("interior_members", Ac, l, u, ne, nlo, nhi)
        x = self._alloc(dev, (batch, d), np.float64)
        ok = self._alloc(dev, (batch,), np.uint8)
        status = self._alloc(dev, (batch,), np.int32)
        self._call("qpn_interior_members", batch, r, d, _ptr(Ac), _ptr(l), _ptr(u), float(delta), ne, nlo, nhi, _ptr(x), _ptr(ok),
                   _ptr(status), self._mem(dev))
        return x, ok, status

    def assemble_parent_nodes(self, form, ne, m, p, sQc, sRc, sqd, sAc, sBc, sl, su, mb_true, piece_desc, pA, pl, pu, map_off,
                              map_data, parent_of, piece_of, map_of):
        """The records of inner nodes made on the device (qpn_assemble_parent_nodes; level_batch.assemble_parent_records_host
        is its numpy twin and says what every argument is).  form 0: the verify form, 1: the solve form with ne equality rows
        in the free block; m, p: the output's padded row and parameter counts.  Static store: sQc [P, n0, n0], sRc [P, ps, n0],
        sqd [P, n0], sAc [P, n0, mb], sBc [P, ps, mb], sl, su [P, mb], mb_true [P] int32.  Piece pool: piece_desc [pieces, 4]
        int32 (row0, rows, c, off), pA (flat), pl, pu.  Maps: map_off [maps + 1], map_data int32.  Items: parent_of [items],
        piece_of, map_of [items, 8] int32.  Host arrays in: numpy out, a bad item raises; device tensors in: tensors out, err
        tells.  Returns (Qc [items, n, n], Rc [items, p, n], qd [items, n], Ac [items, n, m], Bc [items, p, m], l, u
        [items, m], err [items] int32)."""
        who = "assemble_parent_nodes"
        (dev, sQc, sRc, sqd, sAc, sBc, sl, su, pA, pl, pu, mb_true, piece_desc, map_off, map_data, parent_of, piece_of,
         map_of) = self._stage(who, "sQc sRc sqd sAc sBc sl su pA pl pu mb_true piece_desc map_off map_data parent_of piece_of map_of",
                               f64=(sQc, sRc, sqd, sAc, sBc, sl, su, pA, pl, pu),
                               i32=(mb_true, piece_desc, map_off, map_data, parent_of, piece_of, map_of))
        form, ne, m, p = int(form), int(ne) if form else 0, int(m), int(p)
        P, n0 = (int(v) for v in sqd.shape)
        ps, mb = int(sRc.shape[1]), int(sl.shape[1])
        items, pieces, maps = int(parent_of.shape[0]), int(piece_desc.shape[0]), int(map_off.shape[0]) - 1
        slots = _lib.PARENT_SLOTS
        if tuple(sQc.shape) != (P, n0, n0) or tuple(sRc.shape) != (P, ps, n0) or tuple(sAc.shape) != (P, n0, mb) or \
                tuple(sBc.shape) != (P, ps, mb) or tuple(sl.shape) != (P, mb) or tuple(su.shape) != (P, mb) or \
                tuple(mb_true.shape) != (P,) or tuple(piece_desc.shape) != (pieces, 4) or maps < 0 or pA.ndim != 1 or pl.ndim != 1 or \
                tuple(pu.shape) != tuple(pl.shape) or map_data.ndim != 1 or tuple(piece_of.shape) != (items, slots) or \
                tuple(map_of.shape) != (items, slots) or form not in (0, 1):
            raise QpnError(f"{who}: inconsistent shapes")
        n = n0 + ne
        Qo = self._alloc(dev, (items, n, n), np.float64); Ro = self._alloc(dev, (items, p, n), np.float64)
        qo = self._alloc(dev, (items, n), np.float64); Ao = self._alloc(dev, (items, n, m), np.float64)
        Bo = self._alloc(dev, (items, p, m), np.float64)
        lo = self._alloc(dev, (items, m), np.float64); uo = self._alloc(dev, (items, m), np.float64)
        err = self._alloc(dev, (items,), np.int32)
        self._call("qpn_assemble_parent_nodes", items, form, n0, ne, m, p, P, mb, ps, _ptr(sQc), _ptr(sRc), _ptr(sqd), _ptr(sAc), _ptr(sBc),
                   _ptr(sl), _ptr(su), _ptr(mb_true), pieces, _ptr(piece_desc), int(pl.shape[0]), int(pA.shape[0]), _ptr(pA), _ptr(pl),
                   _ptr(pu), maps, _ptr(map_off), int(map_data.shape[0]), _ptr(map_data), _ptr(parent_of), _ptr(piece_of), _ptr(map_of),
                   _ptr(Qo), _ptr(Ro), _ptr(qo), _ptr(Ao), _ptr(Bo), _ptr(lo), _ptr(uo), _ptr(err), self._mem(dev))
        return Qo, Ro, qo, Ao, Bo, lo, uo, err

    def members_outside(self, Ajc, lj, uj, X, pi, pj, t):
        """qpn_members_outside (polyhedra.members_outside_host is its numpy twin): out [pairs] uint8, 1 where member X[pi[q]]
        violates a row of piece pj[q] by more than t.  Ajc [Bj, d, rj] (ABI layout), lj, uj [Bj, rj], X [Bi, d], pi, pj int32."""
        dev, Ajc, lj, uj, X, pi, pj = self._stage("members_outside", "Ajc lj uj X pi pj", f64=(Ajc, lj, uj, X), i32=(pi, pj))
        Bj, d, rj = (int(v) for v in Ajc.shape)
        pairs = int(pi.shape[0])
        if tuple(lj.shape) != (Bj, rj) or tuple(uj.shape) != (Bj, rj) or X.ndim != 2 or int(X.shape[1]) != d or tuple(pj.shape) != (pairs,):
            raise QpnError("members_outside: inconsistent shapes")
        out = self._alloc(dev, (pairs,), np.uint8)
        self._call("qpn_members_outside", pairs, d, rj, _ptr(Ajc), _ptr(lj), _ptr(uj), Bj, _ptr(X), int(X.shape[0]), _ptr(pi), _ptr(pj),
                   float(t), _ptr(out), self._mem(dev))
        return out

    def members_outside_lists(self, Ajc, lj, uj, X, ok, list_ptr, list_mem, list_of, self_pos, word_ptr, t):
        """qpn_members_outside_lists (polyhedra.members_outside_lists_host is its numpy twin): every member of a list against
        every piece of it, the pairs enumerated on the device.  One pack of second pieces Ajc [Bj, d, rj] (ABI layout), lj, uj
        [Bj, rj]; members X [Bi, d] with their flags ok [Bi] uint8; the lists as a CSR, list_ptr [lists + 1] and list_mem int32
        (rows of X, -1 = no member); list_of, self_pos [Bj] int32: the list of piece j and its own position there; word_ptr
        [Bj + 1] int64: piece j owns the words [word_ptr[j], word_ptr[j + 1]) of bits, ceil(k / 32) for a list of k.
        Returns (bits [word_ptr[Bj]] uint32, undecided [Bj] int32): bit s of a piece's segment = the member at position s
        refutes "piece s is a subset of piece j"; undecided = the positions other than the piece's own whose bit is 0.
        Host arrays in: numpy out, and an index out of range raises; device tensors in: tensors out, a bad item answers as the
        header says (list_ptr and word_ptr themselves are checked here in either mode: they bound the buffers)."""
        who = "members_outside_lists"
        dev, Ajc, lj, uj, X, ok, list_ptr, list_mem, list_of, self_pos, word_ptr = self._stage(
            who, "Ajc lj uj X ok list_ptr list_mem list_of self_pos word_ptr", f64=(Ajc, lj, uj, X), u8=(ok,),
            i32=(list_ptr, list_mem, list_of, self_pos), i64=(word_ptr,))
        Bj, d, rj = (int(v) for v in Ajc.shape)
        Bi, lists = int(X.shape[0]), int(list_ptr.shape[0]) - 1
        if tuple(lj.shape) != (Bj, rj) or tuple(uj.shape) != (Bj, rj) or X.ndim != 2 or int(X.shape[1]) != d or \
                tuple(ok.shape) != (Bi,) or list_ptr.ndim != 1 or lists < 0 or list_mem.ndim != 1 or tuple(list_of.shape) != (Bj,) or \
                tuple(self_pos.shape) != (Bj,) or tuple(word_ptr.shape) != (Bj + 1,):
            raise QpnError(f"{who}: inconsistent shapes")
        # the two offset arrays say how far the kernel reads list_mem and writes bits: never taken on trust
        for name, ptr, limit in (("list_ptr", list_ptr, int(list_mem.shape[0])), ("word_ptr", word_ptr, None)):
            bad = bool(ptr[0] != 0) or (ptr.shape[0] > 1 and bool((ptr[1:] < ptr[:-1]).any())) or \
                (limit is not None and int(ptr[-1]) > limit)
            if bad:
                raise QpnError(f"{who}: {name} must start at 0, not decrease" + (" and end inside list_mem" if limit is not None else ""))
        bits = self._alloc(dev, (int(word_ptr[-1]),), np.uint32)
        undecided = self._alloc(dev, (Bj,), np.int32)
        self._call("qpn_members_outside_lists", d, rj, _ptr(Ajc), _ptr(lj), _ptr(uj), Bj, _ptr(X), _ptr(ok), Bi, lists, _ptr(list_ptr),
                   _ptr(list_mem), _ptr(list_of), _ptr(self_pos), _ptr(word_ptr), float(t), _ptr(bits), _ptr(undecided), self._mem(dev))
        return bits, undecided

    # -- the LP solver of the polyhedral primitives --------------------------------------------------------------
    def default_lp_opts(self) -> LpOpts:
        o = LpOpts()
        self.lib.qpn_lp_default_opts(C.byref(o))
        return o

    def _lp_opts(self, opts):
        """opts of an LP entry -- LpOpts, a dict of its fields over the defaults, or None -> LpOpts or None."""
        if not isinstance(opts, dict):
            return opts
        o = self.default_lp_opts()
        for k, v in opts.items():
            setattr(o, k, v)
        return o

    def lp_kernel_class(self, r, d):
        """Which kernel class takes LPs of r rows in d variables: 0 wavefront, 1 workgroup in LDS, 2 workgroup over the workspace,
        -1 beyond the limits (qpn_lp_kernel_class)."""
        return int(self.lib.qpn_lp_kernel_class(int(r), int(d)))

    def solve_lps(self, Ac, l, u, poly_of, cost=None, obj_row=None, obj_sign=None, opts=None):
        """LPs over shared polyhedra (qpn_solve_lps; polyhedra.solve_lps_host is its numpy twin, bit for bit): Ac [polys, d, r]
        (A in the ABI layout, ``colmajor(A)``), l, u [polys, r], poly_of [jobs] int32; job t minimises cost[t]'x or, without
        `cost`, obj_sign[t] * (row obj_row[t] of its polyhedron)'x (int32 arrays).  opts: LpOpts, a dict of its fields, or None.
        Returns dict(status [jobs] int32 (_lib.LP_*), x [jobs, d], obj [jobs], lam [jobs, r], ray [jobs, d], iters [jobs] int32)."""
        if cost is None and (obj_row is None or obj_sign is None):
            raise QpnError("solve_lps: give cost, or obj_row and obj_sign")
        if cost is not None:
            obj_row = obj_sign = None
        dev, Ac, l, u, cost, poly_of, obj_row, obj_sign = self._stage("solve_lps", "Ac l u cost poly_of obj_row obj_sign", f64=(Ac, l, u, cost),
                                                                     i32=(poly_of, obj_row, obj_sign))
        polys, d, r = (int(v) for v in Ac.shape)
        jobs = int(poly_of.shape[0])
        if tuple(l.shape) != (polys, r) or tuple(u.shape) != (polys, r) or (cost is not None and tuple(cost.shape) != (jobs, d)) or (
                cost is None and (tuple(obj_row.shape) != (jobs,) or tuple(obj_sign.shape) != (jobs,))):
            raise QpnError("solve_lps: inconsistent shapes")
        opts = self._lp_opts(opts)
        out = dict(status=self._alloc(dev, (jobs,), np.int32), x=self._alloc(dev, (jobs, d), np.float64), obj=self._alloc(dev, (jobs,), np.float64),
                   lam=self._alloc(dev, (jobs, r), np.float64), ray=self._alloc(dev, (jobs, d), np.float64), iters=self._alloc(dev, (jobs,), np.int32))
        self._call("qpn_solve_lps", polys, r, d, _ptr(Ac), _ptr(l), _ptr(u), jobs, _ptr(poly_of), _ptr(cost), _ptr(obj_row), _ptr(obj_sign),
                   C.byref(opts) if opts is not None else None, _ptr(out["status"]), _ptr(out["x"]), _ptr(out["obj"]), _ptr(out["lam"]),
                   _ptr(out["ray"]), _ptr(out["iters"]), self._mem(dev))
        return out

    def issubset_pairs(self, A1c, l1, u1, A2c, l2, u2, pi, pj, tol=1e-6, opts=None):
        """Subset tests P1 ⊆ P2, one job per pair (qpn_issubset_pairs; polyhedra.issubset_pairs_host is its numpy twin, bit for
        bit): first pieces A1c [B1, d, r1] (ABI layout, ``colmajor(A)``), l1, u1 [B1, r1]; second pieces A2c [B2, d, r2], l2, u2
        [B2, r2]; pair q asks pi[q] against pj[q] (int32).  opts: LpOpts, a dict of its fields, or None.
        Returns dict(sub [pairs] uint8, how [pairs] int32 (_lib.SUBSET_*), bound [pairs] int32, val [pairs], lps, iters [pairs] int32)."""
        dev, A1c, l1, u1, A2c, l2, u2, pi, pj = self._stage("issubset_pairs", "A1c l1 u1 A2c l2 u2 pi pj", f64=(A1c, l1, u1, A2c, l2, u2),
                                                            i32=(pi, pj))
        if A1c.ndim != 3 or A2c.ndim != 3 or pi.ndim != 1:
            raise QpnError("issubset_pairs: inconsistent shapes")
        B1, d, r1 = (int(v) for v in A1c.shape)
        B2, d2, r2 = (int(v) for v in A2c.shape)
        pairs = int(pi.shape[0])
        if d2 != d or tuple(l1.shape) != (B1, r1) or tuple(u1.shape) != (B1, r1) or tuple(l2.shape) != (B2, r2) or tuple(u2.shape) != (B2, r2) or (
                tuple(pj.shape) != (pairs,)):
            raise QpnError("issubset_pairs: inconsistent shapes")
        opts = self._lp_opts(opts)
        out = dict(sub=self._alloc(dev, (pairs,), np.uint8), how=self._alloc(dev, (pairs,), np.int32), bound=self._alloc(dev, (pairs,), np.int32),
                   val=self._alloc(dev, (pairs,), np.float64), lps=self._alloc(dev, (pairs,), np.int32), iters=self._alloc(dev, (pairs,), np.int32))
        self._call("qpn_issubset_pairs", d, B1, r1, _ptr(A1c), _ptr(l1), _ptr(u1), B2, r2, _ptr(A2c), _ptr(l2), _ptr(u2), pairs, _ptr(pi),
                   _ptr(pj), float(tol), C.byref(opts) if opts is not None else None, _ptr(out["sub"]), _ptr(out["how"]), _ptr(out["bound"]),
                   _ptr(out["val"]), _ptr(out["lps"]), _ptr(out["iters"]), self._mem(dev))
        return out

    def implicit_bounds(self, Ac, l, u, tol=1e-4, all_extremes=False, opts=None):
        """`implicit_bounds` of polyhedra of one shape, one job per polyhedron (qpn_implicit_bounds; polyhedra.implicit_bounds_host
        is its numpy twin, bit for bit): Ac [polys, d, r] (ABI layout, ``colmajor(A)``), l, u [polys, r].  all_extremes: every row
        that is no explicit equality gets both extremes (QPN_IB_ALL_EXTREMES).  opts: LpOpts, a dict of its fields, or None.
        Returns dict(status [polys] int32 (_lib.IB_*), fail_row [polys] int32, eq [polys, r] uint8, vals [polys, r], how [polys, r]
        int32 (_lib.IB_HOW_*), lo, hi [polys, r], lps, iters [polys] int32)."""
        dev, Ac, l, u = self._stage("implicit_bounds", "Ac l u", f64=(Ac, l, u))
        if Ac.ndim != 3:
            raise QpnError("implicit_bounds: inconsistent shapes")
        polys, d, r = (int(v) for v in Ac.shape)
        if tuple(l.shape) != (polys, r) or tuple(u.shape) != (polys, r):
            raise QpnError("implicit_bounds: inconsistent shapes")
        opts = self._lp_opts(opts)
        out = dict(status=self._alloc(dev, (polys,), np.int32), fail_row=self._alloc(dev, (polys,), np.int32),
                   eq=self._alloc(dev, (polys, r), np.uint8), vals=self._alloc(dev, (polys, r), np.float64),
                   how=self._alloc(dev, (polys, r), np.int32), lo=self._alloc(dev, (polys, r), np.float64),
                   hi=self._alloc(dev, (polys, r), np.float64), lps=self._alloc(dev, (polys,), np.int32), iters=self._alloc(dev, (polys,), np.int32))
        self._call("qpn_implicit_bounds", polys, r, d, _ptr(Ac), _ptr(l), _ptr(u), float(tol), _lib.IB_ALL_EXTREMES if all_extremes else 0,
                   C.byref(opts) if opts is not None else None, _ptr(out["status"]), _ptr(out["fail_row"]), _ptr(out["eq"]), _ptr(out["vals"]),
                   _ptr(out["how"]), _ptr(out["lo"]), _ptr(out["hi"]), _ptr(out["lps"]), _ptr(out["iters"]), self._mem(dev))
        return out

    def irredundant_bounds(self, Ac, l, u, tol=1e-8, opts=None):
        """Which bounds of polyhedra of one shape their other bounds imply, one job per polyhedron (qpn_irredundant_bounds;
        polyhedra.irredundant_bounds_host is its numpy twin, bit for bit): Ac [polys, d, r] (ABI layout, ``colmajor(A)``), l, u
        [polys, r].  opts: LpOpts, a dict of its fields, or None.
        Returns dict(status [polys] int32 (_lib.IB_*), fail_row [polys] int32, lr, ur [polys, r] (a removed bound is -+inf), how
        [polys, r, 2] int32 (_lib.RED_*), ext [polys, r, 2], lps, iters [polys] int32)."""
        dev, Ac, l, u = self._stage("irredundant_bounds", "Ac l u", f64=(Ac, l, u))
        if Ac.ndim != 3:
            raise QpnError("irredundant_bounds: inconsistent shapes")
        polys, d, r = (int(v) for v in Ac.shape)
        if tuple(l.shape) != (polys, r) or tuple(u.shape) != (polys, r):
            raise QpnError("irredundant_bounds: inconsistent shapes")
        opts = self._lp_opts(opts)
        out = dict(status=self._alloc(dev, (polys,), np.int32), fail_row=self._alloc(dev, (polys,), np.int32),
                   lr=self._alloc(dev, (polys, r), np.float64), ur=self._alloc(dev, (polys, r), np.float64),
                   how=self._alloc(dev, (polys, r, 2), np.int32), ext=self._alloc(dev, (polys, r, 2), np.float64),
                   lps=self._alloc(dev, (polys,), np.int32), iters=self._alloc(dev, (polys,), np.int32))
        self._call("qpn_irredundant_bounds", polys, r, d, _ptr(Ac), _ptr(l), _ptr(u), float(tol), C.byref(opts) if opts is not None else None,
                   _ptr(out["status"]), _ptr(out["fail_row"]), _ptr(out["lr"]), _ptr(out["ur"]), _ptr(out["how"]), _ptr(out["ext"]),
                   _ptr(out["lps"]), _ptr(out["iters"]), self._mem(dev))
        return out

    def exemplar_polys(self, Ac, l, u, open_lo=None, open_hi=None, tol=1e-2, slack_cap=1.0, opts=None):
        """`exemplar` / `isempty` of polyhedra of one shape whose bounds may be open, one job per polyhedron (qpn_exemplar_polys;
        polyhedra.exemplar_polys_host is its numpy twin, bit for bit): Ac [polys, d, n] (ABI layout, ``colmajor(A)``), l, u
        [polys, n], open_lo, open_hi [polys, n] uint8 or None (closed).  opts: LpOpts, a dict of its fields, or None.
        Returns dict(empty [polys] uint8, how [polys] int32 (_lib.EX_*), eps [polys], x [polys, d], row [polys] int32, lam
        [polys, 2 n + 1], iters [polys] int32)."""
        dev, Ac, l, u, open_lo, open_hi = self._stage("exemplar_polys", "Ac l u open_lo open_hi", f64=(Ac, l, u), u8=(open_lo, open_hi))
        if Ac.ndim != 3:
            raise QpnError("exemplar_polys: inconsistent shapes")
        polys, d, n = (int(v) for v in Ac.shape)
        if tuple(l.shape) != (polys, n) or tuple(u.shape) != (polys, n) or any(
                o is not None and tuple(o.shape) != (polys, n) for o in (open_lo, open_hi)):
            raise QpnError("exemplar_polys: inconsistent shapes")
        opts = self._lp_opts(opts)
        out = dict(empty=self._alloc(dev, (polys,), np.uint8), how=self._alloc(dev, (polys,), np.int32), eps=self._alloc(dev, (polys,), np.float64),
                   x=self._alloc(dev, (polys, d), np.float64), row=self._alloc(dev, (polys,), np.int32),
                   lam=self._alloc(dev, (polys, 2 * n + 1), np.float64), iters=self._alloc(dev, (polys,), np.int32))
        self._call("qpn_exemplar_polys", polys, n, d, _ptr(Ac), _ptr(l), _ptr(u), _ptr(open_lo), _ptr(open_hi), float(tol), float(slack_cap),
                   C.byref(opts) if opts is not None else None, _ptr(out["empty"]), _ptr(out["how"]), _ptr(out["eps"]), _ptr(out["x"]),
                   _ptr(out["row"]), _ptr(out["lam"]), _ptr(out["iters"]), self._mem(dev))
        return out

    def exemplar_products(self, A, l, u, open_lo, open_hi, piece_row, factors, n, point=None, point_of=None, point_tol=1e-6, tol=1e-2,
                          slack_cap=1.0, opts=None):
        """The emptiness test of products of pieces, one job per product (qpn_exemplar_products; polyhedra.exemplar_products_host
        is its numpy twin, bit for bit): the pool A [rows, d] (ROW-major: one row per pool row), l, u [rows], open_lo, open_hi
        [rows] uint8 or None (closed); piece_row [pieces + 1] int32; factors [products, k] int32 (-1: no factor in that slot), the
        rows of every product adding up to n; point [points, d] and point_of [products] int32, or both None (no closure test).
        opts: LpOpts, a dict of its fields, or None.  Returns dict(near, empty [products] uint8, how [products] int32 (_lib.EX_*),
        eps [products], x [products, d], row [products] int32, lam [products, 2 n + 1], iters [products] int32)."""
        dev, A, l, u, point, open_lo, open_hi, piece_row, factors, point_of = self._stage(
            "exemplar_products", "A l u point open_lo open_hi piece_row factors point_of", f64=(A, l, u, point), u8=(open_lo, open_hi),
            i32=(piece_row, factors, point_of))
        if A.ndim != 2 or factors.ndim != 2 or piece_row.ndim != 1 or piece_row.shape[0] < 1 or (point is None) != (point_of is None):
            raise QpnError("exemplar_products: inconsistent shapes")
        rows, d = (int(v) for v in A.shape)
        products, k = (int(v) for v in factors.shape)
        pieces, n = int(piece_row.shape[0]) - 1, int(n)
        points = 0 if point is None else int(point.shape[0])
        if tuple(l.shape) != (rows,) or tuple(u.shape) != (rows,) or any(o is not None and tuple(o.shape) != (rows,) for o in (open_lo, open_hi)) or (
                point is not None and (point.ndim != 2 or int(point.shape[1]) != d or tuple(point_of.shape) != (products,))):
            raise QpnError("exemplar_products: inconsistent shapes")
        opts = self._lp_opts(opts)
        out = dict(near=self._alloc(dev, (products,), np.uint8), empty=self._alloc(dev, (products,), np.uint8),
                   how=self._alloc(dev, (products,), np.int32), eps=self._alloc(dev, (products,), np.float64),
                   x=self._alloc(dev, (products, d), np.float64), row=self._alloc(dev, (products,), np.int32),
                   lam=self._alloc(dev, (products, 2 * max(n, 0) + 1), np.float64), iters=self._alloc(dev, (products,), np.int32))
        self._call("qpn_exemplar_products", d, rows, _ptr(A), _ptr(l), _ptr(u), _ptr(open_lo), _ptr(open_hi), pieces, _ptr(piece_row),
                   products, n, k, _ptr(factors), points, _ptr(point), _ptr(point_of), float(point_tol), float(tol), float(slack_cap),
                   C.byref(opts) if opts is not None else None, _ptr(out["near"]), _ptr(out["empty"]), _ptr(out["how"]), _ptr(out["eps"]),
                   _ptr(out["x"]), _ptr(out["row"]), _ptr(out["lam"]), _ptr(out["iters"]), self._mem(dev))
        return out

    def intersection_trees(self, A, l, u, open_lo, open_hi, piece_row, L, list_ptr, list_mem, list_red, cap, point=None, point_of=None,
                           point_tol=1e-6, tol=1e-2, slack_cap=1.0, opts=None):
        """The intersection trees of `combine`, walked breadth first with the empty prefixes pruned depth by depth
        (qpn_intersection_trees; polyhedra.intersection_trees_host is its numpy twin and says what every argument is): the pool of
        exemplar_products (A [rows, d] ROW-major, l, u, open_lo, open_hi [rows] or None, piece_row [pieces + 1] int32); the lists
        of `trees` trees of depth L as a CSR, list_ptr [trees L + 1] and list_mem int32, list_red [trees L] int32 (the trailing
        complement pieces of each list); cap, the most tuples a frontier or a depth's candidates may hold; point [points, d] and
        point_of [trees] int32, or both None.  Returns dict(leaves [cap, L] int32, leaf_tree, leaf_how [cap] int32, n_leaves [1]
        int64, tree_leaves [trees] int32, tested, alive, unanswered [L] int64, overflow [1] int32); only the first n_leaves rows
        of leaves, leaf_tree and leaf_how are written.  Host arrays in: numpy out, cut to n_leaves rows, and a bad index raises;
        device tensors in: tensors out, nothing is read back here, and a bad tree answers tree_leaves = -1."""
        who = "intersection_trees"
        dev, A, l, u, point, open_lo, open_hi, piece_row, list_ptr, list_mem, list_red, point_of = self._stage(
            who, "A l u point open_lo open_hi piece_row list_ptr list_mem list_red point_of", f64=(A, l, u, point), u8=(open_lo, open_hi),
            i32=(piece_row, list_ptr, list_mem, list_red, point_of))
        L, cap = int(L), int(cap)
        if A.ndim != 2 or piece_row.ndim != 1 or piece_row.shape[0] < 1 or list_ptr.ndim != 1 or list_mem.ndim != 1 or list_red.ndim != 1 or \
                L < 1 or int(list_red.shape[0]) % L or int(list_ptr.shape[0]) != int(list_red.shape[0]) + 1 or (point is None) != (point_of is None):
            raise QpnError(f"{who}: inconsistent shapes")
        rows, d = (int(v) for v in A.shape)
        trees, pieces = int(list_red.shape[0]) // L, int(piece_row.shape[0]) - 1
        points = 0 if point is None else int(point.shape[0])
        if tuple(l.shape) != (rows,) or tuple(u.shape) != (rows,) or any(o is not None and tuple(o.shape) != (rows,) for o in (open_lo, open_hi)) or (
                point is not None and (point.ndim != 2 or int(point.shape[1]) != d or tuple(point_of.shape) != (trees,))):
            raise QpnError(f"{who}: inconsistent shapes")
        opts = self._lp_opts(opts)
        rows_out = max(cap, 0)
        out = dict(leaves=self._alloc(dev, (rows_out, L), np.int32), leaf_tree=self._alloc(dev, (rows_out,), np.int32),
                   leaf_how=self._alloc(dev, (rows_out,), np.int32), n_leaves=self._alloc(dev, (1,), np.int64),
                   tree_leaves=self._alloc(dev, (trees,), np.int32), tested=self._alloc(dev, (L,), np.int64),
                   alive=self._alloc(dev, (L,), np.int64), unanswered=self._alloc(dev, (L,), np.int64), overflow=self._alloc(dev, (1,), np.int32))
        self._call("qpn_intersection_trees", d, rows, _ptr(A), _ptr(l), _ptr(u), _ptr(open_lo), _ptr(open_hi), pieces, _ptr(piece_row), trees,
                   L, int(list_mem.shape[0]), _ptr(list_ptr), _ptr(list_mem), _ptr(list_red), points, _ptr(point), _ptr(point_of),
                   float(point_tol), float(tol), float(slack_cap), C.byref(opts) if opts is not None else None, cap, _ptr(out["leaves"]),
                   _ptr(out["leaf_tree"]), _ptr(out["leaf_how"]), _ptr(out["n_leaves"]), _ptr(out["tree_leaves"]), _ptr(out["tested"]),
                   _ptr(out["alive"]), _ptr(out["unanswered"]), _ptr(out["overflow"]), self._mem(dev))
        if not dev:
            k = int(out["n_leaves"][0])
            for key in ("leaves", "leaf_tree", "leaf_how"):
                out[key] = out[key][:k]
        return out


class Nodes:
    """Resident node records (``qpn_nodes_upload``): the records of a level's single-node pools live in HBM owned by the
    library; a sweep hands over only the parameters ``w`` and the output buffers.  What the outer loop
    (src/algorithm.jl:13-117) does between two sweeps -- new parameters, same nodes -- costs no record traffic, and the
    handle remembers what depends on the records alone (whether any node needs the general kernel; the longest-first
    schedule).  ``solve`` = Engine.solve_nodes, ``verify`` = Engine.verify_nodes with the records in place."""

    FIELDS = dict(Qd=0, R=1, qd=2, Ad=3, B=4, l=5, u=6)

    def __init__(self, eng: "Engine", Qc, Rc, qd, Ac, Bc, l, u):
        self.eng = eng
        dev, Qc, Rc, qd, Ac, Bc, l, u = eng._stage("upload_nodes", "Qc Rc qd Ac Bc l u", f64=(Qc, Rc, qd, Ac, Bc, l, u))
        self.batch, self.n = qd.shape
        self.m = l.shape[1]
        self.p = Rc.shape[1]
        h = C.c_void_p()
        eng._call("qpn_nodes_upload", self.batch, self.n, self.m, self.p, _ptr(Qc), _ptr(Rc), _ptr(qd), _ptr(Ac), _ptr(Bc), _ptr(l),
                  _ptr(u), eng._mem(dev), C.byref(h))
        self.h = h
        self._fast = [None, None]

    def close(self):
        if getattr(self, "h", None) and getattr(self.eng, "ctx", None):
            self.eng.lib.qpn_nodes_free(self.eng.ctx, self.h)
        self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def update(self, field: str, data):
        """Replace one array of the records (same shape), e.g. the bounds after another child piece was chosen."""
        dev, data = self.eng._stage("Nodes.update", "data", f64=(data,))
        self.eng._call("qpn_nodes_update", self.h, self.FIELDS[field], _ptr(data), self.eng._mem(dev))

    def info(self):
        """dict(decline_state, declined, scheduled, symmetric, crash_cached, crash_refused, crash_streamed, big_cached, big_refused,
        sweeps) -- see qpn_nodes_info."""
        a = (C.c_int32 * 4)()
        self.eng._call("qpn_nodes_info", self.h, a)
        return dict(decline_state=a[0], declined=a[1], scheduled=bool(a[2] & 1), symmetric=bool(a[2] & 2), crash_cached=bool(a[2] & 4),
                    crash_refused=bool(a[2] & 8), crash_streamed=bool(a[2] & 16), big_cached=bool(a[2] & 32),
                    big_refused=bool(a[2] & 64), sweeps=a[3])

    def set_schedule(self, period=16):
        self.eng._call("qpn_nodes_set_schedule", self.h, int(period))

    def set_warm(self, on=True):
        """Opt this handle's sweeps in to (or out of) the warm start of the mid-size classes (n, m <= 128, one of them > 32;
        qpn_nodes_set_warm): with it on, solve(..., warm=z_prev) runs the warm kernel ahead of the cold one.  On a handle of another
        shape the call changes nothing.  on: True / False (or 1 / 0)."""
        self.eng._call("qpn_nodes_set_warm", self.h, int(on))

    def _outputs(self, rows, dev, want, out, warm):
        """The output buffers of a sweep over `rows` items: a caller-supplied set checked, or the ones `want` names made (status
        always); a hint goes in through z."""
        eng, N = self.eng, self.n + self.m
        spec = dict(status=((rows,), np.int32), z=((rows, N), np.float64), resid=((rows,), np.float64),
                    pivots=((rows,), np.int32), active=((rows, N), np.uint8))
        if out is not None:
            # a caller-supplied set of output buffers is checked once, when it is first seen
            for k, (shape, dt) in spec.items():
                t = out.get(k)
                if t is None:
                    if k == "status":
                        raise QpnError("out['status'] is required")
                    continue
                if _is_dev(t) != dev:
                    raise QpnError(f"out['{k}'] and w must both be host arrays or both device tensors")
                ok = tuple(t.shape) == shape and (t.is_contiguous() and t.dtype == _torch_dt(dt) and t.device.index == eng.device
                                                  if dev else t.flags["C_CONTIGUOUS"] and t.dtype == dt)
                if not ok:
                    raise QpnError(f"out['{k}'] must be a contiguous {np.dtype(dt).name} buffer of shape {shape} on the engine's device")
            for k in ("z", "resid", "pivots", "active"):
                out.setdefault(k, None)
        else:
            out = {k: eng._alloc(dev, shape, dt) if k == "status" or k in want else None for k, (shape, dt) in spec.items()}
        if warm is not None:
            if out["z"] is None:
                out["z"] = eng._alloc(dev, (rows, N), np.float64)
            if warm is not out["z"]:                             # the hint goes in through z
                if dev:
                    out["z"].copy_(warm)
                else:
                    out["z"][...] = warm
        return out

    def solve(self, w, opts=None, want=("z", "resid", "pivots", "active"), out=None, x_out=None, warm=None):
        """One sweep over the resident nodes with parameters w ((p,) shared or (batch, p)); cold duals.  `want` names the
        optional outputs (status always comes back); x_out as in Engine.solve_nodes.

        warm = the z of an earlier sweep over these nodes ([batch, n + m], where w lives): its multipliers name the active set
        every node starts from (QPN_AVI_FLAG_WARM_DUALS, include/qpn_hip.h): always when n, m <= 32, and in the mid-size classes
        (n, m <= 128, one of them > 32) once the handle has opted in with set_warm(); without that the hint is ignored there and
        the sweep is cold.  A node whose hint holds comes back with pivots = 0, every other one -- in the mid-size classes also
        one whose hint has more rows than level_batch.warm_mid_fits admits -- is solved cold in the same call.  Large symmetric records
        (64 < n <= 256, m <= 256) take the hint too once the engine has set_option(OPT_WARM_BIG, 1): it seeds block principal
        pivoting, a node whose hint holds comes back with pivots = n (n + the pairs switched otherwise), and a wrong hint costs
        rounds, never the result; without the option the hint is ignored there.  warm may be out["z"] itself (the
        sweep loop's form: the hint is overwritten by the solution).  The same through opts: with AVI_FLAG_WARM_DUALS set (and
        AVI_FLAG_COLD_START clear) out["z"] carries the hint."""
        eng = self.eng
        # the sweep loop's call (same output buffers as the previous sweep, device parameters): everything but w's address is
        # what it was -- the checks and conversions below were done when these buffers were first seen
        # (a cold and a warm sweep loop over one handle keep an entry each: [0] cold, [1] warm with the hint in out["z"])
        fast = self._fast[warm is not None]
        if fast is not None and out is fast[0] and x_out is fast[1] and opts is None and _is_dev(w) and w.dtype is torch.float64 \
                and w.stride(-1) == 1 and (warm is None or warm is out.get("z")):
            # the cached argument tail holds raw device addresses: it is valid only while every tensor it was built from is
            # the same object at the same address (a swapped or deleted dict entry, or a resized tensor, rebuilds it below),
            # and only for a w of the handle's own shape on the handle's device
            same = all((out.get(k) is t) and (t is None or t.data_ptr() == a) for k, t, a in fast[4]) and \
                (x_out is None or x_out.data_ptr() == fast[5])
            w_ok = w.shape[-1] == self.p and w.device == fast[6] and (w.ndim == 1 or (w.ndim == 2 and w.shape[0] == self.batch))
            if same and w_ok:
                eng._bind_stream(True)
                rc = eng.lib.qpn_solve_nodes_h(eng.ctx, self.h, w.data_ptr(), 0 if w.ndim == 1 else w.stride(0), *fast[2])
                eng._chk(rc, "qpn_solve_nodes_h")
                return out
            self._fast[warm is not None] = None
        dev, = eng._stage("Nodes.solve", "", raw=(w, x_out))    # (w has its own rule: its rows may be strided)
        if not dev:
            w = np.ascontiguousarray(w, dtype=np.float64)
        elif w.dtype != torch.float64 or w.stride(-1) != 1:
            raise QpnError("w must be a float64 tensor with unit inner stride")
        N = self.n + self.m
        if w.shape[-1] != self.p or w.ndim > 2 or (w.ndim == 2 and w.shape[0] != self.batch):
            raise QpnError(f"w must have shape ({self.p},) or ({self.batch}, {self.p})")
        if dev and w.device.index != eng.device:
            raise QpnError("w lives on another device than the engine")
        sw = 0 if w.ndim == 1 else int(w.stride(0) if dev else w.strides[0] // 8)
        o = AviOpts.from_buffer_copy(opts) if opts is not None else eng.default_opts()   # (the flags below are this call's)
        if warm is not None:
            o.flags = (o.flags | _lib.AVI_FLAG_WARM_DUALS) & ~_lib.AVI_FLAG_COLD_START
            if _is_dev(warm) != dev or tuple(warm.shape) != (self.batch, N):
                raise QpnError(f"warm must have shape ({self.batch}, {N}) and live where w lives")
            want = tuple(want) + ("z",)
        hinted = bool(o.flags & _lib.AVI_FLAG_WARM_DUALS) and not (o.flags & _lib.AVI_FLAG_COLD_START)
        if hinted and warm is None and (out is None or out.get("z") is None):
            raise QpnError("AVI_FLAG_WARM_DUALS: out['z'] has to carry the hint (or pass warm=)")
        if not hinted:
            o.flags |= _lib.AVI_FLAG_COLD_START
        out = self._outputs(self.batch, dev, want, out, warm)
        sx = eng._x_stride(x_out, dev, self.batch, self.n)
        tail = (_ptr(out["z"]), _ptr(out["status"]), _ptr(out["resid"]), _ptr(out["pivots"]), _ptr(out["active"]), C.byref(o),
                eng._mem(dev), _ptr(x_out), sx)
        eng._call("qpn_solve_nodes_h", self.h, _ptr(w), sw, *tail)
        if dev and opts is None and (warm is None or warm is out["z"]):
            # (o is kept alive: tail holds a reference to it; the tensors the addresses in `tail` came from are recorded with
            #  those addresses, so that the fast path above can tell when they are no longer what they were)
            snap = tuple((k, out.get(k), None if out.get(k) is None else out[k].data_ptr())
                         for k in ("z", "status", "resid", "pivots", "active"))
            self._fast[warm is not None] = (out, x_out, tail, o, snap, None if x_out is None else x_out.data_ptr(), w.device)
        return out

    def solve_subset(self, idx, w, opts=None, want=("z", "resid", "pivots", "active"), out=None, x_out=None, warm=None):
        """One sweep over the nodes idx names (qpn_solve_nodes_subset_h): the conventions of solve with count = len(idx) in the
        place of batch and every array compact -- slot s of w ((p,) shared or (count, p)), of the outputs, of x_out and of the hint
        warm ([count, n + m]) belongs to node idx[s].  idx: an int32 array or tensor living where w lives, its entries distinct and
        in [0, batch), in any order.  Slot s of every output equals what solve returns for node idx[s] when that node gets the same
        w row (and hint), bit for bit.  On the fused routes (n, m <= 128) only the listed nodes are solved and the handle's state --
        info() -- does not move; larger records run a full sweep and return the listed rows (no saving there).  A device idx with
        a bad entry is not an error: such a slot answers status = FAILURE and zeros."""
        eng = self.eng
        dev, idx = eng._stage("Nodes.solve_subset", "idx", raw=(w, x_out, warm), i32=(idx,))
        if idx is None or idx.ndim != 1:
            raise QpnError("idx must be a one-dimensional int32 array")
        count = int(idx.shape[0])
        if count > self.batch:
            raise QpnError(f"idx names {count} nodes, the handle has {self.batch}")
        if not dev:
            w = np.ascontiguousarray(w, dtype=np.float64)
        elif w.dtype != torch.float64 or (w.numel() and w.stride(-1) != 1):       # (an empty tensor's strides say nothing)
            raise QpnError("w must be a float64 tensor with unit inner stride")
        N = self.n + self.m
        if w.shape[-1] != self.p or w.ndim > 2 or (w.ndim == 2 and w.shape[0] != count):
            raise QpnError(f"w must have shape ({self.p},) or ({count}, {self.p})")
        if dev and w.device.index != eng.device:
            raise QpnError("w lives on another device than the engine")
        sw = 0 if w.ndim == 1 else int(w.stride(0) if dev else w.strides[0] // 8)
        o = AviOpts.from_buffer_copy(opts) if opts is not None else eng.default_opts()   # (the flags below are this call's)
        if warm is not None:
            o.flags = (o.flags | _lib.AVI_FLAG_WARM_DUALS) & ~_lib.AVI_FLAG_COLD_START
            if tuple(warm.shape) != (count, N):
                raise QpnError(f"warm must have shape ({count}, {N}) and live where w lives")
            want = tuple(want) + ("z",)
        hinted = bool(o.flags & _lib.AVI_FLAG_WARM_DUALS) and not (o.flags & _lib.AVI_FLAG_COLD_START)
        if hinted and warm is None and (out is None or out.get("z") is None):
            raise QpnError("AVI_FLAG_WARM_DUALS: out['z'] has to carry the hint (or pass warm=)")
        if not hinted:
            o.flags |= _lib.AVI_FLAG_COLD_START
        out = self._outputs(count, dev, want, out, warm)
        sx = eng._x_stride(x_out, dev, count, self.n) if count else 0         # (an empty array's strides say nothing)
        eng._call("qpn_solve_nodes_subset_h", self.h, count, _ptr(idx), _ptr(w), sw, _ptr(out["z"]), _ptr(out["status"]),
                  _ptr(out["resid"]), _ptr(out["pivots"]), _ptr(out["active"]), C.byref(o), eng._mem(dev), _ptr(x_out), sx)
        return out

    def verify(self, xd, w, tol=1e-4):
        dev, xd, w = self.eng._stage("Nodes.verify", "xd w", f64=(xd, w))
        return self.eng._verify("qpn_verify_nodes_h", dev, (self.h,), self.batch, self.m, self.p, xd, w, tol)

    def verify_subset(self, idx, xd, w, tol=1e-4):
        """The accept gate over the nodes idx names (qpn_verify_nodes_subset_h): the conventions of verify with count = len(idx)
        in the place of batch and every array compact -- slot s of xd ([count, n]), of w ((p,) shared or (count, p)) and of the
        outputs belongs to node idx[s].  idx: an int32 array or tensor living where xd and w live, its entries in [0, batch), in
        any order; an entry may come more than once (one node at several points), so count may exceed batch.  Returns
        (solution [count], lambda [count, m], path [count]); slot s equals what verify returns for node idx[s] at the same xd and
        w rows, bit for bit.  The launches cover count blocks.  A device idx with a bad entry is not an error: such a slot
        answers solution 0, a zero lambda row and path 6."""
        eng = self.eng
        dev, idx, xd, w = eng._stage("Nodes.verify_subset", "idx xd w", i32=(idx,), f64=(xd, w))
        if idx is None or idx.ndim != 1:
            raise QpnError("idx must be a one-dimensional int32 array")
        count = int(idx.shape[0])
        if xd is None or tuple(xd.shape) != (count, self.n):
            raise QpnError(f"xd must have shape ({count}, {self.n})")
        if w is None or w.shape[-1] != self.p or w.ndim > 2 or (w.ndim == 2 and w.shape[0] != count):
            raise QpnError(f"w must have shape ({self.p},) or ({count}, {self.p})")
        return eng._verify("qpn_verify_nodes_subset_h", dev, (self.h, count, _ptr(idx)), count, self.m, self.p, xd, w, tol)


_default = {}


def default_engine(device: int = 0) -> Engine:
    """Process-wide engine per device (created on first use)."""
    if device not in _default:
        _default[device] = Engine(device)
    return _default[device]
