"""qpn_solve_avi_batch, qpn_solve_mcp_csc and qpn_check_avi_batch on general box-MCPs (STD and GAVI rows in any order) against
planted, exactly known solutions.

The other box-MCP tests compare with the CPU oracle, which shares the kernels' pivot rule and was written with them; here the
truth is the exact solution of the rounded data (tests/mcp_ref.py: longdouble refinement, proved by a certificate), on the
smallest sizes at which each instantiation can go wrong (tests/mcp_cases.py: both ends of every register block size, the four
scan kernels behind a declining Schur kernel, every rows-per-thread class of the big kernel up to the ABI's N = 1024, the gated
big kernel behind a declining blocked crash, shared M and shared kind, several flagged items per scan block and the scan loop's
second trip).  Per item: status SUCCESS, active[] equal to the masks of the truth,

    error <= max(16 E_ref, 64 eps),   E_ref = the CPU oracle's worst error against the truth on the same cell and family

(solve_ref.accuracy_bar), parity with the oracle (status, pivots, active, |dz| <= 1e-9), and resid within the rounding bound of
the natural-map residual at the returned z.  The measured tallies are in profiles/planted_mcp_accuracy.txt.
"""
import numpy as np
import pytest

import mcp_cases as MC
import mcp_ref as MR
import solve_ref as SR

pytestmark = pytest.mark.gpu

# (cell, family) -> factor where the global 16 does not hold, with the reason; none needed so far
FACTORS = {}
ZTOL = 1e-9
KEYS = ("z", "status", "resid", "pivots", "active")


def _np(res):
    out = {}
    for k, v in res.items():
        if v is not None:
            out[k] = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
    return out


def _solve(engine, cases, shared=False, device=False, z0=None, opts=None):
    """One batch through Engine.solve_avi_batch: host arrays, or the same buffers as device tensors."""
    from qpn_amd.engine import colmajor
    M, q, l, u, kind = MC.stack(cases, shared)
    args = [colmajor(M), q, l, u, z0, kind]
    if device:
        import torch
        args = [None if a is None else torch.tensor(a, device="cuda:0") for a in args]
    Mc, q, l, u, z0, kind = args
    res = engine.solve_avi_batch(Mc, q, l, u, z0=z0, kind=kind, opts=opts)
    if device:
        engine.synchronize()
    return _np(res)


def _parity(res, ref, where):
    """What the parity tests ask: status and pivots equal, on solved items active bit-equal and |dz| <= 1e-9 relative."""
    assert np.array_equal(res["status"], ref["status"]), f"{where}: status {res['status']} against the oracle's {ref['status']}"
    assert np.array_equal(res["pivots"], ref["pivots"]), f"{where}: pivots {res['pivots']} against the oracle's {ref['pivots']}"
    ok = ref["status"] == MC.SUCCESS
    if ok.any():
        zc, zg = ref["z"][ok], res["z"][ok]
        err = np.max(np.abs(zg - zc) / np.maximum(1.0, np.max(np.abs(zc), axis=1, keepdims=True)))
        assert err <= ZTOL, f"{where}: deviation {err:g} from the oracle"
        assert np.array_equal(res["active"][ok], ref["active"][ok]), f"{where}: active[] differs from the oracle's"


def _resid(cases, res, where):
    """resid against the longdouble natural-map residual at the RETURNED z: within gamma = 2 N eps max_i (|M| |z| + |q|)_i, the
    rounding bound of the kernel's N-term fma sum (the residual is 1-Lipschitz in r), and <= 1e-8."""
    for i, c in enumerate(cases):
        M, q, l, u, kind = MC.data(c)
        nat = float(MR.natural_residual_ld(M, q, l, u, kind, res["z"][i]))
        g = MR.matvec_bound(M, q, res["z"][i])
        assert abs(res["resid"][i] - nat) <= g, f"{where} [{i}]: resid {res['resid'][i]:.3e}, longdouble {nat:.3e}, gamma {g:.1e}"
        assert res["resid"][i] <= 1e-8, f"{where} [{i}]: resid {res['resid'][i]:.3e}"


class _Cell:
    """The checks of one cell: every run is compared with its truths and with the oracle's error on the same cell and family."""

    def __init__(self, cell):
        self.cell = cell
        self.runs = []                                    # (where, cases, outputs)
        self.e_ref = {}
        self.notes = []

    def add(self, where, cases, res, ref):
        assert np.all(ref["status"] == MC.SUCCESS), f"{self.cell} {where}: the oracle does not solve its own reference cases"
        for i, c in enumerate(cases):
            e = MR.mcp_error(ref["z"][i], MC.truth(c)[0])
            self.e_ref[c["family"]] = max(self.e_ref.get(c["family"], 0.0), e)
        _parity(res, ref, f"{self.cell} {where}")
        _resid(cases, res, f"{self.cell} {where}")
        self.runs.append((where, cases, res))

    def finish(self, capsys):
        fails, tally = [], {}
        for where, cases, res in self.runs:
            for fam in sorted({c["family"] for c in cases}):
                idx = [i for i, c in enumerate(cases) if c["family"] == fam]
                f, worst, cnt = MC.check_against_truth([cases[i] for i in idx], {k: res[k][idx] for k in ("z", "status", "active")},
                                                       f"{self.cell} {where}", e_ref=self.e_ref[fam],
                                                       factor=FACTORS.get((self.cell, fam)))
                fails += f
                t = tally.setdefault(fam, [0.0, 0])
                t[0] = max(t[0], worst); t[1] += cnt
        with capsys.disabled():
            print(f"\n[mcp {self.cell}] runs: " + ", ".join(r[0] for r in self.runs))
            for f, (e, cnt) in sorted(tally.items()):
                er = self.e_ref[f]
                print(f"[mcp {self.cell}]   {f:5s} items {cnt:6d}  kernel {e:.2e}  E_ref {er:.2e}  ratio {e / max(er, 1e-300):7.2f}  "
                      f"bar {SR.accuracy_bar(er, FACTORS.get((self.cell, f), SR.FACTOR)):.2e}")
            for note in self.notes:
                print(f"[mcp {self.cell}]   {note}")
        assert not fails, "\n".join(fails[:12]) + (f"\n... {len(fails)} in all" if len(fails) > 12 else "")
        # no case was skipped: every item of every run was compared
        assert sum(t[1] for t in tally.values()) == sum(len(r[1]) for r in self.runs)


def _bit_equal(a, b, where):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), f"{where}: {k} differs between host and device buffers"


@pytest.mark.parametrize("cell", list(MC.CELLS))
def test_cell(engine, oracle, cell, capsys):
    """Every batch of a cell in host mode; the cell's middle batch again as device tensors, bit-equal."""
    ck = _Cell(cell)
    shared = cell == "shared"
    batches = {}
    for N, kinds, f, cases in MC.cell_cases(cell):
        # the shared cell: one M and one kind vector per batch (strideM = 0, stride_kind = 0); elsewhere the families of one
        # size go into one batch
        batches.setdefault((N, kinds, f) if shared else (N, kinds), []).extend(cases)
    for k, (key, cases) in enumerate(batches.items()):
        where = " ".join(map(str, key))
        res = _solve(engine, cases, shared)
        ck.add(f"N={where}", cases, res, MC.oracle_solve(oracle, cases, shared))
        if k == len(batches) // 2:
            _bit_equal(res, _solve(engine, cases, shared, device=True), f"{cell} N={where}")
    assert sum(len(r[1]) for r in ck.runs) == sum(len(cs) for _, _, _, cs in MC.cell_cases(cell))
    ck.finish(capsys)


def test_starts(engine, oracle, capsys):
    """The solution is unique, so the start may change the pivot count and nothing else: zeros, NaNs, the plant, the plant +- 10
    (outside the bounds), N(0, 1) and the cold-start flag over a z prefilled with NaN all end at the truth within the bar."""
    from qpn_amd import _lib
    ck = _Cell("starts")
    rng = np.random.default_rng(3)
    for N, kinds, f, cases in MC.cell_cases("shared"):
        plant = np.stack([c["plant"] for c in cases])
        starts = dict(zeros=np.zeros_like(plant), nan=np.full_like(plant, np.nan), plant=plant, plus10=plant + 10.0,
                      minus10=plant - 10.0, normal=rng.standard_normal(plant.shape))
        for name, z0 in starts.items():
            ck.add(f"{N}/{f}/{name}", cases, _solve(engine, cases, shared=True, z0=z0),
                   MC.oracle_solve(oracle, cases, shared=True, z0=z0))
        o = engine.default_opts()
        o.flags |= _lib.AVI_FLAG_COLD_START
        ck.add(f"{N}/{f}/cold-flag", cases, _solve(engine, cases, shared=True, z0=starts["nan"], opts=o),
               MC.oracle_solve(oracle, cases, shared=True))
    ck.finish(capsys)


@pytest.mark.parametrize("N", MC.NONSOLUTION_SIZES)
def test_non_solutions_in_company(engine, oracle, N, capsys):
    """Item 1 is planted infeasible: RAY_TERM as in the oracle, and items 0, 2 and 3 at their truths within the bar.  The same
    batch under a budget of one pivot: MAX_ITERS wherever the oracle stops, and the oracle's pivot counts."""
    cases = MC.nonsolution_batch(N)
    res, ref = _solve(engine, cases), MC.oracle_solve(oracle, cases)
    assert list(ref["status"]) == [MC.SUCCESS, MC.RAY_TERM, MC.SUCCESS, MC.SUCCESS]
    assert res["status"][1] == MC.RAY_TERM == ref["status"][1]
    _parity(res, ref, f"non-solutions N={N}")
    keep = [0, 2, 3]
    ck = _Cell(f"company N={N}")
    ck.add("items 0, 2, 3", [cases[i] for i in keep], {k: res[k][keep] for k in KEYS}, {k: ref[k][keep] for k in KEYS})
    ck.finish(capsys)
    o = engine.default_opts()
    o.max_pivots = 1
    res1, ref1 = _solve(engine, cases, z0=np.zeros((4, N)), opts=o), MC.oracle_solve(oracle, cases, max_pivots=1)
    assert np.all(ref1["status"] == MC.MAX_ITERS)
    assert np.array_equal(res1["status"], ref1["status"]) and np.array_equal(res1["pivots"], ref1["pivots"]), \
        f"budget 1: status {res1['status']} pivots {res1['pivots']}, the oracle's {ref1['status']} {ref1['pivots']}"


def test_scan_many_nine(engine, oracle, capsys):
    """4101 items of N = 9, every third node-shaped (the Schur kernel keeps it), the others for the scan kernel: several
    flagged items per scan block, beside items that are not flagged."""
    cases = MC.scan_many_nine()
    ck = _Cell("scan_many N=9")
    res, ref = _solve(engine, cases), MC.oracle_solve(oracle, cases)
    ck.add(f"{len(cases)} items, every third node-shaped", cases, res, ref)
    # the two kernels of this launch apart: the scan kernel does the oracle's arithmetic, the Schur kernel a blocked elimination
    worst = {}
    for i, c in enumerate(cases):
        w = worst.setdefault((c["kinds"], c["family"]), [0.0, 0.0])
        w[0], w[1] = max(w[0], MR.mcp_error(res["z"][i], MC.truth(c)[0])), max(w[1], MR.mcp_error(ref["z"][i], MC.truth(c)[0]))
    for kinds in ("mixed", "node"):
        ck.notes.append(f"{kinds:5s} items: " + "  ".join(f"{f} kernel {worst[kinds, f][0]:.2e} oracle {worst[kinds, f][1]:.2e}"
                                                         for f in MC.FAMILIES))
    ck.finish(capsys)


def test_scan_many_two(engine, oracle, capsys):
    """64 * 2048 + 3 items of N = 2, 16 distinct planted ones tiled in rotation: the scan loop's second trip.  Every copy has to
    be the first copy bit for bit; the 16 are compared with their truths."""
    from qpn_amd.engine import colmajor
    cases, idx = MC.scan_many_two()
    M, q, l, u, kind = (a[idx] for a in MC.stack(cases))
    res = _np(engine.solve_avi_batch(colmajor(M), q, l, u, kind=kind))
    n = len(cases)
    for k in KEYS:
        same = res[k] == res[k][:n][idx]
        assert same.all(), f"{k}: {(~same.reshape(len(idx), -1).all(axis=1)).sum()} of {len(idx)} items differ from their first copy"
    ck = _Cell("scan_many N=2")
    ck.add(f"{len(idx)} items, {n} distinct", cases, {k: res[k][:n] for k in KEYS}, MC.oracle_solve(oracle, cases))
    ck.finish(capsys)


@pytest.mark.parametrize("N", [12, 130])
def test_mcp_csc(engine, oracle, N, capsys):
    """qpn_solve_mcp_csc on a thinned planted item in 1-based CSC; the same matrix stored with a split entry, an explicit zero
    and an empty column gives the same answer bit for bit."""
    c, j, first, second = MC.csc_case(N)
    zt = MC.truth(c)[0]
    ref = MC.oracle_solve(oracle, [c])
    e_ref = MR.mcp_error(ref["z"][0], zt)
    bar = SR.accuracy_bar(e_ref)
    zs = []
    for name, (colptr, rowval, nzval) in (("canonical", first), ("split / zero / empty column", second)):
        assert (colptr[j + 1] == colptr[j]) == (name != "canonical")
        st, z, info = engine.solve_mcp_csc(N, colptr, rowval, nzval, c["q"], c["l"], c["u"], np.zeros(N))
        e = MR.mcp_error(z, zt)
        with capsys.disabled():
            print(f"\n[mcp csc] N={N} {name}: kernel {e:.2e}  E_ref {e_ref:.2e}  bar {bar:.2e}  pivots {info['pivots']}")
        assert st == MC.SUCCESS == ref["status"][0] and info["pivots"] == ref["pivots"][0]
        assert e <= bar, f"N={N} {name}: error {e:.3e} > bar {bar:.3e}"
        _resid([c], dict(z=z[None], resid=np.array([info["resid"]])), f"csc N={N} {name}")
        zs.append(z)
    assert np.array_equal(zs[0], zs[1])


@pytest.mark.parametrize("N", list(MC.CHECK_FORMS))
def test_check_avi_batch(engine, N):
    """qpn_check_avi_batch against the longdouble restatement of src/avi.jl:152-154: degree 0 and r = M z + q at the truth, the
    restated count with one row moved by 1e-3 (each of the four violations, on an STD and on a GAVI row), degree > 0 for a NaN."""
    from qpn_amd.engine import colmajor
    cases, sm, sk = MC.check_batch(N)
    M, q, l, u, kind = MC.stack(cases)
    Mc = colmajor(cases[0]["M"] if sm else M)
    kd = cases[0]["kind"] if sk else kind
    zt = np.stack([np.asarray(MC.truth(c)[0], dtype=np.float64) for c in cases])
    deg, r = engine.check_avi_batch(Mc, q, l, u, zt, kind=kd)
    assert np.all(np.asarray(deg) == 0), deg
    for i, c in enumerate(cases):
        rl = MR.residual_ld(c["M"], c["q"], zt[i])
        assert np.max(np.abs(np.asarray(r)[i] - rl)) <= MR.matvec_bound(c["M"], c["q"], zt[i])
    rep = lambda a: np.repeat(a, len(MC.VIOLATIONS), axis=0)
    qv, zv, want = rep(q), rep(zt), []
    for i, c in enumerate(cases):
        for w in range(len(MC.VIOLATIONS)):
            k = i * len(MC.VIOLATIONS) + w
            qv[k], zv[k], _ = MC.violated(c, w)
            want.append(MR.check_degree(c["M"], qv[k], c["l"], c["u"], c["kind"], zv[k])[0])
    deg, _ = engine.check_avi_batch(Mc if sm else colmajor(rep(M)), qv, rep(l), rep(u), zv, kind=kd if sk else rep(kind), want_r=False)
    assert list(np.asarray(deg)) == want and min(want) >= 1
    zn = zt.copy()
    zn[:, N // 2] = np.nan
    deg, _ = engine.check_avi_batch(Mc, q, l, u, zn, kind=kd, want_r=False)
    assert np.all(np.asarray(deg) > 0), deg
