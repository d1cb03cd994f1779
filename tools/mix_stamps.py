#!/usr/bin/env python3
"""Diagnostic only: phase stamps of ONE mixed reuse sweep of the fused symmetric n = m = 32 kernel, by kind of wavefront
(computing, reusing among the computing ones, reusing in the tail).  Needs a library built with -DQPN_STAMPS (in-kernel clock
stamps: never the product build, never a timed number -- read the SHARES), named by QPN_HIP_LIB:
    QPN_OUT=build/lib_stamps.so QPN_OBJ=/tmp/qpn_obj_stamps bash quadraticprogramnetworks.jl_amd/csrc/build.sh -DQPN_STAMPS
    QPN_HIP_LIB=build/lib_stamps.so python tools/mix_stamps.py [nodes] [sweeps before the stamped one]
Resident handle, natural order (launch position = node index), the bench's ring of parameter vectors; the sweeps before the
stamped one bring the caches into the state of a sweep loop."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import qpn_amd
from qpn_amd import synthetic
from qpn_amd.engine import colmajor
import crash_mix_rule as rule

cnt = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
pre = int(sys.argv[2]) if len(sys.argv) > 2 else 200
n = m = 32; p = 8
eng = qpn_amd.Engine(0)
dev = "cuda:0"
t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
Q, R, qd, A, B, l, u = synthetic.synth_nodes(0, cnt, n, m, p)
h = eng.upload_nodes(t(colmajor(Q)), t(colmajor(R)), t(qd), t(colmajor(A)), t(colmajor(B)), t(l), t(u))
h.set_schedule(0)
w0 = synthetic.shared_params(p)
ring = t(w0[None, :] + 0.25 * np.random.Generator(np.random.Philox(key=[synthetic.SEED, 2 ** 41])).standard_normal((64, p)))
x = torch.zeros((cnt, n), dtype=torch.float64, device=dev)
out = None
for k in range(pre):
    out = h.solve(ring[k % 64], out=out, x_out=x)
st = torch.zeros((cnt, 8), dtype=torch.int64, device=dev)
eng.lib.qpn_debug_set_stamps(C.c_void_p(st.data_ptr()))
out = h.solve(ring[pre % 64], out=out, x_out=x)
torch.cuda.synchronize()
eng.lib.qpn_debug_set_stamps(C.c_void_p(0))
print(h.info())
s = st.cpu().numpy()
raw = s[:, 7].astype(np.uint64)
start = (raw >> np.uint64(32)).astype(np.float64) * 0.01; endt = (raw & np.uint64(0xffffffff)).astype(np.float64) * 0.01
t0 = start.min(); start -= t0; endt -= t0
s = s[:, :7].astype(np.float64)
from_ = rule.reuse_from(cnt)
comp = np.array([rule.recomputes(i, rule.SHARE, from_) for i in range(cnt)])
tail = np.arange(cnt) >= from_
print(f"share {rule.SHARE}/256, reuse_from {from_}: {int(comp.sum())} computing, {int((~comp & ~tail).sum())} reusing among them, "
      f"{int(tail.sum())} reusing in the tail")
print(f"launch: last start {start.max():.1f} us, last end {endt.max():.1f} us")
names = ["setup+load", "B: column via LDS", "B: ratio test+row", "B: row via LDS+exchange", "B: bookkeeping/flips", "readback+check",
         "A: crash / replay"]
for tag, sel in (("computing wavefronts", comp), ("reusing wavefronts among them", ~comp & ~tail), ("reusing wavefronts of the tail", tail)):
    if not sel.any():
        continue
    tot = s[sel].sum(axis=1).mean()
    print(f"{tag}: {int(sel.sum())}, mean cycles per solve {tot:.0f}, mean block duration {(endt[sel] - start[sel]).mean():.1f} us")
    for i, nm in enumerate(names):
        print(f"  {nm:26s} {s[sel, i].mean():10.0f} cycles  {100 * s[sel, i].mean() / tot:5.1f} %")
