"""What the records of inner nodes cost on either route of level_batch.PARENT_RECORDS_ROUTE, on the
net of tools/outer_loop_profile.py: synthetic_pairs(pairs, n, m), default 250 pairs of (32, 32).

  (a) the bare assembly of one level's items, caught from a solve(): the busiest verify_items call (form 0) and the busiest
      solve_level call (form 1) over the leaders.
        host     node_record (+ free_equalities) + batch_records / RecordBatch in numpy, then the records copied to the device
                 (what the staging inside solve_nodes / verify_nodes does with them), timed apart
        device   level_batch.parent_batches: the twin's inputs built, one assemble_parent_nodes call per shape, records in HBM
  (b) algorithm.solve on that net with either route, alternating, and the share of the host route's wall time that node_record +
      free_equalities + batch_records take (clocks around the three functions during one more solve).

Every time is a host clock around work that ends in a synchronise.  Prints one JSON line per measurement and the medians.
usage: python tools/parent_records_rate.py [--pairs 250] [--n 32] [--m 32] [--rounds 3]"""
import argparse
import time

import numpy as np

from rate_common import emit, examples, on_device, quiet_solve, qpn_amd, report, timed
from qpn_amd import level_batch


def catch_calls(net, eng):
    """The busiest verify_items call with children and the busiest solve_level call with inner nodes of one solve()."""
    seen = dict(verify=None, solve=None)
    real_v, real_s = level_batch.verify_items, level_batch.solve_level

    def verify(qpn, items, x, *a, **k):
        if any(ch for _, ch in items) and (seen["verify"] is None or len(items) > len(seen["verify"][0])):
            seen["verify"] = ([(pid, list(ch)) for pid, ch in items], np.array(x, dtype=np.float64))
        return real_v(qpn, items, x, *a, **k)

    def solve(qpn, players, x, assign=None, **k):
        inner = [i for i in players if qpn.network_edges[i]]
        if inner and assign and (seen["solve"] is None or len(inner) > len(seen["solve"][0])):
            seen["solve"] = ([(i, [assign[j] for j in sorted(qpn.network_edges[i]) if j in assign]) for i in inner],
                             np.array(x, dtype=np.float64))
        return real_s(qpn, players, x, assign, **k)

    level_batch.verify_items, level_batch.solve_level = verify, solve
    try:
        ret = quiet_solve(net, engine=eng)
    finally:
        level_batch.verify_items, level_batch.solve_level = real_v, real_s
    return ret, seen


def host_share(net, eng):
    """Wall time of one host-route solve() and the seconds inside node_record, free_equalities and batch_records."""
    spent = dict(node_record=0.0, free_equalities=0.0, batch_records=0.0)
    real = {k: getattr(level_batch, k) for k in spent}

    def clocked(name):
        def fn(*a, **k):
            t0 = time.perf_counter()
            try:
                return real[name](*a, **k)
            finally:
                spent[name] += time.perf_counter() - t0
        return fn
    for k in spent:
        setattr(level_batch, k, clocked(k))
    try:
        wall = timed(lambda: quiet_solve(net, engine=eng))
    finally:
        for k in spent:
            setattr(level_batch, k, real[k])
    return wall, spent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=250)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    eng = qpn_amd.default_engine(0)
    make = lambda: examples.setup("synthetic_pairs", pairs=a.pairs, n=a.n, m=a.m)
    info = dict(pairs=a.pairs, n=a.n, m=a.m)
    net = make()
    ret, seen = catch_calls(net, eng)                              # (also the warm-up: module loads, first launches)
    emit(what="warm_solve", solved=bool(ret["solved"]), **info)

    # ---- (a) the bare assembly
    for form, key in ((0, "verify"), (1, "solve")):
        if seen[key] is None:
            continue
        items, _ = seen[key]
        pieces = len({id(P) for _, ch in items for P in ch})

        def host_numpy():
            recs = [level_batch.node_record(net, pid, ch) for pid, ch in items]
            return level_batch.batch_records([level_batch.free_equalities(r) for r in recs] if form else recs)
        batches = host_numpy()
        rec_bytes = sum(8 * sum(arr.size for arr in (b.Qc, b.Rc, b.qd, b.Ac, b.Bc, b.l, b.u)) for b in batches)

        def host_upload():
            return [on_device(eng, (b.Qc, b.Rc, b.qd, b.Ac, b.Bc, b.l, b.u)) for b in batches]

        def host_both():
            return [on_device(eng, (b.Qc, b.Rc, b.qd, b.Ac, b.Bc, b.l, b.u)) for b in host_numpy()]

        def device():
            got, rest = level_batch.parent_batches(net, items, eng, form)
            assert not rest
            return got
        dev = device()
        same = all(g.where == w.where and all(np.asarray(getattr(g, nm)).tobytes() == getattr(w, nm).tobytes()
                                              for nm in ("Qc", "Rc", "qd", "Ac", "Bc", "l", "u")) for g, w in zip(dev, batches))
        emit(what="assembly_inputs", form=form, items=len(items), distinct_pieces=pieces, shapes=[(b.n, b.m, b.p, len(b)) for b in batches],
             record_bytes=rec_bytes, routes_agree_bitwise=bool(same and len(dev) == len(batches)), **info)
        report(f"assembly_form{form}", [("host_numpy", host_numpy), ("host_upload", host_upload), ("host_numpy_and_upload", host_both),
                                        ("device", device)], a.rounds, items=len(items), **info)

    # ---- (b) solve() with either route, alternating; nets are made outside the clock
    def run(route):
        def fn():
            level_batch.PARENT_RECORDS_ROUTE = route
            try:
                r = quiet_solve(nets.pop(), engine=eng)
            finally:
                level_batch.PARENT_RECORDS_ROUTE = "host"
            xs.setdefault(route, r["x_opt"])
        return fn
    nets = [make() for _ in range(2 * a.rounds)]
    xs = {}
    report("solve", [("host", run("host")), ("device", run("device"))], a.rounds, **info)
    emit(what="solve_routes_agree_bitwise", same=bool(xs["host"].tobytes() == xs["device"].tobytes()), **info)
    wall, spent = host_share(make(), eng)
    emit(what="host_assembly_share_of_solve", wall_seconds=wall, **spent, share=sum(spent.values()) / wall, **info)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
