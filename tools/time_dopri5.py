#!/usr/bin/env python3
"""Time the adaptive 'dopri5' rollout against the fixed-grid 'rk4' one at a BASELINE workload's shapes (default configs[0]):
forward without and with the record, and the reverse sweep, each bracketed by events on the current stream; prints the step
statistics of the adaptive solve next to the times.  With --dense the dense-output mode (steps free of the output grid, outputs
interpolated) is timed in the same run.

Everything that is compared is timed in the SAME run in alternating windows: one window = ``--window`` back-to-back calls of one
variant between two events; the variants take turns, ``--reps`` windows each, and the figure is the median over the windows of
the time per call.

    python tools/time_dopri5.py [--workload cfg1] [--reps 20] [--window 10] [--tol 1e-3 1e-5] [--dense] [--out FILE.json]

--per_traj_ts measures what a time grid per trajectory costs instead: rk4, dopri5 landing and dopri5 dense (at the first --tol), each as
rollout, rollout with record and reverse sweep, in three variants that take turns window by window --
  shared    ts (T,), the launches as they always were
  per_traj  the same grid values expanded to (N,T): the `_nt` entry points, the same arithmetic, one row pointer per trajectory
  parent    `shared` through the library of the parent commit given with --parent_lib SO (loaded next to this build's, the same process)
and reports per entry the medians, the window spreads (max - min over the median), `shared_vs_parent` = shared / parent - 1 with its
condition -- not beyond the larger of the two spreads -- and `per_traj_vs_shared` = per_traj / shared - 1, which is reported, not gated.
(The adaptive reverse sweeps never read ts: their two variants of this build are the same launch and measure the windows' noise.)

    python tools/time_dopri5.py --per_traj_ts [--parent_lib SO] [--workload cfg1] [--reps 20] [--window 10] [--tol 1e-4] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_together(fns, reps, window):
    """{name: callable} -> {name: median ms per call}; the callables take turns, window by window."""
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(window):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / window)
    return {k: sorted(v)[len(v) // 2] for k, v in ms.items()}


def timed_windows(fns, reps, window):
    """timed_together, keeping every window: {name: [ms per call, one per window]}"""
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(window):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / window)
    return ms


def time_grids(a, ops, c, z0, ts, order, gw, res):
    """--per_traj_ts: shared against per-trajectory grids, and against the parent's library (see the module docstring)"""
    from vae_gp_ode_amd import _lib
    N, tol = z0.shape[0], a.tol[0]
    rows = ts[None].expand(N, -1).contiguous()
    this, parent = _lib.load(), None
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name, (rt, args) in _lib.SIGNATURES.items():
            if hasattr(parent, name):                  # the parent's header is a subset of this build's
                getattr(parent, name).restype, getattr(parent, name).argtypes = rt, args

    def through_parent(f):
        def g():
            _lib._lib = parent
            try:
                return f()
            finally:
                _lib._lib = this
        return g
    _, xs4 = ops.rollout(c, z0, ts, order, 'rk4', save_stages=True)
    entries = {}                                       # entry -> grid -> callable
    entries['rk4.fwd'] = lambda t: (lambda: ops.rollout(c, z0, t, order, 'rk4'))
    entries['rk4.fwd_record'] = lambda t: (lambda: ops.rollout(c, z0, t, order, 'rk4', save_stages=True))
    entries['rk4.bwd'] = lambda t: (lambda: ops.rollout_bwd(c, xs4, gw, t, order, 'rk4'))
    for name, dense in (('landing', False), ('dense', True)):
        rec = ops.rollout_adaptive(c, z0, ts, order, tol, tol, save_stages=True, dense=dense)
        rec_t = ops.rollout_adaptive(c, z0, rows, order, tol, tol, save_stages=True, dense=dense)
        res[name + '_same_bits'] = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(rec, rec_t))
        res[name] = stats(rec[1], rec[3].shape[-1])
        entries[name + '.fwd'] = lambda t, dense=dense: (lambda: ops.rollout_adaptive(c, z0, t, order, tol, tol, dense=dense))
        entries[name + '.fwd_record'] = lambda t, dense=dense: (lambda: ops.rollout_adaptive(c, z0, t, order, tol, tol, save_stages=True, dense=dense))
        entries[name + '.bwd'] = lambda t, rec=rec: (lambda: ops.rollout_adaptive_bwd(c, rec[2], rec[3], rec[4], gw, order,
                                                                                       theta=rec[5] if len(rec) > 5 else None))
    res['tol'], res['parent_lib'] = tol, bool(parent)
    ok = True
    for entry, make in entries.items():
        fns = {'shared': make(ts), 'per_traj': make(rows)}
        if parent is not None:
            fns['parent'] = through_parent(make(ts))
        win = timed_windows(fns, a.reps, a.window)
        med = {k: sorted(v)[len(v) // 2] for k, v in win.items()}
        spread = {k: round((max(v) - min(v)) / med[k], 4) for k, v in win.items()}
        r = dict(ms={k: round(v, 5) for k, v in med.items()}, spread=spread, per_traj_vs_shared=round(med['per_traj'] / med['shared'] - 1, 4))
        if parent is not None:
            r['shared_vs_parent'] = round(med['shared'] / med['parent'] - 1, 4)
            r['shared_vs_parent_allowed'] = max(spread['shared'], spread['parent'])
            r['shared_not_slower_than_parent'] = r['shared_vs_parent'] <= r['shared_vs_parent_allowed']
            ok = ok and r['shared_not_slower_than_parent']
        res[entry] = r
    if parent is not None:
        res['shared_not_slower_than_parent'] = ok


def stats(cnt, budget):
    cnt = cnt.cpu().long()
    return dict(accepted_mean=cnt[:, 0].float().mean().item(), accepted_max=int(cnt[:, 0].max()), rejected_mean=cnt[:, 1].float().mean().item(),
                evals_mean=cnt[:, 3].float().mean().item(), evals_max=int(cnt[:, 3].max()), failed=int((cnt[:, 2] != 0).sum()), budget=int(budget))


def main():
    import bench
    from vae_gp_ode_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='cfg1')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--window', type=int, default=10)
    ap.add_argument('--tol', type=float, nargs='+', default=[1e-3, 1e-5])
    ap.add_argument('--dense', action='store_true', help='time the dense-output mode next to the landing mode and rk4')
    ap.add_argument('--out', default=None, help='also write the JSON result to this file')
    ap.add_argument('--per_traj_ts', action='store_true', help='time a time grid per trajectory (the same grid values, expanded to (N,T)) '
                                                              'against the shared grid, rk4 and dopri5 landing / dense')
    ap.add_argument('--parent_lib', default=None, help="with --per_traj_ts: the parent commit's libgpode_hip.so, timed in the same windows")
    a = ap.parse_args()
    w = bench.WORKLOADS[a.workload]
    dev = torch.device('cuda:0')
    flow, _, _, _, _, nz, z0, ts = bench.make_inputs(w, 121, dev, 0)
    gp = flow.odefunc.diffeq
    order = w['order']
    with torch.no_grad():
        gp.set_noise(nz)
        c = gp.build_cache()
    c.check_factorisation()
    gw = torch.randn(z0.shape[0], ts.shape[0], z0.shape[1], device=dev)

    res = {'workload': w['desc'], 'reps': a.reps, 'window': a.window, 'N': int(z0.shape[0]), 'T': int(ts.shape[0]),
           'rk4_evals': 4 * (ts.shape[0] - 1)}
    if a.per_traj_ts:
        time_grids(a, ops, c, z0, ts, order, gw, res)
        print(json.dumps(res))
        if a.out:
            with open(a.out, 'w') as f:
                f.write(json.dumps(res, indent=1) + '\n')
        return
    _, xs4 = ops.rollout(c, z0, ts, order, 'rk4', save_stages=True)
    rk4 = {'rk4_fwd_ms': lambda: ops.rollout(c, z0, ts, order, 'rk4'),
           'rk4_fwd_record_ms': lambda: ops.rollout(c, z0, ts, order, 'rk4', save_stages=True),
           'rk4_bwd_ms': lambda: ops.rollout_bwd(c, xs4, gw, ts, order, 'rk4')}
    for tol in a.tol:
        modes = {'landing': False}
        if a.dense:
            modes['dense'] = True
        fns, rec = dict(rk4), {}
        for name, dense in modes.items():
            out = ops.rollout_adaptive(c, z0, ts, order, tol, tol, save_stages=True, dense=dense)
            rec[name] = out
            fns[name + '.fwd_ms'] = lambda dense=dense: ops.rollout_adaptive(c, z0, ts, order, tol, tol, dense=dense)
            fns[name + '.fwd_record_ms'] = lambda dense=dense: ops.rollout_adaptive(c, z0, ts, order, tol, tol, save_stages=True, dense=dense)
            fns[name + '.bwd_ms'] = lambda out=out: ops.rollout_adaptive_bwd(c, out[2], out[3], out[4], gw, order, theta=out[5] if len(out) > 5 else None)
        t = timed_together(fns, a.reps, a.window)
        r = {k: v for k, v in t.items() if k.startswith('rk4')}               # rk4 in this tolerance's run: the yardstick of its windows
        for name in modes:
            sub = {k.split('.', 1)[1]: v for k, v in t.items() if k.startswith(name + '.')}
            sub.update(stats(rec[name][1], rec[name][3].shape[-1]))
            if name == 'landing':
                r.update(sub)
            else:
                sub['max_abs_diff_to_landing'] = (rec['dense'][0] - rec['landing'][0]).abs().max().item()
                r[name] = sub
        res['dopri5_tol_%g' % tol] = r
        for k in ('rk4_fwd_ms', 'rk4_fwd_record_ms', 'rk4_bwd_ms'):
            res.setdefault(k, r[k])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
