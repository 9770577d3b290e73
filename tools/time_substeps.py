#!/usr/bin/env python3
"""Time the sub-steps of the fixed-grid solvers (ops.rollout(..., substeps=s), the `_ns` entry points) at a BASELINE workload's shapes
(default configs[0]), in the manner of tools/time_dopri5.py --per_traj_ts: everything that is compared is timed in the SAME run in
alternating windows (one window = ``--window`` back-to-back calls of one variant between two events; the variants take turns,
``--reps`` windows each); the figure is the median over the windows of the time per call, spread = (max - min) / median.

Three entries -- rollout, rollout with record, reverse sweep -- for rk4 and euler, each in three legs:
  (a) twins      the `_nt`-family launches of this build (ops.rollout as it always was) against the same through the parent commit's
                 library, given with --parent_lib SO (loaded next to this build's, the same process); skipped without it
  (b) ns1        the `_ns` entry points at substeps = 1, called directly, against the twins: the same launch through another door
  (c) s = 2, 4   the `_ns` launch against the emulation it replaces: the twin on the refined grid (T-1) s + 1, plus the slice that
                 keeps every s-th frame of zt (rollout) or the scatter of dL/dzt into every s-th frame (reverse sweep)
(a) and (b) are the untouched path and carry a condition: the difference, in either direction, is not beyond the larger of the two
window spreads.
(c) has no target: `ns_vs_emulation` = ns / emulation - 1 is reported with its spreads, whichever way it falls.

    python tools/time_substeps.py [--workload cfg1|cfg2] [--parent_lib SO] [--reps 20] [--window 10] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from time_dopri5 import timed_windows  # noqa: E402


def refine(ts, s):
    """ts (T,) -> ((T-1) s + 1,): s equal steps in every interval"""
    k = torch.arange(s, dtype=ts.dtype, device=ts.device)
    inner = (ts[:-1, None] + (ts[1:] - ts[:-1])[:, None] * k / s).reshape(-1)
    return torch.cat([inner, ts[-1:]]).contiguous()


def summarise(win, pairs):
    """{variant: [ms per window]} -> medians, spreads, and for every (a, b, gated) of pairs a / b - 1 with the larger of the two spreads"""
    med = {k: sorted(v)[len(v) // 2] for k, v in win.items()}
    spread = {k: round((max(v) - min(v)) / med[k], 4) for k, v in win.items()}
    r = dict(ms={k: round(v, 5) for k, v in med.items()}, spread=spread)
    ok = True
    for a, b, gated in pairs:
        key = '%s_vs_%s' % (a, b)
        r[key] = round(med[a] / med[b] - 1, 4)
        r[key + '_spread'] = max(spread[a], spread[b])
        if gated:
            r[key + '_within_spread'] = abs(r[key]) <= r[key + '_spread']
            ok = ok and r[key + '_within_spread']
    return r, ok


def main():
    import bench
    from vae_gp_ode_amd import _lib, ops
    from vae_gp_ode_amd.ops import KERNEL_ID, METHOD_ID, NSTAGE, _ptr, _stream
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='cfg1', choices=['cfg1', 'cfg2'])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--window', type=int, default=10)
    ap.add_argument('--parent_lib', default=None, help="the parent commit's libgpode_hip.so, timed in the same windows (leg a)")
    ap.add_argument('--out', default=None, help='also write the JSON result to this file')
    a = ap.parse_args()
    w = bench.WORKLOADS[a.workload]
    dev = torch.device('cuda:0')
    flow, _, _, _, _, nz, z0, ts = bench.make_inputs(w, 121, dev, 0)
    gp, order = flow.odefunc.diffeq, w['order']
    with torch.no_grad():
        gp.set_noise(nz)
        c = gp.build_cache()
    c.check_factorisation()
    N, D, T = z0.shape[0], z0.shape[1], ts.shape[0]
    gw = torch.randn(N, T, D, device=dev)

    this, parent = _lib.load(), None
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name, (rt, args) in _lib.SIGNATURES.items():
            if hasattr(parent, name):                  # the parent's header is a subset of this build's
                getattr(parent, name).restype, getattr(parent, name).argtypes = rt, args

    def through_parent(f):
        # as tools/time_dopri5.py and tools/eval_bench.py do: vae_gp_ode_amd._lib keeps the loaded library in `_lib._lib`, which `load()` and
        # `call()` read on every call; the swap lasts for the one call and is undone in `finally`
        def g():
            _lib._lib = parent
            try:
                return f()
            finally:
                _lib._lib = this
        return g

    def ns_fwd(method, s, record):
        """gpode_rollout_fwd_ns called directly (ops.rollout sends substeps = 1 to the twin): the allocations of ops.rollout, then the call"""
        def f():
            zt = torch.empty(c.lead + (N, T, D), dtype=torch.float32, device=dev)
            xs = torch.empty(c.lead + (N, T - 1, s, NSTAGE[method], D), dtype=torch.float32, device=dev) if record else None
            _lib.call('gpode_rollout_fwd_ns', KERNEL_ID[c.kernel], order, METHOD_ID[method], c.Di, c.Do, c.M, c.S, c.nd, _ptr(c.pack), _ptr(z0),
                      _ptr(ts), N, T, _ptr(zt), _ptr(xs), 0, 0, s, _stream())
            return zt, xs
        return f

    def ns_bwd(method, s, xs):
        def f():
            gz0 = torch.empty(c.lead + (N, D), dtype=torch.float32, device=dev)
            ast = torch.empty(c.lead + (N, T - 1, s, NSTAGE[method], c.Do), dtype=torch.float32, device=dev)
            _lib.call('gpode_rollout_bwd_ns', KERNEL_ID[c.kernel], order, METHOD_ID[method], c.Di, c.Do, c.M, c.S, c.nd, _ptr(c.pack), _ptr(xs),
                      _ptr(gw), _ptr(ts), N, T, _ptr(gz0), _ptr(ast), 0, s, _stream())
            return gz0, ast
        return f

    res = {'workload': w['desc'], 'reps': a.reps, 'window': a.window, 'N': int(N), 'T': int(T), 'parent_lib': bool(parent)}
    ok = True
    for method in ('rk4', 'euler'):
        _, xs1 = ops.rollout(c, z0, ts, order, method, save_stages=True)
        twins = {'fwd': lambda m=method: ops.rollout(c, z0, ts, order, m),
                 'fwd_record': lambda m=method: ops.rollout(c, z0, ts, order, m, save_stages=True),
                 'bwd': lambda m=method, x=xs1: ops.rollout_bwd(c, x, gw, ts, order, m)}
        ns1 = {'fwd': ns_fwd(method, 1, False), 'fwd_record': ns_fwd(method, 1, True), 'bwd': ns_bwd(method, 1, xs1.unsqueeze(-3).contiguous())}
        za, zb = twins['fwd'](), ns1['fwd']()[0]
        res['%s.ns1_same_bits' % method] = bool(torch.equal(za, zb))
        for entry in ('fwd', 'fwd_record', 'bwd'):
            fns, pairs = {'twin': twins[entry], 'ns1': ns1[entry]}, [('ns1', 'twin', True)]
            if parent is not None:
                fns['parent'] = through_parent(twins[entry])
                pairs.append(('twin', 'parent', True))
            r, good = summarise(timed_windows(fns, a.reps, a.window), pairs)
            res['%s.%s' % (method, entry)], ok = r, ok and good
        for s in (2, 4):
            fine = refine(ts, s)
            Tf = fine.shape[0]
            _, xs_s = ops.rollout(c, z0, ts, order, method, save_stages=True, substeps=s)
            zt_f, xs_f = ops.rollout(c, z0, fine, order, method, save_stages=True)
            res['%s.s%d_max_abs_diff_to_emulation' % (method, s)] = (ops.rollout(c, z0, ts, order, method, substeps=s)
                                                                     - zt_f[..., ::s, :]).abs().max().item()

            def emu_bwd(m=method, x=xs_f, s=s, Tf=Tf, fine=fine):
                g = torch.zeros(N, Tf, D, device=dev)
                g[:, ::s] = gw
                return ops.rollout_bwd(c, x, g, fine, order, m)
            legs = {'fwd': (lambda m=method, s=s: ops.rollout(c, z0, ts, order, m, substeps=s),
                            lambda m=method, s=s, fine=fine: ops.rollout(c, z0, fine, order, m)[..., ::s, :].contiguous()),
                    'fwd_record': (lambda m=method, s=s: ops.rollout(c, z0, ts, order, m, save_stages=True, substeps=s),
                                   lambda m=method, s=s, fine=fine: (lambda o: (o[0][..., ::s, :].contiguous(), o[1]))(
                                       ops.rollout(c, z0, fine, order, m, save_stages=True))),
                    'bwd': (lambda m=method, s=s, x=xs_s: ops.rollout_bwd(c, x, gw, ts, order, m, substeps=s), emu_bwd)}
            for entry, (ns, emu) in legs.items():
                r, _ = summarise(timed_windows({'ns': ns, 'emulation': emu}, a.reps, a.window), [('ns', 'emulation', False)])
                res['%s.s%d.%s' % (method, s, entry)] = r
    res['untouched_path_within_spread'] = ok
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
