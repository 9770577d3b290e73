#!/usr/bin/env python3
"""Time the adaptive 'dopri5' rollout against the fixed-grid 'rk4' one at a BASELINE workload's shapes (default configs[0]):
forward without and with the record, and the reverse sweep, each bracketed by events on the current stream; prints the step
statistics of the adaptive solve next to the times.

    python tools/time_dopri5.py [--workload cfg1] [--reps 20] [--tol 1e-3 1e-5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    from vae_gp_ode_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='cfg1')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--tol', type=float, nargs='+', default=[1e-3, 1e-5])
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

    def timed(fn):
        ms = []
        for _ in range(a.reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = sorted(ms[3:])
        return out, ms[len(ms) // 2]

    res = {'workload': w['desc'], 'reps': a.reps}
    _, res['rk4_fwd_ms'] = timed(lambda: ops.rollout(c, z0, ts, order, 'rk4'))
    (_, xs), res['rk4_fwd_record_ms'] = timed(lambda: ops.rollout(c, z0, ts, order, 'rk4', save_stages=True))
    _, res['rk4_bwd_ms'] = timed(lambda: ops.rollout_bwd(c, xs, gw, ts, order, 'rk4'))
    res['rk4_evals'] = 4 * (ts.shape[0] - 1)
    for tol in a.tol:
        r = {}
        _, r['fwd_ms'] = timed(lambda: ops.rollout_adaptive(c, z0, ts, order, tol, tol))
        (zt, cnt, xs, hs, ie), r['fwd_record_ms'] = timed(lambda: ops.rollout_adaptive(c, z0, ts, order, tol, tol, save_stages=True))
        _, r['bwd_ms'] = timed(lambda: ops.rollout_adaptive_bwd(c, xs, hs, ie, gw, order))
        cnt = cnt.cpu().long()
        r.update(accepted_mean=cnt[:, 0].float().mean().item(), accepted_max=int(cnt[:, 0].max()), rejected_mean=cnt[:, 1].float().mean().item(),
                 evals_mean=cnt[:, 3].float().mean().item(), evals_max=int(cnt[:, 3].max()), failed=int((cnt[:, 2] != 0).sum()),
                 budget=int(hs.shape[-1]))
        res['dopri5_tol_%g' % tol] = r
    print(json.dumps(res))


if __name__ == '__main__':
    main()
