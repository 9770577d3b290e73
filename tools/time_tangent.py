"""Time the tangent-linear rollout (ops.rollout_jvp, ops.rhs_jacobian; csrc/gp_tangent.hip) at the benchmark's GP sizes, rk4, T = 16.

    python tools/time_tangent.py [--parent_lib SO] [--windows 7] [--min_window_s 0.3] [--out FILE.json]

For configs[0] (RBF, N = 32, D = 6) and configs[1] (DF, N = 256), the protocol of tools/time_posterior.py: windows that take turns, a
host clock around `reps` calls that end in a device synchronise, reps sized per leg so that a window lasts --min_window_s, every leg
warmed first; median ms per call and spread = (max - min) / median:
  rollout       ops.rollout alone                                           -- what the D tangent columns are priced against
  rollout_jvp   ops.rollout_jvp with the identity directions (K = D): zt and Phi_t for every t
  emulation     the only way to Phi_{T-1} without it: one recorded rollout plus D reverse sweeps with a unit gzt at the last time
  rhs           ops.rhs at 256 rows;  rhs_jacobian: ops.rhs_jacobian at the same rows (K = D columns)
  rollout_parent  ops.rollout through the parent commit's library (--parent_lib SO, loaded next to this build's): the untouched path
                  against the parent build, never against itself; `rollout_vs_rollout_parent` is held to the larger of the two spreads
`rollout_jvp_vs_rollout` and `rollout_jvp_vs_emulation` are reported with their spreads, whichever way they fall: this is analysis,
there is no speed target.  No GPU: nothing is measured and the tool says so."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--min_window_s', type=float, default=0.3)
    ap.add_argument('--rows', type=int, default=256, help='rows of the rhs / rhs_jacobian legs')
    ap.add_argument('--parent_lib', default=None, help="the parent commit's libgpode_hip.so, timed in the same windows")
    ap.add_argument('--out', default=None, help='also write the JSON result to this file')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_tangent.py measures on an MI355X: no GPU found, nothing measured')
    import bench
    from time_substeps import summarise
    from vae_gp_ode_amd import _lib, ops
    dev = torch.device('cuda:0')
    this, parent = _lib.load(), None
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name, (rt, args) in _lib.SIGNATURES.items():
            if hasattr(parent, name):                  # the parent's header is a subset of this build's
                getattr(parent, name).restype, getattr(parent, name).argtypes = rt, args

    def through_parent(f):
        def g():
            _lib._lib = parent                         # as tools/time_substeps.py: the swap lasts for the one call
            try:
                return f()
            finally:
                _lib._lib = this
        return g

    def timed_windows(legs):
        """{leg: [ms per call, one per window]}, and the calls per window"""
        reps = {}
        for k, f in legs.items():
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                f()
            torch.cuda.synchronize()
            reps[k] = max(10, int(a.min_window_s / ((time.perf_counter() - t0) / 10)) + 1)
        ms = {k: [] for k in legs}
        for _ in range(a.windows):
            for k, f in legs.items():                  # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps[k]):
                    f()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) / reps[k] * 1e3)
        return ms, reps

    res = dict(method='rk4', windows=a.windows, min_window_s=a.min_window_s, device=torch.cuda.get_device_name(0), parent_lib=bool(parent))
    ok = True
    for name in ('cfg1', 'cfg2'):
        w = bench.WORKLOADS[name]
        flow, _, _, _, _, nz, z0, ts = bench.make_inputs(w, 121, dev, 0)
        gp, order = flow.odefunc.diffeq, w['order']
        with torch.no_grad():
            gp.set_noise(nz)
            c = gp.build_cache()
        c.check_factorisation()
        N, D, T = z0.shape[0], z0.shape[1], ts.shape[0]
        x = torch.randn(a.rows, D, device=dev)
        units = [torch.zeros(N, T, D, device=dev) for _ in range(D)]
        for i, u in enumerate(units):
            u[:, -1, i] = 1.0

        def emulation():
            _, xs = ops.rollout(c, z0, ts, order, 'rk4', save_stages=True)
            return torch.stack([ops.rollout_bwd(c, xs, u, ts, order, 'rk4')[0] for u in units], 1)     # rows of Phi_{T-1}
        # what is timed computes the same thing: Phi_{T-1} both ways, on the inputs that are timed
        _, vt = ops.rollout_jvp(c, z0, ts, order, 'rk4')
        tag = this.gpode_last_launch().decode()
        same = ((vt[:, -1].transpose(-1, -2) - emulation()).abs().max() / vt[:, -1].abs().max()).item()
        legs = {'rollout': lambda: ops.rollout(c, z0, ts, order, 'rk4'), 'rollout_jvp': lambda: ops.rollout_jvp(c, z0, ts, order, 'rk4'),
                'emulation': emulation, 'rhs': lambda: ops.rhs(c, x), 'rhs_jacobian': lambda: ops.rhs_jacobian(c, x)}
        pairs = [('rollout_jvp', 'rollout', False), ('rollout_jvp', 'emulation', False), ('rhs_jacobian', 'rhs', False)]
        if parent is not None:
            legs['rollout_parent'] = through_parent(legs['rollout'])
            pairs.append(('rollout', 'rollout_parent', True))
        ms, reps = timed_windows(legs)
        r, good = summarise(ms, pairs)
        ok = ok and good
        res[name] = dict(r, calls_per_window=reps, workload=w['desc'], N=int(N), D=int(D), T=int(T), K=int(D), rhs_rows=a.rows, tag=tag,
                         phi_last_jvp_vs_emulation_relerr=same)
    res['untouched_path_within_spread'] = ok if parent is not None else None
    txt = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')
    print(txt)


if __name__ == '__main__':
    main()
