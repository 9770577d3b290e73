"""Time the posterior moments of the divergence-free layer (ops.conditional_df) at the benchmark's GP size.

    python tools/time_posterior.py [--M 100] [--D 6] [--N 256] [--windows 7] [--min_window_s 0.3] [--out FILE.json]

Legs: cov = 'diag' and cov = 'point', one call each (fill, Cholesky chain, rows kernel, for 'point' the covariance kernel, and the
read-back of the factorisation status).  Timed in alternating windows on the same inputs -- a host clock around `reps` calls, each of
which ends in a synchronise (the status read-back), reps sized so that a window lasts --min_window_s, every leg warmed first; median
and spread (max - min over the median) per leg.  For information: this is analysis, not the training step.  No GPU: nothing is
measured and the tool says so."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--M', type=int, default=100)
    ap.add_argument('--D', type=int, default=6)
    ap.add_argument('--N', type=int, default=256)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--min_window_s', type=float, default=0.3)
    ap.add_argument('--seed', type=int, default=121)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_posterior.py measures on an MI355X: no GPU found, nothing measured')
    from vae_gp_ode_amd import _lib, ops
    from vae_gp_ode_amd.model.misc.constraint_utils import invsoftplus
    M, D, N = a.M, a.D, a.N
    g = torch.Generator().manual_seed(a.seed)
    r = lambda *s: torch.randn(*s, generator=g)
    Us = torch.tril(0.2 * r(D, M, M)) + 0.5 * torch.eye(M)
    rows, cols = torch.tril_indices(M, M)
    args = [invsoftplus(2.0 + 0.02 * torch.rand(D, D, generator=g)), invsoftplus(0.7 + 0.2 * torch.rand(D, generator=g)), 1.5 * r(M, D),
            0.3 * r(M, D), Us[:, rows, cols].contiguous(), 2.0 * r(N, D)]
    args = [t.float().cuda() for t in args]
    legs = [(cov, (lambda cov=cov: ops.conditional_df(*args, cov=cov))) for cov in ('diag', 'point')]
    chunks = ops.conditional_df_chunks(D, M, N)
    reps, route = {}, {}
    for name, fn in legs:
        fn()
        route[name] = _lib.load().gpode_last_launch().decode()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        reps[name] = max(5, int(a.min_window_s / ((time.perf_counter() - t0) / 5)) + 1)
    times = {name: [] for name, _ in legs}
    for _ in range(a.windows):
        for name, fn in legs:                          # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps[name]):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / reps[name] * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    out = dict(M=M, D=D, N=N, system_rows=(M + N) * D, chunks=len(chunks), route=route, device=torch.cuda.get_device_name(0), windows=a.windows,
               calls_per_window=reps, ms_per_call={k: [round(t, 4) for t in v] for k, v in times.items()},
               median_ms={k: round(v, 4) for k, v in med.items()}, spread={k: round((max(v) - min(v)) / med[k], 4) for k, v in times.items()})
    txt = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')
    print(txt)


if __name__ == '__main__':
    main()
